"""Time the route seeds in the volume (K9v) on the cfg5 volume (1024 x 1024 x 64, built as
bench.py builds it): uam_route3d_field per UAM_OPT_K9V_TILE_XY x UAM_OPT_K9V_TILE_Z x
UAM_OPT_K9V_INNER (host wall ms of the whole call, --reps samples per row, rounds, tile visits,
visits per tile) for a goal near the centre and one in a corner, both at mid altitude; every row
must give the first row's dist and next bits (asserted).  Then uam_route3d_paths at --queries
random starts.  With --smooth SPAN [SPAN ...]: uam_route3d_free_bits once per field and
uam_route3d_paths_smooth at each span (device ms between two events, three calls after one
untimed), and per span the seeds' shape: vertices per status-0 seed, the share of status-0 seeds
with climb_sum == 0 and the mean cost under eval_waypoints3d with a 10 degree climb limit, beside
span 0's.  One JSON line per measurement.
usage: python tools/time_route3d.py [--R R] [--nz NZ] [--queries Q] [--lam L] [--reps K]
       [--tile-xy T ..] [--tile-z T ..] [--inner I ..] [--smooth SPAN ..]"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_BYTES_PER_S = 8.0e12    # the MI355X's nominal HBM3E rate


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--R", type=int, default=1024)
    ap.add_argument("--nz", type=int, default=64)
    ap.add_argument("--queries", type=int, default=100000)
    ap.add_argument("--lam", type=float, default=1.0)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--tile-xy", type=int, nargs="*", default=[8, 16])
    ap.add_argument("--tile-z", type=int, nargs="*", default=[4, 8])
    ap.add_argument("--inner", type=int, nargs="*", default=[4, 16, 64])
    ap.add_argument("--smooth", type=int, nargs="+", default=[])
    a = ap.parse_args()
    import numpy as np
    import torch

    from uam_path_planning_amd import profiles
    from uam_path_planning_amd.engine import Engine, Vertical
    from uam_path_planning_amd.geometry import compile_map
    from uam_path_planning_amd.scenario import (CONFIGS, build_region_map, canonical_params,
                                                canonical_spec, layer_weights, raster_geo)
    from uam_path_planning_amd.synthetic import random_pairs3d, synthetic_dem

    cfg = CONFIGS["cfg5"]
    spec = canonical_spec(nfz_polygons=cfg["nfz_polygons"])
    eng = Engine(0)
    eng.set_geometry(compile_map(build_region_map(spec)))
    eng.set_params(canonical_params(spec, N=cfg["N"], altitude=320.0))
    geo = raster_geo(a.R)
    raster = eng.raster_build(geo, eng.tensor(synthetic_dem(a.R), torch.float32), summary=False)
    volume = eng.volume_build(raster, a.nz, cfg["z0"], cfg["dz"], layer_weights(a.nz))
    z_mid = cfg["z0"] + (a.nz // 2 + 0.5) * cfg["dz"]

    def free_near(x, y):
        """The first point on a fixed ray from (x, y) outside every no-fly shape."""
        for k in range(200):
            p = np.array([[x + 0.37 * k, y - 0.29 * k]])
            pe = eng.eval_points(torch.tensor(p, device="cuda"), want=("psi_raw", "collide"))
            if float(pe["psi_raw"][0]) == 0 and int(pe["collide"][0]) == 0:
                return np.array([p[0, 0], p[0, 1], z_mid])
        raise RuntimeError("no free goal found")

    goals = {"centre": free_near(30.0, -10.0), "corner": free_near(0.4, 19.6)}
    voxels = a.R * a.R * a.nz
    floor_ms = voxels * 17 / HBM_BYTES_PER_S * 1e3
    print(json.dumps({"goals": {k: v.tolist() for k, v in goals.items()}, "voxels": voxels,
                      "traffic_floor_ms": round(floor_ms, 4), "reps": a.reps}), flush=True)
    first = {}
    combos = [(txy, tz, i) for txy in a.tile_xy for tz in a.tile_z for i in a.inner]
    for txy, tz, inner in combos:
        for name, g in goals.items():
            eng.set_option("k9v_tile_xy", txy)
            eng.set_option("k9v_tile_z", tz)
            eng.set_option("k9v_inner", inner)
            ms = []
            for _ in range(a.reps):
                f = None
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                f = eng.route_field3d(volume, g.reshape(1, 3), lam=a.lam)
                torch.cuda.synchronize()
                ms.append(round((time.perf_counter() - t0) * 1e3, 2))
            ntiles = (-(-a.R // txy)) ** 2 * (-(-a.nz // tz))
            if name not in first:
                first[name] = (f.dist.clone(), f.next.clone())
            same = bool(torch.equal(f.dist.view(torch.int64), first[name][0].view(torch.int64))
                        and torch.equal(f.next, first[name][1]))
            print(json.dumps({"tile_xy": txy, "tile_z": tz, "inner": inner, "goal": name,
                              "ms": ms, "x_floor": round(min(ms) / floor_ms),
                              "rounds": f.rounds, "visits": f.visits,
                              "visits_per_tile": round(f.visits / ntiles, 2),
                              "reachable_voxels": int(torch.isfinite(f.dist).sum()),
                              "same_bits_as_first": same}), flush=True)
            assert same, "the field's bits depend on the options"
            del f
    f = eng.route_field3d(volume, goals["centre"].reshape(1, 3), lam=a.lam)
    s = eng.tensor(random_pairs3d(a.queries, seed=5, zmin=cfg["z0"],
                                  zmax=cfg["z0"] + a.nz * cfg["dz"])[:, :3], torch.float64)
    gi = eng.tensor(np.zeros(a.queries, dtype=np.int32), torch.int32)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def timed(call):
        """(device ms of three calls after one untimed, the last call's result)"""
        call()
        torch.cuda.synchronize()
        ms = []
        for _ in range(3):
            e0.record()
            out = call()
            e1.record()
            torch.cuda.synchronize()
            ms.append(round(e0.elapsed_time(e1), 3))
        return ms, out

    ms, o = timed(lambda: eng.route_paths3d(f, s, gi))
    st = o["status"].cpu().numpy()
    steps = o["steps"].cpu().numpy()
    print(json.dumps({"route_paths3d_queries": a.queries, "ms_each": ms,
                      "status_counts": {int(k): int((st == k).sum()) for k in np.unique(st)},
                      "steps_mean": float(steps[st == 0].mean()) if (st == 0).any() else None,
                      "steps_max": int(steps.max())}), flush=True)
    if not a.smooth:
        return

    def rebuild_bits():
        f.free_bits = None
        return eng.route_free_bits3d(f)

    ms, words = timed(rebuild_bits)
    print(json.dumps({"route_free_bits3d_ms_each": ms, "words": words.numel()}), flush=True)
    vert = Vertical(f.z_scale, profiles.sin_of_angle(10.0), profiles.sin_of_angle(10.0))
    ok = st == 0

    def shape(out):
        ev = eng.eval_waypoints3d(out["wp3"], volume, vertical=vert)
        climb = ev["climb_sum"].cpu().numpy()[ok]
        cost = ev["cost"].cpu().numpy()[ok]
        return {"climb_free_share": round(float((climb == 0).mean()), 4),
                "climb_sum_mean": float(climb.mean()), "cost_mean": float(cost.mean()),
                "below_terrain": int((ev["below_terrain"].cpu().numpy()[ok] > 0).sum()),
                "nfz_hit": int((ev["nfz_hits"].cpu().numpy()[ok] > 0).sum())}

    print(json.dumps({"span": 0, **shape(o)}), flush=True)
    for span in a.smooth:
        ms, so = timed(lambda: eng.route_paths3d(f, s, gi, smooth=span))
        assert bool(torch.equal(so["status"], o["status"]) and torch.equal(so["steps"],
                                                                           o["steps"]))
        v = so["vertices"].cpu().numpy()[ok]
        print(json.dumps({"span": span, "ms_each": ms, "vertices_mean": round(float(v.mean()), 2),
                          "vertices_max": int(v.max()), **shape(so)}), flush=True)


if __name__ == "__main__":
    main()
