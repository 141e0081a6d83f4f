"""Time the route seeds in the volume (K9v) on the cfg5 volume (1024 x 1024 x 64, built as
bench.py builds it): uam_route3d_field per UAM_OPT_K9V_TILE_XY x UAM_OPT_K9V_TILE_Z x
UAM_OPT_K9V_INNER (host wall ms of the whole call, --reps samples per row, rounds, tile visits,
visits per tile) for a goal near the centre and one in a corner, both at mid altitude; every row
must give the first row's dist and next bits (asserted).  Then uam_route3d_paths at --queries
random starts.  With --smooth SPAN [SPAN ...]: uam_route3d_free_bits once per field and
uam_route3d_paths_smooth at each span (device ms between two events, three calls after one
untimed), and per span the seeds' shape: vertices per status-0 seed, the share of status-0 seeds
with climb_sum == 0 and the mean cost under eval_waypoints3d with a 10 degree climb limit, beside
span 0's.  One JSON line per measurement.  --joint G adds
the joint field (K9vj) of G vertiports (free voxels drawn from random_pairs3d) next to
uam_route3d_field for the same goals -- wall ms, rounds, visits, memory, bridge 1 checked on the
full volume, voxels owned -- the owner stage's traffic floor, and route_paths3d on the joint field
(span 0 and 64).  --joint-only skips everything else (the run to put under rocprofv3
--kernel-trace for the owner stage's kernel times).
usage: python tools/time_route3d.py [--R R] [--nz NZ] [--queries Q] [--lam L] [--reps K]
       [--tile-xy T ..] [--tile-z T ..] [--inner I ..] [--smooth SPAN ..] [--joint G]
       [--joint-only]"""
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
    ap.add_argument("--joint", type=int, default=0, metavar="G",
                    help="time the joint field of G vertiports against the per-goal fields")
    ap.add_argument("--joint-only", action="store_true",
                    help="with --joint: skip the sweep, the paths and the smoothing rows")
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
    if a.joint and a.joint_only:
        joint_rows(a, cfg, eng, volume, None, None, None, np, torch)
        return
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
    if a.joint:
        joint_rows(a, cfg, eng, volume, f, s, gi, np, torch)
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


def joint_rows(a, cfg, eng, volume, centre, s, gi, np, torch):
    """The --joint rows: one sample each of the per-goal and the joint field for the same
    vertiports, twice over (the repeat's spread), the owner stage's traffic floor, then the
    paths (centre: the centre goal's own field, None with --joint-only)."""
    from uam_path_planning_amd.engine import RouteField3D
    from uam_path_planning_amd.synthetic import random_pairs3d

    geo = volume.geo
    for key, default in (("k9v_tile_xy", 8), ("k9v_tile_z", 4), ("k9v_inner", 64)):
        eng.set_option(key, default)
    # the vertiports: the first G candidates in free voxels (the free bits of the same parameters)
    cand = random_pairs3d(8 * a.joint + 64, seed=4, zmin=cfg["z0"],
                          zmax=cfg["z0"] + a.nz * cfg["dz"])[:, :3]
    probe = RouteField3D(geo, None, None, None, 0, 0, volume.buf, float(a.lam))
    words = eng.route_free_bits3d(probe).cpu().numpy().view(np.uint32)
    ix = np.floor((cand[:, 0] - geo.x0) * (1.0 / geo.dx)).astype(np.int64)
    iy = np.floor((geo.y_top - cand[:, 1]) * (1.0 / geo.dy)).astype(np.int64)
    iz = np.floor((cand[:, 2] - geo.z0) * (1.0 / geo.dz)).astype(np.int64)
    inside = (ix >= 0) & (ix < geo.nx) & (iy >= 0) & (iy < geo.ny) & (iz >= 0) & (iz < geo.nz)
    v = np.where(inside, (iy * geo.nx + ix) * geo.nz + iz, 0)
    free = inside & ((words[v >> 5] >> (v & 31).astype(np.uint32)) & 1).astype(bool)
    ports = cand[free][:a.joint]
    G = len(ports)
    voxels = geo.nx * geo.ny * geo.nz

    def wall(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return out, round((time.perf_counter() - t0) * 1e3, 2)

    jf = None
    for rep in range(2):
        row = {"joint_ports": G, "sample": rep}
        if not a.joint_only:
            per, ms_per = wall(lambda: eng.route_field3d(volume, ports, lam=a.lam))
            row.update(per_goal_ms=ms_per, per_goal_rounds=per.rounds,
                       per_goal_visits=per.visits, per_goal_bytes=G * voxels * 9)
        jf = None
        jf, ms_joint = wall(lambda: eng.route_field3d(volume, ports, lam=a.lam, joint=True))
        owner = jf.owner
        row.update(joint_ms=ms_joint, joint_rounds=jf.rounds, joint_visits=jf.visits,
                   joint_bytes=voxels * 13, joint_workspace_parent_bytes=voxels * 4,
                   owners=int(torch.unique(owner[owner >= 0]).numel()),
                   voxels_owned=int((owner >= 0).sum()),
                   voxels_with_a_route_but_no_owner=int(((owner < 0)
                                                         & (jf.next[0] != 255)).sum()))
        if not a.joint_only:
            row.update(ratio=round(ms_per / ms_joint, 2),
                       bridge_1=bool(torch.equal(jf.dist[0].view(torch.int64),
                                                 per.dist.min(dim=0).values.view(torch.int64))))
            assert row["bridge_1"], "the joint field is not the minimum of the per-goal fields"
            del per
        print(json.dumps(row), flush=True)
    # the owner stage's traffic floor, counted as DESIGN section 4 K9j counts it: per voxel the
    # parent launch's 1 B read of next and 4 B + 4 B writes of parent and owner, one 4-B read of
    # the parent volume per jump round, the last launch's 4 B read and 4 B write
    jumps = max(voxels - 1, 0).bit_length()
    per_voxel = 1 + 4 + 4 + 4 * jumps + 4 + 4
    print(json.dumps({"owner_stage_jump_rounds": jumps, "owner_stage_floor_bytes_per_voxel":
                      per_voxel, "owner_stage_floor_ms":
                      round(per_voxel * voxels / HBM_BYTES_PER_S * 1e3, 4)}), flush=True)
    if a.joint_only:
        return
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def timed(fn, reps=3):
        out = fn()
        torch.cuda.synchronize()
        ms = []
        for _ in range(reps):
            e0.record()
            out = fn()
            e1.record()
            torch.cuda.synchronize()
            ms.append(round(e0.elapsed_time(e1), 3))
        return out, ms

    for span in (0, 64):
        o, ms_per = timed(lambda: eng.route_paths3d(centre, s, gi, smooth=span))
        j, ms_joint = timed(lambda: eng.route_paths3d(jf, s, smooth=span))
        st = j["status"].cpu().numpy()
        steps = j["steps"].cpu().numpy()
        print(json.dumps({
            "joint_paths_span": span, "queries": a.queries, "per_goal_ms_each": ms_per,
            "joint_ms_each": ms_joint,
            "status_counts": {int(k): int((st == k).sum()) for k in np.unique(st)},
            "steps_mean": float(steps[st == 0].mean()) if (st == 0).any() else None,
            "per_goal_steps_mean": float(o["steps"][o["status"] == 0].double().mean())}),
            flush=True)


if __name__ == "__main__":
    main()
