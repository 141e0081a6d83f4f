"""Time the route seeds (K9) on the cfg3 raster: uam_route_field per UAM_OPT_K9_TILE x
UAM_OPT_K9_INNER (host wall ms of the whole call, rounds, tile visits, visits per tile) for a
goal near the centre and one in a corner, checking that every setting gives the same bits, then
uam_route_paths at --queries starts, uam_route_free_bits, and uam_route_paths_smooth per
--smooth SPAN (its bits at span 1 checked against uam_route_paths').  One JSON line per
measurement.  --joint PORTS adds the joint field (K9j) of PORTS vertiports
(tools/route_seed_feasibility.py's draw and inflate = 1) next to uam_route_field for the same
goals -- wall ms, memory, bridge 1 checked -- and route_paths on the joint field (span 0 and 64)
next to the per-goal calls on the centre goal's own field.
usage: python tools/time_route.py [--R R] [--queries Q] [--lam L] [--inflate I]
       [--smooth SPAN ..] [--no-sweep] [--joint PORTS]"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

COMBOS = [(t, i) for t in (16, 32, 64) for i in (4, 16, 32, 64)] + [
    (32, 1), (32, 128), (32, 256), (64, 128), (64, 256)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--R", type=int, default=4096)
    ap.add_argument("--queries", type=int, default=100000)
    ap.add_argument("--lam", type=float, default=1.0)
    ap.add_argument("--inflate", type=int, default=0)
    ap.add_argument("--smooth", type=int, nargs="*", default=[],
                    help="spans to time uam_route_paths_smooth at")
    ap.add_argument("--no-sweep", action="store_true",
                    help="skip the tile x inner sweep of uam_route_field")
    ap.add_argument("--joint", type=int, default=0, metavar="PORTS",
                    help="time the joint field of PORTS vertiports against the per-goal fields")
    a = ap.parse_args()
    import numpy as np
    import torch

    from uam_path_planning_amd.engine import Engine
    from uam_path_planning_amd.geometry import compile_map
    from uam_path_planning_amd.scenario import (build_region_map, canonical_params,
                                                canonical_spec, raster_geo)
    from uam_path_planning_amd.synthetic import random_pairs, synthetic_dem

    spec = canonical_spec(nfz_polygons=64)
    eng = Engine(0)
    eng.set_geometry(compile_map(build_region_map(spec)))
    eng.set_params(canonical_params(spec, N=80, anchor=tuple(spec["x_start"])))
    raster = eng.raster_build(raster_geo(a.R), synthetic_dem(a.R), packed=False)

    def free_near(x, y):
        """The first point on a fixed ray from (x, y) outside every no-fly shape."""
        for k in range(200):
            p = np.array([[x + 0.37 * k, y - 0.29 * k]])
            pe = eng.eval_points(torch.tensor(p, device="cuda"), want=("psi_raw", "collide"))
            if float(pe["psi_raw"][0]) == 0 and int(pe["collide"][0]) == 0:
                return p[0]
        raise RuntimeError("no free goal found")

    goals = {"centre": free_near(30.0, -10.0), "corner": free_near(0.4, 19.6)}
    print(json.dumps({"goals": {k: v.tolist() for k, v in goals.items()}}), flush=True)
    first = {}
    for tile, inner in ([] if a.no_sweep else COMBOS):
        for name, g in goals.items():
            eng.set_option("k9_tile", tile)
            eng.set_option("k9_inner", inner)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            f = eng.route_field(raster, g.reshape(1, 2), lam=a.lam, inflate=a.inflate)
            torch.cuda.synchronize()
            ms = (time.perf_counter() - t0) * 1e3
            ntiles = ((a.R + tile - 1) // tile) ** 2
            if name not in first:
                first[name] = (f.dist.clone(), f.next.clone())
            same = bool(torch.equal(f.dist.view(torch.int64), first[name][0].view(torch.int64))
                        and torch.equal(f.next, first[name][1]))
            print(json.dumps({"tile": tile, "inner": inner, "goal": name, "ms": round(ms, 2),
                              "rounds": f.rounds, "visits": f.visits,
                              "visits_per_tile": round(f.visits / ntiles, 2),
                              "reachable_cells": int(torch.isfinite(f.dist).sum()),
                              "same_bits_as_first": same}), flush=True)
    eng.set_option("k9_tile", 32)
    eng.set_option("k9_inner", 16)
    f = eng.route_field(raster, goals["centre"].reshape(1, 2), lam=a.lam, inflate=a.inflate)
    s = eng.tensor(random_pairs(a.queries, seed=5)[:, :2], torch.float64)
    gi = eng.tensor(np.zeros(a.queries, dtype=np.int32), torch.int32)
    eng.route_paths(f, s, gi)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    o = eng.route_paths(f, s, gi)
    e1.record()
    torch.cuda.synchronize()
    st = o["status"].cpu().numpy()
    steps = o["steps"].cpu().numpy()
    print(json.dumps({"route_paths_queries": a.queries, "ms": round(e0.elapsed_time(e1), 3),
                      "status_counts": {int(k): int((st == k).sum()) for k in np.unique(st)},
                      "steps_mean": float(steps[st == 0].mean()) if (st == 0).any() else None,
                      "steps_max": int(steps.max())}), flush=True)
    if a.joint:
        joint_rows(a, eng, raster, f, s, gi, np, torch)
    if not a.smooth:
        return

    def timed(fn, reps=3):
        """ms of each of reps calls (events around the call), after one untimed call."""
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

    _, ms = timed(lambda: eng.route_paths(f, s, gi))
    print(json.dumps({"route_paths_queries": a.queries, "ms_each": ms}), flush=True)

    def build_bits():
        f.free_bits = None
        return eng.route_free_bits(f)

    bits, ms = timed(build_bits)
    print(json.dumps({"route_free_bits": True, "ms_each": ms, "bytes": bits.numel() * 4}),
          flush=True)
    one = eng.route_paths(f, s, gi, smooth=1)
    print(json.dumps({"span_1_equals_route_paths": bool(
        torch.equal(one["wp"].view(torch.int64), o["wp"].view(torch.int64))
        and torch.equal(one["status"], o["status"]) and torch.equal(one["steps"], o["steps"]))}),
        flush=True)
    ok = torch.as_tensor(st == 0, device=o["status"].device)
    for span in a.smooth:
        sm, ms = timed(lambda: eng.route_paths(f, s, gi, smooth=span))
        v = sm["vertices"][ok].double()
        print(json.dumps({"route_paths_smooth_span": span, "queries": a.queries, "ms_each": ms,
                          "vertices_mean": float(v.mean()) if v.numel() else None,
                          "vertices_max": int(v.max()) if v.numel() else None,
                          "same_status_and_steps": bool(torch.equal(sm["status"], o["status"])
                                                        and torch.equal(sm["steps"],
                                                                        o["steps"]))}),
              flush=True)


def joint_rows(a, eng, raster, centre, s, gi, np, torch):
    """The --joint rows: one sample each of the per-goal and the joint field for the same
    vertiports, twice over (the repeat's spread), then the paths."""
    from uam_path_planning_amd.synthetic import random_pairs

    cand = random_pairs(8 * a.joint + 64, seed=4)[:, :2]
    pe = eng.eval_points(torch.tensor(cand, device="cuda"), want=("psi_raw", "collide"))
    ok = ((pe["psi_raw"] == 0) & (pe["collide"] == 0)).cpu().numpy()
    ports = cand[ok][:a.joint]
    cells = a.R * a.R

    def wall(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return out, round((time.perf_counter() - t0) * 1e3, 2)

    for rep in range(2):
        per, ms_per = wall(lambda: eng.route_field(raster, ports, lam=a.lam, inflate=1))
        jf, ms_joint = wall(lambda: eng.route_field(raster, ports, lam=a.lam, inflate=1,
                                                    joint=True))
        owner = jf.owner
        print(json.dumps({
            "joint_ports": len(ports), "sample": rep, "per_goal_ms": ms_per,
            "joint_ms": ms_joint, "ratio": round(ms_per / ms_joint, 2),
            "per_goal_rounds": per.rounds, "joint_rounds": jf.rounds,
            "per_goal_visits": per.visits, "joint_visits": jf.visits,
            "per_goal_bytes": len(ports) * cells * 9, "joint_bytes": cells * 13,
            "joint_workspace_parent_bytes": cells * 4,
            "bridge_1": bool(torch.equal(jf.dist[0].view(torch.int64),
                                         per.dist.min(dim=0).values.view(torch.int64))),
            "owners": int(torch.unique(owner[owner >= 0]).numel()),
            "cells_owned": int((owner >= 0).sum()),
            "cells_with_a_route_but_no_owner": int(((owner < 0) & (jf.next[0] != 255)).sum())}),
            flush=True)
        del per
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
        o, ms_per = timed(lambda: eng.route_paths(centre, s, gi, smooth=span))
        j, ms_joint = timed(lambda: eng.route_paths(jf, s, smooth=span))
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
