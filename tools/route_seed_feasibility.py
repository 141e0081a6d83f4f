"""Does a route seed help refinement on the cfg3 map?  tools/time_refine.py's set-up (the cfg3
map, random pairs, endpoints outside every no-fly shape, default refine settings) with the
goals drawn from a small set of vertiports so that one cost-to-go field serves many pairs.
Refines the 5 arc candidates of every pair, and separately the route seed
(Engine.route_field -> route_paths), and prints the share of pairs whose best candidate reaches
sum g^2 <= 1e-3 with the arcs alone and with the arcs plus the seed, for n_restart 0 and 1,
plus the seed's own share.  --smooth SPAN .. repeats the seed's rows per span of
route_paths(..., smooth=SPAN) (0: the unsmoothed trace), with the mean vertices per path.
usage: python tools/route_seed_feasibility.py [--pairs Q] [--ports V] [--N N] [--R R]
       [--lam L] [--inflate I] [--seed S] [--smooth SPAN ..]"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=20000)
    ap.add_argument("--ports", type=int, default=16, help="vertiports the goals are drawn from")
    ap.add_argument("--N", type=int, default=80)
    ap.add_argument("--R", type=int, default=4096, help="raster edge in cells")
    ap.add_argument("--nfz", type=int, default=64)
    ap.add_argument("--lam", type=float, default=1.0, help="weight of phi in the cell cost")
    ap.add_argument("--inflate", type=int, default=1)
    ap.add_argument("--seed", type=int, default=3)
    ap.add_argument("--threshold", type=float, default=1e-3)
    ap.add_argument("--smooth", type=int, nargs="*", default=[0],
                    help="spans of route_paths' smooth (0: none), one set of seed rows each")
    a = ap.parse_args()
    import numpy as np
    import torch

    from uam_path_planning_amd.arcs import arc_table
    from uam_path_planning_amd.engine import Engine
    from uam_path_planning_amd.geometry import compile_map
    from uam_path_planning_amd.scenario import (build_region_map, canonical_params,
                                                canonical_spec, displacements, raster_geo)
    from uam_path_planning_amd.synthetic import random_pairs, synthetic_dem

    spec = canonical_spec(nfz_polygons=a.nfz)
    eng = Engine(0)
    eng.set_geometry(compile_map(build_region_map(spec)))
    eng.set_params(canonical_params(spec, N=a.N, anchor=tuple(spec["x_start"])))

    def feasible(pts):
        pe = eng.eval_points(torch.tensor(pts, device="cuda"), want=("psi_raw", "collide"))
        return ((pe["psi_raw"] == 0) & (pe["collide"] == 0)).cpu().numpy()

    # vertiports: the first --ports feasible points of a seeded draw; starts likewise
    cand = random_pairs(8 * a.ports + 64, seed=a.seed + 1)[:, :2]
    ports = cand[feasible(cand)][:a.ports]
    starts = random_pairs(a.pairs, seed=a.seed)[:, :2]
    ok = feasible(starts)
    starts = starts[ok]
    Q = len(starts)
    gi = np.random.default_rng(a.seed + 2).integers(0, len(ports), size=Q).astype(np.int32)
    pairs = np.concatenate([starts, ports[gi]], axis=1)

    raster = eng.raster_build(raster_geo(a.R), synthetic_dem(a.R), packed=False)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    field = eng.route_field(raster, ports, lam=a.lam, inflate=a.inflate)
    torch.cuda.synchronize()
    t_field = time.perf_counter() - t0
    seeds = {span: eng.route_paths(field, starts, gi, smooth=span) for span in a.smooth}
    seed = seeds[a.smooth[0]]
    status = seed["status"].cpu().numpy()
    arcs = eng.gen_paths(torch.tensor(pairs, device="cuda"), arc_table(a.N, displacements(5)))
    seed_hits = eng.eval_waypoints(seed["wp"], raster=raster)["nfz_hits"].cpu().numpy()
    arc_hits = eng.eval_waypoints(arcs, raster=raster)["nfz_hits"].cpu().numpy().reshape(Q, 5)
    out = {"pairs_feasible_endpoints": Q, "ports": len(ports), "N": a.N, "R": a.R,
           "lam": a.lam, "inflate": a.inflate, "threshold": a.threshold,
           "route_field_s": t_field, "route_rounds": field.rounds, "route_visits": field.visits,
           "seed_status_counts": {int(k): int((status == k).sum()) for k in np.unique(status)},
           "seed_unrefined_share_nfz_free": float((seed_hits[status == 0] == 0).mean()),
           "pairs_share_with_an_nfz_free_arc": float((arc_hits == 0).any(axis=1).mean())}
    ok = status == 0
    for span, sd in seeds.items():
        if span:
            hits = eng.eval_waypoints(sd["wp"], raster=raster)["nfz_hits"].cpu().numpy()
            out[f"smooth_{span}"] = {
                "vertices_mean": float(sd["vertices"].cpu().numpy()[ok].mean()),
                "steps_mean": float(sd["steps"].cpu().numpy()[ok].mean()),
                "seed_unrefined_share_nfz_free": float((hits[ok] == 0).mean())}
    for n_restart in (0, 1):
        rp = {"n_restart": n_restart}
        ia = eng.refine(arcs, rp)["infeas"].cpu().numpy().reshape(Q, 5).min(axis=1)
        for span, sd in seeds.items():
            isd = eng.refine(sd["wp"], rp)["infeas"].cpu().numpy()
            isd = np.where(ok, isd, np.inf)   # a failed seed is the straight line: no seed
            key = f"n_restart_{n_restart}" + (f"_smooth_{span}" if span else "")
            out[key] = {
                "pairs_share_arcs": float((ia <= a.threshold).mean()),
                "pairs_share_arcs_plus_seed": float((np.minimum(ia, isd) <= a.threshold).mean()),
                "seed_share": float((isd <= a.threshold).mean()),
                "seed_rescues": int(((isd <= a.threshold) & (ia > a.threshold)).sum()),
                "seed_median_infeas": float(np.median(isd[np.isfinite(isd)])) if
                np.isfinite(isd).any() else None,
                "arcs_median_best_infeas": float(np.median(ia))}
            print(json.dumps({key: out[key]}), flush=True)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
