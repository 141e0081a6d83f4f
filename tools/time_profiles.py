#!/usr/bin/env python3
"""Time the fused altitude-profile evaluation (K4p, Engine.eval_generated3d_profiles) on the
cfg5 volume (1024^2 x 64 layers, 100k pairs, D = 5) for A in {1, 2, 4, 8} lift profiles, against
the same work without sharing: A separate eval_generated3d calls on pairs whose end altitudes
are shifted by the lift heights, once in the K4 form (no packed copy) and once in K4h.  The
shifted pairs fly the straight climb at another height, not the lift's ramp: the comparison is
of the work (A x Q x D paths through the same volume), not of the bits.  Last, the same lift
tables in the sorted form on the packed copy (K4hp, packed=True): one call that flies the
profiles themselves and selects over D x A, where the K4h column is a stand-in.  Beside each fused
form its form with the vertical terms (K4p+v: 3-D length, turn and climb rows per profile), and
for A = 1 the explicit forms K4e / K4e+v on the same waypoints.  --vertical alone times the
calls that charge the climb side by side: K4p+v, then on the packed copy K4hp (no vertical
terms), K4hp+v (eval_generated3d_profiles_hv) and K4hp+v's exact form.

Times are HIP events on the launch stream around --steps calls after --warmup, the median of
--repeats such windows.  One JSON line per measurement; needs an MI355X.

    python tools/time_profiles.py                  # the table
    python tools/time_profiles.py --only-fused 8   # one fused form alone (for rocprofv3)
    python tools/time_profiles.py --only-fused 8 --vertical    # ... with the vertical terms
    python tools/time_profiles.py --vertical       # K4p+v beside K4hp, K4hp+v and its exact form
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=100_000)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--only-fused", type=int, default=0, metavar="A",
                    help="run only the fused call with A profiles (a profiler's target)")
    ap.add_argument("--vertical", action="store_true",
                    help="with --only-fused: the form with the vertical terms (K4p+v); alone: "
                         "the vertical comparison, K4p+v / K4hp / K4hp+v / K4hp+v exact")
    ap.add_argument("--pair-order", type=int, default=1, choices=(0, 1),
                    help="the pair_order option (K4 / K4p: pairs in a spatial order)")
    args = ap.parse_args()

    import torch

    from uam_path_planning_amd import build, profiles
    from uam_path_planning_amd.arcs import arc_table
    from uam_path_planning_amd.engine import Engine, Vertical
    from uam_path_planning_amd.geometry import compile_map
    from uam_path_planning_amd.scenario import (CONFIGS, build_region_map, canonical_params,
                                                canonical_spec, displacements, layer_weights,
                                                raster_geo)
    from uam_path_planning_amd.synthetic import random_pairs3d, synthetic_dem

    if not torch.cuda.is_available():
        sys.exit("time_profiles.py needs a GPU")
    build.build_library()
    cfg = CONFIGS["cfg5"]
    R, D, N, Q = cfg["R"], cfg["D"], cfg["N"], args.pairs
    W = N + 2
    spec = canonical_spec(nfz_polygons=cfg["nfz_polygons"])
    eng = Engine(0)
    eng.set_geometry(compile_map(build_region_map(spec)))
    eng.set_params(canonical_params(spec, N=N, altitude=320.0))
    eng.set_option("pair_order", args.pair_order)
    raster = eng.raster_build(raster_geo(R), eng.tensor(synthetic_dem(R), torch.float32),
                              summary=False)
    volume = eng.volume_build(raster, cfg["nz"], cfg["z0"], cfg["dz"], layer_weights(cfg["nz"]))
    pairs_host = random_pairs3d(Q, seed=0)
    ut = eng.tensor(arc_table(N, displacements(D)), torch.float64)
    heights = [0.0, 40.0, 80.0, 120.0, -40.0, -80.0, 20.0, 60.0]   # pairs fly at 100 .. 500 m

    def timed(fn):
        for _ in range(args.warmup):
            fn()
        torch.cuda.synchronize()
        ms = []
        for _ in range(args.repeats):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.steps):
                fn()
            e1.record()
            torch.cuda.synchronize()
            ms.append(e0.elapsed_time(e1) / args.steps)
        return statistics.median(ms), min(ms), max(ms)

    def report(form, A, t, kernel):
        med, lo, hi = t
        print(json.dumps({"form": form, "A": A, "pairs": Q, "D": D, "N": N, "paths": Q * D * A,
                          "ms_per_call_set": round(med, 4), "ms_min": round(lo, 4),
                          "ms_max": round(hi, 4),
                          "ns_per_waypoint": round(med * 1e6 / (Q * D * A * W), 4),
                          "pair_order": args.pair_order,
                          "kernel": kernel}), flush=True)

    pairs = eng.tensor(pairs_host, torch.float64)
    # isotropic, climbs and descents limited to 10 degrees: every term of the definition runs
    vert = Vertical(1e-3, profiles.sin_of_angle(10.0), profiles.sin_of_angle(10.0))
    for A in ([args.only_fused] if args.only_fused else [1, 2, 4, 8]):
        zt = eng.tensor(profiles.stack(*[profiles.lift(N, h) for h in heights[:A]]),
                        torch.float64)
        outs = eng.outputs(Q * D * A, W, n_pairs=Q)

        def fused():
            eng.eval_generated3d_profiles(pairs, ut, zt, volume, outputs=outs)

        def fused_v():
            eng.eval_generated3d_profiles(pairs, ut, zt, volume, outputs=outs, vertical=vert)

        if not args.vertical:
            report("fused", A, timed(fused), eng.last_kernel())
        if not args.only_fused or args.vertical:
            report("fused+v", A, timed(fused_v), eng.last_kernel())
        del outs
        # the explicit forms on the same waypoints
        if A == 1 and not args.only_fused and not args.vertical:
            wp3 = eng.gen_paths3d(pairs, ut, zt)
            eng.set_option("wave_max_paths", 0)
            report("explicit", A, timed(lambda: eng.eval_waypoints3d(wp3, volume)),
                   eng.last_kernel())
            report("explicit+v", A,
                   timed(lambda: eng.eval_waypoints3d(wp3, volume, vertical=vert)),
                   eng.last_kernel())
            del wp3
    if args.only_fused:
        return
    if args.vertical:   # the vertical comparison alone: K4p+v above, then K4hp, K4hp+v and its
        #                 exact form on the packed copy
        eng.volume_pack(volume)
        for A in (1, 2, 4, 8):
            zt = eng.tensor(profiles.stack(*[profiles.lift(N, h) for h in heights[:A]]),
                            torch.float64)
            outs = eng.outputs(Q * D * A, W, n_pairs=Q)

            def packed():
                eng.eval_generated3d_profiles(pairs, ut, zt, volume, outputs=outs, packed=True)

            def packed_v():
                eng.eval_generated3d_profiles_hv(pairs, ut, zt, volume, vert, outputs=outs)

            report("packed", A, timed(packed), eng.last_kernel())
            report("packed+v", A, timed(packed_v), eng.last_kernel())
            eng.set_option("exact_sum_volume", 1)
            report("packed+v exact", A, timed(packed_v), eng.last_kernel())
            eng.set_option("exact_sum_volume", 0)
            del outs
        return

    # the same work without sharing: A calls on pairs with shifted end altitudes
    shifted = []
    for h in heights:
        p = pairs_host.copy()
        p[:, 2] += h
        p[:, 5] += h
        shifted.append(eng.tensor(p, torch.float64))
    outs = eng.outputs(Q * D, W, n_pairs=Q)
    for form in ("K4", "K4h"):
        if form == "K4h":
            eng.volume_pack(volume)          # K4h reads the packed copy; K4 runs without one
        for A in (1, 2, 4, 8):
            def separate():
                for a in range(A):
                    eng.eval_generated3d(shifted[a], ut, volume, outputs=outs)

            t = timed(separate)
            report("separate " + form, A, t, eng.last_kernel())
    del outs
    # the profiles themselves in the sorted form (the volume is packed by now)
    for A in (1, 2, 4, 8):
        zt = eng.tensor(profiles.stack(*[profiles.lift(N, h) for h in heights[:A]]),
                        torch.float64)
        outs = eng.outputs(Q * D * A, W, n_pairs=Q)

        def packed():
            eng.eval_generated3d_profiles(pairs, ut, zt, volume, outputs=outs, packed=True)

        report("packed", A, timed(packed), eng.last_kernel())
        del outs


if __name__ == "__main__":
    main()
