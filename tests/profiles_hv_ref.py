"""The definition of uam_eval_generated3d_profiles_hv (include/uampath.h, "Vertical terms for the
profiles on the packed, sorted volume") restated in numpy from existing pieces only: the reference
of test_profiles_hv_cpu.py and test_gpu_profiles_hv.py.

  * profiles_h_ref.evaluate gives the voxel of every waypoint and the outputs the vertical terms
    do not touch (nfz_sum, nfz_hits, offmap, below_terrain, min_clearance);
  * vertical_ref.geometry on profiles_h_ref.waypoints gives length_q, length, kin_sum and
    climb_sum, sequentially per path;
  * cost is profiles_h_ref.grouped_sum on the base (N+1) L (the exact variant: the base plus
    profiles_h_ref._exact_field's fl(S_risk), truly divided by N);
  * the selections are oracle.argmin over D*A on the new cost and length."""
import numpy as np

import exact_sum_ref as X
import profiles_h_ref as H
import vertical_ref as V

KEYS = H.KEYS + ("climb_sum",)
BEST = H.BEST
GEO = ("length_q", "length", "kin_sum", "climb_sum")
UNTOUCHED = ("nfz_sum", "min_clearance", "nfz_hits", "offmap", "below_terrain")


def evaluate(oracle_mod, orc, vox, cols, pr6, ut, ztab, G, geo, vert, exact=False, base=None):
    """Every output of the definition for pr6 [Q, 6] x ut [D, N, 2] x ztab [A, W, 3] (None: the
    straight climb, A = 1), group length G, under geo (vertical_ref.Geo) and vert
    (vertical_ref.Vert).  orc: an oracle without maxratio_smooth (its similarity-form geometry
    is computed by profiles_h_ref.evaluate and dropped here).  base: profiles_h_ref.evaluate of
    the same (inputs, G, exact), to share it among several geo / vert."""
    pr6 = np.asarray(pr6, np.float64).reshape(-1, 6)
    ut = np.asarray(ut, np.float64)
    D, N = ut.shape[0], ut.shape[1]
    A = 1 if ztab is None else ztab.shape[0]
    if base is None:
        base = H.evaluate(oracle_mod, orc, vox, cols, pr6, ut, ztab, G, exact=exact)
    out = {k: base[k] for k in UNTOUCHED + ("cells",)}
    out.update(V.geometry(H.waypoints(oracle_mod, pr6, ut, ztab), geo, vert))
    cells = base["cells"]
    inside = cells >= 0
    words = vox.reshape(-1, 2)
    with np.errstate(invalid="ignore", over="ignore"):
        start = np.float64(N + 1) * out["length_q"]
        if exact:
            rw = words[:, 0].tolist()
            frisk = H._exact_field(rw, cells, X.exponent(rw))
            out["cost"] = start + frisk / np.float64(N)
        else:
            at = np.where(inside, cells, 0)
            risk = words[:, 0].view(np.float32)[at].astype(np.float64) / np.float64(N)
            out["cost"] = H.grouped_sum(start, risk, inside, G)
        out["best_fval_idx"] = oracle_mod.argmin(out["cost"], D * A, True)
    out["best_length_idx"] = oracle_mod.argmin(out["length"], D * A, False)
    return out
