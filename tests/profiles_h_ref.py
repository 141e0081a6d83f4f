"""The definition of uam_eval_generated3d_profiles_h (include/uampath.h, "Altitude-profile
candidates on the packed, sorted volume") restated in numpy from oracle outputs only: the
reference of test_profiles_h_cpu.py and test_gpu_profiles_h.py.

  * Oracle.eval_paths3d(want_cells=True) on profiles_ref.reference_wp3 gives the voxel index of
    every waypoint (-1 outside the volume) and the order-independent outputs (nfz_hits, offmap,
    below, min_clearance), which are the expected values themselves;
  * Oracle.eval_generated_h(mode="volume", group=G) gives lq, length and kin per (q, d), repeated
    over the A profiles;
  * cost and nfz_sum are the grouped partial sums over the voxel words at those indices, each
    numpy operation rounded on its own;
  * the selections are oracle.argmin over D*A;
  * the exact variant takes its sums from exact_sum_ref (Python integers and Fraction)."""
import numpy as np

import exact_sum_ref as X
import profiles_ref as R

KEYS = ("cost", "length_q", "length", "kin_sum", "nfz_sum", "min_clearance", "nfz_hits", "offmap",
        "below_terrain")
BEST = ("best_fval_idx", "best_length_idx")


def grouped_sum(acc, term, inside, G):
    """acc + P_0 + P_1 + ... per row: P_k the sum from +0.0, in column order, of term over the
    columns of [k G, min((k+1) G, W)) that are inside."""
    W = term.shape[1]
    acc = np.array(acc, np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        for k in range(0, W, G):
            p = np.zeros(term.shape[0])
            for j in range(k, min(k + G, W)):
                p = np.where(inside[:, j], p + term[:, j], p)
            acc = acc + p
    return acc


def _exact_field(words, cells, e):
    """fl(S) of the words at each row's cells (-1: nothing) at exponent e."""
    out = np.empty(cells.shape[0])
    for p, row in enumerate(cells.tolist()):
        pw = [words[c] for c in row if c >= 0]
        S = sum(X.term(w, e) for w in pw if (w >> 23) & 255 != 255)
        out[p] = X.result(S, X.flags(pw), e)
    return out


def waypoints(oracle_mod, pr6, ut, ztab):
    """wp3 [Q*D*A, W, 3]; ztab None: A = 1 on oracle.gen_paths3d's straight climb."""
    if ztab is None:
        return oracle_mod.gen_paths3d(pr6, ut)
    return R.reference_wp3(oracle_mod, pr6, ut, ztab)


def evaluate(oracle_mod, orc, vox, cols, pr6, ut, ztab, G, exact=False, vdesc=None):
    """Every output of the definition for pr6 [Q, 6] x ut [D, N, 2] x ztab [A, W, 3] (None: the
    straight climb, A = 1) on the voxels vox [ny, nx, nz, 2] / cols [ny, nx, 2] (uint32 words),
    group length G; exact: the UAM_OPT_EXACT_SUM_VOLUME form."""
    pr6 = np.asarray(pr6, np.float64).reshape(-1, 6)
    ut = np.asarray(ut, np.float64)
    Q, D, N = pr6.shape[0], ut.shape[0], ut.shape[1]
    A = 1 if ztab is None else ztab.shape[0]
    vd = vdesc if vdesc is not None else R.volume_desc(oracle_mod)
    host = R.host_volume(vox, cols)
    seq = orc.eval_paths3d(waypoints(oracle_mod, pr6, ut, ztab), vd, host, want_cells=True)
    geo = orc.eval_generated_h(pr6, ut, mode="volume", vdesc=vd, vol=host, group=G)
    out = {"length_q": np.repeat(geo["lq"], A), "length": np.repeat(geo["length"], A),
           "kin_sum": np.repeat(geo["kin"], A), "nfz_hits": seq["nfz_hits"],
           "offmap": seq["offmap"], "below_terrain": seq["below"],
           "min_clearance": seq["min_clearance"], "cells": seq["cells"]}
    cells = seq["cells"]
    inside = cells >= 0
    words = vox.reshape(-1, 2)
    at = np.where(inside, cells, 0)
    with np.errstate(invalid="ignore", over="ignore"):
        base = np.float64(N + 1) * out["length_q"]
        if exact:
            rw, pw = words[:, 0].tolist(), words[:, 1].tolist()
            frisk = _exact_field(rw, cells, X.exponent(rw))
            out["nfz_sum"] = _exact_field(pw, cells, X.exponent(pw))
            out["cost"] = base + frisk / np.float64(N)
        else:
            risk = words[:, 0].view(np.float32)[at].astype(np.float64) / np.float64(N)
            psi = words[:, 1].view(np.float32)[at].astype(np.float64)
            out["cost"] = grouped_sum(base, risk, inside, G)
            out["nfz_sum"] = grouped_sum(np.zeros(Q * D * A), psi, inside, G)
        out["best_fval_idx"] = oracle_mod.argmin(out["cost"], D * A, True)
    out["best_length_idx"] = oracle_mod.argmin(out["length"], D * A, False)
    out["sequential_cost"] = seq["cost"]
    out["sequential_length_q"] = seq["lq"]
    return out
