"""uam_eval_generated3d_profiles_hv (K4hp+v) without a GPU: the symbol (header, _lib.SIGNATURES
and the built library agree), the clauses of its definition in the header, the numpy restatement
of that definition (profiles_hv_ref.py) pinned to the oracle's sequential x/y bits at kappa = 0,
and -- by the reference alone -- how far the grouped costs lie from the sequential K4p+v ones and
that the inputs of the GPU tests tell the forms apart."""
import ctypes
import math
import os
import re

import numpy as np
import pytest

import profiles_h_ref as H
import profiles_hv_ref as HV
import profiles_ref as R
import vertical_ref as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
Q = 130


def _spec():
    from uam_path_planning_amd.scenario import canonical_spec

    return canonical_spec(nfz_polygons=16)


def _oracle(oracle_mod, N):
    spec = _spec()
    opts = dict(spec["options"])
    opts["maxratio_smooth"] = False
    return oracle_mod.Oracle(oracle_mod.compile_spec(spec), N, opts, spec["maxratio"],
                             spec["maxalpha"], spec["enlargement"], spec["weights"],
                             altitude=320.0)


def _geo():
    """The oracle's geometry parameters: the quirk with the anchor at p_0."""
    spec = _spec()
    return V.Geo(length_smooth=bool(spec["options"]["length_smooth"]), maxratio_smooth=False,
                 maxratio=spec["maxratio"], maxalpha=spec["maxalpha"])


def _utab(N, D):
    from uam_path_planning_amd.arcs import arc_table

    return arc_table(N, np.linspace(-0.6, 0.6, D) if D > 1 else np.array([0.3]))


def _family(N, order=None):
    from uam_path_planning_amd import profiles as P

    fam = R.family(P, N)
    return fam if order is None else np.ascontiguousarray(fam[order])


def _same(got, want, what):
    """Bit equality; any NaN equals any NaN."""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape, what
    if want.dtype == np.float64:
        n = np.isnan(want)
        np.testing.assert_array_equal(np.isnan(got), n, err_msg=what)
        got = np.where(n, 0.0, got).view(np.uint64)
        want = np.where(n, 0.0, want).view(np.uint64)
    np.testing.assert_array_equal(got, want, err_msg=what)


def _differ(a, b):
    """Rows whose float64 bits differ (a NaN equals a NaN)."""
    n = np.isnan(a) & np.isnan(b)
    return (np.where(n, 0.0, a).view(np.uint64) != np.where(n, 0.0, b).view(np.uint64))


# ---- the ABI ----------------------------------------------------------------------------------
def test_symbol_and_prototype():
    from uam_path_planning_amd import _lib, build

    build.build_library()
    lib = _lib.load()
    with open(os.path.join(ROOT, "include", "uampath.h")) as f:
        text = re.sub(r"/\*.*?\*/", " ", f.read(), flags=re.S)
    text = re.sub(r"\s+", " ", text)
    proto = ("int uam_eval_generated3d_profiles_hv(uam_ctx* ctx, const uam_volume_desc* desc, "
             "const void* vol_dev, const void* packed_dev, const double* pairs6_dev, "
             "int64_t n_pairs, const double* utab_dev, int32_t D, const double* ztab_dev, "
             "int32_t A, const uam_vertical* vert, const uam_path_outputs* out, "
             "double* climb_sum_dev , uam_stream stream);")
    assert proto in text
    vp, i32, i64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64
    vd, po = ctypes.POINTER(_lib.VolumeDesc), ctypes.POINTER(_lib.PathOutputs)
    ve = ctypes.POINTER(_lib.Vertical)
    args = [vp, vd, vp, vp, vp, i64, vp, i32, vp, i32, ve, po, vp, vp]
    name = "uam_eval_generated3d_profiles_hv"
    assert _lib.SIGNATURES[name] == (ctypes.c_int, args)
    # uam_eval_generated3d_profiles_h's arguments, vert before out and climb_sum after it
    h = _lib.SIGNATURES["uam_eval_generated3d_profiles_h"][1]
    assert args == h[:10] + [ve, h[10], vp, h[11]]
    fn = getattr(lib, name)
    assert fn.restype is ctypes.c_int and list(fn.argtypes) == args
    assert lib.uam_abi_version() == _lib.ABI_VERSION == 2     # no ABI bump, no new option
    assert max(_lib.OPTIONS.values()) == 24
    # no GPU is touched by a NULL context: the argument check answers
    v = _lib.Vertical(2, 1e-3, math.inf, math.inf)
    assert fn(None, None, None, None, None, 0, None, 1, None, 1, ctypes.byref(v), None, None,
              None) == _lib.UAM_E_INVALID
    assert fn(None, None, None, None, None, 0, None, 1, None, 1, None, None, None,
              None) == _lib.UAM_E_INVALID


def test_header_states_the_definition():
    with open(os.path.join(ROOT, "include", "uampath.h")) as f:
        text = re.sub(r"[\s*]+", " ", f.read())
    start = text.index("Vertical terms for the profiles on the packed, sorted volume")
    sec = text[start:text.index("int uam_eval_generated3d_profiles_hv(", start)]
    for clause in (
            "Every float64 operation is rounded, none is contracted",
            "p = (q D + d) A + a, c = d A + a, 1 <= A <= 8, D <= 16",
            "ztab_dev == NULL with A = 1 is the straight climb",
            "length_q, length, kin_sum and climb_sum are the uam_vertical loop above over those "
            "points, sequentially, j = 1 .. N+1",
            "the bits uam_eval_generated3d_profiles_v gives for the same inputs",
            "They differ among the A profiles of a lateral candidate",
            "K4hp's group order with the 3-D L as the base: cost = ((N+1) L + P_0) + P_1 + ...",
            "nfz_sum, nfz_hits, offmap, below_terrain, min_clearance: K4hp's, bit for bit",
            "uam_argmin's rule over the pair's D A candidates on the new cost and the new length",
            "best_length_idx need not be a multiple of A",
            "equal uam_eval_generated3d_profiles' sequential x/y bits (not K4hp's "
            "similarity-form bits), and climb_sum is +0",
            "uam_last_group reports G",
            "\"K4hpv+pack\"", "\"K4hpxv+pack\"",
            "cost = (double)(N+1) L + fl(S_risk) / (double)N",
            "UAM_E_STATE when no volume sum scale is set",
            "before any launch or allocation",
            "a path's bits do not depend on the batch it is in",
            "prefixed \"uam_eval_generated3d_profiles_hv needs K4hpv\"",
            "maxratio_smooth is taken",
            "UAM_OPT_K2G_SIM is not read",
            "UAM_E_INVALID for vert == NULL, UAM_E_VERSION for a wrong abi_version",
            "climb_sum is NaN like the other float64 outputs"):
        assert clause in sec, clause
    # K4hp's own section keeps its clause, qualified after the words
    k4hp = text[text.index("Altitude-profile candidates on the packed, sorted volume"):start]
    assert "there is no _v variant of this definition; uam_eval_generated3d_profiles_hv" in k4hp


def test_python_layer_has_the_method_and_keeps_the_refusal():
    import inspect

    from uam_path_planning_amd.engine import Engine

    sig = inspect.signature(Engine.eval_generated3d_profiles_hv)
    assert list(sig.parameters) == ["self", "pairs6", "utab", "ztab", "volume", "vertical",
                                    "outputs"]
    assert sig.parameters["outputs"].default is None
    src = inspect.getsource(Engine.eval_generated3d_profiles)
    assert "packed=True has no vertical form" in src and "eval_generated3d_profiles_hv" in src
    assert "K4hpv+pack" in Engine.last_kernel.__doc__


# ---- kappa = 0, the oracle-pinned anchor ---------------------------------------------------------
@pytest.mark.parametrize("N,D,G", [(9, 5, 4), (40, 5, 21), (1, 1, 21)])
def test_zero_scale_geometry_is_the_oracles_sequential_one(oracle_mod, N, D, G):
    """With kappa = 0 and finite altitudes the restatement's length_q, length and kin_sum are
    eval_paths3d's sequential x/y bits -- not the similarity form's, which differ -- climb_sum
    is +0, and what the vertical terms do not touch is K4hp's."""
    orc = _oracle(oracle_mod, N)
    vox, cols = R.hand_volume()
    pr = R.pairs6(Q)          # (finite altitudes; one pair holds a NaN y)
    assert np.isfinite(pr[:, [2, 5]]).all()
    ut, zt = _utab(N, D), _family(N)
    A = zt.shape[0]
    base = H.evaluate(oracle_mod, orc, vox, cols, pr, ut, zt, G)
    seq = orc.eval_paths3d(H.waypoints(oracle_mod, pr, ut, zt), R.volume_desc(oracle_mod),
                           R.host_volume(vox, cols))
    for lim in (math.inf, 0.0, 0.1):
        got = HV.evaluate(oracle_mod, orc, vox, cols, pr, ut, zt, G, _geo(),
                          V.Vert(0.0, lim, lim), base=base)
        _same(got["length_q"], seq["lq"], "length_q")
        _same(got["length_q"], base["sequential_length_q"], "length_q")
        _same(got["length"], seq["length"], "length")
        _same(got["kin_sum"], seq["kin"], "kin_sum")
        assert not got["climb_sum"].any() and not np.signbit(got["climb_sum"]).any()
        for k in HV.UNTOUCHED:
            _same(got[k], base[k], k)
        assert got["best_fval_idx"].shape == (pr.shape[0],) and got["best_fval_idx"].max() < D * A
    if N > 1:   # the anchor is worth having: the similarity form's bits are others
        assert _differ(got["length"], base["length"]).any()


# ---- grouped against sequential, by the reference alone -----------------------------------------
_CASES = {}


def _case(oracle_mod, N, D, G, kappa, order=None):
    """(restatement, K4hp's restatement, the sequential K4p+v reference) of the 130 pairs x D
    arcs x the 8-profile family, limits 0.1; cached."""
    key = (N, D, G, kappa, None if order is None else tuple(order))
    if key not in _CASES:
        bkey = key[:3] + key[4:]
        if bkey not in _CASES:
            orc = _oracle(oracle_mod, N)
            vox, cols = R.hand_volume()
            pr, ut, zt = R.pairs6(Q), _utab(N, D), _family(N, order)
            _CASES[bkey] = (orc, vox, cols, pr, ut, zt,
                            H.evaluate(oracle_mod, orc, vox, cols, pr, ut, zt, G))
        orc, vox, cols, pr, ut, zt, base = _CASES[bkey]
        vert = V.Vert(kappa, 0.1, 0.1)
        got = HV.evaluate(oracle_mod, orc, vox, cols, pr, ut, zt, G, _geo(), vert, base=base)
        seq = V.reference_eval_v(oracle_mod, orc, vox, cols, H.waypoints(oracle_mod, pr, ut, zt),
                                 _geo(), vert, Q, D * zt.shape[0], base={"cells": base["cells"]})
        _CASES[key] = (got, base, seq)
    return _CASES[key]


@pytest.mark.parametrize("kappa", [1e-3, 1e-2])
@pytest.mark.parametrize("N,D,G", [(40, 5, 4), (40, 5, 21), (9, 5, 4)])
def test_grouped_costs_lie_within_rounding_of_the_sequential_ones(oracle_mod, N, D, G, kappa):
    """Two orders of the same W + 1 terms -- (N+1) L and the W risk terms -- so the grouped cost
    lies within 2 W 2^-53 (sum |risk_j| / N + (N+1) |L|) of vertical_ref.reference_eval_v's
    sequential cost on every finite path; the geometry is that reference's, bit for bit."""
    W = N + 2
    got, base, seq = _case(oracle_mod, N, D, G, kappa)
    for k in HV.GEO:
        _same(got[k], seq[k], k)
    cells = base["cells"]
    vox, _ = R.hand_volume()
    risk = np.abs(vox.reshape(-1, 2)[:, 0].view(np.float32).astype(np.float64))
    mag = np.where(cells >= 0, risk[np.where(cells >= 0, cells, 0)], 0.0).sum(axis=1) / N
    ok = np.isfinite(seq["cost"]) & np.isfinite(got["cost"])
    assert ok.sum() > 0.9 * ok.size
    _same(np.isfinite(seq["cost"]), np.isfinite(got["cost"]), "finite paths")
    bound = 2.0 * W * 2.0 ** -53 * (mag + (N + 1) * np.abs(got["length_q"]))
    err = np.abs(got["cost"] - seq["cost"])
    print(f"N={N} D={D} G={G} kappa={kappa}: finite {int(ok.sum())} of {ok.size}, worst "
          f"err / bound {float((err[ok] / bound[ok]).max()):.3f}")
    assert (err[ok] <= bound[ok]).all()
    # the climb is charged: some path's climb rows are positive, and the 3-D length is longer
    assert (got["climb_sum"][ok] > 0).any()
    assert (got["length"][ok] > base["length"][ok]).any()


@pytest.mark.parametrize("N,D,G", [(9, 5, 4), (40, 5, 21)])
def test_the_grouped_cost_is_not_the_sequential_one(oracle_mod, N, D, G):
    got, _, seq = _case(oracle_mod, N, D, G, 1e-3)
    ok = np.isfinite(seq["cost"])
    n = int(_differ(got["cost"], seq["cost"])[ok].sum())
    print(f"N={N} D={D} G={G}: cost bits differ on {n} of {int(ok.sum())} finite paths")
    assert n > 0


@pytest.mark.parametrize("kappa", [1e-3, 1e-2])
def test_the_vertical_terms_change_the_selection_by_cost(oracle_mod, kappa):
    got, base, _ = _case(oracle_mod, 9, 5, 4, kappa)
    n = int((got["best_fval_idx"] != base["best_fval_idx"]).sum())
    print(f"kappa={kappa}: best_fval_idx differs from K4hp's on {n} of {Q} pairs")
    assert n > 0


def test_best_length_idx_need_not_be_a_multiple_of_A(oracle_mod):
    """With the 150 m cruise as profile 0 the straight climb (profile 1) is the shorter 3-D path
    of most lateral candidates."""
    order = [1, 0] + list(range(2, 8))
    got, base, _ = _case(oracle_mod, 9, 5, 4, 1e-3, order)
    A = 8
    n = int((got["best_length_idx"] % A != 0).sum())
    print(f"best_length_idx % A != 0 on {n} of {Q} pairs")
    assert n > 0
    assert got["best_length_idx"].max() < 5 * A
