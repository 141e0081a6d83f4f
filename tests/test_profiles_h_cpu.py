"""uam_eval_generated3d_profiles_h without a GPU: the symbol (header, _lib.SIGNATURES and the
built library agree), the clauses of its definition in the header, the numpy restatement of that
definition (profiles_h_ref.py) pinned to the oracle's orc_eval_generated_h on the straight climb,
and -- by the reference alone -- how far the grouped costs lie from the sequential ones and that a
choice among the profiles changes a selection."""
import ctypes
import os
import re

import numpy as np
import pytest

import profiles_h_ref as H
import profiles_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _oracle(oracle_mod, N):
    from uam_path_planning_amd.scenario import canonical_spec

    spec = canonical_spec(nfz_polygons=16)
    opts = dict(spec["options"])
    opts["maxratio_smooth"] = False
    return oracle_mod.Oracle(oracle_mod.compile_spec(spec), N, opts, spec["maxratio"],
                             spec["maxalpha"], spec["enlargement"], spec["weights"],
                             altitude=320.0)


def _utab(N, D):
    from uam_path_planning_amd.arcs import arc_table

    return arc_table(N, np.linspace(-0.6, 0.6, D) if D > 1 else np.array([0.3]))


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


def test_symbol_and_prototype():
    from uam_path_planning_amd import _lib, build

    build.build_library()
    lib = _lib.load()
    with open(os.path.join(ROOT, "include", "uampath.h")) as f:
        text = re.sub(r"/\*.*?\*/", " ", f.read(), flags=re.S)
    text = re.sub(r"\s+", " ", text)
    proto = ("int uam_eval_generated3d_profiles_h(uam_ctx* ctx, const uam_volume_desc* desc, "
             "const void* vol_dev, const void* packed_dev, const double* pairs6_dev, "
             "int64_t n_pairs, const double* utab_dev, int32_t D, const double* ztab_dev, "
             "int32_t A, const uam_path_outputs* out, uam_stream stream);")
    assert proto in text
    vp, i32, i64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64
    vd, po = ctypes.POINTER(_lib.VolumeDesc), ctypes.POINTER(_lib.PathOutputs)
    args = [vp, vd, vp, vp, vp, i64, vp, i32, vp, i32, po, vp]
    name = "uam_eval_generated3d_profiles_h"
    assert _lib.SIGNATURES[name] == (ctypes.c_int, args)
    fn = getattr(lib, name)
    assert fn.restype is ctypes.c_int and list(fn.argtypes) == args
    assert lib.uam_abi_version() == _lib.ABI_VERSION == 2     # no ABI bump, no new option
    assert max(_lib.OPTIONS.values()) == 24
    # no GPU is touched by a NULL context: the argument check answers
    assert fn(None, None, None, None, None, 0, None, 1, None, 1, None, None) == _lib.UAM_E_INVALID


def test_header_states_the_definition():
    with open(os.path.join(ROOT, "include", "uampath.h")) as f:
        text = re.sub(r"[\s*]+", " ", f.read())
    start = text.index("Altitude-profile candidates on the packed, sorted volume")
    sec = text[start:text.index("int uam_eval_generated3d_profiles_h(", start)]
    for clause in (
            "Every float64 operation is rounded, none is contracted",
            "group order: cost = ((N+1) L + P_0) + P_1 + ...",
            "[k G, min((k+1) G, W))",
            "(z0 ztab[a][j][0] + zf ztab[a][j][1]) + ztab[a][j][2]",
            "NULL-table rule: ztab_dev == NULL (A must be 1)",
            "min_clearance is +inf when no waypoint lies inside the volume",
            "uam_argmin's rule over the pair's D A candidates",
            "never falling back to K4p, K4 or K4w",
            "UAM_OPT_SORTED_MIN_PATHS and UAM_OPT_WAVE_MAX_PATHS do not apply",
            "\"K4hp+pack\"", "\"K4hpx+pack\"",
            "cost = (double)(N+1) L + fl(S_risk) / (double)N",
            "UAM_E_STATE when no volume sum scale is set",
            "before any launch or allocation",
            "there is no _v variant"):
        assert clause in sec, clause


@pytest.mark.parametrize("D", [1, 5])
@pytest.mark.parametrize("N", [1, 9, 40])
def test_restatement_equals_the_oracle_on_the_straight_climb(oracle_mod, N, D):
    """A = 1 with oracle.gen_paths3d's z: the restatement (voxel words at eval_paths3d's voxel
    indices, grouped in numpy) against orc_eval_generated_h(group=G), every output, bit for
    bit."""
    orc = _oracle(oracle_mod, N)
    vox, cols = R.hand_volume()
    pr, ut = R.pairs6(130), _utab(N, D)
    W = N + 2
    host = R.host_volume(vox, cols)
    for G in (1, 3, 21, W, W + 5):
        got = H.evaluate(oracle_mod, orc, vox, cols, pr, ut, None, G)
        want = orc.eval_generated_h(pr, ut, mode="volume", vdesc=R.volume_desc(oracle_mod),
                                    vol=host, group=G)
        for gk, ok in (("cost", "cost"), ("length_q", "lq"), ("length", "length"),
                       ("kin_sum", "kin"), ("nfz_sum", "nfz"), ("nfz_hits", "nfz_hits"),
                       ("offmap", "offmap"), ("min_clearance", "min_clearance"),
                       ("below_terrain", "below")):
            _same(got[gk], want[ok], f"N={N} D={D} G={G} {gk}")
        with np.errstate(invalid="ignore"):
            _same(got["best_fval_idx"], oracle_mod.argmin(want["cost"], D, True), "best_fval")
        _same(got["best_length_idx"], oracle_mod.argmin(want["length"], D, False), "best_length")
    assert (got["offmap"] > 0).any() and np.isposinf(got["min_clearance"]).any()


@pytest.mark.parametrize("G", [4, 21])
def test_grouped_costs_lie_within_rounding_of_the_sequential_ones(oracle_mod, G):
    """The 8-profile family, by the reference alone: the grouped cost differs from
    eval_paths3d's sequential one by the rounding of W additions of terms bounded by
    sum |risk_j| / N + (N+1) |L| -- at most 2 W 2^-53 times that -- and some pair's best
    candidate is not its lateral candidate's first profile."""
    from uam_path_planning_amd import profiles as P

    N, D = 40, 5
    W = N + 2
    orc = _oracle(oracle_mod, N)
    vox, cols = R.hand_volume()
    pr, ut, zt = R.pairs6(130), _utab(N, D), R.family(P, N)
    A = zt.shape[0]
    ref = H.evaluate(oracle_mod, orc, vox, cols, pr, ut, zt, G)
    cells = ref["cells"]
    risk = np.abs(vox.reshape(-1, 2)[:, 0].view(np.float32).astype(np.float64))
    mag = np.where(cells >= 0, risk[np.where(cells >= 0, cells, 0)], 0.0).sum(axis=1) / N
    ok = np.isfinite(ref["sequential_cost"]) & np.isfinite(ref["cost"])
    assert ok.sum() > 0.9 * ok.size
    bound = 2.0 * W * 2.0 ** -53 * (mag + (N + 1) * np.abs(ref["length_q"]))
    err = np.abs(ref["cost"] - ref["sequential_cost"])
    assert (err[ok] <= bound[ok]).all()
    assert (err[ok] > 0).any()          # the two orders do differ
    assert (ref["best_fval_idx"] % A != 0).any()
    assert ref["best_fval_idx"].shape == (130,) and ref["best_fval_idx"].max() < D * A
