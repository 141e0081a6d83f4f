"""Engine.eval_generated3d_profiles_hv: uam_eval_generated3d_profiles_hv ("K4hpv+pack"), the
altitude-profile candidates on the packed, sorted volume with the vertical terms, against the
numpy restatement of its definition (profiles_hv_ref.py: profiles_h_ref's sums, vertical_ref's
sequential geometry) and against the existing calls on the device.  Every comparison is bit
equality (uint64 views, NaN equals NaN).

Volume, pairs, arc and profile tables: test_gpu_profiles.py's (the hand volume of 100 x 76
columns x 7 layers; the first eight pairs are the special ones).  The sums' part of a reference
(test_gpu_profiles_h._ref) is computed once per (N, D, A, G) on the 130-pair batch, the geometry
once per (case, parameters, vertical) on top of it, and both are sliced for the smaller batches."""
import ctypes
import math

import numpy as np
import pytest

import profiles_h_ref as H
import profiles_hv_ref as HV
import profiles_ref as R
import vertical_ref as V
from test_gpu_profiles import DEFAULTS, Ctx, _same, _same_outputs, _table, _utab
from test_gpu_profiles_h import BASE, _planted
from test_gpu_profiles_h import _ref as _base

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

KEYS = HV.KEYS + HV.BEST
ANCHOR = (3.0, -2.0)
INF = math.inf
# z_scale x (sin_climb, sin_descent): every scale with no limit, and 0 and 0.1 in both roles
VERTS = [(zs, sc, sd) for zs in (0.0, 1e-3, 1e-2)
         for sc, sd in ((INF, INF), (0.0, 0.1), (0.1, 0.0))]
VERT = (1e-3, 0.1, 0.0)


@pytest.fixture(scope="module")
def cx(oracle_mod):
    from uam_path_planning_amd.engine import Vertical

    c = Ctx(oracle_mod)
    c.refs, c.hv = {}, {}
    c.Vertical = Vertical
    return c


def _use(cx, N, ls=None, ms=False, quirk=True, anchored=False, **opts):
    """Params and options of the next evaluations; returns the reference's Geo.  ls None: the
    canonical map's own length_smooth, and with quirk set and anchored unset the anchor is p_0:
    then the parameters are Ctx.use(N)'s, the ones the other calls' tests run under."""
    s = cx.spec
    o = dict(s["options"])
    ls = bool(o["length_smooth"]) if ls is None else bool(ls)
    o["length_smooth"], o["maxratio_smooth"] = ls, bool(ms)
    anchor = ANCHOR if quirk and anchored else None
    cx.e.set_params(cx.PathParams(N=N, **o, maxratio=s["maxratio"], maxalpha=s["maxalpha"],
                                  enlargement=s["enlargement"], weights=tuple(s["weights"]),
                                  altitude=320.0, quirk_length=bool(quirk), anchor=anchor))
    cx.state = None       # (Ctx.use sets its own parameters again)
    for k, v in {**DEFAULTS, **BASE, **opts}.items():
        cx.e.set_option(k, v)
    return V.Geo(length_smooth=ls, maxratio_smooth=bool(ms), quirk_length=bool(quirk),
                 anchor=anchor, maxratio=s["maxratio"], maxalpha=s["maxalpha"])


def _ref(cx, N, D, A, G, vert, geo_kw=(), exact=False, table=True, vox=None):
    """The definition's outputs for pairs6(130); the sums are cached per case and the whole per
    (case, parameters, vertical).  vox: another volume's voxels (not cached)."""
    key = (N, D, A, G, exact, table, tuple(sorted(dict(geo_kw).items())), vert)
    if vox is not None or key not in cx.hv:
        base = _base(cx, N, D, A, G, exact=exact, table=table, vox=vox)
        geo = _use(cx, N, **dict(geo_kw))
        zt = _table(N, A) if table else None
        r = HV.evaluate(cx.O, None, cx.vox if vox is None else vox, cx.cols, R.pairs6(130),
                        _utab(N, D), zt, G, geo, V.Vert(*vert), exact=exact, base=base)
        if vox is not None:
            return r
        cx.hv[key] = r
    return cx.hv[key]


def _run(cx, N, pr, D, A, vert, geo_kw=(), vol=None, table=True, **opts):
    _use(cx, N, **dict(geo_kw), **opts)
    zt = _table(N, A) if table else None
    out = cx.e.eval_generated3d_profiles_hv(pr, _utab(N, D), zt, vol or cx.vol,
                                            cx.Vertical(*vert))
    return {k: out[k].cpu().numpy() for k in KEYS}


def _rows(ref, Q, C, q0=0):
    """The reference's rows of pairs [q0, q0 + Q) with C candidates each."""
    out = {k: ref[k][q0 * C:(q0 + Q) * C] for k in HV.KEYS}
    out.update({k: ref[k][q0:q0 + Q] for k in HV.BEST})
    return out


# ---- 1. against the restatement ----------------------------------------------------------------
@pytest.mark.parametrize("A", [1, 3, 8])
@pytest.mark.parametrize("D", [1, 5, 16])
@pytest.mark.parametrize("N", [1, 9, 40])
def test_equals_the_restatement(cx, N, D, A):
    """W = 3, 11, 42 in groups of 21 (W < G, a ragged last group, W a multiple of G); every
    z_scale with no limit and with 0 and 0.1 in both roles; the family table's cruises above the
    top and below the floor (A = 3, 8); the special pairs."""
    pr = R.pairs6(130)
    for vert in VERTS:
        ref = _ref(cx, N, D, A, 21, vert)
        got = _run(cx, N, pr, D, A, vert, group=21)
        assert cx.e.last_kernel() == "K4hpv+pack" and cx.e.last_group() == 21
        _same_outputs(got, ref, KEYS, f"N={N} D={D} A={A} vert={vert}")
        if vert[0] == 0.0:
            assert not got["climb_sum"].any() and not np.signbit(got["climb_sum"]).any()
    if A == 8 and D > 1 and N >= 9:   # the batch holds what the comparison is meant to cover
        assert (ref["offmap"] > 0).any() and (ref["offmap"] == N + 2).any()
        assert (ref["below_terrain"] > 0).any() and (ref["nfz_hits"] > 0).any()
        assert np.isposinf(ref["min_clearance"]).any() and np.isnan(ref["cost"]).any()
        assert (ref["climb_sum"] > 0).any()


@pytest.mark.parametrize("N,G", [(40, 4), (9, 1), (40, 64)])
def test_group_lengths(cx, N, G):
    D, A = 5, 3
    pr = R.pairs6(130)
    for vert in (VERTS[0], VERTS[4], VERTS[8]):
        got = _run(cx, N, pr, D, A, vert, group=G)
        assert cx.e.last_kernel() == "K4hpv+pack" and cx.e.last_group() == G
        _same_outputs(got, _ref(cx, N, D, A, G, vert), KEYS, f"N={N} G={G} vert={vert}")


@pytest.mark.parametrize("quirk", [False, True])
@pytest.mark.parametrize("ms", [False, True])
@pytest.mark.parametrize("ls", [False, True])
def test_geometry_parameters(cx, ls, ms, quirk):
    """length_smooth, maxratio_smooth (accepted here, refused by K4hp) and the length quirk with
    an anchor of its own."""
    N, D, A = 9, 5, 3
    kw = (("ls", ls), ("ms", ms), ("quirk", quirk), ("anchored", quirk))
    pr = R.pairs6(130)
    for vert in (VERTS[3], VERTS[5], VERTS[7]):
        got = _run(cx, N, pr, D, A, vert, kw)
        assert cx.e.last_kernel() == "K4hpv+pack"
        _same_outputs(got, _ref(cx, N, D, A, 21, vert, kw), KEYS,
                      f"ls={ls} ms={ms} quirk={quirk} vert={vert}")


# ---- 2. against the existing calls on the device -------------------------------------------------
def test_against_k4pv_and_k4hp_which_stay_as_they_were(cx):
    N, D, A = 40, 5, 8
    pr, ut, zt = R.pairs6(130), _utab(N, D), _table(N, A)
    vert = cx.Vertical(*VERT)
    geo, sums = HV.GEO, HV.UNTOUCHED
    host = lambda o, keys: {k: o[k].cpu().numpy() for k in keys}

    def k4pv():
        _use(cx, N)
        o = cx.e.eval_generated3d_profiles(pr, ut, zt, cx.vol, vertical=vert)
        assert cx.e.last_kernel() == "K4p+v"
        return host(o, HV.KEYS + HV.BEST)

    def k4hp():
        _use(cx, N)
        o = cx.e.eval_generated3d_profiles(pr, ut, zt, cx.vol, packed=True)
        assert cx.e.last_kernel() == "K4hp+pack"
        return host(o, H.KEYS + H.BEST)

    pv, hp = k4pv(), k4hp()
    got = _run(cx, N, pr, D, A, VERT)
    assert cx.e.last_kernel() == "K4hpv+pack"
    _same_outputs(got, pv, geo, "geometry against K4p+v")
    _same_outputs(got, hp, sums, "sums against K4hp")
    _same(got["best_length_idx"], pv["best_length_idx"], "best_length_idx against K4p+v")
    assert (got["length"] != hp["length"]).any()
    _same_outputs(k4pv(), pv, HV.KEYS + HV.BEST, "K4p+v after the new call")
    _same_outputs(k4hp(), hp, H.KEYS + H.BEST, "K4hp after the new call")


# ---- 3. only work moves ------------------------------------------------------------------------
@pytest.mark.parametrize("terrain", [0, 1])
@pytest.mark.parametrize("chunk", [6, 7, 8, 11, 16])
def test_chunks_only_move_work(cx, chunk, terrain):
    N, D, A = 40, 5, 3
    ref = _ref(cx, N, D, A, 21, VERT)
    got = _run(cx, N, R.pairs6(130), D, A, VERT, k2g_chunk=chunk, k4h_terrain=terrain)
    _same_outputs(got, ref, KEYS, f"chunk={chunk} terrain={terrain}")


@pytest.mark.parametrize("tile_bits,band", [(5, 0), (6, 0), (4, 2), (3, 16), (3, 1)])
def test_tile_bits_and_bands_only_move_work(cx, tile_bits, band):
    N, D, A = 40, 5, 8
    ref = _ref(cx, N, D, A, 21, VERT)
    for curve in (1, 0):
        got = _run(cx, N, R.pairs6(130), D, A, VERT, k2g_tile_bits=tile_bits, k4h_band=band,
                   k2g_curve=curve)
        _same_outputs(got, ref, KEYS, f"tile_bits={tile_bits} band={band} curve={curve}")


def test_outputs_do_not_depend_on_the_batch_or_the_thresholds(cx):
    N, D, A = 40, 5, 8
    pr = R.pairs6(130)
    C = D * A
    ref = _ref(cx, N, D, A, 21, VERT)
    for Q in (1, 63, 65, 130):
        for opts in (dict(sorted_min_paths=0, wave_max_paths=0),
                     dict(sorted_min_paths=1 << 30, wave_max_paths=1 << 20)):
            got = _run(cx, N, pr[:Q], D, A, VERT, **opts)
            assert cx.e.last_kernel() == "K4hpv+pack"
            _same_outputs(got, _rows(ref, Q, C), KEYS, f"prefix Q={Q} {opts}")
    for q0, Q in ((64, 1), (5, 63), (129, 1)):
        got = _run(cx, N, pr[q0:q0 + Q], D, A, VERT)
        _same_outputs(got, _rows(ref, Q, C, q0), KEYS, f"slice {q0}+{Q}")


# ---- 4. the exact form -------------------------------------------------------------------------
def test_exact_form_has_one_bit_pattern(cx):
    from uam_path_planning_amd import _lib

    N, D, A = 40, 5, 3
    pr, ut, zt = R.pairs6(130), _utab(N, D), _table(N, A)
    C = D * A
    vox, vol = _planted(cx)
    ref = _ref(cx, N, D, A, 21, VERT, exact=True, vox=vox)
    assert np.isnan(ref["cost"]).any() and np.isinf(ref["cost"]).any()
    try:
        first = None
        for G in (1, 4, 21, 64):
            got = _run(cx, N, pr, D, A, VERT, vol=vol, exact_sum_volume=1, group=G)
            assert cx.e.last_kernel() == "K4hpxv+pack" and cx.e.last_group() == G
            _same_outputs(got, ref, KEYS, f"exact G={G}")
            first = first or got
            _same_outputs(got, first, KEYS, f"exact G={G} against the first run")
        a = _run(cx, N, pr[:65], D, A, VERT, vol=vol, exact_sum_volume=1, k2g_chunk=11)
        b = _run(cx, N, pr[65:], D, A, VERT, vol=vol, exact_sum_volume=1, k4h_terrain=1)
        for k in KEYS:
            _same(np.concatenate([a[k], b[k]]), first[k], f"shards {k}")
        # the ordered form on the same voxels is its own definition's
        plain = _run(cx, N, pr, D, A, VERT, vol=vol)
        assert cx.e.last_kernel() == "K4hpv+pack"
        _same_outputs(plain, _ref(cx, N, D, A, 21, VERT, vox=vox), KEYS, "ordered, planted volume")
        # no scale set: UAM_E_STATE through the raw ABI (the Python layer always sets one)
        e = cx.e
        _use(cx, N, exact_sum_volume=1)
        _lib.check(e.lib.uam_set_volume_sum_scale(e._ctx, None), "uam_set_volume_sum_scale")
        prd, utd = e.tensor(pr, torch.float64), e.tensor(ut, torch.float64)
        ztd = e.tensor(zt, torch.float64)
        o, s = e.outputs(130 * C, N + 2, n_pairs=130)
        vd, vs = vol.geo.as_struct(), cx.Vertical(*VERT).as_struct()
        p = lambda t: ctypes.c_void_p(t.data_ptr())
        st = e.lib.uam_eval_generated3d_profiles_hv(
            e._ctx, ctypes.byref(vd), p(vol.buf), p(vol.packed), p(prd), 130, p(utd), D, p(ztd),
            A, ctypes.byref(vs), ctypes.byref(s), None, e.stream)
        assert st == _lib.UAM_E_STATE
        got = _run(cx, N, pr, D, A, VERT, vol=vol, exact_sum_volume=1)   # usable, scale set again
        _same_outputs(got, first, KEYS, "after the refusal")
    finally:
        cx.e.set_option("exact_sum_volume", 0)


# ---- 5. the NULL table -------------------------------------------------------------------------
@pytest.mark.parametrize("N,D,G", [(1, 5, 21), (9, 16, 4), (40, 5, 21), (40, 1, 64)])
def test_no_table_is_the_straight_climb(cx, N, D, G):
    pr = R.pairs6(130)
    for vert in (VERTS[3], VERTS[7]):
        ref = _ref(cx, N, D, 1, G, vert, table=False)
        got = _run(cx, N, pr, D, 1, vert, table=False, group=G)
        assert cx.e.last_kernel() == "K4hpv+pack" and cx.e.last_group() == G
        _same_outputs(got, ref, KEYS, f"ztab=None N={N} D={D} G={G} vert={vert}")
    got = _run(cx, N, pr[:1], D, 1, vert, table=False, group=G)   # sorted at every size
    _same_outputs(got, _rows(ref, 1, D), KEYS, "one pair")
    # the straight climb with the vertical terms is K4p+v's too, in its geometry
    _use(cx, N)
    pv = cx.e.eval_generated3d_profiles(pr, _utab(N, D), None, cx.vol,
                                        vertical=cx.Vertical(*vert))
    _same_outputs(_rows(ref, 130, D), {k: pv[k].cpu().numpy() for k in HV.GEO}, HV.GEO,
                  "against K4p+v")
    if N == 40 and D == 5:
        try:
            ref = _ref(cx, N, D, 1, G, vert, exact=True, table=False)
            got = _run(cx, N, pr, D, 1, vert, table=False, group=4, exact_sum_volume=1)
            assert cx.e.last_kernel() == "K4hpxv+pack" and cx.e.last_group() == 4
            _same_outputs(got, ref, KEYS, "ztab=None, exact")
        finally:
            cx.e.set_option("exact_sum_volume", 0)


# ---- 6. refusals ---------------------------------------------------------------------------------
def test_refusals_name_their_reason_and_leave_the_engine_usable(cx):
    from uam_path_planning_amd import _lib
    from uam_path_planning_amd.engine import VolumeGeo

    N, D, A = 9, 5, 3
    e, vol = cx.e, cx.vol
    pr, ut, zt = R.pairs6(130)[:16], _utab(N, D), _table(N, A)
    W = N + 2
    good = cx.Vertical(*VERT)
    needs = "uam_eval_generated3d_profiles_hv needs K4hpv: "
    want = _rows(_ref(cx, N, D, A, 21, VERT), 16, D * A)
    _run(cx, N, pr, D, A, VERT)   # (packs the volume if no test before did)

    def call(match, pr=pr, ut=ut, zt=zt, vertical=good, **kw):
        with pytest.raises(ValueError, match=match):
            e.eval_generated3d_profiles_hv(pr, ut, zt, vol, vertical, **kw)

    _use(cx, N, group=0)
    call(needs + "UAM_OPT_GROUP is 0")
    call(needs + "UAM_OPT_GROUP is 0", zt=None)      # the NULL table names the same call
    # what K4hp refuses and this call takes: a correct result under each
    got = _run(cx, N, pr, D, A, VERT, k2g_sim=0)
    _same_outputs(got, want, KEYS, "k2g_sim = 0")
    kw = (("ms", True),)
    got = _run(cx, N, pr, D, A, VERT, kw)
    _same_outputs(got, _rows(_ref(cx, N, D, A, 21, VERT, kw), 16, D * A), KEYS, "maxratio_smooth")
    got = _run(cx, N, pr, D, 1, VERT, kw, table=False, k2g_sim=0)
    _same_outputs(got, _rows(_ref(cx, N, D, 1, 21, VERT, kw, table=False), 16, D), KEYS,
                  "maxratio_smooth and k2g_sim = 0, no table")
    _use(cx, N)
    call(r"D outside \[1, 16\]", ut=_utab(N, 17))
    call(r"A = 9 outside \[1, 8\]", zt=np.zeros((9, W, 3)))
    call(r"A = 0 outside \[1, 8\]", zt=np.zeros((0, W, 3)))
    call(needs + "cells or g_rows requested",
         outputs=e.outputs(16 * D * A, W, n_pairs=16, want_cells=True))
    with pytest.raises(ValueError, match="needs a Vertical"):
        e.eval_generated3d_profiles_hv(pr, ut, zt, vol, None)
    with pytest.raises(ValueError, match="packed=True has no vertical form.*"
                                         "eval_generated3d_profiles_hv"):
        e.eval_generated3d_profiles(pr, ut, zt, vol, packed=True, vertical=good)
    with pytest.raises(ValueError, match="outputs\\['climb_sum'\\] holds 3 entries"):
        outs = e.outputs(16 * D * A, W, n_pairs=16)
        outs[0]["climb_sum"] = e.empty((3,), torch.float64)
        e.eval_generated3d_profiles_hv(pr, ut, zt, vol, good, outputs=outs)
    # the checks of vert, through the Python layer and the raw ABI
    for bad in (math.nan, -1e-3, INF):
        call("z_scale must be finite and >= 0", vertical=cx.Vertical(bad))
    for sc, sd in ((math.nan, 0.1), (0.1, math.nan), (-0.1, 0.1), (0.1, -0.1)):
        call("sin_climb and sin_descent must be >= 0", vertical=cx.Vertical(1e-3, sc, sd))
    prd, utd = e.tensor(pr, torch.float64), e.tensor(ut, torch.float64)
    ztd = e.tensor(zt, torch.float64)
    o, s = e.outputs(16 * D * A, W, n_pairs=16)
    vd, gv = vol.geo.as_struct(), good.as_struct()
    p = lambda t: ctypes.c_void_p(t) if isinstance(t, int) else ctypes.c_void_p(t.data_ptr())

    def status(vert, packed=vol.packed, prs=prd, zts=ztd, a=A, d=D, outs=s, n=16, desc=vd):
        return e.lib.uam_eval_generated3d_profiles_hv(
            e._ctx, ctypes.byref(desc), p(vol.buf), None if packed is None else p(packed),
            p(prs), n, p(utd), d, None if zts is None else p(zts), a,
            None if vert is None else ctypes.byref(vert), ctypes.byref(outs), None, e.stream)

    def raw(match, **kw):
        with pytest.raises(ValueError, match=match):
            _lib.check(status(gv, **kw))

    # vert comes before the dimensions (D = 17 here), as in uam_eval_generated3d_profiles_v
    assert status(None, d=17) == _lib.UAM_E_INVALID and "vert is NULL" in _lib.last_error()
    assert status(_lib.Vertical(3, 1e-3, 0.1, 0.1), d=17) == _lib.UAM_E_VERSION
    assert "uam_vertical.abi_version 3 != 2" in _lib.last_error()
    assert status(_lib.Vertical(2, math.nan, 0.1, 0.1), d=17) == _lib.UAM_E_INVALID
    assert "z_scale must be finite" in _lib.last_error()
    raw(r"D outside \[1, 16\]", d=17)
    raw("needs K4hpv: no packed_dev", packed=None)
    raw("ztab is NULL .* A = 2: A must be 1", zts=None, a=2)
    raw("packed volume not 256-B aligned", packed=vol.packed.data_ptr() + 8)
    raw("not 16-B or ztab_dev not 8-B aligned", prs=prd.data_ptr() + 8)
    raw("2\\^31 or more paths", n=(1 << 31) // (D * A) + 1)
    nocost = _lib.PathOutputs.from_buffer_copy(s)
    nocost.cost = None
    raw("best_fval_idx needs the cost output", outs=nocost)
    rows = _lib.PathOutputs.from_buffer_copy(s)
    rows.g_rows = o["cost"].data_ptr()     # (any non-NULL pointer: refused before a launch)
    raw("needs K4hpv: cells or g_rows requested", outs=rows)
    # 2^31 (path, group) items with fewer than 2^31 paths (groups of 1); refused on the host, so
    # the buffers' sizes never matter
    _use(cx, N, group=1)
    n_items = (1 << 31) // (D * A * W) + 1
    assert n_items * D * A < (1 << 31) - 1 <= n_items * D * A * W
    raw(r"needs K4hpv: more than 2\^31 \(path, group\) items", n=n_items)
    raw(r"needs K4hpv: more than 2\^31 \(path, group\) items", n=(1 << 31) // (D * W) + 1,
        zts=None, a=1)
    _use(cx, N)
    # made-up descriptors with the real pointers (nothing is read before the refusal)
    geo = lambda nx, ny, nz: VolumeGeo(nx, ny, nz, R.X0, R.Y_TOP, R.DX, R.DY, R.Z0,
                                       R.DZ).as_struct()
    raw("needs K4hpv: the packed header exceeds its LDS share", desc=geo(4000, 4000, 1))
    raw("needs K4hpv: the packed copy is 4 GiB or larger", desc=geo(1024, 1024, 128))
    raw(r"needs K4hpv: the packed copy is 4 GiB or larger, or a layer or side holds 2\^24",
        desc=geo(8192, 8192, 1))
    for n_big, a_big, match in ((4097, 1, "N > 4096"), (1000, 2, "profile table exceeds its LDS")):
        _use(cx, n_big)
        with pytest.raises(ValueError, match="needs K4hpv: .*" + match):
            e.eval_generated3d_profiles_hv(pr, np.zeros((2, n_big, 2)),
                                           np.zeros((a_big, n_big + 2, 3)), vol, good)
    _use(cx, 1600)
    with pytest.raises(ValueError, match="needs K4hpv: the unit-arc table exceeds its LDS share"):
        e.eval_generated3d_profiles_hv(pr, np.zeros((2, 1600, 2)), np.zeros((1, 1602, 3)), vol,
                                       good)
    # the context is still usable and right, and a caller's own climb_sum buffer is the one written
    got = _run(cx, N, pr, D, A, VERT)
    _same_outputs(got, want, KEYS, "after the refusals")
    outs = e.outputs(16 * D * A, W, n_pairs=16)
    outs[0]["climb_sum"] = e.empty((16 * D * A,), torch.float64)
    out = e.eval_generated3d_profiles_hv(pr, ut, zt, vol, good, outputs=outs)
    assert out["climb_sum"] is outs[0]["climb_sum"]
    _same_outputs(out, want, KEYS, "caller's outputs")
