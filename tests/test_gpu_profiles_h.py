"""Engine.eval_generated3d_profiles(..., packed=True): uam_eval_generated3d_profiles_h ("K4hp"),
the altitude-profile candidates on the packed, sorted volume, against the numpy restatement of
its definition (profiles_h_ref.py, built from oracle outputs only).  Every comparison is bit
equality (uint64 views, NaN equals NaN).

Volume, pairs, arc and profile tables: test_gpu_profiles.py's (the hand volume of 100 x 76
columns x 7 layers; the first eight pairs are the special ones: below / above / east of the
volume, start == goal, a NaN coordinate, top to bottom, wholly outside).  A reference is computed
once per (N, D, A, G) on the 130-pair batch and sliced for the smaller ones."""
import ctypes

import numpy as np
import pytest

import profiles_h_ref as H
import profiles_ref as R
from test_gpu_profiles import Ctx, _same, _same_outputs, _table, _utab

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

KEYS = H.KEYS + H.BEST
# every option a run of this file depends on beyond Ctx.use's defaults
BASE = dict(k2g_chunk=0, k4h_terrain=0, k2g_tile_bits=0, k2g_curve=1, k4h_band=0,
            k2g_lds_floor=0, k2g_sim=1, test_sort_fault=0)


@pytest.fixture(scope="module")
def cx(oracle_mod):
    c = Ctx(oracle_mod)
    c.refs = {}
    return c


def _ref(cx, N, D, A, G, exact=False, table=True, vox=None):
    """The definition's outputs for pairs6(130); cached per case on the hand volume."""
    key = (N, D, A, G, exact, table)
    if vox is not None or key not in cx.refs:
        orc = cx.use(N)
        zt = _table(N, A) if table else None
        r = H.evaluate(cx.O, orc, cx.vox if vox is None else vox, cx.cols, R.pairs6(130),
                       _utab(N, D), zt, G, exact=exact)
        if vox is not None:
            return r
        cx.refs[key] = r
    return cx.refs[key]


def _run(cx, N, pr, D, A, vol=None, table=True, **opts):
    cx.use(N, **{**BASE, **opts})
    zt = _table(N, A) if table else None
    out = cx.e.eval_generated3d_profiles(pr, _utab(N, D), zt, vol or cx.vol, packed=True)
    return {k: out[k].cpu().numpy() for k in KEYS}


def _rows(ref, Q, C, q0=0):
    """The reference's rows of pairs [q0, q0 + Q) with C candidates each."""
    out = {k: ref[k][q0 * C:(q0 + Q) * C] for k in H.KEYS}
    out.update({k: ref[k][q0:q0 + Q] for k in H.BEST})
    return out


# ---- 1. against the restatement ----------------------------------------------------------------
@pytest.mark.parametrize("A", [1, 3, 8])
@pytest.mark.parametrize("D", [1, 5, 16])
@pytest.mark.parametrize("N", [1, 9, 40])
def test_equals_the_restatement(cx, N, D, A):
    """Groups of 1, 4, 21 and 64 (W = 3, 11, 42: W < G, W a multiple of G -- 42 = 2 x 21 --
    and a ragged last group), both terrain forms, batches of 1 / 63 / 65 / 130 pairs; the family
    table's cruises above the top and below the floor (A = 3, 8); the special pairs."""
    pr = R.pairs6(130)
    C = D * A
    for G in (1, 4, 21, 64):
        ref = _ref(cx, N, D, A, G)
        for terrain in (0, 1):
            got = _run(cx, N, pr, D, A, group=G, k4h_terrain=terrain)
            assert cx.e.last_kernel() == "K4hp+pack" and cx.e.last_group() == G
            _same_outputs(got, ref, KEYS, f"N={N} D={D} A={A} G={G} terrain={terrain}")
    ref = _ref(cx, N, D, A, 21)
    for Q in (1, 63, 65):
        got = _run(cx, N, pr[:Q], D, A, group=21, k4h_terrain=Q & 1)
        _same_outputs(got, _rows(ref, Q, C), KEYS, f"N={N} D={D} A={A} Q={Q}")
    if A == 8 and D > 1 and N >= 9:   # the batch holds what the comparison is meant to cover
        assert (ref["offmap"] > 0).any() and (ref["offmap"] == N + 2).any()
        assert (ref["below_terrain"] > 0).any() and (ref["nfz_hits"] > 0).any()
        assert np.isposinf(ref["min_clearance"]).any() and np.isnan(ref["cost"]).any()
        assert (ref["best_fval_idx"] % A != 0).any(), "the first profile won every pair"


@pytest.mark.parametrize("terrain", [0, 1])
@pytest.mark.parametrize("chunk", [6, 7, 8, 11, 16])
def test_chunks_only_move_work(cx, chunk, terrain):
    N, D, A = 40, 5, 3
    ref = _ref(cx, N, D, A, 21)
    got = _run(cx, N, R.pairs6(130), D, A, k2g_chunk=chunk, k4h_terrain=terrain)
    _same_outputs(got, ref, KEYS, f"chunk={chunk} terrain={terrain}")
    got = _run(cx, N, R.pairs6(130), D, A, k2g_chunk=chunk, k4h_terrain=terrain,
               k2g_lds_floor=90000)   # the raised dynamic-LDS attribute
    _same_outputs(got, ref, KEYS, f"chunk={chunk} terrain={terrain} floor=90000")


@pytest.mark.parametrize("tile_bits,band", [(5, 0), (6, 0), (4, 2), (3, 16), (3, 1)])
def test_tile_bits_and_bands_only_move_work(cx, tile_bits, band):
    N, D, A = 40, 5, 8
    ref = _ref(cx, N, D, A, 21)
    for curve in (1, 0):
        got = _run(cx, N, R.pairs6(130), D, A, k2g_tile_bits=tile_bits, k4h_band=band,
                   k2g_curve=curve)
        _same_outputs(got, ref, KEYS, f"tile_bits={tile_bits} band={band} curve={curve}")


# ---- 2. the NULL table ------------------------------------------------------------------------
@pytest.mark.parametrize("N,D,G", [(1, 5, 21), (9, 16, 4), (40, 5, 21), (40, 1, 64)])
def test_no_table_is_k4h_itself(cx, N, D, G):
    pr, ut = R.pairs6(130), _utab(N, D)
    got = _run(cx, N, pr, D, 1, table=False, group=G)
    assert cx.e.last_kernel() == "K4h+pack" and cx.e.last_group() == G
    cx.use(N, **{**BASE, "group": G, "sorted_min_paths": 0})
    k4h = cx.e.eval_generated3d(pr, ut, cx.vol)
    assert cx.e.last_kernel() == "K4h+pack"
    _same_outputs(got, {k: k4h[k].cpu().numpy() for k in KEYS}, KEYS, "against K4h")
    orc = cx.use(N)
    o = orc.eval_generated_h(pr, ut, mode="volume", vdesc=R.volume_desc(cx.O),
                             vol=R.host_volume(cx.vox, cx.cols), group=G)
    want = {"cost": o["cost"], "length_q": o["lq"], "length": o["length"], "kin_sum": o["kin"],
            "nfz_sum": o["nfz"], "min_clearance": o["min_clearance"], "nfz_hits": o["nfz_hits"],
            "offmap": o["offmap"], "below_terrain": o["below"]}
    with np.errstate(invalid="ignore"):
        want["best_fval_idx"] = cx.O.argmin(o["cost"], D, True)
    want["best_length_idx"] = cx.O.argmin(o["length"], D, False)
    _same_outputs(got, want, KEYS, "against eval_generated_h")
    _same_outputs(got, _ref(cx, N, D, 1, G, table=False), KEYS, "against the restatement")
    # a small batch too: sorted at every size
    got = _run(cx, N, pr[:1], D, 1, table=False, group=G)
    assert cx.e.last_kernel() == "K4h+pack"
    _same_outputs(got, _rows(want, 1, D), KEYS, "one pair")


# ---- 3. a path's bits do not depend on its batch -----------------------------------------------
def test_outputs_do_not_depend_on_the_batch_or_the_thresholds(cx):
    N, D, A = 40, 5, 8
    pr = R.pairs6(130)
    C = D * A
    full = _run(cx, N, pr, D, A)
    _same_outputs(full, _ref(cx, N, D, A, 21), KEYS, "the full batch")
    for Q in (1, 63, 130):
        for opts in (dict(sorted_min_paths=0, wave_max_paths=0),
                     dict(sorted_min_paths=1 << 30, wave_max_paths=1 << 20)):
            got = _run(cx, N, pr[:Q], D, A, **opts)
            assert cx.e.last_kernel() == "K4hp+pack"
            _same_outputs(got, _rows(full, Q, C), KEYS, f"prefix Q={Q} {opts}")
    for q0, Q in ((64, 1), (5, 63), (129, 1)):
        got = _run(cx, N, pr[q0:q0 + Q], D, A)
        _same_outputs(got, _rows(full, Q, C, q0), KEYS, f"slice {q0}+{Q}")


# ---- 4. the exact form -------------------------------------------------------------------------
def _planted(cx):
    """The hand volume with non-finite and far-apart words planted under waypoints of the batch
    (voxels the N = 40, D = 5, A = 3 reference visits), as a fresh packed volume."""
    from uam_path_planning_amd.engine import VolumeGeo

    ref = _ref(cx, 40, 5, 3, 21)
    seen = np.unique(ref["cells"][ref["cells"] >= 0])
    vox = cx.vox.copy()
    w = vox.reshape(-1, 2)
    f = lambda x: int(np.float32(x).view(np.uint32))
    pick = seen[:: max(1, len(seen) // 40)]
    w[pick[0], 0] = f(np.inf)
    w[pick[1], 0] = f(-np.inf)
    w[pick[2], 1] = f(np.nan)
    w[pick[3], 1] = f(np.inf)
    w[pick[4:20:2], 0] = f(2.0 ** 40)
    w[pick[5:20:2], 0] = f(-(2.0 ** -60))
    w[pick[20:30], 1] = f(2.0 ** 40)
    w[pick[30:40], 1] = f(2.0 ** -60)
    vol = cx.e.volume_alloc(VolumeGeo(R.NX, R.NY, R.NZ, R.X0, R.Y_TOP, R.DX, R.DY, R.Z0, R.DZ))
    vol.buf.zero_()
    vol.vox.copy_(cx.e.tensor(vox.view(np.int32), torch.int32))
    vol.cols.copy_(cx.e.tensor(cx.cols.view(np.int32), torch.int32))
    vol.cbits.fill_(-1)
    return vox, vol


def test_exact_form_has_one_bit_pattern(cx):
    N, D, A = 40, 5, 3
    pr, ut, zt = R.pairs6(130), _utab(N, D), _table(N, A)
    C = D * A
    vox, vol = _planted(cx)
    ref = _ref(cx, N, D, A, 21, exact=True, vox=vox)
    assert np.isnan(ref["cost"]).any() and np.isinf(ref["cost"]).any()
    assert np.isinf(ref["nfz_sum"]).any() and (np.abs(ref["cost"]) > 2.0 ** 30).any()
    try:
        first = None
        for G, chunk, terrain, tb in ((21, 0, 0, 0), (1, 6, 1, 5), (4, 8, 0, 3), (64, 16, 1, 4),
                                      (11, 11, 0, 6), (42, 7, 1, 0)):
            got = _run(cx, N, pr, D, A, vol=vol, exact_sum_volume=1, group=G, k2g_chunk=chunk,
                       k4h_terrain=terrain, k2g_tile_bits=tb)
            assert cx.e.last_kernel() == "K4hpx+pack" and cx.e.last_group() == G
            what = f"exact G={G} chunk={chunk} terrain={terrain} tile_bits={tb}"
            # (length_q / length / kin_sum do not depend on G: the reference's are G = 21's)
            _same_outputs(got, ref, KEYS, what)
            first = first or got
            _same_outputs(got, first, KEYS, what + " against the first run")
        # shards: 1 + 129 and 65 + 65
        for cut in (1, 65):
            a = _run(cx, N, pr[:cut], D, A, vol=vol, exact_sum_volume=1)
            b = _run(cx, N, pr[cut:], D, A, vol=vol, exact_sum_volume=1)
            for k in KEYS:
                _same(np.concatenate([a[k], b[k]]), first[k], f"shards {cut} {k}")
        # the ordered form on the same voxels differs from the exact one by rounding only, and
        # is its own definition's
        plain = _run(cx, N, pr, D, A, vol=vol, exact_sum_volume=0)
        _same_outputs(plain, _ref(cx, N, D, A, 21, vox=vox), KEYS, "ordered, planted volume")
        # no scale set: UAM_E_STATE through the raw ABI (the Python layer always sets one)
        from uam_path_planning_amd import _lib

        e = cx.e
        cx.use(N, **{**BASE, "exact_sum_volume": 1})
        _lib.check(e.lib.uam_set_volume_sum_scale(e._ctx, None), "uam_set_volume_sum_scale")
        prd, utd = e.tensor(pr, torch.float64), e.tensor(ut, torch.float64)
        ztd = e.tensor(zt, torch.float64)
        o, s = e.outputs(130 * C, N + 2, n_pairs=130)
        vd = vol.geo.as_struct()
        st = e.lib.uam_eval_generated3d_profiles_h(
            e._ctx, ctypes.byref(vd), ctypes.c_void_p(vol.buf.data_ptr()),
            ctypes.c_void_p(vol.packed.data_ptr()), ctypes.c_void_p(prd.data_ptr()), 130,
            ctypes.c_void_p(utd.data_ptr()), D, ctypes.c_void_p(ztd.data_ptr()), A,
            ctypes.byref(s), e.stream)
        assert st == _lib.UAM_E_STATE
        # the old calls still refuse under the option
        with pytest.raises(ValueError, match="UAM_OPT_EXACT_SUM_VOLUME"):
            e.eval_generated3d_profiles(pr, ut, zt, vol)
        with pytest.raises(ValueError, match="UAM_OPT_EXACT_SUM_VOLUME"):
            e.eval_waypoints3d(np.zeros((4, N + 2, 3)), vol)
        got = _run(cx, N, pr, D, A, vol=vol, exact_sum_volume=1)   # usable, scale set again
        _same_outputs(got, first, KEYS, "after the refusals")
    finally:
        cx.e.set_option("exact_sum_volume", 0)


# ---- 5. refusals, repacking, names --------------------------------------------------------------
def test_refusals_name_their_reason_and_leave_the_engine_usable(cx):
    from uam_path_planning_amd import _lib

    N, D, A = 9, 5, 3
    e, vol = cx.e, cx.vol
    pr, ut, zt = R.pairs6(130)[:16], _utab(N, D), _table(N, A)   # (the reference's pairs)
    W = N + 2
    _run(cx, N, pr, D, A)   # (packs the volume if no test before did)

    def call(match, pr=pr, ut=ut, zt=zt, **kw):
        with pytest.raises(ValueError, match=match):
            e.eval_generated3d_profiles(pr, ut, zt, vol, packed=True, **kw)

    for opt, bad, match in (("group", 0, "UAM_OPT_GROUP is 0"), ("k2g_sim", 0, "UAM_OPT_K2G_SIM is 0")):
        cx.use(N, **{**BASE, opt: bad})
        call("uam_eval_generated3d_profiles_h needs K4hp: " + match)
        cx.use(N, **{**BASE, opt: bad})
        with pytest.raises(ValueError, match="uam_eval_generated3d_profiles_h needs K4h: " + match):
            e.eval_generated3d_profiles(pr, ut, None, vol, packed=True)   # the NULL table too
    cx.use(N, **BASE)
    call(r"D outside \[1, 16\]", ut=_utab(N, 17))
    call(r"A = 9 outside \[1, 8\]", zt=np.zeros((9, W, 3)))
    call(r"A = 0 outside \[1, 8\]", zt=np.zeros((0, W, 3)))
    call("cells or g_rows requested", want_cells=True)
    with pytest.raises(ValueError, match="packed=True has no vertical form"):
        from uam_path_planning_amd.engine import Vertical

        e.eval_generated3d_profiles(pr, ut, zt, vol, packed=True, vertical=Vertical(1e-3))
    cx.use(N, ms=True, **BASE)
    call("maxratio_smooth is set")
    cx.use(N, **BASE)
    # straight to the C ABI: what the Python layer cannot express
    prd, utd = e.tensor(pr, torch.float64), e.tensor(ut, torch.float64)
    ztd = e.tensor(zt, torch.float64)
    o, s = e.outputs(16 * D * A, W, n_pairs=16)
    vd = vol.geo.as_struct()
    p = lambda t: ctypes.c_void_p(t) if isinstance(t, int) else ctypes.c_void_p(t.data_ptr())

    def raw(match, packed=vol.packed, prs=prd, zts=ztd, a=A, outs=s, n=16, desc=vd):
        with pytest.raises(ValueError, match=match):
            _lib.check(e.lib.uam_eval_generated3d_profiles_h(
                e._ctx, ctypes.byref(desc), p(vol.buf), None if packed is None else p(packed),
                p(prs), n, p(utd), D, None if zts is None else p(zts), a, ctypes.byref(outs),
                e.stream))

    raw("needs K4hp: no packed_dev", packed=None)
    raw("ztab is NULL .* A = 2: A must be 1", zts=None, a=2)
    raw("packed volume not 256-B aligned", packed=vol.packed.data_ptr() + 8)
    raw("not 16-B or ztab_dev not 8-B aligned", prs=prd.data_ptr() + 8)
    raw("2\\^31 or more paths", n=(1 << 31) // (D * A) + 1)
    nocost = _lib.PathOutputs.from_buffer_copy(s)
    nocost.cost = None
    raw("best_fval_idx needs the cost output", outs=nocost)
    rows = _lib.PathOutputs.from_buffer_copy(s)
    rows.g_rows = o["cost"].data_ptr()     # (any non-NULL pointer: refused before a launch)
    raw("needs K4hp: cells or g_rows requested", outs=rows)
    # 2^31 (path, group) items with fewer than 2^31 paths: the one refusal the A factor enters
    # (groups of 1: W = 11 items a path).  Refused on the host, so the buffers' sizes never matter
    from uam_path_planning_amd.engine import VolumeGeo

    cx.use(N, **{**BASE, "group": 1})
    n_items = (1 << 31) // (D * A * W) + 1
    assert n_items * D * A < (1 << 31) - 1 <= n_items * D * A * W
    raw(r"needs K4hp: more than 2\^31 \(path, group\) items", n=n_items)
    with pytest.raises(ValueError, match=r"needs K4h: more than 2\^31 \(path, group\) items"):
        _lib.check(e.lib.uam_eval_generated3d_profiles_h(     # the NULL table, A = 1
            e._ctx, ctypes.byref(vd), p(vol.buf), p(vol.packed), p(prd),
            (1 << 31) // (D * W) + 1, p(utd), D, None, 1, ctypes.byref(s), e.stream))
    cx.use(N, **BASE)
    # made-up descriptors with the real pointers (nothing is read before the refusal): a packed
    # header over its 64 KiB of LDS (4000 x 4000 columns: 61 KiB of codes + 39 KiB of bounds, the
    # layer still under 2^24 entries), and a copy K4h stands aside for (1024^2 x 128: 4.5 GiB)
    geo = lambda nx, ny, nz: VolumeGeo(nx, ny, nz, R.X0, R.Y_TOP, R.DX, R.DY, R.Z0,
                                       R.DZ).as_struct()
    raw("needs K4hp: the packed header exceeds its LDS share", desc=geo(4000, 4000, 1))
    raw("needs K4hp: the packed copy is 4 GiB or larger", desc=geo(1024, 1024, 128))
    raw(r"needs K4hp: the packed copy is 4 GiB or larger, or a layer or side holds 2\^24",
        desc=geo(8192, 8192, 1))
    # (the list's "too many bins" and "scan blocks" cannot occur for a volume: the key lowers
    # its tile bits until (tile, band) bins fit the sort, there are at most 16 bands, and the
    # counts of that many bins stay under 4096 scan blocks; K2h's tests reach them on rasters)
    # N > 4096, and a profile table over its LDS share (24 A W bytes > 40 KiB)
    for n_big, a_big, match in ((4097, 1, "N > 4096"), (1000, 2, "profile table exceeds its LDS")):
        cx.use(n_big, **BASE)
        with pytest.raises(ValueError, match=match):
            e.eval_generated3d_profiles(pr, np.zeros((2, n_big, 2)),
                                        np.zeros((a_big, n_big + 2, 3)), vol, packed=True)
    cx.use(1600, **BASE)
    with pytest.raises(ValueError, match="unit-arc table exceeds its LDS share"):
        e.eval_generated3d_profiles(pr, np.zeros((2, 1600, 2)), np.zeros((1, 1602, 3)), vol,
                                    packed=True)
    # the context is still usable and right
    got = _run(cx, N, pr, D, A)
    _same_outputs(got, _rows(_ref(cx, N, D, A, 21), 16, D * A), KEYS, "after the refusals")


def test_packs_first_and_repacks_after_a_voxel_write(cx):
    from uam_path_planning_amd.engine import VolumeGeo

    N, D, A = 9, 5, 3
    pr = R.pairs6(130)
    e = cx.e
    vol = e.volume_alloc(VolumeGeo(R.NX, R.NY, R.NZ, R.X0, R.Y_TOP, R.DX, R.DY, R.Z0, R.DZ))
    vol.buf.zero_()
    vol.vox.copy_(e.tensor(cx.vox.view(np.int32), torch.int32))
    vol.cols.copy_(e.tensor(cx.cols.view(np.int32), torch.int32))
    assert vol.packed is None
    got = _run(cx, N, pr, D, A, vol=vol)
    assert vol.packed is not None and cx.e.last_kernel() == "K4hp+pack"
    _same_outputs(got, _ref(cx, N, D, A, 21), KEYS, "packed on first use")
    old = vol.packed
    vol.vox[::3, 1::2, :, 0] = int(np.float32(2.5).view(np.int32))
    vol.vox[::5, 2::7, 3, 1] = int(np.float32(-0.25).view(np.int32))
    torch.cuda.synchronize()
    vox = vol.vox.cpu().numpy().view(np.uint32)
    got = _run(cx, N, pr, D, A, vol=vol)
    assert vol.packed is not old
    _same_outputs(got, _ref(cx, N, D, A, 21, vox=np.ascontiguousarray(vox)), KEYS,
                  "after a voxel write")
    # the default packed=False is the old call
    cx.use(N)
    e.eval_generated3d_profiles(pr, _utab(N, D), _table(N, A), vol)
    assert (e.last_kernel(), e.last_group()) == ("K4p", 0)


# ---- 6. the sort's device check -----------------------------------------------------------------
def test_device_check_surfaces(cx):
    from uam_path_planning_amd import _lib

    N, D, A = 40, 5, 3
    pr = R.pairs6(130)
    try:
        cx.use(N, **{**BASE, "test_sort_fault": 1})
        bad = cx.e.eval_generated3d_profiles(pr, _utab(N, D), _table(N, A), cx.vol, packed=True)
        assert cx.e.last_kernel() == "K4hp+pack"
        with pytest.raises(_lib.DeviceCheckError):
            cx.e.synchronize()
    finally:
        cx.e.set_option("test_sort_fault", 0)
    for k in ("cost", "length_q", "length", "kin_sum", "nfz_sum", "min_clearance"):
        assert np.isnan(bad[k].cpu().numpy()).all(), k
    for k in ("nfz_hits", "offmap", "below_terrain", "best_fval_idx", "best_length_idx"):
        assert (bad[k].cpu().numpy() == -1).all(), k
    got = _run(cx, N, pr, D, A)
    cx.e.synchronize()
    _same_outputs(got, _ref(cx, N, D, A, 21), KEYS, "after the device check")
