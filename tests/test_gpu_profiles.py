"""The volume over explicit 3-D waypoints and altitude-profile candidates: Engine.gen_paths3d,
Engine.eval_waypoints3d ("K4e" lane per path, "K4ew" wave per path) and
Engine.eval_generated3d_profiles ("K4p") against the oracle's eval_paths3d, bit for bit (uint64
views, NaN equals NaN) on every output.

Volume: hand-written, 100 x 76 columns x 7 layers, dz = 640 / 7 (profiles_ref.hand_volume),
written through vol.vox / vol.cols; canonical map with 16 polygons, maxratio_smooth both ways.
Reference: orc.eval_paths3d on waypoints whose x/y are oracle.gen_paths3d's and whose z is the
numpy restatement of the table rule (profiles_ref.table_z); selections by oracle.argmin.  A
reference is computed once for the largest batch of a case and sliced for the smaller ones (the
oracle evaluates path by path)."""
import ctypes
import dataclasses

import numpy as np
import pytest

import profiles_ref as R

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

PATH_KEYS = ("cost", "length_q", "length", "kin_sum", "nfz_sum", "min_clearance", "nfz_hits",
             "offmap", "below_terrain", "cells")
BEST_KEYS = ("best_fval_idx", "best_length_idx")
QS = (1, 63, 65, 130)
# every option a run depends on, set before each evaluation (the engine is shared)
DEFAULTS = dict(group=21, sorted_min_paths=65536, wave_max_paths=0, exact_sum=0,
                exact_sum_volume=0, pair_order=1)
WAVE = 1 << 20   # wave_max_paths that sends every batch of these tests to the wave form


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype == np.float64 else a


def _same(got, want, what=""):
    """Bit equality; any NaN equals any NaN."""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if want.dtype == np.float64:
        n = np.isnan(want)
        np.testing.assert_array_equal(np.isnan(got), n, err_msg=what)
        got, want = np.where(n, 0.0, got), np.where(n, 0.0, want)
    np.testing.assert_array_equal(_bits(got), _bits(want), err_msg=what)


def _same_outputs(got, want, keys, what="", rows=None):
    for k in keys:
        g = got[k].cpu().numpy() if hasattr(got[k], "cpu") else got[k]
        w = want[k] if rows is None else want[k][rows]
        _same(g, w, f"{what} {k}")


class Ctx:
    """The shared engine, its hand volume and the per-(N, maxratio_smooth) oracle."""

    def __init__(self, oracle_mod):
        from uam_path_planning_amd import build
        from uam_path_planning_amd.engine import Engine, PathParams, VolumeGeo
        from uam_path_planning_amd.geometry import compile_map
        from uam_path_planning_amd.scenario import build_region_map, canonical_spec

        if not torch.cuda.is_available():
            pytest.fail("GPU tests need an MI355X")
        build.build_library()
        self.O = oracle_mod
        self.e = Engine(0)
        self.spec = canonical_spec(nfz_polygons=16)
        self.e.set_geometry(compile_map(build_region_map(self.spec)))
        self.PathParams = PathParams
        self.geom = oracle_mod.compile_spec(self.spec)
        self.vox, self.cols = R.hand_volume()
        self.vol = self.e.volume_alloc(VolumeGeo(R.NX, R.NY, R.NZ, R.X0, R.Y_TOP, R.DX, R.DY,
                                                 R.Z0, R.DZ))
        self.vol.buf.zero_()
        self.vol.vox.copy_(self.e.tensor(self.vox.view(np.int32), torch.int32))
        self.vol.cols.copy_(self.e.tensor(self.cols.view(np.int32), torch.int32))
        # the column bitmap K4 / K4w skip clear blocks by (uam_volume_build derives it; the new
        # forms do not read it): every block marked "read the columns", which is always valid
        self.vol.cbits.fill_(-1)
        self._orc = {}
        self.state = None

    def use(self, N, ms=False, **opts):
        """Params and options of the next evaluations; returns the matching oracle."""
        s = self.spec
        o = dict(s["options"])
        o["maxratio_smooth"] = bool(ms)
        if self.state != (N, ms):
            self.e.set_params(self.PathParams(N=N, **o, maxratio=s["maxratio"],
                                              maxalpha=s["maxalpha"],
                                              enlargement=s["enlargement"],
                                              weights=tuple(s["weights"]), altitude=320.0))
            self.state = (N, ms)
        for k, v in {**DEFAULTS, **opts}.items():
            self.e.set_option(k, v)
        if (N, ms) not in self._orc:
            self._orc[(N, ms)] = self.O.Oracle(self.geom, N, o, s["maxratio"], s["maxalpha"],
                                               s["enlargement"], s["weights"], altitude=320.0)
        return self._orc[(N, ms)]

    def ref(self, orc, wp3, n_pairs=None, G=None):
        return R.reference_eval(self.O, orc, self.vox, self.cols, wp3, n_pairs, G)


@pytest.fixture(scope="module")
def cx(oracle_mod):
    return Ctx(oracle_mod)


def _utab(N, D):
    from uam_path_planning_amd.arcs import arc_table

    return arc_table(N, np.linspace(-0.6, 0.6, D) if D > 1 else np.array([0.3]))


def _table(N, A):
    from uam_path_planning_amd import profiles as P

    fam = R.family(P, N)
    return {1: fam[:1], 3: np.ascontiguousarray(fam[[0, 2, 7]]), 8: fam}[A]


# ---- 1. gen_paths3d ---------------------------------------------------------------------------
@pytest.mark.parametrize("N", [1, 9, 80])
def test_gen_paths3d_equals_the_reference_waypoints(cx, N):
    cx.use(N)
    pr = R.pairs6(130)
    for D in (1, 5, 16):
        ut = _utab(N, D)
        for A in (1, 3, 8):
            zt = _table(N, A)
            got = cx.e.gen_paths3d(pr, ut, zt).cpu().numpy()
            _same(got, R.reference_wp3(cx.O, pr, ut, zt), f"wp3 D={D} A={A}")
        # no table: the straight climb of eval_generated3d, the oracle's own bits
        got = cx.e.gen_paths3d(pr, ut).cpu().numpy()
        _same(got, cx.O.gen_paths3d(pr, ut), f"wp3 D={D} ztab=None")


# ---- 2. eval_waypoints3d, lane and wave form ---------------------------------------------------
def _free_waypoints(cx, N, P=257, seed=3):
    """P polylines: arcs jittered off their circle (kin_sum != 0), altitudes that no table
    produces, some waypoints outside the volume on every side, a NaN and an infinite z."""
    rng = np.random.default_rng(seed + N)
    pr = R.pairs6(max(8, (P + 4) // 5), seed=seed)
    wp3 = cx.O.gen_paths3d(pr, _utab(N, 5))[:P].copy()
    W = N + 2
    wp3[:, :, :2] += rng.normal(0.0, 0.4, (P, W, 2))
    wp3[:, :, 2] = rng.uniform(-80.0, 760.0, (P, W))
    wp3[0, :, 2] = rng.uniform(20.0, 600.0, W)       # one path wholly inside in z
    wp3[min(2, P - 1), 0, 2] = np.nan
    wp3[min(3, P - 1), -1, 2] = np.inf
    wp3[min(4, P - 1), :, 2] = R.Z_TOP                # exactly the top face: outside
    wp3[min(5, P - 1), :, 2] = R.Z0                   # exactly the floor: inside
    return wp3


@pytest.mark.parametrize("ms", [False, True])
@pytest.mark.parametrize("N", [1, 2, 7, 8, 9, 40, 80, 256])
def test_eval_waypoints3d_equals_the_oracle(cx, N, ms):
    wp3 = _free_waypoints(cx, N)
    orc = cx.use(N, ms)
    ref = cx.ref(orc, wp3)
    assert (ref["kin_sum"][np.isfinite(ref["kin_sum"])] > 0).any()
    assert (ref["offmap"] > 0).any() and (ref["offmap"] < N + 2).any()
    for form, wave_max, name in (("lane", 0, "K4e"), ("wave", WAVE, "K4ew")):
        cx.use(N, ms, wave_max_paths=wave_max)
        for P in (1, 63, 65, 257):
            got = cx.e.eval_waypoints3d(wp3[:P], cx.vol, want_cells=True)
            assert cx.e.last_kernel() == name and cx.e.last_group() == 0
            _same_outputs(got, ref, PATH_KEYS, f"{form} N={N} P={P}", rows=slice(0, P))


# ---- 3. / 4. the fused call ----------------------------------------------------------------------
def _assert_batch_is_telling(pr, wp3, ref, D, A):
    """The reference of the full batch (130 pairs, 8 profiles) really holds the cases the
    comparison is meant to cover."""
    cells = ref["cells"]
    x, y, z = wp3[..., 0], wp3[..., 1], wp3[..., 2]
    with np.errstate(invalid="ignore"):
        out_xy = ((x < R.X0) | (x >= R.X0 + R.NX * R.DX) | (y > R.Y_TOP) |
                  (y <= R.Y_TOP - R.NY * R.DY))
        out_xy = out_xy & np.isfinite(x) & np.isfinite(y)
    in_xy = ~out_xy & np.isfinite(x) & np.isfinite(y)
    assert (out_xy & (cells < 0)).any(), "no waypoint off the volume in x/y"
    assert (in_xy & (z >= R.Z_TOP) & (cells < 0)).any(), "no waypoint above the volume"
    assert (in_xy & (z < R.Z0) & (cells < 0)).any(), "no waypoint below the volume"
    assert (ref["below_terrain"] > 0).any()
    assert (ref["nfz_hits"] > 0).any()
    assert np.isposinf(ref["min_clearance"]).any()
    assert np.isfinite(ref["min_clearance"]).any()
    assert (ref["best_fval_idx"] % A != 0).any(), "the first profile won every pair"


@pytest.mark.parametrize("ms", [False, True])
@pytest.mark.parametrize("A", [1, 3, 8])
@pytest.mark.parametrize("D", [1, 5, 16])
@pytest.mark.parametrize("N", [1, 9, 40, 80])
def test_profiles_equal_the_oracle_and_the_unfused_calls(cx, N, D, A, ms):
    orc = cx.use(N, ms)
    pr = R.pairs6(130)
    ut, zt = _utab(N, D), _table(N, A)
    wp3 = R.reference_wp3(cx.O, pr, ut, zt)
    ref = cx.ref(orc, wp3, 130, D * A)
    if A == 8 and D > 1 and N >= 9:
        _assert_batch_is_telling(pr, wp3, ref, D, A)
    G = D * A
    for Q in QS:
        got = cx.e.eval_generated3d_profiles(pr[:Q], ut, zt, cx.vol, want_cells=True)
        assert cx.e.last_kernel() == "K4p" and cx.e.last_group() == 0
        what = f"N={N} D={D} A={A} Q={Q}"
        _same_outputs(got, ref, PATH_KEYS, what, rows=slice(0, Q * G))
        _same_outputs(got, ref, BEST_KEYS, what, rows=slice(0, Q))
    # 4. the fused call == eval_waypoints3d(gen_paths3d(...)), on the device's own waypoints
    dev_wp3 = cx.e.gen_paths3d(pr, ut, zt)
    for wave_max in (0, WAVE):
        cx.use(N, ms, wave_max_paths=wave_max)
        two = cx.e.eval_waypoints3d(dev_wp3, cx.vol, want_cells=True)
        _same_outputs(got, {k: two[k].cpu().numpy() for k in PATH_KEYS}, PATH_KEYS,
                      f"unfused wave_max={wave_max}")
    _same(cx.e.argmin(two["cost"], G, True).cpu().numpy(), got["best_fval_idx"].cpu().numpy())
    _same(cx.e.argmin(two["length"], G, False).cpu().numpy(),
          got["best_length_idx"].cpu().numpy())


@pytest.mark.parametrize("Q", [4095, 4096, 4133])
def test_profiles_in_the_pair_order(cx, Q):
    """Batches of 4096 pairs and more run in K4's spatial pair order (workgroups remapped per
    XCD): the threshold, one pair below it, and a count that fills neither the last wave nor
    the eight XCDs evenly.  Same bits as the oracle, and with the order switched off."""
    N, D, A = 9, 5, 3
    orc = cx.use(N)
    rng = np.random.default_rng(Q)
    pr = np.concatenate([R.pairs6(130), R.pairs6(Q - 130, seed=11)])[rng.permutation(Q)]
    ut, zt = _utab(N, D), _table(N, A)
    ref = cx.ref(orc, R.reference_wp3(cx.O, pr, ut, zt), Q, D * A)
    keys = PATH_KEYS + BEST_KEYS
    got = cx.e.eval_generated3d_profiles(pr, ut, zt, cx.vol, want_cells=True)
    _same_outputs(got, ref, keys, f"ordered Q={Q}")
    cx.use(N, pair_order=0)
    got = cx.e.eval_generated3d_profiles(pr, ut, zt, cx.vol, want_cells=True)
    _same_outputs(got, ref, keys, f"unordered Q={Q}")


# ---- 5. no table == eval_generated3d's straight climb ---------------------------------------
@pytest.mark.parametrize("N,D", [(1, 5), (9, 16), (80, 5), (40, 1)])
def test_no_table_equals_eval_generated3d(cx, N, D):
    pr, ut = R.pairs6(130), _utab(N, D)
    keys = PATH_KEYS + BEST_KEYS
    assert cx.vol.packed is None     # no packed copy: eval_generated3d cannot take K4h
    for wave_max, name in ((0, "K4"), (WAVE, "K4w")):
        cx.use(N, False, group=0, wave_max_paths=wave_max)
        W = N + 2
        outs = cx.e.outputs(130 * D, W, n_pairs=130, want_cells=True)
        want = cx.e.eval_generated3d(pr, ut, cx.vol, outputs=outs)
        assert cx.e.last_kernel() == name
        got = cx.e.eval_generated3d_profiles(pr, ut, None, cx.vol, want_cells=True)
        assert cx.e.last_kernel() == "K4p"
        _same_outputs(got, {k: want[k].cpu().numpy() for k in keys}, keys, f"{name} N={N}")


# ---- 6. a path's bits do not depend on its batch -----------------------------------------------
def test_outputs_do_not_depend_on_the_batch(cx):
    N, D, A = 40, 5, 8
    cx.use(N)
    pr, ut, zt = R.pairs6(130), _utab(N, D), _table(N, A)
    G = D * A
    full = cx.e.eval_generated3d_profiles(pr, ut, zt, cx.vol, want_cells=True)
    full = {k: v.cpu().numpy() for k, v in full.items()}
    for q in (0, 1, 5, 64, 129):
        one = cx.e.eval_generated3d_profiles(pr[q:q + 1], ut, zt, cx.vol, want_cells=True)
        _same_outputs(one, full, PATH_KEYS, f"pair {q} alone", rows=slice(q * G, (q + 1) * G))
        _same_outputs(one, full, BEST_KEYS, f"pair {q} alone", rows=slice(q, q + 1))
    # and the explicit form: a path alone (wave form) against the batch (lane form)
    wp3 = cx.e.gen_paths3d(pr, ut, zt)
    for p in (0, 7, 130 * G - 1):
        cx.use(N, wave_max_paths=WAVE)
        one = cx.e.eval_waypoints3d(wp3[p:p + 1], cx.vol, want_cells=True)
        _same_outputs(one, full, PATH_KEYS, f"path {p} alone", rows=slice(p, p + 1))


# ---- 7. refusals ------------------------------------------------------------------------------
def _check_still_right(cx, N, D, A):
    orc = cx.use(N)
    pr, ut, zt = R.pairs6(16), _utab(N, D), _table(N, A)
    ref = cx.ref(orc, R.reference_wp3(cx.O, pr, ut, zt), 16, D * A)
    got = cx.e.eval_generated3d_profiles(pr, ut, zt, cx.vol, want_cells=True)
    _same_outputs(got, ref, PATH_KEYS + BEST_KEYS, "after a refusal")
    two = cx.e.eval_waypoints3d(cx.e.gen_paths3d(pr, ut, zt), cx.vol, want_cells=True)
    _same_outputs(two, ref, PATH_KEYS, "after a refusal (explicit)")


def test_refusals_name_their_reason_and_leave_the_engine_usable(cx):
    from uam_path_planning_amd import _lib

    N, D = 9, 5
    cx.use(N)
    e, vol = cx.e, cx.vol
    pr, ut, zt = R.pairs6(16), _utab(N, D), _table(N, 3)
    W = N + 2
    with pytest.raises(ValueError, match=r"A = 0 outside \[1, 8\]"):
        e.eval_generated3d_profiles(pr, ut, np.zeros((0, W, 3)), vol)
    with pytest.raises(ValueError, match=r"A = 9 outside \[1, 8\]"):
        e.eval_generated3d_profiles(pr, ut, np.zeros((9, W, 3)), vol)
    with pytest.raises(ValueError, match=r"A = 9 outside \[1, 8\]"):
        e.gen_paths3d(pr, ut, np.zeros((9, W, 3)))
    with pytest.raises(ValueError, match=r"D outside \[1, 16\]"):
        e.eval_generated3d_profiles(pr, _utab(N, 17), zt, vol)
    with pytest.raises(ValueError, match=r"D outside \[1, 16\]"):
        e.gen_paths3d(pr, _utab(N, 17), zt)
    # shape checks of the Python layer
    with pytest.raises(ValueError, match="profile table has shape"):
        e.eval_generated3d_profiles(pr, ut, np.zeros((3, W + 1, 3)), vol)
    with pytest.raises(ValueError, match="arc table has shape"):
        e.eval_generated3d_profiles(pr, _utab(N + 1, D), zt, vol)
    with pytest.raises(ValueError, match="waypoints have shape"):
        e.eval_waypoints3d(np.zeros((4, W, 2)), vol)
    # no table with A = 2 (the Python layer cannot express it: straight to the C ABI)
    prd, utd = e.tensor(pr, torch.float64), e.tensor(ut, torch.float64)
    o, s = e.outputs(16 * D * 2, W, n_pairs=16)
    vd = vol.geo.as_struct()
    with pytest.raises(ValueError, match="ztab is NULL .* A = 2: A must be 1"):
        _lib.check(e.lib.uam_eval_generated3d_profiles(
            e._ctx, ctypes.byref(vd), ctypes.c_void_p(vol.buf.data_ptr()),
            ctypes.c_void_p(prd.data_ptr()), 16, ctypes.c_void_p(utd.data_ptr()), D, None, 2,
            ctypes.byref(s), e.stream))
    with pytest.raises(ValueError, match="2\\^31 or more paths"):   # refused before any pointer
        _lib.check(e.lib.uam_eval_generated3d_profiles(
            e._ctx, ctypes.byref(vd), None, None, (1 << 31) // D + 1, None, D, None, 1, None,
            None))
    # a misaligned volume buffer (8 bytes into the real one; never read)
    bad = dataclasses.replace(vol, buf=vol.buf[2:])
    with pytest.raises(ValueError, match="volume buffer not 256-B aligned"):
        e.eval_generated3d_profiles(pr, ut, zt, bad)
    with pytest.raises(ValueError, match="volume buffer not 256-B aligned"):
        e.eval_waypoints3d(np.zeros((4, W, 3)), bad)
    _check_still_right(cx, N, D, 3)
    # the exact volume sums: exact or an error, never ordered
    try:
        e.set_option("exact_sum_volume", 1)
        with pytest.raises(ValueError, match="UAM_OPT_EXACT_SUM_VOLUME"):
            e.eval_generated3d_profiles(pr, ut, zt, vol)
        with pytest.raises(ValueError, match="UAM_OPT_EXACT_SUM_VOLUME"):
            e.eval_waypoints3d(np.zeros((4, W, 3)), vol)
        e.gen_paths3d(pr, ut, zt)      # sums nothing: not refused
    finally:
        e.set_option("exact_sum_volume", 0)
    _check_still_right(cx, N, D, 3)


# ---- 8. the kernel names ---------------------------------------------------------------------
def test_last_kernel_names_the_new_forms(cx):
    N, D = 9, 5
    cx.use(N)
    pr, ut, zt = R.pairs6(16), _utab(N, D), _table(N, 3)
    cx.e.eval_generated3d_profiles(pr, ut, zt, cx.vol)
    assert (cx.e.last_kernel(), cx.e.last_group()) == ("K4p", 0)
    wp3 = cx.e.gen_paths3d(pr, ut, zt)
    assert cx.e.last_kernel() == "K4p"          # generation is no evaluation
    cx.e.eval_waypoints3d(wp3, cx.vol)
    assert (cx.e.last_kernel(), cx.e.last_group()) == ("K4e", 0)
    cx.use(N, wave_max_paths=16 * D * 3)        # the threshold itself: still the wave form
    cx.e.eval_waypoints3d(wp3, cx.vol)
    assert (cx.e.last_kernel(), cx.e.last_group()) == ("K4ew", 0)
    cx.use(N, wave_max_paths=16 * D * 3 - 1)
    cx.e.eval_waypoints3d(wp3, cx.vol)
    assert cx.e.last_kernel() == "K4e"
