"""The vertical terms on the GPU: Engine.eval_waypoints3d(..., vertical=) ("K4e+v" lane per path,
"K4ew+v" wave per path) and Engine.eval_generated3d_profiles(..., vertical=) ("K4p+v") against
tests/vertical_ref.py, bit for bit (uint64 views, NaN equals NaN) on every float64 output, count
and selection.

Volume, pairs and profile family: test_gpu_profiles.py's (profiles_ref), Q = 130 pairs so that
the last wave is partial, plus one pair with a NaN altitude.  The oracle part of a reference
(risk, no-fly, counts, voxels) depends on the waypoints alone and is computed once per
waypoint set; the geometry terms are a few numpy passes per evaluation."""
import ctypes
import math

import numpy as np
import pytest

import profiles_ref as R
import vertical_ref as V

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

PATH_KEYS = ("cost", "length_q", "length", "kin_sum", "climb_sum", "nfz_sum", "min_clearance",
             "nfz_hits", "offmap", "below_terrain", "cells")
OLD_KEYS = tuple(k for k in PATH_KEYS if k != "climb_sum")
BEST_KEYS = ("best_fval_idx", "best_length_idx")
DEFAULTS = dict(group=21, sorted_min_paths=65536, wave_max_paths=0, exact_sum=0,
                exact_sum_volume=0, pair_order=1)
WAVE = 1 << 20   # wave_max_paths that sends every batch of these tests to the wave form
ANCHOR = (3.0, -2.0)
Q = 130
# z_scale x (sin_climb, sin_descent): every scale with no limit, and 0 and 0.1 in both roles
VERTS = [(zs, sc, sd) for zs in (0.0, 1e-3, 1e-2)
         for sc, sd in ((math.inf, math.inf), (0.0, 0.1), (0.1, 0.0))]
COMBOS = [(ls, ms, quirk) for ls in (False, True) for ms in (False, True)
          for quirk in (False, True)]


def _same(got, want, what=""):
    """Bit equality; any NaN equals any NaN."""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if want.dtype == np.float64:
        n = np.isnan(want)
        np.testing.assert_array_equal(np.isnan(got), n, err_msg=what)
        got = np.where(n, 0.0, got).view(np.uint64)
        want = np.where(n, 0.0, want).view(np.uint64)
    np.testing.assert_array_equal(got, want, err_msg=what)


def _host(o):
    return {k: (v.cpu().numpy() if hasattr(v, "cpu") else v) for k, v in o.items()}


def _same_outputs(got, want, keys, what="", rows=None):
    got = _host(got)
    for k in keys:
        _same(got[k], want[k] if rows is None else want[k][rows], f"{what} {k}")


class Ctx:
    """The shared engine, its hand volume, the oracles and the references' oracle parts."""

    def __init__(self, oracle_mod):
        from uam_path_planning_amd import build
        from uam_path_planning_amd.engine import Engine, PathParams, Vertical, VolumeGeo
        from uam_path_planning_amd.geometry import compile_map
        from uam_path_planning_amd.scenario import build_region_map, canonical_spec

        if not torch.cuda.is_available():
            pytest.fail("GPU tests need an MI355X")
        build.build_library()
        self.O = oracle_mod
        self.e = Engine(0)
        self.spec = canonical_spec(nfz_polygons=16)
        self.e.set_geometry(compile_map(build_region_map(self.spec)))
        self.PathParams, self.Vertical = PathParams, Vertical
        self.geom = oracle_mod.compile_spec(self.spec)
        self.vox, self.cols = R.hand_volume()
        self.vol = self.e.volume_alloc(VolumeGeo(R.NX, R.NY, R.NZ, R.X0, R.Y_TOP, R.DX, R.DY,
                                                 R.Z0, R.DZ))
        self.vol.buf.zero_()
        self.vol.vox.copy_(self.e.tensor(self.vox.view(np.int32), torch.int32))
        self.vol.cols.copy_(self.e.tensor(self.cols.view(np.int32), torch.int32))
        self.vol.cbits.fill_(-1)
        self._orc, self._base = {}, {}
        self.state = None

    def use(self, N, ls=False, ms=False, quirk=True, anchored=True, **opts):
        """Params and options of the next evaluations; returns the reference's Geo.  With the
        quirk on the anchor is ANCHOR (anchored unset: p_0, the oracle's default)."""
        s = self.spec
        o = dict(s["options"])
        o["length_smooth"], o["maxratio_smooth"] = bool(ls), bool(ms)
        anchor = ANCHOR if quirk and anchored else None
        if self.state != (N, ls, ms, quirk, anchored):
            self.e.set_params(self.PathParams(N=N, **o, maxratio=s["maxratio"],
                                              maxalpha=s["maxalpha"],
                                              enlargement=s["enlargement"],
                                              weights=tuple(s["weights"]), altitude=320.0,
                                              quirk_length=bool(quirk), anchor=anchor))
            self.state = (N, ls, ms, quirk, anchored)
        for k, v in {**DEFAULTS, **opts}.items():
            self.e.set_option(k, v)
        return V.Geo(length_smooth=bool(ls), maxratio_smooth=bool(ms), quirk_length=bool(quirk),
                     anchor=anchor, maxratio=s["maxratio"], maxalpha=s["maxalpha"])

    def orc(self, N):
        if N not in self._orc:
            s = self.spec
            self._orc[N] = self.O.Oracle(self.geom, N, dict(s["options"]), s["maxratio"],
                                         s["maxalpha"], s["enlargement"], s["weights"],
                                         altitude=320.0)
        return self._orc[N]

    def base(self, key, wp3):
        """The oracle part of the reference of waypoints wp3, computed once per key."""
        if key not in self._base:
            self._base[key] = R.reference_eval(self.O, self.orc(wp3.shape[1] - 2), self.vox,
                                               self.cols, wp3)
        return self._base[key]

    def ref(self, key, wp3, geo, vert, n_pairs=None, G=None):
        return V.reference_eval_v(self.O, self.orc(wp3.shape[1] - 2), self.vox, self.cols, wp3,
                                  geo, V.Vert(*vert), n_pairs, G, base=self.base(key, wp3))

    def old_ref(self, wp3, n_pairs=None, G=None, ms=False):
        """The oracle's own evaluation (x/y geometry terms) for the calls without vertical."""
        s = self.spec
        o = dict(s["options"])
        o["length_smooth"], o["maxratio_smooth"] = False, bool(ms)   # use(N, False, ms)
        orc = self.O.Oracle(self.geom, wp3.shape[1] - 2, o, s["maxratio"], s["maxalpha"],
                            s["enlargement"], s["weights"], altitude=320.0)
        return R.reference_eval(self.O, orc, self.vox, self.cols, wp3, n_pairs, G)


@pytest.fixture(scope="module")
def cx(oracle_mod):
    return Ctx(oracle_mod)


def _utab(N, D):
    from uam_path_planning_amd.arcs import arc_table

    return arc_table(N, np.linspace(-0.6, 0.6, D) if D > 1 else np.array([0.3]))


def _table(N, A):
    """A profiles of the family; for A = 2, 4 and 5 the straight climb is not profile 0."""
    from uam_path_planning_amd import profiles as P

    fam = R.family(P, N)
    rows = {1: [0], 2: [1, 0], 3: [0, 2, 7], 4: [1, 0, 4, 5], 5: [3, 0, 2, 6, 7],
            8: list(range(8))}[A]
    return np.ascontiguousarray(fam[rows])


def _pairs(n=Q, finite_altitudes=False):
    pr = R.pairs6(n)
    if not finite_altitudes:
        pr[8, 2] = np.nan           # one pair with a NaN altitude
    return pr


def _free_waypoints(cx, N, P=257, seed=3):
    """P polylines: arcs jittered off their circle (kin_sum != 0), altitudes that no table
    produces, some waypoints outside the volume, a NaN and an infinite altitude, one level
    path and one whose points coincide."""
    rng = np.random.default_rng(seed + N)
    pr = R.pairs6(max(8, (P + 4) // 5), seed=seed)
    wp3 = cx.O.gen_paths3d(pr, _utab(N, 5))[:P].copy()
    W = N + 2
    wp3[:, :, :2] += rng.normal(0.0, 0.4, (P, W, 2))
    wp3[:, :, 2] = rng.uniform(-80.0, 760.0, (P, W))
    wp3[0, :, 2] = rng.uniform(20.0, 600.0, W)
    wp3[2, 0, 2] = np.nan
    wp3[3, -1, 2] = np.inf
    wp3[4, :, 2] = 300.0                              # level flight
    wp3[5, :, :] = wp3[5, :1, :]                      # every segment has length 0
    wp3[6, :, :2] = wp3[6, :1, :2]                    # a vertical path
    return wp3


# ---- 1. explicit waypoints: lane and wave form ----------------------------------------------------
@pytest.mark.parametrize("ls,ms,quirk", COMBOS)
@pytest.mark.parametrize("N", [1, 2, 3, 9])
def test_explicit_forms_equal_the_reference(cx, N, ls, ms, quirk):
    wp3 = _free_waypoints(cx, N)
    geo = cx.use(N, ls, ms, quirk)
    seen_climb = False
    for vert in VERTS:
        ref = cx.ref(("free", N), wp3, geo, vert)
        seen_climb |= bool((ref["climb_sum"] > 0).any())
        if vert[0] > 0:
            assert (ref["kin_sum"][np.isfinite(ref["kin_sum"])] > 0).any() or N == 1
        for wave_max, name in ((0, "K4e+v"), (WAVE, "K4ew+v")):
            cx.use(N, ls, ms, quirk, wave_max_paths=wave_max)
            for P in (65, 257):
                got = cx.e.eval_waypoints3d(wp3[:P], cx.vol, want_cells=True,
                                            vertical=cx.Vertical(*vert))
                assert cx.e.last_kernel() == name and cx.e.last_group() == 0
                _same_outputs(got, ref, PATH_KEYS, f"{name} N={N} P={P} vert={vert}",
                              rows=slice(0, P))
    assert seen_climb


# ---- 2. the fused call ------------------------------------------------------------------------
@pytest.mark.parametrize("ls,ms,quirk", COMBOS)
@pytest.mark.parametrize("N", [1, 2, 3, 9])
def test_profiles_equal_the_reference_and_the_explicit_form(cx, N, ls, ms, quirk):
    geo = cx.use(N, ls, ms, quirk)
    pr = _pairs()
    i = COMBOS.index((ls, ms, quirk)) + N
    used = set()
    for D in (1, 5, 16):
        ut = _utab(N, D)
        for A in (1, 2, 3, 4, 5, 8):
            zt = _table(N, A)
            vert = VERTS[i % len(VERTS)]
            i += 1
            used.add(vert)
            wp3 = R.reference_wp3(cx.O, pr, ut, zt)
            ref = cx.ref(("fam", N, D, A), wp3, geo, vert, Q, D * A)
            got = cx.e.eval_generated3d_profiles(pr, ut, zt, cx.vol, want_cells=True,
                                                 vertical=cx.Vertical(*vert))
            assert cx.e.last_kernel() == "K4p+v" and cx.e.last_group() == 0
            what = f"N={N} D={D} A={A} vert={vert}"
            _same_outputs(got, ref, PATH_KEYS + BEST_KEYS, what)
            if vert[0] > 0 and A in (2, 4, 5) and N > 1:
                assert (ref["best_length_idx"] % A != 0).any(), what
    assert len(used) == len(VERTS)
    # K4p+v == K4e+v / K4ew+v on the device's own waypoints (the last table, D = 16, A = 8)
    got = _host(got)
    dev_wp3 = cx.e.gen_paths3d(pr, ut, zt)
    for wave_max in (0, WAVE):
        cx.use(N, ls, ms, quirk, wave_max_paths=wave_max)
        two = cx.e.eval_waypoints3d(dev_wp3, cx.vol, want_cells=True,
                                    vertical=cx.Vertical(*vert))
        _same_outputs(two, got, PATH_KEYS, f"unfused wave_max={wave_max}")
    _same(cx.e.argmin(two["cost"], 16 * 8, True).cpu().numpy(), got["best_fval_idx"])
    _same(cx.e.argmin(two["length"], 16 * 8, False).cpu().numpy(), got["best_length_idx"])


@pytest.mark.parametrize("N,D", [(1, 5), (3, 1), (9, 16)])
def test_no_table_is_the_straight_climb_with_vertical_terms(cx, N, D):
    geo = cx.use(N)
    pr, ut = _pairs(), _utab(N, D)
    wp3 = cx.O.gen_paths3d(pr, ut)       # the oracle's own straight climb
    for vert in (VERTS[3], VERTS[7]):
        ref = cx.ref(("climb", N, D), wp3, geo, vert, Q, D)
        got = cx.e.eval_generated3d_profiles(pr, ut, None, cx.vol, want_cells=True,
                                             vertical=cx.Vertical(*vert))
        assert cx.e.last_kernel() == "K4p+v"
        _same_outputs(got, ref, PATH_KEYS + BEST_KEYS, f"ztab=None N={N} D={D} vert={vert}")


@pytest.mark.parametrize("Qn", [63, 64, 65, 1])
def test_a_pairs_bits_do_not_depend_on_the_batch(cx, Qn):
    N, D, A = 9, 5, 3
    geo = cx.use(N)
    pr, ut, zt = _pairs(), _utab(N, D), _table(N, A)
    vert = VERTS[4]
    ref = cx.ref(("fam", N, D, A), R.reference_wp3(cx.O, pr, ut, zt), geo, vert, Q, D * A)
    got = cx.e.eval_generated3d_profiles(pr[:Qn], ut, zt, cx.vol, want_cells=True,
                                         vertical=cx.Vertical(*vert))
    _same_outputs(got, ref, PATH_KEYS, f"Q={Qn}", rows=slice(0, Qn * D * A))
    _same_outputs(got, ref, BEST_KEYS, f"Q={Qn}", rows=slice(0, Qn))


# ---- 3. z_scale = 0 is the existing call; the existing call is untouched ------------------------
@pytest.mark.parametrize("ms", [False, True])
def test_zero_scale_equals_the_existing_calls_which_stay_as_they_were(cx, ms):
    N, D, A = 9, 5, 8
    cx.use(N, False, ms, True, anchored=False)      # the oracle's params
    pr, ut, zt = _pairs(finite_altitudes=True), _utab(N, D), _table(N, A)
    wp3 = R.reference_wp3(cx.O, pr, ut, zt)
    assert np.isfinite(wp3[..., 2]).all()
    oracle = cx.old_ref(wp3, Q, D * A, ms)
    before = _host(cx.e.eval_generated3d_profiles(pr, ut, zt, cx.vol, want_cells=True))
    assert cx.e.last_kernel() == "K4p" and "climb_sum" not in before
    _same_outputs(before, oracle, OLD_KEYS + BEST_KEYS, "K4p before")
    for sc, sd in ((math.inf, math.inf), (0.0, 0.1)):
        got = _host(cx.e.eval_generated3d_profiles(pr, ut, zt, cx.vol, want_cells=True,
                                                   vertical=cx.Vertical(0.0, sc, sd)))
        assert cx.e.last_kernel() == "K4p+v"
        _same_outputs(got, before, OLD_KEYS + BEST_KEYS, f"K4p+v z_scale=0 limits={sc, sd}")
        assert not got["climb_sum"].any() and not np.signbit(got["climb_sum"]).any()
    after = cx.e.eval_generated3d_profiles(pr, ut, zt, cx.vol, want_cells=True)
    assert cx.e.last_kernel() == "K4p"
    _same_outputs(after, before, OLD_KEYS + BEST_KEYS, "K4p after a _v call")
    # the explicit forms, on the same waypoints
    for wave_max, name in ((0, "K4e"), (WAVE, "K4ew")):
        cx.use(N, False, ms, True, anchored=False, wave_max_paths=wave_max)
        old = _host(cx.e.eval_waypoints3d(wp3, cx.vol, want_cells=True))
        assert cx.e.last_kernel() == name
        _same_outputs(old, oracle, OLD_KEYS, f"{name} before")
        got = _host(cx.e.eval_waypoints3d(wp3, cx.vol, want_cells=True,
                                          vertical=cx.Vertical(0.0, 0.1, 0.0)))
        assert cx.e.last_kernel() == name + "+v"
        _same_outputs(got, old, OLD_KEYS, f"{name}+v z_scale=0")
        assert not got["climb_sum"].any()
        again = cx.e.eval_waypoints3d(wp3, cx.vol, want_cells=True)
        assert cx.e.last_kernel() == name
        _same_outputs(again, old, OLD_KEYS, f"{name} after a _v call")


# ---- 4. the pair order --------------------------------------------------------------------------
def test_pair_order_on_and_off_give_the_same_bits(cx):
    N, D, A, Qn = 9, 5, 3, 4133
    geo = cx.use(N)
    rng = np.random.default_rng(Qn)
    pr = np.concatenate([_pairs(), R.pairs6(Qn - Q, seed=11)])[rng.permutation(Qn)]
    ut, zt = _utab(N, D), _table(N, A)
    vert = VERTS[5]
    ref = cx.ref(("order", Qn), R.reference_wp3(cx.O, pr, ut, zt), geo, vert, Qn, D * A)
    for order in (1, 0):
        cx.use(N, pair_order=order)
        got = cx.e.eval_generated3d_profiles(pr, ut, zt, cx.vol, want_cells=True,
                                             vertical=cx.Vertical(*vert))
        _same_outputs(got, ref, PATH_KEYS + BEST_KEYS, f"pair_order={order}")


# ---- 5. refusals: argument checks that return before any launch --------------------------------
def test_refusals_name_their_reason_and_leave_the_engine_usable(cx):
    from uam_path_planning_amd import _lib

    N, D, A = 9, 5, 3
    geo = cx.use(N)
    e, vol = cx.e, cx.vol
    pr, ut, zt = _pairs(16), _utab(N, D), _table(N, A)
    W = N + 2
    wp3 = np.zeros((4, W, 3))
    good = cx.Vertical(1e-3, 0.1, 0.1)

    def both(vertical):
        yield lambda: e.eval_generated3d_profiles(pr, ut, zt, vol, vertical=vertical)
        yield lambda: e.eval_waypoints3d(wp3, vol, vertical=vertical)

    for bad in (math.nan, -1e-3, math.inf):
        for call in both(cx.Vertical(bad)):
            with pytest.raises(ValueError, match="z_scale must be finite and >= 0"):
                call()
    for sc, sd in ((math.nan, 0.1), (0.1, math.nan), (-0.1, 0.1), (0.1, -0.1)):
        for call in both(cx.Vertical(1e-3, sc, sd)):
            with pytest.raises(ValueError, match="sin_climb and sin_descent must be >= 0"):
                call()
    # a NULL vert and a wrong abi_version: straight to the C ABI
    prd, utd, ztd = (e.tensor(a, torch.float64) for a in (pr, ut, zt))
    wpd = e.tensor(wp3, torch.float64)
    o, s = e.outputs(16 * D * A, W, n_pairs=16)
    vd = vol.geo.as_struct()
    vp = ctypes.c_void_p
    for vert, status, text in ((None, _lib.UAM_E_INVALID, "vert is NULL"),
                               (_lib.Vertical(3, 1e-3, 0.1, 0.1), _lib.UAM_E_VERSION,
                                "uam_vertical.abi_version 3 != 2")):
        vref = None if vert is None else ctypes.byref(vert)
        st = e.lib.uam_eval_generated3d_profiles_v(
            e._ctx, ctypes.byref(vd), vp(vol.buf.data_ptr()), vp(prd.data_ptr()), 16,
            vp(utd.data_ptr()), D, vp(ztd.data_ptr()), A, vref, ctypes.byref(s), None, e.stream)
        assert st == status and text in _lib.last_error()
        st = e.lib.uam_eval_waypoints3d_v(
            e._ctx, ctypes.byref(vd), vp(vol.buf.data_ptr()), vp(wpd.data_ptr()), 4, vref,
            ctypes.byref(s), None, e.stream)
        assert st == status and text in _lib.last_error()
    # the checks of the calls they extend
    with pytest.raises(ValueError, match=r"A = 9 outside \[1, 8\]"):
        e.eval_generated3d_profiles(pr, ut, np.zeros((9, W, 3)), vol, vertical=good)
    with pytest.raises(ValueError, match=r"D outside \[1, 16\]"):
        e.eval_generated3d_profiles(pr, _utab(N, 17), zt, vol, vertical=good)
    gv = good.as_struct()
    with pytest.raises(ValueError, match="ztab is NULL .* A = 2: A must be 1"):
        _lib.check(e.lib.uam_eval_generated3d_profiles_v(
            e._ctx, ctypes.byref(vd), vp(vol.buf.data_ptr()), vp(prd.data_ptr()), 16,
            vp(utd.data_ptr()), D, None, 2, ctypes.byref(gv), ctypes.byref(s), None, e.stream))
    with pytest.raises(ValueError, match="n_paths < 0"):
        _lib.check(e.lib.uam_eval_waypoints3d_v(
            e._ctx, ctypes.byref(vd), vp(vol.buf.data_ptr()), vp(wpd.data_ptr()), -1,
            ctypes.byref(gv), ctypes.byref(s), None, e.stream))
    with pytest.raises(ValueError, match="outputs\\['climb_sum'\\] holds 3 entries"):
        outs = e.outputs(16 * D * A, W, n_pairs=16)
        outs[0]["climb_sum"] = e.empty((3,), torch.float64)
        e.eval_generated3d_profiles(pr, ut, zt, vol, outputs=outs, vertical=good)
    # the exact volume sums: exact or an error, never ordered
    try:
        e.set_option("exact_sum_volume", 1)
        for call in both(good):
            with pytest.raises(ValueError, match="UAM_OPT_EXACT_SUM_VOLUME"):
                call()
    finally:
        e.set_option("exact_sum_volume", 0)
    # still right afterwards
    vert = (1e-3, 0.1, 0.1)
    ref = cx.ref(("fam16", N, D, A), R.reference_wp3(cx.O, pr, ut, zt), geo, vert, 16, D * A)
    got = e.eval_generated3d_profiles(pr, ut, zt, vol, want_cells=True, vertical=good)
    _same_outputs(got, ref, PATH_KEYS + BEST_KEYS, "after the refusals")
    # a caller's own climb_sum buffer is the one written
    outs = e.outputs(16 * D * A, W, n_pairs=16, want_cells=True)
    outs[0]["climb_sum"] = e.empty((16 * D * A,), torch.float64)
    got = e.eval_generated3d_profiles(pr, ut, zt, vol, outputs=outs, vertical=good)
    assert got["climb_sum"] is outs[0]["climb_sum"]
    _same_outputs(got, ref, PATH_KEYS + BEST_KEYS, "caller's outputs")
