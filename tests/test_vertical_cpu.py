"""The vertical terms (uam_vertical: 3-D length, turn and climb rows) without a GPU: the two new
symbols (header, _lib.SIGNATURES and the built library agree), the header's statement of the
definition, and the numpy reference tests/vertical_ref.py itself -- against the oracle at
z_scale = 0, against an independent extended-precision restatement, against a closed form, and
that the vertical terms change the selections."""
import ctypes
import math
import os
import re

import numpy as np
import pytest

import profiles_ref as R
import vertical_ref as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -53


def _spec():
    from uam_path_planning_amd.scenario import canonical_spec

    return canonical_spec(nfz_polygons=16)


def _oracle(oracle_mod, N, maxratio_smooth=False):
    spec = _spec()
    opts = dict(spec["options"])
    opts["maxratio_smooth"] = maxratio_smooth
    return oracle_mod.Oracle(oracle_mod.compile_spec(spec), N, opts, spec["maxratio"],
                             spec["maxalpha"], spec["enlargement"], spec["weights"],
                             altitude=320.0)


def _geo(ms=False, **kw):
    spec = _spec()
    return V.Geo(length_smooth=bool(spec["options"]["length_smooth"]), maxratio_smooth=ms,
                 maxratio=spec["maxratio"], maxalpha=spec["maxalpha"], **kw)


def _batch(oracle_mod, N=9, D=5, Q=130, first=None):
    """(pairs, wp3, table) of the hand volume's pairs x D arcs x the 8-profile family; first:
    the family's row that goes to profile 0 (None: the family's own order, the straight
    climb)."""
    from uam_path_planning_amd import profiles as P
    from uam_path_planning_amd.arcs import arc_table
    from uam_path_planning_amd.scenario import displacements

    fam = R.family(P, N)
    if first is not None:
        order = [first] + [a for a in range(fam.shape[0]) if a != first]
        fam = np.ascontiguousarray(fam[order])
    pr = R.pairs6(Q)
    ut = arc_table(N, displacements(D))
    return pr, R.reference_wp3(oracle_mod, pr, ut, fam), fam


def _same_bits(a, b, what):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.dtype == np.float64:
        n = np.isnan(b)
        np.testing.assert_array_equal(np.isnan(a), n, err_msg=what)
        a, b = np.where(n, 0.0, a).view(np.uint64), np.where(n, 0.0, b).view(np.uint64)
    np.testing.assert_array_equal(a, b, err_msg=what)


# ---- the ABI ----------------------------------------------------------------------------------
def test_symbols_and_prototypes():
    from uam_path_planning_amd import _lib, build

    build.build_library()
    lib = _lib.load()
    with open(os.path.join(ROOT, "include", "uampath.h")) as f:
        text = re.sub(r"/\*.*?\*/", " ", f.read(), flags=re.S)
    text = re.sub(r"\s+", " ", text)
    for proto in (
            "typedef struct { uint32_t abi_version; double z_scale; double sin_climb; "
            "double sin_descent; } uam_vertical;",
            "int uam_eval_waypoints3d_v(uam_ctx* ctx, const uam_volume_desc* desc, "
            "const void* vol_dev, const double* wp3_dev , int64_t n_paths, "
            "const uam_vertical* vert, const uam_path_outputs* out, double* climb_sum_dev , "
            "uam_stream stream);",
            "int uam_eval_generated3d_profiles_v(uam_ctx* ctx, const uam_volume_desc* desc, "
            "const void* vol_dev, const double* pairs6_dev, int64_t n_pairs, "
            "const double* utab_dev, int32_t D, const double* ztab_dev, int32_t A, "
            "const uam_vertical* vert, const uam_path_outputs* out, double* climb_sum_dev , "
            "uam_stream stream);"):
        assert proto in text, proto
    vp, i32, i64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64
    vd, po = ctypes.POINTER(_lib.VolumeDesc), ctypes.POINTER(_lib.PathOutputs)
    ve = ctypes.POINTER(_lib.Vertical)
    want = {"uam_eval_waypoints3d_v": [vp, vd, vp, vp, i64, ve, po, vp, vp],
            "uam_eval_generated3d_profiles_v": [vp, vd, vp, vp, i64, vp, i32, vp, i32, ve, po, vp,
                                                vp]}
    for name, args in want.items():
        assert _lib.SIGNATURES[name] == (ctypes.c_int, args), name
        fn = getattr(lib, name)
        assert fn.restype is ctypes.c_int and list(fn.argtypes) == args, name
    assert [f[0] for f in _lib.Vertical._fields_] == ["abi_version", "z_scale", "sin_climb",
                                                      "sin_descent"]
    assert ctypes.sizeof(_lib.Vertical) == 32 and _lib.Vertical.z_scale.offset == 8
    assert lib.uam_abi_version() == _lib.ABI_VERSION == 2     # no ABI bump, no new option
    assert max(_lib.OPTIONS.values()) == 24
    # no GPU is touched by a NULL context: the argument check answers
    v = _lib.Vertical(2, 1e-3, math.inf, math.inf)
    assert lib.uam_eval_waypoints3d_v(None, None, None, None, 0, ctypes.byref(v), None, None,
                                      None) == _lib.UAM_E_INVALID
    assert lib.uam_eval_generated3d_profiles_v(None, None, None, None, 0, None, 1, None, 1,
                                               ctypes.byref(v), None, None,
                                               None) == _lib.UAM_E_INVALID
    assert lib.uam_eval_waypoints3d_v(None, None, None, None, 0, None, None, None,
                                      None) == _lib.UAM_E_INVALID


def test_python_layer_names_the_vertical_terms():
    from uam_path_planning_amd import _lib, profiles
    from uam_path_planning_amd.engine import Vertical

    s = Vertical(1e-3).as_struct()
    assert isinstance(s, _lib.Vertical) and s.abi_version == 2 and s.z_scale == 1e-3
    assert s.sin_climb == math.inf and s.sin_descent == math.inf
    s = Vertical(2e-3, 0.25, 0.5).as_struct()
    assert (s.z_scale, s.sin_climb, s.sin_descent) == (2e-3, 0.25, 0.5)
    assert profiles.sin_of_angle(0.0) == 0.0 and profiles.sin_of_angle(90.0) == 1.0
    assert abs(profiles.sin_of_angle(30.0) - 0.5) <= 2 * U
    for bad in (-1.0, 90.5, math.nan):
        with pytest.raises(ValueError):
            profiles.sin_of_angle(bad)


def test_header_states_the_definition():
    with open(os.path.join(ROOT, "include", "uampath.h")) as f:
        text = re.sub(r"\s+", " ", re.sub(r"^ \*", " ", f.read(), flags=re.M))
    for phrase in (
            "dz = (z_j - z_{j-1}) * kappa",
            "s = ((0 + dx*dx) + dy*dy) + dz*dz; n = sqrt(s)",
            "if (!quirk || j <= N) L += ls ? n*n : n",
            "dt = ((0 + pdx*dx) + pdy*dy) + pdz*dz",
            "cu = fmax(0, dz - sin_climb*n); cd = fmax(0, (-dz) - sin_descent*n)",
            "climb_sum = (climb_sum + cu) + cd",
            "The anchor term stays x/y only",
            "With kappa = 0 and finite altitudes every output equals the call without _v bit for bit",
            '"K4e+v" / "K4ew+v" / "K4p+v"',
            "best_length_idx selects among all D*A candidates",
            "sees the climb through (N+1) L",
            "the rule's first index wins"):          # still stated, for the call without _v
        assert phrase in text, phrase


# ---- z_scale = 0 is the oracle-pinned definition ------------------------------------------------
@pytest.mark.parametrize("ms", [False, True])
def test_zero_scale_equals_the_oracle(oracle_mod, ms):
    N, D = 9, 5
    orc = _oracle(oracle_mod, N, ms)
    vox, cols = R.hand_volume()
    pr, wp3, fam = _batch(oracle_mod, N, D)
    A = fam.shape[0]
    assert np.isfinite(wp3[..., 2]).all()
    want = R.reference_eval(oracle_mod, orc, vox, cols, wp3, pr.shape[0], D * A)
    for lim in (math.inf, 0.0, 0.1):
        got = V.reference_eval_v(oracle_mod, orc, vox, cols, wp3, _geo(ms), V.Vert(0.0, lim, lim),
                                 pr.shape[0], D * A)
        for k in want:
            _same_bits(got[k], want[k], f"{k} limit={lim}")
        assert not got["climb_sum"].any() and not np.signbit(got["climb_sum"]).any()
    assert (want["kin_sum"][np.isfinite(want["kin_sum"])] > 0).any()


# ---- an independent restatement in extended precision ------------------------------------------
def _longdouble_sums(wp3, geo, vert):
    """The four sums and the sums of their terms' magnitudes, whole arrays at once in
    np.longdouble (no loop over the segments; the reference loops and rounds to float64)."""
    ld = np.longdouble
    w = wp3.astype(ld)
    d = np.diff(w, axis=1)
    dx, dy, dz = d[..., 0], d[..., 1], d[..., 2] * ld(vert.z_scale)
    n = np.sqrt(dx * dx + dy * dy + dz * dz)                      # [P, N+1]
    N = n.shape[1] - 1
    lt = n * n if geo.length_smooth else n
    if geo.quirk_length:
        a = (w[:, 0, :2] - np.asarray(geo.anchor, ld)) if geo.anchor is not None else \
            np.zeros((w.shape[0], 2), ld)
        an = np.sqrt((a * a).sum(axis=1))
        lt = np.concatenate([(an * an if geo.length_smooth else an)[:, None], lt[:, :N]], axis=1)
    nk = n * n if geo.maxratio_smooth else n
    r = ld(geo.maxratio) ** (2 if geo.maxratio_smooth else 1)
    mincos = ld(math.cos(geo.maxalpha))
    pn, qn = nk[:, :-1], nk[:, 1:]
    dt = dx[:, :-1] * dx[:, 1:] + dy[:, :-1] * dy[:, 1:] + dz[:, :-1] * dz[:, 1:]
    ratio = dt / (pn * qn)
    rows = [np.maximum(0, qn - r * pn), np.maximum(0, pn / r - qn), np.maximum(0, mincos - ratio)]
    kmag = (qn + r * pn) + (pn / r + qn) + (abs(mincos) + np.abs(ratio))
    sc, sd = ld(vert.sin_climb), ld(vert.sin_descent)
    cu, cd = np.maximum(0, dz - sc * n), np.maximum(0, -dz - sd * n)
    cmag = (np.abs(dz) + sc * n) + (np.abs(dz) + sd * n)
    return {"length": (n.sum(axis=1), n.sum(axis=1)),
            "length_q": (lt.sum(axis=1), lt.sum(axis=1)),
            "kin_sum": (sum(rows).sum(axis=1), kmag.sum(axis=1)),
            "climb_sum": ((cu + cd).sum(axis=1), cmag.sum(axis=1))}


@pytest.mark.parametrize("ls,ms,quirk", [(False, False, False), (False, False, True),
                                         (True, True, True)])
def test_reference_agrees_with_an_extended_precision_restatement(oracle_mod, ls, ms, quirk):
    """|reference - restatement| <= (W + 4) 2^-53 sum|terms| for each of the four sums; the
    terms of a kinematic or climb row are the magnitudes the row is formed from (the row is
    their difference).  Finite limits, so that every row has a finite magnitude."""
    if np.finfo(np.longdouble).eps >= 2.0 ** -60:
        pytest.fail("np.longdouble is no wider than float64 here: the restatement would not "
                    "be independent")
    N, D = 9, 5
    W = N + 2
    pr, wp3, _ = _batch(oracle_mod, N, D)
    # finite paths without a zero-length segment (start == goal): a 0 / 0 row counts 0 in the
    # definition (fmax), which the whole-array restatement does not model
    ok = np.isfinite(wp3).all(axis=(1, 2))
    ok &= (np.abs(np.diff(wp3[..., :2], axis=1)).sum(axis=2) > 0).all(axis=1)
    wp3 = wp3[ok]
    assert wp3.shape[0] > 4000
    geo = _geo(ms, quirk_length=quirk, anchor=(3.0, -2.0) if quirk else None)
    geo.length_smooth = ls
    for zs in (1e-3, 1e-2):
        vert = V.Vert(zs, 0.1, 0.05)
        ref = V.geometry(wp3, geo, vert)
        for k, (val, mag) in _longdouble_sums(wp3, geo, vert).items():
            err = np.abs(ref[k].astype(np.longdouble) - val)
            bound = (W + 4) * np.longdouble(U) * mag
            worst = float((err / np.maximum(bound, np.finfo(np.float64).tiny)).max())
            print(f"z_scale={zs} {k}: largest error / bound = {worst:.3f}")
            assert (err <= bound).all(), (k, zs, worst)
        assert (ref["climb_sum"] > 0).any() and (ref["kin_sum"] > 0).any()


# ---- a closed form ----------------------------------------------------------------------------
@pytest.mark.parametrize("down", [False, True])
def test_straight_path_with_a_constant_climb(down):
    """N = 7: eight equal segments (0.75, 1.0) km with 3072 m of climb each at z_scale = 2^-10,
    i.e. (0.75, 1, 3) km: every segment's 3-D norm is 3.25 and every value is exact."""
    N, W, zs = 7, 9, 2.0 ** -10
    j = np.arange(W, dtype=np.float64)
    wp3 = np.stack([2.0 + 0.75 * j, -5.0 + 1.0 * j, 100.0 + 3072.0 * j], axis=1)[None]
    if down:
        wp3 = wp3[:, ::-1].copy()
    geo = V.Geo(quirk_length=False, maxratio=1.5, maxalpha=0.3)
    h, dzeta = math.hypot(0.75 * 8, 1.0 * 8), 3072.0 * 8 * zs
    closed = math.sqrt(h * h + dzeta * dzeta)
    assert closed == 26.0
    bound = (W + 4) * U * closed
    free = V.geometry(wp3, geo, V.Vert(zs))
    assert abs(free["length"][0] - closed) <= bound and abs(free["length_q"][0] - closed) <= bound
    assert free["climb_sum"][0] == 0.0 and free["kin_sum"][0] == 0.0   # straight, equal steps
    # sin of this climb is 3 / 3.25 = 0.923...: a limit above it charges nothing, one below
    # charges kappa |dz| - sin * length, summed by segments
    lim_hi, lim_lo = 0.95, 0.5
    other = math.inf
    for lim, want in ((lim_hi, 0.0), (lim_lo, 8 * (3.0 - lim_lo * 3.25))):
        vert = V.Vert(zs, other, lim) if down else V.Vert(zs, lim, other)
        got = V.geometry(wp3, geo, vert)["climb_sum"][0]
        assert abs(got - want) <= (W + 4) * U * 8 * (3.0 + lim * 3.25), (lim, got, want)
        # the limit of the other direction does not matter
        vert = V.Vert(zs, 0.0, lim) if down else V.Vert(zs, lim, 0.0)
        assert V.geometry(wp3, geo, vert)["climb_sum"][0] == got
    # z_scale = 0: the x/y length
    flat = V.geometry(wp3, geo, V.Vert(0.0, 0.0, 0.0))
    assert abs(flat["length"][0] - h) <= (W + 4) * U * h and flat["climb_sum"][0] == 0.0


# ---- the vertical terms take part in the selections ------------------------------------------------
def test_vertical_terms_change_the_selections(oracle_mod):
    """By the reference alone, on the hand volume, N = 9, D = 5 and the 8-profile family with the
    150 m cruise moved to profile 0, so that the straight climb is profile 1."""
    from uam_path_planning_amd import profiles as P

    N, D = 9, 5
    orc = _oracle(oracle_mod, N)
    vox, cols = R.hand_volume()
    pr, wp3, fam = _batch(oracle_mod, N, D, first=1)
    A, Q = fam.shape[0], pr.shape[0]
    assert np.array_equal(fam[1], P.linear(N)) and not np.array_equal(fam[0], P.linear(N))
    plain = R.reference_eval(oracle_mod, orc, vox, cols, wp3, Q, D * A)
    # x/y lengths: the first index wins, but for the rule's zero quirk (start == goal)
    quirk = (plain["length"].reshape(Q, D * A) == 0).any(axis=1)
    assert quirk.sum() == 1 and (plain["best_length_idx"][~quirk] % A == 0).all()
    changed = {}
    for zs in (1e-3, 1e-2):
        got = V.reference_eval_v(oracle_mod, orc, vox, cols, wp3, _geo(), V.Vert(zs), Q, D * A)
        n_len = int((got["best_length_idx"][~quirk] % A != 0).sum())
        changed[zs] = int((got["best_fval_idx"] != plain["best_fval_idx"]).sum())
        print(f"z_scale={zs}: best_length_idx is no multiple of A for {n_len} of {Q} pairs, "
              f"best_fval_idx differs from the uncharged selection for {changed[zs]}")
        assert n_len > 0
    # both scales change cost selections on this volume (printed above); the isotropic one is
    # the one asserted
    assert changed[1e-3] > 0, changed
