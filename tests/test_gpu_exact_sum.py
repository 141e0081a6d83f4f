"""UAM_OPT_EXACT_SUM: K2h's raster sums as exact integers ("K2hx+pack").  cost, nfz_sum and
best_fval_idx must not depend on the group length, the chunk, the terrain form, the sort key,
the batch size or the sharding; they must equal the definition (tests/exact_sum_ref.py: Python
integers and Fraction, fed with the raster words under the returned waypoint cells) bit for bit;
every other output must be K2h's; and against the default ordered sums they may differ by the
rounding of W float64 additions and divisions only.

Shape: a 100 x 76 raster (ragged against the 4 x 8, 4 x 4 and 8 x 8 blocks), N = 40 (W = 42),
D = 5, 300 pairs, some running partly off the raster.  rec is written by hand: whole 8 x 8
blocks of each pack code (all zero / phi only / psi >= 0 with no-fly flags / negative psi), phi
and psi spread over 2^+-20 in both signs, a finite random terrain."""
import ctypes
import math

import numpy as np
import pytest

import exact_sum_ref as X

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

N, W, D, Q = 40, 42, 5, 300
NX, NY = 100, 76
GROUPS = (4, 7, 11, 14, 21, 42, 64)
# every option a run depends on, set before each evaluation (the engine is shared)
DEFAULTS = dict(group=21, k2g_chunk=0, k2h_terrain=1, k2g_tile_bits=0, k2g_curve=1,
                sorted_min_paths=0, wave_max_paths=0, exact_sum=1)
EXACT = ("cost", "nfz_sum", "best_fval_idx")
OTHERS = ("length_q", "length", "kin_sum", "nfz_hits", "offmap", "min_clearance",
          "best_length_idx", "cells")


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype == np.float64 else a


def _same(a, b, what=""):
    np.testing.assert_array_equal(_bits(a), _bits(b), err_msg=what)


def _same_nan(got, want, what=""):
    """Bit equality of float64 arrays where any NaN equals any NaN."""
    n = np.isnan(want)
    np.testing.assert_array_equal(np.isnan(got), n, err_msg=what)
    _same(np.where(n, 0.0, got), np.where(n, 0.0, want), what)


def _engine(n=N):
    from uam_path_planning_amd import build
    from uam_path_planning_amd.engine import Engine, PathParams
    from uam_path_planning_amd.geometry import compile_map
    from uam_path_planning_amd.scenario import build_region_map, canonical_spec

    if not torch.cuda.is_available():
        pytest.fail("GPU tests need an MI355X")
    build.build_library()
    e = Engine(0)
    spec = canonical_spec(nfz_polygons=16)
    e.set_geometry(compile_map(build_region_map(spec)))

    def params(**kw):
        opts = dict(spec["options"])
        opts["maxratio_smooth"] = False
        opts.update(kw)
        return PathParams(N=n, **opts, maxratio=spec["maxratio"], maxalpha=spec["maxalpha"],
                          enlargement=spec["enlargement"], weights=tuple(spec["weights"]),
                          altitude=320.0)

    e.set_params(params())
    return e, params


def _hand_rec(rng):
    """[NY, NX, 4] uint32 records; kind [nby, nbx]: the pack code each 8 x 8 block must get."""
    nby, nbx = (NY + 7) // 8, (NX + 7) // 8
    kind = rng.integers(0, 4, (nby, nbx))
    kind[0, :4] = (0, 1, 2, 3)
    K = np.kron(kind, np.ones((8, 8), np.int64))[:NY, :NX]

    def mag():
        return (2.0 ** rng.uniform(-20.0, 20.0, (NY, NX)) *
                rng.choice([-1.0, 1.0], (NY, NX))).astype(np.float32)

    phi = np.where(K >= 1, mag(), np.float32(0.0)).astype(np.float32)
    psi = np.where(K == 2, np.abs(mag()), np.where(K == 3, mag(), np.float32(0.0)))
    psi = psi.astype(np.float32)
    # a kind-3 block holds a negative psi, whatever the signs drew
    neg = np.zeros((NY, NX), bool)
    neg[::8, ::8] = True
    psi = np.where((K == 3) & neg, -np.abs(psi), psi).astype(np.float32)
    flags = np.where((K == 2) & (rng.random((NY, NX)) < 0.3), 1, 0).astype(np.uint32)  # NFZ
    dem = np.where(K == 0, np.float32(0.0),
                   rng.uniform(-50.0, 900.0, (NY, NX)).astype(np.float32)).astype(np.float32)
    rec = np.stack([phi.view(np.uint32), psi.view(np.uint32), dem.view(np.uint32), flags], -1)
    return np.ascontiguousarray(rec), kind


def _upload(e, rec):
    from uam_path_planning_amd.engine import CostRaster, RasterGeo

    geo = RasterGeo(nx=NX, ny=NY, x0=0.0, y_top=20.0, dx=0.6, dy=0.75)
    r = CostRaster(geo, e.tensor(rec.view(np.int32), torch.int32))
    e.raster_summary(r, 0, packed=True)
    assert r.block == 8 and r.sum_scale is None
    return r


def _pack_codes(raster):
    nby, nbx = (NY + 7) // 8, (NX + 7) // 8
    nb = nby * nbx
    w = raster.packed.cpu().numpy().reshape(-1)[:((nb + 15) // 16) * 4].view(np.uint32)
    b = np.arange(nb)
    return ((w[b >> 4] >> ((b & 15) * 2).astype(np.uint32)) & 3).reshape(nby, nbx)


def _run(e, raster, pairs, ut, want_cells=False, **opts):
    o = dict(DEFAULTS)
    o.update(opts)
    for k, v in o.items():
        e.set_option(k, v)
    out = e.eval_generated(pairs, ut, raster=raster, want_cells=want_cells)
    return {k: v.cpu().numpy() for k, v in out.items()}


def _field_sums(rec, cells, col):
    """fl(S) of one field under every path's cells (-1: nothing), by the Python reference at the
    whole raster's exponent; also sum |v| per path."""
    ws = rec.reshape(-1, 4)[:, col].tolist()
    e = X.exponent(ws)
    out = np.empty(cells.shape[0], np.float64)
    mag = np.zeros(cells.shape[0], np.float64)
    vals = np.abs(rec.reshape(-1, 4)[:, col].copy().view(np.float32).astype(np.float64))
    for p, row in enumerate(cells.tolist()):
        pw = [ws[c] for c in row if c >= 0]
        S = sum(X.term(w, e) for w in pw if (w >> 23) & 255 != 255)
        out[p] = X.result(S, X.flags(pw), e)
        mag[p] = math.fsum(vals[c] for c in row if c >= 0)
    return out, e, mag


def _expected(e, rec, o):
    """cost, nfz_sum and best_fval_idx by the definition from a run's cells and length_q."""
    fphi, e_phi, _ = _field_sums(rec, o["cells"], 0)
    fpsi, e_psi, _ = _field_sums(rec, o["cells"], 1)
    with np.errstate(invalid="ignore"):
        cost = np.float64(N + 1) * o["length_q"] + fphi / np.float64(N)
    best = e.argmin(cost, D, True).cpu().numpy()
    return cost, fpsi, best, (e_phi, e_psi)


def _check_reference(e, rec, o):
    cost, nsum, best, _ = _expected(e, rec, o)
    _same_nan(o["cost"], cost, "cost")
    _same_nan(o["nfz_sum"], nsum, "nfz_sum")
    _same(o["best_fval_idx"], best, "best_fval_idx")


@pytest.fixture(scope="module")
def case():
    from uam_path_planning_amd.arcs import arc_table
    from uam_path_planning_amd.scenario import displacements

    e, params = _engine()
    rng = np.random.default_rng(23)
    rec, kind = _hand_rec(rng)
    raster = _upload(e, rec)
    np.testing.assert_array_equal(_pack_codes(raster), kind)   # all four pack codes, as meant
    assert set(kind.ravel().tolist()) == {0, 1, 2, 3}
    pairs = np.stack([rng.uniform(1.0, 59.0, Q), rng.uniform(-36.0, 19.0, Q),
                      rng.uniform(1.0, 59.0, Q), rng.uniform(-36.0, 19.0, Q)], 1)
    pairs[::7, 0] += 25.0    # starts east of the raster: paths partly off it
    ut = arc_table(N, displacements(D))
    base = _run(e, raster, pairs, ut, want_cells=True, group=7)   # the shared exact run
    assert e.last_kernel() == "K2hx+pack" and e.last_group() == 7
    off = base["offmap"]
    assert (off == 0).any() and ((off > 0) & (off < W)).any()
    return dict(e=e, params=params, rec=rec, raster=raster, pairs=pairs, ut=ut, base=base)


def test_independent_of_group_chunk_terrain_and_key(case):
    """cost, nfz_sum and best_fval_idx: one bit pattern over G x chunk x terrain form x tile
    bits x curve -- while the default sums of the same G values differ."""
    e, raster, pairs, ut, base = (case[k] for k in ("e", "raster", "pairs", "ut", "base"))
    costs = [_run(e, raster, pairs, ut, group=g, exact_sum=0)["cost"].view(np.uint64)
             for g in GROUPS]
    assert e.last_kernel() == "K2h+pack"
    distinct = (np.stack(costs) != costs[0]).any(axis=0)
    print(f"ordered sums: {distinct.sum()} of {distinct.size} paths differ across G")
    assert distinct.sum() * 2 >= distinct.size   # (else this test would pass vacuously)
    for g in GROUPS:
        for chunk in (6, 7, 8, 11):
            for te in (0, 1):
                for tb in (3, 6):
                    for curve in (0, 1):
                        o = _run(e, raster, pairs, ut, group=g, k2g_chunk=chunk,
                                 k2h_terrain=te, k2g_tile_bits=tb, k2g_curve=curve)
                        assert e.last_kernel() == "K2hx+pack" and e.last_group() == g
                        for k in EXACT:
                            _same(o[k], base[k], f"{k} G={g} chunk={chunk} te={te} "
                                                 f"tile_bits={tb} curve={curve}")


def test_equals_the_definition(case):
    """nfz_sum = fl(S_psi), cost = (N+1) length_q + fl(S_phi) / N, best_fval_idx = the selection
    rule on that cost: from the raster words under the returned cells."""
    _check_reference(case["e"], case["rec"], case["base"])
    assert np.isfinite(case["base"]["cost"]).all()


@pytest.mark.parametrize("terrain", [1, 0])
@pytest.mark.parametrize("group", [7, 4, 64])   # nseg 6 (<= 8), 11 (the loop), 1 (<= 4)
def test_other_outputs_are_k2h(case, group, terrain):
    """Everything but cost, nfz_sum and best_fval_idx: bit-identical to the option off."""
    e, raster, pairs, ut = (case[k] for k in ("e", "raster", "pairs", "ut"))
    on = _run(e, raster, pairs, ut, want_cells=True, group=group, k2h_terrain=terrain)
    off = _run(e, raster, pairs, ut, want_cells=True, group=group, k2h_terrain=terrain,
               exact_sum=0)
    assert e.last_kernel() == "K2h+pack"
    for k in OTHERS:
        _same(on[k], off[k], k)
    for k in EXACT:
        _same(on[k], case["base"][k], k)


def test_sharding_and_small_batches(case):
    """The whole batch at G = 7 against shards of 1 + 299 pairs at G = 11 and 150 + 150 at
    G = 21, at the library's default batch-size thresholds: the same bits, K2hx at every size."""
    e, raster, pairs, ut, base = (case[k] for k in ("e", "raster", "pairs", "ut", "base"))
    sizes = dict(sorted_min_paths=65536, wave_max_paths=16384)
    whole = _run(e, raster, pairs, ut, group=7, **sizes)
    assert e.last_kernel() == "K2hx+pack"
    for k in EXACT:
        _same(whole[k], base[k], k)
    for cut, g in ((1, 11), (150, 21)):
        parts = []
        for sl in (slice(0, cut), slice(cut, Q)):
            parts.append(_run(e, raster, pairs[sl], ut, group=g, **sizes))
            assert e.last_kernel() == "K2hx+pack" and e.last_group() == g
        for k in EXACT + ("length_q", "min_clearance", "best_length_idx"):
            _same(np.concatenate([p[k] for p in parts]), whole[k], f"{k} cut={cut}")


def test_non_finite_and_extreme_cells(case):
    """+inf, -inf, both, NaN (phi and psi) and a 2^-60 beside a 2^40 planted under known
    waypoints: IEEE's outcome as the reference states it; the scale words are the Python
    exponents and flags."""
    e, pairs, ut, base = (case[k] for k in ("e", "pairs", "ut", "base"))
    rec = case["rec"].copy()
    cells = base["cells"]
    # nine paths of different pairs, their waypoints 10 and 20 on 18 distinct cells
    pth, used = [], set()
    for p in range(0, Q * D, D):
        c10, c20 = int(cells[p, 10]), int(cells[p, 20])
        if min(c10, c20) >= 0 and c10 != c20 and not {c10, c20} & used:
            used |= {c10, c20}
            pth.append(p)
    pth = np.array(pth)[np.linspace(0, len(pth) - 1, 9).astype(int)]
    assert np.unique(pth).size == 9
    f32 = lambda v: int(np.array([v], np.float32).view(np.uint32)[0])
    inf, nan = float("inf"), float("nan")
    flat = rec.reshape(-1, 4)
    plant = [(0, 0, inf, None), (1, 0, -inf, None), (2, 0, inf, -inf), (3, 0, nan, None),
             (4, 1, inf, None), (5, 1, -inf, None), (6, 1, -inf, inf), (7, 1, nan, None),
             (8, 0, 2.0 ** 40, 2.0 ** -60)]
    for i, col, v10, v20 in plant:
        flat[cells[pth[i], 10], col] = f32(v10)
        if v20 is not None:
            flat[cells[pth[i], 20], col] = f32(v20)
    raster = _upload(e, rec)
    for g, te in ((7, 1), (21, 0)):
        o = _run(e, raster, pairs, ut, want_cells=True, group=g, k2h_terrain=te)
        _same(o["cells"], cells)
        _check_reference(e, rec, o)
        # every outcome occurs (which path shows which is the reference's business: paths
        # may cross each other's planted cells)
        for k in ("cost", "nfz_sum"):
            assert np.isposinf(o[k]).any() and np.isneginf(o[k]).any() and np.isnan(o[k]).any()
        c = o["cost"]
        assert (np.isfinite(c) & (np.abs(c) > 2.0 ** 33)).any()   # the 2^40 cell, finite
        assert np.isfinite(c).sum() > Q * D // 2
    _, _, _, (e_phi, e_psi) = _expected(e, rec, o)
    assert e_phi == 41
    fl = X.flags(flat[:, 0].tolist()) | (X.flags(flat[:, 1].tolist()) << 3)
    assert fl == 0o77
    assert raster.sum_scale.cpu().tolist() == [e_phi, e_psi, fl, 0]
    # the clean raster's words too
    sc = case["raster"].sum_scale.cpu().tolist()
    cf = case["rec"].reshape(-1, 4)
    assert sc == [X.exponent(cf[:, 0].tolist()), X.exponent(cf[:, 1].tolist()), 0, 0]


def test_close_to_the_ordered_sums():
    """A K1-built raster of the canonical map (R = 256): the exact and the default sums differ
    by at most the worst-case rounding of W ordered float64 additions and divisions,
    2 W 2^-53 (sum |phi_j| / N + (N+1) L) (nfz_sum: 2 W 2^-53 sum |psi_j|); the selection may
    differ only between candidates within that bound of each other."""
    from uam_path_planning_amd.arcs import arc_table
    from uam_path_planning_amd.scenario import displacements, raster_geo
    from uam_path_planning_amd.synthetic import random_pairs, synthetic_dem

    e, _ = _engine()
    raster = e.raster_build(raster_geo(256), synthetic_dem(256))
    rec = raster.rec.cpu().numpy().view(np.uint32)
    pairs, ut = random_pairs(Q, seed=4), arc_table(N, displacements(D))
    on = _run(e, raster, pairs, ut, want_cells=True)
    assert e.last_kernel() == "K2hx+pack"
    off = _run(e, raster, pairs, ut, want_cells=True, exact_sum=0)
    assert e.last_kernel() == "K2h+pack"
    assert np.isfinite(off["cost"]).all() and np.isfinite(on["cost"]).all()
    _, _, mphi = _field_sums(rec, on["cells"], 0)
    _, _, mpsi = _field_sums(rec, on["cells"], 1)
    u = 2.0 * W * 2.0 ** -53
    bc = u * (mphi / N + (N + 1) * np.abs(on["length_q"]))
    bn = u * mpsi
    dc, dn = np.abs(on["cost"] - off["cost"]), np.abs(on["nfz_sum"] - off["nfz_sum"])
    print(f"max |cost_on - cost_off| / bound = {np.max(dc / bc):.3g}, "
          f"nfz_sum: {np.max(dn / np.maximum(bn, 1e-300)):.3g}, "
          f"differing cost bits: {(dc > 0).sum()} of {dc.size}")
    assert (dc <= bc).all() and (dn <= bn).all()
    assert (mphi > 0).any() and (mpsi > 0).any()
    q = np.flatnonzero(on["best_fval_idx"] != off["best_fval_idx"])
    c, b = off["cost"].reshape(Q, D), bc.reshape(Q, D)
    for i in q:
        a, z = on["best_fval_idx"][i], off["best_fval_idx"][i]
        assert abs(c[i, a] - c[i, z]) <= b[i, a] + b[i, z]
    _check_reference(e, rec, on)


def test_errors_are_loud_and_leave_the_context_usable(case):
    """Never a silent fall-back to ordered sums: no scale -> UAM_E_STATE; a batch K2h does not
    take -> UAM_E_INVALID with its reason; each rejected on the host, and a valid call on the
    same context then gives the shared run's bits."""
    from uam_path_planning_amd import _lib

    e, raster, pairs, ut, base = (case[k] for k in ("e", "raster", "pairs", "ut", "base"))

    def valid():
        o = _run(e, raster, pairs, ut, group=7)
        assert e.last_kernel() == "K2hx+pack"
        for k in EXACT:
            _same(o[k], base[k], k)

    valid()
    # no scale: the C ABI directly (the engine would compute it)
    vp = lambda t: ctypes.c_void_p(t.data_ptr())
    pr, u = e.tensor(pairs, torch.float64), e.tensor(ut, torch.float64)
    _, s = e.outputs(Q * D, W, n_pairs=Q)
    assert e.lib.uam_set_sum_scale(e._ctx, None) == _lib.UAM_OK
    st = e.lib.uam_eval_generated(e._ctx, _lib.MODE_RASTER, ctypes.byref(raster.geo.as_struct()),
                                  vp(raster.rec), vp(raster.summary), raster.block,
                                  vp(raster.packed), vp(pr), Q, vp(u), D, ctypes.byref(s),
                                  e.stream)
    assert st == _lib.UAM_E_STATE and "scale" in _lib.last_error()
    valid()
    # no packed copy
    bare = type(raster)(raster.geo, raster.rec, raster.summary, raster.block, None)
    with pytest.raises(ValueError, match="packed"):
        _run(e, bare, pairs, ut, group=7)
    valid()
    e.set_params(case["params"](maxratio_smooth=True))
    with pytest.raises(ValueError, match="maxratio_smooth"):
        _run(e, raster, pairs, ut, group=7)
    e.set_params(case["params"]())
    valid()
    with pytest.raises(ValueError, match="UAM_OPT_GROUP"):
        _run(e, raster, pairs, ut, group=0)
    valid()
    with pytest.raises(ValueError, match="UAM_OPT_K2G_SIM"):
        _run(e, raster, pairs, ut, group=7, k2g_sim=0)
    e.set_option("k2g_sim", 1)
    valid()
    with pytest.raises(ValueError, match="not 0 or 1"):
        e.set_option("exact_sum", 2)
    assert e.get_option("exact_sum") == 1
    valid()
    e.synchronize()
