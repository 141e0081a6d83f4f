"""UAM_OPT_EXACT_SUM_VOLUME: K4h's voxel sums as exact integers ("K4hx+pack").  cost, nfz_sum
and best_fval_idx must not depend on the group length, the chunk, the terrain form, the sort
key (tiles, bands, curve), the batch size or the sharding; they must equal the definition
(tests/exact_sum_ref.py: Python integers and Fraction, fed with the voxel words at the oracle's
voxel index of every waypoint) bit for bit; every other output must be K4h's; and against the
default ordered sums they may differ by the rounding of W float64 additions and divisions only.

Shape: 100 x 76 columns (ragged against the 4 x 8, 4 x 2, 4 x 4 and 8 x 8 blocks) x 7 layers
(the last altitude band partial), N = 40 (W = 42), D = 5, 300 pairs, some starting below the
volume, ending above it or starting east of it, one with start == goal.  Voxels and columns are
written by hand through vol.vox / vol.cols: whole 8 x 8-column blocks of each pack code (all
zero / risk only / psi >= 0 with no-fly flags / negative psi), risk and psi spread over 2^+-20
in both signs, a finite random terrain."""
import ctypes
import math

import numpy as np
import pytest

import exact_sum_ref as X

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

N, W, D, Q = 40, 42, 5, 300
NX, NY, NZ = 100, 76, 7
X0, Y_TOP, DX, DY, Z0, DZ = 0.0, 20.0, 0.6, 0.75, 0.0, 640.0 / 7
GROUPS = (4, 7, 11, 14, 21, 42, 64)
# every option a run depends on, set before each evaluation (the engine is shared)
DEFAULTS = dict(group=21, k2g_chunk=0, k4h_terrain=0, k2g_tile_bits=0, k2g_curve=1, k4h_band=0,
                sorted_min_paths=0, wave_max_paths=0, exact_sum=0, exact_sum_volume=1)
EXACT = ("cost", "nfz_sum", "best_fval_idx")
OTHERS = ("length_q", "length", "kin_sum", "nfz_hits", "offmap", "min_clearance",
          "below_terrain", "best_length_idx")
ALL = EXACT + OTHERS


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


def _engine(oracle_mod, n=N):
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
    opts = dict(spec["options"])
    opts["maxratio_smooth"] = False
    orc = oracle_mod.Oracle(oracle_mod.compile_spec(spec), n, opts, spec["maxratio"],
                            spec["maxalpha"], spec["enlargement"], spec["weights"],
                            altitude=320.0)
    return e, params, orc


def _hand_volume(rng):
    """vox [NY, NX, NZ, 2] and cols [NY, NX, 2] uint32; kind [nby, nbx]: the pack code each
    8 x 8-column block must get."""
    nby, nbx = (NY + 7) // 8, (NX + 7) // 8
    kind = rng.integers(0, 4, (nby, nbx))
    kind[0, :4] = (0, 1, 2, 3)
    K2 = np.kron(kind, np.ones((8, 8), np.int64))[:NY, :NX]
    K = np.broadcast_to(K2[:, :, None], (NY, NX, NZ))

    def mag():
        return (2.0 ** rng.uniform(-20.0, 20.0, (NY, NX, NZ)) *
                rng.choice([-1.0, 1.0], (NY, NX, NZ))).astype(np.float32)

    risk = np.where(K >= 1, mag(), np.float32(0.0)).astype(np.float32)
    psi = np.where(K == 2, np.abs(mag()), np.where(K == 3, mag(), np.float32(0.0)))
    psi = psi.astype(np.float32)
    # a kind-3 block holds a negative psi, whatever the signs drew (one layer of one column)
    neg = np.zeros((NY, NX, NZ), bool)
    neg[::8, ::8, 3] = True
    psi = np.where((K == 3) & neg, -np.abs(psi), psi).astype(np.float32)
    flags = np.where((K2 == 2) & (rng.random((NY, NX)) < 0.3), 1, 0).astype(np.uint32)  # NFZ
    ter = np.where(K2 == 0, np.float32(0.0),
                   rng.uniform(-50.0, 900.0, (NY, NX)).astype(np.float32)).astype(np.float32)
    vox = np.stack([risk.view(np.uint32), psi.view(np.uint32)], -1)
    cols = np.stack([ter.view(np.uint32), flags], -1)
    return np.ascontiguousarray(vox), np.ascontiguousarray(cols), kind


def _geo(nx=NX, ny=NY, nz=NZ):
    from uam_path_planning_amd.engine import VolumeGeo

    return VolumeGeo(nx, ny, nz, X0, Y_TOP, DX, DY, Z0, DZ)


def _upload(e, vox, cols):
    """A fresh volume holding the given words, written through the views, and its packed copy."""
    vol = e.volume_alloc(_geo())
    vol.buf.zero_()
    vol.vox.copy_(e.tensor(vox.view(np.int32), torch.int32))
    vol.cols.copy_(e.tensor(cols.view(np.int32), torch.int32))
    e.volume_pack(vol)
    assert vol.sum_scale is None
    return vol


def _pack_codes(vol):
    nby, nbx = (NY + 7) // 8, (NX + 7) // 8
    nb = nby * nbx
    w = vol.packed.cpu().numpy().reshape(-1)[:((nb + 15) // 16) * 4].view(np.uint32)
    b = np.arange(nb)
    return ((w[b >> 4] >> ((b & 15) * 2).astype(np.uint32)) & 3).reshape(nby, nbx)


def _pairs(rng):
    """300 pairs over the grid, altered as test_gpu_k4h._pairs3d alters its own."""
    pr = np.stack([rng.uniform(1.0, 59.0, Q), rng.uniform(-36.0, 19.0, Q),
                   rng.uniform(100.0, 500.0, Q), rng.uniform(1.0, 59.0, Q),
                   rng.uniform(-36.0, 19.0, Q), rng.uniform(100.0, 500.0, Q)], 1)
    pr[::41, 2] = -50.0          # climbs in from below the volume
    pr[::43, 5] = 900.0          # leaves it at the top
    pr[::7, 0] += 25.0           # starts east of the grid
    pr[11, 3:5] = pr[11, 0:2]    # start == goal (h = 0)
    return pr


def _run(e, vol, pairs, ut, keys=ALL, **opts):
    o = dict(DEFAULTS)
    o.update(opts)
    for k, v in o.items():
        e.set_option(k, v)
    out = e.eval_generated3d(pairs, ut, vol)
    return {k: out[k].cpu().numpy() for k in keys}


def _oracle(oracle_mod, orc, vox, cols, pairs, ut, group=0, geo=None):
    g = geo or _geo()
    vd = oracle_mod.volume_desc(g.nx, g.ny, g.nz, g.x0, g.y_top, g.dx, g.dy, g.z0, g.dz)
    host = (vox.view(np.float32), cols.view(np.float32))
    return orc.eval_generated_h(pairs, ut, mode="volume", vdesc=vd, vol=host, group=group,
                                want_cells=True)


def _field_sums(vox, cells, col):
    """fl(S) of one field at every path's voxel indices (-1: nothing), by the Python reference
    at the whole volume's exponent; also sum |v| per path."""
    ws = vox.reshape(-1, 2)[:, col].tolist()
    e = X.exponent(ws)
    out = np.empty(cells.shape[0], np.float64)
    mag = np.zeros(cells.shape[0], np.float64)
    vals = np.abs(vox.reshape(-1, 2)[:, col].copy().view(np.float32).astype(np.float64))
    for p, row in enumerate(cells.tolist()):
        pw = [ws[c] for c in row if c >= 0]
        S = sum(X.term(w, e) for w in pw if (w >> 23) & 255 != 255)
        out[p] = X.result(S, X.flags(pw), e)
        mag[p] = math.fsum(vals[c] for c in row if c >= 0)
    return out, e, mag


def _expected(e, vox, cells, o):
    """cost, nfz_sum and best_fval_idx by the definition from the oracle's voxel indices and a
    run's length_q."""
    frisk, e_risk, _ = _field_sums(vox, cells, 0)
    fpsi, e_psi, _ = _field_sums(vox, cells, 1)
    with np.errstate(invalid="ignore"):
        cost = np.float64(N + 1) * o["length_q"] + frisk / np.float64(N)
    best = e.argmin(cost, D, True).cpu().numpy()
    return cost, fpsi, best, (e_risk, e_psi)


def _check_reference(e, vox, cells, o):
    # the oracle's voxel indices are the kernel's: as many -1 as off-volume waypoints
    _same((cells < 0).sum(axis=1).astype(np.int32), o["offmap"], "offmap against the cells")
    cost, nsum, best, _ = _expected(e, vox, cells, o)
    _same_nan(o["cost"], cost, "cost")
    _same_nan(o["nfz_sum"], nsum, "nfz_sum")
    _same(o["best_fval_idx"], best, "best_fval_idx")


@pytest.fixture(scope="module")
def case(oracle_mod):
    from uam_path_planning_amd.arcs import arc_table
    from uam_path_planning_amd.scenario import displacements

    e, params, orc = _engine(oracle_mod)
    rng = np.random.default_rng(24)
    vox, cols, kind = _hand_volume(rng)
    vol = _upload(e, vox, cols)
    np.testing.assert_array_equal(_pack_codes(vol), kind)   # all four pack codes, as meant
    assert set(kind.ravel().tolist()) == {0, 1, 2, 3}
    pairs = _pairs(rng)
    ut = arc_table(N, displacements(D))
    ref = _oracle(oracle_mod, orc, vox, cols, pairs, ut, group=7)
    base = _run(e, vol, pairs, ut, group=7)   # the shared exact run
    assert e.last_kernel() == "K4hx+pack" and e.last_group() == 7
    off = base["offmap"]
    assert (off == 0).any() and ((off > 0) & (off < W)).any()
    assert (base["below_terrain"] > 0).any()
    return dict(e=e, params=params, orc=orc, O=oracle_mod, vox=vox, cols=cols, vol=vol,
                pairs=pairs, ut=ut, base=base, cells=ref["cells"])


def test_equals_the_definition(case):
    """nfz_sum = fl(S_psi), cost = (N+1) length_q + fl(S_risk) / N, best_fval_idx = the
    selection rule on that cost: from the voxel words at the oracle's voxel indices."""
    _check_reference(case["e"], case["vox"], case["cells"], case["base"])
    assert np.isfinite(case["base"]["cost"]).all()


def test_independent_of_group_chunk_terrain_and_key(case):
    """cost, nfz_sum and best_fval_idx: one bit pattern over G x chunk x terrain form x tile
    bits x band x curve -- while the default sums of the same G values differ (the oracle's
    grouped sums first: a condition on the drawn volume, then K4h's own)."""
    e, vol, pairs, ut, base = (case[k] for k in ("e", "vol", "pairs", "ut", "base"))
    oc = [_oracle(case["O"], case["orc"], case["vox"], case["cols"], pairs, ut,
                  group=g)["cost"].view(np.uint64) for g in GROUPS]
    odistinct = (np.stack(oc) != oc[0]).any(axis=0)
    print(f"oracle's ordered sums: {odistinct.sum()} of {odistinct.size} paths differ across G")
    assert odistinct.sum() * 2 >= odistinct.size   # (else this test would pass vacuously)
    costs = []
    for g in GROUPS:
        costs.append(_run(e, vol, pairs, ut, ("cost",), group=g,
                          exact_sum_volume=0)["cost"].view(np.uint64))
        assert e.last_kernel() == "K4h+pack"
    distinct = (np.stack(costs) != costs[0]).any(axis=0)
    print(f"ordered sums: {distinct.sum()} of {distinct.size} paths differ across G")
    assert distinct.sum() * 2 >= distinct.size
    for g in GROUPS:
        for chunk in (6, 7, 8, 11, 16):
            for te in (0, 1):
                for tb in (3, 6):
                    for band in (0, 1, 2):
                        for curve in (0, 1):
                            o = _run(e, vol, pairs, ut, EXACT, group=g, k2g_chunk=chunk,
                                     k4h_terrain=te, k2g_tile_bits=tb, k4h_band=band,
                                     k2g_curve=curve)
                            assert e.last_kernel() == "K4hx+pack" and e.last_group() == g
                            for k in EXACT:
                                _same(o[k], base[k], f"{k} G={g} chunk={chunk} te={te} "
                                                     f"tile_bits={tb} band={band} curve={curve}")


@pytest.mark.parametrize("terrain", [1, 0])
@pytest.mark.parametrize("group", [7, 4, 64])   # nseg 6, 11 and 1
def test_other_outputs_are_k4h(case, group, terrain):
    """Everything but cost, nfz_sum and best_fval_idx: bit-identical to the option off."""
    e, vol, pairs, ut = (case[k] for k in ("e", "vol", "pairs", "ut"))
    on = _run(e, vol, pairs, ut, group=group, k4h_terrain=terrain)
    assert e.last_kernel() == "K4hx+pack"
    off = _run(e, vol, pairs, ut, group=group, k4h_terrain=terrain, exact_sum_volume=0)
    assert e.last_kernel() == "K4h+pack"
    for k in OTHERS:
        _same(on[k], off[k], k)
    for k in EXACT:
        _same(on[k], case["base"][k], k)


def test_sharding_and_small_batches(case):
    """The whole batch at G = 7 against shards of 1 + 299 pairs at G = 11 and 150 + 150 at
    G = 21, at the library's default batch-size thresholds: the same bits, K4hx at every size."""
    e, vol, pairs, ut, base = (case[k] for k in ("e", "vol", "pairs", "ut", "base"))
    sizes = dict(sorted_min_paths=65536, wave_max_paths=16384)
    whole = _run(e, vol, pairs, ut, group=7, **sizes)
    assert e.last_kernel() == "K4hx+pack"
    for k in EXACT:
        _same(whole[k], base[k], k)
    for cut, g in ((1, 11), (150, 21)):
        parts = []
        for sl in (slice(0, cut), slice(cut, Q)):
            parts.append(_run(e, vol, pairs[sl], ut, group=g, **sizes))
            assert e.last_kernel() == "K4hx+pack" and e.last_group() == g
        for k in EXACT + ("min_clearance", "below_terrain", "best_length_idx"):
            _same(np.concatenate([p[k] for p in parts]), whole[k], f"{k} cut={cut}")


def test_non_finite_and_extreme_voxels(case):
    """+inf, -inf, both, NaN (risk and psi) and a 2^-60 beside a 2^40 planted under known
    waypoints by writes through vol.vox: IEEE's outcome as the reference states it; the writes
    alone make the evaluation repack and rescale; the scale words are the Python exponents and
    flags."""
    e, pairs, ut, cells = (case[k] for k in ("e", "pairs", "ut", "cells"))
    vox = case["vox"].copy()
    vol = _upload(e, vox, case["cols"])
    o = _run(e, vol, pairs, ut, group=7)
    for k in EXACT:
        _same(o[k], case["base"][k], k)
    clean_scale, old_packed = vol.sum_scale, vol.packed
    cf = vox.reshape(-1, 2)
    assert clean_scale.cpu().tolist() == [X.exponent(cf[:, 0].tolist()),
                                          X.exponent(cf[:, 1].tolist()), 0, 0]
    # nine paths of different pairs, their waypoints 10 and 20 on 18 distinct voxels
    pth, used = [], set()
    for p in range(0, Q * D, D):
        c10, c20 = int(cells[p, 10]), int(cells[p, 20])
        if min(c10, c20) >= 0 and c10 != c20 and not {c10, c20} & used:
            used |= {c10, c20}
            pth.append(p)
    pth = np.array(pth)[np.linspace(0, len(pth) - 1, 9).astype(int)]
    assert np.unique(pth).size == 9
    f32 = lambda v: int(np.array([v], np.float32).view(np.int32)[0])
    inf, nan = float("inf"), float("nan")
    plant = [(0, 0, inf, None), (1, 0, -inf, None), (2, 0, inf, -inf), (3, 0, nan, None),
             (4, 1, inf, None), (5, 1, -inf, None), (6, 1, -inf, inf), (7, 1, nan, None),
             (8, 0, 2.0 ** 40, 2.0 ** -60)]
    flat_dev = vol.vox.view(-1, 2)     # a view of vol.buf: the writes move its version counter
    for i, col, v10, v20 in plant:
        for c, v in ((cells[pth[i], 10], v10), (cells[pth[i], 20], v20)):
            if v is not None:
                flat_dev[int(c), col] = f32(v)
                cf[int(c), col] = np.array([v], np.float32).view(np.uint32)[0]
    for g, te in ((7, 1), (21, 0)):
        o = _run(e, vol, pairs, ut, group=g, k4h_terrain=te)
        assert e.last_kernel() == "K4hx+pack"
        assert vol.packed is not old_packed and vol.sum_scale is not clean_scale
        _check_reference(e, vox, cells, o)
        # every outcome occurs (which path shows which is the reference's business: paths
        # may cross each other's planted voxels)
        for k in ("cost", "nfz_sum"):
            assert np.isposinf(o[k]).any() and np.isneginf(o[k]).any() and np.isnan(o[k]).any()
        c = o["cost"]
        assert (np.isfinite(c) & (np.abs(c) > 2.0 ** 33)).any()   # the 2^40 voxel, finite
        assert np.isfinite(c).sum() > Q * D // 2
    _, _, _, (e_risk, e_psi) = _expected(e, vox, cells, o)
    assert e_risk == 41
    fl = X.flags(cf[:, 0].tolist()) | (X.flags(cf[:, 1].tolist()) << 3)
    assert fl == 0o77
    assert vol.sum_scale.cpu().tolist() == [e_risk, e_psi, fl, 0]
    np.testing.assert_array_equal(vol.vox.cpu().numpy().view(np.uint32), vox)


def test_close_to_the_ordered_sums(oracle_mod):
    """A volume built from a K1 raster of the canonical map (R = 256, 16 layers): the exact and
    the default sums differ by at most the worst-case rounding of W ordered float64 additions
    and divisions, 2 W 2^-53 (sum |risk_j| / N + (N+1) |L|) (nfz_sum: 2 W 2^-53 sum |psi_j|);
    the selection may differ only between candidates within that bound of each other."""
    from uam_path_planning_amd.arcs import arc_table
    from uam_path_planning_amd.scenario import displacements, layer_weights, raster_geo
    from uam_path_planning_amd.synthetic import random_pairs3d, synthetic_dem

    e, _, orc = _engine(oracle_mod)
    R, nz = 256, 16
    g2 = raster_geo(R)
    vol = e.volume_build(e.raster_build(g2, synthetic_dem(R)), nz, 0.0, 640.0 / nz,
                         layer_weights(nz))
    e.volume_pack(vol)
    vox = vol.vox.cpu().numpy().view(np.uint32)
    cols = vol.cols.cpu().numpy().view(np.uint32)
    pairs, ut = random_pairs3d(Q, seed=4), arc_table(N, displacements(D))
    on = _run(e, vol, pairs, ut)
    assert e.last_kernel() == "K4hx+pack"
    off = _run(e, vol, pairs, ut, exact_sum_volume=0)
    assert e.last_kernel() == "K4h+pack"
    assert np.isfinite(off["cost"]).all() and np.isfinite(on["cost"]).all()
    cells = _oracle(oracle_mod, orc, vox, cols, pairs, ut, group=21, geo=vol.geo)["cells"]
    _, _, mrisk = _field_sums(vox, cells, 0)
    _, _, mpsi = _field_sums(vox, cells, 1)
    u = 2.0 * W * 2.0 ** -53
    bc = u * (mrisk / N + (N + 1) * np.abs(on["length_q"]))
    bn = u * mpsi
    dc, dn = np.abs(on["cost"] - off["cost"]), np.abs(on["nfz_sum"] - off["nfz_sum"])
    print(f"max |cost_on - cost_off| / bound = {np.max(dc / bc):.3g}, "
          f"nfz_sum: {np.max(dn / np.maximum(bn, 1e-300)):.3g}, "
          f"differing cost bits: {(dc > 0).sum()} of {dc.size}")
    assert (dc <= bc).all() and (dn <= bn).all()
    assert (mrisk > 0).any() and (mpsi > 0).any()
    q = np.flatnonzero(on["best_fval_idx"] != off["best_fval_idx"])
    c, b = off["cost"].reshape(Q, D), bc.reshape(Q, D)
    for i in q:
        a, z = on["best_fval_idx"][i], off["best_fval_idx"][i]
        assert abs(c[i, a] - c[i, z]) <= b[i, a] + b[i, z]
    _check_reference(e, vox, cells, on)


def test_errors_are_loud_and_leave_the_context_usable(case):
    """Never a silent fall-back to K4 / K4w or to ordered sums: no scale -> UAM_E_STATE; a batch
    K4h does not take -> UAM_E_INVALID with its reason; each rejected on the host, and a valid
    call on the same context then gives the shared run's bits.  UAM_OPT_EXACT_SUM leaves the
    volume alone."""
    from uam_path_planning_amd import _lib

    e, vol, pairs, ut, base = (case[k] for k in ("e", "vol", "pairs", "ut", "base"))

    def valid():
        o = _run(e, vol, pairs, ut, group=7)
        assert e.last_kernel() == "K4hx+pack"
        for k in EXACT:
            _same(o[k], base[k], k)

    valid()
    # no scale: the C ABI directly (the engine would compute it)
    vp = lambda t: ctypes.c_void_p(t.data_ptr())
    pr, u = e.tensor(pairs, torch.float64), e.tensor(ut, torch.float64)
    _, s = e.outputs(Q * D, W, n_pairs=Q)
    assert e.lib.uam_set_volume_sum_scale(e._ctx, None) == _lib.UAM_OK
    st = e.lib.uam_eval_generated3d(e._ctx, ctypes.byref(vol.geo.as_struct()), vp(vol.buf),
                                    vp(vol.packed), vp(pr), Q, vp(u), D, ctypes.byref(s),
                                    e.stream)
    assert st == _lib.UAM_E_STATE and "scale" in _lib.last_error()
    valid()
    # no packed copy
    bare = type(vol)(vol.geo, vol.buf, vol.vox, vol.cols, vol.cbits)
    with pytest.raises(ValueError, match="packed"):
        _run(e, bare, pairs, ut, group=7)
    valid()
    e.set_params(case["params"](maxratio_smooth=True))
    with pytest.raises(ValueError, match="maxratio_smooth"):
        _run(e, vol, pairs, ut, group=7)
    e.set_params(case["params"]())
    valid()
    with pytest.raises(ValueError, match="UAM_OPT_GROUP"):
        _run(e, vol, pairs, ut, group=0)
    valid()
    with pytest.raises(ValueError, match="UAM_OPT_K2G_SIM"):
        _run(e, vol, pairs, ut, group=7, k2g_sim=0)
    e.set_option("k2g_sim", 1)
    valid()
    with pytest.raises(ValueError, match="not 0 or 1"):
        e.set_option("exact_sum_volume", 2)
    assert e.get_option("exact_sum_volume") == 1
    valid()
    # the raster's option leaves the volume alone: K4h's ordered bits
    ordered = _run(e, vol, pairs, ut, group=7, exact_sum_volume=0)
    with_raster_option = _run(e, vol, pairs, ut, group=7, exact_sum_volume=0, exact_sum=1)
    assert e.last_kernel() == "K4h+pack"
    for k in ALL:
        _same(with_raster_option[k], ordered[k], k)
    valid()
    e.synchronize()
