"""The sorted forms' item order: K2h and K4h (and their exact forms) sort the (path, group) items
on ONE bin per tile (per tile and altitude band), so a wave freely mixes full groups with the
ragged last one; K2g keeps the last groups' bins of their own.  The order only decides which
lane evaluates an item: every output and both selections must equal the oracle's statement
(orc_eval_generated_h; orc_eval_paths_g for K2g) bit for bit, and the exact sums their
definition (tests/exact_sum_ref.py).

Shapes: the canonical map's 256^2 raster and its 256^2 x 16 volume; N = 80 (W = 82 = 21 + 21 +
21 + 19) and N = 82 (W = 84 = 4 x 21); G = 21, 64 (> W: one group a path, and it is the last),
1, 5 (chunks of 6 and 16), and 16 / 12 with chunks of 7 / 11, where a full group takes more
chunks than the ragged one (3 against 1, 2 against 1); D = 1 and 5; batches of under one to 40
workgroups of 256 items, with and without a partial last workgroup; pair sets whose items all
fall into one bin (every pair off the grid or NaN; every pair inside one tile); two different
batches back to back on one context (every test shares one context per N, too)."""
import numpy as np
import pytest

import exact_sum_ref as X

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

R, NZ = 256, 16
# every option a run depends on, set before each evaluation (the engines are shared)
DEFAULTS = dict(group=21, k2g_chunk=0, k2g_tile_bits=0, sorted_min_paths=0, wave_max_paths=0,
                exact_sum=0, exact_sum_volume=0, test_sort_fault=0)
KEYS = (("cost", "cost"), ("length_q", "lq"), ("length", "length"), ("kin_sum", "kin"),
        ("nfz_sum", "nfz"), ("nfz_hits", "nfz_hits"), ("offmap", "offmap"),
        ("min_clearance", "min_clearance"))
EXACT = ("cost", "nfz_sum", "best_fval_idx")
# (group, N, chunk)
CASES = [(21, 80, 0), (21, 82, 0), (64, 80, 0), (1, 80, 0), (5, 80, 6), (5, 80, 16),
         (16, 80, 7), (12, 80, 11)]
_WORLDS = {}


def _world(oracle_mod, N, maxratio_smooth=False):
    """One context per (N, maxratio_smooth) with the 256^2 raster, its packed copy, the
    256^2 x 16 volume and the oracle; built once and left unchanged."""
    key = (N, maxratio_smooth)
    if key in _WORLDS:
        return _WORLDS[key]
    from uam_path_planning_amd import build
    from uam_path_planning_amd.engine import Engine, PathParams
    from uam_path_planning_amd.geometry import compile_map
    from uam_path_planning_amd.scenario import (build_region_map, canonical_spec, layer_weights,
                                                raster_geo)
    from uam_path_planning_amd.synthetic import synthetic_dem

    if not torch.cuda.is_available():
        pytest.fail("GPU tests need an MI355X")
    build.build_library()
    e = Engine(0)
    spec = canonical_spec(nfz_polygons=16)
    opts = dict(spec["options"])
    opts["maxratio_smooth"] = maxratio_smooth
    e.set_geometry(compile_map(build_region_map(spec)))
    e.set_params(PathParams(N=N, **opts, maxratio=spec["maxratio"], maxalpha=0.015,
                            enlargement=spec["enlargement"], weights=tuple(spec["weights"]),
                            altitude=320.0))
    orc = oracle_mod.Oracle(oracle_mod.compile_spec(spec), N, opts, spec["maxratio"], 0.015,
                            spec["enlargement"], spec["weights"], altitude=320.0)
    geo = raster_geo(R)
    raster = e.raster_build(geo, synthetic_dem(R), summary=False)
    e.raster_summary(raster, 0, packed=True)
    rd = oracle_mod.Oracle.raster_desc(geo.nx, geo.ny, geo.x0, geo.y_top, geo.dx, geo.dy,
                                       geo.nodata, geo.dem_threshold)
    w = dict(e=e, orc=orc, O=oracle_mod, N=N, geo=geo, raster=raster, rd=rd,
             rec=raster.rec.cpu().numpy().view(np.float32))
    if not maxratio_smooth:
        vol = e.volume_build(raster, NZ, 0.0, 640.0 / NZ, layer_weights(NZ))
        e.volume_pack(vol)
        w["vol"] = vol
        w["vd"] = oracle_mod.volume_desc(R, R, NZ, geo.x0, geo.y_top, geo.dx, geo.dy, 0.0,
                                         640.0 / NZ)
        w["vox"] = vol.vox.cpu().numpy().view(np.uint32)
        w["host"] = (w["vox"].view(np.float32), vol.cols.cpu().numpy().view(np.float32))
    _WORLDS[key] = w
    return w


def _ut(N, D):
    from uam_path_planning_amd.arcs import arc_table
    from uam_path_planning_amd.scenario import displacements

    return arc_table(N, displacements(D) if D > 1 else np.array([0.3]))


def _pairs(n, seed, form="k2h"):
    """n random pairs (with altitudes for K4h); some off the grid, one NaN, one of length 0."""
    from uam_path_planning_amd.synthetic import random_pairs, random_pairs3d

    pr = random_pairs(n, seed=seed) if form != "k4h" else random_pairs3d(n, seed=seed)
    g = 2 if form != "k4h" else 3    # the goal's first column
    pr[::13, 0] += 70.0              # off the grid
    if n > 5:
        pr[5, 1] = np.nan
    if n > 11:
        pr[11, g:g + 2] = pr[11, 0:2]    # start == goal (h = 0)
    if form == "k4h":
        pr[::41, 2] = -50.0          # climbs in from below the volume
        pr[::43, 5] = 900.0          # leaves it at the top
    return pr


def _n_pairs(items, G, N, D):
    """Pairs for about `items` (path, group) items, never a multiple of 256 of them."""
    per = D * -(-(N + 2) // G)
    n = max(1, items // per)
    return n + 1 if (n * per) % 256 == 0 else n


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype == np.float64 else a


def _same_nan(got, want, what):
    """Bit equality of float64 arrays where any NaN equals any NaN."""
    n = np.isnan(want)
    np.testing.assert_array_equal(np.isnan(got), n, err_msg=what)
    np.testing.assert_array_equal(_bits(np.where(n, 0.0, got)), _bits(np.where(n, 0.0, want)),
                                  err_msg=what)


def _field_sum(words, e, cells):
    """fl(S) of one field's words at every path's cells (-1: nothing), at exponent e."""
    out = np.empty(cells.shape[0], np.float64)
    for p, row in enumerate(cells.tolist()):
        pw = [words[c] for c in row if c >= 0]
        S = sum(X.term(v, e) for v in pw if (v >> 23) & 255 != 255)
        out[p] = X.result(S, X.flags(pw), e)
    return out


def _exact_fields(w, form):
    """The two summed fields' words and exponents, once per world and form."""
    k = "xf_" + form
    if k not in w:
        src = (w["rec"].view(np.uint32).reshape(-1, 4) if form == "k2h"
               else w["vox"].reshape(-1, 2))
        cols = [src[:, c].tolist() for c in (0, 1)]
        w[k] = [(ws, X.exponent(ws)) for ws in cols]
    return w[k]


def _run_and_check(w, form, pairs, D, group, chunk=0, exact=False, **opts):
    """One batch through K2h / K4h (exact: K2hx / K4hx) against the oracle, every output and
    both selections bit for bit; the exact sums against their definition."""
    e, orc, O, N = w["e"], w["orc"], w["O"], w["N"]
    ut = _ut(N, D)
    o = dict(DEFAULTS, group=group, k2g_chunk=chunk, **opts)
    o["exact_sum" if form == "k2h" else "exact_sum_volume"] = int(exact)
    for k, v in o.items():
        e.set_option(k, v)
    if form == "k2h":
        ref = orc.eval_generated_h(pairs, ut, rdesc=w["rd"], rec=w["rec"], group=group,
                                   want_cells=True)
        gpu = e.eval_generated(pairs, ut, raster=w["raster"])
        keys = KEYS
    else:
        ref = orc.eval_generated_h(pairs, ut, mode="volume", vdesc=w["vd"], vol=w["host"],
                                   group=group, want_cells=True)
        gpu = e.eval_generated3d(pairs, ut, w["vol"])
        keys = KEYS + (("below_terrain", "below"),)
    want = ("K2h" if form == "k2h" else "K4h") + ("x" if exact else "") + "+pack"
    assert e.last_kernel() == want and e.last_group() == group
    g = {k: v.cpu().numpy() for k, v in gpu.items()}
    if exact:   # cost, nfz_sum and the selection on cost by the definition
        (wc, ec), (wn, en) = _exact_fields(w, form)
        cells = ref["cells"].reshape(-1, N + 2)
        with np.errstate(invalid="ignore"):
            cost = np.float64(N + 1) * g["length_q"] + _field_sum(wc, ec, cells) / np.float64(N)
        _same_nan(g["cost"], cost, "cost")
        _same_nan(g["nfz_sum"], _field_sum(wn, en, cells), "nfz_sum")
        np.testing.assert_array_equal(g["best_fval_idx"], e.argmin(cost, D, True).cpu().numpy())
        keys = tuple(k for k in keys if k[0] not in EXACT)
    else:
        np.testing.assert_array_equal(g["best_fval_idx"], O.argmin(ref["cost"], D, True))
    for gk, ok in keys:
        np.testing.assert_array_equal(g[gk], ref[ok], err_msg=gk)
    np.testing.assert_array_equal(g["best_length_idx"], O.argmin(ref["length"], D, False))
    return ref


FORMS = [("k2h", False), ("k2h", True), ("k4h", False)]


@pytest.mark.parametrize("form,exact", FORMS)
@pytest.mark.parametrize("D", [1, 5])
@pytest.mark.parametrize("group,N,chunk", CASES)
def test_group_lengths_mixed_in_a_wave(oracle_mod, group, N, chunk, D, form, exact):
    """About 10 workgroups of items with a partial last one; W = 82 at G = 21, 5, 16, 12 has a
    ragged last group whose items now share their tile's bin with the full groups'."""
    w = _world(oracle_mod, N)
    pairs = _pairs(_n_pairs(2500, group, N, D), 100 + group + D, form)
    _run_and_check(w, form, pairs, D, group, chunk, exact)


# (D, pairs, workgroups of 256 items) at G = 21, N = 80: 4 items a path
BATCHES = [(5, 3, 1), (5, 30, 3), (5, 100, 8), (1, 512, 8), (5, 509, 40), (5, 512, 40)]


@pytest.mark.parametrize("form,exact", FORMS + [("k4h", True)])
@pytest.mark.parametrize("D,n,chunks", BATCHES)
def test_batch_sizes(oracle_mod, D, n, chunks, form, exact):
    """Fewer workgroups than XCDs (empty ranges), exactly 8 (2000 items and 2048), 40 with and
    without a partial last workgroup."""
    w = _world(oracle_mod, 80)
    assert -(-n * D * 4 // 256) == chunks
    _run_and_check(w, form, _pairs(n, 7 * n + D, form), D, 21, exact=exact)


@pytest.mark.parametrize("form,exact", FORMS)
def test_single_bin(oracle_mod, form, exact):
    """Every pair off the grid or NaN (all items in the last bin), then every pair inside one
    tile of the 8 x 8 (all items in that tile's bin)."""
    w = _world(oracle_mod, 80)
    D = 5
    off = _pairs(200, 31, form)
    off[:, 0] += 200.0
    off[:, 2 if form == "k2h" else 3] += 200.0
    off[::3] = np.nan
    ref = _run_and_check(w, form, off, D, 21, exact=exact)
    ok = ~np.isnan(ref["cost"])
    assert (ref["offmap"][ok] == 82).all() and ok.any()
    rng = np.random.default_rng(5)
    geo = w["geo"]
    side = 32 * geo.dx   # a tile of 32 x 32 cells; tile (3, 3)'s centre +- 1/8 of its side
    cx, cy = geo.x0 + 3.5 * side, geo.y_top - 3.5 * side
    one = np.stack([cx + rng.uniform(-1, 1, 200) * side / 8, cy + rng.uniform(-1, 1, 200) * side / 8,
                    cx + rng.uniform(-1, 1, 200) * side / 8, cy + rng.uniform(-1, 1, 200) * side / 8],
                   1)
    if form == "k4h":   # one layer of 40 m too
        one = np.stack([one[:, 0], one[:, 1], rng.uniform(290.0, 310.0, 200), one[:, 2],
                        one[:, 3], rng.uniform(290.0, 310.0, 200)], 1)
    ref = _run_and_check(w, form, one, D, 21, exact=exact)
    if form == "k2h":
        c = ref["cells"]
        assert (c >= 0).all() and ((c % R) // 32 == 3).all() and ((c // R) // 32 == 3).all()
    else:
        assert (ref["offmap"] == 0).all()


@pytest.mark.parametrize("form,exact", FORMS + [("k4h", True)])
def test_two_batches_back_to_back(oracle_mod, form, exact):
    """A 40-workgroup batch, then a different 8-workgroup one, then the first again on the same
    context: slots, keys or counts left by the one before would show."""
    w = _world(oracle_mod, 80)
    a, b = _pairs(509, 61, form), _pairs(100, 62, form)
    for pairs in (a, b, a):
        _run_and_check(w, form, pairs, 5, 21, exact=exact)


@pytest.mark.parametrize("tile_bits", [3, 6])
@pytest.mark.parametrize("form,exact", FORMS)
def test_tile_bits(oracle_mod, form, exact, tile_bits):
    """Coarse and the finest tiles (UAM_OPT_K2G_TILE_BITS): the bins only move items."""
    w = _world(oracle_mod, 80)
    _run_and_check(w, form, _pairs(300, 71, form), 5, 21, exact=exact, k2g_tile_bits=tile_bits)


def test_maxratio_smooth_runs_k2g_with_ragged_bins(oracle_mod):
    """maxratio_smooth: the batch runs K2g, whose key keeps the ragged last group's bins
    (W = 82 at G = 21), and equals orc_eval_paths_g bit for bit."""
    w = _world(oracle_mod, 80, maxratio_smooth=True)
    e, orc, O = w["e"], w["orc"], w["O"]
    D = 5
    ut = _ut(80, D)
    for k, v in DEFAULTS.items():
        e.set_option(k, v)
    for n in (509, 100):
        pairs = _pairs(n, 80 + n)
        gpu = e.eval_generated(pairs, ut, raster=w["raster"])
        assert e.last_kernel() == "K2g+pack" and e.last_group() == 21
        ref = orc.eval_paths(O.gen_paths(pairs, ut), mode="raster", rdesc=w["rd"], rec=w["rec"],
                             group=21)
        for gk, ok in KEYS:
            np.testing.assert_array_equal(gpu[gk].cpu().numpy(), ref[ok], err_msg=gk)
        np.testing.assert_array_equal(gpu["best_fval_idx"].cpu().numpy(),
                                      O.argmin(ref["cost"], D, True))
        np.testing.assert_array_equal(gpu["best_length_idx"].cpu().numpy(),
                                      O.argmin(ref["length"], D, False))
