"""Route seeds (K9) on the GPU: uam_route_field / uam_route_paths against tests/route_ref.py
(and hence the host twin, tests/test_route_cpu.py) bit for bit on dist, next, wp, status and
steps, for every tile edge and sweep count: one bit pattern per case.  Then, with no reference
involved, the seeds under eval_waypoints; an analytic wall where every arc candidate fails and
the seed refines; the error paths.

Cases: tests/route_cases.py (100 x 76 cells: 7 x 5, 4 x 3 and 2 x 2 tiles, all with partial
tiles)."""
import ctypes

import numpy as np
import pytest

import route_cases as C

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

TILES = (16, 32, 64)
INNERS = (1, 4, 64)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype == np.float64 else a


def same(a, b, what=""):
    np.testing.assert_array_equal(bits(a), bits(b), err_msg=what)


def rect(xa, xb, ya, yb):
    return {"kind": "polygon", "vertices": [[xa, ya], [xa, yb], [xb, yb], [xb, ya]]}


# the analytic wall of the end-to-end test: three polygons 0.6 km thick across the whole
# raster (and far beyond it: nothing flies round its ends) with one gap of 0.12 km near the
# northern edge
WALL = {"obstacles": [rect(0.6, 1.2, -14.0, -4.0), rect(0.6, 1.2, -5.0, 2.84),
                      rect(0.6, 1.2, 2.96, 14.0)],
        "regions": [], "x_start": [0.45, 1.96], "x_goal": [1.35, 1.96],
        "options": {"length_smooth": True, "penalty_smooth": True, "obstacle_smooth": True,
                    "maxratio_smooth": False},
        "maxratio": 1.1, "maxalpha": 0.3, "enlargement": 0.0, "weights": []}
WALL_PAIRS = np.array([[0.45, 1.96, 1.35, 1.96], [0.47, 1.98, 1.34, 1.94],
                       [1.36, 1.96, 0.46, 1.99]])


@pytest.fixture(scope="module")
def eng():
    from uam_path_planning_amd import build
    from uam_path_planning_amd.engine import Engine, PathParams
    from uam_path_planning_amd.geometry import compile_map
    from uam_path_planning_amd.scenario import build_region_map

    if not torch.cuda.is_available():
        pytest.fail("GPU tests need an MI355X")
    build.build_library()
    e = Engine(0)
    e.set_geometry(compile_map(build_region_map(WALL)))
    e.set_params(PathParams(N=C.N_DEFAULT, **WALL["options"], maxratio=WALL["maxratio"],
                            maxalpha=WALL["maxalpha"], enlargement=0.0, weights=()))
    return e


def raster_of(eng, c):
    from uam_path_planning_amd.engine import CostRaster, RasterGeo

    g = c["geo"]
    geo = RasterGeo(g.nx, g.ny, g.x0, g.y_top, g.dx, g.dy)
    rec = torch.from_numpy(c["rec"].view(np.int32).copy()).to(eng.torch_device)
    return CostRaster(geo, rec)


def run(eng, c, raster, tile=32, inner=32, max_rounds=0):
    eng.set_option("k9_tile", tile)
    eng.set_option("k9_inner", inner)
    f = eng.route_field(raster, c["goals"], c["lam"], c["block_flags"], c["inflate"], max_rounds)
    assert eng.last_kernel() == "K9"
    o = eng.route_paths(f, c["starts"], c["goal_idx"])
    assert eng.last_kernel() == "K9t"
    return f, o


def check(f, o, name, what):
    dist, nxt, wp, status, steps, _ = C.reference(name)
    same(f.dist.cpu().numpy(), dist, f"dist {what}")
    same(f.next.cpu().numpy(), nxt, f"next {what}")
    same(o["status"].cpu().numpy(), status, f"status {what}")
    same(o["steps"].cpu().numpy(), steps, f"steps {what}")
    same(o["wp"].cpu().numpy(), wp, f"wp {what}")


@pytest.mark.parametrize("name", C.NAMES)
def test_matches_reference_for_every_tile_and_inner(eng, name):
    """One bit pattern per case, whatever the tile edge and the sweeps per round; and, with no
    reference involved, every status-0 seed clears the no-fly cells and the raster."""
    c = C.BY_NAME[name]
    assert c["N"] == eng.params.N
    raster = raster_of(eng, c)
    rounds = {}
    for tile in TILES:
        for inner in INNERS:
            f, o = run(eng, c, raster, tile, inner)
            check(f, o, name, f"{name} tile {tile} inner {inner}")
            rounds[tile, inner] = f.rounds
            assert f.visits >= f.rounds
    if name == "spiral":
        # the options are not ignored: fewer sweeps per round take more rounds
        for tile in TILES:
            assert rounds[tile, 1] > rounds[tile, 64], rounds
    ok = (o["status"] == 0).cpu().numpy()
    if name in ("sealed_ring", "blocked_and_offmap_goal"):
        assert not ok.any()
    if c["block_flags"] & C.NFZ and ok.any():
        ev = eng.eval_waypoints(o["wp"], raster=raster)
        assert np.all(ev["nfz_hits"].cpu().numpy()[ok] == 0)
        assert np.all(ev["offmap"].cpu().numpy()[ok] == 0)


def test_max_rounds_is_an_error_and_the_context_stays_usable(eng):
    from uam_path_planning_amd import _lib

    c = C.BY_NAME["spiral"]
    raster = raster_of(eng, c)
    with pytest.raises(_lib.UamError, match="max_rounds") as ei:
        run(eng, c, raster, 32, 4, max_rounds=1)
    assert "status -4" in str(ei.value)           # UAM_E_STATE
    f, o = run(eng, c, raster, 32, 4)
    check(f, o, "spiral", "after the failed call")


def test_invalid_arguments_come_before_any_launch(eng):
    from uam_path_planning_amd import _lib

    c = C.BY_NAME["open"]
    raster = raster_of(eng, c)
    for kw in (dict(lam=float("nan")), dict(lam=-0.5), dict(inflate=9)):
        with pytest.raises(ValueError):
            eng.route_field(raster, c["goals"], **kw)
    with pytest.raises(ValueError, match="n_goals"):
        eng.route_field(raster, np.zeros((0, 2)))
    # NULL buffers, straight at the C ABI
    gs = raster.geo.as_struct()
    rp = _lib.RouteParams(_lib.ABI_VERSION, 1.0, 1, 0, 0)
    need = eng.lib.uam_route_workspace_bytes(ctypes.byref(gs), ctypes.byref(rp))
    n = raster.geo.nx * raster.geo.ny
    bufs = dict(rec=raster.rec, goals=eng.tensor(c["goals"], torch.float64),
                dist=eng.empty((n,), torch.float64), next=eng.empty((n,), torch.uint8),
                ws=eng.empty((need // 256 + 1, 256), torch.uint8))

    def call(**null):
        p = {k: (None if k in null else ctypes.c_void_p(v.data_ptr())) for k, v in bufs.items()}
        return eng.lib.uam_route_field(eng._ctx, ctypes.byref(gs), p["rec"], ctypes.byref(rp),
                                       p["goals"], 1, p["dist"], p["next"], p["ws"], need, None,
                                       eng.stream)

    for k in bufs:
        assert call(**{k: True}) == _lib.UAM_E_INVALID, k
    assert call() == _lib.UAM_OK
    with pytest.raises(ValueError, match="UAM_OPT_K9_TILE"):
        eng.set_option("k9_tile", 48)
    with pytest.raises(ValueError, match="UAM_OPT_K9_INNER"):
        eng.set_option("k9_inner", 0)
    # and the ordinary call still gives the reference's bits
    f, o = run(eng, c, raster)
    check(f, o, "open", "after the refused calls")


def test_wall_with_one_gap_end_to_end(eng):
    """A wall every one of the D = 5 arcs runs into: the route seed passes the gap, and
    refinement turns it into a far better path than the best arc (which stalls with its
    waypoints on the two sides of the wall).  Chosen so that the same holds for route_ref's
    path under the CPU oracle's refinement: arcs end at sum g^2 of 0.3 .. 0.5, the seeds
    below 1e-5."""
    from uam_path_planning_amd.arcs import REFERENCE_DISPLACEMENTS, arc_table
    from uam_path_planning_amd.engine import RasterGeo

    g = C.GEO
    N = eng.params.N
    geo = RasterGeo(g.nx, g.ny, g.x0, g.y_top, g.dx, g.dy)
    raster = eng.raster_build(geo)
    arcs = eng.gen_paths(WALL_PAIRS, arc_table(N, REFERENCE_DISPLACEMENTS))
    hits = eng.eval_waypoints(arcs, raster=raster)["nfz_hits"].cpu().numpy()
    assert np.all(hits > 0), hits
    eng.set_option("k9_tile", 32)
    eng.set_option("k9_inner", 32)
    f = eng.route_field(raster, WALL_PAIRS[:, 2:4], inflate=1)
    seed = eng.route_paths(f, WALL_PAIRS[:, 0:2], np.arange(len(WALL_PAIRS)))
    assert np.all(seed["status"].cpu().numpy() == 0)
    ev = eng.eval_waypoints(seed["wp"], raster=raster)
    assert np.all(ev["nfz_hits"].cpu().numpy() == 0) and np.all(ev["offmap"].cpu().numpy() == 0)
    best_arc = eng.refine(arcs)["infeas"].cpu().numpy().reshape(-1, 5).min(axis=1)
    refined = eng.refine(seed["wp"])["infeas"].cpu().numpy()
    print("sum g^2 after refine: best arc", best_arc, "route seed", refined)
    assert np.all(refined < best_arc), (refined, best_arc)
