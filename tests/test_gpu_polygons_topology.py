"""GPU land polygons (K8: k_ccl_tile, k_ccl_bmerge and its skip rules, the root bitmaps and
ranks, k_ccl_stats_rows with its full-table path, k_ccl_extents_rows, and all of it again on the
cut sub-grids of large regions) on masks built to break a labelling (polygons_masks): thousands
of single-cell components, diagonals, one-cell-wide paths through tile corners, a spiral, nested
rings, percolating noise, all 512 patterns of the 3 x 3 cells around a tile corner, and box cuts
on, one before, one after and inside the tile edges of the refined grid.

Every case is held to two things: the rectangles equal the oracle's bit for bit (the contract
of test_gpu_polygons.py), and on their own they fit the pieces of a flood-fill reference that
shares no code with either (polygons_ref.check_rects), so a mistake the oracle shared would not
hide.  The oracle meets the same reference on the CPU in test_polygons_topology_cpu.py."""
import numpy as np
import pytest

import polygons_masks as M
import polygons_ref as R

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


def _engine(option, value):
    from uam_path_planning_amd import build
    from uam_path_planning_amd.engine import Engine

    if not torch.cuda.is_available():
        pytest.fail("GPU tests need an MI355X")
    build.build_library()
    e = Engine(0)
    e.set_option(option, value)
    return e


@pytest.fixture(scope="module", params=[1, 0], ids=["tiled", "cells"])
def eng(request):
    return _engine("k8_tiled", request.param)


@pytest.fixture(scope="module", params=[1, 8], ids=["streams1", "streams8"])
def eng_streams(request):
    return _engine("k8_streams", request.param)


def _geo(mask):
    from uam_path_planning_amd.engine import RasterGeo

    ny, nx = mask.shape
    return RasterGeo(nx=nx, ny=ny, x0=0.0, y_top=ny * M.DX, dx=M.DX, dy=M.DX, nodata=-9999.0,
                     dem_threshold=0.0)


def _gpu(e, dem, thr, prm):
    from uam_path_planning_amd import _lib

    p = _lib.PolyprocParams(prm.min_area, prm.large_area, prm.min_approx_area, prm.divisions, 0)
    got = e.dem_polygons(dem, _geo(dem), thr, M.UNIT_M, params=p)
    return np.asarray(got, np.int64).reshape(-1, 4, 2)


_oracle_rects = {}   # case -> the oracle's rectangles, computed once for both engines
_fits = {}           # case -> rectangles (bytes) that check_rects has already accepted


def _verify(O, got, key, dem, thr, prm, pieces):
    # on its own against the flood fill (check_rects is a pure function of its arguments: the
    # same rectangles for the same case are not measured twice) ...
    if _fits.get(key) != got.tobytes():
        ny = dem.shape[0]
        stats = {}
        R.check_rects(got, pieces, M.DX_M, 0.0, ny * M.DX_M, stats)
        print(f"{key}: {len(pieces)} pieces, {stats}")
        _fits[key] = got.tobytes()
    # ... and bit for bit against the oracle
    if key not in _oracle_rects:
        _oracle_rects[key] = M.oracle_rects(O, dem, thr, prm)
    np.testing.assert_array_equal(got, _oracle_rects[key])


@pytest.mark.parametrize("name,kind", M.CASES, ids=M.CASE_IDS)
def test_adversarial_masks(eng, oracle_mod, name, kind):
    mask, prm, pieces = M.case(name, kind)
    dem = M.dem_of(mask)
    got = _gpu(eng, dem, 0.0, prm)
    _verify(oracle_mod, got, (name, kind), dem, 0.0, prm, pieces)


def _semantics_dem(thr):
    """White-noise terrain around the threshold with a few percent each of the values a mask
    can get wrong."""
    rng = np.random.default_rng(7)
    dem = rng.normal(100.0, 150.0, (M.NY, M.NX)).astype(np.float32)
    t = np.float32(thr)
    special = [np.nan, np.inf, -np.inf, -0.0, t, np.nextafter(t, np.float32(np.inf)), -9999.0]
    pick = rng.random((M.NY, M.NX))
    for k, v in enumerate(special):
        dem[(pick >= 0.04 * k) & (pick < 0.04 * (k + 1))] = v
    return dem


@pytest.mark.parametrize("thr", [0.0, 150.0, -9999.0])
def test_mask_semantics(eng, oracle_mod, thr):
    """NaN, infinities, -0.0, cells at the threshold and one float32 above it, nodata: the
    mask is polygons_ref.mask_of's (dem == -9999 for thr -9999, else dem > thr; NaN false)."""
    dem = _semantics_dem(thr)
    for v in (np.inf, -np.inf, -9999.0, np.float32(thr)):
        assert 0.02 * dem.size < (dem == v).sum()
    assert 0.02 * dem.size < np.isnan(dem).sum()
    prm = M.params()
    pieces = R.expected_pieces(R.mask_of(dem, thr), prm, M.DX_M)
    assert len(pieces) > 100
    got = _gpu(eng, dem, thr, prm)
    _verify(oracle_mod, got, ("semantics", thr), dem, thr, prm, pieces)


def test_many_regions_on_streams(eng_streams, oracle_mod):
    """Dozens of divided regions of the percolation mask in flight on 1 or 8 streams; the
    engine stays usable: an ordinary call afterwards still equals the oracle."""
    from uam_path_planning_amd.scenario import raster_geo
    from uam_path_planning_amd.synthetic import synthetic_dem

    mask, prm, pieces = M.case("noise59_L40", "own")
    assert sum(len(c) > 40 for c in R.components(mask)) > 24
    dem = M.dem_of(mask)
    got = _gpu(eng_streams, dem, 0.0, prm)
    _verify(oracle_mod, got, ("noise59_L40", "own"), dem, 0.0, prm, pieces)
    geo = raster_geo(256)
    dem2 = synthetic_dem(256, seed=3)
    again = np.asarray(eng_streams.dem_polygons(dem2, geo, 0.0), np.int64).reshape(-1, 4, 2)
    rd = oracle_mod.Oracle.raster_desc(geo.nx, geo.ny, geo.x0, geo.y_top, geo.dx, geo.dy)
    ref = oracle_mod.dem_polygons(dem2, rd, 0.0, 1000.0)
    assert len(ref) > 0
    np.testing.assert_array_equal(again, ref)
