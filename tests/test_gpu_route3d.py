"""Route seeds in the volume (K9v) on the GPU: uam_route3d_field / uam_route3d_paths against
tests/route3d_ref.py (and hence the host twin, tests/test_route3d_cpu.py) bit for bit on dist,
next, wp3, status and steps, for every tile shape and sweep count: one bit pattern per case.
Then, with no reference involved, the seeds under eval_waypoints3d; the ridge end to end (every
arc candidate of the straight climb flies below the terrain, the seed clears it); the error
paths.

Cases: tests/route3d_cases.py (43 x 29 x 11 voxels: partial tiles on every axis for every tile
shape)."""
import ctypes

import numpy as np
import pytest

import route3d_cases as C

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

TILES = ((8, 4), (8, 8), (16, 4), (16, 8))
INNERS = (1, 4, 64)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype == np.float64 else a


def same(a, b, what=""):
    np.testing.assert_array_equal(bits(a), bits(b), err_msg=what)


@pytest.fixture(scope="module")
def eng():
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
    e.set_params(PathParams(N=C.N, **spec["options"], maxratio=spec["maxratio"],
                            maxalpha=spec["maxalpha"], enlargement=spec["enlargement"],
                            weights=tuple(spec["weights"]), altitude=320.0))
    return e


_volumes = {}


def volume_of(eng, c):
    """The case's volume on the device (built once per case): the words of C.volume_words at
    the front of uam_volume_shape's buffer, the column bitmap all set (every column is read)."""
    from uam_path_planning_amd.engine import VolumeGeo

    if c["name"] not in _volumes:
        vol = eng.volume_alloc(VolumeGeo(*c["geo"]))
        w = C.volume_words(c)
        vol.buf.zero_()
        vol.buf[:w.size].copy_(eng.tensor(w.view(np.int32), torch.int32))
        vol.cbits.fill_(-1)
        _volumes[c["name"]] = vol
    return _volumes[c["name"]]


def run(eng, c, vol, tile=(8, 8), inner=16, max_rounds=0):
    eng.set_option("k9v_tile_xy", tile[0])
    eng.set_option("k9v_tile_z", tile[1])
    eng.set_option("k9v_inner", inner)
    f = eng.route_field3d(vol, c["goals"], c["lam"], c["block_flags"], c["inflate"], c["agl"],
                          c["kappa"], max_rounds)
    assert eng.last_kernel() == "K9v"
    o = eng.route_paths3d(f, c["starts"], c["goal_idx"])
    assert eng.last_kernel() == "K9vt"
    return f, o


def check(f, o, name, what):
    dist, nxt, wp, status, steps, _ = C.reference(name)
    same(f.dist.cpu().numpy(), dist, f"dist {what}")
    same(f.next.cpu().numpy(), nxt, f"next {what}")
    same(o["status"].cpu().numpy(), status, f"status {what}")
    same(o["steps"].cpu().numpy(), steps, f"steps {what}")
    same(o["wp3"].cpu().numpy(), wp, f"wp3 {what}")


@pytest.mark.parametrize("name", C.NAMES)
def test_matches_reference_for_every_tile_and_inner(eng, name):
    """One bit pattern per case, whatever the tile shape and the sweeps per round; and, with no
    reference involved, every status-0 seed stays inside the volume, out of the no-fly columns
    and above the terrain."""
    from uam_path_planning_amd.engine import Vertical

    c = C.BY_NAME[name]
    assert c["N"] == eng.params.N
    vol = volume_of(eng, c)
    rounds = {}
    for tile in TILES:
        for inner in INNERS:
            f, o = run(eng, c, vol, tile, inner)
            check(f, o, name, f"{name} tile {tile} inner {inner}")
            rounds[tile, inner] = f.rounds
            assert f.visits >= f.rounds
    if name == "layer_tradeoff_lam50":
        # the options are not ignored: fewer sweeps per round take more rounds
        for tile in TILES:
            assert rounds[tile, 1] > rounds[tile, 64], rounds
    ok = (o["status"] == 0).cpu().numpy()
    if name in ("sealed_box", "blocked_goal_and_offvolume_goal"):
        assert not ok.any()
    if ok.any():
        ev = eng.eval_waypoints3d(o["wp3"], vol, vertical=Vertical(c["kappa"]))
        assert np.all(ev["offmap"].cpu().numpy()[ok] == 0)
        assert np.all(ev["below_terrain"].cpu().numpy()[ok] == 0)
        if c["block_flags"] & C.NFZ:
            assert np.all(ev["nfz_hits"].cpu().numpy()[ok] == 0)


def test_ridge_end_to_end(eng):
    """A ridge no straight climb clears: every one of the D = 5 arc candidates between the low
    end points has waypoints below the terrain; the seed through the field has none and a
    finite cost under the vertical terms."""
    from uam_path_planning_amd.arcs import REFERENCE_DISPLACEMENTS, arc_table
    from uam_path_planning_amd.engine import Vertical

    c = C.BY_NAME["ridge"]
    vol = volume_of(eng, c)
    q = [0, 3]                                # the starts on the row of goal 0 / towards goal 1
    pairs6 = np.concatenate([c["starts"][q], c["goals"][c["goal_idx"][q]]], axis=1)
    arcs = eng.eval_generated3d(pairs6, arc_table(C.N, REFERENCE_DISPLACEMENTS), vol)
    below = arcs["below_terrain"].cpu().numpy()
    assert below.shape == (10,) and np.all(below > 0), below
    assert np.all(arcs["offmap"].cpu().numpy() == 0)
    f, o = run(eng, c, vol)
    assert np.all(o["status"].cpu().numpy() == 0)
    ev = eng.eval_waypoints3d(o["wp3"], vol, vertical=Vertical(c["kappa"]))
    assert np.all(ev["below_terrain"].cpu().numpy() == 0)
    assert np.all(ev["offmap"].cpu().numpy() == 0)
    cost = ev["cost"].cpu().numpy()
    assert np.all(np.isfinite(cost)) and np.all(cost > 0), cost
    assert np.all(ev["climb_sum"].cpu().numpy() == 0)      # no climb limit set


def test_max_rounds_is_an_error_and_the_context_stays_usable(eng):
    from uam_path_planning_amd import _lib

    c = C.BY_NAME["layer_tradeoff_lam50"]
    vol = volume_of(eng, c)
    with pytest.raises(_lib.UamError, match="max_rounds") as ei:
        run(eng, c, vol, (8, 4), 4, max_rounds=1)
    assert "status -4" in str(ei.value)           # UAM_E_STATE
    f, o = run(eng, c, vol, (8, 4), 4)
    check(f, o, c["name"], "after the failed call")


def test_invalid_arguments_come_before_any_launch(eng):
    from uam_path_planning_amd import _lib

    c = C.BY_NAME["open3d"]
    vol = volume_of(eng, c)
    for kw in (dict(lam=float("nan")), dict(lam=-0.5), dict(inflate=9), dict(agl=-1.0),
               dict(agl=float("inf")), dict(z_scale=0.0), dict(z_scale=float("nan"))):
        with pytest.raises(ValueError):
            eng.route_field3d(vol, c["goals"], **kw)
    with pytest.raises(ValueError, match="n_goals"):
        eng.route_field3d(vol, np.zeros((0, 3)))
    # NULL buffers, straight at the C ABI
    gs = vol.geo.as_struct()
    rp = _lib.Route3dParams(_lib.ABI_VERSION, 1.0, 1, 0, 0, 0.0, 1e-3)
    need = eng.lib.uam_route3d_workspace_bytes(ctypes.byref(gs), ctypes.byref(rp))
    n = vol.geo.nx * vol.geo.ny * vol.geo.nz
    bufs = dict(vol=vol.buf, goals=eng.tensor(c["goals"], torch.float64),
                dist=eng.empty((n,), torch.float64), next=eng.empty((n,), torch.uint8),
                ws=eng.empty((need // 256 + 1, 256), torch.uint8))

    def call(**null):
        p = {k: (None if k in null else ctypes.c_void_p(v.data_ptr())) for k, v in bufs.items()}
        return eng.lib.uam_route3d_field(eng._ctx, ctypes.byref(gs), p["vol"], ctypes.byref(rp),
                                         p["goals"], 1, p["dist"], p["next"], p["ws"], need,
                                         None, eng.stream)

    for k in bufs:
        assert call(**{k: True}) == _lib.UAM_E_INVALID, k
    assert call() == _lib.UAM_OK
    for name, bad in (("k9v_tile_xy", 32), ("k9v_tile_z", 2), ("k9v_inner", 0)):
        with pytest.raises(ValueError, match="UAM_OPT_" + name.upper()):
            eng.set_option(name, bad)
    assert eng.get_option("k9v_tile_xy") in (8, 16) and eng.get_option("k9v_tile_z") in (4, 8)
    # and the ordinary call still gives the reference's bits
    f, o = run(eng, c, vol)
    check(f, o, "open3d", "after the refused calls")
