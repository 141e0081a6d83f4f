"""The joint route field (K9j) on the GPU: uam_route_field_joint / uam_route_paths_joint against
the host twin and tests/route_joint_ref.py bit for bit on dist, next, owner, wp, status, steps,
vertices and goal, for every tile edge and sweep count: one bit pattern per case.  Bridge 1
against Engine.route_field on the GPU; a long-lived context that runs the per-goal and the joint
calls in turn; a second stream; the kernel names; the error paths.

Cases: tests/route_joint_cases.py (100 x 76 cells: 7 x 5, 4 x 3 and 2 x 2 tiles, all with partial
tiles; 1 x 1 and 3 x 2 cells)."""
import ctypes

import numpy as np
import pytest

import route_joint_cases as JC

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

TILES = (16, 32, 64)
INNERS = (1, 4, 64)
KEYS = ("wp", "status", "steps", "vertices", "goal")
# the analytic map the context is given (the route calls read the record raster, not the map)
MAP = {"obstacles": [{"kind": "polygon",
                      "vertices": [[0.6, -1.0], [0.6, 1.0], [1.2, 1.0], [1.2, -1.0]]}],
       "regions": [], "x_start": [0.45, 1.96], "x_goal": [1.35, 1.96],
       "options": {"length_smooth": True, "penalty_smooth": True, "obstacle_smooth": True,
                   "maxratio_smooth": False},
       "maxratio": 1.1, "maxalpha": 0.3, "enlargement": 0.0, "weights": []}


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
    from uam_path_planning_amd.scenario import build_region_map

    if not torch.cuda.is_available():
        pytest.fail("GPU tests need an MI355X")
    build.build_library()
    e = Engine(0)
    e.set_geometry(compile_map(build_region_map(MAP)))
    e.set_params(PathParams(N=JC.C.N_DEFAULT, **MAP["options"], maxratio=MAP["maxratio"],
                            maxalpha=MAP["maxalpha"], enlargement=0.0, weights=()))
    return e


def raster_of(eng, c):
    from uam_path_planning_amd.engine import CostRaster, RasterGeo

    g = c["geo"]
    geo = RasterGeo(g.nx, g.ny, g.x0, g.y_top, g.dx, g.dy)
    rec = torch.from_numpy(c["rec"].view(np.int32).copy()).to(eng.torch_device)
    return CostRaster(geo, rec)


def joint_field(eng, c, raster, tile=32, inner=16, max_rounds=0):
    eng.set_option("k9_tile", tile)
    eng.set_option("k9_inner", inner)
    f = eng.route_field(raster, c["goals"], c["lam"], c["block_flags"], c["inflate"], max_rounds,
                        joint=True)
    assert eng.last_kernel() == "K9j"
    return f


def check_field(f, name, what):
    r = JC.reference(name)
    assert f.joint and tuple(f.dist.shape) == (1,) + r["dist"].shape == tuple(f.next.shape)
    same(f.dist[0].cpu().numpy(), r["dist"], f"dist {what}")
    same(f.next[0].cpu().numpy(), r["next"], f"next {what}")
    same(f.owner.cpu().numpy(), r["owner"], f"owner {what}")


def check_paths(eng, f, name, what, spans=JC.SPANS):
    c = JC.BY_NAME[name]
    for span in spans:
        o = eng.route_paths(f, c["starts"], smooth=span)
        assert eng.last_kernel() == ("K9js" if span else "K9jt")
        want = JC.reference_paths(name, span)
        for k in KEYS:
            same(o[k].cpu().numpy(), want[k], f"{k} {what} span {span}")


@pytest.mark.parametrize("name", JC.NAMES)
def test_matches_reference_for_every_tile_and_inner(eng, name):
    """GPU == reference (== host twin, tests/test_route_joint_cpu.py) whatever the tile edge and
    the sweeps per round; the host twin once more, directly."""
    from uam_path_planning_amd.engine import Engine

    c = JC.BY_NAME[name]
    assert c["N"] == eng.params.N
    raster = raster_of(eng, c)
    rounds = {}
    for tile in TILES:
        for inner in INNERS:
            f = joint_field(eng, c, raster, tile, inner)
            check_field(f, name, f"{name} tile {tile} inner {inner}")
            rounds[tile, inner] = f.rounds
            assert f.visits >= f.rounds
    check_paths(eng, f, name, name)
    if name == "spiral_ends":
        for tile in TILES:
            assert rounds[tile, 1] > rounds[tile, 64], rounds
    if name == "no_valid_goal":
        assert set(rounds.values()) == {0}
    h = Engine.route_field_host(raster.geo, c["rec"], c["goals"], c["lam"], c["block_flags"],
                                c["inflate"], joint=True)
    for k in ("dist", "next", "owner"):
        same(getattr(f, k).cpu().numpy(), getattr(h, k), f"host twin {k} {name}")
    for span in (0, 64):
        o = eng.route_paths(f, c["starts"], smooth=span)
        ho = Engine.route_paths_host(h, c["starts"], None, c["N"], smooth=span)
        for k in KEYS:
            same(o[k].cpu().numpy(), ho[k], f"host twin {k} {name} span {span}")


@pytest.mark.parametrize("name", ["open_five", "shared_and_invalid", "symmetric", "pocket",
                                  "inflate_2", "raster_3x2"])
def test_bridge_1_on_the_gpu(eng, name):
    """dist == the elementwise minimum of Engine.route_field's per-goal planes; the owner
    property against those planes."""
    c = JC.BY_NAME[name]
    raster = raster_of(eng, c)
    f = joint_field(eng, c, raster)
    per = eng.route_field(raster, c["goals"], c["lam"], c["block_flags"], c["inflate"])
    assert eng.last_kernel() == "K9" and not per.joint and per.owner is None
    same(f.dist[0].cpu().numpy(), per.dist.min(dim=0).values.cpu().numpy(), f"bridge 1 {name}")
    owner = f.owner.cpu().numpy()
    iy, ix = np.nonzero(owner >= 0)
    same(f.dist[0].cpu().numpy()[iy, ix], per.dist.cpu().numpy()[owner[iy, ix], iy, ix],
         f"owner property {name}")


@pytest.mark.parametrize("name", sorted(JC.SINGLE))
def test_one_goal_is_the_per_goal_field(eng, name):
    """Bridges 2 and 3 on the GPU."""
    c = JC.BY_NAME[name]
    raster = raster_of(eng, c)
    f = joint_field(eng, c, raster)
    per = eng.route_field(raster, c["goals"], c["lam"], c["block_flags"], c["inflate"])
    same(f.dist.cpu().numpy(), per.dist.cpu().numpy(), "bridge 2 dist")
    same(f.next.cpu().numpy(), per.next.cpu().numpy(), "bridge 2 next")
    gi = np.zeros(len(c["starts"]), dtype=np.int32)
    for span in JC.SPANS:
        o = eng.route_paths(f, c["starts"], smooth=span)
        p = eng.route_paths(per, c["starts"], gi, smooth=span)
        st = p["status"].cpu().numpy()
        assert not np.any(st == 4)
        same(o["status"].cpu().numpy(), st, f"bridge 3 status span {span}")
        same(o["steps"].cpu().numpy(), p["steps"].cpu().numpy(), f"bridge 3 steps span {span}")
        if span:
            same(o["vertices"].cpu().numpy(), p["vertices"].cpu().numpy(), f"vertices {span}")
        same(o["wp"].cpu().numpy()[st == 0], p["wp"].cpu().numpy()[st == 0], f"wp span {span}")


def test_one_context_runs_per_goal_joint_per_goal(eng):
    """A long-lived context: the per-goal field before and after a joint field has identical
    bits (the joint call leaves nothing behind in the context or the shared kernels' state)."""
    c = JC.BY_NAME["shared_and_invalid"]
    raster = raster_of(eng, c)
    eng.set_option("k9_tile", 16)
    eng.set_option("k9_inner", 4)
    gi = np.arange(len(c["starts"]), dtype=np.int32) % len(c["goals"])

    def per_goal():
        f = eng.route_field(raster, c["goals"], c["lam"], c["block_flags"], c["inflate"])
        assert eng.last_kernel() == "K9"
        o = eng.route_paths(f, c["starts"], gi, smooth=7)
        assert eng.last_kernel() == "K9s"
        return [f.dist.cpu().numpy(), f.next.cpu().numpy()] + [o[k].cpu().numpy() for k in
                                                              ("wp", "status", "steps", "vertices")]

    first = per_goal()
    f = joint_field(eng, c, raster, 16, 4)
    check_field(f, "shared_and_invalid", "between the per-goal calls")
    check_paths(eng, f, "shared_and_invalid", "between the per-goal calls", spans=(0, 7))
    third = per_goal()
    for a, b in zip(first, third):
        same(a, b, "per-goal bits before and after the joint call")
    with pytest.raises(ValueError, match="goal_idx"):
        eng.route_paths(f, c["starts"], gi)
    with pytest.raises(ValueError, match="goal_idx"):
        eng.route_paths(eng.route_field(raster, c["goals"]), c["starts"])


def test_second_stream_gives_the_same_bits(eng):
    name = "spiral_ends"
    c = JC.BY_NAME[name]
    raster = raster_of(eng, c)
    torch.cuda.synchronize()
    with torch.cuda.stream(torch.cuda.Stream(eng.torch_device)):
        f = joint_field(eng, c, raster)
        check_field(f, name, "second stream")
        check_paths(eng, f, name, "second stream", spans=(0, 64))
    torch.cuda.synchronize()


def test_max_rounds_is_an_error_and_the_context_stays_usable(eng):
    from uam_path_planning_amd import _lib

    c = JC.BY_NAME["spiral_ends"]
    raster = raster_of(eng, c)
    with pytest.raises(_lib.UamError, match="max_rounds") as ei:
        joint_field(eng, c, raster, 32, 4, max_rounds=1)
    assert "status -4" in str(ei.value)           # UAM_E_STATE
    f = joint_field(eng, c, raster, 32, 4)
    check_field(f, "spiral_ends", "after the failed call")


def test_invalid_arguments_come_before_any_launch(eng):
    from uam_path_planning_amd import _lib

    name = "open_five"
    c = JC.BY_NAME[name]
    raster = raster_of(eng, c)
    for kw in (dict(lam=float("nan")), dict(lam=-0.5), dict(inflate=9)):
        with pytest.raises(ValueError):
            eng.route_field(raster, c["goals"], joint=True, **kw)
    with pytest.raises(ValueError, match="n_goals"):
        eng.route_field(raster, np.zeros((0, 2)), joint=True)
    gs = raster.geo.as_struct()
    rp = _lib.RouteParams(_lib.ABI_VERSION, 1.0, 1, 0, 0)
    G = len(c["goals"])
    need = eng.lib.uam_route_joint_workspace_bytes(ctypes.byref(gs), ctypes.byref(rp), G)
    ny, nx = raster.geo.ny, raster.geo.nx
    FILL = 0x5A
    bufs = dict(rec=raster.rec, goals=eng.tensor(c["goals"], torch.float64),
                dist=eng.empty((ny, nx), torch.float64), next=eng.empty((ny, nx), torch.uint8),
                owner=eng.empty((ny, nx), torch.int32),
                ws=eng.empty((need // 256 + 1, 256), torch.uint8))
    outs = ("dist", "next", "owner")

    def call(n_goals=G, ws_bytes=need, shift=None, **null):
        for k in outs:
            bufs[k].view(torch.uint8).fill_(FILL)
        p = {k: (None if k in null else v.data_ptr()) for k, v in bufs.items()}
        if shift:
            p[shift[0]] += shift[1]
        st = eng.lib.uam_route_field_joint(eng._ctx, ctypes.byref(gs), p["rec"], ctypes.byref(rp),
                                           p["goals"], n_goals, p["dist"], p["next"], p["owner"],
                                           p["ws"], ws_bytes, None, eng.stream)
        if st != _lib.UAM_OK:
            eng.synchronize()
            for k in outs:
                assert bool((bufs[k].view(torch.uint8) == FILL).all()), k
        return st

    for k in bufs:
        assert call(**{k: True}) == _lib.UAM_E_INVALID, k
    for n in (0, 2 ** 20 + 1):
        assert call(n_goals=n) == _lib.UAM_E_INVALID
    assert call(ws_bytes=need - 1) == _lib.UAM_E_INVALID
    for shift in (("ws", 128), ("dist", 4), ("owner", 2)):
        assert call(shift=shift) == _lib.UAM_E_INVALID, shift
    assert call() == _lib.UAM_OK
    eng.synchronize()
    same(bufs["owner"].cpu().numpy(), JC.reference(name)["owner"], "raw call")

    f = joint_field(eng, c, raster)
    Q, N = len(c["starts"]), c["N"]
    pb = dict(rec=raster.rec, bits=eng.route_free_bits(f), next=f.next, owner=f.owner,
              goals=f.goals, starts=eng.tensor(c["starts"], torch.float64),
              wp=eng.empty((Q, N + 2, 2), torch.float64), status=eng.empty((Q,), torch.int32),
              steps=eng.empty((Q,), torch.int32), vertices=eng.empty((Q,), torch.int32),
              goal=eng.empty((Q,), torch.int32))
    pouts = ("wp", "status", "steps", "vertices", "goal")

    def paths(span=7, n_goals=G, n_queries=Q, **null):
        for k in pouts:
            pb[k].view(torch.uint8).fill_(FILL)
        p = {k: (None if k in null else v.data_ptr()) for k, v in pb.items()}
        st = eng.lib.uam_route_paths_joint(
            eng._ctx, ctypes.byref(gs), p["rec"], ctypes.byref(rp), p["bits"], p["next"],
            p["owner"], p["goals"], n_goals, p["starts"], n_queries, span, p["wp"], p["status"],
            p["steps"], p["vertices"], p["goal"], eng.stream)
        if st != _lib.UAM_OK:
            eng.synchronize()
            for k in pouts:
                assert bool((pb[k].view(torch.uint8) == FILL).all()), k
        return st

    for k in ("next", "owner", "goals", "starts", "wp", "status"):
        assert paths(**{k: True}) == _lib.UAM_E_INVALID, k
    assert paths(span=0, rec=True) == _lib.UAM_E_INVALID
    assert paths(span=1, bits=True) == _lib.UAM_E_INVALID
    for span in (-1, 1025):
        assert paths(span=span) == _lib.UAM_E_INVALID
    assert paths(n_goals=0) == _lib.UAM_E_INVALID
    assert paths(n_queries=-1) == _lib.UAM_E_INVALID
    assert paths(steps=True, vertices=True, goal=True) == _lib.UAM_OK     # each may be NULL
    eng.synchronize()
    same(pb["wp"].cpu().numpy(), JC.reference_paths(name, 7)["wp"], "steps / vertices / goal NULL")
    assert paths(span=0, bits=True) == _lib.UAM_OK
    eng.synchronize()
    same(pb["goal"].cpu().numpy(), JC.reference_paths(name, 0)["goal"], "span 0, bits NULL")


def test_needs_params():
    """UAM_E_STATE without uam_set_params."""
    from uam_path_planning_amd import _lib
    from uam_path_planning_amd.engine import Engine, RasterGeo

    e = Engine(0)
    g = JC.GEO
    gs = RasterGeo(g.nx, g.ny, g.x0, g.y_top, g.dx, g.dy).as_struct()
    rp = _lib.RouteParams(_lib.ABI_VERSION, 1.0, 1, 0, 0)
    one = e.empty((64,), torch.float64).data_ptr()
    assert e.lib.uam_route_paths_joint(e._ctx, ctypes.byref(gs), one, ctypes.byref(rp), one, one,
                                       one, one, 1, one, 1, 4, one, one, None, None, None,
                                       e.stream) == _lib.UAM_E_STATE
