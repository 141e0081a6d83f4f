"""The joint route field in the volume (K9vj) on the GPU: uam_route3d_field_joint /
uam_route3d_paths_joint against the host twin and tests/route3d_joint_ref.py bit for bit on dist,
next, owner, wp3, status, steps, vertices and goal, for every tile shape and sweep count: one bit
pattern per case.  Bridge 1 against Engine.route_field3d on the GPU; a long-lived context that
runs the per-goal and the joint calls in turn; a second stream; the kernel names; the error paths.

Cases: tests/route3d_joint_cases.py (43 x 29 x 11 voxels: partial tiles on every axis for every
tile shape; one-layer volumes of 100 x 76; 1 x 1 x 1 and 3 x 2 x 2 voxels)."""
import ctypes

import numpy as np
import pytest

import route3d_cases as C
import route3d_joint_cases as JC

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

TILES = ((8, 4), (8, 8), (16, 4), (16, 8))
INNERS = (1, 8, 64)
KEYS = ("wp3", "status", "steps", "vertices", "goal")
# the analytic map the context is given (the route calls read the volume, not the map)
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
    e.set_params(PathParams(N=C.N, **MAP["options"], maxratio=MAP["maxratio"],
                            maxalpha=MAP["maxalpha"], enlargement=0.0, weights=()))
    return e


_volumes = {}


def volume_of(eng, c):
    """The case's volume on the device (built once per case): the words of C.volume_words at
    the front of uam_volume_shape's buffer, the column bitmap all set."""
    from uam_path_planning_amd.engine import VolumeGeo

    if c["name"] not in _volumes:
        vol = eng.volume_alloc(VolumeGeo(*c["geo"]))
        w = C.volume_words(c)
        vol.buf.zero_()
        vol.buf[:w.size].copy_(eng.tensor(w.view(np.int32), torch.int32))
        vol.cbits.fill_(-1)
        _volumes[c["name"]] = vol
    return _volumes[c["name"]]


def set_tile(eng, tile, inner):
    eng.set_option("k9v_tile_xy", tile[0])
    eng.set_option("k9v_tile_z", tile[1])
    eng.set_option("k9v_inner", inner)


def joint_field(eng, c, vol, tile=(8, 8), inner=16, max_rounds=0):
    set_tile(eng, tile, inner)
    f = eng.route_field3d(vol, c["goals"], c["lam"], c["block_flags"], c["inflate"], c["agl"],
                          c["kappa"], max_rounds, joint=True)
    assert eng.last_kernel() == "K9vj"
    return f


def per_goal_field(eng, c, vol):
    f = eng.route_field3d(vol, c["goals"], c["lam"], c["block_flags"], c["inflate"], c["agl"],
                          c["kappa"])
    assert eng.last_kernel() == "K9v" and not f.joint and f.owner is None
    return f


def check_field(f, name, what):
    r = JC.reference(name)
    assert f.joint and tuple(f.dist.shape) == (1,) + r["dist"].shape == tuple(f.next.shape)
    assert tuple(f.owner.shape) == r["owner"].shape and f.owner.dtype == torch.int32
    same(f.dist[0].cpu().numpy(), r["dist"], f"dist {what}")
    same(f.next[0].cpu().numpy(), r["next"], f"next {what}")
    same(f.owner.cpu().numpy(), r["owner"], f"owner {what}")


def check_paths(eng, f, name, what, spans=JC.SPANS):
    c = JC.BY_NAME[name]
    for span in spans:
        o = eng.route_paths3d(f, c["starts"], smooth=span)
        assert eng.last_kernel() == ("K9vjs" if span else "K9vjt")
        want = JC.reference_paths(name, span)
        assert sorted(o) == sorted(KEYS)
        for k in KEYS:
            same(o[k].cpu().numpy(), want[k], f"{k} {what} span {span}")


@pytest.mark.parametrize("name", JC.NAMES)
def test_matches_reference_for_every_tile_and_inner(eng, name):
    """GPU == reference (== host twin, tests/test_route3d_joint_cpu.py) whatever the tile shape
    and the sweeps per round; the host twin once more, directly."""
    from uam_path_planning_amd.engine import Engine, VolumeGeo

    c = JC.BY_NAME[name]
    assert c["N"] == eng.params.N
    vol = volume_of(eng, c)
    rounds = {}
    for tile in TILES:
        for inner in INNERS:
            f = joint_field(eng, c, vol, tile, inner)
            check_field(f, name, f"{name} tile {tile} inner {inner}")
            rounds[tile, inner] = f.rounds
            assert f.visits >= f.rounds
    check_paths(eng, f, name, name)
    if name == "serpentine_ends":
        for tile in TILES:
            assert rounds[tile, 1] > rounds[tile, 64], rounds
    if name == "no_valid_goal":
        assert set(rounds.values()) == {0}
    h = Engine.route_field3d_host(VolumeGeo(*c["geo"]), C.volume_words(c), c["goals"], c["lam"],
                                  c["block_flags"], c["inflate"], c["agl"], c["kappa"], joint=True)
    for k in ("dist", "next", "owner"):
        same(getattr(f, k).cpu().numpy(), getattr(h, k), f"host twin {k} {name}")
    for span in (0, 64):
        o = eng.route_paths3d(f, c["starts"], smooth=span)
        ho = Engine.route_paths3d_host(h, c["starts"], None, c["N"], smooth=span)
        for k in KEYS:
            same(o[k].cpu().numpy(), ho[k], f"host twin {k} {name} span {span}")


@pytest.mark.parametrize("name", JC.BRIDGE1_GPU)
def test_bridge_1_on_the_gpu(eng, name):
    """dist == the elementwise minimum of Engine.route_field3d's per-goal volumes; the owner
    property against those volumes."""
    c = JC.BY_NAME[name]
    vol = volume_of(eng, c)
    f = joint_field(eng, c, vol)
    per = per_goal_field(eng, c, vol)
    same(f.dist[0].cpu().numpy(), per.dist.min(dim=0).values.cpu().numpy(), f"bridge 1 {name}")
    owner = f.owner.cpu().numpy()
    iy, ix, iz = np.nonzero(owner >= 0)
    assert len(iy)
    same(f.dist[0].cpu().numpy()[iy, ix, iz],
         per.dist.cpu().numpy()[owner[iy, ix, iz], iy, ix, iz], f"owner property {name}")


@pytest.mark.parametrize("name", sorted(JC.SINGLE))
def test_one_goal_is_the_per_goal_field(eng, name):
    """Bridges 2 and 3 on the GPU."""
    c = JC.BY_NAME[name]
    vol = volume_of(eng, c)
    f = joint_field(eng, c, vol)
    per = per_goal_field(eng, c, vol)
    same(f.dist.cpu().numpy(), per.dist.cpu().numpy(), "bridge 2 dist")
    same(f.next.cpu().numpy(), per.next.cpu().numpy(), "bridge 2 next")
    gi = np.zeros(len(c["starts"]), dtype=np.int32)
    for span in JC.SPANS:
        o = eng.route_paths3d(f, c["starts"], smooth=span)
        p = eng.route_paths3d(per, c["starts"], gi, smooth=span)
        st = p["status"].cpu().numpy()
        assert not np.any(st == 4)
        same(o["status"].cpu().numpy(), st, f"bridge 3 status span {span}")
        same(o["steps"].cpu().numpy(), p["steps"].cpu().numpy(), f"bridge 3 steps span {span}")
        if span:
            same(o["vertices"].cpu().numpy(), p["vertices"].cpu().numpy(), f"vertices {span}")
        same(o["wp3"].cpu().numpy()[st == 0], p["wp3"].cpu().numpy()[st == 0], f"wp3 span {span}")


def test_one_context_runs_per_goal_joint_per_goal(eng):
    """A long-lived context running per-goal, joint, per-goal, per-goal smooth, joint smooth in
    turn: every result bit-exact, the per-goal bits before and after the joint calls identical
    (the joint call leaves nothing behind in the context or the shared kernels' state)."""
    name = "shared_and_invalid"
    c = JC.BY_NAME[name]
    vol = volume_of(eng, c)
    set_tile(eng, (8, 4), 4)
    gi = np.arange(len(c["starts"]), dtype=np.int32) % len(c["goals"])

    def per_goal(span):
        f = per_goal_field(eng, c, vol)
        o = eng.route_paths3d(f, c["starts"], gi, smooth=span)
        assert eng.last_kernel() == ("K9vs" if span else "K9vt")
        keys = ("wp3", "status", "steps") + (("vertices",) if span else ())
        return [f.dist.cpu().numpy(), f.next.cpu().numpy()] + [o[k].cpu().numpy() for k in keys]

    first = per_goal(0)
    f = joint_field(eng, c, vol, (8, 4), 4)
    check_field(f, name, "between the per-goal calls")
    check_paths(eng, f, name, "between the per-goal calls", spans=(0,))
    third = per_goal(0)
    for a, b in zip(first, third):
        same(a, b, "per-goal bits before and after the joint call")
    smooth = per_goal(7)
    check_paths(eng, f, name, "after the per-goal smoothing", spans=(7,))
    again = per_goal(7)
    for a, b in zip(smooth, again):
        same(a, b, "per-goal smoothed bits before and after the joint smoothing")
    same(smooth[0], first[0])
    with pytest.raises(ValueError, match="a joint RouteField3D takes no goal_idx"):
        eng.route_paths3d(f, c["starts"], gi)
    with pytest.raises(ValueError, match="goal_idx"):
        eng.route_paths3d(per_goal_field(eng, c, vol), c["starts"])


def test_second_stream_gives_the_same_bits(eng):
    name = "serpentine_ends"
    c = JC.BY_NAME[name]
    vol = volume_of(eng, c)
    torch.cuda.synchronize()
    with torch.cuda.stream(torch.cuda.Stream(eng.torch_device)):
        f = joint_field(eng, c, vol)
        check_field(f, name, "second stream")
        check_paths(eng, f, name, "second stream", spans=(0, 64))
    torch.cuda.synchronize()


def test_max_rounds_is_an_error_and_the_context_stays_usable(eng):
    from uam_path_planning_amd import _lib

    c = JC.BY_NAME["serpentine_ends"]
    vol = volume_of(eng, c)
    with pytest.raises(_lib.UamError, match="max_rounds") as ei:
        joint_field(eng, c, vol, (8, 8), 4, max_rounds=1)
    assert "status -4" in str(ei.value)           # UAM_E_STATE
    f = joint_field(eng, c, vol, (8, 8), 4)
    check_field(f, "serpentine_ends", "after the failed call")


def test_invalid_arguments_come_before_any_launch(eng):
    from uam_path_planning_amd import _lib

    name = "open_five"
    c = JC.BY_NAME[name]
    vol = volume_of(eng, c)
    per_goal_field(eng, c, vol)                   # leaves "K9v": no refused call may change it
    for kw in (dict(lam=float("nan")), dict(lam=-0.5), dict(inflate=9), dict(z_scale=0.0),
               dict(agl=-1.0)):
        with pytest.raises(ValueError):
            eng.route_field3d(vol, c["goals"], joint=True, **kw)
    with pytest.raises(ValueError, match="n_goals"):
        eng.route_field3d(vol, np.zeros((0, 3)), joint=True)
    gs = vol.geo.as_struct()
    rp = _lib.Route3dParams(_lib.ABI_VERSION, c["lam"], c["block_flags"], c["inflate"], 0,
                            c["agl"], c["kappa"])
    G = len(c["goals"])
    need = eng.lib.uam_route3d_joint_workspace_bytes(ctypes.byref(gs), ctypes.byref(rp), G)
    shape = (vol.geo.ny, vol.geo.nx, vol.geo.nz)
    FILL = 0x5A
    bufs = dict(vol=vol.buf, goals=eng.tensor(c["goals"], torch.float64),
                dist=eng.empty(shape, torch.float64), next=eng.empty(shape, torch.uint8),
                owner=eng.empty(shape, torch.int32),
                ws=eng.empty((need // 256 + 1, 256), torch.uint8))
    outs = ("dist", "next", "owner")

    def call(n_goals=G, ws_bytes=need, shift=None, **null):
        for k in outs:
            bufs[k].view(torch.uint8).fill_(FILL)
        p = {k: (None if k in null else v.data_ptr()) for k, v in bufs.items()}
        if shift:
            p[shift[0]] += shift[1]
        st = eng.lib.uam_route3d_field_joint(eng._ctx, ctypes.byref(gs), p["vol"],
                                             ctypes.byref(rp), p["goals"], n_goals, p["dist"],
                                             p["next"], p["owner"], p["ws"], ws_bytes, None,
                                             eng.stream)
        if st != _lib.UAM_OK:
            assert eng.last_kernel() == "K9v"
            eng.synchronize()
            for k in outs:
                assert bool((bufs[k].view(torch.uint8) == FILL).all()), k
        return st

    for k in bufs:
        assert call(**{k: True}) == _lib.UAM_E_INVALID, k
    for n in (0, 2 ** 20 + 1):
        assert call(n_goals=n) == _lib.UAM_E_INVALID
    assert call(ws_bytes=need - 1) == _lib.UAM_E_INVALID
    for shift in (("ws", 128), ("vol", 128), ("dist", 4), ("owner", 2)):
        assert call(shift=shift) == _lib.UAM_E_INVALID, shift
    assert call() == _lib.UAM_OK
    assert eng.last_kernel() == "K9vj"
    eng.synchronize()
    same(bufs["owner"].cpu().numpy(), JC.reference(name)["owner"], "raw call")

    f = joint_field(eng, c, vol)
    Q, N = len(c["starts"]), c["N"]
    pb = dict(vol=vol.buf, bits=eng.route_free_bits3d(f), next=f.next, owner=f.owner,
              goals=f.goals, starts=eng.tensor(c["starts"], torch.float64),
              wp=eng.empty((Q, N + 2, 3), torch.float64), status=eng.empty((Q,), torch.int32),
              steps=eng.empty((Q,), torch.int32), vertices=eng.empty((Q,), torch.int32),
              goal=eng.empty((Q,), torch.int32))
    pouts = ("wp", "status", "steps", "vertices", "goal")
    before = eng.last_kernel()
    assert before == "K9vb"

    def paths(span=7, n_goals=G, n_queries=Q, **null):
        for k in pouts:
            pb[k].view(torch.uint8).fill_(FILL)
        p = {k: (None if k in null else v.data_ptr()) for k, v in pb.items()}
        st = eng.lib.uam_route3d_paths_joint(
            eng._ctx, ctypes.byref(gs), p["vol"], ctypes.byref(rp), p["bits"], p["next"],
            p["owner"], p["goals"], n_goals, p["starts"], n_queries, span, p["wp"], p["status"],
            p["steps"], p["vertices"], p["goal"], eng.stream)
        if st != _lib.UAM_OK:
            assert eng.last_kernel() == before
            eng.synchronize()
            for k in pouts:
                assert bool((pb[k].view(torch.uint8) == FILL).all()), k
        return st

    for k in ("next", "owner", "goals", "starts", "wp", "status"):
        assert paths(**{k: True}) == _lib.UAM_E_INVALID, k
    assert paths(span=0, vol=True) == _lib.UAM_E_INVALID
    assert paths(span=1, bits=True) == _lib.UAM_E_INVALID
    for span in (-1, 1025):
        assert paths(span=span) == _lib.UAM_E_INVALID
    for n in (0, 2 ** 20 + 1):
        assert paths(n_goals=n) == _lib.UAM_E_INVALID
    assert paths(n_queries=-1) == _lib.UAM_E_INVALID
    assert paths(steps=True, vertices=True, goal=True) == _lib.UAM_OK     # each may be NULL
    eng.synchronize()
    same(pb["wp"].cpu().numpy(), JC.reference_paths(name, 7)["wp3"], "steps / vertices / goal NULL")
    assert paths(span=7, vol=True) == _lib.UAM_OK     # span >= 1 reads the bits, not the volume
    eng.synchronize()
    same(pb["wp"].cpu().numpy(), JC.reference_paths(name, 7)["wp3"], "span 7, vol NULL")
    assert paths(span=0, bits=True) == _lib.UAM_OK
    eng.synchronize()
    same(pb["goal"].cpu().numpy(), JC.reference_paths(name, 0)["goal"], "span 0, bits NULL")


def test_needs_params():
    """UAM_E_STATE without uam_set_params."""
    from uam_path_planning_amd import _lib
    from uam_path_planning_amd.engine import Engine, VolumeGeo

    e = Engine(0)
    gs = VolumeGeo(*JC.GEO).as_struct()
    rp = _lib.Route3dParams(_lib.ABI_VERSION, 1.0, 1, 0, 0, 0.0, 1e-3)
    one = e.empty((64,), torch.float64).data_ptr()
    assert e.lib.uam_route3d_paths_joint(e._ctx, ctypes.byref(gs), one, ctypes.byref(rp), one, one,
                                         one, one, 1, one, 1, 4, one, one, None, None, None,
                                         e.stream) == _lib.UAM_E_STATE
