"""Route seeds in the volume (K9v) without a GPU: uam_route3d_field_host /
uam_route3d_paths_host -- the inline functions the kernels run -- against tests/route3d_ref.py's
independent statement of the definition, bit for bit, on every case of tests/route3d_cases.py;
route3d_ref's Dijkstra itself against a brute-force Bellman-Ford; what the cases are there to
reach, from the reference alone; the bridge to the flat route seeds; the argument checks."""
import ctypes

import numpy as np
import pytest

import route3d_cases as C
import route3d_ref as R


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype == np.float64 else a


def engine_geo(geo):
    from uam_path_planning_amd.engine import VolumeGeo

    return VolumeGeo(*geo)


@pytest.fixture(scope="module")
def Engine():
    from uam_path_planning_amd import build
    from uam_path_planning_amd.engine import Engine

    build.build_library()
    return Engine


def host_field(Engine, c):
    return Engine.route_field3d_host(engine_geo(c["geo"]), C.volume_words(c), c["goals"],
                                     c["lam"], c["block_flags"], c["inflate"], c["agl"],
                                     c["kappa"])


@pytest.mark.parametrize("name", C.NAMES)
def test_host_matches_reference(Engine, name):
    c = C.BY_NAME[name]
    dist, nxt, wp, status, steps, _ = C.reference(name)
    f = host_field(Engine, c)
    assert np.array_equal(bits(f.dist), bits(dist))
    assert np.array_equal(f.next, nxt)
    o = Engine.route_paths3d_host(f, c["starts"], c["goal_idx"], c["N"])
    assert np.array_equal(o["status"], status), (o["status"], status)
    assert np.array_equal(o["steps"], steps)
    assert np.array_equal(bits(o["wp3"]), bits(wp))


def layers_of(c, wp):
    """The layer of every waypoint of one path."""
    return [R.voxel_of(c["geo"], *p)[2] for p in wp]


def test_cases_reach_what_they_are_there_for():
    """From the reference alone (a reference that agreed with the library on nothing but
    straight lines would be noticed)."""
    seen = set()
    for name in C.NAMES:
        seen |= set(C.reference(name)[3].tolist())
    assert {0, 1, 2, 4} <= seen
    assert list(C.reference("sealed_box")[3]) == [2, 2, 2, 2]
    dist, nxt, _, st, _, _ = C.reference("blocked_goal_and_offvolume_goal")
    assert np.all(np.isinf(dist)) and np.all(nxt == R.NONE) and list(st) == [4] * 5
    st = C.reference("open3d")[3]
    assert list(st[-4:]) == [1, 1, 1, 1] and np.all(st[:-4] == 0)
    # in the goal voxel, then face-, edge- and corner-adjacent to it
    assert list(C.reference("open3d")[4][5:9]) == [1, 2, 2, 2]
    st = C.reference("three_goals")[3]
    assert st[3] == 4 and st[4] == 4
    # the ridge: every route climbs to a layer whose centre clears it
    c = C.BY_NAME["ridge"]
    _, _, wp, st, _, _ = C.reference("ridge")
    top = float(c["terrain"].max())
    clear = min(iz for iz in range(c["geo"].nz) if not C.layer_centre(iz) < top)
    assert clear == 6 and np.all(st == 0)
    for q in range(len(wp)):
        lay = layers_of(c, wp[q])
        assert max(lay) >= clear and lay[0] < clear and lay[-1] < clear, (q, lay)
    # risk falling with altitude: the routes peak in different layers at the two lambdas
    _, _, wp0, st0, _, _ = C.reference("layer_tradeoff_lam0")
    _, _, wp50, st50, _, _ = C.reference("layer_tradeoff_lam50")
    assert np.all(st0 == 0) and np.all(st50 == 0)
    for q in range(len(wp0)):
        lo = max(layers_of(C.BY_NAME["layer_tradeoff_lam0"], wp0[q]))
        hi = max(layers_of(C.BY_NAME["layer_tradeoff_lam50"], wp50[q]))
        assert hi > lo, (q, lo, hi)
    # the diagonal sheet holds under the box rule: every route from its far side passes the
    # one gap, so the start one diagonal step from the near side walks a long way round
    c = C.BY_NAME["diagonal_sheet"]
    dist, nxt, _, st, steps, _ = C.reference("diagonal_sheet")
    assert np.all(st == 0)
    gap = (17, 20, 3)
    for q in (0, 1, 3, 4):
        v = R.voxel_of(c["geo"], *c["starts"][q])
        chain = [v]
        while nxt[0][v[1], v[0], v[2]] != R.GOAL:
            d = R.DIRS[int(nxt[0][v[1], v[0], v[2]])]
            v = (v[0] + d[0], v[1] + d[1], v[2] + d[2])
            chain.append(v)
        assert gap in chain and len(chain) == steps[q], q
    assert steps[2] < steps[1]                # the start already past the sheet


def test_waypoints_lie_in_free_voxels():
    """The box rule's consequence: every waypoint of a status-0 path lies in a free voxel."""
    for name in C.NAMES:
        c = C.BY_NAME[name]
        _, _, wp, status, _, cost = C.reference(name)
        for q in np.flatnonzero(status == 0):
            for p in wp[q]:
                v = R.voxel_of(c["geo"], *p)
                assert v is not None and cost[v[1]][v[0]][v[2]] != R.INF, (name, q)


def bellman_ford(geo, c, L, g):
    """Brute force: sweeps of d[v] = min(d[v], d[u] + w) over every voxel and direction, the
    box rule spelled out, until nothing changes."""
    nx, ny, nz = geo.nx, geo.ny, geo.nz
    d = np.full((ny, nx, nz), R.INF)
    d[g[1], g[0], g[2]] = 0.0
    changed = True
    while changed:
        changed = False
        for iy in range(ny):
            for ix in range(nx):
                for iz in range(nz):
                    if c[iy][ix][iz] == R.INF:
                        continue
                    for k, (a, b, e) in enumerate(R.DIRS):
                        ux, uy, uz = ix + a, iy + b, iz + e
                        if not (0 <= ux < nx and 0 <= uy < ny and 0 <= uz < nz):
                            continue
                        box = [(x, y, z) for x in (ix, ux) for y in (iy, uy) for z in (iz, uz)]
                        if any(c[y][x][z] == R.INF for x, y, z in box):
                            continue
                        t = float(d[uy, ux, uz]) + (0.5 * (c[uy][ux][uz] + c[iy][ix][iz])) * L[k]
                        if t < d[iy, ix, iz]:
                            d[iy, ix, iz] = t
                            changed = True
    return d


@pytest.mark.parametrize("name", ["random30", "nonfinite_risk", "open3d"])
def test_reference_dijkstra_against_bellman_ford(name):
    c = C.BY_NAME[name]
    g0 = c["geo"]
    geo = C.Geo(10, 8, 5, g0.x0, g0.y_top, g0.dx, g0.dy, g0.z0, g0.dz)
    cost = R.cost_volume(geo, c["risk"][:8, :10, :5], c["terrain"][:8, :10], c["flags"][:8, :10],
                         c["lam"], c["block_flags"], 0, c["agl"])
    free = [(ix, iy, iz) for iy in range(8) for ix in range(10) for iz in range(5)
            if cost[iy][ix][iz] != R.INF]
    g = free[len(free) // 2]
    dist, _ = R.field(geo, cost, R.centre(geo, *g), c["kappa"])
    ref = bellman_ford(geo, cost, R.step_lengths(geo, c["kappa"]), g)
    assert np.array_equal(bits(dist), bits(ref))
    assert np.isfinite(dist).sum() > 10


def test_nz1_bridge_to_the_flat_route_seeds(Engine):
    """One layer above every terrain value, layer_w = 1, agl = 0: dist is uam_route_field's bit
    for bit and next agrees wherever the flat value is a direction."""
    from uam_path_planning_amd.engine import RasterGeo

    c = C.BY_NAME["nz1_bridge"]
    g = c["geo"]
    assert g.nz == 1 and c["agl"] == 0.0 and C.layer_centre(0, g) > float(c["terrain"].max())
    rec = np.zeros((g.ny, g.nx, 4), dtype=np.uint32)
    rec[..., 0] = c["risk"][:, :, 0].view(np.uint32)
    rec[..., 2] = c["terrain"].view(np.uint32)
    rec[..., 3] = c["flags"]
    flat = Engine.route_field_host(RasterGeo(g.nx, g.ny, g.x0, g.y_top, g.dx, g.dy), rec,
                                   c["goals"][:, :2], c["lam"], c["block_flags"], c["inflate"])
    f = host_field(Engine, c)
    assert np.array_equal(bits(f.dist[..., 0]), bits(flat.dist))
    assert np.isfinite(flat.dist).sum() > 500
    dirs = flat.next < 8
    assert dirs.sum() > 500 and np.array_equal(f.next[..., 0][dirs], flat.next[dirs])
    assert np.array_equal(f.next[..., 0] == 26, flat.next == 8)
    assert np.array_equal(f.next[..., 0] == 255, flat.next == 255)


def test_invalid_arguments():
    """UAM_E_INVALID on the host, before anything runs."""
    from uam_path_planning_amd import _lib

    lib = _lib.load()
    c = C.BY_NAME["open3d"]
    gd = engine_geo(c["geo"]).as_struct()
    n = c["geo"].nx * c["geo"].ny * c["geo"].nz
    dist = np.empty(n)
    nxt = np.empty(n, dtype=np.uint8)
    vol, goals = C.volume_words(c), c["goals"]
    inf, nan = float("inf"), float("nan")

    def params(lam=1.0, inflate=0, max_rounds=0, agl=0.0, z_scale=1e-3, abi=_lib.ABI_VERSION):
        return _lib.Route3dParams(abi, lam, 1, inflate, max_rounds, agl, z_scale)

    def field(p, n_goals=1, v=vol.ctypes.data, g=goals.ctypes.data, d=dist.ctypes.data,
              x=nxt.ctypes.data, desc=gd):
        return lib.uam_route3d_field_host(ctypes.byref(desc), v, ctypes.byref(p), g, n_goals, d,
                                          x)

    assert field(params()) == _lib.UAM_OK
    for bad in (params(lam=nan), params(lam=-1.0), params(lam=inf), params(inflate=9),
                params(inflate=-1), params(max_rounds=-1), params(agl=nan), params(agl=-1.0),
                params(agl=inf), params(z_scale=0.0), params(z_scale=-1e-3),
                params(z_scale=nan), params(z_scale=inf)):
        assert field(bad) == _lib.UAM_E_INVALID
        assert lib.uam_route3d_workspace_bytes(ctypes.byref(gd), ctypes.byref(bad)) == -1
    assert field(params(abi=1)) == _lib.UAM_E_VERSION
    assert field(params(), n_goals=0) == _lib.UAM_E_INVALID
    assert b"n_goals" in lib.uam_last_error()
    for kw in ("v", "g", "d", "x"):
        assert field(params(), **{kw: None}) == _lib.UAM_E_INVALID
    bad_desc = _lib.VolumeDesc(0, 29, 11, 0.0, 1.0, 0.1, 0.1, 0.0, 10.0)
    assert field(params(), desc=bad_desc) == _lib.UAM_E_INVALID
    # n_goals * voxels >= 2^40
    big = _lib.VolumeDesc(1024, 1024, 1024, 0.0, 1.0, 0.1, 0.1, 0.0, 10.0)
    assert field(params(), n_goals=1024, desc=big) == _lib.UAM_E_INVALID
    assert lib.uam_route3d_workspace_bytes(ctypes.byref(gd), ctypes.byref(params())) > n * 12
    st = np.zeros(1, dtype=np.int32)
    wp = np.empty((C.N + 2) * 3)
    start = np.array(C.pt(1, 1, 1))
    gi = np.zeros(1, dtype=np.int32)

    def paths(p=params(), Q=1, N=C.N, v=vol.ctypes.data, x=nxt.ctypes.data,
              w=wp.ctypes.data):
        return lib.uam_route3d_paths_host(ctypes.byref(gd), v, ctypes.byref(p), x,
                                          goals.ctypes.data, 1, start.ctypes.data,
                                          gi.ctypes.data, Q, N, w, st.ctypes.data, None)

    assert paths() == _lib.UAM_OK and st[0] == 0
    assert paths(Q=0, w=None) == _lib.UAM_OK
    assert paths(Q=-1) == _lib.UAM_E_INVALID and paths(N=-1) == _lib.UAM_E_INVALID
    assert paths(v=None) == _lib.UAM_E_INVALID and paths(x=None) == _lib.UAM_E_INVALID
    assert paths(w=None) == _lib.UAM_E_INVALID
    assert paths(p=params(z_scale=0.0)) == _lib.UAM_E_INVALID
    # the device calls refuse the same before they touch a device
    assert lib.uam_route3d_field(None, None, None, None, None, 1, None, None, None, 0, None,
                                 None) == _lib.UAM_E_INVALID
    assert lib.uam_route3d_paths(None, None, None, None, None, None, 1, None, None, 0, None,
                                 None, None, None) == _lib.UAM_E_INVALID
    assert lib.uam_route3d_visits(None) == 0


def test_option_names():
    from uam_path_planning_amd import _lib

    assert _lib.ROUTE3D_OPTIONS == {"k9v_tile_xy": 29, "k9v_tile_z": 30, "k9v_inner": 31}
    keys = set(_lib.ROUTE3D_OPTIONS.values())
    assert not keys & set(_lib.OPTIONS.values()) and not keys & set(_lib.ROUTE_OPTIONS.values())
    assert not set(_lib.ROUTE3D_OPTIONS) & (set(_lib.OPTIONS) | set(_lib.ROUTE_OPTIONS))
