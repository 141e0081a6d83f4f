"""Route seeds (K9) without a GPU: uam_route_field_host / uam_route_paths_host -- the inline
functions the kernels run -- against tests/route_ref.py's independent statement of the
definition, bit for bit, on every case of tests/route_cases.py; route_ref's Dijkstra itself
against a brute-force Bellman-Ford; the calls' argument checks."""
import ctypes

import numpy as np
import pytest

import route_cases as C
import route_ref as R


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype == np.float64 else a


def engine_geo(geo):
    from uam_path_planning_amd.engine import RasterGeo

    return RasterGeo(geo.nx, geo.ny, geo.x0, geo.y_top, geo.dx, geo.dy)


@pytest.fixture(scope="module")
def Engine():
    from uam_path_planning_amd import build
    from uam_path_planning_amd.engine import Engine

    build.build_library()
    return Engine


@pytest.mark.parametrize("name", C.NAMES)
def test_host_matches_reference(Engine, name):
    c = C.BY_NAME[name]
    dist, nxt, wp, status, steps, _ = C.reference(name)
    f = Engine.route_field_host(engine_geo(c["geo"]), c["rec"], c["goals"], c["lam"],
                                c["block_flags"], c["inflate"])
    assert np.array_equal(bits(f.dist), bits(dist))
    assert np.array_equal(f.next, nxt)
    o = Engine.route_paths_host(f, c["starts"], c["goal_idx"], c["N"])
    assert np.array_equal(o["status"], status), (o["status"], status)
    assert np.array_equal(o["steps"], steps)
    assert np.array_equal(bits(o["wp"]), bits(wp))


def test_cases_cover_every_status():
    """The cases reach what they are there for (so a reference that agreed with the library on
    nothing but straight lines would be noticed)."""
    seen = set()
    for name in C.NAMES:
        seen |= set(C.reference(name)[3].tolist())
    assert {0, 1, 2, 4} <= seen
    st = C.reference("sealed_ring")[3]
    assert list(st) == [2, 2, 2, 2]
    dist, nxt, _, st, _, _ = C.reference("blocked_and_offmap_goal")
    assert np.all(np.isinf(dist)) and np.all(nxt == 255) and list(st) == [4, 4, 4, 4]
    assert list(C.reference("blocked_start")[3]) == [1, 1, 0]
    st = C.reference("open")[3]
    assert list(st[-3:]) == [1, 1, 1] and np.all(st[:-3] == 0)
    assert list(C.reference("open")[4][6:9]) == [1, 2, 2]     # in the goal cell, adjacent
    st = C.reference("three_goals")[3]
    assert st[3] == 4 and st[4] == 4
    # the diagonal wall holds: the start one diagonal step from the far side walks round
    # through the gap
    _, _, _, st, steps, _ = C.reference("diagonal_wall")
    assert np.all(st == 0) and steps[3] > 30
    # the spiral's walk is long
    assert C.reference("spiral")[4][0] > 1500 and C.reference("spiral")[3][0] == 0
    assert set(C.reference("absorption")[3].tolist()) <= {0, 3}


def test_waypoints_lie_in_free_cells():
    """The corner rule's consequence: every waypoint of a status-0 path lies in a free cell."""
    for name in C.NAMES:
        c = C.BY_NAME[name]
        _, _, wp, status, _, cost = C.reference(name)
        for q in np.flatnonzero(status == 0):
            for x, y in wp[q]:
                cell = R.cell_of(c["geo"], x, y)
                assert cell is not None and cost[cell[1]][cell[0]] != R.INF, (name, q)


def bellman_ford(c, L, nx, ny, g):
    """Brute force on the corner [0, nx) x [0, ny) of a cost plane: sweeps of
    d[v] = min(d[v], d[u] + w) over every cell and direction until nothing changes."""
    d = [[R.INF] * nx for _ in range(ny)]
    d[g[1]][g[0]] = 0.0
    changed = True
    while changed:
        changed = False
        for iy in range(ny):
            for ix in range(nx):
                if c[iy][ix] == R.INF:
                    continue
                for k, (dix, diy) in enumerate(R.DIRS):
                    ux, uy = ix + dix, iy + diy
                    if not (0 <= ux < nx and 0 <= uy < ny) or c[uy][ux] == R.INF:
                        continue
                    if dix and diy and (c[iy][ux] == R.INF or c[uy][ix] == R.INF):
                        continue
                    t = d[uy][ux] + (0.5 * (c[uy][ux] + c[iy][ix])) * L[k]
                    if t < d[iy][ix]:
                        d[iy][ix] = t
                        changed = True
    return np.array(d)


@pytest.mark.parametrize("name", ["random30", "nonfinite_phi", "open"])
def test_reference_dijkstra_against_bellman_ford(name):
    c = C.BY_NAME[name]
    nx, ny = 12, 9
    geo = C.Geo(nx, ny, c["geo"].x0, c["geo"].y_top, c["geo"].dx, c["geo"].dy)
    rec = np.ascontiguousarray(c["rec"][:ny, :nx]).view(np.uint32)
    cost = R.cost_plane(geo, rec, c["lam"], c["block_flags"], 0)
    free = [(ix, iy) for iy in range(ny) for ix in range(nx) if cost[iy][ix] != R.INF]
    g = free[len(free) // 2]
    goal = (geo.x0 + (g[0] + 0.5) * geo.dx, geo.y_top - (g[1] + 0.5) * geo.dy)
    dist, _ = R.field(geo, cost, goal)
    ref = bellman_ford(cost, R.step_lengths(geo), nx, ny, g)
    assert np.array_equal(bits(dist), bits(ref))
    assert np.isfinite(dist).sum() > 10


def test_invalid_arguments():
    """UAM_E_INVALID on the host, before anything runs."""
    from uam_path_planning_amd import _lib

    lib = _lib.load()
    c = C.BY_NAME["open"]
    gd = engine_geo(c["geo"]).as_struct()
    n = c["geo"].nx * c["geo"].ny
    dist = np.empty(n)
    nxt = np.empty(n, dtype=np.uint8)
    rec, goals = c["rec"], c["goals"]

    def params(lam=1.0, inflate=0, max_rounds=0, abi=_lib.ABI_VERSION):
        return _lib.RouteParams(abi, lam, 1, inflate, max_rounds)

    def field(p, n_goals=1, r=rec.ctypes.data, g=goals.ctypes.data, d=dist.ctypes.data,
              x=nxt.ctypes.data, desc=gd):
        return lib.uam_route_field_host(ctypes.byref(desc), r, ctypes.byref(p), g, n_goals, d, x)

    assert field(params()) == _lib.UAM_OK
    for bad in (params(lam=float("nan")), params(lam=-1.0), params(lam=float("inf")),
                params(inflate=9), params(inflate=-1), params(max_rounds=-1)):
        assert field(bad) == _lib.UAM_E_INVALID
        assert lib.uam_route_workspace_bytes(ctypes.byref(gd), ctypes.byref(bad)) == -1
    assert field(params(abi=1)) == _lib.UAM_E_VERSION
    assert field(params(), n_goals=0) == _lib.UAM_E_INVALID
    assert b"n_goals" in lib.uam_last_error()
    for kw in ("r", "g", "d", "x"):
        assert field(params(), **{kw: None}) == _lib.UAM_E_INVALID
    bad_desc = _lib.RasterDesc(0, 76, 0.0, 1.0, 0.1, 0.1, -9999.0, 0.0)
    assert field(params(), desc=bad_desc) == _lib.UAM_E_INVALID
    assert lib.uam_route_workspace_bytes(ctypes.byref(gd), ctypes.byref(params())) > n * 8
    # the device calls refuse the same before they touch a device
    assert lib.uam_route_field(None, None, None, None, None, 1, None, None, None, 0, None,
                               None) == _lib.UAM_E_INVALID
    assert lib.uam_route_paths(None, None, None, None, None, None, 1, None, None, 0, None, None,
                               None, None) == _lib.UAM_E_INVALID
    assert lib.uam_route_visits(None) == 0
    assert _lib.ROUTE_OPTIONS == {"k9_tile": 27, "k9_inner": 28}
    assert not set(_lib.ROUTE_OPTIONS.values()) & set(_lib.OPTIONS.values())
