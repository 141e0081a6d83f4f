"""Route seeds, smoothing (K9b / K9s) without a GPU: uam_route_free_bits_host /
uam_route_paths_smooth_host / uam_route_visible_host -- the inline functions the kernels run --
against tests/route_smooth_ref.py's independent statement, bit for bit, on every case of
tests/route_smooth_cases.py and every span; the tie cases; the symbols; the argument checks."""
import ctypes
import os
import re

import numpy as np
import pytest

import route_ref as R
import route_smooth_cases as SC
import route_smooth_ref as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = {}


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


def host_field(Engine, name):
    """The host twin's field of a case, once per process."""
    if name not in FIELDS:
        c = SC.BY_NAME[name]
        FIELDS[name] = Engine.route_field_host(engine_geo(c["geo"]), c["rec"], c["goals"],
                                               c["lam"], c["block_flags"], c["inflate"])
    return FIELDS[name]


def cell_id(cell):
    return cell[1] * SC.GEO.nx + cell[0]


def visible(geo, words, pairs):
    """uam_route_visible_host on ((ax, ay), (bx, by)) pairs."""
    from uam_path_planning_amd import _lib

    a = np.array([p[0][1] * geo.nx + p[0][0] for p in pairs], dtype=np.int32)
    b = np.array([p[1][1] * geo.nx + p[1][0] for p in pairs], dtype=np.int32)
    out = np.full(len(pairs), 7, dtype=np.uint8)
    words = np.ascontiguousarray(words, dtype=np.uint32)
    _lib.check(_lib.load().uam_route_visible_host(
        ctypes.byref(engine_geo(geo).as_struct()), words.ctypes.data, len(pairs), a.ctypes.data,
        b.ctypes.data, out.ctypes.data), "uam_route_visible_host")
    return out


@pytest.mark.parametrize("name", SC.NAMES)
def test_host_matches_reference(Engine, name):
    """wp, status, steps and vertices for every span; the free bits; span 1 = route_paths_host;
    every status-0 waypoint in a free cell of the reference's cost plane; S_m never longer than
    the unsmoothed path's."""
    c = SC.BY_NAME[name]
    _, _, wp0, status0, steps0, cost = SC.field_reference(name)
    f = host_field(Engine, name)
    assert np.array_equal(Engine.route_free_bits_host(f), SC.free_bits(name))
    plain = Engine.route_paths_host(f, c["starts"], c["goal_idx"], c["N"])
    length1 = SC.reference(name, 1)[4]
    for span in SC.SPANS:
        wp, status, steps, vertices, length = SC.reference(name, span)
        o = Engine.route_paths_host(f, c["starts"], c["goal_idx"], c["N"], smooth=span)
        what = f"{name} span {span}"
        assert np.array_equal(o["status"], status), what
        assert np.array_equal(o["steps"], steps), what
        assert np.array_equal(o["vertices"], vertices), (what, o["vertices"], vertices)
        assert np.array_equal(bits(o["wp"]), bits(wp)), what
        assert np.array_equal(status, status0) and np.array_equal(steps, steps0)
        if span == 1:
            for k in ("wp", "status", "steps"):
                assert np.array_equal(bits(o[k]), bits(plain[k])), k
            assert np.array_equal(bits(wp), bits(wp0))
        ok = np.flatnonzero(status == 0)
        assert np.all(vertices[status != 0] == 0) and np.all(vertices[ok] >= 2)
        assert np.all(vertices[ok] <= np.maximum(steps[ok], 2))
        # the triangle inequality, up to rounding
        assert np.all(length[ok] <= length1[ok] * (1.0 + 1e-12)), what
        for q in ok:
            for x, y in wp[q]:
                cell = R.cell_of(c["geo"], x, y)
                assert cell is not None and cost[cell[1]][cell[0]] != R.INF, (what, q)


def test_adjacent_chain_cells_are_visible():
    """The corner rule's consequence the anchors rest on, on every step of every query."""
    seen = 0
    for name in SC.NAMES:
        status, cost = SC.field_reference(name)[3], SC.field_reference(name)[5]
        for q in np.flatnonzero(status == 0):
            cells = SC.chain_of(name, q)
            for a, b in zip(cells, cells[1:]):
                assert S.los(cost, a, b), (name, q, a, b)
                seen += 1
    assert seen > 5000


def test_cases_reach_what_they_are_for():
    # the ties: the blocked cell is touched by equality alone, and nothing else hides B from A
    for name, ties in SC.TIES.items():
        cost = SC.field_reference(name)[5]
        for a, b, w in ties:
            dx, dy = b[0] - a[0], b[1] - a[1]
            assert cost[w[1]][w[0]] == R.INF and w in S.touched(a, b)
            assert 2 * abs(dx * (w[1] - a[1]) - dy * (w[0] - a[0])) == abs(dx) + abs(dy)
            assert [t for t in S.touched(a, b) if cost[t[1]][t[0]] == R.INF] == [w]
            assert not S.los(cost, a, b)
    # (0,0) -> (3,1) touches (1,0), (2,0), (1,1), (2,1)
    assert set(S.touched((0, 0), (3, 1))) == {(0, 0), (1, 0), (2, 0), (1, 1), (2, 1), (3, 1)}
    # the gap is threaded, and smoothing uses it: far fewer vertices than cells
    cost = SC.field_reference("one_cell_gap")[5]
    for a, b in SC.THREADS["one_cell_gap"]:
        assert S.los(cost, a, b) and any(t == (50, 38) for t in S.touched(a, b))
    _, status, steps, vertices, _ = SC.reference("one_cell_gap", 64)
    assert np.all(status == 0) and vertices[0] == 4 and steps[0] == 11
    # the staircase: c_3 hidden from c_1, c_4 in sight again, and the anchor after c_1 is c_2
    cells = SC.chain_of("staircase", 0)
    assert cells[:5] == [(39, 30), (40, 30), (41, 30), (41, 31), (42, 31)]
    cost = SC.field_reference("staircase")[5]
    assert S.los(cost, cells[1], cells[2]) and not S.los(cost, cells[1], cells[3])
    assert S.los(cost, cells[1], cells[4])
    for span in (3, 7, 1024):
        assert S.anchors(cost, cells, span)[:2] == [1, 2]
    # s = g, adjacent cells, n = 3 and 4
    _, status, steps, vertices, _ = SC.reference("short_chains", 64)
    assert list(status) == [0] * 7 and list(steps) == [1, 2, 2, 3, 3, 3, 4]
    assert list(vertices) == [2, 2, 2, 3, 3, 3, 4]
    # smoothing does something: the spiral's vertices drop by more than an order of magnitude,
    # the open field's to a handful
    assert SC.reference("spiral", 1)[3][0] > 2000 > 100 > SC.reference("spiral", 64)[3][0] > 30
    v = SC.reference("open", 1024)[3]
    assert np.all(v[:6] <= 6) and np.any(SC.reference("open", 1)[3][:6] > 20)
    # 64 / 65 differ somewhere (a run of more than 64 visible cells exists)
    assert any(not np.array_equal(SC.reference(n, 64)[3], SC.reference(n, 65)[3])
               for n in SC.NAMES)


def test_visible_host_matches_brute_force():
    rng = np.random.default_rng(9)
    for name in ("random30", "inflate_1", "tie_slope1", "tie_slope13", "one_cell_gap", "comb"):
        c = SC.BY_NAME[name]
        geo = c["geo"]
        cost = SC.field_reference(name)[5]
        words = SC.free_bits(name)
        pairs = []
        for reach in (3, 12, 100):
            for _ in range(300):
                ax, ay = int(rng.integers(geo.nx)), int(rng.integers(geo.ny))
                bx = int(np.clip(ax + rng.integers(-reach, reach + 1), 0, geo.nx - 1))
                by = int(np.clip(ay + rng.integers(-reach, reach + 1), 0, geo.ny - 1))
                pairs.append(((ax, ay), (bx, by)))
        pairs += [(a, b) for a, b, _ in SC.TIES.get(name, [])] + SC.THREADS.get(name, [])
        want = np.array([S.los(cost, a, b) for a, b in pairs], dtype=np.uint8)
        got = visible(geo, words, pairs)
        assert np.array_equal(got, want), (name, [p for p, g, w in zip(pairs, got, want) if g != w])
        assert 0 < want.sum() < len(want)
    # beyond the largest span the walk runs in 64-bit integers: a 3000 x 2 strip
    geo = SC.C.Geo(3000, 2, 0.0, 1.0, 0.01, 0.01)
    cost = [[1.0] * 3000 for _ in range(2)]
    words = np.full((2, 94), 0xFFFFFFFF, dtype=np.uint32)
    pairs = [((0, 0), (2999, 1)), ((2999, 0), (0, 1)), ((5, 1), (2900, 1))]
    assert list(visible(geo, words, pairs)) == [1, 1, 1]
    words[1, 1500 // 32] &= ~np.uint32(1 << (1500 % 32))
    cost[1][1500] = R.INF
    assert list(visible(geo, words, pairs)) == [int(S.los(cost, a, b)) for a, b in pairs]
    assert list(visible(geo, words, pairs)) == [0, 0, 0]


def test_symbols():
    """The header, _lib.SIGNATURES and the built library agree on the new symbols."""
    from uam_path_planning_amd import _lib, build

    build.build_library()
    lib = _lib.load()
    with open(os.path.join(ROOT, "include", "uampath.h")) as f:
        text = f.read()
    vp, i32, i64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64
    desc, rp = ctypes.POINTER(_lib.RasterDesc), ctypes.POINTER(_lib.RouteParams)
    want = {
        "uam_route_free_bits_bytes": (i64, [desc]),
        "uam_route_free_bits": (ctypes.c_int, [vp, desc, vp, rp, vp, vp]),
        "uam_route_paths_smooth": (ctypes.c_int, [vp, desc, vp, vp, vp, i32, vp, vp, i64, i32,
                                                  vp, vp, vp, vp, vp]),
        "uam_route_free_bits_host": (ctypes.c_int, [desc, vp, rp, vp]),
        "uam_route_paths_smooth_host": (ctypes.c_int, [desc, vp, vp, vp, i32, vp, vp, i64, i32,
                                                       i32, vp, vp, vp, vp]),
        "uam_route_visible_host": (ctypes.c_int, [desc, vp, i64, vp, vp, vp]),
    }
    for name, sig in want.items():
        assert _lib.SIGNATURES[name] == sig, name
        assert hasattr(lib, name), name
        m = re.search(r"^(?:int|int64_t)\s+" + name + r"\s*\(([^;]*)\);", text, re.M)
        assert m, name
        assert len(m.group(1).split(",")) == len(sig[1]), name
    assert re.search(r"#define UAM_ROUTE_SPAN_MAX %d\b" % _lib.ROUTE_SPAN_MAX, text)
    assert re.search(r"#define UAM_ROUTE_SMOOTH_LIST %d\b" % _lib.ROUTE_SMOOTH_LIST, text)
    assert _lib.ROUTE_SPAN_MAX == S.SPAN_MAX
    assert "#define UAM_ABI_VERSION 2" in text and _lib.ABI_VERSION == 2
    assert '"K9b"' in text and '"K9s"' in text


def test_invalid_arguments(Engine):
    """The status codes of the refused calls, on the host and before any device is touched."""
    from uam_path_planning_amd import _lib

    lib = _lib.load()
    c = SC.BY_NAME["open"]
    f = host_field(Engine, "open")
    gd = engine_geo(c["geo"]).as_struct()
    ny, nx = c["geo"].ny, c["geo"].nx
    assert lib.uam_route_free_bits_bytes(ctypes.byref(gd)) == ny * ((nx + 31) // 32) * 4
    bad_desc = _lib.RasterDesc(0, 76, 0.0, 1.0, 0.1, 0.1, -9999.0, 0.0)
    assert lib.uam_route_free_bits_bytes(ctypes.byref(bad_desc)) == -1
    assert lib.uam_route_free_bits_bytes(None) == -1
    words = Engine.route_free_bits_host(f).copy()
    rec = np.ascontiguousarray(c["rec"])

    def params(lam=1.0, inflate=0, abi=_lib.ABI_VERSION):
        return _lib.RouteParams(abi, lam, 1, inflate, 0)

    def fb(p, r=rec.ctypes.data, b=words.ctypes.data, desc=gd):
        return lib.uam_route_free_bits_host(ctypes.byref(desc), r, ctypes.byref(p), b)

    assert fb(params()) == _lib.UAM_OK
    assert fb(params(lam=float("nan"))) == _lib.UAM_E_INVALID
    assert fb(params(inflate=9)) == _lib.UAM_E_INVALID
    assert fb(params(abi=1)) == _lib.UAM_E_VERSION
    assert fb(params(), r=None) == _lib.UAM_E_INVALID
    assert fb(params(), b=None) == _lib.UAM_E_INVALID
    assert fb(params(), desc=bad_desc) == _lib.UAM_E_INVALID

    Q, N = len(c["starts"]), c["N"]
    bufs = dict(bits=words, next=f.next, goals=f.goals, starts=c["starts"],
                gi=c["goal_idx"], wp=np.empty((Q, N + 2, 2)), status=np.empty(Q, np.int32),
                steps=np.empty(Q, np.int32), vertices=np.empty(Q, np.int32))

    def smooth(span=7, n_goals=1, n_queries=Q, n=N, desc=gd, **null):
        p = {k: (None if k in null else v.ctypes.data) for k, v in bufs.items()}
        return lib.uam_route_paths_smooth_host(
            ctypes.byref(desc), p["bits"], p["next"], p["goals"], n_goals, p["starts"], p["gi"],
            n_queries, n, span, p["wp"], p["status"], p["steps"], p["vertices"])

    assert smooth() == _lib.UAM_OK
    assert smooth(steps=True, vertices=True) == _lib.UAM_OK        # both may be NULL
    for span in (0, -1, 1025):
        assert smooth(span=span) == _lib.UAM_E_INVALID
        assert b"span" in lib.uam_last_error()
    assert smooth(span=1024) == _lib.UAM_OK
    assert smooth(n_goals=0) == _lib.UAM_E_INVALID
    assert smooth(n_queries=-1) == _lib.UAM_E_INVALID
    assert smooth(n=-1) == _lib.UAM_E_INVALID
    assert smooth(desc=bad_desc) == _lib.UAM_E_INVALID
    # chain indices are int32: a raster of 2^31 - 1 cells is a raster, but not one to smooth on
    huge = _lib.RasterDesc(2 ** 31 - 1, 1, 0.0, 1.0, 0.1, 0.1, -9999.0, 0.0)
    assert lib.uam_route_free_bits_bytes(ctypes.byref(huge)) == 2 ** 26 * 4
    assert smooth(desc=huge) == _lib.UAM_E_INVALID
    assert b"2^31" in lib.uam_last_error()
    for k in ("bits", "next", "goals", "starts", "gi", "wp", "status"):
        assert smooth(**{k: True}) == _lib.UAM_E_INVALID, k
    assert smooth(n_queries=0, wp=True) == _lib.UAM_OK
    with pytest.raises(ValueError, match="span"):
        Engine.route_paths_host(f, c["starts"], c["goal_idx"], N, smooth=2000)

    one = np.zeros(1, dtype=np.int32)
    out = np.zeros(1, dtype=np.uint8)

    def vis(a=one.ctypes.data, b=one.ctypes.data, o=out.ctypes.data, w=words.ctypes.data, n=1):
        return lib.uam_route_visible_host(ctypes.byref(gd), w, n, a, b, o)

    assert vis() == _lib.UAM_OK
    for kw in ("a", "b", "o", "w"):
        assert vis(**{kw: None}) == _lib.UAM_E_INVALID
    assert vis(n=-1) == _lib.UAM_E_INVALID
    off = np.array([nx * ny], dtype=np.int32)
    assert vis(a=off.ctypes.data) == _lib.UAM_E_INVALID
    neg = np.array([-1], dtype=np.int32)
    assert vis(b=neg.ctypes.data) == _lib.UAM_E_INVALID
    # the device calls refuse the same before they touch a device
    assert lib.uam_route_free_bits(None, None, None, None, None, None) == _lib.UAM_E_INVALID
    assert lib.uam_route_paths_smooth(None, None, None, None, None, 1, None, None, 0, 1, None,
                                      None, None, None, None) == _lib.UAM_E_INVALID
