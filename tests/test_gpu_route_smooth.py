"""Route seeds, smoothing (K9b / K9s) on the GPU: uam_route_free_bits / uam_route_paths_smooth
against tests/route_smooth_ref.py (and hence the host twin, tests/test_route_smooth_cpu.py) bit
for bit on wp, status, steps and vertices, for every case and span; the launch shapes (one
query, several workgroups with a partial last one, many 64-candidate batches, an anchor list
that overflows); then, with no reference involved, the seeds under eval_waypoints and the
analytic wall end to end; the error paths.

Cases: tests/route_smooth_cases.py."""
import ctypes

import numpy as np
import pytest

import route_cases as C
import route_smooth_cases as SC
import route_smooth_ref as S
from test_gpu_route import WALL, WALL_PAIRS

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


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
    e.set_geometry(compile_map(build_region_map(WALL)))
    e.set_params(PathParams(N=C.N_DEFAULT, **WALL["options"], maxratio=WALL["maxratio"],
                            maxalpha=WALL["maxalpha"], enlargement=0.0, weights=()))
    return e


FIELDS = {}


def field_of(eng, name):
    """(raster, RouteField) of a case, once per process; the field is test_gpu_route.py's
    subject and is checked against the reference's next here only."""
    if name not in FIELDS:
        from uam_path_planning_amd.engine import CostRaster, RasterGeo

        c = SC.BY_NAME[name]
        g = c["geo"]
        rec = torch.from_numpy(c["rec"].view(np.int32).copy()).to(eng.torch_device)
        raster = CostRaster(RasterGeo(g.nx, g.ny, g.x0, g.y_top, g.dx, g.dy), rec)
        eng.set_option("k9_tile", 32)
        eng.set_option("k9_inner", 32)
        f = eng.route_field(raster, c["goals"], c["lam"], c["block_flags"], c["inflate"])
        same(f.next.cpu().numpy(), SC.field_reference(name)[1], f"next {name}")
        FIELDS[name] = raster, f
    return FIELDS[name]


def check(o, name, span, what=""):
    wp, status, steps, vertices, _ = SC.reference(name, span)
    what = f"{name} span {span} {what}"
    same(o["status"].cpu().numpy(), status, f"status {what}")
    same(o["steps"].cpu().numpy(), steps, f"steps {what}")
    same(o["vertices"].cpu().numpy(), vertices, f"vertices {what}")
    same(o["wp"].cpu().numpy(), wp, f"wp {what}")


@pytest.mark.parametrize("name", SC.NAMES)
def test_matches_reference_for_every_span(eng, name):
    """The bits built by uam_route_free_bits are the reference's and the host twin's; one bit
    pattern per case and span; span 1 is route_paths; and, with no reference involved, every
    status-0 path clears the no-fly cells and the raster."""
    from uam_path_planning_amd.engine import Engine

    c = SC.BY_NAME[name]
    assert c["N"] == eng.params.N
    raster, f = field_of(eng, name)
    f.free_bits = None
    words = eng.route_free_bits(f)
    assert eng.last_kernel() == "K9b"
    got = words.cpu().numpy().view(np.uint32)
    same(got, SC.free_bits(name), f"free bits {name}")
    hf = Engine.route_field_host(raster.geo, c["rec"], c["goals"], c["lam"], c["block_flags"],
                                 c["inflate"])
    same(got, Engine.route_free_bits_host(hf), f"host free bits {name}")
    plain = eng.route_paths(f, c["starts"], c["goal_idx"])
    assert eng.last_kernel() == "K9t" and "vertices" not in plain
    for span in SC.SPANS:
        o = eng.route_paths(f, c["starts"], c["goal_idx"], smooth=span)
        assert eng.last_kernel() == "K9s"
        check(o, name, span)
        if span == 1:
            for k in ("wp", "status", "steps"):
                same(o[k].cpu().numpy(), plain[k].cpu().numpy(), f"{k} {name} span 1 = K9t")
        status = o["status"].cpu().numpy()
        ok = status == 0
        # nonzero statuses leave the straight line (a goal index out of range: the start)
        gi = c["goal_idx"]
        for q in np.flatnonzero(~ok):
            s = c["starts"][q]
            e = c["goals"][gi[q]] if 0 <= gi[q] < len(c["goals"]) else s
            t = (np.arange(1, c["N"] + 1, dtype=np.float64) / float(c["N"] + 1))[:, None]
            line = np.concatenate([s[None], s + (e - s) * t, e[None]])
            same(o["wp"].cpu().numpy()[q], line, f"straight line {name} q {q}")
        if c["block_flags"] & C.NFZ and ok.any():
            ev = eng.eval_waypoints(o["wp"], raster=raster)
            assert np.all(ev["nfz_hits"].cpu().numpy()[ok] == 0), (name, span)
            assert np.all(ev["offmap"].cpu().numpy()[ok] == 0), (name, span)


def test_one_query_and_a_partial_last_workgroup(eng):
    """Q = 1, and the cases' starts tiled to Q = 4k + 1 = 261 over 66 workgroups: every copy
    of a query gets that query's bits."""
    for name in ("open", "three_goals", "random30"):
        c = SC.BY_NAME[name]
        _, f = field_of(eng, name)
        n = len(c["starts"])
        for span in (7, 64):
            wp, status, steps, vertices, _ = SC.reference(name, span)
            for q in (0, n - 1):
                o = eng.route_paths(f, c["starts"][q:q + 1], c["goal_idx"][q:q + 1], smooth=span)
                same(o["wp"].cpu().numpy()[0], wp[q], f"{name} span {span} Q = 1, query {q}")
                assert int(o["status"][0]) == status[q] and int(o["steps"][0]) == steps[q]
                assert int(o["vertices"][0]) == vertices[q]
            idx = np.arange(261) % n
            o = eng.route_paths(f, c["starts"][idx], c["goal_idx"][idx], smooth=span)
            same(o["wp"].cpu().numpy(), wp[idx], f"{name} span {span} Q = 261")
            same(o["status"].cpu().numpy(), status[idx])
            same(o["steps"].cpu().numpy(), steps[idx])
            same(o["vertices"].cpu().numpy(), vertices[idx])


def test_long_chain_batches_and_the_anchor_list(eng):
    """The spiral (2 425 cells): runs crossing several 64-candidate batches, spans on either
    side of one batch, and anchor counts on either side of the list K9s keeps in LDS
    (uam_route_paths_smooth recomputes the smoothing in its second pass when the list
    overflows: the same bits)."""
    from uam_path_planning_amd import _lib

    c = SC.BY_NAME["spiral"]
    _, f = field_of(eng, "spiral")
    cap = _lib.ROUTE_SMOOTH_LIST
    assert SC.reference("spiral", 1)[2][0] == 2425
    assert SC.reference("spiral", 1)[3][0] - 2 > cap          # span 1: far over the list
    # the anchors of the longest query by span; the spans that straddle the capacity
    count = {s: int(SC.reference("spiral", s)[3][0]) - 2 for s in range(2, 17)}
    under = min((s for s in count if count[s] <= cap), key=lambda s: cap - count[s])
    over = min((s for s in count if count[s] > cap), key=lambda s: count[s] - cap)
    print("anchors by span", count, "list", cap, "spans", over, under)
    assert count[over] > cap >= count[under]
    for span in sorted({1, 2, over, under, 63, 64, 65, 128, 1024}):
        o = eng.route_paths(f, c["starts"], c["goal_idx"], smooth=span)
        check(o, "spiral", span)
    # exactly at the capacity: starts further along the spiral's corridor whose chains have
    # cap - 1, cap and cap + 1 interior cells, all kept at span 1
    cells = SC.chain_of("spiral", 0)
    starts = np.array([C.pt(*cells[len(cells) - n]) for n in (cap + 1, cap + 2, cap + 3)])
    gi = np.zeros(3, dtype=np.int32)
    _, nxt, _, _, _, cost = SC.field_reference("spiral")
    for span in (1, 2):
        wp, status, steps, vertices, _ = S.smooth_paths(c["geo"], cost, nxt, c["goals"], starts,
                                                        gi, c["N"], span)
        if span == 1:
            assert list(vertices) == [cap + 1, cap + 2, cap + 3] and not status.any()
        o = eng.route_paths(f, starts, gi, smooth=span)
        same(o["vertices"].cpu().numpy(), vertices, f"vertices at the capacity, span {span}")
        same(o["steps"].cpu().numpy(), steps)
        same(o["wp"].cpu().numpy(), wp, f"wp at the capacity, span {span}")
    # a run of more than 64 visible cells exists, so 64 and 65 are different answers
    assert not np.array_equal(SC.reference("comb", 64)[0], SC.reference("comb", 65)[0]) or \
        not np.array_equal(SC.reference("spiral", 64)[0], SC.reference("spiral", 65)[0])


def test_invalid_arguments_come_before_any_launch(eng):
    from uam_path_planning_amd import _lib

    name = "inflate_1"
    c = SC.BY_NAME[name]
    raster, f = field_of(eng, name)
    for span in (-1, 1025, 4096):
        with pytest.raises(ValueError, match="span"):
            eng.route_paths(f, c["starts"], c["goal_idx"], smooth=span)
    with pytest.raises(ValueError, match="goal indices"):
        eng.route_paths(f, c["starts"], c["goal_idx"][:-1], smooth=4)
    # NULL buffers and bad counts, straight at the C ABI
    gs = raster.geo.as_struct()
    Q, N = len(c["starts"]), eng.params.N
    words = eng.route_free_bits(f)
    assert words.numel() * 4 == eng.lib.uam_route_free_bits_bytes(ctypes.byref(gs))
    bufs = dict(bits=words, next=f.next, goals=f.goals,
                starts=eng.tensor(c["starts"], torch.float64),
                gi=eng.tensor(c["goal_idx"], torch.int32),
                wp=eng.empty((Q, N + 2, 2), torch.float64), status=eng.empty((Q,), torch.int32),
                steps=eng.empty((Q,), torch.int32), vertices=eng.empty((Q,), torch.int32))

    def call(span=7, n_goals=1, n_queries=Q, desc=gs, **null):
        p = {k: (None if k in null else ctypes.c_void_p(v.data_ptr())) for k, v in bufs.items()}
        return eng.lib.uam_route_paths_smooth(
            eng._ctx, ctypes.byref(desc), p["bits"], p["next"], p["goals"], n_goals, p["starts"],
            p["gi"], n_queries, span, p["wp"], p["status"], p["steps"], p["vertices"],
            eng.stream)

    for k in ("bits", "next", "goals", "starts", "gi", "wp", "status"):
        assert call(**{k: True}) == _lib.UAM_E_INVALID, k
    assert call(span=0) == _lib.UAM_E_INVALID
    assert call(n_goals=0) == _lib.UAM_E_INVALID
    assert call(n_queries=-1) == _lib.UAM_E_INVALID
    assert call(desc=_lib.RasterDesc(0, 76, 0.0, 1.0, 0.1, 0.1, -9999.0, 0.0)) == \
        _lib.UAM_E_INVALID
    rp = f.params()
    for kw in (dict(rec=None), dict(out=None)):
        r = kw.get("rec", ctypes.c_void_p(raster.rec.data_ptr()))
        b = kw.get("out", ctypes.c_void_p(words.data_ptr()))
        assert eng.lib.uam_route_free_bits(eng._ctx, ctypes.byref(gs), r, ctypes.byref(rp), b,
                                           eng.stream) == _lib.UAM_E_INVALID
    assert call(steps=True, vertices=True) == _lib.UAM_OK       # both may be NULL
    eng.synchronize()
    same(bufs["wp"].cpu().numpy(), SC.reference(name, 7)[0], "steps / vertices NULL")
    # and the ordinary call still gives the reference's bits
    check(eng.route_paths(f, c["starts"], c["goal_idx"], smooth=7), name, 7,
          "after the refused calls")


def test_needs_params():
    """UAM_E_STATE without uam_set_params."""
    from uam_path_planning_amd import _lib
    from uam_path_planning_amd.engine import Engine, RasterGeo

    e = Engine(0)
    g = C.GEO
    gs = RasterGeo(g.nx, g.ny, g.x0, g.y_top, g.dx, g.dy).as_struct()
    one = ctypes.c_void_p(e.empty((64,), torch.float64).data_ptr())
    assert e.lib.uam_route_paths_smooth(e._ctx, ctypes.byref(gs), one, one, one, 1, one, one, 1,
                                        4, one, one, None, None, e.stream) == _lib.UAM_E_STATE


def test_wall_with_one_gap_end_to_end(eng):
    """test_gpu_route.py's analytic wall with the smoothed seed: it still passes the gap
    without touching a no-fly cell, and refinement takes it far below the best arc.  The same
    holds for route_smooth_ref's seed under the CPU oracle's refinement (spans 1 .. 1024: sum
    g^2 of 2e-9 .. 2.4e-8 against the arcs' 0.33 .. 0.46), which is why this is asserted."""
    from uam_path_planning_amd.arcs import REFERENCE_DISPLACEMENTS, arc_table
    from uam_path_planning_amd.engine import RasterGeo

    g = C.GEO
    N = eng.params.N
    raster = eng.raster_build(RasterGeo(g.nx, g.ny, g.x0, g.y_top, g.dx, g.dy))
    arcs = eng.gen_paths(WALL_PAIRS, arc_table(N, REFERENCE_DISPLACEMENTS))
    best_arc = eng.refine(arcs)["infeas"].cpu().numpy().reshape(-1, 5).min(axis=1)
    eng.set_option("k9_tile", 32)
    eng.set_option("k9_inner", 32)
    f = eng.route_field(raster, WALL_PAIRS[:, 2:4], inflate=1)
    plain = eng.route_paths(f, WALL_PAIRS[:, 0:2], np.arange(len(WALL_PAIRS)))
    for span in (16, 64):
        seed = eng.route_paths(f, WALL_PAIRS[:, 0:2], np.arange(len(WALL_PAIRS)), smooth=span)
        assert np.all(seed["status"].cpu().numpy() == 0)
        same(seed["steps"].cpu().numpy(), plain["steps"].cpu().numpy())
        vertices = seed["vertices"].cpu().numpy()
        assert np.all(vertices < plain["steps"].cpu().numpy() // 4), vertices
        ev = eng.eval_waypoints(seed["wp"], raster=raster)
        assert np.all(ev["nfz_hits"].cpu().numpy() == 0)
        assert np.all(ev["offmap"].cpu().numpy() == 0)
        refined = eng.refine(seed["wp"])["infeas"].cpu().numpy()
        print("span", span, "vertices", vertices, "sum g^2 after refine: best arc", best_arc,
              "smoothed seed", refined)
        assert np.all(refined < best_arc), (span, refined, best_arc)
