"""The oracle's land polygons (orc_dem_polygons: label4, comps_of, the cut tables of divided
regions, the piece order) against a flood-fill reference that shares no code with it
(polygons_ref), on masks built to break a labelling (polygons_masks): single-cell components by
the thousand, diagonals that 8-connectivity would merge, one-cell-wide paths through tile
corners, a spiral, nested rings, percolating noise, every 3 x 3 pattern around a tile corner,
and large regions whose box cuts fall on, before, after and inside cell edges.  The GPU side of
the same cases is test_gpu_polygons_topology.py; this file is what makes "GPU == oracle" there
mean something."""
import numpy as np
import pytest

import polygons_masks as M
import polygons_ref as R


def test_reference_on_hand_built_masks():
    """The reference itself, on masks whose answer is known by construction."""
    sizes = lambda m: [len(c) for c in R.components(m)]
    assert sizes(M.checkerboard()) == [1] * 13600
    assert sizes(M.diagonal()) == [1] * 136
    for one in (M.staircase, M.anti_staircase, M.hcomb, M.vcomb, M.serpentine, M.spiral):
        m = one()
        assert sizes(m) == [int(m.sum())], one.__name__
    sp = M.spiral()
    assert 13000 < sp.sum() < 14500            # a one-cell-wide arm over half the raster
    # one-cell-wide: no 2 x 2 block of set cells
    assert not (sp[1:, 1:] & sp[1:, :-1] & sp[:-1, 1:] & sp[:-1, :-1]).any()
    assert len(R.components(M.rings())) == 33
    # raster order of the first cell, and (x, y) columns
    m = np.zeros((4, 5), bool)
    m[0, 3] = m[1, 3] = m[1, 0] = m[3, 4] = True
    cs = R.components(m)
    assert [c[0].tolist() for c in cs] == [[3, 0], [0, 1], [4, 3]]
    assert sorted(map(tuple, cs[0].tolist())) == [(3, 0), (3, 1)]
    # the two corner-window masks hold all 512 patterns, each at rows / columns 63..65 of a tile
    seen = set()
    for call in (0, 1):
        w = M.corner_windows(call)
        for j in range(1, 17):
            for i in range(1, 17):
                win = w[64 * j - 1:64 * j + 2, 64 * i - 1:64 * i + 2]
                seen.add(int(sum(int(v) << b for b, v in enumerate(win.ravel()))))
        near = np.zeros(M.CORNER_N, bool)
        near[[64 * k + d for k in range(1, 17) for d in (-1, 0, 1)]] = True
        assert not w[~near].any() and not w[:, ~near].any()   # all else is empty
    assert seen == set(range(512))


def test_mask_of():
    inf, nan = np.inf, np.nan
    d = np.array([nan, inf, -inf, -0.0, 0.0, np.nextafter(np.float32(0), np.float32(1)),
                  -9999.0, 150.0, np.nextafter(np.float32(150), np.float32(inf)), 1e-50],
                 np.float32)
    assert R.mask_of(d, 0.0).tolist() == [0, 1, 0, 0, 0, 1, 0, 1, 1, 0]
    assert R.mask_of(d, 150.0).tolist() == [0, 1, 0, 0, 0, 0, 0, 0, 1, 0]
    assert R.mask_of(d, -9999.0).tolist() == [0, 0, 0, 0, 0, 0, 1, 0, 0, 0]


def test_expected_pieces_division_order():
    """A full 10 x 10 block cut 5 x 5: 25 pieces of 2 x 2 cells, x box outer, y box inner
    from the bottom; with 11 x 10 the box edges fall inside cells and f = 5."""
    m = np.zeros((12, 14), bool)
    m[1:11, 2:12] = True
    ps = R.expected_pieces(m, R.Params(0.0, 50 * 1e4, -1.0, 5), 100.0)
    assert len(ps) == 25 and all(p.f == 1 and len(p.cells) == 4 for p in ps)
    assert [p.cells.min(axis=0).tolist() for p in ps[:6]] == \
        [[2, 9], [2, 7], [2, 5], [2, 3], [2, 1], [4, 9]]
    m[1:11, 12] = True
    ps = R.expected_pieces(m, R.Params(0.0, 50 * 1e4, -1.0, 5), 100.0)
    assert len(ps) == 25 and all(p.f == 5 and len(p.cells) == 11 * 10 for p in ps)
    assert ps[1].cells.min(axis=0).tolist() == [2 * 5, 7 * 5]
    # below the large-area bound the block is one piece; at or below min_area it is dropped
    assert len(R.expected_pieces(m, R.Params(0.0, 110 * 1e4, -1.0, 5), 100.0)) == 1
    assert R.expected_pieces(m, R.Params(110 * 1e4, 1e30, -1.0, 5), 100.0) == []


def test_check_rects_rejects_wrong_rectangles():
    """check_rects has teeth: a cell attached to the wrong piece, a lost piece, a swapped
    order and a bloated rectangle all fail; the exact rectangle in either orientation passes."""
    m = np.zeros((8, 8), bool)
    m[1:3, 1:4] = True
    m[5:7, 2:7] = True
    ps = R.expected_pieces(m, R.Params(0.0, 1e30, -1.0, 5), 100.0)
    box = lambda x0, y0, x1, y1: [[x0, y0], [x0, y1], [x1, y1], [x1, y0]]
    good = [box(100, 500, 400, 700), box(200, 100, 700, 300)]
    R.check_rects(good, ps, 100.0, 0.0, 800.0)
    R.check_rects([g[::-1] for g in good], ps, 100.0, 0.0, 800.0)
    bad = {
        "swapped": good[::-1],
        "lost": good[:1],
        "narrow": [box(100, 500, 300, 700), good[1]],
        "wide": [box(100, 500, 500, 700), good[1]],
        "degenerate": [box(100, 500, 100, 700), good[1]],
    }
    for why, rects in bad.items():
        with pytest.raises(AssertionError):
            R.check_rects(rects, ps, 100.0, 0.0, 800.0)
            pytest.fail(why + " passed")


def test_components_match_scipy():
    ndi = pytest.importorskip("scipy.ndimage")
    for name in ("noise59", "rings_complement", "spiral", "checkerboard"):
        mask = M.case(name, "small")[0]
        lab, n = ndi.label(mask)       # default structure: 4-connectivity, raster order
        cs = R.components(mask)
        assert len(cs) == n
        for k, c in enumerate(cs):
            assert (lab[c[:, 1], c[:, 0]] == k + 1).all() and len(c) == (lab == k + 1).sum()


_worst = {}


@pytest.mark.parametrize("name,kind", M.CASES, ids=M.CASE_IDS)
def test_oracle_matches_flood_fill(oracle_mod, name, kind):
    mask, prm, pieces = M.case(name, kind)
    assert len(pieces) > 0
    rects = M.oracle_rects(oracle_mod, M.dem_of(mask), 0.0, prm)
    M.check(rects, name, kind, _worst)
    print(f"{name}-{kind}: {len(pieces)} pieces, worst so far {_worst}")
