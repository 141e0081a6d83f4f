"""Plain reference for the labelling behind the land polygons (K8, uam_dem_polygons and the
oracle's orc_dem_polygons): no project code, numpy only.

The product turns a DEM mask into 4-connected regions, drops the small ones, cuts the large
ones into D x D boxes over their bounding box (data_processor.py:34-51 of the reference) and
approximates every region or box piece by its minimum-area rectangle in integer metres.  This
module restates the *topology* of that -- which cells belong together, in which order the
pieces come out -- by an explicit-stack flood fill, and checks rectangles against the cell sets
geometrically (check_rects), so that no union-find, no tile, no cut table and no hull code is
shared with what is tested.

Conventions: mask[y, x], row 0 = north edge; cells are squares of dx_m metres; the raster's
top-left corner is (x0_m, ytop_m).
"""
import math
from collections import namedtuple

import numpy as np

# cells: int64 [n, 2] of (x, y) on the raster refined f times (x counted from the raster's left
# edge, y from its top edge, both in units of dx_m / f)
Piece = namedtuple("Piece", "cells f")

# what polyproc needs: areas in m^2, divisions D
Params = namedtuple("Params", "min_area large_area min_approx_area divisions")


def mask_of(dem, thr):
    """data_manager.py:14-17: nodata cells if thr == -9999, else cells above thr.  float32
    comparisons; NaN is false either way."""
    d = np.asarray(dem, np.float32)
    t = np.float32(thr)
    with np.errstate(invalid="ignore"):
        return d == t if t == np.float32(-9999.0) else d > t


def components(mask):
    """4-connected components of the set cells, in raster order of their first cell; each an
    int64 [n, 2] array of (x, y).  Flood fill with an explicit stack (a one-cell-wide path of
    any length is fine)."""
    m = np.asarray(mask, bool)
    ny, nx = m.shape
    W = nx + 2  # one cell of padding all round: no bounds tests in the loop
    pad = np.zeros((ny + 2, W), np.uint8)
    pad[1:-1, 1:-1] = m
    todo = bytearray(pad.tobytes())  # 1 = set and not yet reached
    out = []
    for s in np.flatnonzero(pad.ravel()).tolist():
        if not todo[s]:
            continue
        todo[s] = 0
        stack, cells = [s], []
        while stack:
            i = stack.pop()
            cells.append(i)
            for j in (i - 1, i + 1, i - W, i + W):
                if todo[j]:
                    todo[j] = 0
                    stack.append(j)
        c = np.asarray(cells, np.int64)
        out.append(np.stack([c % W - 1, c // W - 1], axis=1))
    return out


def _refinement(extent, D):
    """Smallest f with every box edge j * extent / D on the 1/f-cell grid."""
    return D // math.gcd(extent, D)


def expected_pieces(mask, params, dx_m):
    """The cell sets that must each yield one rectangle, in output order."""
    cell = float(dx_m) * float(dx_m)
    D = int(params.divisions)
    out = []
    for comp in components(mask):
        area = len(comp) * cell
        if area <= params.min_area:
            continue
        if area <= params.large_area:
            out.append(Piece(comp, 1))
            continue
        x0, y0 = comp.min(axis=0)
        x1, y1 = comp.max(axis=0)
        Wc, Hc = int(x1 - x0 + 1), int(y1 - y0 + 1)
        fx, fy = _refinement(Wc, D), _refinement(Hc, D)
        f = fx * fy // math.gcd(fx, fy)
        local = np.zeros((Hc, Wc), np.uint8)
        local[comp[:, 1] - y0, comp[:, 0] - x0] = 1
        up = np.kron(local, np.ones((f, f), np.uint8))
        bw, bh = Wc * f // D, Hc * f // D
        assert bw * D == Wc * f and bh * D == Hc * f
        for j in range(D):              # x boxes outer
            for k in range(D):          # y boxes inner, k = 0 at the bottom
                r0 = Hc * f - (k + 1) * bh
                for part in components(up[r0:r0 + bh, j * bw:(j + 1) * bw]):
                    out.append(Piece(part + [j * bw + x0 * f, r0 + y0 * f], f))
    return out


def piece_corners(piece, dx_m, x0_m, ytop_m):
    """The corners of the piece's cells in metres, float64 [4 n, 2] (shared ones repeated)."""
    c = piece.cells
    step = float(dx_m) / piece.f
    k = np.concatenate([c, c + [1, 0], c + [0, 1], c + [1, 1]])
    return np.stack([x0_m + k[:, 0] * step, ytop_m - k[:, 1] * step], axis=1)


def outside_distance(rect, pts):
    """How far (metres) the farthest of pts lies outside the convex quadrilateral rect, by the
    signed distance to its four edges; <= 0 if all are inside.  Either orientation."""
    r = np.asarray(rect, np.float64).reshape(4, 2)
    e = np.roll(r, -1, axis=0) - r
    ln = np.hypot(e[:, 0], e[:, 1])
    if not np.all(ln > 0):
        return math.inf
    twice_area = float(np.sum(r[:, 0] * np.roll(r[:, 1], -1) - np.roll(r[:, 0], -1) * r[:, 1]))
    if twice_area == 0.0:
        return math.inf
    sgn = 1.0 if twice_area > 0 else -1.0   # counter-clockwise: the inside is on the left
    d = pts[:, None, :] - r[None, :, :]
    cross = e[None, :, 0] * d[:, :, 1] - e[None, :, 1] * d[:, :, 0]
    return float(np.max(-sgn * cross / ln[None, :]))


def rect_area(rect):
    r = np.asarray(rect, np.float64).reshape(4, 2)
    return abs(0.5 * float(np.sum(r[:, 0] * np.roll(r[:, 1], -1) -
                                  np.roll(r[:, 0], -1) * r[:, 1])))


OUTSIDE_TOL_M = 2.0  # corners are truncated to integer metres: an edge moves by <= sqrt(2) m


def check_rects(rects, pieces, dx_m, x0_m, ytop_m, stats=None):
    """(a) one rectangle per piece; (b) no cell corner of piece i more than 2 m outside
    rectangle i; (c) rectangle i no larger than the piece's bounding box w x h, up to rounding:
    area <= w * h + 3 * (a + b) + 9 with a, b the rectangle's own sides.  stats (a dict) receives
    the worst figures seen."""
    rects = np.asarray(rects, np.int64).reshape(-1, 4, 2)
    assert len(rects) == len(pieces), f"{len(rects)} rectangles for {len(pieces)} pieces"
    worst_out, worst_excess = -math.inf, -math.inf
    for i, (r, p) in enumerate(zip(rects, pieces)):
        pts = piece_corners(p, dx_m, x0_m, ytop_m)
        out = outside_distance(r, pts)
        worst_out = max(worst_out, out)
        assert out <= OUTSIDE_TOL_M, (
            f"piece {i} ({len(p.cells)} cells, first {p.cells[0].tolist()}, f={p.f}) sticks "
            f"{out:.2f} m out of rectangle {r.tolist()}")
        w, h = pts.max(axis=0) - pts.min(axis=0)
        rf = r.astype(np.float64)
        a = math.hypot(*(rf[1] - rf[0]))
        b = math.hypot(*(rf[2] - rf[1]))
        excess = rect_area(r) - (w * h + 3.0 * (a + b) + 9.0)
        worst_excess = max(worst_excess, excess)
        assert excess <= 0.0, (
            f"rectangle {i} {r.tolist()} has area {rect_area(r):.0f} m^2, the piece's "
            f"{w:.0f} x {h:.0f} m bounding box allows {w * h + 3.0 * (a + b) + 9.0:.0f}")
    if stats is not None:
        stats["outside_m"] = max(stats.get("outside_m", -math.inf), worst_out)
        stats["area_excess_m2"] = max(stats.get("area_excess_m2", -math.inf), worst_excess)
