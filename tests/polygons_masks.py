"""Deterministic adversarial masks for the K8 labelling tests (test_polygons_topology_cpu.py,
test_gpu_polygons_topology.py), the geometry they sit on, and the case tables both files share.
Plain numpy; the expected pieces of a case are computed once per process (polygons_ref).

Geometry: 100 m cells (dx = dy = 0.1 with unit_m = 1000), x0 = 0, y_top = ny * 0.1, so every
pixel corner and every box edge is an integer number of metres."""
import functools

import numpy as np

import polygons_ref as R

NX, NY = 200, 136          # 3.1 x 2.1 tiles of 64 x 64: partial tiles on both edges
DX, UNIT_M = 0.1, 1000.0
DX_M = 100.0
LARGE_CELLS = 400          # "divided" runs: components above this many cells are cut D x D


def _xy(nx=NX, ny=NY):
    y, x = np.mgrid[0:ny, 0:nx]
    return x, y


def checkerboard():
    x, y = _xy()
    return (x + y) % 2 == 0


def diagonal():
    x, y = _xy()
    return x == y


def staircase():
    x, y = _xy()
    return (x == y) | (x == y + 1)


def anti_staircase():          # through the tile corner (64, 64) from the other side
    x, y = _xy()
    return (x + y == 127) | (x + y == 128)


def hcomb():
    x, y = _xy()
    return (y % 2 == 0) | (x == 0)


def vcomb():
    x, y = _xy()
    return (x % 2 == 0) | (y == 0)


def serpentine():
    x, y = _xy()
    return (y % 2 == 0) | ((y % 4 == 1) & (x == NX - 1)) | ((y % 4 == 3) & (x == 0))


def spiral(nx=NX, ny=NY):
    """A one-cell-wide arm with one-cell gaps, wound clockwise from the top-left corner to the
    centre: go straight while the next cell touches no set cell but the current one, else
    turn right."""
    m = np.zeros((ny, nx), bool)
    x = y = 0
    dx, dy = 1, 0
    m[0, 0] = True

    def free(px, py):
        return not (0 <= px < nx and 0 <= py < ny) or not m[py, px]

    def can_go(ddx, ddy):
        px, py = x + ddx, y + ddy
        return (0 <= px < nx and 0 <= py < ny and not m[py, px] and free(px + ddx, py + ddy)
                and free(px - ddy, py + ddx) and free(px + ddy, py - ddx))

    while True:
        if not can_go(dx, dy):
            dx, dy = -dy, dx                      # turn right (y grows downwards)
            if not can_go(dx, dy):
                return m
        x, y = x + dx, y + dy
        m[y, x] = True


def rings():
    x, y = _xy()
    return np.maximum(abs(x - 100), abs(y - 68)) % 4 == 0


def noise(p, seed, nx=NX, ny=NY):
    return np.random.default_rng(seed).random((ny, nx)) < p


CORNER_N = 1088            # 17 x 17 tiles: 16 x 16 = 256 interior tile corners


def corner_windows(call):
    """One 3 x 3 pattern per interior tile corner, centred on the first cell of the tile below
    and right of it (rows and columns 63 / 64 / 65 of the tile grid); pattern number
    256 * call + corner, bit 3 * row + column.  call 0 and 1 together: all 512 patterns."""
    m = np.zeros((CORNER_N, CORNER_N), bool)
    for j in range(16):
        for i in range(16):
            pat = 256 * call + 16 * j + i
            cx, cy = 64 * (i + 1), 64 * (j + 1)
            for b in range(9):
                if pat >> b & 1:
                    m[cy - 1 + b // 3, cx - 1 + b % 3] = True
    return m


FRAME_N = 330              # raster of the cut-placement masks


def frame(W, H, seed=11, nx=FRAME_N, ny=FRAME_N):
    """A solid one-cell frame of W x H cells at the top-left, p = 0.8 noise inside: one large
    component whose bounding box is the frame (plus a few enclosed specks)."""
    m = np.zeros((ny, nx), bool)
    m[:H, :W] = noise(0.8, seed, W, H)
    m[0, :W] = m[H - 1, :W] = True
    m[:H, 0] = m[:H, W - 1] = True
    return m


def params(large_cells=None, D=5):
    large = 1e30 if large_cells is None else large_cells * DX_M * DX_M
    return R.Params(0.0, large, -1.0, D)


# name -> mask builder; every one of these runs small-only and divided (LARGE_CELLS, D = 5)
BASIC = {
    "checkerboard": checkerboard,
    "diagonal": diagonal,
    "staircase": staircase,
    "anti_staircase": anti_staircase,
    "hcomb": hcomb,
    "vcomb": vcomb,
    "serpentine": serpentine,
    "spiral": spiral,
    "spiral_complement": lambda: ~spiral(),
    "rings": rings,
    "rings_complement": lambda: ~rings(),
    "noise30": lambda: noise(0.3, 30),
    "noise50": lambda: noise(0.5, 50),
    "noise59": lambda: noise(0.59, 59),
    "noise70": lambda: noise(0.7, 70),
    "noise90": lambda: noise(0.9, 90),
}

# name -> (mask builder, large_cells or None, D): cases with their own parameters
SPECIAL = {
    "corners0": (lambda: corner_windows(0), None, 5),
    "corners1": (lambda: corner_windows(1), None, 5),
    # cuts of the refined grid on a tile edge (320), one column / row before (315), one after
    "frame315x315": (lambda: frame(315, 315), LARGE_CELLS, 5),
    "frame320x320": (lambda: frame(320, 320), LARGE_CELLS, 5),
    "frame325x325": (lambda: frame(325, 325), LARGE_CELLS, 5),
    "frame315x325": (lambda: frame(315, 325), LARGE_CELLS, 5),
    "frame320x315": (lambda: frame(320, 315), LARGE_CELLS, 5),
    # box edges inside pixels: the refined grid has split columns and rows
    "frame202x138": (lambda: frame(202, 138, nx=210, ny=140), LARGE_CELLS, 5),
    "noise70_D3": (lambda: noise(0.7, 70), LARGE_CELLS, 3),
    "noise59_D7": (lambda: noise(0.59, 59), LARGE_CELLS, 7),
    # dozens of divided regions at once (the GPU labels them together, on side streams)
    "noise59_L40": (lambda: noise(0.59, 59), 40, 5),
}

CASES = [(name, "small") for name in BASIC] + [(name, "divided") for name in BASIC] + \
        [(name, "own") for name in SPECIAL]
CASE_IDS = [f"{n}-{k}" for n, k in CASES]


@functools.lru_cache(maxsize=None)
def case(name, kind):
    """-> (mask, Params, expected pieces); built once, never modified (the arrays are
    read-only)."""
    if kind == "own":
        build, large_cells, D = SPECIAL[name]
    else:
        build, large_cells, D = BASIC[name], (LARGE_CELLS if kind == "divided" else None), 5
    mask = np.ascontiguousarray(build())
    mask.setflags(write=False)
    prm = params(large_cells, D)
    pieces = R.expected_pieces(mask, prm, DX_M)
    for p in pieces:
        p.cells.setflags(write=False)
    return mask, prm, pieces


def dem_of(mask):
    return np.where(mask, np.float32(10.0), np.float32(-9999.0)).astype(np.float32)


ORACLE_CAP = 16384         # the checkerboard has 13 600 components


def oracle_rects(O, dem, thr, prm):
    """oracle.dem_polygons on this module's geometry with the polyproc parameters prm."""
    ny, nx = dem.shape
    rd = O.Oracle.raster_desc(nx, ny, 0.0, ny * DX, DX, DX)
    pp = O.polyproc(prm.min_area, prm.large_area, prm.divisions, prm.min_approx_area)
    return O.dem_polygons(dem, rd, thr, UNIT_M, pp, cap=ORACLE_CAP)


def check(rects, name, kind, stats=None):
    mask, _, pieces = case(name, kind)
    R.check_rects(rects, pieces, DX_M, 0.0, mask.shape[0] * DX_M, stats)
