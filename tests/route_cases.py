"""The route seeds' test cases (tests/test_route_cpu.py, tests/test_gpu_route.py): 100 x 76
cells with dx != dy, neither edge a multiple of the tile edges 16, 32 and 64 (7 x 5, 4 x 3 and
2 x 2 tiles), records written by hand (phi, flags).  Seeded; reference(case) computes
tests/route_ref.py's answer once per process and case."""
import collections
import functools

import numpy as np

import route_ref as R

Geo = collections.namedtuple("Geo", "nx ny x0 y_top dx dy")
GEO = Geo(100, 76, 0.25, 3.0, 0.013, 0.0171)
NFZ, MASK = 1, 2
N_DEFAULT = 20


def blank(phi=0.0):
    rec = np.zeros((GEO.ny, GEO.nx, 4), dtype=np.float32)
    rec[..., 0] = phi
    return rec


def flags_of(rec):
    return rec.view(np.uint32)[..., 3]


def pt(ix, iy, fx=0.3, fy=0.7):
    """A point inside cell (ix, iy) that is not its centre (fractions of the cell from its
    western and northern edge)."""
    return [GEO.x0 + (ix + fx) * GEO.dx, GEO.y_top - (iy + fy) * GEO.dy]


def case(name, rec, goals, starts, goal_idx=None, lam=1.0, block_flags=NFZ, inflate=0,
         N=N_DEFAULT):
    starts = np.asarray(starts, dtype=np.float64).reshape(-1, 2)
    if goal_idx is None:
        goal_idx = np.zeros(len(starts), dtype=np.int32)
    return dict(name=name, geo=GEO, rec=np.ascontiguousarray(rec),
                goals=np.asarray(goals, dtype=np.float64).reshape(-1, 2), starts=starts,
                goal_idx=np.asarray(goal_idx, dtype=np.int32), lam=float(lam),
                block_flags=int(block_flags), inflate=int(inflate), N=int(N))


def random_starts(rng, n):
    return [pt(int(rng.integers(GEO.nx)), int(rng.integers(GEO.ny)), rng.random(), rng.random())
            for _ in range(n)]


def open_field(rng):
    rec = blank()
    rec[..., 0] = np.exp2(rng.uniform(-10.0, 10.0, size=(GEO.ny, GEO.nx))).astype(np.float32)
    return rec


def spiral():
    """A corridor two cells wide between walls one cell thick, wound inward."""
    rec = blank(0.5)
    fl = flags_of(rec)
    fl[...] = NFZ
    x, y = 1, 1
    xa, xb, ya, yb = 1, GEO.nx - 3, 1, GEO.ny - 3   # the corridor's north-west corners' box
    first = (x, y)
    d = 0
    while xa <= xb and ya <= yb:
        tx, ty = ((xb, y), (x, yb), (xa, y), (x, ya))[d]
        for cx in range(min(x, tx), max(x, tx) + 1):
            for cy in range(min(y, ty), max(y, ty) + 1):
                fl[cy:cy + 2, cx:cx + 2] = 0
        x, y = tx, ty
        if d == 0:
            ya += 3
        elif d == 1:
            xb -= 3
        elif d == 2:
            yb -= 3
        else:
            xa += 3
        d = (d + 1) % 4
    return rec, first, (x, y)


def comb():
    rec = blank(1.0)
    fl = flags_of(rec)
    for i, x in enumerate(range(6, GEO.nx - 4, 5)):
        if i % 2:
            fl[2:, x] = NFZ
        else:
            fl[:GEO.ny - 2, x] = NFZ
    return rec


def all_cases():
    rng = np.random.default_rng(20251)
    cases = []
    rec = open_field(rng)
    goal = pt(71, 40)
    special = [pt(71, 40, 0.9, 0.1),       # in the goal cell
               pt(72, 40), pt(70, 39),     # adjacent: orthogonal and diagonal
               [GEO.x0 - 0.001, 2.5],      # off the raster
               [1.0, GEO.y_top + 5.0],
               [float("nan"), 2.5]]
    cases.append(case("open", rec, [goal], random_starts(rng, 6) + special))
    cases.append(case("open_lambda0", rec, [goal], random_starts(rng, 4), lam=0.0))

    rec = blank()
    rec[..., 0] = rng.uniform(0.0, 4.0, size=(GEO.ny, GEO.nx)).astype(np.float32)
    flags_of(rec)[rng.random((GEO.ny, GEO.nx)) < 0.3] = NFZ
    flags_of(rec)[33, 48] = 0
    cases.append(case("random30", rec, [pt(48, 33)], random_starts(rng, 12)))

    rec, outer, inner = spiral()
    cases.append(case("spiral", rec, [pt(*inner)], [pt(*outer), pt(50, 1), pt(0, 0)]))
    cases.append(case("comb", comb(), [pt(97, 70)], [pt(1, 1), pt(8, 74), pt(50, 30)]))

    rec = blank(0.25)
    for i in range(GEO.ny):            # the wall x - y = 12, one cell wide, one gap
        if i != 40:
            flags_of(rec)[i, 12 + i] = NFZ
    cases.append(case("diagonal_wall", rec, [pt(80, 20)],
                      [pt(5, 60), pt(51, 40), pt(52, 39), pt(20, 9), pt(13, 0)]))

    rec = blank(0.25)
    fl = flags_of(rec)
    fl[20:41, 30] = fl[20:41, 50] = NFZ
    fl[20, 30:51] = fl[40, 30:51] = NFZ
    cases.append(case("sealed_ring", rec, [pt(40, 30)],
                      [pt(5, 5), pt(90, 70), pt(29, 30), pt(51, 41)]))
    cases.append(case("blocked_and_offmap_goal", rec, [pt(30, 25), [9.0, 9.0]],
                      [pt(5, 5), pt(40, 30), pt(5, 5), pt(30, 25)], goal_idx=[0, 0, 1, 1]))
    cases.append(case("blocked_start", rec, [pt(5, 5)], [pt(30, 25), pt(50, 40), pt(60, 20)]))

    rec = open_field(rng)
    u = rng.random((GEO.ny, GEO.nx))
    phi = rec[..., 0]
    phi[u < 0.04] = np.nan
    phi[(u >= 0.04) & (u < 0.08)] = np.inf
    phi[(u >= 0.08) & (u < 0.12)] = -np.inf
    phi[(u >= 0.12) & (u < 0.16)] = -5.0     # c = -4
    phi[(u >= 0.16) & (u < 0.20)] = -1.0     # c = 0: not > 0
    phi[38, 50] = 1.0
    cases.append(case("nonfinite_phi", rec, [pt(50, 38)], random_starts(rng, 10),
                      block_flags=0))

    rec = blank(0.0)                         # absorption: a corridor through one huge cell
    fl = flags_of(rec)
    fl[...] = NFZ
    fl[30:32, 3:97] = 0
    rec[30:32, 50, 0] = 1e30
    cases.append(case("absorption", rec, [pt(4, 30), pt(95, 31)],
                      [pt(90, 30), pt(90, 30), pt(10, 31), pt(10, 31), pt(60, 30)],
                      goal_idx=[0, 1, 0, 1, 0]))

    rec = blank()
    rec[..., 0] = rng.uniform(0.0, 2.0, size=(GEO.ny, GEO.nx)).astype(np.float32)
    u = rng.random((GEO.ny, GEO.nx))
    fl = flags_of(rec)
    fl[u < 0.15] = NFZ
    fl[(u >= 0.15) & (u < 0.30)] = MASK
    fl[(u >= 0.30) & (u < 0.33)] = NFZ | MASK
    fl[(u >= 0.33) & (u < 0.36)] = 4         # NODATA: never blocks here
    fl[33, 48] = 0
    st = random_starts(rng, 8)
    for bf in (NFZ, MASK, NFZ | MASK, 0):
        cases.append(case(f"block_flags_{bf}", rec, [pt(48, 33)], st, block_flags=bf))

    rec = blank()
    rec[..., 0] = rng.uniform(0.0, 2.0, size=(GEO.ny, GEO.nx)).astype(np.float32)
    fl = flags_of(rec)
    fl[rng.random((GEO.ny, GEO.nx)) < 0.012] = NFZ
    fl[28:39, 43:54] = 0
    st = random_starts(rng, 8) + [pt(0, 0), pt(99, 75)]
    for inflate in (0, 1, 3):
        cases.append(case(f"inflate_{inflate}", rec, [pt(48, 33)], st, inflate=inflate))

    rec = blank()
    rec[..., 0] = rng.uniform(0.0, 4.0, size=(GEO.ny, GEO.nx)).astype(np.float32)
    fl = flags_of(rec)
    fl[rng.random((GEO.ny, GEO.nx)) < 0.2] = NFZ
    goals = [pt(10, 10), pt(90, 60), pt(55, 5)]
    for ix, iy in ((10, 10), (90, 60), (55, 5)):
        fl[iy, ix] = 0
    st = random_starts(rng, 10)
    cases.append(case("three_goals", rec, goals, st, goal_idx=[0, 1, 2, 3, -1, 2, 1, 0, 1, 2]))
    return cases


CASES = all_cases()
NAMES = [c["name"] for c in CASES]
BY_NAME = {c["name"]: c for c in CASES}


@functools.lru_cache(maxsize=None)
def reference(name):
    """route_ref's (dist, next, wp, status, steps, cost plane) of a case; treat as read-only."""
    c = BY_NAME[name]
    dist, nxt, cost = R.route_field(c["geo"], c["rec"].view(np.uint32), c["goals"], c["lam"],
                                    c["block_flags"], c["inflate"])
    wp, status, steps = R.route_paths(c["geo"], cost, nxt, c["goals"], c["starts"],
                                      c["goal_idx"], c["N"])
    for a in (dist, nxt, wp, status, steps):
        a.setflags(write=False)
    return dist, nxt, wp, status, steps, cost
