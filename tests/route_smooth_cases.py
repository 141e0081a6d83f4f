"""The smoothing's test cases (tests/test_route_smooth_cpu.py, tests/test_gpu_route_smooth.py):
every case of tests/route_cases.py, and hand-built ones where a tie of the touched-cell
inequality, a one-cell gap or the order of the visibility tests decides.  reference(name, span)
computes tests/route_smooth_ref.py's answer once per process; "blocked" is always the
reference's verdict, never written down here."""
import functools

import numpy as np

import route_cases as C
import route_ref as R
import route_smooth_ref as S

SPANS = (1, 2, 7, 64, 65, 1024)
GEO = C.GEO


def tie_slope1():
    """One blocked cell whose corner lies on the slope-1 segments through the cells
    (31 + i, 39 - i): the corner (41, 30) | (40, 29) between (40, 30) and (41, 29)."""
    rec = C.blank(0.25)
    C.flags_of(rec)[30, 41] = C.NFZ
    return C.case("tie_slope1", rec, [C.pt(50, 20)],
                  [C.pt(30, 40), C.pt(31, 39), C.pt(36, 34), C.pt(28, 40)])


def tie_slope13():
    """(20, 20) -> (23, 21) passes through the corner shared by (21, 20), (22, 20), (21, 21),
    (22, 21); (21, 21) is touched there and nowhere else."""
    rec = C.blank(0.25)
    C.flags_of(rec)[21, 21] = C.NFZ
    return C.case("tie_slope13", rec, [C.pt(44, 28)],
                  [C.pt(19, 20), C.pt(20, 20), C.pt(17, 19), C.pt(14, 18)])


def one_cell_gap():
    """A wall one cell thick with one free cell: straight segments thread it."""
    rec = C.blank(0.25)
    fl = C.flags_of(rec)
    fl[:, 50] = C.NFZ
    fl[38, 50] = 0
    return C.case("one_cell_gap", rec, [C.pt(55, 38), C.pt(55, 39), C.pt(60, 42)],
                  [C.pt(45, 38), C.pt(45, 37), C.pt(40, 34), C.pt(45, 30), C.pt(30, 38),
                   C.pt(44, 36)], goal_idx=[0, 1, 2, 0, 0, 2])


def staircase():
    """Two wall ends force the chain (39,30) (40,30) (41,30) (41,31) (42,31): from c_1 =
    (40,30), c_3 is hidden behind (40,31) and c_4 is in sight again -- "advance while visible"
    stops at c_2, "the farthest visible" would not."""
    rec = C.blank(0.25)
    fl = C.flags_of(rec)
    fl[31:, 40] = C.NFZ
    fl[:31, 42] = C.NFZ
    return C.case("staircase", rec, [C.pt(55, 15)], [C.pt(39, 30), C.pt(30, 45), C.pt(39, 33)])


def short_chains():
    """n = 1 (s = g), n = 2 (adjacent), n = 3 (one interior cell, kept), n = 4."""
    rec = C.blank(0.25)
    return C.case("short_chains", rec, [C.pt(71, 40)],
                  [C.pt(71, 40, 0.9, 0.1), C.pt(72, 40), C.pt(70, 39), C.pt(73, 40),
                   C.pt(73, 42), C.pt(73, 41), C.pt(74, 40)])


EXTRA = [tie_slope1(), tie_slope13(), one_cell_gap(), staircase(), short_chains()]
CASES = C.CASES + EXTRA
NAMES = [c["name"] for c in CASES]
BY_NAME = {c["name"]: c for c in CASES}

# cell pairs (A, B, the blocked cell) where the blocked cell is touched by equality alone
TIES = {
    "tie_slope1": [((31, 39), (45, 25), (41, 30)), ((40, 30), (41, 29), (41, 30)),
                   ((45, 25), (36, 34), (41, 30))],
    "tie_slope13": [((20, 20), (23, 21), (21, 21)), ((20, 20), (26, 22), (21, 21)),
                    ((23, 21), (20, 20), (21, 21)), ((21, 19), (22, 22), (21, 21))],
}
# cell pairs in plain sight through the gap
THREADS = {"one_cell_gap": [((45, 38), (55, 38)), ((45, 37), (55, 39)), ((45, 36), (55, 40)),
                            ((55, 40), (45, 36))]}


@functools.lru_cache(maxsize=None)
def field_reference(name):
    """route_ref's (dist, next, wp, status, steps, cost plane) of a case; read-only."""
    if name in C.BY_NAME:
        return C.reference(name)
    c = BY_NAME[name]
    dist, nxt, cost = R.route_field(c["geo"], c["rec"].view(np.uint32), c["goals"], c["lam"],
                                    c["block_flags"], c["inflate"])
    wp, status, steps = R.route_paths(c["geo"], cost, nxt, c["goals"], c["starts"],
                                      c["goal_idx"], c["N"])
    for a in (dist, nxt, wp, status, steps):
        a.setflags(write=False)
    return dist, nxt, wp, status, steps, cost


@functools.lru_cache(maxsize=None)
def reference(name, span):
    """route_smooth_ref's (wp, status, steps, vertices, length) of a case; read-only."""
    c = BY_NAME[name]
    _, nxt, _, _, _, cost = field_reference(name)
    out = S.smooth_paths(c["geo"], cost, nxt, c["goals"], c["starts"], c["goal_idx"], c["N"],
                         span)
    for a in out:
        a.setflags(write=False)
    return out


def free_bits(name):
    """The reference's cost plane < inf as the library's bit plane [ny, (nx + 31) // 32]."""
    cost = np.array(field_reference(name)[5])
    ny, nx = cost.shape
    free = np.zeros((ny, (nx + 31) // 32 * 32), dtype=np.uint64)
    free[:, :nx] = cost < np.inf
    words = (free.reshape(ny, -1, 32) << np.arange(32, dtype=np.uint64)).sum(axis=2)
    return words.astype(np.uint32)


def chain_of(name, q):
    """The reference's cell chain of a status-0 query."""
    c = BY_NAME[name]
    _, nxt, _, _, _, cost = field_reference(name)
    goals = [tuple(map(float, g)) for g in c["goals"]]
    st, cells = S.chain(c["geo"], cost, nxt, goals, c["starts"][q], int(c["goal_idx"][q]))
    assert st == 0
    return cells
