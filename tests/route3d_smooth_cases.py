"""The volume smoothing's test cases (tests/test_route3d_smooth_cpu.py,
tests/test_gpu_route3d_smooth.py): every case of tests/route3d_cases.py, and hand-built ones
where a tie of one of the three touched-voxel inequalities, a voxel round a corner, a one-voxel
gap, the order of the visibility tests, a run longer than one 64-candidate batch or the anchor
list's capacity decides.  reference(name, span) computes tests/route3d_smooth_ref.py's answer
once per process; "blocked" is always the reference's verdict, never written down here."""
import functools

import numpy as np

import route3d_cases as C
import route3d_ref as R
import route3d_smooth_ref as S

SPANS = (1, 2, 7, 64, 65, 1024)
GEO = C.GEO
CAP = 256                                     # UAM_ROUTE_SMOOTH_LIST (asserted by the tests)


def block(vol, ix, iy, iz):
    """One voxel blocked by a non-finite risk (its column stays unflagged)."""
    vol[0][iy, ix, iz] = np.nan


# voxel pairs (A, B, the blocked voxel, the inequality 0 = (x,y), 1 = (x,z), 2 = (y,z)) where
# the blocked voxel lies in T3(A, B) by equality in that inequality alone
TIES = {"ties3d": [
    ((5, 5, 2), (6, 8, 4), (6, 6, 3), 0), ((6, 8, 4), (5, 5, 2), (6, 6, 3), 0),
    ((6, 15, 4), (5, 18, 2), (5, 16, 3), 0),
    ((15, 5, 2), (16, 7, 5), (16, 6, 3), 1), ((16, 7, 5), (15, 5, 2), (16, 6, 3), 1),
    ((16, 17, 2), (15, 15, 5), (15, 16, 3), 1),
    ((25, 5, 2), (26, 7, 8), (25, 6, 3), 2), ((26, 7, 8), (25, 5, 2), (25, 6, 3), 2),
    ((26, 15, 8), (25, 17, 2), (26, 16, 7), 2),
]}


def ties3d():
    vol = C.blank(0.25)
    for _, _, w, _ in TIES["ties3d"]:
        block(vol, *w)
    starts = [C.pt(*a) for a, _, _, _ in TIES["ties3d"]] + [C.pt(2, 6, 1), C.pt(3, 16, 9)]
    return C.case("ties3d", vol, [C.pt(40, 10, 5), C.pt(30, 8, 9)], starts,
                  goal_idx=[0, 1] * 5 + [0])


# the segment (10,10,2) -> (14,14,6) runs through voxel corners; CORNER is the pair and the
# corner between (11,11,3) and (12,12,4), whose eight voxels are {11,12} x {11,12} x {3,4}
CORNER = ((10, 10, 2), (14, 14, 6))
CORNER_VOXELS = [(x, y, z) for x in (11, 12) for y in (11, 12) for z in (3, 4)]


def corner():
    """One voxel round a corner of the 3-D diagonal blocked: the diagonal's chain has to leave
    it, and no shortcut may pass through the corner."""
    vol = C.blank(0.25)
    block(vol, 12, 11, 3)
    return C.case("corner", vol, [C.pt(16, 16, 8), C.pt(14, 14, 6)],
                  [C.pt(9, 9, 1), C.pt(10, 10, 2), C.pt(8, 10, 2), C.pt(10, 10, 2)],
                  goal_idx=[0, 0, 0, 1])


GAP = (25, 14, 5)


def sheet_gap():
    """A sheet one voxel thick across the volume with one free voxel: straight segments thread
    it from other rows and other layers."""
    vol = C.blank(0.25)
    vol[0][:, GAP[0], :] = np.nan
    vol[0][GAP[1], GAP[0], GAP[2]] = 0.25
    return C.case("sheet_gap", vol, [C.pt(31, 14, 5), C.pt(31, 17, 7), C.pt(40, 3, 1)],
                  [C.pt(19, 14, 5), C.pt(19, 11, 3), C.pt(13, 8, 1), C.pt(20, 25, 10),
                   C.pt(3, 14, 5), C.pt(22, 12, 4)], goal_idx=[0, 1, 2, 0, 0, 2])


def staircase():
    """Two wall ends over every layer force the chain (19,15) (20,15) (21,15) (21,16) (22,16)
    in layer 5: from c_1, c_3 is hidden behind (20,16) and c_4 is in sight again -- "advance
    while visible" stops at c_2, "the farthest visible" would not."""
    vol = C.blank(0.25)
    vol[2][16:, 20] = C.NFZ
    vol[2][:16, 22] = C.NFZ
    return C.case("staircase3d", vol, [C.pt(35, 22, 5)],
                  [C.pt(19, 15, 5), C.pt(10, 4, 5), C.pt(19, 12, 3)])


def open_climb():
    """Open volume, 8 layers up over 37 columns."""
    return C.case("open_climb", C.blank(0.25), [C.pt(40, 14, 9)],
                  [C.pt(3, 14, 1), C.pt(3, 3, 0)])


def short_chains():
    """n = 1 (s = g), n = 2 (face-, edge- and corner-adjacent), n = 3 and n = 4."""
    return C.case("short_chains3d", C.blank(0.25), [C.pt(30, 14, 5)],
                  [C.pt(30, 14, 5, 0.9, 0.1, 0.8), C.pt(31, 14, 5), C.pt(31, 14, 6),
                   C.pt(31, 15, 6), C.pt(32, 14, 5), C.pt(32, 15, 7), C.pt(30, 14, 8),
                   C.pt(33, 16, 5)])


LONG_GEO = C.Geo(140, 3, 2, 0.25, 3.0, 0.013, 0.0171, 40.0, 30.0)


def long_sight():
    """A thin open volume: from c_1 every voxel of the chain is in sight, so one anchor's
    candidates cross several 64-lane batches and spans 63 / 64 / 65 / 128 keep different
    voxels."""
    g = LONG_GEO
    return C.case("long_sight", C.blank(0.25, geo=g), [C.pt(138, 2, 1, geo=g)],
                  [C.pt(1, 0, 0, geo=g), C.pt(70, 1, 1, geo=g)], geo=g)


LONG_SPANS = (63, 64, 65, 128)
CORRIDOR_GEO = C.Geo(23, 29, 3, 0.25, 3.0, 0.013, 0.0171, 40.0, 30.0)
CORRIDOR_LEGS = 14
CORRIDOR_LAYERS = (0, 1, 2, 1)                # leg r lies in layer CORRIDOR_LAYERS[r % 4]


def corridor_volume():
    """Legs along x in the odd rows, each in one layer, joined at alternating ends by a
    three-row connector that is free in both legs' layers; everything else is blocked."""
    g = CORRIDOR_GEO
    vol = C.blank(np.nan, geo=g)
    layer = [CORRIDOR_LAYERS[r % 4] for r in range(CORRIDOR_LEGS)]
    for r in range(CORRIDOR_LEGS):
        vol[0][2 * r + 1, 1:22, layer[r]] = 0.25
        if r + 1 < CORRIDOR_LEGS:
            end = 21 if r % 2 == 0 else 1
            for lz in (layer[r], layer[r + 1]):
                vol[0][2 * r + 1:2 * r + 4, end, lz] = 0.25
    return vol


def corridor():
    """A winding corridor through three layers whose chain keeps more than CAP anchors at span
    1; the further starts lie on that chain, with exactly CAP - 1, CAP and CAP + 1 interior
    voxels left."""
    g = CORRIDOR_GEO
    vol = corridor_volume()
    goal = C.pt(1, 2 * CORRIDOR_LEGS - 1, CORRIDOR_LAYERS[(CORRIDOR_LEGS - 1) % 4], geo=g)
    start = C.pt(1, 1, 0, geo=g)
    cost = R.cost_volume(g, vol[0], vol[1], vol[2], 1.0, C.NFZ, 0, 0.0)
    _, nxt = R.field(g, cost, goal, C.KAPPA)
    st, cells = S.chain(g, cost, nxt[None], [tuple(goal)], start, 0)
    assert st == 0 and len(cells) > CAP + 3
    more = [C.pt(*cells[len(cells) - n], geo=g) for n in (CAP + 1, CAP + 2, CAP + 3)]
    return C.case("corridor", vol, [goal], [start] + more, geo=g)


BRIDGE_GEO = C.BY_NAME["nz1_bridge"]["geo"]


def nz1_smooth_bridge():
    """route3d_cases' one-layer volume with every start and the goal at the layer centre: the
    bridge to uam_route_paths_smooth."""
    c = C.BY_NAME["nz1_bridge"]
    zc = C.layer_centre(0, BRIDGE_GEO)
    goals, starts = c["goals"].copy(), c["starts"].copy()
    goals[:, 2] = zc
    starts[:, 2] = zc
    return C.case("nz1_smooth_bridge", (c["risk"], c["terrain"], c["flags"]), goals, starts,
                  geo=BRIDGE_GEO)


EXTRA = [ties3d(), corner(), sheet_gap(), staircase(), open_climb(), short_chains(),
         long_sight(), corridor(), nz1_smooth_bridge()]
CASES = C.CASES + EXTRA
NAMES = [c["name"] for c in CASES]
BY_NAME = {c["name"]: c for c in CASES}


@functools.lru_cache(maxsize=None)
def field_reference(name):
    """route3d_ref's (dist, next, wp3, status, steps, cost volume) of a case; read-only."""
    if name in C.BY_NAME:
        return C.reference(name)
    c = BY_NAME[name]
    dist, nxt, cost = R.route_field3d(c["geo"], c["risk"], c["terrain"], c["flags"], c["goals"],
                                      c["lam"], c["block_flags"], c["inflate"], c["agl"],
                                      c["kappa"])
    wp, status, steps = R.route_paths3d(c["geo"], cost, nxt, c["goals"], c["starts"],
                                        c["goal_idx"], c["N"], c["kappa"])
    for a in (dist, nxt, wp, status, steps):
        a.setflags(write=False)
    return dist, nxt, wp, status, steps, cost


def smooth(name, span, starts=None, goal_idx=None):
    """route3d_smooth_ref's answer for a case's field and other starts."""
    c = BY_NAME[name]
    _, nxt, _, _, _, cost = field_reference(name)
    starts = c["starts"] if starts is None else starts
    goal_idx = c["goal_idx"] if goal_idx is None else goal_idx
    return S.smooth_paths3d(c["geo"], cost, nxt, c["goals"], starts, goal_idx, c["N"],
                            c["kappa"], span)


@functools.lru_cache(maxsize=None)
def reference(name, span):
    """route3d_smooth_ref's (wp3, status, steps, vertices, length) of a case; read-only."""
    out = smooth(name, span)
    for a in out:
        a.setflags(write=False)
    return out


def pack_bits(free):
    """A [ny, nx, nz] boolean volume as the library's words: bit v & 31 of word v >> 5."""
    flat = np.asarray(free, dtype=bool).reshape(-1)
    padded = np.zeros((flat.size + 31) // 32 * 32, dtype=np.uint64)
    padded[:flat.size] = flat
    words = (padded.reshape(-1, 32) << np.arange(32, dtype=np.uint64)).sum(axis=1)
    return words.astype(np.uint32)


def free_bits(name):
    """The reference's cost volume < inf as the library's bits."""
    return pack_bits(np.array(field_reference(name)[5]) < np.inf)


def chain_of(name, q):
    """The reference's voxel chain of a status-0 query."""
    c = BY_NAME[name]
    _, nxt, _, _, _, cost = field_reference(name)
    goals = [tuple(map(float, g)) for g in c["goals"]]
    st, cells = S.chain(c["geo"], cost, nxt, goals, c["starts"][q], int(c["goal_idx"][q]))
    assert st == 0
    return cells
