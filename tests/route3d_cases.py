"""The volume route seeds' test cases (tests/test_route3d_cpu.py, tests/test_gpu_route3d.py):
43 x 29 x 11 voxels with dx != dy -- partial tiles on every axis for every tile shape (8 or 16
voxels in x/y, 4 or 8 layers), 3 x 2 x 2 tiles at the largest -- written by hand as risk,
terrain and column flags.  Seeded; reference(name) computes tests/route3d_ref.py's answer once
per process and case.  volume_words(case) lays a case out as the volume buffer of
include/uampath.h (uam_volume_desc)."""
import collections
import functools

import numpy as np

import route3d_ref as R

Geo = collections.namedtuple("Geo", "nx ny nz x0 y_top dx dy z0 dz")
GEO = Geo(43, 29, 11, 0.25, 3.0, 0.013, 0.0171, 40.0, 30.0)
NFZ, MASK = 1, 2
N = 9
KAPPA = 1e-3


def blank(risk=0.0, geo=GEO):
    return (np.full((geo.ny, geo.nx, geo.nz), risk, dtype=np.float32),
            np.zeros((geo.ny, geo.nx), dtype=np.float32),
            np.zeros((geo.ny, geo.nx), dtype=np.uint32))


def pt(ix, iy, iz, fx=0.3, fy=0.7, fz=0.4, geo=GEO):
    """A point inside voxel (ix, iy, iz) that is not its centre."""
    return [geo.x0 + (ix + fx) * geo.dx, geo.y_top - (iy + fy) * geo.dy,
            geo.z0 + (iz + fz) * geo.dz]


def case(name, vol, goals, starts, goal_idx=None, lam=1.0, block_flags=NFZ, inflate=0, agl=0.0,
         kappa=KAPPA, geo=GEO):
    risk, terrain, flags = vol
    starts = np.asarray(starts, dtype=np.float64).reshape(-1, 3)
    if goal_idx is None:
        goal_idx = np.zeros(len(starts), dtype=np.int32)
    return dict(name=name, geo=geo, risk=np.ascontiguousarray(risk, dtype=np.float32),
                terrain=np.ascontiguousarray(terrain, dtype=np.float32),
                flags=np.ascontiguousarray(flags, dtype=np.uint32),
                goals=np.asarray(goals, dtype=np.float64).reshape(-1, 3), starts=starts,
                goal_idx=np.asarray(goal_idx, dtype=np.int32), lam=float(lam),
                block_flags=int(block_flags), inflate=int(inflate), agl=float(agl),
                kappa=float(kappa), N=N)


def random_starts(rng, n, geo=GEO):
    return [pt(int(rng.integers(geo.nx)), int(rng.integers(geo.ny)), int(rng.integers(geo.nz)),
               rng.random(), rng.random(), rng.random(), geo=geo) for _ in range(n)]


def open_volume(rng):
    risk, terrain, flags = blank()
    risk[...] = np.exp2(rng.uniform(-8.0, 6.0, size=risk.shape)).astype(np.float32)
    return risk, terrain, flags


def layer_centre(iz, geo=GEO):
    return geo.z0 + (iz + 0.5) * geo.dz


def all_cases():
    rng = np.random.default_rng(20253)
    cases = []

    vol = open_volume(rng)
    vol[2][3, 5] = NFZ                        # one blocked column, for a blocked start
    goal = pt(30, 14, 5)
    special = [pt(30, 14, 5, 0.9, 0.1, 0.8),  # in the goal voxel
               pt(31, 14, 5),                 # face-adjacent
               pt(31, 14, 6),                 # edge-adjacent
               pt(29, 13, 4),                 # corner-adjacent
               [GEO.x0 - 0.001, 2.8, 200.0],  # outside in x
               [0.5, 2.8, GEO.z0 + GEO.nz * GEO.dz + 1.0],   # outside in z
               [0.5, float("nan"), 200.0],    # by NaN
               pt(5, 3, 7)]                   # in a blocked voxel
    cases.append(case("open3d", vol, [goal], random_starts(rng, 5) + special))

    # a terrain wall across the volume, higher than the centres of layers 0..5
    risk, terrain, flags = blank(0.5)
    risk[...] = rng.uniform(0.2, 1.0, size=risk.shape).astype(np.float32)
    # (eight voxels wide: wider than two waypoint spacings of a straight or arc candidate)
    terrain[:, 18:26] = layer_centre(5) + 1.0
    cases.append(case("ridge", (risk, terrain, flags), [pt(38, 14, 1), pt(36, 5, 0)],
                      [pt(4, 14, 1), pt(6, 25, 0), pt(16, 10, 2), pt(4, 14, 1)],
                      goal_idx=[0, 0, 1, 1]))

    # risk falling with altitude: flying high pays only when the risk weighs enough
    risk, terrain, flags = blank()
    for iz in range(GEO.nz):
        risk[:, :, iz] = 8.0 * 0.5 ** iz
    st = [pt(3, 14, 0), pt(5, 4, 1), pt(2, 25, 0)]
    cases.append(case("layer_tradeoff_lam0", (risk, terrain, flags), [pt(40, 14, 0)], st,
                      lam=0.0))
    cases.append(case("layer_tradeoff_lam50", (risk, terrain, flags), [pt(40, 14, 0)], st,
                      lam=50.0))

    # a one-voxel-thick sheet along the 3-D diagonal ix = iz + 14, blocked voxel by voxel
    # (non-finite risk: the columns stay unflagged), with one gap
    risk, terrain, flags = blank(0.25)
    for iz in range(GEO.nz):
        risk[:, iz + 14, iz] = np.nan
    risk[20, 3 + 14, 3] = 0.25                # the gap
    cases.append(case("diagonal_sheet", (risk, terrain, flags), [pt(35, 8, 2)],
                      [pt(4, 8, 2), pt(15, 20, 2), pt(16, 20, 1), pt(20, 2, 9), pt(2, 27, 10)]))

    # a sealed box round the goal: walls, floor and lid
    risk, terrain, flags = blank(0.25)
    risk[8:19, 10:21, 2:9] = np.inf
    risk[9:18, 11:20, 3:8] = 0.25
    cases.append(case("sealed_box", (risk, terrain, flags), [pt(15, 13, 5)],
                      [pt(2, 2, 2), pt(40, 27, 10), pt(9, 13, 5), pt(15, 13, 9)]))
    cases.append(case("blocked_goal_and_offvolume_goal", (risk, terrain, flags),
                      [pt(10, 13, 5), [9.0, 9.0, 100.0], pt(5, 5, 0, fz=-0.5)],
                      [pt(2, 2, 2), pt(15, 13, 5), pt(2, 2, 2), pt(10, 13, 5), pt(2, 2, 2)],
                      goal_idx=[0, 0, 1, 1, 2]))

    risk, terrain, flags = blank()
    risk[...] = rng.uniform(0.0, 4.0, size=risk.shape).astype(np.float32)
    flags[rng.random(flags.shape) < 0.15] = NFZ
    terrain[...] = rng.uniform(0.0, 150.0, size=terrain.shape).astype(np.float32)
    goals = [pt(5, 5, 6), pt(38, 24, 8), pt(22, 3, 9)]
    for ix, iy in ((5, 5), (38, 24), (22, 3)):
        flags[iy, ix] = 0
    cases.append(case("three_goals", (risk, terrain, flags), goals, random_starts(rng, 10),
                      goal_idx=[0, 1, 2, 3, -1, 2, 1, 0, 1, 2]))

    risk, terrain, flags = blank()
    risk[...] = rng.uniform(0.0, 2.0, size=risk.shape).astype(np.float32)
    flags[rng.random(flags.shape) < 0.02] = NFZ
    terrain[rng.random(terrain.shape) < 0.03] = layer_centre(3) + 1.0
    flags[10:19, 17:26] = 0
    terrain[10:19, 17:26] = 0.0
    cases.append(case("inflate2", (risk, terrain, flags), [pt(21, 14, 5)],
                      random_starts(rng, 8) + [pt(0, 0, 10), pt(42, 28, 0)], inflate=2))

    risk, terrain, flags = open_volume(rng)
    u = rng.random(risk.shape)
    risk[u < 0.04] = np.nan
    risk[(u >= 0.04) & (u < 0.08)] = np.inf
    risk[(u >= 0.08) & (u < 0.12)] = -np.inf
    risk[(u >= 0.12) & (u < 0.16)] = -5.0    # c = -4
    risk[(u >= 0.16) & (u < 0.20)] = -1.0    # c = 0: not > 0
    risk[14, 21, 5] = 1.0
    cases.append(case("nonfinite_risk", (risk, terrain, flags), [pt(21, 14, 5)],
                      random_starts(rng, 10), block_flags=0))

    # 30 % of the columns blocked up to a random height (the rest of the column is free)
    risk, terrain, flags = blank()
    risk[...] = rng.uniform(0.0, 4.0, size=risk.shape).astype(np.float32)
    hit = rng.random(terrain.shape) < 0.3
    height = GEO.z0 + rng.uniform(0.0, GEO.nz * GEO.dz, size=terrain.shape)
    terrain[hit] = height[hit].astype(np.float32)
    terrain[14, 21] = 0.0
    cases.append(case("random30", (risk, terrain, flags), [pt(21, 14, 2)],
                      random_starts(rng, 12), agl=20.0))

    # the bridge to the flat route seeds: one layer whose centre lies above every terrain value
    geo1 = Geo(GEO.nx, GEO.ny, 1, GEO.x0, GEO.y_top, GEO.dx, GEO.dy, 1000.0, 50.0)
    risk, terrain, flags = blank(geo=geo1)
    risk[...] = rng.uniform(0.0, 4.0, size=risk.shape).astype(np.float32)
    flags[rng.random(flags.shape) < 0.25] = NFZ
    terrain[...] = rng.uniform(0.0, 900.0, size=terrain.shape).astype(np.float32)
    flags[14, 21] = 0
    cases.append(case("nz1_bridge", (risk, terrain, flags), [pt(21, 14, 0, geo=geo1)],
                      random_starts(rng, 8, geo=geo1), geo=geo1))
    return cases


CASES = all_cases()
NAMES = [c["name"] for c in CASES]
BY_NAME = {c["name"]: c for c in CASES}


def volume_words(c):
    """The case as the volume buffer's 32-bit words: 8-B voxels {risk, psi_nfz} [ny][nx][nz],
    then at the 256-B aligned column offset the 8-B columns {terrain, flags} [ny][nx] (the
    column bitmap that follows in uam_volume_shape's buffer is not part of it).  psi_nfz is 1
    in a no-fly column, as uam_volume_build writes it."""
    g = c["geo"]
    nvox, ncol = g.nx * g.ny * g.nz, g.nx * g.ny
    col_off = (nvox * 8 + 255) // 256 * 256
    w = np.zeros(col_off // 4 + ncol * 2, dtype=np.uint32)
    vox = w[:nvox * 2].reshape(g.ny, g.nx, g.nz, 2)
    vox[..., 0] = c["risk"].view(np.uint32)
    psi = np.where(c["flags"] & NFZ, np.float32(1.0), np.float32(0.0)).astype(np.float32)
    vox[..., 1] = psi.view(np.uint32)[:, :, None]
    cols = w[col_off // 4:].reshape(g.ny, g.nx, 2)
    cols[..., 0] = c["terrain"].view(np.uint32)
    cols[..., 1] = c["flags"]
    return w


@functools.lru_cache(maxsize=None)
def reference(name):
    """route3d_ref's (dist, next, wp3, status, steps, cost volume) of a case; read-only."""
    c = BY_NAME[name]
    dist, nxt, cost = R.route_field3d(c["geo"], c["risk"], c["terrain"], c["flags"], c["goals"],
                                      c["lam"], c["block_flags"], c["inflate"], c["agl"],
                                      c["kappa"])
    wp, status, steps = R.route_paths3d(c["geo"], cost, nxt, c["goals"], c["starts"],
                                        c["goal_idx"], c["N"], c["kappa"])
    for a in (dist, nxt, wp, status, steps):
        a.setflags(write=False)
    return dist, nxt, wp, status, steps, cost
