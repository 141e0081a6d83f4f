"""Independent statement of the volume route seeds' definition (include/uampath.h "Route seeds
in the volume"): plain Python / numpy, a heap Dijkstra, no code shared with the library and none
with tests/route_ref.py.  Python floats are IEEE float64 and never fused, so every operation
below is rounded separately, in the order written.

A volume is given as risk [ny, nx, nz] float32, terrain [ny, nx] float32 and flags [ny, nx]
uint32; geo is anything with nx, ny, nz, x0, y_top, dx, dy, z0, dz.  A voxel is the tuple
(ix, iy, iz); planes are dicts or nested lists indexed [iy][ix][iz]."""
import heapq
import math

import numpy as np

INF = float("inf")
# the eight lateral steps: E, NE, N, NW, W, SW, S, SE (row 0 is the northern edge)
_LATERAL = ((1, 0), (1, -1), (0, -1), (-1, -1), (-1, 0), (-1, 1), (0, 1), (1, 1))
# k = 0..25: level, climbing, descending, straight up, straight down
DIRS = (tuple((a, b, 0) for a, b in _LATERAL) + tuple((a, b, 1) for a, b in _LATERAL) +
        tuple((a, b, -1) for a, b in _LATERAL) + ((0, 0, 1), (0, 0, -1)))
GOAL, NONE = 26, 255


def step_lengths(geo, kappa):
    dx, dy = float(geo.dx), float(geo.dy)
    vz = float(geo.dz) * float(kappa)
    out = []
    for a, b, c in DIRS:
        hx = dx if a else 0.0
        hy = dy if b else 0.0
        hz = vz if c else 0.0
        out.append(math.sqrt((hx * hx + hy * hy) + hz * hz))
    return tuple(out)


def _floor_index(t, n):
    if math.isnan(t) or math.isinf(t):
        return None
    i = math.floor(t)
    return i if 0 <= i < n else None


def voxel_of(geo, x, y, z):
    """(ix, iy, iz) of a point, None outside the volume."""
    ix = _floor_index((float(x) - float(geo.x0)) * (1.0 / float(geo.dx)), geo.nx)
    iy = _floor_index((float(geo.y_top) - float(y)) * (1.0 / float(geo.dy)), geo.ny)
    iz = _floor_index((float(z) - float(geo.z0)) * (1.0 / float(geo.dz)), geo.nz)
    if ix is None or iy is None or iz is None:
        return None
    return ix, iy, iz


def centre(geo, ix, iy, iz):
    return (float(geo.x0) + (ix + 0.5) * float(geo.dx),
            float(geo.y_top) - (iy + 0.5) * float(geo.dy),
            float(geo.z0) + (iz + 0.5) * float(geo.dz))


def cost_volume(geo, risk, terrain, flags, lam, block_flags, inflate, agl):
    """c [ny][nx][nz] as nested lists of Python floats, INF where the voxel is blocked."""
    nx, ny, nz = geo.nx, geo.ny, geo.nz
    lam, agl = float(lam), float(agl)
    risk = np.asarray(risk, dtype=np.float32).astype(np.float64)
    terrain = np.asarray(terrain, dtype=np.float32).astype(np.float64)
    flags = np.asarray(flags).astype(np.uint32)
    c = [[[0.0] * nz for _ in range(nx)] for _ in range(ny)]
    b0 = [[[False] * nz for _ in range(nx)] for _ in range(ny)]
    for iy in range(ny):
        for ix in range(nx):
            flagged = (int(flags[iy, ix]) & int(block_flags)) != 0
            floor_z = float(terrain[iy, ix]) + agl
            for iz in range(nz):
                cv = 1.0 + lam * float(risk[iy, ix, iz])
                low = float(geo.z0) + (float(iz) + 0.5) * float(geo.dz) < floor_z
                c[iy][ix][iz] = cv
                b0[iy][ix][iz] = (flagged or low or math.isnan(cv) or math.isinf(cv)
                                  or not cv > 0.0)
    for iy in range(ny):
        ys = range(max(0, iy - inflate), min(ny - 1, iy + inflate) + 1)
        for ix in range(nx):
            xs = range(max(0, ix - inflate), min(nx - 1, ix + inflate) + 1)
            for iz in range(nz):
                if any(b0[y][x][iz] for y in ys for x in xs):
                    c[iy][ix][iz] = INF
    return c


def has_edge(geo, c, v, k):
    """Whether the free voxel v has an edge to its neighbour in direction k: the neighbour is
    inside the volume and every voxel of the box the two span is free."""
    ix, iy, iz = v
    a, b, d = DIRS[k]
    if not (0 <= ix + a < geo.nx and 0 <= iy + b < geo.ny and 0 <= iz + d < geo.nz):
        return False
    for x in {ix, ix + a}:
        for y in {iy, iy + b}:
            for z in {iz, iz + d}:
                if c[y][x][z] == INF:
                    return False
    return True


def weight(cu, cv, length):
    return (0.5 * (cu + cv)) * length


def field(geo, c, goal, kappa):
    """(dist [ny, nx, nz] float64, next [ny, nx, nz] uint8) of one goal point."""
    nx, ny, nz = geo.nx, geo.ny, geo.nz
    L = step_lengths(geo, kappa)
    dist = np.full((ny, nx, nz), INF, dtype=np.float64)
    d = {}
    g = voxel_of(geo, *goal)
    if g is not None and c[g[1]][g[0]][g[2]] == INF:
        g = None
    if g is not None:
        d[g] = 0.0
        heap = [(0.0, g)]
        while heap:
            du, u = heapq.heappop(heap)
            if du > d[u]:
                continue
            cu = c[u[1]][u[0]][u[2]]
            for k in range(26):
                if not has_edge(geo, c, u, k):
                    continue
                v = (u[0] + DIRS[k][0], u[1] + DIRS[k][1], u[2] + DIRS[k][2])
                t = du + weight(cu, c[v[1]][v[0]][v[2]], L[k])
                if t < d.get(v, INF):
                    d[v] = t
                    heapq.heappush(heap, (t, v))
    nxt = np.full((ny, nx, nz), NONE, dtype=np.uint8)
    for v, dv in d.items():
        dist[v[1], v[0], v[2]] = dv
        if v == g:
            nxt[v[1], v[0], v[2]] = GOAL
            continue
        cv = c[v[1]][v[0]][v[2]]
        for k in range(26):
            if has_edge(geo, c, v, k):
                u = (v[0] + DIRS[k][0], v[1] + DIRS[k][1], v[2] + DIRS[k][2])
                if u in d and d[u] + weight(c[u[1]][u[0]][u[2]], cv, L[k]) == dv:
                    nxt[v[1], v[0], v[2]] = k
                    break
    return dist, nxt


def route_field3d(geo, risk, terrain, flags, goals, lam=1.0, block_flags=1, inflate=0, agl=0.0,
                  kappa=1e-3):
    """dist [G, ny, nx, nz] float64, next [G, ny, nx, nz] uint8 and the cost volume."""
    c = cost_volume(geo, risk, terrain, flags, lam, block_flags, inflate, agl)
    out = [field(geo, c, g, kappa) for g in np.asarray(goals, dtype=np.float64).reshape(-1, 3)]
    return np.stack([a for a, _ in out]), np.stack([b for _, b in out]), c


def trace(geo, c, nxt, goals, start, gi, N, kappa):
    """(wp3 [N+2, 3], status, steps) of one query."""
    s_pt = tuple(float(t) for t in start)
    kappa = float(kappa)
    wp = np.empty((N + 2, 3), dtype=np.float64)

    def straight(status, g_pt):
        wp[0] = s_pt
        wp[N + 1] = g_pt
        for j in range(1, N + 1):
            f = float(j) / float(N + 1)
            wp[j] = [s_pt[i] + (g_pt[i] - s_pt[i]) * f for i in range(3)]
        return wp, status, 0

    if not 0 <= gi < len(goals):
        return straight(4, s_pt)
    g_pt = tuple(float(t) for t in goals[gi])
    g = voxel_of(geo, *g_pt)
    if g is None or c[g[1]][g[0]][g[2]] == INF:
        return straight(4, g_pt)
    s = voxel_of(geo, *s_pt)
    if s is None or c[s[1]][s[0]][s[2]] == INF:
        return straight(1, g_pt)
    nf = nxt[gi]
    if nf[s[1], s[0], s[2]] == NONE:
        return straight(2, g_pt)
    chain = [s]
    while chain[-1] != g:
        if len(chain) >= geo.nx * geo.ny * geo.nz:
            return straight(3, g_pt)
        ix, iy, iz = chain[-1]
        a, b, d = DIRS[int(nf[iy, ix, iz])]
        chain.append((ix + a, iy + b, iz + d))
    V = [s_pt] + [centre(geo, *v) for v in chain[1:-1]] + [g_pt]
    m = len(V) - 1
    S = [0.0]
    for i in range(1, m + 1):
        ex, ey = V[i][0] - V[i - 1][0], V[i][1] - V[i - 1][1]
        ez = (V[i][2] - V[i - 1][2]) * kappa
        S.append(S[i - 1] + math.sqrt((ex * ex + ey * ey) + ez * ez))
    wp[0] = V[0]
    wp[N + 1] = V[m]
    i = 1
    for j in range(1, N + 1):
        t = S[m] * (float(j) / float(N + 1))
        while i < m and not S[i] > t:
            i += 1
        den = S[i] - S[i - 1]
        u = (t - S[i - 1]) / den if den > 0.0 else 0.0
        wp[j] = [V[i - 1][n] + u * (V[i][n] - V[i - 1][n]) for n in range(3)]
    return wp, 0, len(chain)


def route_paths3d(geo, c, nxt, goals, starts, goal_idx, N, kappa):
    goals = [tuple(map(float, g)) for g in np.asarray(goals, dtype=np.float64).reshape(-1, 3)]
    starts = np.asarray(starts, dtype=np.float64).reshape(-1, 3)
    Q = len(starts)
    wp = np.empty((Q, N + 2, 3), dtype=np.float64)
    status = np.empty(Q, dtype=np.int32)
    steps = np.empty(Q, dtype=np.int32)
    for q in range(Q):
        wp[q], status[q], steps[q] = trace(geo, c, nxt, goals, starts[q], int(goal_idx[q]), N,
                                           kappa)
    return wp, status, steps
