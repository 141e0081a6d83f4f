"""Independent statement of the route seeds' definition (include/uampath.h "Route seeds"):
plain Python / numpy, a heap Dijkstra, no code shared with the library.  Python floats are IEEE
float64 and never fused, so every operation below is rounded separately, in the order written.

rec is the record raster as float32 words [ny, nx, 4] = {phi, psi_nfz, dem, flags} (the flags
word viewed as uint32); geo is anything with nx, ny, x0, y_top, dx, dy."""
import heapq
import math

import numpy as np

INF = float("inf")
# k = 0..7: E, NE, N, NW, W, SW, S, SE as (dix, diy); row 0 is the northern edge
DIRS = ((1, 0), (1, -1), (0, -1), (-1, -1), (-1, 0), (-1, 1), (0, 1), (1, 1))


def step_lengths(geo):
    dx, dy = float(geo.dx), float(geo.dy)
    diag = math.sqrt(dx * dx + dy * dy)
    return (dx, diag, dy, diag, dx, diag, dy, diag)


def cell_of(geo, x, y):
    """(ix, iy) of a point, None off the raster."""
    x, y = float(x), float(y)
    tx = (x - float(geo.x0)) * (1.0 / float(geo.dx))
    ty = (float(geo.y_top) - y) * (1.0 / float(geo.dy))
    if math.isnan(tx) or math.isnan(ty) or math.isinf(tx) or math.isinf(ty):
        return None
    ix, iy = math.floor(tx), math.floor(ty)
    if 0 <= ix < geo.nx and 0 <= iy < geo.ny:
        return ix, iy
    return None


def centre(geo, ix, iy):
    return (float(geo.x0) + (ix + 0.5) * float(geo.dx),
            float(geo.y_top) - (iy + 0.5) * float(geo.dy))


def cost_plane(geo, rec, lam, block_flags, inflate):
    """c [ny][nx] as nested lists of Python floats, INF where the cell is blocked."""
    rec = np.asarray(rec)
    phi = rec[..., 0].view(np.float32).astype(np.float64)
    flags = rec[..., 3].view(np.uint32)
    ny, nx = geo.ny, geo.nx
    lam = float(lam)
    c = [[0.0] * nx for _ in range(ny)]
    blocked0 = [[False] * nx for _ in range(ny)]
    for iy in range(ny):
        for ix in range(nx):
            cv = 1.0 + lam * float(phi[iy, ix])
            b = (int(flags[iy, ix]) & int(block_flags)) != 0
            if b or math.isnan(cv) or math.isinf(cv) or not cv > 0.0:
                blocked0[iy][ix] = True
            c[iy][ix] = cv
    for iy in range(ny):
        for ix in range(nx):
            hit = False
            for y in range(max(0, iy - inflate), min(ny - 1, iy + inflate) + 1):
                row = blocked0[y]
                for x in range(max(0, ix - inflate), min(nx - 1, ix + inflate) + 1):
                    if row[x]:
                        hit = True
                        break
                if hit:
                    break
            if hit:
                c[iy][ix] = INF
    return c


def has_edge(c, nx, ny, ix, iy, k):
    """Whether the free cell (ix, iy) has an edge to its neighbour in direction k."""
    dix, diy = DIRS[k]
    ux, uy = ix + dix, iy + diy
    if not (0 <= ux < nx and 0 <= uy < ny) or c[uy][ux] == INF:
        return False
    if dix != 0 and diy != 0 and (c[iy][ux] == INF or c[uy][ix] == INF):
        return False
    return True


def weight(cu, cv, length):
    return (0.5 * (cu + cv)) * length


def field(geo, c, goal):
    """(dist [ny][nx] float64 array, next [ny][nx] uint8 array) of one goal point."""
    nx, ny = geo.nx, geo.ny
    L = step_lengths(geo)
    dist = [[INF] * nx for _ in range(ny)]
    g = cell_of(geo, goal[0], goal[1])
    if g is not None and c[g[1]][g[0]] == INF:
        g = None
    if g is not None:
        dist[g[1]][g[0]] = 0.0
        heap = [(0.0, g[0], g[1])]
        while heap:
            d, ux, uy = heapq.heappop(heap)
            if d > dist[uy][ux]:
                continue
            cu = c[uy][ux]
            for k in range(8):
                if not has_edge(c, nx, ny, ux, uy, k):
                    continue
                vx, vy = ux + DIRS[k][0], uy + DIRS[k][1]
                t = d + weight(cu, c[vy][vx], L[k])
                if t < dist[vy][vx]:
                    dist[vy][vx] = t
                    heapq.heappush(heap, (t, vx, vy))
    nxt = np.full((ny, nx), 255, dtype=np.uint8)
    for iy in range(ny):
        for ix in range(nx):
            dv = dist[iy][ix]
            if dv == INF:
                continue
            if (ix, iy) == g:
                nxt[iy, ix] = 8
                continue
            for k in range(8):
                if has_edge(c, nx, ny, ix, iy, k):
                    ux, uy = ix + DIRS[k][0], iy + DIRS[k][1]
                    if dist[uy][ux] + weight(c[uy][ux], c[iy][ix], L[k]) == dv:
                        nxt[iy, ix] = k
                        break
    return np.array(dist, dtype=np.float64), nxt


def route_field(geo, rec, goals, lam=1.0, block_flags=1, inflate=0):
    """dist [G, ny, nx] float64, next [G, ny, nx] uint8 and the cost plane."""
    c = cost_plane(geo, rec, lam, block_flags, inflate)
    out = [field(geo, c, g) for g in np.asarray(goals, dtype=np.float64).reshape(-1, 2)]
    return (np.stack([d for d, _ in out]), np.stack([n for _, n in out]), c)


def trace(geo, c, nxt, goals, start, gi, N):
    """(wp [N+2, 2], status, steps) of one query."""
    sx, sy = float(start[0]), float(start[1])
    n_goals = len(goals)
    wp = np.empty((N + 2, 2), dtype=np.float64)

    def straight(status, gx, gy):
        wp[0] = (sx, sy)
        wp[N + 1] = (gx, gy)
        for j in range(1, N + 1):
            f = float(j) / float(N + 1)
            wp[j] = (sx + (gx - sx) * f, sy + (gy - sy) * f)
        return wp, status, 0

    if not 0 <= gi < n_goals:
        return straight(4, sx, sy)
    gx, gy = float(goals[gi][0]), float(goals[gi][1])
    g = cell_of(geo, gx, gy)
    if g is None or c[g[1]][g[0]] == INF:
        return straight(4, gx, gy)
    s = cell_of(geo, sx, sy)
    if s is None or c[s[1]][s[0]] == INF:
        return straight(1, gx, gy)
    nf = nxt[gi]
    if nf[s[1], s[0]] == 255:
        return straight(2, gx, gy)
    cells = [s]
    while cells[-1] != g:
        if len(cells) >= geo.nx * geo.ny:
            return straight(3, gx, gy)
        ix, iy = cells[-1]
        k = int(nf[iy, ix])
        cells.append((ix + DIRS[k][0], iy + DIRS[k][1]))
    V = [(sx, sy)] + [centre(geo, ix, iy) for ix, iy in cells[1:-1]] + [(gx, gy)]
    m = len(V) - 1
    S = [0.0]
    for i in range(1, m + 1):
        ex, ey = V[i][0] - V[i - 1][0], V[i][1] - V[i - 1][1]
        S.append(S[i - 1] + math.sqrt(ex * ex + ey * ey))
    wp[0] = V[0]
    wp[N + 1] = V[m]
    i = 1
    for j in range(1, N + 1):
        t = S[m] * (float(j) / float(N + 1))
        while i < m and not S[i] > t:
            i += 1
        den = S[i] - S[i - 1]
        u = (t - S[i - 1]) / den if den > 0.0 else 0.0
        wp[j] = (V[i - 1][0] + u * (V[i][0] - V[i - 1][0]),
                 V[i - 1][1] + u * (V[i][1] - V[i - 1][1]))
    return wp, 0, len(cells)


def route_paths(geo, c, nxt, goals, starts, goal_idx, N):
    goals = [tuple(map(float, g)) for g in np.asarray(goals, dtype=np.float64).reshape(-1, 2)]
    starts = np.asarray(starts, dtype=np.float64).reshape(-1, 2)
    Q = len(starts)
    wp = np.empty((Q, N + 2, 2), dtype=np.float64)
    status = np.empty(Q, dtype=np.int32)
    steps = np.empty(Q, dtype=np.int32)
    for q in range(Q):
        wp[q], status[q], steps[q] = trace(geo, c, nxt, goals, starts[q], int(goal_idx[q]), N)
    return wp, status, steps
