"""Independent statement of the volume route seeds' smoothing (include/uampath.h "Route seeds in
the volume, smoothing"): plain Python, the touched voxels by the three brute-force inequalities
over the bounding box, the anchors by "advance while visible", then route3d_ref's vertices and
resampling.  No code shared with the library.

c is route3d_ref's cost volume (nested lists [iy][ix][iz], INF = blocked); voxels are
(ix, iy, iz)."""
import math

import numpy as np

import route3d_ref as R

INF = R.INF
SPAN_MAX = 1024


def touched(a, b):
    """T3(A, B): the voxels of the bounding box that satisfy all three inequalities."""
    (ax, ay, az), (bx, by, bz) = a, b
    dx, dy, dz = bx - ax, by - ay, bz - az
    out = []
    for z in range(min(az, bz), max(az, bz) + 1):
        rz = z - az
        for y in range(min(ay, by), max(ay, by) + 1):
            ry = y - ay
            if 2 * abs(dy * rz - dz * ry) > abs(dy) + abs(dz):
                continue
            for x in range(min(ax, bx), max(ax, bx) + 1):
                rx = x - ax
                if (2 * abs(dx * ry - dy * rx) <= abs(dx) + abs(dy)
                        and 2 * abs(dx * rz - dz * rx) <= abs(dx) + abs(dz)):
                    out.append((x, y, z))
    return out


def los(c, a, b):
    return all(c[y][x][z] != INF for x, y, z in touched(a, b))


def anchors(c, cells, span):
    """Chain indices a_0, a_1, .. of the voxels kept."""
    n = len(cells)
    if n <= 2:
        return []
    A = [1]
    while A[-1] != n - 2:
        a = A[-1]
        j = a
        while j + 1 <= min(a + span, n - 2) and los(c, cells[a], cells[j + 1]):
            j += 1
        assert j > a, "adjacent chain voxels must be visible"
        A.append(j)
    return A


def chain(geo, c, nxt, goals, start, gi):
    """(status, voxels) of one query: route3d_ref.trace's status rules and walk."""
    if not 0 <= gi < len(goals):
        return 4, None
    g = R.voxel_of(geo, *goals[gi])
    if g is None or c[g[1]][g[0]][g[2]] == INF:
        return 4, None
    s = R.voxel_of(geo, float(start[0]), float(start[1]), float(start[2]))
    if s is None or c[s[1]][s[0]][s[2]] == INF:
        return 1, None
    nf = nxt[gi]
    if nf[s[1], s[0], s[2]] == R.NONE:
        return 2, None
    cells = [s]
    while cells[-1] != g:
        if len(cells) >= geo.nx * geo.ny * geo.nz:
            return 3, None
        ix, iy, iz = cells[-1]
        d = R.DIRS[int(nf[iy, ix, iz])]
        cells.append((ix + d[0], iy + d[1], iz + d[2]))
    return 0, cells


def resample(V, N, kappa):
    """route3d_ref.trace's S_i and waypoints for the vertices V; (wp3 [N+2, 3], S_m)."""
    kappa = float(kappa)
    m = len(V) - 1
    S = [0.0]
    for i in range(1, m + 1):
        ex, ey = V[i][0] - V[i - 1][0], V[i][1] - V[i - 1][1]
        ez = (V[i][2] - V[i - 1][2]) * kappa
        S.append(S[i - 1] + math.sqrt((ex * ex + ey * ey) + ez * ez))
    wp = np.empty((N + 2, 3), dtype=np.float64)
    wp[0] = V[0]
    wp[N + 1] = V[m]
    i = 1
    for j in range(1, N + 1):
        t = S[m] * (float(j) / float(N + 1))
        while i < m and not S[i] > t:
            i += 1
        den = S[i] - S[i - 1]
        u = (t - S[i - 1]) / den if den > 0.0 else 0.0
        wp[j] = [V[i - 1][k] + u * (V[i][k] - V[i - 1][k]) for k in range(3)]
    return wp, S[m]


def smooth_paths3d(geo, c, nxt, goals, starts, goal_idx, N, kappa, span):
    """wp3 [Q, N+2, 3], status, steps, vertices [Q] and the lengths S_m [Q] (nan for a nonzero
    status)."""
    assert 1 <= span <= SPAN_MAX
    goals = [tuple(map(float, g)) for g in np.asarray(goals, dtype=np.float64).reshape(-1, 3)]
    starts = np.asarray(starts, dtype=np.float64).reshape(-1, 3)
    Q = len(starts)
    wp = np.empty((Q, N + 2, 3), dtype=np.float64)
    status = np.zeros(Q, dtype=np.int32)
    steps = np.zeros(Q, dtype=np.int32)
    vertices = np.zeros(Q, dtype=np.int32)
    length = np.full(Q, np.nan)
    for q in range(Q):
        gi = int(goal_idx[q])
        st, cells = chain(geo, c, nxt, goals, starts[q], gi)
        status[q] = st
        if st:
            # the straight line and every other output of a nonzero status: route3d_ref's
            wp[q] = R.trace(geo, c, nxt, goals, starts[q], gi, N, kappa)[0]
            continue
        A = anchors(c, cells, span)
        V = ([tuple(float(t) for t in starts[q])] + [R.centre(geo, *cells[a]) for a in A]
             + [goals[gi]])
        wp[q], length[q] = resample(V, N, kappa)
        steps[q] = len(cells)
        vertices[q] = len(V)
    return wp, status, steps, vertices, length
