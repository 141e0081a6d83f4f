"""Independent statement of the route seeds' smoothing (include/uampath.h "Route seeds,
smoothing"): plain Python, the touched cells by the brute-force inequality over the bounding
box, the anchors by "advance while visible", then route_ref's vertices and resampling.  No code
shared with the library.

c is route_ref's cost plane (nested lists, INF = blocked); cells are (ix, iy)."""
import math

import numpy as np

import route_ref as R

INF = R.INF
SPAN_MAX = 1024


def touched(a, b):
    """T(A, B): the cells of the bounding box with 2*|dx*(y-ay) - dy*(x-ax)| <= |dx| + |dy|."""
    (ax, ay), (bx, by) = a, b
    dx, dy = bx - ax, by - ay
    lim = abs(dx) + abs(dy)
    return [(x, y)
            for y in range(min(ay, by), max(ay, by) + 1)
            for x in range(min(ax, bx), max(ax, bx) + 1)
            if 2 * abs(dx * (y - ay) - dy * (x - ax)) <= lim]


def los(c, a, b):
    return all(c[y][x] != INF for x, y in touched(a, b))


def anchors(c, cells, span):
    """Chain indices a_0, a_1, .. of the cells kept."""
    n = len(cells)
    if n <= 2:
        return []
    A = [1]
    while A[-1] != n - 2:
        a = A[-1]
        j = a
        while j + 1 <= min(a + span, n - 2) and los(c, cells[a], cells[j + 1]):
            j += 1
        assert j > a, "adjacent chain cells must be visible"
        A.append(j)
    return A


def chain(geo, c, nxt, goals, start, gi):
    """(status, cells) of one query: route_ref.trace's status rules and walk."""
    sx, sy = float(start[0]), float(start[1])
    if not 0 <= gi < len(goals):
        return 4, None
    g = R.cell_of(geo, goals[gi][0], goals[gi][1])
    if g is None or c[g[1]][g[0]] == INF:
        return 4, None
    s = R.cell_of(geo, sx, sy)
    if s is None or c[s[1]][s[0]] == INF:
        return 1, None
    nf = nxt[gi]
    if nf[s[1], s[0]] == 255:
        return 2, None
    cells = [s]
    while cells[-1] != g:
        if len(cells) >= geo.nx * geo.ny:
            return 3, None
        ix, iy = cells[-1]
        k = int(nf[iy, ix])
        cells.append((ix + R.DIRS[k][0], iy + R.DIRS[k][1]))
    return 0, cells


def resample(V, N):
    """route_ref.trace's S_i and waypoints for the vertices V; (wp [N+2, 2], S_m)."""
    m = len(V) - 1
    S = [0.0]
    for i in range(1, m + 1):
        ex, ey = V[i][0] - V[i - 1][0], V[i][1] - V[i - 1][1]
        S.append(S[i - 1] + math.sqrt(ex * ex + ey * ey))
    wp = np.empty((N + 2, 2), dtype=np.float64)
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
    return wp, S[m]


def smooth_paths(geo, c, nxt, goals, starts, goal_idx, N, span):
    """wp [Q, N+2, 2], status, steps, vertices [Q] and the lengths S_m [Q] (nan for a nonzero
    status)."""
    assert 1 <= span <= SPAN_MAX
    goals = [tuple(map(float, g)) for g in np.asarray(goals, dtype=np.float64).reshape(-1, 2)]
    starts = np.asarray(starts, dtype=np.float64).reshape(-1, 2)
    Q = len(starts)
    wp = np.empty((Q, N + 2, 2), dtype=np.float64)
    status = np.zeros(Q, dtype=np.int32)
    steps = np.zeros(Q, dtype=np.int32)
    vertices = np.zeros(Q, dtype=np.int32)
    length = np.full(Q, np.nan)
    for q in range(Q):
        gi = int(goal_idx[q])
        st, cells = chain(geo, c, nxt, goals, starts[q], gi)
        status[q] = st
        if st:
            # the straight line and every other output of a nonzero status: route_ref's
            wp[q] = R.trace(geo, c, nxt, goals, starts[q], gi, N)[0]
            continue
        A = anchors(c, cells, span)
        V = ([(float(starts[q][0]), float(starts[q][1]))]
             + [R.centre(geo, *cells[a]) for a in A] + [goals[gi]])
        wp[q], length[q] = resample(V, N)
        steps[q] = len(cells)
        vertices[q] = len(V)
    return wp, status, steps, vertices, length
