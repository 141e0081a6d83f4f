"""Independent statement of the joint route field's definition (include/uampath.h "Route seeds,
joint field (K9j)"): plain Python, a heap Dijkstra seeded with every valid goal's cell over
route_ref's own cost, blocking and edge functions, the next hop by the lowest-k rule with
membership in Gc as the goal test, the owner by walking every chain to its end, the paths by
route_ref / route_smooth_ref applied to the resolved goal.  No code shared with the library.

rec, geo and the cost plane c are route_ref's."""
import heapq

import numpy as np

import route_ref as R
import route_smooth_ref as S

INF = R.INF


def goal_cells(geo, c, goals):
    """g_i of every goal ((ix, iy), None for an invalid goal) and Gc as {cell: lowest index}."""
    cells, gc = [], {}
    for i, g in enumerate(goals):
        v = R.cell_of(geo, g[0], g[1])
        if v is not None and c[v[1]][v[0]] == INF:
            v = None
        cells.append(v)
        if v is not None and v not in gc:
            gc[v] = i
    return cells, gc


def field(geo, c, goals):
    """(dist [ny, nx] float64, next [ny, nx] uint8, owner [ny, nx] int32) of the goals jointly."""
    nx, ny = geo.nx, geo.ny
    L = R.step_lengths(geo)
    _, gc = goal_cells(geo, c, goals)
    dist = [[INF] * nx for _ in range(ny)]
    heap = []
    for ix, iy in gc:
        dist[iy][ix] = 0.0
        heap.append((0.0, ix, iy))
    heapq.heapify(heap)
    while heap:
        d, ux, uy = heapq.heappop(heap)
        if d > dist[uy][ux]:
            continue
        cu = c[uy][ux]
        for k in range(8):
            if not R.has_edge(c, nx, ny, ux, uy, k):
                continue
            vx, vy = ux + R.DIRS[k][0], uy + R.DIRS[k][1]
            t = d + R.weight(cu, c[vy][vx], L[k])
            if t < dist[vy][vx]:
                dist[vy][vx] = t
                heapq.heappush(heap, (t, vx, vy))
    nxt = np.full((ny, nx), 255, dtype=np.uint8)
    for iy in range(ny):
        for ix in range(nx):
            dv = dist[iy][ix]
            if dv == INF:
                continue
            if (ix, iy) in gc:
                nxt[iy, ix] = 8
                continue
            for k in range(8):
                if R.has_edge(c, nx, ny, ix, iy, k):
                    ux, uy = ix + R.DIRS[k][0], iy + R.DIRS[k][1]
                    if dist[uy][ux] + R.weight(c[uy][ux], c[iy][ix], L[k]) == dv:
                        nxt[iy, ix] = k
                        break
    # owner: walk the chain of every cell.  known[cell] = (owner, hops to its goal cell) of a
    # cell whose chain has been walked before: a chain that meets one ends as that cell's does
    # (the chain from a cell on is a function of the cell).  A walk of nx*ny cells without
    # meeting Gc has no owner, and neither has any cell on it.
    owner = np.full((ny, nx), -1, dtype=np.int32)
    known = {v: (i, 0) for v, i in gc.items()}
    longest = 0
    for iy in range(ny):
        for ix in range(nx):
            if nxt[iy, ix] == 255 or (ix, iy) in known:
                continue
            walk = [(ix, iy)]
            x, y = ix, iy
            end = (-1, 0)
            while len(walk) <= nx * ny:
                k = int(nxt[y, x])
                assert k < 8, "a cell with a direction leads to cells with a route"
                x, y = x + R.DIRS[k][0], y + R.DIRS[k][1]
                if (x, y) in known:
                    end = known[(x, y)]
                    break
                walk.append((x, y))
            for hops, v in enumerate(reversed(walk), 1):
                known[v] = (end[0], end[1] + hops if end[0] >= 0 else 0)
    for (x, y), (o, hops) in known.items():
        owner[y, x] = o
        longest = max(longest, hops)
    return np.array(dist, dtype=np.float64), nxt, owner, longest


def paths(geo, c, nxt, owner, goals, starts, N, span):
    """wp [Q, N+2, 2], status, steps, vertices, goal [Q] of the start points; span 0 is the
    plain trace (route_ref), span >= 1 the shortcuts (route_smooth_ref)."""
    goals = [tuple(map(float, g)) for g in np.asarray(goals, dtype=np.float64).reshape(-1, 2)]
    starts = np.asarray(starts, dtype=np.float64).reshape(-1, 2)
    Q = len(starts)
    wp = np.empty((Q, N + 2, 2), dtype=np.float64)
    status = np.zeros(Q, dtype=np.int32)
    steps = np.zeros(Q, dtype=np.int32)
    vertices = np.zeros(Q, dtype=np.int32)
    goal = np.full(Q, -1, dtype=np.int32)
    plane = nxt[None]
    for q in range(Q):
        sx, sy = float(starts[q][0]), float(starts[q][1])
        s = R.cell_of(geo, sx, sy)
        if s is None or c[s[1]][s[0]] == INF:
            st = 1
        elif nxt[s[1], s[0]] == 255:
            st = 2
        elif owner[s[1], s[0]] < 0:
            st = 3
        else:
            st = 0
        status[q] = st
        if st:
            wp[q] = (sx, sy)
            continue
        o = int(owner[s[1], s[0]])
        goal[q] = o
        # the existing calls on the one joint plane, with the resolved goal as their only goal
        if span == 0:
            wp[q], st0, steps[q] = R.trace(geo, c, plane, [goals[o]], starts[q], 0, N)
            vertices[q] = max(int(steps[q]), 2)
        else:
            w, s1, n1, v1, _ = S.smooth_paths(geo, c, plane, [goals[o]], [starts[q]], [0], N, span)
            wp[q], st0, steps[q], vertices[q] = w[0], int(s1[0]), n1[0], v1[0]
        assert st0 == 0, "a start with an owner reaches that owner's goal"
    return wp, status, steps, vertices, goal
