"""Independent statement of the volume's joint route field (include/uampath.h "Route seeds in the
volume, joint field (K9vj)"): plain Python, a heap Dijkstra seeded with every valid goal's voxel
over route3d_ref's own cost volume, edge rule and weight, the next hop by the lowest-k rule with
membership in Gc as the goal test, the owner by walking every chain to its end, the paths by
route3d_ref / route3d_smooth_ref applied to the resolved goal.  No code shared with the library.

geo, the cost volume c (nested lists [iy][ix][iz], INF = blocked) and voxels (ix, iy, iz) are
route3d_ref's."""
import heapq

import numpy as np

import route3d_ref as R
import route3d_smooth_ref as S

INF = R.INF


def goal_voxels(geo, c, goals):
    """g_i of every goal ((ix, iy, iz), None for an invalid goal) and Gc as {voxel: lowest
    index}."""
    voxels, gc = [], {}
    for i, g in enumerate(np.asarray(goals, dtype=np.float64).reshape(-1, 3)):
        v = R.voxel_of(geo, float(g[0]), float(g[1]), float(g[2]))
        if v is not None and c[v[1]][v[0]][v[2]] == INF:
            v = None
        voxels.append(v)
        if v is not None and v not in gc:
            gc[v] = i
    return voxels, gc


def _step(v, k):
    return v[0] + R.DIRS[k][0], v[1] + R.DIRS[k][1], v[2] + R.DIRS[k][2]


def field(geo, c, goals, kappa):
    """(dist [ny, nx, nz] float64, next [ny, nx, nz] uint8, owner [ny, nx, nz] int32, the longest
    chain in hops) of the goals jointly."""
    nx, ny, nz = geo.nx, geo.ny, geo.nz
    L = R.step_lengths(geo, kappa)
    _, gc = goal_voxels(geo, c, goals)
    d = {v: 0.0 for v in gc}
    heap = [(0.0, v) for v in gc]
    heapq.heapify(heap)
    while heap:
        du, u = heapq.heappop(heap)
        if du > d[u]:
            continue
        cu = c[u[1]][u[0]][u[2]]
        for k in range(26):
            if not R.has_edge(geo, c, u, k):
                continue
            v = _step(u, k)
            t = du + R.weight(cu, c[v[1]][v[0]][v[2]], L[k])
            if t < d.get(v, INF):
                d[v] = t
                heapq.heappush(heap, (t, v))
    dist = np.full((ny, nx, nz), INF, dtype=np.float64)
    nxt = np.full((ny, nx, nz), R.NONE, dtype=np.uint8)
    for v, dv in d.items():
        dist[v[1], v[0], v[2]] = dv
        if v in gc:
            nxt[v[1], v[0], v[2]] = R.GOAL
            continue
        cv = c[v[1]][v[0]][v[2]]
        for k in range(26):
            if R.has_edge(geo, c, v, k):
                u = _step(v, k)
                if u in d and d[u] + R.weight(c[u[1]][u[0]][u[2]], cv, L[k]) == dv:
                    nxt[v[1], v[0], v[2]] = k
                    break
    # owner: walk the chain of every voxel.  known[voxel] = (owner, hops to its goal voxel) of a
    # voxel whose chain has been walked before: a chain that meets one ends as that voxel's does
    # (the chain from a voxel on is a function of the voxel).  A walk of nx*ny*nz voxels without
    # meeting Gc has no owner, and neither has any voxel on it.
    owner = np.full((ny, nx, nz), -1, dtype=np.int32)
    known = {v: (i, 0) for v, i in gc.items()}
    longest = 0
    for v0 in d:
        if v0 in known or nxt[v0[1], v0[0], v0[2]] == R.NONE:
            continue
        walk = [v0]
        v = v0
        end = (-1, 0)
        while len(walk) <= nx * ny * nz:
            k = int(nxt[v[1], v[0], v[2]])
            assert k < 26, "a voxel with a direction leads to voxels with a route"
            v = _step(v, k)
            if v in known:
                end = known[v]
                break
            walk.append(v)
        for hops, w in enumerate(reversed(walk), 1):
            known[w] = (end[0], end[1] + hops if end[0] >= 0 else 0)
    for (x, y, z), (o, hops) in known.items():
        owner[y, x, z] = o
        longest = max(longest, hops)
    return dist, nxt, owner, longest


def paths(geo, c, nxt, owner, goals, starts, N, kappa, span):
    """wp3 [Q, N+2, 3], status, steps, vertices, goal [Q] of the start points; span 0 is the
    plain trace (route3d_ref), span >= 1 the shortcuts (route3d_smooth_ref)."""
    goals = [tuple(map(float, g)) for g in np.asarray(goals, dtype=np.float64).reshape(-1, 3)]
    starts = np.asarray(starts, dtype=np.float64).reshape(-1, 3)
    Q = len(starts)
    wp = np.empty((Q, N + 2, 3), dtype=np.float64)
    status = np.zeros(Q, dtype=np.int32)
    steps = np.zeros(Q, dtype=np.int32)
    vertices = np.zeros(Q, dtype=np.int32)
    goal = np.full(Q, -1, dtype=np.int32)
    volume = nxt[None]
    for q in range(Q):
        s_pt = tuple(float(t) for t in starts[q])
        s = R.voxel_of(geo, *s_pt)
        if s is None or c[s[1]][s[0]][s[2]] == INF:
            st = 1
        elif nxt[s[1], s[0], s[2]] == R.NONE:
            st = 2
        elif owner[s[1], s[0], s[2]] < 0:
            st = 3
        else:
            st = 0
        status[q] = st
        if st:
            wp[q] = s_pt
            continue
        o = int(owner[s[1], s[0], s[2]])
        goal[q] = o
        # the existing calls on the one joint volume, with the resolved goal as their only goal
        if span == 0:
            wp[q], st0, steps[q] = R.trace(geo, c, volume, [goals[o]], starts[q], 0, N, kappa)
            vertices[q] = max(int(steps[q]), 2)
        else:
            w, s1, n1, v1, _ = S.smooth_paths3d(geo, c, volume, [goals[o]], [starts[q]], [0], N,
                                                kappa, span)
            wp[q], st0, steps[q], vertices[q] = w[0], int(s1[0]), n1[0], v1[0]
        assert st0 == 0, "a start with an owner reaches that owner's goal"
    return wp, status, steps, vertices, goal
