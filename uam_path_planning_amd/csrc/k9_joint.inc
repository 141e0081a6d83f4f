// k9_joint.inc -- K9j, the joint route field: one cost-to-go field to the nearest of many goals,
// the owner of every cell and the seed paths to the owning goal (include/uampath.h "Route seeds,
// joint field").  k_route_joint_clear, k_route_joint_seed (the start state of all goals at once),
// k_route_joint_next, k_route_joint_mark, k_route_joint_parent, k_owner_jump, k_owner_final (the
// owner by pointer jumping), k_route_joint_trace, k_route_joint_smooth, and the host twin of the
// field.  The relaxation is k_route_relax<T> itself: nothing in it knows how many cells start at 0.
// Included in the anonymous namespace of uampath.hip, after k9_smooth.inc.

constexpr int32_t R9J_GOALS_MAX = 1 << 20;
constexpr int32_t R9J_NO_GOAL = INT32_MAX;  // a root's goal index before the goals' atomicMin

// the cell of goal i when the goal is valid (on the raster and free), else -1
__host__ __device__ __forceinline__ int32_t r9j_goal_cell(const KRoute& g, const double* c,
                                                          const double* goals, int64_t i) {
    const int32_t gcell = r9_cell(g, goals[2 * i], goals[2 * i + 1]);
    return gcell >= 0 && c[gcell] < r9_inf() ? gcell : -1;
}

// ---- the field's start state ----------------------------------------------------------------
// dist = +inf everywhere, both tile-flag planes cleared, both lists empty
__global__ __launch_bounds__(R9_THREADS) void k_route_joint_clear(KRoute g,
                                                                  double* __restrict__ dist,
                                                                  int ntiles,
                                                                  uint32_t* __restrict__ flags,
                                                                  int32_t* __restrict__ ctl) {
    const int64_t n = (int64_t)g.nx * g.ny;
    const int64_t i0 = (int64_t)blockIdx.x * R9_THREADS + threadIdx.x;
    const int64_t step = (int64_t)gridDim.x * R9_THREADS;
    for (int64_t i = i0; i < n; i += step) dist[i] = r9_inf();
    for (int64_t i = i0; i < 2 * (int64_t)ntiles; i += step) flags[i] = 0u;
    if (i0 == 0) ctl[0] = ctl[1] = 0;
}

// One lane per goal: dist = 0 at the cell of a valid goal (goals that share a cell store the same
// word) and the cell's tile into list 0, once: the tile's flag of plane 0 is taken with atomicExch
// as k_route_relax enters tiles, so the list holds distinct tiles (at most ntiles entries) however
// many goals there are and however they repeat.  The round that visits the tile clears the flag.
__global__ __launch_bounds__(R9_THREADS) void k_route_joint_seed(
    const double* __restrict__ c, KRoute g, const double* __restrict__ goals, int32_t n_goals,
    double* __restrict__ dist, int tile, int ntx, uint32_t* __restrict__ flag0,
    int32_t* __restrict__ list0, int32_t* __restrict__ ctl) {
    const int64_t i = (int64_t)blockIdx.x * R9_THREADS + threadIdx.x;
    if (i >= n_goals) return;
    const int32_t gcell = r9j_goal_cell(g, c, goals, i);
    if (gcell < 0) return;
    dist[gcell] = 0.0;
    const int t = ((gcell / g.nx) / tile) * ntx + (gcell % g.nx) / tile;
    if (atomicExch(flag0 + t, 1u) == 0u) list0[atomicAdd(ctl, 1)] = t;
}

// ---- next hop and owner ---------------------------------------------------------------------
// r9_next's plane with no goal cell (k_route_joint_mark sets the 8s), and every cell's goal index
// set to "none yet"
__global__ __launch_bounds__(R9_THREADS) void k_route_joint_next(const double* __restrict__ c,
                                                                 const double* __restrict__ dist,
                                                                 KRoute g,
                                                                 uint8_t* __restrict__ next,
                                                                 int32_t* __restrict__ owner) {
    const int64_t n = (int64_t)g.nx * g.ny;
    for (int64_t i = (int64_t)blockIdx.x * R9_THREADS + threadIdx.x; i < n;
         i += (int64_t)gridDim.x * R9_THREADS) {
        next[i] = r9_next(g, c, dist, (int)(i % g.nx), (int)(i / g.nx), -1);
        owner[i] = R9J_NO_GOAL;
    }
}

// One lane per goal: next = 8 at the cell of a valid goal (membership in Gc, not dist == 0) and the
// lowest goal index of the cell by a 32-bit atomicMin
__global__ __launch_bounds__(R9_THREADS) void k_route_joint_mark(const double* __restrict__ c,
                                                                 KRoute g,
                                                                 const double* __restrict__ goals,
                                                                 int32_t n_goals,
                                                                 uint8_t* __restrict__ next,
                                                                 int32_t* __restrict__ owner) {
    const int64_t i = (int64_t)blockIdx.x * R9_THREADS + threadIdx.x;
    if (i >= n_goals) return;
    const int32_t gcell = r9j_goal_cell(g, c, goals, i);
    if (gcell < 0) return;
    next[gcell] = 8;
    atomicMin(owner + gcell, (int32_t)i);
}

// The parent plane of the chains: a goal cell is its own root (its goal index stays in owner), a
// cell with a direction points to that neighbour, a cell without a route to -1 (owner -1 for both)
__global__ __launch_bounds__(R9_THREADS) void k_route_joint_parent(
    KRoute g, const uint8_t* __restrict__ next, int32_t* __restrict__ parent,
    int32_t* __restrict__ owner) {
    const int64_t n = (int64_t)g.nx * g.ny;
    for (int64_t i = (int64_t)blockIdx.x * R9_THREADS + threadIdx.x; i < n;
         i += (int64_t)gridDim.x * R9_THREADS) {
        const int k = next[i];
        if (k == 8) {
            parent[i] = (int32_t)i;
            continue;
        }
        int32_t p = -1;
        if (k < 8) {
            const int ix = (int)(i % g.nx) + r9_dix(k), iy = (int)(i / g.nx) + r9_diy(k);
            if (ix >= 0 && ix < g.nx && iy >= 0 && iy < g.ny) p = iy * g.nx + ix;
        }
        parent[i] = p;
        owner[i] = -1;
    }
}

// The owner stage over a plain parent array (nothing below knows the raster: a field in the
// volume can use it as it is).  parent[v] = v at a root, an ancestor's index elsewhere, -1 for no
// chain; owner holds a root's goal index and -1 elsewhere.
//
// k_owner_jump is one round of pointer jumping, parent[v] = parent[parent[v]], in place, launched
// ceil(log2(n)) times with nothing between the launches but the stream's order.  In place, the
// read of parent[parent[v]] meets that cell's value of this round or of the one before (4-B
// relaxed atomic accesses: one of the two, never a mix).  Both are ancestors of v on its chain, the
// newer one the farther, so after round r parent[v] is the root or an ancestor at least 2^r cells
// up: a chain has fewer than n cells, so ceil(log2(n)) rounds bring every cell whose chain ends in
// a root to that root, and the root is the one the chain ends in whatever the schedule.  A cell on
// a cycle, or on a chain into one, has no root among its ancestors: it ends at some cell of the
// cycle (which may be itself: not a root, its owner is -1) and k_owner_final gives it -1.
__global__ __launch_bounds__(R9_THREADS) void k_owner_jump(int32_t* __restrict__ parent,
                                                           int64_t n) {
    for (int64_t i = (int64_t)blockIdx.x * R9_THREADS + threadIdx.x; i < n;
         i += (int64_t)gridDim.x * R9_THREADS) {
        const int32_t p = __hip_atomic_load(parent + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (p < 0 || p == i) continue;
        const int32_t pp =
            __hip_atomic_load(parent + p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (pp != p)
            __hip_atomic_store(parent + i, pp, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// owner[v] = the goal index of the root parent[v] names; -1 when it names none.  A cell that
// points to itself keeps its word (a root its goal index, a cycle's cell its -1), so no word
// read here is written here.
__global__ __launch_bounds__(R9_THREADS) void k_owner_final(const int32_t* __restrict__ parent,
                                                            int32_t* __restrict__ owner,
                                                            int64_t n) {
    for (int64_t i = (int64_t)blockIdx.x * R9_THREADS + threadIdx.x; i < n;
         i += (int64_t)gridDim.x * R9_THREADS) {
        const int32_t p = parent[i];
        if (p == i) continue;
        int32_t o = -1;
        if (p >= 0 && parent[p] == p) o = owner[p];
        owner[i] = o;
    }
}

// ---- paths ----------------------------------------------------------------------------------
// one lane per query: the goal resolved from the owner plane, then r9_trace's walks
__global__ __launch_bounds__(R9_THREADS) void k_route_joint_trace(
    KRoute g, const uint4* __restrict__ rec, const uint8_t* __restrict__ next,
    const int32_t* __restrict__ owner, const double* __restrict__ goals, int32_t n_goals,
    const double* __restrict__ starts, int64_t n_queries, int32_t N, double* __restrict__ wp,
    int32_t* __restrict__ status, int32_t* __restrict__ steps, int32_t* __restrict__ vertices,
    int32_t* __restrict__ goal_out) {
    const int64_t q = (int64_t)blockIdx.x * R9_THREADS + threadIdx.x;
    if (q < n_queries)
        r9_trace<true>(g, rec, next, goals, n_goals, starts, owner, q, N, wp, status, steps,
                       vertices, goal_out);
}

// one wave per query: the goal resolved from the owner plane, then the smoothing's one body
__global__ __launch_bounds__(R9S_WAVES * 64) void k_route_joint_smooth(
    KRoute g, const uint32_t* __restrict__ bits, const uint8_t* __restrict__ next,
    const int32_t* __restrict__ owner, const double* __restrict__ goals, int32_t n_goals,
    const double* __restrict__ starts, int64_t n_queries, int32_t N, int32_t span,
    double* __restrict__ wp, int32_t* __restrict__ status, int32_t* __restrict__ steps,
    int32_t* __restrict__ vertices, int32_t* __restrict__ goal_out) {
    __shared__ int32_t s_ring[R9S_WAVES][R9S_RING];
    __shared__ int32_t s_list[R9S_WAVES][R9S_LIST];
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int lane = threadIdx.x & 63;
    const int64_t q = (int64_t)blockIdx.x * R9S_WAVES + wave;
    if (q >= n_queries) return;  // whole waves leave; no workgroup barrier below
    r9_smooth_wave<true>(g, bits, next, goals, n_goals, starts, owner, q, N, span, wp, status,
                         steps, vertices, goal_out, s_ring[wave], s_list[wave], lane);
}

// ---- host side ------------------------------------------------------------------------------
// workspace: K9's, then the parent plane
struct R9jWs {
    R9Ws field;
    int64_t parent_off, bytes;
};
inline R9jWs r9j_workspace(int nx, int ny) {
    R9jWs w;
    w.field = r9_workspace(nx, ny);
    w.parent_off = w.field.bytes;
    w.bytes = w.parent_off + r9_al256((int64_t)nx * ny * 4);
    return w;
}

// rounds of pointer jumping: ceil(log2(n))
inline int r9j_jumps(int64_t n) {
    int r = 0;
    while (((int64_t)1 << r) < n) ++r;
    return r;
}

// The host twin: the cost plane by r9_cost, r9_dijkstra seeded with every valid goal's cell,
// r9_next with the goal cells marked afterwards, and the owner by following each chain to its end
// (a cell met again on the walk under way closes a cycle: -1 for the walk's cells).
inline void r9j_field_host(const KRoute& g, const uint4* rec, const double* goals, int32_t n_goals,
                           double* dist, uint8_t* next, int32_t* owner) {
    const int64_t n = (int64_t)g.nx * g.ny;
    std::vector<double> c((size_t)n);
    for (int64_t i = 0; i < n; ++i) {
        c[(size_t)i] = r9_cost(g, rec, (int)(i % g.nx), (int)(i / g.nx));
        dist[i] = r9_inf();
        owner[i] = R9J_NO_GOAL;
    }
    std::vector<std::pair<double, int32_t>> heap;
    for (int32_t gi = 0; gi < n_goals; ++gi) {
        const int32_t gcell = r9j_goal_cell(g, c.data(), goals, gi);
        if (gcell < 0) continue;
        if (owner[gcell] == R9J_NO_GOAL) {
            owner[gcell] = gi;  // the lowest index: the goals come in order
            dist[gcell] = 0.0;
            heap.emplace_back(0.0, gcell);
        }
    }
    r9_dijkstra(heap, dist, [&](int32_t u, auto visit) { r9_edges(g, c.data(), dist, u, visit); });
    for (int64_t i = 0; i < n; ++i)
        next[i] = owner[i] != R9J_NO_GOAL
                      ? (uint8_t)8
                      : r9_next(g, c.data(), dist, (int)(i % g.nx), (int)(i / g.nx), -1);
    // owner: 0 = not known yet, 1 = on the walk under way, 2 = known
    std::vector<uint8_t> state((size_t)n, 0);
    std::vector<int32_t> walk;
    for (int64_t i = 0; i < n; ++i) {
        if (state[(size_t)i]) continue;
        walk.clear();
        int32_t v = (int32_t)i, o = -1;
        for (;;) {
            if (state[(size_t)v] == 2) {
                o = owner[v];
                break;
            }
            if (state[(size_t)v] == 1) break;  // a cycle
            const int k = next[v];
            if (k == 8) {
                o = owner[v];
                state[(size_t)v] = 2;
                break;
            }
            state[(size_t)v] = 1;
            walk.push_back(v);
            if (k > 7) break;
            v = (v / g.nx + r9_diy(k)) * g.nx + v % g.nx + r9_dix(k);
        }
        for (int32_t w : walk) {
            owner[w] = o;
            state[(size_t)w] = 2;
        }
    }
}
