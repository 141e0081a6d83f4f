// k9v_joint.inc -- K9vj, the joint route field in the volume: one 3-D cost-to-go field to the
// nearest of many goals, the owner of every voxel and the seed paths to the owning goal
// (include/uampath.h "Route seeds in the volume, joint field").  What is the volume's own of K9j:
// k_route3_joint_clear, k_route3_joint_seed (the start state of all goals at once),
// k_route3_joint_next, k_route3_joint_mark, k_route3_joint_parent (the parent volume over the 26
// directions), k_route3_joint_trace, k_route3_joint_smooth, and the host twin of the field.  The
// relaxation is k_route3_relax<TXY, TZ> itself, the owner stage k9_joint.inc's k_owner_jump and
// k_owner_final over the plain parent array; R9J_GOALS_MAX, R9J_NO_GOAL and r9j_jumps are K9j's.
// Included in the anonymous namespace of uampath.hip, after k9v_smooth.inc and k9_joint.inc.

// the voxel of goal i when the goal is valid (in the volume and free), else -1
__host__ __device__ __forceinline__ int32_t r9vj_goal_voxel(const KRoute3& g, const double* c,
                                                            const double* goals, int64_t i) {
    const int32_t gvox = r9v_voxel(g, goals[3 * i], goals[3 * i + 1], goals[3 * i + 2]);
    return gvox >= 0 && c[gvox] < r9_inf() ? gvox : -1;
}

// ---- the field's start state ----------------------------------------------------------------
// dist = +inf everywhere, both tile-flag planes cleared, both lists empty
__global__ __launch_bounds__(R9_THREADS) void k_route3_joint_clear(KRoute3 g,
                                                                   double* __restrict__ dist,
                                                                   int ntiles,
                                                                   uint32_t* __restrict__ flags,
                                                                   int32_t* __restrict__ ctl) {
    const int64_t n = r9v_voxels(g);
    const int64_t i0 = (int64_t)blockIdx.x * R9_THREADS + threadIdx.x;
    const int64_t step = (int64_t)gridDim.x * R9_THREADS;
    for (int64_t i = i0; i < n; i += step) dist[i] = r9_inf();
    for (int64_t i = i0; i < 2 * (int64_t)ntiles; i += step) flags[i] = 0u;
    if (i0 == 0) ctl[0] = ctl[1] = 0;
}

// One lane per goal: dist = 0 at the voxel of a valid goal (goals that share a voxel store the
// same word) and the voxel's tile, (ty*ntx + tx)*ntz + tz, into list 0, once: the tile's flag of
// plane 0 is taken with atomicExch as k_route3_relax enters tiles, so the list holds distinct
// tiles (at most ntiles entries) however many goals there are and however they repeat.  The round
// that visits the tile clears the flag.
__global__ __launch_bounds__(R9_THREADS) void k_route3_joint_seed(
    const double* __restrict__ c, KRoute3 g, const double* __restrict__ goals, int32_t n_goals,
    double* __restrict__ dist, int txy, int tz, int ntx, int ntz, uint32_t* __restrict__ flag0,
    int32_t* __restrict__ list0, int32_t* __restrict__ ctl) {
    const int64_t i = (int64_t)blockIdx.x * R9_THREADS + threadIdx.x;
    if (i >= n_goals) return;
    const int32_t gvox = r9vj_goal_voxel(g, c, goals, i);
    if (gvox < 0) return;
    dist[gvox] = 0.0;
    const int c2 = gvox / g.nz;
    const int t = (((c2 / g.nx) / txy) * ntx + (c2 % g.nx) / txy) * ntz + (gvox % g.nz) / tz;
    if (atomicExch(flag0 + t, 1u) == 0u) list0[atomicAdd(ctl, 1)] = t;
}

// ---- next hop and owner ---------------------------------------------------------------------
// r9v_next's volume with no goal voxel (k_route3_joint_mark sets the 26s), and every voxel's goal
// index set to "none yet"
__global__ __launch_bounds__(R9_THREADS) void k_route3_joint_next(
    const double* __restrict__ c, const uint32_t* __restrict__ mask,
    const double* __restrict__ dist, KRoute3 g, uint8_t* __restrict__ next,
    int32_t* __restrict__ owner) {
    const int64_t n = r9v_voxels(g);
    for (int64_t i = (int64_t)blockIdx.x * R9_THREADS + threadIdx.x; i < n;
         i += (int64_t)gridDim.x * R9_THREADS) {
        next[i] = r9v_next(g, c, mask, dist, (int32_t)i, -1);
        owner[i] = R9J_NO_GOAL;
    }
}

// One lane per goal: next = 26 at the voxel of a valid goal (membership in Gc, not dist == 0) and
// the lowest goal index of the voxel by a 32-bit atomicMin
__global__ __launch_bounds__(R9_THREADS) void k_route3_joint_mark(
    const double* __restrict__ c, KRoute3 g, const double* __restrict__ goals, int32_t n_goals,
    uint8_t* __restrict__ next, int32_t* __restrict__ owner) {
    const int64_t i = (int64_t)blockIdx.x * R9_THREADS + threadIdx.x;
    if (i >= n_goals) return;
    const int32_t gvox = r9vj_goal_voxel(g, c, goals, i);
    if (gvox < 0) return;
    next[gvox] = R9V_GOAL;
    atomicMin(owner + gvox, (int32_t)i);
}

// The parent volume of the chains: a goal voxel is its own root (its goal index stays in owner),
// a voxel with a direction points to that neighbour (-1 when the direction would lead outside the
// volume, as r9_hop treats it), a voxel without a route to -1 (owner -1 for all but the roots)
__global__ __launch_bounds__(R9_THREADS) void k_route3_joint_parent(
    KRoute3 g, const uint8_t* __restrict__ next, int32_t* __restrict__ parent,
    int32_t* __restrict__ owner) {
    const int64_t n = r9v_voxels(g);
    for (int64_t i = (int64_t)blockIdx.x * R9_THREADS + threadIdx.x; i < n;
         i += (int64_t)gridDim.x * R9_THREADS) {
        const int k = next[i];
        if (k == R9V_GOAL) {
            parent[i] = (int32_t)i;
            continue;
        }
        int32_t p = -1;
        if (k < R9V_DIRS) {
            const int c2 = (int)(i / g.nz);
            const int ix = c2 % g.nx + r9v_dix(k), iy = c2 / g.nx + r9v_diy(k),
                      iz = (int)(i % g.nz) + r9v_diz(k);
            if (ix >= 0 && ix < g.nx && iy >= 0 && iy < g.ny && iz >= 0 && iz < g.nz)
                p = r9v_index(g, ix, iy, iz);
        }
        parent[i] = p;
        owner[i] = -1;
    }
}

// ---- paths ----------------------------------------------------------------------------------
// one lane per query: the goal resolved from the owner volume, then r9_trace's walks
__global__ __launch_bounds__(R9_THREADS) void k_route3_joint_trace(
    KRoute3 g, const uint2* __restrict__ vox, const uint2* __restrict__ col,
    const uint8_t* __restrict__ next, const int32_t* __restrict__ owner,
    const double* __restrict__ goals, int32_t n_goals, const double* __restrict__ starts,
    int64_t n_queries, int32_t N, double* __restrict__ wp, int32_t* __restrict__ status,
    int32_t* __restrict__ steps, int32_t* __restrict__ vertices, int32_t* __restrict__ goal_out) {
    const int64_t q = (int64_t)blockIdx.x * R9_THREADS + threadIdx.x;
    if (q < n_queries)
        r9_trace<true>(g, R9vVolume{vox, col}, next, goals, n_goals, starts, owner, q, N, wp,
                       status, steps, vertices, goal_out);
}

// one wave per query: the goal resolved from the owner volume, then the smoothing's one body
__global__ __launch_bounds__(R9S_WAVES * 64) void k_route3_joint_smooth(
    KRoute3 g, const uint32_t* __restrict__ bits, const uint8_t* __restrict__ next,
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
// workspace: K9v's, then the parent volume
struct R9vjWs {
    R9vWs field;
    int64_t parent_off, bytes;
};
inline R9vjWs r9vj_workspace(const KRoute3& g) {
    R9vjWs w;
    w.field = r9v_workspace(g);
    w.parent_off = w.field.field.bytes;
    w.bytes = w.parent_off + r9_al256(r9v_voxels(g) * 4);
    return w;
}

// The host twin: the cost volume by r9v_cost, the masks by r9v_mask, r9_dijkstra seeded with every
// valid goal's voxel, r9v_next with the goal voxels marked afterwards, and the owner by following
// each chain to its end (a voxel met again on the walk under way closes a cycle: -1 for the
// walk's voxels).
inline void r9vj_field_host(const KRoute3& g, const uint2* vox, const uint2* col,
                            const double* goals, int32_t n_goals, double* dist, uint8_t* next,
                            int32_t* owner) {
    const int64_t n = r9v_voxels(g);
    std::vector<double> c((size_t)n);
    std::vector<uint32_t> mask((size_t)n);
    for (int64_t i = 0; i < n; ++i) {
        const int64_t c2 = i / g.nz;
        c[(size_t)i] = r9v_cost(g, vox, col, (int)(c2 % g.nx), (int)(c2 / g.nx), (int)(i % g.nz));
        dist[i] = r9_inf();
        owner[i] = R9J_NO_GOAL;
    }
    for (int64_t i = 0; i < n; ++i) {
        const int64_t c2 = i / g.nz;
        mask[(size_t)i] =
            r9v_mask(g, c.data(), (int)(c2 % g.nx), (int)(c2 / g.nx), (int)(i % g.nz));
    }
    std::vector<std::pair<double, int32_t>> heap;
    for (int32_t gi = 0; gi < n_goals; ++gi) {
        const int32_t gvox = r9vj_goal_voxel(g, c.data(), goals, gi);
        if (gvox < 0) continue;
        if (owner[gvox] == R9J_NO_GOAL) {
            owner[gvox] = gi;  // the lowest index: the goals come in order
            dist[gvox] = 0.0;
            heap.emplace_back(0.0, gvox);
        }
    }
    r9_dijkstra(heap, dist, [&](int32_t u, auto visit) {
        const uint32_t m = mask[(size_t)u];
        for (int k = 0; k < R9V_DIRS; ++k) {
            if (!(m >> k & 1u)) continue;
            // the edge u -> v seen from v (r9_weight commutes)
            const int32_t v = u + (r9v_diy(k) * g.nx + r9v_dix(k)) * g.nz + r9v_diz(k);
            visit(v, dist[u] + r9_weight(c[(size_t)u], c[(size_t)v], g.len[r9v_len_index(k)]));
        }
    });
    for (int64_t i = 0; i < n; ++i)
        next[i] = owner[i] != R9J_NO_GOAL
                      ? (uint8_t)R9V_GOAL
                      : r9v_next(g, c.data(), mask.data(), dist, (int32_t)i, -1);
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
            if (k == R9V_GOAL) {
                o = owner[v];
                state[(size_t)v] = 2;
                break;
            }
            state[(size_t)v] = 1;
            walk.push_back(v);
            if (k >= R9V_DIRS) break;
            // an admissible direction of v's mask: the neighbour is inside the volume
            v += (r9v_diy(k) * g.nx + r9v_dix(k)) * g.nz + r9v_diz(k);
        }
        for (int32_t w : walk) {
            owner[w] = o;
            state[(size_t)w] = 2;
        }
    }
}
