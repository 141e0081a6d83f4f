// k9_route.inc -- K9, the route seeds: cost-to-go field of a goal on the record raster and
// the seed paths traced through it (include/uampath.h "Route seeds").  k_route_cost,
// k_route_init, k_route_relax<T>, k_route_next, k_route_trace, and the __host__ __device__
// pieces of the definition they share with uam_route_field_host / uam_route_paths_host.
// Included in the anonymous namespace of uampath.hip.

constexpr int R9_THREADS = 256;
constexpr int R9_INFLATE_MAX = 8;
constexpr int R9_SELF = 8;  // the bit after the eight directions: the tile itself

// the raster grid and the call's parameters, as the kernels and the host twins take them
struct KRoute {
    int32_t nx, ny;
    double x0, y_top, dx, dy, inv_dx, inv_dy;
    double len[3];  // step lengths: E/W, N/S, diagonal
    double lambda;
    uint32_t block_flags;
    int32_t inflate;
};

__host__ __device__ __forceinline__ double r9_inf() { return __builtin_huge_val(); }
// direction k = 0..7: E, NE, N, NW, W, SW, S, SE (row 0 is the northern edge)
__host__ __device__ __forceinline__ int r9_dix(int k) {
    return (k == 0 || k == 1 || k == 7) ? 1 : (k >= 3 && k <= 5) ? -1 : 0;
}
__host__ __device__ __forceinline__ int r9_diy(int k) {
    return (k >= 1 && k <= 3) ? -1 : (k >= 5) ? 1 : 0;
}
__host__ __device__ __forceinline__ int r9_len_index(int k) {
    return (k & 1) ? 2 : (k & 2) ? 1 : 0;
}

__host__ __device__ __forceinline__ void r9_set_lengths(KRoute* g) {
    g->len[0] = g->dx;
    g->len[1] = g->dy;
    g->len[2] = sqrt(g->dx * g->dx + g->dy * g->dy);
}

// cell of a point by the header's rule; -1 off the raster (a NaN coordinate is off it)
__host__ __device__ __forceinline__ int32_t r9_cell(const KRoute& g, double x, double y) {
    const double fx = floor((x - g.x0) * g.inv_dx);
    const double fy = floor((g.y_top - y) * g.inv_dy);
    if (!((fx >= 0.0) && (fx < (double)g.nx) && (fy >= 0.0) && (fy < (double)g.ny))) return -1;
    return (int32_t)fy * g.nx + (int32_t)fx;
}

// c_v of one record, +inf for a blocked0 cell
__host__ __device__ __forceinline__ double r9_cost0(const KRoute& g, const uint4& r) {
    const float phi = __builtin_bit_cast(float, r.x);
    const double c = 1.0 + g.lambda * (double)phi;
    const bool free0 = !(r.w & g.block_flags) && (c > 0.0) && (c < r9_inf());
    return free0 ? c : r9_inf();
}

// c_v with the inflation folded in: +inf when a blocked0 cell lies within Chebyshev distance
// inflate (cells outside the raster do not count)
__host__ __device__ __forceinline__ double r9_cost(const KRoute& g, const uint4* rec, int ix,
                                                   int iy) {
    const double own = r9_cost0(g, rec[(int64_t)iy * g.nx + ix]);
    if (!(own < r9_inf())) return own;
    const int xa = ix - g.inflate > 0 ? ix - g.inflate : 0;
    const int xb = ix + g.inflate < g.nx - 1 ? ix + g.inflate : g.nx - 1;
    const int ya = iy - g.inflate > 0 ? iy - g.inflate : 0;
    const int yb = iy + g.inflate < g.ny - 1 ? iy + g.inflate : g.ny - 1;
    for (int y = ya; y <= yb; ++y)
        for (int x = xa; x <= xb; ++x)
            if (!(r9_cost0(g, rec[(int64_t)y * g.nx + x]) < r9_inf())) return r9_inf();
    return own;
}

// edge weight (symmetric: the sum commutes)
__host__ __device__ __forceinline__ double r9_weight(double cu, double cv, double len) {
    return (0.5 * (cu + cv)) * len;
}

// fl(dist[u_k] + w(u_k, v)) for the neighbour of the free cell v = (ix, iy) in direction k on
// the cost plane c; +inf when u_k is off the raster or blocked or the corner rule forbids the
// step (a diagonal needs both orthogonally adjacent cells free)
__host__ __device__ __forceinline__ double r9_candidate(const KRoute& g, const double* c,
                                                        const double* dist, int ix, int iy,
                                                        double cv, int k) {
    const int dx = r9_dix(k), dy = r9_diy(k);
    const int ux = ix + dx, uy = iy + dy;
    if (ux < 0 || ux >= g.nx || uy < 0 || uy >= g.ny) return r9_inf();
    const double cu = c[(int64_t)uy * g.nx + ux];
    if (!(cu < r9_inf())) return r9_inf();
    if (k & 1) {
        if (!(c[(int64_t)iy * g.nx + ux] < r9_inf())) return r9_inf();
        if (!(c[(int64_t)uy * g.nx + ix] < r9_inf())) return r9_inf();
    }
    return dist[(int64_t)uy * g.nx + ux] + r9_weight(cu, cv, g.len[r9_len_index(k)]);
}

// next hop of a cell after convergence
__host__ __device__ __forceinline__ uint8_t r9_next(const KRoute& g, const double* c,
                                                    const double* dist, int ix, int iy,
                                                    int32_t gcell) {
    const int64_t v = (int64_t)iy * g.nx + ix;
    const double dv = dist[v];
    if (!(dv < r9_inf())) return 255;
    if (v == gcell) return 8;
    const double cv = c[v];
    for (int k = 0; k < 8; ++k)
        if (r9_candidate(g, c, dist, ix, iy, cv, k) == dv) return (uint8_t)k;
    return 255;  // not at a fixed point (cannot happen after convergence)
}

// ---- trace and resample -------------------------------------------------------------------
// One query: the walk along next from the start's cell to the goal's, twice (the first walk
// for S_m, the second emits the waypoints; S_i is recomputed identically).
struct R9Walk {
    int32_t cell, gcell, count;
    double vx, vy;  // V_{i-1}
    double s;       // S_{i-1}
};

// the next interior vertex of the walk; 0 = the goal cell was reached (no vertex), 1 = a
// vertex, -1 = the walk left the field (more than nx*ny cells, or a next value that is no
// direction or leads off the raster: not a field of uam_route_field)
__host__ __device__ __forceinline__ int r9_step(const KRoute& g, const uint8_t* next, R9Walk& w,
                                                double* x, double* y) {
    if (w.cell == w.gcell) return 0;
    if (w.count >= (int64_t)g.nx * g.ny) return -1;
    const int k = next[w.cell];
    if (k > 7) return -1;
    const int ix = w.cell % g.nx + r9_dix(k), iy = w.cell / g.nx + r9_diy(k);
    if (ix < 0 || ix >= g.nx || iy < 0 || iy >= g.ny) return -1;
    w.cell = iy * g.nx + ix;
    ++w.count;
    if (w.cell == w.gcell) return 0;
    *x = g.x0 + ((double)ix + 0.5) * g.dx;
    *y = g.y_top - ((double)iy + 0.5) * g.dy;
    return 1;
}

__host__ __device__ __forceinline__ double r9_seg(double ax, double ay, double bx, double by) {
    const double ex = bx - ax, ey = by - ay;
    return sqrt(ex * ex + ey * ey);
}

// J (a joint field, k9_joint.inc): next is the one joint plane, goal_idx the owner plane
// [ny][nx]; the goal is owner[cell(start)], the status tests are 1, 2, 3 (no owner) and every
// nonzero status leaves the start point in all waypoints.  vertices and goal_out are written
// for J alone.
template <bool J = false>
__host__ __device__ inline void r9_trace(const KRoute& g, const uint4* rec, const uint8_t* next,
                                         const double* goals, int32_t n_goals,
                                         const double* starts, const int32_t* goal_idx,
                                         int64_t q, int32_t N, double* wp, int32_t* status,
                                         int32_t* steps, int32_t* vertices = nullptr,
                                         int32_t* goal_out = nullptr) {
    const double sx = starts[2 * q], sy = starts[2 * q + 1];
    int32_t gi = J ? -1 : goal_idx[q];
    double* out = wp + q * (int64_t)(N + 2) * 2;
    const double dn1 = (double)(N + 1);
    double gx = sx, gy = sy;  // a goal index out of range: every waypoint is the start point
    int st = 0;
    int32_t gcell = -1, scell = -1;
    const uint8_t* nf = next;
    if (J) {
        scell = r9_cell(g, sx, sy);
        if (scell < 0 || !(r9_cost(g, rec, scell % g.nx, scell / g.nx) < r9_inf())) {
            st = 1;
        } else if (nf[scell] == 255) {
            st = 2;
        } else {
            gi = goal_idx[scell];
            // an owner that is no goal of this call is no field of uam_route_field_joint
            gcell = gi < 0 || gi >= n_goals
                        ? -1
                        : r9_cell(g, goals[2 * (int64_t)gi], goals[2 * (int64_t)gi + 1]);
            if (gcell < 0)
                st = 3;
            else
                gx = goals[2 * (int64_t)gi], gy = goals[2 * (int64_t)gi + 1];
        }
    } else {
        if (gi < 0 || gi >= n_goals) {
            st = 4;
        } else {
            gx = goals[2 * (int64_t)gi], gy = goals[2 * (int64_t)gi + 1];
            nf = next + (int64_t)gi * g.nx * g.ny;
            gcell = r9_cell(g, gx, gy);
            if (gcell < 0 || nf[gcell] != 8) st = 4;
        }
        if (!st) {
            scell = r9_cell(g, sx, sy);
            if (scell < 0 || !(r9_cost(g, rec, scell % g.nx, scell / g.nx) < r9_inf())) st = 1;
        }
        if (!st && nf[scell] == 255) st = 2;
    }
    double sm = 0.0;
    int32_t count = 0;
    if (!st) {  // first walk: S_m
        R9Walk w{scell, gcell, 1, sx, sy, 0.0};
        double x, y;
        int r;
        while ((r = r9_step(g, nf, w, &x, &y)) == 1) {
            w.s = w.s + r9_seg(w.vx, w.vy, x, y);
            w.vx = x, w.vy = y;
        }
        if (r < 0) st = 3;
        sm = w.s + r9_seg(w.vx, w.vy, gx, gy);
        count = w.count;
    }
    if (J) {
        if (st) gx = sx, gy = sy, gi = -1;
        if (vertices) vertices[q] = st ? 0 : count > 2 ? count : 2;
        if (goal_out) goal_out[q] = gi;
    }
    out[0] = sx, out[1] = sy;
    out[2 * (N + 1)] = gx, out[2 * (N + 1) + 1] = gy;
    status[q] = st;
    if (steps) steps[q] = st ? 0 : count;
    if (st) {
        for (int j = 1; j <= N; ++j) {
            const double f = (double)j / dn1;
            out[2 * j] = sx + (gx - sx) * f;
            out[2 * j + 1] = sy + (gy - sy) * f;
        }
        return;
    }
    // second walk: waypoint j lies on the first segment i (not before the previous
    // waypoint's) with S_i > t_j, on the last one when there is none
    R9Walk w{scell, gcell, 1, sx, sy, 0.0};
    int j = 1;
    for (;;) {
        double x = gx, y = gy;
        const int r = r9_step(g, nf, w, &x, &y);
        const bool last = r != 1;
        const double si = w.s + r9_seg(w.vx, w.vy, x, y);
        while (j <= N) {
            const double t = sm * ((double)j / dn1);
            if (!last && !(si > t)) break;
            const double den = si - w.s;
            const double u = den > 0.0 ? (t - w.s) / den : 0.0;
            out[2 * j] = w.vx + u * (x - w.vx);
            out[2 * j + 1] = w.vy + u * (y - w.vy);
            ++j;
        }
        if (last) break;
        w.s = si;
        w.vx = x, w.vy = y;
    }
}

// ---- kernels --------------------------------------------------------------------------------
// the cost plane of a call, shared by all its goals: c [ny][nx] f64, +inf = blocked
__global__ __launch_bounds__(R9_THREADS) void k_route_cost(const uint4* __restrict__ rec,
                                                           KRoute g, double* __restrict__ c) {
    const int64_t n = (int64_t)g.nx * g.ny;
    for (int64_t i = (int64_t)blockIdx.x * R9_THREADS + threadIdx.x; i < n;
         i += (int64_t)gridDim.x * R9_THREADS)
        c[i] = r9_cost(g, rec, (int)(i % g.nx), (int)(i / g.nx));
}

// One goal's start state: dist = +inf but 0 at the free goal cell, both tile-flag planes
// cleared, and the first active list: the goal's tile, or nothing when the goal is off the
// raster or blocked.  ctl = {count of list 0, count of list 1}.
__global__ __launch_bounds__(R9_THREADS) void k_route_init(const double* __restrict__ c, KRoute g,
                                                           const double* __restrict__ goal,
                                                           double* __restrict__ dist, int tile,
                                                           int ntx, int ntiles,
                                                           uint32_t* __restrict__ flags,
                                                           int32_t* __restrict__ lists,
                                                           int32_t* __restrict__ ctl) {
    const int64_t n = (int64_t)g.nx * g.ny;
    int32_t gcell = r9_cell(g, goal[0], goal[1]);
    if (gcell >= 0 && !(c[gcell] < r9_inf())) gcell = -1;
    const int64_t i0 = (int64_t)blockIdx.x * R9_THREADS + threadIdx.x;
    const int64_t step = (int64_t)gridDim.x * R9_THREADS;
    for (int64_t i = i0; i < n; i += step) dist[i] = i == gcell ? 0.0 : r9_inf();
    for (int64_t i = i0; i < 2 * (int64_t)ntiles; i += step) flags[i] = 0u;
    if (i0 == 0) {
        ctl[0] = gcell >= 0 ? 1 : 0;
        ctl[1] = 0;
        if (gcell >= 0) lists[0] = ((gcell / g.nx) / tile) * ntx + (gcell % g.nx) / tile;
    }
}

// A round of the label-correcting relaxation: workgroup b takes tile list_cur[b], loads its dist
// and c with a one-cell halo into LDS and runs up to `inner` pull sweeps (every free cell takes
// the min over its admissible neighbours of dist[u] + w; a sweep reads, a barrier, then writes,
// so its result does not depend on the lanes' order), stopping when a sweep changes nothing.
// It writes the changed cells back and enters into the next round's list (once: flag_nxt) itself
// when its last sweep still changed something, and each neighbour tile toward which a cell of
// its own border ring decreased.  dist only ever decreases and only this workgroup writes the
// tile's cells; a halo value read while the neighbour's workgroup lowers it is the old or the
// new one (8-B relaxed atomic accesses), and that neighbour enters this tile into the next
// round, so no decrease is lost.  No waiting on another workgroup anywhere.
// ctl[cur] (this round's count, already read by the host) is reset for the round after next.
template <int T>
__global__ __launch_bounds__(R9_THREADS) void k_route_relax(
    const double* __restrict__ c, double* __restrict__ dist, KRoute g, int ntx, int nty,
    const int32_t* __restrict__ list_cur, uint32_t* __restrict__ flag_cur,
    uint32_t* __restrict__ flag_nxt, int32_t* __restrict__ list_nxt, int32_t* __restrict__ ctl,
    int cur, int inner) {
    extern __shared__ double r9_lds[];
    constexpr int S = T + 2;
    constexpr int CPT = T * T / R9_THREADS;  // cells per lane
    double* sd = r9_lds;
    double* sc = r9_lds + S * S;
    __shared__ uint32_t s_mask;
    const int tid = threadIdx.x;
    const int tile = list_cur[blockIdx.x];
    const int tx = tile % ntx, ty = tile / ntx;
    const int bx = tx * T, by = ty * T;
    if (tid == 0) {
        flag_cur[tile] = 0u;
        s_mask = 0u;
        if (blockIdx.x == 0) ctl[cur] = 0;
    }
    for (int e = tid; e < S * S; e += R9_THREADS) {
        const int gx = bx + e % S - 1, gy = by + e / S - 1;
        double d = r9_inf(), cc = r9_inf();
        if (gx >= 0 && gx < g.nx && gy >= 0 && gy < g.ny) {
            const int64_t i = (int64_t)gy * g.nx + gx;
            cc = c[i];
            d = __hip_atomic_load(dist + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        sd[e] = d;
        sc[e] = cc;
    }
    __syncthreads();
    const double l0 = g.len[0], l1 = g.len[1], l2 = g.len[2];
    uint32_t dirty = 0u;
    int open = 0;  // the last sweep run changed something
    for (int it = 0; it < inner; ++it) {
        double nv[CPT];
        uint32_t ch = 0u;
#pragma unroll
        for (int q = 0; q < CPT; ++q) {
            const int e = tid + q * R9_THREADS;
            const int idx = (e / T + 1) * S + e % T + 1;
            const double cv = sc[idx], dv = sd[idx];
            double best = dv;
            if (cv < r9_inf()) {
                const double ce = sc[idx + 1], cw = sc[idx - 1], cn = sc[idx - S],
                             cs = sc[idx + S];
                double t;
                t = sd[idx + 1] + r9_weight(ce, cv, l0);
                best = t < best ? t : best;
                t = sd[idx - 1] + r9_weight(cw, cv, l0);
                best = t < best ? t : best;
                t = sd[idx - S] + r9_weight(cn, cv, l1);
                best = t < best ? t : best;
                t = sd[idx + S] + r9_weight(cs, cv, l1);
                best = t < best ? t : best;
                const bool fe = ce < r9_inf(), fw = cw < r9_inf(), fn = cn < r9_inf(),
                           fs = cs < r9_inf();
                if (fe && fn) {
                    t = sd[idx - S + 1] + r9_weight(sc[idx - S + 1], cv, l2);
                    best = t < best ? t : best;
                }
                if (fw && fn) {
                    t = sd[idx - S - 1] + r9_weight(sc[idx - S - 1], cv, l2);
                    best = t < best ? t : best;
                }
                if (fw && fs) {
                    t = sd[idx + S - 1] + r9_weight(sc[idx + S - 1], cv, l2);
                    best = t < best ? t : best;
                }
                if (fe && fs) {
                    t = sd[idx + S + 1] + r9_weight(sc[idx + S + 1], cv, l2);
                    best = t < best ? t : best;
                }
            }
            nv[q] = best;
            if (best < dv) ch |= 1u << q;
        }
        open = __syncthreads_or((int)ch);  // also: every read of the sweep before its writes
        if (!open) break;
#pragma unroll
        for (int q = 0; q < CPT; ++q)
            if (ch >> q & 1u) {
                const int e = tid + q * R9_THREADS;
                sd[(e / T + 1) * S + e % T + 1] = nv[q];
            }
        dirty |= ch;
        __syncthreads();
    }
    uint32_t bm = 0u;
#pragma unroll
    for (int q = 0; q < CPT; ++q)
        if (dirty >> q & 1u) {
            // a changed cell is free, hence inside the raster
            const int e = tid + q * R9_THREADS;
            const int lx = e % T, ly = e / T;
            __hip_atomic_store(dist + (int64_t)(by + ly) * g.nx + bx + lx,
                               sd[(ly + 1) * S + lx + 1], __ATOMIC_RELAXED,
                               __HIP_MEMORY_SCOPE_AGENT);
            const bool we = lx == 0, ea = lx == T - 1, no = ly == 0, so = ly == T - 1;
            bm |= (ea ? 1u : 0u) | (ea && no ? 2u : 0u) | (no ? 4u : 0u) | (we && no ? 8u : 0u) |
                  (we ? 16u : 0u) | (we && so ? 32u : 0u) | (so ? 64u : 0u) |
                  (ea && so ? 128u : 0u);
        }
    if (bm) atomicOr(&s_mask, bm);
    __syncthreads();
    if (tid <= R9_SELF) {
        int t = -1;
        if (tid == R9_SELF) {
            if (open) t = tile;
        } else if (s_mask >> tid & 1u) {
            const int ux = tx + r9_dix(tid), uy = ty + r9_diy(tid);
            if (ux >= 0 && ux < ntx && uy >= 0 && uy < nty) t = uy * ntx + ux;
        }
        if (t >= 0 && atomicExch(flag_nxt + t, 1u) == 0u)
            list_nxt[atomicAdd(ctl + (cur ^ 1), 1)] = t;
    }
}

// the next hops of one goal's converged field
__global__ __launch_bounds__(R9_THREADS) void k_route_next(const double* __restrict__ c,
                                                           const double* __restrict__ dist,
                                                           KRoute g,
                                                           const double* __restrict__ goal,
                                                           uint8_t* __restrict__ next) {
    const int64_t n = (int64_t)g.nx * g.ny;
    const int32_t gcell = r9_cell(g, goal[0], goal[1]);
    for (int64_t i = (int64_t)blockIdx.x * R9_THREADS + threadIdx.x; i < n;
         i += (int64_t)gridDim.x * R9_THREADS)
        next[i] = r9_next(g, c, dist, (int)(i % g.nx), (int)(i / g.nx), gcell);
}

// the seed paths: one lane per query, sequential
__global__ __launch_bounds__(R9_THREADS) void k_route_trace(
    KRoute g, const uint4* __restrict__ rec, const uint8_t* __restrict__ next,
    const double* __restrict__ goals, int32_t n_goals, const double* __restrict__ starts,
    const int32_t* __restrict__ goal_idx, int64_t n_queries, int32_t N, double* __restrict__ wp,
    int32_t* __restrict__ status, int32_t* __restrict__ steps) {
    const int64_t q = (int64_t)blockIdx.x * R9_THREADS + threadIdx.x;
    if (q < n_queries)
        r9_trace(g, rec, next, goals, n_goals, starts, goal_idx, q, N, wp, status, steps);
}

// ---- host side ------------------------------------------------------------------------------
constexpr int R9_TILE_MIN = 16;
inline int r9_tiles(int n, int tile) { return (n + tile - 1) / tile; }
inline int64_t r9_al256(int64_t v) { return (v + 255) & ~(int64_t)255; }
// workspace: the cost plane, then the two flag planes, the two lists (sized for the smallest
// tile) and the two counts
struct R9Ws {
    int64_t c_off, flags_off, lists_off, ctl_off, bytes;
};
inline R9Ws r9_workspace(int nx, int ny) {
    const int64_t nt = (int64_t)r9_tiles(nx, R9_TILE_MIN) * r9_tiles(ny, R9_TILE_MIN);
    R9Ws w;
    w.c_off = 0;
    w.flags_off = r9_al256((int64_t)nx * ny * 8);
    w.lists_off = w.flags_off + r9_al256(2 * nt * 4);
    w.ctl_off = w.lists_off + r9_al256(2 * nt * 4);
    w.bytes = w.ctl_off + 256;
    return w;
}

// one round: n workgroups over list `cur`, entering tiles into list cur ^ 1
template <int T>
void route_relax_launch(int n, hipStream_t s, const double* c, double* dist,
                               const KRoute& g, int ntx, int nty, uint32_t* flags,
                               int32_t* lists, int32_t* ctl, int cur, int inner) {
    const int nt = ntx * nty;
    const size_t lds = (size_t)2 * (T + 2) * (T + 2) * sizeof(double);
    hipLaunchKernelGGL(k_route_relax<T>, dim3(n), dim3(R9_THREADS), lds, s, c, dist, g, ntx, nty,
                       lists + cur * nt, flags + cur * nt, flags + (cur ^ 1) * nt,
                       lists + (cur ^ 1) * nt, ctl, cur, inner);
}

// the host twin of the field: the cost plane by r9_cost, a heap Dijkstra over r9_weight's
// edges (the same minimum as any relaxation order: fl(a + w) is monotone in a), r9_next
inline void r9_field_host(const KRoute& g, const uint4* rec, const double* goals, int32_t n_goals,
                          double* dist, uint8_t* next) {
    const int64_t n = (int64_t)g.nx * g.ny;
    std::vector<double> c((size_t)n);
    for (int64_t i = 0; i < n; ++i)
        c[(size_t)i] = r9_cost(g, rec, (int)(i % g.nx), (int)(i / g.nx));
    std::vector<std::pair<double, int32_t>> heap;
    auto later = [](const std::pair<double, int32_t>& a, const std::pair<double, int32_t>& b) {
        return a.first > b.first;
    };
    for (int32_t gi = 0; gi < n_goals; ++gi) {
        double* d = dist + (int64_t)gi * n;
        uint8_t* nx = next + (int64_t)gi * n;
        for (int64_t i = 0; i < n; ++i) d[i] = r9_inf();
        int32_t gcell = r9_cell(g, goals[2 * gi], goals[2 * gi + 1]);
        if (gcell >= 0 && c[(size_t)gcell] < r9_inf()) {
            d[gcell] = 0.0;
            heap.clear();
            heap.emplace_back(0.0, gcell);
            while (!heap.empty()) {
                std::pop_heap(heap.begin(), heap.end(), later);
                const auto top = heap.back();
                heap.pop_back();
                const int32_t u = top.second;
                if (top.first > d[u]) continue;
                const int ux = u % g.nx, uy = u / g.nx;
                for (int k = 0; k < 8; ++k) {
                    // the edge u -> v seen from v: v's neighbour in the opposite direction
                    const int vx = ux + r9_dix(k), vy = uy + r9_diy(k);
                    if (vx < 0 || vx >= g.nx || vy < 0 || vy >= g.ny) continue;
                    const int64_t v = (int64_t)vy * g.nx + vx;
                    if (!(c[(size_t)v] < r9_inf())) continue;
                    const double t =
                        r9_candidate(g, c.data(), d, vx, vy, c[(size_t)v], (k + 4) & 7);
                    if (t < d[v]) {
                        d[v] = t;
                        heap.emplace_back(t, (int32_t)v);
                        std::push_heap(heap.begin(), heap.end(), later);
                    }
                }
            }
        }
        for (int64_t i = 0; i < n; ++i)
            nx[i] = r9_next(g, c.data(), d, (int)(i % g.nx), (int)(i / g.nx), gcell);
    }
}
