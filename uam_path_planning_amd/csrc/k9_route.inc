// k9_route.inc -- K9, the route seeds: cost-to-go field of a goal on the record raster and
// the seed paths traced through it (include/uampath.h "Route seeds").  k_route_cost,
// k_route_init, k_route_relax<T>, k_route_next, k_route_trace, and the __host__ __device__
// pieces of the definition they share with uam_route_field_host / uam_route_paths_host.
// Also what the whole K9 family shares, written over the grid type G (KRoute here, KRoute3 in
// k9v_route.inc) and reaching the grid only through the overloads of "the grid vocabulary":
// the query's status tests, the resampling and the trace (r9_query, r9_vertex, r9_walk,
// r9_trace) and the host twins' Dijkstra (r9_dijkstra).  The float64 operations are the same
// for both grids but r9_seg's, in the same order.
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
    static constexpr int D = 2;     // coordinates of a point
    static constexpr int GOAL = 8;  // next at the goal's cell
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

// ---- the grid vocabulary ---------------------------------------------------------------------
// What the trace, the smoothing and the host Dijkstra need from a grid, as overloads on KRoute
// (here and in k9_smooth.inc) and on KRoute3 (k9v_route.inc, k9v_smooth.inc); a cell is the
// int32 index of a cell or voxel, a point G::D doubles.  G::GOAL is next at the goal's cell.
__host__ __device__ __forceinline__ int64_t r9_count(const KRoute& g) {
    return (int64_t)g.nx * g.ny;
}
__host__ __device__ __forceinline__ int32_t r9_locate(const KRoute& g, const double* p) {
    return r9_cell(g, p[0], p[1]);
}
// one step of the chain from cell in direction k (count cells visited so far): 1 = moved, -1 =
// the walk left the field (more than nx*ny cells, or a next value that is no direction or leads
// off the raster: not a field of uam_route_field)
__host__ __device__ __forceinline__ int r9_hop(const KRoute& g, int k, int32_t* cell,
                                               int64_t count) {
    if (count >= r9_count(g)) return -1;
    if (k > 7) return -1;
    const int ix = *cell % g.nx + r9_dix(k), iy = *cell / g.nx + r9_diy(k);
    if (ix < 0 || ix >= g.nx || iy < 0 || iy >= g.ny) return -1;
    *cell = iy * g.nx + ix;
    return 1;
}
__host__ __device__ __forceinline__ void r9_centre(const KRoute& g, int32_t cell, double* p) {
    p[0] = g.x0 + ((double)(cell % g.nx) + 0.5) * g.dx;
    p[1] = g.y_top - ((double)(cell / g.nx) + 0.5) * g.dy;
}
__host__ __device__ __forceinline__ double r9_seg(const KRoute&, const double* a,
                                                  const double* b) {
    const double ex = b[0] - a[0], ey = b[1] - a[1];
    return sqrt(ex * ex + ey * ey);
}
// the start's blocking as the trace reads it: from the records (the smoothing reads the bits)
__host__ __device__ __forceinline__ bool r9_start_blocked(const KRoute& g, const uint4* rec,
                                                          int32_t cell) {
    return !(r9_cost(g, rec, cell % g.nx, cell / g.nx) < r9_inf());
}

// ---- trace and resample, on either grid ---------------------------------------------------
// a query's end points, cells, field and status 4 / 1 / 2 (J: 1 / 2 / 3)
template <typename G>
struct R9Query {
    double s[G::D], t[G::D];  // the start point; the goal point (the start's until one is known)
    int32_t scell, gcell;
    const uint8_t* nf;
    int st;
    int32_t gi;  // the goal index (J: the start cell's owner, -1 for a nonzero status)
};

// src says whether the start's cell is blocked (r9_start_blocked): the records or the volume
// for the trace, the free bits for the smoothing.
// J (a joint field, k9_joint.inc): next is the one joint plane, goal_idx the owner plane; the
// goal is owner[cell(start)], the status tests are 1, 2, 3 (no owner: an owner that is no goal
// of this call is no field of uam_route_field_joint).
template <bool J = false, typename G, typename Src>
__host__ __device__ inline R9Query<G> r9_query(const G& g, Src src, const uint8_t* next,
                                               const double* goals, int32_t n_goals,
                                               const double* starts, const int32_t* goal_idx,
                                               int64_t q) {
    constexpr int D = G::D;
    R9Query<G> u;
    // a goal index out of range: every waypoint is the start point
    for (int i = 0; i < D; ++i) u.s[i] = u.t[i] = starts[D * q + i];
    u.scell = u.gcell = -1;
    u.nf = next;
    u.st = 0;
    if (J) {
        u.gi = -1;
        u.scell = r9_locate(g, u.s);
        if (u.scell < 0 || r9_start_blocked(g, src, u.scell)) {
            u.st = 1;
        } else if (u.nf[u.scell] == 255) {
            u.st = 2;
        } else {
            const int32_t o = goal_idx[u.scell];
            if (o >= 0 && o < n_goals) u.gcell = r9_locate(g, goals + D * (int64_t)o);
            if (u.gcell < 0) {
                u.st = 3;
            } else {
                u.gi = o;
                for (int i = 0; i < D; ++i) u.t[i] = goals[D * (int64_t)o + i];
            }
        }
        return u;
    }
    const int32_t gi = goal_idx[q];
    u.gi = gi;
    if (gi < 0 || gi >= n_goals) {
        u.st = 4;
    } else {
        for (int i = 0; i < D; ++i) u.t[i] = goals[D * (int64_t)gi + i];
        u.nf = next + (int64_t)gi * r9_count(g);
        u.gcell = r9_locate(g, u.t);
        if (u.gcell < 0 || u.nf[u.gcell] != G::GOAL) u.st = 4;
    }
    if (!u.st) {
        u.scell = r9_locate(g, u.s);
        if (u.scell < 0 || r9_start_blocked(g, src, u.scell)) u.st = 1;
    }
    if (!u.st && u.nf[u.scell] == 255) u.st = 2;
    return u;
}

// A query's fixed outputs once its walk is done: J with a nonzero status leaves the start point
// as the goal and no goal index; then (write: the lane that stores them) the two end points,
// the status, steps = n and vertices = nv (0 for a nonzero status), the goal index.
template <bool J, typename G>
__host__ __device__ inline void r9_ends(R9Query<G>& u, int64_t q, int32_t N, double* out,
                                        int32_t* status, int32_t* steps, int32_t n,
                                        int32_t* vertices, int32_t nv, int32_t* goal_out,
                                        bool write) {
    constexpr int D = G::D;
    if (J && u.st) {
        for (int i = 0; i < D; ++i) u.t[i] = u.s[i];
        u.gi = -1;
    }
    if (!write) return;
    for (int i = 0; i < D; ++i) out[i] = u.s[i], out[D * (N + 1) + i] = u.t[i];
    status[q] = u.st;
    if (steps) steps[q] = u.st ? 0 : n;
    if (vertices) vertices[q] = u.st ? 0 : nv;
    if (goal_out) goal_out[q] = u.gi;
}

// the straight line of a nonzero status: waypoints j0, j0 + stride, ..
template <typename G>
__host__ __device__ inline void r9_straight(const R9Query<G>& u, int32_t N, double* out, int j0,
                                            int stride) {
    constexpr int D = G::D;
    const double dn1 = (double)(N + 1);
    for (int j = j0; j <= N; j += stride) {
        const double f = (double)j / dn1;
        for (int i = 0; i < D; ++i) out[D * j + i] = u.s[i] + (u.t[i] - u.s[i]) * f;
    }
}

// The vertices V_1, V_2, .. of a path taken one after the other: pass 1 (out NULL) sums S_m,
// pass 2 (sm known) places the waypoints: waypoint j lies on the first segment i (not before
// the previous waypoint's) with S_i > t_j, on the last one when there is none.
template <int D>
struct R9Path {
    double v[D];  // V_{i-1}
    double s;     // S_{i-1}
    double sm, dn1;
    int32_t j, N;
    double* out;  // NULL: pass 1
    bool write;   // this lane stores the waypoints
};

template <int D>
__host__ __device__ __forceinline__ R9Path<D> r9_path(const double* start, double sm, int32_t N,
                                                      double* out, bool write) {
    R9Path<D> p;
    for (int i = 0; i < D; ++i) p.v[i] = start[i];
    p.s = 0.0, p.sm = sm, p.dn1 = (double)(N + 1);
    p.j = 1, p.N = N;
    p.out = out, p.write = write;
    return p;
}

template <typename G>
__host__ __device__ inline void r9_vertex(const G& g, R9Path<G::D>& p, const double* x,
                                          bool last) {
    constexpr int D = G::D;
    const double si = p.s + r9_seg(g, p.v, x);
    if (p.out) {
        while (p.j <= p.N) {
            const double t = p.sm * ((double)p.j / p.dn1);
            if (!last && !(si > t)) break;
            const double den = si - p.s;
            const double u = den > 0.0 ? (t - p.s) / den : 0.0;
            double w[D];
            for (int i = 0; i < D; ++i) w[i] = p.v[i] + u * (x[i] - p.v[i]);
            if (p.write)
                for (int i = 0; i < D; ++i) p.out[D * p.j + i] = w[i];
            ++p.j;
        }
    }
    p.s = si;
    for (int i = 0; i < D; ++i) p.v[i] = x[i];
}

// the walk along nf from scell to gcell, the centre of every cell between them a vertex of p;
// the number of cells visited, -1 when the walk left the field
template <typename G>
__host__ __device__ inline int64_t r9_walk(const G& g, const uint8_t* nf, int32_t scell,
                                           int32_t gcell, R9Path<G::D>& p) {
    int32_t cell = scell;
    int64_t count = 1;
    while (cell != gcell) {
        // the centre and the hop of one cell in one iteration: its index is taken apart once
        if (count > 1) {
            double x[G::D];
            r9_centre(g, cell, x);
            r9_vertex(g, p, x, false);
        }
        if (r9_hop(g, nf[cell], &cell, count) < 0) return -1;
        ++count;
    }
    return count;
}

// One query: the walk from the start's cell to the goal's, twice (the first for S_m, the second
// emits the waypoints; S_i is recomputed identically).  vertices and goal_out are written for J
// alone.
template <bool J = false, typename G, typename Src>
__host__ __device__ inline void r9_trace(const G& g, Src src, const uint8_t* next,
                                         const double* goals, int32_t n_goals,
                                         const double* starts, const int32_t* goal_idx,
                                         int64_t q, int32_t N, double* wp, int32_t* status,
                                         int32_t* steps, int32_t* vertices = nullptr,
                                         int32_t* goal_out = nullptr) {
    constexpr int D = G::D;
    R9Query<G> u = r9_query<J>(g, src, next, goals, n_goals, starts, goal_idx, q);
    double* out = wp + q * (int64_t)(N + 2) * D;
    R9Path<D> p = r9_path<D>(u.s, 0.0, N, nullptr, true);
    int64_t count = 0;
    if (!u.st && (count = r9_walk(g, u.nf, u.scell, u.gcell, p)) < 0) u.st = 3;
    r9_ends<J>(u, q, N, out, status, steps, (int32_t)count, vertices,
               (int32_t)(count > 2 ? count : 2), goal_out, true);
    if (u.st) {
        r9_straight(u, N, out, 1, 1);
        return;
    }
    r9_vertex(g, p, u.t, true);  // S_m
    p = r9_path<D>(u.s, p.s, N, out, true);
    (void)r9_walk(g, u.nf, u.scell, u.gcell, p);
    r9_vertex(g, p, u.t, true);
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

// The heap Dijkstra of the host twins, on either grid: from the seeds in heap, each (0.0, cell)
// with d = 0 there already (all keys equal: a heap as it stands), over the edges that
// edges(u, visit) names by calling visit(v, fl(d[u] + w(u, v))) for the neighbours v of u.  The
// same minimum as any relaxation order: fl(a + w) is monotone in a.
template <typename Edges>
inline void r9_dijkstra(std::vector<std::pair<double, int32_t>>& heap, double* d, Edges edges) {
    auto later = [](const std::pair<double, int32_t>& a, const std::pair<double, int32_t>& b) {
        return a.first > b.first;
    };
    while (!heap.empty()) {
        std::pop_heap(heap.begin(), heap.end(), later);
        const auto top = heap.back();
        heap.pop_back();
        const int32_t u = top.second;
        if (top.first > d[u]) continue;
        edges(u, [&](int32_t v, double t) {
            if (t < d[v]) {
                d[v] = t;
                heap.emplace_back(t, v);
                std::push_heap(heap.begin(), heap.end(), later);
            }
        });
    }
}

// the raster's edges out of u: the edge u -> v seen from v, v's neighbour in the opposite
// direction, by r9_candidate
template <typename Visit>
inline void r9_edges(const KRoute& g, const double* c, const double* d, int32_t u, Visit visit) {
    const int ux = u % g.nx, uy = u / g.nx;
    for (int k = 0; k < 8; ++k) {
        const int vx = ux + r9_dix(k), vy = uy + r9_diy(k);
        if (vx < 0 || vx >= g.nx || vy < 0 || vy >= g.ny) continue;
        const int64_t v = (int64_t)vy * g.nx + vx;
        if (!(c[v] < r9_inf())) continue;
        visit((int32_t)v, r9_candidate(g, c, d, vx, vy, c[v], (k + 4) & 7));
    }
}

// the host twin of the field: the cost plane by r9_cost, r9_dijkstra over r9_weight's edges,
// r9_next
inline void r9_field_host(const KRoute& g, const uint4* rec, const double* goals, int32_t n_goals,
                          double* dist, uint8_t* next) {
    const int64_t n = r9_count(g);
    std::vector<double> c((size_t)n);
    for (int64_t i = 0; i < n; ++i)
        c[(size_t)i] = r9_cost(g, rec, (int)(i % g.nx), (int)(i / g.nx));
    std::vector<std::pair<double, int32_t>> heap;
    for (int32_t gi = 0; gi < n_goals; ++gi) {
        double* d = dist + (int64_t)gi * n;
        uint8_t* nx = next + (int64_t)gi * n;
        for (int64_t i = 0; i < n; ++i) d[i] = r9_inf();
        const int32_t gcell = r9_cell(g, goals[2 * gi], goals[2 * gi + 1]);
        if (gcell >= 0 && c[(size_t)gcell] < r9_inf()) {
            d[gcell] = 0.0;
            heap.assign(1, {0.0, gcell});
            r9_dijkstra(heap, d, [&](int32_t u, auto visit) { r9_edges(g, c.data(), d, u, visit); });
        }
        for (int64_t i = 0; i < n; ++i)
            nx[i] = r9_next(g, c.data(), d, (int)(i % g.nx), (int)(i / g.nx), gcell);
    }
}
