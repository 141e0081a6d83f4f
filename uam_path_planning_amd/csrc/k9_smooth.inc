// k9_smooth.inc -- K9b / K9s, any-angle shortcuts on the traced route (include/uampath.h "Route
// seeds", "smoothing"): k_route_free_bits (one bit per cell, set = free) with its host twin,
// k_route_smooth (one wave per query: the chain along next, the anchors by "advance while
// visible", the resampled waypoints), the raster's sight line r9s_los and its walk along next.
// The smoothing itself is written once over the grid type G, for this file's kernel, for
// k_route_joint_smooth (k9_joint.inc) and for k_route3_smooth (k9v_smooth.inc): r9_pass,
// r9_smooth_wave and the host twin r9_smooth_host, which reach the grid only through the
// vocabulary of k9_route.inc and the three overloads on the free bits given here and in
// k9v_smooth.inc (r9_bit_free, r9_visible, r9_advance).  Integer arithmetic decides every
// visibility; the float64 operations are r9_trace's, in its order.
// Included in the anonymous namespace of uampath.hip, after k9_route.inc.

constexpr int R9S_WAVES = 4;                  // waves (queries) per workgroup
constexpr int R9S_RING = UAM_ROUTE_SPAN_MAX;  // chain cells a wave keeps in LDS (a power of two)
constexpr int R9S_LIST = UAM_ROUTE_SMOOTH_LIST;  // anchors a wave keeps for the resampling pass
static_assert((R9S_RING & (R9S_RING - 1)) == 0, "the ring is indexed with a mask");

// words per row of the free bits
__host__ __device__ __forceinline__ int r9s_wpr(int nx) {
    return (int)(((int64_t)nx + 31) >> 5);
}

__host__ __device__ __forceinline__ bool r9s_free(const uint32_t* bits, int wpr, int64_t x,
                                                  int64_t y) {
    return (bits[y * wpr + (x >> 5)] >> (x & 31)) & 1u;
}

// LOS(A, B): every cell of T(A, B) is free.  T is walked along the segment's major axis; for
// the i-th column (row) the cells v = lo..hi of the minor axis are those with
// 2*|amaj*v - amin*i| <= amaj + amin.  Both cells are on the raster, and so is their bounding
// box.  I = int32_t serves |d| <= 1024 (2*amin*i + amaj + amin < 2^22).
template <typename I>
__host__ __device__ inline bool r9s_los(const uint32_t* bits, int wpr, I ax, I ay, I bx, I by) {
    const I dx = bx - ax, dy = by - ay;
    const I adx = dx < 0 ? -dx : dx, ady = dy < 0 ? -dy : dy;
    const bool swap = ady > adx;  // the major axis is y
    const I amaj = swap ? ady : adx, amin = swap ? adx : ady;
    if (amaj == 0) return r9s_free(bits, wpr, ax, ay);
    const I smaj = (swap ? dy : dx) > 0 ? 1 : -1, smin = (swap ? dx : dy) >= 0 ? 1 : -1;
    const I s = amaj + amin, den = 2 * amaj;
    for (I i = 0; i <= amaj; ++i) {
        const I c = 2 * amin * i;
        const I lo = c > s ? (c - s + den - 1) / den : 0;
        I hi = (c + s) / den;
        hi = hi < amin ? hi : amin;
        for (I v = lo; v <= hi; ++v) {
            const I x = swap ? ax + smin * v : ax + smaj * i;
            const I y = swap ? ay + smaj * i : ay + smin * v;
            if (!r9s_free(bits, wpr, x, y)) return false;
        }
    }
    return true;
}

// ---- the grid vocabulary on the free bits ---------------------------------------------------
__host__ __device__ __forceinline__ bool r9_bit_free(const KRoute& g, const uint32_t* bits,
                                                     int32_t cell) {
    return r9s_free(bits, r9s_wpr(g.nx), cell % g.nx, cell / g.nx);
}

// LOS between two cells of the chain
__host__ __device__ __forceinline__ bool r9_visible(const KRoute& g, const uint32_t* bits,
                                                    int32_t a, int32_t b) {
    return r9s_los<int32_t>(bits, r9s_wpr(g.nx), a % g.nx, a / g.nx, b % g.nx, b / g.nx);
}

// the start's blocking as the smoothing reads it, on either grid
template <typename G>
__host__ __device__ __forceinline__ bool r9_start_blocked(const G& g, const uint32_t* bits,
                                                          int32_t cell) {
    return !r9_bit_free(g, bits, cell);
}

// The walk along next, the same in every lane of the wave; every cell reached goes into the
// wave's ring (slot = chain index & mask).
struct R9sWalk {
    int32_t cell;  // c_idx
    int32_t idx;   // chain index of cell
    bool done;     // cell is the goal's: n = idx + 1
    bool fail;     // status 3
};

// one hop of the walk taken with direction k; false when the walk ends here
template <typename G>
__device__ __forceinline__ bool r9s_hopped(const G& g, int k, int32_t gcell, R9sWalk& w,
                                           int32_t* ring, int lane) {
    if (r9_hop(g, k, &w.cell, (int64_t)w.idx + 1) < 0) {
        w.fail = true;
        return false;
    }
    ++w.idx;
    if (lane == 0) ring[w.idx & (R9S_RING - 1)] = w.cell;
    if (w.cell == gcell) w.done = true;
    return !w.done;
}

// The raster's walk up to chain index upto: the lanes load the 8 x 8 patch of next around the
// current cell, and the chain is followed inside it with shuffles until it leaves the patch.
__device__ inline void r9_advance(const KRoute& g, const uint8_t* __restrict__ nf, int32_t gcell,
                                  R9sWalk& w, int32_t upto, int32_t* ring, int lane) {
    while (!w.done && !w.fail && w.idx < upto) {
        const int ox = w.cell % g.nx - 4, oy = w.cell / g.nx - 4;
        const int px = ox + (lane & 7), py = oy + (lane >> 3);
        int mine = 255;
        if (px >= 0 && px < g.nx && py >= 0 && py < g.ny) mine = nf[(int64_t)py * g.nx + px];
        for (;;) {
            const int lx = w.cell % g.nx - ox, ly = w.cell / g.nx - oy;
            if (lx < 0 || lx > 7 || ly < 0 || ly > 7) break;  // the next patch
            if (!r9s_hopped(g, __shfl(mine, ly * 8 + lx, 64), gcell, w, ring, lane)) break;
            if (w.idx >= upto) break;
        }
    }
    wave_sync();
}

// ---- the smoothing, on either grid ------------------------------------------------------------
// One pass over a query's chain: anchors by "advance while visible", 64 candidates at a time,
// one lane each.  Every anchor goes to path (pass 1: S_m; pass 2: the waypoints) and, while
// there is room, into list.  Returns the number of anchors, -1 for status 3; *n_out = steps.
template <typename G>
__device__ inline int32_t r9_pass(const G& g, const uint32_t* __restrict__ bits,
                                  const R9Query<G>& u, int32_t span, int32_t* ring, int32_t* list,
                                  R9Path<G::D>& path, int32_t* n_out, int lane) {
    R9sWalk w{u.scell, 0, u.scell == u.gcell, false};
    r9_advance(g, u.nf, u.gcell, w, 2, ring, lane);
    if (w.fail) return -1;
    int32_t na = 0;
    if (!(w.done && w.idx < 2)) {  // n > 2
        int32_t a = 1;
        int32_t acell = ring[1];
        for (;;) {
            double x[G::D];
            r9_centre(g, acell, x);
            r9_vertex(g, path, x, false);
            if (list && na < R9S_LIST && lane == 0) list[na] = acell;
            ++na;
            r9_advance(g, u.nf, u.gcell, w, a + span, ring, lane);
            if (w.fail) return -1;
            if (w.done && a == w.idx - 1) break;  // a = n - 2
            const int32_t top = w.done && w.idx - 1 < a + span ? w.idx - 1 : a + span;
            int32_t j = top;
            for (int32_t base = a + 1; base <= top; base += 64) {
                const int32_t i = base + lane;
                bool blocked = false;
                if (i <= top && i > a + 1)  // adjacent chain cells are visible
                    blocked = !r9_visible(g, bits, acell, ring[i & (R9S_RING - 1)]);
                const uint64_t m = __ballot(blocked);
                if (m) {
                    j = base + (__ffsll((unsigned long long)m) - 1) - 1;
                    break;
                }
            }
            a = j;
            acell = ring[a & (R9S_RING - 1)];
        }
    }
    *n_out = w.idx + 1;
    return na;
}

// One wave's query, the body of k_route_smooth, k_route3_smooth and (J, a joint field:
// r9_query<true>'s rules and goal_out) k_route_joint_smooth.  ring and list are the wave's LDS.
template <bool J, typename G>
__device__ __forceinline__ void r9_smooth_wave(
    const G& g, const uint32_t* __restrict__ bits, const uint8_t* __restrict__ next,
    const double* __restrict__ goals, int32_t n_goals, const double* __restrict__ starts,
    const int32_t* __restrict__ goal_idx, int64_t q, int32_t N, int32_t span,
    double* __restrict__ wp, int32_t* __restrict__ status, int32_t* __restrict__ steps,
    int32_t* __restrict__ vertices, int32_t* __restrict__ goal_out, int32_t* ring, int32_t* list,
    int lane) {
    constexpr int D = G::D;
    R9Query<G> u = r9_query<J>(g, bits, next, goals, n_goals, starts, goal_idx, q);
    double* out = wp + q * (int64_t)(N + 2) * D;
    int32_t n = 0, na = 0;
    R9Path<D> p = r9_path<D>(u.s, 0.0, N, nullptr, false);
    if (!u.st) {
        na = r9_pass(g, bits, u, span, ring, list, p, &n, lane);
        if (na < 0) u.st = 3;
    }
    r9_ends<J>(u, q, N, out, status, steps, n, vertices, na + 2, goal_out, lane == 0);
    if (u.st) {
        r9_straight(u, N, out, 1 + lane, 64);
        return;
    }
    r9_vertex(g, p, u.t, true);  // S_m
    R9Path<D> e = r9_path<D>(u.s, p.s, N, out, lane == 0);
    if (na <= R9S_LIST) {
        wave_sync();
        for (int32_t k = 0; k < na; ++k) {
            double x[D];
            r9_centre(g, list[k], x);
            r9_vertex(g, e, x, false);
        }
    } else {  // the list overflowed: the same anchors again, placed as they are found
        (void)r9_pass(g, bits, u, span, ring, nullptr, e, &n, lane);
    }
    r9_vertex(g, e, u.t, true);
}

// the host twin: the chain in cells, the anchors one candidate at a time, the two passes
template <bool J = false, typename G>
inline void r9_smooth_host(const G& g, const uint32_t* bits, const uint8_t* next,
                           const double* goals, int32_t n_goals, const double* starts,
                           const int32_t* goal_idx, int64_t q, int32_t N, int32_t span,
                           double* wp, int32_t* status, int32_t* steps, int32_t* vertices,
                           std::vector<int32_t>& cells, std::vector<int32_t>& anchors,
                           int32_t* goal_out = nullptr) {
    constexpr int D = G::D;
    R9Query<G> u = r9_query<J>(g, bits, next, goals, n_goals, starts, goal_idx, q);
    double* out = wp + q * (int64_t)(N + 2) * D;
    cells.clear();
    anchors.clear();
    if (!u.st) {
        int32_t cell = u.scell;
        cells.push_back(cell);
        while (cell != u.gcell) {
            if (r9_hop(g, u.nf[cell], &cell, (int64_t)cells.size()) < 0) {
                u.st = 3;
                break;
            }
            cells.push_back(cell);
        }
    }
    const int64_t n = (int64_t)cells.size();
    if (!u.st && n > 2) {
        int64_t a = 1;
        anchors.push_back(cells[1]);
        while (a != n - 2) {
            const int64_t jmax = a + span < n - 2 ? a + span : n - 2;
            // advance while visible; c_{a+1} is taken untested (adjacent chain cells are visible)
            int64_t j = a + 1;
            while (j < jmax && r9_visible(g, bits, cells[(size_t)a], cells[(size_t)j + 1])) ++j;
            a = j;
            anchors.push_back(cells[(size_t)a]);
        }
    }
    r9_ends<J>(u, q, N, out, status, steps, (int32_t)n, vertices, (int32_t)anchors.size() + 2,
               goal_out, true);
    if (u.st) {
        r9_straight(u, N, out, 1, 1);
        return;
    }
    R9Path<D> p = r9_path<D>(u.s, 0.0, N, nullptr, true);
    for (int pass = 0; pass < 2; ++pass) {
        for (int32_t c : anchors) {
            double x[D];
            r9_centre(g, c, x);
            r9_vertex(g, p, x, false);
        }
        r9_vertex(g, p, u.t, true);
        if (pass == 0) p = r9_path<D>(u.s, p.s, N, out, true);
    }
}

// ---- the free bits ----------------------------------------------------------------------------
// one wave per 64 cells of a row, one lane per cell; lanes 0 and 32 store the two words of the
// wave's ballot (bits past nx stay 0)
__global__ __launch_bounds__(R9_THREADS) void k_route_free_bits(const uint4* __restrict__ rec,
                                                                KRoute g,
                                                                uint32_t* __restrict__ bits) {
    const int lane = threadIdx.x & 63;
    const int cpr = (int)(((int64_t)g.nx + 63) >> 6);  // 64-cell chunks per row
    const int wpr = r9s_wpr(g.nx);
    const int64_t chunks = (int64_t)cpr * g.ny;
    const int64_t w0 = (int64_t)blockIdx.x * (R9_THREADS / 64) + (threadIdx.x >> 6);
    for (int64_t w = w0; w < chunks; w += (int64_t)gridDim.x * (R9_THREADS / 64)) {
        const int iy = (int)(w / cpr), ch = (int)(w % cpr);
        const int64_t ix = (int64_t)ch * 64 + lane;
        const bool fr = ix < g.nx && r9_cost(g, rec, (int)ix, iy) < r9_inf();
        const uint64_t m = __ballot(fr);
        const int word = 2 * ch + (lane >> 5);
        if ((lane & 31) == 0 && word < wpr)
            bits[(int64_t)iy * wpr + word] = (uint32_t)(m >> (lane & 32));
    }
}

inline void r9s_free_bits_host(const KRoute& g, const uint4* rec, uint32_t* bits) {
    const int wpr = r9s_wpr(g.nx);
    for (int iy = 0; iy < g.ny; ++iy)
        for (int w = 0; w < wpr; ++w) {
            uint32_t m = 0u;
            for (int b = 0; b < 32 && (int64_t)w * 32 + b < g.nx; ++b)
                if (r9_cost(g, rec, w * 32 + b, iy) < r9_inf()) m |= 1u << b;
            bits[(int64_t)iy * wpr + w] = m;
        }
}

// ---- the smoothing kernel ----------------------------------------------------------------------
// (k_route_joint_smooth and k_route3_smooth are these lines again: the kernel owns its LDS)
__global__ __launch_bounds__(R9S_WAVES * 64) void k_route_smooth(
    KRoute g, const uint32_t* __restrict__ bits, const uint8_t* __restrict__ next,
    const double* __restrict__ goals, int32_t n_goals, const double* __restrict__ starts,
    const int32_t* __restrict__ goal_idx, int64_t n_queries, int32_t N, int32_t span,
    double* __restrict__ wp, int32_t* __restrict__ status, int32_t* __restrict__ steps,
    int32_t* __restrict__ vertices) {
    __shared__ int32_t s_ring[R9S_WAVES][R9S_RING];
    __shared__ int32_t s_list[R9S_WAVES][R9S_LIST];
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int lane = threadIdx.x & 63;
    const int64_t q = (int64_t)blockIdx.x * R9S_WAVES + wave;
    if (q >= n_queries) return;  // whole waves leave; no workgroup barrier below
    r9_smooth_wave<false>(g, bits, next, goals, n_goals, starts, goal_idx, q, N, span, wp, status,
                          steps, vertices, nullptr, s_ring[wave], s_list[wave], lane);
}
