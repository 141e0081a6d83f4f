// k9_smooth.inc -- K9b / K9s, any-angle shortcuts on the traced route (include/uampath.h "Route
// seeds", "smoothing"): k_route_free_bits (one bit per cell, set = free), k_route_smooth (one wave
// per query: the chain along next, the anchors by "advance while visible", the resampled
// waypoints), and the __host__ __device__ pieces they share with uam_route_free_bits_host /
// uam_route_paths_smooth_host / uam_route_visible_host.  Integer arithmetic decides every
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

// LOS between two cells of the chain (cell indices)
__host__ __device__ __forceinline__ bool r9s_visible(const uint32_t* bits, int nx, int32_t a,
                                                     int32_t b) {
    return r9s_los<int32_t>(bits, r9s_wpr(nx), a % nx, a / nx, b % nx, b / nx);
}

// a query's end points, cells, field and status 4 / 1 / 2 (r9_trace's tests in its order; the
// start's blocking from the bits)
struct R9sQuery {
    double sx, sy, gx, gy;
    int32_t scell, gcell;
    const uint8_t* nf;
    int st;
    int32_t gi;  // the goal index (J: the start cell's owner, -1 for a nonzero status)
};

// J (a joint field): r9_trace<true>'s rules, the start's blocking from the bits
template <bool J = false>
__host__ __device__ inline R9sQuery r9s_query(const KRoute& g, const uint32_t* bits,
                                              const uint8_t* next, const double* goals,
                                              int32_t n_goals, const double* starts,
                                              const int32_t* goal_idx, int64_t q) {
    R9sQuery u;
    u.sx = starts[2 * q], u.sy = starts[2 * q + 1];
    u.gx = u.sx, u.gy = u.sy;  // a goal index out of range: every waypoint is the start point
    u.scell = u.gcell = -1;
    u.nf = next;
    u.st = 0;
    if (J) {
        u.gi = -1;
        u.scell = r9_cell(g, u.sx, u.sy);
        if (u.scell < 0 || !r9s_free(bits, r9s_wpr(g.nx), u.scell % g.nx, u.scell / g.nx)) {
            u.st = 1;
        } else if (u.nf[u.scell] == 255) {
            u.st = 2;
        } else {
            const int32_t o = goal_idx[u.scell];
            if (o >= 0 && o < n_goals)
                u.gcell = r9_cell(g, goals[2 * (int64_t)o], goals[2 * (int64_t)o + 1]);
            if (u.gcell < 0) {
                u.st = 3;
            } else {
                u.gi = o;
                u.gx = goals[2 * (int64_t)o], u.gy = goals[2 * (int64_t)o + 1];
            }
        }
        return u;
    }
    const int32_t gi = goal_idx[q];
    u.gi = gi;
    if (gi < 0 || gi >= n_goals) {
        u.st = 4;
    } else {
        u.gx = goals[2 * (int64_t)gi], u.gy = goals[2 * (int64_t)gi + 1];
        u.nf = next + (int64_t)gi * g.nx * g.ny;
        u.gcell = r9_cell(g, u.gx, u.gy);
        if (u.gcell < 0 || u.nf[u.gcell] != 8) u.st = 4;
    }
    if (!u.st) {
        u.scell = r9_cell(g, u.sx, u.sy);
        if (u.scell < 0 || !r9s_free(bits, r9s_wpr(g.nx), u.scell % g.nx, u.scell / g.nx))
            u.st = 1;
    }
    if (!u.st && u.nf[u.scell] == 255) u.st = 2;
    return u;
}

// the straight line of a nonzero status: waypoints j0, j0 + stride, ..
__host__ __device__ inline void r9s_straight(const R9sQuery& u, int32_t N, double* out, int j0,
                                             int stride) {
    const double dn1 = (double)(N + 1);
    for (int j = j0; j <= N; j += stride) {
        const double f = (double)j / dn1;
        out[2 * j] = u.sx + (u.gx - u.sx) * f;
        out[2 * j + 1] = u.sy + (u.gy - u.sy) * f;
    }
}

__host__ __device__ __forceinline__ void r9s_centre(const KRoute& g, int32_t cell, double* x,
                                                    double* y) {
    *x = g.x0 + ((double)(cell % g.nx) + 0.5) * g.dx;
    *y = g.y_top - ((double)(cell / g.nx) + 0.5) * g.dy;
}

// The vertices V_1, V_2, .. of a path taken one after the other: pass 1 sums S_m, pass 2 (sm
// known) places the waypoints, r9_trace's second walk operation for operation.
struct R9sPath {
    double vx, vy;  // V_{i-1}
    double s;       // S_{i-1}
    double sm, dn1;
    int32_t j, N;
    double* out;    // NULL: pass 1
    bool write;     // this lane stores the waypoints
};

__host__ __device__ inline void r9s_vertex(R9sPath& p, double x, double y, bool last) {
    const double si = p.s + r9_seg(p.vx, p.vy, x, y);
    if (p.out) {
        while (p.j <= p.N) {
            const double t = p.sm * ((double)p.j / p.dn1);
            if (!last && !(si > t)) break;
            const double den = si - p.s;
            const double u = den > 0.0 ? (t - p.s) / den : 0.0;
            const double wx = p.vx + u * (x - p.vx), wy = p.vy + u * (y - p.vy);
            if (p.write) p.out[2 * p.j] = wx, p.out[2 * p.j + 1] = wy;
            ++p.j;
        }
    }
    p.s = si;
    p.vx = x, p.vy = y;
}

// one step of the chain from cell (count cells visited so far): 1 = moved, -1 = the walk left
// the field (r9_step's rules)
__host__ __device__ __forceinline__ int r9s_hop(const KRoute& g, int k, int32_t* cell,
                                                int64_t count) {
    if (count >= (int64_t)g.nx * g.ny) return -1;
    if (k > 7) return -1;
    const int ix = *cell % g.nx + r9_dix(k), iy = *cell / g.nx + r9_diy(k);
    if (ix < 0 || ix >= g.nx || iy < 0 || iy >= g.ny) return -1;
    *cell = iy * g.nx + ix;
    return 1;
}

// ---- host twin ------------------------------------------------------------------------------
template <bool J = false>
inline void r9s_smooth_host(const KRoute& g, const uint32_t* bits, const uint8_t* next,
                            const double* goals, int32_t n_goals, const double* starts,
                            const int32_t* goal_idx, int64_t q, int32_t N, int32_t span,
                            double* wp, int32_t* status, int32_t* steps, int32_t* vertices,
                            std::vector<int32_t>& cells, std::vector<int32_t>& anchors,
                            int32_t* goal_out = nullptr) {
    R9sQuery u = r9s_query<J>(g, bits, next, goals, n_goals, starts, goal_idx, q);
    double* out = wp + q * (int64_t)(N + 2) * 2;
    cells.clear();
    anchors.clear();
    if (!u.st) {
        int32_t cell = u.scell;
        cells.push_back(cell);
        while (cell != u.gcell) {
            if (r9s_hop(g, u.nf[cell], &cell, (int64_t)cells.size()) < 0) {
                u.st = 3;
                break;
            }
            cells.push_back(cell);
        }
    }
    if (J) {
        if (u.st) u.gx = u.sx, u.gy = u.sy, u.gi = -1;
        if (goal_out) goal_out[q] = u.gi;
    }
    out[0] = u.sx, out[1] = u.sy;
    out[2 * (N + 1)] = u.gx, out[2 * (N + 1) + 1] = u.gy;
    status[q] = u.st;
    if (steps) steps[q] = u.st ? 0 : (int32_t)cells.size();
    if (u.st) {
        if (vertices) vertices[q] = 0;
        r9s_straight(u, N, out, 1, 1);
        return;
    }
    const int64_t n = (int64_t)cells.size();
    if (n > 2) {
        int64_t a = 1;
        anchors.push_back(cells[1]);
        while (a != n - 2) {
            const int64_t jmax = a + span < n - 2 ? a + span : n - 2;
            // advance while visible; c_{a+1} is taken untested (adjacent chain cells are visible)
            int64_t j = a + 1;
            while (j < jmax && r9s_visible(bits, g.nx, cells[(size_t)a], cells[(size_t)j + 1])) ++j;
            a = j;
            anchors.push_back(cells[(size_t)a]);
        }
    }
    if (vertices) vertices[q] = (int32_t)anchors.size() + 2;
    R9sPath p{u.sx, u.sy, 0.0, 0.0, (double)(N + 1), 1, N, nullptr, true};
    double x, y;
    for (int32_t c : anchors) {
        r9s_centre(g, c, &x, &y);
        r9s_vertex(p, x, y, false);
    }
    r9s_vertex(p, u.gx, u.gy, true);
    p = R9sPath{u.sx, u.sy, 0.0, p.s, (double)(N + 1), 1, N, out, true};
    for (int32_t c : anchors) {
        r9s_centre(g, c, &x, &y);
        r9s_vertex(p, x, y, false);
    }
    r9s_vertex(p, u.gx, u.gy, true);
}

// ---- kernels --------------------------------------------------------------------------------
// the free bits: one wave per 64 cells of a row, one lane per cell; lanes 0 and 32 store the
// two words of the wave's ballot (bits past nx stay 0)
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

// The walk along next, the same in every lane of the wave: the lanes load the 8 x 8 patch of
// next around the current cell, and the chain is followed inside it with shuffles until it
// leaves the patch; every cell reached goes into the wave's ring (slot = chain index & mask).
struct R9sWalk {
    int32_t cell;  // c_idx
    int32_t idx;   // chain index of cell
    bool done;     // cell is the goal's: n = idx + 1
    bool fail;     // status 3
};

__device__ inline void r9s_advance(const KRoute& g, const uint8_t* __restrict__ nf, int32_t gcell,
                                   R9sWalk& w, int32_t upto, int32_t* ring, int lane) {
    while (!w.done && !w.fail && w.idx < upto) {
        const int ox = w.cell % g.nx - 4, oy = w.cell / g.nx - 4;
        const int px = ox + (lane & 7), py = oy + (lane >> 3);
        int mine = 255;
        if (px >= 0 && px < g.nx && py >= 0 && py < g.ny) mine = nf[(int64_t)py * g.nx + px];
        for (;;) {
            const int cx = w.cell % g.nx, cy = w.cell / g.nx;
            const int lx = cx - ox, ly = cy - oy;
            if (lx < 0 || lx > 7 || ly < 0 || ly > 7) break;  // the next patch
            const int k = __shfl(mine, ly * 8 + lx, 64);
            if (r9s_hop(g, k, &w.cell, (int64_t)w.idx + 1) < 0) {
                w.fail = true;
                break;
            }
            ++w.idx;
            if (lane == 0) ring[w.idx & (R9S_RING - 1)] = w.cell;
            if (w.cell == gcell) {
                w.done = true;
                break;
            }
            if (w.idx >= upto) break;
        }
    }
    wave_sync();
}

// One pass over a query's chain: anchors by "advance while visible", 64 candidates at a time,
// one lane each.  Every anchor goes to path (pass 1: S_m; pass 2: the waypoints) and, while
// there is room, into list.  Returns the number of anchors, -1 for status 3; *n_out = steps.
__device__ inline int32_t r9s_pass(const KRoute& g, const uint32_t* __restrict__ bits,
                                   const R9sQuery& u, int32_t span, int32_t* ring, int32_t* list,
                                   R9sPath& path, int32_t* n_out, int lane) {
    R9sWalk w{u.scell, 0, u.scell == u.gcell, false};
    r9s_advance(g, u.nf, u.gcell, w, 2, ring, lane);
    if (w.fail) return -1;
    int32_t na = 0;
    if (!(w.done && w.idx < 2)) {  // n > 2
        int32_t a = 1;
        int32_t acell = ring[1];
        for (;;) {
            double x, y;
            r9s_centre(g, acell, &x, &y);
            r9s_vertex(path, x, y, false);
            if (list && na < R9S_LIST && lane == 0) list[na] = acell;
            ++na;
            r9s_advance(g, u.nf, u.gcell, w, a + span, ring, lane);
            if (w.fail) return -1;
            if (w.done && a == w.idx - 1) break;  // a = n - 2
            const int32_t top = w.done && w.idx - 1 < a + span ? w.idx - 1 : a + span;
            int32_t j = top;
            for (int32_t base = a + 1; base <= top; base += 64) {
                const int32_t i = base + lane;
                bool blocked = false;
                if (i <= top && i > a + 1)  // adjacent chain cells are visible
                    blocked = !r9s_visible(bits, g.nx, acell, ring[i & (R9S_RING - 1)]);
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

// One wave's query, k_route_smooth's body and (J, a joint field: r9s_query<true>'s rules and
// goal_out) k_route_joint_smooth's.  ring and list are the wave's LDS.
template <bool J>
__device__ __forceinline__ void r9s_smooth_wave(
    const KRoute& g, const uint32_t* __restrict__ bits, const uint8_t* __restrict__ next,
    const double* __restrict__ goals, int32_t n_goals, const double* __restrict__ starts,
    const int32_t* __restrict__ goal_idx, int64_t q, int32_t N, int32_t span,
    double* __restrict__ wp, int32_t* __restrict__ status, int32_t* __restrict__ steps,
    int32_t* __restrict__ vertices, int32_t* __restrict__ goal_out, int32_t* ring, int32_t* list,
    int lane) {
    R9sQuery u = r9s_query<J>(g, bits, next, goals, n_goals, starts, goal_idx, q);
    double* out = wp + q * (int64_t)(N + 2) * 2;
    int32_t n = 0, na = 0;
    R9sPath p{u.sx, u.sy, 0.0, 0.0, (double)(N + 1), 1, N, nullptr, false};
    if (!u.st) {
        na = r9s_pass(g, bits, u, span, ring, list, p, &n, lane);
        if (na < 0) u.st = 3;
    }
    if (J) {
        if (u.st) u.gx = u.sx, u.gy = u.sy, u.gi = -1;
        if (goal_out && lane == 0) goal_out[q] = u.gi;
    }
    if (lane == 0) {
        out[0] = u.sx, out[1] = u.sy;
        out[2 * (N + 1)] = u.gx, out[2 * (N + 1) + 1] = u.gy;
        status[q] = u.st;
        if (steps) steps[q] = u.st ? 0 : n;
        if (vertices) vertices[q] = u.st ? 0 : na + 2;
    }
    if (u.st) {
        r9s_straight(u, N, out, 1 + lane, 64);
        return;
    }
    r9s_vertex(p, u.gx, u.gy, true);  // S_m
    R9sPath e{u.sx, u.sy, 0.0, p.s, (double)(N + 1), 1, N, out, lane == 0};
    if (na <= R9S_LIST) {
        wave_sync();
        for (int32_t k = 0; k < na; ++k) {
            double x, y;
            r9s_centre(g, list[k], &x, &y);
            r9s_vertex(e, x, y, false);
        }
    } else {  // the list overflowed: the same anchors again, placed as they are found
        (void)r9s_pass(g, bits, u, span, ring, nullptr, e, &n, lane);
    }
    r9s_vertex(e, u.gx, u.gy, true);
}

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
    r9s_smooth_wave<false>(g, bits, next, goals, n_goals, starts, goal_idx, q, N, span, wp, status,
                           steps, vertices, nullptr, s_ring[wave], s_list[wave], lane);
}
