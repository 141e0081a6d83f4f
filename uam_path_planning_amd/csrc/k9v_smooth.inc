// k9v_smooth.inc -- K9vb / K9vs, any-angle shortcuts on the traced route in the volume
// (include/uampath.h "Route seeds in the volume, smoothing"): k_route3_free_bits (one bit per
// voxel, set = free), k_route3_smooth (one wave per query: the chain along next, the anchors by
// "advance while visible", the resampled waypoints), and the __host__ __device__ pieces they
// share with uam_route3d_free_bits_host / uam_route3d_paths_smooth_host /
// uam_route3d_visible_host.  Integer arithmetic decides every visibility; the float64
// operations are r9v_trace's, in its order.  This is K9s (k9_smooth.inc) restated over voxels:
// the anchor loop and the two-pass skeleton are K9s', written out again here so that
// k_route_smooth's code and resources stay what they were (DESIGN section 4, K9vb / K9vs).
// R9S_WAVES, R9S_RING and R9S_LIST are K9s'.
// Included in the anonymous namespace of uampath.hip, after k9v_route.inc and k9_smooth.inc.

// bit v & 31 of word v >> 5, v the voxel index (layer fastest)
__host__ __device__ __forceinline__ bool r9vs_free(const uint32_t* bits, int64_t v) {
    return (bits[v >> 5] >> (v & 31)) & 1u;
}

// one minor axis' interval at step i of the major axis: the v = lo..hi in [0, amin] with
// 2*|amaj*v - amin*i| <= amaj + amin
template <typename I>
__host__ __device__ __forceinline__ void r9vs_interval(I amaj, I amin, I i, I* lo, I* hi) {
    const I c = 2 * amin * i, s = amaj + amin, den = 2 * amaj;
    *lo = c > s ? (c - s + den - 1) / den : 0;
    const I h = (c + s) / den;
    *hi = h < amin ? h : amin;
}

// LOS3(A, B): every voxel of T3(A, B) is free.  T3 is walked along the segment's major axis m;
// at step i the two inequalities that involve m give one interval on each minor axis (u, v: the
// other two axes in x, y, z order), and the third inequality is tested per pair inside them.
// Reflected into d >= 0 the three cross terms are |am*p - au*i|, |am*r - av*i|, |au*r - av*p|.
// Both voxels are in the volume, and so is their bounding box; a voxel of it has the index
// va + i*sm + p*su + r*sv with the signed strides of the three axes.  I = int32_t serves
// |d| <= 1024 (2*amin*i + amaj + amin < 2^22) and indices below 2^31.
template <typename I>
__host__ __device__ inline bool r9vs_los(const uint32_t* bits, I nx, I nz, I ax, I ay, I az, I bx,
                                         I by, I bz) {
    const I dx = bx - ax, dy = by - ay, dz = bz - az;
    const I adx = dx < 0 ? -dx : dx, ady = dy < 0 ? -dy : dy, adz = dz < 0 ? -dz : dz;
    const int m = adx >= ady ? (adx >= adz ? 0 : 2) : (ady >= adz ? 1 : 2);
    const I am = m == 0 ? adx : m == 1 ? ady : adz;
    const I au = m == 0 ? ady : adx;
    const I av = m == 2 ? ady : adz;
    const I va = (ay * nx + ax) * nz + az;
    if (am == 0) return r9vs_free(bits, va);
    const I tx = dx < 0 ? -nz : nz, ty = dy < 0 ? -(nx * nz) : nx * nz, tz = dz < 0 ? -1 : 1;
    const I sm = m == 0 ? tx : m == 1 ? ty : tz;
    const I su = m == 0 ? ty : tx;
    const I sv = m == 2 ? ty : tz;
    const I s3 = au + av;
    for (I i = 0; i <= am; ++i) {
        I plo, phi, rlo, rhi;
        r9vs_interval<I>(am, au, i, &plo, &phi);
        r9vs_interval<I>(am, av, i, &rlo, &rhi);
        for (I p = plo; p <= phi; ++p)
            for (I r = rlo; r <= rhi; ++r) {
                const I t = au * r - av * p;
                if (2 * (t < 0 ? -t : t) <= s3 && !r9vs_free(bits, va + i * sm + p * su + r * sv))
                    return false;
            }
    }
    return true;
}

// LOS3 between two voxels of the chain (voxel indices)
__host__ __device__ __forceinline__ bool r9vs_visible(const uint32_t* bits, const KRoute3& g,
                                                      int32_t a, int32_t b) {
    const int32_t ca = a / g.nz, cb = b / g.nz;
    return r9vs_los<int32_t>(bits, g.nx, g.nz, ca % g.nx, ca / g.nx, a % g.nz, cb % g.nx,
                             cb / g.nx, b % g.nz);
}

// a query's end points, voxels, field and status 4 / 1 / 2 (r9v_trace's tests in its order; the
// start's blocking from the bits)
struct R9vsQuery {
    double sx, sy, sz, gx, gy, gz;
    int32_t svox, gvox;
    const uint8_t* nf;
    int st;
};

__host__ __device__ inline R9vsQuery r9vs_query(const KRoute3& g, const uint32_t* bits,
                                                const uint8_t* next, const double* goals,
                                                int32_t n_goals, const double* starts,
                                                const int32_t* goal_idx, int64_t q) {
    R9vsQuery u;
    u.sx = starts[3 * q], u.sy = starts[3 * q + 1], u.sz = starts[3 * q + 2];
    u.gx = u.sx, u.gy = u.sy, u.gz = u.sz;  // a goal index out of range: the start point
    u.svox = u.gvox = -1;
    u.nf = next;
    u.st = 0;
    const int32_t gi = goal_idx[q];
    if (gi < 0 || gi >= n_goals) {
        u.st = 4;
    } else {
        u.gx = goals[3 * (int64_t)gi], u.gy = goals[3 * (int64_t)gi + 1],
        u.gz = goals[3 * (int64_t)gi + 2];
        u.nf = next + (int64_t)gi * r9v_voxels(g);
        u.gvox = r9v_voxel(g, u.gx, u.gy, u.gz);
        if (u.gvox < 0 || u.nf[u.gvox] != R9V_GOAL) u.st = 4;
    }
    if (!u.st) {
        u.svox = r9v_voxel(g, u.sx, u.sy, u.sz);
        if (u.svox < 0 || !r9vs_free(bits, u.svox)) u.st = 1;
    }
    if (!u.st && u.nf[u.svox] == 255) u.st = 2;
    return u;
}

// the straight line of a nonzero status: waypoints j0, j0 + stride, ..
__host__ __device__ inline void r9vs_straight(const R9vsQuery& u, int32_t N, double* out, int j0,
                                              int stride) {
    const double dn1 = (double)(N + 1);
    for (int j = j0; j <= N; j += stride) {
        const double f = (double)j / dn1;
        out[3 * j] = u.sx + (u.gx - u.sx) * f;
        out[3 * j + 1] = u.sy + (u.gy - u.sy) * f;
        out[3 * j + 2] = u.sz + (u.gz - u.sz) * f;
    }
}

__host__ __device__ __forceinline__ void r9vs_centre(const KRoute3& g, int32_t vox, double* x,
                                                     double* y, double* z) {
    const int32_t col = vox / g.nz;
    *x = g.x0 + ((double)(col % g.nx) + 0.5) * g.dx;
    *y = g.y_top - ((double)(col / g.nx) + 0.5) * g.dy;
    *z = g.z0 + ((double)(vox % g.nz) + 0.5) * g.dz;
}

// The vertices V_1, V_2, .. of a path taken one after the other: pass 1 sums S_m, pass 2 (sm
// known) places the waypoints, r9v_trace's second walk operation for operation.
struct R9vsPath {
    double vx, vy, vz;  // V_{i-1}
    double s;           // S_{i-1}
    double sm, dn1;
    int32_t j, N;
    double* out;        // NULL: pass 1
    bool write;         // this lane stores the waypoints
};

__host__ __device__ inline void r9vs_vertex(const KRoute3& g, R9vsPath& p, double x, double y,
                                            double z, bool last) {
    const double si = p.s + r9v_seg(g, p.vx, p.vy, p.vz, x, y, z);
    if (p.out) {
        while (p.j <= p.N) {
            const double t = p.sm * ((double)p.j / p.dn1);
            if (!last && !(si > t)) break;
            const double den = si - p.s;
            const double u = den > 0.0 ? (t - p.s) / den : 0.0;
            const double wx = p.vx + u * (x - p.vx), wy = p.vy + u * (y - p.vy),
                         wz = p.vz + u * (z - p.vz);
            if (p.write) p.out[3 * p.j] = wx, p.out[3 * p.j + 1] = wy, p.out[3 * p.j + 2] = wz;
            ++p.j;
        }
    }
    p.s = si;
    p.vx = x, p.vy = y, p.vz = z;
}

// one step of the chain from vox (count voxels visited so far): 1 = moved, -1 = the walk left
// the field (r9v_step's rules)
__host__ __device__ __forceinline__ int r9vs_hop(const KRoute3& g, int k, int32_t* vox,
                                                 int64_t count) {
    if (count >= r9v_voxels(g)) return -1;
    if (k >= R9V_DIRS) return -1;
    const int col = *vox / g.nz;
    const int ix = col % g.nx + r9v_dix(k), iy = col / g.nx + r9v_diy(k),
              iz = *vox % g.nz + r9v_diz(k);
    if (ix < 0 || ix >= g.nx || iy < 0 || iy >= g.ny || iz < 0 || iz >= g.nz) return -1;
    *vox = r9v_index(g, ix, iy, iz);
    return 1;
}

// ---- host twins -----------------------------------------------------------------------------
inline void r9vs_free_bits_host(const KRoute3& g, const uint2* vox, const uint2* col,
                                uint32_t* bits) {
    const int64_t n = r9v_voxels(g);
    for (int64_t w = 0; w < (n + 31) >> 5; ++w) {
        uint32_t m = 0u;
        for (int b = 0; b < 32 && w * 32 + b < n; ++b) {
            const int64_t i = w * 32 + b, c2 = i / g.nz;
            if (r9v_cost(g, vox, col, (int)(c2 % g.nx), (int)(c2 / g.nx), (int)(i % g.nz)) <
                r9_inf())
                m |= 1u << b;
        }
        bits[w] = m;
    }
}

inline void r9vs_smooth_host(const KRoute3& g, const uint32_t* bits, const uint8_t* next,
                             const double* goals, int32_t n_goals, const double* starts,
                             const int32_t* goal_idx, int64_t q, int32_t N, int32_t span,
                             double* wp, int32_t* status, int32_t* steps, int32_t* vertices,
                             std::vector<int32_t>& cells, std::vector<int32_t>& anchors) {
    R9vsQuery u = r9vs_query(g, bits, next, goals, n_goals, starts, goal_idx, q);
    double* out = wp + q * (int64_t)(N + 2) * 3;
    cells.clear();
    anchors.clear();
    if (!u.st) {
        int32_t vox = u.svox;
        cells.push_back(vox);
        while (vox != u.gvox) {
            if (r9vs_hop(g, u.nf[vox], &vox, (int64_t)cells.size()) < 0) {
                u.st = 3;
                break;
            }
            cells.push_back(vox);
        }
    }
    out[0] = u.sx, out[1] = u.sy, out[2] = u.sz;
    out[3 * (N + 1)] = u.gx, out[3 * (N + 1) + 1] = u.gy, out[3 * (N + 1) + 2] = u.gz;
    status[q] = u.st;
    if (steps) steps[q] = u.st ? 0 : (int32_t)cells.size();
    if (u.st) {
        if (vertices) vertices[q] = 0;
        r9vs_straight(u, N, out, 1, 1);
        return;
    }
    const int64_t n = (int64_t)cells.size();
    if (n > 2) {
        int64_t a = 1;
        anchors.push_back(cells[1]);
        while (a != n - 2) {
            const int64_t jmax = a + span < n - 2 ? a + span : n - 2;
            // advance while visible; c_{a+1} is taken untested (adjacent chain voxels are
            // visible)
            int64_t j = a + 1;
            while (j < jmax && r9vs_visible(bits, g, cells[(size_t)a], cells[(size_t)j + 1])) ++j;
            a = j;
            anchors.push_back(cells[(size_t)a]);
        }
    }
    if (vertices) vertices[q] = (int32_t)anchors.size() + 2;
    R9vsPath p{u.sx, u.sy, u.sz, 0.0, 0.0, (double)(N + 1), 1, N, nullptr, true};
    double x, y, z;
    for (int32_t c : anchors) {
        r9vs_centre(g, c, &x, &y, &z);
        r9vs_vertex(g, p, x, y, z, false);
    }
    r9vs_vertex(g, p, u.gx, u.gy, u.gz, true);
    p = R9vsPath{u.sx, u.sy, u.sz, 0.0, p.s, (double)(N + 1), 1, N, out, true};
    for (int32_t c : anchors) {
        r9vs_centre(g, c, &x, &y, &z);
        r9vs_vertex(g, p, x, y, z, false);
    }
    r9vs_vertex(g, p, u.gx, u.gy, u.gz, true);
}

// ---- kernels --------------------------------------------------------------------------------
// the free bits: one wave per 64 consecutive voxel indices, one lane per voxel; lanes 0 and 32
// store the two words of the wave's ballot (bits past the last voxel stay 0)
__global__ __launch_bounds__(R9_THREADS) void k_route3_free_bits(const uint2* __restrict__ vox,
                                                                 const uint2* __restrict__ col,
                                                                 KRoute3 g,
                                                                 uint32_t* __restrict__ bits) {
    const int lane = threadIdx.x & 63;
    const int64_t n = r9v_voxels(g);
    const int64_t chunks = (n + 63) >> 6, words = (n + 31) >> 5;
    const int64_t w0 = (int64_t)blockIdx.x * (R9_THREADS / 64) + (threadIdx.x >> 6);
    for (int64_t w = w0; w < chunks; w += (int64_t)gridDim.x * (R9_THREADS / 64)) {
        const int64_t i = w * 64 + lane;
        bool fr = false;
        if (i < n) {
            const int64_t c2 = i / g.nz;
            fr = r9v_cost(g, vox, col, (int)(c2 % g.nx), (int)(c2 / g.nx), (int)(i % g.nz)) <
                 r9_inf();
        }
        const uint64_t m = __ballot(fr);
        const int64_t word = 2 * w + (lane >> 5);
        if ((lane & 31) == 0 && word < words) bits[word] = (uint32_t)(m >> (lane & 32));
    }
}

// The walk along next, the same in every lane of the wave: one load of next per hop; every
// voxel reached goes into the wave's ring (slot = chain index & mask).
struct R9vsWalk {
    int32_t vox;  // c_idx
    int32_t idx;  // chain index of vox
    bool done;    // vox is the goal's: n = idx + 1
    bool fail;    // status 3
};

__device__ inline void r9vs_advance(const KRoute3& g, const uint8_t* __restrict__ nf,
                                    int32_t gvox, R9vsWalk& w, int32_t upto, int32_t* ring,
                                    int lane) {
    while (!w.done && !w.fail && w.idx < upto) {
        if (r9vs_hop(g, nf[w.vox], &w.vox, (int64_t)w.idx + 1) < 0) {
            w.fail = true;
            break;
        }
        ++w.idx;
        if (lane == 0) ring[w.idx & (R9S_RING - 1)] = w.vox;
        if (w.vox == gvox) w.done = true;
    }
    wave_sync();
}

// One pass over a query's chain: anchors by "advance while visible", 64 candidates at a time,
// one lane each.  Every anchor goes to path (pass 1: S_m; pass 2: the waypoints) and, while
// there is room, into list.  Returns the number of anchors, -1 for status 3; *n_out = steps.
__device__ inline int32_t r9vs_pass(const KRoute3& g, const uint32_t* __restrict__ bits,
                                    const R9vsQuery& u, int32_t span, int32_t* ring,
                                    int32_t* list, R9vsPath& path, int32_t* n_out, int lane) {
    R9vsWalk w{u.svox, 0, u.svox == u.gvox, false};
    r9vs_advance(g, u.nf, u.gvox, w, 2, ring, lane);
    if (w.fail) return -1;
    int32_t na = 0;
    if (!(w.done && w.idx < 2)) {  // n > 2
        int32_t a = 1;
        int32_t avox = ring[1];
        for (;;) {
            double x, y, z;
            r9vs_centre(g, avox, &x, &y, &z);
            r9vs_vertex(g, path, x, y, z, false);
            if (list && na < R9S_LIST && lane == 0) list[na] = avox;
            ++na;
            r9vs_advance(g, u.nf, u.gvox, w, a + span, ring, lane);
            if (w.fail) return -1;
            if (w.done && a == w.idx - 1) break;  // a = n - 2
            const int32_t top = w.done && w.idx - 1 < a + span ? w.idx - 1 : a + span;
            int32_t j = top;
            for (int32_t base = a + 1; base <= top; base += 64) {
                const int32_t i = base + lane;
                bool blocked = false;
                if (i <= top && i > a + 1)  // adjacent chain voxels are visible
                    blocked = !r9vs_visible(bits, g, avox, ring[i & (R9S_RING - 1)]);
                const uint64_t m = __ballot(blocked);
                if (m) {
                    j = base + (__ffsll((unsigned long long)m) - 1) - 1;
                    break;
                }
            }
            a = j;
            avox = ring[a & (R9S_RING - 1)];
        }
    }
    *n_out = w.idx + 1;
    return na;
}

__global__ __launch_bounds__(R9S_WAVES * 64) void k_route3_smooth(
    KRoute3 g, const uint32_t* __restrict__ bits, const uint8_t* __restrict__ next,
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
    int32_t* ring = s_ring[wave];
    int32_t* list = s_list[wave];
    R9vsQuery u = r9vs_query(g, bits, next, goals, n_goals, starts, goal_idx, q);
    double* out = wp + q * (int64_t)(N + 2) * 3;
    int32_t n = 0, na = 0;
    R9vsPath p{u.sx, u.sy, u.sz, 0.0, 0.0, (double)(N + 1), 1, N, nullptr, false};
    if (!u.st) {
        na = r9vs_pass(g, bits, u, span, ring, list, p, &n, lane);
        if (na < 0) u.st = 3;
    }
    if (lane == 0) {
        out[0] = u.sx, out[1] = u.sy, out[2] = u.sz;
        out[3 * (N + 1)] = u.gx, out[3 * (N + 1) + 1] = u.gy, out[3 * (N + 1) + 2] = u.gz;
        status[q] = u.st;
        if (steps) steps[q] = u.st ? 0 : n;
        if (vertices) vertices[q] = u.st ? 0 : na + 2;
    }
    if (u.st) {
        r9vs_straight(u, N, out, 1 + lane, 64);
        return;
    }
    r9vs_vertex(g, p, u.gx, u.gy, u.gz, true);  // S_m
    R9vsPath e{u.sx, u.sy, u.sz, 0.0, p.s, (double)(N + 1), 1, N, out, lane == 0};
    if (na <= R9S_LIST) {
        wave_sync();
        for (int32_t k = 0; k < na; ++k) {
            double x, y, z;
            r9vs_centre(g, list[k], &x, &y, &z);
            r9vs_vertex(g, e, x, y, z, false);
        }
    } else {  // the list overflowed: the same anchors again, placed as they are found
        (void)r9vs_pass(g, bits, u, span, ring, nullptr, e, &n, lane);
    }
    r9vs_vertex(g, e, u.gx, u.gy, u.gz, true);
}
