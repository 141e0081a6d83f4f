// k9v_smooth.inc -- K9vb / K9vs, any-angle shortcuts on the traced route in the volume
// (include/uampath.h "Route seeds in the volume, smoothing"): what is the volume's own of the
// smoothing written once in k9_smooth.inc.  k_route3_free_bits (one bit per voxel, set = free)
// with its host twin, the sight line r9vs_los (another algorithm than the raster's, not its
// third dimension), KRoute3's overloads of the vocabulary on the free bits (r9_bit_free,
// r9_visible, and r9_advance: a plain load per hop where the raster shuffles a patch, DESIGN
// section 4, K9vb / K9vs), and k_route3_smooth round r9_smooth_wave.  R9S_WAVES, R9S_RING and
// R9S_LIST are K9s'.
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

// ---- the grid vocabulary on the free bits ---------------------------------------------------
__host__ __device__ __forceinline__ bool r9_bit_free(const KRoute3&, const uint32_t* bits,
                                                     int32_t vox) {
    return r9vs_free(bits, vox);
}

// LOS3 between two voxels of the chain
__host__ __device__ __forceinline__ bool r9_visible(const KRoute3& g, const uint32_t* bits,
                                                    int32_t a, int32_t b) {
    const int32_t ca = a / g.nz, cb = b / g.nz;
    return r9vs_los<int32_t>(bits, g.nx, g.nz, ca % g.nx, ca / g.nx, a % g.nz, cb % g.nx,
                             cb / g.nx, b % g.nz);
}

// the volume's walk up to chain index upto: one load of next per hop
__device__ inline void r9_advance(const KRoute3& g, const uint8_t* __restrict__ nf, int32_t gvox,
                                  R9sWalk& w, int32_t upto, int32_t* ring, int lane) {
    while (!w.done && !w.fail && w.idx < upto)
        (void)r9s_hopped(g, nf[w.cell], gvox, w, ring, lane);
    wave_sync();
}

// ---- the free bits ----------------------------------------------------------------------------
// one wave per 64 consecutive voxel indices, one lane per voxel; lanes 0 and 32 store the two
// words of the wave's ballot (bits past the last voxel stay 0)
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

// ---- the smoothing kernel ----------------------------------------------------------------------
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
    r9_smooth_wave<false>(g, bits, next, goals, n_goals, starts, goal_idx, q, N, span, wp, status,
                          steps, vertices, nullptr, s_ring[wave], s_list[wave], lane);
}
