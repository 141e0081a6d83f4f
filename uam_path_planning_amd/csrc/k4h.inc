// k4h.inc -- K4h, the packed volume in the similarity form: VSlot / VSlotX, KVol4, the pack
// kernels (k_volume_pack_planes, k_volume_pack_t4, k_volume_codes), KProf, v_path_seed,
// k_v_eval (k_v_eval_x: its exact form; k_vp_eval / k_vp_eval_x: its instances with the profile
// table), v_path_slots, k_v_final / k_v_final_x.  The histogram launch (k_v_hist / k_vp_hist) is
// gsort.inc's k_sort_hist.
// Included in the anonymous namespace of uampath.hip; relies on its text above (the device tables,
// arc_point, pk_bound_decode, pk_terms_k, xcd_chunk, K2g's KGrp, UGeo, sim_geo, put_*) and on
// k2h.inc (X128, x_add, x_term, x_result).
//
// The seed, the histogram and the evaluation serve two forms of the altitude: K4h's straight
// climb and K4hp's profile table (k4hp.inc), which they take as a trailing parameter pack of
// zero or one KProf -- K4h's instances keep their argument list.  PROF, the pack's presence,
// guards every statement that is per form: the path split (the profile rides inside the path
// index), the table staged in LDS after the arc rows, and where z comes from.

// ---- K4h: the volume (config 5) in K2h's form -------------------------------------------------
// The packed volume (uam_volume_pack; layout: VpkDims).  Planes in K2h's 4 x 8-column blocks,
// one per layer (layer-major), all at one index i4: r4 {risk}, e8 {risk, |psi| | nfz << 31} and
// v16, the whole voxel {risk, psi_nfz, terrain, flags} (the column's terrain and flags beside
// the layer's pair); t4 the column terrain (one layer, the same column index).  A header
// (staged in LDS) holds a 2-bit code per 8 x 8-column block -- 0: every voxel of its columns has
// risk == +-0, psi == +-0 and no no-fly flag (nothing to read but the terrain); 1: psi == +-0 and
// no flag (r4); 2: no psi below zero (e8); 3: v16 -- then the column terrain's bounds (the
// raster's scheme: u16 codes per bound block of columns, float2 {base, step} per 4 x 4 bound
// blocks).  The (path, group) items are sorted on the altitude band and the Hilbert tile of the
// middle waypoint (band-major, so the items an XCD runs together share a band's lines),
// evaluated with K2h's grouped partial sums, and the output launch adds the similarity-form
// geometry.  Definition: oracle orc_eval_generated_h, mode 2.

struct alignas(16) VSlot {  // 32 B per (path, group)
    double cost;   // risk / N of the group's waypoints, from +0.0 in waypoint order
    double psi;    // psi_nfz likewise
    double cm;     // min over the group's waypoints of z_j - terrain (+inf: none)
    uint32_t cnt;  // nfz hits | off-volume << 8 | below-terrain << 16
    uint32_t pad;
};

struct alignas(16) VSlotX {  // the exact form's slot (UAM_OPT_EXACT_SUM_VOLUME): 48 B
    uint64_t c_lo, c_hi;  // the sum of the group's risk terms
    uint64_t n_lo, n_hi;  // the sum of its psi terms
    double cm;            // as VSlot's
    uint32_t cnt;         // as VSlot's | risk flags << 24 | psi flags << 27
    uint32_t pad;
};

struct KVol4 {
    int32_t nx, ny, nz;
    double x0, y_top, z0, dz, inv_dx, inv_dy, inv_dz;
    int32_t zshift, nbands;
    const uint32_t* __restrict__ hdr;   // codes | bounds | superblocks
    int32_t hwords, cnbx, bnd_off, sbt_off, bshift, bnbx, sbnbx;
    int32_t nb8, lnby4;
    uint32_t layer;                     // i4 entries per layer (lnby4 nb8 32)
    // the planes from the packed base by 32-bit byte offsets (o4: r4, o8: e8, o16: v16, ot4:
    // t4); null when the copy is 4 GiB or larger or a layer holds 2^24 entries (K4h stands aside)
    const char* __restrict__ pk;
    uint32_t o4, o8, o16, ot4;
    // the terrain-in-entry form's plane q8 {risk, column terrain} in 4 x 4-column blocks per
    // layer (nb4 blocks a row, layer44 entries a layer) at byte offset oq8
    uint32_t oq8, layer44;
    int32_t nb4;
    // v16 in 4 x 2-column blocks per layer (8 entries, one 128-B line): nbx4 blocks a row,
    // layer42 entries a layer
    uint32_t layer42;
    int32_t nbx4;
    // the exact form's scale words {e_risk, e_psi, flags, 0} (uam_volume_sum_scale; read by the
    // EX kernels only, null otherwise)
    const int32_t* __restrict__ xscale;
};

constexpr int VPK_CSHIFT = 3;           // code blocks of 8 x 8 columns
constexpr int VPK_HDR_LDS = 64 * 1024;  // the header in LDS up to this

// the column (ix, iy)'s index in the 4 x 8-column blocks (t4; i4 = it + iz layer)
__device__ __forceinline__ uint32_t vt4_index(const KVol4& v, int32_t ix, int32_t iy) {
    return ((__umul24((uint32_t)(iy >> 2), (uint32_t)v.nb8) + (uint32_t)(ix >> 3)) << 5) |
           (((uint32_t)iy & 3u) << 3) | ((uint32_t)ix & 7u);
}

// v16's in-layer index of column (ix, iy): 4 x 2-column blocks (8 entries of 16 B, one line)
__device__ __forceinline__ uint32_t vv16_index(const KVol4& v, int32_t ix, int32_t iy) {
    return ((__umul24((uint32_t)(iy >> 1), (uint32_t)v.nbx4) + (uint32_t)(ix >> 2)) << 3) |
           (((uint32_t)iy & 1u) << 2) | ((uint32_t)ix & 3u);
}

// q8's in-layer index of column (ix, iy): 4 x 4-column blocks (16 entries of 8 B, one line)
__device__ __forceinline__ uint32_t vq8_index(const KVol4& v, int32_t ix, int32_t iy) {
    return ((__umul24((uint32_t)(iy >> 2), (uint32_t)v.nb4) + (uint32_t)(ix >> 2)) << 4) |
           (((uint32_t)iy & 3u) << 2) | ((uint32_t)ix & 3u);
}

// the layer planes r4, e8, v16 and q8: one thread per i4 entry (r4 / e8 at i4, v16 and q8 at
// their own block indices), which writes all four (padding: zero)
__global__ __launch_bounds__(256) void k_volume_pack_planes(const uint2* __restrict__ vox,
                                                            const uint2* __restrict__ col,
                                                            KVol4 v, uint32_t* __restrict__ r4,
                                                            uint2* __restrict__ e8,
                                                            uint4* __restrict__ v16,
                                                            uint2* __restrict__ q8) {
    const int64_t total = (int64_t)v.nz * v.layer;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total;
         i += (int64_t)gridDim.x * blockDim.x) {
        const int32_t w = (int32_t)(i & 31);
        const int64_t blk = i >> 5;
        const int32_t bx = (int32_t)(blk % v.nb8);
        const int64_t r = blk / v.nb8;
        const int32_t by = (int32_t)(r % v.lnby4), iz = (int32_t)(r / v.lnby4);
        const int32_t ix = bx * 8 + (w & 7), iy = by * 4 + (w >> 3);
        uint2 a = make_uint2(0u, 0u), cl = make_uint2(0u, 0u);
        if (ix < v.nx && iy < v.ny) {
            const int64_t c = (int64_t)iy * v.nx + ix;
            a = vox[c * v.nz + iz];
            cl = col[c];
        }
        r4[i] = a.x;
        e8[i] = make_uint2(a.x, (a.y & 0x7fffffffu) | ((cl.y & UAM_FLAG_NFZ) ? 0x80000000u : 0u));
        if (ix < v.nbx4 * 4 && iy < ((v.ny + 1) >> 1) * 2)  // (v16's padded extent)
            v16[(int64_t)iz * v.layer42 + vv16_index(v, ix, iy)] = make_uint4(a.x, a.y, cl.x, cl.y);
        if (ix < v.nb4 * 4 && iy < v.lnby4 * 4)  // (q8 is narrower: nb4 4-column blocks)
            q8[(int64_t)iz * v.layer44 + vq8_index(v, ix, iy)] = make_uint2(a.x, cl.x);
    }
}

// the column terrain plane (one thread per entry; padding: zero)
__global__ __launch_bounds__(256) void k_volume_pack_t4(const uint2* __restrict__ col, KVol4 v,
                                                        float* __restrict__ t4) {
    const int64_t total = (int64_t)v.lnby4 * v.nb8 * 32;
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const int32_t w = (int32_t)(i & 31);
    const int64_t blk = i >> 5;
    const int32_t bx = (int32_t)(blk % v.nb8), by = (int32_t)(blk / v.nb8);
    const int32_t ix = bx * 8 + (w & 7), iy = by * 4 + (w >> 3);
    t4[i] = (ix < v.nx && iy < v.ny) ? __uint_as_float(col[(int64_t)iy * v.nx + ix].x) : 0.0f;
}

// the code map: one thread per 32-bit word (16 blocks of 8 x 8 columns)
__global__ __launch_bounds__(256) void k_volume_codes(const uint2* __restrict__ vox,
                                                      const uint2* __restrict__ col, int nx,
                                                      int ny, int nz, int cnbx, int nblocks,
                                                      int cwords, uint32_t* __restrict__ cmap) {
    const int wd = blockIdx.x * blockDim.x + threadIdx.x;
    if (wd >= cwords) return;
    uint32_t word = 0;
    for (int k = 0; k < 16; ++k) {
        const int b = wd * 16 + k;
        if (b >= nblocks) break;
        const int by = b / cnbx, bx = b - by * cnbx;
        bool need = false, neg = false, nz_r = false;
        for (int y = by << VPK_CSHIFT; y < min(ny, (by + 1) << VPK_CSHIFT); ++y)
            for (int x = bx << VPK_CSHIFT; x < min(nx, (bx + 1) << VPK_CSHIFT); ++x) {
                const int64_t c = (int64_t)y * nx + x;
                if (col[c].y & UAM_FLAG_NFZ) need = true;
                for (int iz = 0; iz < nz; ++iz) {  // every layer's own psi and risk
                    const uint2 a = vox[c * nz + iz];
                    if (a.y & 0x7fffffffu) need = true;
                    if ((a.y >> 31) && a.y != 0x80000000u) neg = true;
                    if (a.x & 0x7fffffffu) nz_r = true;
                }
            }
        const uint32_t code = need ? (neg ? 3u : 2u) : nz_r ? 1u : 0u;
        word |= code << (2 * k);
    }
    cmap[wd] = word;
}

// the altitude of waypoint j (uam_eval_generated3d: z0 + (zf - z0) (j / (N+1)))
__device__ __forceinline__ double vz_at(double za, double zb, double jw) {
    return za + (zb - za) * jw;
}

// the voxel of a generated point (false outside the volume or NaN, with (0, 0, 0) then: valid
// header and plane indices)
__device__ __forceinline__ bool vol_voxel(const KVol4& vs, double x0, double x1, double z,
                                          int32_t& ix, int32_t& iy, int32_t& iz) {
    const double tx = (x0 - vs.x0) * vs.inv_dx, ty = (vs.y_top - x1) * vs.inv_dy;
    const double tz = (z - vs.z0) * vs.inv_dz;
    const bool in = (tx >= 0.0) & (tx < (double)vs.nx) & (ty >= 0.0) & (ty < (double)vs.ny) &
                    (tz >= 0.0) & (tz < (double)vs.nz);
    ix = in ? (int32_t)tx : 0;
    iy = in ? (int32_t)ty : 0;
    iz = in ? (int32_t)tz : 0;
    return in;
}

// K4hp (uam_eval_generated3d_profiles_h): the altitude of waypoint j from the profile table
// instead of the straight climb.  The profile rides inside the path index, p = (q D + d) A + a,
// so KGrp describes P = Q D A paths with kg.D the lateral candidates (the unit-arc rows and
// k_g_scatter's UGeo rows are per d) and every shared launch (the scan, k_g_scatter) runs
// unchanged.  KGrp itself stays as it is -- it is a kernel argument of K2g / K2h / K4h -- and
// what the profile form adds travels in KProf.
struct KProf {
    const double* __restrict__ ztab;  // [A][W][3]
    int32_t A;
    int32_t sh_a;
    uint64_t m_a;  // div_magic's multiplier and shift for / A
};

constexpr int VPK_ZTAB_LDS = 40 * 1024;  // the profile rows in LDS up to this

// A kernel's optional trailing KProf argument (a parameter pack of zero or one), as vert_of
__device__ __forceinline__ KProf prof_of() { return KProf{}; }
__device__ __forceinline__ const KProf& prof_of(const KProf& f) { return f; }

// the table rule: two products, their sum, then the sum with the third coefficient (row: the
// profile's 3 W coefficients)
__device__ __forceinline__ double vp_z(const double* row, int j, double za, double zb) {
    const double* c = row + 3 * j;
    return (za * c[0] + zb * c[1]) + c[2];
}

// a path = (lateral path, profile); the lateral path = (pair, displacement)
__device__ __forceinline__ void vp_split(const KGrp& kg, const KProf& kf, int32_t path,
                                         int32_t& q, int32_t& d, int32_t& a) {
    const int32_t lat = (int32_t)div_magic((uint32_t)path, kf.m_a, kf.sh_a);
    a = path - lat * kf.A;
    q = (int32_t)div_magic((uint32_t)lat, kg.m_d, kg.sh_d);
    d = lat - q * kg.D;
}

// A path's clearance seed (k_v_eval's E and Ub): the exact clearance z - T (T the column's
// terrain, t4) of the in-volume sampled waypoint with the smallest z - lb, over j = 0, s, 2s,
// ... (s = kg.lb_stride) and j = W - 1, at their own voxels and altitudes by the evaluation's
// operations (+inf: none).  It is an exact clearance of the path, so at least the path's
// minimum M.  hdr / u: the packed header and the unit-arc table (LDS copies when staged).
// PROF: z by the table rule on the profile's row in global memory, formed with the sample's
// loads.
template <class... F>
__device__ __forceinline__ double v_path_seed(const KParams& p, const KVol4& vs, const KGrp& kg,
                                             int32_t path, const uint32_t* __restrict__ hdr,
                                             const double2* __restrict__ utab, const F&... f) {
    constexpr bool PROF = sizeof...(F) != 0;
    [[maybe_unused]] const KProf kf = prof_of(f...);
    int32_t q, d;
    [[maybe_unused]] int32_t a = 0;
    if constexpr (PROF) {
        vp_split(kg, kf, path, q, d, a);
    } else {
        q = (int32_t)div_magic((uint32_t)path, kg.m_d, kg.sh_d), d = path - q * kg.D;
    }
    const double* pr = kg.pairs + (int64_t)q * 6;
    const double ax = pr[0], ay = pr[1], za = pr[2], bx = pr[3], by = pr[4], zb = pr[5];
    const double2* u = utab + d * p.N - 1;
    const int W = kg.W;
    [[maybe_unused]] const double* zrow = nullptr;
    if constexpr (PROF) zrow = kf.ztab + (int64_t)a * W * 3;
    constexpr uint32_t NONE = 0xffffffffu;
    double Ub = INFINITY, zbest = 0.0;
    uint32_t best = NONE;  // the t4 index of the sample holding Ub
    auto take = [&](double x0, double x1, double z) {
        int32_t ix, iy, iz;
        const bool in = vol_voxel(vs, x0, x1, z, ix, iy, iz);
        const uint32_t bx2 = (uint32_t)(ix >> vs.bshift), by2 = (uint32_t)(iy >> vs.bshift);
        const uint32_t e = reinterpret_cast<const uint16_t*>(hdr + vs.bnd_off)[by2 * vs.bnbx + bx2];
        const float2 sb =
            reinterpret_cast<const float2*>(hdr + vs.sbt_off)[(by2 >> 2) * vs.sbnbx + (bx2 >> 2)];
        float ub, lb;
        pk_bound_decode(e, sb, ub, lb);
        const double v = z - (double)lb;
        const bool dn = in && v < Ub;  // (a NaN bound: no)
        Ub = dn ? v : Ub;
        zbest = dn ? z : zbest;
        best = dn ? vt4_index(vs, ix, iy) : best;
    };
    if constexpr (PROF) {
        take(ax, ay, vp_z(zrow, 0, za, zb));
        take(bx, by, vp_z(zrow, W - 1, za, zb));
    } else {
        take(ax, ay, vz_at(za, zb, 0.0 / (double)(W - 1)));
        take(bx, by, vz_at(za, zb, (double)(W - 1) / (double)(W - 1)));
    }
    // four samples at a time, every load of the four issued together (a sample past the last
    // interior waypoint repeats it)
    constexpr int K = 4;
    for (int j0 = kg.lb_stride; j0 < W - 1; j0 += K * kg.lb_stride) {
        double2 uu[K];
        int jj[K];
        [[maybe_unused]] double zz[K];
#pragma unroll
        for (int k = 0; k < K; ++k) {
            jj[k] = min(j0 + k * kg.lb_stride, W - 2);
            uu[k] = u[jj[k]];
            if constexpr (PROF) zz[k] = vp_z(zrow, jj[k], za, zb);
        }
#pragma unroll
        for (int k = 0; k < K; ++k) {
            double x0, x1;
            arc_point(ax, ay, bx, by, uu[k].x, uu[k].y, x0, x1);
            if constexpr (PROF) take(x0, x1, zz[k]);
            else take(x0, x1, vz_at(za, zb, (double)jj[k] / (double)(W - 1)));
        }
    }
    return best == NONE ? INFINITY
                        : zbest - (double)reinterpret_cast<const float*>(vs.pk + vs.ot4)[best];
}

// every (path, group) item in sorted order (h_item's phases): the CH waypoints' voxels (x, y by
// the arc formula or the pair's end points, z on the linear climb), the header reads, then per
// slot the decisions and two unconditional loads -- the code's entry (r4 / e8 / v16, the dummy
// line in code 0 or outside the volume) and the terrain (the first t4 word unless fetched) -- by
// 32-bit offsets from the packed base; then the branch-free consume.
//
// The terrain by bounds (as K2h's; the outputs are exactly the per-waypoint ones).  Waypoint j
// in the volume has lb_j <= T_j <= ub_j (the column grid's bounds) and
//   below_j = zc_j < T_j (zc_j its layer centre): decided when zc_j < lb_j (1) or zc_j >= ub_j
//       (0), else its terrain is fetched;
//   c_j = z_j - T_j, whose path minimum is min_clearance: z_j - ub_j <= c_j <= z_j - lb_j (the
//       float64 subtraction is monotone).  The item keeps Ub, an upper bound of the path minimum
//       M (the path's seed, then its own waypoints' z - lb), and E, the minimum of exact c_j of
//       the path: the seed (v_path_seed: the exact clearance of the sampled waypoint with the
//       smallest z - lb, formed once per path by the histogram launch) and those it takes
//       (fetched, v16's, one-value blocks); it fetches w iff it is undecided or
//       !(z_w - ub_w >= E) && !(z_w - ub_w > Ub).  If w* holds M and is not taken: z - ub >= E
//       gives M >= E >= M, and z - ub > Ub >= M is impossible.  NaN bounds (no bound) always
//       fetch.
// EX (UAM_OPT_EXACT_SUM_VOLUME; k_v_eval_x below): the risk and psi words added as 128-bit
// integer terms at the volume's exponents e_risk / e_psi (x_term) into a VSlotX, the non-finite
// ones as side flags.  One body for both forms, in the kernel itself: moved into an inlined
// function, the EX = false instantiations no longer allocated the registers they had (DESIGN
// §10), so the exact form is this kernel's third template flag and vs.xscale its scale.
// PROF (a trailing KProf: k_vp_eval, K4hp): the profile rows staged in LDS beside the arc rows
// (24 A W bytes + padding, in place of the j / (W-1) table): a lane's row is s_jw + 3 a W, and
// waypoint j's altitude is the table rule on it (vp_z), formed once in phase 1 and kept in
// registers for the consume loop (the straight climb forms vz_at a second time there from one LDS
// word; three words per slot read again cost 24 VGPRs at CH = 7 and spilled at CH = 6, 8 and 16
// -- DESIGN §10.1).  A slot past the group's end reads the next row or the padding (zeros): its
// voxel is masked, and whatever its z, vol_voxel gives indices inside the volume.  The per-form
// statements stand under `if constexpr (PROF)` in this body, not in a shared inlined function,
// for the reason above.
template <int CH, bool TE, bool EX = false, class... F>  // TE: the terrain in the entry
                                                         // (UAM_OPT_K4H_TERRAIN 1)
__global__ __launch_bounds__(256, CH >= 11 ? 2 : CH >= 7 ? 3 : 4) void k_v_eval(KParams p, KVol4 vs,
                                                                              KGrp kg, F... f) {
    PK_CODES_CHECK(CH);
    constexpr bool PROF = sizeof...(F) != 0;
    static_assert(sizeof...(F) <= 1, "at most one KProf");
    [[maybe_unused]] const KProf kf = prof_of(f...);
    // unit-arc rows + padding, then j / (W-1) or the profile rows (+ padding), then the header
    extern __shared__ __attribute__((aligned(16))) double2 s_u[];
    const int N = p.N, W = kg.W;
    const int nu = kg.D * N, npad = kg.G + 16;  // a lane's slots reach j <= W + G + CH - 3
    double* s_jw = reinterpret_cast<double*>(s_u + nu + npad);
    int njw;
    if constexpr (PROF) njw = (kf.A * W + npad) * 3;
    else njw = W + npad;
    uint32_t* s_hdr = reinterpret_cast<uint32_t*>(s_jw + ((njw + 1) & ~1));
    // the item's order entry, pair and path bound before the staging (their round trips
    // overlap it)
    const int64_t pos = xcd_chunk(blockIdx.x, gridDim.x) * 256 + threadIdx.x;
    const bool live = pos < kg.n_items;
    const int32_t item = live ? kg.order[pos] : 0;
    const int32_t path = (int32_t)div_magic((uint32_t)item, kg.m_nseg, kg.sh_nseg);
    const int s = item - path * kg.nseg;
    int32_t q, d;
    [[maybe_unused]] int32_t a = 0;  // PROF: the path's profile
    if constexpr (PROF) {
        vp_split(kg, kf, path, q, d, a);
    } else {
        q = (int32_t)div_magic((uint32_t)path, kg.m_d, kg.sh_d), d = path - q * kg.D;
    }
    const double* prp = kg.pairs + (int64_t)q * 6;
    const double2 pa = *reinterpret_cast<const double2*>(prp);
    const double2 pb = *reinterpret_cast<const double2*>(prp + 2);
    const double2 pc = *reinterpret_cast<const double2*>(prp + 4);
    const double seed = kg.ubp ? kg.ubp[path] : INFINITY;  // an exact clearance of the path
    double Ub = seed;
    for (int i = threadIdx.x; i < nu + npad; i += 256)
        s_u[i] = i < nu ? reinterpret_cast<const double2*>(kg.utab)[i] : make_double2(0.0, 0.0);
    if constexpr (PROF) {
        const int nz3 = kf.A * W * 3;
        for (int i = threadIdx.x; i < njw; i += 256) s_jw[i] = i < nz3 ? kf.ztab[i] : 0.0;
    } else {
        for (int j = threadIdx.x; j < njw; j += 256)
            s_jw[j] = j < W ? (double)j / (double)(W - 1) : 0.0;
    }
    {
        const uint4* src = reinterpret_cast<const uint4*>(vs.hdr);
        uint4* dst = reinterpret_cast<uint4*>(s_hdr);
        const int hw = TE ? vs.bnd_off : vs.hwords;  // (TE: the code map alone)
        for (int i = threadIdx.x; i < (hw >> 2); i += 256) dst[i] = src[i];
    }
    __syncthreads();
    const double ax = pa.x, ay = pa.y, za = pb.x, bx = pb.y, by = pc.x, zb = pc.y;
    const double2* urow = s_u + d * N - 1;  // waypoint j's unit vector: urow[j]
    // PROF: waypoint j's coefficients, zrow[3 j ..]
    [[maybe_unused]] const double* zrow = s_jw + a * W * 3;
    const int j0 = s * kg.G, j1 = live ? min(j0 + kg.G, W) : j0;
    int nch = (j1 - j0 + CH - 1) / CH;  // the wave's most: a wave-uniform loop
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) nch = max(nch, __shfl_xor(nch, o));
    const double vx = ax - bx, vy = ay - by;
    const double cx = (bx + ax) * 0.5, cy = (by + ay) * 0.5;
    const double dN = (double)N, yN = kg.inv_n;
    auto over_n = [&](double v) {  // (K4h: N <= 4096)
        const double q0 = v * yN;
        const double q1 = fma(fma(-q0, dN, v), yN, q0);
        return __builtin_isinf(v) ? q0 : q1;
    };
    // the layer centre of layer iz (the below-terrain test)
    auto zc_of = [&](int32_t iz) { return vs.z0 + ((double)iz + 0.5) * vs.dz; };
    // the end points' voxels, formed once
    int32_t ixF, iyF, izF, ixL, iyL, izL;
    double zF, zL;
    if constexpr (PROF) zF = vp_z(zrow, 0, za, zb), zL = vp_z(zrow, W - 1, za, zb);
    else zF = vz_at(za, zb, s_jw[0]), zL = vz_at(za, zb, s_jw[W - 1]);
    const bool inF = vol_voxel(vs, ax, ay, zF, ixF, iyF, izF);
    const bool inL = vol_voxel(vs, bx, by, zL, ixL, iyL, izL);
    const uint16_t* const bnd = reinterpret_cast<const uint16_t*>(s_hdr + vs.bnd_off);
    const float2* const sbt = reinterpret_cast<const float2*>(s_hdr + vs.sbt_off);
    const char* const pk = vs.pk;
    const uint32_t o4 = __builtin_amdgcn_readfirstlane(vs.o4);
    const uint32_t o8 = __builtin_amdgcn_readfirstlane(vs.o8);
    const uint32_t o16 = __builtin_amdgcn_readfirstlane(vs.o16);
    const uint32_t ot4 = __builtin_amdgcn_readfirstlane(vs.ot4);
    const uint32_t layer = __builtin_amdgcn_readfirstlane(vs.layer);
    const uint32_t oq8 = __builtin_amdgcn_readfirstlane(vs.oq8);
    const uint32_t layer44 = __builtin_amdgcn_readfirstlane(vs.layer44);
    const uint32_t layer42 = __builtin_amdgcn_readfirstlane(vs.layer42);
    double gc = 0.0, gn = 0.0, E = seed;
    uint32_t nh = 0, off = 0, bel = 0;
    X128 xc = {0, 0}, xn = {0, 0};  // EX: the group's risk and psi terms
    uint32_t xf = 0;                // EX: their side flags (risk | psi << 3)
    // EX: the volume's exponents, read once per workgroup at a uniform address
    int32_t e_risk = 0, e_psi = 0;
    if constexpr (EX) {
        e_risk = __builtin_amdgcn_readfirstlane(vs.xscale[0]);
        e_psi = __builtin_amdgcn_readfirstlane(vs.xscale[1]);
    }
    // EX: one word into its field's sum (straight-line, as h_item's)
    auto x_take = [&](X128& acc, uint32_t w, int32_t e, int fs) {
        acc = x_add(acc, x_term(w, e));
        xf |= x_word_flags(w) << fs;
    };
    // one chunk ahead, as h_item: iteration c issues chunk c + 1 (B arrays) and consumes chunk
    // c (A arrays)
    // (the slot's layer rides in its kind word's high bits; consume recomputes its altitude)
    uint4 rA[CH];
    float tvA[CH];
    uint32_t kcA[CH], vinA = 0, tkA = 0, bvA = 0;
    int nvA = 0, jcA = 0;
    constexpr bool ahead = false;  // (h_item's)
    static_assert(!PROF || !ahead, "the kept zB is the chunk the same iteration consumes");
    for (int c = ahead ? -1 : 0; c < nch; ++c) {  // (nch wave-uniform)
        const int ci = ahead ? c + 1 : c;  // the chunk issued by this iteration
        uint4 rB[CH];
        float tvB[CH];
        uint32_t kcB[CH], vinB = 0, tkB = 0, bvB = 0;
        int nvB = 0;
        double zB[CH];  // the slots' altitudes (PROF: kept for the consume loop)
        const int jc = j0 + ci * CH;
        if (ci < nch) {
            int32_t izB[CH];
            const double2* uc = urow + jc;
            // phase 1: the voxels
            int32_t ix[CH], iy[CH];
#pragma unroll
            for (int t = 0; t < CH; ++t) {
                const int j = jc + t;
                const double2 u = uc[t];
                double z;
                if constexpr (PROF) z = vp_z(zrow, j, za, zb);
                else z = vz_at(za, zb, s_jw[j]);
                int32_t x, y, zz;
                bool in = vol_voxel(vs, cx + 0.5 * (vx * u.x - vy * u.y),
                                    cy + 0.5 * (vy * u.x + vx * u.y), z, x, y, zz);
                if (t == 0) {  // (j == 0 only in a chunk's first slot)
                    const bool f = jc == 0;
                    x = f ? ixF : x;
                    y = f ? iyF : y;
                    zz = f ? izF : zz;
                    in = f ? inF : in;
                }
                const bool l = j == W - 1;
                ix[t] = l ? ixL : x;
                iy[t] = l ? iyL : y;
                izB[t] = l ? izL : zz;
                in = l ? inL : in;
                zB[t] = z;  // (the end points' z by the same formula)
                vinB |= (uint32_t)(in & (j < j1)) << t;
            }
            // phase 2: the header reads (column (0, 0) outside the volume: valid reads)
            uint32_t cw[CH], be[CH];
            float2 sb[CH];
#pragma unroll
            for (int t = 0; t < CH; ++t) {
                const uint32_t b = __umul24((uint32_t)(iy[t] >> VPK_CSHIFT), (uint32_t)vs.cnbx) +
                                   (uint32_t)(ix[t] >> VPK_CSHIFT);
                cw[t] = s_hdr[b >> 4] >> ((b & 15u) * 2u);
                if constexpr (!TE) {
                    const uint32_t bx2 = (uint32_t)(ix[t] >> vs.bshift);
                    const uint32_t by2 = (uint32_t)(iy[t] >> vs.bshift);
                    be[t] = bnd[__umul24(by2, (uint32_t)vs.bnbx) + bx2];
                    sb[t] = sbt[__umul24(by2 >> 2, (uint32_t)vs.sbnbx) + (bx2 >> 2)];
                }
            }
            // phase 3: the decisions and the loads
#pragma unroll
            for (int t = 0; t < CH; ++t) {
                const bool vin = (vinB >> t) & 1u;
                const uint32_t code = cw[t] & (vin ? 3u : 0u);
                if constexpr (TE) {
                    // codes 0 / 1: the 8-B {risk, column terrain} entry (q8); 2 / 3: v16
                    const bool rec = code & 2u;
                    const uint32_t iz = (uint32_t)izB[t];
                    const uint32_t a16 = vv16_index(vs, ix[t], iy[t]) + __umul24(iz, layer42);
                    const uint32_t ab = (vq8_index(vs, ix[t], iy[t]) + __umul24(iz, layer44)) << 3;
                    const uint32_t voff = rec ? o16 + (a16 << 4) : oq8 + (ab & ~15u);
                    kcB[t] = code | (rec ? 0u : (ab & 8u)) | (iz << 8);
                    rB[t] = *reinterpret_cast<const uint4*>(pk + voff);
                    continue;
                }
                float ub, lb;
                pk_bound_decode(be[t], sb[t], ub, lb);
                const double z = zB[t], zc = zc_of(izB[t]);
                const bool k1 = zc < (double)lb, k0 = zc >= (double)ub;
                // a one-value block: the exact term; every in-volume waypoint's z - lb bounds M
                E = (vin & (lb == ub)) ? fmin(E, z - (double)ub) : E;
                Ub = vin ? fmin(Ub, z - (double)lb) : Ub;
                const double clo = z - (double)ub;
                const bool fetch =
                    vin & (code != 3u) & (!(k1 | k0) | (!(clo >= E) & !(clo > Ub)));
                const uint32_t it = vt4_index(vs, ix[t], iy[t]);
                const uint32_t a4 = it + __umul24((uint32_t)izB[t], layer);
                // codes 1 / 2: the r4 / e8 entry's aligned 16 B and word; 3: v16 (its own index)
                const uint32_t ab = a4 << (code + 1u);
                const uint32_t a16 = vv16_index(vs, ix[t], iy[t]) + __umul24((uint32_t)izB[t], layer42);
                const uint32_t voff = code == 3u ? o16 + (a16 << 4)
                                                 : (code == 2u ? o8 : o4) + (code ? (ab & ~15u) : 0u);
                kcB[t] = code | (code == 3u ? 0u : (ab & 12u)) | ((uint32_t)izB[t] << 8);
                rB[t] = *reinterpret_cast<const uint4*>(pk + voff);
                tvB[t] = *reinterpret_cast<const float*>(pk + (ot4 + (fetch ? it * 4u : 0u)));
                tkB |= (uint32_t)fetch << t;
                bvB |= (uint32_t)k1 << t;
            }
            nvB = max(0, min(CH, j1 - jc));  // slots past the group's end: no waypoint
        }
        if (!ahead) {
#pragma unroll
            for (int t = 0; t < CH; ++t) rA[t] = rB[t], tvA[t] = tvB[t], kcA[t] = kcB[t];
            vinA = vinB, tkA = tkB, bvA = bvB, nvA = nvB, jcA = jc;
        }
        if (c >= 0) {
#pragma unroll
            for (int t = 0; t < CH; ++t) {
                const bool vl = t < nvA, in = (vinA >> t) & 1u;
                if constexpr (TE) {
                    const uint4 r = rA[t];
                    const bool rec = kcA[t] & 2u, s1 = kcA[t] & 8u;
                    const uint32_t lo = s1 ? r.z : r.x, hi = s1 ? r.w : r.y;
                    const uint32_t risk = in ? (rec ? r.x : lo) : 0u;
                    const float ter = __uint_as_float(rec ? r.z : hi);  // (+0 on nodata)
                    nh += (rec && (r.w & UAM_FLAG_NFZ)) ? 1u : 0u;
                    off += (vl && !in) ? 1u : 0u;
                    if constexpr (EX) {
                        x_take(xc, risk, e_risk, 0);
                        x_take(xn, rec ? r.y : 0u, e_psi, 3);
                    } else {
                        gc = gc + over_n((double)__uint_as_float(risk));
                        gn = gn + (rec ? (double)__uint_as_float(r.y) : 0.0);
                    }
                    double z;
                    if constexpr (PROF) z = zB[t];
                    else z = vz_at(za, zb, s_jw[jcA + t]);
                    bel += (in && zc_of((int32_t)(kcA[t] >> 8)) < (double)ter) ? 1u : 0u;
                    E = in ? fmin(E, z - (double)ter) : E;
                    continue;
                }
                uint32_t risk, psi, hit;
                float rter;
                pk_terms_k(rA[t], kcA[t], risk, psi, hit, rter);
                const bool c3 = (kcA[t] & 3u) == 3u;
                if constexpr (EX) {
                    x_take(xc, risk, e_risk, 0);
                    x_take(xn, psi, e_psi, 3);
                } else {
                    gc = gc + over_n((double)__uint_as_float(risk));
                    gn = gn + (double)__uint_as_float(psi);
                }
                nh += hit;
                off += (vl && !in) ? 1u : 0u;
                // the exact terrain, where taken: v16's (code 3) or the fetched one
                const bool ex = in & (c3 | ((tkA >> t) & 1u));
                const float ter = c3 ? rter : tvA[t];
                double z;
                if constexpr (PROF) z = zB[t];
                else z = vz_at(za, zb, s_jw[jcA + t]);
                const uint32_t below =
                    ex ? (zc_of((int32_t)(kcA[t] >> 8)) < (double)ter ? 1u : 0u) : ((bvA >> t) & 1u);
                bel += in ? below : 0u;
                E = ex ? fmin(E, z - (double)ter) : E;
            }
        }
        if (ahead) {
#pragma unroll
            for (int t = 0; t < CH; ++t) rA[t] = rB[t], tvA[t] = tvB[t], kcA[t] = kcB[t];
            vinA = vinB, tkA = tkB, bvA = bvB, nvA = nvB, jcA = jc;
        }
    }
    if constexpr (EX) {
        VSlotX o;
        o.c_lo = xc.lo, o.c_hi = xc.hi;
        o.n_lo = xn.lo, o.n_hi = xn.hi;
        o.cm = E;
        o.cnt = nh | (off << 8) | (bel << 16) | (xf << 24);
        o.pad = 0;
        if (live) reinterpret_cast<VSlotX*>(kg.slot)[(int64_t)s * kg.P + path] = o;
        return;
    }
    VSlot o;
    o.cost = gc;
    o.psi = gn;
    o.cm = E;
    o.cnt = nh | (off << 8) | (bel << 16);
    o.pad = 0;
    if (live) reinterpret_cast<VSlot*>(kg.slot)[(int64_t)s * kg.P + path] = o;
}
// the exact form (UAM_OPT_EXACT_SUM_VOLUME), k_v_eval's sibling: the same body with EX set
template <int CH, bool TE>
constexpr auto k_v_eval_x = k_v_eval<CH, TE, true>;
// K4hp's instances (the host tables' names)
template <int CH, bool TE, bool EX = false>
constexpr auto k_vp_eval = k_v_eval<CH, TE, EX, KProf>;
template <int CH, bool TE>
constexpr auto k_vp_eval_x = k_v_eval<CH, TE, true, KProf>;

// path gp's slots in group order (the K4h, K4hp and K4hp+v output launches): the risk / N
// partials onto cost (the caller's (N+1) L), nfz_sum, the minimum clearance and the three counts
// EX (UAM_OPT_EXACT_SUM_VOLUME): the VSlotX sums added as integers and their flags ORed, each
// field rounded once (x_result, a true division): cost = (N+1) L + fl(S_risk) / N, nfz_sum =
// fl(S_psi)
template <bool EX>
__device__ __forceinline__ void v_path_slots(const KGrp& kg, int64_t gp, int N, int32_t e_risk,
                                             int32_t e_psi, double& cost, double& nsum,
                                             double& cm, int32_t& nh, int32_t& off,
                                             int32_t& bel) {
    using Slot = std::conditional_t<EX, VSlotX, VSlot>;
    const Slot* slot = reinterpret_cast<const Slot*>(kg.slot);
    nsum = 0.0, cm = INFINITY;
    nh = off = bel = 0;
    X128 xc = {0, 0}, xn = {0, 0};
    uint32_t xfl = 0;
    for (int s = 0; s < kg.nseg; ++s) {
        const Slot g = slot[(int64_t)s * kg.P + gp];
        if constexpr (EX) {
            xc = x_add(xc, X128{g.c_lo, g.c_hi});
            xn = x_add(xn, X128{g.n_lo, g.n_hi});
            xfl |= g.cnt >> 24;
        } else {
            cost = cost + g.cost;
            nsum = nsum + g.psi;
        }
        cm = fmin(cm, g.cm);
        nh += (int32_t)(g.cnt & 255u);
        off += (int32_t)((g.cnt >> 8) & 255u);
        bel += (int32_t)((g.cnt >> 16) & 255u);
    }
    if constexpr (EX) {
        cost = cost + x_result(xc, xfl & 7u, e_risk) / (double)N;
        nsum = x_result(xn, (xfl >> 3) & 7u, e_psi);
    }
}

// outputs of every path (block = 64 pairs x D): the similarity-form geometry (sim_geo on the
// pair's x/y), cost = (N+1) L + the slots' partials (v_path_slots), min clearance, the counts,
// and the main.py:175-180 selection
template <bool EX>
__device__ __forceinline__ void v_final_wg(KParams p, KGrp kg, KOut out,
                                           int32_t* __restrict__ best_f,
                                           int32_t* __restrict__ best_l, int32_t e_risk,
                                           int32_t e_psi) {
    extern __shared__ __attribute__((aligned(16))) double smem[];
    const int D = kg.D, t = threadIdx.x;
    double* s_cost = smem;
    double* s_len = smem + 64 * D;
    const int64_t q0 = (int64_t)blockIdx.x * 64;
    const int qi = t / D, di = t - qi * D;
    const bool bad = *kg.err != 0;  // an inconsistent sort (k_g_scatter / k_v_hist)
    if (q0 + qi < kg.n_pairs) {
        const int64_t gp = (q0 + qi) * D + di;
        const double* pr = kg.pairs + (q0 + qi) * 6;
        double L, len, ksum;
        sim_geo(p, kg.ugeo[di], pr[0], pr[1], pr[3], pr[4], L, len, ksum);
        double cost = (double)(p.N + 1) * L, nsum, cm;
        int32_t nh, off, bel;
        v_path_slots<EX>(kg, gp, p.N, e_risk, e_psi, cost, nsum, cm, nh, off, bel);
        put_outputs(out, gp, bad, cost, L, len, ksum, nsum, cm, nh, off, bel);
        s_cost[di * 64 + qi] = cost;
        s_len[di * 64 + qi] = len;
    }
    __syncthreads();
    put_selection(kg, bad, q0, t, s_cost, s_len, best_f, best_l);
}
__global__ __launch_bounds__(1024) void k_v_final(KParams p, KGrp kg, KOut out,
                                                  int32_t* __restrict__ best_f,
                                                  int32_t* __restrict__ best_l) {
    v_final_wg<false>(p, kg, out, best_f, best_l, 0, 0);
}
__global__ __launch_bounds__(1024) void k_v_final_x(KParams p, KGrp kg, KOut out,
                                                    int32_t* __restrict__ best_f,
                                                    int32_t* __restrict__ best_l,
                                                    const int32_t* __restrict__ scale) {
    const int32_t e_risk = __builtin_amdgcn_readfirstlane(scale[0]);
    const int32_t e_psi = __builtin_amdgcn_readfirstlane(scale[1]);
    v_final_wg<true>(p, kg, out, best_f, best_l, e_risk, e_psi);
}
