// k4hp.inc -- K4hp, the altitude-profile candidates on the packed, sorted volume: KProf,
// vp_z, vp_path_seed, k_vp_hist, k_vp_eval (k_vp_eval_x: its exact form), k_vp_final /
// k_vp_final_x, k_vp_final_v / k_vp_final_xv (K4hp+v: the output launch under the vertical
// terms), k_vp_sel_check.
// Included in the anonymous namespace of uampath.hip after k4h.inc; relies on its text (VSlot /
// VSlotX, KVol4, vol_voxel, the plane indices) and on what k4h.inc relies on; K4hp+v also on
// KVert, VertAcc, vert_begin and vert_segment (uampath.hip, K4e+v / K4p+v).

// ---- K4hp: uam_eval_generated3d_profiles_h ---------------------------------------------------
// K4h with the altitude of waypoint j taken from the profile table instead of the straight
// climb.  The profile rides inside the path index, p = (q D + d) A + a, so KGrp describes P =
// Q D A paths with kg.D the lateral candidates (the unit-arc rows and k_g_scatter's UGeo rows
// are per d) and every shared launch (the scan, k_g_scatter) runs unchanged.  KGrp itself stays
// as it is -- it is a kernel argument of K2g / K2h / K4h -- and what the profile form adds
// travels in KProf.  The items' key is (altitude band, tile) of the middle waypoint at the
// profile's own z, so the profiles of a lateral candidate that fly at different heights fall
// into different bands.  Definition: include/uampath.h.

struct KProf {
    const double* __restrict__ ztab;  // [A][W][3]
    int32_t A;
    int32_t sh_a;
    uint64_t m_a;  // div_magic's multiplier and shift for / A
};

constexpr int VPK_ZTAB_LDS = 40 * 1024;  // the profile rows in LDS up to this

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

// v_path_seed with the profile's z per sampled waypoint (zrow: the profile's row of the table
// in global memory)
__device__ __forceinline__ double vp_path_seed(const KParams& p, const KVol4& vs, const KGrp& kg,
                                              const KProf& kf, int32_t path,
                                              const uint32_t* __restrict__ hdr,
                                              const double2* __restrict__ utab) {
    int32_t q, d, a;
    vp_split(kg, kf, path, q, d, a);
    const double* pr = kg.pairs + (int64_t)q * 6;
    const double ax = pr[0], ay = pr[1], za = pr[2], bx = pr[3], by = pr[4], zb = pr[5];
    const double2* u = utab + d * p.N - 1;
    const int W = kg.W;
    const double* zrow = kf.ztab + (int64_t)a * W * 3;
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
    take(ax, ay, vp_z(zrow, 0, za, zb));
    take(bx, by, vp_z(zrow, W - 1, za, zb));
    constexpr int K = 4;
    for (int j0 = kg.lb_stride; j0 < W - 1; j0 += K * kg.lb_stride) {
        double2 uu[K];
        double zz[K];
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const int jj = min(j0 + k * kg.lb_stride, W - 2);
            uu[k] = u[jj];
            zz[k] = vp_z(zrow, jj, za, zb);
        }
#pragma unroll
        for (int k = 0; k < K; ++k) {
            double x0, x1;
            arc_point(ax, ay, bx, by, uu[k].x, uu[k].y, x0, x1);
            take(x0, x1, zz[k]);
        }
    }
    return best == NONE ? INFINITY
                        : zbest - (double)reinterpret_cast<const float*>(vs.pk + vs.ot4)[best];
}

// sort, launch 1 (K4hp): k_v_hist with z from the table
__global__ __launch_bounds__(1024) void k_vp_hist(KParams p, KVol4 vs, KGrp kg, KProf kf) {
    __shared__ __attribute__((aligned(16))) int32_t h[G_BINS_MAX];
    __shared__ uint16_t tk[1 << (2 * G_TBITS_MAX)];
    // with kg.seed_lds: the packed header and the unit-arc table staged for the seeds
    extern __shared__ __attribute__((aligned(16))) uint32_t s_vphist_dyn[];
    const int t = threadIdx.x, b = blockIdx.x;
    if (b == 0 && t == 0) *kg.err = 0;
    for (int k = t; k < kg.bins; k += 1024) h[k] = 0;
    for (int k = t; k < (1 << (2 * kg.tbits)); k += 1024) tk[k] = kg.tkey[k];
    const uint32_t* s_hdr = vs.hdr;
    const double2* s_ut = reinterpret_cast<const double2*>(kg.utab);
    if (kg.ubp && kg.seed_lds) {
        uint4* dh = reinterpret_cast<uint4*>(s_vphist_dyn);
        const uint4* gh = reinterpret_cast<const uint4*>(vs.hdr);
        for (int k = t; k < (vs.hwords >> 2); k += 1024) dh[k] = gh[k];
        double2* du = reinterpret_cast<double2*>(s_vphist_dyn + vs.hwords);
        for (int k = t; k < kg.D * p.N; k += 1024) du[k] = s_ut[k];
        s_hdr = s_vphist_dyn;
        s_ut = du;
    }
    __syncthreads();
    const int64_t lo = ((int64_t)kg.P * b / G_NBK) * kg.nseg;
    const int64_t hi = ((int64_t)kg.P * (b + 1) / G_NBK) * kg.nseg;
    const int N = p.N, W = kg.W;
    const int tiles = 1 << (2 * kg.tbits);
    constexpr int U = 4;
    for (int64_t i0 = lo + t; i0 < hi; i0 += 1024 * U) {
        double pr[U][6], zc[U][3];
        double2 u[U];
        int jm[U];
#pragma unroll
        for (int k = 0; k < U; ++k) {
            const int32_t i = (int32_t)min(i0 + k * 1024, hi - 1);
            const int32_t path = (int32_t)div_magic((uint32_t)i, kg.m_nseg, kg.sh_nseg);
            const int sg = (int)(i - (int64_t)path * kg.nseg);
            int32_t q, d, a;
            vp_split(kg, kf, path, q, d, a);
            const int j0 = sg * kg.G, j1 = min(j0 + kg.G, W);
            jm[k] = (j0 + j1 - 1) >> 1;
            const double2* pp = reinterpret_cast<const double2*>(kg.pairs + (int64_t)q * 6);
            const double2 a2 = pp[0], b2 = pp[1], c = pp[2];
            pr[k][0] = a2.x, pr[k][1] = a2.y, pr[k][2] = b2.x, pr[k][3] = b2.y, pr[k][4] = c.x,
            pr[k][5] = c.y;
            u[k] = reinterpret_cast<const double2*>(kg.utab)[d * N + min(max(jm[k] - 1, 0), N - 1)];
            const double* zr = kf.ztab + ((int64_t)a * W + jm[k]) * 3;
            zc[k][0] = zr[0], zc[k][1] = zr[1], zc[k][2] = zr[2];
        }
#pragma unroll
        for (int k = 0; k < U; ++k) {
            const int64_t i = i0 + k * 1024;
            if (i >= hi) break;
            double x0, x1;
            if (jm[k] == 0) {
                x0 = pr[k][0], x1 = pr[k][1];
            } else if (jm[k] == W - 1) {
                x0 = pr[k][3], x1 = pr[k][4];
            } else {
                arc_point(pr[k][0], pr[k][1], pr[k][3], pr[k][4], u[k].x, u[k].y, x0, x1);
            }
            const double z = (pr[k][2] * zc[k][0] + pr[k][5] * zc[k][1]) + zc[k][2];
            const double tx = (x0 - vs.x0) * vs.inv_dx, ty = (vs.y_top - x1) * vs.inv_dy;
            const double tz = (z - vs.z0) * vs.inv_dz;
            uint32_t key = kg.bins - 1;
            if ((tx >= 0.0) && (tx < (double)vs.nx) && (ty >= 0.0) && (ty < (double)vs.ny) &&
                (tz >= 0.0) && (tz < (double)vs.nz)) {
                const uint32_t cx = (uint32_t)tx >> kg.tshift, cy = (uint32_t)ty >> kg.tshift;
                // (kg.last_bin is 0: one bin per tile and band, as K4h's)
                key = ((uint32_t)tz >> vs.zshift) * tiles + tk[(cy << kg.tbits) | cx];
            }
            kg.key[i] = (uint16_t)key;
            atomicAdd(&h[key], 1);
        }
    }
    if (kg.ubp) {  // the partition's paths' clearance seeds, one thread per path
        const int64_t plo = (int64_t)kg.P * b / G_NBK, phi = (int64_t)kg.P * (b + 1) / G_NBK;
        for (int64_t pth = plo + t; pth < phi; pth += 1024)
            kg.ubp[pth] = vp_path_seed(p, vs, kg, kf, (int32_t)pth, s_hdr, s_ut);
    }
    __syncthreads();
    for (int k = t; k < kg.bins; k += 1024) kg.cnt[(int64_t)k * G_NBK + b] = h[k];
}

// k_v_eval with the profile rows staged in LDS beside the arc rows (24 A W bytes + padding, in
// place of k_v_eval's j / (W-1) table): a lane's row is s_zt + 3 a W, and waypoint j's altitude
// is the table rule on it (vp_z), formed once in phase 1 and kept for the consume loop (k_v_eval
// forms vz_at a second time there from one LDS word; three words per slot read again cost 24
// VGPRs at CH = 7 and spilled at CH = 6, 8 and 16 -- DESIGN §10.1).  A slot past the group's end
// reads the next row or the padding (zeros): its voxel is masked, and whatever its z, vol_voxel
// gives indices inside the volume.  The phases, the terrain forms and the
// exact form are k_v_eval's; a body of its own, so k_v_eval's instances keep their registers
// (DESIGN §10.1).
template <int CH, bool TE, bool EX = false>
__global__ __launch_bounds__(256, CH >= 11 ? 2 : CH >= 7 ? 3 : 4) void k_vp_eval(KParams p, KVol4 vs,
                                                                               KGrp kg, KProf kf) {
    PK_CODES_CHECK(CH);
    // unit-arc rows + padding, then the profile rows (+ padding), then the header
    extern __shared__ __attribute__((aligned(16))) double2 s_u[];
    const int N = p.N, W = kg.W;
    const int nu = kg.D * N, npad = kg.G + 16;  // a lane's slots reach j <= W + G + CH - 3
    double* s_zt = reinterpret_cast<double*>(s_u + nu + npad);
    const int nzt = (kf.A * W + npad) * 3;
    uint32_t* s_hdr = reinterpret_cast<uint32_t*>(s_zt + ((nzt + 1) & ~1));
    const int64_t pos = xcd_chunk(blockIdx.x, gridDim.x) * 256 + threadIdx.x;
    const bool live = pos < kg.n_items;
    const int32_t item = live ? kg.order[pos] : 0;
    const int32_t path = (int32_t)div_magic((uint32_t)item, kg.m_nseg, kg.sh_nseg);
    const int s = item - path * kg.nseg;
    int32_t q, d, a;
    vp_split(kg, kf, path, q, d, a);
    const double* prp = kg.pairs + (int64_t)q * 6;
    const double2 pa = *reinterpret_cast<const double2*>(prp);
    const double2 pb = *reinterpret_cast<const double2*>(prp + 2);
    const double2 pc = *reinterpret_cast<const double2*>(prp + 4);
    const double seed = kg.ubp ? kg.ubp[path] : INFINITY;  // an exact clearance of the path
    double Ub = seed;
    for (int i = threadIdx.x; i < nu + npad; i += 256)
        s_u[i] = i < nu ? reinterpret_cast<const double2*>(kg.utab)[i] : make_double2(0.0, 0.0);
    {
        const int nz3 = kf.A * W * 3;
        for (int i = threadIdx.x; i < nzt; i += 256) s_zt[i] = i < nz3 ? kf.ztab[i] : 0.0;
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
    const double* zrow = s_zt + a * W * 3;  // waypoint j's coefficients: zrow[3 j ..]
    const int j0 = s * kg.G, j1 = live ? min(j0 + kg.G, W) : j0;
    int nch = (j1 - j0 + CH - 1) / CH;  // the wave's most: a wave-uniform loop
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) nch = max(nch, __shfl_xor(nch, o));
    const double vx = ax - bx, vy = ay - by;
    const double cx = (bx + ax) * 0.5, cy = (by + ay) * 0.5;
    const double dN = (double)N, yN = kg.inv_n;
    auto over_n = [&](double v) {  // (N <= 4096)
        const double q0 = v * yN;
        const double q1 = fma(fma(-q0, dN, v), yN, q0);
        return __builtin_isinf(v) ? q0 : q1;
    };
    auto zc_of = [&](int32_t iz) { return vs.z0 + ((double)iz + 0.5) * vs.dz; };
    // the end points' voxels, formed once
    int32_t ixF, iyF, izF, ixL, iyL, izL;
    const bool inF = vol_voxel(vs, ax, ay, vp_z(zrow, 0, za, zb), ixF, iyF, izF);
    const bool inL = vol_voxel(vs, bx, by, vp_z(zrow, W - 1, za, zb), ixL, iyL, izL);
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
    int32_t e_risk = 0, e_psi = 0;
    if constexpr (EX) {
        e_risk = __builtin_amdgcn_readfirstlane(vs.xscale[0]);
        e_psi = __builtin_amdgcn_readfirstlane(vs.xscale[1]);
    }
    auto x_take = [&](X128& acc, uint32_t w, int32_t e, int fs) {
        acc = x_add(acc, x_term(w, e));
        xf |= x_word_flags(w) << fs;
    };
    for (int c = 0; c < nch; ++c) {  // (nch wave-uniform)
        uint4 rB[CH];
        float tvB[CH];
        uint32_t kcB[CH], vinB = 0, tkB = 0, bvB = 0;
        const int jc = j0 + c * CH;
        double zB[CH];  // the slots' altitudes, kept for the consume loop
        {
            int32_t izB[CH];
            const double2* uc = urow + jc;
            // phase 1: the voxels
            int32_t ix[CH], iy[CH];
#pragma unroll
            for (int t = 0; t < CH; ++t) {
                const int j = jc + t;
                const double2 u = uc[t];
                const double z = vp_z(zrow, j, za, zb);
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
                zB[t] = z;
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
                E = (vin & (lb == ub)) ? fmin(E, z - (double)ub) : E;
                Ub = vin ? fmin(Ub, z - (double)lb) : Ub;
                const double clo = z - (double)ub;
                const bool fetch =
                    vin & (code != 3u) & (!(k1 | k0) | (!(clo >= E) & !(clo > Ub)));
                const uint32_t it = vt4_index(vs, ix[t], iy[t]);
                const uint32_t a4 = it + __umul24((uint32_t)izB[t], layer);
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
        }
        const int nv = max(0, min(CH, j1 - jc));  // slots past the group's end: no waypoint
#pragma unroll
        for (int t = 0; t < CH; ++t) {
            const bool vl = t < nv, in = (vinB >> t) & 1u;
            if constexpr (TE) {
                const uint4 r = rB[t];
                const bool rec = kcB[t] & 2u, s1 = kcB[t] & 8u;
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
                const double z = zB[t];
                bel += (in && zc_of((int32_t)(kcB[t] >> 8)) < (double)ter) ? 1u : 0u;
                E = in ? fmin(E, z - (double)ter) : E;
                continue;
            }
            uint32_t risk, psi, hit;
            float rter;
            pk_terms_k(rB[t], kcB[t], risk, psi, hit, rter);
            const bool c3 = (kcB[t] & 3u) == 3u;
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
            const bool ex = in & (c3 | ((tkB >> t) & 1u));
            const float ter = c3 ? rter : tvB[t];
            const double z = zB[t];
            const uint32_t below =
                ex ? (zc_of((int32_t)(kcB[t] >> 8)) < (double)ter ? 1u : 0u) : ((bvB >> t) & 1u);
            bel += in ? below : 0u;
            E = ex ? fmin(E, z - (double)ter) : E;
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
template <int CH, bool TE>
constexpr auto k_vp_eval_x = k_vp_eval<CH, TE, true>;

// outputs of every path, one thread per path (v_final_wg's 64 x D block does not reach D A =
// 128): the similarity-form geometry of the path's (q, d) -- the same for its A profiles -- and
// the partials in group order, as v_final_wg; the selections follow in k_argmin over D A
template <bool EX>
__device__ __forceinline__ void vp_final_path(const KParams& p, const KGrp& kg, const KProf& kf,
                                              const KOut& out, int32_t e_risk, int32_t e_psi) {
    using Slot = std::conditional_t<EX, VSlotX, VSlot>;
    const int64_t gp = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const bool bad = *kg.err != 0;  // an inconsistent sort (k_g_scatter / k_vp_hist)
    if (bad && gp == 0 && kg.herr) *kg.herr = 1;
    if (gp >= kg.P) return;
    int32_t q, di, a;
    vp_split(kg, kf, (int32_t)gp, q, di, a);
    const Slot* slot = reinterpret_cast<const Slot*>(kg.slot);
    const double* pr = kg.pairs + (int64_t)q * 6;
    const double x0 = pr[0], y0 = pr[1], xf = pr[3], yf = pr[4];
    const UGeo u = kg.ugeo[di];
    const double vx = x0 - xf, vy = y0 - yf;
    const double sv = vx * vx + vy * vy;
    const double h = sqrt(sv) * 0.5, h2 = sv * 0.25;
    const bool ls = p.length_smooth != 0;
    double L;
    if (p.quirk_length) {
        const double axx = p.anchor_mode ? p.anchor_x : x0;
        const double ayy = p.anchor_mode ? p.anchor_y : y0;
        const double dx = x0 - axx, dy = y0 - ayy;
        const double n = sqrt(dx * dx + dy * dy);
        L = (ls ? n * n : n) + (ls ? h2 * u.s2n : h * u.s1n);
    } else {
        L = ls ? h2 * u.s2a : h * u.s1a;
    }
    const double len = h * u.s1a;
    const double ksum = (h > 0.0 && h < INFINITY) ? h * u.e12 + u.e3 : 0.0;
    double cost = (double)(p.N + 1) * L, nsum = 0.0, cm = INFINITY;
    int32_t nh = 0, off = 0, bel = 0;
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
    if constexpr (EX) {  // one rounding per field, a true division
        cost = cost + x_result(xc, xfl & 7u, e_risk) / (double)p.N;
        nsum = x_result(xn, (xfl >> 3) & 7u, e_psi);
    }
    put_outputs(out, gp, bad, cost, L, len, ksum, nsum, cm, nh, off, bel);
}
__global__ __launch_bounds__(256) void k_vp_final(KParams p, KGrp kg, KProf kf, KOut out) {
    vp_final_path<false>(p, kg, kf, out, 0, 0);
}
__global__ __launch_bounds__(256) void k_vp_final_x(KParams p, KGrp kg, KProf kf, KOut out,
                                                    const int32_t* __restrict__ scale) {
    const int32_t e_risk = __builtin_amdgcn_readfirstlane(scale[0]);
    const int32_t e_psi = __builtin_amdgcn_readfirstlane(scale[1]);
    vp_final_path<true>(p, kg, kf, out, e_risk, e_psi);
}

// ---- K4hp+v: uam_eval_generated3d_profiles_hv -------------------------------------------------
// The output launch under the vertical terms (KVert, uam_vertical): dz enters the segment norm,
// so the geometry is no similarity form of the pair's chord and differs among the A profiles of
// a lateral candidate.  One thread per path walks its W points once -- x/y by k_vp_eval phase
// 1's operations (arc_point's with the pair's terms hoisted), z by vp_z, or PathSrc::alt's
// straight climb with no table (kf.ztab null, A = 1: the slots are then K4h's own k_v_eval's)
// -- through vert_begin / vert_segment, K4p+v's pass 1, so length_q, length, kin_sum and
// climb_sum are K4p+v's bits; then the slots in group order (EX: as integers) from (N+1) L, as
// vp_final_path.  The arc and profile rows are read through the cache: a wave's lanes are A
// profiles of consecutive lateral candidates, so they share a few rows of each table.
template <bool EX>
__device__ __forceinline__ void vp_final_v_path(const KParams& p, const KGrp& kg, const KProf& kf,
                                                const KVert& v, const KOut& out, int32_t e_risk,
                                                int32_t e_psi) {
    using Slot = std::conditional_t<EX, VSlotX, VSlot>;
    const int64_t gp = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const bool bad = *kg.err != 0;  // an inconsistent sort (k_g_scatter / k_vp_hist / k_v_hist)
    if (bad && gp == 0 && kg.herr) *kg.herr = 1;
    if (gp >= kg.P) return;
    int32_t q, di, a;
    vp_split(kg, kf, (int32_t)gp, q, di, a);
    const int N = p.N, W = kg.W;
    const double* pr = kg.pairs + (int64_t)q * 6;
    const double ax = pr[0], ay = pr[1], za = pr[2], bx = pr[3], by = pr[4], zb = pr[5];
    const double2* urow = reinterpret_cast<const double2*>(kg.utab) + di * N - 1;  // urow[j]
    const double* zrow = kf.ztab ? kf.ztab + (int64_t)a * W * 3 : nullptr;
    auto alt = [&](int j) {
        return zrow ? vp_z(zrow, j, za, zb) : za + (zb - za) * ((double)j / (double)(W - 1));
    };
    const double vx = ax - bx, vy = ay - by;
    const double cx = (bx + ax) * 0.5, cy = (by + ay) * 0.5;
    VertAcc g;
    vert_begin(p, ax, ay, g);
    double px = ax, py = ay, pz = alt(0), pdx = 0.0, pdy = 0.0;
    for (int j = 1; j < W; ++j) {
        double qx = bx, qy = by;
        if (j < W - 1) {
            const double2 u = urow[j];
            qx = cx + 0.5 * (vx * u.x - vy * u.y);
            qy = cy + 0.5 * (vy * u.x + vx * u.y);
        }
        const double qz = alt(j);
        const double dx = qx - px, dy = qy - py;
        double sxy = 0.0, dxy = 0.0;
        sxy = sxy + dx * dx;
        sxy = sxy + dy * dy;
        dxy = dxy + pdx * dx;
        dxy = dxy + pdy * dy;
        vert_segment(p, v, j, sxy, dxy, (qz - pz) * v.zs, g);
        pdx = dx, pdy = dy;
        px = qx, py = qy, pz = qz;
    }
    const Slot* slot = reinterpret_cast<const Slot*>(kg.slot);
    double cost = (double)(N + 1) * g.L, nsum = 0.0, cm = INFINITY;
    int32_t nh = 0, off = 0, bel = 0;
    X128 xc = {0, 0}, xn = {0, 0};
    uint32_t xfl = 0;
    for (int s = 0; s < kg.nseg; ++s) {
        const Slot sl = slot[(int64_t)s * kg.P + gp];
        if constexpr (EX) {
            xc = x_add(xc, X128{sl.c_lo, sl.c_hi});
            xn = x_add(xn, X128{sl.n_lo, sl.n_hi});
            xfl |= sl.cnt >> 24;
        } else {
            cost = cost + sl.cost;
            nsum = nsum + sl.psi;
        }
        cm = fmin(cm, sl.cm);
        nh += (int32_t)(sl.cnt & 255u);
        off += (int32_t)((sl.cnt >> 8) & 255u);
        bel += (int32_t)((sl.cnt >> 16) & 255u);
    }
    if constexpr (EX) {  // one rounding per field, a true division
        cost = cost + x_result(xc, xfl & 7u, e_risk) / (double)N;
        nsum = x_result(xn, (xfl >> 3) & 7u, e_psi);
    }
    put_outputs(out, gp, bad, cost, g.L, g.len, g.ksum, nsum, cm, nh, off, bel);
    if (v.climb) v.climb[gp] = bad ? __builtin_nan("") : g.csum;
}
__global__ __launch_bounds__(256) void k_vp_final_v(KParams p, KGrp kg, KProf kf, KVert v,
                                                    KOut out) {
    vp_final_v_path<false>(p, kg, kf, v, out, 0, 0);
}
__global__ __launch_bounds__(256) void k_vp_final_xv(KParams p, KGrp kg, KProf kf, KVert v,
                                                     KOut out,
                                                     const int32_t* __restrict__ scale) {
    const int32_t e_risk = __builtin_amdgcn_readfirstlane(scale[0]);
    const int32_t e_psi = __builtin_amdgcn_readfirstlane(scale[1]);
    vp_final_v_path<true>(p, kg, kf, v, out, e_risk, e_psi);
}

// after k_argmin: a failed sort check leaves -1 in both selections, as the other output
// launches do
__global__ __launch_bounds__(256) void k_vp_sel_check(const int32_t* __restrict__ err,
                                                      int64_t n_pairs, int32_t* __restrict__ best_f,
                                                      int32_t* __restrict__ best_l) {
    if (*err == 0) return;
    const int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (q >= n_pairs) return;
    if (best_f) best_f[q] = -1;
    if (best_l) best_l[q] = -1;
}
