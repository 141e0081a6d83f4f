// k4hp.inc -- K4hp, the altitude-profile candidates on the packed, sorted volume: the output
// launches k_vp_final / k_vp_final_x, k_vp_final_v / k_vp_final_xv (K4hp+v: under the vertical
// terms) and k_vp_sel_check.  The sort and the evaluation are k4h.inc's kernels with a trailing
// KProf (k_vp_hist, k_vp_eval / k_vp_eval_x); KProf, vp_z and vp_split stand there.
// Included in the anonymous namespace of uampath.hip after k4h.inc; relies on its text (VSlot /
// VSlotX, KProf, v_path_slots) and on what k4h.inc relies on; K4hp+v also on KVert, VertAcc, vert_begin and
// vert_segment (uampath.hip, K4e+v / K4p+v).  Definition: include/uampath.h.

// outputs of every path, one thread per path (v_final_wg's 64 x D block does not reach D A =
// 128): the similarity-form geometry of the path's (q, d) -- the same for its A profiles -- and
// the partials in group order, as v_final_wg; the selections follow in k_argmin over D A
template <bool EX>
__device__ __forceinline__ void vp_final_path(const KParams& p, const KGrp& kg, const KProf& kf,
                                              const KOut& out, int32_t e_risk, int32_t e_psi) {
    const int64_t gp = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const bool bad = *kg.err != 0;  // an inconsistent sort (k_g_scatter / k_vp_hist)
    if (bad && gp == 0 && kg.herr) *kg.herr = 1;
    if (gp >= kg.P) return;
    int32_t q, di, a;
    vp_split(kg, kf, (int32_t)gp, q, di, a);
    const double* pr = kg.pairs + (int64_t)q * 6;
    double L, len, ksum;
    sim_geo(p, kg.ugeo[di], pr[0], pr[1], pr[3], pr[4], L, len, ksum);
    double cost = (double)(p.N + 1) * L, nsum, cm;
    int32_t nh, off, bel;
    v_path_slots<EX>(kg, gp, p.N, e_risk, e_psi, cost, nsum, cm, nh, off, bel);
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
    double cost = (double)(N + 1) * g.L, nsum, cm;
    int32_t nh, off, bel;
    v_path_slots<EX>(kg, gp, N, e_risk, e_psi, cost, nsum, cm, nh, off, bel);
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
