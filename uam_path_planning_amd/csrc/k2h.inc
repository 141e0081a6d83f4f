// k2h.inc -- K2h, the similarity form: HSlot / HSlotX, the exact-sum arithmetic host and device
// share (X128, x_add, x_term, x_to_double, x_result), the terrain maximum by bounds, k_h_eval /
// k_h_eval_x, k_cells, k_h_final / k_h_final_x.
// Included in the anonymous namespace of uampath.hip, after K2g; relies on its text above: the
// device tables, the packed raster (gen_cell, p4_addr, pk_*), xcd_chunk, K2g's KGrp, UGeo, put_*.

// ---- K2h: generated candidates in the similarity form (oracle orc_eval_generated_h) --------
// The candidate arcs are p_k = C + (1/2) R(v) u_k (u_0 = (1, 0), u_{N+1} = (-1, 0)): the unit
// polyline of the displacement's table row under a similarity of scale h = |v| / 2.  Every
// term that depends on the geometry only -- get_cost's L (problem.py:130-146, with the quirk's
// anchor term), the true length (solver.py:49), the kinematic rows (problem.py:100-107, their
// ratio rows scale with h, their turn rows are the unit polyline's) -- is a per-displacement
// sum of the unit polyline times h (maxratio_smooth = 0), formed once per launch (UGeo) and
// scaled per path in the output launch.  What stays per waypoint is what the raster decides:
// the point, its cell and its record (Phi / N, psi, terrain, no-fly hit), with K2g's sort,
// staging and grouped partial sums; so an item carries no f64 geometry (no segment norms, no
// square roots, no kinematic rows) and its slot is 24 B.  Exact in real arithmetic; in float64
// the geometry terms differ from per-segment sums by rounding only (bench.py
// parity.vs_sequential_order on the whole cfg3 batch).

struct alignas(8) HSlot {  // 24 B per (path, group), written by one lane
    double cost;   // Phi / N of the group's waypoints, from +0.0 in waypoint order
    double psi;    // the no-fly psi, likewise
    float hmax;    // max terrain of the group's waypoints as consume reads it
    uint32_t cnt;  // nfz hits | off-raster << 8
};

// ---- exact raster sums (UAM_OPT_EXACT_SUM; the definition: include/uampath.h) ---------------
// A field's float32 words are added as integers in units of the raster's quantum
// q = 2^(e - 96), e = max(1, largest biased exponent field among the finite cells) - 126: a
// word is a signed 24-bit significand shifted by sh = max(b, 1) - 54 - e <= 72 (a right shift
// truncates the magnitude), so |term| < 2^96 and a 128-bit two's-complement sum holds 2^31 of
// them.  Integer addition is associative: the sum does not depend on the group length, on the
// order of the groups or on which lane adds what.  One rounding, to float64, at the end.
// The same functions run on the host (uam_exact_sum_host) and in the kernels.
struct X128 {  // two's complement, two 64-bit limbs
    uint64_t lo, hi;
};
enum : uint32_t { XF_NAN = 1u, XF_PINF = 2u, XF_NINF = 4u };  // a field's side flags
constexpr int X_E_MIN = -125, X_E_MAX = 128;                  // the exponents a raster can give

__host__ __device__ __forceinline__ X128 x_add(X128 a, X128 b) {
    X128 r;
    r.lo = a.lo + b.lo;
    r.hi = a.hi + b.hi + (r.lo < a.lo ? 1u : 0u);  // the low limb's carry
    return r;
}
__host__ __device__ __forceinline__ X128 x_neg(X128 a) {
    X128 r;
    r.lo = ~a.lo + 1u;
    r.hi = ~a.hi + (r.lo == 0 ? 1u : 0u);
    return r;
}
// the exponent a word asks of its raster: max(b, 1) - 126 for a finite word, X_E_MIN otherwise
__host__ __device__ __forceinline__ int32_t x_word_exp(uint32_t w) {
    const int32_t b = (int32_t)((w >> 23) & 255u);
    return b == 255 ? X_E_MIN : (b > 1 ? b : 1) - 126;
}
// a word's side flags (0 for a finite word)
__host__ __device__ __forceinline__ uint32_t x_word_flags(uint32_t w) {
    const uint32_t f = (w & 0x7fffffu) ? XF_NAN : (w >> 31) ? XF_NINF : XF_PINF;
    return ((w >> 23) & 255u) == 255u ? f : 0u;
}
// a word's term at the exponent e >= x_word_exp(w) (0 for a non-finite word): selects and masks
// only, so the kernels' consume loops stay straight-line code
__host__ __device__ __forceinline__ X128 x_term(uint32_t w, int32_t e) {
    const uint32_t b = (w >> 23) & 255u;
    // the 24-bit significand: no hidden bit in a denormal, nothing from a non-finite word
    const uint32_t m = b == 255u ? 0u : (w & 0x7fffffu) | (b ? 0x800000u : 0u);
    const int sh = (int)(b ? b : 1u) - 54 - e;  // <= 72
    const int rs = sh < 0 ? (-sh < 24 ? -sh : 24) : 0;  // a right shift of >= 24 leaves nothing
    const int ls = sh > 0 ? sh : 0;
    const int s = ls & 63;
    const uint64_t a = (uint64_t)(m >> rs) << s;
    const uint64_t c = ((uint64_t)m >> 1) >> (63 - s);  // the bits shifted past the low limb
    const uint64_t lo = ls < 64 ? a : 0u;
    const uint64_t hi = ls < 64 ? c : a;  // (ls >= 64: s <= 8, so a holds every bit)
    // the sign: -t = ~t + 1 through a mask (the low limb carries only when it is 0)
    const uint64_t sg = w >> 31, mk = 0u - sg;
    X128 t;
    t.lo = (lo ^ mk) + sg;
    t.hi = (hi ^ mk) + (sg & (lo == 0 ? 1u : 0u));
    return t;
}
// S 2^(e - 96) rounded once to float64, to nearest even: the magnitude normalised by its
// leading zeros, its top 53 bits, a guard bit and the sticky rest (no int128 -> double
// conversion: the device has none).  e in [X_E_MIN, X_E_MAX] keeps the result a normal double.
__host__ __device__ __forceinline__ double x_to_double(X128 s, int32_t e) {
    const bool neg = (s.hi >> 63) != 0;
    if (neg) s = x_neg(s);
    if ((s.lo | s.hi) == 0) return 0.0;
    const int lz = s.hi ? __builtin_clzll(s.hi) : 64 + __builtin_clzll(s.lo);
    X128 n;  // s << lz: bit 127 set
    if (lz >= 64) {
        n.hi = s.lo << (lz - 64);
        n.lo = 0;
    } else if (lz) {
        n.hi = (s.hi << lz) | (s.lo >> (64 - lz));
        n.lo = s.lo << lz;
    } else {
        n = s;
    }
    const uint64_t mant = n.hi >> 11;  // in [2^52, 2^53)
    const bool guard = (n.hi >> 10) & 1u, sticky = ((n.hi & 0x3ffu) | n.lo) != 0;
    const uint64_t inc = (guard && (sticky || (mant & 1u))) ? 1u : 0u;
    const int ex = 127 - lz + e - 96;  // the leading bit's binade
    // (a carry out of the fraction steps the exponent field: the next power of two)
    uint64_t bits = ((uint64_t)(ex + 1023) << 52) + (mant - ((uint64_t)1 << 52)) + inc;
    bits |= neg ? (uint64_t)1 << 63 : 0u;
    double r;
    __builtin_memcpy(&r, &bits, 8);
    return r;
}
// a field's result: IEEE's for the non-finite words that were left out of S
__host__ __device__ __forceinline__ double x_result(X128 s, uint32_t flags, int32_t e) {
    if ((flags & XF_NAN) || ((flags & XF_PINF) && (flags & XF_NINF))) return __builtin_nan("");
    if (flags & XF_PINF) return __builtin_inf();
    if (flags & XF_NINF) return -__builtin_inf();
    return x_to_double(s, e);
}

struct alignas(8) HSlotX {  // the exact form's slot: 40 B per (path, group)
    uint64_t c_lo, c_hi;  // the sum of the group's phi terms
    uint64_t n_lo, n_hi;  // the sum of its psi terms
    float hmax;           // as HSlot's
    uint32_t cnt;         // as HSlot's | phi flags << 16 | psi flags << 19
};

// every (path, group) item in K2g's sorted order: the group's points, cells and packed entries
// only.  Every chunk is straight-line, in three phases so the LDS and memory round trips of its
// CH slots overlap: the CH cells (the arc formula; p_0 / p_{W-1} from the pair's cells), the CH
// header reads (code word, bound entry, superblock), then per slot the decisions and two
// unconditional loads -- the code's entry (a slot with nothing to read takes the first p4 line)
// and the terrain (the first t4 word unless fetched) -- by 32-bit offsets from the packed
// copy's base; then the branch-free consume.
//
// The terrain maximum by bounds (build-defined; the outputs are exactly the per-waypoint
// maximum's): min_clearance needs only the path's maximum terrain M, an order-free maximum, so
// a waypoint's exact terrain is fetched (t4) only when it could still be M.  Every in-raster
// waypoint w has decoded bounds lb_w <= terrain_w <= ub_w (pk_bound_raw + pk_bound_decode).  The item keeps
//   Lb: a lower bound of M: the path's seed (below), raised by its own waypoints' lb as it
//       goes; off-raster waypoints count +0.0, their exact value;
//   E:  the maximum of exact terrain values of the path: the seed E0 (h_path_seed, formed once
//       per path by the histogram launch: the exact terrain of the sampled waypoint with the
//       largest lb) and those the item takes (fetched, code-3 records, off-raster +0.0, blocks
//       whose bounds coincide).
// It fetches w iff !(ub_w <= E) && !(ub_w < Lb) (NaN bounds: "no bound", always fetched).
// Exactness: let w* hold M, in this item's group.  If w* was not taken exactly, then either
// ub_w* <= E, so M <= E and E -- an exact terrain value of the path -- is M; or ub_w* < Lb <= M,
// impossible since M <= ub_w*.  So the group holding M reports M, every group reports at most
// its own maximum (E holds exact values), and the output launch's maximum over the groups is M.
// (A group without M may report less than its own maximum: only the path's is an output.)
// The slot's hmax is that E.  (Measured, cfg3: 0.19 fetches per waypoint with the sampled lb
// alone and chunks issued one ahead, tools/k2h_counts.py.)
// K2h workgroup: 256 items (cfg3 0.297 ms against 0.306 at 512, profiles/r05/k2h12)
constexpr int H_BS = UAM_K2H_BS;
// EX (UAM_OPT_EXACT_SUM): the phi and psi words added as 128-bit integer terms at the raster's
// exponents e_phi / e_psi (x_term) into an HSlotX, the non-finite ones as side flags
template <int CH, bool TE, bool EX = false>  // TE: the terrain in the entry (UAM_OPT_K2H_TERRAIN 1)
__device__ __forceinline__ void h_item(const KParams& p, const KRaster& rs, const KGrp& kg,
                                       const uint32_t* __restrict__ s_hdr,
                                       const double2* __restrict__ s_u, bool live, int32_t item,
                                       int32_t path, int32_t q, const double4& pr,
                                       float seed, int32_t e_phi = 0, int32_t e_psi = 0) {
    // a lane past the last item evaluates nothing and writes nothing
    const int s = item - path * kg.nseg;
    const int32_t d = path - q * kg.D;
    const int N = p.N, W = kg.W;
    // waypoint j's unit vector is urow[j] (j = 1..N); the slots past a row's ends read the
    // neighbouring rows or the staged padding (LDS either way), and their cells are replaced
    const double2* urow = s_u + d * N - 1;
    const int j0 = s * kg.G, j1 = live ? min(j0 + kg.G, W) : j0;
    // chunks: the wave's most, so the loop is wave-uniform
    int nch = (j1 - j0 + CH - 1) / CH;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) nch = max(nch, __shfl_xor(nch, o));
    const double vx = pr.x - pr.z, vy = pr.y - pr.w;
    const double cx = (pr.z + pr.x) * 0.5, cy = (pr.w + pr.y) * 0.5;
    const double dN = (double)N, yN = kg.inv_n;
    auto over_n = [&](double a) {  // Phi / N exactly as k_g_eval forms it (K2h: N <= 4096)
        const double q0 = a * yN;
        const double q1 = fma(fma(-q0, dN, a), yN, q0);
        return __builtin_isinf(a) ? q0 : q1;
    };
    // the end points' cells, formed once
    int32_t ixF, iyF, ixL, iyL;
    const bool inF = gen_cell(rs, pr.x, pr.y, ixF, iyF);
    const bool inL = gen_cell(rs, pr.z, pr.w, ixL, iyL);
    const uint16_t* const bnd = reinterpret_cast<const uint16_t*>(s_hdr + rs.bnd_off);
    const float2* const sbt = reinterpret_cast<const float2*>(s_hdr + rs.sbt_off);
    const char* const pk = rs.pk;
    // the plane offsets as values (a select between the struct's fields otherwise becomes a
    // select of their addresses and a memory read per slot)
    const uint32_t o4 = __builtin_amdgcn_readfirstlane(rs.o4);
    const uint32_t o8 = __builtin_amdgcn_readfirstlane(rs.o8);
    const uint32_t o16 = __builtin_amdgcn_readfirstlane(rs.o16);
    const uint32_t ot4 = __builtin_amdgcn_readfirstlane(rs.ot4);
    const uint32_t op8 = __builtin_amdgcn_readfirstlane(rs.op8);
    double gc = 0.0, gn = 0.0;
    X128 xc = {0, 0}, xn = {0, 0};  // EX: the group's phi and psi terms
    uint32_t xf = 0;                // EX: their side flags (phi | psi << 3)
    // EX: one word into its field's sum (straight-line: wave-uniform skips of all-zero slots
    // and of the flags, and slots split into aligned planes, gained nothing at cfg3, DESIGN §10)
    auto x_take = [&](X128& acc, uint32_t w, int32_t e, int fs) {
        acc = x_add(acc, x_term(w, e));
        xf |= x_word_flags(w) << fs;
    };
    float Lb = seed, E = seed;  // the path's seed: an exact terrain value of the path
    uint32_t nh = 0, off = 0;
    // one chunk ahead: chunk c + 1's loads are issued before chunk c is consumed (the fetch
    // rule then sees E without chunk c's fetched values: valid, E only holds exact values).
    // Iteration c issues chunk c + 1 into the B arrays and consumes chunk c from the A arrays.
    uint4 rA[CH];
    float tvA[CH];
    uint32_t kcA[CH], vinA = 0, tkA = 0;
    int nvA = 0;
    // (ahead: chunk c + 1 issued before chunk c is consumed -- the same at cfg3 with 256-item
    // workgroups, profiles/r05/k2h12)
    constexpr bool ahead = false;
    for (int c = ahead ? -1 : 0; c < nch; ++c) {  // (nch wave-uniform)
        const int ci = ahead ? c + 1 : c;  // the chunk issued by this iteration
        uint4 rB[CH];
        float tvB[CH];
        uint32_t kcB[CH], vinB = 0, tkB = 0;
        int nvB = 0;
        if (ci < nch) {
            const int jc = j0 + ci * CH;
            const double2* uc = urow + jc;
            // phase 1: the cells (in-raster and in-group bits per slot)
            int32_t ix[CH], iy[CH];
            uint32_t vjb = 0;
#pragma unroll
            for (int t = 0; t < CH; ++t) {
                const int j = jc + t;
                const double2 u = uc[t];
                int32_t x, y;
                bool in = gen_cell(rs, cx + 0.5 * (vx * u.x - vy * u.y),
                                   cy + 0.5 * (vy * u.x + vx * u.y), x, y);
                if (t == 0) {  // (j == 0 only in a chunk's first slot)
                    const bool f = jc == 0;
                    x = f ? ixF : x;
                    y = f ? iyF : y;
                    in = f ? inF : in;
                }
                const bool l = j == W - 1;
                ix[t] = l ? ixL : x;
                iy[t] = l ? iyL : y;
                in = l ? inL : in;
                const bool vj = j < j1;
                vjb |= (uint32_t)vj << t;
                vinB |= (uint32_t)(in & vj) << t;
            }
            // phase 2: the header reads (cell (0, 0) for a slot off the raster: valid reads)
            uint32_t cw[CH], be[CH];
            float2 sb[CH];
#pragma unroll
            for (int t = 0; t < CH; ++t) {
                const int32_t b = pk_block(rs, ix[t], iy[t]);
                cw[t] = s_hdr[b >> 4] >> ((b & 15) * 2);
                if constexpr (!TE) {
                    const uint32_t bx = (uint32_t)(ix[t] >> rs.bshift);
                    const uint32_t by = (uint32_t)(iy[t] >> rs.bshift);
                    be[t] = bnd[__umul24(by, (uint32_t)rs.bnbx) + bx];
                    sb[t] = sbt[__umul24(by >> 2, (uint32_t)rs.sbnbx) + (bx >> 2)];
                }
            }
            // phase 3: the decisions and the loads
#pragma unroll
            for (int t = 0; t < CH; ++t) {
                const bool vin = (vinB >> t) & 1u, vj = (vjb >> t) & 1u;
                const uint32_t code = cw[t] & (vin ? 3u : 0u);
                if constexpr (TE) {
                    // code 1: the 8-B {phi, terrain} entry; 2 / 3: the 16-B record (both carry
                    // the exact terrain); code 0: nothing to read (phi, psi +-0, terrain +0.0)
                    const bool rec = code & 2u;
                    const uint32_t a4 = (uint32_t)p4_addr(rs, ix[t], iy[t]);
                    const uint32_t ab = (uint32_t)p44_addr(rs, ix[t], iy[t]) << 3;
                    const uint32_t voff = rec ? o16 + (a4 << 4) : code ? op8 + (ab & ~15u) : o4;
                    kcB[t] = code | (rec ? 0u : (ab & 8u));
                    rB[t] = *reinterpret_cast<const uint4*>(pk + voff);
                    (void)vj;
                    continue;
                }
                float ub, lb;
                pk_bound_decode(be[t], sb[t], ub, lb);
                // off the raster or code 0: +0.0, an exact value and a lower bound; a block
                // of one value: ub
                const bool zero = !vin | (code == 0u);
                Lb = fmaxf(Lb, vj ? (zero ? 0.0f : lb) : -INFINITY);
                E = fmaxf(E, vj ? (zero ? 0.0f : lb == ub ? ub : -INFINITY) : -INFINITY);
                const bool fetch = !zero & (code != 3u) & !(ub <= E) & !(ub < Lb);
                const uint32_t a4 = (uint32_t)p4_addr(rs, ix[t], iy[t]);
                // the entry's byte offset in its plane: a4 * 4 / 8 / 16 for codes 1 / 2 / 3;
                // its aligned 16 B and the cell's word in them
                const uint32_t ab = a4 << (code + 1u);
                const uint32_t base = (code & 2u) ? ((code & 1u) ? o16 : o8) : o4;
                const uint32_t voff = base + (code ? (ab & ~15u) : 0u);
                kcB[t] = code | (ab & 12u);
                rB[t] = *reinterpret_cast<const uint4*>(pk + voff);
                tvB[t] = *reinterpret_cast<const float*>(pk + (ot4 + (fetch ? a4 * 4u : 0u)));
                tkB |= (uint32_t)fetch << t;
            }
            nvB = max(0, min(CH, j1 - jc));  // slots past the group's end: no waypoint
        }
        if (!ahead) {
#pragma unroll
            for (int t = 0; t < CH; ++t) rA[t] = rB[t], tvA[t] = tvB[t], kcA[t] = kcB[t];
            vinA = vinB, tkA = tkB, nvA = nvB;
        }
        if (c >= 0) {
#pragma unroll
            for (int t = 0; t < CH; ++t) {
                const bool vl = t < nvA;
                const bool in = (vinA >> t) & 1u;
                if constexpr (TE) {
                    const uint4 r = rA[t];
                    const uint32_t code = kcA[t] & 3u;  // (0 off the raster)
                    const bool rec = code & 2u, s1 = kcA[t] & 8u;
                    const uint32_t lo = s1 ? r.z : r.x, hi = s1 ? r.w : r.y;
                    const uint32_t phi = code ? (rec ? r.x : lo) : 0u;
                    const uint32_t tb = rec ? ((r.w & UAM_FLAG_NODATA) ? 0u : r.z) : hi;
                    nh += (rec && (r.w & UAM_FLAG_NFZ)) ? 1u : 0u;
                    off += (vl && !in) ? 1u : 0u;
                    if constexpr (EX) {
                        x_take(xc, phi, e_phi, 0);
                        x_take(xn, rec ? r.y : 0u, e_psi, 3);
                    } else {
                        gc = gc + over_n((double)__uint_as_float(phi));
                        gn = gn + (rec ? (double)__uint_as_float(r.y) : 0.0);
                    }
                    // (off the raster, or code 0: +0.0 exactly)
                    E = fmaxf(E, code ? __uint_as_float(tb) : vl ? 0.0f : -INFINITY);
                    continue;
                }
                uint32_t phi, psi, hit;
                float rter;
                pk_terms_k(rA[t], kcA[t], phi, psi, hit, rter);
                nh += hit;
                off += (vl && !in) ? 1u : 0u;
                if constexpr (EX) {
                    x_take(xc, phi, e_phi, 0);
                    x_take(xn, psi, e_psi, 3);
                } else {
                    gc = gc + over_n((double)__uint_as_float(phi));
                    gn = gn + (double)__uint_as_float(psi);
                }
                const float ter = (kcA[t] & 3u) == 3u ? rter : ((tkA >> t) & 1u) ? tvA[t] : -INFINITY;
                E = fmaxf(E, ter);
            }
        }
        if (ahead) {
#pragma unroll
            for (int t = 0; t < CH; ++t) rA[t] = rB[t], tvA[t] = tvB[t], kcA[t] = kcB[t];
            vinA = vinB, tkA = tkB, nvA = nvB;
        }
    }
    if constexpr (EX) {
        HSlotX o;
        o.c_lo = xc.lo, o.c_hi = xc.hi;
        o.n_lo = xn.lo, o.n_hi = xn.hi;
        o.hmax = E;
        o.cnt = nh | (off << 8) | (xf << 16);
        if (live) reinterpret_cast<HSlotX*>(kg.slot)[(int64_t)s * kg.P + path] = o;
        return;
    }
    HSlot o;
    o.cost = gc;
    o.psi = gn;
    o.hmax = E;
    o.cnt = nh | (off << 8);
    if (live) reinterpret_cast<HSlot*>(kg.slot)[(int64_t)s * kg.P + path] = o;
}

// K2h evaluation: workgroups of H_BS items (xcd_chunk), the packed raster's header (codes,
// bounds, superblocks) and the unit-arc rows (+ G + CH padding slots) staged in LDS, then one item
// per lane (h_item)
template <int CH, bool TE, bool EX>
__device__ __forceinline__ void h_eval_wg(KParams p, KRaster rs, KGrp kg, int32_t e_phi,
                                          int32_t e_psi) {
    PK_CODES_CHECK(CH);
    extern __shared__ __attribute__((aligned(16))) uint32_t s_dyn[];
    uint32_t* s_hdr = s_dyn;
    // the header in LDS: codes, bounds and superblocks; the code map alone with TE
    const int hw = TE ? rs.bnd_off : rs.hwords;
    double2* s_u = reinterpret_cast<double2*>(s_dyn + hw);
    // the item's order entry, pair and path bound first: their dependent round trips overlap
    // the staging below instead of following it
    const int64_t pos = xcd_chunk(blockIdx.x, gridDim.x) * H_BS + threadIdx.x;
    const bool live = pos < kg.n_items;
    const int32_t item = live ? kg.order[pos] : 0;
    const int32_t path = (int32_t)div_magic((uint32_t)item, kg.m_nseg, kg.sh_nseg);
    const int32_t q = (int32_t)div_magic((uint32_t)path, kg.m_d, kg.sh_d);
    const double4 pr = reinterpret_cast<const double4*>(kg.pairs)[q];
    const float seed = kg.lbp ? kg.lbp[path] : -INFINITY;
    const int nu = kg.D * p.N;
    {  // staging: every load of a thread issued before its first LDS store (hw % 4 == 0)
        constexpr int U = 4;
        const int nv = hw >> 2;
        const uint4* src = reinterpret_cast<const uint4*>(rs.pmap);
        uint4* dst = reinterpret_cast<uint4*>(s_hdr);
        const uint4* gu = reinterpret_cast<const uint4*>(kg.utab);
        uint4* du = reinterpret_cast<uint4*>(s_u);
        for (int i0 = threadIdx.x; i0 < nv + nu; i0 += H_BS * U) {
            uint4 v[U];
#pragma unroll
            for (int k = 0; k < U; ++k) {  // unconditional loads (past the end: the first word)
                const int i = i0 + k * H_BS;
                v[k] = *(i < nv ? src + i : i < nv + nu ? gu + (i - nv) : src);
            }
#pragma unroll
            for (int k = 0; k < U; ++k) {  // unconditional stores (past the end: a pad slot)
                const int i = i0 + k * H_BS;
                *(i < nv ? dst + i : du + min(i - nv, nu)) = v[k];
            }
        }
    }
    __syncthreads();
    // the padding: a lane's slots reach index nu + G + CH - 2 at most (a last group of one
    // waypoint in a wave of full ones)
    if ((int)threadIdx.x < kg.G + CH) s_u[nu + threadIdx.x] = make_double2(0.0, 0.0);
    __syncthreads();
    h_item<CH, TE, EX>(p, rs, kg, s_hdr, s_u, live, item, path, q, pr, seed, e_phi, e_psi);
}
template <int CH, bool TE>
__global__ __launch_bounds__(H_BS, UAM_K2H_MINW) void k_h_eval(KParams p, KRaster rs, KGrp kg) {
    h_eval_wg<CH, TE, false>(p, rs, kg, 0, 0);
}
// the exact form (UAM_OPT_EXACT_SUM): the raster's exponents scale = {e_phi, e_psi, ...}
// (uam_raster_sum_scale) read once per workgroup at a uniform address
template <int CH, bool TE>
__global__ __launch_bounds__(H_BS, UAM_K2H_MINW) void k_h_eval_x(
    KParams p, KRaster rs, KGrp kg, const int32_t* __restrict__ scale) {
    const int32_t e_phi = __builtin_amdgcn_readfirstlane(scale[0]);
    const int32_t e_psi = __builtin_amdgcn_readfirstlane(scale[1]);
    h_eval_wg<CH, TE, true>(p, rs, kg, e_phi, e_psi);
}

// The waypoint cells (the reference's returned waypoints as raster cells, solver.py:49,
// main.py:186-190) of the sorted forms: cells[path][j] = iy nx + ix (-1 off the raster) by the
// evaluations' own point and cell arithmetic (gen_cell), one thread per (path, j), so
// consecutive threads write consecutive cells -- whole lines, no gathers.  (Written by the
// evaluation's lanes through LDS instead, the 21-cell runs of scattered items cost K2h ~120 us
// of partial-line writes per cfg3 step: 402 MB of WRITE_SIZE for 164 MB of cells,
// profiles/r04/final2/cells.)
// The waypoint cells of paths [path0, path0 + np) by one workgroup of nt threads (np <= 1024):
// each path's chord terms (cx, cy, vx, vy: arc_point's) and end-point cells go to s_cv / s_e
// once, then work item w = (path lp = w / R, run k = w % R) forms the run's 4 cells
// j = 4k ... 4k + 3 of one path (R = ceil(W / 4) runs a path; cells past W are not stored),
// so a lane reads its path's terms once and selects nothing per cell; items advance by nt a
// step (nt = lstep R + kstep, one conditional subtraction).  Every thread of the workgroup
// calls it (it synchronises).  u_rows: the unit-arc rows (LDS when staged).
__device__ __forceinline__ void cells_rows(const KParams& p, const KGrp& kg, int64_t path0,
                                           int np, double4* s_cv, int4* s_e,
                                           const double2* __restrict__ u_rows, int t, int nt) {
    const int W = kg.W, N = p.N;
    __syncthreads();  // (a previous block's reads of s_cv / s_e are done)
    for (int i = t; i < np; i += nt) {
        const int32_t path = (int32_t)(path0 + i);
        const int32_t q = (int32_t)div_magic((uint32_t)path, kg.m_d, kg.sh_d);
        const double4 pr = reinterpret_cast<const double4*>(kg.pairs)[q];
        s_cv[i] = make_double4((pr.z + pr.x) * 0.5, (pr.w + pr.y) * 0.5, pr.x - pr.z,
                               pr.y - pr.w);
        int32_t ix, iy;  // the end points: the pair's own coordinates
        const int32_t c0 = gen_cell_g(kg.cx0, kg.cy_top, kg.cinv_dx, kg.cinv_dy, kg.cnx, kg.cny,
                                      pr.x, pr.y, ix, iy) ? iy * kg.cnx + ix : -1;
        const int32_t c1 = gen_cell_g(kg.cx0, kg.cy_top, kg.cinv_dx, kg.cinv_dy, kg.cnx, kg.cny,
                                      pr.z, pr.w, ix, iy) ? iy * kg.cnx + ix : -1;
        s_e[i] = make_int4((path - q * kg.D) * N, c0, c1, 0);
    }
    __syncthreads();
    int32_t* out = kg.cells + path0 * W;
    const int R = (W + 3) >> 2, items = np * R;
    int lp = t / R, k = t - lp * R;
    const int lstep = nt / R, kstep = nt - lstep * R;
    for (int w = t; w < items; w += nt) {
        const double4 cv = s_cv[lp];
        const int4 e = s_e[lp];
        const int j0 = 4 * k;
        int32_t v[4];
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const int jj = j0 + c;
            const double2 u = u_rows[e.x + min(max(jj - 1, 0), N - 1)];
            const double x0 = cv.x + 0.5 * (cv.z * u.x - cv.w * u.y);  // arc_point's ops
            const double x1 = cv.y + 0.5 * (cv.w * u.x + cv.z * u.y);
            int32_t ix, iy;
            const bool in = gen_cell_g(kg.cx0, kg.cy_top, kg.cinv_dx, kg.cinv_dy, kg.cnx, kg.cny,
                                       x0, x1, ix, iy);
            v[c] = jj == 0 ? e.y : jj == W - 1 ? e.z : in ? iy * kg.cnx + ix : -1;
        }
        // streaming stores: the 164 MB of cfg3's cells do not stay in L2 / the Infinity Cache
        // as dirty lines whose write-back the next step's gathers would meet (plain stores:
        // cfg3 with cells 0.399 against 0.374 ms, profiles/r05/cc6); a wave's runs cover ~3
        // paths' contiguous rows
        int32_t* o = out + (int64_t)lp * W + j0;
        if (j0 + 3 < W && !(((uintptr_t)o) & 7)) {
            typedef int32_t v2i __attribute__((ext_vector_type(2)));
            const v2i w0 = {v[0], v[1]}, w1 = {v[2], v[3]};
            __builtin_nontemporal_store(w0, reinterpret_cast<v2i*>(o));
            __builtin_nontemporal_store(w1, reinterpret_cast<v2i*>(o) + 1);
        } else {
#pragma unroll
            for (int c = 0; c < 4; ++c)
                if (j0 + c < W) o[c] = v[c];
        }
        lp += lstep, k += kstep;
        if (k >= R) k -= R, ++lp;
    }
}

// The waypoint cells (the reference's returned waypoints as raster cells, solver.py:49,
// main.py:186-190) of the sorted forms that do not write them in their output launch (K2g):
// cells[path][j] = iy nx + ix (-1 off the raster) by the evaluations' own point and cell
// arithmetic, workgroups of 64 consecutive paths (cells_rows) looping over the path blocks.
// (Written by the evaluation's lanes through LDS instead, the 21-cell runs of scattered items
// cost K2h ~120 us of partial-line writes per cfg3 step: 402 MB of WRITE_SIZE for 164 MB of
// cells, profiles/r04/final2/cells.)
template <bool ULDS>  // the unit-arc rows staged in LDS (D N <= 1024) or read from global
__global__ __launch_bounds__(256) void k_cells(KParams p, KGrp kg) {
    constexpr int kUtabLds = 1024;  // (16 KiB)
    __shared__ double4 s_cv[64];
    __shared__ int4 s_e[64];
    __shared__ double2 s_u[ULDS ? kUtabLds : 1];
    const int t = threadIdx.x;
    const double2* __restrict__ gu = reinterpret_cast<const double2*>(kg.utab);
    if (ULDS)
        for (int k = t; k < kg.D * p.N; k += 256) s_u[k] = gu[k];
    const int64_t nblk = ((int64_t)kg.P + 63) / 64;
    // (a grid smaller than nblk loops over the blocks: the side-stream launch's share of CUs)
    for (int64_t blk = blockIdx.x; blk < nblk; blk += gridDim.x) {
        const int64_t path0 = blk * 64;
        const int np = (int)min((int64_t)64, (int64_t)kg.P - path0);
        cells_rows(p, kg, path0, np, s_cv, s_e, ULDS ? s_u : gu, t, 256);
    }
}

// outputs of every path (block = 64 pairs x D, k_g_final's layout): the geometry terms from
// the pair's scale and the displacement's unit sums (oracle sim_geo), cost = (N+1) L + the
// Phi / N partials in group order, and the main.py:175-180 selection
// EX (UAM_OPT_EXACT_SUM): a path's HSlotX sums added as integers and their flags ORed, each
// field rounded once (x_result), cost = (N+1) L + fl(S_phi) / N, nfz_sum = fl(S_psi)
template <int NR, bool EX>  // slots per path held in registers (0: a loop for long paths)
__device__ __forceinline__ void h_final_wg(KParams p, KGrp kg, KOut out,
                                           int32_t* __restrict__ best_f,
                                           int32_t* __restrict__ best_l, int32_t e_phi,
                                           int32_t e_psi) {
    using Slot = std::conditional_t<EX, HSlotX, HSlot>;
    extern __shared__ __attribute__((aligned(16))) double smem[];
    const int D = kg.D, t = threadIdx.x;
    double* s_cost = smem;
    double* s_len = smem + 64 * D;
    const int64_t q0 = (int64_t)blockIdx.x * 64;
    const int qi = t / D, di = t - qi * D;
    const bool bad = *kg.err != 0;  // an inconsistent sort (k_g_scatter / k_v_hist)
    const Slot* slot = reinterpret_cast<const Slot*>(kg.slot);
    if (q0 + qi < kg.n_pairs) {
        const int64_t gp = (q0 + qi) * D + di;
        Slot g[NR > 0 ? NR : 1];
        if (NR > 0) {
#pragma unroll
            for (int s = 0; s < NR; ++s) g[s] = slot[(int64_t)min(s, kg.nseg - 1) * kg.P + gp];
        }
        const double4 pr = reinterpret_cast<const double4*>(kg.pairs)[q0 + qi];
        double L, len, ksum;
        sim_geo(p, kg.ugeo[di], pr.x, pr.y, pr.z, pr.w, L, len, ksum);
        double nsum = 0.0, hmax = -INFINITY;
        int32_t nh = 0, off = 0;
        double cost = (double)(p.N + 1) * L;
        X128 xc = {0, 0}, xn = {0, 0};
        uint32_t xf = 0;
        auto take = [&](const Slot& gs) {
            if constexpr (EX) {
                xc = x_add(xc, X128{gs.c_lo, gs.c_hi});
                xn = x_add(xn, X128{gs.n_lo, gs.n_hi});
                xf |= gs.cnt >> 16;
            } else {
                cost = cost + gs.cost;
                nsum = nsum + gs.psi;
            }
            hmax = fmax(hmax, (double)gs.hmax);
            nh += (int32_t)(gs.cnt & 255u);
            off += (int32_t)((gs.cnt >> 8) & 255u);
        };
        if (NR > 0) {
#pragma unroll
            for (int s = 0; s < NR; ++s) {
                if (s >= kg.nseg) break;
                take(g[s]);
            }
        } else {
            for (int s = 0; s < kg.nseg; ++s) {
                const Slot gs = slot[(int64_t)s * kg.P + gp];
                take(gs);
            }
        }
        if constexpr (EX) {  // one rounding per field, a true division
            cost = cost + x_result(xc, xf & 7u, e_phi) / (double)p.N;
            nsum = x_result(xn, (xf >> 3) & 7u, e_psi);
        }
        put_outputs(out, gp, bad, cost, L, len, ksum, nsum, p.altitude - hmax, nh, off, 0);
        s_cost[di * 64 + qi] = cost;
        s_len[di * 64 + qi] = len;
    }
    __syncthreads();
    put_selection(kg, bad, q0, t, s_cost, s_len, best_f, best_l);
}
template <int NR>
__global__ __launch_bounds__(1024) void k_h_final(KParams p, KGrp kg, KOut out,
                                                  int32_t* __restrict__ best_f,
                                                  int32_t* __restrict__ best_l) {
    h_final_wg<NR, false>(p, kg, out, best_f, best_l, 0, 0);
}
template <int NR>
__global__ __launch_bounds__(1024) void k_h_final_x(KParams p, KGrp kg, KOut out,
                                                    int32_t* __restrict__ best_f,
                                                    int32_t* __restrict__ best_l,
                                                    const int32_t* __restrict__ scale) {
    const int32_t e_phi = __builtin_amdgcn_readfirstlane(scale[0]);
    const int32_t e_psi = __builtin_amdgcn_readfirstlane(scale[1]);
    h_final_wg<NR, true>(p, kg, out, best_f, best_l, e_phi, e_psi);
}
