// gsort.inc -- the counting sort of the grouped forms (K2g / K2h on the raster, K4h / K4hp on
// the volume): its constants, the histogram launch k_sort_hist (one body; k_g_hist, k_v_hist and
// k_vp_hist are its instances) and the scatter launch k_g_scatter.  The scan between them is
// k_scan_local / k_scan_totals (uampath.hip, utilities).
// Included in the anonymous namespace of uampath.hip after k4hp.inc: the histogram seeds the
// paths through h_path_seed (uampath.hip) or v_path_seed (k4h.inc), so it stands after both;
// relies on KGrp, div_magic, arc_point and unit_geo_block (uampath.hip) and on KVol4, KProf,
// prof_of, vp_split and vz_at (k4h.inc).

constexpr int G_TBITS_MAX = 6;                          // up to 64 x 64 tiles over the raster
// tile bins twice over (K2g: a ragged last group's items have their own; K2h / K4h sort on one
// bin per tile and use half of them) + one for off-raster / NaN
constexpr int G_BINS_MAX = (2 << (2 * G_TBITS_MAX)) + 1;
constexpr int G_NBK = UAM_G_NBK;                        // partitions of the counting sort
constexpr int G_HIST_DYN_MAX = 119 * 1024;  // k_sort_hist's dynamic LDS (seeds) beside its 40 KiB
constexpr int G_MAXLEN = 64;                            // longest group
constexpr int G_UTAB_LDS = 48 * 1024;                   // K2g: unit-arc table (in LDS) up to this

// counting sort, launch 1: partition b = paths [P b / NBK, P (b+1) / NBK); keys of all their
// groups and the partition's histogram, stored bin-major so the scan yields each (bin,
// partition)'s offset; then the partition's paths' seeds, where the form has them.
// Grid: the raster's KRaster (K2g / K2h: the key is the tile under the group's middle waypoint;
// the seeds are K2h's terrain seeds, h_path_seed into kg.lbp) or the volume's KVol4 (K4h: the
// key is (altitude band, tile) of that waypoint; the seeds are the clearance seeds, v_path_seed
// into kg.ubp).  A trailing KProf (K4hp, the volume only): the waypoint's z by the table rule
// on the profile's own row (its three coefficients loaded with the batch), so the profiles of a
// lateral candidate that fly at different heights fall into different bands.
// The per-form statements stand under `if constexpr` in this body, not in a shared inlined
// function (DESIGN section 10: the evaluation kernels' registers moved that way).
template <class Grid, class... F>
__global__ __launch_bounds__(1024) void k_sort_hist(KParams p, Grid gs, KGrp kg, F... f) {
    constexpr bool VOL = std::is_same_v<Grid, KVol4>;
    constexpr bool PROF = sizeof...(F) != 0;
    static_assert(VOL || std::is_same_v<Grid, KRaster>, "the raster's or the volume's view");
    static_assert(sizeof...(F) <= (VOL ? 1 : 0), "at most one KProf, on the volume");
    [[maybe_unused]] const KProf kf = prof_of(f...);
    __shared__ __attribute__((aligned(16))) int32_t h[G_BINS_MAX];
    __shared__ uint16_t tk[1 << (2 * G_TBITS_MAX)];  // the tile-key table (curve order)
    // with kg.seed_lds: the packed header and the unit-arc table staged for the seeds
    extern __shared__ __attribute__((aligned(16))) uint32_t s_hist_dyn[];
    const int t = threadIdx.x, b = blockIdx.x;
    if (b == 0 && t == 0) *kg.err = 0;
    for (int k = t; k < kg.bins; k += 1024) h[k] = 0;
    for (int k = t; k < (1 << (2 * kg.tbits)); k += 1024) tk[k] = kg.tkey[k];
    const uint32_t* s_hdr;  // the packed header
    bool seeds;             // the form's seed array is there
    if constexpr (VOL) s_hdr = gs.hdr, seeds = kg.ubp != nullptr;
    else s_hdr = gs.pmap, seeds = kg.lbp != nullptr;
    const double2* s_ut = reinterpret_cast<const double2*>(kg.utab);
    if (seeds && kg.seed_lds) {
        uint4* dh = reinterpret_cast<uint4*>(s_hist_dyn);
        const uint4* gh = reinterpret_cast<const uint4*>(s_hdr);
        for (int k = t; k < (gs.hwords >> 2); k += 1024) dh[k] = gh[k];
        double2* du = reinterpret_cast<double2*>(s_hist_dyn + gs.hwords);
        for (int k = t; k < kg.D * p.N; k += 1024) du[k] = s_ut[k];
        s_hdr = s_hist_dyn;
        s_ut = du;
    }
    __syncthreads();
    // thread = item (consecutive threads: the groups of one path, then the next path's), so
    // the key stores are coalesced and a path's pair is one broadcast load; U items per thread
    // with all their loads issued first (indices clamped into the partition)
    const int64_t lo = ((int64_t)kg.P * b / G_NBK) * kg.nseg;
    const int64_t hi = ((int64_t)kg.P * (b + 1) / G_NBK) * kg.nseg;
    const int N = p.N, W = kg.W;
    [[maybe_unused]] const int tiles = 1 << (2 * kg.tbits);
    [[maybe_unused]] const double inv_w1 = 1.0 / (double)(W - 1);
    constexpr int U = 4;
    for (int64_t i0 = lo + t; i0 < hi; i0 += 1024 * U) {
        double ax[U], ay[U], bx[U], by[U];         // the pair's end points
        [[maybe_unused]] double za[U], zb[U];      // and altitudes
        [[maybe_unused]] double zc[U][3];          // the profile's coefficients at jm
        double2 u[U];
        int jm[U], sg[U];
#pragma unroll
        for (int k = 0; k < U; ++k) {
            const int32_t i = (int32_t)min(i0 + k * 1024, hi - 1);
            const int32_t path = (int32_t)div_magic((uint32_t)i, kg.m_nseg, kg.sh_nseg);
            sg[k] = (int)(i - (int64_t)path * kg.nseg);
            int32_t q, d;
            [[maybe_unused]] int32_t ap = 0;  // the profile
            if constexpr (PROF) {
                vp_split(kg, kf, path, q, d, ap);
            } else {
                q = (int32_t)div_magic((uint32_t)path, kg.m_d, kg.sh_d);
                d = path - q * kg.D;
            }
            const int j0 = sg[k] * kg.G, j1 = min(j0 + kg.G, W);
            jm[k] = (j0 + j1 - 1) >> 1;  // the group's middle waypoint
            if constexpr (VOL) {
                const double2* pp = reinterpret_cast<const double2*>(kg.pairs + (int64_t)q * 6);
                const double2 a = pp[0], b2 = pp[1], c = pp[2];
                ax[k] = a.x, ay[k] = a.y, za[k] = b2.x, bx[k] = b2.y, by[k] = c.x, zb[k] = c.y;
            } else {
                const double4 pr = reinterpret_cast<const double4*>(kg.pairs)[q];
                ax[k] = pr.x, ay[k] = pr.y, bx[k] = pr.z, by[k] = pr.w;
            }
            u[k] = reinterpret_cast<const double2*>(kg.utab)[d * N + min(max(jm[k] - 1, 0), N - 1)];
            if constexpr (PROF) {
                const double* zr = kf.ztab + ((int64_t)ap * W + jm[k]) * 3;
                zc[k][0] = zr[0], zc[k][1] = zr[1], zc[k][2] = zr[2];
            }
        }
#pragma unroll
        for (int k = 0; k < U; ++k) {
            const int64_t i = i0 + k * 1024;
            if (i >= hi) break;
            double x0, x1;  // PathSrc::at's point
            if (jm[k] == 0) {
                x0 = ax[k], x1 = ay[k];
            } else if (jm[k] == W - 1) {
                x0 = bx[k], x1 = by[k];
            } else {
                arc_point(ax[k], ay[k], bx[k], by[k], u[k].x, u[k].y, x0, x1);
            }
            // the key: the position of the point's tile of the 2^tbits x 2^tbits grid on the
            // tile curve (Hilbert by default: consecutive tiles always adjacent), on the volume
            // after its altitude band; bins - 1 outside the grid or NaN.  (tx, ty >= 0 there,
            // so the conversions truncate as gen_cell's floor does.)
            const double tx = (x0 - gs.x0) * gs.inv_dx, ty = (gs.y_top - x1) * gs.inv_dy;
            bool in = (tx >= 0.0) && (tx < (double)gs.nx) && (ty >= 0.0) && (ty < (double)gs.ny);
            [[maybe_unused]] double tz = 0.0;
            if constexpr (VOL) {
                // (the key only orders the items: j / (W-1) by a reciprocal is exact enough)
                double z;
                if constexpr (PROF) z = (za[k] * zc[k][0] + zb[k] * zc[k][1]) + zc[k][2];
                else z = vz_at(za[k], zb[k], (double)jm[k] * inv_w1);
                tz = (z - gs.z0) * gs.inv_dz;
                in = in && (tz >= 0.0) && (tz < (double)gs.nz);
            }
            uint32_t key = kg.bins - 1;
            if (in) {
                const uint32_t cx = (uint32_t)tx >> kg.tshift, cy = (uint32_t)ty >> kg.tshift;
                key = tk[(cy << kg.tbits) | cx];
                if constexpr (VOL) key += ((uint32_t)tz >> gs.zshift) * tiles;
                // kg.last_bin > 0 (K2g alone): a ragged last group's items in their own bins;
                // the waves then rarely mix group lengths, so k_g_eval's straight-line chunks
                // stay wave-uniform.  K2h and K4h set it to 0 (one bin per tile, or per tile
                // and band): h_item and k_v_eval run the wave's most chunks, mask every slot
                // past a lane's own group and pad their LDS rows by G + 16 slots, so a wave
                // may mix group lengths freely and the last groups' items stay among their
                // tile's other items.  The profile form never had the statement.
                if constexpr (!PROF)
                    if (sg[k] == kg.nseg - 1) key += kg.last_bin;
            }
            kg.key[i] = (uint16_t)key;
            atomicAdd(&h[key], 1);
        }
    }
    if (seeds) {  // the partition's paths' seeds, one thread per path
        const int64_t plo = (int64_t)kg.P * b / G_NBK, phi = (int64_t)kg.P * (b + 1) / G_NBK;
        for (int64_t pth = plo + t; pth < phi; pth += 1024) {
            const int32_t path = (int32_t)pth;
            if constexpr (VOL) kg.ubp[pth] = v_path_seed(p, gs, kg, path, s_hdr, s_ut, f...);
            else kg.lbp[pth] = h_path_seed(p, gs, kg, path, s_hdr, s_ut);
        }
    }
    __syncthreads();
    // the partition's count per bin, bin-major ([bin][partition]): k_scan_local's exclusive
    // scan of it is each (bin, partition)'s place, up to its scan block's total
    for (int k = t; k < kg.bins; k += 1024) kg.cnt[(int64_t)k * G_NBK + b] = h[k];
}
constexpr auto k_g_hist = k_sort_hist<KRaster>;
constexpr auto k_v_hist = k_sort_hist<KVol4>;
constexpr auto k_vp_hist = k_sort_hist<KVol4, KProf>;

// launch 3 (after k_scan_local over cnt; the scan blocks' totals are scanned here, or by
// k_scan_totals beyond 1024 of them): LDS cursors, items scattered; U keys per thread loaded
// before the first cursor update.  The order of the items inside a (bin, partition) run follows
// the LDS atomics: it only decides which lane evaluates an item, never what the item computes.
// (A two-launch form -- device-scope
// atomics on the bin totals in the histogram launch, their scan in this one -- ran the
// histogram 11 -> 34 us at cfg3: 256 partitions' atomics on each bin address serialise
// across the XCDs; profiles/r04/prof1.)
__global__ __launch_bounds__(1024) void k_g_scatter(KParams p, KGrp kg) {
    __shared__ __attribute__((aligned(16))) int32_t cur[G_BINS_MAX];
    __shared__ int32_t stot[1024];
    __shared__ int32_t wsum[16];
    const int t = threadIdx.x;
    // K2h / K4h: block 0 forms the unit rows through its LDS (dispatched first, so hidden under
    // the scatter); the partitions are the other blocks
    if (kg.ugeo && blockIdx.x == 0) {
        unit_geo_block(p, kg, reinterpret_cast<double2*>(cur), (int)sizeof(cur));
        return;
    }
    const int b = blockIdx.x - (kg.ugeo ? 1 : 0);
    if (kg.test_fault && b == 0 && t == 0) atomicOr(kg.err, 1);  // (UAM_OPT_TEST_SORT_FAULT)
    const int nsb = kg.nsb_raw;
    if (nsb > 0) {  // the scan's block totals, scanned here (replaces k_scan_totals' launch)
        const int32_t v = t < nsb ? kg.tot[t] : 0;
        const int lane = t & 63, wv = t >> 6;
        int32_t x = v;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int32_t y = __shfl_up(x, o, 64);
            if (lane >= o) x += y;
        }
        if (lane == 63) wsum[wv] = x;
        __syncthreads();
        int32_t woff = 0;
        for (int k = 0; k < wv; ++k) woff += wsum[k];
        stot[t] = woff + x - v;
        __syncthreads();
    }
    for (int k = t; k < kg.bins; k += 1024) {
        const int64_t c = (int64_t)k * G_NBK + b;
        const int sb = (int)(c / (256 * SCAN_ITEMS));
        cur[k] = kg.cnt[c] + (nsb > 0 ? stot[sb] : kg.tot[sb]);
    }
    __syncthreads();
    const int64_t lo = ((int64_t)kg.P * b / G_NBK) * kg.nseg;
    const int64_t hi = ((int64_t)kg.P * (b + 1) / G_NBK) * kg.nseg;
    constexpr int U = 8;
    for (int64_t i0 = lo + t; i0 < hi; i0 += 1024 * U) {
        uint16_t kk[U];
#pragma unroll
        for (int k = 0; k < U; ++k) kk[k] = kg.key[min(i0 + k * 1024, hi - 1)];
#pragma unroll
        for (int k = 0; k < U; ++k) {
            const int64_t i = i0 + k * 1024;
            if (i < hi) {
                const int32_t at = atomicAdd(&cur[kk[k]], 1);
                if ((uint32_t)at < (uint32_t)kg.n_items)
                    kg.order[at] = (int32_t)i;
                else
                    atomicOr(kg.err, 1);  // never in a consistent sort: poisons the outputs
            }
        }
    }
}
