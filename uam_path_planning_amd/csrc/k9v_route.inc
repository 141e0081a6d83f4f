// k9v_route.inc -- K9v, the route seeds in the risk volume: cost-to-go field of a goal over the
// volume's voxels and the 3-D seed paths traced through it (include/uampath.h "Route seeds in
// the volume").  k_route3_cost, k_route3_mask, k_route3_init, k_route3_relax<TXY, TZ>,
// k_route3_next, k_route3_trace, and the __host__ __device__ pieces of the definition they share
// with uam_route3d_field_host / uam_route3d_paths_host.  K9's own helpers (k9_route.inc) are
// used where the definition is literally K9's: r9_inf, r9_dix, r9_diy, r9_weight.  The trace
// and the host Dijkstra are k9_route.inc's, written over the grid type: this file gives them
// KRoute3's overloads of the grid vocabulary.
// Included in the anonymous namespace of uampath.hip, after k9_route.inc.

constexpr int R9V_DIRS = 26;
constexpr int R9V_GOAL = 26;  // next at the goal voxel; also the bit of "the tile itself"

// the volume grid and the call's parameters, as the kernels and the host twins take them
struct KRoute3 {
    int32_t nx, ny, nz;
    double x0, y_top, dx, dy, inv_dx, inv_dy;
    double z0, dz, inv_dz;
    double len[8];  // step lengths by (dix != 0) | (diy != 0) << 1 | (diz != 0) << 2
    double lambda, agl, kappa;
    uint32_t block_flags;
    int32_t inflate;
    static constexpr int D = 3;            // coordinates of a point
    static constexpr int GOAL = R9V_GOAL;  // next at the goal's voxel
};

// direction k = 0..25: K9's eight with diz = 0, the same with diz = +1, with diz = -1, up, down
__host__ __device__ __forceinline__ int r9v_dix(int k) { return k < 24 ? r9_dix(k & 7) : 0; }
__host__ __device__ __forceinline__ int r9v_diy(int k) { return k < 24 ? r9_diy(k & 7) : 0; }
__host__ __device__ __forceinline__ int r9v_diz(int k) {
    return k < 8 ? 0 : k < 16 ? 1 : k < 24 ? -1 : k == 24 ? 1 : -1;
}
__host__ __device__ __forceinline__ int r9v_len_index(int k) {
    return (r9v_dix(k) ? 1 : 0) | (r9v_diy(k) ? 2 : 0) | (r9v_diz(k) ? 4 : 0);
}

__host__ __device__ __forceinline__ void r9v_set_lengths(KRoute3* g) {
    const double vz = g->dz * g->kappa;
    for (int m = 0; m < 8; ++m) {
        const double hx = (m & 1) ? g->dx : 0.0, hy = (m & 2) ? g->dy : 0.0,
                     hz = (m & 4) ? vz : 0.0;
        g->len[m] = sqrt((hx * hx + hy * hy) + hz * hz);
    }
}

__host__ __device__ __forceinline__ int64_t r9v_voxels(const KRoute3& g) {
    return (int64_t)g.nx * g.ny * g.nz;
}
__host__ __device__ __forceinline__ int32_t r9v_index(const KRoute3& g, int ix, int iy, int iz) {
    return (iy * g.nx + ix) * g.nz + iz;
}

// voxel of a point by uam_volume_desc's rule; -1 outside the volume (a NaN coordinate is)
__host__ __device__ __forceinline__ int32_t r9v_voxel(const KRoute3& g, double x, double y,
                                                      double z) {
    const double fx = floor((x - g.x0) * g.inv_dx);
    const double fy = floor((g.y_top - y) * g.inv_dy);
    const double fz = floor((z - g.z0) * g.inv_dz);
    if (!((fx >= 0.0) && (fx < (double)g.nx) && (fy >= 0.0) && (fy < (double)g.ny) &&
          (fz >= 0.0) && (fz < (double)g.nz)))
        return -1;
    return r9v_index(g, (int32_t)fx, (int32_t)fy, (int32_t)fz);
}

// c_v of one voxel {risk, psi} in the column {terrain, flags}, +inf for a blocked0 voxel
__host__ __device__ __forceinline__ double r9v_cost0(const KRoute3& g, const uint2& vox,
                                                     const uint2& col, int iz) {
    const float risk = __builtin_bit_cast(float, vox.x);
    const float terrain = __builtin_bit_cast(float, col.x);
    const double c = 1.0 + g.lambda * (double)risk;
    const double hc = g.z0 + ((double)iz + 0.5) * g.dz;
    const bool below = hc < (double)terrain + g.agl;
    const bool free0 = !(col.y & g.block_flags) && (c > 0.0) && (c < r9_inf()) && !below;
    return free0 ? c : r9_inf();
}

// c_v with the inflation folded in: +inf when a blocked0 voxel of the same layer lies within
// Chebyshev distance inflate in x/y (voxels outside the volume do not count)
__host__ __device__ __forceinline__ double r9v_cost(const KRoute3& g, const uint2* vox,
                                                    const uint2* col, int ix, int iy, int iz) {
    const double own =
        r9v_cost0(g, vox[r9v_index(g, ix, iy, iz)], col[(int64_t)iy * g.nx + ix], iz);
    if (!(own < r9_inf())) return own;
    const int xa = ix - g.inflate > 0 ? ix - g.inflate : 0;
    const int xb = ix + g.inflate < g.nx - 1 ? ix + g.inflate : g.nx - 1;
    const int ya = iy - g.inflate > 0 ? iy - g.inflate : 0;
    const int yb = iy + g.inflate < g.ny - 1 ? iy + g.inflate : g.ny - 1;
    for (int y = ya; y <= yb; ++y)
        for (int x = xa; x <= xb; ++x)
            if (!(r9v_cost0(g, vox[r9v_index(g, x, y, iz)], col[(int64_t)y * g.nx + x], iz) <
                  r9_inf()))
                return r9_inf();
    return own;
}

// the admissible directions of voxel (ix, iy, iz) on the cost plane c: bit k set when the
// neighbour in direction k is inside the volume and every voxel of the axis-aligned box the two
// span (2, 4 or 8 voxels) is free; 0 for a blocked voxel
__host__ __device__ __forceinline__ uint32_t r9v_mask(const KRoute3& g, const double* c, int ix,
                                                      int iy, int iz) {
    if (!(c[r9v_index(g, ix, iy, iz)] < r9_inf())) return 0u;
    uint32_t m = 0u;
    for (int k = 0; k < R9V_DIRS; ++k) {
        const int dx = r9v_dix(k), dy = r9v_diy(k), dz = r9v_diz(k);
        const int ux = ix + dx, uy = iy + dy, uz = iz + dz;
        if (ux < 0 || ux >= g.nx || uy < 0 || uy >= g.ny || uz < 0 || uz >= g.nz) continue;
        bool ok = true;
        for (int bz = 0; bz <= (dz ? 1 : 0); ++bz)
            for (int by = 0; by <= (dy ? 1 : 0); ++by)
                for (int bx = 0; bx <= (dx ? 1 : 0); ++bx)
                    ok = ok && (c[r9v_index(g, ix + bx * dx, iy + by * dy, iz + bz * dz)] <
                                r9_inf());
        if (ok) m |= 1u << k;
    }
    return m;
}

// fl(dist[u_k] + w(u_k, v)) for the neighbour of voxel v in direction k, v's mask bit k set
__host__ __device__ __forceinline__ double r9v_candidate(const KRoute3& g, const double* c,
                                                         const double* dist, int32_t v, double cv,
                                                         int k) {
    const int32_t u = v + (r9v_diy(k) * g.nx + r9v_dix(k)) * g.nz + r9v_diz(k);
    return dist[u] + r9_weight(c[u], cv, g.len[r9v_len_index(k)]);
}

// next hop of a voxel after convergence
__host__ __device__ __forceinline__ uint8_t r9v_next(const KRoute3& g, const double* c,
                                                     const uint32_t* mask, const double* dist,
                                                     int32_t v, int32_t gvox) {
    const double dv = dist[v];
    if (!(dv < r9_inf())) return 255;
    if (v == gvox) return R9V_GOAL;
    const double cv = c[v];
    const uint32_t m = mask[v];
    for (int k = 0; k < R9V_DIRS; ++k)
        if ((m >> k & 1u) && r9v_candidate(g, c, dist, v, cv, k) == dv) return (uint8_t)k;
    return 255;  // not at a fixed point (cannot happen after convergence)
}

// ---- the grid vocabulary (k9_route.inc) -----------------------------------------------------
__host__ __device__ __forceinline__ int64_t r9_count(const KRoute3& g) { return r9v_voxels(g); }
__host__ __device__ __forceinline__ int32_t r9_locate(const KRoute3& g, const double* p) {
    return r9v_voxel(g, p[0], p[1], p[2]);
}
// one step of the chain from vox in direction k (count voxels visited so far): 1 = moved, -1 =
// the walk left the field (more than nx*ny*nz voxels, or a next value that is no direction or
// leads outside the volume: not a field of uam_route3d_field)
__host__ __device__ __forceinline__ int r9_hop(const KRoute3& g, int k, int32_t* vox,
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
__host__ __device__ __forceinline__ void r9_centre(const KRoute3& g, int32_t vox, double* p) {
    const int32_t col = vox / g.nz;
    p[0] = g.x0 + ((double)(col % g.nx) + 0.5) * g.dx;
    p[1] = g.y_top - ((double)(col / g.nx) + 0.5) * g.dy;
    p[2] = g.z0 + ((double)(vox % g.nz) + 0.5) * g.dz;
}
__host__ __device__ __forceinline__ double r9_seg(const KRoute3& g, const double* a,
                                                  const double* b) {
    const double ex = b[0] - a[0], ey = b[1] - a[1], ez = (b[2] - a[2]) * g.kappa;
    return sqrt((ex * ex + ey * ey) + ez * ez);
}
// the start's blocking as the trace reads it: from the volume's voxels and columns
struct R9vVolume {
    const uint2 *vox, *col;
};
__host__ __device__ __forceinline__ bool r9_start_blocked(const KRoute3& g, R9vVolume v,
                                                          int32_t vox) {
    const int c2 = vox / g.nz;
    return !(r9v_cost(g, v.vox, v.col, c2 % g.nx, c2 / g.nx, vox % g.nz) < r9_inf());
}

// ---- kernels --------------------------------------------------------------------------------
// the cost plane of a call, shared by all its goals: c [ny][nx][nz] f64, +inf = blocked
__global__ __launch_bounds__(R9_THREADS) void k_route3_cost(const uint2* __restrict__ vox,
                                                            const uint2* __restrict__ col,
                                                            KRoute3 g, double* __restrict__ c) {
    const int64_t n = r9v_voxels(g);
    for (int64_t i = (int64_t)blockIdx.x * R9_THREADS + threadIdx.x; i < n;
         i += (int64_t)gridDim.x * R9_THREADS) {
        const int64_t c2 = i / g.nz;
        c[i] = r9v_cost(g, vox, col, (int)(c2 % g.nx), (int)(c2 / g.nx), (int)(i % g.nz));
    }
}

// the admissible-direction masks of the finished cost plane: the box rule as one bit test
__global__ __launch_bounds__(R9_THREADS) void k_route3_mask(const double* __restrict__ c,
                                                            KRoute3 g,
                                                            uint32_t* __restrict__ mask) {
    const int64_t n = r9v_voxels(g);
    for (int64_t i = (int64_t)blockIdx.x * R9_THREADS + threadIdx.x; i < n;
         i += (int64_t)gridDim.x * R9_THREADS) {
        const int64_t c2 = i / g.nz;
        mask[i] = r9v_mask(g, c, (int)(c2 % g.nx), (int)(c2 / g.nx), (int)(i % g.nz));
    }
}

// One goal's start state: dist = +inf but 0 at the free goal voxel, both tile-flag planes
// cleared, and the first active list: the goal's tile, or nothing when the goal is outside the
// volume or blocked.  Tile (tx, ty, tz) has the index (ty*ntx + tx)*ntz + tz.
__global__ __launch_bounds__(R9_THREADS) void k_route3_init(
    const double* __restrict__ c, KRoute3 g, const double* __restrict__ goal,
    double* __restrict__ dist, int txy, int tz, int ntx, int ntz, int ntiles,
    uint32_t* __restrict__ flags, int32_t* __restrict__ lists, int32_t* __restrict__ ctl) {
    const int64_t n = r9v_voxels(g);
    int32_t gvox = r9v_voxel(g, goal[0], goal[1], goal[2]);
    if (gvox >= 0 && !(c[gvox] < r9_inf())) gvox = -1;
    const int64_t i0 = (int64_t)blockIdx.x * R9_THREADS + threadIdx.x;
    const int64_t step = (int64_t)gridDim.x * R9_THREADS;
    for (int64_t i = i0; i < n; i += step) dist[i] = i == gvox ? 0.0 : r9_inf();
    for (int64_t i = i0; i < 2 * (int64_t)ntiles; i += step) flags[i] = 0u;
    if (i0 == 0) {
        ctl[0] = gvox >= 0 ? 1 : 0;
        ctl[1] = 0;
        if (gvox >= 0) {
            const int c2 = gvox / g.nz;
            lists[0] = (((c2 / g.nx) / txy) * ntx + (c2 % g.nx) / txy) * ntz + (gvox % g.nz) / tz;
        }
    }
}

// A round of the label-correcting relaxation, K9's scheme on TXY x TXY x TZ voxels: workgroup b
// takes tile list_cur[b], loads its dist and c with a one-voxel halo on all six sides into LDS
// (z fastest, as in memory) and the masks of its own voxels into registers, and runs up to
// `inner` pull sweeps (every voxel takes the min over its admissible neighbours of dist[u] + w;
// a sweep reads, a barrier, then writes), stopping when a sweep changes nothing.  It writes the
// changed voxels back and enters into the next round's list (once: flag_nxt) itself when its
// last sweep still changed something, and each of its up to 26 neighbour tiles toward which a
// voxel of the face, edge or corner on that side decreased.  dist only ever decreases and only
// this workgroup writes the tile's voxels; a halo value read while the neighbour's workgroup
// lowers it is the old or the new one (8-B relaxed atomic accesses), and that neighbour enters
// this tile into the next round, so no decrease is lost.  No waiting on another workgroup.
template <int TXY, int TZ>
__global__ __launch_bounds__(R9_THREADS) void k_route3_relax(
    const double* __restrict__ c, const uint32_t* __restrict__ mask, double* __restrict__ dist,
    KRoute3 g, int ntx, int nty, int ntz, const int32_t* __restrict__ list_cur,
    uint32_t* __restrict__ flag_cur, uint32_t* __restrict__ flag_nxt,
    int32_t* __restrict__ list_nxt, int32_t* __restrict__ ctl, int cur, int inner) {
    extern __shared__ double r9v_lds[];
    constexpr int SX = TXY + 2, SZ = TZ + 2;
    constexpr int HALO = SX * SX * SZ;
    constexpr int VPT = TXY * TXY * TZ / R9_THREADS;  // voxels per lane
    static_assert(VPT >= 1 && VPT * R9_THREADS == TXY * TXY * TZ, "whole voxels per lane");
    double* sd = r9v_lds;
    double* sc = r9v_lds + HALO;
    __shared__ uint32_t s_mask;
    const int tid = threadIdx.x;
    const int tile = list_cur[blockIdx.x];
    const int tz = tile % ntz, tx = (tile / ntz) % ntx, ty = tile / (ntz * ntx);
    const int bx = tx * TXY, by = ty * TXY, bz = tz * TZ;
    if (tid == 0) {
        flag_cur[tile] = 0u;
        s_mask = 0u;
        if (blockIdx.x == 0) ctl[cur] = 0;
    }
    for (int e = tid; e < HALO; e += R9_THREADS) {
        const int gz = bz + e % SZ - 1, gx = bx + (e / SZ) % SX - 1, gy = by + e / (SZ * SX) - 1;
        double d = r9_inf(), cc = r9_inf();
        if (gx >= 0 && gx < g.nx && gy >= 0 && gy < g.ny && gz >= 0 && gz < g.nz) {
            const int32_t i = r9v_index(g, gx, gy, gz);
            cc = c[i];
            d = __hip_atomic_load(dist + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        sd[e] = d;
        sc[e] = cc;
    }
    // this lane's voxels: e = tid + q*256, lz = e % TZ, lx = (e / TZ) % TXY, ly = e / (TZ*TXY)
    uint32_t vm[VPT];
#pragma unroll
    for (int q = 0; q < VPT; ++q) {
        const int e = tid + q * R9_THREADS;
        const int gz = bz + e % TZ, gx = bx + (e / TZ) % TXY, gy = by + e / (TZ * TXY);
        vm[q] = (gx < g.nx && gy < g.ny && gz < g.nz) ? mask[r9v_index(g, gx, gy, gz)] : 0u;
    }
    __syncthreads();
    uint32_t dirty = 0u;
    int open = 0;  // the last sweep run changed something
    for (int it = 0; it < inner; ++it) {
        double nv[VPT];
        uint32_t ch = 0u;
#pragma unroll
        for (int q = 0; q < VPT; ++q) {
            const int e = tid + q * R9_THREADS;
            const int idx = ((e / (TZ * TXY) + 1) * SX + (e / TZ) % TXY + 1) * SZ + e % TZ + 1;
            const double dv = sd[idx];
            double best = dv;
            const uint32_t m = vm[q];
            if (m) {
                const double cv = sc[idx];
#pragma unroll
                for (int k = 0; k < R9V_DIRS; ++k)
                    if (m >> k & 1u) {
                        const int u = idx + (r9v_diy(k) * SX + r9v_dix(k)) * SZ + r9v_diz(k);
                        const double t = sd[u] + r9_weight(sc[u], cv, g.len[r9v_len_index(k)]);
                        best = t < best ? t : best;
                    }
            }
            nv[q] = best;
            if (best < dv) ch |= 1u << q;
        }
        open = __syncthreads_or((int)ch);  // also: every read of the sweep before its writes
        if (!open) break;
#pragma unroll
        for (int q = 0; q < VPT; ++q)
            if (ch >> q & 1u) {
                const int e = tid + q * R9_THREADS;
                sd[((e / (TZ * TXY) + 1) * SX + (e / TZ) % TXY + 1) * SZ + e % TZ + 1] = nv[q];
            }
        dirty |= ch;
        __syncthreads();
    }
    uint32_t bm = 0u;
#pragma unroll
    for (int q = 0; q < VPT; ++q)
        if (dirty >> q & 1u) {
            // a changed voxel is free, hence inside the volume
            const int e = tid + q * R9_THREADS;
            const int lz = e % TZ, lx = (e / TZ) % TXY, ly = e / (TZ * TXY);
            __hip_atomic_store(dist + r9v_index(g, bx + lx, by + ly, bz + lz),
                               sd[((ly + 1) * SX + lx + 1) * SZ + lz + 1], __ATOMIC_RELAXED,
                               __HIP_MEMORY_SCOPE_AGENT);
#pragma unroll
            for (int k = 0; k < R9V_DIRS; ++k) {
                const int dx = r9v_dix(k), dy = r9v_diy(k), dz = r9v_diz(k);
                const bool on = (dx == 0 || lx == (dx > 0 ? TXY - 1 : 0)) &&
                                (dy == 0 || ly == (dy > 0 ? TXY - 1 : 0)) &&
                                (dz == 0 || lz == (dz > 0 ? TZ - 1 : 0));
                bm |= on ? 1u << k : 0u;
            }
        }
    if (bm) atomicOr(&s_mask, bm);
    __syncthreads();
    if (tid <= R9V_GOAL) {
        int t = -1;
        if (tid == R9V_GOAL) {
            if (open) t = tile;
        } else if (s_mask >> tid & 1u) {
            const int ux = tx + r9v_dix(tid), uy = ty + r9v_diy(tid), uz = tz + r9v_diz(tid);
            if (ux >= 0 && ux < ntx && uy >= 0 && uy < nty && uz >= 0 && uz < ntz)
                t = (uy * ntx + ux) * ntz + uz;
        }
        if (t >= 0 && atomicExch(flag_nxt + t, 1u) == 0u)
            list_nxt[atomicAdd(ctl + (cur ^ 1), 1)] = t;
    }
}

// the next hops of one goal's converged field
__global__ __launch_bounds__(R9_THREADS) void k_route3_next(const double* __restrict__ c,
                                                            const uint32_t* __restrict__ mask,
                                                            const double* __restrict__ dist,
                                                            KRoute3 g,
                                                            const double* __restrict__ goal,
                                                            uint8_t* __restrict__ next) {
    const int64_t n = r9v_voxels(g);
    const int32_t gvox = r9v_voxel(g, goal[0], goal[1], goal[2]);
    for (int64_t i = (int64_t)blockIdx.x * R9_THREADS + threadIdx.x; i < n;
         i += (int64_t)gridDim.x * R9_THREADS)
        next[i] = r9v_next(g, c, mask, dist, (int32_t)i, gvox);
}

// the seed paths: one lane per query, sequential
__global__ __launch_bounds__(R9_THREADS) void k_route3_trace(
    KRoute3 g, const uint2* __restrict__ vox, const uint2* __restrict__ col,
    const uint8_t* __restrict__ next, const double* __restrict__ goals, int32_t n_goals,
    const double* __restrict__ starts, const int32_t* __restrict__ goal_idx, int64_t n_queries,
    int32_t N, double* __restrict__ wp, int32_t* __restrict__ status,
    int32_t* __restrict__ steps) {
    const int64_t q = (int64_t)blockIdx.x * R9_THREADS + threadIdx.x;
    if (q < n_queries)
        r9_trace(g, R9vVolume{vox, col}, next, goals, n_goals, starts, goal_idx, q, N, wp, status,
                 steps);
}

// ---- host side ------------------------------------------------------------------------------
constexpr int R9V_TXY_MIN = 8, R9V_TZ_MIN = 4;
// workspace: the cost plane, the mask plane, then the two flag planes, the two lists (sized for
// the smallest tile) and the two counts
struct R9vWs {
    R9Ws field;  // K9's parts, at the volume's offsets; bytes is the whole workspace
    int64_t mask_off;
};
inline R9vWs r9v_workspace(const KRoute3& g) {
    const int64_t nt = (int64_t)r9_tiles(g.nx, R9V_TXY_MIN) * r9_tiles(g.ny, R9V_TXY_MIN) *
                       r9_tiles(g.nz, R9V_TZ_MIN);
    const int64_t n = r9v_voxels(g);
    R9vWs w;
    w.field.c_off = 0;
    w.mask_off = r9_al256(n * 8);
    w.field.flags_off = w.mask_off + r9_al256(n * 4);
    w.field.lists_off = w.field.flags_off + r9_al256(2 * nt * 4);
    w.field.ctl_off = w.field.lists_off + r9_al256(2 * nt * 4);
    w.field.bytes = w.field.ctl_off + 256;
    return w;
}

// one round: n workgroups over list `cur`, entering tiles into list cur ^ 1
template <int TXY, int TZ>
void route3_relax_launch(int n, hipStream_t s, const double* c, const uint32_t* mask, double* dist,
                         const KRoute3& g, int ntx, int nty, int ntz, uint32_t* flags,
                         int32_t* lists, int32_t* ctl, int cur, int inner) {
    const int nt = ntx * nty * ntz;
    const size_t lds = (size_t)2 * (TXY + 2) * (TXY + 2) * (TZ + 2) * sizeof(double);
    hipLaunchKernelGGL((k_route3_relax<TXY, TZ>), dim3(n), dim3(R9_THREADS), lds, s, c, mask, dist,
                       g, ntx, nty, ntz, lists + cur * nt, flags + cur * nt,
                       flags + (cur ^ 1) * nt, lists + (cur ^ 1) * nt, ctl, cur, inner);
}

// the host twin of the field: the cost plane by r9v_cost, the masks by r9v_mask, r9_dijkstra
// over r9_weight's edges, r9v_next
inline void r9v_field_host(const KRoute3& g, const uint2* vox, const uint2* col,
                           const double* goals, int32_t n_goals, double* dist, uint8_t* next) {
    const int64_t n = r9v_voxels(g);
    std::vector<double> c((size_t)n);
    std::vector<uint32_t> mask((size_t)n);
    for (int64_t i = 0; i < n; ++i) {
        const int64_t c2 = i / g.nz;
        c[(size_t)i] = r9v_cost(g, vox, col, (int)(c2 % g.nx), (int)(c2 / g.nx), (int)(i % g.nz));
    }
    for (int64_t i = 0; i < n; ++i) {
        const int64_t c2 = i / g.nz;
        mask[(size_t)i] =
            r9v_mask(g, c.data(), (int)(c2 % g.nx), (int)(c2 / g.nx), (int)(i % g.nz));
    }
    std::vector<std::pair<double, int32_t>> heap;
    for (int32_t gi = 0; gi < n_goals; ++gi) {
        double* d = dist + (int64_t)gi * n;
        uint8_t* nx = next + (int64_t)gi * n;
        for (int64_t i = 0; i < n; ++i) d[i] = r9_inf();
        int32_t gvox = r9v_voxel(g, goals[3 * gi], goals[3 * gi + 1], goals[3 * gi + 2]);
        if (gvox >= 0 && !(c[(size_t)gvox] < r9_inf())) gvox = -1;
        if (gvox >= 0) {
            d[gvox] = 0.0;
            heap.assign(1, {0.0, gvox});
            r9_dijkstra(heap, d, [&](int32_t u, auto visit) {
                const uint32_t m = mask[(size_t)u];
                for (int k = 0; k < R9V_DIRS; ++k) {
                    if (!(m >> k & 1u)) continue;
                    // the edge u -> v seen from v: v's neighbour in the opposite direction,
                    // whose weight is the same sum (r9_weight commutes)
                    const int32_t v = u + (r9v_diy(k) * g.nx + r9v_dix(k)) * g.nz + r9v_diz(k);
                    visit(v, d[u] + r9_weight(c[(size_t)u], c[(size_t)v],
                                              g.len[r9v_len_index(k)]));
                }
            });
        }
        for (int64_t i = 0; i < n; ++i)
            nx[i] = r9v_next(g, c.data(), mask.data(), d, (int32_t)i, gvox);
    }
}
