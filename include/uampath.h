/*
 * uampath.h -- C ABI of libuampath.so, the MI355X (gfx950) batched candidate-path cost
 * evaluator for the uam_path_planning hot path.
 *
 * The reference (nomaporon/uam_path_planning) has no FFI: its boundary is the Python class
 * surface of geo_simulation_project/path_generation.  Each entry point below replaces one
 * reference call (file:line relative to /root/reference/geo_simulation_project/); the Python
 * package uam_path_planning_amd keeps those class names and binds these symbols with ctypes
 * (INTEGRATION.md shows the binding a maintainer would add).
 *
 *   uam_set_geometry     RegionMap.add_obstacles / new_region / add_shape(s)_to_region
 *                        (path_generation/region_map.py:14-56) + polygon()/ball()/square()
 *                        inequalities (polygon.py:7-143, ball.py:7-52, square.py:6-65)
 *   uam_set_params       Problem.params / set_weight / options (problem.py:12-34) and the
 *                        OpEn parameter vector p = [xs, xg, maxratio, maxalpha, e, w...]
 *                        (solver.py:60-78)
 *   uam_eval_points      Problem.get_total_penalty_function / get_penalty_function(region|None)
 *                        (problem.py:49-82), QuadraticObstacle.contains / Map.collides
 *                        (quadratic_obstacle.py:89-94, map.py:41-43)
 *   uam_eval_waypoints   Problem.get_cost (problem.py:38-44) + get_nonlincon (84-114) +
 *                        length_of (130-146), batched over paths
 *   uam_eval_generated   Main.run candidate loop (main.py:158-193) with Solver.create_x_init
 *                        (solver.py:103-136) fused on device
 *   uam_gen_paths        Solver.create_x_init (solver.py:103-136), batched
 *   uam_argmin           main.py:175-180 best-candidate selection
 *   uam_path_length      Problem.length_of (problem.py:130-146) for arbitrary point counts
 *   uam_raster_build     map_generation DataManager.load_dem_polygons_from_geotiff mask
 *                        (map_generation/data_manager.py:11-17) + the region / no-fly
 *                        penalty at every cell centre: the per-cell cost record the raster
 *                        mode gathers
 *   uam_dem_mosaic       the VRT tile mosaic (data/raw/nagasaki_geotiff/mergeLL.vrt:1-10)
 *
 * Conventions: all array pointers marked _dev are device pointers (hipMalloc'd or torch
 * CUDA tensors); the caller owns every buffer; the library never frees caller memory.
 * Streams are hipStream_t passed as void* (NULL = default stream).  Calls are asynchronous
 * on that stream except uam_set_geometry.  Every function returns UAM_OK (0) or a negative
 * status; uam_last_error() returns a thread-local message for the last failure.
 */
#ifndef UAMPATH_H
#define UAMPATH_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 2 (round 5): uam_eval_generated gained summary_dev / block / packed_dev and
 * uam_eval_generated3d packed_dev, and the _s / _p entry points were folded into them */
#define UAM_ABI_VERSION 2
#define UAM_MAX_REGIONS 16
#define UAM_RECORD_BYTES 16

enum {
    UAM_OK = 0,
    UAM_E_INVALID = -1, /* bad argument: the reference raises ValueError/AssertionError */
    UAM_E_HIP = -2,     /* HIP runtime failure */
    UAM_E_NOMEM = -3,
    UAM_E_STATE = -4,   /* call order: e.g. eval before set_geometry / set_params */
    UAM_E_VERSION = -5, /* abi_version field does not match UAM_ABI_VERSION */
    UAM_E_DEVICE = -6   /* a device-side consistency check of an earlier call failed: that
                           call's outputs were poisoned (uam_device_status) */
};

/* inequality kinds h(x) <= 0 (parameters p[0..5]) */
enum {
    UAM_INEQ_HALFPLANE = 0, /* polygon edge a->b: h = s*((by-ay)*(x0-ax) - (bx-ax)*(x1-ay));
                               p = {ax, ay, bx-ax, by-ay, s = -sgn, 0} (polygon.py:69-71,98) */
    UAM_INEQ_ELLIPSE = 1,   /* h = ((x0-c0)/r1)^2 + ((x1-c1)/r2)^2 - 1; p = {c0,c1,r1,r2,0,0} */
    UAM_INEQ_AXIS = 2       /* square side h = s*(x_k - c) - r; p = {k, c, r, s, 0, 0} */
};

enum { UAM_MODE_ANALYTIC = 0, UAM_MODE_RASTER = 1, UAM_MODE_VOLUME = 2 };

/* record flag bits (record = {float phi, float psi_nfz, float dem, uint32 flags}; a volume
 * column = {float terrain, uint32 flags}) */
enum { UAM_FLAG_NFZ = 1u, UAM_FLAG_MASK = 2u, UAM_FLAG_NODATA = 4u };

typedef struct uam_ctx uam_ctx;
typedef void* uam_stream; /* hipStream_t */

/* Host-side flat geometry.  Shapes: no-fly obstacles [0, n_obstacles) in add order, then
 * region shapes region-major; region r owns shapes [region_first[r], region_first[r+1]). */
typedef struct {
    uint32_t abi_version;
    int32_t n_ineq;
    const int32_t* ineq_kind;    /* [n_ineq] */
    const double* ineq_par;      /* [n_ineq][6] */
    int32_t n_shapes;
    const int32_t* shape_first;  /* [n_shapes] first inequality */
    const int32_t* shape_count;  /* [n_shapes] number of inequalities (>= 1) */
    const double* shape_center;  /* [n_shapes][2]; NaN => penalty not normalised */
    int32_t n_obstacles;
    int32_t n_regions;           /* <= UAM_MAX_REGIONS */
    const int32_t* region_first; /* [n_regions + 1] */
} uam_geometry;

/* Problem options + OpEn parameter vector. */
typedef struct {
    uint32_t abi_version;
    int32_t N;               /* interior waypoints; a path has W = N + 2 points */
    int32_t length_smooth;   /* problem.py:13-16 */
    int32_t penalty_smooth;
    int32_t obstacle_smooth;
    int32_t maxratio_smooth;
    int32_t quirk_length;    /* 1 = reference get_cost length term: y = [anchor, p_0..p_{N+1}],
                                first N+1 segments (drops p_N->p_{N+1}); 0 = all segments */
    int32_t anchor_mode;     /* 0: anchor = each path's p_0 (segment is 0); 1: anchor_x/y
                                (the map.x_start baked into a reference solver build) */
    double anchor_x, anchor_y;
    double maxratio, maxalpha, enlargement;
    double altitude;         /* cruise altitude for min-clearance (raster mode), metres */
    double weights[UAM_MAX_REGIONS];
} uam_params;

/* Raster geotransform (GeoTIFF convention: row 0 is the northern edge).
 * cell (ix, iy) covers x in [x0 + ix*dx, x0 + (ix+1)*dx), y in (y_top - (iy+1)*dy, y_top - iy*dy];
 * a point maps to ix = floor((x - x0) * (1/dx)), iy = floor((y_top - y) * (1/dy)) in float64. */
typedef struct {
    int32_t nx, ny;
    double x0, y_top, dx, dy;
    float nodata;          /* DEM nodata value (-9999 in the reference DEM) */
    float dem_threshold;   /* data_manager.py:11-17 mask: (dem == -9999) if thr == -9999 else
                              (dem > thr) */
} uam_raster_desc;

/* 3-D risk volume (BASELINE config 5; no reference counterpart; SURVEY §8(d)'s layout): the
 * raster's x/y grid times nz altitude layers [z0 + iz*dz, z0 + (iz+1)*dz) in metres,
 * iz = floor((z - z0) * (1/dz)).  One device buffer (uam_volume_shape): 8-B voxels
 * {float risk, float psi_nfz} [ny][nx][nz] (layer fastest), then at col_offset the 8-B column
 * plane {float terrain (+0 for nodata), uint32 flags} [ny][nx]. */
typedef struct {
    int32_t nx, ny, nz;
    double x0, y_top, dx, dy;
    double z0, dz;
} uam_volume_desc;

/* Per-path outputs (device pointers, any may be NULL).  Index p of a path. */
typedef struct {
    double* cost;          /* get_cost (problem.py:38-44) */
    double* length_q;      /* the length term inside get_cost (quirk per params) */
    double* length;        /* true polyline length, non-smooth (solver.py:49) */
    double* kin_sum;       /* sum of the 3N kinematic g rows (problem.py:100-107) */
    double* nfz_sum;       /* sum of the no-fly g rows (problem.py:109-112) */
    int32_t* nfz_hits;     /* waypoints inside a no-fly zone (Map.collides) */
    double* min_clearance; /* raster: altitude - max terrain over the waypoints; volume: min
                              over waypoints of (waypoint altitude - terrain); analytic NaN */
    int32_t* offmap;       /* raster: waypoints outside the raster */
    int32_t* cells;        /* [P][W] raster cell index iy*nx+ix, -1 off-raster (raster only) */
    double* g_rows;        /* [P][3N + n_obstacles*W] full get_nonlincon vector (analytic) */
    int32_t* best_fval_idx;   /* uam_eval_generated only: [Q] per pair, the displacement index
                                 the reference keeps as "Min fval result" (main.py:175-177) */
    int32_t* best_length_idx; /* [Q] "Min path length result" (main.py:178-180) */
    int32_t* below_terrain;   /* volume mode: waypoints whose altitude layer lies below the
                                 column's terrain */
} uam_path_outputs;

/* Batched refinement: the reference's OpEn ALM problem
 * min get_cost s.t. get_nonlincon in {0} (solver.py:82-93), solved per path by n_outer ALM
 * updates (y += c g; c = min(c rho, c_max) when sum g^2 > theta * previous; stop when
 * sqrt(sum g^2) <= delta) around up to n_inner L-BFGS steps (memory pairs, 0..8; 0 = steepest
 * descent) on L = f + sum (c/2)(g + y/c)^2 with Armijo backtracking, stopping when
 * |grad L| <= inner_tol.  First trial step: 1 (L-BFGS) or 2 * previous step (steepest),
 * capped so the waypoint move is <= max_step (km).  Definition: oracle/uam_oracle.c
 * orc_refine.  Needs penalty_smooth and obstacle_smooth. */
typedef struct {
    int32_t n_outer, n_inner, max_backtrack, memory;
    double c0, rho, c_max, alpha0, armijo, theta, max_step, inner_tol, delta;
    int32_t n_restart;       /* restarts of a path ending with sqrt(sum g^2) > delta (0: none):
                                the obstacle holding most interior waypoints has them moved
                                along the start-goal chord's normal to restart_margin km past
                                its boundary, multipliers and penalty reset; the attempt with
                                the smallest sum g^2 is returned (oracle refine_restart) */
    double restart_margin;
} uam_refine_params;

int uam_abi_version(void);
const char* uam_last_error(void);
int uam_device_count(int* n);

int uam_ctx_create(int device, uam_ctx** out);
void uam_ctx_destroy(uam_ctx* ctx);

/* Copies the geometry to the device (synchronous). */
int uam_set_geometry(uam_ctx* ctx, const uam_geometry* geom);
/* Stores params and computes per-shape normalisers psi(centre) on the device. */
int uam_set_params(uam_ctx* ctx, const uam_params* params, uam_stream stream);

/* Per point (pts_dev [n][2] f64): phi = total penalty, phi_regions [n][n_regions] weighted
 * region penalties, obs_norm = get_penalty_function(None), psi_raw = sum of raw obstacle psi
 * (constraint semantics), collide = Map.collides. */
int uam_eval_points(uam_ctx* ctx, const double* pts_dev, int64_t n, double* phi_dev,
                    double* phi_regions_dev, double* obs_norm_dev, double* psi_raw_dev,
                    int32_t* collide_dev, uam_stream stream);

/* K1: one 16-byte record per cell, row-major.  dem_dev [ny][nx] f32 (NULL = all zero). */
int uam_raster_build(uam_ctx* ctx, const uam_raster_desc* desc, const float* dem_dev,
                     void* rec_dev, uam_stream stream);

/* VRT mosaic: n_tiles tiles of th x tw f32 (tiles_dev [n_tiles][th][tw]) placed at
 * (xoff[t], yoff[t]) (DstRect) into dem_dev [ny][nx]; cells no tile covers keep their value. */
int uam_dem_mosaic(uam_ctx* ctx, const float* tiles_dev, int32_t n_tiles, int32_t th,
                   int32_t tw, const int32_t* xoff_dev, const int32_t* yoff_dev, float* dem_dev,
                   int32_t nx, int32_t ny, uam_stream stream);
/* The mosaic's source tiles (data_manager.py:11-17 over mergeLL.vrt:1-10; build-defined host
 * reader): n_tiles GeoTIFF files (classic little-endian TIFF, one Float32 band in strips, no
 * predictor, uncompressed or deflate), each th x tw, read on up to n_threads host threads
 * (0: the machine's, at most 16) into dst [n_tiles][th][tw] host memory -- page-locked for an
 * asynchronous copy to uam_dem_mosaic's tiles_dev.  A tile that cannot be read fails the call
 * (UAM_E_INVALID, its path in uam_last_error). */
int uam_read_tiles(const char* const* paths, int32_t n_tiles, int32_t th, int32_t tw, float* dst,
                   int32_t n_threads);
/* The same tiles straight into device memory tiles_dev [n_tiles][th][tw] (uam_dem_mosaic's
 * input): read on the thread pool in ~32 MiB chunks into two page-locked buffers the context
 * keeps, each chunk copied on stream while the next one is read.  Returns once the last copy
 * is enqueued (the buffers are reused after their copies complete). */
int uam_load_tiles(uam_ctx* ctx, const char* const* paths, int32_t n_tiles, int32_t th,
                   int32_t tw, float* tiles_dev, int32_t n_threads, uam_stream stream);

/* K4: pairs_dev [Q][4] (x0,y0,xf,yf), utab_dev [D][N][2] unit-arc table -> wp [Q*D][N+2][2]. */
int uam_gen_paths(uam_ctx* ctx, const double* pairs_dev, int64_t n_pairs,
                  const double* utab_dev, int32_t D, double* wp_dev, uam_stream stream);

/* K2 (raster) / K3 (analytic) over explicit waypoints wp_dev [P][N+2][2]. */
int uam_eval_waypoints(uam_ctx* ctx, int32_t mode, const uam_raster_desc* desc,
                       const void* rec_dev, const double* wp_dev, int64_t n_paths,
                       const uam_path_outputs* out, uam_stream stream);

/* K2/K3 with the candidate generator fused: path p = q*D + d.  Raster mode takes two optional
 * derived copies of rec, both built with the same block (uam_raster_summary /
 * uam_raster_pack, below; NULL = none; ignored in analytic mode): summary_dev, the gather-skip
 * bitmap the lane- and wave-per-path forms read, and packed_dev, the packed raster the sorted
 * forms read (K2h by default; without it the sorted batches run K2s on rec).  Every choice
 * gives the same outputs (uam_last_group names the sum order). */
int uam_eval_generated(uam_ctx* ctx, int32_t mode, const uam_raster_desc* desc,
                       const void* rec_dev, const uint32_t* summary_dev, int32_t block,
                       const void* packed_dev, const double* pairs_dev, int64_t n_pairs,
                       const double* utab_dev, int32_t D, const uam_path_outputs* out,
                       uam_stream stream);

/* K2 gather skip (build-defined; no reference counterpart; results unchanged).  A bitmap
 * summary of a record raster: one bit per block x block cells (blocks row-major, nby x nbx;
 * bit b in 32-bit word b / 32), set when every cell of the block has phi == +-0,
 * psi_nfz == +-0, no no-fly flag and a terrain that reads +0.0 (a nodata cell, or a dem value
 * of +0.0f).  K2 / K2s keep the bitmap in LDS and do not gather the records of waypoints in set
 * blocks: they add exactly nothing to cost, no-fly sum and hits, and +0.0 to the terrain
 * maximum, so every output stays bit-identical to uam_eval_generated.  block: a power of two in [1, 1024] with at most 65536 blocks, or 0 =
 * automatic (8, doubled until the blocks fit).  The bitmap holds ceil(nbx * nby / 32) words and
 * must be rebuilt whenever rec changes. */
int uam_raster_summary_shape(const uam_raster_desc* desc, int32_t block, int32_t* block_out,
                             int32_t* nbx, int32_t* nby);
int uam_raster_summary(uam_ctx* ctx, const uam_raster_desc* desc, const void* rec_dev,
                       int32_t block, uint32_t* summary_dev, uam_stream stream);
/* Packed raster (build-defined; no reference counterpart; results unchanged).  A derived copy
 * of rec for the sorted evaluations (K2h / K2g / K2s), 256-B aligned sections:
 *   header  the 2-bit code per summary block (16 per 32-bit word): 0 = every cell has
 *           phi == +-0, psi_nfz == +-0, no no-fly flag and terrain +0.0 as read (nothing to
 *           read); 1 = psi_nfz == +-0 and no flag (phi from the 4-B plane, or phi and terrain
 *           from the 8-B {phi, terrain} plane); 2 = no psi_nfz below zero (phi, |psi_nfz| and
 *           the flag from the 8-B plane); 3 = the 16-B record;
 *           then the terrain bounds: one u16 {ub code, lb code << 8} per bound block (the
 *           smallest power-of-two square of >= 8 cells giving <= 16384 blocks), and one float2
 *           {base, step} per superblock of 4 x 4 bound blocks; a bound decodes as
 *           base + (float)code * step (f32, step a power of two) and holds every cell's terrain
 *           as read (+0 on nodata); {NaN, NaN} where the superblock holds a non-finite terrain;
 *   scratch the bound blocks' {min, max} (float2 each) while packing;
 *   planes  phi (4 B) and the terrain as read (4 B) in 4 x 8-cell blocks (one 128-B line),
 *           {phi, |psi_nfz| | nfz << 31} (8 B) in the same blocks (two 128-B lines) and the
 *           16-B records (four lines), at one index for all four; then {phi, terrain} (8 B) in
 *           4 x 4-cell blocks (one line; K2h's code-1 entry): 40 B per cell in all.
 * K2h reads a waypoint's terrain only where its bound could still be the path's maximum (the
 * maximum is order-free, so min_clearance is unchanged bit for bit); K2g and K2s read it for
 * every waypoint.  K2h addresses the copy by 32-bit offsets: for a copy of 4 GiB or more (about
 * 10^4 x 10^4 cells) it stands aside and the batch runs K2g / K2s on the same copy (slower, same
 * outputs in their documented sum order); packing needs nx, ny < 2^24.  uam_raster_pack_shape
 * gives the bytes of the caller's buffer (4096^2: 640.2 MiB = 56 KiB of header + 128 KiB of
 * scratch + 640 MiB of planes; 8192^2: 2.5 GiB); block as
 * uam_raster_summary
 * (0 = automatic), and the same block must be passed to uam_eval_generated.  Rebuild the copy
 * whenever rec changes. */
int uam_raster_pack_shape(const uam_raster_desc* desc, int32_t block, int32_t* block_out,
                          int64_t* bytes);
int uam_raster_pack(uam_ctx* ctx, const uam_raster_desc* desc, const void* rec_dev,
                    int32_t block, void* packed_dev, uam_stream stream);
/* K5: per group of G consecutive values, the reference's selection rule (main.py:175-180):
 * compare sqrt(v) when take_sqrt (fval = sqrt(cost), solver.py:48), else v. */
int uam_argmin(uam_ctx* ctx, const double* values_dev, int64_t groups, int32_t G,
               int32_t take_sqrt, int32_t* best_dev, uam_stream stream);

/* length_of: pts_dev [n_paths][n_points][2]; sum of the first n_segments segment norms
 * (squared-after-sqrt when smooth). */
int uam_path_length(uam_ctx* ctx, const double* pts_dev, int64_t n_paths, int32_t n_points,
                    int32_t n_segments, int32_t smooth, double* out_dev, uam_stream stream);

/* Waits for stream, then reports uam_device_status (below). */
int uam_synchronize(uam_ctx* ctx, uam_stream stream);
/* Device-side errors.  The sorted forms (K2h / K2g / K4h) check on the device that their
 * counting sort is consistent (every item lands on one position of the order).  A call whose
 * check fails writes NaN to every floating-point output and -1 to every count and selection of
 * the whole batch, and sets a word in page-locked host memory (no copy is issued otherwise).
 * Once the failing call has completed on its stream, uam_device_status returns UAM_E_DEVICE
 * with the text in uam_last_error() and clears the word; UAM_OK otherwise.  uam_synchronize
 * and the next uam_eval_generated* call on ctx report it too (the reference's convention of
 * raising on a failed solve, path_generation/solver.py:22-38, 53-55). */
int uam_device_status(uam_ctx* ctx);

/* Bytes of the volume buffer (256-B aligned sections) and the column plane's byte offset. */
int uam_volume_shape(const uam_volume_desc* desc, int64_t* bytes, int64_t* col_offset);
/* Config 5: build the volume (vol_dev: uam_volume_shape bytes, 256-B aligned) from a 2-D record
 * raster with the same x/y grid (rec2d_dev): risk = phi * layer_w[iz] (f64 product rounded to
 * f32; layer_w_dev [nz] f64), psi_nfz of the column; the column plane holds the column's DEM
 * (+0 for nodata) and its NFZ / MASK / NODATA flags. */
int uam_volume_build(uam_ctx* ctx, const uam_volume_desc* desc, const void* rec2d_dev,
                     const double* layer_w_dev, void* vol_dev, uam_stream stream);
/* Config 5 path evaluation: pairs6_dev [Q][6] = (x0, y0, z0, xf, yf, zf) (km, km, m); x/y
 * candidates as uam_eval_generated, altitude z_j = z0 + (zf - z0) * (j / (N+1)); cost =
 * (N+1) L + sum_j risk(voxel_j) / N; min_clearance = min_j (z_j - terrain of the column);
 * below_terrain counts waypoints whose layer centre z0 + (iz + 0.5) dz lies below it.  D <= 16.
 * packed_dev (uam_volume_pack, below; NULL = none): batches of >= UAM_OPT_SORTED_MIN_PATHS
 * paths (maxratio_smooth off, no cells) run K4h on it -- the (path, group) items sorted on the
 * altitude band and x/y tile of their middle waypoint, grouped partial sums (UAM_OPT_GROUP),
 * the geometry terms in the similarity form (oracle orc_eval_generated_h mode 2;
 * uam_last_kernel "K4h+pack"); every other batch runs on vol_dev. */
int uam_eval_generated3d(uam_ctx* ctx, const uam_volume_desc* desc, const void* vol_dev,
                         const void* packed_dev, const double* pairs6_dev, int64_t n_pairs,
                         const double* utab_dev, int32_t D, const uam_path_outputs* out,
                         uam_stream stream);

/* ---- The volume over explicit 3-D waypoints and altitude-profile candidates -----------------
 * uam_eval_generated3d flies every candidate of a pair along the straight climb between the
 * pair's end altitudes.  The three calls below let the caller choose the altitudes: any 3-D
 * polyline (uam_eval_waypoints3d), or per lateral candidate a family of A altitude profiles
 * (uam_gen_paths3d writes their waypoints, uam_eval_generated3d_profiles evaluates them fused,
 * without the 24 W bytes per path the waypoints would take).  All three read vol_dev only (no
 * packed copy, no sum scale).
 *
 * The altitude-profile table ztab_dev [A][W][3] float64, W = N + 2, is caller-built data like
 * the unit-arc table.  Waypoint j of the pair (x0, y0, z0, xf, yf, zf) under profile a has
 *   z_j = (z0 * ztab[a][j][0] + zf * ztab[a][j][1]) + ztab[a][j][2]
 * -- two products, their sum, then the sum with the third coefficient, each rounded to float64
 * (no fused multiply-add).  Affine in the end altitudes: (1 - t, t, 0) with t = j / (N+1) is the
 * straight climb, (0, 0, h) an absolute altitude h, (1 - t, t, h) a lift of h above the chord.
 * ztab_dev == NULL is allowed only with A = 1 and means uam_eval_generated3d's own expression
 * z0 + (zf - z0) * ((double)j / (double)(N+1)), with its bits.  x/y are exactly uam_gen_paths'
 * points (the pair's end points at j = 0 and j = N+1).  Path index p = (q*D + d)*A + a;
 * candidate index within a pair c = d*A + a.  1 <= A <= 8, 1 <= D <= 16, fewer than 2^31 paths
 * (UAM_E_INVALID otherwise, and for ztab_dev == NULL with A != 1). */
int uam_gen_paths3d(uam_ctx* ctx, const double* pairs6_dev, int64_t n_pairs,
                    const double* utab_dev, int32_t D, const double* ztab_dev, int32_t A,
                    double* wp3_dev /* [Q*D*A][W][3] */, uam_stream stream);
/* The volume evaluation of explicit waypoints wp3_dev [P][W][3] = (x km, y km, z m): the oracle's
 * orc_eval_paths3d bit for bit.  cost = (N+1) L + sum_j risk(voxel_j) / N and nfz_sum, added
 * sequentially in waypoint order over the waypoints inside the volume (x, y and z); nfz_hits;
 * offmap counts the waypoints outside it; below_terrain as uam_eval_generated3d; min_clearance =
 * min over the waypoints inside the volume of z_j - terrain of the column, +inf when there is
 * none; cells [P][W] = the voxel index (iy nx + ix) nz + iz, -1 outside the volume (a volume of
 * 2^31 voxels or more is refused by the descriptor check, so every index fits).  The length term
 * L, length and the kinematic rows (length_q, length, kin_sum) are formed from x/y alone and
 * ignore altitude, exactly as in uam_eval_generated3d.  g_rows, best_fval_idx and
 * best_length_idx are not written.  Batches of up to UAM_OPT_WAVE_MAX_PATHS paths run wave per
 * path (uam_last_kernel "K4ew"), larger ones lane per path ("K4e"); same bits.
 * Failures, in order: an earlier call's device check; the context; UAM_OPT_EXACT_SUM_VOLUME on
 * (below); n_paths < 0 (0 returns UAM_OK); the descriptor; wp3_dev / vol_dev NULL; vol_dev not
 * 256-B aligned. */
int uam_eval_waypoints3d(uam_ctx* ctx, const uam_volume_desc* desc, const void* vol_dev,
                         const double* wp3_dev /* [P][W][3] (x km, y km, z m) */,
                         int64_t n_paths, const uam_path_outputs* out, uam_stream stream);
/* uam_eval_waypoints3d applied to uam_gen_paths3d's waypoints, bit for bit, in one kernel
 * (uam_last_kernel "K4p"): the A profiles of a lateral candidate share its x/y points, the
 * geometry terms and each waypoint's column.  best_fval_idx [Q] and best_length_idx [Q] are
 * uam_argmin's rule over the pair's D*A candidates in index order c (take_sqrt set for the cost,
 * unset for the length); they need the cost / length output respectively (UAM_E_INVALID
 * otherwise).  A length does not depend on the profile, so among the profiles of one
 * displacement the rule's first index wins: best_length_idx is a multiple of A unless the rule's
 * zero quirk applies (a length of exactly 0 is replaced by whatever follows it).  That holds for
 * this call only: under the vertical terms (uam_eval_generated3d_profiles_v, below) a length
 * depends on the profile, best_length_idx selects among all D*A candidates, and best_fval_idx
 * sees the climb through (N+1) L. */
int uam_eval_generated3d_profiles(uam_ctx* ctx, const uam_volume_desc* desc, const void* vol_dev,
                                  const double* pairs6_dev, int64_t n_pairs,
                                  const double* utab_dev, int32_t D, const double* ztab_dev,
                                  int32_t A, const uam_path_outputs* out, uam_stream stream);

/* ---- The vertical terms: 3-D length, turn and climb rows ------------------------------------
 * The two evaluations above form length_q, length and kin_sum from x/y alone, so a climb costs
 * nothing but the risk it flies through.  The _v calls below charge it.  uam_vertical is plain
 * data like uam_params:
 *   z_scale      kappa, km of path length per metre of altitude change (1e-3: isotropic);
 *   sin_climb    the largest climb per unit of 3-D path length, +inf = no limit;
 *   sin_descent  the same for descending.
 * For the waypoints p_j = (x_j, y_j, z_j), j = 0 .. N+1, with ls = length_smooth, ms =
 * maxratio_smooth, quirk = quirk_length and the anchor as in uam_params:
 *
 *   L = quirk ? 0 + anchor term : 0;  length = kin_sum = climb_sum = 0
 *   for j = 1 .. N+1:
 *     dx = x_j - x_{j-1};  dy = y_j - y_{j-1};  dz = (z_j - z_{j-1}) * kappa
 *     s  = ((0 + dx*dx) + dy*dy) + dz*dz;   n = sqrt(s)
 *     length += n;   if (!quirk || j <= N)  L += ls ? n*n : n
 *     nk = ms ? n*n : n
 *     if j >= 2:  dt = ((0 + pdx*dx) + pdy*dy) + pdz*dz;  (c1, c2, c3) = kin_row(pn, nk, dt);
 *                 kin_sum += c1;  kin_sum += c2;  kin_sum += c3
 *     cu = fmax(0, dz - sin_climb*n);   cd = fmax(0, (-dz) - sin_descent*n)
 *     climb_sum = (climb_sum + cu) + cd
 *     pdx, pdy, pdz, pn = dx, dy, dz, nk
 *
 * with kin_row(pn, nk, dt) = (fmax(0, nk - r*pn), fmax(0, pn/r - nk), fmax(0, mincos - dt/(pn*nk)))
 * as in the 2-D calls (r = maxratio, squared when ms; mincos = cos(maxalpha)).  The altitude
 * difference is taken first and scaled by one product.  The anchor term stays x/y only: the
 * anchor flies at p_0's altitude.  length_q = L, cost = (N+1) L + sum_j risk(voxel_j) / N as
 * before; the risk, no-fly, clearance, off-volume and below-terrain outputs do not change.
 * Every operation is rounded to float64, none is contracted.  fmax is C's: a NaN row counts 0;
 * only the sums are output, so the sign of a zero row cannot show.
 * With kappa = 0 and finite altitudes every output equals the call without _v bit for bit
 * (s + 0*0 = s, dt + 0 = dt) and climb_sum is +0. */
typedef struct {
    uint32_t abi_version;   /* UAM_ABI_VERSION */
    double z_scale;         /* km of path length per metre of altitude change; >= 0, finite */
    double sin_climb;       /* largest climb per unit of 3-D path length; >= 0, +inf = no limit */
    double sin_descent;     /* the same for descending */
} uam_vertical;

/* uam_eval_waypoints3d with the vertical terms (uam_last_kernel "K4e+v" / "K4ew+v", same bits;
 * uam_last_group 0).  climb_sum_dev [P] receives climb_sum (NULL: not wanted); uam_path_outputs
 * does not grow.  Failures as uam_eval_waypoints3d, in its order, with -- after
 * UAM_OPT_EXACT_SUM_VOLUME's refusal and before n_paths -- UAM_E_INVALID for vert == NULL,
 * UAM_E_VERSION for a wrong abi_version, UAM_E_INVALID for a NaN, negative or infinite z_scale
 * and for a NaN or negative sin_climb / sin_descent. */
int uam_eval_waypoints3d_v(uam_ctx* ctx, const uam_volume_desc* desc, const void* vol_dev,
                           const double* wp3_dev /* [P][W][3] (x km, y km, z m) */,
                           int64_t n_paths, const uam_vertical* vert,
                           const uam_path_outputs* out, double* climb_sum_dev /* [P] or NULL */,
                           uam_stream stream);
/* uam_eval_generated3d_profiles with the vertical terms: uam_eval_waypoints3d_v applied to
 * uam_gen_paths3d's waypoints, bit for bit, in one kernel (uam_last_kernel "K4p+v").  The A
 * profiles of a lateral candidate still share its x/y points and each waypoint's column, but no
 * longer the geometry terms.  Here a length does depend on the profile: best_length_idx selects
 * among all D*A candidates and need not be a multiple of A, and best_fval_idx sees the climb
 * through (N+1) L.  ztab_dev == NULL with A = 1 is the straight climb with the vertical terms
 * (uam_eval_generated3d itself has no such form).  Failures as uam_eval_generated3d_profiles,
 * with the checks of vert where uam_eval_waypoints3d_v has them. */
int uam_eval_generated3d_profiles_v(uam_ctx* ctx, const uam_volume_desc* desc,
                                    const void* vol_dev, const double* pairs6_dev,
                                    int64_t n_pairs, const double* utab_dev, int32_t D,
                                    const double* ztab_dev, int32_t A, const uam_vertical* vert,
                                    const uam_path_outputs* out,
                                    double* climb_sum_dev /* [Q*D*A] or NULL */,
                                    uam_stream stream);

/* The packed volume (K4h), 256-B aligned sections:
 *   header  a 2-bit code per 8 x 8 columns (0: risk, psi_nfz +-0 in every layer and no no-fly
 *           flag; 1: psi_nfz +-0 and no flag; 2: no psi_nfz below zero; 3: otherwise), then the
 *           column terrain's bounds in the packed raster's scheme (u16 per bound block of
 *           columns, float2 {base, step} per 4 x 4 bound blocks);
 *   scratch the bound blocks' {min, max} while packing;
 *   4-B risk per voxel in 4 x 8-column blocks of one layer, layer-major (code 1; index i4);
 *   the 4-B column terrain (+0 on nodata) in the same blocks (one layer);
 *   8-B {risk, |psi_nfz| | nfz << 31} per voxel at i4 (code 2);
 *   16-B voxels {float risk, float psi_nfz, float terrain, uint32 flags} in 4 x 2-column
 *   blocks of one layer (one 128-B line; code 3);
 *   8-B {risk, column terrain} voxels in 4 x 4-column blocks of one layer (the
 *   UAM_OPT_K4H_TERRAIN = 1 form's entry): 36 B per voxel + 4 B per column in all.
 * K4h addresses the copy by 32-bit offsets: it stands aside (the batch runs K4 on vol_dev) for a
 * copy of 4 GiB or more or a layer of 2^24 or more entries.
 * K4h reads a waypoint's terrain only where it could still decide min_clearance or
 * below_terrain (the outputs are unchanged bit for bit).  uam_volume_pack derives it from a
 * built volume (vol_dev); packed_dev holds uam_volume_packed_bytes bytes (2.25 GiB at
 * 1024^2 x 64), 256-B aligned.  The copy is not tracked: rebuild it (uam_volume_pack) after
 * any write to vol_dev, including uam_volume_build into the same buffer and uam_bcast_raster. */
int uam_volume_packed_bytes(const uam_volume_desc* desc, int64_t* bytes);
int uam_volume_pack(uam_ctx* ctx, const uam_volume_desc* desc, const void* vol_dev,
                    void* packed_dev, uam_stream stream);

/* ---- Raster broadcast over RCCL / xGMI (the reference has no
 * collective at all -- its only IPC is the solver's TCP socket, path_generation/solver.py:26-38).
 * The record raster (or volume) is built once and broadcast once; the candidate loop of
 * main.py:160-193 then shards by pair with no collective.  RCCL is loaded at run time
 * (librccl.so.1: the one torch already loaded, else the system's); these calls return
 * UAM_E_STATE when it is absent.
 *   multi-process (one process per GPU): rank 0 calls uam_comm_unique_id, the caller ships
 *   the 128 bytes to every rank (e.g. torch.distributed.broadcast_object_list), each rank calls
 *   uam_comm_init (collective: returns once all nranks joined), then uam_bcast_raster.
 *   single process, several GPUs: uam_bcast_raster_group (ncclCommInitAll over the contexts'
 *   devices + one grouped broadcast; the communicators stay with the contexts for later
 *   uam_bcast_raster calls).
 * Asynchronous on the stream(s) given, like every other entry point. */
#define UAM_COMM_ID_BYTES 128
int uam_comm_unique_id(uint8_t* id_out /* [UAM_COMM_ID_BYTES] */);
int uam_comm_init(uam_ctx* ctx, const uint8_t* id /* [UAM_COMM_ID_BYTES] */, int32_t nranks,
                  int32_t rank);
int uam_comm_destroy(uam_ctx* ctx);
int uam_bcast_raster(uam_ctx* ctx, void* buf_dev, int64_t bytes, int32_t root,
                     uam_stream stream);
int uam_bcast_raster_group(uam_ctx** ctxs, void** bufs_dev, int32_t n, int64_t bytes,
                           int32_t root, uam_stream* streams);

/* ---- Coordinate reference systems ------------------------------
 * Transverse Mercator on an ellipsoid (Krueger series to n^6, Karney 2011) between geographic
 * (lon, lat) degrees and plane (x = easting, y = northing) metres -- what pyproj's to_crs does
 * for EPSG:4612/6668 <-> EPSG:2443..2461 in the reference (map_generation/data_manager.py:24-26
 * and 84-85, path_generation/main.py:106-115).  Definition: oracle/uam_oracle.c tm_*. */
typedef struct {
    double a, f, k0, lat0_deg, lon0_deg, false_easting, false_northing;
} uam_tm_params;
/* GRS80 / k0 0.9999 / origin of Japan Plane Rectangular CS zone 1..19 (EPSG:2442 + zone). */
int uam_tm_jprcs(int32_t zone, uam_tm_params* out);
/* Batched transforms of interleaved device arrays [n][2]: lon,lat -> x,y and back. */
int uam_geo_to_plane(uam_ctx* ctx, const uam_tm_params* tm, const double* lonlat_dev,
                     int64_t n, double* xy_dev, uam_stream stream);
int uam_plane_to_geo(uam_ctx* ctx, const uam_tm_params* tm, const double* xy_dev, int64_t n,
                     double* lonlat_dev, uam_stream stream);
/* North-up geographic grid (the mergeLL.vrt mosaic, mergeLL.vrt:1-3): pixel (i, j) covers
 * lon in lon0 + [i, i+1) dlon, lat in lat_top - [j, j+1) dlat. */
typedef struct {
    int32_t nx, ny;
    double lon0, lat_top, dlon, dlat;
    float nodata;
    int32_t pad;
} uam_geo_grid_desc;
/* Reproject a geographic DEM onto the plane raster grid dst (units of dst: unit_m metres):
 * each output cell centre -> inverse TM -> source pixel; resample 0 = nearest, 1 = bilinear
 * when all four neighbours are valid (else nearest); outside / nodata -> src nodata. */
int uam_reproject_dem(uam_ctx* ctx, const uam_tm_params* tm, const float* src_dev,
                      const uam_geo_grid_desc* src, const uam_raster_desc* dst, double unit_m,
                      int32_t resample, float* dst_dev, uam_stream stream);

/* ---- Land / populated-area polygons --------------------------------
 * DataProcessor(min_area, large_area, divisions, min_approx_polygon_area) of
 * map_generation/data_processor.py:9-13 (defaults 750000 m^2, 32000000 m^2, 5, 780000 m^2). */
typedef struct {
    double min_area, large_area, min_approx_area;
    int32_t divisions, pad;
} uam_polyproc_params;
/* DataProcessor.process_polygons (data_processor.py:15-75) on polygons in plane metres (host):
 * unary_union (inputs must have disjoint interiors; shared boundaries merge), area filter,
 * divisions^2 split of large polygons, cv2.minAreaRect + boxPoints + np.intp per polygon /
 * piece, final area filter.  Rings: ring r = xy[ring_start[r] .. ring_start[r+1]) (open or
 * closed), ring_hole[r] != 0 for holes.  Output: *n_rects rectangles, rect_xy[r][4][2]
 * integer metres in cv2.boxPoints order (at most max_rects written; more -> UAM_E_INVALID
 * with *n_rects set).  Definition: oracle/uam_oracle.c orc_process_polygons. */
int uam_process_polygons(const double* xy, const int64_t* ring_start, int32_t n_rings,
                         const int32_t* ring_hole, const uam_polyproc_params* params,
                         int64_t* rect_xy, int32_t max_rects, int32_t* n_rects);

/* The DEM route (DataManager.load_dem_polygons_from_geotiff + process_polygons,
 * map_generation/main.py:27-35): mask (dem == -9999 if threshold == -9999 else
 * dem > threshold, data_manager.py:14-17) -> 4-connected regions (rasterio.features.shapes)
 * labelled on the GPU -> the same approximation as uam_process_polygons, with pixel corners
 * at x0 + i dx, y_top - j dy (times unit_m metres).  Large regions are split into their box
 * pieces by a second labelling on the grid refined at the box edges.  Output as
 * uam_process_polygons (regions in raster order of their first cell).  Definition:
 * oracle/uam_oracle.c orc_dem_polygons.  Work is enqueued on `stream` and, for the large
 * regions, on up to 3 side streams the context owns (UAM_OPT_K8_STREAMS, 1-8, 4 in all);
 * the call synchronises all of them before it returns. */
int uam_dem_polygons(uam_ctx* ctx, const float* dem_dev, const uam_raster_desc* desc,
                     float threshold, double unit_m, const uam_polyproc_params* params,
                     int64_t* rect_xy, int32_t max_rects, int32_t* n_rects, uam_stream stream);

/* Measurement (bench.py's roofline; build-defined).  uam_kernel_timing(ctx, 1) resets and
 * starts timing, 0 stops it: while on, the context records a HIP event pair on the launch
 * stream around every timed path evaluation of uam_eval_generated* -- around the whole launch
 * sequence of K2g and K2s (sorts, evaluation, output launch; K2s's side-stream sorts are
 * joined inside it), around the k_eval_pairs / k_eval_wave launch of the other forms (excluding
 * their pair order and selection launches).  uam_kernel_time waits for those events and returns
 * the summed time and the count since the last call (then resets both).  Every 4096 timed
 * calls the pending pairs are folded into a running total (the timed call waits for the last
 * of them once), so any number of calls may pass between queries. */
int uam_kernel_timing(uam_ctx* ctx, int32_t enable);
int uam_kernel_time(uam_ctx* ctx, double* ms_total, int64_t* launches);
/* The path evaluation the last uam_eval_generated* / uam_eval_waypoints3d call on ctx ran: "K2h+pack" (segment-grouped
 * raster with the similarity-form geometry, the default for packed rasters and batches >=
 * UAM_OPT_SORTED_MIN_PATHS paths), "K2g+pack" (the same with per-segment geometry:
 * UAM_OPT_K2G_SIM = 0 or maxratio_smooth), "K4h+pack" (the packed volume, K2h's form),
 * "K2hx+pack" / "K4hx+pack" (their exact-sum forms, UAM_OPT_EXACT_SUM / _VOLUME),
 * "K2s+pack" / "K2s+skip" / "K2s" (segment-sorted raster, sequential sums), "K2+skip" / "K2"
 * (lane per path), "K2w" (wave per path), "K2d" (D > 16), "K3b", "K3", "K3d", "K4", "K4w";
 * "K4e" / "K4ew" (uam_eval_waypoints3d lane / wave per path), "K4p"
 * (uam_eval_generated3d_profiles), "K4e+v" / "K4ew+v" / "K4p+v" (their _v forms with the
 * vertical terms); "K9" (uam_route_field) / "K9t" (uam_route_paths) / "K9b"
 * (uam_route_free_bits) / "K9s" (uam_route_paths_smooth); "K9v" (uam_route3d_field) / "K9vt"
 * (uam_route3d_paths) / "K9vb" (uam_route3d_free_bits) / "K9vs" (uam_route3d_paths_smooth);
 * "K9vj" (uam_route3d_field_joint) / "K9vjt" / "K9vjs" (uam_route3d_paths_joint, span 0 / span
 * >= 1); "" before the first call.
 * The string is static (never freed).  For benchmarks and tests:
 * which kernel a number belongs to. */
const char* uam_last_kernel(const uam_ctx* ctx);

/* Waypoint-group length of the per-path sums of the last uam_eval_generated* call on ctx: G > 0
 * when a segment-grouped evaluation ran -- K2g: cost, length_q, length, kin_sum and nfz_sum
 * formed as per-group partial sums, each term attached to a waypoint of the group
 * [kG, (k+1)G), added in group order (oracle/uam_oracle.c orc_eval_paths_g); K2h / K4h: the
 * raster (volume) terms of cost and nfz_sum so, length_q / length / kin_sum in the similarity
 * form (orc_eval_generated_h) -- 0 for the reference's sequential order (problem.py:38-44,
 * 84-114, 130-146).
 * Tolerance against the sequential order: rounding only.  Measured: <= 8.2e-14 relative on
 * cost and 4.4e-14 on length over the whole cfg3 batch (500k paths), <= 1e-12 on every test
 * map, against the north_star's 1e-5; the selections (best_fval_idx, best_length_idx) agreed
 * on all 100k cfg3 pairs (bench.py parity.vs_sequential_order) -- they can differ only where
 * two candidates of a pair are within that rounding of each other.  A caller that needs the
 * sequential bits sets UAM_OPT_GROUP = 0 (K2s / K4).  uam_eval_waypoints3d and
 * uam_eval_generated3d_profiles (K4e / K4ew / K4p) and their _v forms always add sequentially:
 * they report 0. */
int32_t uam_last_group(const uam_ctx* ctx);

/* Context options: which kernel form runs (results never depend on them, except for the sum
 * order UAM_OPT_GROUP selects, which uam_last_group reports).  Read by the calls that follow.
 *   UAM_OPT_GROUP                K2g waypoints per group, 1..64 (default 21); 0 = no K2g (the
 *                                raster batches it takes run K2s: the reference's sum order)
 *   UAM_OPT_SORTED_MIN_PATHS     smallest raster batch (paths) the sorted forms K2g / K2s take
 *                                (default 65536; smaller batches run K2 / K2w)
 *   UAM_OPT_K2S_SEGMENTS         K2s segments per path, 2..8 (default 2)
 *   UAM_OPT_WAVE_MAX_PATHS       batches of up to this many paths run one wave per path (K2w /
 *                                K4w; default 16384; 0 = never)
 *   UAM_OPT_PAIR_ORDER           1 (default): batches of >= 4096 pairs through the lane-per-path
 *                                kernels in a spatial pair order; 0: in index order
 *   UAM_OPT_K1_ROWS              raster build: cells (rows) per lane, 1, 2 (default), 4, 8
 *   UAM_OPT_K3B_SEGMENT          analytic K3b: waypoints sorted together, 2/4/6/8 (default)/16;
 *                                0 = the lane-per-path K3
 *   UAM_OPT_K3B_POINTS_PER_LANE  analytic K3b evaluation phase: 1 (default) or 2
 *   UAM_OPT_K8_TILED             DEM polygons: 1 (default) tile labelling in LDS, 0 cell-parallel
 *   UAM_OPT_K8_STREAMS           DEM polygons: streams the large regions spread over, 1..8 (4)
 *   UAM_OPT_K2G_TILE_BITS        K2g sort key: 2^b x 2^b tiles over the raster, b = 3..6; 0
 *                                (default) = tiles of ~256 x 256 cells, coarser for batches
 *                                whose sort counts would exceed half their (path, group) items
 *   UAM_OPT_K2G_LDS_FLOOR        K2g / K2h / K4h evaluation: dynamic-LDS floor per workgroup in
 *                                bytes, which caps the workgroups resident per CU; 0 (default):
 *                                none for K2g and K2h (512-item workgroups, 2 per CU by their
 *                                ~62 KiB of tables), 60 000 (2 per CU) for K4h
 *   UAM_OPT_K2G_CHUNK            K2g / K2h / K4h evaluation: gathers in flight per lane,
 *                                6/7/8/11/16/21 (K2g: 7 runs as 6, 16 at two waves per SIMD, 21
 *                                as 16; K2h: 6/7/8/11, 16 and 21 as 11; K4h: 6/7/8/11/16, 21
 *                                as 16);
 *                                0 (default) = 8 for K2g, 7 for K2h, 11 for K4h
 *   UAM_OPT_K2G_CURVE            K2g sort key: tiles in Hilbert (1, default) or Morton (0) order
 *   UAM_OPT_K2G_SIM              1 (default): generated raster batches take K2h, K2g's sort and
 *                                grouped raster sums with the geometry terms (L, length,
 *                                kinematic rows) in the similarity form -- the unit arc's sums
 *                                scaled by |x0 - xf| / 2 (oracle orc_eval_generated_h; needs
 *                                maxratio_smooth = 0); 0: K2g, the geometry per waypoint
 *                                segment in the grouped order (orc_eval_paths_g)
 *   UAM_OPT_K4H_BAND             K4h sort key: altitude layers per band, a power of two
 *                                (default 0: the fewest giving at most 16 bands); tiles from
 *                                UAM_OPT_K2G_TILE_BITS (default 3: 8 x 8 tiles), at most
 *                                4096 (tile, band) bins
 *   UAM_OPT_K2H_LB_STRIDE        K2h / K4h terrain bounds: the histogram launch samples every
 *                                n-th waypoint of each path and seeds the path's items with the
 *                                exact terrain (clearance) of the sample with the best bound
 *                                (1..1024; default 16; 0: no seed); fewer terrain fetches at
 *                                smaller n, more arithmetic in that launch.  Same outputs.
 *   UAM_OPT_K2H_TERRAIN          K2h's terrain: 1 (default) in the entry (8-B {phi, terrain}
 *                                entries, the 16-B records in no-fly / psi blocks), 0 by bounds
 *                                (4-B phi entries, the terrain plane read only where a waypoint
 *                                could still hold the path maximum).  Same outputs.
 *   UAM_OPT_K4H_TERRAIN          K4h's likewise: 0 (default) by bounds (4-B risk / 8-B
 *                                {risk, psi|nfz} voxels, the column terrain only where it could
 *                                still decide an output), 1 in the entry (8-B {risk, terrain}
 *                                voxels, 16-B voxels in no-fly / psi columns).  Same outputs.
 *   UAM_OPT_EXACT_SUM            0 (default): K2h's raster sums in float64, in group order;
 *                                1: as exact integers, independent of every option above (the
 *                                section "Exact, order-independent raster sums" below)
 *   UAM_OPT_EXACT_SUM_VOLUME     0 (default): K4h's voxel sums in float64, in group order;
 *                                1: as exact integers, independent of every option above (the
 *                                section "Exact, order-independent volume sums" below) */
enum {
    UAM_OPT_GROUP = 1,
    UAM_OPT_SORTED_MIN_PATHS = 2,
    UAM_OPT_K2S_SEGMENTS = 3,
    UAM_OPT_WAVE_MAX_PATHS = 4,
    UAM_OPT_PAIR_ORDER = 5,
    UAM_OPT_K1_ROWS = 6,
    UAM_OPT_K3B_SEGMENT = 7,
    UAM_OPT_K3B_POINTS_PER_LANE = 8,
    UAM_OPT_K8_TILED = 9,
    UAM_OPT_K8_STREAMS = 10,
    UAM_OPT_K2G_TILE_BITS = 11,
    UAM_OPT_K2G_LDS_FLOOR = 12,
    UAM_OPT_K2G_CHUNK = 13,
    UAM_OPT_K2G_CURVE = 14,
    UAM_OPT_K2G_SIM = 15,
    UAM_OPT_K4H_BAND = 17,
    UAM_OPT_K2H_LB_STRIDE = 19,
    UAM_OPT_K2H_TERRAIN = 20,
    UAM_OPT_K4H_TERRAIN = 21,
    UAM_OPT_TEST_SORT_FAULT = 22, /* tests only: 1 makes the next sorted calls flag their sort as
                                     inconsistent (the uam_device_status path); 0 (default) off */
    UAM_OPT_EXACT_SUM = 23,       /* 0 (default) / 1: exact, order-independent raster sums (below) */
    UAM_OPT_EXACT_SUM_VOLUME = 24 /* 0 (default) / 1: the same for the volume, K4h (below) */
};
/* The route seeds' two options ("Route seeds" below) are keys of uam_set_option / uam_get_option
 * like the ones above, kept apart from the evaluation options' list (25 and 26 stay
 * unassigned): the tile edge in cells, 16, 32 (default) or 64, and the sweeps inside a tile per
 * round, 1..256 (default 16).  No output depends on either. */
#define UAM_OPT_K9_TILE 27
#define UAM_OPT_K9_INNER 28
/* The volume route seeds' three ("Route seeds in the volume" below): the tile edge in x/y, 8
 * (default) or 16 voxels, the tile edge in z, 4 (default) or 8 layers, and the sweeps inside a
 * tile per round, 1..256 (default 64).  No output depends on any of them. */
#define UAM_OPT_K9V_TILE_XY 29
#define UAM_OPT_K9V_TILE_Z 30
#define UAM_OPT_K9V_INNER 31
int uam_set_option(uam_ctx* ctx, int32_t option, int64_t value);
int uam_get_option(const uam_ctx* ctx, int32_t option, int64_t* value);

/* ---- Exact, order-independent raster sums (UAM_OPT_EXACT_SUM = 1; off by default) ----------
 * K2h's default sums add each path's Phi / N and psi_nfz terms as float64 in group order, so
 * the bits of cost, nfz_sum and best_fval_idx depend on UAM_OPT_GROUP.  With the option on, the
 * raster terms are added as integers: the result depends on the path and the raster only -- not
 * on the group length, the chunk, the sort key, the terrain form, the batch size or the
 * sharding -- so every rank may run its own fastest G and still agree bit for bit.
 * Definition, for one float32 field of the record raster (phi, and separately psi_nfz):
 *   exponent  e = max(1, largest biased exponent field among the finite cells) - 126, so every
 *             finite |v| < 2^e; a raster with no finite nonzero cell gives e = -125
 *   quantum   q = 2^(e - 96)
 *   term      a finite v with sign s, 24-bit significand M (no hidden bit when the biased
 *             exponent field b is 0) gives t = s (sh >= 0 ? M << sh : M >> -sh) with
 *             sh = max(b, 1) - 54 - e <= 72, so |t| < 2^96.  A right shift truncates the
 *             magnitude toward zero: only values more than 72 binades below the raster's
 *             largest lose bits, deterministically and at most one quantum each
 *   sum       S = the sum of the terms in 128-bit two's complement (no overflow below 2^31
 *             terms)
 *   result    fl(S) = S 2^(e - 96) rounded once to float64, to nearest even; S = 0 gives +0.0
 *   non-finite records are not added; they set side flags (NaN, +inf, -inf per field) and the
 *             result follows IEEE: NaN if any NaN or both infinities, else the infinity, else
 *             fl(S)
 *   off-raster waypoints, code-0 blocks and padding slots contribute 0.
 * Path outputs with the option on: nfz_sum = fl(S_psi); cost = (double)(N+1) L + fl(S_phi) /
 * (double)N (a true division); best_fval_idx = the selection rule on that cost; L, length_q,
 * length, kin_sum, nfz_hits, offmap, min_clearance, cells and best_length_idx are exactly
 * K2h's.  Against the default sums: rounding only, |cost_on - cost_off| <=
 * 2 W 2^-53 (sum |phi_j| / N + (N+1) L).
 * Dispatch: a raster-mode uam_eval_generated batch runs K2h's exact form at every size
 * (uam_last_kernel "K2hx+pack"; UAM_OPT_SORTED_MIN_PATHS and UAM_OPT_WAVE_MAX_PATHS do not
 * apply; uam_last_group reports G as usual) and never falls back to ordered sums: UAM_E_STATE
 * when no sum scale is set, UAM_E_INVALID (reason in uam_last_error) for a batch K2h does not
 * take -- no packed_dev, maxratio_smooth, UAM_OPT_K2G_SIM = 0, UAM_OPT_GROUP = 0, D > 16,
 * N > 4096, a packed copy of 4 GiB or more.  Analytic mode, uam_eval_waypoints and uam_refine
 * ignore the option, and so does the volume: uam_eval_generated3d ignores UAM_OPT_EXACT_SUM,
 * and UAM_OPT_EXACT_SUM_VOLUME is its own option (the next section).
 *
 * uam_raster_sum_scale writes the raster's 16-byte scale {e_phi, e_psi, flags, 0} to the
 * caller's device buffer scale_dev (flags: bits 0-2 = a phi cell holds NaN / +inf / -inf, bits
 * 3-5 = a psi_nfz cell does), asynchronously on stream, no host sync.  The exponents are integer
 * maxima: the words do not depend on the reduction's order.  Like the summary and the packed
 * copy it is a derived, untracked copy of rec: rebuild it whenever rec changes.
 * uam_set_sum_scale: the context keeps the pointer (not the words) for the uam_eval_generated
 * calls that follow; NULL clears it.
 * uam_exact_sum_host (host only, no GPU): the definition applied to values[n] by the same
 * inline functions the kernels run; e = INT32_MIN derives the exponent from values, any other
 * e must be at least that and at most 128 (UAM_E_INVALID otherwise); *e_out (optional) is the
 * exponent used. */
int uam_raster_sum_scale(uam_ctx* ctx, const uam_raster_desc* desc, const void* rec_dev,
                         int32_t* scale_dev, uam_stream stream);
int uam_set_sum_scale(uam_ctx* ctx, const int32_t* scale_dev);
int uam_exact_sum_host(const float* values, int64_t n, int32_t e, double* sum_out,
                       int32_t* e_out);

/* ---- Exact, order-independent volume sums (UAM_OPT_EXACT_SUM_VOLUME = 1; off by default) -----
 * K4h's default sums add each path's risk / N and psi_nfz terms as float64 in group order, and
 * a batch K4h does not take runs K4 / K4w with sequential sums, so the bits of cost, nfz_sum and
 * best_fval_idx depend on UAM_OPT_GROUP and on the batch size.  With the option on they depend
 * on the path and the volume only -- not on the group length, the chunk, the sort key (tiles,
 * bands, curve), the terrain form, the batch size or the sharding.  A separate option:
 * UAM_OPT_EXACT_SUM keeps its meaning (the raster only), and with this one off every call gives
 * the bits it gave before.
 * Definition: the raster section's, applied to the two float32 fields of the volume's voxels
 * (risk, and separately psi_nfz):
 *   scale     e_risk and e_psi = max(1, largest biased exponent field among the finite words)
 *             - 126, taken over all ny nx nz voxels of vol_dev's voxel section {risk, psi_nfz};
 *             the column plane is not included; a field with no finite nonzero voxel gives -125
 *   term, truncation rule, 128-bit sum, single rounding fl(S) and side flags: exactly as the
 *             raster section states them (the same inline functions)
 *   a path adds the words of the voxel under each of its W waypoints that lies inside the
 *             volume (x, y and z); waypoints outside the volume, code-0 column blocks and
 *             padding slots add 0.  The psi_nfz word of a code-2 block is the packed |psi| word:
 *             code 2 holds no negative psi, so the term is the voxel's own, and a positive NaN
 *             or +inf still raises its flag
 * Path outputs with the option on: nfz_sum = fl(S_psi); cost = (double)(N+1) L + fl(S_risk) /
 * (double)N (a true division); best_fval_idx = the selection rule on that cost; length_q,
 * length, kin_sum, nfz_hits, offmap, min_clearance, below_terrain and best_length_idx are
 * exactly K4h's.  Against the default sums: rounding only, |cost_on - cost_off| <=
 * 2 W 2^-53 (sum |risk_j| / N + (N+1) L), |nfz_on - nfz_off| <= 2 W 2^-53 sum |psi_j|.
 * Dispatch: uam_eval_generated3d runs K4h's exact form at every batch size (uam_last_kernel
 * "K4hx+pack"; UAM_OPT_SORTED_MIN_PATHS and UAM_OPT_WAVE_MAX_PATHS do not apply; uam_last_group
 * reports G as usual) and never falls back to K4 / K4w or to ordered sums: UAM_E_STATE when no
 * volume sum scale is set, UAM_E_INVALID (reason in uam_last_error) for a batch K4h does not
 * take -- no packed_dev, maxratio_smooth, UAM_OPT_K2G_SIM = 0, UAM_OPT_GROUP = 0, D > 16,
 * N > 4096, a unit-arc table or packed header too large for LDS, more (tile, band) bins than
 * the sort holds, 2^31 or more paths or (path, group) items, a packed copy K4h stands aside for
 * (4 GiB or more, 2^24 entries a layer or columns a side).  The errors are raised on the host
 * before any launch; the context stays usable.
 * uam_eval_waypoints3d and uam_eval_generated3d_profiles form ordered sums and have no exact
 * form yet (a follow-up): with the option on both fail on the host with UAM_E_INVALID, naming the
 * option -- exact or an error, never ordered.  uam_gen_paths3d sums nothing and ignores it.
 *
 * uam_volume_sum_scale writes the volume's 16-byte scale {e_risk, e_psi, flags, 0} to the
 * caller's device buffer scale_dev (flags: bits 0-2 = a risk word holds NaN / +inf / -inf, bits
 * 3-5 = a psi_nfz word does -- the raster word's layout), asynchronously on stream, no host
 * sync.  Integer maxima and ORs: the words do not depend on the reduction's order.  Like the
 * packed copy it is a derived, untracked copy of vol_dev: rebuild it whenever the voxels change.
 * uam_set_volume_sum_scale: the context keeps the pointer (not the words) for the
 * uam_eval_generated3d calls that follow; NULL clears it.  Independent of uam_set_sum_scale. */
int uam_volume_sum_scale(uam_ctx* ctx, const uam_volume_desc* desc, const void* vol_dev,
                         int32_t* scale_dev, uam_stream stream);
int uam_set_volume_sum_scale(uam_ctx* ctx, const int32_t* scale_dev);

/* ---- Altitude-profile candidates on the packed, sorted volume (K4hp) -------------------------
 * uam_eval_generated3d_profiles walks vol_dev one lane per lateral candidate at every batch
 * size.  This call takes the profile table's altitudes through K4h's form instead: the
 * (path, group) items sorted on the altitude band and tile of their middle waypoint at the
 * profile's own z, gathers from packed_dev (uam_volume_pack), grouped partial sums, the
 * geometry in the similarity form.  Layout as uam_eval_generated3d_profiles: path p =
 * (q*D + d)*A + a, candidate c = d*A + a, 1 <= A <= 8, D <= 16.  vol_dev is not read (NULL is
 * allowed).
 *
 * Definition (normative).  Every float64 operation is rounded, none is contracted.  G =
 * UAM_OPT_GROUP (G >= 1), W = N + 2.
 *   points     x/y of waypoint j are uam_gen_paths3d's: the pair's own end points at j = 0 and
 *              j = N+1, the arc formula in between (K4h's operations).  z_j follows the table
 *              rule (z0 * ztab[a][j][0] + zf * ztab[a][j][1]) + ztab[a][j][2].
 *              NULL-table rule: ztab_dev == NULL (A must be 1) means uam_eval_generated3d's
 *              straight climb z0 + (zf - z0) * ((double)j / (double)(N+1)); the call then runs
 *              K4h's own kernels and gives uam_eval_generated3d's K4h bits (uam_last_kernel
 *              "K4h+pack" / "K4hx+pack").
 *   geometry   length_q, length and kin_sum are K4h's similarity-form values of (q, d) (oracle
 *              sim_geo, orc_eval_generated_h), identical for the A profiles.
 *   cost       group order: cost = ((N+1) L + P_0) + P_1 + ... with P_k the sum from +0.0, in
 *              waypoint order, of (double)risk_j / (double)N over the waypoints j in
 *              [k G, min((k+1) G, W)) that lie inside the volume by their own (x, y, z).
 *   nfz_sum    the same group order from +0.0 with (double)psi_j as the term (the oracle's gacc
 *              on the profile's voxels).
 *   nfz_hits, offmap, below_terrain, min_clearance: per path, exactly as uam_eval_waypoints3d
 *              defines them; min_clearance is +inf when no waypoint lies inside the volume.
 *   selections best_fval_idx and best_length_idx follow uam_argmin's rule over the pair's D*A
 *              candidates in index order c; they need the cost / length output respectively.
 *   reporting  uam_last_group reports G; uam_last_kernel "K4hp+pack" ("K4hpx+pack": exact form).
 * Exact form: with UAM_OPT_EXACT_SUM_VOLUME = 1 the call uses the exact volume sums above (the
 * same term, 128-bit sum, single rounding, side flags and volume scale as K4h's exact form):
 * cost = (double)(N+1) L + fl(S_risk) / (double)N, nfz_sum = fl(S_psi), every other output as
 * above.  The bits then do not depend on G, the chunk, the terrain form, tile bits, band, curve,
 * the batch size or the sharding.  UAM_E_STATE when no volume sum scale is set.
 * Dispatch: the call has a sum order of its own, so it is never falling back to K4p, K4 or
 * K4w, at any batch size: UAM_OPT_SORTED_MIN_PATHS and UAM_OPT_WAVE_MAX_PATHS do not apply, and
 * a path's bits do not depend on the batch it is in.  Every case it does not take is
 * UAM_E_INVALID with its reason (uam_last_error), raised on the host before any launch or
 * allocation, the context staying usable: no packed_dev; UAM_OPT_GROUP = 0; maxratio_smooth;
 * UAM_OPT_K2G_SIM = 0; D > 16; A outside [1, 8] or a NULL table with A != 1; N > 4096; cells or
 * g_rows requested; a unit-arc table (48 KiB), profile table (40 KiB) or packed header (64 KiB)
 * over its LDS share; more (tile, band) bins, (path, group) items (Q D A groups >= 2^31) or scan
 * blocks than the sort holds; a packed copy K4h stands aside for; packed_dev / vol_dev not
 * 256-B, pairs6_dev / utab_dev not 16-B or ztab_dev not 8-B aligned.  The sort's device check
 * applies as for K4h (uam_device_status).  The vertical terms have no such form (the similarity
 * form is not scale-free once the altitude differences enter the norm): there is no _v variant
 * of this definition; uam_eval_generated3d_profiles_hv below keeps the sorted sums and takes the
 * geometry per path. */
int uam_eval_generated3d_profiles_h(uam_ctx* ctx, const uam_volume_desc* desc,
                                    const void* vol_dev, const void* packed_dev,
                                    const double* pairs6_dev, int64_t n_pairs,
                                    const double* utab_dev, int32_t D, const double* ztab_dev,
                                    int32_t A, const uam_path_outputs* out, uam_stream stream);

/* ---- Vertical terms for the profiles on the packed, sorted volume (K4hp+v) --------------------
 * uam_eval_generated3d_profiles_h's sorted sums with uam_vertical's geometry: the call that both
 * charges altitude changes and reads packed_dev.  The sort and the evaluation are K4hp's,
 * unchanged (they never look at the geometry terms); the output launch walks each path's W
 * waypoints once, sequentially, as uam_eval_generated3d_profiles_v does.  Arguments as
 * uam_eval_generated3d_profiles_h, plus vert and climb_sum_dev [Q*D*A] (NULL: not wanted);
 * uam_path_outputs does not grow.  vol_dev is not read (NULL is allowed).
 *
 * Definition (normative).  Layout as K4hp: p = (q*D + d)*A + a, c = d*A + a, 1 <= A <= 8,
 * D <= 16.  Every float64 operation is rounded, none is contracted.  G = UAM_OPT_GROUP, W = N + 2.
 *   points     K4hp's: x/y are uam_gen_paths3d's, z_j follows the table rule; ztab_dev == NULL
 *              with A = 1 is the straight climb z0 + (zf - z0) * ((double)j / (double)(N+1)).
 *   geometry   length_q, length, kin_sum and climb_sum are the uam_vertical loop above over those
 *              points, sequentially, j = 1 .. N+1: the bits uam_eval_generated3d_profiles_v gives
 *              for the same inputs.  They differ among the A profiles of a lateral candidate.
 *   cost       K4hp's group order with the 3-D L as the base: cost = ((N+1) L + P_0) + P_1 + ...
 *              with P_k as in K4hp's section.
 *   nfz_sum, nfz_hits, offmap, below_terrain, min_clearance: K4hp's, bit for bit; the vertical
 *              terms do not touch them.
 *   selections uam_argmin's rule over the pair's D A candidates on the new cost and the new
 *              length; best_length_idx need not be a multiple of A.
 *   kappa = 0  with finite altitudes length_q, length and kin_sum equal
 *              uam_eval_generated3d_profiles' sequential x/y bits (not K4hp's similarity-form
 *              bits), and climb_sum is +0.
 *   reporting  uam_last_group reports G; uam_last_kernel "K4hpv+pack" ("K4hpxv+pack": exact
 *              form), with or without a table.
 * Exact form: with UAM_OPT_EXACT_SUM_VOLUME = 1, cost = (double)(N+1) L + fl(S_risk) / (double)N
 * and nfz_sum = fl(S_psi) as in K4hp's exact form; the bits then do not depend on G, the batch or
 * the sharding.  UAM_E_STATE when no volume sum scale is set.
 * Dispatch: as K4hp, sorted at every batch size or UAM_E_INVALID with its reason before any
 * launch or allocation; a path's bits do not depend on the batch it is in.  The refusals are
 * K4hp's, their messages prefixed "uam_eval_generated3d_profiles_hv needs K4hpv", with two
 * differences: maxratio_smooth is taken (the sequential rows handle it as in
 * uam_eval_generated3d_profiles_v), and UAM_OPT_K2G_SIM is not read (no similarity form is
 * used).  vert is checked where uam_eval_generated3d_profiles_v checks it, after the context and
 * before the dimensions: UAM_E_INVALID for vert == NULL, UAM_E_VERSION for a wrong abi_version,
 * UAM_E_INVALID for a NaN, negative or infinite z_scale and for a NaN or negative sin_climb /
 * sin_descent.  On a failed sort check (uam_device_status) climb_sum is NaN like the other
 * float64 outputs. */
int uam_eval_generated3d_profiles_hv(uam_ctx* ctx, const uam_volume_desc* desc,
                                     const void* vol_dev, const void* packed_dev,
                                     const double* pairs6_dev, int64_t n_pairs,
                                     const double* utab_dev, int32_t D, const double* ztab_dev,
                                     int32_t A, const uam_vertical* vert,
                                     const uam_path_outputs* out,
                                     double* climb_sum_dev /* [Q*D*A] or NULL */,
                                     uam_stream stream);

/* ---- Route seeds (K9): cost-to-go field of a goal and traced paths on the record raster ------
 * Every candidate the calls above score or refine is one of the D circular arcs.  These calls
 * give a path of another shape: the cheapest 8-connected route over the raster's cells from any
 * start to a goal, resampled to the N+2 waypoints uam_eval_waypoints and uam_refine take.  One
 * field serves every query that shares the goal: uam_route_field is a per-goal SETUP call like
 * uam_raster_pack (it may synchronise the stream: the host reads a convergence word between
 * rounds), uam_route_paths is asynchronous.
 *
 * Definition (normative; independent statement: tests/route_ref.py).  Every float64 operation
 * is rounded separately, in the order written (no fused multiply-add).
 *   cells      a point maps to a cell by uam_raster_desc's rule; the centre of cell (ix, iy) is
 *              (x0 + (ix + 0.5)*dx, y_top - (iy + 0.5)*dy).  Directions k = 0..7 are
 *              (dix, diy) = E(1,0), NE(1,-1), N(0,-1), NW(-1,-1), W(-1,0), SW(-1,1), S(0,1),
 *              SE(1,1); step lengths L_k = dx (E/W), dy (N/S), sqrt(dx*dx + dy*dy) (diagonals).
 *   cell cost  c_v = 1.0 + lambda * (double)phi_v (the record's float32 phi).  A cell is
 *              blocked0 when (flags_v & block_flags) != 0, or c_v is not finite, or c_v is not
 *              > 0 (NaN, +-inf and very negative phi all land here).  A cell is blocked when a
 *              blocked0 cell lies within Chebyshev distance inflate of it (cells outside the
 *              raster do not count); inflate = 0: blocked = blocked0.  Otherwise it is free.
 *   edges      between free neighbours u, v in one of the 8 directions; a diagonal step also
 *              needs both cells orthogonally adjacent to it free (a one-cell-wide diagonal wall
 *              is a wall; no path cuts a corner).  w(u,v) = (0.5 * (c_u + c_v)) * L_k, symmetric.
 *   field      for a goal point with cell g: dist[g] = 0 when g is on the raster and free;
 *              elsewhere dist[v] = the minimum over edge paths g = v_0, .., v_n = v of the left
 *              fold fl(fl(fl(0 + w_01) + w_12) + ..); +inf for blocked and unreachable cells,
 *              and everywhere when g is blocked or off the raster.  fl(a + w) is monotone in a,
 *              so this minimum is the one fixed point of d[v] = min(d[v], fl(d[u] + w(u,v)))
 *              started from +inf / 0: the bits do not depend on the relaxation order, the tile
 *              edge or the sweeps per round.
 *   next hop   uint8 per cell, formed after convergence: 8 at the goal cell, 255 where dist is
 *              +inf, else the lowest k whose neighbour u_k = v + (dix, diy)_k has an edge to v
 *              with fl(dist[u_k] + w(u_k, v)) == dist[v].
 *   path       for a query (start point, goal index): status, tested in this order,
 *                4  the goal index is outside [0, n_goals), or the goal is off the raster or
 *                   blocked;
 *                1  the start is off the raster or in a blocked cell;
 *                2  the goal is unreachable from the start's cell s (dist[s] = +inf, g free);
 *                3  the walk along next from s visited nx*ny cells without reaching g (possible
 *                   only when huge costs absorb small weights and equal dist values form a
 *                   cycle; also a next value that is no direction or leads off the raster, which
 *                   uam_route_field never writes);
 *                0  ok.
 *              steps = the number of cells the walk visited, s and g included (1 when s = g); 0
 *              for a nonzero status.  Vertices: V_0 = the start point itself, then the centres
 *              of the visited cells strictly between s and g, V_m = the goal point itself (s = g
 *              or adjacent cells: the straight segment, m = 1).  S_0 = 0, S_i = S_{i-1} +
 *              sqrt(ex*ex + ey*ey) with e = V_i - V_{i-1}, sequentially.  Waypoints p_0 = V_0 and
 *              p_{N+1} = V_m, copied; for j = 1..N: t = S_m * ((double)j / (double)(N+1)); i =
 *              the first index >= the previous waypoint's i (1 at j = 1) with S_i > t, m if there
 *              is none; u = (t - S_{i-1}) / (S_i - S_{i-1}), 0 if the denominator is not > 0;
 *              p_j = V_{i-1} + u * (V_i - V_{i-1}) per component.  By the corner rule every
 *              waypoint of a status-0 path lies in a free cell.  For a nonzero status the
 *              waypoints are the straight line p_j = start + (goal - start) * ((double)j /
 *              (double)(N+1)) with the end points copied (a goal index out of range: every
 *              waypoint is the start point), so a downstream call never reads garbage.
 *
 * uam_route_params: lambda finite and >= 0; inflate 0..8; max_rounds >= 0 bounds the relaxation
 * rounds of one goal, 0 = nx*ny (each round settles at least the cells whose best path crosses
 * one more tile border than the round before).
 * uam_route_field: the fields of n_goals goals (goals_dev [n_goals][2]) into dist_dev
 * [n_goals][ny][nx] f64 and next_dev [n_goals][ny][nx] u8; workspace_dev holds
 * uam_route_workspace_bytes(desc, params) bytes, 256-B aligned (the cost plane, shared by the
 * goals, and the active-tile sets).  The goals are relaxed one after the other: label-correcting
 * rounds over the set of active tiles, one ordinary launch per round, the host reading the next
 * round's tile count after each.  rounds_out (host, may be NULL): the rounds of all goals
 * together; uam_route_visits: the tiles those rounds visited.  uam_last_kernel: "K9".
 * Failures: UAM_E_INVALID before any launch or allocation for ctx / desc / params / a buffer
 * NULL, a bad descriptor, lambda NaN, infinite or negative, inflate outside [0, 8], max_rounds
 * < 0, n_goals < 1 or n_goals * nx * ny >= 2^40, a workspace too small or misaligned;
 * UAM_E_VERSION for a wrong abi_version; UAM_E_STATE, the message naming max_rounds, when a field
 * has not converged within max_rounds rounds -- the outputs are then unspecified and the context
 * stays usable.
 * uam_route_paths: Q queries (starts_dev [Q][2], goal_idx_dev [Q]) against next_dev as
 * uam_route_field wrote it for the same desc, rec_dev, params (the start's blocking is read from
 * rec_dev) and goals_dev, into wp_dev [Q][N+2][2], status_dev [Q] and steps_dev [Q] (or NULL);
 * N from uam_set_params (UAM_E_STATE without it).  One lane per query, two sequential walks
 * bounded by nx*ny steps: seed generation, not a per-step call.  uam_last_kernel: "K9t".
 * The _host calls take host pointers and run, without a GPU, the same inline functions as the
 * kernels (cell cost, blocking, edge weight, next-hop choice, trace and resample; the field's
 * minimum by a heap Dijkstra).
 * UAM_OPT_K9_TILE (16, 32 (default), 64) and UAM_OPT_K9_INNER (1..256) choose the tile edge and
 * the sweeps inside a tile per round; no output depends on them (rounds and visits do). */
typedef struct {
    uint32_t abi_version; /* UAM_ABI_VERSION */
    double lambda;        /* weight of phi in the cell cost; finite, >= 0 */
    uint32_t block_flags; /* UAM_FLAG_* bits that block a cell */
    int32_t inflate;      /* cells of clearance around a blocked0 cell, 0..8 */
    int32_t max_rounds;   /* 0 = nx*ny */
} uam_route_params;
int64_t uam_route_workspace_bytes(const uam_raster_desc* desc, const uam_route_params* params);
int uam_route_field(uam_ctx* ctx, const uam_raster_desc* desc, const void* rec_dev,
                    const uam_route_params* params, const double* goals_dev, int32_t n_goals,
                    double* dist_dev, uint8_t* next_dev, void* workspace_dev,
                    int64_t workspace_bytes, int32_t* rounds_out, uam_stream stream);
int64_t uam_route_visits(const uam_ctx* ctx);
int uam_route_paths(uam_ctx* ctx, const uam_raster_desc* desc, const void* rec_dev,
                    const uam_route_params* params, const uint8_t* next_dev,
                    const double* goals_dev, int32_t n_goals, const double* starts_dev,
                    const int32_t* goal_idx_dev, int64_t n_queries, double* wp_dev,
                    int32_t* status_dev, int32_t* steps_dev, uam_stream stream);
int uam_route_field_host(const uam_raster_desc* desc, const void* rec,
                         const uam_route_params* params, const double* goals, int32_t n_goals,
                         double* dist, uint8_t* next);
int uam_route_paths_host(const uam_raster_desc* desc, const void* rec,
                         const uam_route_params* params, const uint8_t* next,
                         const double* goals, int32_t n_goals, const double* starts,
                         const int32_t* goal_idx, int64_t n_queries, int32_t N, double* wp,
                         int32_t* status, int32_t* steps);

/* Route seeds, smoothing (K9b / K9s): any-angle shortcuts on the traced path.  An 8-connected
 * route turns by 45 degrees per kink; these calls keep of the traced cell chain only the cells
 * from which the next one kept is no longer in straight sight, and resample that polyline.
 *
 * Definition (normative; independent statement: tests/route_smooth_ref.py).  The trace is
 * uam_route_paths': the status rules, steps and the cell chain c_0 = s, c_1, .., c_{n-1} = g
 * along next (n = steps) are unchanged.  Smoothing chooses a subsequence of the interior cells;
 * the vertices and the resampling are uam_route_paths' own rules applied to that subsequence.
 *   touched    for cells A = (ax, ay), B = (bx, by), d = (bx - ax, by - ay): T(A, B) is the set
 *              of cells (x, y) in the integer bounding box of A and B with
 *              2*|dx*(y - ay) - dy*(x - ax)| <= |dx| + |dy|: the closed supercover of the
 *              segment between the two cell centres (a segment through a cell corner touches
 *              all four cells around it).  Integers only; |dx|, |dy| <= span <= 1024.
 *   visible    LOS(A, B) holds iff every cell of T(A, B) is free (not blocked, inflation
 *              included).  Adjacent chain cells are always visible: a diagonal step's T is the
 *              2 x 2 square, free by the corner rule.
 *   anchors    none for n <= 2.  Otherwise a_0 = 1; a_{k+1} = the largest j <= min(a_k + span,
 *              n - 2) such that LOS(c_{a_k}, c_i) holds for every i in (a_k, j] ("advance while
 *              visible", not "the farthest visible"; never less than a_k + 1); stop at a_k =
 *              n - 2.  c_1 and c_{n-2} are always kept: the start and goal points are no cell
 *              centres, so the first and last segments stay the ones uam_route_paths flies.
 *   vertices   V_0 = the start point, the centres of c_{a_0}, c_{a_1}, .., V_m = the goal
 *              point.  S_i, the waypoints p_j, the straight line of a nonzero status and the
 *              status values: uam_route_paths' text, word for word.  vertices[q] = m + 1 (2 +
 *              the number of anchors); 0 for a nonzero status.
 *   guarantee  every point of a segment lies in a closed cell of its T, all free: every
 *              waypoint of a status-0 path lies in a free cell.
 *   bridge     span = 1 keeps every interior cell: wp, status and steps are uam_route_paths'
 *              bits.
 * The shortcut test is geometric: it does not weigh phi along the segment; span bounds how far
 * a shortcut may leave the field's route.
 *
 * uam_route_free_bits: the free cells of (desc, rec_dev, params) as one bit per cell, set =
 * free, row-major, bit ix & 31 of word iy * ((nx + 31) / 32) + ix / 32 (rows padded to uint32
 * words, the padding 0), uam_route_free_bits_bytes(desc) bytes (-1 for a bad descriptor),
 * 4-B aligned.  uam_last_kernel: "K9b".  Failures as uam_route_field's for ctx / desc / params /
 * a NULL buffer.
 * uam_route_paths_smooth: uam_route_paths with shortcuts of at most span chain cells, 1 <= span
 * <= UAM_ROUTE_SPAN_MAX, against bits_dev and next_dev of the same desc, rec and params (the
 * start's blocking is read from the bits); steps_dev and vertices_dev may be NULL.  One wave
 * per query; a query with more than UAM_ROUTE_SMOOTH_LIST anchors is smoothed twice (no output
 * depends on that).  Asynchronous.  uam_last_kernel: "K9s".  UAM_E_INVALID before any launch
 * for ctx / desc / a buffer NULL, a bad descriptor, span outside the range, n_goals < 1 or too
 * many cells, nx*ny > 2^31 - 1 - UAM_ROUTE_SPAN_MAX (chain indices are int32), n_queries < 0 or
 * too large; UAM_E_STATE without uam_set_params.
 * The _host calls run the same inline functions without a GPU.  uam_route_visible_host: the
 * library's LOS on n pairs of cell indices (iy * nx + ix; UAM_E_INVALID for one off the
 * raster) into out_u8 (1 = visible). */
#define UAM_ROUTE_SPAN_MAX 1024
#define UAM_ROUTE_SMOOTH_LIST 256
int64_t uam_route_free_bits_bytes(const uam_raster_desc* desc);
int uam_route_free_bits(uam_ctx* ctx, const uam_raster_desc* desc, const void* rec_dev,
                        const uam_route_params* params, uint32_t* bits_dev, uam_stream stream);
int uam_route_paths_smooth(uam_ctx* ctx, const uam_raster_desc* desc, const uint32_t* bits_dev,
                           const uint8_t* next_dev, const double* goals_dev, int32_t n_goals,
                           const double* starts_dev, const int32_t* goal_idx_dev,
                           int64_t n_queries, int32_t span, double* wp_dev, int32_t* status_dev,
                           int32_t* steps_dev, int32_t* vertices_dev, uam_stream stream);
int uam_route_free_bits_host(const uam_raster_desc* desc, const void* rec,
                             const uam_route_params* params, uint32_t* bits);
int uam_route_paths_smooth_host(const uam_raster_desc* desc, const uint32_t* bits,
                                const uint8_t* next, const double* goals, int32_t n_goals,
                                const double* starts, const int32_t* goal_idx,
                                int64_t n_queries, int32_t N, int32_t span, double* wp,
                                int32_t* status, int32_t* steps, int32_t* vertices);
int uam_route_visible_host(const uam_raster_desc* desc, const uint32_t* bits, int64_t n,
                           const int32_t* a_cells, const int32_t* b_cells, uint8_t* out_u8);

/* Route seeds, joint field (K9j): one field to the nearest of many goals, with an owner map.
 * uam_route_field answers "what is the cheapest route to that goal?" once per goal.  These calls
 * answer "which goal is cheapest to reach from here, and how?" for all goals in one relaxation:
 * the contingency landing site of any point of a route, the service area of each vertiport under
 * the risk-weighted metric, a start whose goal is not fixed yet.
 *
 * Definition (normative; independent statement: tests/route_joint_ref.py).  Cells, directions,
 * cell cost, blocking, inflation, edges, the corner rule and the edge weight are the "Route
 * seeds" text, unchanged.  Every float64 operation is rounded separately, with no fused
 * multiply-add.
 *   valid goal goal i is valid when its point maps to a cell g_i on the raster and that cell is
 *              free.  Gc is the set of cells of the valid goals.  Several goals may share a cell.
 *              Gc may be empty.
 *   field      dist[v] = 0 for v in Gc; elsewhere the minimum, over edge paths that start in any
 *              cell of Gc and end in v, of the left fold fl(fl(0 + w_01) + w_12) + ..; +inf for
 *              blocked and unreachable cells, and everywhere when Gc is empty.  It is the one
 *              fixed point of d[v] = min(d[v], fl(d[u] + w(u,v))) started from 0 on Gc and +inf
 *              elsewhere: the bits do not depend on the relaxation order, the tile edge or the
 *              sweeps per round.
 *   bridge 1   dist equals the elementwise minimum over i of the planes uam_route_field writes
 *              for the same goals, bit for bit (the path sets are a union; an invalid goal's
 *              plane is all +inf).
 *   bridge 2   with n_goals = 1, dist and next are uam_route_field's bits.
 *   next hop   uint8 per cell, formed after convergence: 8 at every cell of Gc, 255 where dist is
 *              +inf, otherwise the lowest k whose neighbour u_k has an edge to v with
 *              fl(dist[u_k] + w(u_k, v)) == dist[v].  The goal test is membership in Gc, not
 *              dist == 0.
 *   owner      int32 per cell: -1 where next is 255; at a cell of Gc the lowest index i with
 *              g_i = v; otherwise the owner of the first cell of Gc on the chain v -> v +
 *              dir(next[v]) -> ..; -1 when the chain visits nx*ny cells without reaching Gc
 *              (only where huge costs absorb small weights and equal dist values form a cycle).
 *              Owner is defined through the chain, not through a comparison of per-goal
 *              distances: ties are broken by the next-hop rule alone.
 *   owner      if owner[v] = i >= 0 then dist[v] == dist_i[v] bit for bit, dist_i being goal i's
 *   property   own field: the chain realises dist[v] as a fold from g_i, and dist is the minimum
 *              over all goals.
 *   path       a query is a start point only.  Status, tested in this order:
 *                1  the start is off the raster or in a blocked cell;
 *                2  next[s] = 255 (with no valid goal every free start gets 2);
 *                3  owner[s] = -1 although dist[s] is finite;
 *                0  ok.  There is no status 4.
 *              Status 0: goal_out[q] = o = owner[s], the goal point is goals[o], and the chain,
 *              steps, vertices, S_i, waypoints and (span >= 1) anchors are uam_route_paths' and
 *              uam_route_paths_smooth's text word for word, along the joint next from s to g_o.
 *              vertices[q] at span 0 counts every interior cell: max(steps, 2), span 1's value.
 *              A nonzero status: goal_out[q] = -1, steps = 0, vertices = 0 and every waypoint is
 *              the start point (the existing rule for a goal index out of range).
 *   bridge 3   with n_goals = 1, status, steps and vertices equal uam_route_paths' (span 0) and
 *              uam_route_paths_smooth's (span >= 1) with goal_idx = 0 for every query whose
 *              status there is not 4; the waypoints are equal as well for status 0.
 *   guarantee  every waypoint of a status-0 path lies in a free cell, as for the existing calls.
 *
 * uam_route_field_joint: goals_dev [n_goals][2] into dist_dev [ny][nx] f64, next_dev [ny][nx] u8
 * and owner_dev [ny][nx] int32; workspace_dev holds uam_route_joint_workspace_bytes(desc, params,
 * n_goals) bytes (-1 for bad arguments), 256-B aligned: uam_route_field's workspace and an int32
 * parent plane.  One start state for all goals (the distinct tiles of Gc form the first active
 * set), then uam_route_field's rounds with its kernel, UAM_OPT_K9_TILE / UAM_OPT_K9_INNER and
 * max_rounds (the call may synchronise the stream between rounds); the owner by pointer jumping
 * over the parent plane, ceil(log2(nx*ny)) ordinary launches with no host read between them.
 * rounds_out and uam_route_visits as for uam_route_field.  uam_last_kernel: "K9j".
 * uam_route_paths_joint: Q start points against next_dev, owner_dev and goals_dev of one
 * uam_route_field_joint call, into wp_dev [Q][N+2][2], status_dev [Q] and (each may be NULL)
 * steps_dev, vertices_dev, goal_out_dev [Q].  span = 0: the plain trace, one lane per query, the
 * start's blocking read from rec_dev, bits_dev may be NULL; uam_last_kernel "K9jt".  1 <= span <=
 * UAM_ROUTE_SPAN_MAX: shortcuts as uam_route_paths_smooth makes them, one wave per query, the
 * blocking from bits_dev (uam_route_free_bits of the same desc, rec, params), rec_dev may be
 * NULL; uam_last_kernel "K9js".  Asynchronous.  N from uam_set_params.
 * Failures: uam_route_field's and uam_route_paths_smooth's lists, UAM_E_INVALID before any launch
 * or allocation; in addition n_goals < 1 or > 2^20 and nx*ny > 2^31 - 1 - UAM_ROUTE_SPAN_MAX
 * (parents and owners are int32), owner_dev not 4-B aligned, span outside [0,
 * UAM_ROUTE_SPAN_MAX].  UAM_E_STATE, the message naming max_rounds, when the field has not
 * converged within max_rounds rounds (outputs unspecified, the context stays usable), and for
 * uam_route_paths_joint without uam_set_params.
 * The _host calls run the same inline functions without a GPU: the field's minimum by a heap
 * Dijkstra seeded with all of Gc, the owner by following the chains. */
int64_t uam_route_joint_workspace_bytes(const uam_raster_desc* desc,
                                        const uam_route_params* params, int32_t n_goals);
int uam_route_field_joint(uam_ctx* ctx, const uam_raster_desc* desc, const void* rec_dev,
                          const uam_route_params* params, const double* goals_dev,
                          int32_t n_goals, double* dist_dev, uint8_t* next_dev,
                          int32_t* owner_dev, void* workspace_dev, int64_t workspace_bytes,
                          int32_t* rounds_out, uam_stream stream);
int uam_route_paths_joint(uam_ctx* ctx, const uam_raster_desc* desc, const void* rec_dev,
                          const uam_route_params* params, const uint32_t* bits_dev,
                          const uint8_t* next_dev, const int32_t* owner_dev,
                          const double* goals_dev, int32_t n_goals, const double* starts_dev,
                          int64_t n_queries, int32_t span, double* wp_dev, int32_t* status_dev,
                          int32_t* steps_dev, int32_t* vertices_dev, int32_t* goal_out_dev,
                          uam_stream stream);
int uam_route_field_joint_host(const uam_raster_desc* desc, const void* rec,
                               const uam_route_params* params, const double* goals,
                               int32_t n_goals, double* dist, uint8_t* next, int32_t* owner);
int uam_route_paths_joint_host(const uam_raster_desc* desc, const void* rec,
                               const uam_route_params* params, const uint32_t* bits,
                               const uint8_t* next, const int32_t* owner, const double* goals,
                               int32_t n_goals, const double* starts, int64_t n_queries,
                               int32_t N, int32_t span, double* wp, int32_t* status,
                               int32_t* steps, int32_t* vertices, int32_t* goal_out);

/* ---- Route seeds in the volume (K9v): 3-D cost-to-go field and traced 3-D routes --------------
 * The route seeds above are flat: they know neither the terrain nor the altitude layers.  These
 * calls are their counterpart over the risk volume's voxels: the cheapest 26-connected route
 * from any 3-D start to a goal, resampled to the [N+2][3] waypoints uam_eval_waypoints3d and
 * uam_eval_waypoints3d_v take.  uam_route3d_field is a per-goal SETUP call like uam_route_field
 * (it synchronises the stream between rounds), uam_route3d_paths is asynchronous.
 *
 * Definition (normative; independent statement: tests/route3d_ref.py).  Every float64 operation
 * is rounded separately, in the order written (no fused multiply-add).
 *   voxels     a point maps to a voxel by uam_volume_desc's rule in x, y and z; the centre of
 *              voxel (ix, iy, iz) is (x0 + (ix + 0.5)*dx, y_top - (iy + 0.5)*dy,
 *              z0 + (iz + 0.5)*dz); its index is (iy*nx + ix)*nz + iz (the cells convention of
 *              uam_eval_waypoints3d).  Field outputs are laid out [n_goals][ny][nx][nz].
 *   directions k = 0..25 as (dix, diy, diz): k = 0..7 the route seeds' (dix, diy) table with
 *              diz = 0, k = 8..15 the same table with diz = +1, k = 16..23 with diz = -1,
 *              k = 24 (0, 0, +1), k = 25 (0, 0, -1).
 *   step       hx = dix ? dx : 0, hy = diy ? dy : 0, hz = diz ? (dz * kappa) : 0 (the product
 *              formed once), L_k = sqrt((hx*hx + hy*hy) + hz*hz).  kappa = z_scale is
 *              uam_vertical's unit, km of path length per metre of altitude change: the field's
 *              metric is the one the _v evaluations charge.  kappa is finite and > 0 (a zero
 *              vertical weight would give zero-weight edges and next-hop cycles).
 *   voxel cost c_v = 1.0 + lambda * (double)risk_v (the voxel's float32 risk).  A voxel is
 *              blocked0 when (the column's flags & block_flags) != 0, or c_v is not finite, or
 *              c_v is not > 0, or z0 + ((double)iz + 0.5)*dz < (double)terrain + agl (the
 *              column plane's float32 terrain; agl finite and >= 0, metres; with agl = 0 this
 *              is uam_eval_waypoints3d's below_terrain test).  A voxel is blocked when a
 *              blocked0 voxel of the same layer lies within Chebyshev distance inflate of it in
 *              x/y (voxels outside the volume do not count).  Otherwise it is free.
 *   edges      between voxels u, v that differ by a direction, when every voxel of the
 *              axis-aligned box the two span (2, 4 or 8 voxels) is free: the route seeds'
 *              corner rule generalised, so every point of a step's segment lies in a free voxel
 *              and a one-voxel-thick diagonal sheet is a wall.  w(u,v) = (0.5 * (c_u + c_v)) *
 *              L_k, symmetric.
 *   field, next hop, path status, steps
 *              the route seeds' text with "cell" read as "voxel": dist is the left-fold minimum,
 *              the one fixed point of d[v] = min(d[v], fl(d[u] + w(u,v))); next is uint8, the
 *              lowest k whose neighbour attains dist[v], 26 at the goal voxel, 255 where dist is
 *              +inf; status 4 / 1 / 2 / 3 / 0 tested in that order (4 bad goal index or goal
 *              outside the volume or blocked, 1 start outside the volume or blocked, 2
 *              unreachable, 3 the walk visited nx*ny*nz voxels without reaching the goal, 0 ok);
 *              steps = the voxels the walk visited, s and g included, 0 for a nonzero status.
 *   vertices   V_0 = the start point (x, y, z) itself, then the centres of the visited voxels
 *              strictly between s and g, V_m = the goal point itself.  S_0 = 0, S_i = S_{i-1} +
 *              sqrt((ex*ex + ey*ey) + ez*ez) with (ex, ey) = the x/y differences of V_i and
 *              V_{i-1} and ez = (z_i - z_{i-1}) * kappa (the difference first, then one product,
 *              as in uam_vertical).  The choice of segment, the parameter u and the
 *              interpolation are the route seeds', applied to all three components; a nonzero
 *              status gives the straight line in all three components with the end points
 *              copied (a goal index out of range: every waypoint is the start point).
 *   bridge     nz = 1, a volume built from a raster with layer_w = 1, the layer centre above
 *              every terrain value, agl = 0: dist equals uam_route_field's bit for bit
 *              (sqrt(dx*dx) = dx unless the square overflows or underflows), and next agrees
 *              wherever uam_route_field's value is < 8.
 *
 * uam_route3d_params: lambda, block_flags, inflate and max_rounds as uam_route_params' (max_rounds
 * 0 = nx*ny*nz); agl finite and >= 0; z_scale finite and > 0.
 * uam_route3d_field: vol_dev is the volume buffer of uam_volume_shape / uam_volume_build (8-B
 * voxels {float risk, float psi_nfz} [ny][nx][nz], then at col_offset the 8-B columns {float
 * terrain, uint32 flags} [ny][nx]; 256-B aligned; the column bitmap behind them is not read, so
 * a test may fill the buffer by hand); goals_dev [n_goals][3]; dist_dev [n_goals][ny][nx][nz]
 * f64 and next_dev likewise u8; workspace_dev holds uam_route3d_workspace_bytes(desc, params)
 * bytes, 256-B aligned (the cost plane and the 26-bit admissible-direction masks, shared by the
 * goals, and the active-tile sets).  Rounds as uam_route_field: one ordinary launch per round
 * over the active tiles, the host reading one word after each.  rounds_out (host, may be NULL):
 * the rounds of all goals together; uam_route3d_visits: the tiles those rounds visited.
 * uam_last_kernel: "K9v".  Failures: UAM_E_INVALID before any launch or allocation for ctx / desc
 * / params / a buffer NULL, a bad descriptor, lambda NaN, infinite or negative, inflate outside
 * [0, 8], max_rounds < 0, agl NaN, negative or infinite, z_scale not finite or not > 0, n_goals
 * < 1 or n_goals * nx * ny * nz >= 2^40, a workspace too small, a misaligned buffer;
 * UAM_E_VERSION for a wrong abi_version; UAM_E_STATE, the message naming max_rounds, when a field
 * has not converged -- the outputs are then unspecified and the context stays usable.
 * uam_route3d_paths: Q queries (starts_dev [Q][3], goal_idx_dev [Q]) against next_dev as
 * uam_route3d_field wrote it for the same desc, vol_dev, params (the start's blocking is derived
 * again from vol_dev and params) and goals_dev, into wp3_dev [Q][N+2][3], status_dev [Q] and
 * steps_dev [Q] (or NULL); N from uam_set_params (UAM_E_STATE without it).  One lane per query,
 * two sequential walks.  uam_last_kernel: "K9vt".
 * The _host calls take host pointers and run, without a GPU, the same inline functions as the
 * kernels (the field's minimum by a heap Dijkstra).
 * UAM_OPT_K9V_TILE_XY (8 (default), 16), UAM_OPT_K9V_TILE_Z (4 (default), 8) and
 * UAM_OPT_K9V_INNER (1..256, default 64) choose
 * the tile and the sweeps inside a tile per round; no output depends on them (rounds and visits
 * do). */
typedef struct {
    uint32_t abi_version; /* UAM_ABI_VERSION */
    double lambda;        /* weight of the risk in the voxel cost; finite, >= 0 */
    uint32_t block_flags; /* UAM_FLAG_* bits of the column that block its voxels */
    int32_t inflate;      /* voxels of x/y clearance around a blocked0 voxel, 0..8 */
    int32_t max_rounds;   /* 0 = nx*ny*nz */
    double agl;           /* metres a layer centre must lie above the terrain; finite, >= 0 */
    double z_scale;       /* kappa, km of path length per metre of altitude; finite, > 0 */
} uam_route3d_params;
int64_t uam_route3d_workspace_bytes(const uam_volume_desc* desc,
                                    const uam_route3d_params* params);
int uam_route3d_field(uam_ctx* ctx, const uam_volume_desc* desc, const void* vol_dev,
                      const uam_route3d_params* params, const double* goals_dev, int32_t n_goals,
                      double* dist_dev, uint8_t* next_dev, void* workspace_dev,
                      int64_t workspace_bytes, int32_t* rounds_out, uam_stream stream);
int64_t uam_route3d_visits(const uam_ctx* ctx);
int uam_route3d_paths(uam_ctx* ctx, const uam_volume_desc* desc, const void* vol_dev,
                      const uam_route3d_params* params, const uint8_t* next_dev,
                      const double* goals_dev, int32_t n_goals, const double* starts_dev,
                      const int32_t* goal_idx_dev, int64_t n_queries, double* wp3_dev,
                      int32_t* status_dev, int32_t* steps_dev, uam_stream stream);
int uam_route3d_field_host(const uam_volume_desc* desc, const void* vol,
                           const uam_route3d_params* params, const double* goals,
                           int32_t n_goals, double* dist, uint8_t* next);
int uam_route3d_paths_host(const uam_volume_desc* desc, const void* vol,
                           const uam_route3d_params* params, const uint8_t* next,
                           const double* goals, int32_t n_goals, const double* starts,
                           const int32_t* goal_idx, int64_t n_queries, int32_t N, double* wp3,
                           int32_t* status, int32_t* steps);

/* Route seeds in the volume, smoothing (K9vb / K9vs): any-angle shortcuts on the traced 3-D
 * path.  A 26-connected route turns by 45 degrees per kink in plan view and flies every altitude
 * change at the grid's own angle, one layer per voxel step; these calls keep of the traced voxel
 * chain only the voxels from which the next one kept is no longer in straight sight, and
 * resample that polyline.  "Route seeds, smoothing" above, restated over voxels.
 *
 * Definition (normative; independent statement: tests/route3d_smooth_ref.py).  The trace is
 * uam_route3d_paths': the status rules, steps and the voxel chain c_0 = s, c_1, .., c_{n-1} = g
 * along next (n = steps) are unchanged.  Smoothing chooses a subsequence of the interior voxels;
 * the vertices and the resampling are uam_route3d_paths' own rules applied to that subsequence.
 * Integer arithmetic alone decides every visibility; the float64 operations are
 * uam_route3d_paths', in its order, each rounded separately.
 *   touched    for voxels A, B (integer triples), d = B - A, and a voxel p with r = p - A:
 *              T3(A, B) is the set of voxels in the integer bounding box of A and B with
 *                  2*|dx*ry - dy*rx| <= |dx| + |dy|,
 *                  2*|dx*rz - dz*rx| <= |dx| + |dz| and
 *                  2*|dy*rz - dz*ry| <= |dy| + |dz|:
 *              the closed supercover of the segment between the two voxel centres (as
 *              separating axes of a segment against a box, the bounding box is the three face
 *              axes and the inequalities are the three edge-cross-direction axes; a segment
 *              through a voxel corner touches all eight voxels around it).  For a single
 *              direction step T3 is the 2-, 4- or 8-voxel box of the edge rule; with dz = 0 it
 *              is T.  Integers only; |dx|, |dy|, |dz| <= span <= 1024, every product < 2^22.
 *   visible    LOS3(A, B) holds iff every voxel of T3(A, B) is free (not blocked in
 *              uam_route3d_field's sense, inflation included).  Adjacent chain voxels are
 *              always visible, by the edge rule.
 *   anchors    none for n <= 2.  Otherwise a_0 = 1; a_{k+1} = the largest j <= min(a_k + span,
 *              n - 2) such that LOS3(c_{a_k}, c_i) holds for every i in (a_k, j] ("advance
 *              while visible", not "the farthest visible"; never less than a_k + 1); stop at
 *              a_k = n - 2.  c_1 and c_{n-2} are always kept: the start and goal points are no
 *              voxel centres, so the first and last segments stay the ones uam_route3d_paths
 *              flies.
 *   vertices   V_0 = the start point, the centres of c_{a_0}, c_{a_1}, .., V_m = the goal
 *              point.  S_i (ez = (z_i - z_{i-1}) * kappa, the difference first), the waypoints
 *              p_j in all three components, the straight line of a nonzero status and the
 *              status values: uam_route3d_paths' text, word for word.  vertices[q] = m + 1 (2 +
 *              the number of anchors); 0 for a nonzero status.
 *   guarantee  every point of a segment lies in a closed voxel of its T3, all free: every
 *              waypoint of a status-0 path lies in a free voxel.
 *   bridge     span = 1 keeps every interior voxel: wp3, status and steps are
 *              uam_route3d_paths' bits.
 *   second bridge
 *              nz = 1, the layer centre above every terrain value, agl = 0, start and goal z at
 *              the layer centre: status, steps, vertices and the x/y of wp3 equal
 *              uam_route_paths_smooth's on the equivalent raster bit for bit (ez = 0, and
 *              sqrt((ex*ex + ey*ey) + 0) = sqrt(ex*ex + ey*ey)).
 * The shortcut test is geometric: it does not weigh the risk along the segment, so a shortcut may
 * cut a climb to cheaper layers away; span bounds how far a shortcut may leave the field's route.
 *
 * uam_route3d_free_bits: the free voxels of (desc, vol_dev, params) as one bit per voxel, set =
 * free: bit v & 31 of word v >> 5, v = (iy*nx + ix)*nz + iz the voxel index (layer fastest: a
 * column's layers sit in one or two words), 4 * ((nx*ny*nz + 31) / 32) =
 * uam_route3d_free_bits_bytes(desc) bytes (-1 for a bad descriptor), 4-B aligned, the unused
 * bits of the last word 0.  uam_last_kernel: "K9vb".  Failures as uam_route3d_field's for ctx /
 * desc / params / a NULL or misaligned buffer.
 * uam_route3d_paths_smooth: uam_route3d_paths with shortcuts of at most span chain voxels, 1 <=
 * span <= UAM_ROUTE_SPAN_MAX, against bits_dev and next_dev of the same desc, vol and params
 * (the start's blocking is read from the bits; params is validated as in uam_route3d_field, but
 * only z_scale is used); steps_dev and vertices_dev may be NULL.  One wave per query; a query
 * with more than UAM_ROUTE_SMOOTH_LIST anchors is smoothed twice (no output depends on that).
 * Asynchronous.  uam_last_kernel: "K9vs".  UAM_E_INVALID before any launch for ctx / desc /
 * params / a required buffer NULL, a bad descriptor or parameter, span outside the range,
 * n_goals < 1 or too many voxels, nx*ny*nz > 2^31 - 1 - UAM_ROUTE_SPAN_MAX (voxel and chain
 * indices are int32), n_queries < 0 or too large; UAM_E_VERSION for a wrong abi_version;
 * UAM_E_STATE without uam_set_params.
 * The _host calls run the same inline functions without a GPU.  uam_route3d_visible_host: the
 * library's LOS3 on n pairs of voxel indices (UAM_E_INVALID for one off the volume) into out_u8
 * (1 = visible). */
int64_t uam_route3d_free_bits_bytes(const uam_volume_desc* desc);
int uam_route3d_free_bits(uam_ctx* ctx, const uam_volume_desc* desc, const void* vol_dev,
                          const uam_route3d_params* params, uint32_t* bits_dev,
                          uam_stream stream);
int uam_route3d_paths_smooth(uam_ctx* ctx, const uam_volume_desc* desc,
                             const uam_route3d_params* params, const uint32_t* bits_dev,
                             const uint8_t* next_dev, const double* goals_dev, int32_t n_goals,
                             const double* starts_dev, const int32_t* goal_idx_dev,
                             int64_t n_queries, int32_t span, double* wp3_dev,
                             int32_t* status_dev, int32_t* steps_dev, int32_t* vertices_dev,
                             uam_stream stream);
int uam_route3d_free_bits_host(const uam_volume_desc* desc, const void* vol,
                               const uam_route3d_params* params, uint32_t* bits);
int uam_route3d_paths_smooth_host(const uam_volume_desc* desc, const uam_route3d_params* params,
                                  const uint32_t* bits, const uint8_t* next, const double* goals,
                                  int32_t n_goals, const double* starts, const int32_t* goal_idx,
                                  int64_t n_queries, int32_t N, int32_t span, double* wp3,
                                  int32_t* status, int32_t* steps, int32_t* vertices);
int uam_route3d_visible_host(const uam_volume_desc* desc, const uint32_t* bits, int64_t n,
                             const int32_t* a_vox, const int32_t* b_vox, uint8_t* out_u8);

/* Route seeds in the volume, joint field (K9vj): one 3-D field to the nearest of many goals, with
 * an owner volume.  "Route seeds, joint field" above, restated over voxels: from this point of
 * the route, at this altitude, which vertiport is cheapest to reach, and along which 3-D route?
 * One relaxation, one f64 volume, one u8 volume and one int32 volume whatever the number of goals,
 * where uam_route3d_field pays a relaxation and a pair of volumes per goal.
 *
 * Definition (normative; independent statement: tests/route3d_joint_ref.py).  Voxels, the 26
 * directions, the step lengths with kappa = z_scale, the voxel cost, blocked0 and blocked (flags,
 * a non-finite or non-positive cost, agl, the inflation per layer), the box rule for edges and
 * w(u,v) = (0.5 * (c_u + c_v)) * L_k are the "Route seeds in the volume" text, unchanged.  Every
 * float64 operation is rounded separately, with no fused multiply-add.
 *   valid goal goal i is valid when its point maps to a voxel g_i of the volume and that voxel is
 *              free.  Gc is the set of voxels of the valid goals.  Several goals may share a
 *              voxel.  Gc may be empty.
 *   field      dist[v] = 0 for v in Gc; elsewhere the minimum, over edge paths that start in any
 *              voxel of Gc and end in v, of the left fold fl(fl(0 + w_01) + w_12) + ..; +inf for
 *              blocked and unreachable voxels, and everywhere when Gc is empty.  It is the one
 *              fixed point of d[v] = min(d[v], fl(d[u] + w(u,v))) started from 0 on Gc and +inf
 *              elsewhere: the bits do not depend on the tile shape, the sweeps per round or the
 *              schedule.
 *   next hop   uint8 per voxel, formed after convergence: 26 at every voxel of Gc (the test is
 *              membership in Gc, not dist == 0), 255 where dist is +inf, otherwise the lowest k
 *              whose neighbour u_k has an edge to v with fl(dist[u_k] + w(u_k, v)) == dist[v].
 *   owner      int32 per voxel, laid out [ny][nx][nz]: -1 where next is 255; at a voxel of Gc the
 *              lowest index i with g_i = v; otherwise the owner of the first voxel of Gc on the
 *              chain v -> v + dir(next[v]) -> ..; -1 when the chain visits nx*ny*nz voxels
 *              without reaching Gc (only where huge costs absorb small weights and equal dist
 *              values form a cycle).  Ties between goals are broken by the next-hop rule alone,
 *              never by a comparison of per-goal distances.
 *   owner      if owner[v] = i >= 0 then dist[v] == dist_i[v] bit for bit, dist_i being goal i's
 *   property   own uam_route3d_field volume.
 *   path       a query is a start point [3] only.  Status, tested in this order:
 *                1  the start is outside the volume or in a blocked voxel;
 *                2  next[s] = 255 (with no valid goal every free start gets 2);
 *                3  owner[s] = -1 although dist[s] is finite;
 *                0  ok.  There is no status 4.
 *              Status 0: goal_out[q] = o = owner[s], the goal point is goals[o], and the chain,
 *              steps, vertices, S_i (ez = (z_i - z_{i-1}) * kappa), waypoints and (span >= 1)
 *              anchors are uam_route3d_paths' and uam_route3d_paths_smooth's text word for word,
 *              along the joint next from s to g_o.  vertices[q] at span 0 counts every interior
 *              voxel: max(steps, 2), span 1's value.  A nonzero status: goal_out[q] = -1, steps =
 *              0, vertices = 0 and every waypoint is the start point.
 *   guarantee  every waypoint of a status-0 path lies in a free voxel.
 *   bridge 1   dist equals the elementwise minimum over i of the volumes uam_route3d_field writes
 *              for the same goals, bit for bit (an invalid goal's volume is all +inf).
 *   bridge 2   with n_goals = 1, dist and next are uam_route3d_field's bits.
 *   bridge 3   with n_goals = 1, status, steps and vertices equal uam_route3d_paths' (span 0) and
 *              uam_route3d_paths_smooth's (span >= 1) with goal_idx = 0 for every query whose
 *              status there is not 4; the waypoints are equal as well for status 0.
 *   bridge 4   nz = 1, a volume built from a raster as in "Route seeds in the volume"'s bridge,
 *              agl = 0: dist and owner equal uam_route_field_joint's bits on the equivalent
 *              raster, and next agrees wherever the flat value is < 8.
 *
 * uam_route3d_field_joint: goals_dev [n_goals][3] into dist_dev [ny][nx][nz] f64, next_dev
 * likewise u8 and owner_dev likewise int32; workspace_dev holds
 * uam_route3d_joint_workspace_bytes(desc, params, n_goals) bytes (-1 for bad arguments), 256-B
 * aligned: uam_route3d_field's workspace and an int32 parent volume.  One start state for all
 * goals (the distinct tiles of Gc form the first active set), then uam_route3d_field's rounds with
 * its kernel, UAM_OPT_K9V_TILE_XY / _TILE_Z / _INNER and max_rounds (the call may synchronise the
 * stream between rounds); the owner by pointer jumping over the parent volume,
 * ceil(log2(nx*ny*nz)) ordinary launches with no host read between them.  rounds_out and
 * uam_route3d_visits as for uam_route3d_field.  uam_last_kernel: "K9vj".
 * uam_route3d_paths_joint: Q start points against next_dev, owner_dev and goals_dev of one
 * uam_route3d_field_joint call, into wp3_dev [Q][N+2][3], status_dev [Q] and (each may be NULL)
 * steps_dev, vertices_dev, goal_out_dev [Q].  span = 0: the plain trace, one lane per query, the
 * start's blocking derived from vol_dev, bits_dev may be NULL; uam_last_kernel "K9vjt".  1 <= span
 * <= UAM_ROUTE_SPAN_MAX: shortcuts as uam_route3d_paths_smooth makes them, one wave per query, the
 * blocking from bits_dev (uam_route3d_free_bits of the same desc, vol, params), vol_dev may be
 * NULL; uam_last_kernel "K9vjs".  Asynchronous.  N from uam_set_params.
 * Failures: uam_route3d_field's and uam_route3d_paths_smooth's lists, UAM_E_INVALID before any
 * launch or allocation; in addition n_goals < 1 or > 2^20, nx*ny*nz > 2^31 - 1 -
 * UAM_ROUTE_SPAN_MAX (parents and owners are int32), owner_dev NULL or not 4-B aligned, span
 * outside [0, UAM_ROUTE_SPAN_MAX].  UAM_E_VERSION for a wrong abi_version.  UAM_E_STATE, the
 * message naming max_rounds, when the field has not converged within max_rounds rounds (outputs
 * unspecified, the context stays usable), and for uam_route3d_paths_joint without
 * uam_set_params.
 * The _host calls run the same inline functions without a GPU: the field's minimum by a heap
 * Dijkstra seeded with all of Gc, the owner by following the chains. */
int64_t uam_route3d_joint_workspace_bytes(const uam_volume_desc* desc,
                                          const uam_route3d_params* params, int32_t n_goals);
int uam_route3d_field_joint(uam_ctx* ctx, const uam_volume_desc* desc, const void* vol_dev,
                            const uam_route3d_params* params, const double* goals_dev,
                            int32_t n_goals, double* dist_dev, uint8_t* next_dev,
                            int32_t* owner_dev, void* workspace_dev, int64_t workspace_bytes,
                            int32_t* rounds_out, uam_stream stream);
int uam_route3d_paths_joint(uam_ctx* ctx, const uam_volume_desc* desc, const void* vol_dev,
                            const uam_route3d_params* params, const uint32_t* bits_dev,
                            const uint8_t* next_dev, const int32_t* owner_dev,
                            const double* goals_dev, int32_t n_goals, const double* starts_dev,
                            int64_t n_queries, int32_t span, double* wp3_dev,
                            int32_t* status_dev, int32_t* steps_dev, int32_t* vertices_dev,
                            int32_t* goal_out_dev, uam_stream stream);
int uam_route3d_field_joint_host(const uam_volume_desc* desc, const void* vol,
                                 const uam_route3d_params* params, const double* goals,
                                 int32_t n_goals, double* dist, uint8_t* next, int32_t* owner);
int uam_route3d_paths_joint_host(const uam_volume_desc* desc, const void* vol,
                                 const uam_route3d_params* params, const uint32_t* bits,
                                 const uint8_t* next, const int32_t* owner, const double* goals,
                                 int32_t n_goals, const double* starts, int64_t n_queries,
                                 int32_t N, int32_t span, double* wp3, int32_t* status,
                                 int32_t* steps, int32_t* vertices, int32_t* goal_out);

/* Workspace bytes uam_refine needs for n_paths (after uam_set_geometry/uam_set_params). */
int64_t uam_refine_workspace_bytes(uam_ctx* ctx, int64_t n_paths,
                                   const uam_refine_params* params);
/* Refines wp_dev [P][N+2][2] in place (endpoints fixed); per path: final cost (get_cost),
 * final sum of squared constraint rows, gradient steps taken.  Any output may be NULL. */
int uam_refine(uam_ctx* ctx, double* wp_dev, int64_t n_paths, const uam_refine_params* params,
               void* workspace_dev, int64_t workspace_bytes, double* cost_dev,
               double* infeas_dev, int32_t* iters_dev, uam_stream stream);

#ifdef __cplusplus
}
#endif

#endif /* UAMPATH_H */
