"""Device engine: one libuampath context per GPU, torch tensors as device buffers.

PyTorch is plumbing here (allocation, streams, H2D/D2H); every arithmetic step of the hot path
runs in the hand-written HIP kernels of csrc/uampath.hip.  There is no CPU fallback: without a
visible GPU or without libuampath.so, constructing an Engine raises.
"""
import collections
import ctypes
import os
from dataclasses import dataclass, field

import numpy as np

from . import _lib
from .geometry import FlatGeometry, compile_map, compile_shapes


def _torch():
    import torch

    return torch


@dataclass
class PathParams:
    """Problem options + the OpEn parameter vector p (solver.py:60-78, problem.py:12-22)."""
    N: int
    length_smooth: bool = False
    penalty_smooth: bool = True
    obstacle_smooth: bool = False
    maxratio_smooth: bool = False
    maxratio: float = 1.0
    maxalpha: float = 0.0
    enlargement: float = 0.0
    weights: tuple = ()
    quirk_length: bool = True
    anchor: tuple = None          # map.x_start baked into a reference build; None = p_0
    altitude: float = 150.0       # cruise altitude (m) for min-clearance in raster mode

    def as_struct(self):
        w = [float(x) for x in self.weights]
        if len(w) > _lib.MAX_REGIONS:
            raise ValueError(f"at most {_lib.MAX_REGIONS} region weights")
        arr = (ctypes.c_double * _lib.MAX_REGIONS)(*(w + [1.0] * (_lib.MAX_REGIONS - len(w))))
        a = self.anchor
        return _lib.Params(_lib.ABI_VERSION, int(self.N), int(bool(self.length_smooth)),
                           int(bool(self.penalty_smooth)), int(bool(self.obstacle_smooth)),
                           int(bool(self.maxratio_smooth)), int(bool(self.quirk_length)),
                           0 if a is None else 1, 0.0 if a is None else float(a[0]),
                           0.0 if a is None else float(a[1]), float(self.maxratio),
                           float(self.maxalpha), float(self.enlargement), float(self.altitude),
                           arr)


@dataclass
class RasterGeo:
    """GeoTIFF-convention geotransform of the cost raster (row 0 = north edge)."""
    nx: int
    ny: int
    x0: float
    y_top: float
    dx: float
    dy: float
    nodata: float = -9999.0
    dem_threshold: float = 0.0

    def as_struct(self):
        return _lib.RasterDesc(int(self.nx), int(self.ny), float(self.x0), float(self.y_top),
                               float(self.dx), float(self.dy), float(self.nodata),
                               float(self.dem_threshold))

    def cell_centres(self):
        ix = np.arange(self.nx, dtype=np.float64)
        iy = np.arange(self.ny, dtype=np.float64)
        return self.x0 + (ix + 0.5) * self.dx, self.y_top - (iy + 0.5) * self.dy


@dataclass
class CostRaster:
    """Device record raster: rec [ny, nx, 4] int32 view of {phi f32, psi f32, dem f32, flags};
    summary: the K2 gather-skip bitmap of rec (uam_raster_summary, one bit per block x block
    cells; None = K2 gathers every waypoint); packed: the K2s packed copy of rec
    (uam_raster_pack, 8-B planes in 4 x 4-cell blocks; None = K2s gathers rec).  Rebuild both
    (Engine.raster_summary) after rec changes.  sum_scale: the raster's exponents and flags for
    the exact sums (Engine.raster_sum_scale: [4] int32 {e_phi, e_psi, flags, 0}; None until an
    evaluation with the "exact_sum" option needs it; raster_summary resets it)."""
    geo: RasterGeo
    rec: object = field(repr=False)
    summary: object = field(default=None, repr=False)
    block: int = 0
    packed: object = field(default=None, repr=False)  # uam_raster_pack copy for K2s (or None)
    sum_scale: object = field(default=None, repr=False)  # uam_raster_sum_scale words (or None)

    @property
    def nbytes(self):
        return self.geo.nx * self.geo.ny * _lib.RECORD_BYTES


@dataclass
class VolumeGeo:
    """3-D risk volume grid (config 5): the raster's x/y grid x nz altitude layers (m)."""
    nx: int
    ny: int
    nz: int
    x0: float
    y_top: float
    dx: float
    dy: float
    z0: float
    dz: float

    def as_struct(self):
        return _lib.VolumeDesc(int(self.nx), int(self.ny), int(self.nz), float(self.x0),
                               float(self.y_top), float(self.dx), float(self.dy),
                               float(self.z0), float(self.dz))


@dataclass
class Vertical:
    """The vertical terms of eval_waypoints3d / eval_generated3d_profiles (uam_vertical):
    z_scale km of path length per metre of altitude change (1e-3: isotropic), sin_climb /
    sin_descent the largest climb / descent per unit of 3-D path length (inf: no limit;
    profiles.sin_of_angle gives one from an angle)."""
    z_scale: float
    sin_climb: float = float("inf")
    sin_descent: float = float("inf")

    def as_struct(self):
        return _lib.Vertical(_lib.ABI_VERSION, float(self.z_scale), float(self.sin_climb),
                             float(self.sin_descent))


@dataclass
class RiskVolume:
    geo: VolumeGeo
    buf: object = field(repr=False)     # the device buffer (uam_volume_shape bytes)
    vox: object = field(repr=False)     # [ny, nx, nz, 2] int32 view: 8-B voxels {risk, psi}
    cols: object = field(repr=False)    # [ny, nx, 2] int32 view: columns {terrain, flags}
    cbits: object = field(repr=False, default=None)  # int32 view: the column bitmap words
    # the packed copy K4h reads (Engine.volume_pack: 4-B / 8-B / 16-B voxel planes in 4 x 8-
    # column blocks per layer, codes, terrain bounds), or None; eval_generated3d rebuilds it
    # when buf (or a view of it: vox, cols) was written in place since (torch's version counter)
    packed: object = field(repr=False, default=None)
    packed_version: int = field(repr=False, default=-1)
    # the voxels' exponents and flags for the exact sums (Engine.volume_sum_scale: [4] int32
    # {e_risk, e_psi, flags, 0}); None until an evaluation with the "exact_sum_volume" option
    # needs it, recomputed by the rule that repacks the packed copy; volume_pack resets it
    sum_scale: object = field(repr=False, default=None)
    sum_scale_version: int = field(repr=False, default=-1)


@dataclass
class RouteField:
    """The cost-to-go fields of some goals on a cost raster (Engine.route_field, K9;
    include/uampath.h "Route seeds"): dist [G, ny, nx] float64 (+inf: blocked or unreachable),
    next [G, ny, nx] uint8 (direction 0..7 = E, NE, N, NW, W, SW, S, SE; 8 = the goal cell;
    255 = no route), goals [G, 2], rounds = relaxation rounds of all goals together, visits =
    tiles those rounds visited.  rec and the parameters are kept for route_paths (the start's
    blocking is read from rec).  Device tensors from route_field, numpy arrays from
    route_field_host.  A derived, untracked product of rec: rebuild it when rec changes.
    free_bits: the free cells as one bit per cell ([ny, (nx + 31) // 32] 32-bit words;
    Engine.route_free_bits), built and kept here by the first route_paths(..., smooth >= 1).
    joint = True (route_field(..., joint=True), K9j; "Route seeds, joint field"): one field to the
    nearest of the goals, dist and next [1, ny, nx] (8 at every valid goal's cell), and owner
    [ny, nx] int32: the index of the goal a cell's route ends at, -1 where there is none."""
    geo: RasterGeo
    goals: object = field(repr=False)
    dist: object = field(repr=False)
    next: object = field(repr=False)
    rounds: int = 0
    visits: int = 0
    rec: object = field(default=None, repr=False)
    lam: float = 1.0
    block_flags: int = _lib.FLAG_NFZ
    inflate: int = 0
    free_bits: object = field(default=None, repr=False)
    owner: object = field(default=None, repr=False)
    joint: bool = False

    def params(self, max_rounds=0):
        return _route_params(self.lam, self.block_flags, self.inflate, max_rounds)


def _route_params(lam, block_flags, inflate, max_rounds):
    return _lib.RouteParams(_lib.ABI_VERSION, float(lam), int(block_flags), int(inflate),
                            int(max_rounds))


@dataclass
class RouteField3D:
    """The cost-to-go fields of some goals over a risk volume's voxels (Engine.route_field3d,
    K9v; include/uampath.h "Route seeds in the volume"): dist [G, ny, nx, nz] float64 (+inf:
    blocked or unreachable), next [G, ny, nx, nz] uint8 (direction 0..25; 26 = the goal voxel;
    255 = no route), goals [G, 3], rounds / visits as RouteField's.  vol (the volume buffer)
    and the parameters are kept for route_paths3d (the start's blocking is derived from them).
    Device tensors from route_field3d, numpy arrays from route_field3d_host.  A derived,
    untracked product of the volume: rebuild it when the voxels or columns change.
    free_bits: the free voxels as one bit per voxel ([(nx*ny*nz + 31) // 32] 32-bit words, bit
    v & 31 of word v >> 5 for the voxel index v; Engine.route_free_bits3d), built and kept here
    by the first route_paths3d(..., smooth >= 1).
    joint = True (route_field3d(..., joint=True), K9vj; "Route seeds in the volume, joint field"):
    one field to the nearest of the goals, dist and next [1, ny, nx, nz] (26 at every valid goal's
    voxel), and owner [ny, nx, nz] int32: the index of the goal a voxel's route ends at, -1 where
    there is none."""
    geo: VolumeGeo
    goals: object = field(repr=False)
    dist: object = field(repr=False)
    next: object = field(repr=False)
    rounds: int = 0
    visits: int = 0
    vol: object = field(default=None, repr=False)
    lam: float = 1.0
    block_flags: int = _lib.FLAG_NFZ
    inflate: int = 0
    agl: float = 0.0
    z_scale: float = 1e-3
    free_bits: object = field(default=None, repr=False)
    owner: object = field(default=None, repr=False)
    joint: bool = False

    def params(self, max_rounds=0):
        return _route3d_params(self.lam, self.block_flags, self.inflate, self.agl,
                               self.z_scale, max_rounds)


def _route3d_params(lam, block_flags, inflate, agl, z_scale, max_rounds):
    return _lib.Route3dParams(_lib.ABI_VERSION, float(lam), int(block_flags), int(inflate),
                              int(max_rounds), float(agl), float(z_scale))


def _option_key(name):
    for table in (_lib.ROUTE_OPTIONS, _lib.ROUTE3D_OPTIONS):
        if name in table:
            return table[name]
    return _lib.OPTIONS[name]


def _host_vol(vol, geo):
    """A volume buffer as contiguous 32-bit words on the host: the voxels and, at the 256-B
    aligned column offset, the column plane (include/uampath.h uam_volume_desc)."""
    v = np.ascontiguousarray(vol).reshape(-1)
    col_off = (geo.nx * geo.ny * geo.nz * 8 + 255) // 256 * 256
    if v.dtype.itemsize != 4 or v.size * 4 < col_off + geo.nx * geo.ny * 8:
        raise ValueError(f"vol must hold 32-bit words: {geo.ny}x{geo.nx}x{geo.nz} 8-B voxels "
                         f"and, at byte {col_off}, {geo.ny}x{geo.nx} 8-B columns")
    return v


def _host_rec(rec, geo):
    """A record raster as contiguous 16-B records on the host ([ny, nx, 4] 32-bit words)."""
    r = np.ascontiguousarray(rec)
    if r.dtype.itemsize != 4 or r.size != geo.ny * geo.nx * 4:
        raise ValueError(f"rec must hold [{geo.ny}, {geo.nx}, 4] 32-bit words")
    return r


def _ptr(t):
    return ctypes.c_void_p(0 if t is None else t.data_ptr())


def _check_outputs(o, P, Q, W):
    """Caller-supplied outputs (Engine.outputs) must hold this batch: the kernels write P paths
    and Q best indices, so a smaller buffer set would be overrun."""
    for k, t in o.items():
        need = P * W if k == "cells" else (Q if k.startswith("best_") else P)
        if k == "g_rows":
            continue
        if t.numel() < need:
            raise ValueError(f"outputs[{k!r}] holds {t.numel()} entries, this batch needs {need}"
                             f" ({P} paths, {Q} pairs): allocate with Engine.outputs")


# refinement defaults (same as oracle.refine_params)
REFINE_DEFAULTS = dict(n_outer=15, n_inner=50, max_backtrack=30, c0=10.0, rho=5.0, c_max=1e8,
                       alpha0=1e-4, armijo=1e-4, theta=0.25, max_step=0.5, memory=8,
                       inner_tol=1e-3, delta=1e-4, n_restart=0, restart_margin=0.05)


class Engine:
    """libuampath context bound to one GPU."""

    def __init__(self, device=0):
        torch = _torch()
        if not torch.cuda.is_available():
            raise RuntimeError("no GPU visible: uam_path_planning_amd runs only on the HIP "
                               "kernels of libuampath.so (there is no CPU path)")
        self.lib = _lib.load()
        self.device = int(device)
        self.torch_device = torch.device("cuda", self.device)
        h = ctypes.c_void_p()
        _lib.check(self.lib.uam_ctx_create(self.device, ctypes.byref(h)), "uam_ctx_create")
        self._ctx = h
        self._geom_sig = None
        self._exact_sum = False   # the "exact_sum" option as set_option last set it
        self._exact_sum_volume = False   # "exact_sum_volume" likewise
        self.geometry = None
        self.params = None

    def __del__(self):
        try:
            if getattr(self, "_ctx", None):
                self.lib.uam_ctx_destroy(self._ctx)
                self._ctx = None
        except Exception:
            pass

    # -- helpers --------------------------------------------------------------------------
    @property
    def stream(self):
        return ctypes.c_void_p(_torch().cuda.current_stream(self.device).cuda_stream)

    def tensor(self, x, dtype):
        torch = _torch()
        if isinstance(x, torch.Tensor):
            t = x.to(device=self.torch_device, dtype=dtype)
        else:
            t = torch.as_tensor(np.asarray(x), dtype=dtype, device=self.torch_device)
        return t.contiguous()

    def empty(self, shape, dtype):
        return _torch().empty(shape, dtype=dtype, device=self.torch_device)

    # -- state ----------------------------------------------------------------------------
    def set_geometry(self, geom):
        if not isinstance(geom, FlatGeometry):
            geom = compile_map(geom)
        sig = geom.signature()
        if sig != self._geom_sig:
            _lib.check(self.lib.uam_set_geometry(self._ctx, ctypes.byref(geom.as_struct())),
                       "uam_set_geometry")
            self._geom_sig = sig
            self.params = None
        self.geometry = geom
        return geom

    def set_params(self, params):
        if params != self.params:
            _lib.check(self.lib.uam_set_params(self._ctx, ctypes.byref(params.as_struct()),
                                               self.stream), "uam_set_params")
            self.params = params
        return params

    # -- points ---------------------------------------------------------------------------
    def eval_points(self, pts, want=("phi", "phi_regions", "obs_norm", "psi_raw", "collide")):
        torch = _torch()
        p = self.tensor(pts, torch.float64).reshape(-1, 2)
        n = p.shape[0]
        R = self.geometry.n_regions
        out = {}
        if "phi" in want:
            out["phi"] = self.empty((n,), torch.float64)
        if "phi_regions" in want:
            out["phi_regions"] = self.empty((n, R), torch.float64)
        if "obs_norm" in want:
            out["obs_norm"] = self.empty((n,), torch.float64)
        if "psi_raw" in want:
            out["psi_raw"] = self.empty((n,), torch.float64)
        if "collide" in want:
            out["collide"] = self.empty((n,), torch.int32)
        _lib.check(self.lib.uam_eval_points(
            self._ctx, _ptr(p), n, _ptr(out.get("phi")), _ptr(out.get("phi_regions")),
            _ptr(out.get("obs_norm")), _ptr(out.get("psi_raw")), _ptr(out.get("collide")),
            self.stream), "uam_eval_points")
        return out

    # -- raster ---------------------------------------------------------------------------
    def raster_build(self, geo, dem=None, out=None, summary=True, packed=True):
        """K1 record raster (+ its K2 gather-skip summary and, with packed, the K2s packed copy,
        unless summary=False)."""
        torch = _torch()
        d = None if dem is None else self.tensor(dem, torch.float32).reshape(geo.ny, geo.nx)
        rec = out if out is not None else self.empty((geo.ny, geo.nx, 4), torch.int32)
        _lib.check(self.lib.uam_raster_build(self._ctx, ctypes.byref(geo.as_struct()), _ptr(d),
                                             _ptr(rec), self.stream), "uam_raster_build")
        r = CostRaster(geo, rec)
        return self.raster_summary(r, packed=packed) if summary else r

    def raster_summary(self, raster, block=0, packed=True):
        """(Re)build raster.summary (and raster.packed unless packed=False; else it is dropped)
        from raster.rec (block 0 = automatic); returns raster.  Both are derived copies that
        are not tracked: call this again after any write to raster.rec (raster_build into it,
        a broadcast, a raw-pointer writer) -- distributed.broadcast_raster does."""
        torch = _torch()
        g = raster.geo.as_struct()
        b, nbx, nby = ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int32()
        _lib.check(self.lib.uam_raster_summary_shape(ctypes.byref(g), int(block), ctypes.byref(b),
                                                     ctypes.byref(nbx), ctypes.byref(nby)),
                   "uam_raster_summary_shape")
        sm = self.empty(((nby.value * nbx.value + 31) // 32,), torch.int32)
        _lib.check(self.lib.uam_raster_summary(self._ctx, ctypes.byref(g), _ptr(raster.rec),
                                               b.value, _ptr(sm), self.stream),
                   "uam_raster_summary")
        raster.summary, raster.block, raster.packed = sm, b.value, None
        raster.sum_scale = None   # rec changed: the exponents are derived from it too
        if packed:
            nbytes = ctypes.c_int64()
            _lib.check(self.lib.uam_raster_pack_shape(ctypes.byref(g), b.value, None,
                                                      ctypes.byref(nbytes)),
                       "uam_raster_pack_shape")
            pk = self.empty(((nbytes.value + 255) // 256, 256), torch.uint8)
            _lib.check(self.lib.uam_raster_pack(self._ctx, ctypes.byref(g), _ptr(raster.rec),
                                                b.value, _ptr(pk), self.stream),
                       "uam_raster_pack")
            raster.packed = pk
        return raster

    def raster_sum_scale(self, raster):
        """Fill raster.sum_scale, the exact sums' scale of raster.rec (uam_raster_sum_scale:
        [4] int32 {e_phi, e_psi, flags, 0} on the device, no host sync); returns raster.  A
        derived, untracked copy like the summary: raster_summary resets it, and eval_generated
        computes it when the "exact_sum" option is on and it is None."""
        torch = _torch()
        sc = self.empty((4,), torch.int32)
        _lib.check(self.lib.uam_raster_sum_scale(self._ctx, ctypes.byref(raster.geo.as_struct()),
                                                 _ptr(raster.rec), _ptr(sc), self.stream),
                   "uam_raster_sum_scale")
        raster.sum_scale = sc
        return raster

    @staticmethod
    def exact_sum_host(values, e=None):
        """The exact sum's definition (include/uampath.h) applied to float32 values on the host
        by the functions the kernels run (uam_exact_sum_host; needs no GPU): (sum, e) with e
        the exponent used -- derived from values when e is None."""
        v = np.ascontiguousarray(values, dtype=np.float32).reshape(-1)
        out, eo = ctypes.c_double(), ctypes.c_int32()
        _lib.check(_lib.load().uam_exact_sum_host(
            v.ctypes.data, v.size, -2 ** 31 if e is None else int(e), ctypes.byref(out),
            ctypes.byref(eo)), "uam_exact_sum_host")
        return out.value, eo.value

    def read_tiles(self, paths, th, tw, n_threads=0, pinned=False):
        """GeoTIFF tiles -> host float32 [T, th, tw] (uam_read_tiles: parallel native reader;
        pinned=True reads into page-locked memory)."""
        torch = _torch()
        out = torch.empty((len(paths), th, tw), dtype=torch.float32, pin_memory=bool(pinned))
        arr = (ctypes.c_char_p * max(1, len(paths)))(*[os.fsencode(str(p)) for p in paths])
        _lib.check(self.lib.uam_read_tiles(arr, len(paths), int(th), int(tw),
                                           ctypes.c_void_p(out.data_ptr()), int(n_threads)),
                   "uam_read_tiles")
        return out

    def load_tiles(self, paths, th, tw, n_threads=0):
        """GeoTIFF tiles -> device float32 [T, th, tw] (uam_load_tiles: the parallel reader
        streaming ~32 MiB chunks through the context's page-locked buffers, each copied while
        the next is read)."""
        torch = _torch()
        out = self.empty((len(paths), th, tw), torch.float32)
        arr = (ctypes.c_char_p * max(1, len(paths)))(*[os.fsencode(str(p)) for p in paths])
        _lib.check(self.lib.uam_load_tiles(self._ctx, arr, len(paths), int(th), int(tw),
                                           _ptr(out), int(n_threads), self.stream),
                   "uam_load_tiles")
        return out

    def dem_mosaic(self, tiles, xoff, yoff, nx, ny, fill=-9999.0, dem=None):
        torch = _torch()
        t = self.tensor(tiles, torch.float32)
        nt, th, tw = t.shape
        xo = self.tensor(xoff, torch.int32)
        yo = self.tensor(yoff, torch.int32)
        if dem is None:
            dem = torch.full((ny, nx), float(fill), dtype=torch.float32, device=self.torch_device)
        _lib.check(self.lib.uam_dem_mosaic(self._ctx, _ptr(t), nt, th, tw, _ptr(xo), _ptr(yo),
                                           _ptr(dem), nx, ny, self.stream), "uam_dem_mosaic")
        return dem

    # -- paths ----------------------------------------------------------------------------
    def outputs(self, P, W, n_pairs=None, want_cells=False, want_g=False):
        """Preallocated per-path (and per-pair best-index) outputs, reusable across launches."""
        return self._outputs(P, W, None, want_cells, want_g, n_pairs)

    def kernel_timing(self, enable=True):
        """Start (and reset) or stop HIP-event timing of the path evaluation: the context records
        an event pair on the launch stream around every k_eval_pairs / k_eval_wave launch (not
        around K2's pair order or the selection kernels), and around the whole K2s sequence
        (its sorts, segment launches and output launch)."""
        _lib.check(self.lib.uam_kernel_timing(self._ctx, 1 if enable else 0),
                   "uam_kernel_timing")

    def kernel_time(self):
        """(total ms, launches) of the timed kernel launches since the last call / reset."""
        ms, n = ctypes.c_double(), ctypes.c_int64()
        _lib.check(self.lib.uam_kernel_time(self._ctx, ctypes.byref(ms), ctypes.byref(n)),
                   "uam_kernel_time")
        return ms.value, n.value

    def last_kernel(self):
        """Which path evaluation the last eval_generated / eval_generated3d ran (uam_last_kernel:
        "K2h+pack", "K2hx+pack" (the exact sums), "K2g+pack", "K4h+pack", "K4hx+pack" (the
        volume's exact sums), "K2s+pack", "K2+skip", "K2w", "K3b", ...), or the last
        eval_waypoints3d ("K4e" / "K4ew") / eval_generated3d_profiles ("K4p"; packed=True:
        "K4hp+pack", "K4hpx+pack" with the exact sums); with vertical= "K4e+v" / "K4ew+v" /
        "K4p+v"; eval_generated3d_profiles_hv: "K4hpv+pack", "K4hpxv+pack" with the exact sums."""
        return self.lib.uam_last_kernel(self._ctx).decode()

    def last_group(self):
        """Waypoint-group length of the last eval_generated / eval_generated3d's sums
        (uam_last_group): G > 0 when a segment-grouped evaluation ran -- K2h / K4h (the oracle's
        orc_eval_generated_h order) or K2g (orc_eval_paths_g) -- 0 = sequential.  With the
        "exact_sum" option G is still reported, but the raster sums do not depend on it
        ("exact_sum_volume": the volume's likewise)."""
        return int(self.lib.uam_last_group(self._ctx))

    def set_option(self, name, value):
        """uam_set_option (include/uampath.h UAM_OPT_*; the names are _lib.OPTIONS' keys):
        "group" (K2h / K2g / K4h waypoints per group, 0 = K2s / K4), "sorted_min_paths",
        "k2s_segments", "wave_max_paths", "pair_order", "k1_rows", "k3b_segment",
        "k3b_points_per_lane", "k8_tiled", "k8_streams", "k2g_tile_bits", "k2g_lds_floor",
        "k2g_chunk", "k2g_curve", "k2g_sim", "k4h_band", "k2h_lb_stride", "k2h_terrain",
        "k4h_terrain", "test_sort_fault" (tests only), "exact_sum" (1: K2h's raster sums as
        exact integers, independent of the group length -- "K2hx+pack") and "exact_sum_volume"
        (1: the same for K4h's voxel sums in eval_generated3d -- "K4hx+pack"); "k9_tile" (16,
        32, 64) and "k9_inner" (1..256; _lib.ROUTE_OPTIONS): route_field's tile edge and sweeps
        per round, which its outputs do not depend on; "k9v_tile_xy" (8, 16), "k9v_tile_z"
        (4, 8) and "k9v_inner" (1..256; _lib.ROUTE3D_OPTIONS): route_field3d's likewise."""
        key = _option_key(name)
        _lib.check(self.lib.uam_set_option(self._ctx, key, int(value)), "uam_set_option")
        if name == "exact_sum":
            self._exact_sum = bool(int(value))
        elif name == "exact_sum_volume":
            self._exact_sum_volume = bool(int(value))

    def get_option(self, name):
        v = ctypes.c_int64()
        key = _option_key(name)
        _lib.check(self.lib.uam_get_option(self._ctx, key, ctypes.byref(v)), "uam_get_option")
        return v.value

    def _outputs(self, P, W, mode, want_cells, want_g, n_pairs=None):
        torch = _torch()
        o = {k: self.empty((P,), torch.float64) for k in ("cost", "length_q", "length",
                                                           "kin_sum", "nfz_sum",
                                                           "min_clearance")}
        o["nfz_hits"] = self.empty((P,), torch.int32)
        o["offmap"] = self.empty((P,), torch.int32)
        o["below_terrain"] = self.empty((P,), torch.int32)
        if want_cells:
            o["cells"] = self.empty((P, W), torch.int32)
        if want_g:
            n_rows = 3 * (W - 2) + self.geometry.n_obstacles * W
            o["g_rows"] = self.empty((P, n_rows), torch.float64)
        if n_pairs is not None:
            o["best_fval_idx"] = self.empty((n_pairs,), torch.int32)
            o["best_length_idx"] = self.empty((n_pairs,), torch.int32)
        s = _lib.PathOutputs(*[ctypes.c_void_p(o[k].data_ptr()) if k in o else None
                               for k, _ in _lib.PathOutputs._fields_])
        return o, s

    def _mode(self, raster):
        return _lib.MODE_ANALYTIC if raster is None else _lib.MODE_RASTER

    def eval_waypoints(self, wp, raster=None, want_cells=False, want_g=False):
        """wp [P, N+2, 2] float64 (p_0 = start .. p_{N+1} = goal).  raster=None: analytic."""
        torch = _torch()
        N = self.params.N
        w = self.tensor(wp, torch.float64).reshape(-1, N + 2, 2)
        P = w.shape[0]
        o, s = self._outputs(P, N + 2, self._mode(raster), want_cells and raster is not None,
                             want_g and raster is None)
        geo = None if raster is None else ctypes.byref(raster.geo.as_struct())
        _lib.check(self.lib.uam_eval_waypoints(
            self._ctx, self._mode(raster), geo, _ptr(None if raster is None else raster.rec),
            _ptr(w), P, ctypes.byref(s), self.stream), "uam_eval_waypoints")
        return o

    def eval_generated(self, pairs, utab, raster=None, want_cells=False, outputs=None):
        """pairs [Q, 4] (x0, y0, xf, yf); utab [D, N, 2]; path p = q*D + d."""
        torch = _torch()
        pr = self.tensor(pairs, torch.float64).reshape(-1, 4)
        ut = self.tensor(utab, torch.float64)
        D = ut.shape[0]
        if ut.shape[1] != self.params.N:
            raise ValueError(f"arc table has N={ut.shape[1]}, params N={self.params.N}")
        Q = pr.shape[0]
        if outputs is None:
            o, s = self._outputs(Q * D, self.params.N + 2, self._mode(raster),
                                 want_cells and raster is not None, False, n_pairs=Q)
        else:
            o, s = outputs
            _check_outputs(o, Q * D, Q, self.params.N + 2)
        geo = None if raster is None else ctypes.byref(raster.geo.as_struct())
        rec = summary = packed = None
        block = 0
        if raster is not None:
            rec, summary, packed, block = raster.rec, raster.summary, raster.packed, raster.block
            if self._exact_sum:   # the exact sums' scale: computed once per rec, then handed over
                if raster.sum_scale is None:
                    self.raster_sum_scale(raster)
                _lib.check(self.lib.uam_set_sum_scale(self._ctx, _ptr(raster.sum_scale)),
                           "uam_set_sum_scale")
        _lib.check(self.lib.uam_eval_generated(
            self._ctx, self._mode(raster), geo, _ptr(rec), _ptr(summary), int(block or 0),
            _ptr(packed), _ptr(pr), Q, _ptr(ut), D, ctypes.byref(s), self.stream),
            "uam_eval_generated")
        return o

    # -- volume (config 5) -------------------------------------------------------------
    def volume_alloc(self, vg):
        """An uninitialised volume buffer of VolumeGeo vg (uam_volume_shape), e.g. for a rank
        that receives it by broadcast."""
        torch = _torch()
        nbytes, off = ctypes.c_int64(), ctypes.c_int64()
        _lib.check(self.lib.uam_volume_shape(ctypes.byref(vg.as_struct()), ctypes.byref(nbytes),
                                             ctypes.byref(off)), "uam_volume_shape")
        buf = self.empty((nbytes.value // 4,), torch.int32)   # caching allocator: 512-B aligned
        nv = vg.nx * vg.ny * vg.nz * 2
        vox = buf[:nv].view(vg.ny, vg.nx, vg.nz, 2)
        nc = vg.nx * vg.ny * 2
        cols = buf[off.value // 4: off.value // 4 + nc].view(vg.ny, vg.nx, 2)
        bits0 = off.value // 4 + (nc * 4 + 255) // 256 * 64
        return RiskVolume(vg, buf, vox, cols, buf[bits0:])

    def volume_build(self, raster, nz, z0, dz, layer_w):
        torch = _torch()
        g = raster.geo
        vg = VolumeGeo(g.nx, g.ny, int(nz), g.x0, g.y_top, g.dx, g.dy, float(z0), float(dz))
        lw = self.tensor(layer_w, torch.float64).reshape(-1)
        if lw.numel() != nz:
            raise ValueError(f"layer_w has {lw.numel()} entries, nz = {nz}")
        vol = self.volume_alloc(vg)
        _lib.check(self.lib.uam_volume_build(self._ctx, ctypes.byref(vg.as_struct()),
                                             _ptr(raster.rec), _ptr(lw), _ptr(vol.buf),
                                             self.stream), "uam_volume_build")
        return vol

    def volume_pack(self, volume):
        """Derive the packed copy K4h evaluates (uam_volume_pack) into volume.packed.
        eval_generated3d repacks by itself when torch's version counter of volume.buf moved;
        a write that bypasses torch (uam_volume_build into the same buffer, an RCCL broadcast
        through the C ABI, DLPack or ctypes writers) does not move it, so call this after
        one (distributed.broadcast_raster does)."""
        torch = _torch()
        nb = ctypes.c_int64()
        _lib.check(self.lib.uam_volume_packed_bytes(ctypes.byref(volume.geo.as_struct()),
                                                    ctypes.byref(nb)), "uam_volume_packed_bytes")
        packed = self.empty((nb.value // 4,), torch.int32)
        _lib.check(self.lib.uam_volume_pack(self._ctx, ctypes.byref(volume.geo.as_struct()),
                                            _ptr(volume.buf), _ptr(packed), self.stream),
                   "uam_volume_pack")
        volume.packed = packed
        volume.packed_version = volume.buf._version
        volume.sum_scale = None   # the voxels changed: the exponents are derived from them too
        return packed

    def volume_sum_scale(self, volume):
        """Fill volume.sum_scale, the exact sums' scale of the volume's voxels
        (uam_volume_sum_scale: [4] int32 {e_risk, e_psi, flags, 0} on the device, no host sync);
        returns volume.  A derived copy like the packed one: eval_generated3d computes it when
        the "exact_sum_volume" option is on and it is None or torch's version counter of
        volume.buf moved since; volume_pack -- the call after a write that bypasses torch --
        resets it."""
        torch = _torch()
        sc = self.empty((4,), torch.int32)
        _lib.check(self.lib.uam_volume_sum_scale(self._ctx, ctypes.byref(volume.geo.as_struct()),
                                                 _ptr(volume.buf), _ptr(sc), self.stream),
                   "uam_volume_sum_scale")
        volume.sum_scale = sc
        volume.sum_scale_version = volume.buf._version
        return volume

    def _fresh_packed(self, volume, need=False):
        """The derived copies K4h / K4hp read, brought up to date with volume.buf: the packed copy
        rebuilt when torch's version counter moved since it was made (need: made when there is
        none), and with the "exact_sum_volume" option on the volume's sum scale computed once per
        voxel state and set on the context."""
        if volume.packed is None:
            if need:
                self.volume_pack(volume)
        elif volume.buf._version != volume.packed_version:
            self.volume_pack(volume)   # the voxels changed since the copy: K4h reads only it
        if self._exact_sum_volume:   # the exact sums' scale: computed once per voxel state
            if volume.sum_scale is None or volume.buf._version != volume.sum_scale_version:
                self.volume_sum_scale(volume)
            _lib.check(self.lib.uam_set_volume_sum_scale(self._ctx, _ptr(volume.sum_scale)),
                       "uam_set_volume_sum_scale")

    def eval_generated3d(self, pairs6, utab, volume, outputs=None):
        """pairs6 [Q, 6] = (x0, y0, z0, xf, yf, zf) (km, km, m); path p = q*D + d."""
        torch = _torch()
        pr = self.tensor(pairs6, torch.float64).reshape(-1, 6)
        ut = self.tensor(utab, torch.float64)
        D = ut.shape[0]
        if ut.shape[1] != self.params.N:
            raise ValueError(f"arc table has N={ut.shape[1]}, params N={self.params.N}")
        Q = pr.shape[0]
        if outputs is not None:
            o, s = outputs
            _check_outputs(o, Q * D, Q, self.params.N + 2)
        else:
            o, s = self._outputs(Q * D, self.params.N + 2, _lib.MODE_VOLUME, False, False,
                                 n_pairs=Q)
        self._fresh_packed(volume)
        _lib.check(self.lib.uam_eval_generated3d(
            self._ctx, ctypes.byref(volume.geo.as_struct()), _ptr(volume.buf),
            _ptr(volume.packed), _ptr(pr), Q, _ptr(ut), D, ctypes.byref(s), self.stream),
            "uam_eval_generated3d")
        return o

    # -- volume: explicit 3-D waypoints and altitude-profile candidates -------------------
    def _profile_inputs(self, pairs6, utab, ztab):
        """(pairs6 [Q, 6], utab [D, N, 2], ztab [A, N+2, 3] or None, Q, D, A) on the device,
        shapes checked against params.N (profiles.py builds the tables)."""
        torch = _torch()
        N = self.params.N
        pr = self.tensor(pairs6, torch.float64).reshape(-1, 6)
        ut = self.tensor(utab, torch.float64)
        if ut.dim() != 3 or ut.shape[1] != N or ut.shape[2] != 2:
            raise ValueError(f"arc table has shape {tuple(ut.shape)}, params N={N} needs "
                             f"[D, {N}, 2]")
        zt, A = None, 1
        if ztab is not None:
            zt = self.tensor(ztab, torch.float64)
            if zt.dim() != 3 or zt.shape[1] != N + 2 or zt.shape[2] != 3:
                raise ValueError(f"profile table has shape {tuple(zt.shape)}, params N={N} "
                                 f"needs [A, {N + 2}, 3]")
            A = zt.shape[0]
        return pr, ut, zt, pr.shape[0], ut.shape[0], A

    def gen_paths3d(self, pairs6, utab, ztab=None):
        """The waypoints [Q*D*A, N+2, 3] (x km, y km, z m) of pairs6 [Q, 6] x utab [D, N, 2] x
        the altitude-profile table ztab [A, N+2, 3] (uam_gen_paths3d; None: A = 1, the straight
        climb of eval_generated3d); path p = (q*D + d)*A + a."""
        torch = _torch()
        pr, ut, zt, Q, D, A = self._profile_inputs(pairs6, utab, ztab)
        wp3 = self.empty((Q * D * A, self.params.N + 2, 3), torch.float64)
        _lib.check(self.lib.uam_gen_paths3d(self._ctx, _ptr(pr), Q, _ptr(ut), D, _ptr(zt), A,
                                            _ptr(wp3), self.stream), "uam_gen_paths3d")
        return wp3

    def _climb_sum(self, o, P):
        """The climb_sum output of a _v call: the caller's (outputs["climb_sum"]) or a new one."""
        torch = _torch()
        if "climb_sum" not in o:
            o["climb_sum"] = self.empty((P,), torch.float64)
        elif o["climb_sum"].numel() < P:
            raise ValueError(f"outputs['climb_sum'] holds {o['climb_sum'].numel()} entries, "
                             f"this batch needs {P}")
        return o["climb_sum"]

    def eval_waypoints3d(self, wp3, volume, want_cells=False, vertical=None):
        """wp3 [P, N+2, 3] float64 (x km, y km, z m) against the volume's voxels
        (uam_eval_waypoints3d: the oracle's eval_paths3d bit for bit).  Reads volume.buf only.
        vertical (a Vertical): the 3-D length, turn and climb rows (uam_eval_waypoints3d_v);
        the result then holds climb_sum too."""
        torch = _torch()
        W = self.params.N + 2
        w = self.tensor(wp3, torch.float64)
        if w.dim() < 2 or w.shape[-1] != 3 or w.shape[-2] != W:
            raise ValueError(f"waypoints have shape {tuple(w.shape)}, params N={W - 2} needs "
                             f"[P, {W}, 3]")
        w = w.reshape(-1, W, 3)
        P = w.shape[0]
        o, s = self._outputs(P, W, _lib.MODE_VOLUME, want_cells, False)
        if vertical is not None:
            climb = self._climb_sum(o, P)
            _lib.check(self.lib.uam_eval_waypoints3d_v(
                self._ctx, ctypes.byref(volume.geo.as_struct()), _ptr(volume.buf), _ptr(w), P,
                ctypes.byref(vertical.as_struct()), ctypes.byref(s), _ptr(climb), self.stream),
                "uam_eval_waypoints3d_v")
            return o
        _lib.check(self.lib.uam_eval_waypoints3d(
            self._ctx, ctypes.byref(volume.geo.as_struct()), _ptr(volume.buf), _ptr(w), P,
            ctypes.byref(s), self.stream), "uam_eval_waypoints3d")
        return o

    def eval_generated3d_profiles(self, pairs6, utab, ztab, volume, want_cells=False,
                                  outputs=None, vertical=None, packed=False):
        """eval_waypoints3d of gen_paths3d's waypoints in one kernel, with the selection over
        each pair's D*A candidates (uam_eval_generated3d_profiles): path p = (q*D + d)*A + a,
        best_fval_idx / best_length_idx [Q] hold the candidate c = d*A + a.  Reads volume.buf
        only.  vertical (a Vertical): the 3-D length, turn and climb rows
        (uam_eval_generated3d_profiles_v); the lengths and both selections then depend on the
        profile, and the result holds climb_sum too.
        packed=True: the sorted form on volume.packed (uam_eval_generated3d_profiles_h, "K4hp":
        grouped sums in UAM_OPT_GROUP order, the geometry in the similarity form, exact sums
        with the "exact_sum_volume" option) at every batch size or a ValueError with its reason.
        The copy is packed first when there is none and repacked when the voxels changed, by
        eval_generated3d's rules.  It has no vertical form: eval_generated3d_profiles_hv is the
        sorted call with the vertical terms, a definition of its own."""
        if packed and vertical is not None:
            raise ValueError("packed=True has no vertical form: the similarity-form geometry "
                             "is not scale-free under the vertical terms; "
                             "eval_generated3d_profiles_hv keeps the sorted sums and takes the "
                             "geometry per path")
        pr, ut, zt, Q, D, A = self._profile_inputs(pairs6, utab, ztab)
        W = self.params.N + 2
        if outputs is not None:
            o, s = outputs
            _check_outputs(o, Q * D * A, Q, W)
        else:
            o, s = self._outputs(Q * D * A, W, _lib.MODE_VOLUME, want_cells, False, n_pairs=Q)
        if packed:
            self._fresh_packed(volume, need=True)
            _lib.check(self.lib.uam_eval_generated3d_profiles_h(
                self._ctx, ctypes.byref(volume.geo.as_struct()), _ptr(volume.buf),
                _ptr(volume.packed), _ptr(pr), Q, _ptr(ut), D, _ptr(zt), A, ctypes.byref(s),
                self.stream), "uam_eval_generated3d_profiles_h")
            return o
        if vertical is not None:
            climb = self._climb_sum(o, Q * D * A)
            _lib.check(self.lib.uam_eval_generated3d_profiles_v(
                self._ctx, ctypes.byref(volume.geo.as_struct()), _ptr(volume.buf), _ptr(pr), Q,
                _ptr(ut), D, _ptr(zt), A, ctypes.byref(vertical.as_struct()), ctypes.byref(s),
                _ptr(climb), self.stream), "uam_eval_generated3d_profiles_v")
            return o
        _lib.check(self.lib.uam_eval_generated3d_profiles(
            self._ctx, ctypes.byref(volume.geo.as_struct()), _ptr(volume.buf), _ptr(pr), Q,
            _ptr(ut), D, _ptr(zt), A, ctypes.byref(s), self.stream),
            "uam_eval_generated3d_profiles")
        return o

    def eval_generated3d_profiles_hv(self, pairs6, utab, ztab, volume, vertical, outputs=None):
        """The altitude-profile candidates on volume.packed with the vertical terms
        (uam_eval_generated3d_profiles_hv, "K4hpv+pack"; "K4hpxv+pack" with the
        "exact_sum_volume" option): eval_generated3d_profiles(packed=True)'s sort, gathers and
        grouped (or exact) sums, with length_q, length, kin_sum and climb_sum formed per path
        under vertical (a Vertical) as eval_generated3d_profiles(vertical=) forms them, and both
        selections over each pair's D*A candidates on the new cost and length.  Sorted at every
        batch size or a ValueError with its reason; maxratio_smooth is taken and the "k2g_sim"
        option is not read.  ztab=None: A = 1, the straight climb.  The copy is packed first when
        there is none and repacked when the voxels changed, by eval_generated3d's rules.  Returns
        the usual dict plus climb_sum (outputs["climb_sum"] when the caller provides one)."""
        if vertical is None:
            raise ValueError("eval_generated3d_profiles_hv needs a Vertical; without one the "
                             "call is eval_generated3d_profiles(..., packed=True)")
        pr, ut, zt, Q, D, A = self._profile_inputs(pairs6, utab, ztab)
        W = self.params.N + 2
        if outputs is not None:
            o, s = outputs
            _check_outputs(o, Q * D * A, Q, W)
        else:
            o, s = self._outputs(Q * D * A, W, _lib.MODE_VOLUME, False, False, n_pairs=Q)
        climb = self._climb_sum(o, Q * D * A)
        self._fresh_packed(volume, need=True)
        _lib.check(self.lib.uam_eval_generated3d_profiles_hv(
            self._ctx, ctypes.byref(volume.geo.as_struct()), _ptr(volume.buf),
            _ptr(volume.packed), _ptr(pr), Q, _ptr(ut), D, _ptr(zt), A,
            ctypes.byref(vertical.as_struct()), ctypes.byref(s), _ptr(climb), self.stream),
            "uam_eval_generated3d_profiles_hv")
        return o

    def gen_paths(self, pairs, utab):
        torch = _torch()
        pr = self.tensor(pairs, torch.float64).reshape(-1, 4)
        ut = self.tensor(utab, torch.float64)
        D, N = ut.shape[0], ut.shape[1]
        if N != self.params.N:
            raise ValueError(f"arc table has N={N}, params N={self.params.N}")
        wp = self.empty((pr.shape[0] * D, N + 2, 2), torch.float64)
        _lib.check(self.lib.uam_gen_paths(self._ctx, _ptr(pr), pr.shape[0], _ptr(ut), D,
                                          _ptr(wp), self.stream), "uam_gen_paths")
        return wp

    def argmin(self, values, G, take_sqrt, out=None):
        torch = _torch()
        v = self.tensor(values, torch.float64).reshape(-1)
        groups = v.shape[0] // G
        best = out if out is not None else self.empty((groups,), torch.int32)
        _lib.check(self.lib.uam_argmin(self._ctx, _ptr(v), groups, int(G), int(bool(take_sqrt)),
                                       _ptr(best), self.stream), "uam_argmin")
        return best

    def path_length(self, pts, n_segments, smooth):
        torch = _torch()
        p = self.tensor(pts, torch.float64)
        if p.dim() == 2:
            p = p.unsqueeze(0)
        P, n_points = p.shape[0], p.shape[1]
        out = self.empty((P,), torch.float64)
        _lib.check(self.lib.uam_path_length(self._ctx, _ptr(p), P, n_points, int(n_segments),
                                            int(bool(smooth)), _ptr(out), self.stream),
                   "uam_path_length")
        return out

    def refine(self, wp, params=None, inplace=False):
        """Batched ALM refinement of waypoint paths (the reference's
        OpEn solve, solver.py:82-93).  wp: [P, N+2, 2] float64; endpoints stay fixed.
        Returns {"wp", "cost", "infeas", "iters"} (device tensors).  Definition and
        defaults: oracle/uam_oracle.c orc_refine, REFINE_DEFAULTS."""
        torch = _torch()
        W = self.params.N + 2
        z = self.tensor(wp, torch.float64)
        if z.dim() == 2:
            z = z.unsqueeze(0)
        if tuple(z.shape[1:]) != (W, 2):
            raise ValueError(f"wp must be [P, {W}, 2], got {tuple(z.shape)}")
        if not inplace:
            z = z.clone(memory_format=torch.contiguous_format)
        elif not z.is_contiguous():
            raise ValueError("inplace refinement needs a contiguous tensor")
        P = z.shape[0]
        rp = dict(REFINE_DEFAULTS)
        rp.update(params or {})
        unknown = set(rp) - set(REFINE_DEFAULTS)
        if unknown:
            raise ValueError(f"unknown refine settings {sorted(unknown)}")
        st = _lib.RefineParams(int(rp["n_outer"]), int(rp["n_inner"]), int(rp["max_backtrack"]),
                               int(rp["memory"]), float(rp["c0"]), float(rp["rho"]),
                               float(rp["c_max"]), float(rp["alpha0"]), float(rp["armijo"]),
                               float(rp["theta"]), float(rp["max_step"]),
                               float(rp["inner_tol"]), float(rp["delta"]),
                               int(rp["n_restart"]), float(rp["restart_margin"]))
        nbytes = self.lib.uam_refine_workspace_bytes(self._ctx, P, ctypes.byref(st))
        if nbytes < 0:
            raise _lib.UamError("uam_refine_workspace_bytes: set geometry and params first")
        ws = self.empty((max(nbytes, 8) // 8,), torch.float64)
        out = {"wp": z, "cost": self.empty((P,), torch.float64),
               "infeas": self.empty((P,), torch.float64), "iters": self.empty((P,), torch.int32)}
        _lib.check(self.lib.uam_refine(self._ctx, _ptr(z), P, ctypes.byref(st), _ptr(ws), nbytes,
                                       _ptr(out["cost"]), _ptr(out["infeas"]), _ptr(out["iters"]),
                                       self.stream), "uam_refine")
        return out

    # -- route seeds (K9) -------------------------------------------------------------------
    def route_field(self, raster, goals, lam=1.0, block_flags=_lib.FLAG_NFZ, inflate=0,
                    max_rounds=0, joint=False):
        """The cost-to-go fields of goals [G, 2] on raster (uam_route_field): a per-goal setup
        product like the packed copy -- the call waits for the stream between its rounds.  Cell
        cost 1 + lam * phi, cells with a block_flags bit (or a non-finite or non-positive cost)
        blocked, inflate cells of clearance around them; max_rounds 0 = nx*ny.  Returns a
        RouteField; raises UamError when a field has not converged within max_rounds.
        joint=True (uam_route_field_joint, K9j): one field to the nearest of the goals in one
        relaxation -- dist and next [1, ny, nx] and owner [ny, nx], the goal each cell's route
        ends at -- for the time and memory of about one goal."""
        torch = _torch()
        geo = raster.geo
        g = self.tensor(goals, torch.float64).reshape(-1, 2)
        G = g.shape[0]
        rp = _route_params(lam, block_flags, inflate, max_rounds)
        gs = geo.as_struct()
        if joint:
            nbytes = self.lib.uam_route_joint_workspace_bytes(ctypes.byref(gs), ctypes.byref(rp),
                                                              G)
            ws = None if nbytes < 0 else self.empty(((nbytes + 255) // 256, 256), torch.uint8)
            dist = self.empty((1, geo.ny, geo.nx), torch.float64)
            nxt = self.empty((1, geo.ny, geo.nx), torch.uint8)
            owner = self.empty((geo.ny, geo.nx), torch.int32)
            rounds = ctypes.c_int32()
            _lib.check(self.lib.uam_route_field_joint(
                self._ctx, ctypes.byref(gs), _ptr(raster.rec), ctypes.byref(rp), _ptr(g), G,
                _ptr(dist), _ptr(nxt), _ptr(owner), _ptr(ws), max(nbytes, 0),
                ctypes.byref(rounds), self.stream), "uam_route_field_joint")
            return RouteField(geo, g, dist, nxt, rounds.value,
                              int(self.lib.uam_route_visits(self._ctx)), raster.rec, float(lam),
                              int(block_flags), int(inflate), None, owner, True)
        nbytes = self.lib.uam_route_workspace_bytes(ctypes.byref(gs), ctypes.byref(rp))
        ws = None if nbytes < 0 else self.empty(((nbytes + 255) // 256, 256), torch.uint8)
        dist = self.empty((G, geo.ny, geo.nx), torch.float64)
        nxt = self.empty((G, geo.ny, geo.nx), torch.uint8)
        rounds = ctypes.c_int32()
        _lib.check(self.lib.uam_route_field(
            self._ctx, ctypes.byref(gs), _ptr(raster.rec), ctypes.byref(rp), _ptr(g), G,
            _ptr(dist), _ptr(nxt), _ptr(ws), max(nbytes, 0), ctypes.byref(rounds), self.stream),
            "uam_route_field")
        return RouteField(geo, g, dist, nxt, rounds.value,
                          int(self.lib.uam_route_visits(self._ctx)), raster.rec, float(lam),
                          int(block_flags), int(inflate))

    def route_free_bits(self, field):
        """The free cells of a RouteField's raster and parameters as one bit per cell
        (uam_route_free_bits, K9b): [ny, (nx + 31) // 32] int32 words, bit ix & 31 of word
        ix // 32 set = free.  Computed once and kept on the field."""
        if field.free_bits is None:
            torch = _torch()
            geo = field.geo
            bits = self.empty((geo.ny, (geo.nx + 31) // 32), torch.int32)
            rp = field.params()
            _lib.check(self.lib.uam_route_free_bits(
                self._ctx, ctypes.byref(geo.as_struct()), _ptr(field.rec), ctypes.byref(rp),
                _ptr(bits), self.stream), "uam_route_free_bits")
            field.free_bits = bits
        return field.free_bits

    def route_paths(self, field, starts, goal_idx=None, smooth=0):
        """Seed paths through a RouteField (uam_route_paths): starts [Q, 2], goal_idx [Q] into
        field.goals.  Returns {"wp" [Q, N+2, 2], "status" [Q], "steps" [Q]} (device tensors);
        status 0 ok, 1 start off the raster or blocked, 2 goal unreachable, 3 walk too long,
        4 bad goal -- a nonzero status leaves the straight line in wp.  wp is what
        eval_waypoints and refine take.
        smooth >= 1 (uam_route_paths_smooth, K9s): any-angle shortcuts over at most smooth
        chain cells (1..1024) wherever the cells between lie in straight sight; adds "vertices"
        [Q] (the polyline's vertices, end points included; 0 for a nonzero status).  smooth = 1
        keeps every cell: the bits of smooth = 0.
        A joint field (uam_route_paths_joint) takes no goal_idx: every start goes to the goal
        that owns its cell, returned as "goal" [Q] (-1 for a nonzero status, which is 1, 2 or 3
        -- no owner -- and leaves the start point in every waypoint); "vertices" for every
        smooth."""
        torch = _torch()
        s = self.tensor(starts, torch.float64).reshape(-1, 2)
        if field.joint:
            if goal_idx is not None:
                raise ValueError("a joint RouteField takes no goal_idx")
            Q = s.shape[0]
            N = self.params.N
            out = {"wp": self.empty((Q, N + 2, 2), torch.float64)}
            for k in ("status", "steps", "vertices", "goal"):
                out[k] = self.empty((Q,), torch.int32)
            bits = self.route_free_bits(field) if smooth else None
            rp = field.params()
            _lib.check(self.lib.uam_route_paths_joint(
                self._ctx, ctypes.byref(field.geo.as_struct()), _ptr(field.rec), ctypes.byref(rp),
                _ptr(bits), _ptr(field.next), _ptr(field.owner), _ptr(field.goals),
                field.goals.shape[0], _ptr(s), Q, int(smooth), _ptr(out["wp"]),
                _ptr(out["status"]), _ptr(out["steps"]), _ptr(out["vertices"]), _ptr(out["goal"]),
                self.stream), "uam_route_paths_joint")
            return out
        if goal_idx is None:
            raise ValueError("a per-goal RouteField needs goal_idx")
        gi = self.tensor(goal_idx, torch.int32).reshape(-1)
        Q = s.shape[0]
        if gi.shape[0] != Q:
            raise ValueError(f"{Q} starts but {gi.shape[0]} goal indices")
        N = self.params.N
        out = {"wp": self.empty((Q, N + 2, 2), torch.float64),
               "status": self.empty((Q,), torch.int32), "steps": self.empty((Q,), torch.int32)}
        if smooth:
            out["vertices"] = self.empty((Q,), torch.int32)
            bits = self.route_free_bits(field)
            _lib.check(self.lib.uam_route_paths_smooth(
                self._ctx, ctypes.byref(field.geo.as_struct()), _ptr(bits), _ptr(field.next),
                _ptr(field.goals), field.goals.shape[0], _ptr(s), _ptr(gi), Q, int(smooth),
                _ptr(out["wp"]), _ptr(out["status"]), _ptr(out["steps"]),
                _ptr(out["vertices"]), self.stream), "uam_route_paths_smooth")
            return out
        rp = field.params()
        _lib.check(self.lib.uam_route_paths(
            self._ctx, ctypes.byref(field.geo.as_struct()), _ptr(field.rec), ctypes.byref(rp),
            _ptr(field.next), _ptr(field.goals), field.goals.shape[0], _ptr(s), _ptr(gi), Q,
            _ptr(out["wp"]), _ptr(out["status"]), _ptr(out["steps"]), self.stream),
            "uam_route_paths")
        return out

    @staticmethod
    def route_field_host(geo, rec, goals, lam=1.0, block_flags=_lib.FLAG_NFZ, inflate=0,
                         joint=False):
        """route_field on the host (uam_route_field_host; needs no GPU): the definition applied
        by the inline functions the kernels run, the minimum by a heap Dijkstra.  rec: numpy
        [ny, nx, 4] 32-bit words.  Returns a RouteField of numpy arrays (rounds 0).  joint=True:
        uam_route_field_joint_host, the owner by following the chains."""
        r = _host_rec(rec, geo)
        g = np.ascontiguousarray(goals, dtype=np.float64).reshape(-1, 2)
        G = g.shape[0]
        if joint:
            dist = np.empty((1, geo.ny, geo.nx), dtype=np.float64)
            nxt = np.empty((1, geo.ny, geo.nx), dtype=np.uint8)
            owner = np.empty((geo.ny, geo.nx), dtype=np.int32)
            rp = _route_params(lam, block_flags, inflate, 0)
            _lib.check(_lib.load().uam_route_field_joint_host(
                ctypes.byref(geo.as_struct()), r.ctypes.data, ctypes.byref(rp), g.ctypes.data, G,
                dist.ctypes.data, nxt.ctypes.data, owner.ctypes.data),
                "uam_route_field_joint_host")
            return RouteField(geo, g, dist, nxt, 0, 0, r, float(lam), int(block_flags),
                              int(inflate), None, owner, True)
        dist = np.empty((G, geo.ny, geo.nx), dtype=np.float64)
        nxt = np.empty((G, geo.ny, geo.nx), dtype=np.uint8)
        rp = _route_params(lam, block_flags, inflate, 0)
        _lib.check(_lib.load().uam_route_field_host(
            ctypes.byref(geo.as_struct()), r.ctypes.data, ctypes.byref(rp), g.ctypes.data, G,
            dist.ctypes.data, nxt.ctypes.data), "uam_route_field_host")
        return RouteField(geo, g, dist, nxt, 0, 0, r, float(lam), int(block_flags), int(inflate))

    @staticmethod
    def route_free_bits_host(field):
        """route_free_bits on the host (uam_route_free_bits_host) for a RouteField of numpy
        arrays: [ny, (nx + 31) // 32] uint32, kept on the field."""
        if field.free_bits is None:
            geo = field.geo
            bits = np.empty((geo.ny, (geo.nx + 31) // 32), dtype=np.uint32)
            rp = field.params()
            _lib.check(_lib.load().uam_route_free_bits_host(
                ctypes.byref(geo.as_struct()), _host_rec(field.rec, geo).ctypes.data,
                ctypes.byref(rp), bits.ctypes.data), "uam_route_free_bits_host")
            field.free_bits = bits
        return field.free_bits

    @staticmethod
    def route_paths_host(field, starts, goal_idx=None, N=None, smooth=0):
        """route_paths on the host (uam_route_paths_host; needs no GPU) for a RouteField of
        numpy arrays; N interior waypoints.  Returns {"wp", "status", "steps"} numpy arrays,
        and "vertices" for smooth >= 1 (uam_route_paths_smooth_host).  A joint field
        (uam_route_paths_joint_host) takes goal_idx = None and adds "vertices" and "goal"."""
        if N is None:
            raise ValueError("route_paths_host needs N")
        s = np.ascontiguousarray(starts, dtype=np.float64).reshape(-1, 2)
        if field.joint:
            if goal_idx is not None:
                raise ValueError("a joint RouteField takes no goal_idx")
            Q, N = s.shape[0], int(N)
            out = {"wp": np.empty((Q, max(N, 0) + 2, 2), dtype=np.float64)}
            for k in ("status", "steps", "vertices", "goal"):
                out[k] = np.empty((Q,), dtype=np.int32)
            rp = field.params()
            nxt = np.ascontiguousarray(field.next, dtype=np.uint8)
            own = np.ascontiguousarray(field.owner, dtype=np.int32)
            goals = np.ascontiguousarray(field.goals, dtype=np.float64)
            bits = Engine.route_free_bits_host(field) if smooth else None
            _lib.check(_lib.load().uam_route_paths_joint_host(
                ctypes.byref(field.geo.as_struct()), _host_rec(field.rec, field.geo).ctypes.data,
                ctypes.byref(rp), bits.ctypes.data if smooth else None, nxt.ctypes.data,
                own.ctypes.data, goals.ctypes.data, goals.shape[0], s.ctypes.data, Q, N,
                int(smooth), out["wp"].ctypes.data, out["status"].ctypes.data,
                out["steps"].ctypes.data, out["vertices"].ctypes.data, out["goal"].ctypes.data),
                "uam_route_paths_joint_host")
            return out
        if goal_idx is None:
            raise ValueError("a per-goal RouteField needs goal_idx")
        gi = np.ascontiguousarray(goal_idx, dtype=np.int32).reshape(-1)
        Q = s.shape[0]
        if gi.shape[0] != Q:
            raise ValueError(f"{Q} starts but {gi.shape[0]} goal indices")
        N = int(N)
        out = {"wp": np.empty((Q, max(N, 0) + 2, 2), dtype=np.float64),
               "status": np.empty((Q,), dtype=np.int32), "steps": np.empty((Q,), dtype=np.int32)}
        rp = field.params()
        nxt = np.ascontiguousarray(field.next, dtype=np.uint8)
        goals = np.ascontiguousarray(field.goals, dtype=np.float64)
        if smooth:
            out["vertices"] = np.empty((Q,), dtype=np.int32)
            bits = Engine.route_free_bits_host(field)
            _lib.check(_lib.load().uam_route_paths_smooth_host(
                ctypes.byref(field.geo.as_struct()), bits.ctypes.data, nxt.ctypes.data,
                goals.ctypes.data, goals.shape[0], s.ctypes.data, gi.ctypes.data, Q, N,
                int(smooth), out["wp"].ctypes.data, out["status"].ctypes.data,
                out["steps"].ctypes.data, out["vertices"].ctypes.data),
                "uam_route_paths_smooth_host")
            return out
        _lib.check(_lib.load().uam_route_paths_host(
            ctypes.byref(field.geo.as_struct()), _host_rec(field.rec, field.geo).ctypes.data,
            ctypes.byref(rp), nxt.ctypes.data, goals.ctypes.data, goals.shape[0], s.ctypes.data,
            gi.ctypes.data, Q, N, out["wp"].ctypes.data, out["status"].ctypes.data,
            out["steps"].ctypes.data), "uam_route_paths_host")
        return out

    # -- route seeds in the volume (K9v) ------------------------------------------------------
    def route_field3d(self, volume, goals, lam=1.0, block_flags=_lib.FLAG_NFZ, inflate=0,
                      agl=0.0, z_scale=1e-3, max_rounds=0, joint=False):
        """The cost-to-go fields of goals [G, 3] (x km, y km, z m) over volume's voxels
        (uam_route3d_field): a per-goal setup product like route_field's.  Voxel cost 1 + lam *
        risk; voxels of a column with a block_flags bit, with a non-finite or non-positive cost
        or whose layer centre lies less than agl metres above the terrain are blocked, inflate
        voxels of x/y clearance around them; z_scale is Vertical's unit (km per metre of
        altitude), so the field's metric is the one eval_waypoints3d(..., vertical=) charges;
        max_rounds 0 = nx*ny*nz.  Returns a RouteField3D; raises UamError when a field has not
        converged within max_rounds.
        joint=True (uam_route3d_field_joint, K9vj): one field to the nearest of the goals in one
        relaxation -- dist and next [1, ny, nx, nz] and owner [ny, nx, nz], the goal each voxel's
        route ends at -- for the time and memory of about one goal."""
        torch = _torch()
        geo = volume.geo
        g = self.tensor(goals, torch.float64).reshape(-1, 3)
        G = g.shape[0]
        rp = _route3d_params(lam, block_flags, inflate, agl, z_scale, max_rounds)
        gs = geo.as_struct()
        if joint:
            nbytes = self.lib.uam_route3d_joint_workspace_bytes(ctypes.byref(gs),
                                                                ctypes.byref(rp), G)
            ws = None if nbytes < 0 else self.empty(((nbytes + 255) // 256, 256), torch.uint8)
            dist = self.empty((1, geo.ny, geo.nx, geo.nz), torch.float64)
            nxt = self.empty((1, geo.ny, geo.nx, geo.nz), torch.uint8)
            owner = self.empty((geo.ny, geo.nx, geo.nz), torch.int32)
            rounds = ctypes.c_int32()
            _lib.check(self.lib.uam_route3d_field_joint(
                self._ctx, ctypes.byref(gs), _ptr(volume.buf), ctypes.byref(rp), _ptr(g), G,
                _ptr(dist), _ptr(nxt), _ptr(owner), _ptr(ws), max(nbytes, 0),
                ctypes.byref(rounds), self.stream), "uam_route3d_field_joint")
            return RouteField3D(geo, g, dist, nxt, rounds.value,
                                int(self.lib.uam_route3d_visits(self._ctx)), volume.buf,
                                float(lam), int(block_flags), int(inflate), float(agl),
                                float(z_scale), None, owner, True)
        nbytes = self.lib.uam_route3d_workspace_bytes(ctypes.byref(gs), ctypes.byref(rp))
        ws = None if nbytes < 0 else self.empty(((nbytes + 255) // 256, 256), torch.uint8)
        dist = self.empty((G, geo.ny, geo.nx, geo.nz), torch.float64)
        nxt = self.empty((G, geo.ny, geo.nx, geo.nz), torch.uint8)
        rounds = ctypes.c_int32()
        _lib.check(self.lib.uam_route3d_field(
            self._ctx, ctypes.byref(gs), _ptr(volume.buf), ctypes.byref(rp), _ptr(g), G,
            _ptr(dist), _ptr(nxt), _ptr(ws), max(nbytes, 0), ctypes.byref(rounds), self.stream),
            "uam_route3d_field")
        return RouteField3D(geo, g, dist, nxt, rounds.value,
                            int(self.lib.uam_route3d_visits(self._ctx)), volume.buf, float(lam),
                            int(block_flags), int(inflate), float(agl), float(z_scale))

    def route_free_bits3d(self, field):
        """The free voxels of a RouteField3D's volume and parameters as one bit per voxel
        (uam_route3d_free_bits, K9vb): [(nx*ny*nz + 31) // 32] int32 words, bit v & 31 of word
        v >> 5 set = free, v = (iy*nx + ix)*nz + iz.  Computed once and kept on the field."""
        if field.free_bits is None:
            torch = _torch()
            geo = field.geo
            bits = self.empty(((geo.nx * geo.ny * geo.nz + 31) // 32,), torch.int32)
            rp = field.params()
            _lib.check(self.lib.uam_route3d_free_bits(
                self._ctx, ctypes.byref(geo.as_struct()), _ptr(field.vol), ctypes.byref(rp),
                _ptr(bits), self.stream), "uam_route3d_free_bits")
            field.free_bits = bits
        return field.free_bits

    def route_paths3d(self, field, starts, goal_idx=None, smooth=0):
        """Seed paths through a RouteField3D (uam_route3d_paths): starts [Q, 3], goal_idx [Q]
        into field.goals.  Returns {"wp3" [Q, N+2, 3], "status" [Q], "steps" [Q]} (device
        tensors); status as route_paths' -- a nonzero status leaves the straight line in wp3.
        wp3 is what eval_waypoints3d(..., vertical=Vertical(field.z_scale, ...)) takes.
        smooth >= 1 (uam_route3d_paths_smooth, K9vs): any-angle shortcuts over at most smooth
        chain voxels (1..1024) wherever the voxels between lie in straight sight, in plan view
        and in altitude; adds "vertices" [Q] (the polyline's vertices, end points included; 0
        for a nonzero status).  smooth = 1 keeps every voxel: the bits of smooth = 0.  The test
        is geometric and does not weigh risk: a long span may cut a climb to cheaper layers.
        A joint field (uam_route3d_paths_joint) takes no goal_idx: every start goes to the goal
        that owns its voxel, returned as "goal" [Q] (-1 for a nonzero status, which is 1, 2 or 3
        -- no owner -- and leaves the start point in every waypoint); "vertices" for every
        smooth."""
        torch = _torch()
        s = self.tensor(starts, torch.float64).reshape(-1, 3)
        if field.joint:
            if goal_idx is not None:
                raise ValueError("a joint RouteField3D takes no goal_idx")
            Q = s.shape[0]
            N = self.params.N
            out = {"wp3": self.empty((Q, N + 2, 3), torch.float64)}
            for k in ("status", "steps", "vertices", "goal"):
                out[k] = self.empty((Q,), torch.int32)
            bits = self.route_free_bits3d(field) if smooth else None
            rp = field.params()
            _lib.check(self.lib.uam_route3d_paths_joint(
                self._ctx, ctypes.byref(field.geo.as_struct()), _ptr(field.vol), ctypes.byref(rp),
                _ptr(bits), _ptr(field.next), _ptr(field.owner), _ptr(field.goals),
                field.goals.shape[0], _ptr(s), Q, int(smooth), _ptr(out["wp3"]),
                _ptr(out["status"]), _ptr(out["steps"]), _ptr(out["vertices"]), _ptr(out["goal"]),
                self.stream), "uam_route3d_paths_joint")
            return out
        if goal_idx is None:
            raise ValueError("a per-goal RouteField3D needs goal_idx")
        gi = self.tensor(goal_idx, torch.int32).reshape(-1)
        Q = s.shape[0]
        if gi.shape[0] != Q:
            raise ValueError(f"{Q} starts but {gi.shape[0]} goal indices")
        N = self.params.N
        out = {"wp3": self.empty((Q, N + 2, 3), torch.float64),
               "status": self.empty((Q,), torch.int32), "steps": self.empty((Q,), torch.int32)}
        rp = field.params()
        if smooth:
            out["vertices"] = self.empty((Q,), torch.int32)
            bits = self.route_free_bits3d(field)
            _lib.check(self.lib.uam_route3d_paths_smooth(
                self._ctx, ctypes.byref(field.geo.as_struct()), ctypes.byref(rp), _ptr(bits),
                _ptr(field.next), _ptr(field.goals), field.goals.shape[0], _ptr(s), _ptr(gi), Q,
                int(smooth), _ptr(out["wp3"]), _ptr(out["status"]), _ptr(out["steps"]),
                _ptr(out["vertices"]), self.stream), "uam_route3d_paths_smooth")
            return out
        _lib.check(self.lib.uam_route3d_paths(
            self._ctx, ctypes.byref(field.geo.as_struct()), _ptr(field.vol), ctypes.byref(rp),
            _ptr(field.next), _ptr(field.goals), field.goals.shape[0], _ptr(s), _ptr(gi), Q,
            _ptr(out["wp3"]), _ptr(out["status"]), _ptr(out["steps"]), self.stream),
            "uam_route3d_paths")
        return out

    @staticmethod
    def route_field3d_host(geo, vol, goals, lam=1.0, block_flags=_lib.FLAG_NFZ, inflate=0,
                           agl=0.0, z_scale=1e-3, joint=False):
        """route_field3d on the host (uam_route3d_field_host; needs no GPU).  vol: the volume
        buffer as numpy 32-bit words in the header's layout (8-B voxels {risk, psi}
        [ny][nx][nz], then at the 256-B aligned offset the 8-B columns {terrain, flags}
        [ny][nx]).  Returns a RouteField3D of numpy arrays (rounds 0).  joint=True:
        uam_route3d_field_joint_host, the owner by following the chains."""
        v = _host_vol(vol, geo)
        g = np.ascontiguousarray(goals, dtype=np.float64).reshape(-1, 3)
        G = g.shape[0]
        if joint:
            dist = np.empty((1, geo.ny, geo.nx, geo.nz), dtype=np.float64)
            nxt = np.empty((1, geo.ny, geo.nx, geo.nz), dtype=np.uint8)
            owner = np.empty((geo.ny, geo.nx, geo.nz), dtype=np.int32)
            rp = _route3d_params(lam, block_flags, inflate, agl, z_scale, 0)
            _lib.check(_lib.load().uam_route3d_field_joint_host(
                ctypes.byref(geo.as_struct()), v.ctypes.data, ctypes.byref(rp), g.ctypes.data, G,
                dist.ctypes.data, nxt.ctypes.data, owner.ctypes.data),
                "uam_route3d_field_joint_host")
            return RouteField3D(geo, g, dist, nxt, 0, 0, v, float(lam), int(block_flags),
                                int(inflate), float(agl), float(z_scale), None, owner, True)
        dist = np.empty((G, geo.ny, geo.nx, geo.nz), dtype=np.float64)
        nxt = np.empty((G, geo.ny, geo.nx, geo.nz), dtype=np.uint8)
        rp = _route3d_params(lam, block_flags, inflate, agl, z_scale, 0)
        _lib.check(_lib.load().uam_route3d_field_host(
            ctypes.byref(geo.as_struct()), v.ctypes.data, ctypes.byref(rp), g.ctypes.data, G,
            dist.ctypes.data, nxt.ctypes.data), "uam_route3d_field_host")
        return RouteField3D(geo, g, dist, nxt, 0, 0, v, float(lam), int(block_flags),
                            int(inflate), float(agl), float(z_scale))

    @staticmethod
    def route_free_bits3d_host(field):
        """route_free_bits3d on the host (uam_route3d_free_bits_host) for a RouteField3D of
        numpy arrays: [(nx*ny*nz + 31) // 32] uint32, kept on the field."""
        if field.free_bits is None:
            geo = field.geo
            bits = np.empty(((geo.nx * geo.ny * geo.nz + 31) // 32,), dtype=np.uint32)
            rp = field.params()
            _lib.check(_lib.load().uam_route3d_free_bits_host(
                ctypes.byref(geo.as_struct()), _host_vol(field.vol, geo).ctypes.data,
                ctypes.byref(rp), bits.ctypes.data), "uam_route3d_free_bits_host")
            field.free_bits = bits
        return field.free_bits

    @staticmethod
    def route_paths3d_host(field, starts, goal_idx, N, smooth=0):
        """route_paths3d on the host (uam_route3d_paths_host; needs no GPU) for a RouteField3D
        of numpy arrays; N interior waypoints.  Returns {"wp3", "status", "steps"}, and
        "vertices" for smooth >= 1 (uam_route3d_paths_smooth_host).  A joint field
        (uam_route3d_paths_joint_host) takes goal_idx = None and adds "vertices" and "goal"."""
        s = np.ascontiguousarray(starts, dtype=np.float64).reshape(-1, 3)
        if field.joint:
            if goal_idx is not None:
                raise ValueError("a joint RouteField3D takes no goal_idx")
            Q, N = s.shape[0], int(N)
            out = {"wp3": np.empty((Q, max(N, 0) + 2, 3), dtype=np.float64)}
            for k in ("status", "steps", "vertices", "goal"):
                out[k] = np.empty((Q,), dtype=np.int32)
            rp = field.params()
            nxt = np.ascontiguousarray(field.next, dtype=np.uint8)
            own = np.ascontiguousarray(field.owner, dtype=np.int32)
            goals = np.ascontiguousarray(field.goals, dtype=np.float64)
            bits = Engine.route_free_bits3d_host(field) if smooth else None
            _lib.check(_lib.load().uam_route3d_paths_joint_host(
                ctypes.byref(field.geo.as_struct()), _host_vol(field.vol, field.geo).ctypes.data,
                ctypes.byref(rp), bits.ctypes.data if smooth else None, nxt.ctypes.data,
                own.ctypes.data, goals.ctypes.data, goals.shape[0], s.ctypes.data, Q, N,
                int(smooth), out["wp3"].ctypes.data, out["status"].ctypes.data,
                out["steps"].ctypes.data, out["vertices"].ctypes.data, out["goal"].ctypes.data),
                "uam_route3d_paths_joint_host")
            return out
        if goal_idx is None:
            raise ValueError("a per-goal RouteField3D needs goal_idx")
        gi = np.ascontiguousarray(goal_idx, dtype=np.int32).reshape(-1)
        Q = s.shape[0]
        if gi.shape[0] != Q:
            raise ValueError(f"{Q} starts but {gi.shape[0]} goal indices")
        N = int(N)
        out = {"wp3": np.empty((Q, max(N, 0) + 2, 3), dtype=np.float64),
               "status": np.empty((Q,), dtype=np.int32), "steps": np.empty((Q,), dtype=np.int32)}
        rp = field.params()
        nxt = np.ascontiguousarray(field.next, dtype=np.uint8)
        goals = np.ascontiguousarray(field.goals, dtype=np.float64)
        if smooth:
            out["vertices"] = np.empty((Q,), dtype=np.int32)
            bits = Engine.route_free_bits3d_host(field)
            _lib.check(_lib.load().uam_route3d_paths_smooth_host(
                ctypes.byref(field.geo.as_struct()), ctypes.byref(rp), bits.ctypes.data,
                nxt.ctypes.data, goals.ctypes.data, goals.shape[0], s.ctypes.data,
                gi.ctypes.data, Q, N, int(smooth), out["wp3"].ctypes.data,
                out["status"].ctypes.data, out["steps"].ctypes.data,
                out["vertices"].ctypes.data), "uam_route3d_paths_smooth_host")
            return out
        _lib.check(_lib.load().uam_route3d_paths_host(
            ctypes.byref(field.geo.as_struct()), _host_vol(field.vol, field.geo).ctypes.data,
            ctypes.byref(rp), nxt.ctypes.data, goals.ctypes.data, goals.shape[0], s.ctypes.data,
            gi.ctypes.data, Q, N, out["wp3"].ctypes.data, out["status"].ctypes.data,
            out["steps"].ctypes.data), "uam_route3d_paths_host")
        return out

    # -- coordinate reference systems (K7) --------------------------
    def _tm(self, tm):
        if tm is None or isinstance(tm, int):
            out = _lib.TmParams()
            _lib.check(self.lib.uam_tm_jprcs(1 if tm is None else int(tm), ctypes.byref(out)),
                       "uam_tm_jprcs")
            return out
        return tm

    def _points(self, fn, name, pts, tm):
        torch = _torch()
        p = self.tensor(pts, torch.float64).reshape(-1, 2).contiguous()
        out = self.empty(tuple(p.shape), torch.float64)
        _lib.check(fn(self._ctx, ctypes.byref(self._tm(tm)), _ptr(p), p.shape[0], _ptr(out),
                      self.stream), name)
        return out

    def geo_to_plane(self, lonlat, tm=None):
        """[n, 2] lon, lat (deg) -> x (easting), y (northing) in metres; tm = JPRCS zone
        number (default 1 = EPSG:2443) or a TmParams."""
        return self._points(self.lib.uam_geo_to_plane, "uam_geo_to_plane", lonlat, tm)

    def plane_to_geo(self, xy, tm=None):
        """[n, 2] x, y metres -> lon, lat (deg)."""
        return self._points(self.lib.uam_plane_to_geo, "uam_plane_to_geo", xy, tm)

    def reproject_dem(self, src, src_grid, dst_geo, unit_m=1000.0, resample=0, tm=None):
        """Geographic DEM [ny, nx] float32 on src_grid (GeoGridDesc) -> plane DEM on the
        RasterGeo dst_geo (coordinates in units of unit_m metres)."""
        torch = _torch()
        s = self.tensor(src, torch.float32).contiguous()
        if tuple(s.shape) != (src_grid.ny, src_grid.nx):
            raise ValueError(f"src must be [{src_grid.ny}, {src_grid.nx}]")
        out = self.empty((dst_geo.ny, dst_geo.nx), torch.float32)
        _lib.check(self.lib.uam_reproject_dem(
            self._ctx, ctypes.byref(self._tm(tm)), _ptr(s), ctypes.byref(src_grid),
            ctypes.byref(dst_geo.as_struct()), float(unit_m), int(resample), _ptr(out),
            self.stream), "uam_reproject_dem")
        return out

    # -- land polygons from the DEM (K8) -------------------------------
    def dem_polygons(self, dem, geo, threshold=0.0, unit_m=1000.0, params=None):
        """DEM mask -> 4-connected regions (GPU labelling) -> DataProcessor approximation.
        dem [ny, nx] float32 on RasterGeo geo (units of unit_m metres).  -> list of int64
        [4, 2] rectangles in metres (cv2.boxPoints order)."""
        torch = _torch()
        d = self.tensor(dem, torch.float32).contiguous()
        if tuple(d.shape) != (geo.ny, geo.nx):
            raise ValueError(f"dem must be [{geo.ny}, {geo.nx}]")
        prm = params if params is not None else _lib.PolyprocParams(750000.0, 32000000.0,
                                                                    780000.0, 5, 0)
        n = ctypes.c_int32(0)
        cap = 256
        while True:
            out = np.zeros((cap, 4, 2), np.int64)
            st = self.lib.uam_dem_polygons(self._ctx, _ptr(d), ctypes.byref(geo.as_struct()),
                                           float(threshold), float(unit_m), ctypes.byref(prm),
                                           out.ctypes.data, cap, ctypes.byref(n), self.stream)
            if st == _lib.UAM_OK:
                return [out[i] for i in range(n.value)]
            if n.value > cap:
                cap = n.value
                continue
            _lib.check(st, "uam_dem_polygons")

    # -- raster broadcast over RCCL (uam_comm_* / uam_bcast_raster) ---------------------------
    def comm_unique_id(self):
        """128-byte RCCL unique id (rank 0 creates it, every rank passes it to comm_init)."""
        buf = (ctypes.c_uint8 * _lib.COMM_ID_BYTES)()
        _lib.check(self.lib.uam_comm_unique_id(buf), "uam_comm_unique_id")
        return bytes(buf)

    def comm_init(self, uid, nranks, rank):
        """Join the RCCL communicator of uid as rank of nranks (collective over the ranks)."""
        if len(uid) != _lib.COMM_ID_BYTES:
            raise ValueError(f"unique id must be {_lib.COMM_ID_BYTES} bytes")
        buf = (ctypes.c_uint8 * _lib.COMM_ID_BYTES).from_buffer_copy(uid)
        _lib.check(self.lib.uam_comm_init(self._ctx, buf, int(nranks), int(rank)),
                   "uam_comm_init")

    def bcast_raster(self, t, root=0):
        """Broadcast device tensor t (in place) from root over the context's communicator, on
        this engine's current stream."""
        if not t.is_cuda or not t.is_contiguous():
            raise ValueError("bcast_raster needs a contiguous device tensor")
        _lib.check(self.lib.uam_bcast_raster(self._ctx, _ptr(t), t.numel() * t.element_size(),
                                             int(root), self.stream), "uam_bcast_raster")
        return t

    def synchronize(self):
        """Wait for this engine's stream; raises DeviceCheckError when a call's device-side
        check failed (its outputs then hold NaN / -1)."""
        _lib.check(self.lib.uam_synchronize(self._ctx, self.stream), "uam_synchronize")

    def device_status(self):
        """Raise DeviceCheckError if a completed call's device-side check failed (no wait)."""
        _lib.check(self.lib.uam_device_status(self._ctx), "uam_device_status")


_default = {}


def default_engine(device=None):
    torch = _torch()
    if device is None:
        device = torch.cuda.current_device() if torch.cuda.is_available() else 0
    if device not in _default:
        _default[device] = Engine(device)
    return _default[device]


# ---- single-shape helpers used by the drop-in classes (scratch contexts) ------------------
# The reference evaluates psi / contains / collides point by point (problem.py:72-80 calls
# psi(x) per shape per point).  Each distinct (geometry, options) pair gets one context with its
# geometry and parameters uploaded once, kept in a small LRU cache, so a per-point loop costs
# one copy in, one launch and one copy out per call -- no allocation, upload or k_prepare.
_SCRATCH_MAX = 64
_scratch_cache = collections.OrderedDict()


def _scratch(geom, params):
    dev = default_engine().device
    key = (dev, geom.signature(), repr(params))
    eng = _scratch_cache.get(key)
    if eng is not None:
        _scratch_cache.move_to_end(key)
        return eng
    eng = Engine(dev)
    eng.set_geometry(geom)
    eng.set_params(params)
    _scratch_cache[key] = eng
    if len(_scratch_cache) > _SCRATCH_MAX:
        _scratch_cache.popitem(last=False)
    return eng


def _as_points(x):
    a = np.asarray(x, dtype=np.float64)
    single = a.size == 2
    return a.reshape(-1, 2), single


def shape_psi(obs, x, smooth, enlargement):
    """psi(x) of one shape: a one-region geometry with no centre and weight 1 -> phi = psi."""
    pts, single = _as_points(x)
    shape = type(obs).__new__(type(obs))
    shape.__dict__.update(obs.__dict__)
    shape.center = float("nan")
    geom = compile_shapes((), [[shape]])
    eng = _scratch(geom, PathParams(N=1, penalty_smooth=smooth, enlargement=enlargement,
                                    weights=(1.0,)))
    v = eng.eval_points(pts, want=("phi",))["phi"].cpu().numpy()
    return float(v[0]) if single else v


def shape_contains(obs, x):
    pts, single = _as_points(x)
    eng = _scratch(compile_shapes([obs], []), PathParams(N=1))
    v = eng.eval_points(pts, want=("collide",))["collide"].cpu().numpy().astype(bool)
    return bool(v[0]) if single else v


def map_collides(m, x):
    pts, single = _as_points(x)
    eng = _scratch(compile_shapes(list(m.obstacles), []), PathParams(N=1))
    v = eng.eval_points(pts, want=("collide",))["collide"].cpu().numpy().astype(bool)
    return bool(v[0]) if single else v
