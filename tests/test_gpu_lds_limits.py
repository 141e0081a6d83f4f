"""The dynamic-LDS limit is raised per kernel, on the kernel's first launch that needs it, and
remembered per context: one long-lived context that meets its kernels one at a time, in a mixed
order, must compute what a new context computes.

A launch that asks for more than 64 KiB of dynamic LDS fails unless the kernel's limit was raised
first, and the context raises it for the one instance it is about to launch.  With
k2g_lds_floor = 90000 every sorted evaluation asks for more than that, so each call below that
selects an instance the context has not launched yet (another chunk, the exact form, another
family) depends on the rule; the calls that come back to an instance depend on its being
remembered.  Every output of every call is compared, bit for bit, with the same call on a new
context with the same options -- the values the per-family tests (test_gpu_k2h.py, _k2g, _k4h,
_profiles_h, _exact_sum*, _route) hold against the oracle."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

N, Q, D = 19, 40, 3
# every option a call of this file sets; a call's own values go on top of these
BASE = dict(wave_max_paths=0, sorted_min_paths=0, group=7, k2g_lds_floor=90000, k2g_chunk=0,
            k2g_sim=1, exact_sum=0, exact_sum_volume=0, k9_tile=32)

# (the call, its options, uam_last_kernel afterwards -- None: the call does not set it)
CALLS = [
    ("raster", dict(k2g_chunk=7), "K2h+pack"),
    ("raster", dict(k2g_chunk=11), "K2h+pack"),
    ("raster", dict(k2g_chunk=6), "K2h+pack"),
    ("raster", dict(exact_sum=1), "K2hx+pack"),
    ("raster", dict(k2g_sim=0, k2g_chunk=8), "K2g+pack"),
    ("raster", dict(k2g_sim=0, k2g_chunk=16), "K2g+pack"),
    ("volume", dict(k2g_chunk=7), "K4h+pack"),
    ("volume", dict(k2g_chunk=8), "K4h+pack"),
    ("volume", dict(exact_sum_volume=1), "K4hx+pack"),
    ("profiles", dict(k2g_chunk=7), "K4hp+pack"),
    ("profiles", dict(k2g_chunk=11), "K4hp+pack"),
    ("route", dict(k9_tile=64), None),
    ("raster", dict(group=0), "K2s+pack"),
]


class Scene:
    """The inputs every context of this file evaluates (device buffers are not tied to the
    context that made them)."""

    def __init__(self):
        from uam_path_planning_amd import build, profiles
        from uam_path_planning_amd.arcs import arc_table
        from uam_path_planning_amd.engine import RasterGeo
        from uam_path_planning_amd.geometry import compile_map
        from uam_path_planning_amd.scenario import (build_region_map, canonical_params,
                                                    canonical_spec, displacements, layer_weights)
        from uam_path_planning_amd.synthetic import random_pairs, random_pairs3d

        if not torch.cuda.is_available():
            pytest.fail("GPU tests need an MI355X")
        build.build_library()
        spec = canonical_spec()
        self.geom = compile_map(build_region_map(spec))
        self.params = canonical_params(spec, N=N)
        e = self.engine()
        # a 96 x 80 raster over the canonical extent with a random DEM, packed; the volume is
        # built from the same DEM at half the resolution: 48 x 40 columns x 6 layers, packed
        dem = np.random.default_rng(5).uniform(0.0, 400.0, (80, 96)).astype(np.float32)
        geo = RasterGeo(nx=96, ny=80, x0=0.0, y_top=20.0, dx=60.0 / 96, dy=60.0 / 80,
                        nodata=-9999.0, dem_threshold=0.0)
        self.raster = e.raster_build(geo, dem)
        geo2 = RasterGeo(nx=48, ny=40, x0=0.0, y_top=20.0, dx=60.0 / 48, dy=60.0 / 40,
                         nodata=-9999.0, dem_threshold=0.0)
        self.volume = e.volume_build(e.raster_build(geo2, dem[::2, ::2].copy()), 6, 0.0, 100.0,
                                     layer_weights(6))
        e.volume_pack(self.volume)
        e.synchronize()
        self.pairs = random_pairs(Q, seed=3)
        self.pairs6 = random_pairs3d(Q, seed=3)
        self.utab = arc_table(N, displacements(D))
        self.ztab = profiles.stack(profiles.linear(N), profiles.cruise(N, 300.0))  # A = 2
        self.goals = np.array([[31.0, -9.0]])

    def engine(self):
        from uam_path_planning_amd.engine import Engine

        e = Engine(0)
        e.set_geometry(self.geom)
        e.set_params(self.params)
        return e

    def call(self, e, kind, opts):
        """The call on context e under BASE + opts: ({output: host array}, uam_last_kernel)."""
        for k, v in {**BASE, **opts}.items():
            e.set_option(k, v)
        if kind == "raster":
            o = e.eval_generated(self.pairs, self.utab, raster=self.raster)
        elif kind == "volume":
            o = e.eval_generated3d(self.pairs6, self.utab, self.volume)
        elif kind == "profiles":
            o = e.eval_generated3d_profiles(self.pairs6, self.utab, self.ztab, self.volume,
                                            packed=True)
        else:
            f = e.route_field(self.raster, self.goals)
            o = {"dist": f.dist, "next": f.next}
        return {k: v.cpu().numpy() for k, v in o.items()}, e.last_kernel()


def test_limits_are_raised_per_kernel_in_any_order():
    sc = Scene()
    long_lived = sc.engine()
    for i, (kind, opts, name) in enumerate(CALLS):
        what = f"call {i}: {kind} {opts}"
        got, got_name = sc.call(long_lived, kind, opts)
        want, want_name = sc.call(sc.engine(), kind, opts)
        if name is not None:
            assert got_name == name and want_name == name, (what, got_name, want_name)
        assert got.keys() == want.keys() and len(got) >= 2, what
        for k in want:
            assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, (what, k)
            assert got[k].tobytes() == want[k].tobytes(), f"{what}: {k} differs"
        if kind != "route":   # the batch is one the comparison says something about
            assert np.isfinite(want["cost"]).any(), what
