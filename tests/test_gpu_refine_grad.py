"""GPU refinement (k_refine / k_rf_push behind Engine.refine) against an independent statement
of what it minimises, at the launch shapes no other test reaches.

Independent side: the augmented Lagrangian rebuilt from Engine.eval_waypoints(want_g=True)
(tests/refine_ref.py), nothing of orc_refine.  Per shape:
  * the gradient the kernel descends along, read back through one step of known length,
    against central differences of that Lagrangian -- at y = 0 and, after one multiplier
    update, at y != 0; allowance = 10 x the finite difference's own error estimate + the
    read-back rounding (refine_ref.grad_check); at most 1% of the coordinates excluded as kinks;
  * within one outer iteration the independent objective does not go up;
  * the reported cost / infeas are those of the returned path (rtol 1e-12), iters within budget;
  * every run, the probes included, is also GPU == orc_refine bit for bit.
The shapes come from uam_refine's own launch formula, restated below and checked against the
source text and against the library's accept / refuse boundary: wpb = min(4, 65536 / per_wave)
waves per workgroup, per_wave = (6W + 3N + 2 RF_MAXM + mask_words W) * 8 bytes.
Measured on an MI355X over this file: error / allowance <= 0.30, error / the path's largest
component <= 4.3e-7, no coordinate excluded (DESIGN.md's parity section)."""
import os
import re

import numpy as np
import pytest

import golden_io as G
import refine_ref as R

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

OPTS = {"length_smooth": True, "penalty_smooth": True, "obstacle_smooth": True,
        "maxratio_smooth": False}
LDS = 65536


def _source():
    import uam_path_planning_amd

    # the one translation unit: the root and every piece it includes
    csrc = os.path.join(os.path.dirname(uam_path_planning_amd.__file__), "csrc")
    names = ["uampath.hip"] + sorted(f for f in os.listdir(csrc) if f.endswith(".inc"))
    text = []
    for name in names:
        with open(os.path.join(csrc, name)) as f:
            text.append(f.read())
    return "".join(text)


def _constants():
    src = _source()
    maxm = int(re.search(r"constexpr int RF_MAXM = (\d+);", src).group(1))
    maskw = int(re.search(r"constexpr int RF_MASKW = (\d+);", src).group(1))
    return src, maxm, maskw


_SRC, RF_MAXM, RF_MASKW = _constants()


def _mask_words(S):
    return (S + 63) >> 6 if 0 < S <= 64 * RF_MASKW else 0


def _per_wave(N, S):
    W = N + 2
    return (6 * W + 3 * N + 2 * RF_MAXM + _mask_words(S) * W) * 8


def _wpb(N, S):
    """Waves per workgroup uam_refine launches with; None where it refuses the size."""
    pw = _per_wave(N, S)
    return None if pw > LDS else min(4, LDS // pw)


def _largest_N(S, wpb):
    return max(N for N in range(1, 4096) if _wpb(N, S) == wpb)


@pytest.fixture(scope="module")
def eng():
    from uam_path_planning_amd import build
    from uam_path_planning_amd.engine import Engine

    if not torch.cuda.is_available():
        pytest.fail("GPU tests need an MI355X")
    build.build_library()
    return Engine(0)


def _setup(eng, oracle_mod, spec, N, opts=OPTS, enl=None, anchored=True):
    from uam_path_planning_amd.engine import PathParams
    from uam_path_planning_amd.geometry import compile_map
    from uam_path_planning_amd.scenario import build_region_map

    enl = spec["enlargement"] if enl is None else enl
    anchor = tuple(spec["x_start"]) if anchored else None
    eng.set_geometry(compile_map(build_region_map(spec)))
    eng.set_params(PathParams(N=N, **opts, maxratio=spec["maxratio"], maxalpha=spec["maxalpha"],
                              enlargement=enl, weights=tuple(spec["weights"]), anchor=anchor))
    return oracle_mod.Oracle(oracle_mod.compile_spec(spec), N, opts, spec["maxratio"],
                             spec["maxalpha"], enl, spec["weights"], anchor=anchor)


def _paths(oracle_mod, N, P, seed):
    from uam_path_planning_amd.arcs import arc_table
    from uam_path_planning_amd.scenario import displacements
    from uam_path_planning_amd.synthetic import random_pairs

    wp = oracle_mod.gen_paths(random_pairs((P + 4) // 5, seed=seed),
                              arc_table(N, displacements(5))).reshape(-1, N + 2, 2)
    return R.jitter(wp, seed)[:P]


def _both(eng, orc, oracle_mod):
    """Engine.refine as refine_ref's refine_fn; every call is also compared with orc_refine bit
    for bit (test_gpu_refine.py's _check)."""
    def fn(z, rp):
        gpu = eng.refine(z, rp)
        torch.cuda.synchronize()
        out = {k: v.cpu().numpy() for k, v in gpu.items()}
        ref = orc.refine(z, oracle_mod.refine_params(**rp))
        for k in ("iters", "wp", "cost", "infeas"):
            np.testing.assert_array_equal(out[k], ref[k], err_msg=k)
        return out
    return fn


def _full_check(eng, orc, oracle_mod, wp, n_grad, wpb, need_second=True):
    fn, ev = _both(eng, orc, oracle_mod), R.engine_eval(eng)
    R.assert_gradients(fn, ev, wp[:n_grad], need_second)
    for rp in (dict(n_outer=1, n_inner=6, memory=3), dict(n_outer=3, n_inner=8)):
        out = fn(wp, rp)
        np.testing.assert_array_equal(out["wp"][:, 0], wp[:, 0])
        np.testing.assert_array_equal(out["wp"][:, -1], wp[:, -1])
        R.check_contract(out, ev, rp)
        if rp["n_outer"] == 1:
            R.check_descent(wp, out["wp"], ev)
        # batches that fill no, one and two workgroups, each with a part-filled last one
        for P in sorted({1, wpb - 1, wpb + 1} - {len(wp)}):
            sub = fn(wp[:P], rp)
            for k in ("iters", "wp", "cost", "infeas"):
                np.testing.assert_array_equal(sub[k], out[k][:P], err_msg=f"P={P} {k}")


def test_launch_formula_is_the_librarys():
    """The restated formula is the one in uam_refine and k_refine (source text); its accept /
    refuse boundary is compared with the library's in test_refine_largest_n."""
    flat = re.sub(r"\s+", " ", _SRC)
    assert ("(6 * W + 3 * N + 2 * RF_MAXM + rf_mask_words(ctx->kg.n_obstacles) * W) * "
            "(int64_t)sizeof(double)") in flat
    assert "const int wpb = (int)std::min<int64_t>(4, 65536 / per_wave);" in flat
    assert "(6 * W + 3 * N + 2 * RF_MAXM + nmw * W)" in flat
    assert "return (S > 0 && S <= 64 * RF_MASKW) ? (S + 63) >> 6 : 0;" in flat
    assert (_mask_words(5), _mask_words(106), _mask_words(64 * RF_MASKW + 1)) == (1, 2, 0)


@pytest.mark.parametrize("N", [1, 2, 3, 62, 63])
def test_refine_short_paths_and_second_slot(eng, oracle_mod, N):
    """N = 1, 2, 3: W < 64, idle lanes, kinematic rows k = j-2..j clipped at both ends.
    N = 62, 63: W = 64, 65, the first lane that owns a second waypoint."""
    from uam_path_planning_amd.scenario import canonical_spec

    spec = canonical_spec()
    S = len(spec["obstacles"])
    assert _wpb(N, S) == 4
    orc = _setup(eng, oracle_mod, spec, N, dict(OPTS, length_smooth=bool(N & 1)),
                 anchored=bool(N & 2))
    _full_check(eng, orc, oracle_mod, _paths(oracle_mod, N, 9, 30 + N), 9, 4, N >= 62)


@pytest.mark.parametrize("wpb", [4, 3, 2])
def test_refine_waves_per_workgroup_boundaries(eng, oracle_mod, wpb):
    """The largest N launched with wpb waves per workgroup and the smallest with wpb - 1,
    P = 2 wpb + 1 paths and the smaller batches of _full_check."""
    from uam_path_planning_amd.scenario import canonical_spec

    spec = canonical_spec()
    S = len(spec["obstacles"])
    N = _largest_N(S, wpb)
    for n, w in ((N, wpb), (N + 1, wpb - 1)):
        assert _wpb(n, S) == w and _per_wave(n, S) * (w + 1) > LDS
        orc = _setup(eng, oracle_mod, spec, n)
        _full_check(eng, orc, oracle_mod, _paths(oracle_mod, n, 2 * w + 1, 40 + w), 2, w)


def test_refine_largest_n(eng, oracle_mod):
    """The largest N the LDS check accepts with S = 5 (one wave per workgroup, the whole 64 KiB)
    and N + 1 refused by the host check (nothing is launched)."""
    from uam_path_planning_amd.scenario import canonical_spec

    spec = canonical_spec()
    S = len(spec["obstacles"])
    assert S == 5
    N = _largest_N(S, 1)
    assert _wpb(N, S) == 1 and _wpb(N + 1, S) is None and _per_wave(N + 1, S) > LDS
    orc = _setup(eng, oracle_mod, spec, N)
    _full_check(eng, orc, oracle_mod, _paths(oracle_mod, N, 3, 50), 1, 1)
    _setup(eng, oracle_mod, spec, N + 1)
    with pytest.raises(ValueError, match="LDS"):
        eng.refine(_paths(oracle_mod, N + 1, 1, 51), dict(n_outer=1, n_inner=1))


def test_refine_restart_width_limit(eng, oracle_mod):
    """n_restart > 0 at W = 512 runs (k_rf_push stages 2W doubles per wave), W = 513 is
    refused; without restarts W = 513 runs."""
    from uam_path_planning_amd.scenario import canonical_spec

    spec = canonical_spec(nfz_polygons=16)
    S = len(spec["obstacles"])
    rp = dict(n_outer=2, n_inner=6, n_restart=1)
    orc = _setup(eng, oracle_mod, spec, 510)
    wpb = _wpb(510, S)
    wp = _paths(oracle_mod, 510, 2 * wpb + 1, 60)
    fn, ev = _both(eng, orc, oracle_mod), R.engine_eval(eng)
    out = fn(wp, rp)
    R.check_contract(out, ev, rp)
    plain = fn(wp, dict(rp, n_restart=0))
    assert (out["infeas"] <= plain["infeas"]).all()
    assert (out["iters"] > plain["iters"]).any()            # some path was restarted
    orc = _setup(eng, oracle_mod, spec, 511)
    wp = _paths(oracle_mod, 511, 2, 61)
    with pytest.raises(ValueError, match="restart"):
        eng.refine(wp, rp)
    _both(eng, orc, oracle_mod)(wp, dict(rp, n_restart=0))


@pytest.mark.parametrize("kind", ["two_mask_words", "full_rows", "region_list"])
def test_refine_gradient_many_shapes(eng, oracle_mod, kind):
    """The wave-cooperative geometry walk in each of its forms against the independent
    gradient: 106 obstacles (two active-row mask words per waypoint), 306 (no masks: every
    row), and a region table of more than 256 shapes (no per-cell bitmask).  Inside a polygon
    the gradient reaches 1e21: alpha0 per path (refine_ref.pick_alpha0)."""
    from uam_path_planning_amd.scenario import canonical_spec
    from uam_path_planning_amd.synthetic import random_convex_polygons

    if kind == "two_mask_words":
        spec = canonical_spec(nfz_polygons=100, seed=5)
        assert _mask_words(len(spec["obstacles"])) == 2
    elif kind == "full_rows":
        spec = canonical_spec(nfz_polygons=300, seed=4)
        assert len(spec["obstacles"]) > 64 * RF_MASKW
    else:
        spec = canonical_spec()
        spec["regions"][1]["shapes"] = spec["regions"][1]["shapes"] + [
            {"kind": "polygon", "vertices": v} for v in random_convex_polygons(260, seed=6)]
        assert sum(len(r["shapes"]) for r in spec["regions"]) > 256
    N = 40
    wpb = _wpb(N, len(spec["obstacles"]))
    orc = _setup(eng, oracle_mod, spec, N, dict(OPTS, length_smooth=False), enl=0.3)
    _full_check(eng, orc, oracle_mod, _paths(oracle_mod, N, 8, 70), 8, wpb)


def test_refine_batch_independence(eng, oracle_mod):
    """A path's result bits depend neither on its position in the batch nor on the batch size:
    a shuffled batch, and P = 1 against P = 9 (canonical candidates and generated ones)."""
    from uam_path_planning_amd.scenario import canonical_spec

    meta, arr = G.canonical()
    spec = canonical_spec()
    N = meta["N"]
    assert spec["N"] == N and spec["x_start"] == meta["map"]["x_start"]
    _setup(eng, oracle_mod, spec, N, spec["options"])
    wp = np.concatenate([G.canonical_paths(meta, arr), _paths(oracle_mod, N, 4, 80)])
    assert len(wp) == 9
    rp = dict(n_outer=3, n_inner=8)

    def run(z):
        out = eng.refine(z, rp)
        torch.cuda.synchronize()
        return {k: v.cpu().numpy() for k, v in out.items()}

    base = run(wp)
    perm = np.random.default_rng(3).permutation(len(wp))
    assert (perm != np.arange(len(wp))).any()
    shuffled = run(wp[perm])
    for k in ("iters", "wp", "cost", "infeas"):
        np.testing.assert_array_equal(shuffled[k], base[k][perm], err_msg=k)
    for p in range(len(wp)):
        one = run(wp[p:p + 1])
        for k in ("iters", "wp", "cost", "infeas"):
            np.testing.assert_array_equal(one[k][0], base[k][p], err_msg=f"path {p} {k}")
