"""Randomized refinement parity: the map, the options, the path size, the batch and the
optimiser's settings drawn from a seed (24 seeds of its own; test_gpu_fuzz.py does not cover
refinement).  Each case asserts

  * GPU == orc_refine bit for bit on wp, cost, infeas and iters;
  * against Engine.eval_waypoints(want_g=True), independent of orc_refine (refine_ref.py): the
    reported cost / infeas are those of the returned path (rtol 1e-12), iters stays within
    n_outer n_inner (1 + n_restart), the endpoints are untouched, and where n_outer = 1 the
    independent augmented objective of the plain (restart-free) run does not go up.

UAM_REFINE_FUZZ_SEEDS=a:b widens the sweep."""
import os

import numpy as np
import pytest

import refine_ref as R

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


def _seeds():
    v = os.environ.get("UAM_REFINE_FUZZ_SEEDS", "0:24")
    a, b = (int(x) for x in v.split(":"))
    return list(range(a, b))


def _draw(seed):
    rng = np.random.default_rng(7000 + seed)
    c = {}
    c["nfz"] = int(rng.choice([0, 8, 32, 100, 300]))
    c["map_seed"] = int(rng.integers(0, 50))
    c["opts"] = {"length_smooth": bool(rng.integers(0, 2)), "penalty_smooth": True,
                 "obstacle_smooth": True, "maxratio_smooth": bool(rng.integers(0, 2))}
    c["enl"] = float(rng.choice([0.0, 0.1, 0.35]))
    c["maxratio"] = float(rng.choice([1.04, 1.25, 2.0]))
    c["maxalpha"] = float(np.pi / rng.choice([5.0, 10.0, 80.0]))
    c["wscale"] = float(rng.choice([0.0, 1.0, 1.0, 3.7]))
    c["anchored"] = bool(rng.integers(0, 2))
    c["N"] = int(rng.choice([1, 2, 7, 40, 62, 63, 130, 254, 300]))
    c["P"] = int(rng.integers(1, 13))
    c["pair_seed"] = int(rng.integers(0, 1 << 30))
    c["rp"] = {"memory": int(rng.choice([0, 1, 3, 8])), "n_outer": int(rng.integers(1, 4)),
               "n_inner": int(rng.integers(1, 9)), "c0": float(rng.choice([1.0, 10.0, 100.0])),
               "rho": float(rng.choice([2.0, 5.0, 10.0])),
               "theta": float(rng.choice([0.1, 0.25, 0.5])),
               "n_restart": int(rng.choice([0, 0, 1, 2])) if c["N"] + 2 <= 512 else 0}
    return c


@pytest.fixture(scope="module")
def eng():
    from uam_path_planning_amd import build
    from uam_path_planning_amd.engine import Engine

    if not torch.cuda.is_available():
        pytest.fail("GPU tests need an MI355X")
    build.build_library()
    return Engine(0)


def _setup(eng, oracle_mod, c):
    from uam_path_planning_amd.engine import PathParams
    from uam_path_planning_amd.geometry import compile_map
    from uam_path_planning_amd.scenario import build_region_map, canonical_spec

    spec = canonical_spec(nfz_polygons=c["nfz"], seed=c["map_seed"])
    w = [float(x) * c["wscale"] for x in spec["weights"]]
    anchor = tuple(spec["x_start"]) if c["anchored"] else None
    eng.set_geometry(compile_map(build_region_map(spec)))
    eng.set_params(PathParams(N=c["N"], **c["opts"], maxratio=c["maxratio"],
                              maxalpha=c["maxalpha"], enlargement=c["enl"], weights=tuple(w),
                              anchor=anchor))
    return oracle_mod.Oracle(oracle_mod.compile_spec(spec), c["N"], c["opts"], c["maxratio"],
                             c["maxalpha"], c["enl"], w, anchor=anchor)


def _run(eng, orc, oracle_mod, wp, rp):
    gpu = eng.refine(wp, rp)
    torch.cuda.synchronize()
    out = {k: v.cpu().numpy() for k, v in gpu.items()}
    ref = orc.refine(wp, oracle_mod.refine_params(**rp))
    for k in ("iters", "wp", "cost", "infeas"):
        np.testing.assert_array_equal(out[k], ref[k], err_msg=k)
    return out


@pytest.mark.parametrize("seed", _seeds())
def test_refine_fuzz(eng, oracle_mod, seed):
    from uam_path_planning_amd.arcs import arc_table
    from uam_path_planning_amd.scenario import displacements
    from uam_path_planning_amd.synthetic import random_pairs

    c = _draw(seed)
    orc = _setup(eng, oracle_mod, c)
    N, P, rp = c["N"], c["P"], c["rp"]
    wp = oracle_mod.gen_paths(random_pairs((P + 4) // 5, seed=c["pair_seed"]),
                              arc_table(N, displacements(5))).reshape(-1, N + 2, 2)
    wp = R.jitter(wp, c["pair_seed"])[:P]
    ev = R.engine_eval(eng)
    out = _run(eng, orc, oracle_mod, wp, rp)
    np.testing.assert_array_equal(out["wp"][:, 0], wp[:, 0])
    np.testing.assert_array_equal(out["wp"][:, -1], wp[:, -1])
    R.check_contract(out, ev, rp)
    if rp["n_outer"] == 1:
        plain = out if rp["n_restart"] == 0 else _run(eng, orc, oracle_mod, wp,
                                                      dict(rp, n_restart=0))
        R.check_descent(wp, plain["wp"], ev, rp["c0"])
