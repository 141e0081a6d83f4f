"""Drawn call sequences for one long-lived context (test_gpu_sequence.py runs them on the GPU,
test_sequence_cases_cpu.py checks the generator and the oracle side without one).

draw(seed) returns the steps of one sequence: a list of dicts, every field drawn from
np.random.default_rng(7000 + seed), with the context's first geometry and parameters in its
.start.  Step kinds (the key "kind"):

  params         set_params with another N and other options
  geometry       set_geometry with another canonical map, then set_params
  k1             raster_build into raster slot 0 / 1 (a RasterGeo of its own), summary and pack
  raster_sorted  eval_generated on a slot with the sorted forms forced (K2h, or K2g under
                 maxratio_smooth / k2g_sim 0)
  raster_seq     the same with group 0: the reference's sequential order (K2s / K2 / K2w)
  raster_exact   exact_sum 1 (K2hx), then back to 0
  volume         volume_build + volume_pack over a slot's raster (kept until another is asked
                 for), eval_generated3d sorted (K4h, K4hx with exact) or sequential (K4)
  profiles       eval_generated3d_profiles(packed=True) on such a volume (K4hp)
  analytic       eval_generated(raster=None) (K3b / K3)
  reproject      reproject_dem onto a grid of drawn size
  polygons       dem_polygons on one of polygons_masks' small masks

Every sequence holds 13 or 14 steps: the two k1 steps, the chain

  raster_sorted(0)  raster_sorted(1, the largest)  volume|profiles (small)  analytic  geometry
  analytic  raster_exact(0)  params  raster_sorted(0)

two reproject steps (the larger grid first) and, in most seeds, one more step of a drawn kind at
a place that breaks none of the chain's adjacent pairs.  That is what conditions (a)-(h) of
test_sequence_cases_cpu.py need; the walk at the end of draw cuts every other step's batch below
the largest step's item count and keeps maxratio_smooth off where a form refuses it.

items(step): the (path, group) items of an evaluating step, Q D A ceil((N + 2) / G); a step
with sequential sums (group 0) counts one item a path.

Reference: the oracle's side of a sequence (geometry, parameters, rasters, the volume) and the
expected outputs of every evaluating step, as the per-family tests form them."""
import numpy as np

NS = (1, 7, 40, 80)
DS = (1, 2, 5, 16)
Q_MIN, Q_MAX = 16, 3000
RASTER_KINDS = ("raster_sorted", "raster_seq", "raster_exact")
VOLUME_KINDS = ("volume", "profiles")
EVALUATING = RASTER_KINDS + VOLUME_KINDS + ("analytic",)
# waypoints (Q D A W) an evaluating step may hold: what keeps its oracle (and, for the exact
# forms, the Python-integer reference) within a fraction of a second
WAYPOINT_CAP = {"raster_sorted": 600_000, "raster_seq": 600_000, "raster_exact": 30_000,
                "volume": 300_000, "volume_exact": 30_000, "profiles": 120_000,
                "analytic": 120_000}
BIG_CAP = 1_500_000
SMALL_MASKS = ("checkerboard", "diagonal", "staircase", "anti_staircase", "serpentine", "spiral",
               "rings", "noise50", "noise59", "noise70")

PATH_KEYS = ("cost", "length_q", "length", "kin_sum", "nfz_sum", "nfz_hits", "offmap",
             "min_clearance")
BEST_KEYS = ("best_fval_idx", "best_length_idx")


class Steps(list):
    """The steps of one sequence; start: the context's first geometry and parameters."""
    start = None


def family(step):
    k = step["kind"]
    return ("raster" if k in RASTER_KINDS else "volume" if k in VOLUME_KINDS else
            "analytic" if k == "analytic" else None)


def is_sorted(step):
    k = step["kind"]
    return k in ("raster_sorted", "raster_exact", "profiles") or \
        (k == "volume" and step["form"] == "sorted")


def effective_tile_bits(tbits):
    """The tile bits a raster of at most 2048 cells a side sorts on (0: the automatic 3)."""
    return tbits or 3


def items(step):
    W = step["N"] + 2
    G = step.get("group", 0) if is_sorted(step) else 0
    return step["Q"] * step["D"] * step.get("A", 1) * (-(-W // G) if G else 1)


def waypoints(step):
    return step["Q"] * step["D"] * step.get("A", 1) * (step["N"] + 2)


# ---- the draw ---------------------------------------------------------------------------------
def _log_uniform(rng, lo, hi):
    return int(round(float(np.exp(rng.uniform(np.log(lo), np.log(hi))))))


def _params(rng, N=None, not_N=None):
    ns = [n for n in NS if n != not_N]
    # (penalty_smooth off makes phi NaN at every point, by the reference's own arithmetic: it
    # is drawn seldom, so that most steps compare finite costs)
    return {"N": int(rng.choice(ns)) if N is None else N,
            "opts": {"length_smooth": bool(rng.integers(0, 2)),
                     "penalty_smooth": bool(rng.random() < 0.85),
                     "obstacle_smooth": bool(rng.integers(0, 2)),
                     "maxratio_smooth": bool(rng.random() < 0.3)},
            "enl": float(rng.choice([0.0, 0.1, 0.35])),
            "maxratio": float(rng.choice([1.04, 1.25, 2.0])),
            "maxalpha": float(np.pi / rng.choice([5.0, 10.0, 80.0])),
            "wscale": float(rng.choice([0.0, 1.0, 1.0, 3.7]))}


def _geometry(rng, not_like=None):
    while True:
        g = {"nfz": int(rng.choice([0, 8, 32])), "map_seed": int(rng.integers(0, 50))}
        if not_like is None or (g["nfz"], g["map_seed"]) != (not_like["nfz"],
                                                             not_like["map_seed"]):
            return g


def _batch(rng, lo=Q_MIN, hi=Q_MAX, ds=DS):
    return {"Q": _log_uniform(rng, lo, hi), "D": int(rng.choice(ds)),
            "pair_seed": int(rng.integers(0, 1 << 30))}


def _sort_options(rng, group=None):
    return {"group": int(rng.integers(1, 65)) if group is None else group,
            "chunk": int(rng.choice([0, 6, 7, 8, 11])), "terrain": int(rng.integers(0, 2)),
            "tbits": int(rng.choice([0, 3, 5])), "curve": int(rng.integers(0, 2))}


def _k1(rng, slot, not_dims=None):
    while True:
        nx, ny = int(rng.integers(120, 385)), int(rng.integers(120, 385))
        if nx != ny and (nx, ny) != not_dims:
            break
    # cells of 0.08-0.3 km: from a corner of the 60 km map to more than all of it
    return {"kind": "k1", "raster": slot,
            "geo": (nx, ny, float(rng.uniform(-5.0, 20.0)), float(rng.uniform(0.0, 25.0)),
                    float(rng.uniform(0.08, 0.3)), float(rng.uniform(0.08, 0.3))),
            "thr": float(rng.choice([0.0, 100.0, -9999.0])),
            "k1_rows": int(rng.choice([1, 2, 4, 8])), "dem_seed": int(rng.integers(1, 20))}


def _raster_sorted(rng, slot, **kw):
    s = {"kind": "raster_sorted", "raster": slot, **_batch(rng), **_sort_options(rng),
         "sim": int(rng.random() < 0.8), "cells": bool(rng.random() < 0.4)}
    s.update(kw)
    return s


def _raster_seq(rng, slot):
    return {"kind": "raster_seq", "raster": slot, **_batch(rng),
            "thresholds": str(rng.choice(["own", "zero"])), "cells": bool(rng.random() < 0.4)}


def _raster_exact(rng, slot):
    return {"kind": "raster_exact", "raster": slot, **_batch(rng), **_sort_options(rng)}


def _volume(rng, slot, small=False, form=None):
    s = {"kind": "volume", "raster": slot, "nz": int(rng.choice([7, 16, 33])),
         **(_batch(rng, 16, 60, (1, 2)) if small else _batch(rng)),
         **_sort_options(rng, int(rng.integers(16, 65)) if small else None),
         "form": form or str(rng.choice(["sorted", "sorted", "seq"]))}
    s["exact"] = bool(s["form"] == "sorted" and rng.random() < 0.35)
    return s


def _profiles(rng, slot, small=False):
    return {"kind": "profiles", "raster": slot, "nz": int(rng.choice([7, 16, 33])),
            **(_batch(rng, 16, 60, (1, 2)) if small else _batch(rng)),
            **_sort_options(rng, int(rng.integers(16, 65)) if small else None),
            "A": int(rng.choice([1, 3] if small else [1, 3, 8]))}


def _analytic(rng):
    return {"kind": "analytic", **_batch(rng), "k3b_segment": int(rng.choice([0, 8])),
            "pair_order": int(rng.integers(0, 2))}


def _reproject(rng, lo, hi):
    return {"kind": "reproject", "nx": int(rng.integers(lo, hi)), "ny": int(rng.integers(lo, hi)),
            "src_n": int(rng.choice([256, 300])), "resample": int(rng.integers(0, 2)),
            "dem_seed": int(rng.integers(1, 20))}


def _polygons(rng):
    return {"kind": "polygons", "mask": str(rng.choice(SMALL_MASKS)),
            "divided": bool(rng.integers(0, 2))}


def _shrink(step):
    """One cut of a step's item count: Q first, then D, the profiles, and the group length."""
    if step["Q"] > Q_MIN:
        step["Q"] = max(Q_MIN, step["Q"] // 2)
    elif step["D"] > 1:
        step["D"] = DS[DS.index(step["D"]) - 1]
    elif step.get("A", 1) > 1:
        step["A"] = 1
    else:
        assert step.get("group", 64) < 64, step
        step["group"] = min(64, step["group"] * 2)


def draw(seed):
    rng = np.random.default_rng(7000 + seed)
    start = {**_geometry(rng), "params": _params(rng)}
    k1a = _k1(rng, 0)
    k1b = _k1(rng, 1, not_dims=k1a["geo"][:2])
    ra = _raster_sorted(rng, 0)
    # (c): the next raster_sorted step sorts on another tile-key table
    while True:
        big = _raster_sorted(rng, 1, group=int(rng.integers(1, 5)), D=int(rng.choice([5, 16])),
                             Q=_log_uniform(rng, 1000, Q_MAX), big=True)
        if (effective_tile_bits(big["tbits"]), big["curve"]) != \
                (effective_tile_bits(ra["tbits"]), ra["curve"]):
            break
    # (a), (b): the largest step, then a small sorted step on the volume
    small = (_volume(rng, int(rng.integers(0, 2)), small=True, form="sorted")
             if rng.random() < 0.6 else _profiles(rng, int(rng.integers(0, 2)), small=True))
    geometry = {"kind": "geometry", **_geometry(rng, not_like=start), "params": _params(rng)}
    chain = [ra, big, small, _analytic(rng), geometry, _analytic(rng), _raster_exact(rng, 0),
             {"kind": "params", "params": None}, _raster_sorted(rng, 0)]
    chain[7]["params"] = _params(rng, not_N=geometry["params"]["N"])
    # positions in the chain before which another step may stand: none of (a)-(c)'s adjacent
    # pairs is split, and nothing comes between the exact step and the sorted step after it
    free = [0, 4, 5, len(chain)]
    extra = []
    rb, rs = _reproject(rng, 200, 321), _reproject(rng, 60, 151)
    for r, at in zip((rb, rs), sorted(rng.choice(free, 2).tolist())):
        extra.append((at, r))
    if rng.random() < 0.9:
        kind = str(rng.choice(["polygons", "profiles", "volume", "raster_seq"]))
        slot = int(rng.integers(0, 2))
        step = {"polygons": lambda: _polygons(rng), "profiles": lambda: _profiles(rng, slot),
                "volume": lambda: _volume(rng, slot),
                "raster_seq": lambda: _raster_seq(rng, slot)}[kind]()
        extra.append((int(rng.choice(free)), step))
    steps = Steps([k1a, k1b])
    for i in range(len(chain) + 1):
        steps.extend(s for at, s in extra if at == i)   # (stable: the larger grid stays first)
        if i < len(chain):
            steps.append(chain[i])
    steps.start = start
    # the walk: the parameters in force at every step
    cur = start["params"]
    for s in steps:
        if s["kind"] in ("params", "geometry"):
            cur = s["params"]
        elif is_sorted(s) and s["kind"] != "raster_sorted":
            cur["opts"]["maxratio_smooth"] = False   # K2hx / K4h / K4hp refuse it
    cur = start["params"]
    for s in steps:
        if s["kind"] in ("params", "geometry"):
            cur = s["params"]
        elif s["kind"] in EVALUATING:
            s["N"] = cur["N"]
    # sizes: each step within its oracle's budget, and the largest step the largest
    while waypoints(big) > BIG_CAP:
        big["Q"] = max(1000, big["Q"] * 3 // 4)
    for s in steps:
        if s["kind"] in EVALUATING and s is not big:
            cap = WAYPOINT_CAP["volume_exact" if s.get("exact") else s["kind"]]
            while waypoints(s) > cap and s["Q"] > Q_MIN:
                s["Q"] = max(Q_MIN, s["Q"] * 3 // 4)
            while items(s) >= items(big):
                _shrink(s)
    assert 4 * items(small) <= items(big)
    return steps


# ---- what both sides of a step are made from ----------------------------------------------------
def spec_of(g):
    from uam_path_planning_amd.scenario import canonical_spec

    return canonical_spec(nfz_polygons=g["nfz"], seed=g["map_seed"])


def weights_of(spec, p):
    return [float(x) * p["wscale"] for x in spec["weights"]]


def path_params(spec, p):
    """PathParams' keyword arguments for the drawn parameters p on the map spec."""
    return dict(N=p["N"], **p["opts"], maxratio=p["maxratio"], maxalpha=p["maxalpha"],
                enlargement=p["enl"], weights=tuple(weights_of(spec, p)), altitude=320.0)


def dem_of(step):
    from uam_path_planning_amd.synthetic import synthetic_dem

    nx, ny = step["geo"][:2]
    return synthetic_dem(max(nx, ny), seed=step["dem_seed"])[:ny, :nx].copy()


def pairs_of(step):
    """The step's pairs with the fuzz suite's edge rows: off the raster (volume), NaN,
    start == goal, below and above the volume."""
    from uam_path_planning_amd.synthetic import random_pairs, random_pairs3d

    Q = step["Q"]
    if step["kind"] in VOLUME_KINDS:
        pr = random_pairs3d(Q, seed=step["pair_seed"])
        pr[::41, 2] = -50.0
        pr[::43, 5] = 900.0
        pr[::97, 0] += 70.0
        pr[5, 1] = np.nan
        pr[11, 3:5] = pr[11, 0:2]
        return pr
    pr = random_pairs(Q, seed=step["pair_seed"])
    pr[::97, 0] += 70.0
    pr[5, 1] = np.nan
    pr[11, 2:] = pr[11, :2]
    return pr


def utab_of(step):
    from uam_path_planning_amd.arcs import arc_table
    from uam_path_planning_amd.scenario import displacements

    return arc_table(step["N"], displacements(step["D"]))


def ztab_of(step):
    import profiles_ref as R
    from uam_path_planning_amd import profiles as P

    fam = R.family(P, step["N"])
    return {1: fam[:1], 3: np.ascontiguousarray(fam[[0, 2, 7]]), 8: fam}[step["A"]]


def reproject_inputs(step):
    """(src DEM, (nx, ny, lon0, lat_top, dlon, dlat) of its grid, (nx, ny, x0, y_top, dx, dy) of
    the plane grid, in km): a lat/lon mosaic over part of the plane raster, as
    test_gpu_crs.py's."""
    from uam_path_planning_amd.synthetic import synthetic_dem

    n = step["src_n"]
    d = 5.5555555555554013e-05 * 8 * 1024 / n
    nx, ny = step["nx"], step["ny"]
    return (synthetic_dem(n, seed=step["dem_seed"]), (n, n, 129.55, 33.2, d, d),
            (nx, ny, 0.0, 20.0, 60.0 / nx, 60.0 / ny))


def options_of(step, defaults):
    """Every option the step's evaluation depends on (set before it: the context is shared);
    defaults: the library's own sorted_min_paths / wave_max_paths."""
    k = step["kind"]
    o = {"exact_sum": 0, "exact_sum_volume": 0, "k2g_sim": 1, "pair_order": 1, "k3b_segment": 8,
         "group": 21, "k2g_chunk": 0, "k2h_terrain": 1, "k4h_terrain": 0, "k2g_tile_bits": 0,
         "k2g_curve": 1, **defaults}
    if "group" in step:
        o.update(group=step["group"], k2g_chunk=step["chunk"], k2h_terrain=step["terrain"],
                 k4h_terrain=step["terrain"], k2g_tile_bits=step["tbits"],
                 k2g_curve=step["curve"], sorted_min_paths=0, wave_max_paths=0)
    if k == "raster_sorted":
        o["k2g_sim"] = step["sim"]
    elif k == "raster_seq":
        o["group"] = 0
        if step["thresholds"] == "zero":
            o.update(sorted_min_paths=0, wave_max_paths=0)
    elif k == "raster_exact":
        o["exact_sum"] = 1
    elif k == "volume":
        o["exact_sum_volume"] = int(step["exact"])
        if step["form"] == "seq":
            o["group"] = 0
    elif k == "analytic":
        o.update(k3b_segment=step["k3b_segment"], pair_order=step["pair_order"])
    return o


def _exact_field(words, cells):
    """fl(S) of the float32 words under each row's cells (-1: nothing) at the exponent of all
    the words: exact_sum_ref's definition, as test_gpu_exact_sum.py applies it."""
    import exact_sum_ref as X
    import profiles_h_ref as H

    ws = words.tolist()
    return H._exact_field(ws, cells, X.exponent(ws))


class Reference:
    """The oracle's side of one sequence."""

    def __init__(self, oracle_mod, start):
        self.O = oracle_mod
        self.rasters = {}
        self.vol = None
        self.geometry(start)

    def geometry(self, g):
        self.spec = spec_of(g)
        self.geom = self.O.compile_spec(self.spec)
        self.params(g["params"])

    def params(self, p):
        self.p = p
        self.orc = self.O.Oracle(self.geom, p["N"], p["opts"], p["maxratio"], p["maxalpha"],
                                 p["enl"], weights_of(self.spec, p), altitude=320.0)

    def k1(self, step):
        """The record raster [ny, nx, 4] float32 of a k1 step; kept as the slot's raster."""
        nx, ny, x0, yt, dx, dy = step["geo"]
        rd = self.O.Oracle.raster_desc(nx, ny, x0, yt, dx, dy, -9999.0, step["thr"])
        rec = self.orc.raster_build(rd, dem_of(step))
        self.rasters[step["raster"]] = {"rd": rd, "rec": rec, "geo": step["geo"]}
        if self.vol is not None and self.vol["key"][0] == step["raster"]:
            self.vol = None
        return rec

    def volume(self, step):
        """The step's volume (vdesc, vox, cols as float32), built when it is not the one held;
        returns (volume, whether it was built now)."""
        from uam_path_planning_amd.scenario import layer_weights

        key = (step["raster"], step["nz"])
        if self.vol is not None and self.vol["key"] == key:
            return self.vol, False
        r, nz = self.rasters[step["raster"]], step["nz"]
        nx, ny, x0, yt, dx, dy = r["geo"]
        vd = self.O.volume_desc(nx, ny, nz, x0, yt, dx, dy, 0.0, 640.0 / nz)
        vox, cols = self.O.volume_build(vd, r["rec"], layer_weights(nz))
        self.vol = {"key": key, "vd": vd, "vox": vox, "cols": cols}
        return self.vol, True

    def forced(self, step):
        """(kernel, group) the step's options force; kernel None: whichever sequential form the
        library's thresholds pick."""
        k, ms = step["kind"], self.p["opts"]["maxratio_smooth"]
        if k == "raster_sorted":
            return ("K2h+pack" if step["sim"] and not ms else "K2g+pack"), step["group"]
        if k == "raster_seq":
            return None, 0
        if k == "raster_exact":
            return "K2hx+pack", step["group"]
        if k == "volume":
            if step["form"] == "seq":
                return "K4", 0
            return ("K4hx+pack" if step["exact"] else "K4h+pack"), step["group"]
        if k == "profiles":
            return "K4hp+pack", step["group"]
        return ("K3b" if step["k3b_segment"] else "K3"), 0

    def _named(self, r, C):
        out = {"cost": r["cost"], "length_q": r["lq"], "length": r["length"],
               "kin_sum": r["kin"], "nfz_sum": r["nfz"], "nfz_hits": r["nfz_hits"],
               "offmap": r["offmap"], "min_clearance": r["min_clearance"]}
        if "below" in r:
            out["below_terrain"] = r["below"]
        if "cells" in r:
            out["cells"] = r["cells"]
        return self._select(out, C)

    def _select(self, out, C):
        with np.errstate(invalid="ignore"):
            out["best_fval_idx"] = self.O.argmin(out["cost"], C, True)
        out["best_length_idx"] = self.O.argmin(out["length"], C, False)
        return out

    def expect(self, step, kernel, group):
        """The expected outputs of an evaluating step that ran `kernel` with group length
        `group` (Engine.last_kernel / last_group, or forced()'s), under the product's names."""
        O, orc, k = self.O, self.orc, step["kind"]
        assert orc.N == step["N"]
        pairs, ut, D, N = pairs_of(step), utab_of(step), step["D"], step["N"]
        if k == "analytic":
            r = self._named(orc.eval_paths(O.gen_paths(pairs, ut), mode="analytic"), D)
            return {x: r[x] for x in PATH_KEYS[:6] + BEST_KEYS}
        if k in RASTER_KINDS:
            rs = self.rasters[step["raster"]]
            cells = k == "raster_exact" or step["cells"]
            if kernel.startswith("K2h"):
                r = orc.eval_generated_h(pairs, ut, rdesc=rs["rd"], rec=rs["rec"], group=group,
                                         want_cells=cells)
            else:   # K2g in group order, or a sequential form (group 0)
                r = orc.eval_paths(O.gen_paths(pairs, ut), mode="raster", rdesc=rs["rd"],
                                   rec=rs["rec"], group=group, want_cells=cells)
            out = self._named(r, D)
            if k == "raster_exact":
                w = rs["rec"].view(np.uint32).reshape(-1, 4)
                with np.errstate(invalid="ignore"):
                    out["cost"] = np.float64(N + 1) * out["length_q"] + \
                        _exact_field(w[:, 0], r["cells"]) / np.float64(N)
                out["nfz_sum"] = _exact_field(w[:, 1], r["cells"])
                self._select(out, D)
            return out
        v, _ = self.volume(step)
        host = (v["vox"], v["cols"])
        if k == "profiles":
            import profiles_h_ref as H

            r = H.evaluate(O, orc, v["vox"].view(np.uint32), v["cols"].view(np.uint32), pairs,
                           ut, ztab_of(step), group, vdesc=v["vd"])
            return {x: r[x] for x in H.KEYS + H.BEST}
        if not kernel.startswith("K4h"):   # the sequential lane-per-path K4
            return self._named(orc.eval_paths3d(O.gen_paths3d(pairs, ut), v["vd"], host), D)
        r = orc.eval_generated_h(pairs, ut, mode="volume", vdesc=v["vd"], vol=host, group=group,
                                 want_cells=step["exact"])
        out = self._named(r, D)
        if step["exact"]:
            w = v["vox"].view(np.uint32).reshape(-1, 2)
            with np.errstate(invalid="ignore"):
                out["cost"] = np.float64(N + 1) * out["length_q"] + \
                    _exact_field(w[:, 0], r["cells"]) / np.float64(N)
            out["nfz_sum"] = _exact_field(w[:, 1], r["cells"])
            self._select(out, D)
            del out["cells"]
        return out

    def reproject(self, step):
        src, gg, plane = reproject_inputs(step)
        rd = self.O.Oracle.raster_desc(*plane)
        return self.O.reproject(src, self.O.geo_grid(*gg), rd, 1000.0, step["resample"])

    def polygons(self, step):
        """(dem, Params, expected pieces, the oracle's rectangles) of a polygons step."""
        import polygons_masks as M

        mask, prm, pieces = M.case(step["mask"], "divided" if step["divided"] else "small")
        dem = M.dem_of(mask)
        return dem, prm, pieces, M.oracle_rects(self.O, dem, 0.0, prm)
