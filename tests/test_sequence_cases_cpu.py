"""The drawn sequences of test_gpu_sequence.py without a GPU: draw(seed) is deterministic, every
sequence holds what makes a long-lived context go wrong (conditions (a)-(h) below, asserted for
the default seeds and for seeds 0-199), stays within the sizes the GPU test is allowed, and the
oracle side accepts every step of seeds 0-1 -- none is skipped."""
import copy

import numpy as np
import pytest

import sequence_cases as S

DEFAULT_SEEDS = range(8)
SWEEP = range(200)
KINDS = ("params", "geometry", "k1", "raster_sorted", "raster_seq", "raster_exact", "volume",
         "profiles", "analytic", "reproject", "polygons")


def _evaluating(steps):
    return [(i, s) for i, s in enumerate(steps) if s["kind"] in S.EVALUATING]


def _holds(steps):
    """Which of (a)-(h) the sequence satisfies."""
    n = len(steps)
    kinds = [s["kind"] for s in steps]
    fam = [S.family(s) for s in steps]
    srt = [s["kind"] in S.EVALUATING and S.is_sorted(s) for s in steps]
    ev = _evaluating(steps)
    ok = {}
    # (a) the step with the most items is followed directly by a sorted step of another family
    # with at most a quarter as many
    most = max(S.items(s) for _, s in ev)
    at = [i for i, s in ev if S.items(s) == most]
    ok["a"] = len(at) == 1 and at[0] + 1 < n and srt[at[0]] and srt[at[0] + 1] and \
        fam[at[0] + 1] != fam[at[0]] and 4 * S.items(steps[at[0] + 1]) <= most
    # (b) raster -> volume, volume -> analytic, analytic -> raster as adjacent steps
    adj = set(zip(fam, fam[1:]))
    ok["b"] = {("raster", "volume"), ("volume", "analytic"), ("analytic", "raster")} <= adj
    # (c) two adjacent raster_sorted steps sort on different tile-key tables
    ok["c"] = any(a["kind"] == b["kind"] == "raster_sorted" and
                  (S.effective_tile_bits(a["tbits"]), a["curve"]) !=
                  (S.effective_tile_bits(b["tbits"]), b["curve"])
                  for a, b in zip(steps, steps[1:]))
    # (d) a params step that changes N between two sorted steps
    ok["d"] = False
    cur = steps.start["params"]["N"]
    for i, s in enumerate(steps):
        if s["kind"] in ("params", "geometry"):
            if s["kind"] == "params" and s["params"]["N"] != cur and any(srt[:i]) and \
                    any(srt[i + 1:]):
                ok["d"] = True
            cur = s["params"]["N"]
    # (e) a geometry step between two analytic steps
    ok["e"] = any(k == "geometry" and "analytic" in kinds[:i] and "analytic" in kinds[i + 1:]
                  for i, k in enumerate(kinds))
    # (f) a second raster of other dimensions is evaluated, then the first one again
    geo = {s["raster"]: s["geo"][:2] for s in steps if s["kind"] == "k1"}
    slots = [s["raster"] for s in steps if S.family(s) == "raster"]
    first = slots[0]
    other = [i for i, r in enumerate(slots) if r != first and geo[r] != geo[first]]
    ok["f"] = bool(other) and first in slots[other[0] + 1:]
    # (g) a reproject onto a smaller grid after a larger one
    rp = [s for s in steps if s["kind"] == "reproject"]
    ok["g"] = any(b["nx"] < a["nx"] and b["ny"] < a["ny"] for i, a in enumerate(rp)
                  for b in rp[i + 1:])
    # (h) exact sums on and off again between two ordinary sorted steps on the same raster
    ok["h"] = any(x["kind"] == "raster_exact" and
                  any(s["kind"] == "raster_sorted" and s["raster"] == x["raster"]
                      for s in steps[:i]) and
                  any(s["kind"] == "raster_sorted" and s["raster"] == x["raster"]
                      for s in steps[i + 1:])
                  for i, x in enumerate(steps))
    return ok


def _check_sizes(steps):
    assert 10 <= len(steps) <= 14
    built = set()
    N = steps.start["params"]["N"]
    for s in steps:
        assert s["kind"] in KINDS
        if s["kind"] in ("params", "geometry"):
            N = s["params"]["N"]
            assert N in (1, 7, 40, 80)
            if s["kind"] == "geometry":
                assert s["nfz"] in (0, 8, 32)
        elif s["kind"] == "k1":
            nx, ny = s["geo"][:2]
            assert 120 <= nx <= 400 and 120 <= ny <= 400 and nx != ny
            built.add(s["raster"])
        elif s["kind"] == "reproject":
            assert s["resample"] in (0, 1)
        if s["kind"] in S.EVALUATING:
            assert s["N"] == N                          # the annotation is the N in force
            assert 16 <= s["Q"] <= 3000 and s["D"] in (1, 2, 5, 16)
            assert s["Q"] * s["D"] <= 3000 * 16         # no batch above the fuzz suite's
            if "group" in s and S.is_sorted(s):
                assert 1 <= s["group"] <= 64
            if "raster" in s:
                assert s["raster"] in built             # built before it is evaluated
            if s["kind"] in S.VOLUME_KINDS:
                assert s["nz"] in (7, 16, 33)
            if s["kind"] == "profiles":
                assert s["A"] in (1, 3, 8)
            if s["kind"] == "raster_sorted":
                assert s["tbits"] in (0, 3, 5) and s["curve"] in (0, 1)
            if s["kind"] == "analytic":
                assert s["k3b_segment"] in (0, 8) and s["pair_order"] in (0, 1)


def test_draw_is_deterministic():
    for seed in SWEEP:
        a, b = S.draw(seed), S.draw(seed)
        assert a == b and a.start == b.start
    assert S.draw(0) != S.draw(1)


@pytest.mark.parametrize("seeds", [DEFAULT_SEEDS, SWEEP], ids=["default", "0-199"])
def test_every_sequence_holds_the_conditions(seeds):
    seen = set()
    for seed in seeds:
        steps = S.draw(seed)
        _check_sizes(steps)
        missing = [k for k, v in _holds(steps).items() if not v]
        assert not missing, (seed, missing, [s["kind"] for s in steps])
        seen |= {s["kind"] for s in steps}
    assert seen == set(KINDS)   # every kind of step occurs in the range


def test_the_conditions_can_fail():
    """The checker is not vacuous: taking a condition's step away is noticed."""
    steps = S.draw(0)

    def without(pred):
        t = S.Steps(copy.deepcopy([s for s in steps if not pred(s)]))
        t.start = steps.start
        return _holds(t)

    assert all(_holds(steps).values())
    assert not without(lambda s: s.get("big"))["a"]
    assert not without(lambda s: s["kind"] == "raster_exact")["h"]
    assert not without(lambda s: s["kind"] == "geometry")["e"]
    assert not without(lambda s: s["kind"] == "params")["d"]
    assert not without(lambda s: s["kind"] == "reproject" and s["nx"] < 160)["g"]
    assert not without(lambda s: s["kind"] in S.VOLUME_KINDS)["b"]
    assert not without(lambda s: s.get("raster") == 1 and s["kind"] != "k1")["f"]


@pytest.mark.parametrize("seed", [0, 1])
def test_the_oracle_accepts_every_step(oracle_mod, seed):
    """Every evaluating step of the sequence through the oracle side alone, in the form its
    options force (raster_seq: the sequential order): a drawn combination the reference
    refuses raises here."""
    import polygons_ref as R
    import polygons_masks as M

    steps = S.draw(seed)
    ref = S.Reference(oracle_mod, steps.start)
    ran = 0
    for s in steps:
        k = s["kind"]
        if k == "geometry":
            ref.geometry(s)
        elif k == "params":
            ref.params(s["params"])
        elif k == "k1":
            rec = ref.k1(s)
            assert rec.shape == (s["geo"][1], s["geo"][0], 4)
        elif k == "reproject":
            out = ref.reproject(s)
            assert out.shape == (s["ny"], s["nx"]) and (out != -9999.0).any()
        elif k == "polygons":
            dem, prm, pieces, rects = ref.polygons(s)
            R.check_rects(rects, pieces, M.DX_M, 0.0, dem.shape[0] * M.DX_M, {})
        else:
            kernel, group = ref.forced(s)
            out = ref.expect(s, kernel or "K2", group)
            P = s["Q"] * s["D"] * s.get("A", 1)
            assert out["cost"].shape == (P,) and out["best_fval_idx"].shape == (s["Q"],)
            if k == "analytic" and ref.p["opts"]["penalty_smooth"]:
                assert np.isfinite(out["cost"]).any()
        ran += 1
    assert ran == len(steps)
