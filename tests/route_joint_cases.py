"""The joint route field's test cases (tests/test_route_joint_cpu.py,
tests/test_gpu_route_joint.py), built from tests/route_cases.py's helpers on its 100 x 76 raster
(dx != dy, neither edge a multiple of the tile edges 16, 32 and 64): the smallest shapes at which
the joint seeding, the goal marking, the owner's pointer jumping and the resolved paths can each go
wrong.  reference(name) and reference_paths(name, span) compute tests/route_joint_ref.py's answer
once per process; the module asserts at import that the cases cover what they are meant to."""
import functools

import numpy as np

import route_cases as C
import route_joint_ref as J
import route_ref as R

GEO, NFZ, pt = C.GEO, C.NFZ, C.pt
SPANS = (0, 1, 7, 64)


def case(name, rec, goals, starts, lam=1.0, block_flags=NFZ, inflate=0, N=C.N_DEFAULT, geo=GEO):
    return dict(name=name, geo=geo, rec=np.ascontiguousarray(rec),
                goals=np.asarray(goals, dtype=np.float64).reshape(-1, 2),
                starts=np.asarray(starts, dtype=np.float64).reshape(-1, 2), lam=float(lam),
                block_flags=int(block_flags), inflate=int(inflate), N=int(N))


def small(nx, ny, rng):
    geo = C.Geo(nx, ny, -1.0, 2.0, 0.5, 0.25)
    rec = np.zeros((ny, nx, 4), dtype=np.float32)
    rec[..., 0] = rng.uniform(0.0, 2.0, size=(ny, nx)).astype(np.float32)
    return geo, rec


def all_cases():
    rng = np.random.default_rng(20252)
    cases = []
    # 1. five valid goals in five different tiles (of edge 16 and of edge 32)
    rec = C.open_field(rng)
    goals = [pt(10, 10), pt(90, 60), pt(55, 5), pt(20, 70), pt(50, 40)]
    cases.append(case("open_five", rec, goals, C.random_starts(rng, 10) + [pt(10, 10, 0.9, 0.1)]))

    # 2. an off-raster goal, two goals in one cell (indices 1 and 4: 1 owns it), a blocked goal,
    #    two goals in one tile
    rec = C.blank()
    rec[..., 0] = rng.uniform(0.0, 4.0, size=(GEO.ny, GEO.nx)).astype(np.float32)
    fl = C.flags_of(rec)
    fl[rng.random((GEO.ny, GEO.nx)) < 0.2] = NFZ
    for ix, iy in ((60, 50), (10, 10), (12, 11)):
        fl[iy, ix] = 0
    fl[30, 30] = NFZ
    goals = [[9.0, 9.0], pt(60, 50, 0.2, 0.2), pt(30, 30), pt(10, 10), pt(60, 50, 0.8, 0.8),
             pt(12, 11)]
    cases.append(case("shared_and_invalid", rec, goals,
                      C.random_starts(rng, 10) + [pt(60, 50), pt(30, 30), pt(11, 10)]))

    # 3. uniform phi and goals placed symmetrically: ties decided by the next-hop rule alone
    goals = [pt(25, 20), pt(74, 20), pt(25, 55), pt(74, 55)]
    cases.append(case("symmetric", C.blank(0.5), goals,
                      [pt(49, 37), pt(50, 38), pt(49, 20), pt(25, 37), pt(0, 0), pt(99, 75),
                       pt(50, 0), pt(60, 38)]))

    # 4. the spiral with goals at its two ends: chains longer than 1024 steps
    rec, outer, inner = C.spiral()
    cases.append(case("spiral_ends", rec, [pt(*inner), pt(*outer)],
                      [pt(50, 1), pt(97, 40), pt(40, 30), pt(0, 0), pt(2, 40)]))

    # 5. a walled pocket no goal reaches (status 2) and starts in blocked cells (status 1)
    rec = C.blank(0.25)
    fl = C.flags_of(rec)
    fl[20:41, 30] = fl[20:41, 50] = NFZ
    fl[20, 30:51] = fl[40, 30:51] = NFZ
    cases.append(case("pocket", rec, [pt(5, 5), pt(90, 70), pt(70, 10)],
                      [pt(40, 30), pt(31, 21), pt(30, 25), pt(50, 40), pt(60, 20), pt(10, 60),
                       [GEO.x0 - 0.001, 2.5], [float("nan"), 2.5]]))

    # 6. the existing absorption case with its first goal alone: equal dist values form a cycle
    ab = C.BY_NAME["absorption"]
    cases.append(case("absorption_joint", ab["rec"], ab["goals"][:1],
                      list(ab["starts"]) + [pt(51, 31), pt(49, 30), pt(96, 30)]))

    # 7. no valid goal at all
    cases.append(case("no_valid_goal", rec, [pt(30, 25), [9.0, 9.0], [float("nan"), 0.0]],
                      [pt(5, 5), pt(40, 30), pt(30, 25)]))

    # 8. inflate = 2 with a goal that the inflation blocks (two cells from an NFZ cell)
    rec = C.blank()
    rec[..., 0] = rng.uniform(0.0, 2.0, size=(GEO.ny, GEO.nx)).astype(np.float32)
    fl = C.flags_of(rec)
    fl[rng.random((GEO.ny, GEO.nx)) < 0.012] = NFZ
    fl[28:39, 43:54] = 0
    fl[60:71, 15:26] = 0
    fl[10, 80] = NFZ
    cases.append(case("inflate_2", rec, [pt(48, 33), pt(82, 12), pt(20, 65)],
                      C.random_starts(rng, 8) + [pt(82, 12)], inflate=2))

    # 9. rasters of 1 x 1 and 3 x 2 cells
    geo, rec = small(1, 1, rng)
    cases.append(case("raster_1x1", rec, [[-0.8, 1.9]], [[-0.6, 1.8], [0.0, 0.0]], geo=geo))
    geo, rec = small(3, 2, rng)
    C.flags_of(rec)[0, 1] = NFZ
    cases.append(case("raster_3x2", rec, [[-0.9, 1.9], [0.4, 1.6], [0.4, 1.9]],
                      [[0.3, 1.9], [-0.9, 1.6], [-0.3, 1.9], [-0.3, 1.6], [5.0, 5.0]], geo=geo))

    # 10. one goal, on two of the existing cases: bridges 2 and 3
    for name in ("open", "random30"):
        c = C.BY_NAME[name]
        cases.append(case(f"single_{name}", c["rec"], c["goals"], c["starts"], lam=c["lam"],
                          block_flags=c["block_flags"], inflate=c["inflate"], N=c["N"]))
    return cases


CASES = all_cases()
NAMES = [c["name"] for c in CASES]
BY_NAME = {c["name"]: c for c in CASES}
SINGLE = {"single_open": "open", "single_random30": "random30"}  # case -> route_cases' name
# the cases the standalone sanitizer program is fed (tools/san_route_joint.cpp)
SANITIZE = ("shared_and_invalid", "spiral_ends", "raster_1x1", "raster_3x2")


@functools.lru_cache(maxsize=None)
def reference(name):
    """route_joint_ref's dict(dist, next, owner, longest, cost) of a case; read-only."""
    c = BY_NAME[name]
    cost = R.cost_plane(c["geo"], c["rec"].view(np.uint32), c["lam"], c["block_flags"],
                        c["inflate"])
    dist, nxt, owner, longest = J.field(c["geo"], cost, c["goals"])
    for a in (dist, nxt, owner):
        a.setflags(write=False)
    return dict(dist=dist, next=nxt, owner=owner, longest=longest, cost=cost)


@functools.lru_cache(maxsize=None)
def reference_paths(name, span):
    """route_joint_ref's dict(wp, status, steps, vertices, goal) of a case's starts; read-only."""
    c, r = BY_NAME[name], reference(name)
    out = J.paths(c["geo"], r["cost"], r["next"], r["owner"], c["goals"], c["starts"], c["N"],
                  span)
    for a in out:
        a.setflags(write=False)
    return dict(zip(("wp", "status", "steps", "vertices", "goal"), out))


@functools.lru_cache(maxsize=None)
def per_goal_reference(name):
    """route_ref's per-goal (dist [G, ny, nx], next [G, ny, nx]) of a case's goals."""
    c = BY_NAME[name]
    dist, nxt, _ = R.route_field(c["geo"], c["rec"].view(np.uint32), c["goals"], c["lam"],
                                 c["block_flags"], c["inflate"])
    return dist, nxt


def _check_cover():
    """What the cases are there for, asserted against the reference: no comparison downstream
    can pass vacuously."""
    owners, statuses = set(), set()
    for name in NAMES:
        owners |= set(np.unique(reference(name)["owner"]).tolist())
        statuses |= set(reference_paths(name, 0)["status"].tolist())
    assert len([o for o in owners if o >= 0]) >= 3, owners
    assert statuses == {0, 1, 2, 3}, statuses
    assert reference("spiral_ends")["longest"] > 1024, reference("spiral_ends")["longest"]
    assert 3 in reference_paths("absorption_joint", 0)["status"]
    r = reference("shared_and_invalid")
    assert r["owner"][50, 60] == 1 and set(np.unique(r["owner"]).tolist()) <= {-1, 1, 3, 5}
    r = reference("no_valid_goal")
    assert np.all(np.isinf(r["dist"])) and np.all(r["owner"] == -1)
    r = reference("pocket")
    assert np.any((r["owner"] == -1) & np.isfinite(np.array(r["cost"])))
    r = reference("inflate_2")
    assert 1 not in np.unique(r["owner"]).tolist() and r["next"][12, 82] == 255
    r = reference("symmetric")
    assert sorted(np.unique(r["owner"]).tolist()) == [0, 1, 2, 3]


_check_cover()
