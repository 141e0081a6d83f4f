"""The volume's joint route field's test cases (tests/test_route3d_joint_cpu.py,
tests/test_gpu_route3d_joint.py), built from tests/route3d_cases.py's helpers on its 43 x 29 x 11
volume (partial tiles on every axis for every tile shape): the smallest shapes at which the joint
seeding, the goal marking, the parent volume over 26 directions, the owner's pointer jumping and
the resolved paths can each go wrong.  reference(name) and reference_paths(name, span) compute
tests/route3d_joint_ref.py's answer once per process; the module asserts at import that the cases
cover what they are meant to."""
import functools

import numpy as np

import route3d_cases as C
import route3d_joint_ref as J
import route3d_ref as R
import route_cases as C2
import route_joint_cases as JC2

GEO, NFZ, pt, Geo = C.GEO, C.NFZ, C.pt, C.Geo
SPANS = (0, 1, 7, 64)


def case(name, vol, goals, starts, flat=None, **kw):
    c = C.case(name, vol, goals, starts, **kw)
    del c["goal_idx"]
    c["flat"] = flat   # the raster case a one-layer volume was carried over from
    return c


def from_raster(rc, points):
    """A raster case's records as a one-layer volume, the nz1_bridge way (the layer centre above
    every terrain value, agl = 0), and its points at the layer centre."""
    g2 = rc["geo"]
    geo = Geo(g2.nx, g2.ny, 1, g2.x0, g2.y_top, g2.dx, g2.dy, 1000.0, 50.0)
    rec = np.ascontiguousarray(rc["rec"])
    risk = np.ascontiguousarray(rec[..., 0], dtype=np.float32)[:, :, None]
    terrain = np.zeros((g2.ny, g2.nx), dtype=np.float32)
    flags = np.ascontiguousarray(rec.view(np.uint32)[..., 3])
    p = np.asarray(points, dtype=np.float64).reshape(-1, 2)
    return geo, (risk, terrain, flags), np.column_stack([p, np.full(len(p), 1025.0)])


def serpentine():
    """A corridor one voxel wide through the even layers, everything else blocked by non-finite
    risk: every even layer holds the same snake over the rows 0, 2, .., 28, walked forward and
    backward in turn, and a shaft of one voxel through the odd layer between joins the ends.
    Returns the volume and the corridor's two ends."""
    risk, terrain, flags = C.blank(np.nan)
    for iz in range(0, GEO.nz, 2):
        for j, iy in enumerate(range(0, GEO.ny, 2)):
            risk[iy, :, iz] = 0.25
            if iy + 1 < GEO.ny:
                risk[iy + 1, GEO.nx - 1 if j % 2 == 0 else 0, iz] = 0.25
    last = (GEO.nx - 1, GEO.ny - 1)   # 15 rows: the snake ends in the south-east corner
    for j, iz in enumerate(range(1, GEO.nz, 2)):
        x, y = last if j % 2 == 0 else (0, 0)
        risk[y, x, iz] = 0.25
    return (risk, terrain, flags), (0, 0, 0), (0, 0, GEO.nz - 1)


def all_cases():
    rng = np.random.default_rng(20254)
    cases = []
    # 1. five valid goals in five different tiles of the largest shape (16 x 16 x 8), each at a
    #    layer of its own, and two more that share one 8 x 8 x 4 tile
    vol = C.open_volume(rng)
    goals = [pt(5, 5, 1), pt(38, 24, 9), pt(22, 3, 4), pt(6, 22, 10), pt(20, 20, 6),
             pt(33, 9, 2), pt(38, 14, 3)]
    cases.append(case("open_five", vol, goals,
                      C.random_starts(rng, 10) + [pt(5, 5, 1, 0.9, 0.1, 0.8)]))

    # 2. invalid goals (off the volume in x, in z, by NaN, in a flagged column, below terrain +
    #    agl), two goals in one voxel (indices 1 and 6: 1 owns it), two valid ones besides
    risk, terrain, flags = C.blank()
    risk[...] = rng.uniform(0.0, 4.0, size=risk.shape).astype(np.float32)
    flags[rng.random(flags.shape) < 0.15] = NFZ
    for ix, iy in ((30, 20), (8, 6), (12, 25), (25, 10)):
        flags[iy, ix] = 0
    flags[15, 15] = NFZ
    terrain[10, 25] = C.layer_centre(4)       # layers 0..4 lie below terrain + agl
    goals = [[GEO.x0 - 0.001, 2.8, 200.0], pt(30, 20, 5, 0.2, 0.2, 0.2),
             [0.5, 2.8, GEO.z0 + GEO.nz * GEO.dz + 1.0], pt(8, 6, 2), [0.5, float("nan"), 200.0],
             pt(15, 15, 5), pt(30, 20, 5, 0.8, 0.8, 0.8), pt(25, 10, 4), pt(12, 25, 9)]
    cases.append(case("shared_and_invalid", (risk, terrain, flags), goals,
                      C.random_starts(rng, 10) + [pt(30, 20, 5), pt(15, 15, 5), pt(25, 10, 4),
                                                  pt(25, 10, 5)], agl=10.0))

    # 3. uniform risk and goals placed symmetrically in x, y and z: ties decided by the next-hop
    #    rule alone
    goals = [pt(x, y, z, 0.5, 0.5, 0.5) for z in (2, 8) for y in (7, 21) for x in (10, 32)]
    cases.append(case("symmetric", C.blank(0.5), goals,
                      [pt(21, 14, 5), pt(21, 14, 2), pt(10, 14, 5), pt(21, 7, 8), pt(0, 0, 0),
                       pt(42, 28, 10), pt(22, 14, 5), pt(21, 15, 6)]))

    # 4. the serpentine with goals at its two ends: chains longer than 1024 voxels
    vol, a, b = serpentine()
    cases.append(case("serpentine_ends", vol, [pt(*a), pt(*b)],
                      [pt(20, 14, 4), pt(42, 28, 5), pt(0, 0, 6), pt(42, 28, 4), pt(30, 0, 10),
                       pt(5, 5, 5)]))

    # 5. a sealed box no goal reaches (status 2), starts in blocked voxels, off the volume and by
    #    NaN (status 1)
    sb = C.BY_NAME["sealed_box"]
    vol = (sb["risk"], sb["terrain"], sb["flags"])
    cases.append(case("pocket", vol, [pt(2, 2, 2), pt(40, 27, 10), pt(30, 5, 0)],
                      [pt(15, 13, 5), pt(12, 10, 4), pt(10, 13, 5), pt(18, 18, 8), pt(30, 20, 3),
                       pt(3, 25, 9), [GEO.x0 - 0.001, 2.8, 200.0],
                       [0.5, 2.8, GEO.z0 + GEO.nz * GEO.dz + 1.0], [float("nan"), 2.8, 200.0]]))

    # 6. the flat absorption case with its first goal alone, carried over as one layer: equal
    #    dist values form a cycle
    ab = C2.BY_NAME["absorption"]
    flat = JC2.BY_NAME["absorption_joint"]
    geo, vol, pts = from_raster(ab, np.vstack([flat["goals"], flat["starts"]]))
    cases.append(case("absorption_joint", vol, pts[:1], pts[1:], flat="absorption_joint", geo=geo))

    # 7. no valid goal at all (a goal in the box's wall, one off the volume, one by NaN)
    vol = (sb["risk"], sb["terrain"], sb["flags"])
    cases.append(case("no_valid_goal", vol,
                      [pt(10, 13, 5), [9.0, 9.0, 100.0], [float("nan"), 2.8, 200.0]],
                      [pt(2, 2, 2), pt(15, 13, 5), pt(10, 13, 5)]))

    # 8. inflate = 2 with a goal that the inflation blocks (two columns from a flagged one), and
    #    agl = 20 over random terrain as in route3d_cases' random30
    risk, terrain, flags = C.blank()
    risk[...] = rng.uniform(0.0, 2.0, size=risk.shape).astype(np.float32)
    flags[rng.random(flags.shape) < 0.02] = NFZ
    terrain[rng.random(terrain.shape) < 0.03] = C.layer_centre(3) + 1.0
    for ys, xs in ((slice(10, 19), slice(17, 26)), (slice(2, 9), slice(2, 9))):
        flags[ys, xs] = 0
        terrain[ys, xs] = 0.0
    flags[22, 36] = NFZ
    cases.append(case("inflate_2", (risk, terrain, flags),
                      [pt(21, 14, 5), pt(38, 24, 6), pt(5, 5, 8)],
                      C.random_starts(rng, 8) + [pt(38, 24, 6)], inflate=2))
    r30 = C.BY_NAME["random30"]
    vol = (r30["risk"].copy(), r30["terrain"].copy(), r30["flags"])
    vol[1][5, 8] = vol[1][24, 36] = 0.0
    cases.append(case("agl_20", vol, [pt(21, 14, 2), pt(8, 5, 0), pt(36, 24, 7)],
                      C.random_starts(rng, 10), agl=20.0))

    # 9. volumes of 1 x 1 x 1 and 3 x 2 x 2 voxels
    geo = Geo(1, 1, 1, -1.0, 2.0, 0.5, 0.25, 40.0, 30.0)
    vol = C.blank(0.5, geo=geo)
    cases.append(case("volume_1x1x1", vol, [pt(0, 0, 0, geo=geo)],
                      [pt(0, 0, 0, 0.8, 0.2, 0.9, geo=geo), [0.0, 0.0, 50.0]], geo=geo))
    geo = Geo(3, 2, 2, -1.0, 2.0, 0.5, 0.25, 40.0, 30.0)
    risk, terrain, flags = C.blank(geo=geo)
    risk[...] = rng.uniform(0.0, 2.0, size=risk.shape).astype(np.float32)
    flags[0, 1] = NFZ
    cases.append(case("volume_3x2x2", (risk, terrain, flags),
                      [pt(0, 0, 0, geo=geo), pt(2, 1, 1, geo=geo), pt(2, 0, 1, geo=geo)],
                      [pt(2, 0, 0, geo=geo), pt(0, 1, 1, geo=geo), pt(1, 0, 0, geo=geo),
                       pt(1, 1, 1, geo=geo), [5.0, 5.0, 50.0]], geo=geo))

    # 10. one goal, on two of the existing cases: bridges 2 and 3
    for name in ("open3d", "random30"):
        c = C.BY_NAME[name]
        cases.append(case(f"single_{name}", (c["risk"], c["terrain"], c["flags"]), c["goals"],
                          c["starts"], lam=c["lam"], block_flags=c["block_flags"],
                          inflate=c["inflate"], agl=c["agl"], kappa=c["kappa"]))

    # 11. nz = 1: the flat joint field's shared_and_invalid raster carried over (bridge 4)
    flat = JC2.BY_NAME["shared_and_invalid"]
    geo, vol, pts = from_raster(flat, np.vstack([flat["goals"], flat["starts"]]))
    G = len(flat["goals"])
    cases.append(case("nz1_shared_and_invalid", vol, pts[:G], pts[G:], flat="shared_and_invalid",
                      lam=flat["lam"], block_flags=flat["block_flags"], inflate=flat["inflate"],
                      geo=geo))
    return cases


CASES = all_cases()
NAMES = [c["name"] for c in CASES]
BY_NAME = {c["name"]: c for c in CASES}
SINGLE = {"single_open3d": "open3d", "single_random30": "random30"}  # -> route3d_cases' name
FLAT = {n: c["flat"] for n, c in BY_NAME.items() if c["flat"]}         # -> route_joint_cases'
# bridge 1 against the per-goal device call (cases 1, 2, 3, 5, 8 and the 3 x 2 x 2 volume)
BRIDGE1_GPU = ("open_five", "shared_and_invalid", "symmetric", "pocket", "inflate_2", "agl_20",
               "volume_3x2x2")
# the cases the stand-alone sanitizer program is fed (tools/san_route3d_joint.cpp): 2, 4 and 9
SANITIZE = ("shared_and_invalid", "serpentine_ends", "volume_1x1x1", "volume_3x2x2")


@functools.lru_cache(maxsize=None)
def reference(name):
    """route3d_joint_ref's dict(dist, next, owner, longest, cost) of a case; read-only."""
    c = BY_NAME[name]
    cost = R.cost_volume(c["geo"], c["risk"], c["terrain"], c["flags"], c["lam"],
                         c["block_flags"], c["inflate"], c["agl"])
    dist, nxt, owner, longest = J.field(c["geo"], cost, c["goals"], c["kappa"])
    for a in (dist, nxt, owner):
        a.setflags(write=False)
    return dict(dist=dist, next=nxt, owner=owner, longest=longest, cost=cost)


@functools.lru_cache(maxsize=None)
def reference_paths(name, span):
    """route3d_joint_ref's dict(wp3, status, steps, vertices, goal) of a case's starts;
    read-only."""
    c, r = BY_NAME[name], reference(name)
    out = J.paths(c["geo"], r["cost"], r["next"], r["owner"], c["goals"], c["starts"], c["N"],
                  c["kappa"], span)
    for a in out:
        a.setflags(write=False)
    return dict(zip(("wp3", "status", "steps", "vertices", "goal"), out))


def free(name):
    """The free voxels of a case's reference cost volume, [ny, nx, nz] bool."""
    return np.isfinite(np.array(reference(name)["cost"], dtype=np.float64))


def _check_cover():
    """What the cases are there for, asserted against the reference: no comparison downstream
    can pass vacuously."""
    owners, statuses = set(), set()
    for name in NAMES:
        owners |= set(np.unique(reference(name)["owner"]).tolist())
        statuses |= set(reference_paths(name, 0)["status"].tolist())
    assert len([o for o in owners if o >= 0]) >= 3, owners
    assert statuses == {0, 1, 2, 3}, statuses
    # 1: five tiles of the largest shape, seven layers, two goals in one 8 x 8 x 4 tile
    vox, gc = J.goal_voxels(GEO, reference("open_five")["cost"], BY_NAME["open_five"]["goals"])
    assert None not in vox and len(gc) == 7
    assert len({(x // 16, y // 16, z // 8) for x, y, z in vox[:5]}) == 5
    assert len({z for _, _, z in vox}) == 7
    assert len({(x // 8, y // 8, z // 4) for x, y, z in vox[5:]}) == 1
    assert sorted(np.unique(reference("open_five")["owner"]).tolist()) == list(range(7))
    # 2
    r = reference("shared_and_invalid")
    vox, gc = J.goal_voxels(GEO, r["cost"], BY_NAME["shared_and_invalid"]["goals"])
    assert [i for i, v in enumerate(vox) if v is None] == [0, 2, 4, 5, 7], vox
    assert vox[1] == vox[6] == (30, 20, 5) and r["owner"][20, 30, 5] == 1
    assert set(np.unique(r["owner"]).tolist()) == {-1, 1, 3, 8}
    assert r["next"][10, 25, 4] == 255 and r["next"][10, 25, 5] < 26   # below / above terrain + agl
    # 3
    r = reference("symmetric")
    assert sorted(np.unique(r["owner"]).tolist()) == list(range(8))
    # 4
    r = reference("serpentine_ends")
    assert r["longest"] > 1024, r["longest"]
    assert sorted(np.unique(r["owner"]).tolist()) == [-1, 0, 1]
    # 5
    r = reference("pocket")
    assert np.any((r["owner"] == -1) & free("pocket"))
    assert {1, 2} <= set(reference_paths("pocket", 0)["status"].tolist())
    # 6
    assert 3 in reference_paths("absorption_joint", 0)["status"]
    r = reference("absorption_joint")
    assert np.any((r["owner"] == -1) & np.isfinite(r["dist"]))
    # 7
    r = reference("no_valid_goal")
    assert np.all(np.isinf(r["dist"])) and np.all(r["owner"] == -1)
    assert reference_paths("no_valid_goal", 0)["status"].tolist() == [2, 2, 1]
    # 8
    r = reference("inflate_2")
    assert 1 not in np.unique(r["owner"]).tolist() and r["next"][24, 38, 6] == 255
    assert sorted(set(np.unique(r["owner"]).tolist()) - {-1}) == [0, 2]
    r = reference("agl_20")
    assert sorted(set(np.unique(r["owner"]).tolist()) - {-1}) == [0, 1, 2]
    # 9
    assert reference("volume_1x1x1")["owner"].tolist() == [[[0]]]
    assert len(set(np.unique(reference("volume_3x2x2")["owner"]).tolist()) - {-1}) >= 2


_check_cover()
