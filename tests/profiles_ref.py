"""Shared inputs and references of test_profiles_cpu.py / test_gpu_profiles.py: the hand-written
volume, the pairs, the numpy restatement of the altitude-profile rule (include/uampath.h) and
the oracle evaluation of a pairs x arcs x profiles batch."""
import numpy as np

# 100 x 76 columns x 7 layers: ragged against every block size (4 x 8, 4 x 2, 4 x 4, 8 x 8
# columns; 64 lanes; the last altitude band partial)
NX, NY, NZ = 100, 76, 7
X0, Y_TOP, DX, DY, Z0, DZ = 0.0, 20.0, 0.6, 0.75, 0.0, 640.0 / 7
Z_TOP = Z0 + NZ * DZ


def hand_volume(seed=5):
    """vox [NY, NX, NZ, 2] {risk, psi_nfz} and cols [NY, NX, 2] {terrain, flags} as uint32
    words.  Risk and psi in one moderate sign-mixed range (some exact +-0), a finite random
    terrain in -50 .. 900 m (so below-terrain occurs), some no-fly flags."""
    rng = np.random.default_rng(seed)
    risk = rng.uniform(-4.0, 4.0, (NY, NX, NZ)).astype(np.float32)
    psi = rng.uniform(-4.0, 4.0, (NY, NX, NZ)).astype(np.float32)
    zero = rng.random((NY, NX, NZ))
    risk[zero < 0.05] = 0.0
    risk[(zero >= 0.05) & (zero < 0.08)] = -0.0
    psi[rng.random((NY, NX, NZ)) < 0.3] = 0.0
    ter = rng.uniform(-50.0, 900.0, (NY, NX)).astype(np.float32)
    ter[rng.random((NY, NX)) < 0.5] *= np.float32(0.2)   # half of the columns mostly flyable
    flags = (rng.random((NY, NX)) < 0.1).astype(np.uint32)   # UAM_FLAG_NFZ
    vox = np.stack([risk.view(np.uint32), psi.view(np.uint32)], -1)
    cols = np.stack([ter.view(np.uint32), flags], -1)
    return np.ascontiguousarray(vox), np.ascontiguousarray(cols)


def volume_desc(oracle_mod):
    return oracle_mod.volume_desc(NX, NY, NZ, X0, Y_TOP, DX, DY, Z0, DZ)


def host_volume(vox, cols):
    """The (voxels, columns) float32 views Oracle.eval_paths3d takes."""
    return vox.view(np.float32), cols.view(np.float32)


def pairs6(Q=130, seed=9):
    """Q >= 8 pairs (x0, y0, z0, xf, yf, zf) over the grid; the first eight hold the special
    ones, so every prefix of 8 or more keeps them."""
    rng = np.random.default_rng(seed)
    pr = np.stack([rng.uniform(1.0, 59.0, Q), rng.uniform(-36.0, 19.0, Q),
                   rng.uniform(100.0, 500.0, Q), rng.uniform(1.0, 59.0, Q),
                   rng.uniform(-36.0, 19.0, Q), rng.uniform(100.0, 500.0, Q)], 1)
    pr[1, 2] = -50.0            # starts below the volume
    pr[2, 5] = 900.0            # ends above it
    pr[3, 0] = 75.0             # starts east of the grid
    pr[4, 3:5] = pr[4, 0:2]     # start == goal
    pr[5, 1] = np.nan           # one NaN coordinate
    pr[6, 2], pr[6, 5] = 630.0, 20.0   # top layer down to the bottom one
    pr[7, 0], pr[7, 3] = 200.0, 230.0  # wholly east of the grid: no waypoint inside, +inf clearance
    return pr


def table_z(pr6, ztab):
    """z [Q, A, W] by the table rule as separate numpy operations: two products, their sum,
    then the sum with the third coefficient (numpy never fuses them)."""
    pr6 = np.asarray(pr6, np.float64).reshape(-1, 6)
    zt = np.asarray(ztab, np.float64)
    z0 = pr6[:, 2][:, None, None]
    zf = pr6[:, 5][:, None, None]
    p0 = z0 * zt[None, :, :, 0]
    p1 = zf * zt[None, :, :, 1]
    s = p0 + p1
    return s + zt[None, :, :, 2]


def reference_wp3(oracle_mod, pr6, ut, ztab):
    """wp3 [Q*D*A, W, 3], path (q*D + d)*A + a: x/y from oracle.gen_paths3d repeated over the
    A profiles, z from table_z."""
    pr6 = np.asarray(pr6, np.float64).reshape(-1, 6)
    ut = np.asarray(ut, np.float64)
    A, W = ztab.shape[0], ztab.shape[1]
    Q, D = pr6.shape[0], ut.shape[0]
    xy = oracle_mod.gen_paths3d(pr6, ut).reshape(Q, D, 1, W, 3)[..., :2]
    wp3 = np.empty((Q, D, A, W, 3))
    wp3[..., :2] = xy
    wp3[..., 2] = table_z(pr6, ztab)[:, None, :, :]
    return wp3.reshape(Q * D * A, W, 3)


def reference_eval(oracle_mod, orc, vox, cols, wp3, n_pairs=None, G=None):
    """Oracle.eval_paths3d under the product's output names, with the selections over groups
    of G consecutive paths when n_pairs is given."""
    r = orc.eval_paths3d(wp3, volume_desc(oracle_mod), host_volume(vox, cols), want_cells=True)
    out = {"cost": r["cost"], "length_q": r["lq"], "length": r["length"], "kin_sum": r["kin"],
           "nfz_sum": r["nfz"], "min_clearance": r["min_clearance"], "nfz_hits": r["nfz_hits"],
           "offmap": r["offmap"], "below_terrain": r["below"], "cells": r["cells"]}
    if n_pairs is not None:
        with np.errstate(invalid="ignore"):
            out["best_fval_idx"] = oracle_mod.argmin(r["cost"], G, True)
        out["best_length_idx"] = oracle_mod.argmin(r["length"], G, False)
    return out


def family(profiles_mod, N):
    """The 8-profile table of the tests: the straight climb, cruises at three altitudes inside
    the volume, a lift up and one down, a cruise above the volume's top and one below its
    floor."""
    P = profiles_mod
    return P.stack(P.linear(N), P.cruise(N, 150.0), P.cruise(N, 320.0), P.cruise(N, 600.0, 0.4),
                   P.lift(N, 200.0), P.lift(N, -120.0, 0.1), P.cruise(N, Z_TOP + 60.0),
                   P.cruise(N, Z0 - 40.0))
