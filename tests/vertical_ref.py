"""The vertical terms of include/uampath.h (uam_vertical) restated in numpy: the definition
uam_eval_waypoints3d_v and uam_eval_generated3d_profiles_v (K4e+v / K4ew+v / K4p+v) are held to
bit for bit.

geometry() is the definition's loop over the segments j = 1 .. N+1, vectorised over the paths:
every product, sum, square root and division is one numpy operation on float64 arrays (numpy
never fuses two), np.fmax is C's fmax (a NaN row counts 0) and kin_row is the plain formula.
reference_eval_v() completes it to the full output set: the risk, no-fly, clearance and count
outputs and the voxel of every waypoint come from the oracle (profiles_ref.reference_eval; the
vertical terms do not touch them), the cost is (N+1) L plus the oracle-located voxels' risk / N
added in waypoint order, and the selections are oracle.argmin over the new cost and length."""
import dataclasses
import math

import numpy as np

import profiles_ref as R


@dataclasses.dataclass
class Vert:
    """uam_vertical without the ABI version."""
    z_scale: float
    sin_climb: float = math.inf
    sin_descent: float = math.inf


@dataclasses.dataclass
class Geo:
    """The fields of uam_params the geometry terms read."""
    length_smooth: bool = False
    maxratio_smooth: bool = False
    quirk_length: bool = True
    anchor: tuple = None      # None: the anchor is p_0 (anchor_mode 0)
    maxratio: float = 1.0
    maxalpha: float = 0.0


def geometry(wp3, geo, vert):
    """length_q (L), length, kin_sum and climb_sum [P] of wp3 [P, W, 3] = (x km, y km, z m)."""
    wp3 = np.ascontiguousarray(wp3, dtype=np.float64)
    P, W = wp3.shape[0], wp3.shape[1]
    N = W - 2
    x, y, z = wp3[:, :, 0], wp3[:, :, 1], wp3[:, :, 2]
    ls, ms, quirk = bool(geo.length_smooth), bool(geo.maxratio_smooth), bool(geo.quirk_length)
    kappa = np.float64(vert.z_scale)
    sc, sd = np.float64(vert.sin_climb), np.float64(vert.sin_descent)
    r = np.float64(geo.maxratio)
    if ms:
        r = r * r
    mincos = np.float64(math.cos(geo.maxalpha))      # libm's cos, as the library's host side
    zero = np.zeros(P)
    L, length, kin, climb = zero.copy(), zero.copy(), zero.copy(), zero.copy()
    with np.errstate(all="ignore"):
        if quirk:   # the anchor term: x/y only, the anchor flies at p_0's altitude
            ax = x[:, 0] if geo.anchor is None else np.float64(geo.anchor[0])
            ay = y[:, 0] if geo.anchor is None else np.float64(geo.anchor[1])
            dx, dy = x[:, 0] - ax, y[:, 0] - ay
            s = (zero + dx * dx) + dy * dy
            n = np.sqrt(s)
            L = L + (n * n if ls else n)
        pdx = pdy = pdz = pn = None
        for j in range(1, N + 2):
            dx = x[:, j] - x[:, j - 1]
            dy = y[:, j] - y[:, j - 1]
            dz = (z[:, j] - z[:, j - 1]) * kappa          # difference first, one product
            s = ((zero + dx * dx) + dy * dy) + dz * dz
            n = np.sqrt(s)
            length = length + n
            if not quirk or j <= N:
                L = L + (n * n if ls else n)
            nk = n * n if ms else n
            if j >= 2:
                dt = ((zero + pdx * dx) + pdy * dy) + pdz * dz
                c1 = np.fmax(0.0, nk - r * pn)
                c2 = np.fmax(0.0, pn / r - nk)
                c3 = np.fmax(0.0, mincos - dt / (pn * nk))
                kin = kin + c1
                kin = kin + c2
                kin = kin + c3
            cu = np.fmax(0.0, dz - sc * n)
            cd = np.fmax(0.0, (-dz) - sd * n)
            climb = (climb + cu) + cd
            pdx, pdy, pdz, pn = dx, dy, dz, nk
    return {"length_q": L, "length": length, "kin_sum": kin, "climb_sum": climb}


def cost_of(L, cells, vox, N):
    """(N+1) L + the risk / N of the waypoints inside the volume, added in waypoint order.
    cells [P, W]: the voxel index per waypoint, -1 outside (the oracle's)."""
    risk = np.ascontiguousarray(vox).view(np.float32).reshape(-1, 2)[:, 0].astype(np.float64)
    cost = np.float64(N + 1) * L
    dN = np.float64(N)
    with np.errstate(all="ignore"):
        for j in range(cells.shape[1]):
            c = cells[:, j]
            inside = c >= 0
            term = risk[np.where(inside, c, 0)] / dN
            cost = np.where(inside, cost + term, cost)
    return cost


def reference_eval_v(oracle_mod, orc, vox, cols, wp3, geo, vert, n_pairs=None, G=None,
                     base=None):
    """The full output set under the product's names (profiles_ref.reference_eval's, plus
    climb_sum), the selections over groups of G consecutive paths when n_pairs is given.
    base: profiles_ref.reference_eval(..., wp3) computed earlier (it does not depend on geo or
    vert), to share it among several evaluations of the same waypoints."""
    wp3 = np.ascontiguousarray(wp3, dtype=np.float64)
    out = dict(R.reference_eval(oracle_mod, orc, vox, cols, wp3) if base is None else base)
    out.update(geometry(wp3, geo, vert))
    out["cost"] = cost_of(out["length_q"], out["cells"], vox, wp3.shape[1] - 2)
    if n_pairs is not None:
        with np.errstate(invalid="ignore"):
            out["best_fval_idx"] = oracle_mod.argmin(out["cost"], G, True)
        out["best_length_idx"] = oracle_mod.argmin(out["length"], G, False)
    return out
