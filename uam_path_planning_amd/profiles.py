"""Altitude-profile tables for Engine.gen_paths3d / Engine.eval_generated3d_profiles.

A table is data, like the unit-arc table (arcs.py): ztab [A, N+2, 3] float64.  Waypoint j of a
pair (x0, y0, z0, xf, yf, zf) under profile a flies at

    z_j = (z0 * ztab[a, j, 0] + zf * ztab[a, j, 1]) + ztab[a, j, 2]

(include/uampath.h: two products, their sum, then the third coefficient, each rounded;
sin_of_angle() gives the climb limits of engine.Vertical from an angle).  The
helpers below build common rows with t_j = j / (N+1); their own rounding is not normative, any
[N+2, 3] array is a valid profile.  Rows 0 and N+1 are exactly (1, 0, 0) and (0, 1, 0), so a
path starts and ends at the pair's own altitudes, bit for bit.
"""
import numpy as np


def _t(N):
    N = int(N)
    if N < 1:
        raise ValueError(f"N = {N} must be >= 1")
    return np.arange(N + 2, dtype=np.float64) / np.float64(N + 1)


def _ramp(t, ramp):
    """w = min(1, t / ramp, (1 - t) / ramp): 0 at both ends, 1 over the cruise."""
    ramp = float(ramp)
    if not ramp > 0.0:
        raise ValueError(f"ramp = {ramp} must be > 0")
    return np.minimum(1.0, np.minimum(t / ramp, (1.0 - t) / ramp))


def _finish(tab):
    tab[0] = (1.0, 0.0, 0.0)
    tab[-1] = (0.0, 1.0, 0.0)
    return tab


def linear(N):
    """The straight climb between the end altitudes: (1 - t, t, 0)."""
    t = _t(N)
    return _finish(np.stack([1.0 - t, t, np.zeros_like(t)], axis=1))


def cruise(N, altitude_m, ramp=0.25):
    """Climb over the first `ramp` of the path to the absolute altitude altitude_m, cruise,
    descend over the last `ramp`: ((1 - w)(1 - t), (1 - w) t, w altitude_m)."""
    t = _t(N)
    w = _ramp(t, ramp)
    return _finish(np.stack([(1.0 - w) * (1.0 - t), (1.0 - w) * t, w * float(altitude_m)],
                            axis=1))


def lift(N, height_m, ramp=0.25):
    """The straight climb raised by height_m (lowered when negative) over its middle:
    (1 - t, t, w height_m)."""
    t = _t(N)
    w = _ramp(t, ramp)
    return _finish(np.stack([1.0 - t, t, w * float(height_m)], axis=1))


def sin_of_angle(degrees):
    """sin of a climb (or descent) angle in degrees, for Vertical.sin_climb / sin_descent: the
    largest altitude change per unit of 3-D path length, both in the length's unit (the
    altitude change scaled by Vertical.z_scale).  0 <= degrees <= 90; 90 gives 1, which no
    segment exceeds (use inf for "no limit")."""
    d = float(degrees)
    if not 0.0 <= d <= 90.0:
        raise ValueError(f"climb angle = {d} degrees must be in [0, 90]")
    return 1.0 if d == 90.0 else float(np.sin(np.deg2rad(d)))


def stack(*tables):
    """[A, N+2, 3] from A profiles of one N."""
    if not tables:
        raise ValueError("stack needs at least one profile")
    tabs = [np.asarray(t, dtype=np.float64) for t in tables]
    for t in tabs:
        if t.ndim != 2 or t.shape[1] != 3 or t.shape != tabs[0].shape:
            raise ValueError(f"profiles must share one shape [N+2, 3], got "
                             f"{[tuple(x.shape) for x in tabs]}")
    return np.ascontiguousarray(np.stack(tabs, axis=0))
