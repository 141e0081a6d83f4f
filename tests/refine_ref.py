"""An independent statement of what the refinement (orc_refine / k_refine) minimises, and a probe
that reads the optimiser's own gradient back through the public entry point (test
infrastructure).

The augmented Lagrangian is rebuilt from the golden-pinned evaluation -- cost and the
constraint rows g of Oracle.eval_paths / Engine.eval_waypoints(want_g=True), 3N kinematic rows
then S*W no-fly rows -- by other code than refine_L uses:

    L(z; y, c) = cost(z) + (c/2) * sum_i (g_i(z) + y_i/c)^2

Its gradient comes from central differences (Richardson over h and 2h).  The optimiser's
gradient is read from one steepest-descent step of exactly known length (probe_params): the
first trial step is a = min(2 alpha0, max_step/|g|) = 2 alpha0, the negative Armijo constant
accepts it, so g = (z_in - z_out) / (2 alpha0) up to the rounding of z.  With n_outer = 2 the
second step is taken at z1 (the n_outer = 1 result) with y = c0 g(z1) and, the first penalty
update comparing against prev = inf, c = c0 still; its trial step is 2 * (2 alpha0)."""
import math

import numpy as np

EPS = float(np.finfo(np.float64).eps)
MAX_ELEMS = 1 << 25          # constraint-row entries per eval_fn call (256 MiB of float64)
ALPHA0_MAX = 2.0 ** -11      # a vanishing gradient: any step is small
KINK = 1e-3                  # |fd(h) - fd(2h)| above this share of the path scale: a kink


def jitter(wp, seed, share=0.3):
    """Every second path with its interior waypoints moved by up to `share` of its segment
    length.  The arc candidates are evenly spaced, so their segment-ratio rows (c1, c2) are
    never active and their derivatives would go unchecked."""
    wp = np.array(wp, dtype=np.float64, copy=True)
    rng = np.random.default_rng(seed)
    seg = np.linalg.norm(wp[:, 1] - wp[:, 0], axis=-1)
    d = rng.uniform(-share, share, size=wp[:, 1:-1].shape) * seg[:, None, None]
    d[::2] = 0.0
    wp[:, 1:-1] += d
    return wp


def oracle_eval(orc):
    def fn(z):
        o = orc.eval_paths(z, want_g=True)
        return o["cost"], o["g"]
    return fn


def engine_eval(eng):
    """cost and rows stay on the device; aug_lagrangian sums them there."""
    def fn(z):
        o = eng.eval_waypoints(z, want_g=True)
        return o["cost"], o["g_rows"]
    return fn


def _host(a):
    return a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)


def rows_of(eval_fn, z):
    """g[P, rows] of z as a host array."""
    return _host(eval_fn(np.ascontiguousarray(z))[1]).copy()


def aug_lagrangian(eval_fn, z, y, c, index=None):
    """L per path of z [P, W, 2] under multipliers y [., rows] and penalty c.  index[P]: the row
    of y each path uses (default: its own).  Evaluated in chunks of at most MAX_ELEMS rows."""
    z = np.ascontiguousarray(z, dtype=np.float64)
    y = np.asarray(y, dtype=np.float64)
    P = z.shape[0]
    idx = np.arange(P) if index is None else np.asarray(index)
    step = max(1, MAX_ELEMS // max(1, y.shape[1]))
    out = np.zeros(P)
    for a in range(0, P, step):
        cost, g = eval_fn(z[a:a + step])
        yc = y[idx[a:a + step]] / c
        if hasattr(g, "new_tensor"):
            yc = g.new_tensor(yc)
        t = g + yc
        out[a:a + step] = _host(cost + (0.5 * c) * (t * t).sum(-1))
    return out


def lagrangian_diff(eval_fn, za, zb, y, c, index=None):
    """L(za) - L(zb) per path, formed row by row: cost_a - cost_b + (c/2) sum_i (ta_i - tb_i)
    (ta_i + tb_i) with t = g + y/c.  A row that za and zb share (the no-fly rows of a fixed
    endpoint inside a polygon reach 1e13 and more) cancels exactly and never enters the sum,
    which the difference of two rounded L would lose everything else to."""
    za = np.ascontiguousarray(za, dtype=np.float64)
    zb = np.ascontiguousarray(zb, dtype=np.float64)
    y = np.asarray(y, dtype=np.float64)
    P = za.shape[0]
    idx = np.arange(P) if index is None else np.asarray(index)
    step = max(1, MAX_ELEMS // (2 * max(1, y.shape[1])))
    out = np.zeros(P)
    for a in range(0, P, step):
        ca, ga = eval_fn(za[a:a + step])
        cb, gb = eval_fn(zb[a:a + step])
        yc = y[idx[a:a + step]] / c
        if hasattr(ga, "new_tensor"):
            yc = ga.new_tensor(yc)
        rows = ((ga - gb) * (ga + gb + 2.0 * yc)).sum(-1)
        out[a:a + step] = _host((ca - cb) + (0.5 * c) * rows)
    return out


def fd_gradient(eval_fn, z, y, c, h=1e-5):
    """Central differences of L over every interior coordinate, all perturbed copies of all
    paths in one batch (the differences by lagrangian_diff).  Returns (richardson [P, W, 2],
    selferr [P, W, 2]): (4 fd(h) - fd(2h))/3 and |fd(h) - fd(2h)|, the reference's own error
    estimate.  Endpoint entries are 0.  The
    quotient divides by the step that was actually taken, (z + h) - (z - h) as rounded."""
    z = np.ascontiguousarray(z, dtype=np.float64)
    P, W, _ = z.shape
    N = W - 2
    # copies [P, step, coordinate, sign, W, 2]
    zz = np.broadcast_to(z[:, None, None, None], (P, 2, 2 * N, 2, W, 2)).copy()
    k = np.arange(2 * N)
    for s, hs in enumerate((h, 2.0 * h)):
        for sg, d in enumerate((hs, -hs)):
            zz[:, s, k, sg, 1 + k // 2, k % 2] += d
    taken = zz[:, :, k, 0, 1 + k // 2, k % 2] - zz[:, :, k, 1, 1 + k // 2, k % 2]
    index = np.repeat(np.arange(P), 8 * N)
    index = index[::2]
    dL = lagrangian_diff(eval_fn, zz[:, :, :, 0].reshape(-1, W, 2),
                         zz[:, :, :, 1].reshape(-1, W, 2), y, c, index).reshape(P, 2, 2 * N)
    fd = dL / taken                                         # [P, step, 2N]
    rich = np.zeros((P, W, 2))
    selferr = np.zeros((P, W, 2))
    rich[:, 1:-1] = ((4.0 * fd[:, 0] - fd[:, 1]) / 3.0).reshape(P, N, 2)
    selferr[:, 1:-1] = np.abs(fd[:, 0] - fd[:, 1]).reshape(P, N, 2)
    return rich, selferr


def probe_params(alpha0, n_outer=1, c0=10.0):
    """Settings under which refinement takes n_outer steepest-descent steps of known length."""
    if not (alpha0 > 0.0 and math.frexp(alpha0)[0] == 0.5):
        raise ValueError(f"alpha0 = {alpha0} must be a power of two")
    return dict(n_outer=int(n_outer), n_inner=1, memory=0, max_backtrack=1, armijo=-1e30,
                max_step=1e30, inner_tol=0.0, delta=0.0, alpha0=float(alpha0), c0=float(c0),
                n_restart=0)


def pick_alpha0(gmax_ref):
    """The power of two with 2 alpha0 gmax_ref in [2^-21, 2^-20): no waypoint moves by more
    than ~1e-6, whatever the gradient's magnitude (1e1 .. 4e21 on the polygon maps)."""
    if not gmax_ref > 0.0:
        return ALPHA0_MAX
    return min(ALPHA0_MAX, 2.0 ** (-21 - math.frexp(float(gmax_ref))[1]))


def probe_gradient(refine_fn, z, alpha0, c0=10.0, second=False):
    """The optimiser's gradient at z (second: at z1 = the n_outer = 1 result, under y = c0
    g(z1)), read back per bucket of paths with the same alpha0.  refine_fn(wp, params) ->
    {"wp", "iters"} as host arrays.  Returns (grad [P, W, 2], z1 or z, steps [P], ok [P]);
    ok marks the paths that took the step the formula assumes (one per outer iteration)."""
    z = np.ascontiguousarray(z, dtype=np.float64)
    alpha0 = np.asarray(alpha0, dtype=np.float64)
    grad = np.zeros_like(z)
    at = z.copy()
    ok = np.zeros(z.shape[0], bool)
    for a in np.unique(alpha0):
        sel = np.nonzero(alpha0 == a)[0]
        one = refine_fn(z[sel], probe_params(float(a), 1, c0))
        if not second:
            grad[sel] = (z[sel] - one["wp"]) / (2.0 * a)
            ok[sel] = one["iters"] == 1
            continue
        two = refine_fn(z[sel], probe_params(float(a), 2, c0))
        at[sel] = one["wp"]
        grad[sel] = (one["wp"] - two["wp"]) / (4.0 * a)
        ok[sel] = two["iters"] == 2
    return grad, at, (4.0 if second else 2.0) * alpha0, ok


def grad_check(probe, rich, selferr, z, steps, cost, h=1e-5):
    """Per path: error = max |probe - richardson| over the coordinates where the reference is
    differentiable; allowance = 10 max selferr (the factor covers the difference of two
    roundings of L) + the read-back rounding eps max|z| / step + the rounding of the cost in
    the difference quotient, eps |cost| / h (what is left of a gradient that is exactly zero).
    Returns (ratio [P], relerr [P], excluded share).  A coordinate is excluded only where
    fd(h) and fd(2h) disagree by more than KINK of the path's largest component."""
    P = z.shape[0]
    scale = np.abs(rich).reshape(P, -1).max(axis=1)
    bad = selferr > KINK * scale[:, None, None]
    bad[:, 0] = bad[:, -1] = False
    n_coord = max(1, 2 * (z.shape[1] - 2) * P)
    err = np.where(bad, 0.0, np.abs(probe - rich)).reshape(P, -1).max(axis=1)
    own = np.where(bad, 0.0, selferr).reshape(P, -1).max(axis=1)
    allow = (10.0 * own + EPS * np.abs(z).reshape(P, -1).max(axis=1) / steps
             + EPS * np.abs(cost) / h)
    with np.errstate(divide="ignore", invalid="ignore"):
        rel = np.where(scale > 0.0, err / scale, 0.0)
    return err / allow, rel, bad.sum() / n_coord


def check_gradients(refine_fn, eval_fn, z, c0=10.0, h=1e-5, second=True):
    """The whole probe-against-reference comparison of a batch z: at y = 0 and (second) at
    z1 under y = c0 g(z1).  Returns one dict of per-path figures per step; the caller asserts
    on them.  alpha0 comes from the reference's gradient at z, per path."""
    z = np.ascontiguousarray(z, dtype=np.float64)
    P = z.shape[0]
    y = np.zeros_like(rows_of(eval_fn, z))
    rich, selferr = fd_gradient(eval_fn, z, y, c0, h)
    alpha0 = np.array([pick_alpha0(np.abs(rich[p]).max()) for p in range(P)])
    out = []
    for sec in ((False, True) if second else (False,)):
        probe, at, steps, ok = probe_gradient(refine_fn, z, alpha0, c0, sec)
        if sec:
            y = c0 * rows_of(eval_fn, at)
            rich, selferr = fd_gradient(eval_fn, at, y, c0, h)
        cost = _host(eval_fn(at)[0])
        ratio, rel, excluded = grad_check(probe, rich, selferr, at, steps, cost, h)
        out.append({"ratio": ratio, "rel": rel, "excluded": excluded, "ok": ok,
                    "alpha0": alpha0, "probe": probe, "ref": rich, "at": at,
                    "moved": float(np.abs(at - z).max()),
                    "gmax": np.abs(rich).reshape(P, -1).max(axis=1)})
    return out


def assert_gradients(refine_fn, eval_fn, wp, need_second=True):
    """check_gradients with its assertions: error < allowance on every path (under y != 0: on
    every path that took the second step), at most 1% of the coordinates excluded as kinks, no
    probe step above 1e-3.  Prints the measured figures and returns the largest ratio."""
    worst = 0.0
    for step, r in enumerate(check_gradients(refine_fn, eval_fn, wp)):
        use = r["ok"] if step else np.ones(len(wp), bool)
        assert r["excluded"] <= 0.01, r["excluded"]
        assert r["moved"] <= 1e-3
        ratio = r["ratio"][use]
        print(f"step {step}: {use.sum()}/{len(wp)} paths, gmax {r['gmax'].min():.3g}.."
              f"{r['gmax'].max():.3g}, error/gmax {r['rel'][use].max(initial=0):.3g}, "
              f"error/allowance {ratio.max(initial=0):.3g}, excluded {r['excluded']:.3g}")
        assert (ratio < 1.0).all(), (step, r["ratio"], r["rel"], use)
        worst = max(worst, float(ratio.max(initial=0.0)))
        if step and need_second:
            assert use.any()                # some path took the step under y != 0
    return worst


def check_contract(out, eval_fn, rp):
    """The reported numbers are those of the returned path (n_outer >= 1): infeas = sum g^2 and
    cost = cost of eval_fn(out["wp"]), both to rtol 1e-12 (they differ by summation order
    only), and iters within the step budget.  out: host arrays; rp: the refine settings."""
    cost, g = eval_fn(np.ascontiguousarray(out["wp"]))
    cost, g = _host(cost), _host(g)
    np.testing.assert_allclose(out["infeas"], (g * g).sum(axis=1), rtol=1e-12, atol=0.0)
    np.testing.assert_allclose(out["cost"], cost, rtol=1e-12, atol=0.0)
    budget = rp["n_outer"] * rp["n_inner"] * (1 + rp.get("n_restart", 0))
    assert (out["iters"] >= 0).all() and (out["iters"] <= budget).all(), (out["iters"], budget)


def check_descent(z_in, z_out, eval_fn, c0=10.0):
    """n_outer = 1 (y = 0 and c = c0 throughout): the independent L does not go up."""
    y = np.zeros_like(rows_of(eval_fn, z_in))
    change = lagrangian_diff(eval_fn, z_out, z_in, y, c0)
    assert (change <= 0.0).all(), change
    return change
