"""A plain numpy L-BFGS in the TWO-LOOP form, the independent reference of ecckd_opt_minimize (csrc/optimize.hip), whose device
kernels use the compact matrix form of lbfgs_history.hpp.  Same rules as the driver, read from its code:
  m = 6 pairs; gamma = s.y / y.y of the newest pair (1 without pairs); a pair is kept only if s.y > 1e-12 (the ring makes room
  for it - drops the oldest of six - before that is known); q = the gradient projected to zero at active bounds and at pinned
  elements (x = -1e20); d = -H q, set to 0 where q = 0 and g != 0; slope d.g with the full gradient;
  first trial min(1, 1/|d|) while there is no pair, later 1, never longer than |step d| = 2; Armijo 1e-4 with halving, up to 30
  trials; the trial point is clamped to the bounds, pinned elements do not move; if the direction is no descent direction or the
  line search fails, the pairs are dropped once and the projected steepest descent is tried.
Every sum goes through `total`, so that the same iteration can be run with another summation order or in np.longdouble: the
spread between those runs is what rounding alone does to a trajectory, and sizes the tolerance of the device comparison."""
import numpy as np

M = 6
MIN_X = -1.0e20

# Largest relative spread of (J, |q|, x) between the float64, shuffled-sum and long-double runs of `minimize` on the problem of
# each state length (opt_shapes.minimiser_problem + cosh_problem, bounded and unbounded, 12 iterations), rounded up from what
# test_lbfgs_ref.py measures and holds against these: 3.2e-15, 4.2e-15, 1.6e-14, 1.7e-13.  The device test allows 1 000 x.
SPREAD = {1023: 1.0e-14, 1024: 1.0e-14, 1025: 3.0e-14, 327680: 3.0e-13}


def total_plain(v):
    return v.sum()


def total_permuted(seed=12345):
    cache = {}

    def total(v):
        if v.size not in cache:
            cache[v.size] = np.random.RandomState(seed).permutation(v.size)
        return np.cumsum(v[cache[v.size]])[-1]              # a strictly sequential sum in a shuffled order

    return total


def minimize(cost_grad, x0, lo=None, hi=None, max_iterations=12, convergence_criterion=0.0, total=total_plain, dtype=np.float64):
    """-> dict(x, status, history [(it, J, |q|)], kept (pairs kept), halvings, first_trial (iterations accepted at the first trial))"""
    dot = lambda a, b: total(a * b)
    x = np.asarray(x0, dtype=dtype).copy()
    bounded = lo is not None
    if bounded:
        lo, hi = np.asarray(lo, dtype=dtype), np.asarray(hi, dtype=dtype)
    free = x > MIN_X

    def project(x, g):
        q = g.copy()
        if bounded:
            q[((x <= lo) & (g > 0)) | ((x >= hi) & (g < 0))] = 0
        q[~free] = 0
        return q

    J, g = cost_grad(x)
    q = project(x, g)
    S, Y = [], []                                           # oldest first
    gamma = dtype(1.0)
    history, kept, halvings, first_trial = [], 0, 0, 0
    status, it = 2, 0
    for it in range(max_iterations + 1):
        gnorm = np.sqrt(dot(q, q))
        history.append((it, J, gnorm))
        if not gnorm == gnorm:
            status = 7
            break
        if gnorm <= convergence_criterion:
            status = 0
            break
        if it == max_iterations:
            status = 2
            break
        restarted, ok = False, False
        while True:
            r = q.copy()
            alpha = [None] * len(S)
            for i in range(len(S) - 1, -1, -1):
                alpha[i] = dot(S[i], r) / dot(S[i], Y[i])
                r = r - alpha[i] * Y[i]
            r = (gamma if S else dtype(1.0)) * r
            for i in range(len(S)):
                beta = dot(Y[i], r) / dot(S[i], Y[i])
                r = r + S[i] * (alpha[i] - beta)
            d = -r
            d[(q == 0) & (g != 0)] = 0
            dg, dn = dot(d, g), np.sqrt(dot(d, d))
            step = min(dtype(1.0), 1 / max(dn, dtype(1e-300))) if not S else dtype(1.0)
            if step * dn > 2:
                step = 2 / dn
            if not dg < 0:
                if restarted or not S:
                    status = 7 if dg != dg else 4
                    break
                restarted, S, Y = True, [], []
                continue

            def trial(step):
                xn = x + step * d
                if bounded:
                    xn = np.minimum(np.maximum(xn, lo), hi)
                xn[~free] = x[~free]
                return (xn,) + tuple(cost_grad(xn))

            xn, Jn, gn = trial(step)
            ok = Jn == Jn and Jn <= J + dtype(1.0e-4) * step * dg
            ntrial = 1
            while not ok and ntrial < 30:
                step = step * dtype(0.5)
                xn, Jn, gn = trial(step)
                ok = Jn == Jn and Jn <= J + dtype(1.0e-4) * step * dg
                ntrial += 1
            if ok:
                halvings += ntrial - 1
                first_trial += ntrial == 1
            if not ok and S and not restarted:
                restarted, S, Y = True, [], []
                continue
            if not ok:
                status = 3
            break
        if not ok:
            break
        if len(S) == M:
            S.pop(0)
            Y.pop(0)
        s, y = xn - x, gn - g
        sy = dot(s, y)
        if sy > 1.0e-12:
            S.append(s)
            Y.append(y)
            gamma = sy / dot(y, y)
            kept += 1
        x, g, J = xn, gn, Jn
        q = project(x, g)
    return dict(x=x, status=status, iterations=it, history=history, kept=kept, halvings=halvings, first_trial=first_trial)


# ---- the test problem: J = sum a_i (cosh(x_i - c_i) - 1) over the free elements -----------------------------------------

def cosh_problem(x0, seed, tight=(), nfar=600):
    """a in [0.5, 2]; c = x0 + offsets of three kinds, chosen so that 12 iterations see every rule of the driver at work and
    are not enough to converge (a converged |q| is a difference of rounded numbers and says little):
      * most elements: 3 / sqrt(n) N(0,1), close to their minimum;
      * `nfar` elements spread over the vector: +-1.5, beyond the bounds ecckd_opt_initial_state gives (+-ln 2 about x0): the
        capped steps take most of the run to bring them there, the bounded run then has to hold them;
      * the elements `tight` (their upper bound lies 5e-10 above x0, minimiser_problem of opt_shapes.py): +10.  They carry nearly
        all of the first gradient, the clamp lets them deliver nearly nothing of the decrease the slope promises, and the
        bounded line search has to halve its first step many times; the pair of that step has s.y < 1e-12 and is dropped;
        unbounded they stay far from their minimum.
    -> cost_grad factory (total, dtype) -> f(x) -> (J, g), g = 0 at pinned elements"""
    rs = np.random.RandomState(seed)
    n = len(x0)
    free = np.asarray(x0) > MIN_X
    a = rs.uniform(0.5, 2.0, size=n)
    off = 3.0 / np.sqrt(n) * rs.normal(size=n)
    idx = np.unique(np.linspace(1, n - 1, nfar).astype(int))
    off[idx] = 1.5 * np.where(np.arange(idx.size) % 2 == 0, 1.0, -1.0)
    off[list(tight)] = 10.0
    c = np.where(free, np.asarray(x0) + off, 0.0)

    def make(total=total_plain, dtype=np.float64):
        aa, cc = a.astype(dtype), c.astype(dtype)

        def cost_grad(x):
            u = np.where(free, np.asarray(x, dtype=dtype) - cc, 0)
            return total(aa * (np.cosh(u) - 1)), np.where(free, aa * np.sinh(u), 0).astype(dtype)

        return cost_grad

    return make


def run_three_ways(make, x0, lo, hi, max_iterations=12):
    """The reference in float64, in float64 with every sum in a shuffled sequential order, and in np.longdouble; -> the three
    results and the largest relative spread of J, |q| (per iteration) and x (relative to the largest |x| of a free element)."""
    runs = [minimize(make(total_plain, np.float64), x0, lo, hi, max_iterations, total=total_plain),
            minimize(make(total_permuted(), np.float64), x0, lo, hi, max_iterations, total=total_permuted()),
            minimize(make(total_plain, np.longdouble), x0, lo, hi, max_iterations, total=total_plain, dtype=np.longdouble)]
    return runs, max(difference(runs[0], r) for r in runs[1:])


def difference(a, b):
    """largest relative difference of two runs: J and |q| per iteration, x relative to the largest |x| of a free element"""
    if len(a["history"]) != len(b["history"]):
        return np.inf
    worst = 0.0
    for (i1, J1, q1), (i2, J2, q2) in zip(a["history"], b["history"]):
        if i1 != i2:
            return np.inf
        worst = max(worst, float(abs(J1 - J2) / abs(J1)), float(abs(q1 - q2) / abs(q1)))
    xa, xb = np.asarray(a["x"], dtype=np.float64), np.asarray(b["x"], dtype=np.float64)
    free = xa > MIN_X
    return max(worst, float(np.abs(xa[free] - xb[free]).max() / np.abs(xa[free]).max()))
