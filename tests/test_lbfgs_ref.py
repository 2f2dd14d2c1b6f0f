"""The numpy two-loop L-BFGS of tests/lbfgs_ref.py, the reference of the device minimiser (test_optimize_edges_gpu.py), on the
CPU: what rounding alone does to its trajectories - which sizes the tolerance of the device comparison -, and that the test
problem makes the run meet every rule of the driver."""
import numpy as np
import pytest

import lbfgs_ref
import opt_shapes


@pytest.mark.parametrize("bounded", [True, False], ids=["bounded", "unbounded"])
@pytest.mark.parametrize("nx", sorted(opt_shapes.MINIMISER_SHAPES))
def test_spread_of_the_reference_under_reordering_and_precision(nx, bounded):
    """float64, float64 with all sums in a shuffled sequential order, np.longdouble: the largest relative spread of J and |q|
    per iteration and of the final x stays within lbfgs_ref.SPREAD[nx], and 1 000 x that is still below 1e-9."""
    model, scenes, x0, lo, hi, tight = opt_shapes.minimiser_problem(nx)
    make = lbfgs_ref.cosh_problem(x0, seed=nx, tight=tight)
    runs, spread = lbfgs_ref.run_three_ways(make, x0, lo if bounded else None, hi if bounded else None, max_iterations=12)
    print(nx, bounded, "spread", spread, [(r["kept"], r["halvings"], r["first_trial"]) for r in runs])
    assert spread <= lbfgs_ref.SPREAD[nx] and 1000.0 * lbfgs_ref.SPREAD[nx] <= 1.0e-9
    for r in runs:
        # the ring of six pairs wraps, steps are accepted at the first trial, and (bounded) the clamp makes the first step fail
        # Armijo's test until it is halved many times, with a pair too flat to keep: 11 of 12
        assert r["status"] == 2 and r["iterations"] == 12 and r["kept"] >= 7 and r["first_trial"] >= 1
        assert (r["halvings"], r["kept"], r["first_trial"]) == (runs[0]["halvings"], runs[0]["kept"], runs[0]["first_trial"])
        if bounded:
            assert r["halvings"] >= 1 and r["kept"] == 11
            x = np.asarray(r["x"], dtype=np.float64)
            free = x0 > lbfgs_ref.MIN_X
            assert np.all(x[free] >= lo[free]) and np.all(x[free] <= hi[free]) and (x[free] == hi[free]).sum() > 16
        assert np.array_equal(np.asarray(r["x"], dtype=np.float64)[x0 <= lbfgs_ref.MIN_X], x0[x0 <= lbfgs_ref.MIN_X])
    assert runs[0]["history"][-1][1] < runs[0]["history"][0][1]


def test_reference_minimises_a_quadratic():
    """on a convex quadratic with exact curvature pairs the two-loop recursion converges to the known minimum"""
    rs = np.random.RandomState(0)
    n = 40
    A = rs.normal(size=(n, n))
    A = A @ A.T / n + np.eye(n)
    b = rs.normal(size=n)
    f = lambda x: (0.5 * x @ A @ x - b @ x, A @ x - b)
    r = lbfgs_ref.minimize(f, np.zeros(n), max_iterations=200, convergence_criterion=1e-7)
    assert r["status"] == 0 and np.allclose(r["x"], np.linalg.solve(A, b), atol=1e-6)
    # and with bounds the solution is the projected one: the projected gradient vanishes, no bound is violated
    lo, hi = np.full(n, -0.05), np.full(n, 0.05)
    r = lbfgs_ref.minimize(f, np.zeros(n), lo, hi, max_iterations=200, convergence_criterion=1e-7)
    g = A @ r["x"] - b
    assert np.all(r["x"] >= lo) and np.all(r["x"] <= hi)
    inside = (r["x"] > lo) & (r["x"] < hi)
    assert r["status"] == 0 and np.all(g[r["x"] == lo] >= 0) and np.all(g[r["x"] == hi] <= 0) and np.abs(g[inside]).max() < 1e-6
