"""CPU checks of the NumPy twin of the batched bvp_solver (tests/bvp_twin.py) against scipy.integrate.solve_bvp: the
discretisation (Simpson / Lobatto-IIIa collocation on a fixed mesh, forward-difference Jacobian, Armijo damping, bvpinit's
constant guess) reaches the boundary-value solution of the optimality system on the reference's own script case, at fourth
order, and reports the instance that does not converge as such.  The GPU tests compare the device against this twin."""
import numpy as np
import pytest

from tests import bvp_twin as bt

BOUNDS = [[0.0, 1.0]]


def scipy_solution(prob, x0, T):
    """solve_bvp(tol = 1e-9) of y' = optSys(t, y), x(0) = x0, lam(T) = 0 from the constant guess (its own, adaptive mesh)."""
    from scipy.integrate import solve_bvp
    tm = np.linspace(0.0, T, 201)
    s = solve_bvp(lambda t, y: bt.optsys(prob, t, y), lambda a, b: np.array([a[0] - x0, b[1]]), tm,
                  np.vstack([np.full(tm.size, x0), np.zeros(tm.size)]), tol=1e-9, max_nodes=200000)
    assert s.status == 0, s.message
    return s.sol


@pytest.mark.parametrize("x0", [0.1, 0.2, 0.3, 0.45])
def test_twin_meets_solve_bvp_on_the_reference_script_case(oracle, x0):
    """tests/symbolic_test2.m (c 4, m .5, r 0, [0, 5]): the twin converges in a few iterations and agrees with solve_bvp.
    Bound: the twin's own refinement difference N = 200 against N = 400, measured here, x 4, + 1e-8 for SciPy's tolerance."""
    prob = oracle.TestOCProblem({"c": 4.0, "m": 0.5, "r": 0.0}, BOUNDS)
    ts, ts2 = oracle.linspace(0, 5, 201), oracle.linspace(0, 5, 401)
    r, r2 = bt.solve(prob, [x0], ts), bt.solve(prob, [x0], ts2)
    assert r["converged"] and r2["converged"] and r["iterations"] <= 6 and r["resnorm"] <= 1e-10
    refine = float(np.max(np.abs(r["y"] - r2["y"][:, ::2])))
    err = float(np.max(np.abs(scipy_solution(prob, x0, 5.0)(ts) - r["y"])))
    print(f"x0 {x0}: iterations {r['iterations']}, residual {r['resnorm']:.2e}, refinement {refine:.2e}, to solve_bvp {err:.2e}")
    assert err <= 4 * refine + 1e-8


@pytest.mark.parametrize("x0", [2.0, 2.5])
def test_twin_is_fourth_order_on_the_bl3_problem(oracle, test_problem_params, x0):
    """BL-3 (c 1.5, m 3, r .05, [0, 10]): the difference to solve_bvp falls by 5^4 = 625 from N = 40 to N = 200."""
    prob = oracle.TestOCProblem(test_problem_params, BOUNDS)
    sol = scipy_solution(prob, x0, 10.0)
    err = {}
    for N in (40, 200):
        ts = oracle.linspace(0, 10, N + 1)
        r = bt.solve(prob, [x0], ts)
        assert r["converged"] and r["iterations"] <= 8
        err[N] = float(np.max(np.abs(sol(ts) - r["y"])))
    print(f"x0 {x0}: to solve_bvp at N = 40 {err[40]:.3e}, at N = 200 {err[200]:.3e}, ratio {err[40] / err[200]:.0f}")
    assert 300 <= err[40] / err[200] <= 1200


def test_twin_reports_the_instance_that_does_not_converge(oracle, test_problem_params):
    """x0 = .5 on the BL-3 problem does not converge from the constant guess; the neighbour x0 = 2.2 does."""
    prob = oracle.TestOCProblem(test_problem_params, BOUNDS)
    ts = oracle.linspace(0, 10, 201)
    bad, good = bt.solve(prob, [0.5], ts), bt.solve(prob, [2.2], ts)
    assert not bad["converged"] and bad["resnorm"] > 1e-6 and bad["why"] in ("MaxIter", "line search")
    assert good["converged"] and good["resnorm"] <= 1e-10
