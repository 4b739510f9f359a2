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


# ---- the cases of tests/test_gpu_bvp_iteration.py can tell a right Newton step from a wrong one ----
from tests import bvp_cases as bc


def test_trace_and_step_noise_are_what_they_say(oracle, test_problem_params):
    """solve(trace=True) lists the iterates of the same solve; without it the dict is as before; one step of a solve from
    y_{k-1} gives y_k bit for bit; step_noise is small against the step and not zero on a generic iterate."""
    prob, ts = oracle.TestOCProblem(test_problem_params, BOUNDS), bc.NONUNIFORM
    plain, tr = bt.solve(prob, [2.0], ts), bt.solve(prob, [2.0], ts, trace=True)
    assert set(plain) == {"iterations", "converged", "why", "y", "resnorm"} and set(tr) == set(plain) | {"trace", "start"}
    assert np.array_equal(plain["y"], tr["y"]) and len(tr["trace"]) == tr["iterations"] == plain["iterations"] == 6
    assert np.array_equal(tr["trace"][-1]["y"], tr["y"]) and tr["trace"][-1]["resinf"] == tr["resnorm"]
    assert np.array_equal(tr["start"]["y"], bt.constant_guess(prob, [2.0], ts)) and tr["start"]["alpha"] is None
    prev = tr["start"]["y"]
    for s in tr["trace"]:
        one = bt.solve(prob, [2.0], ts, y0=prev, MaxIter=1, trace=True)
        assert np.array_equal(one["y"], s["y"]) and one["trace"][0]["alpha"] == s["alpha"]
        r = bt.residual(prob, [2.0], ts, s["y"])
        assert s["resinf"] == np.max(np.abs(r)) and s["res2"] == float(np.sqrt(np.sum(r * r)))
        prev = s["y"]
    noise = bt.step_noise(prob, [2.0], ts, tr["trace"][0]["y"])
    assert 0 < noise < 1e-6 * np.max(np.abs(tr["trace"][1]["y"] - tr["trace"][0]["y"]))


def test_step_cases_tell_a_wrong_jacobian_from_the_right_one(oracle):
    """For every case of the device's one-step test: (a) three wrong Newton matrices a kernel bug could produce -- the sign
    of the h/8 term of dy_m/dy flipped, that term dropped, the right node's Jacobian taken one interval stale -- move the
    first iterate by at least 100 x the bound the device is held to there (all three converge to the same root: the end of
    a solve does not see them); (b) no iterate's ||Phi||_inf lies within a factor 30 of NewtonTol, so the iteration count is
    not decided by rounding; (c) step_noise <= 1e-6 x the size of every step taken: none starts on a kink of ControlChar's
    clamp, where a last-bit change would move the step itself."""

    def mutant(kind):
        sign = {"flipped": -1.0, "dropped": 0.0, "stale": 1.0}[kind]

        def jacobian(prob, x0, tspan, y):
            nS = prob.nS
            nY = 2 * nS
            tn, tm, h = bt.grid(tspan)
            _, f, ym, fm = bt.residual(prob, x0, tspan, y, parts=True)
            Jn, Jm = bt.fd_jacobian(prob, tn, y, f), bt.fd_jacobian(prob, tm, ym, fm)
            n = nY * (h.size + 1)
            D, I = np.zeros((n, n)), np.eye(nY)
            D[:nS, :nS] = np.eye(nS)
            for i in range(h.size):
                Jl, Jr, Jc = Jn[:, :, i], Jn[:, :, i if kind == "stale" else i + 1], Jm[:, :, i]
                r0 = nS + nY * i
                D[r0:r0 + nY, nY * i:nY * (i + 1)] = -I - h[i] / 6 * (Jl + 4 * Jc @ (0.5 * I + sign * h[i] / 8 * Jl))
                D[r0:r0 + nY, nY * (i + 1):nY * (i + 2)] = I - h[i] / 6 * (Jr + 4 * Jc @ (0.5 * I - sign * h[i] / 8 * Jr))
            D[n - nS:, n - nS:] = np.eye(nS)
            return D
        return jacobian

    mutants = {kind: mutant(kind) for kind in ("flipped", "dropped", "stale")}
    worst = {}
    for case in bc.STEP_CASES:
        tw, prob = case.solve(oracle), case.problem(oracle)
        assert tw["converged"], case.name
        assert bc.eligible_for_counts(tw["trace"]), (case.name, [s["resinf"] for s in tw["trace"]])          # (b)
        recs = case.step_records(oracle)
        for rec in recs:                                                                                     # (c)
            size = float(np.max(np.abs(rec["y"] - rec["from"])))
            assert rec["alpha"] > 0 and rec["noise"] <= 1e-6 * size, (case.name, rec["k"], rec["noise"], size)
            assert rec["noise"] >= 1e-10 * size, (case.name, rec["k"], rec["noise"], size)   # (no degenerate sample, see wavy_guess)
        first = recs[0]
        bound = bc.step_bound(first["noise"], first["y"])
        for kind, jac in mutants.items():                                                                    # (a)
            ym = bt.solve(prob, case.x0, case.tspan, y0=first["from"], MaxIter=1, jacobian=jac)["y"]
            ratio = float(np.max(np.abs(ym - first["y"]) / bound))
            worst[case.family] = min(worst.get(case.family, np.inf), ratio)
            assert ratio >= 100, (case.name, kind, ratio)
    print("smallest mutant gap / one-step bound per family:", {k: f"{v:.1e}" for k, v in worst.items()})
    for kind, jac in mutants.items():   # ... and the end of a solve does not notice them
        case = bc.FULL[0]
        a, b = case.solve(oracle), bt.solve(case.problem(oracle), case.x0, case.tspan, jacobian=jac)
        assert b["converged"] and np.max(np.abs(a["y"] - b["y"])) < 1e-9 and b["iterations"] > a["iterations"], kind


def test_count_cases_and_damped_instances(oracle):
    """The whole solves whose iteration counts the device must reproduce are eligible (no ||Phi||_inf near NewtonTol), under
    every maxBacktracks the GPU test runs; the damped instances take the step lengths written down in bvp_cases: one with
    1/2 or 1/4 only (first stage of the device's line search), two with 1/8 or less (second stage)."""
    for case in bc.COUNT_CASES:
        tw = case.solve(oracle)
        assert tw["converged"] and bc.eligible_for_counts(tw["trace"]), case.name
    for case in bc.DAMPED:
        alphas = [s["alpha"] for s in case.solve(oracle)["trace"]]
        assert alphas == bc.DAMPED_ALPHAS[case.x0[0]], (case.name, alphas)
    first = [a for a in bc.DAMPED_ALPHAS.values() if 0.25 <= min(a) < 1.0]
    second = [a for a in bc.DAMPED_ALPHAS.values() if min(a) <= 0.125]
    assert first and second
    for mb in (0, 2, 3, 12):
        for case in bc.DAMPED + bc.FULL + [bc.NOT_CONVERGING]:
            tw = case.solve(oracle, maxBacktracks=mb)
            assert bc.eligible_for_counts(tw["trace"]), (case.name, mb)
            print(f"maxBacktracks {mb}, x0 {case.x0}: {tw['why']} after {tw['iterations']}, alpha {[s['alpha'] for s in tw['trace']][:8]}")
    so = bc.SYMBOLIC_TEST2
    prob, ts = oracle.TestOCProblem(so["par"], BOUNDS), oracle.linspace(0, so["T"], so["N"] + 1)
    for x0 in so["x0"]:
        tw = bt.solve(prob, [x0], ts, trace=True)
        assert tw["converged"] and bc.eligible_for_counts(tw["trace"]), (x0, [s["resinf"] for s in tw["trace"]])
