"""The NumPy twin of the batched shooting driver (tests/spg_twin.py) is itself right: on the CPU oracle's nlpObjective it
reaches the optimum SLSQP finds, keeps the invariants of the iteration in every case of the table, and every case of the
table shows what it was made for among its decisive instances.  No GPU."""
import numpy as np
import pytest

from tests import spg_twin as T


@pytest.fixture(scope="module")
def runs(oracle):
    """every case of the table once on oracle evaluations (shared, read-only)"""
    out = {}
    for name in T.CASES:
        c = T.make_inputs(name)
        ev, v0, Lb, Ub = T.oracle_setup(oracle, c)
        out[name] = (c, T.spg_twin(ev, v0, Lb, Ub, MaxIter=c.K, **c.opts), v0, Lb, Ub)
    return out


def test_twin_reaches_the_slsqp_optimum(oracle):
    """TestOCProblem, N = 100, 11 PWLinear points, three instances with different c and x0: J within 2e-6 and v within 5e-3
    of SLSQP on the same oracle objective (the tolerances of test_single_shooting_batch_on_device)."""
    from scipy.optimize import minimize
    c = T.make_inputs("blocks257", N=100, T=10.0, nB=11, batch=3, start=(0.7, 0.7), memory=10, seed=12)
    ev, v0, Lb, Ub = T.oracle_setup(oracle, c)
    tw = T.spg_twin(ev, v0, Lb, Ub, TolX=1e-12, TolFun=1e-6, MaxIter=400, memory=10, maxBacktracks=25)
    assert tw.converged.all() and np.all(tw.iterations < 400)
    go = oracle.RK4Integrator(oracle.linspace(0, c.T, c.N + 1))
    co = oracle.PWLinearControl(go.t, c.nB, 1)
    for b in range(3):
        po = oracle.TestOCProblem({"c": c.cs[b], "m": T.P["m"], "r": T.P["r"]}, T.BOUNDS)
        res = minimize(lambda v: oracle.nlp_objective(go, po, co, c.x0[:, b], v)[:2], v0[:, b], jac=True, method="SLSQP",
                       bounds=[(0.0, 1.0)] * c.nB, options={"ftol": 1e-12, "maxiter": 500})
        assert abs(tw.J[b] - res.fun) < 2e-6 * abs(res.fun)
        assert np.max(np.abs(tw.v[:, b] - res.x)) < 5e-3


@pytest.mark.parametrize("name", list(T.CASES))
def test_invariants(runs, name):
    """v inside [Lb, Ub], every accepted step satisfies its Armijo inequality, iterations <= MaxIter, a stopped instance
    does not move."""
    c, tw, v0, Lb, Ub = runs[name]
    T.check_invariants(c, tw, Lb, Ub)
    assert np.array_equal(tw.snap[0].v, v0) and tw.backtracks.shape == (len(tw.steps), c.batch)


@pytest.mark.parametrize("name", list(T.CASES))
def test_case_is_not_vacuous(runs, name):
    """at most 5 % of the batch is indecisive (margin < 1e-9) and the case's purpose occurs in the decisive part"""
    c, tw, v0, Lb, Ub = runs[name]
    dec = T.decisive_mask(tw)
    print(name, "indecisive", int(np.count_nonzero(~dec)), "of", c.batch, "smallest margin", float(tw.margin.min()))
    T.check_purpose(c, tw, dec, Lb, Ub)


def test_snapshots_are_the_shorter_runs(runs, oracle):
    """snap[k] of one run is what a run with MaxIter = k returns (the GPU test relies on it)"""
    c, tw, v0, Lb, Ub = runs["exhausted2"]
    ev = T.oracle_setup(oracle, c)[0]
    for k in (0, 1, 3):
        r = T.spg_twin(ev, v0, Lb, Ub, MaxIter=k, **c.opts)
        s = tw.snap[k]
        assert np.array_equal(r.v, s.v) and np.array_equal(r.J, s.J) and np.array_equal(r.iterations, s.iterations)
        assert np.array_equal(r.converged, s.converged) and np.array_equal(r.pgn, s.pgn) and np.array_equal(r.margin, s.margin)


def test_nan_trial_is_a_rejection():
    """a trial point whose objective is NaN is rejected and the instance recovers by halving (k_spg_accept: Jt <= ... is
    false for a NaN); an instance whose every trial is NaN stops where it is after maxBacktracks evaluations"""
    def ev(V):                       # 0.5 v^2: undefined near 0 (instance 0), anywhere but at the start (instance 1)
        J = 0.5 * np.sum(V * V, axis=0)
        J[0] = np.nan if abs(V[0, 0]) < 0.25 else J[0]
        J[1] = np.nan if V[0, 1] != 1.0 else J[1]
        return J, V.copy()
    tw = T.spg_twin(ev, np.ones((1, 3)), [-4.0], [4.0], TolX=1e-12, TolFun=1e-9, MaxIter=2, memory=2, maxBacktracks=4)
    st = tw.steps[0]                 # first step: alpha = 1 / pgn = 1, d = -1, trial point 0
    assert st.accepted.tolist() == [True, False, True] and st.failed.tolist() == [False, True, False]
    assert st.backtracks.tolist() == [1, 4, 0] and tw.snap[1].v[0].tolist() == [0.5, 1.0, 0.0]
    assert tw.v[0, 1] == 1.0 and tw.iterations[1] == 1 and not tw.active[1] and np.isfinite(tw.J).all()
