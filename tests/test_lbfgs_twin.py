"""The NumPy twin of the projected L-BFGS iteration (tests/lbfgs_twin.py) is itself right: on the CPU oracle's nlpObjective it
keeps the invariants of the iteration in every case of its table, every case shows what it was made for among its decisive
instances, it ends at SPG's KKT point, and on a long horizon it needs fewer batch evaluations than SPG.  No GPU."""
import numpy as np
import pytest

from tests import lbfgs_twin as L
from tests import spg_twin as T


@pytest.fixture(scope="module")
def runs(oracle):
    """every case of the table once on oracle evaluations (shared, read-only)"""
    out = {}
    for name in L.LCASES:
        c = L.make_case(name)
        ev, v0, Lb, Ub = T.oracle_setup(oracle, c)
        out[name] = (c, L.lbfgs_twin(ev, v0, Lb, Ub, MaxIter=c.K, pairs=c.pairs, **c.opts), v0, Lb, Ub)
    return out


@pytest.mark.parametrize("name", list(L.LCASES))
def test_invariants(runs, name):
    """v inside [Lb, Ub], every accepted step satisfies its Armijo inequality, J never increases, iterations <= MaxIter, a
    stopped instance does not move, every stored pair has s'y > 0."""
    c, tw, v0, Lb, Ub = runs[name]
    T.check_invariants(c, tw, Lb, Ub)
    L.check_lbfgs_invariants(tw)
    assert np.array_equal(tw.snap[0].v, v0) and tw.backtracks.shape == (len(tw.steps), c.batch)


@pytest.mark.parametrize("name", list(L.LCASES))
def test_case_is_not_vacuous(runs, name):
    """at most 5 % of the batch is indecisive (margin < 1e-9) and the case's purpose, (a) to (f), occurs in the decisive part"""
    c, tw, v0, Lb, Ub = runs[name]
    dec = T.decisive_mask(tw)
    print(name, "indecisive", int(np.count_nonzero(~dec)), "of", c.batch, {k: float(m.min()) for k, m in tw.margins.items()})
    L.check_case_purpose(c, tw, dec, Lb, Ub)


def test_snapshots_are_the_shorter_runs(runs, oracle):
    """snap[k] of one run is what a run with MaxIter = k returns (the GPU test relies on it)"""
    c, tw, v0, Lb, Ub = runs["fail257"]
    ev = T.oracle_setup(oracle, c)[0]
    for k in (0, 1, 4):
        r = L.lbfgs_twin(ev, v0, Lb, Ub, MaxIter=k, pairs=c.pairs, **c.opts)
        s = tw.snap[k]
        assert np.array_equal(r.v, s.v) and np.array_equal(r.J, s.J) and np.array_equal(r.iterations, s.iterations)
        assert np.array_equal(r.converged, s.converged) and np.array_equal(r.pgn, s.pgn) and np.array_equal(r.margin, s.margin)


def test_same_kkt_point_as_spg(oracle):
    """TestOCProblem, N = 60, T = 6, 15 PWLinear points, 12 instances with their own c and x0, bounds active for part of them,
    both twins run to TolFun = 1e-8: every instance of both converges, and they end at the same point.  The two methods stop
    at different points inside the same TolFun ball, so the difference is set by conditioning, not by round-off.
    Measured on the CPU oracle: J differs by 8.9e-16 relative to max(1, |J|), v by 8.4e-8 absolute (22 SPG and 19 L-BFGS
    iterations at the most); 10 x that is asserted."""
    c = T.make_inputs("blocks257", N=60, T=6.0, nB=15, batch=12, start=(0.3, 0.9), seed=7)
    ev, v0, Lb, Ub = T.oracle_setup(oracle, c)
    opts = dict(TolX=1e-14, TolFun=1e-8, maxBacktracks=25)
    sp = T.spg_twin(ev, v0, Lb, Ub, MaxIter=3000, memory=10, **opts)
    lb = L.lbfgs_twin(ev, v0, Lb, Ub, MaxIter=3000, pairs=8, **opts)
    assert sp.converged.all() and lb.converged.all()
    on = (lb.v == Lb[:, None]) | (lb.v == Ub[:, None])
    assert on.any() and np.array_equal(on, (sp.v == Lb[:, None]) | (sp.v == Ub[:, None])), "the same active bounds"
    dJ = float(np.max(np.abs(sp.J - lb.J) / np.maximum(1.0, np.abs(lb.J))))
    dv = float(np.max(np.abs(sp.v - lb.v)))
    print("SPG - L-BFGS at TolFun 1e-8: dJ", dJ, "dv", dv, "iterations", int(sp.iterations.max()), int(lb.iterations.max()))
    assert dJ <= 8.9e-15 and dv <= 8.4e-7


def test_fewer_batch_evaluations_than_spg(oracle):
    """The purpose.  PWLinear, 41 control points, N = 200, T = 40, bounds [0, 1] active for part of the 16 instances,
    per-instance c and x0, the defaults TolFun = 3e-4, TolX = 1e-5: until every instance has stopped the L-BFGS twin calls
    evaluate 27 times, the SPG twin 32 times (CPU oracle).  The gain is in iterations (17 against 26); L-BFGS spends part of
    it on rejected unit steps, and on short horizons (T = 10) SPG needs no more evaluations than L-BFGS (NOTES.md)."""
    c = L.make_case(L.PURPOSE_CPU)
    ev, v0, Lb, Ub = T.oracle_setup(oracle, c)
    es, el = L.counted(ev), L.counted(ev)
    sp = T.spg_twin(es, v0, Lb, Ub, MaxIter=c.K, **c.opts)
    lb = L.lbfgs_twin(el, v0, Lb, Ub, MaxIter=c.K, pairs=c.pairs, **c.opts)
    print("batch evaluations: SPG", es.calls, "L-BFGS", el.calls, "iterations", int(sp.iterations.max()), int(lb.iterations.max()))
    assert not sp.active.any() and not lb.active.any() and sp.converged.all() and lb.converged.all()
    on = (lb.v == Lb[:, None]) | (lb.v == Ub[:, None])
    assert 0 < np.count_nonzero(on.any(axis=0)) < c.batch, "bounds active for part of the batch"
    assert el.calls < es.calls


def test_nan_trial_is_a_rejection():
    """a trial point whose objective is NaN is rejected and the instance recovers by halving; an instance whose every trial
    is NaN stops where it is after maxBacktracks evaluations (SPG's direction: no pair is held yet)"""
    def ev(V):                       # 0.5 v^2: undefined near 0 (instance 0), anywhere but at the start (instance 1)
        J = 0.5 * np.sum(V * V, axis=0)
        J[0] = np.nan if abs(V[0, 0]) < 0.25 else J[0]
        J[1] = np.nan if V[0, 1] != 1.0 else J[1]
        return J, V.copy()
    tw = L.lbfgs_twin(ev, np.ones((1, 3)), [-4.0], [4.0], TolX=1e-12, TolFun=1e-9, MaxIter=2, maxBacktracks=4, pairs=2)
    st = tw.steps[0]
    assert st.accepted.tolist() == [True, False, True] and st.failed.tolist() == [False, True, False]
    assert st.backtracks.tolist() == [1, 4, 0] and tw.snap[1].v[0].tolist() == [0.5, 1.0, 0.0]
    assert tw.v[0, 1] == 1.0 and tw.iterations[1] == 1 and not tw.active[1] and np.isfinite(tw.J).all()
