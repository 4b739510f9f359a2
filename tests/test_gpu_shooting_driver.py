"""The batched shooting driver (ocs_single_shooting_batch_dev + the k_spg_* kernels) against its step-exact NumPy twin
(tests/spg_twin.py).  The twin evaluates objective and gradient with the library's own nlp_objective_dev on the same
handles, the whole batch in one call, so it sees the bits the driver sees and only the driver's bookkeeping is under test.
The driver is deterministic: its state after k iterations is what it returns with MaxIter = k, taken for k = 0..K.

Tolerance: measured, not guessed.  The twin runs a second time with every d and alpha moved by one ulp in a seeded random
direction; 16 x the largest difference between the two runs (relative to max(1, |.|), over v, J and the projected gradient
at every k), at least 1e-13, is allowed between driver and twin.  Instances with a comparison closer than 1e-9 or with
discrete results that differ between the two twin runs are indecisive and left out, at most 5 % of a batch.
Measured on an MI355X (spread of the two twin runs -> tolerance; largest driver-twin difference), 0-2 indecisive each:
  blocks257 2.0e-15 -> 1e-13 (2.2e-15)    blocks600 2.1e-15 -> 1e-13 (1.8e-15)    backtrack 2.4e-12 -> 3.8e-11 (1.4e-14)
  exhausted1 1.6e-15 -> 1e-13 (2.2e-16)   exhausted2 7.7e-15 -> 1.2e-13 (8.2e-15) tolx 7.2e-16 -> 1e-13 (3.9e-16)
  zero 0 -> 1e-13 (0)                     free 3.0e-12 -> 4.8e-11 (3.5e-13)
  cheb64on 3.0e-11 -> 4.8e-10 (4.6e-12)   cheb64off 1.7e-11 -> 2.8e-10 (6.8e-12)
  cheb70on 7.3e-11 -> 1.2e-9 (7.3e-12)    cheb70off 7.9e-11 -> 1.3e-9 (1.5e-11)
(the Chebyshev cases have no bounds and steps of several hundred, backtrack has instances that recover from a non-finite
trial point, free sits next to the collapse of its second state: there the iteration itself amplifies a last-place difference)."""
import numpy as np
import pytest

from tests import spg_twin as T

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ocs():
    import torch
    assert torch.cuda.is_available()
    import __graft_entry__ as g
    return g.load_package()


_CACHE = {}


def _case(ocs, oracle, name):
    """handles, the K + 1 driver runs and the two twin runs of a case (computed once, read-only)"""
    if name in _CACHE:
        return _CACHE[name]
    c = T.make_inputs(name)
    s = T.device_setup(ocs, oracle, c)
    s.runs = [s.solve(k) for k in range(c.K + 1)]
    s.tw = T.spg_twin(s.evaluate, s.v0, s.Lb, s.Ub, MaxIter=c.K, **c.opts)
    s.tw2 = T.spg_twin(s.evaluate, s.v0, s.Lb, s.Ub, MaxIter=c.K, ulp_seed=c.seed, **c.opts)
    _CACHE[name] = s
    return s


@pytest.mark.parametrize("name", list(T.CASES))
def test_driver_follows_the_twin(ocs, oracle, name):
    """every decisive instance at every k = 0..K: iterations, converged and the moving set equal to the twin's; v, J and
    projected_gradient within the measured tolerance; the case's purpose asserted on the twin (module docstring)."""
    s = _case(ocs, oracle, name)
    dec, spread, tol = T.measured_tolerance(s.tw, s.tw2)
    T.check_invariants(s.c, s.tw, s.Lb, s.Ub)
    T.check_purpose(s.c, s.tw, dec, s.Lb, s.Ub)
    worst = T.compare_with_twin(s.runs, s.tw, dec, tol)
    print(f"{name}: indecisive {np.count_nonzero(~dec)}/{s.c.batch} spread {spread:.3e} tolerance {tol:.3e} driver-twin {worst:.3e}")


@pytest.mark.parametrize("name", list(T.CASES))
def test_driver_against_itself_bit_for_bit(ocs, oracle, name):
    """no twin: an instance that finished keeps v, J and iterations in every longer run; the returned J is nlp_objective_dev
    at the returned v (and x0); projected_gradient is max |P(v - g) - v| of that gradient, exactly; v inside the bounds."""
    s = _case(ocs, oracle, name)
    runs, free = s.runs, list(s.c.free)
    for k, r in enumerate(runs):
        assert np.all(r.iterations <= k) and np.all(r.iterations >= 0)
        assert np.all(r.v >= s.Lb[:, None]) and np.all(r.v <= s.Ub[:, None])
        done = r.iterations < k                         # stopped before iteration k
        for r2 in runs[k + 1:]:
            assert np.array_equal(r2.v[:, done], r.v[:, done]) and np.array_equal(r2.J[done], r.J[done])
            assert np.array_equal(r2.iterations[done], r.iterations[done])
        J, G, x0n = s.evaluate(r.v, want_x0=True)
        assert np.array_equal(J, r.J) and np.array_equal(x0n, r.x0)
        pgn = np.fmax.reduce(np.abs(np.fmin(np.fmax(r.v - G, s.Lb[:, None]), s.Ub[:, None]) - r.v), axis=0, initial=0.0)
        assert np.array_equal(pgn, r.pgn)
        assert np.array_equal(r.converged, pgn <= 10.0 * s.c.TolFun)
        for i, f in enumerate(free):                    # single_shooting.m:121-124
            assert np.array_equal(r.x0[f - 1], r.v[s.c.nB + i])


@pytest.mark.parametrize("name", ["exhausted1", "exhausted2"])
def test_failed_line_search_stops_where_it_is(ocs, oracle, name):
    """an instance whose line search ran out of backtracks: v and J bit-equal to their values one k earlier, iterations
    counts that iteration, and it never moves again"""
    s = _case(ocs, oracle, name)
    dec = T.measured_tolerance(s.tw, s.tw2)[0]
    seen = 0
    for it, st in enumerate(s.tw.steps):
        f = st.failed & dec
        seen += int(np.count_nonzero(f))
        a, b = s.runs[it], s.runs[it + 1]
        assert np.array_equal(b.v[:, f], a.v[:, f]) and np.array_equal(b.J[f], a.J[f])
        assert np.all(b.iterations[f] == it + 1) and np.all(s.runs[-1].iterations[f] == it + 1)
        assert np.array_equal(s.runs[-1].v[:, f], a.v[:, f])
    assert seen >= 5


def test_tolx_stop_is_not_convergence(ocs, oracle):
    s = _case(ocs, oracle, "tolx")                      # the call returned and did not raise
    dec = T.measured_tolerance(s.tw, s.tw2)[0]
    tolx = np.any([st.tolx for st in s.tw.steps], axis=0) & dec
    last = s.runs[-1]
    assert tolx.any() and not last.converged[tolx].any() and np.all(last.iterations[tolx] < s.c.K)
    assert np.all(last.pgn[tolx] > 10.0 * s.c.TolFun)


def test_maxiter_zero(ocs, oracle):
    s = _case(ocs, oracle, "zero")
    r = s.runs[0]
    J0, _ = s.evaluate(s.v0)
    assert np.array_equal(r.v, s.v0) and np.array_equal(r.J, J0) and np.all(r.iterations == 0)


def test_max_backtracks_default(ocs, oracle):
    """maxBacktracks=None is the value of ocs_ss_default_options: on the inputs the backtrack and exhausted cases share, the
    call without the keyword equals the call with that value bit for bit and differs from the call with maxBacktracks=2"""
    import ctypes as C
    import torch
    from ocs_amd._lib import SsOptions, lib
    o = SsOptions()
    assert lib.ocs_ss_default_options(C.byref(o)) == 0
    s, s2 = _case(ocs, oracle, "backtrack"), _case(ocs, oracle, "exhausted2")
    c = s.c
    assert c.maxBacktracks == o.maxBacktracks and s2.c.maxBacktracks == 2 and np.array_equal(c.v0, s2.c.v0)
    tspan = oracle.linspace(0, c.T, c.N + 1)
    prob = ocs.TestOCProblem(T.P, T.BOUNDS)
    prob.set_batch_params([0, 1], np.vstack([c.cs, c.ms]))
    r = ocs.single_shooting_batch(prob, c.x0, tspan, c.nB, v0=c.v0, MaxIter=c.K, TolX=c.TolX, TolFun=c.TolFun, memory=c.memory)
    torch.cuda.synchronize()
    v, it = r["v"].cpu().numpy(), r["iterations"].cpu().numpy()
    assert np.array_equal(v, s.runs[-1].v) and np.array_equal(it, s.runs[-1].iterations)
    assert not np.array_equal(it, s2.runs[-1].iterations) and not np.array_equal(v, s2.runs[-1].v)
