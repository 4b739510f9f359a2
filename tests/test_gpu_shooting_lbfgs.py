"""The batched shooting driver with Algorithm = "lbfgs" (ocs_single_shooting_batch_dev + the k_lbfgs_* kernels) against its
step-exact NumPy twin (tests/lbfgs_twin.py), as tests/test_gpu_shooting_driver.py does for SPG.  The twin evaluates objective
and gradient with the library's own nlp_objective_dev on the same handles, the whole batch in one call, so only the driver's
bookkeeping is under test.  The driver's state after k iterations is what it returns with MaxIter = k, taken for k = 0..K.

Tolerance: measured.  The twin runs a second time with every d and alpha moved by one ulp in a seeded random direction;
16 x the largest difference between the two runs (relative to max(1, |.|), over v, J and the projected gradient at every k),
at least 1e-13, is allowed between driver and twin.  Instances with a comparison closer than 1e-9 or with discrete results
that differ between the two twin runs are indecisive and left out, at most 5 % of a batch.
Measured on an MI355X (spread of the two twin runs -> tolerance; largest driver-twin difference; indecisive):
  ring257 6.7e-15 -> 1.1e-13 (4.3e-15; 1)    ring600 4.4e-14 -> 7.1e-13 (3.8e-15; 0)    fail257 4.4e-15 -> 1e-13 (2.8e-15; 0)
  free257 2.1e-7 -> 3.3e-6 (9.1e-8; 2)       cheb257 4.4e-8 -> 7.1e-7 (6.9e-8; 0)
(free257 sits next to the collapse of its second state and cheb257 has no bounds and steps of several hundred: there most pairs
fail their test, the line searches run to 25 halvings, and the iteration itself amplifies a last-place difference.)"""
import ctypes as C

import numpy as np
import pytest

from tests import lbfgs_twin as L
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
    """the K + 1 driver runs and the two twin runs of a case (computed once, read-only)"""
    if name in _CACHE:
        return _CACHE[name]
    c = L.make_case(name)
    s = T.device_setup(ocs, oracle, c)
    s.runs = [s.solve(k, Algorithm="lbfgs", pairs=c.pairs) for k in range(c.K + 1)]
    s.tw = L.lbfgs_twin(s.evaluate, s.v0, s.Lb, s.Ub, MaxIter=c.K, pairs=c.pairs, **c.opts)
    s.tw2 = L.lbfgs_twin(s.evaluate, s.v0, s.Lb, s.Ub, MaxIter=c.K, pairs=c.pairs, ulp_seed=c.seed, **c.opts)
    _CACHE[name] = s
    return s


@pytest.mark.parametrize("name", list(L.LCASES))
def test_driver_follows_the_twin(ocs, oracle, name):
    """every decisive instance at every k = 0..K: iterations, converged and the moving set equal to the twin's; v, J and
    projected_gradient within the measured tolerance; the case's purpose asserted on the twin (module docstring)."""
    s = _case(ocs, oracle, name)
    dec, spread, tol = T.measured_tolerance(s.tw, s.tw2)
    T.check_invariants(s.c, s.tw, s.Lb, s.Ub)
    L.check_lbfgs_invariants(s.tw)
    print(f"{name}: indecisive {np.count_nonzero(~dec)}/{s.c.batch} spread {spread:.3e} tolerance {tol:.3e}")
    L.check_case_purpose(s.c, s.tw, dec, s.Lb, s.Ub)
    worst = T.compare_with_twin(s.runs, s.tw, dec, tol)
    print(f"{name}: driver-twin {worst:.3e}")


@pytest.mark.parametrize("name", list(L.LCASES))
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


def test_default_is_spg_untouched(ocs, oracle):
    """Algorithm="spg" (any case of letters) and no Algorithm at all return the same bits, with the same keys; "lbfgs" returns
    other iteration counts on the same inputs"""
    s = _case(ocs, oracle, "ring257")
    K = s.c.K
    a, b, u = s.solve(K), s.solve(K, Algorithm="spg"), s.solve(K, Algorithm="SPG", pairs=3)
    for r in (b, u):
        assert np.array_equal(a.v, r.v) and np.array_equal(a.J, r.J) and np.array_equal(a.iterations, r.iterations)
        assert np.array_equal(a.pgn, r.pgn) and np.array_equal(a.converged, r.converged) and a.keys == r.keys
    lb = s.runs[-1]
    assert lb.keys == a.keys and not np.array_equal(lb.iterations, a.iterations)
    low = s.solve(K, Algorithm="LBFGS", pairs=s.c.pairs)
    assert np.array_equal(low.v, lb.v) and np.array_equal(low.iterations, lb.iterations)
    dflt, eight = s.solve(K, Algorithm="lbfgs"), s.solve(K, Algorithm="lbfgs", pairs=8)     # pairs=None: the default, 8
    assert np.array_equal(dflt.v, eight.v) and not np.array_equal(dflt.v, lb.v)


def test_usage_errors(ocs, oracle):
    """algorithm = 2, and pairs = 0 or 17 under L-BFGS, are OCS_ERR_INVALID; pairs is not looked at under SPG; a bad Algorithm
    string is a ValueError before any library call"""
    import torch
    from ocs_amd._lib import SsOptions, lib
    s = _case(ocs, oracle, "ring257")
    c = s.c
    o = SsOptions()
    assert lib.ocs_ss_default_options(C.byref(o)) == 0 and (o.algorithm, o.pairs) == (0, 8)
    dev = torch.device("cuda:0")
    B = c.batch

    def call(algorithm, pairs):
        o.algorithm, o.pairs, o.MaxIter = algorithm, pairs, 1
        x0 = torch.tensor(c.x0, device=dev).contiguous()
        v = torch.tensor(np.ascontiguousarray(s.v0), device=dev).contiguous()
        J = torch.empty(B, dtype=torch.float64, device=dev)
        Lb, Ub = np.ascontiguousarray(s.Lb), np.ascontiguousarray(s.Ub)
        dp = C.POINTER(C.c_double)
        rc = lib.ocs_single_shooting_batch_dev(s.integ._h, s.prob._h, s.ctrl._h, B, C.c_void_p(x0.data_ptr()),
                                               C.c_void_p(v.data_ptr()), 0, None, Lb.ctypes.data_as(dp), Ub.ctypes.data_as(dp),
                                               C.byref(o), C.c_void_p(J.data_ptr()), None, None, None, None)
        torch.cuda.synchronize()
        return rc
    INVALID = -1
    assert call(2, 8) == INVALID and call(-1, 8) == INVALID
    assert call(1, 0) == INVALID and call(1, 17) == INVALID
    assert call(1, 1) >= 0 and call(1, 16) >= 0 and call(0, 0) >= 0
    for bad in ("sqp", "", None, 1):
        with pytest.raises(ValueError):
            s.solve(1, Algorithm=bad)


def test_end_to_end_fewer_batch_evaluations(ocs, oracle):
    """the purpose at GPU-test size (PWLinear, 21 points, N = 60, T = 50, batch 257, the defaults TolFun = 3e-4, TolX = 1e-5):
    the L-BFGS solve reports every instance converged, as the SPG solve does, and needs fewer batch evaluations -- counted in
    the twins fed by the GPU evaluations, the driver has no counter.
    Measured on an MI355X: SPG 66 evaluations (34 iterations at the most), L-BFGS 49 (20)."""
    c = L.make_case(L.PURPOSE_GPU)
    s = T.device_setup(ocs, oracle, c)
    es, el = L.counted(s.evaluate), L.counted(s.evaluate)
    sp = T.spg_twin(es, s.v0, s.Lb, s.Ub, MaxIter=c.K, **c.opts)
    lb = L.lbfgs_twin(el, s.v0, s.Lb, s.Ub, MaxIter=c.K, pairs=c.pairs, **c.opts)
    print("batch evaluations: SPG", es.calls, "L-BFGS", el.calls, "iterations", int(sp.iterations.max()), int(lb.iterations.max()))
    assert not sp.active.any() and not lb.active.any()
    rl, rs = s.solve(c.K, Algorithm="lbfgs", pairs=c.pairs), s.solve(c.K)
    assert rl.converged.all() and rs.converged.all() and np.all(rl.iterations < c.K)
    on = (rl.v == s.Lb[:, None]) | (rl.v == s.Ub[:, None])
    assert 0 < np.count_nonzero(on.any(axis=0)) < c.batch, "bounds active for part of the batch"
    assert el.calls < es.calls
