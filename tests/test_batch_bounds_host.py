"""Host side of the per-trajectory control bounds (no GPU needed): the two new C-ABI symbols are declared, bound and
exported, OCProblem.set_batch_bounds refuses wrong shapes and orders before it reaches the library, the library's own
argument checks come before any device work, and the start / box of single_shooting_batch under such bounds is what
single_shooting.m:56,82,89 builds for B single problems, column by column."""
import re
import subprocess

import numpy as np
import pytest

NEW = ("ocs_problem_set_batch_bounds", "ocs_single_shooting_batch_bounds_dev")
P = {"c": 1.5, "m": 3.0, "r": 0.05}


@pytest.fixture(scope="module")
def pkg():
    import __graft_entry__ as g
    g.build()
    return g.load_package()


def test_new_symbols_are_declared_bound_and_exported(pkg):
    """as tests/test_abi_exports.py inspects the library: header, binding table, dynamic symbol table"""
    from ocs_amd import _lib
    names = _lib.declared_symbols()
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True).stdout
    for n in NEW:
        assert n in names and n in _lib._SIG and hasattr(_lib.lib, n)
        assert f" T {n}\n" in out
    header = open(_lib.HEADER_PATH).read()
    assert re.search(r"int ocs_problem_set_batch_bounds\(ocs_problem p, int batch, const double \*lb, const double \*ub\);",
                     header)
    # the new shooting entry point has the argument list of the old one (only the meaning of Lb, Ub differs)
    flat = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", header, flags=re.S))
    old = re.search(r"int ocs_single_shooting_batch_dev\((.*?)\);", flat).group(1)
    new = re.search(r"int ocs_single_shooting_batch_bounds_dev\((.*?)\);", flat).group(1)
    assert old == new
    assert _lib._SIG[NEW[1]][1][:8] == _lib._SIG["ocs_single_shooting_batch_dev"][1][:8]
    assert _lib._SIG[NEW[1]][1][8:10] == [_lib.vp, _lib.vp]          # device pointers


def test_set_batch_bounds_value_errors(pkg):
    prob = pkg.LQProblem(-np.eye(2), np.ones((2, 2)), [1.0, 1.0], [1.0, 2.0], 0.05, [[-1.0, 1.0], [-2.0, 0.5]])
    ok_lb, ok_ub = np.full((2, 3), -0.5), np.full((2, 3), 0.25)
    bad = [
        (np.zeros((3, 3)), ok_ub),              # wrong nC
        (np.zeros(2), None),                    # 1-D
        (ok_lb, np.zeros((2, 3, 1))),           # 3-D
        (np.zeros((2, 0)), None),               # empty batch
        (ok_lb, np.full((2, 4), 0.25)),         # batches of lb and ub differ
        (np.full((2, 3), 0.3), ok_ub),          # lb > ub
        (None, np.array([[0.0, 0.0, 0.0], [-2.5, 0.0, 0.0]])),   # ub below the SHARED lb of control 2
        (np.array([[np.nan, 0, 0], [0, 0, 0]], dtype=float), np.ones((2, 3))),   # NaN is not ordered
    ]
    for lb, ub in bad:
        with pytest.raises(ValueError):
            prob.set_batch_bounds(lb, ub)
    assert prob.batch_bounds is None
    # clearing needs no device and no batch
    assert prob.set_batch_bounds() is prob and prob.batch_bounds is None


def test_batch_bounds_host_fills_the_missing_side(pkg):
    from ocs_amd.problem import batch_bounds_host
    cb = np.array([[-1.0, 1.0], [-2.0, 0.5]])
    assert batch_bounds_host(None, None, cb) is None
    ub = np.array([[0.1, 0.2, 0.3], [0.5, 0.4, np.inf]])
    lo, hi = batch_bounds_host(None, ub, cb)
    assert lo.flags.f_contiguous and hi.flags.f_contiguous
    assert np.array_equal(lo, [[-1.0] * 3, [-2.0] * 3]) and np.array_equal(hi, ub)
    assert np.array_equal(hi.ravel(order="K"), [0.1, 0.5, 0.2, 0.4, 0.3, np.inf])   # trajectory b at [nC b, nC (b + 1))
    lb = np.array([[-np.inf], [0.5]])
    lo, hi = batch_bounds_host(lb, None, cb)                    # lb == ub and -inf are allowed
    assert np.array_equal(lo, lb) and np.array_equal(hi, [[1.0], [0.5]])


def test_library_checks_its_arguments_before_any_device_work(pkg):
    from ocs_amd import _lib
    lib, dp = _lib.lib, _lib.dp
    prob = pkg.TestOCProblem(P, [[0.0, 1.0]])
    lb, ub = np.asfortranarray(np.zeros((1, 4))), np.asfortranarray(np.ones((1, 4)))
    q = lambda a: a.ctypes.data_as(dp)   # noqa: E731
    assert lib.ocs_problem_set_batch_bounds(None, 4, q(lb), q(ub)) == -1
    assert lib.ocs_problem_set_batch_bounds(prob._h, 4, q(lb), None) == -1
    assert lib.ocs_problem_set_batch_bounds(prob._h, 4, None, q(ub)) == -1
    assert lib.ocs_problem_set_batch_bounds(prob._h, 0, q(lb), q(ub)) == -1
    assert lib.ocs_problem_set_batch_bounds(prob._h, -2, q(lb), q(ub)) == -1
    hi = np.asfortranarray(np.array([[1.0, 1.0, -0.5, 1.0]]))
    assert lib.ocs_problem_set_batch_bounds(prob._h, 4, q(lb), q(hi)) == -1
    assert b"trajectory 2" in lib.ocs_last_error()
    nan = np.asfortranarray(np.array([[0.0, np.nan, 0.0, 0.0]]))
    assert lib.ocs_problem_set_batch_bounds(prob._h, 4, q(nan), q(ub)) == -1
    for batch in (0, 7, -1):                                    # both NULL clears, whatever the batch
        assert lib.ocs_problem_set_batch_bounds(prob._h, batch, None, None) == 0


@pytest.mark.parametrize("kind", ["PWLinear", "PWConstant"])
def test_start_and_box_of_single_shooting_batch(pkg, kind):
    """batch_bounds_start against B single problems: u0 clamped as single_shooting.m:56 clamps it for instance b's own
    ControlBounds, v0 = compute_initial_v (:82), [Lb, Ub] = compute_nlp_bounds (:89).  Two controls, bounds that differ per
    control and per instance, one side infinite."""
    from ocs_amd.solvers import batch_bounds_start, clamp_u0_batch
    t = np.linspace(0.0, 4.0, 2 * 24 + 1)
    nC, B = 2, 5
    ctrl = (pkg.PWLinearControl(t, 7, nC) if kind == "PWLinear" else pkg.PWConstantControl(t, 6, nC))
    lo = np.array([[0.0, 0.1, -0.3, -np.inf, 0.2], [-1.0, -0.5, 0.0, -2.0, -0.25]])
    hi = np.array([[0.3, 0.6, 1.0, 0.4, 0.2], [0.5, np.inf, 0.25, -1.0, 0.75]])
    nV = ctrl.nControls * ctrl.nBasis
    for u0 in (0.45, [0.45, -1.5], np.array([[0.5, 0.05, 2.0, -7.0, 0.0], [0.6, 0.0, -1.0, -1.5, 0.8]])):
        v0, Lb, Ub = batch_bounds_start(ctrl, u0, (lo, hi), B)
        assert v0.shape == Lb.shape == Ub.shape == (nV, B)
        for b in range(B):
            cb = np.column_stack([lo[:, b], hi[:, b]])
            u0b = np.asarray(u0, dtype=np.float64)
            u0b = u0b[:, b] if u0b.ndim == 2 else u0b
            u0c, per = clamp_u0_batch(u0b, cb, 1)                # the single problem's clamp
            assert not per
            assert np.array_equal(v0[:, b], ctrl.compute_initial_v(u0c))
            Lb1, Ub1 = ctrl.compute_nlp_bounds(cb)
            assert np.array_equal(Lb[:, b], Lb1) and np.array_equal(Ub[:, b], Ub1)
            assert np.all(Lb[:, b] <= v0[:, b]) and np.all(v0[:, b] <= Ub[:, b])
    # equal columns give what the shared bounds give
    from ocs_amd.solvers import initial_v_batch
    cb = np.array([[0.0, 0.3], [-1.0, 0.5]])
    same = (np.repeat(cb[:, 0:1], B, 1), np.repeat(cb[:, 1:2], B, 1))
    v0, Lb, Ub = batch_bounds_start(ctrl, [0.45, -1.5], same, B)
    assert np.array_equal(v0, initial_v_batch(ctrl, [0.45, -1.5], cb, B))
    Lb1, Ub1 = ctrl.compute_nlp_bounds(cb)
    assert np.array_equal(Lb, np.repeat(Lb1[:, None], B, 1)) and np.array_equal(Ub, np.repeat(Ub1[:, None], B, 1))
    # another batch than the bounds', a wrong u0
    with pytest.raises(ValueError, match="batch"):
        batch_bounds_start(ctrl, 0.1, (lo, hi), B + 1)
    with pytest.raises(ValueError):
        batch_bounds_start(ctrl, np.zeros((3, B)), (lo, hi), B)


def test_a_control_without_nlp_bounds_is_unbounded_per_instance(pkg):
    from ocs_amd.solvers import batch_bounds_start
    t = np.linspace(0.0, 4.0, 2 * 24 + 1)
    ctrl = pkg.ChebyshevControl(t, 5, 1)
    lo, hi = np.zeros((1, 3)), np.array([[0.3, 0.6, 1.0]])
    v0, Lb, Ub = batch_bounds_start(ctrl, 0.45, (lo, hi), 3)
    assert np.all(Lb == -np.inf) and np.all(Ub == np.inf) and v0.shape == Lb.shape
    for b, u in enumerate((0.3, 0.45, 0.45)):
        assert np.array_equal(v0[:, b], ctrl.compute_initial_v([u]))
