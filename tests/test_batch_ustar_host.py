"""Host side of the per-trajectory uStar of RK4InfiniteIntegrator (no GPU needed): the two new C-ABI symbols are declared
and exported, the MATLAB shim calls only exported symbols, and the shape logic of RK4InfiniteIntegrator(uStar),
set_batch_uStar and the u0 of single_shooting_batch does what their docstrings say."""
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("ocs_rk4inf_set_batch_ustar", "ocs_rk4inf_set_batch_ustar_dev")


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
    assert re.search(r"int ocs_rk4inf_set_batch_ustar\(ocs_integrator g, int batch, const double \*uStar\);", header)
    assert re.search(r"int ocs_rk4inf_set_batch_ustar_dev\(ocs_integrator g, int batch, const double \*uStar, void \*stream\);", header)


def test_setters_validate_the_handle_before_any_device_work(pkg):
    """null handle and a plain RK4Integrator: OCS_ERR_INVALID; batch < 0: OCS_ERR_SHAPE; clearing needs no device"""
    import ctypes as C
    from ocs_amd import _lib
    lib = _lib.lib
    U = np.asfortranarray(np.full((1, 4), 0.3))
    assert lib.ocs_rk4inf_set_batch_ustar(None, 4, U.ctypes.data_as(_lib.dp)) == -1
    assert lib.ocs_rk4inf_set_batch_ustar_dev(None, 4, None, None) == -1
    g0 = pkg.RK4Integrator(np.linspace(0, 1, 5))
    assert lib.ocs_rk4inf_set_batch_ustar(g0._h, 4, U.ctypes.data_as(_lib.dp)) == -1
    assert b"RK4InfiniteIntegrator" in lib.ocs_last_error()
    assert lib.ocs_rk4inf_set_batch_ustar_dev(g0._h, 0, None, None) == -1
    gi = pkg.RK4InfiniteIntegrator(np.linspace(0, 1, 5), np.linspace(1, 2, 5), [0.4])
    assert lib.ocs_rk4inf_set_batch_ustar(gi._h, -1, U.ctypes.data_as(_lib.dp)) == -2
    assert lib.ocs_rk4inf_set_batch_ustar_dev(gi._h, -3, None, None) == -2
    assert gi.set_batch_uStar() is gi and gi.batch_uStar is None          # clear: batch 0 / NULL
    assert lib.ocs_rk4inf_set_batch_ustar(gi._h, 4, None) == 0
    assert lib.ocs_rk4inf_set_batch_ustar_dev(gi._h, 0, C.c_void_p(0), None) == 0


def test_matlab_shim_calls_the_new_symbol_and_only_exported_ones(pkg):
    from ocs_amd import _lib
    text = open(os.path.join(ROOT, "matlab", "GpuRK4Integrator.m")).read()
    called = set(re.findall(r"calllib\('libocs',\s*'(ocs_[a-z0-9_]+)'", text))
    assert "ocs_rk4inf_set_batch_ustar" in called
    declared = set(_lib.declared_symbols())
    assert called <= declared, sorted(called - declared)
    for n in called:
        assert hasattr(_lib.lib, n), n


def test_constructor_argument_shared_or_per_trajectory(pkg):
    from ocs_amd.integrator import split_uStar
    for shared_form in (0.4, [0.4], np.array([0.4]), np.array([[0.4]])):
        s, b = split_uStar(shared_form)
        assert b is None and s.shape == (1,) and s[0] == 0.4
    s, b = split_uStar([0.1, -0.2, 0.3])
    assert b is None and np.array_equal(s, [0.1, -0.2, 0.3])
    s, b = split_uStar(np.array([[0.1], [-0.2]]))           # one column: the reference's nC x 1
    assert b is None and np.array_equal(s, [0.1, -0.2])
    U = np.arange(6.0).reshape(2, 3)
    s, b = split_uStar(U)                                    # nC x B: column 0 creates the handle, the matrix is set
    assert np.array_equal(s, [0.0, 3.0]) and np.array_equal(b, U) and b.flags.f_contiguous
    s, b = split_uStar(np.full((1, 70), 0.5))                # nC = 1, B = 70 (compute_equilibrium's uStar of a batch)
    assert s.shape == (1,) and b.shape == (1, 70)
    with pytest.raises(ValueError):
        split_uStar(np.zeros((2, 3, 4)))
    with pytest.raises(ValueError):
        split_uStar([])


def test_set_batch_ustar_shapes(pkg):
    from ocs_amd.integrator import batch_uStar_host
    U = np.arange(8.0).reshape(2, 4)
    a = batch_uStar_host(U, 2)
    assert a.flags.f_contiguous and np.array_equal(a, U)
    assert np.array_equal(a.ravel(order="K"), [0, 4, 1, 5, 2, 6, 3, 7])     # column-major: trajectory b at [nC b, nC (b+1))
    assert batch_uStar_host(U.tolist(), 2).dtype == np.float64
    with pytest.raises(ValueError, match="3 x B"):
        batch_uStar_host(U, 3)                               # wrong nC
    with pytest.raises(ValueError, match="1-D"):
        batch_uStar_host(np.arange(4.0), 1)                  # 1-D: nC values of one trajectory, or nC = 1 for B?
    with pytest.raises(ValueError):
        batch_uStar_host(0.3, 1)
    with pytest.raises(ValueError):
        batch_uStar_host(np.zeros((2, 0)), 2)
    # the method refuses them before it reaches the library
    gi = pkg.RK4InfiniteIntegrator(np.linspace(0, 1, 5), np.linspace(1, 2, 5), [0.4, 0.1])
    for bad in (np.zeros((3, 4)), np.zeros(2), np.zeros((1, 4))):
        with pytest.raises(ValueError):
            gi.set_batch_uStar(bad)
    assert gi.batch_uStar is None


class _Control:
    """compute_initial_v of a control with nBasis = 3: v(c + nC (i - 1)) = u0(c)"""
    def compute_initial_v(self, u0):
        u0 = np.asarray(u0, dtype=np.float64)
        assert u0.ndim == 1
        return np.tile(u0, 3)


def test_u0_of_single_shooting_batch(pkg):
    from ocs_amd.solvers import clamp_u0_batch, initial_v_batch
    bounds = np.array([[0.0, 1.0], [-1.0, 0.5]])
    B = 4
    # shared: a scalar, nC values, a column, a row -- clamped, shape (nC,), as before
    for u0, want in ((0.2, [0.2, 0.2]), ([2.0, -3.0], [1.0, -1.0]), (np.array([[0.3], [0.7]]), [0.3, 0.5]),
                     (np.array([[0.3, 0.7]]), [0.3, 0.5])):
        u0c, per = clamp_u0_batch(u0, bounds, B)
        assert not per and u0c.shape == (2,) and np.array_equal(u0c, want)
    v = initial_v_batch(_Control(), [2.0, -3.0], bounds, B)
    assert v.shape == (6, B) and np.array_equal(v, np.repeat(np.tile([1.0, -1.0], 3)[:, None], B, 1))
    # nC x B: one start per instance, clamped per row, expanded column by column
    U0 = np.array([[0.1, 0.2, 1.5, -0.2], [0.4, 0.6, -2.0, 0.0]])
    u0c, per = clamp_u0_batch(U0, bounds, B)
    assert per and np.array_equal(u0c, [[0.1, 0.2, 1.0, 0.0], [0.4, 0.5, -1.0, 0.0]])
    v = initial_v_batch(_Control(), U0, bounds, B)
    assert v.shape == (6, B)
    for b in range(B):
        assert np.array_equal(v[:, b], np.tile(u0c[:, b], 3))
    # equal columns give what the shared value gives
    assert np.array_equal(initial_v_batch(_Control(), np.repeat([[0.3], [0.2]], B, 1), bounds, B),
                          initial_v_batch(_Control(), [0.3, 0.2], bounds, B))
    # nC = 1: 1 x B is per instance
    u0c, per = clamp_u0_batch(np.array([[0.1, 0.2, 0.3, 1.4]]), bounds[:1], B)
    assert per and np.array_equal(u0c, [[0.1, 0.2, 0.3, 1.0]])
    # wrong nC, wrong B, wrong length
    for bad in (np.zeros((3, B)), np.zeros((2, B + 1)), np.zeros(3), np.zeros((2, 2, 2))):
        with pytest.raises(ValueError):
            clamp_u0_batch(bad, bounds, B)
