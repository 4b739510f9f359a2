"""tests/xlam_err_twin.py is pinned here, on the CPU, before anything is compared with it: its pieces against tests/fbs_twin.py
and tests/rk4_twin.py, the state estimate against a closed-form flow, the coupling term, the refinement rule, errJ against the
difference of two grids; and the new symbols of the library.

errJ: the sum of the cost row's (fine - coarse) alone is not an estimate of the objective's error -- on the case of
test_errJ_is_the_difference_of_two_grids it is 3.3 to 3.6 times J(N) - J(2N), at every N, because the state error of a step
changes the cost of every later step.  With that term, lam_{i+1}' (coarse - fine), errJ / (J(N) - J(2N)) is 1.36, 1.07, 1.05,
1.05 at N = 10, 20, 40, 80 (16/15 in the limit)."""
import ctypes as C

import numpy as np
import pytest

from tests import fbs_twin as ft
from tests import rk4_twin as tw
from tests import xlam_err_twin as xt

L = np.longdouble
PROB = tw.LogisticK([3.0], 1.5, 0.05)


def smooth_u(t):
    return 0.3 + 0.2 * np.sin(np.asarray(t))


def passes(prob, ts, x0, u):
    x, _, J, lam = ft.compute_x_lam(prob, ts, x0, u)
    return x.astype(np.float64), lam.astype(np.float64), J


def test_pieces_are_the_twins_they_restate():
    """slopes / piece in longdouble against fbs_twin.pchip_eval at the quarter points of a non-uniform grid; the coarse steps
    against the passes of fbs_twin: from x_i the state step gives the pass's x_{i+1}, from lam_{i+1} the costate step with the
    pchip midpoint gives the pass's lam_i."""
    ts = np.array([0.0, 0.4, 1.0, 1.3, 2.2, 3.0])
    t, h = tw.grid(ts)
    rng = np.random.default_rng(3)
    y = rng.normal(size=(2, t.size, 3))
    tq, _ = xt.quarter_points(ts)
    want = ft.pchip_eval(t, y, tq)
    u1, u3 = xt.control_quarters(ts, y, L)
    assert np.max(np.abs(u1 - want[:, 0::2])) < 64 * tw.EPS and np.max(np.abs(u3 - want[:, 1::2])) < 64 * tw.EPS
    # the coarse steps are the passes' steps: rebuild x_{i+1} and lam_i from the twin's own pieces
    u = smooth_u(t)[None, :, None]
    x, cost, J, lam = ft.compute_x_lam(PROB, ts, [[2.0]], u)
    dx = xt.slopes(h, x, L)
    for i in range(h.size):
        hi = L(h[i])
        yA = np.concatenate([x[:, i], np.zeros((1, 1), dtype=L)])
        fA = PROB.F(t[2 * i], yA, u[:, 2 * i])
        yc = xt.state_step(PROB, yA, hi, fA, t[2 * i + 1], u[:, 2 * i + 1], t[2 * i + 2], u[:, 2 * i + 2], L)
        assert np.max(np.abs(yc[:-1] - x[:, i + 1])) < 8 * tw.EPS
        xM = xt.piece(x[:, i], x[:, i + 1], dx[:, i], dx[:, i + 1], hi, L(t[2 * i + 1] - t[2 * i]))
        lc = xt.costate_step(PROB, lam[:, i + 1], hi, (t[2 * i + 2], x[:, i + 1], u[:, 2 * i + 2]), (t[2 * i + 1], xM, u[:, 2 * i + 1]),
                             (t[2 * i], x[:, i], u[:, 2 * i]), L)
        assert np.max(np.abs(lc - lam[:, i])) < 8 * tw.EPS * max(1.0, float(np.max(np.abs(lam))))


def test_state_estimate_against_the_closed_form_flow():
    """u = 0, x0 = 1, x' = x (3 - x): the flow from x_i over h is 3 / (1 + (3 / x_i - 1) e^{-3h}), so the true local error of
    every step of the pass is known.  estimate / true over the intervals with true > 1e3 eps: closer to 1 at N = 80 than at
    N = 40, within 10 % at N = 80."""
    worst = {}
    for N in (40, 80):
        ts = np.linspace(0.0, 4.0, N + 1)
        _, h = tw.grid(ts)
        u = np.zeros((1, 2 * N + 1, 1))
        x, _, _, lam = ft.compute_x_lam(PROB, ts, [[1.0]], u)
        e = xt.estimate(PROB, ts, u, x.astype(np.float64), lam.astype(np.float64), 1e-6, 1e-6, L)
        xi = x.astype(np.float64).astype(L)[0, :-1, 0]
        flow = 3 / (1 + (3 / xi - 1) * np.exp(-3 * h.astype(L)))
        # (the estimate starts from the float64 x_i it is given; the pass's step from there is x_{i+1} up to rounding)
        true = np.abs(x[0, 1:, 0] - flow)
        big = true > 1e3 * tw.EPS
        assert big.sum() >= N // 2
        r = (e["ex"][0, :, 0] / true)[big]
        worst[N] = float(np.max(np.abs(r - 1)))
        print(f"N {N}: estimate / true in {float(r.min()):.4f} .. {float(r.max()):.4f} over {int(big.sum())} intervals")
    assert worst[80] < worst[40] and worst[80] < 0.1


def test_the_coupling_error_is_seen():
    """el with the Hermite states of the fine costate steps against el with pchip-of-node states everywhere: they differ by
    far more than rounding, by a good part of el itself"""
    N = 20
    ts = np.linspace(0.0, 10.0, N + 1)
    t, _ = tw.grid(ts)
    u = smooth_u(t)[None, :, None]
    x, lam, _ = passes(PROB, ts, [[2.0]], u)
    a = xt.estimate(PROB, ts, u, x, lam, 1e-6, 1e-6, L)
    b = xt.estimate(PROB, ts, u, x, lam, 1e-6, 1e-6, L, hermite=False)
    gap = float(np.max(np.abs(a["el"] - b["el"])))
    print(f"el {float(np.max(a['el'])):.3e}, with pchip states {float(np.max(b['el'])):.3e}, largest difference {gap:.3e}")
    assert gap > 1e6 * tw.EPS * float(np.max(np.abs(lam))) and gap > 0.05 * float(np.max(a["el"]))
    assert np.array_equal(a["ex"], b["ex"])


def test_refinement_rule():
    mesh = np.array([0.0, 1.0, 2.5, 3.0, 4.0, 6.0, 7.0])
    r = np.array([0.5, 1.0, 1.0000001, 31.999, 32.0, np.nan])
    new = xt.refine(mesh, r, 1, 32)
    want = sorted(list(mesh) + [0.5 * (2.5 + 3.0), 0.5 * (3.0 + 4.0), (2 * 4.0 + 6.0) / 3, (4.0 + 2 * 6.0) / 3, (2 * 6.0 + 7.0) / 3,
                                (6.0 + 2 * 7.0) / 3])
    assert np.array_equal(new, np.array(want))
    assert np.isin(mesh, new).all() and np.all(np.diff(new) > 0)
    assert np.array_equal(xt.refine(mesh, np.zeros(6), 1, 32), mesh) and np.array_equal(xt.refine(mesh, np.ones(6), 1, 32), mesh)
    assert xt.refine(mesh, np.full(6, np.inf), 1, 32).size == mesh.size + 12
    rmax, rinst = xt.reductions(np.array([[1.0, np.nan], [3.0, 0.1]]), np.array([[2.0, 0.0], [0.5, 0.2]]), use=[1, 0])
    assert np.array_equal(rmax, [2.0, 3.0]) and np.array_equal(rinst, [3.0, np.inf])
    rmax, _ = xt.reductions(np.array([[1.0, np.nan]]), np.array([[2.0, 0.0]]), use=[0, 0])
    assert np.array_equal(rmax, [0.0])


def test_errJ_is_the_difference_of_two_grids():
    """errJ against J(N) - J(2N) of the twin, uniform grid, smooth u sampled on either grid: to 20 %"""
    for N in (20, 40):
        ts = np.linspace(0.0, 10.0, N + 1)
        t, _ = tw.grid(ts)
        t2, _ = tw.grid(t)
        x, lam, J = passes(PROB, ts, [[2.0]], smooth_u(t)[None, :, None])
        _, _, J2 = passes(PROB, t, [[2.0]], smooth_u(t2)[None, :, None])
        for dtype in (L, np.float64):
            e = xt.estimate(PROB, ts, smooth_u(t)[None, :, None], x, lam, 1e-6, 1e-6, dtype)
            d = float(J[0] - J2[0])
            print(f"N {N} {np.dtype(dtype).name}: errJ {float(e['errJ'][0]):.6e}, J(N) - J(2N) {d:.6e}")
            assert abs(float(e["errJ"][0]) - d) <= 0.2 * abs(d)


def test_float64_twin_is_float64_and_close():
    N = 13
    ts = np.sort(np.concatenate([[0.0, 6.0], np.random.default_rng(1).uniform(0.0, 6.0, N - 1)]))
    t, _ = tw.grid(ts)
    prob = tw.LogisticK([3.0, 2.5], np.array([1.5, 1.7, 1.9]), 0.05)
    u = np.stack([smooth_u(t + s) for s in (0.0, 0.5, 1.0)], axis=1)[None]
    x, lam, _ = passes(prob, ts, np.array([[2.0, 1.0, 0.5], [1.0, 2.0, 0.7]]), u)
    a, b = xt.estimate(prob, ts, u, x, lam, 1e-6, 1e-6, L), xt.estimate(prob, ts, u, x, lam, 1e-6, 1e-6, np.float64)
    for k in ("ex", "el", "rx", "rl", "errJ"):
        assert a[k].dtype == L and b[k].dtype == np.float64, k
    assert float(np.max(np.abs(b["rx"] - a["rx"]) * a["denx"] / a["sx"])) < 64 * tw.EPS
    assert float(np.max(np.abs(b["rl"] - a["rl"]) * a["denl"] / a["sl"])) < 64 * tw.EPS


# ---- the library's side that needs no GPU ----
@pytest.fixture(scope="module")
def pkg():
    import __graft_entry__ as g
    g.build()
    return g.load_package()


def test_new_symbols_are_exported_and_refuse_null_handles(pkg):
    from ocs_amd import _lib
    assert hasattr(_lib.lib, "ocs_x_lam_err") and hasattr(_lib.lib, "ocs_x_lam_err_dev")
    assert callable(pkg.x_lam_error) and callable(pkg.fb_sweep_adaptive_batch)
    one = np.zeros(4)
    dp = one.ctypes.data_as(_lib.dp)
    rc = _lib.lib.ocs_x_lam_err(None, None, 1, dp, dp, dp, 1e-6, 1e-6, None, None, None, dp, dp, dp)
    assert rc == -1                                                          # OCS_ERR_INVALID
    rc = _lib.lib.ocs_x_lam_err_dev(None, None, 1, None, None, 1, None, C.c_double(1e-6), C.c_double(1e-6), None, None, None, None,
                                    None, None, None)
    assert rc == -1


def test_package_refinement_rule_is_the_twins(pkg):
    from ocs_amd import mesh
    rng = np.random.default_rng(5)
    for _ in range(100):
        n = int(rng.integers(1, 40))
        x = np.sort(rng.uniform(0.0, 10.0, n + 1))
        r = 10 ** rng.uniform(-3, 4, n)
        r[rng.uniform(size=n) < 0.1] = 1.0
        r[rng.uniform(size=n) < 0.1] = 32.0
        r[rng.uniform(size=n) < 0.05] = np.nan
        assert np.array_equal(mesh.refine_mesh(x, r, 1, 32), xt.refine(x, r, 1, 32))
