"""GPU tests of ocs_x_lam_err (k_xlam_err and its reduction) against tests/xlam_err_twin.py.

fine - coarse cancels, so errors are measured where the cancellation happens: a ratio is multiplied back by its (smallest)
denominator and divided by the scale of its rows, s_i = max_k max(|v_{i,k}|, |v_{i+1,k}|), which leaves the error of
16/15 |fine - coarse| in units of the values it was formed from.  The statement is the one of tests/accuracy_check.py with the
float64 twin in the oracle's place, per case (a grid, a batch, a problem):

    max_i,b |r_device - r_longdouble| den / s  <=  K max(max_i,b |r_float64twin - r_longdouble| den / s, 8 eps),   K = 8

K = 8 and the floor 8 eps are what tests/test_gpu_rk4_accuracy.py allows its mappings for FMA contraction and another order of
the same operations; neither is fitted to this kernel.  errJ the same way on the scale |J| + sum_i |lam_{i+1}|' |x_{i+1}|."""
import numpy as np
import pytest

from tests import rk4_twin as tw
from tests import xlam_err_twin as xt
from tests.accuracy_check import FLOOR, K

pytestmark = pytest.mark.gpu
L = np.longdouble
RTOL = ATOL = 1e-6
BOUNDS = [[0.0, 1.0]]
M = [3.0, 2.5, 2.0, 3.5]


@pytest.fixture(scope="module")
def ocs():
    import torch
    assert torch.cuda.is_available()
    import __graft_entry__ as g
    return g.load_package()


def grid_of(N):
    if N == 1:
        return np.array([0.0, 0.7])
    if N == 2:
        return np.array([0.0, 0.5, 1.2])
    if N == 13:      # non-uniform: steps between 0.12 and 0.5 (RK4 on x (3 - x) stays stable)
        ts = np.linspace(0.0, 4.0, N + 1)
        ts[1:-1] += np.random.default_rng(13).uniform(-0.3, 0.3, N - 1) * (4.0 / N)
        return ts
    return np.linspace(0.0, 4.0, N + 1)


def inputs(nS, nC, ts, batch):
    """x0 [nS][B] and ugrid [nC][2N+1][B], different for every instance; the control has extrema and flat pieces (clamped)"""
    t, _ = tw.grid(ts)
    b = np.arange(batch)
    x0 = 0.5 + 2.0 * ((b[None, :] * 0.37 + np.arange(nS)[:, None] * 0.21) % 1.0)
    u = 0.4 + 0.45 * np.sin(1.3 * t[None, :, None] + 0.3 * b[None, None, :] + np.arange(nC)[:, None, None])
    return x0, np.clip(u, 0.0, 0.75)


def check(ocs, what, dev, twin, ts, x0, ug):
    """the device's estimate of its own compute_x_lam under ug against the twins' estimates of the same x, lam"""
    x, lam, J = ocs.compute_x_lam_J(dev, x0, ts, ug)
    got = ocs.x_lam_error(dev, ts, ug, x, lam, RTOL, ATOL)
    ld = xt.estimate(twin, ts, ug, x, lam, RTOL, ATOL, L)
    f64 = xt.estimate(twin, ts, ug, x, lam, RTOL, ATOL, np.float64)
    worst = {}
    for k, s in (("rx", "x"), ("rl", "l")):
        unit = ld["den" + s] / ld["s" + s]
        e = float(np.max(np.abs(got[k].astype(L) - ld[k]) * unit))
        yard = max(float(np.max(np.abs(f64[k].astype(L) - ld[k]) * unit)), FLOOR)
        worst[k] = e / yard
        assert e <= K * yard, (what, k, e / yard)
    sJ = np.abs(J) + np.sum(np.abs(lam[:, 1:] * x[:, 1:]), axis=(0, 1))
    e = float(np.max(np.abs(got["errJ"].astype(L) - ld["errJ"]) / sJ))
    yard = max(float(np.max(np.abs(f64["errJ"].astype(L) - ld["errJ"]) / sJ)), FLOOR)
    worst["errJ"] = e / yard
    assert e <= K * yard, (what, "errJ", e / yard)
    print(f"ACCURACY xlam_err {what}: err / max(err_twin, 8 eps) " + " ".join(f"{k}={v:.2f}" for k, v in worst.items()) +
          f"; ratios up to {np.nanmax(got['rx']):.2e} / {np.nanmax(got['rl']):.2e}")
    rmax, rinst = xt.reductions(got["rx"], got["rl"])
    assert np.array_equal(got["rmax"], rmax) and np.array_equal(got["rinst"], rinst)
    return got, x, lam


@pytest.mark.parametrize("nS", [1, 2, 4])
def test_logistic_family_against_the_longdouble_twin(ocs, nS):
    """N = 1 (pchip of two nodes is linear), 2 (the three-point end rule on both sides), 8 and 9 (one chunk, one chunk plus
    one), 13 (non-uniform) at batch 1, 64, 69"""
    dev = ocs.LogisticProblem(M[:nS], 1.5, 0.05, BOUNDS)
    twin = tw.LogisticK(M[:nS], 1.5, 0.05)
    for N in (1, 2, 8, 9, 13):
        for batch in (1, 64, 69):
            ts = grid_of(N)
            x0, ug = inputs(nS, 1, ts, batch)
            check(ocs, f"logistic{nS} N {N} batch {batch}", dev, twin, ts, x0, ug)


def test_per_trajectory_parameters_and_bounds(ocs):
    """c of its own per trajectory reaches the estimate (the cost row and with it errJ); per-trajectory bounds are not the
    estimate's business (it never calls ControlChar) and must not disturb it"""
    batch, ts = 69, grid_of(13)
    cs = 1.0 + (np.arange(batch) % 7) / 7.0
    x0, ug = inputs(2, 1, ts, batch)
    dev = ocs.LogisticProblem(M[:2], 1.5, 0.05, BOUNDS)
    dev.set_batch_params([0], cs[None, :])
    got, x, lam = check(ocs, "per-trajectory c", dev, tw.LogisticK(M[:2], cs, 0.05), ts, x0, ug)
    shared = ocs.x_lam_error(ocs.LogisticProblem(M[:2], 1.5, 0.05, BOUNDS), ts, ug, x, lam, RTOL, ATOL)
    assert not np.array_equal(shared["errJ"], got["errJ"])
    dev.set_batch_bounds(lb=np.full((1, batch), 0.1), ub=np.linspace(0.5, 1.0, batch)[None, :])
    again = ocs.x_lam_error(dev, ts, ug, x, lam, RTOL, ATOL)
    for k in got:
        assert np.array_equal(again[k], got[k], equal_nan=True), k


def test_plugin(ocs):
    """one hipRTC plugin, nS = 2, nC = 2: the LQ problem as device source, against the twin's LQ"""
    from tests.user_problems import lq_matrices, lq_source
    A, Bu, q, rd = lq_matrices(2, 2)
    par = np.concatenate([[0.05], A.ravel(order="F"), Bu.ravel(order="F"), q, rd])
    dev = ocs.UserProblem(lq_source(2, 2), 2, 2, par, [[-5.0, 5.0], [-5.0, 5.0]])
    twin = tw.LQ(A, Bu, q, rd, 0.05)
    for N, batch in ((2, 1), (9, 69), (13, 64)):
        ts = 0.1 * grid_of(N)        # (the faster eigenvalue of A is -31.6: steps of at most 0.05)
        x0, ug = inputs(2, 2, ts, batch)
        check(ocs, f"plugin N {N} batch {batch}", dev, twin, ts, x0, ug)


def check_reductions(ocs, batch, ts, bad, at):
    """`use` masks rmax but not rinst; a NaN planted in x of instance `bad` at node `at` gives inf in its rinst and, where it is in
    use, in rmax, and leaves every other instance's numbers bit-identical; two calls give equal bits"""
    N = ts.size - 1
    dev = ocs.LogisticProblem(M[:2], 1.5, 0.05, BOUNDS)
    x0, ug = inputs(2, 1, ts, batch)
    res, x, lam = check(ocs, "reductions", dev, tw.LogisticK(M[:2], 1.5, 0.05), ts, x0, ug)
    again = ocs.x_lam_error(dev, ts, ug, x, lam, RTOL, ATOL)
    for k in res:
        assert np.array_equal(res[k], again[k]), k
    use = np.arange(batch) % 3 == 1
    masked = ocs.x_lam_error(dev, ts, ug, x, lam, RTOL, ATOL, use=use)
    assert np.array_equal(masked["rinst"], res["rinst"]) and np.array_equal(masked["errJ"], res["errJ"])
    assert np.array_equal(masked["rmax"], xt.reductions(res["rx"], res["rl"], use)[0])
    assert not np.array_equal(masked["rmax"], res["rmax"])
    none = ocs.x_lam_error(dev, ts, ug, x, lam, RTOL, ATOL, use=np.zeros(batch))
    assert (none["rmax"] == 0).all() and np.array_equal(none["rinst"], res["rinst"])
    xn = x.copy()
    xn[1, at, bad] = np.nan
    nan = ocs.x_lam_error(dev, ts, ug, xn, lam, RTOL, ATOL)
    others = np.arange(batch) != bad
    for k in ("rx", "rl"):
        assert np.array_equal(nan[k][:, others], res[k][:, others]), k
    assert np.array_equal(nan["rinst"][others], res["rinst"][others]) and np.array_equal(nan["errJ"][others], res["errJ"][others])
    assert nan["rinst"][bad] == np.inf and np.isnan(nan["rx"][at, bad])
    assert np.isinf(nan["rmax"][at - 1:at + 1]).all()
    keep = np.ones(N, dtype=bool)
    keep[max(at - 3, 0):at + 3] = False                    # (the pchip slopes of x reach two nodes to either side)
    assert np.array_equal(nan["rmax"][keep], res["rmax"][keep])
    out = ocs.x_lam_error(dev, ts, ug, xn, lam, RTOL, ATOL, use=others)
    assert np.array_equal(out["rmax"], xt.reductions(res["rx"], res["rl"], others)[0]) and out["rinst"][bad] == np.inf
    return dev, ug, x, lam, res


def test_reductions_past_one_stride(ocs):
    """batch 321 = 256 + 64 + 1, N 9: the row loop's second stride and the second workgroup of the per-instance half with its
    partly filled last wave; two chunks, the second a one-interval tail.  The NaN in instance 300 (second stride) at node 8:
    intervals 7 and 8, one in either chunk."""
    check_reductions(ocs, 321, grid_of(9), 300, 8)


def test_reductions_masks_nan_and_bits(ocs):
    """batch 69, N 13; the NaN at node 9: intervals 8 and 9 (chunk 1), instance in the wave tail; then: _dev and host agree bit
    for bit"""
    import torch
    from ocs_amd import _lib
    from ocs_amd.integrator import _dptr
    batch, ts = 69, grid_of(13)
    N = ts.size - 1
    dev, ug, x, lam, res = check_reductions(ocs, batch, ts, 66, 9)
    # the device entry point on the arrays of ocs_compute_x_lam_dev's shapes (x with the cost row, ldx = nS + 1)
    gi = ocs.RK4Integrator(ts)
    cu = lambda a: torch.tensor(np.ascontiguousarray(a), dtype=torch.float64, device="cuda")
    xa = np.concatenate([x, np.zeros((1, N + 1, batch))])
    du, dx, dl = cu(ug.transpose(1, 0, 2)), cu(xa.transpose(1, 0, 2)), cu(lam.transpose(1, 0, 2))
    rx, rl = torch.empty((N, batch), dtype=torch.float64, device="cuda"), torch.empty((N, batch), dtype=torch.float64, device="cuda")
    rmax, rinst, errJ = (torch.empty(n, dtype=torch.float64, device="cuda") for n in (N, batch, batch))
    rc = _lib.lib.ocs_x_lam_err_dev(gi._h, dev._h, batch, _dptr(du), _dptr(dx), 3, _dptr(dl), RTOL, ATOL, None, _dptr(rx), _dptr(rl),
                                    _dptr(rmax), _dptr(rinst), _dptr(errJ), None)
    assert rc == 0
    torch.cuda.synchronize()
    for k, v in (("rx", rx), ("rl", rl), ("rmax", rmax), ("rinst", rinst), ("errJ", errJ)):
        assert np.array_equal(v.cpu().numpy(), res[k]), k
    rmax2, rinst2, errJ2 = (torch.empty(n, dtype=torch.float64, device="cuda") for n in (N, batch, batch))
    rc = _lib.lib.ocs_x_lam_err_dev(gi._h, dev._h, batch, _dptr(du), _dptr(dx), 3, _dptr(dl), RTOL, ATOL, None, None, None,
                                    _dptr(rmax2), _dptr(rinst2), _dptr(errJ2), None)
    assert rc == 0
    torch.cuda.synchronize()
    assert torch.equal(rmax2, rmax) and torch.equal(rinst2, rinst) and torch.equal(errJ2, errJ)


def test_refusals(ocs):
    """LQ, a larger plugin, an RK4InfiniteIntegrator handle and the tiled layout: OCS_ERR_UNSUPPORTED; bad tolerances:
    OCS_ERR_INVALID"""
    from tests.user_problems import lq_matrices, lq_source
    ts = grid_of(9)
    A, Bu, q, rd = lq_matrices(6, 1)
    big = [ocs.LQProblem(A, Bu, q, rd, 0.05, [[-5.0, 5.0]]),
           ocs.UserProblem(lq_source(6, 1), 6, 1, np.concatenate([[0.05], A.ravel(order="F"), Bu.ravel(order="F"), q, rd]), [[-5.0, 5.0]])]
    pr = ocs.TestOCProblem({"c": 1.5, "m": 3.0, "r": 0.05}, BOUNDS)
    calls = [(p, ocs.RK4Integrator(ts)) for p in big]
    calls.append((pr, ocs.RK4Integrator(ts).set_layout("tiled")))
    calls.append((pr, ocs.RK4InfiniteIntegrator(ts, np.linspace(ts[-1], ts[-1] + 2, 5), [0.4])))
    for p, gi in calls:
        n = gi.nSTEPS
        with pytest.raises(ocs.OcsError) as e:
            ocs.x_lam_error(p, gi.tspan, np.full((p.nC, 2 * n + 1, 4), 0.3), np.ones((p.nS, n + 1, 4)), np.ones((p.nS, n + 1, 4)), RTOL,
                            ATOL, integrator=gi)
        assert e.value.code == -6, e.value
    for rt, at in ((-1e-6, 1e-6), (1e-6, -1e-6), (0.0, 0.0), (np.nan, 1e-6)):
        with pytest.raises(ocs.OcsError) as e:
            ocs.x_lam_error(pr, ts, np.full((1, 19, 4), 0.3), np.ones((1, 10, 4)), np.ones((1, 10, 4)), rt, at)
        assert e.value.code == -1, e.value
    ok = ocs.x_lam_error(pr, ts, np.full((1, 19, 4), 0.3), np.ones((1, 10, 4)), np.ones((1, 10, 4)), 0.0, 1e-6)
    assert np.isfinite(ok["rmax"]).all()
