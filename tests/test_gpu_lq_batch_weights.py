"""Per-trajectory cost weights of the linear-quadratic problem (LQProblem.set_batch_weights / set_batch_params on the
weight range of [r | A | Bu | q | rdiag]) on the matrix-core passes of csrc/ocs_lq_kernels.hip, against the CPU oracle:
one oracle.LQProblem(A, Bu, q_b, rdiag_b, ...) per checked trajectory, the tolerance of tests/test_gpu_lq.py (1e-12
relative with its relerr), data from tests.user_problems.lq_matrices, weights q ~ U(0.5, 1.5), rdiag ~ U(1, 2) per (row,
trajectory)."""
import numpy as np
import pytest

from tests.user_problems import lq_matrices

pytestmark = pytest.mark.gpu
RTOL = 1e-12
OCS_ERR_SHAPE, OCS_ERR_UNSUPPORTED = -2, -6
BOUNDS = [-1.0, 1.0]


def relerr(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.max(np.abs(a - b) / np.maximum(1.0, np.abs(b))))


@pytest.fixture(scope="module")
def ocs():
    import torch
    assert torch.cuda.is_available()
    import __graft_entry__ as g
    return g.load_package()


def make(ocs, nS, nC):
    A, Bu, q, rdiag = lq_matrices(nS, nC)
    return ocs.LQProblem(A, Bu, q, rdiag, 0.05, [BOUNDS] * nC), (A, Bu, q, rdiag)


def weights(rng, nS, nC, batch):
    return rng.uniform(0.5, 1.5, (nS, batch)), rng.uniform(1.0, 2.0, (nC, batch))


def oracle_problem(oracle, mats, qb, rb):
    A, Bu = mats[0], mats[1]
    return oracle.LQProblem(A, Bu, qb, rb, 0.05, [BOUNDS] * Bu.shape[1])


def grid(oracle, rng, N, T=1.5):
    return np.concatenate([[0.0], np.sort(rng.uniform(0.0, T, N - 1)), [T]]) if N > 3 else oracle.linspace(0, 0.1, N + 1)


def check_against_oracle(oracle, mats, Q, R, tspan, x0, u, b, x, J, lam, dJdu, lamT=None):
    go = oracle.RK4Integrator(tspan)
    po = oracle_problem(oracle, mats, Q[:, b], R[:, b])
    xo, Jo = go.compute_states(po, x0[:, b], u[:, :, b])
    lamo, do = go.compute_adjoints(po, u[:, :, b]) if lamT is None else go.compute_adjoints(po, u[:, :, b], lamT[:, b])
    errs = (relerr(x[:, :, b], xo), abs(J[b] - Jo) / max(1.0, abs(Jo)), relerr(lam[:, :, b], lamo), relerr(dJdu[:, :, b], do))
    print(f"trajectory {b}: x / J / lam / dJdu {errs}")
    assert max(errs) < RTOL, (b, errs)


@pytest.mark.parametrize("mapping", [0, 1, 2, 3, 4])
@pytest.mark.parametrize("nS,nC,N,batch", [(1, 1, 7, 3), (5, 2, 33, 37), (16, 4, 64, 16), (17, 2, 20, 19), (20, 3, 50, 50),
                                           (32, 4, 96, 68), (32, 1, 3, 1)])
def test_passes_every_mapping(ocs, oracle, nS, nC, N, batch, mapping):
    """The shapes of test_states_adjoints_vs_oracle (every kernel, every tail) with per-trajectory weights: x, J, lam and
    dJdu of trajectories 0, batch // 2 and batch - 1, with the default and with an explicit lamT."""
    pg, mats = make(ocs, nS, nC)
    rng = np.random.default_rng(1000 * N + mapping)
    tspan = grid(oracle, rng, N)
    u = rng.uniform(-1, 1, (nC, 2 * N + 1, batch))
    x0 = rng.normal(size=(nS, batch))
    lamT = rng.normal(size=(nS + 1, batch))
    Q, R = weights(rng, nS, nC, batch)
    pg.set_batch_weights(Q, R)
    g = ocs.RK4Integrator(tspan)
    g.set_mapping(mapping)
    x, J = g.compute_states(pg, x0, u)
    lam, dJdu = g.compute_adjoints(pg, u)
    x2, J2 = g.compute_states(pg, x0, u)
    lam2, d2 = g.compute_adjoints(pg, u, lamT)
    for b in sorted({0, batch // 2, batch - 1}):
        check_against_oracle(oracle, mats, Q, R, tspan, x0, u, b, x, J, lam, dJdu)
        assert np.all(lam[-1, :, b] == 1.0)
        check_against_oracle(oracle, mats, Q, R, tspan, x0, u, b, x2, J2, lam2, d2, lamT)


@pytest.mark.parametrize("nS,nC,N,batch,mapping", [(20, 3, 50, 50, 1), (20, 3, 50, 50, 2), (20, 3, 50, 50, 3),
                                                   (12, 2, 256, 100, 0)])
def test_the_right_column_is_read(ocs, oracle, nS, nC, N, batch, mapping):
    """A trajectory in the middle of a wave and the last one of a ragged batch get all-zero weights: their J, their state
    rows of lam (default lamT) and their dJdu are exactly 0.0, their neighbours match the oracle and are not zero.
    (12, 2, 256, 100) on the automatic mapping runs the time-parallel chunked passes."""
    pg, mats = make(ocs, nS, nC)
    rng = np.random.default_rng(N + batch + mapping)
    tspan = grid(oracle, rng, N, 2.0)
    u = rng.uniform(-1, 1, (nC, 2 * N + 1, batch))
    x0 = rng.normal(size=(nS, batch))
    Q, R = weights(rng, nS, nC, batch)
    zeros = (21, batch - 1)   # lane 5 of the second group of 16; the last trajectory of the ragged last group
    for b in zeros:
        Q[:, b] = 0.0
        R[:, b] = 0.0
    pg.set_batch_weights(Q, R)
    g = ocs.RK4Integrator(tspan)
    g.set_mapping(mapping)
    x, J = g.compute_states(pg, x0, u)
    lam, dJdu = g.compute_adjoints(pg, u)
    if mapping == 0:   # the chunked kernels ran, not the serial ones: equal to round-off, not bit for bit
        gs = ocs.RK4Integrator(tspan).set_mapping(1)
        xs, _ = gs.compute_states(pg, x0, u)
        assert relerr(x, xs) < RTOL and not np.array_equal(x, xs)
    for b in zeros:
        assert J[b] == 0.0 and np.all(x[nS, :, b] == 0.0)
        assert np.all(lam[:nS, :, b] == 0.0) and np.all(lam[nS, :, b] == 1.0)
        assert np.all(dJdu[:, :, b] == 0.0)
    for b in (zeros[0] - 1, zeros[0] + 1, zeros[1] - 1):
        check_against_oracle(oracle, mats, Q, R, tspan, x0, u, b, x, J, lam, dJdu)
        assert J[b] != 0.0 and np.all(lam[:nS, 0, b] != 0.0) and np.any(dJdu[:, :, b] != 0.0)


@pytest.mark.parametrize("nS,nC,N,batch", [(5, 2, 33, 37), (20, 3, 50, 50)])
def test_partial_override(ocs, oracle, nS, nC, N, batch):
    """Only q[1] and rdiag[nC - 1] per trajectory, through raw set_batch_params indices; the rest from the shared block."""
    pg, mats = make(ocs, nS, nC)
    rng = np.random.default_rng(N)
    tspan = grid(oracle, rng, N)
    u = rng.uniform(-1, 1, (nC, 2 * N + 1, batch))
    x0 = rng.normal(size=(nS, batch))
    Q = np.repeat(mats[2][:, None], batch, axis=1)
    R = np.repeat(mats[3][:, None], batch, axis=1)
    Q[1], R[nC - 1] = rng.uniform(0.5, 1.5, batch), rng.uniform(1.0, 2.0, batch)
    w0 = 1 + nS * nS + nS * nC
    pg.set_batch_params([w0 + nS + nC - 1, w0 + 1], np.stack([R[nC - 1], Q[1]]))
    g = ocs.RK4Integrator(tspan)
    x, J = g.compute_states(pg, x0, u)
    lam, dJdu = g.compute_adjoints(pg, u)
    for b in sorted({0, batch // 2, batch - 1}):
        check_against_oracle(oracle, mats, Q, R, tspan, x0, u, b, x, J, lam, dJdu)


def test_clear_and_batch_mismatch(ocs, oracle):
    """set_batch_weights() with no arguments restores the shared-weight results bit for bit; a call whose batch differs from the
    batch the weights were set for fails with OCS_ERR_SHAPE."""
    nS, nC, N, batch = 20, 3, 50, 50
    pg, mats = make(ocs, nS, nC)
    rng = np.random.default_rng(3)
    tspan = grid(oracle, rng, N)
    u = rng.uniform(-1, 1, (nC, 2 * N + 1, batch))
    x0 = rng.normal(size=(nS, batch))
    g = ocs.RK4Integrator(tspan)
    x, J = g.compute_states(pg, x0, u)
    lam, dJdu = g.compute_adjoints(pg, u)
    Q, R = weights(rng, nS, nC, batch)
    pg.set_batch_weights(Q, R)
    xw, Jw = g.compute_states(pg, x0, u)
    assert not np.array_equal(J, Jw) and relerr(x[:nS], xw[:nS]) < RTOL   # the state rows do not read the weights
    with pytest.raises(Exception) as ei:
        g.compute_states(pg, x0[:, :batch - 1], u[:, :, :batch - 1])
    assert getattr(ei.value, "code", None) == OCS_ERR_SHAPE
    pg.set_batch_weights()
    xc, Jc = g.compute_states(pg, x0, u)
    lamc, dc = g.compute_adjoints(pg, u)
    assert np.array_equal(x, xc) and np.array_equal(J, Jc) and np.array_equal(lam, lamc) and np.array_equal(dJdu, dc)
    g.compute_states(pg, x0[:, :batch - 1], u[:, :, :batch - 1])   # any batch again


@pytest.mark.parametrize("mapping", [0, 1])
def test_infinite_horizon_and_shooting_objective(ocs, oracle, mapping):
    """The second half of test_infinite_horizon_and_shooting_objective (tests/test_gpu_lq.py) with weights and uStar != 0:
    RK4InfiniteIntegrator (both legs, the tail's constant-control kernels), then nlp_objective through a PWLinear basis with
    free initial states on 5 candidates (the weights set again for that batch)."""
    nS, nC, N, batch = 32, 4, 80, 40
    pg, mats = make(ocs, nS, nC)
    tspan, tx = oracle.linspace(0, 1, N + 1), oracle.linspace(1, 2, N // 2 + 1)
    rng = np.random.default_rng(5 + mapping)
    u = rng.uniform(-1, 1, (nC, 2 * N + 1, batch))
    x0 = rng.normal(size=(nS, batch))
    ustar = np.array([0.1, -0.2, 0.05, 0.3])
    Q, R = weights(rng, nS, nC, batch)
    pg.set_batch_weights(Q, R)
    gi, go = ocs.RK4InfiniteIntegrator(tspan, tx, ustar), oracle.RK4InfiniteIntegrator(tspan, tx, ustar)
    gi.set_mapping(mapping)
    x, J = gi.compute_states(pg, x0, u)
    lam, dJdu = gi.compute_adjoints(pg, u)
    for b in (0, 17, 39):
        po = oracle_problem(oracle, mats, Q[:, b], R[:, b])
        xo, Jo = go.compute_states(po, x0[:, b], u[:, :, b])
        lamo, do = go.compute_adjoints(po, u[:, :, b])
        errs = (relerr(x[:, :, b], xo), abs(J[b] - Jo) / max(1.0, abs(Jo)), relerr(lam[:, :, b], lamo), relerr(dJdu[:, :, b], do))
        print(f"infinite horizon, trajectory {b}: x / J / lam / dJdu {errs}")
        assert max(errs) < RTOL
    cg, co = ocs.PWLinearControl(gi.t, 9, nC), oracle.PWLinearControl(go.t, 9, nC)
    V = rng.uniform(-1, 1, (nC * 9 + 2, 5))
    free = [3, 30]
    pg.set_batch_weights(Q[:, 10:15], R[:, 10:15])
    Jn, dJdv, _ = ocs.nlp_objective(gi, pg, cg, x0[:, :5], V, free)
    for b in range(5):
        po = oracle_problem(oracle, mats, Q[:, 10 + b], R[:, 10 + b])
        Jo, do, _ = oracle.nlp_objective(go, po, co, x0[:, b], V[:, b], free)
        errs = (abs(Jn[b] - Jo) / max(1.0, abs(Jo)), relerr(dJdv[:, b], do))
        print(f"nlp_objective, candidate {b}: J / dJdv {errs}")
        assert max(errs) < RTOL


def test_single_shooting_batch_instances_are_independent(ocs):
    """single_shooting_batch with per-instance weights: instance b equals instance b of the same driver run on a shared-weight
    problem built from b's weights (same batch size, same start), b = 0 and 5 -- J[b] and v[:, b] to RTOL scaled by
    max(1, |.|), equal iteration counts.  MaxIter = 6 (fixed and small: the comparison is of the same iterates; both runs
    execute the same time loops on the same register values, the weights only come from another prologue load)."""
    nS, nC, N, batch = 8, 2, 60, 6
    pg, mats = make(ocs, nS, nC)
    rng = np.random.default_rng(8)
    tspan = np.linspace(0.0, 2.0, N + 1)
    x0 = rng.normal(size=(nS, batch))
    Q, R = weights(rng, nS, nC, batch)
    pg.set_batch_weights(Q, R)
    kw = dict(u0=0.2, TolFun=1e-12, TolX=1e-14, MaxIter=6)
    r = ocs.single_shooting_batch(pg, x0, tspan, 7, **kw)
    J, v, it = r["J"].cpu().numpy(), r["v"].cpu().numpy(), r["iterations"].cpu().numpy()
    assert len(set(np.round(J, 9))) == batch   # the instances differ
    for b in (0, 5):
        ps = ocs.LQProblem(mats[0], mats[1], Q[:, b], R[:, b], 0.05, [BOUNDS] * nC)
        rs = ocs.single_shooting_batch(ps, x0, tspan, 7, **kw)
        Js, vs, its = rs["J"].cpu().numpy(), rs["v"].cpu().numpy(), rs["iterations"].cpu().numpy()
        errs = (abs(J[b] - Js[b]) / max(1.0, abs(Js[b])), relerr(v[:, b], vs[:, b]))
        print(f"driver, instance {b}: J / v {errs}, iterations {it[b]} / {its[b]}")
        assert max(errs) < RTOL and it[b] == its[b] and it[b] > 0


def test_refusals_that_stay(ocs, oracle):
    """With weights set at nS = 8: the sweep entry points, compute_x_lam and ControlChar refuse with their "per-trajectory
    parameters" messages, the plugin methods refuse, and an index of A is still refused at this size."""
    nS, nC, N, batch = 8, 2, 40, 3
    pg, _ = make(ocs, nS, nC)
    rng = np.random.default_rng(1)
    Q, R = weights(rng, nS, nC, batch)
    pg.set_batch_weights(Q, R)
    tspan = oracle.linspace(0, 2.0, N + 1)
    X0 = rng.normal(size=(nS, batch))
    k = 4
    t, y = rng.uniform(0, 2, k), rng.normal(size=(nS + 1, k))
    uu, v = rng.uniform(-1, 1, (nC, k)), rng.normal(size=(nS + 1, k))
    calls = {
        "fb_sweep_batch": lambda: ocs.fb_sweep_batch(pg, X0, tspan, {"nERROR_PTS": N + 1, "nINTERP_PTS": 21, "nSWEEPS": 3}),
        "compute_x_lam": lambda: ocs.compute_x_lam(pg, X0, tspan, np.zeros((nC, 2 * N + 1, batch))),
        "ControlChar": lambda: pg.ControlChar(t, y[:nS], v[:nS]),
    }
    for name, call in calls.items():
        with pytest.raises(Exception) as ei:
            call()
        assert getattr(ei.value, "code", None) == OCS_ERR_UNSUPPORTED and "per-trajectory parameters" in str(ei.value), name
    for call in (lambda: pg.F(t, y, uu), lambda: pg.dFdx_times_vec(t, y, uu, v), lambda: pg.dFdu_times_vec(t, y, uu, v)):
        with pytest.raises(Exception) as ei:
            call()
        assert getattr(ei.value, "code", None) == OCS_ERR_UNSUPPORTED
    with pytest.raises(Exception) as ei:
        pg.set_batch_params([1], np.full((1, batch), -1.0))   # A(1,1)
    assert getattr(ei.value, "code", None) == OCS_ERR_UNSUPPORTED
    w0 = 1 + nS * nS + nS * nC
    with pytest.raises(Exception) as ei:
        pg.set_batch_params([w0, 1], np.full((2, batch), 1.0))   # a weight together with an entry of A
    assert getattr(ei.value, "code", None) == OCS_ERR_UNSUPPORTED
    # the refused calls left the weights in place; cleared, the plugin methods work again
    g = ocs.RK4Integrator(tspan)
    _, Jw = g.compute_states(pg, X0, np.zeros((nC, 2 * N + 1, batch)))
    pg.set_batch_weights()
    _, Js = g.compute_states(pg, X0, np.zeros((nC, 2 * N + 1, batch)))
    assert not np.array_equal(Jw, Js)
    assert np.all(np.isfinite(pg.F(t, y, uu)))
