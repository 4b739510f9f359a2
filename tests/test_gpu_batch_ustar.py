"""A constant tail control uStar of its own per trajectory on RK4InfiniteIntegrator (RK4InfiniteIntegrator.set_batch_uStar,
ocs_rk4inf_set_batch_ustar[_dev]) on every path the tail leg takes, against the CPU oracle run once per checked trajectory:
oracle.RK4InfiniteIntegrator(tspan, tx, U[:, b]).  RTOL and relerr are those of tests/test_gpu_lq.py and
tests/test_gpu_batch_params.py.

Which case runs which tail path:

    wave-specialised tail on samples (launch_fill_rows)   logistic (2, 64, 64, 96) and (4, 48, 40, 32) on "auto"; split at N2 = 60
    lane kernels k_forward / k_backward<UCONST>           logistic (2, 64, 64, 70) on "auto" (ragged batch), every shape on "lane"
    hipRTC UK_FWD_UCONST / UK_BWD_UCONST                  test_hiprtc_plugin
    LQ one- / two- / four-wave kernels, UCONST            test_lq_matrix_cores, mappings 0 to 3 at N2 = 40
    LQ chunked tail (pass Z over the real batch)          test_lq_matrix_cores mapping 4; test_lq_chunked_tail_on_auto
"""
import ctypes as C

import numpy as np
import pytest

from tests.user_problems import LOGISTIC2_SRC, lq_matrices

pytestmark = pytest.mark.gpu
P = {"c": 1.5, "m": 3.0, "r": 0.05}
BOUNDS = [[0.0, 1.0]]
LQ_BOUNDS = [-1.0, 1.0]
RTOL = 1e-12
OCS_ERR_INVALID, OCS_ERR_SHAPE = -1, -2
_REF = {}   # oracle references shared by the cases that use a shape (computed once, never written again)


def relerr(a, b):
    """max |a-b| / max(1,|b|) (tests/test_gpu_lq.py)"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    e = np.abs(a - b) / np.maximum(1.0, np.abs(b))
    return float("inf") if np.isnan(e).any() else float(np.max(e))


@pytest.fixture(scope="module")
def ocs():
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    import __graft_entry__ as g
    return g.load_package()


def run(g, pg, x0, u):
    x, J = g.compute_states(pg, x0, u)
    lam, dJdu = g.compute_adjoints(pg, u)
    return x, J, lam, dJdu


def same(a, b):
    return all(np.array_equal(p, q) for p, q in zip(a, b))


def oracle_ref(oracle, make, tspan, tx, U, x0, u, which):
    """x, J, lam, dJdu of the trajectories `which`, trajectory b on make(b) under ITS uStar U[:, b]"""
    out = {}
    for b in which:
        go, po = oracle.RK4InfiniteIntegrator(tspan, tx, U[:, b]), make(b)
        xo, Jo = go.compute_states(po, x0[:, b], u[:, :, b])
        lamo, do = go.compute_adjoints(po, u[:, :, b])
        out[b] = (xo, Jo, lamo, do)
    return out


def check(res, ref, what=""):
    x, J, lam, dJdu = res
    worst = 0.0
    for b, (xo, Jo, lamo, do) in ref.items():
        errs = (relerr(x[:, :, b], xo), abs(J[b] - Jo) / max(1.0, abs(Jo)), relerr(lam[:, :, b], lamo), relerr(dJdu[:, :, b], do))
        worst = max(worst, *errs)
        assert max(errs) < RTOL, (what, b, errs)
    print(what, "worst x / J / lam / dJdu error over", len(ref), "trajectories:", worst)


# ---- logistic problems ----------------------------------------------------------------------------------------------
LOGISTIC_SHAPES = [(2, 64, 64, 96), (2, 64, 60, 96), (2, 64, 64, 70), (4, 48, 40, 32)]
M0 = [3.0, 2.5, 2.0, 1.5]


def logistic_case(oracle, nS, N, N2, batch, special=False):
    """Inputs of test_infinite_integrator (tests/test_gpu_batch_params.py): c and every m_k per trajectory, plus
    uStar_b ~ U(0.05, 0.45).  special: trajectory 21 and the last one get 0.66 and 0.9, at least 0.2 away from all others."""
    key = ("logistic", nS, N, N2, batch, special)
    if key not in _REF:
        tspan, tx = oracle.linspace(0, 2.0, N + 1), oracle.linspace(2.0, 4.0, N2 + 1)
        rng = np.random.default_rng(N + N2 + batch)
        u = rng.uniform(0.05, 0.45, (1, 2 * N + 1, batch))
        x0 = rng.uniform(0.8, 2.0, (nS, batch))
        r2 = np.random.default_rng(N2 + batch)
        cs, ms = r2.uniform(1.0, 2.0, batch), r2.uniform(1.5, 3.0, (nS, batch))
        U = np.random.default_rng(7 * N2 + batch).uniform(0.05, 0.45, (1, batch))
        if special:
            U[0, 21], U[0, batch - 1] = 0.66, 0.9
        make = lambda b: oracle.LogisticProblem(ms[:, b], cs[b], P["r"], BOUNDS)
        which = (20, 21, 22, batch - 2, batch - 1) if special else range(batch)
        _REF[key] = (tspan, tx, x0, u, cs, ms, U, oracle_ref(oracle, make, tspan, tx, U, x0, u, which))
    return _REF[key]


def logistic_problem(ocs, nS, cs, ms):
    pg = ocs.LogisticProblem(M0[:nS], P["c"], P["r"], BOUNDS)
    index = [2 + nS - 1, 0] + list(range(2, 2 + nS - 1))   # unsorted, as _set_c_and_m of tests/test_gpu_batch_params.py
    pg.set_batch_params(index, np.vstack([ms[nS - 1], cs] + [ms[k] for k in range(nS - 1)]))
    return pg


@pytest.mark.parametrize("mapping", ["auto", "lane"])
@pytest.mark.parametrize("nS,N,N2,batch", LOGISTIC_SHAPES)
def test_logistic_every_tail_path(ocs, oracle, nS, N, N2, batch, mapping):
    """The shapes of test_infinite_integrator -- wave tail, split tail (N2 = 60), ragged batch 70 on the lane kernels,
    four states -- with c, every m_k and uStar per trajectory: x, J, lam and dJdu of EVERY trajectory against the oracle
    under that trajectory's uStar, on the automatic mapping and on set_mapping(1)."""
    tspan, tx, x0, u, cs, ms, U, ref = logistic_case(oracle, nS, N, N2, batch)
    pg = logistic_problem(ocs, nS, cs, ms)
    gi = ocs.RK4InfiniteIntegrator(tspan, tx, [0.4]).set_mapping(mapping)
    gi.set_batch_uStar(U)
    check(run(gi, pg, x0, u), ref, f"logistic {(nS, N, N2, batch)} {mapping}")


def test_hiprtc_plugin(ocs, oracle):
    """LOGISTIC2_SRC (hand-written full-vector methods, params [c, r, m1, m2]; tests/user_problems.py) with c, m1, m2 and
    uStar per trajectory at (2, 64, 64, 70): the tail leg runs the hipRTC instantiations UK_FWD_UCONST / UK_BWD_UCONST of the
    lane kernels (70 is no whole tile of the vector mappings) -- every trajectory against the oracle, "auto" and "lane"."""
    nS, N, N2, batch = 2, 64, 64, 70
    tspan, tx, x0, u, cs, ms, U, ref = logistic_case(oracle, nS, N, N2, batch)
    pu = ocs.UserProblem(LOGISTIC2_SRC, 2, 1, [P["c"], P["r"], 3.0, 2.5], BOUNDS)
    pu.set_batch_params([3, 0, 2], np.vstack([ms[1], cs, ms[0]]))
    for mapping in ("auto", "lane"):
        gi = ocs.RK4InfiniteIntegrator(tspan, tx, U).set_mapping(mapping)   # the constructor takes nC x B directly
        assert gi.uStar.shape == (1, batch)
        check(run(gi, pu, x0, u), ref, f"hipRTC logistic2 {mapping}")


# ---- LQ problem on the matrix cores ---------------------------------------------------------------------------------
def lq_case(oracle, nS, nC, N, N2, batch, which, special=False, seed=0):
    """tests/test_gpu_lq_batch_weights.py's data (lq_matrices, q ~ U(0.5, 1.5), rdiag ~ U(1, 2) per trajectory) and
    uStar nC x batch ~ U(-0.3, 0.3); special: trajectory 21 and the last one at +0.55 and -0.55 in every row (0.25 away)."""
    key = ("lq", nS, nC, N, N2, batch, tuple(which), special, seed)
    if key not in _REF:
        mats = lq_matrices(nS, nC)
        tspan, tx = oracle.linspace(0, 1, N + 1), oracle.linspace(1, 2, N2 + 1)
        rng = np.random.default_rng(100 * nS + N2 + batch + seed)
        u = rng.uniform(-1, 1, (nC, 2 * N + 1, batch))
        x0 = rng.normal(size=(nS, batch))
        Q, R = rng.uniform(0.5, 1.5, (nS, batch)), rng.uniform(1.0, 2.0, (nC, batch))
        U = rng.uniform(-0.3, 0.3, (nC, batch))
        if special:
            U[:, 21], U[:, batch - 1] = 0.55, -0.55
        make = lambda b: oracle.LQProblem(mats[0], mats[1], Q[:, b], R[:, b], 0.05, [LQ_BOUNDS] * nC)
        _REF[key] = (mats, tspan, tx, x0, u, Q, R, U, oracle_ref(oracle, make, tspan, tx, U, x0, u, which))
    return _REF[key]


def lq_problem(ocs, mats, nC, Q, R):
    pg = ocs.LQProblem(mats[0], mats[1], mats[2], mats[3], 0.05, [LQ_BOUNDS] * nC)
    pg.set_batch_weights(Q, R)
    return pg


@pytest.mark.parametrize("mapping", [0, 1, 2, 3, 4])
@pytest.mark.parametrize("nS,nC", [(5, 2), (17, 2), (32, 4)])
def test_lq_matrix_cores(ocs, oracle, nS, nC, mapping):
    """N = 80, N2 = 40, batch = 40 (a ragged last group of 16): one-wave, two-wave and four-wave kernels and, on mapping 4,
    the chunked tail, with per-trajectory weights and uStar; trajectories 0, 17 and 39 against the oracle."""
    N, N2, batch = 80, 40, 40
    mats, tspan, tx, x0, u, Q, R, U, ref = lq_case(oracle, nS, nC, N, N2, batch, (0, 17, 39))
    pg = lq_problem(ocs, mats, nC, Q, R)
    gi = ocs.RK4InfiniteIntegrator(tspan, tx, np.zeros(nC))
    gi.set_mapping(mapping)
    gi.set_batch_uStar(U)
    check(run(gi, pg, x0, u), ref, f"LQ {(nS, nC)} mapping {mapping}")


CHUNKED = (12, 2, 80, 256, 100)   # the tail of 256 steps at batch 100 takes the chunked passes on the automatic mapping


def test_lq_chunked_tail_on_auto(ocs, oracle):
    """(12, 2), N2 = 256, batch = 100: the automatic mapping runs the tail on the chunked passes (as the same shape does in
    test_the_right_column_is_read of tests/test_gpu_lq_batch_weights.py) -- equal to the set_mapping(1) result to RTOL but
    not bit for bit -- with trajectory 21 and the last one 0.25 away from all other uStar: they and their neighbours match
    their own oracle, and the two differ from a run under the batch mean by more than 1e-6 relative in J."""
    nS, nC, N, N2, batch = CHUNKED
    which = (20, 21, 22, batch - 2, batch - 1)
    mats, tspan, tx, x0, u, Q, R, U, ref = lq_case(oracle, nS, nC, N, N2, batch, which, special=True)
    pg = lq_problem(ocs, mats, nC, Q, R)
    gi = ocs.RK4InfiniteIntegrator(tspan, tx, np.zeros(nC))
    gi.set_batch_uStar(U)
    res = run(gi, pg, x0, u)
    check(res, ref, "LQ chunked tail, auto")
    gs = ocs.RK4InfiniteIntegrator(tspan, tx, U).set_mapping(1)
    ser = run(gs, pg, x0, u)
    errs = [relerr(a, b) for a, b in zip(res, ser)]
    print("chunked against serial:", errs)
    assert max(errs) < RTOL and not same(res, ser)
    gi.set_batch_uStar(np.repeat(U.mean(axis=1, keepdims=True), batch, axis=1))
    Jm = run(gi, pg, x0, u)[1]
    for b in (21, batch - 1):
        assert abs(res[1][b] - Jm[b]) > 1e-6 * abs(res[1][b]), (b, res[1][b], Jm[b])


def test_the_right_column_is_read(ocs, oracle):
    """Logistic (2, 64, 64, 70) on the lane kernels: trajectory 21 (lane 21 of the first wave) and 69 (the last of the ragged
    second wave) have uStar = 0.66 and 0.9, all others below 0.45.  They and their neighbours match their own oracle; under
    the batch mean the two give another J by more than 1e-6 relative, so a kernel that reads a neighbour's or a shared value
    cannot pass."""
    nS, N, N2, batch = 2, 64, 64, 70
    tspan, tx, x0, u, cs, ms, U, ref = logistic_case(oracle, nS, N, N2, batch, special=True)
    pg = logistic_problem(ocs, nS, cs, ms)
    for mapping in ("auto", "lane"):
        gi = ocs.RK4InfiniteIntegrator(tspan, tx, U).set_mapping(mapping)
        res = run(gi, pg, x0, u)
        check(res, ref, f"special columns, {mapping}")
        gi.set_batch_uStar(np.full((1, batch), U.mean()))
        Jm = run(gi, pg, x0, u)[1]
        for b in (21, batch - 1):
            assert abs(res[1][b] - Jm[b]) > 1e-6 * abs(res[1][b]), (mapping, b, res[1][b], Jm[b])


# ---- equal columns, handle reuse, refusals --------------------------------------------------------------------------
@pytest.mark.parametrize("nS,N,N2,batch,mapping", [(2, 64, 64, 70, "auto"), (2, 64, 64, 96, "lane"), (2, 64, 64, 96, "auto")])
def test_equal_columns_equal_the_shared_form(ocs, oracle, nS, N, N2, batch, mapping):
    """set_batch_uStar(repeat(us)) against a handle created with the shared us: x, J, lam, dJdu bit for bit on the lane
    kernels (ragged batch 70; set_mapping(1)) and on the wave tail."""
    tspan, tx, x0, u, cs, ms, _, _ = logistic_case(oracle, nS, N, N2, batch)
    pg = logistic_problem(ocs, nS, cs, ms)
    us = np.array([0.3125 + 1e-3 / 3])
    shared = run(ocs.RK4InfiniteIntegrator(tspan, tx, us).set_mapping(mapping), pg, x0, u)
    gb = ocs.RK4InfiniteIntegrator(tspan, tx, [0.1]).set_mapping(mapping)
    gb.set_batch_uStar(np.repeat(us[:, None], batch, 1))
    assert same(shared, run(gb, pg, x0, u))


def test_equal_columns_on_the_chunked_lq_tail(ocs, oracle):
    """The same on the chunked LQ tail, to RTOL: the shared form takes its chunk responses from one group of 16, the
    per-trajectory form from pass Z over the batch."""
    nS, nC, N, N2, batch = CHUNKED
    mats, tspan, tx, x0, u, Q, R, _, _ = lq_case(oracle, nS, nC, N, N2, batch, (20, 21, 22, batch - 2, batch - 1), special=True)
    pg = lq_problem(ocs, mats, nC, Q, R)
    us = np.array([0.21, -0.13])
    shared = run(ocs.RK4InfiniteIntegrator(tspan, tx, us), pg, x0, u)
    res = run(ocs.RK4InfiniteIntegrator(tspan, tx, np.repeat(us[:, None], batch, 1)), pg, x0, u)
    errs = [relerr(a, b) for a, b in zip(res, shared)]
    print("equal columns against shared, chunked tail:", errs)
    assert max(errs) < RTOL


def reuse_sequence(ocs, oracle, make_problem, make_oracle_problem, tspan, tx, x0, u, us, U1, U2, which):
    """shared -> U1 -> U2 (same handle, same batch: the cached samples / chunk responses must follow) -> a batch - 1 call is
    refused -> the _dev setter equals the host setter -> clear restores the shared results bit for bit, any batch again"""
    import torch
    batch = x0.shape[1]
    pg = make_problem()
    gi = ocs.RK4InfiniteIntegrator(tspan, tx, us)
    before = run(gi, pg, x0, u)
    gi.set_batch_uStar(U1)
    r1 = run(gi, pg, x0, u)
    check(r1, oracle_ref(oracle, make_oracle_problem, tspan, tx, U1, x0, u, which), "U1")
    gi.set_batch_uStar(U2)
    r2 = run(gi, pg, x0, u)
    check(r2, oracle_ref(oracle, make_oracle_problem, tspan, tx, U2, x0, u, which), "U2 into the same handle")
    assert not np.array_equal(r1[1], r2[1])
    with pytest.raises(ocs.OcsError) as e:
        gi.compute_states(pg, x0[:, :batch - 1], u[:, :, :batch - 1])
    assert e.value.code == OCS_ERR_SHAPE
    gi.set_batch_uStar(torch.tensor(np.ascontiguousarray(U1), device="cuda"))
    assert same(r1, run(gi, pg, x0, u))
    gi.set_batch_uStar()
    assert same(before, run(gi, pg, x0, u))
    return gi, pg


def test_handle_reuse_on_the_wave_tail(ocs, oracle):
    nS, N, N2, batch = 2, 64, 64, 96
    tspan, tx, x0, u, cs, ms, U1, _ = logistic_case(oracle, nS, N, N2, batch)
    U2 = np.random.default_rng(1).uniform(0.05, 0.45, (1, batch))
    gi, pg = reuse_sequence(ocs, oracle, lambda: ocs.LogisticProblem(M0[:nS], P["c"], P["r"], BOUNDS),
                            lambda b: oracle.LogisticProblem(M0[:nS], P["c"], P["r"], BOUNDS), tspan, tx, x0, u, [0.4],
                            U1, U2, (0, 50, batch - 1))
    gi.compute_states(pg, x0[:, :batch - 1], u[:, :, :batch - 1])   # any batch again


def test_handle_reuse_on_the_chunked_lq_tail(ocs, oracle):
    nS, nC, N, N2, batch = CHUNKED
    mats, tspan, tx, x0, u, Q, R, U1, _ = lq_case(oracle, nS, nC, N, N2, batch, (20, 21, 22, batch - 2, batch - 1), special=True)
    U2 = np.random.default_rng(2).uniform(-0.3, 0.3, (nC, batch))
    po = oracle.LQProblem(mats[0], mats[1], mats[2], mats[3], 0.05, [LQ_BOUNDS] * nC)
    gi, pg = reuse_sequence(ocs, oracle, lambda: ocs.LQProblem(mats[0], mats[1], mats[2], mats[3], 0.05, [LQ_BOUNDS] * nC),
                            lambda b: po, tspan, tx, x0, u, np.array([0.2, -0.1]), U1, U2, (0, 21, batch - 1))
    gi.compute_states(pg, x0[:, :batch - 1], u[:, :, :batch - 1])


def test_refusals(ocs, oracle):
    """The setters on a plain RK4Integrator (and on a null handle): OCS_ERR_INVALID; batch < 0: OCS_ERR_SHAPE; a problem with
    another nC than the per-trajectory uStar: OCS_ERR_SHAPE; a set between compute_states and compute_adjoints: the adjoint
    pass refuses the stale checkpoints."""
    import torch
    lib = ocs._lib.lib
    tspan, tx = oracle.linspace(0, 1, 17), oracle.linspace(1, 2, 17)
    U = np.asfortranarray(np.full((1, 8), 0.3))
    Ud = torch.tensor(U, device="cuda")
    g0 = ocs.RK4Integrator(tspan)
    assert lib.ocs_rk4inf_set_batch_ustar(g0._h, 8, U.ctypes.data_as(ocs._lib.dp)) == OCS_ERR_INVALID
    assert lib.ocs_rk4inf_set_batch_ustar_dev(g0._h, 8, C.c_void_p(Ud.data_ptr()), None) == OCS_ERR_INVALID
    assert lib.ocs_rk4inf_set_batch_ustar(None, 8, U.ctypes.data_as(ocs._lib.dp)) == OCS_ERR_INVALID
    gi = ocs.RK4InfiniteIntegrator(tspan, tx, [0.4])
    assert lib.ocs_rk4inf_set_batch_ustar(gi._h, -1, U.ctypes.data_as(ocs._lib.dp)) == OCS_ERR_SHAPE
    assert lib.ocs_rk4inf_set_batch_ustar_dev(gi._h, -1, C.c_void_p(Ud.data_ptr()), None) == OCS_ERR_SHAPE
    gi.set_batch_uStar(U)
    A, Bu, q, rdiag = lq_matrices(5, 2)
    p2 = ocs.LQProblem(A, Bu, q, rdiag, 0.05, [LQ_BOUNDS] * 2)
    with pytest.raises(ocs.OcsError) as e:
        gi.compute_states(p2, np.zeros((5, 8)), np.zeros((2, 33, 8)))
    assert e.value.code == OCS_ERR_SHAPE
    pg = ocs.TestOCProblem(P, BOUNDS)
    x0, u = np.full((1, 8), 1.5), np.full((1, 33, 8), 0.3)
    gi.compute_states(pg, x0, u)
    gi.set_batch_uStar(U + 0.1)
    with pytest.raises(ocs.OcsError):
        gi.compute_adjoints(pg, u)
    gi.compute_states(pg, x0, u)
    gi.compute_adjoints(pg, u)


# ---- the reference's driver script as one batch ---------------------------------------------------------------------
def test_solve_test_problem_script_as_one_batch(ocs, oracle):
    """tests/solve_test_problem.m:21-39 for B = 70 instances of TestOCProblem with c ~ U(1.2, 2), m ~ U(3, 3.5) (the ranges
    of test_equilibrium_batched: the root stays interior): compute_equilibrium -> us (1 x B) -> RK4InfiniteIntegrator(tspan,
    tspanExtra, us) -> nlp_objective through PWLinearControl(t, 9, 1): J and dJdv of every instance against
    oracle.nlp_objective on that instance's problem and oracle.RK4InfiniteIntegrator(..., [us_b]).  Then
    single_shooting_batch(..., u0=us): instances 0 and 69 equal the same driver (same batch, same start) on a handle with
    the shared uStar = us_b -- J[b], v[:, b] to RTOL scaled by max(1, |.|), equal iteration counts (the form of
    test_single_shooting_batch_instances_are_independent, tests/test_gpu_batch_params.py)."""
    B = 70
    rng = np.random.default_rng(21)
    cs, ms = rng.uniform(1.2, 2.0, B), rng.uniform(3.0, 3.5, B)
    prob = ocs.TestOCProblem(P, BOUNDS)
    prob.set_batch_params([1, 0], np.vstack([ms, cs]))
    lb, ub = [0.0, -np.inf, 0.0], [np.inf, np.inf, 1.0]
    xG, lG, uG = np.full((1, B), 2.7), np.full((1, B), 2.2), np.full((1, B), 0.7)
    _, _, us, _, _, flag = ocs.compute_equilibrium(prob, xG, lG, uG, lb, ub, P["r"])
    assert np.all(flag == 1) and us.shape == (1, B) and np.ptp(us) > 1e-3
    tspan, tx = oracle.linspace(0, 2, 65), oracle.linspace(2, 4, 65)
    gi = ocs.RK4InfiniteIntegrator(tspan, tx, us)
    cg = ocs.PWLinearControl(gi.t, 9, 1)
    V = rng.uniform(0.1, 0.9, (9, B))
    x0 = rng.uniform(1.0, 2.5, (1, B))
    J, dJdv, _ = ocs.nlp_objective(gi, prob, cg, x0, V)
    worst = 0.0
    for b in range(B):
        po = oracle.TestOCProblem({"c": cs[b], "m": ms[b], "r": P["r"]}, BOUNDS)
        go = oracle.RK4InfiniteIntegrator(tspan, tx, [us[0, b]])
        Jo, do, _ = oracle.nlp_objective(go, po, oracle.PWLinearControl(go.t, 9, 1), x0[:, b], V[:, b])
        errs = (abs(J[b] - Jo) / max(1.0, abs(Jo)), relerr(dJdv[:, b], do))
        worst = max(worst, *errs)
        assert max(errs) < RTOL, (b, errs)
    print("nlp_objective, worst J / dJdv error", worst)
    kw = dict(u0=us, MaxIter=6, TolFun=1e-12, TolX=1e-14)
    r = ocs.single_shooting_batch(prob, x0, tspan, 9, Integrator=gi, **kw)
    Jb, vb, itb = r["J"].cpu().numpy(), r["v"].cpu().numpy(), r["iterations"].cpu().numpy()
    assert np.ptp(vb[0]) > 1e-3   # a start per instance
    for b in (0, B - 1):
        gs = ocs.RK4InfiniteIntegrator(tspan, tx, [us[0, b]])
        rs = ocs.single_shooting_batch(prob, x0, tspan, 9, Integrator=gs, **kw)
        Js, vs, its = rs["J"].cpu().numpy(), rs["v"].cpu().numpy(), rs["iterations"].cpu().numpy()
        errs = (abs(Jb[b] - Js[b]) / max(1.0, abs(Js[b])), relerr(vb[:, b], vs[:, b]))
        print(f"driver, instance {b}: J / v {errs}, iterations {itb[b]} / {its[b]}")
        assert max(errs) < RTOL and itb[b] == its[b] and itb[b] > 0
