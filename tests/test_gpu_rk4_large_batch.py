"""The RK4 pass pair from batch 32768: the lane kernels that re-integrate three of four checkpoints (k_backward<..., XRC>,
record ring of depth 4, non-temporal stores) and the state pass with non-temporal stores (k_forward<..., NT>), against the CPU
oracle on every trajectory (the NumPy twin on sampled trajectories for the coupled hipRTC plugin).  No other test of the pass
pair goes past batch 4096, so below this file these instances are never launched by the suite.

The threshold is on the batch alone (lane_xrc_min_batch() = 32768, csrc/ocs_kernels.hip), so the step counts stay small:
N = 4 .. 17 gives 1 .. 4 chunks of 4 steps (both parities of the double-buffered chunk loop of k_backward) and 0 .. 3
remainder steps at the top of the grid; the batches are the threshold itself, 32769 and 32805 (one and 37 live lanes in the
last wave, the others clamped onto the last trajectory).  Grids are non-uniform from N = 5.

Which kernels a case runs, and the function that decides it (all in csrc/ocs_kernels.hip unless named):

    case                                         state pass                        adjoint pass                      decided by
    test_lane_pair[nS-N-batch], nS = 1..4        k_forward<P,4,pf,true,false,NT>   k_backward<P,4,4,true,true,       run_forward, run_backward
      (forced "lane", batch >= 32768, N >= 4)                                        false,XRC>
    test_device_entry_points[nS-N-batch]         the same                          the three XRC instances (lam +    run_backward
      (forced "lane")                            (x = None: checkpoints to the       dJdu, lam only, dJdu only),
                                                 handle's scratch, same kernel)      default and explicit lamT       leg_forward (ocs_api.cpp)
    test_sub_batch_is_independent[nS]            NT at 32768, plain at 16384       XRC at 32768, plain               run_forward, run_backward
      (forced "lane")                                                                k_backward<P,4,pf_of<P>()> at 16384
    test_automatic_mapping_across_the_seams:                                                                         choose_mapping, scan_pays,
      4-16-16384 (1024 workgroups)               k_forward_p2 (pipeline)           k_backward_scan                   launch_backward
      4-16-16400 (1025 workgroups)               plain k_forward                   plain k_backward
      4-13-32768                                 NT                                XRC (3 chunks + 1 step)
      2-16-32768 (1024 workgroups)               k_forward_p2                      k_backward_scan
      2-16-32800 (1025 workgroups)               NT                                XRC
      1-6-32768  (N < 8: no block of 8 steps,    NT                                XRC (1 chunk + 2 steps)
                  scan_pays false)
      1-16-32832 (513 workgroups > 512)          NT                                k_backward_scan (nS = 1: at every batch)
      3-16-19712 (past 16384 * 6 / 5 = 19660)    k_forward_pv (vector lanes)       plain k_backward
      3-16-32768 (512 workgroups)                k_forward_pv                      XRC on the checkpoints of k_forward_pv
    test_per_trajectory_parameters               NT                                XRC, P::load from the table pb    run_forward, run_backward
    test_coupled_plugin[32768-N]  (hipRTC)       k_forward_pv for 8 steps +        UK_BWD_LAM_DJDU_XRC; lam only,    launch_forward, launch_backward
                                                 UK_FWD_X for the rest             dJdu only: UK_BWD_LAM, UK_BWD_DJDU (the user branch)
    test_coupled_plugin[32805-N]  (ragged tile)  UK_FWD_X                          the same
    test_row_function_plugin (nS = 2, 32800)     UK_FWD_X                          UK_BWD_LAM_DJDU_XRC               launch_forward, launch_backward
    test_infinite_integrator (nS = 4, 32768)     main leg NT; tail leg             main leg XRC with lamT = lam2(:,1); ocs_compute_states_dev,
                                                 k_forward<.., UCONST>             tail leg k_backward<.., UCONST>   tail_leg_wave_ok

(The hipRTC plugins have no NT state pass and an XRC instance for lam + dJdu only: ocs_jit.cpp, kernel_names.)

Tolerance: the project's 1e-12 (RTOL of tests/test_gpu_rk4_parity.py) against the oracle.  Two comparisons are between GPU
runs, and were measured on an MI355X before their assertions were written (NOTES.md):
  * the three XRC instances against one another (test_device_entry_points): bit-equal, asserted with torch.equal;
  * columns [:16384] of a batch-32768 run (XRC, NT) against a batch-16384 run of those columns (plain kernels):
    bit-equal for x, lam and dJdu at nS = 1..4, asserted with np.array_equal.
The coupled plugin's combined call (XRC) against its lam-only / dJdu-only calls (plain) is NOT bit-equal: lam differs by up
to 2.7e-15, dJdu by up to 4.4e-16 (absolute, values of order 1).  The registry functor spells every fused multiply-add out,
so its re-integration repeats the state pass bit for bit; a plugin's expressions are contracted by the compiler, which does
so differently in the two instantiations.  That comparison is held to the 1e-13 that test_single_state_pipeline_adjoint
(tests/test_gpu_rk4_parity.py) sets between two mappings.
"""
import numpy as np
import pytest

from oracle import np_twin as tw
from tests.test_gpu_rk4_parity import BOUNDS, P, RTOL, _inputs, ocs, relerr  # noqa: F401  (ocs: that module's fixture)
from tests.user_problems import LOGISTIC_ROWS_SRC, PREDPREY_PARAMS, PREDPREY_SRC, PredPreyNP

pytestmark = pytest.mark.gpu

M4 = [3.0, 2.5, 2.0, 1.5]
BATCHES = (32768, 32769, 32805)
SAMPLE = (0, 63, 64, 16383, 16384, 32767, 32768)
_REF = {}   # inputs and references shared between tests (computed once, read-only afterwards)
_SHARED = {(4, 12, 32768), (2, 12, 32768), (4, 13, 32805), (2, 13, 32805)}


def _sample(batch, stride=0):
    """the trajectories at the ends of the first wave, at the 16384 and 32768 seams and the last one (+ every stride-th)"""
    idx = {b for b in SAMPLE if b < batch} | {batch - 1}
    if stride:
        idx |= set(range(0, batch, stride))
    return np.array(sorted(idx))


def _grid(oracle, N, T):
    if N < 5:
        return oracle.linspace(0.0, T, N + 1)
    return np.sort(np.concatenate([[0.0, T], np.random.default_rng(N).uniform(0, T, N - 1)]))


def _freeze(*arrays):
    for a in arrays:
        if a is not None:
            a.setflags(write=False)


def _case(oracle, nS, N, batch):
    """Controls and x0 of _inputs (tests/test_gpu_rk4_parity.py) on T = N / 20 (mean step 0.05, as that file's shapes), the
    grid of _grid, and the oracle's x, J, lam, dJdu of every trajectory -- all finite, so that relerr's branch for
    non-finite reference entries hides nothing."""
    key = (nS, N, batch)
    if key in _REF:
        return _REF[key]
    T = N / 20.0
    _, x0, u = _inputs(oracle, nS, N, batch, seed=5000 + 100 * nS + N, T=T)
    tspan = _grid(oracle, N, T)
    po = oracle.LogisticProblem(M4[:nS], P["c"], P["r"], BOUNDS)
    ref = oracle.batch_states_adjoints(po, tspan, x0, u)
    for k, v in ref.items():
        assert np.isfinite(v).all(), k
    _freeze(x0, u, *ref.values())
    if key in _SHARED:
        _REF[key] = (tspan, x0, u, ref)
    return tspan, x0, u, ref


def _logistic(ocs, nS):
    return ocs.LogisticProblem(M4[:nS], P["c"], P["r"], BOUNDS)


def _check_pair(g, pg, x0, u, ref, what):
    x, J = g.compute_states(pg, x0, u)
    lam, dJdu = g.compute_adjoints(pg, u)
    errs = {"x": relerr(x, ref["x"]), "J": relerr(J, ref["J"]), "lam": relerr(lam, ref["lam"]), "dJdu": relerr(dJdu, ref["dJdu"])}
    print(what, errs)
    assert max(errs.values()) < RTOL, (what, errs)
    assert np.all(lam[-1] == 1.0) and np.array_equal(x[-1, -1, :], J)
    return x, J, lam, dJdu


# ---- 1. registry problems on the lane kernels ----------------------------------------------------------------------
FULL_N = (7, 13)       # all three batches: one chunk + three remainder steps; three chunks + one
ONE_BATCH = {4: 32768, 5: 32769, 8: 32805, 9: 32768, 10: 32769, 12: 32768, 17: 32805}   # (10: two remainder steps)
LANE_CASES = ([(nS, N, b) for nS in (1, 2, 3, 4) for N in FULL_N for b in BATCHES] +
              [(nS, N, b) for nS in (1, 2, 3, 4) for N, b in ONE_BATCH.items()])


@pytest.mark.parametrize("nS,N,batch", LANE_CASES)
def test_lane_pair(ocs, oracle, nS, N, batch):
    """k_forward<NT> and k_backward<XRC> (lam + dJdu), forced "lane": x, J, lam, dJdu of every trajectory against the oracle,
    lam(end, :) = 1 exactly and x(end, end) = J bit for bit (the cost row goes through the non-temporal store, J does not)."""
    tspan, x0, u, ref = _case(oracle, nS, N, batch)
    _check_pair(ocs.RK4Integrator(tspan).set_mapping("lane"), _logistic(ocs, nS), x0, u, ref, f"lane {(nS, N, batch)}")


# ---- 2. device entry points: the three XRC instances, explicit lamT, no x ------------------------------------------
@pytest.mark.parametrize("nS,N,batch", [(4, 12, 32768), (4, 13, 32805), (2, 12, 32768), (2, 13, 32805)])
def test_device_entry_points(ocs, oracle, nS, N, batch):
    """compute_states_dev / compute_adjoints_dev, forced "lane": lam + dJdu, lam only and dJdu only are three instantiations
    of k_backward<XRC>; each against the oracle on every trajectory, and bit-equal to one another (measured on an MI355X:
    they are, for the default and the explicit lamT).  With an explicit lamT: against the oracle's single-trajectory passes
    on the sampled trajectories and every 257th.  With x = None the state pass writes its checkpoints to the handle's scratch
    (same kernel): J and the dJdu of the adjoint pass that follows are the bits of the run with x."""
    import torch
    tspan, x0, u, ref = _case(oracle, nS, N, batch)
    pg, po = _logistic(ocs, nS), oracle.LogisticProblem(M4[:nS], P["c"], P["r"], BOUNDS)
    g = ocs.RK4Integrator(tspan).set_mapping("lane")
    dev = torch.device("cuda:0")
    nan = lambda *shape: torch.full(shape, float("nan"), dtype=torch.float64, device=dev)
    host = lambda t: t.cpu().numpy().transpose(1, 0, 2)
    x0d = torch.tensor(np.ascontiguousarray(x0), device=dev)
    ud = torch.tensor(np.ascontiguousarray(u.transpose(1, 0, 2)), device=dev)
    xd = nan(N + 1, nS + 1, batch)
    _, Jd = g.compute_states_dev(pg, x0d, ud, xd)
    lam_b, d_b, lam_o, d_o = nan(*xd.shape), nan(*ud.shape), nan(*xd.shape), nan(*ud.shape)
    g.compute_adjoints_dev(pg, ud, None, lam_b, d_b)
    g.compute_adjoints_dev(pg, ud, None, lam_o, None)
    g.compute_adjoints_dev(pg, ud, None, None, d_o)
    torch.cuda.synchronize()
    assert relerr(host(xd), ref["x"]) < RTOL and relerr(Jd.cpu().numpy(), ref["J"]) < RTOL
    assert torch.equal(xd[-1, -1, :], Jd)
    for name, lam_v, d_v in (("lam + dJdu", lam_b, d_b), ("lam only", lam_o, None), ("dJdu only", None, d_o)):
        errs = (0.0 if lam_v is None else relerr(host(lam_v), ref["lam"]), 0.0 if d_v is None else relerr(host(d_v), ref["dJdu"]))
        print((nS, N, batch), name, errs)
        assert max(errs) < RTOL, (name, errs)
    print("variants, max |difference|: lam", float((lam_b - lam_o).abs().max()), "dJdu", float((d_b - d_o).abs().max()))
    assert torch.equal(lam_b, lam_o) and torch.equal(d_b, d_o)
    assert bool(torch.all(lam_b[:, -1, :] == 1.0))
    # explicit lamT
    lamT = np.random.default_rng(N + batch).normal(size=(nS + 1, batch))
    lamTd = torch.tensor(lamT, device=dev)
    l2_b, d2_b, l2_o, d2_o = nan(*xd.shape), nan(*ud.shape), nan(*xd.shape), nan(*ud.shape)
    g.compute_adjoints_dev(pg, ud, lamTd, l2_b, d2_b)
    g.compute_adjoints_dev(pg, ud, lamTd, l2_o, None)
    g.compute_adjoints_dev(pg, ud, lamTd, None, d2_o)
    torch.cuda.synchronize()
    assert torch.equal(l2_b, l2_o) and torch.equal(d2_b, d2_o)
    assert bool(torch.isfinite(l2_b).all()) and bool(torch.isfinite(d2_b).all())
    l2, d2 = host(l2_b), host(d2_b)
    go = oracle.RK4Integrator(tspan)
    worst = 0.0
    for b in _sample(batch, 257):
        go.compute_states(po, x0[:, b], u[:, :, b])
        lo, do = go.compute_adjoints(po, u[:, :, b], lamT[:, b])
        assert np.isfinite(lo).all() and np.isfinite(do).all()
        errs = (relerr(l2[:, :, b], lo), relerr(d2[:, :, b], do))
        worst = max(worst, *errs)
        assert max(errs) < RTOL, (b, errs)
    print("explicit lamT, worst lam / dJdu error", worst)
    # objective + gradient only: no trajectory outputs
    _, J2 = g.compute_states_dev(pg, x0d, ud, None)
    d3 = nan(*ud.shape)
    g.compute_adjoints_dev(pg, ud, None, None, d3)
    torch.cuda.synchronize()
    assert relerr(J2.cpu().numpy(), ref["J"]) < RTOL and relerr(host(d3), ref["dJdu"]) < RTOL
    assert torch.equal(J2, Jd) and torch.equal(d3, d_b)


# ---- 3. a trajectory does not depend on the batch it rides in -------------------------------------------------------
@pytest.mark.parametrize("nS", [1, 2, 3, 4])
def test_sub_batch_is_independent(ocs, oracle, nS):
    """Forced "lane", N = 13: columns [:16384] of a batch-32768 run (k_forward<NT>, k_backward<XRC>: three of four checkpoints
    integrated again, ring of 4 records) against a batch-16384 run of the same columns (plain kernels: every checkpoint read,
    ring of pf_of<P>() records).  The re-integration repeats the state pass's operations, so nothing may differ: measured
    on an MI355X, the difference is 0 for x, lam and dJdu at every nS; asserted bit for bit."""
    N, batch, half = 13, 32768, 16384
    tspan, x0, u, ref = _case(oracle, nS, N, batch)
    pg = _logistic(ocs, nS)
    g = ocs.RK4Integrator(tspan).set_mapping("lane")
    x, J = g.compute_states(pg, x0, u)
    lam, dJdu = g.compute_adjoints(pg, u)
    assert relerr(lam, ref["lam"]) < RTOL and relerr(dJdu, ref["dJdu"]) < RTOL   # (the large run is the one of test_lane_pair)
    xh, Jh = g.compute_states(pg, x0[:, :half], u[:, :, :half])
    lamh, dh = g.compute_adjoints(pg, u[:, :, :half])
    diff = {k: float(np.max(np.abs(a[..., :half] - b))) for k, a, b in (("x", x, xh), ("J", J, Jh), ("lam", lam, lamh), ("dJdu", dJdu, dh))}
    print("nS", nS, "max |batch 32768 [:16384] - batch 16384|", diff)
    assert np.array_equal(x[:, :, :half], xh) and np.array_equal(J[:half], Jh)
    assert np.array_equal(lam[:, :, :half], lamh) and np.array_equal(dJdu[:, :, :half], dh)


# ---- 4. automatic mapping on both sides of each seam ----------------------------------------------------------------
@pytest.mark.parametrize("nS,N,batch", [(4, 16, 16384), (4, 16, 16400), (4, 13, 32768), (2, 16, 32768), (2, 16, 32800),
                                        (1, 6, 32768), (1, 16, 32832), (3, 16, 19712), (3, 16, 32768)])
def test_automatic_mapping_across_the_seams(ocs, oracle, nS, N, batch):
    """What a caller gets without set_mapping on the last shape of the wave-specialised kernels and the first of the lane
    kernels (the table in the module docstring): x, J, lam, dJdu of every trajectory against the oracle.  Every shape
    computes: a refusal (-6) here would be a fault of the dispatch."""
    tspan, x0, u, ref = _case(oracle, nS, N, batch)
    _check_pair(ocs.RK4Integrator(tspan), _logistic(ocs, nS), x0, u, ref, f"auto {(nS, N, batch)}")


# ---- 5. per-trajectory parameters ------------------------------------------------------------------------------------
def test_per_trajectory_parameters(ocs, oracle):
    """LogisticProblem with four states, c and every m_k per trajectory (c ~ U(1, 2), m ~ U(1.5, 3), as
    tests/test_gpu_batch_params.py draws them; index list unsorted) at batch 32805, N = 9, forced "lane": the NT and XRC
    instances read P::load's table column of THEIR trajectory.  Against one oracle problem per trajectory on the sampled
    trajectories and every 257th, as test_per_trajectory_parameters of tests/test_gpu_rk4_parity.py does."""
    nS, N, batch = 4, 9, 32805
    T = N / 20.0
    _, x0, u = _inputs(oracle, nS, N, batch, seed=77, T=T)
    tspan = _grid(oracle, N, T)
    rng = np.random.default_rng(78)
    cs, ms = rng.uniform(1.0, 2.0, batch), rng.uniform(1.5, 3.0, (nS, batch))
    pg = _logistic(ocs, nS)
    pg.set_batch_params([5, 0, 2, 3, 4], np.vstack([ms[3], cs, ms[0], ms[1], ms[2]]))   # block [c r m_1 .. m_4]
    g = ocs.RK4Integrator(tspan).set_mapping("lane")
    x, J = g.compute_states(pg, x0, u)
    lam, dJdu = g.compute_adjoints(pg, u)
    assert np.all(lam[-1] == 1.0) and np.array_equal(x[-1, -1, :], J)
    go = oracle.RK4Integrator(tspan)
    worst = 0.0
    for b in _sample(batch, 257):
        po = oracle.LogisticProblem(ms[:, b], cs[b], P["r"], BOUNDS)
        xo, Jo = go.compute_states(po, x0[:, b], u[:, :, b])
        lamo, do = go.compute_adjoints(po, u[:, :, b])
        assert np.isfinite(xo).all() and np.isfinite(lamo).all() and np.isfinite(do).all()
        errs = (relerr(x[:, :, b], xo), relerr(J[b], Jo), relerr(lam[:, :, b], lamo), relerr(dJdu[:, :, b], do))
        worst = max(worst, *errs)
        assert max(errs) < RTOL, (b, errs)
    print("worst x / J / lam / dJdu error", worst)


# ---- 6. hipRTC plugins ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("batch", [32768, 32805])
@pytest.mark.parametrize("N", [12, 13])
def test_coupled_plugin(ocs, oracle, N, batch):
    """PREDPREY_SRC (coupled, two states; inputs of test_coupled_plugin of tests/test_gpu_batch_params.py at a step of 0.1)
    on automatic mapping, past the vector scan's limit of 24576: lam + dJdu on UK_BWD_LAM_DJDU_XRC, against the NumPy twin
    (PredPreyNP on RK4IntegratorNP) on the sampled trajectories and every 257th.  Through the device entry points lam-only
    and dJdu-only run the plain kernels (the plugin has no XRC instance for them).  Measured on an MI355X, the combined call
    differs from them by up to 2.7e-15 in lam and 4.4e-16 in dJdu (the compiler contracts the plugin's expressions differently
    in the re-integration; module docstring), so they are held to the 1e-13 between mappings of tests/test_gpu_rk4_parity.py,
    and each to the twin at 1e-12."""
    import torch
    T = 0.1 * N
    tspan = _grid(oracle, N, T)
    rng = np.random.default_rng(N + batch)
    u = rng.uniform(0.0, 1.0, (1, 2 * N + 1, batch))
    x0 = rng.uniform(1.0, 2.5, (2, batch))
    pu = ocs.UserProblem(PREDPREY_SRC, 2, 1, PREDPREY_PARAMS, BOUNDS)
    g = ocs.RK4Integrator(tspan)
    x, J = g.compute_states(pu, x0, u)
    lam, dJdu = g.compute_adjoints(pu, u)
    assert np.all(lam[-1] == 1.0) and np.array_equal(x[-1, -1, :], J)
    gn, pn = tw.RK4IntegratorNP(tspan), PredPreyNP(PREDPREY_PARAMS)
    worst, refs = 0.0, {}
    for b in _sample(batch, 257):
        xn, Jn = gn.compute_states(pn, x0[:, b], u[:, :, b])
        lamn, dn = gn.compute_adjoints(pn, u[:, :, b])
        refs[b] = (lamn, dn)
        assert np.isfinite(xn).all() and np.isfinite(lamn).all() and np.isfinite(dn).all()
        errs = (relerr(x[:, :, b], xn), relerr(J[b], Jn), relerr(lam[:, :, b], lamn), relerr(dJdu[:, :, b], dn))
        worst = max(worst, *errs)
        assert max(errs) < RTOL, (b, errs)
    print("worst x / J / lam / dJdu error", worst)
    dev = torch.device("cuda:0")
    nan = lambda *shape: torch.full(shape, float("nan"), dtype=torch.float64, device=dev)
    x0d = torch.tensor(x0, device=dev)
    ud = torch.tensor(np.ascontiguousarray(u.transpose(1, 0, 2)), device=dev)
    xd = nan(N + 1, 3, batch)
    g.compute_states_dev(pu, x0d, ud, xd)
    lam_b, d_b, lam_o, d_o = nan(*xd.shape), nan(*ud.shape), nan(*xd.shape), nan(*ud.shape)
    g.compute_adjoints_dev(pu, ud, None, lam_b, d_b)
    g.compute_adjoints_dev(pu, ud, None, lam_o, None)
    g.compute_adjoints_dev(pu, ud, None, None, d_o)
    torch.cuda.synchronize()
    assert np.array_equal(lam_b.cpu().numpy().transpose(1, 0, 2), lam) and np.array_equal(d_b.cpu().numpy().transpose(1, 0, 2), dJdu)
    print("XRC - plain, max |difference|: lam", float((lam_b - lam_o).abs().max()), "dJdu", float((d_b - d_o).abs().max()))
    assert bool(torch.isfinite(lam_o).all()) and bool(torch.isfinite(d_o).all())
    assert relerr(lam_b.cpu().numpy(), lam_o.cpu().numpy()) < 1e-13 and relerr(d_b.cpu().numpy(), d_o.cpu().numpy()) < 1e-13
    lo_h, do_h = lam_o.cpu().numpy().transpose(1, 0, 2), d_o.cpu().numpy().transpose(1, 0, 2)
    for b in _sample(batch):
        lamn, dn = refs[b]
        assert relerr(lo_h[:, :, b], lamn) < RTOL and relerr(do_h[:, :, b], dn) < RTOL, b


def test_row_function_plugin(ocs, oracle):
    """LOGISTIC_ROWS_SRC (row functions, two states) at batch 32800 = 1025 workgroups of the wave-specialised kernels, one
    past their limit: lane state pass and UK_BWD_LAM_DJDU_XRC on automatic mapping, every trajectory against the oracle's
    LogisticProblem of the same parameters."""
    nS, N, batch = 2, 13, 32800
    tspan, x0, u, ref = _case(oracle, nS, N, batch)
    pu = ocs.UserProblem(LOGISTIC_ROWS_SRC, nS, 1, [P["c"], P["r"]] + M4[:nS], BOUNDS, row_separable=True)
    _check_pair(ocs.RK4Integrator(tspan), pu, x0, u, ref, "row functions")


# ---- 7. RK4InfiniteIntegrator ----------------------------------------------------------------------------------------
def test_infinite_integrator(ocs, oracle):
    """RK4InfiniteIntegrator at batch 32768 with four states (2048 workgroups: the tail leg stays on the lane kernels with
    the constant control as a parameter): main leg N = 12 on k_forward<NT> and, with lamT = lam2(:, 1) from the tail leg,
    on k_backward<XRC>; tail leg N2 = 8 on the UCONST instances.  Inputs of test_infinite_integrator_tail_leg_mappings
    (tests/test_gpu_controls_shooting.py) at its step of 2 / 64; x, J = J1 + J2, lam (its last column is lamT) and dJdu
    against the oracle on the sampled trajectories and every 257th."""
    nS, N, N2, batch, us = 4, 12, 8, 32768, 0.4
    T1, T2 = N / 32.0, (N + N2) / 32.0
    tspan, tx = oracle.linspace(0, T1, N + 1), oracle.linspace(T1, T2, N2 + 1)
    pg, po = _logistic(ocs, nS), oracle.LogisticProblem(M4[:nS], P["c"], P["r"], BOUNDS)
    gi, go = ocs.RK4InfiniteIntegrator(tspan, tx, [us]), oracle.RK4InfiniteIntegrator(tspan, tx, [us])
    rng = np.random.default_rng(N + N2 + batch)
    u = rng.uniform(0.05, 0.45, (1, 2 * N + 1, batch))
    x0 = rng.uniform(0.8, 2.0, (nS, batch))
    x, J = gi.compute_states(pg, x0, u)
    lam, dJdu = gi.compute_adjoints(pg, u)
    assert np.all(lam[-1] == 1.0)
    worst = 0.0
    for b in _sample(batch, 257):
        xo, Jo = go.compute_states(po, x0[:, b], u[:, :, b])
        lamo, do = go.compute_adjoints(po, u[:, :, b])
        assert np.isfinite(xo).all() and np.isfinite(lamo).all() and np.isfinite(do).all() and np.any(lamo[:nS, -1] != 0.0)
        errs = (relerr(x[:, :, b], xo), relerr(J[b], Jo), relerr(lam[:, -1, b], lamo[:, -1]), relerr(lam[:, :, b], lamo),
                relerr(dJdu[:, :, b], do))
        worst = max(worst, *errs)
        assert max(errs) < RTOL, (b, errs)
    print("worst x / J / lamT / lam / dJdu error", worst)
