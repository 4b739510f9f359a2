"""Rounding error of the forward-backward sweep on the GPU, measured on a local scale against the extended-precision twin.

The sweep's parity tests (tests/test_gpu_fb_sweep.py) compare with the fp64 oracle by max |a - b| / max(1, |b|) < 1e-10:
absolute wherever a value is below 1 -- a costate discounted through ten orders of magnitude, a state that starts at 1e-3, the
product lam e^{rt} that decides the control.  Here compute_x_lam_J and fb_sweep, like the oracle, are compared with
tests/fbs_twin.py (NumPy longdouble; pinned in tests/test_fbs_twin.py) by rk4_twin's local measure `err` -- u on its own local
scale like lam, maxChange relative to the twin's value -- in the regimes of tests/fbs_accuracy_cases.py, and every output of
every trajectory must satisfy the statement of tests/test_gpu_rk4_accuracy.py, with its constants (tests/accuracy_check.py):

    err_gpu <= K * max(err_oracle, 8 eps),      eps = 2^-53,  K = 8.

The yardstick of sweep k is the oracle's error after the same k sweeps: whatever the sweep map does to an error made in
sweep 1 it does to the oracle's as well, so no amplification factor is guessed.  No instance converges within the sweeps
run here (tests/test_fbs_twin.py proves it for the oracle, each test asserts it for the GPU), so no discrete decision lies
inside a test.

The one derived exception: regime B wherever the state pass is k_forward_p2 or k_forward_cc, which carry z = x - m/2; the
bound of trajectory b is then K * S_b * max(err_oracle, 8 eps) with S_b from the twin's states exactly as in
test_logistic_pass_pair_error (tests/test_gpu_rk4_accuracy.py: its docstring derives S_b).  That is every sweep loop of the
registry logistic problem at N >= 8 on a batch tile_ok accepts -- launch_forward (csrc/ocs_kernels.hip) chooses
MAP_PIPELINE for the first 8 floor(N / 8) steps whatever the loop (1, 2 and 5 call it, 4 runs k_forward_cc) -- and not the odd
batch 69 at N = 13, which the lane kernel integrates.

Which case reaches which kernel (the path and matrix-core assertions back it up):

    k_forward_cc + k_costate_scan<MET>     loop 4, logistic N = 72, batch 70 and 64 (2, 3 or 5 workgroups <= 128)
    k_forward_cc + k_costate_plx<MET>      loop 4, logistic N = 16, batch 129 * 64 / nS + 2 (130 workgroups > 128:
                                           costate_scan_ok, csrc/ocs_scan_kernels.hip, batch / (64 / nS) <= 128)
    k_costate_scan (no MET), k_control_grid   loop 2, N = 72; compute_x_lam_J at N = 72
    k_costate_plx (no MET)                 loop 2 at the 130-workgroup batch
    k_costate_pl + k_pchip_mid             loop 1 and loop 5 at N = 72 (midpoints given: fused_update_off = 1; loop 5 is gated
                                           with ownx, so it takes k_costate_scan / plx again)
    k_costate + k_pchip_mid (lane)         N = 13, every loop, and compute_x_lam_J at N = 13; the LQ (5, 2) plugin twin
    k_control_pts_sorted                   loops 1 and 5 of the logistic problems (error points), k_control_pts: the
                                           interpolation points of every run and the error points of LQ (5, 2) (nS > 4)
    k_lq_sweep_costate (matrix cores)      LQ (12, 2), (32, 4): fb_sweep_matrix_core == 1
    hipRTC k_forward_cc + k_costate_scan<MET>   "rows-cc": LOGISTIC_ROWS_CC_SRC with flag bit 2, loop 4
    hipRTC k_forward_pv + k_costate_vscan + k_control_grid   "vector": LOGISTIC2_SRC, loop 2

Every test prints one ACCURACY line of ratios err_gpu / max(err_oracle, 8 eps) per run; the measured table is in NOTES.md."""
import numpy as np
import pytest

from tests import fbs_accuracy_cases as fc
from tests import rk4_accuracy_cases as rc
from tests.accuracy_check import check_ratios

pytestmark = pytest.mark.gpu
NOT_CONVERGED = 2        # OCS_NUM_NOT_CONVERGED (include/ocs.h)


@pytest.fixture(scope="module")
def ocs():
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    import __graft_entry__ as g
    return g.load_package()


def _problem(ocs, family, par, form="registry"):
    bounds = fc.bounds_of(family, par)
    if family == "lq":
        return ocs.LQProblem(par["A"], par["Bu"], par["q"], par["rdiag"], par["r"], bounds)
    if form == "registry":
        return ocs.LogisticProblem(par["m"], par["c"], par["r"], bounds)
    from tests.user_problems import LOGISTIC2_SRC, LOGISTIC_ROWS_CC_SRC
    params = [par["c"], par["r"]] + list(par["m"])
    if form == "rows-cc":
        return ocs.UserProblem(LOGISTIC_ROWS_CC_SRC, len(par["m"]), 1, params, bounds, has_control_char=True, row_separable=True,
                               control_from_costate=True)
    assert form == "vector" and len(par["m"]) == 2
    return ocs.UserProblem(LOGISTIC2_SRC, 2, 1, params, bounds, has_control_char=True)


def _state_pass_carries_z(family, form, nS, N, batch):
    """k_forward_p2 / k_forward_cc integrate (part of) the horizon: pipeline_steps > 0 in csrc/ocs_kernels.hip"""
    return family == "logistic" and form == "registry" and N >= 8 and fc.tile_ok(batch, 64 // nS)


def _factor(par, x_ref):
    """S_b of test_logistic_pass_pair_error (tests/test_gpu_rk4_accuracy.py) from the twin's states x_ref [nS][N+1][B]"""
    half_m = np.asarray(par["m"], dtype=np.longdouble)[:, None, None] / 2
    return np.max(1 + half_m / np.abs(x_ref), axis=(0, 1)).astype(np.float64)


X_LAM = ([("logistic", r, nS, N, b) for r in fc.LOGISTIC_REGIMES for nS, N, b in fc.LOGISTIC_SHAPES] +
         [("lq", r, s, rc.LQ_N, rc.LQ_BATCH) for r in fc.LQ_REGIMES for s in fc.LQ_MC_SHAPES + (fc.LQ_LANE_SHAPE,)])


@pytest.mark.parametrize("family,regime,shape,N,batch", X_LAM, ids=lambda v: str(v).replace(" ", ""))
def test_compute_x_lam_error(ocs, oracle, family, regime, shape, N, batch):
    """ocs.compute_x_lam_J on the regime's own controls and grid: x, J (the cost row's end) and lam.  The costate kernels
    without the convergence metric: k_costate_scan at N = 72 (k_costate_pl's workgroup count is below the scan's limit at
    these batches), the lane k_costate + k_pchip_mid at N = 13 and for LQ (5, 2), the matrix-core costate pass + k_pchip_mid
    for LQ (12, 2) and (32, 4)."""
    par, tspan, x0, u, ref, _, err_oracle = fc.x_lam_case(oracle, family, regime, shape, N, batch)
    g = ocs.RK4Integrator(tspan)
    x, lam, J = ocs.compute_x_lam_J(_problem(ocs, family, par), x0, tspan, u, integrator=g)
    assert np.all(lam[:, -1, :] == 0.0)
    if family == "lq":
        assert ocs.fb_sweep_matrix_core(g) == (1 if shape in fc.LQ_MC_SHAPES else 0)
    factor = None
    if regime == "B" and _state_pass_carries_z(family, "registry", shape, N, batch):
        factor = _factor(par, ref["x"])
    e = fc.errors({"x": x, "J": J, "lam": lam}, ref)
    check_ratios(f"compute_x_lam {family} {regime} {shape} N={N} batch={batch}", e, {k: err_oracle[k] for k in e}, factor)


# loop -> (options beside nSWEEPS / nINTERP_PTS, grid, error points on the nodes)
LOOPS = {4: ({}, "uniform", True), 2: ({"fused_update_off": 3}, "uniform", True), 1: ({"fused_update_off": 1}, "own", True),
         5: ({}, "own", False)}


def _sweep_params():
    out = []
    for regime in fc.LOGISTIC_REGIMES:
        for nS, N, batch in fc.LOGISTIC_SHAPES:
            for loop in ((4, 2, 1, 5) if N % 8 == 0 else (2, 1, 5)):     # (the fold takes whole blocks of 8 steps)
                out.append(("logistic", "registry", regime, nS, N, batch, loop, 3 if N == 72 else 2))
    for nS in (1, 2, 4):
        for loop in (4, 2):
            out.append(("logistic", "registry", "C-r3", nS, fc.BIG_N, fc.big_batch(nS), loop, 2))
    for regime in ("A", "C-r3"):
        for nS in (1, 2, 4):
            out.append(("logistic", "rows-cc", regime, nS, 72, 70, 4, 3))
        out.append(("logistic", "vector", regime, 2, 72, 70, 2, 3))
    for regime in fc.LQ_REGIMES:
        for shape in fc.LQ_MC_SHAPES + (fc.LQ_LANE_SHAPE,):
            for loop in (2, 1, 5):
                out.append(("lq", "registry", regime, shape, rc.LQ_N, rc.LQ_BATCH, loop, 3 if shape == (12, 2) else 2))
    return out


@pytest.mark.parametrize("family,form,regime,shape,N,batch,loop,kmax", _sweep_params(), ids=lambda v: str(v).replace(" ", ""))
def test_sweep_error(ocs, oracle, family, form, regime, shape, N, batch, loop, kmax):
    """ocs.fb_sweep_batch with nSWEEPS = k for k = 1 .. kmax (sweep 1 starts from the flag for u0 = lower bound, from sweep 2
    on the state pass forms its control from the costate of the sweep before: different kernels' work) and nINTERP_PTS =
    2N + 1 and 37: x, J, lam, u and every row of maxChange against the twin after the same k sweeps, the oracle's error
    after the same k sweeps as the yardstick.  k = 3 on the N = 72 logistic shapes and LQ (12, 2) only.

    loop 4 (options default), 2 (fused_update_off = 3), 1 (fused_update_off = 1) with nERROR_PTS = N + 1; loop 5 with
    nERROR_PTS = 41, off the nodes (twin and oracle use the same error points).  Loops 4 and 2 need the error points on
    the nodes, that is a uniform grid; loops 1 and 5 run on the regime's own grid (A random, C jittered).  At N = 13 the
    default options give loop 2 (the fold takes whole blocks of 8 steps), as they do for the LQ problem and the full-vector
    hipRTC form; ocs.fb_sweep_path is asserted each time.  The 130-workgroup batch is beyond costate_scan_ok's limit of
    128, so its loop 4 ran k_costate_plx<MET> where the other loop-4 cases ran k_costate_scan<MET> (module docstring)."""
    opts, grid, on_nodes = LOOPS[loop]
    if loop == 2 and (N % 8 != 0 or family == "lq" or form == "vector"):
        opts = {}                                       # the default options give loop 2 here: run those
    if family == "lq":
        grid = "own"                                    # (one grid: uniform)
    nE = N + 1 if on_nodes else fc.N_OFF_NODES
    tol = fc.tolerances(regime)
    for k in range(1, kmax + 1):
        par, tspan, x0, ref, _, err_oracle = fc.sweep_case(oracle, family, regime, shape, N, batch, grid, k, nE)
        prob = _problem(ocs, family, par, form)
        factor = None
        if regime == "B" and _state_pass_carries_z(family, form, shape, N, batch):
            factor = _factor(par, ref["x"])
        for nI in (2 * N + 1, fc.N_INTERP_OFF):
            g = ocs.RK4Integrator(tspan)
            r = ocs.fb_sweep_batch(prob, x0, tspan, dict(opts, nSWEEPS=k, nERROR_PTS=nE, nINTERP_PTS=nI, uRelTol=tol[0],
                                                         uAbsTol=tol[1]), integrator=g)
            assert ocs.fb_sweep_path(g) == loop, (ocs.fb_sweep_path(g), loop)
            if family == "lq":
                assert ocs.fb_sweep_matrix_core(g) == (1 if shape in fc.LQ_MC_SHAPES else 0)
            assert r["status"] == NOT_CONVERGED and np.all(r["sweeps"] == 0)
            got = {"x": r["x"], "J": r["J"], "lam": r["lam"], "u": r["u"], "maxChange": r["maxChange"]}
            e = fc.errors(got, ref, nI)
            yard = {name: (err_oracle[name][nI] if name == "u" else err_oracle[name]) for name in e}
            check_ratios(f"sweep {family} {form} {regime} {shape} N={N} batch={batch} loop={loop} k={k} nI={nI}", e, yard, factor)
