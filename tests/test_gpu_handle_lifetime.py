"""Device memory across a handle's life: what a handle (or a call) allocates is given back when it is destroyed (or returns).

Free device memory is read with torch.cuda.mem_get_info() after torch.cuda.synchronize(); the inputs are drawn once and stay
alive across both readings.  One warm-up round (code objects, the in-process and on-disk cache of compiled plugins, the pools of
the runtime and of torch) comes before the first reading; then 8 rounds; then the second reading.

The loss may not exceed BOUND = 16 MiB, the x array [nS + 1][N + 1][batch] of the one-state pass at batch 8192, N = 127.  (The
two-state operations hold arrays of 24 MiB, so the bound is below the largest buffer of a cycle: the stricter choice.)  A buffer
leaked once per round is therefore caught from BOUND / 8 = 2 MiB upward.  NOT covered, being smaller than that at these shapes:
the few-byte counters (nactive, nact_slots, the shooting driver's counter, the reduction block of ocs_multi), the parameter
blocks and bounds of a problem (d_ps, d_lb, d_ub), the grid tables of an integrator (d_HT, d_T, TC / TU / REC / RECS: O(N)
doubles), the pchip and point tables of the sweep workspace, the sparse basis of a control, every [batch]-sized array (J, status,
usel, dump: 64 KiB) and everything of the batch-64 operations (LQ weights and chunk workspace, the tail leg's d_utail /
d_lamtail / d_J2 at 64 trajectories: about 100 KiB together).  Streams, events and pinned host memory are not device memory."""
import gc

import numpy as np
import pytest

from tests.user_problems import LOGISTIC_ROWS_SRC, lq_matrices

pytestmark = pytest.mark.gpu
N, NF, B, BS = 127, 128, 8192, 64       # NF: the sweeps' grid (the folded sweep, path 4, needs N % 8 == 0); BS: the small batch
ROUNDS = 8
MIB = 1 << 20
BOUND = 8 * 2 * (N + 1) * B             # bytes of x [nS + 1 = 2][N + 1][B]
assert BOUND == 16 * MIB
C_, R_, M2 = 1.5, 0.05, [3.0, 2.5]
BOUNDS = [[0.0, 1.0]]
TSPAN, TSPAN_F = np.arange(N + 1) / 64.0, np.arange(NF + 1) / 64.0
TX = TSPAN[-1] + np.arange(41) / 20.0
OCS_ERR_INVALID = -1   # include/ocs.h


@pytest.fixture(scope="module")
def ocs():
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    import __graft_entry__ as g
    return g.load_package()


@pytest.fixture(scope="module")
def inputs():
    rng = np.random.default_rng(20261019)
    A, Bu, q, rdiag = lq_matrices(8, 2)
    return {
        "x0_1": rng.uniform(0.8, 2.0, (1, B)), "x0_2": rng.uniform(0.8, 2.0, (2, B)), "x0_2s": rng.uniform(0.8, 2.0, (2, BS)),
        "u": rng.uniform(0.05, 0.45, (1, 2 * N + 1, B)), "us": rng.uniform(0.05, 0.45, (1, 2 * N + 1, BS)),
        "cs": rng.uniform(1.0, 2.0, (1, B)), "V": rng.uniform(0.05, 0.45, (11, B)),
        "lq": (A, Bu, q, rdiag), "lq_x0": rng.normal(size=(8, BS)), "lq_u": rng.uniform(-1, 1, (2, 2 * N + 1, BS)),
        "lq_q": q[:, None] * rng.uniform(0.7, 1.3, (8, BS)), "lq_r": rdiag[:, None] * rng.uniform(0.7, 1.3, (2, BS)),
        "sx0": rng.uniform(0.8, 1.6, (1, B)),
        "t": rng.uniform(0, 2, 9), "y": rng.normal(1.5, 0.5, (3, 9)), "ue": rng.uniform(0, 1, (1, 9)), "v": rng.normal(size=(3, 9)),
    }


def free_bytes():
    import torch
    gc.collect()
    torch.cuda.synchronize()
    return torch.cuda.mem_get_info()[0]


def one_round(ocs, d):
    """creates, uses once and destroys one handle of every kind; returns the sweep paths it saw"""
    g = ocs.RK4Integrator(TSPAN)
    p1 = ocs.LogisticProblem(M2[:1], C_, R_, BOUNDS)
    g.compute_states(p1, d["x0_1"], d["u"])
    g.compute_adjoints(p1, d["u"])
    # RK4InfiniteIntegrator at a small batch: the tail leg on the wave-specialised kernels (d_utail, d_lamtail, d_J2)
    p2 = ocs.LogisticProblem(M2, C_, R_, BOUNDS)
    gi = ocs.RK4InfiniteIntegrator(TSPAN, TX, [0.4])
    gi.compute_states(p2, d["x0_2s"], d["us"])
    gi.compute_adjoints(p2, d["us"])
    # per-trajectory parameters (d_pb), two states
    p2.set_batch_params([0], d["cs"])
    g.compute_states(p2, d["x0_2"], d["u"])
    g.compute_adjoints(p2, d["u"])
    # LQ with per-trajectory weights (d_w, the chunk workspace)
    A, Bu, q, rdiag = d["lq"]
    plq = ocs.LQProblem(A, Bu, q, rdiag, R_, [[-1.0, 1.0]] * 2)
    plq.set_batch_weights(q=d["lq_q"], rdiag=d["lq_r"])
    g.compute_states(plq, d["lq_x0"], d["lq_u"])
    g.compute_adjoints(plq, d["lq_u"])
    # a hipRTC problem given as row functions
    pu = ocs.UserProblem(LOGISTIC_ROWS_SRC, 2, 1, [C_, R_] + M2, BOUNDS, row_separable=True)
    g.compute_states(pu, d["x0_2"], d["u"])
    g.compute_adjoints(pu, d["u"])
    # control + shooting objective
    c = ocs.PWLinearControl(g.t, 11, 1)
    ocs.nlp_objective(g, p1, c, d["x0_1"].copy(), d["V"])
    # host fb_sweep: enqueued ahead with the folded sweep, and kernel by kernel with the host waiting (fused_update_off = 1)
    gf = ocs.RK4Integrator(TSPAN_F)
    opts = {"nERROR_PTS": NF + 1, "nINTERP_PTS": 33, "nSWEEPS": 4}
    ocs.fb_sweep_batch(p1, d["sx0"], TSPAN_F, opts, integrator=gf)
    path_a = ocs.fb_sweep_path(gf)
    ocs.fb_sweep_batch(p1, d["sx0"], TSPAN_F, dict(opts, fused_update_off=1), integrator=gf)
    path_b = ocs.fb_sweep_path(gf)
    # batched single shooting, two iterations (its own integrator and control)
    ocs.single_shooting_batch(p1, d["x0_1"][:, :BS], TSPAN, 7, u0=0.2, MaxIter=2)
    # one-device ocs_multi with the reduced objective
    md = ocs.MultiDevice([0])
    _, _, st, _ = md.compute_states([g], [p1], d["x0_1"], d["u"], want_x=False)
    assert st["count"] == B
    # compute_equilibrium, F / dFdx_times_vec / ControlChar (temporaries of the call)
    big = [np.inf] * 2
    ocs.compute_equilibrium(ocs.LogisticProblem(M2, C_, R_, BOUNDS), [2.6, 2.1], [1.2, 1.2], [0.6], [0, 0, -np.inf, -np.inf, 0],
                            big + big + [np.inf], R_)
    p2.set_batch_params([], None)
    p2.F(d["t"], d["y"], d["ue"])
    p2.dFdx_times_vec(d["t"], d["y"], d["ue"], d["v"])
    p2.ControlChar(d["t"], d["y"][:2], d["v"][:2])
    del g, gi, gf, p1, p2, plq, pu, c, md
    gc.collect()
    return path_a, path_b


def test_handles_give_their_device_memory_back(ocs, inputs):
    """8 rounds of create / use / destroy over every handle kind lose at most BOUND bytes of free device memory."""
    paths = one_round(ocs, inputs)
    assert paths == (4, 1), paths
    before = free_bytes()
    for _ in range(ROUNDS):
        one_round(ocs, inputs)
    after = free_bytes()
    print(f"free device memory: {before} -> {after} bytes, loss {before - after} (bound {BOUND}, {ROUNDS} rounds)")
    assert before - after <= BOUND


def test_a_failing_call_gives_its_staged_arrays_back(ocs, inputs):
    """Host fb_sweep with a given start control and uRelax = 2: both staged arrays (u0 on the grid and on the error points, BIG
    bytes each) are on the device when the option check refuses the call with OCS_ERR_INVALID.  8 such calls lose at most BIG."""
    nE = 2 * NF + 1
    big = 8 * (2 * NF + 1) * B                     # u0 on the grid [2N + 1][nC = 1][B]; on the error points the same
    assert big >= 16 * MIB and 8 * nE * B >= 16 * MIB
    g = ocs.RK4Integrator(TSPAN_F)
    p = ocs.LogisticProblem(M2[:1], C_, R_, BOUNDS)
    opts = {"nERROR_PTS": nE, "nINTERP_PTS": 33, "nSWEEPS": 4, "uRelax": 2.0, "u0": lambda t: np.full((1, t.size), 0.3)}

    def refused():
        with pytest.raises(ocs.OcsError) as e:
            ocs.fb_sweep_batch(p, inputs["sx0"], TSPAN_F, opts, integrator=g)
        assert e.value.code == OCS_ERR_INVALID and "uRelax" in str(e.value)

    refused()
    before = free_bytes()
    for _ in range(ROUNDS):
        refused()
    after = free_bytes()
    print(f"free device memory: {before} -> {after} bytes, loss {before - after} (bound {big}, {ROUNDS} calls)")
    assert before - after <= big
