"""Per-trajectory parameters (OCProblem.set_batch_params, the mask path of ocs_problem_set_batch_params) on every index
and every kernel that reads them, against one CPU-oracle problem per trajectory built from that trajectory's own values
(the NumPy twin for the coupled hipRTC plugin).  Every trajectory of every batch is checked: the question is whether
each lane reads its own column of the table pb[k * B + b], and its own row k.

The index lists are passed unsorted and the values as len(index) x batch, so a transposed table, a table sorted by
assumption or a wrong user-to-functor index map fails.

Which case runs which kernel family with a parameter other than c per trajectory:

    lane kernels (ocs_rk4_kernels.hpp)                  test_integrator_passes_every_mapping[lane], nS = 1..4: all m_k
    row-split (ocs_rowsplit_kernels.hip)                ..[rowsplit], test_one_row_at_a_time[rowsplit]: m_k, one k at a time
    pipeline, adjoint + D wave (ocs_pipeline_kernels)   ..[pipeline], test_one_row_at_a_time[pipeline]
    pipeline-2, state pass (ocs_pipeline2_kernel.hpp)   ..[pipeline] / [auto], test_infinite_integrator (tail leg, u constant)
    scan (ocs_scan_kernel.hpp)                          ..[scan] / [auto], test_one_row_at_a_time[scan]
    vscan (ocs_vscan_kernel.hpp)                        ..[scan] at nS = 3 (registry), test_coupled_plugin[auto] (hipRTC)
    vector-lane state pass (ocs_pipelinev_kernel.hpp)   test_coupled_plugin[auto] at batch 64 and 66
    fold (ocs_fold_kernel.hpp) + costate scan with the
      convergence test (ocs_costate_scan_kernel.hpp)    test_fb_sweep[uniform-*-0], [ragged-*-0]: all m_k
    costate pipeline / lane costate, control grid
      (ocs_pipeline_kernels.hip, ocs_fbs_kernels.hip,
      ocs_control_kernels.hip)                          test_fb_sweep[*-1], [*-2], [*-3], [offnodes-*], [nonuniform-*]
    costate vscan (ocs_costate_vscan_kernel.hpp)        test_hand_written_logistic2_all_indices (fb_sweep part)
    fused control, one wave / two roles
      (ocs_fused_control_kernels.hip)                   test_fused_chebyshev_objective: all m_k
    fused control, wave kernels
      (ocs_fused_wave_kernels.hip)                      test_fused_wave_objective: m at index 2
    fused control, banded (ocs_fused_banded_kernels)    test_fused_banded_objective: all m_k
    equilibrium solver (k_equilibrium)                  test_equilibrium_batched: m through user index 1 of TestOCProblem
    hipRTC register copy behind OCS_PARAMS              test_hand_written_logistic2_all_indices, test_coupled_plugin
    LQProblem, entries of A and Bu                      test_lq_entries_of_A_and_Bu_are_refused_not_ignored

Tolerances are those of the tests whose shapes a case borrows; each docstring names the test."""
import numpy as np
import pytest

from oracle import np_twin as tw
from tests.user_problems import LOGISTIC2_SRC, PREDPREY_PARAMS, PREDPREY_SRC, PredPreyNP, lq_matrices

pytestmark = pytest.mark.gpu
P = {"c": 1.5, "m": 3.0, "r": 0.05}
BOUNDS = [[0.0, 1.0]]
RTOL = 1e-12          # tests/test_gpu_rk4_parity.py, test_gpu_controls_shooting.py, test_gpu_user_problems.py, test_gpu_lq.py
RTOL_SWEEP = 1e-10    # tests/test_gpu_fb_sweep.py
OCS_ERR_INVALID, OCS_ERR_SHAPE, OCS_ERR_UNSUPPORTED = -1, -2, -6
_REF = {}             # references shared by the cases of a parametrised test (computed once, never written again)


def relerr(a, b):
    """max |a-b| / max(1,|b|) (tests/test_gpu_rk4_parity.py); entries that are non-finite in the reference must match exactly."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    bad = ~np.isfinite(b)
    if bad.any():
        same = (np.isnan(a[bad]) & np.isnan(b[bad])) | (a[bad] == b[bad])
        if not same.all():
            return float("inf")
    ok = ~bad
    if not ok.any():
        return 0.0
    with np.errstate(invalid="ignore"):
        e = np.abs(a[ok] - b[ok]) / np.maximum(1.0, np.abs(b[ok]))
    return float("inf") if np.isnan(e).any() else float(np.max(e))


@pytest.fixture(scope="module")
def ocs():
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    import __graft_entry__ as g
    return g.load_package()


def _inputs(oracle, nS, N, batch, seed, T=10.0):
    """x0 ~ U(0.8, 2.5), u in [0.05, 0.45]: _inputs of tests/test_gpu_rk4_parity.py"""
    rng = np.random.default_rng(seed)
    tspan = oracle.linspace(0.0, T, N + 1)
    t = np.zeros(2 * N + 1)
    t[0::2] = tspan
    t[1::2] = (tspan[:-1] + tspan[1:]) / 2
    f, ph = rng.uniform(0, 1, batch), rng.uniform(0, 2 * np.pi, batch)
    u = np.clip(0.25 + 0.2 * np.sin(2 * np.pi * f[None, :] * t[:, None] + ph[None, :]), 0, 1)
    u = np.asfortranarray(u[None, :, :])
    x0 = rng.uniform(0.8, 2.5, (nS, batch))
    return tspan, x0, u


def _draw_cm(seed, nS, batch, mlo=1.5, mhi=3.0):
    rng = np.random.default_rng(seed)
    return rng.uniform(1.0, 2.0, batch), rng.uniform(mlo, mhi, (nS, batch))


def _set_c_and_m(prob, cs, ms):
    """LogisticK block [c r m_1..m_nS]: c and every m_k per trajectory, the index list unsorted (last row first), values
    len(index) x batch in that order."""
    nS = ms.shape[0]
    index = [2 + nS - 1, 0] + list(range(2, 2 + nS - 1))
    prob.set_batch_params(index, np.vstack([ms[nS - 1], cs] + [ms[k] for k in range(nS - 1)]))


def _oracle_passes(oracle, make, tspan, x0, u, lamT):
    """x, J, lam, dJdu (default lamT) and lam, dJdu (explicit lamT) of every trajectory, trajectory b on make(b)"""
    go = oracle.RK4Integrator(tspan)
    batch = x0.shape[1]
    out = {k: [] for k in ("x", "J", "lam", "dJdu", "lam2", "d2")}
    for b in range(batch):
        po = make(b)
        xo, Jo = go.compute_states(po, x0[:, b], u[:, :, b])
        lamo, do = go.compute_adjoints(po, u[:, :, b])
        l2, d2 = go.compute_adjoints(po, u[:, :, b], lamT[:, b])
        for k, v in zip(out, (xo, Jo, lamo, do, l2, d2)):
            out[k].append(v)
    return {k: (np.array(v) if k == "J" else np.stack(v, axis=-1)) for k, v in out.items()}


def _check_passes(g, pg, x0, u, lamT, ref, what=""):
    x, J = g.compute_states(pg, x0, u)
    lam, dJdu = g.compute_adjoints(pg, u)
    lam2, d2 = g.compute_adjoints(pg, u, lamT)
    errs = {"x": relerr(x, ref["x"]), "J": relerr(J, ref["J"]), "lam": relerr(lam, ref["lam"]),
            "dJdu": relerr(dJdu, ref["dJdu"]), "lam(lamT)": relerr(lam2, ref["lam2"]), "dJdu(lamT)": relerr(d2, ref["d2"])}
    print(what, errs)
    assert max(errs.values()) < RTOL, (what, errs)
    assert np.all(lam[-1] == 1.0)


# ---- 1. integrator passes, every mapping ---------------------------------------------------------------------------
SHAPES = [(4, 16, 64, 0.8), (2, 40, 96, 2.0), (4, 48, 32, 2.0), (2, 17, 33, 0.8), (4, 24, 3, 1.0), (4, 37, 1, 2.0),
          (2, 9, 129, 0.5), (4, 7, 16, 0.3), (3, 9, 5, 0.4), (1, 37, 70, 2.0)]


def _logistic_case(oracle, nS, N, batch, T):
    key = ("passes", nS, N, batch)
    if key not in _REF:
        tspan, x0, u = _inputs(oracle, nS, N, batch, seed=300 + nS + N, T=T)
        cs, ms = _draw_cm(17 * N + batch, nS, batch)
        lamT = np.random.default_rng(1).normal(size=(nS + 1, batch))
        ref = _oracle_passes(oracle, lambda b: oracle.LogisticProblem(ms[:, b], cs[b], P["r"], BOUNDS), tspan, x0, u, lamT)
        assert np.all(np.isfinite(ref["x"])) and np.max(np.abs(ref["x"][:nS])) < 3.0
        _REF[key] = (tspan, x0, u, cs, ms, lamT, ref)
    return _REF[key]


@pytest.mark.parametrize("nS,N,batch,T", SHAPES)
@pytest.mark.parametrize("mapping", ["auto", "lane", "rowsplit", "pipeline", "scan"])
def test_integrator_passes_every_mapping(ocs, oracle, nS, N, batch, T, mapping):
    """LogisticProblem with c and every m_k per trajectory (m ~ U(1.5, 3), c ~ U(1, 2)) on the shapes of
    test_both_mappings_match_oracle (tests/test_gpu_rk4_parity.py: whole and ragged tiles, batches below a tile, N % 8 != 0,
    N < 8) plus (3, 9, 5) and (1, 37, 70): x, J, lam and dJdu of EVERY trajectory with the default and an explicit lamT, at that
    file's RTOL.  A forced mapping that does not admit a shape refuses it with -6 as in that test: row-split needs 2 or 4
    states; the pipeline kernels need N >= 8 and whole tiles of 64 / nS trajectories (the state pass also a ragged last tile
    of an even batch beyond one tile; nS = 3 has the vector-lane state pass only, tiles of 64); the scan needs N >= 4."""
    tspan, x0, u, cs, ms, lamT, ref = _logistic_case(oracle, nS, N, batch, T)
    pg = ocs.LogisticProblem([3.0, 2.5, 2.0, 1.5][:nS], P["c"], P["r"], BOUNDS)
    _set_c_and_m(pg, cs, ms)
    g = ocs.RK4Integrator(tspan).set_mapping(mapping)
    tile = 64 if nS == 3 else 64 // nS
    ragged = batch % tile != 0
    no_states = ((mapping == "rowsplit" and nS not in (2, 4)) or
                 (mapping == "pipeline" and (N < 8 or (ragged and (batch < tile or batch % 2 != 0)))))
    if no_states:
        with pytest.raises(ocs.OcsError) as e:
            g.compute_states(pg, x0, u)
        assert e.value.code == OCS_ERR_UNSUPPORTED
        return
    if (mapping == "pipeline" and ragged) or (mapping == "scan" and N < 4):
        x, J = g.compute_states(pg, x0, u)
        assert relerr(x, ref["x"]) < RTOL and relerr(J, ref["J"]) < RTOL
        with pytest.raises(ocs.OcsError) as e:
            g.compute_adjoints(pg, u)
        assert e.value.code == OCS_ERR_UNSUPPORTED
        return
    _check_passes(g, pg, x0, u, lamT, ref, f"{mapping} {(nS, N, batch)}")


# ---- 2. one row at a time -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [0, 1, 2, 3])
@pytest.mark.parametrize("mapping", ["rowsplit", "pipeline", "scan"])
def test_one_row_at_a_time(ocs, oracle, mapping, k):
    """nS = 4 on the row-per-lane kernels with m_k ALONE per trajectory (index 2 + k), everything else shared: a lane that
    reads pb at the wrong row then fails for every k but its own, one that reads the wrong column fails for every k.
    (4, 16, 48): three tiles of 16 trajectories, two blocks of 8 steps, four scan chunks; every trajectory, RTOL of
    tests/test_gpu_rk4_parity.py."""
    nS, N, batch, T = 4, 16, 48, 0.8
    m = [3.0, 2.5, 2.0, 1.5]
    key = ("row", k)
    if key not in _REF:
        tspan, x0, u = _inputs(oracle, nS, N, batch, seed=40 + k, T=T)
        mk = np.random.default_rng(50 + k).uniform(1.5, 3.0, batch)
        lamT = np.random.default_rng(2).normal(size=(nS + 1, batch))
        ref = _oracle_passes(oracle, lambda b: oracle.LogisticProblem(m[:k] + [mk[b]] + m[k + 1:], P["c"], P["r"], BOUNDS),
                             tspan, x0, u, lamT)
        _REF[key] = (tspan, x0, u, mk, lamT, ref)
    tspan, x0, u, mk, lamT, ref = _REF[key]
    pg = ocs.LogisticProblem(m, P["c"], P["r"], BOUNDS)
    pg.set_batch_params([2 + k], mk[None, :])
    _check_passes(ocs.RK4Integrator(tspan).set_mapping(mapping), pg, x0, u, lamT, ref, f"{mapping} m_{k + 1}")


# ---- 3. TestOCProblem: user order [c m r], functor order [c r m] ---------------------------------------------------
@pytest.mark.parametrize("index", [[1], [1, 0]])
@pytest.mark.parametrize("mapping", ["auto", "lane", "pipeline"])
def test_testocproblem_user_order(ocs, oracle, index, mapping):
    """TestOCProblem's parameters are given as [c m r] and kept as [c r m]: user index 1 (m) alone and [1, 0] (m, c) together,
    every trajectory of (1, 40, 128) (two tiles of 64, five blocks: the pipeline kernels take it) at the RTOL of
    tests/test_gpu_rk4_parity.py (test_per_trajectory_parameters)."""
    N, batch = 40, 128
    key = ("testoc", tuple(index))
    if key not in _REF:
        tspan, x0, u = _inputs(oracle, 1, N, batch, seed=5, T=2.0)
        cs, ms = _draw_cm(6, 1, batch)
        vals = {0: cs, 1: ms[0]}
        lamT = np.random.default_rng(3).normal(size=(2, batch))
        pb = lambda b: {"c": cs[b] if 0 in index else P["c"], "m": ms[0, b], "r": P["r"]}
        ref = _oracle_passes(oracle, lambda b: oracle.TestOCProblem(pb(b), BOUNDS), tspan, x0, u, lamT)
        _REF[key] = (tspan, x0, u, np.vstack([vals[i] for i in index]), lamT, ref)
    tspan, x0, u, values, lamT, ref = _REF[key]
    pg = ocs.TestOCProblem(P, BOUNDS)
    pg.set_batch_params(index, values)
    _check_passes(ocs.RK4Integrator(tspan).set_mapping(mapping), pg, x0, u, lamT, ref, f"{mapping} index {index}")


# ---- 4. refusal, clear, mismatch ------------------------------------------------------------------------------------
def test_refusal_clear_and_mismatch(ocs, oracle):
    """User index 2 (r) of TestOCProblem feeds the time-coefficient table: refused alone and inside a larger set
    (OCS_ERR_UNSUPPORTED), an index out of range is OCS_ERR_INVALID, and a refused call leaves the per-trajectory state that
    was in force: results before and after are bit-identical.  A call with another batch is OCS_ERR_SHAPE;
    set_batch_params([], None) restores the shared-parameter results bit for bit and any batch is accepted again."""
    N, batch = 37, 70
    tspan, x0, u = _inputs(oracle, 1, N, batch, seed=9, T=2.0)
    cs, ms = _draw_cm(10, 1, batch)
    pg = ocs.TestOCProblem(P, BOUNDS)
    g = ocs.RK4Integrator(tspan)

    def run():
        x, J = g.compute_states(pg, x0, u)
        lam, dJdu = g.compute_adjoints(pg, u)
        return x, J, lam, dJdu
    shared = run()
    pg.set_batch_params([1, 0], np.vstack([ms[0], cs]))
    before = run()
    assert not np.array_equal(shared[1], before[1])
    other = np.full((1, batch), 0.07)
    for index, values, code in (([2], other, OCS_ERR_UNSUPPORTED), ([0, 2, 1], np.vstack([cs, other, cs]), OCS_ERR_UNSUPPORTED),
                                ([1, 2], np.vstack([cs, other]), OCS_ERR_UNSUPPORTED), ([3], other, OCS_ERR_INVALID),
                                ([-1], other, OCS_ERR_INVALID), ([0, 3], np.vstack([cs + 1.0, other]), OCS_ERR_INVALID)):
        with pytest.raises(ocs.OcsError) as e:
            pg.set_batch_params(index, values)
        assert e.value.code == code, index
        after = run()
        for a, b in zip(before, after):
            assert np.array_equal(a, b), index
    with pytest.raises(ocs.OcsError) as e:
        g.compute_states(pg, x0[:, :batch - 1], u[:, :, :batch - 1])
    assert e.value.code == OCS_ERR_SHAPE
    with pytest.raises(ocs.OcsError) as e:
        ocs.fb_sweep_batch(pg, x0[:, :5], tspan, {"nERROR_PTS": N + 1, "nINTERP_PTS": 9, "nSWEEPS": 2})
    assert e.value.code == OCS_ERR_SHAPE
    pg.set_batch_params([], None)
    for a, b in zip(shared, run()):
        assert np.array_equal(a, b)
    g.compute_states(pg, x0[:, :batch - 1], u[:, :, :batch - 1])   # any batch again


# ---- 5. RK4InfiniteIntegrator ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("nS,N,N2,batch", [(2, 64, 64, 96), (4, 48, 40, 32), (2, 64, 60, 96), (2, 64, 64, 70)])
def test_infinite_integrator(ocs, oracle, nS, N, N2, batch):
    """RK4InfiniteIntegrator (both legs; the tail leg under the constant control uStar on the wave-specialised kernels, split
    at N2 = 60, on the lane kernels for the ragged batch 70) with c and every m_k per trajectory: the nS = 2 and 4 shapes
    of test_infinite_integrator_tail_leg_mappings (tests/test_gpu_controls_shooting.py), its inputs and RTOL, every
    trajectory."""
    us = 0.4
    tspan, tx = oracle.linspace(0, 2.0, N + 1), oracle.linspace(2.0, 4.0, N2 + 1)
    rng = np.random.default_rng(N + N2 + batch)
    u = rng.uniform(0.05, 0.45, (1, 2 * N + 1, batch))
    x0 = rng.uniform(0.8, 2.0, (nS, batch))
    cs, ms = _draw_cm(N2 + batch, nS, batch)
    pg = ocs.LogisticProblem([3.0, 2.5, 2.0, 1.5][:nS], P["c"], P["r"], BOUNDS)
    _set_c_and_m(pg, cs, ms)
    gi, go = ocs.RK4InfiniteIntegrator(tspan, tx, [us]), oracle.RK4InfiniteIntegrator(tspan, tx, [us])
    x, J = gi.compute_states(pg, x0, u)
    lam, dJdu = gi.compute_adjoints(pg, u)
    worst = 0.0
    for b in range(batch):
        po = oracle.LogisticProblem(ms[:, b], cs[b], P["r"], BOUNDS)
        xo, Jo = go.compute_states(po, x0[:, b], u[:, :, b])
        lamo, do = go.compute_adjoints(po, u[:, :, b])
        errs = (relerr(x[:, :, b], xo), abs(J[b] - Jo) / abs(Jo), relerr(lam[:, :, b], lamo), relerr(dJdu[:, :, b], do))
        worst = max(worst, *errs)
        assert max(errs) < RTOL, (b, errs)
    print("worst x / J / lam / dJdu error", worst)


# ---- 6. fb_sweep_batch ----------------------------------------------------------------------------------------------
def _sweep_case(oracle, kind, nS, N, batch):
    """Problem data of a sweep case and the oracle's solution of every instance (shared by the loops run on it)."""
    key = ("sweep", kind, nS, N, batch)
    if key in _REF:
        return _REF[key]
    rng = np.random.default_rng(1000 * nS + N + batch)
    nerr = N + 1
    if kind == "uniform":          # step 2^-5: bitwise uniform (test_fold_on_a_bitwise_uniform_grid)
        tspan = np.arange(N + 1) / 32.0
    elif kind == "nonuniform":     # steps within a factor of the mean; the evenly spaced error points are no grid nodes
        tspan = 0.5 * (np.concatenate([[0.0], np.sort(rng.uniform(0, 1.0, N - 1)), [1.0]]) + oracle.linspace(0, 1.0, N + 1))
    else:                          # "ragged", "offnodes": T = 1 (test_two_kernel_sweep_on_ragged_batches)
        tspan = oracle.linspace(0, 1.0, N + 1)
        if kind == "offnodes":
            nerr = N + 8
    x0 = rng.uniform(0.8, 2.0, (nS, batch))
    cs, ms = rng.uniform(1.0, 2.0, batch), rng.uniform(2.0, 3.0, (nS, batch))
    opts = {"nERROR_PTS": nerr, "nINTERP_PTS": 33, "nSWEEPS": 40}
    refs = []
    for b in range(batch):
        ref = oracle.fb_sweep(oracle.LogisticProblem(ms[:, b], cs[b], P["r"], BOUNDS), x0[:, b], tspan, opts)
        assert ref["_sweeps"] > 0, (b, "the oracle's sweep did not converge: no reference")
        refs.append(ref)
    _REF[key] = (tspan, x0, cs, ms, opts, refs)
    return _REF[key]


SWEEPS = ([("uniform", nS, N, batch, off) for nS, N, batch in ((1, 64, 64), (2, 96, 64), (4, 40, 32)) for off in (0, 1, 2, 3)] +
          [("ragged", nS, 64, batch, off) for nS, batch in ((1, 70), (2, 34), (4, 22)) for off in (0, 1)] +
          [("ragged", 2, 16, 33, 0), ("ragged", 4, 40, 23, 0)] +
          [("offnodes", 1, 64, 70, 0), ("offnodes", 2, 16, 33, 0), ("offnodes", 4, 64, 22, 0)] +
          [("nonuniform", 1, 64, 70, 0), ("nonuniform", 2, 96, 64, 0), ("nonuniform", 4, 40, 23, 0)])


@pytest.mark.parametrize("kind,nS,N,batch,off", SWEEPS, ids=[f"{k}-{s}x{n}x{b}-{o}" for k, s, n, b, o in SWEEPS])
def test_fb_sweep(ocs, oracle, kind, nS, N, batch, off):
    """fb_sweep_batch with c and every m_k per trajectory (m ~ U(2, 3), c ~ U(1, 2), x0 ~ U(0.8, 2), T = 1, nSWEEPS = 40,
    nINTERP_PTS = 33), every sweep loop the tests of tests/test_gpu_fb_sweep.py reach: the two-kernel sweep on a bitwise
    uniform grid (test_fold_on_a_bitwise_uniform_grid) and on ragged even batches beyond one tile
    (test_two_kernel_sweep_on_ragged_batches: path 4), fused_update_off = 1 (path 1, same test), 2 and 3
    (test_fused_costate_update_equals_separate_kernels: the fused control update without the fold, path 2 of
    ocs.fb_sweep_path), odd ragged batches (no fold: path 2), error points off the nodes (N + 8 of them) and a non-uniform
    grid (path 5, as test_fb_sweep_two_kernel_sweep_for_user_row_functions asserts for its "rand" grid).  Every instance
    against oracle.fb_sweep of its own problem: sweep count (from the oracle, which must have converged), x, lam, u, J at
    that file's RTOL = 1e-10, the recorded change at its 1e-6, NaN in maxChange exactly after the last sweep."""
    tspan, x0, cs, ms, opts, refs = _sweep_case(oracle, kind, nS, N, batch)
    pg = ocs.LogisticProblem([3.0, 2.5, 2.0, 1.5][:nS], P["c"], P["r"], BOUNDS)
    _set_c_and_m(pg, cs, ms)
    g = ocs.RK4Integrator(tspan)
    r = ocs.fb_sweep_batch(pg, x0, tspan, dict(opts, fused_update_off=off), integrator=g)
    if kind in ("offnodes", "nonuniform"):
        path = 5
    elif off == 1:
        path = 1
    elif off == 0 and batch % 2 == 0:
        path = 4
    else:
        path = 2
    assert ocs.fb_sweep_path(g) == path
    worst = 0.0
    for b, ref in enumerate(refs):
        k = ref["_sweeps"]
        assert r["sweeps"][b] == k, (b, r["sweeps"][b], k)
        mc = r["maxChange"][:, b]
        assert np.all(np.isnan(mc[k:])) and not np.any(np.isnan(mc[:k])), b
        assert relerr(mc[:k], ref["_maxChange"][:k]) < 1e-6, b
        errs = (abs(r["J"][b] - ref["J"]) / abs(ref["J"]), relerr(r["x"][:, :, b], ref["x"]),
                relerr(r["lam"][:, :, b], ref["lam"]), relerr(r["u"][:, :, b], ref["u"]))
        worst = max(worst, *errs)
        assert max(errs) < RTOL_SWEEP, (b, errs)
    print("sweeps", sorted(set(int(ref["_sweeps"]) for ref in refs)), "worst J / x / lam / u error", worst)


@pytest.mark.parametrize("nS,N,batch", [(1, 64, 70), (2, 96, 64), (4, 40, 23)])
def test_compute_x_lam(ocs, oracle, nS, N, batch):
    """compute_x_lam and compute_x_lam_J on the problems of test_fb_sweep (non-uniform grid) with a given control: every
    instance against oracle.compute_x_lam at the 1e-12 of test_compute_x_lam_matches_oracle (tests/test_gpu_fb_sweep.py)."""
    tspan, x0, cs, ms, _, _ = _sweep_case(oracle, "nonuniform", nS, N, batch)
    pg = ocs.LogisticProblem([3.0, 2.5, 2.0, 1.5][:nS], P["c"], P["r"], BOUNDS)
    _set_c_and_m(pg, cs, ms)
    u = np.random.default_rng(N).uniform(0.05, 0.45, (1, 2 * N + 1, batch))
    x, lam, J = ocs.compute_x_lam_J(pg, x0, tspan, u)
    x2, lam2 = ocs.compute_x_lam(pg, x0, tspan, u)
    assert np.array_equal(x, x2) and np.array_equal(lam, lam2)
    go = oracle.RK4Integrator(tspan)
    for b in range(batch):
        po = oracle.LogisticProblem(ms[:, b], cs[b], P["r"], BOUNDS)
        xo, lo, Jo = oracle.compute_x_lam(go, po, x0[:, b], u[:, :, b], want_J=True)
        assert relerr(x[:, :, b], xo) < 1e-12 and relerr(lam[:, :, b], lo) < 1e-12, b
        assert abs(J[b] - Jo) < 1e-12 * max(1.0, abs(Jo)), b
    assert np.all(lam[:, -1, :] == 0.0)


# ---- 7. fused control objective -------------------------------------------------------------------------------------
def _check_objective(ocs, oracle, g, go, pg, cg, co, make, x0, V, free, modes):
    """J, dJdv and the initial state after nlp_objective of every candidate against the oracle's unfused composition on
    make(b), in every fusion mode"""
    batch = V.shape[1]
    ref = [oracle.nlp_objective(go, make(b), co, x0[:, b], V[:, b], FreeInitStates=free) for b in range(batch)]
    for mode in modes:
        cg.set_fusion(mode)
        J, dJdv, x0n = ocs.nlp_objective(g, pg, cg, x0.copy(), V, FreeInitStates=free)
        worst = 0.0
        for b, (Jo, do, x0o) in enumerate(ref):
            errs = (abs(J[b] - Jo) / max(1.0, abs(Jo)), relerr(dJdv[:, b], do))
            worst = max(worst, *errs)
            assert max(errs) < RTOL, (mode, b, errs)
            assert np.array_equal(x0n[:, b], x0o), (mode, b)
        print("fusion", mode, "worst J / dJdv error", worst)
    cg.set_fusion("auto")


@pytest.mark.parametrize("nS,nB,N,batch", [(1, 5, 7, 3), (4, 32, 64, 64), (3, 1, 9, 65), (2, 12, 48, 130), (1, 3, 24, 64)])
def test_fused_chebyshev_objective(ocs, oracle, nS, nB, N, batch):
    """nlp_objective with ChebyshevControl applied inside the RK4 kernels, c and every m_k per trajectory, free initial
    states: shapes, candidates and RTOL of test_fused_control_objective_gradient (tests/test_gpu_controls_shooting.py) --
    (1, 5, 7, 3), (4, 32, 64, 64) and (3, 1, 9, 65) run the one-wave lane kernels, (2, 12, 48, 130) the two-role kernels
    (N % 8 == 0, nB <= 16, nS <= 2), (1, 3, 24, 64) the lane kernels under "lane" and the wave kernels under "on".  Every
    candidate against the oracle in the modes "on", "lane" and "off"."""
    T = 10.0 if N >= 50 else 1.0
    tspan = oracle.linspace(0, T, N + 1)
    g, go = ocs.RK4Integrator(tspan), oracle.RK4Integrator(tspan)
    cg, co = ocs.ChebyshevControl(g.t, nB, 1), oracle.ChebyshevControl(go.t, nB, 1)
    rng = np.random.default_rng(nB * 100 + N)
    free = [nS, 1] if nS > 1 else [1]
    V = 0.05 * rng.normal(size=(nB, batch)) / np.arange(1, nB + 1)[:, None]
    V[0] += 0.4
    V = np.vstack([V, rng.uniform(0.8, 1.6, (len(free), batch))])
    x0 = rng.uniform(0.8, 1.5, (nS, batch))
    cs, ms = _draw_cm(nB + N, nS, batch, 2.0, 3.0)
    pg = ocs.LogisticProblem([3.0, 2.5, 2.0, 1.5][:nS], P["c"], P["r"], BOUNDS)
    _set_c_and_m(pg, cs, ms)
    _check_objective(ocs, oracle, g, go, pg, cg, co, lambda b: oracle.LogisticProblem(ms[:, b], cs[b], P["r"], BOUNDS),
                     x0, V, free, ("on", "lane", "off"))


@pytest.mark.parametrize("nB,N,batch,grid", [(5, 8, 64, "lin"), (1, 72, 64, "lin"), (32, 64, 192, "rand")])
def test_fused_wave_objective(ocs, oracle, nB, N, batch, grid):
    """The wave kernels of csrc/ocs_fused_wave_kernels.hip (wave-specialised state pass, adjoint scan, basis products on the
    matrix cores; nS = 1) with m (index 2 of LogisticK's block) and c per trajectory: the three smallest shapes of
    test_fused_control_wave_kernels (tests/test_gpu_controls_shooting.py: one and two superblocks, one and eight k-steps,
    three workgroups, a non-uniform grid), its candidates and RTOL, every candidate, modes "on", "lane" and "off"."""
    rng = np.random.default_rng(nB * 1000 + N)
    T = 10.0 if N >= 50 else 1.0
    tspan = {"lin": oracle.linspace(0, T, N + 1),
             "rand": np.concatenate([[0.0], np.sort(rng.uniform(0, T, N - 1)), [T]])}[grid]
    g, go = ocs.RK4Integrator(tspan), oracle.RK4Integrator(tspan)
    cg, co = ocs.ChebyshevControl(g.t, nB, 1), oracle.ChebyshevControl(go.t, nB, 1)
    V = 0.05 * rng.normal(size=(nB, batch)) / np.arange(1, nB + 1)[:, None]
    V[0] += 0.4
    V = np.vstack([V, rng.uniform(0.8, 1.6, (1, batch))])
    x0 = rng.uniform(0.8, 1.5, (1, batch))
    cs, ms = _draw_cm(nB + N, 1, batch, 2.0, 3.0)
    pg = ocs.LogisticProblem([3.0], P["c"], P["r"], BOUNDS)
    pg.set_batch_params([2, 0], np.vstack([ms[0], cs]))
    _check_objective(ocs, oracle, g, go, pg, cg, co, lambda b: oracle.LogisticProblem(ms[:, b], cs[b], P["r"], BOUNDS),
                     x0, V, [1], ("on", "lane", "off"))


@pytest.mark.parametrize("kind,nS,nB,N,batch", [("lin", 1, 2, 7, 3), ("lin", 2, 11, 50, 130), ("lin", 4, 33, 64, 64),
                                                ("const", 2, 1, 9, 65), ("const", 4, 7, 50, 33), ("const", 1, 100, 50, 4)])
def test_fused_banded_objective(ocs, oracle, kind, nS, nB, N, batch):
    """PWLinearControl and PWConstantControl applied inside the RK4 kernels (csrc/ocs_fused_banded_kernels.hip) with c and
    every m_k per trajectory, free initial states: the small shapes of test_fused_banded_control_objective_gradient
    (tests/test_gpu_controls_shooting.py; (4, 33, 64, 64) on its non-uniform grid, (1, 100, 50, 4) with more control points
    than the fused kernels take), its candidates and RTOL, every candidate, modes "on", "lane" and "off"."""
    T = 10.0 if N >= 50 else 1.0
    rng = np.random.default_rng(nB * 100 + N)
    tspan = oracle.linspace(0, T, N + 1) if N != 64 else np.concatenate([[0.0], np.sort(rng.uniform(0, T, N - 1)), [T]])
    g, go = ocs.RK4Integrator(tspan), oracle.RK4Integrator(tspan)
    Cg, Co = (ocs.PWLinearControl, oracle.PWLinearControl) if kind == "lin" else (ocs.PWConstantControl, oracle.PWConstantControl)
    cg, co = Cg(g.t, nB, 1), Co(go.t, nB, 1)
    free = [nS, 1] if nS > 1 else [1]
    V = np.vstack([rng.uniform(0.05, 0.45, (nB, batch)), rng.uniform(0.8, 1.6, (len(free), batch))])
    x0 = rng.uniform(0.8, 1.5, (nS, batch))
    cs, ms = _draw_cm(nB + N, nS, batch, 2.0, 3.0)
    pg = ocs.LogisticProblem([3.0, 2.5, 2.0, 1.5][:nS], P["c"], P["r"], BOUNDS)
    _set_c_and_m(pg, cs, ms)
    _check_objective(ocs, oracle, g, go, pg, cg, co, lambda b: oracle.LogisticProblem(ms[:, b], cs[b], P["r"], BOUNDS),
                     x0, V, free, ("on", "lane", "off"))


# ---- 8. compute_equilibrium -----------------------------------------------------------------------------------------
def _testoc_equilibrium(c, m, r):
    """interior root of TestOCProblem's optimality system (tests/test_gpu_controls_shooting.py, _testoc_equilibrium):
    (r - m + 2 x) c (m - x) = 1 on the branch x in ((3 m - r) / 4, m), u = x (m - x), lam = 2 c u"""
    f = lambda x: (r - m + 2 * x) * c * (m - x) - 1.0
    lo, hi = (3 * m - r) / 4, m
    for _ in range(200):
        mid = 0.5 * (lo + hi)
        lo, hi = (mid, hi) if f(mid) > 0 else (lo, mid)
    x = 0.5 * (lo + hi)
    u = x * (m - x)
    return x, 2 * c * u, u


def test_equilibrium_batched(ocs):
    """compute_equilibrium on 257 instances of TestOCProblem (four waves and one lane) with m and c per instance through user
    indices [1, 0] (c ~ U(1.2, 2) as in test_compute_equilibrium_batched_on_device of tests/test_gpu_controls_shooting.py,
    m ~ U(3.0, 3.5): the root stays inside 0.5 < u < 0.95), the reference's guess and bounds: every instance against the analytic
    root of ITS c and m at that test's 1e-11, exitflag 1, residual norm < 1e-24."""
    B = 257
    rng = np.random.default_rng(21)
    cs, ms = rng.uniform(1.2, 2.0, B), rng.uniform(3.0, 3.5, B)
    ref = np.array([_testoc_equilibrium(c, m, P["r"]) for c, m in zip(cs, ms)]).T
    assert np.all(ref[2] > 0.05) and np.all(ref[2] < 0.95)     # interior: the bounds of u stay inactive
    prob = ocs.TestOCProblem(P, BOUNDS)
    prob.set_batch_params([1, 0], np.vstack([ms, cs]))
    lb, ub = [0.0, -np.inf, 0.0], [np.inf, np.inf, 1.0]
    xG, lG, uG = np.full((1, B), 2.7), np.full((1, B), 2.2), np.full((1, B), 0.7)
    xs, ls, us, resnorm, _, flag = ocs.compute_equilibrium(prob, xG, lG, uG, lb, ub, P["r"])
    assert np.all(flag == 1) and np.max(resnorm) < 1e-24
    errs = [float(np.max(np.abs(a[0] - b))) for a, b in zip((xs, ls, us), ref)]
    print("x / lam / u error", errs)
    assert max(errs) < 1e-11


# ---- 9. single_shooting_batch ---------------------------------------------------------------------------------------
def test_single_shooting_batch_instances_are_independent(ocs):
    """single_shooting_batch on a two-state LogisticProblem with c, m_1 and m_2 per instance: instance b equals instance b of
    the same driver on a shared-parameter problem built from b's values (same batch, same start), for every b -- J[b] and
    v[:, b] to RTOL scaled by max(1, |.|), equal iteration counts, MaxIter = 6: the form and the tolerance of
    test_single_shooting_batch_instances_are_independent (tests/test_gpu_lq_batch_weights.py)."""
    nS, N, batch = 2, 64, 6
    rng = np.random.default_rng(8)
    tspan = np.linspace(0.0, 2.0, N + 1)
    x0 = rng.uniform(0.8, 2.0, (nS, batch))
    cs, ms = _draw_cm(9, nS, batch, 2.0, 3.0)
    pg = ocs.LogisticProblem([3.0, 2.5], P["c"], P["r"], BOUNDS)
    _set_c_and_m(pg, cs, ms)
    kw = dict(u0=0.2, TolFun=1e-12, TolX=1e-14, MaxIter=6)
    r = ocs.single_shooting_batch(pg, x0, tspan, 7, **kw)
    J, v, it = r["J"].cpu().numpy(), r["v"].cpu().numpy(), r["iterations"].cpu().numpy()
    assert len(set(np.round(J, 9))) == batch   # the instances differ
    for b in range(batch):
        ps = ocs.LogisticProblem(ms[:, b], cs[b], P["r"], BOUNDS)
        rs = ocs.single_shooting_batch(ps, x0, tspan, 7, **kw)
        Js, vs, its = rs["J"].cpu().numpy(), rs["v"].cpu().numpy(), rs["iterations"].cpu().numpy()
        errs = (abs(J[b] - Js[b]) / max(1.0, abs(Js[b])), relerr(v[:, b], vs[:, b]))
        print(f"driver, instance {b}: J / v {errs}, iterations {it[b]} / {its[b]}")
        assert max(errs) < RTOL and it[b] == its[b] and it[b] > 0


# ---- 10. hipRTC plugins ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mapping", ["auto", "lane"])
def test_hand_written_logistic2_all_indices(ocs, oracle, mapping):
    """LOGISTIC2_SRC (full-vector methods, params [c, r, m1, m2]; no tabulated coefficient, so r may vary too) with ALL four
    parameters per trajectory, index list [3, 1, 0, 2]: both passes of every trajectory of (2, 64, 66) -- a whole tile of 64
    and a ragged tail on the vector mappings under "auto" -- against oracle.LogisticProblem of its values at the RTOL of
    test_hand_written_logistic2_equals_builtin_and_oracle (tests/test_gpu_user_problems.py); then fb_sweep through the
    plugin's ocs_ControlChar (costate pass as the scan with dense step maps, path 2 as
    test_fb_sweep_full_vector_plugin_on_the_vector_mappings asserts) with c, m1, m2 per instance, every instance against
    oracle.fb_sweep at that test's 1e-10."""
    nS, N, batch = 2, 64, 66
    tspan, x0, u = _inputs(oracle, nS, N, batch, seed=12, T=2.0)
    cs, ms = _draw_cm(13, nS, batch)
    rs = np.random.default_rng(14).uniform(0.03, 0.08, batch)
    lamT = np.random.default_rng(4).normal(size=(nS + 1, batch))
    pu = ocs.UserProblem(LOGISTIC2_SRC, 2, 1, [P["c"], P["r"], 3.0, 2.5], BOUNDS, has_control_char=True)
    pu.set_batch_params([3, 1, 0, 2], np.vstack([ms[1], rs, cs, ms[0]]))
    ref = _oracle_passes(oracle, lambda b: oracle.LogisticProblem(ms[:, b], cs[b], rs[b], BOUNDS), tspan, x0, u, lamT)
    _check_passes(ocs.RK4Integrator(tspan).set_mapping(mapping), pu, x0, u, lamT, ref, f"logistic2 {mapping}")
    if mapping != "auto":
        return
    tsw, x0s, csw, msw, opts, refs = _sweep_case(oracle, "ragged", 2, 64, 34)
    pu.set_batch_params([3, 0, 2], np.vstack([msw[1], csw, msw[0]]))
    g = ocs.RK4Integrator(tsw)
    r = ocs.fb_sweep_batch(pu, x0s, tsw, opts, integrator=g)
    assert ocs.fb_sweep_path(g) == 2
    for b, so in enumerate(refs):
        assert r["sweeps"][b] == so["_sweeps"] and abs(r["J"][b] - so["J"]) < RTOL_SWEEP * abs(so["J"]), b
        assert relerr(r["u"][:, :, b], so["u"]) < RTOL_SWEEP and relerr(r["x"][:, :, b], so["x"]) < RTOL_SWEEP, b
        assert relerr(r["lam"][:, :, b], so["lam"]) < RTOL_SWEEP, b


@pytest.mark.parametrize("mapping,batch", [("auto", 64), ("auto", 66), ("lane", 64), ("lane", 66)])
def test_coupled_plugin(ocs, oracle, mapping, batch):
    """PREDPREY_SRC (coupled, 8 parameters [al, be, de, ga, c, q, xb, r], its own discount factor) with al, de, c, xb and r
    (the last index) per trajectory (each within 10 % of PREDPREY_PARAMS), index list [7, 0, 4, 2, 6]: on "lane" and on "auto" -- the vector-lane state pass and
    the scan adjoint with dense step maps, a whole tile of 64 and its ragged tail at 66 -- every trajectory against the
    NumPy twin (PredPreyNP on RK4IntegratorNP) built from its values, default and explicit lamT, inputs and RTOL of
    test_vector_mappings_for_coupled_problems (tests/test_gpu_user_problems.py) at N = 64."""
    N = 64
    tspan = oracle.linspace(0, 6, N + 1)
    rng = np.random.default_rng(N + batch)
    uu = rng.uniform(0.0, 1.0, (1, 2 * N + 1, batch))
    x0 = rng.uniform(1.0, 2.5, (2, batch))
    lamT = rng.normal(size=(3, batch))
    index = [7, 0, 4, 2, 6]
    base = np.asarray(PREDPREY_PARAMS)
    values = base[index][:, None] * rng.uniform(0.9, 1.1, (len(index), batch))
    pu = ocs.UserProblem(PREDPREY_SRC, 2, 1, PREDPREY_PARAMS, BOUNDS)
    pu.set_batch_params(index, values)
    g = ocs.RK4Integrator(tspan).set_mapping(mapping)
    x, J = g.compute_states(pu, x0, uu)
    lam, dJdu = g.compute_adjoints(pu, uu)
    lam2, d2 = g.compute_adjoints(pu, uu, lamT)
    gn = tw.RK4IntegratorNP(tspan)
    worst = 0.0
    for b in range(batch):
        pb = base.copy()
        pb[index] = values[:, b]
        pn = PredPreyNP(pb)
        xn, Jn = gn.compute_states(pn, x0[:, b], uu[:, :, b])
        lamn, dn = gn.compute_adjoints(pn, uu[:, :, b])
        l2n, d2n = gn.compute_adjoints(pn, uu[:, :, b], lamT[:, b])
        errs = (relerr(x[:, :, b], xn), abs(J[b] - Jn) / max(1, abs(Jn)), relerr(lam[:, :, b], lamn),
                relerr(dJdu[:, :, b], dn), relerr(lam2[:, :, b], l2n), relerr(d2[:, :, b], d2n))
        worst = max(worst, *errs)
        assert max(errs) < RTOL, (b, errs)
    print("worst error", worst)


# ---- 11. LQProblem: entries of A and Bu -----------------------------------------------------------------------------
@pytest.mark.parametrize("mapping", [0, 1, 2, 3, 4])
def test_lq_entries_of_A_and_Bu_are_refused_not_ignored(ocs, oracle, mapping):
    """LQProblem(nS = 4, nC = 1) has 26 parameters, so set_batch_params accepts A(1,1), A(3,2) and Bu(2) per trajectory
    (indices 1, 1 + 2 + 4 * 1 = 7, 17 + 1 = 18 of [r | A | Bu | q | rdiag]).  No kernel of the LQ problem reads such a
    table (the Jacobian is the shared A operand of the matrix instruction), and include/ocs.h says what happens instead:
    every pass fails with OCS_ERR_UNSUPPORTED -- that refusal is what this case expects, on every mapping, for
    compute_states and (with a state pass of the shared problem in place) for compute_adjoints.  Computing with the shared
    A without saying so is the failure it exists to catch; cleared, the problem matches the oracle again at the RTOL of
    tests/test_gpu_lq.py."""
    nS, nC, N, batch = 4, 1, 33, 37
    A, Bu, q, rdiag = lq_matrices(nS, nC)
    bounds = [[-1.0, 1.0]]
    pg, po = ocs.LQProblem(A, Bu, q, rdiag, 0.05, bounds), oracle.LQProblem(A, Bu, q, rdiag, 0.05, bounds)
    rng = np.random.default_rng(N + mapping)
    tspan = np.concatenate([[0.0], np.sort(rng.uniform(0.0, 1.5, N - 1)), [1.5]])
    u = rng.uniform(-1, 1, (nC, 2 * N + 1, batch))
    x0 = rng.normal(size=(nS, batch))
    g = ocs.RK4Integrator(tspan)
    g.set_mapping(mapping)
    g.compute_states(pg, x0, u)
    values = np.vstack([A[2, 1] + 0.1 * rng.normal(size=batch), Bu[1, 0] + 0.1 * rng.normal(size=batch),
                        A[0, 0] * rng.uniform(0.8, 1.2, batch)])
    pg.set_batch_params([1 + 2 + nS * 1, 1 + nS * nS + 1, 1], values)
    with pytest.raises(ocs.OcsError) as e:
        g.compute_adjoints(pg, u)
    assert e.value.code == OCS_ERR_UNSUPPORTED
    with pytest.raises(ocs.OcsError) as e:
        g.compute_states(pg, x0, u)
    assert e.value.code == OCS_ERR_UNSUPPORTED
    pg.set_batch_params([], None)
    x, J = g.compute_states(pg, x0, u)
    lam, dJdu = g.compute_adjoints(pg, u)
    ref = oracle.batch_states_adjoints(po, tspan, x0, u)
    assert relerr(x, ref["x"]) < RTOL and relerr(J, ref["J"]) < RTOL
    assert relerr(lam, ref["lam"]) < RTOL and relerr(dJdu, ref["dJdu"]) < RTOL
