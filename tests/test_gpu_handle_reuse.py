"""Handle reuse: a result must not depend on what the handles did before.

Every OPERATION below is one call (or one pass pair) at a shape an existing GPU test already runs on its own -- the docstring
of each names the test.  It is evaluated FRESH (every handle created for that one evaluation; twice, bit-equal; once against
the CPU oracle at the borrowed tolerance) and SHARED: one bundle of handles -- one RK4Integrator on linspace(0, 2, 65), one
RK4InfiniteIntegrator per control count on that grid plus a 40-step tail (uStar has nC entries, so the logistic and the LQ
problems cannot share one), one handle per problem, one control handle per basis -- walks a whole sequence of operations, and
every result must be BIT-equal to the fresh one, in five orders.  An operation sets all the state it depends on itself
(mapping, per-trajectory parameters, fusion mode); everything else is a cache and must follow.

    cache (where)                              keyed on                             pair of operations that changes exactly that key
    -----------------------------------------  -----------------------------------  -------------------------------------------------
    TC / TU / REC, rec_stride (bind_problem)   (tc_prob, tc_version)                A -> B (problem); reborn.log4: a destroyed
                                                                                    problem's address taken by a new one (version)
    RECS (bind_problem)                        rebuilt for scan / vector problems   B -> F (LQ: left over), F -> J.rows, J.predprey
    checkpoints ck, ck_prob, ck_batch          set by every state pass              A -> C (batch), P.* -> S (fused: ck = nullptr)
    staging d_x0 / d_u / d_x / d_stage         grow-only                            A (70) -> C (33) -> A
    per-trajectory table pb, version           set_batch_params / clear             A -> D -> E (two bumps, E == A)
    LQ chunk workspace lqws                    (ps, version, REC, C, N, nS)         F -> G19 -> G40 (C), G19 -> H (ps), I.* (version)
    LQ per-trajectory weights W                set_batch_weights / clear            F -> I.w0 / I.w4 -> I.clear0 / I.clear4 (== F, G19)
    constant-control response zc               zc_valid, zc_key_u                   U.19.0 -> U.19.4 -> U.40.4 -> U.40.0
    tail leg: d_utail, utail_batch, tail_wave  batch; wave or lane per call         T64 -> T96 (grows) -> T70 (lane) -> T96
    pchip tables (ocs_fbs_state)               built once per grid                  every sweep operation after the first
    point tables KE.. / KI.., err_on_nodes,    (nerr, nint)                         L.65.21 -> L.101.21 (nerr, QSE) -> L.65.33 (nint)
      QSE
    TUE / TUI                                  (new points, tu_prob, tu_version)    L.65.21 -> M (tu_prob), -> N.*, O.*
    lq_TC / lq_REC                             (lq_prob, lq_version, lq_N)          K -> L.* (lq_prob), L -> M, reborn.lq16 (version)
    LQ plugin twin (shadow)                    built once per problem handle        K, L.*, M on their second visit
    h_nact, nact_slots, wevents                nSWEEPS, depth                       N.*.3 -> N.*.40 -> N.*.3
    control d_u / d_dJdu / d_idx, fuse_mode    batch, nFree; set_fusion             P.on -> P.lane -> P.off, Q.on -> Q.off, R.off -> R.on

Calls on different streams racing over a table rebuild are not tested here (no deterministic test exists for them)."""
import numpy as np
import pytest

from oracle import np_twin as tw
from tests.user_problems import (LOGISTIC2_SRC, LOGISTIC_ROWS_CC_SRC, LOGISTIC_ROWS_SRC, PREDPREY_PARAMS, PREDPREY_SRC,
                                 PredPreyNP, lq_matrices)

pytestmark = pytest.mark.gpu
N, N2 = 64, 40        # N % 8 == 0: scan, wave-specialised, fold and RECS paths engage; two chunks of the time-parallel LQ mapping
RTOL = 1e-12          # passes and objectives: tests/test_gpu_rk4_parity.py, test_gpu_lq.py, test_gpu_controls_shooting.py
RTOL_SWEEP = 1e-10    # sweep results: tests/test_gpu_fb_sweep.py, test_gpu_lq_sweep.py
OCS_ERR_ORDER = -3    # include/ocs.h
C_, R_ = 1.5, 0.05
M4 = [3.0, 2.5, 2.0, 1.5]
BOUNDS, LQ_BOUNDS = [[0.0, 1.0]], [[-1.0, 1.0]] * 4
USTAR1, USTAR4 = [0.4], [0.1, -0.2, 0.0, 0.3]
SHUFFLE_SEEDS = (20261018, 7)
TSPAN = np.arange(N + 1) / 32.0               # linspace(0, 2, 65), exactly
TX = 2.0 + np.arange(N2 + 1) / 20.0           # the tail: 40 steps on [2, 4]
_FRESH, _IN, REBORN = {}, {}, {}


def relerr(a, b):
    """max |a-b| / max(1,|b|) (tests/test_gpu_rk4_parity.py); non-finite reference entries must match exactly"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    bad = ~np.isfinite(b)
    if bad.any():
        if not ((np.isnan(a[bad]) & np.isnan(b[bad])) | (a[bad] == b[bad])).all():
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


# ---- handles --------------------------------------------------------------------------------------------------------
def _lq(scale_A=1.0, scale_q=1.0, scale_r=1.0, r=R_):
    A, Bu, q, rdiag = lq_matrices(16, 4)
    return A * scale_A, Bu, q * scale_q, rdiag * scale_r, r, LQ_BOUNDS


PROBLEMS = {
    "log4": lambda o: o.LogisticProblem(M4, C_, R_, BOUNDS),
    "log2": lambda o: o.LogisticProblem(M4[:2], C_, R_, BOUNDS),
    "log1": lambda o: o.LogisticProblem(M4[:1], C_, R_, BOUNDS),
    "lq16": lambda o: o.LQProblem(*_lq()),
    "lq16b": lambda o: o.LQProblem(*_lq(scale_A=0.9)),
    "lq16s": lambda o: o.LQProblem(*_lq(scale_r=8.0)),                     # test_gpu_lq_sweep.make: rdiag * 8
    "lq16s2": lambda o: o.LQProblem(*_lq(scale_q=1.3, scale_r=6.0)),
}
PLUGINS = {
    "rows2": lambda ocs: ocs.UserProblem(LOGISTIC_ROWS_SRC, 2, 1, [C_, R_] + M4[:2], BOUNDS, row_separable=True),
    "predprey": lambda ocs: ocs.UserProblem(PREDPREY_SRC, 2, 1, PREDPREY_PARAMS, BOUNDS),
    "rows2cc": lambda ocs: ocs.UserProblem(LOGISTIC_ROWS_CC_SRC, 2, 1, [C_, R_] + M4[:2], BOUNDS, has_control_char=True,
                                           row_separable=True, control_from_costate=True),
    "log2cc": lambda ocs: ocs.UserProblem(LOGISTIC2_SRC, 2, 1, [C_, R_] + M4[:2], BOUNDS, has_control_char=True),
}


class Bundle:
    """The handles an operation asks for, created on first use and kept: a new bundle per evaluation is the FRESH way, one
    bundle for a whole sequence the SHARED way."""

    def __init__(self, ocs, fresh):
        self.ocs, self.fresh, self._h = ocs, fresh, {}

    def _get(self, key, make):
        if key not in self._h:
            self._h[key] = make()
        return self._h[key]

    def g(self):
        return self._get("g", lambda: self.ocs.RK4Integrator(TSPAN))

    def gi(self, nC):
        return self._get(("gi", nC), lambda: self.ocs.RK4InfiniteIntegrator(TSPAN, TX, USTAR1 if nC == 1 else USTAR4))

    def prob(self, name):
        return self._get(name, lambda: (PROBLEMS[name] if name in PROBLEMS else PLUGINS[name])(self.ocs))

    def ctrl(self, kind, nB):
        return self._get((kind, nB), lambda: getattr(self.ocs, kind)(self.g().t, nB, 1))

    def reborn(self, tag, make_old, make_new, use):
        """A problem created right after another was destroyed, so that the allocator hands out the old handle's address
        again (tables are keyed on (pointer, version): only the version tells the two apart).  SHARED: `use` runs the old
        problem on the bundle's integrator first.  FRESH: the new problem alone.  New handles are created (and kept, so that
        each gets another block) until one has the old address: glibc hands it out on the first try after plain passes and
        within some 30 tries after a sweep, whose teardown frees other blocks of that size first.  REBORN[tag] records
        whether it came back; where it does not, the operation is still a valid change of problem."""
        if self.fresh:
            return make_new()
        drain = [make_new() for _ in range(8)]   # empties the allocator's per-thread list of free blocks of this size (it
        old = make_old()                          # holds 7), so that the block freed below is the next one handed out
        use(old)
        addr = old._h.value
        del old                      # -> ocs_problem_destroy
        spare = []
        for _ in range(64):
            new = make_new()
            if new._h.value == addr:
                break
            spare.append(new)        # (kept alive so that the next try gets another address)
        REBORN[tag] = new._h.value == addr
        print(f"reborn.{tag}: the destroyed handle's address {'came back' if REBORN[tag] else 'did NOT come back'} "
              f"(try {len(spare) + 1})")
        del drain
        return new


# ---- inputs (drawn once, never written again) -----------------------------------------------------------------------
def _inputs(key, make):
    if key not in _IN:
        _IN[key] = make()
    return _IN[key]


def _logistic_inputs(nS, batch):
    """x0 ~ U(0.8, 2), u ~ U(0.05, 0.45): test_infinite_integrator_tail_leg_mappings (tests/test_gpu_controls_shooting.py)"""
    def make():
        rng = np.random.default_rng(1000 * nS + batch)
        return rng.uniform(0.8, 2.0, (nS, batch)), rng.uniform(0.05, 0.45, (1, 2 * N + 1, batch))
    return _inputs(("log", nS, batch), make)


def _lq_inputs(batch):
    """x0 ~ N(0, 1), u ~ U(-1, 1): test_states_adjoints_vs_oracle (tests/test_gpu_lq.py)"""
    def make():
        rng = np.random.default_rng(16000 + batch)
        return rng.normal(size=(16, batch)), rng.uniform(-1, 1, (4, 2 * N + 1, batch))
    return _inputs(("lq", batch), make)


def _lq_weights(batch):
    """q, rdiag within +-30 % of the shared values per trajectory (tests/test_gpu_lq_batch_weights.py)"""
    def make():
        _, _, q, rdiag = lq_matrices(16, 4)
        rng = np.random.default_rng(77 + batch)
        return q[:, None] * rng.uniform(0.7, 1.3, (16, batch)), rdiag[:, None] * rng.uniform(0.7, 1.3, (4, batch))
    return _inputs(("lqw", batch), make)


def _cs(batch):
    return _inputs(("c", batch), lambda: np.random.default_rng(5 + batch).uniform(1.0, 2.0, batch))


def _sweep_x0(nS, batch):
    return _inputs(("sx0", nS, batch), lambda: np.random.default_rng(31 * nS + batch).uniform(0.8, 1.6, (nS, batch)))


def _lq_sweep_x0(batch):
    """x0 = s * linspace(0.5, 1.5, nS), s in (1, 4, 10): x0_of of tests/test_gpu_lq_sweep.py (s = 10 puts the control on a bound)"""
    return np.stack([(1.0, 4.0, 10.0)[b % 3] * np.linspace(0.5, 1.5, 16) for b in range(batch)], axis=1)


def _cheb_V(nB, batch, nFree):
    """SURVEY BL-4 candidates of test_fused_control_objective_gradient (tests/test_gpu_controls_shooting.py)"""
    def make():
        rng = np.random.default_rng(nB * 100 + batch + nFree)
        V = 0.05 * rng.normal(size=(nB, batch)) / np.arange(1, nB + 1)[:, None]
        V[0] += 0.4
        return np.vstack([V, rng.uniform(0.8, 1.6, (nFree, batch))]), rng.uniform(0.8, 1.5, (4, batch))
    return _inputs(("chebV", nB, batch, nFree), make)


def _pwl_V(nB, batch):
    def make():
        rng = np.random.default_rng(nB * 10 + batch)
        return rng.uniform(0.05, 0.45, (nB, batch)), rng.uniform(0.8, 1.5, (4, batch))
    return _inputs(("pwlV", nB, batch), make)


# ---- the calls ------------------------------------------------------------------------------------------------------
def _passes(g, p, x0, u):
    x, J = g.compute_states(p, x0, u)
    lam, dJdu = g.compute_adjoints(p, u)
    return {"x": x, "J": J, "lam": lam, "dJdu": dJdu}


def _sweep(ocs, g, p, x0, opts):
    r = ocs.fb_sweep_batch(p, x0, TSPAN, opts, integrator=g)
    out = {k: r[k] for k in ("x", "lam", "u", "J", "sweeps", "maxChange")}
    out["path"] = np.array([ocs.fb_sweep_path(g), ocs.fb_sweep_matrix_core(g)])
    return out


def _samples(batch):
    return sorted({0, batch // 2, batch - 1})


def _ref_passes(go, make_po, x0, u, res):
    """up to 3 sampled trajectories against the oracle (or the NumPy twin) at RTOL"""
    for b in _samples(x0.shape[1]):
        po = make_po(b)
        xo, Jo = go.compute_states(po, x0[:, b], u[:, :, b])
        lamo, do = go.compute_adjoints(po, u[:, :, b])
        errs = {"x": relerr(res["x"][:, :, b], xo), "J": abs(res["J"][b] - Jo) / max(1.0, abs(Jo)),
                "lam": relerr(res["lam"][:, :, b], lamo), "dJdu": relerr(res["dJdu"][:, :, b], do)}
        assert max(errs.values()) < RTOL, (b, errs)


def _ref_sweep(oracle, po, x0, opts, res):
    """sweep count, NaN pattern and recorded change (1e-6, tests/test_gpu_batch_params.py::test_fb_sweep) of up to 3 sampled
    instances; x, lam, u, J at RTOL_SWEEP where the oracle converged (elsewhere the reference returns an empty struct)"""
    for b in _samples(x0.shape[1]):
        ref = oracle.fb_sweep(po, x0[:, b], TSPAN, opts)
        k = ref["_sweeps"]
        assert res["sweeps"][b] == k, (b, int(res["sweeps"][b]), k)
        n = k if k > 0 else res["maxChange"].shape[0]
        mc = res["maxChange"][:, b]
        assert np.all(np.isnan(mc[n:])) and not np.any(np.isnan(mc[:n])), b
        assert relerr(mc[:n], ref["_maxChange"][:n]) < 1e-6, b
        if k > 0:
            errs = {"J": abs(res["J"][b] - ref["J"]) / abs(ref["J"]), "x": relerr(res["x"][:, :, b], ref["x"]),
                    "lam": relerr(res["lam"][:, :, b], ref["lam"]), "u": relerr(res["u"][:, :, b], ref["u"])}
            assert max(errs.values()) < RTOL_SWEEP, (b, errs)


OPS = {}    # name -> (run(bundle) -> dict of arrays, check(oracle, result) or None)


def op(name, check=None):
    def deco(run):
        OPS[name] = (run, check)
        return run
    return deco


# ---- integrator passes ----------------------------------------------------------------------------------------------
def _logistic_passes(name, pname, nS, batch, per_traj=False, clear_after_set=False):
    """A, B, C, D, E: registry logistic passes -- the nS = 4 and nS = 1 shapes of test_both_mappings_match_oracle
    (tests/test_gpu_rk4_parity.py) at N = 64; c per trajectory as test_integrator_passes_every_mapping
    (tests/test_gpu_batch_params.py), cleared as test_refusal_clear_and_mismatch"""
    x0, u = _logistic_inputs(nS, batch)
    cs = _cs(batch)

    def run(h):
        p, g = h.prob(pname), h.g().set_mapping("auto")
        if per_traj or clear_after_set:
            p.set_batch_params([0], cs[None, :])
        if not per_traj:
            p.set_batch_params([], None)
        return _passes(g, p, x0, u)

    def check(oracle, res):
        _ref_passes(oracle.RK4Integrator(TSPAN), lambda b: oracle.LogisticProblem(M4[:nS], cs[b] if per_traj else C_, R_, BOUNDS),
                    x0, u, res)
    OPS[name] = (run, check)


_logistic_passes("A", "log4", 4, 70)
_logistic_passes("B", "log1", 1, 64)
_logistic_passes("C", "log4", 4, 33)
_logistic_passes("D", "log4", 4, 70, per_traj=True)
_logistic_passes("E", "log4", 4, 70, clear_after_set=True)


def _lq_passes(name, pname, batch, mapping, weights=None, inf=False):
    """F, G, H, I, U: LQProblem(16, 4) passes -- (16, 4, 64, 16) and (17, 2, 20, 19) of test_states_adjoints_vs_oracle and the
    RK4InfiniteIntegrator of test_infinite_horizon_and_shooting_objective (tests/test_gpu_lq.py, mappings 0 and 4: time-parallel
    chunks); weights per trajectory as test_gpu_lq_batch_weights.py.  weights: None (never set), "set", "cleared"."""
    x0, u = _lq_inputs(batch)
    qb, rb = _lq_weights(batch)

    def run(h):
        p = h.prob(pname)
        g = (h.gi(4) if inf else h.g()).set_mapping(mapping)
        if weights:
            p.set_batch_weights(q=qb, rdiag=rb)
        if weights != "set":
            p.set_batch_weights()
        return _passes(g, p, x0, u)

    def check(oracle, res):
        A, Bu, q, rdiag, r, bounds = _lq(scale_A=0.9 if pname == "lq16b" else 1.0)
        make = ((lambda b: oracle.LQProblem(A, Bu, qb[:, b], rb[:, b], r, bounds)) if weights == "set"
                else (lambda b: oracle.LQProblem(A, Bu, q, rdiag, r, bounds)))
        go = oracle.RK4InfiniteIntegrator(TSPAN, TX, USTAR4) if inf else oracle.RK4Integrator(TSPAN)
        _ref_passes(go, make, x0, u, res)
    OPS[name] = (run, check)


_lq_passes("F", "lq16", 19, 0)
_lq_passes("G19", "lq16", 19, 4)
_lq_passes("G40", "lq16", 40, 4)
_lq_passes("F40", "lq16", 40, 0)
_lq_passes("H", "lq16b", 19, 4)
_lq_passes("I.w0", "lq16", 19, 0, weights="set")
_lq_passes("I.w4", "lq16", 19, 4, weights="set")
_lq_passes("I.clear0", "lq16", 19, 0, weights="cleared")
_lq_passes("I.clear4", "lq16", 19, 4, weights="cleared")
for _b in (19, 40):
    for _m in (0, 4):
        _lq_passes(f"U.{_b}.{_m}", "lq16", _b, _m, inf=True)


def _plugin_passes(name, pname, batch):
    """J: row functions (nS = 2, test_row_separable_user_problem_on_the_fast_mappings) and the coupled full-vector plugin
    (test_vector_mappings_for_coupled_problems (64, 64)) of tests/test_gpu_user_problems.py: both rebuild RECS for a User functor"""
    def make():
        rng = np.random.default_rng(len(pname) + batch)
        if pname == "predprey":
            return rng.uniform(1.0, 2.5, (2, batch)), rng.uniform(0.0, 1.0, (1, 2 * N + 1, batch))
        return rng.uniform(0.9, 2.0, (2, batch)), rng.uniform(0.05, 0.45, (1, 2 * N + 1, batch))
    x0, u = _inputs(("plugin", pname, batch), make)

    def run(h):
        return _passes(h.g().set_mapping("auto"), h.prob(pname), x0, u)

    def check(oracle, res):
        if pname == "predprey":
            _ref_passes(tw.RK4IntegratorNP(TSPAN), lambda b: PredPreyNP(), x0, u, res)
        else:
            _ref_passes(oracle.RK4Integrator(TSPAN), lambda b: oracle.LogisticProblem(M4[:2], C_, R_, BOUNDS), x0, u, res)
    OPS[name] = (run, check)


_plugin_passes("J.rows", "rows2", 70)
_plugin_passes("J.predprey", "predprey", 64)


def _tail(name, batch):
    """T: RK4InfiniteIntegrator, logistic nS = 2 -- (2, 64, 64, 96) and (2, 64, 64, 70) of
    test_infinite_integrator_tail_leg_mappings (tests/test_gpu_controls_shooting.py) with a 40-step tail: whole tiles of 32 run
    the tail on the wave-specialised kernels from the sampled constant control kept with the handle, batch 70 on the lane kernels"""
    x0, u = _logistic_inputs(2, batch)

    def run(h):
        p = h.prob("log2")
        p.set_batch_params([], None)
        return _passes(h.gi(1).set_mapping("auto"), p, x0, u)

    def check(oracle, res):
        _ref_passes(oracle.RK4InfiniteIntegrator(TSPAN, TX, USTAR1), lambda b: oracle.LogisticProblem(M4[:2], C_, R_, BOUNDS),
                    x0, u, res)
    OPS[name] = (run, check)


for _b in (64, 96, 70):
    _tail(f"T{_b}", _b)


# ---- sweep entry points ---------------------------------------------------------------------------------------------
def _k_check(oracle, res):
    x0, u = _lq_inputs(19)
    go, po = oracle.RK4Integrator(TSPAN), oracle.LQProblem(*_lq())
    for b in _samples(19):
        xo, lo, Jo = oracle.compute_x_lam(go, po, x0[:, b], u[:, :, b], want_J=True)
        errs = (relerr(res["x"][:, :, b], xo), relerr(res["lam"][:, :, b], lo), abs(res["J"][b] - Jo) / max(1.0, abs(Jo)))
        assert max(errs) < RTOL, (b, errs)


@op("K", _k_check)
def _k(h):
    """compute_x_lam_J on the problem handle of F: test_compute_x_lam_J (tests/test_gpu_lq_sweep.py) at 16 states"""
    x0, u = _lq_inputs(19)
    p, g = h.prob("lq16"), h.g()
    p.set_batch_weights()
    x, lam, J = h.ocs.compute_x_lam_J(p, x0, TSPAN, u, integrator=g)
    return {"x": x, "lam": lam, "J": J, "path": np.array([h.ocs.fb_sweep_matrix_core(g)])}


def _lq_sweep(name, pname, nerr, nint, oracle_args):
    """L, M: fb_sweep_batch on LQProblem(16, 4) with rdiag * 8 (test_sweep_vs_oracle, test_matrix_core_path_ran of
    tests/test_gpu_lq_sweep.py), batch 5: error points on the nodes (path 2), off them (path 5, QSE), other interpolation points"""
    x0 = _lq_sweep_x0(5)
    opts = {"nERROR_PTS": nerr, "nINTERP_PTS": nint, "nSWEEPS": 200}

    def run(h):
        p = h.prob(pname)
        p.set_batch_weights()
        return _sweep(h.ocs, h.g(), p, x0, opts)

    def check(oracle, res):
        assert res["path"][1] == 1 and res["path"][0] == (2 if nerr == N + 1 else 5)
        _ref_sweep(oracle, oracle.LQProblem(*_lq(**oracle_args)), x0, opts, res)
    OPS[name] = (run, check)


_lq_sweep("L.65.21", "lq16s", 65, 21, dict(scale_r=8.0))
_lq_sweep("L.101.21", "lq16s", 101, 21, dict(scale_r=8.0))
_lq_sweep("L.65.33", "lq16s", 65, 33, dict(scale_r=8.0))
_lq_sweep("M", "lq16s2", 65, 21, dict(scale_q=1.3, scale_r=6.0))


def _logistic_sweep(name, pname, nS, batch, nsweeps):
    """N: registry logistic sweeps -- (1, 64, 64) of test_fold_on_a_bitwise_uniform_grid and (4, 54) of
    test_two_kernel_sweep_on_ragged_batches (tests/test_gpu_fb_sweep.py); nSWEEPS = 3 and 40 as
    test_sweeps_enqueued_ahead_equal_the_plain_loop: the ring of sweeps in flight and its counters change size"""
    x0 = _sweep_x0(nS, batch)
    opts = {"nERROR_PTS": N + 1, "nINTERP_PTS": 17, "nSWEEPS": nsweeps}

    def run(h):
        p = h.prob(pname)
        p.set_batch_params([], None)
        return _sweep(h.ocs, h.g(), p, x0, opts)

    def check(oracle, res):
        assert res["path"][1] == 0
        _ref_sweep(oracle, oracle.LogisticProblem(M4[:nS], C_, R_, BOUNDS), x0, opts, res)
    OPS[name] = (run, check)


for _k_ in (3, 40):
    _logistic_sweep(f"N.1.{_k_}", "log1", 1, 64, _k_)
    _logistic_sweep(f"N.4.{_k_}", "log4", 4, 54, _k_)


def _plugin_sweep(name, pname):
    """O: the costate-only row plugin (test_fb_sweep_two_kernel_sweep_for_user_row_functions) and the full-vector plugin
    (test_fb_sweep_full_vector_plugin_on_the_vector_mappings) of tests/test_gpu_user_problems.py, batch 64"""
    x0 = _sweep_x0(2, 64)
    opts = {"nERROR_PTS": N + 1, "nINTERP_PTS": 81}

    def run(h):
        return _sweep(h.ocs, h.g(), h.prob(pname), x0, opts)

    def check(oracle, res):
        assert res["path"][0] == (4 if pname == "rows2cc" else 2) and res["path"][1] == 0
        _ref_sweep(oracle, oracle.LogisticProblem(M4[:2], C_, R_, BOUNDS), x0, dict(opts, nSWEEPS=50), res)
    OPS[name] = (run, check)


_plugin_sweep("O.rows", "rows2cc")
_plugin_sweep("O.vector", "log2cc")


# ---- shooting objective ---------------------------------------------------------------------------------------------
def _objective(name, kind, nB, pname, nS, mode, free=()):
    """P, Q, R: nlp_objective at batch 64 -- Chebyshev-16 on nS = 1 (wave kernels under "on": test_fused_control_wave_kernels)
    and nS = 4 (test_fused_control_objective_gradient (4, 32, 64, 64)), PWLinear-11 (test_fused_banded_control_objective_gradient),
    a free initial state (d_idx / lam0; want_lam0 on the unfused path), tests/test_gpu_controls_shooting.py"""
    batch = 64
    V, x0 = _cheb_V(nB, batch, len(free)) if kind == "ChebyshevControl" else _pwl_V(nB, batch)
    x0 = x0[:nS]

    def run(h):
        p, g, c = h.prob(pname), h.g().set_mapping("auto"), h.ctrl(kind, nB)
        p.set_batch_params([], None)
        c.set_fusion(mode)
        J, dJdv, x0n = h.ocs.nlp_objective(g, p, c, x0.copy(), V, FreeInitStates=list(free))
        return {"J": J, "dJdv": dJdv, "x0": x0n}

    def check(oracle, res):
        go, po = oracle.RK4Integrator(TSPAN), oracle.LogisticProblem(M4[:nS], C_, R_, BOUNDS)
        co = getattr(oracle, kind)(go.t, nB, 1)
        for b in _samples(batch):
            Jo, do, x0o = oracle.nlp_objective(go, po, co, x0[:, b], V[:, b], FreeInitStates=list(free))
            errs = (abs(res["J"][b] - Jo) / max(1.0, abs(Jo)), relerr(res["dJdv"][:, b], do))
            assert max(errs) < RTOL and np.array_equal(res["x0"][:, b], x0o), (b, errs)
    OPS[name] = (run, check)


for _mode in ("on", "lane", "off"):
    _objective(f"P.1.{_mode}", "ChebyshevControl", 16, "log1", 1, _mode)
    _objective(f"P.4.{_mode}", "ChebyshevControl", 16, "log4", 4, _mode)
for _mode in ("on", "off"):
    _objective(f"Q.{_mode}", "PWLinearControl", 11, "log2", 2, _mode)
    _objective(f"R.{_mode}", "ChebyshevControl", 16, "log2", 2, _mode, free=(1,))


@op("S", lambda oracle, res: None)     # (its numbers are A's: test_operations_that_must_agree)
def _s(h):
    """The ordering contract (test_ordering_contract of tests/test_gpu_rk4_parity.py) across a FUSED objective: its checkpoints
    belong to no u in memory, so compute_adjoints on that integrator must fail with OCS_ERR_ORDER, not return numbers -- also
    for the problem and batch of the state pass that ran before it; after a plain compute_states it works again (== A)"""
    x0, u = _logistic_inputs(4, 64)
    xa, ua = _logistic_inputs(4, 70)
    V, _ = _cheb_V(16, 64, 0)
    p, g, c = h.prob("log4"), h.g().set_mapping("auto"), h.ctrl("ChebyshevControl", 16)
    p.set_batch_params([], None)
    g.compute_states(p, x0, u)
    c.set_fusion("on")
    h.ocs.nlp_objective(g, p, c, x0.copy(), V)
    try:
        g.compute_adjoints(p, u)
        code = 0
    except h.ocs.OcsError as e:
        code = e.code
    return dict(_passes(g, p, xa, ua), code=np.array([code]))


# ---- a destroyed problem's address taken by a new problem ------------------------------------------------------------
def _reborn_check_log4(oracle, res):
    x0, u = _logistic_inputs(4, 70)
    _ref_passes(oracle.RK4Integrator(TSPAN), lambda b: oracle.LogisticProblem([2.8, 2.6, 2.2, 1.7], 1.2, 0.11, BOUNDS), x0, u, res)


@op("reborn.log4", _reborn_check_log4)
def _reborn_log4(h):
    """A (nS = 4, batch 70) on a problem with another discount rate whose handle has the address of one just destroyed"""
    x0, u = _logistic_inputs(4, 70)
    g = h.g().set_mapping("auto")
    p = h.reborn("log4", lambda: h.ocs.LogisticProblem(M4, C_, R_, BOUNDS),
                 lambda: h.ocs.LogisticProblem([2.8, 2.6, 2.2, 1.7], 1.2, 0.11, BOUNDS), lambda old: _passes(g, old, x0, u))
    return _passes(g, p, x0, u)


_REBORN_OPTS = {"nERROR_PTS": N + 1, "nINTERP_PTS": 21, "nSWEEPS": 200}


def _reborn_check_lq16(oracle, res):
    assert res["path"][0] == 2 and res["path"][1] == 1
    _ref_sweep(oracle, oracle.LQProblem(*_lq(scale_r=8.0, r=0.12)), _lq_sweep_x0(5), _REBORN_OPTS, res)


@op("reborn.lq16", _reborn_check_lq16)
def _reborn_lq16(h):
    """L.65.21 on an LQ problem with another discount rate whose handle (and whose plugin twin's) has the address of one just
    destroyed: lq_TC / lq_REC are keyed on (lq_prob, lq_version)"""
    x0, g = _lq_sweep_x0(5), h.g()
    p = h.reborn("lq16", lambda: h.ocs.LQProblem(*_lq(scale_r=8.0)), lambda: h.ocs.LQProblem(*_lq(scale_r=8.0, r=0.12)),
                 lambda old: _sweep(h.ocs, g, old, x0, _REBORN_OPTS))
    return _sweep(h.ocs, g, p, x0, _REBORN_OPTS)


# ---- the comparison -------------------------------------------------------------------------------------------------
LISTED = ["A", "B", "C", "A", "D", "E", "F", "G19", "G40", "F40", "F", "H", "I.w0", "I.w4", "I.clear0", "I.clear4", "J.rows",
          "J.predprey", "K", "L.65.21", "L.101.21", "L.65.33", "M", "N.1.3", "N.4.3", "N.1.40", "N.4.40", "N.1.3", "O.rows",
          "O.vector", "P.1.on", "P.1.lane", "P.1.off", "P.4.on", "P.4.lane", "P.4.off", "Q.on", "Q.off", "R.off", "R.on", "S",
          "T64", "T96", "T70", "T96", "U.19.0", "U.19.4", "U.40.4", "U.40.0", "reborn.log4", "reborn.lq16"]
assert set(LISTED) == set(OPS)


def _shuffled(seed):
    return [LISTED[i] for i in np.random.default_rng(seed).permutation(len(LISTED))]


ORDERS = {"listed": LISTED, "reverse": LISTED[::-1], **{f"shuffle{s}": _shuffled(s) for s in SHUFFLE_SEEDS},
          "twice": [name for name in LISTED for _ in range(2)]}


def _first_difference(a, b):
    """name of the first array of result `a` that is not bit-equal to its counterpart in `b` (NaN == NaN in maxChange), or None"""
    assert list(a) == list(b)
    for k in a:
        if not np.array_equal(a[k], b[k], equal_nan=(k == "maxChange")):
            return k
    return None


def _fresh(ocs, name):
    """the FRESH result of an operation: every handle created for this one evaluation; computed once per module"""
    if name not in _FRESH:
        _FRESH[name] = OPS[name][0](Bundle(ocs, fresh=True))
    return _FRESH[name]


@pytest.mark.parametrize("name", sorted(OPS))
def test_fresh_result_is_deterministic_and_matches_the_oracle(ocs, oracle, name):
    """Two fresh evaluations are bit-equal (the kernels combine across lanes with integer atomicAdd / atomicMax on bit patterns
    only) -- the determinism the shared comparison rests on -- and the fresh result is within the borrowed tolerance of the CPU
    oracle (the NumPy twin for the coupled plugin) on up to 3 sampled trajectories, sweep counts equal to the oracle's."""
    first = _fresh(ocs, name)
    again = OPS[name][0](Bundle(ocs, fresh=True))
    diff = _first_difference(first, again)
    assert diff is None, f"operation {name}: two fresh evaluations differ in {diff}"
    OPS[name][1](oracle, first)


def test_operations_that_must_agree(ocs):
    """Clearing per-trajectory parameters / weights restores the shared-parameter results bit for bit (E == A, I.clear0 == F,
    I.clear4 == G19); S fails with OCS_ERR_ORDER after the fused objective and then reproduces A; F40 / G40 and a tail at
    batch 96 differ from their smaller neighbours (the operations are not trivially the same call)."""
    for a, b in (("E", "A"), ("I.clear0", "F"), ("I.clear4", "G19")):
        assert _first_difference(_fresh(ocs, a), _fresh(ocs, b)) is None, (a, b)
    s = _fresh(ocs, "S")
    assert s["code"][0] == OCS_ERR_ORDER
    assert _first_difference({k: s[k] for k in ("x", "J", "lam", "dJdu")}, _fresh(ocs, "A")) is None
    assert not np.array_equal(_fresh(ocs, "D")["J"], _fresh(ocs, "A")["J"])
    assert not np.array_equal(_fresh(ocs, "I.w0")["J"], _fresh(ocs, "F")["J"])
    assert not np.array_equal(_fresh(ocs, "H")["J"], _fresh(ocs, "G19")["J"])


@pytest.mark.parametrize("order", list(ORDERS))
def test_shared_handles_reproduce_the_fresh_results(ocs, order):
    """One bundle of handles for the whole sequence: every result bit-equal to the fresh one, whatever ran before."""
    for name in LISTED:
        _fresh(ocs, name)
    h = Bundle(ocs, fresh=False)
    before = "nothing"
    for name in ORDERS[order]:
        diff = _first_difference(_fresh(ocs, name), OPS[name][0](h))
        assert diff is None, f"operation {name} after {before}: {diff} differs from the fresh result (order {order})"
        before = name
    print("a destroyed problem's address was reused:", REBORN)
