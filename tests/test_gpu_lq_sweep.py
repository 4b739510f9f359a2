"""fb_sweep / compute_x_lam(_J) on OCS_PROBLEM_LQ with the state pass and the costate pass on the matrix-core kernels
(csrc/ocs_lq_kernels.hip's one-wave state pass, csrc/ocs_lq_sweep_kernels.hip; from eight states on) against the CPU oracle and against the same solve on the problem's
plugin form (lane kernels), in the same process.

Inputs: the undamped sweep diverges on lq_matrices(nS, nC) as given once nS >= 8, so the cases weigh the control cost
with rdiag * 8 (the oracle then converges, the decision never near 1) or damp the update (uRelax = 0.25, plain rdiag).
x0 = s * linspace(0.5, 1.5, nS), tspan = linspace(0, 2, N + 1), bounds +-1, r = 0.05; s = 4 and s = 10 put the control on
its bounds.  Sweep counts are the oracle's, never hard-coded.  Tolerances: 1e-10 relative for sweep results (the form and
the value of tests/test_gpu_lq.py::test_fb_sweep_on_the_lq_problem), 1e-12 for a single compute_x_lam_J."""
import numpy as np
import pytest

from tests.user_problems import lq_matrices, lq_source

pytestmark = pytest.mark.gpu
OCS_ERR_UNSUPPORTED = -6


def relerr(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.max(np.abs(a - b) / np.maximum(1.0, np.abs(b))))


@pytest.fixture(scope="module")
def ocs():
    import torch
    assert torch.cuda.is_available()
    import __graft_entry__ as g
    return g.load_package()


BOUNDS = lambda nC: [[-1.0, 1.0]] * nC   # noqa: E731


def data(nS, nC, rscale):
    A, Bu, q, rdiag = lq_matrices(nS, nC)
    return A, Bu, q, rdiag * rscale


def make(ocs, oracle, nS, nC, rscale=8.0):
    A, Bu, q, rdiag = data(nS, nC, rscale)
    return (ocs.LQProblem(A, Bu, q, rdiag, 0.05, BOUNDS(nC)), oracle.LQProblem(A, Bu, q, rdiag, 0.05, BOUNDS(nC)))


def lq_control_char(nS, nC):
    """The Gen-1 ControlChar of the LQ problem, u = clamp(-Bu' lam e^{rt} / (2 R), bounds), as plugin source."""
    oB, oR = 1 + nS * nS, 1 + nS * nS + nS * nC + nS
    return f"""
__device__ void ocs_ControlChar(double t, const double* x, const double* lam, OCS_PARAMS p, const double* lb,
                                const double* ub, double* u) {{
  const double e = exp(p[0] * t);
  for (int l = 0; l < {nC}; ++l) {{
    double a = 0.0;
    for (int i = 0; i < {nS}; ++i) a += p[{oB} + i + {nS} * l] * lam[i];
    u[l] = fmin(ub[l], fmax(lb[l], -a * e / (2 * p[{oR} + l])));
  }}
}}
"""


def make_user(ocs, nS, nC, rscale=8.0):
    A, Bu, q, rdiag = data(nS, nC, rscale)
    par = np.concatenate([[0.05], A.ravel(order="F"), Bu.ravel(order="F"), q, rdiag])
    return ocs.UserProblem(lq_source(nS, nC) + lq_control_char(nS, nC), nS, nC, par, BOUNDS(nC), has_control_char=True)


def x0_of(nS, s):
    return s * np.linspace(0.5, 1.5, nS)


def nan_pattern_ok(mc, sweeps):
    """maxChange [nSWEEPS][batch]: finite up to an instance's own convergence sweep, NaN after it."""
    for b, k in enumerate(sweeps):
        k = int(k) if k > 0 else mc.shape[0]
        if not (np.all(np.isfinite(mc[:k, b])) and np.all(np.isnan(mc[k:, b]))):
            return False
    return True


def test_matrix_core_path_ran(ocs, oracle):
    """ocs_fb_sweep_matrix_core: 1 after a sweep / compute_x_lam on LQProblem with 16 states, 0 on the plugin form of the
    same problem, 0 with four states (the twin's vector mappings), 0 before any call."""
    N = 100
    tspan = oracle.linspace(0, 2.0, N + 1)
    opt = {"nERROR_PTS": N + 1, "nINTERP_PTS": 21, "nSWEEPS": 3}
    integ = ocs.RK4Integrator(tspan)
    assert ocs.fb_sweep_matrix_core(integ) == 0
    p16, _ = make(ocs, oracle, 16, 4)
    ocs.fb_sweep_batch(p16, x0_of(16, 1.0).reshape(16, 1), tspan, opt, integrator=integ)
    assert ocs.fb_sweep_matrix_core(integ) == 1 and ocs.fb_sweep_path(integ) == 2
    ocs.fb_sweep_batch(make_user(ocs, 16, 4), x0_of(16, 1.0).reshape(16, 1), tspan, opt, integrator=integ)
    assert ocs.fb_sweep_matrix_core(integ) == 0 and ocs.fb_sweep_path(integ) == 2
    rng = np.random.default_rng(1)
    ocs.compute_x_lam(p16, x0_of(16, 1.0), tspan, rng.uniform(-1, 1, (4, 2 * N + 1)), integrator=integ)
    assert ocs.fb_sweep_matrix_core(integ) == 1
    p4, _ = make(ocs, oracle, 4, 2)
    ocs.fb_sweep_batch(p4, x0_of(4, 1.0).reshape(4, 1), tspan, opt, integrator=integ)
    assert ocs.fb_sweep_matrix_core(integ) == 0


@pytest.mark.parametrize("nS,nC,N,nerr", [(8, 2, 400, 0), (16, 4, 400, 0), (17, 3, 200, 0), (32, 4, 400, 0),
                                          (16, 4, 400, 1001)])
def test_sweep_vs_oracle(ocs, oracle, nS, nC, N, nerr):
    """One instance per shape against the oracle: error points on the nodes (the loop enqueued ahead, path 2) and, for
    (16, 4, 400), the reference's 1001 error points off the nodes (path 5)."""
    pg, po = make(ocs, oracle, nS, nC)
    tspan = oracle.linspace(0, 2.0, N + 1)
    opt = {"nERROR_PTS": nerr or N + 1, "nINTERP_PTS": 101, "nSWEEPS": 200}
    ref = oracle.fb_sweep(po, x0_of(nS, 1.0), tspan, opt)
    assert ref["_sweeps"] > 0
    integ = ocs.RK4Integrator(tspan)
    r = ocs.fb_sweep_batch(pg, x0_of(nS, 1.0).reshape(nS, 1), tspan, opt, integrator=integ)
    assert ocs.fb_sweep_matrix_core(integ) == 1 and ocs.fb_sweep_path(integ) == (5 if nerr else 2)
    errs = {"J": abs(r["J"][0] - ref["J"]) / abs(ref["J"]), "x": relerr(r["x"][:, :, 0], ref["x"]),
            "lam": relerr(r["lam"][:, :, 0], ref["lam"]), "u": relerr(r["u"][:, :, 0], ref["u"])}
    print(f"nS={nS} nC={nC} N={N} nERR={opt['nERROR_PTS']}: sweeps {int(r['sweeps'][0])} (oracle {ref['_sweeps']}), {errs}")
    assert int(r["sweeps"][0]) == ref["_sweeps"]
    assert errs["J"] < 1e-10 and errs["x"] < 1e-10 and errs["lam"] < 1e-10 and errs["u"] < 1e-10


def check_batch(r, refs, which):
    """instance b of the batch result equals the single-instance oracle solve refs[which[b]]"""
    worst = 0.0
    for b, w in enumerate(which):
        ref = refs[w]
        assert int(r["sweeps"][b]) == ref["_sweeps"], (b, int(r["sweeps"][b]), ref["_sweeps"])
        e = max(abs(r["J"][b] - ref["J"]) / abs(ref["J"]), relerr(r["x"][:, :, b], ref["x"]),
                relerr(r["lam"][:, :, b], ref["lam"]), relerr(r["u"][:, :, b], ref["u"]))
        worst = max(worst, e)
    return worst


def test_frozen_instances_in_a_ragged_batch(ocs, oracle):
    """Instances that converge in different sweeps are frozen one by one while the batch goes on (batch 37: the last wave
    holds 5 trajectories): damped sweeps (uRelax = 0.25, plain rdiag) from x0 scaled by 1, 4 and 10 -- the last two with 5 %
    and 20 % of the control points on a bound -- padded with repeats; and the rdiag * 8, s = 10 instance undamped."""
    nS, nC, N, batch = 32, 4, 400, 37
    tspan = oracle.linspace(0, 2.0, N + 1)
    scales = (1.0, 4.0, 10.0)
    pg, po = make(ocs, oracle, nS, nC, rscale=1.0)
    opt = {"nERROR_PTS": N + 1, "nINTERP_PTS": 101, "nSWEEPS": 200, "uRelax": 0.25}
    refs = [oracle.fb_sweep(po, x0_of(nS, s), tspan, opt) for s in scales]
    assert all(ref["_sweeps"] > 0 for ref in refs)
    which = [b % 3 for b in range(batch)]
    X0 = np.stack([x0_of(nS, scales[w]) for w in which], axis=1)
    integ = ocs.RK4Integrator(tspan)
    r = ocs.fb_sweep_batch(pg, X0, tspan, opt, integrator=integ)
    assert ocs.fb_sweep_matrix_core(integ) == 1
    worst = check_batch(r, refs, which)
    print(f"damped batch: sweeps {sorted(set(int(k) for k in r['sweeps']))}, worst relative error {worst:.3e}")
    assert worst < 1e-10
    assert nan_pattern_ok(r["maxChange"], r["sweeps"])
    # rdiag * 8, s = 10: undamped, the control reaches a bound
    pg8, po8 = make(ocs, oracle, nS, nC)
    opt8 = {"nERROR_PTS": N + 1, "nINTERP_PTS": 1001, "nSWEEPS": 200}
    scales8 = (10.0, 1.0, 4.0)
    refs8 = [oracle.fb_sweep(po8, x0_of(nS, s), tspan, opt8) for s in scales8]
    assert all(ref["_sweeps"] > 0 for ref in refs8) and np.max(np.abs(refs8[0]["u"])) == 1.0
    which8 = [b % 3 for b in range(5)]
    r8 = ocs.fb_sweep_batch(pg8, np.stack([x0_of(nS, scales8[w]) for w in which8], axis=1), tspan, opt8, integrator=integ)
    worst8 = check_batch(r8, refs8, which8)
    print(f"rdiag * 8 batch: sweeps {[int(k) for k in r8['sweeps']]}, worst relative error {worst8:.3e}")
    assert worst8 < 1e-10 and nan_pattern_ok(r8["maxChange"], r8["sweeps"])


def test_same_solve_on_the_plugin_form(ocs, oracle):
    """The identical solve on UserProblem(lq_source + ControlChar): lane kernels for every pass.  Equal sweep counts, x,
    lam, J to 1e-10, the same NaN pattern in maxChange (its values divide a control difference by at least 1e-7 and are
    not compared)."""
    nS, nC, N, batch = 16, 4, 400, 19
    tspan = oracle.linspace(0, 2.0, N + 1)
    pg, _ = make(ocs, oracle, nS, nC)
    pu = make_user(ocs, nS, nC)
    opt = {"nERROR_PTS": N + 1, "nINTERP_PTS": 101, "nSWEEPS": 200}
    X0 = np.stack([x0_of(nS, (1.0, 4.0, 10.0)[b % 3]) for b in range(batch)], axis=1)
    ga, gb = ocs.RK4Integrator(tspan), ocs.RK4Integrator(tspan)
    ra = ocs.fb_sweep_batch(pg, X0, tspan, opt, integrator=ga)
    rb = ocs.fb_sweep_batch(pu, X0, tspan, opt, integrator=gb)
    assert ocs.fb_sweep_matrix_core(ga) == 1 and ocs.fb_sweep_matrix_core(gb) == 0
    assert ocs.fb_sweep_path(ga) == ocs.fb_sweep_path(gb)
    assert np.all(ra["sweeps"] > 0) and np.array_equal(ra["sweeps"], rb["sweeps"])
    errs = (relerr(ra["x"], rb["x"]), relerr(ra["lam"], rb["lam"]), float(np.max(np.abs(ra["J"] - rb["J"]) / np.abs(rb["J"]))))
    print(f"matrix-core vs plugin form: sweeps {sorted(set(int(k) for k in ra['sweeps']))}, x / lam / J {errs}")
    assert max(errs) < 1e-10
    assert np.array_equal(np.isnan(ra["maxChange"]), np.isnan(rb["maxChange"]))
    assert nan_pattern_ok(ra["maxChange"], ra["sweeps"])


def test_compute_x_lam_J(ocs, oracle):
    nS, nC, N, batch = 32, 4, 200, 19
    pg, po = make(ocs, oracle, nS, nC)
    tspan = oracle.linspace(0, 2.0, N + 1)
    rng = np.random.default_rng(20260405)
    u = rng.uniform(-1, 1, (nC, 2 * N + 1, batch))
    x0 = rng.normal(size=(nS, batch))
    integ = ocs.RK4Integrator(tspan)
    x, lam, J = ocs.compute_x_lam_J(pg, x0, tspan, u, integrator=integ)
    assert ocs.fb_sweep_matrix_core(integ) == 1
    go = oracle.RK4Integrator(tspan)
    for b in (0, 9, 18):
        xo, lo, Jo = oracle.compute_x_lam(go, po, x0[:, b], u[:, :, b], want_J=True)
        errs = (relerr(x[:, :, b], xo), relerr(lam[:, :, b], lo), abs(J[b] - Jo) / max(1.0, abs(Jo)))
        print(f"compute_x_lam_J instance {b}: x / lam / J {errs}")
        assert max(errs) < 1e-12
        assert np.all(lam[:, N, b] == 0.0)


@pytest.mark.parametrize("nS,nC,batch", [(8, 2, 3), (16, 4, 17), (17, 3, 17), (32, 4, 33)])
def test_state_pass_is_the_integrators_one_wave_pass(ocs, oracle, nS, nC, batch):
    """The sweep's state pass IS RK4Integrator's one-wave kernel (mapping 1; for nS > 16 the automatic choice is another
    mapping with another summation order): the state rows of compute_x_lam_J's x and its J equal compute_states' bit for
    bit.  N = 7 (odd), ragged groups of 16, random u in [-1, 1]."""
    N = 7
    pg, _ = make(ocs, oracle, nS, nC)
    tspan = oracle.linspace(0, 2.0, N + 1)
    rng = np.random.default_rng(20261019 + nS)
    u = rng.uniform(-1, 1, (nC, 2 * N + 1, batch))
    X0 = np.stack([x0_of(nS, (1.0, 4.0, 10.0)[b % 3]) for b in range(batch)], axis=1)
    integ = ocs.RK4Integrator(tspan)
    x, _, J = ocs.compute_x_lam_J(pg, X0, tspan, u, integrator=integ)
    assert ocs.fb_sweep_matrix_core(integ) == 1
    xi, Ji = ocs.RK4Integrator(tspan).set_mapping(1).compute_states(pg, X0, u)
    assert np.all(np.isfinite(x)) and np.all(np.isfinite(J))
    assert np.array_equal(x, xi[:nS]) and np.array_equal(J, Ji)


def test_batch_params_are_still_refused(ocs, oracle):
    """Per-trajectory parameters on an LQ problem end in OCS_ERR_UNSUPPORTED as before: where the matrix-core passes apply
    (nS >= 8: more than 32 parameters) they cannot even be set; where they can be set (nS = 4, nC = 1: 26 parameters; parameter 1 = A(1,1)) the
    sweep entry points refuse the problem with their existing message."""
    batch = 3
    p8, _ = make(ocs, oracle, 8, 2)
    with pytest.raises(Exception) as ei:
        p8.set_batch_params([1], np.full((1, batch), -1.0))
    assert getattr(ei.value, "code", None) == OCS_ERR_UNSUPPORTED
    nS, nC, N = 4, 1, 40
    pg, _ = make(ocs, oracle, nS, nC)
    pg.set_batch_params([1], np.full((1, batch), -1.0))
    tspan = oracle.linspace(0, 2.0, N + 1)
    X0 = np.stack([x0_of(nS, 1.0)] * batch, axis=1)
    with pytest.raises(Exception) as ei:
        ocs.fb_sweep_batch(pg, X0, tspan, {"nERROR_PTS": N + 1, "nINTERP_PTS": 21, "nSWEEPS": 3})
    assert getattr(ei.value, "code", None) == OCS_ERR_UNSUPPORTED and "per-trajectory parameters" in str(ei.value)
    with pytest.raises(Exception) as ei:
        ocs.compute_x_lam(pg, X0, tspan, np.zeros((nC, 2 * N + 1, batch)))
    assert getattr(ei.value, "code", None) == OCS_ERR_UNSUPPORTED and "per-trajectory parameters" in str(ei.value)
