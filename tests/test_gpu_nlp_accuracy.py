"""Rounding error of the shooting objective [J, dJdv] = nlpObjective(v) on the GPU, measured on a local scale against the
extended-precision twin (tests/nlp_twin.py, pinned in tests/test_nlp_twin.py).

tests/test_gpu_controls_shooting.py compares ocs_nlp_objective with the fp64 oracle by max |a - b| / max(1, |b|) < 1e-12: absolute
wherever a value is below 1, which is most of dJdv under a discount and every high-degree Chebyshev row.  Here every kernel
family that produces [J, dJdv] -- five summation orders of the same sums -- is compared with the twin by its measure (J relative,
dJdv windowed over the basis index, each free-initial-state row relative to itself), and every output of every trajectory must
satisfy the statement of tests/test_gpu_rk4_accuracy.py with its constants (tests/accuracy_check.py):

    err_gpu <= K * max(err_oracle, 8 eps),      eps = 2^-53,  K = 8,

the yardstick being the oracle's error on the same trajectories (all of them: the oracle takes one per call and is fast enough
at these shapes).

Which kernels a (case, fusion mode) pair reaches is restated from ocs_nlp_objective_dev in nlp_accuracy_cases.family, and what
can be observed of it is asserted on every run: after a fused call the device-side adjoint pass refuses the
integrator's checkpoints (they belong to no control in memory) and after an unfused one it accepts them
(nlp_accuracy_cases.leaves_checkpoints); the wave path's bits differ from the lane kernels' on the
same inputs; OCS_FC2, which would move the two-role boundary, is unset.  tests/test_nlp_twin.py asserts that the plan reaches every
family in every regime.  A case that fell back to the unfused path where a fused family is planned fails the refusal.

The derived exception, regime B where the state pass carries z = x - m/2.  From the kernel text: the fused wave path launches
k_forward_p2<P, true, false, UNI, NKS, TPW> (csrc/ocs_fused_wave_kernels.hip run_forward_fcw_t), and the recursion wave of that
kernel (csrc/ocs_pipeline2_body.inc, wave == 1) starts from z = x0 - mh with mh = P::row_shift(rp) = m/2 for the logistic rows
(P::HAS_SHIFT), advances z by row_f_shifted through the four stages and adds mh back only when it stores x(t_N); the expansion
waves (NKS > 0) change where the control samples come from, not what the recursion carries.  So the fused wave state pass
commits eps |x - m/2| per operation where the plain recursion commits eps |x|, and the bound of trajectory b is
K * S_b * max(err_oracle, 8 eps) for J, dJdv and lam0, S_b = max (1 + m / (2 |x|)) from the twin's states, exactly as
test_logistic_pass_pair_error derives it.  The same holds for the UNFUSED families in B wherever the automatic pass pair takes
k_forward_p2 for the leading whole 8-step blocks (launch_forward, csrc/ocs_kernels.hip: N >= 8 and a batch tile_ok accepts --
every unfused case of B here).  The lane and banded kernels carry x itself and are held to the plain K in every regime, and
so is every family in A and C.

Every run prints one ACCURACY line of ratios; the measured table is in NOTES.md."""
import os

import numpy as np
import pytest

from tests import fbs_accuracy_cases as fc
from tests import nlp_accuracy_cases as cs
from tests import nlp_twin as nt
from tests import rk4_accuracy_cases as rc
from tests import rk4_twin as tw
from tests.accuracy_check import check_ratios

pytestmark = pytest.mark.gpu
CASES = cs.all_cases()


@pytest.fixture(scope="module")
def ocs():
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    import __graft_entry__ as g
    return g.load_package()


def _carries_z(c, fam):
    """module docstring: the state pass of this run is k_forward_p2 on (part of) the horizon"""
    if fam == "wave":
        return True
    return fam.startswith("unfused") and c.N >= 8 and fc.tile_ok(c.batch, 64 // c.nS)


@pytest.mark.parametrize("c", CASES, ids=[cs.case_id(c) for c in CASES])
def test_objective_error(ocs, oracle, c):
    """nlp_objective once per fusion mode that reaches another family (nlp_accuracy_cases.modes), c per trajectory, free
    initial states: J, dJdv and lam0 of every trajectory against the twin."""
    assert os.environ.get("OCS_FC2") is None
    par, tspan, x0, v, cc, _, ref = cs.reference(c)
    yard = {k: e for k, e in cs.oracle_errors(oracle, c).items() if k != "u"}
    free = cs.free_states(c)
    pg = ocs.LogisticProblem(par["m"], par["c"], par["r"], cs.BOUNDS)
    pg.set_batch_params([0], cc[None, :])                 # LogisticK parameter block [c r m_1..m_nS]: c per trajectory
    g = ocs.RK4Integrator(tspan)
    assert np.array_equal(g.t, tw.grid(tspan)[0])        # the grid is data: the same bits for the twin and the library
    cg = getattr(ocs, c.kind)(g.t, c.nB, 1)
    got = {}
    try:
        for mode in cs.modes(c, cg.B):
            fam = cs.family(c, mode, cg.B)
            cg.set_fusion(mode)
            J, d, x0n = ocs.nlp_objective(g, pg, cg, x0.copy(), v, FreeInitStates=free)
            assert np.array_equal(x0n, ref["x0"])
            assert cs.leaves_checkpoints(g, pg, c.N, c.batch) == (fam not in cs.FUSED), (mode, fam)
            got[fam] = (J, d)
            factor = cs.state_factor(c) if c.regime == "B" and _carries_z(c, fam) else None
            check_ratios(f"nlp {cs.case_id(c)} {mode} {fam}", nt.errors({"J": J, "dJdv": d}, ref), yard, factor)
    finally:
        cg.set_fusion("auto")
    if "wave" in got:
        lane = got["lane-fc2"] if "lane-fc2" in got else got["lane-2group"]
        assert not (np.array_equal(got["wave"][0], lane[0]) and np.array_equal(got["wave"][1], lane[1]))


STANDALONE = [("PWLinearControl", 21, 3, 1.0), ("PWConstantControl", 10, 2, 1.0), ("ChebyshevControl", 16, 1, 1.0),
              ("ChebyshevControl", 16, 2, 1.0), ("ChebyshevControl", 17, 1, 1.0), ("ChebyshevControl", 17, 2, 1.0),
              ("ChebyshevControl", 16, 1, 1e-8), ("ChebyshevControl", 17, 2, 1e-8), ("PWLinearControl", 21, 3, 1e-8)]


@pytest.mark.parametrize("kind,nB,nC,scale", STANDALONE, ids=[f"{k[:-7]}{n}x{m}-{s:g}" for k, n, m, s in STANDALONE])
def test_standalone_basis_kernels_error(ocs, oracle, kind, nB, nC, scale):
    """compute_u and compute_dJdv alone, batch 70, on the jittered grid of regime C (N = 72, T = 8): v and dJdu standard normal
    (both signs), the columns of dJdu scaled by e^{-3t} so that the sum of a row spans eleven orders.  The sparse kernels
    k_basis_expand / k_basis_contract (PWLinear 21 x 3 controls, PWConstant 10 x 2) and the dense ones k_basis_expand_dense /
    k_basis_contract_dense (Chebyshev 16 and 17: the 16- and the 32-column table; 1 and 2 controls) against the twin's products
    with the twin's B, the oracle's compute_u / compute_dJdv per trajectory as the yardstick.  scale = 1e-8 repeats a sparse
    and two dense shapes with v and dJdu that small, so that every output is far below 1 in absolute size (the measure is
    relative; a kernel that treated small outputs differently is seen only here)."""
    batch = 70
    _, tspan, _, _, _ = rc.logistic_regime("C-r3", 1, 72)
    t = tw.grid(tspan)[0]
    rng = np.random.default_rng([nB, nC, len(kind)])
    v = scale * rng.normal(size=(nC * nB, batch))
    dJdu = scale * rng.normal(size=(nC, t.size, batch)) * np.exp(-3.0 * t)[None, :, None]
    Bt = nt.basis(kind, t, nB)
    ref = {"u": nt.compute_u(Bt, v, nC), "dJdv": nt.compute_dJdv(Bt, dJdu)}
    co, cg = getattr(oracle, kind)(t, nB, nC), getattr(ocs, kind)(t, nB, nC)
    uo = np.stack([co.compute_u(v[:, b]) for b in range(batch)], axis=-1)
    do = np.stack([co.compute_dJdv(dJdu[:, :, b]) for b in range(batch)], axis=-1)

    def errs(u, d):
        return {"u": np.max(np.stack([tw.err(u[k:k + 1], ref["u"][k:k + 1]) for k in range(nC)]), axis=0),
                "dJdv": nt.err_dJdv(d, ref["dJdv"], nC)}
    check_ratios(f"basis {kind} {nB} x {nC} scale {scale:g}", errs(cg.compute_u(v), cg.compute_dJdv(dJdu)), errs(uo, do))


B_CONTRACTIONS = [cs.Case("B", "ChebyshevControl", 16, 1, 72, 64, True), cs.Case("B", "ChebyshevControl", 32, 2, 72, 70, True),
                  cs.Case("B", "PWLinearControl", 21, 1, 72, 70, True), cs.Case("B", "PWConstantControl", 10, 4, 72, 70, True)]


@pytest.mark.parametrize("c", B_CONTRACTIONS, ids=[cs.case_id(c) for c in B_CONTRACTIONS])
def test_contraction_of_regime_B_gradient_error(ocs, oracle, c):
    """compute_dJdv alone on regime B's dJdu (the oracle's fp64 dJdu of the case: lam of order 1e4, no state pass involved)
    under the plain K: in test_objective_error the unfused contractions of B stand behind the state pass's factor S_b; here
    the dense and the sparse kernel are held to K on the same data.  (The contraction inside the fused wave adjoint has no
    entry point of its own; in B it stays behind S_b.)"""
    tspan = cs.reference(c)[1]
    orc = cs.oracle_objective(oracle, c)
    t = tw.grid(tspan)[0]
    dJdu = np.ascontiguousarray(orc["dJdu"])
    ref = nt.compute_dJdv(nt.basis(c.kind, t, c.nB), dJdu)
    co, cg = getattr(oracle, c.kind)(t, c.nB, 1), getattr(ocs, c.kind)(t, c.nB, 1)
    do = np.stack([co.compute_dJdv(dJdu[:, :, b]) for b in range(c.batch)], axis=-1)
    check_ratios(f"contraction {cs.case_id(c)}", {"dJdv": nt.err_dJdv(cg.compute_dJdv(dJdu), ref)},
                 {"dJdv": nt.err_dJdv(do, ref)})
