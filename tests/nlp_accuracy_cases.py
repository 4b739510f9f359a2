"""Cases and shared references of the shooting objective's accuracy tests (tests/test_nlp_twin.py on the CPU,
tests/test_gpu_nlp_accuracy.py on the GPU): where [J, dJdv] = nlpObjective(v) is run to measure its rounding error against
tests/nlp_twin.py.

The regimes are those of tests/rk4_accuracy_cases.py -- its grids, its x0, its m and r -- with the control now given by
coefficients v and c per trajectory (uniform in [1, 2], as the parity tests set it; r stays one value per problem:
ocs_problem_set_batch_params refuses it).  What had to move, and why, stands next to each constant below.

    A         random grid on T = 0.03 N, states of order 1
    B         growth from x0 in [1e-3, 1e-2] to saturation on T = 6 (uniform grid), lam(:, 1) of order 1e4
    C-r0.05   jittered grid on T = 8
    C-r3      the same under the discount e^{-3t}: dJdu falls through ten orders

Shapes (nS, N, batch), smallest at which each kernel family can still go wrong: N = 72 is three superblocks of the adjoint scan
with dead chunks and nine whole 8-step blocks, N = 13 is odd (lane kernels only, the banded cursor ends mid-band); batch 64 is a
whole tile (the fused wave path is reachable), 70 = 64 + 6 a partial last wave; nS <= 2 takes the two-role lane kernels at
N % 8 == 0, nS = 4 the one-wave ones.  Every case has free initial states ([nS, 1] where nS > 1, else [1]) but the repeats of
NO_FREE, one per family.

`family` restates the dispatch of ocs_nlp_objective_dev (csrc/ocs_control.cpp) and its support predicates, so that a test can
say which kernels a (case, fusion mode) pair must reach and assert what is observable of it."""
import collections
import zlib

import numpy as np

from tests import nlp_twin as nt
from tests import rk4_accuracy_cases as rc
from tests import rk4_twin as tw

Case = collections.namedtuple("Case", "regime kind nB nS N batch free")

REGIMES = ("A", "B", "C-r0.05", "C-r3")
BOUNDS = [[0.0, 1.0]]
C_RANGE = (1.0, 2.0)          # c per trajectory (tests/test_gpu_controls_shooting.py)
PW_RANGE = (0.05, 0.45)       # the range of rk4_accuracy_cases._benign_controls, 0.25 +- 0.2
# Chebyshev in A and C: the parity tests' decaying coefficients 0.05 randn / k around a constant; the constant is 0.25, the
# centre of the benign range, not the parity tests' 0.4: on T = 8 the row with m = 1.5 sustains a harvest of at most
# m^2 / 4 = 0.5625, which 0.4 + sum_k 0.05 |randn| / k exceeds on some trajectories, sending that state through zero
CHEB_CENTRE, CHEB_DECAY = 0.25, 0.05
# B: the controls of the pass-pair regime fall in time, 1e-4 U(0.2, 1) e^{-rate t} with rate in [0.1, 1], so that the
# equilibrium the state chases keeps rising and x (m - x) - u > 0 holds at every stage.  The same function sampled at the
# control points (PWLinear, PWConstant); for Chebyshev its linear part v_1 = -0.4 v_0 with v_0 = 5e-5 U(0.2, 1) and the higher
# coefficients 0.01 v_0 randn / k^2: the slope they add, at most sum_k k^2 0.01 |randn| / k^2 of v_0 per unit of tTrans,
# stays below the 0.4 v_0 of the linear part, so u still falls
B_SCALE, B_CHEB_SLOPE, B_CHEB_HIGHER = 1e-4, -0.4, 0.01
# Cancellation by construction (Chebyshev cases): x and lam do not depend on c, so dJdu = -sum_k lam_k (..) + c 2 u e^{-rt} (..)
# and every row dJdv_k = -a_k + c b_k is affine in c.  The first CANCELLING trajectories of a Chebyshev case take c = a_k / b_k,
# the value at which row k cancels completely: row 0 on trajectory 0 (a_0, b_0 > 0 always: the integrals of sum lam and of
# 2 u e^{-rt}), the highest row with a_k / b_k > 0 on trajectory 1.  These c lie outside C_RANGE (6 to 40 in A and C, 1e7 to
# 1e8 in B where lam is 1e4 and u 1e-4: the cost weight tests/fbs_accuracy_cases.py needs in B as well); c weighs the cost
# alone, so the states and the validity of the regime are untouched.  Without it a row of a one-signed dJdu (all of B) or of
# degree <= 4 never comes within 1e-3 of its condition scale.
CANCELLING = 2
# B at N = 13: horizon 3 instead of 6, as in tests/fbs_accuracy_cases.py (a step of 6 / 13 overshoots the saturated state)
B_SHORT_SCALE = 0.5

CHEB_SHAPES = {(1, 72, 64): (5, 16, 17, 32), (1, 72, 70): (16, 17), (2, 72, 70): (16, 32), (4, 72, 70): (5, 17),
               (2, 13, 70): (16, 17), (1, 13, 64): (5, 32)}
# PWLinear 30 at N = 13: more control points than the 27 grid points, the band moves by two rows: unfused sparse kernels
PWL_SHAPES = {(1, 72, 70): (2, 21), (2, 72, 64): (21,), (4, 72, 70): (21,), (1, 13, 70): (2, 21, 30), (2, 13, 70): (2,),
              (4, 13, 64): (21,)}
PWC_SHAPES = {(1, 72, 70): (10,), (2, 72, 64): (10,), (4, 72, 70): (10,), (1, 13, 70): (10,), (2, 13, 70): (10,)}
NO_FREE = (Case("A", "ChebyshevControl", 16, 1, 72, 64, False), Case("A", "ChebyshevControl", 17, 4, 72, 70, False),
           Case("A", "ChebyshevControl", 5, 4, 72, 70, False),
           Case("A", "PWLinearControl", 21, 1, 72, 70, False), Case("A", "PWConstantControl", 10, 2, 72, 64, False))


def all_cases():
    out = []
    for regime in REGIMES:
        for kind, shapes in (("ChebyshevControl", CHEB_SHAPES), ("PWLinearControl", PWL_SHAPES), ("PWConstantControl", PWC_SHAPES)):
            for (nS, N, batch), sizes in shapes.items():
                out += [Case(regime, kind, nB, nS, N, batch, True) for nB in sizes]
    return out + list(NO_FREE)


def case_id(c):
    return f"{c.regime}-{c.kind[:-7]}{c.nB}-nS{c.nS}-N{c.N}-b{c.batch}" + ("" if c.free else "-nofree")


def free_states(c):
    """FreeInitStates (1-based) of a case"""
    if not c.free:
        return []
    return [c.nS, 1] if c.nS > 1 else [1]


def inputs(c):
    """(par, tspan, x0 [nS][batch], v [nB + nFree][batch], cs [batch]); par = dict(m, c, r) with the shared c of the regime --
    the per-trajectory values are cs"""
    par, tspan, x0, _, _ = rc.logistic_regime(c.regime, c.nS, c.N, rc.LOGISTIC_BATCH)
    x0 = np.ascontiguousarray(x0[:, :c.batch])
    if c.regime == "B" and c.N < 72:
        tspan = tspan * B_SHORT_SCALE
    rng = np.random.default_rng([zlib.crc32(case_id(c).encode()), c.nB, c.nS, c.N])
    cheb = c.kind == "ChebyshevControl"
    k = np.arange(1, c.nB + 1)[:, None]
    if c.regime == "B":
        amp, rate = rng.uniform(0.2, 1.0, c.batch), rng.uniform(0.1, 1.0, c.batch)
        if cheb:
            v = B_CHEB_HIGHER * rng.normal(size=(c.nB, c.batch)) / k ** 2
            v[0] = 1.0
            if c.nB > 1:
                v[1] = B_CHEB_SLOPE
            v = v * (0.5 * B_SCALE * amp)[None, :]
        else:
            pts = nt.linspace(tspan[0], tspan[-1], c.nB + (c.kind == "PWConstantControl"))[:c.nB]
            v = B_SCALE * amp[None, :] * np.exp(-rate[None, :] * pts[:, None])
        xfree = rng.uniform(1e-3, 1e-2, (2, c.batch))
    else:
        if cheb:
            v = CHEB_DECAY * rng.normal(size=(c.nB, c.batch)) / k
            v[0] += CHEB_CENTRE
        else:
            v = rng.uniform(PW_RANGE[0], PW_RANGE[1], (c.nB, c.batch))
        xfree = rng.uniform(0.8, 2.5, (2, c.batch))
    v = np.vstack([v, xfree[:len(free_states(c))]])
    cs = rng.uniform(C_RANGE[0], C_RANGE[1], c.batch)
    if cheb:
        cs[:CANCELLING] = _cancelling_c(c, par, tspan, x0[:, :CANCELLING], v[:, :CANCELLING])
    return par, tspan, x0, v, cs


def _cancelling_c(c, par, tspan, x0, v):
    """c of the first CANCELLING trajectories of a Chebyshev case (the comment at CANCELLING): the root of dJdv_k(c) = 0, from
    the twin at c = 1 and c = 2, rounded to fp64"""
    Bt = nt.basis(c.kind, tw.grid(tspan)[0], c.nB)
    free = free_states(c)
    x0 = np.array(x0)
    for f, s in enumerate(free):
        x0[s - 1] = v[c.nB + f]
    u = nt.compute_u(Bt, v[:c.nB], 1)
    lamT = np.zeros((c.nS + 1, x0.shape[1]))
    lamT[-1] = 1
    d = [Bt @ tw.passes(tw.LogisticK(par["m"], cv, par["r"]), tspan, x0, u, lamT)["dJdu"][0] for cv in (1.0, 2.0)]
    b = d[1] - d[0]                     # dJdv = -a + c b
    a = b - d[0]
    out = np.empty(x0.shape[1])
    for t in range(x0.shape[1]):
        rows = [0] if t == 0 else [k for k in range(c.nB - 1, -1, -1) if a[k, t] / b[k, t] > 0]
        out[t] = float(a[rows[0], t] / b[rows[0], t])
    assert np.all(out > 0)
    return out


def banded(B):
    """upload_control's test of a banded basis (csrc/ocs_control.cpp): every column has one or two consecutive non-zeros and the
    band's first row moves up by at most one from column to column"""
    nB, nT = B.shape
    rprev = 0
    for j in range(nT):
        nz = np.flatnonzero(B[:, j])
        if nz.size == 0 or nz.size > 2 or nz[-1] - nz[0] + 1 != nz.size:
            return False
        first = int(nz[0])
        if nz.size == 2 or j == 0 or first in (rprev, rprev + 1):
            r = first if (nz.size == 2 or j == 0) else rprev
        else:
            r = first - 1
        if j > 0 and not 0 <= r - rprev <= 1:
            return False
        rprev = r
    return True


def family(c, mode, B):
    """Which kernels ocs_nlp_objective_dev runs for case c under set_fusion(mode), B the library's basis matrix (fp64):

        "wave"            k_forward_p2 + k_backward_fcs, the products as fp64 MFMA tiles (fused_wave_supported)
        "lane-fc2"        k_forward_fc2 / k_backward_fc2 (nBasis <= 16, nS <= 2, whole 8-step blocks, batch < 32768)
        "lane-2group"     k_forward_fc / k_backward_fc in the two-group form (nBasis > 16)
        "lane-fc"         k_forward_fc / k_backward_fc, one wave
        "banded"          k_forward_fb / k_backward_fb
        "unfused-dense"   k_basis_expand_dense / k_basis_contract_dense around the automatic pass pair
        "unfused-sparse"  k_basis_expand / k_basis_contract around the automatic pass pair

    dense: more than half of B non-zero and nBasis <= 32 (upload_control) -- PWLinear with two control points is dense.  Only
    the forced modes are restated: "auto" fuses the lane and banded kernels from batch 16384 / 32768 on, far above the batches
    here, but takes the fused wave path at ANY batch up to 32768 whose shape fused_wave_supported accepts (nS = 1, N = 72,
    batch 64 here); no test runs "auto"."""
    assert mode in ("on", "lane", "off")
    dense = c.nB <= 32 and 2 * np.count_nonzero(B) > B.size
    if dense:
        if mode == "off":
            return "unfused-dense"
        if mode == "on" and c.nS == 1 and c.N >= 8 and c.N % 8 == 0 and c.batch % 64 == 0:
            return "wave"
        if c.nB > 16:
            return "lane-2group"
        return "lane-fc2" if c.nS <= 2 and c.N >= 8 and c.N % 8 == 0 else "lane-fc"
    if mode == "on" and banded(B):       # ("lane" does not select the banded kernels: fuse_mode == 2 || batch >= 32768)
        return "banded"
    return "unfused-sparse"


def leaves_checkpoints(g, prob, N, batch):
    """What can be observed of fused / unfused after nlp_objective: the device-side adjoint pass (ocs_compute_adjoints_dev)
    accepts the integrator's checkpoints after an unfused evaluation and refuses them (OCS_ERR_ORDER) after a fused one,
    whose checkpoints belong to no control in memory.  (The host-array compute_adjoints refuses after both: it wants the
    checkpoints of a host compute_states.)  True: accepted."""
    import torch
    u = torch.zeros((2 * N + 1, 1, batch), dtype=torch.float64, device="cuda:0")
    try:
        g.compute_adjoints_dev(prob, u, dJdu=torch.empty_like(u))
        torch.cuda.synchronize()
    except Exception as e:
        if "needs compute_states first" in str(e):
            return False
        raise
    return True


FAMILIES = ("wave", "lane-fc2", "lane-2group", "lane-fc", "banded", "unfused-dense", "unfused-sparse")
FUSED = ("wave", "lane-fc2", "lane-2group", "lane-fc", "banded")


def modes(c, B):
    """the fusion modes a case is run under: every one that reaches another family"""
    dense = c.nB <= 32 and 2 * np.count_nonzero(B) > B.size
    return ("on", "lane", "off") if dense and family(c, "on", B) == "wave" else (("lane", "off") if dense else ("on", "off"))


_CASES = {}   # computed once per case, shared by the tests that need it, never written again


def reference(c):
    """(par, tspan, x0, v, cs, Btwin, ref): inputs, the twin's basis matrix and the twin's nlp_objective"""
    key = ("ref", c)
    if key not in _CASES:
        par, tspan, x0, v, cs = inputs(c)
        Bt = nt.basis(c.kind, tw.grid(tspan)[0], c.nB)
        ref = nt.nlp_objective(tw.LogisticK(par["m"], cs, par["r"]), tspan, Bt, x0, v, free_states(c))
        _CASES[key] = (par, tspan, x0, v, cs, Bt, ref)
    return _CASES[key]


def oracle_objective(oracle, c):
    """The oracle's nlp_objective on every trajectory of the case (one call each): dict J [batch], dJdv [nB + nFree][batch],
    u [1][2N+1][batch], dJdu [1][2N+1][batch], x [nS+1][N+1][batch], B (its basis matrix)"""
    key = ("oracle", c)
    if key not in _CASES:
        par, tspan, x0, v, cs, _, _ = reference(c)
        go = oracle.RK4Integrator(tspan)
        co = getattr(oracle, c.kind)(go.t, c.nB, 1)
        out = {k: [] for k in ("J", "dJdv", "u", "dJdu", "x")}
        free = free_states(c)
        for b in range(c.batch):
            po = oracle.LogisticProblem(par["m"], cs[b], par["r"], BOUNDS)
            J, d, x0b = oracle.nlp_objective(go, po, co, x0[:, b], v[:, b], FreeInitStates=free)
            u = co.compute_u(v[:c.nB, b])
            x, J2 = go.compute_states(po, x0b, u)
            _, dJdu = go.compute_adjoints(po, u)
            assert J2 == J
            for k, a in zip(out, (J, d, u, dJdu, x)):
                out[k].append(a)
        res = {k: (np.array(a) if k == "J" else np.stack(a, axis=-1)) for k, a in out.items()}
        res["B"] = co.B
        _CASES[key] = res
    return _CASES[key]


def oracle_errors(oracle, c):
    """the oracle's error against the twin per output and trajectory: the yardstick (u included)"""
    key = ("oerr", c)
    if key not in _CASES:
        orc, ref = oracle_objective(oracle, c), reference(c)[-1]
        _CASES[key] = nt.errors({"J": orc["J"], "dJdv": orc["dJdv"], "u": orc["u"]}, ref)
    return _CASES[key]


def state_factor(c):
    """S_b = max (1 + m / (2 |x|)) over the rows and nodes of trajectory b, from the twin's states: the derived loss of a state
    pass that carries z = x - m/2 (tests/test_gpu_rk4_accuracy.py::test_logistic_pass_pair_error derives it)"""
    par, ref = reference(c)[0], reference(c)[-1]
    half_m = np.asarray(par["m"], dtype=np.longdouble)[:, None, None] / 2
    return np.max(1 + half_m / np.abs(ref["x"]), axis=(0, 1)).astype(np.float64)
