"""CPU tests that pin the instrument of tests/test_gpu_nlp_accuracy.py: the extended-precision twin of the shooting objective
(tests/nlp_twin.py) against an mpmath restatement at 50 digits, against the oracle by the parity tests' measure, the host-built
basis matrices under the new measure, the non-vacuity of every case of tests/nlp_accuracy_cases.py, and the condition the error
measure has to meet: another legitimate fp64 summation order of dJdv = dJdu B' stays within K of the oracle's own error."""
import numpy as np
import pytest
from mpmath import mp

from tests import nlp_accuracy_cases as cs
from tests import nlp_twin as nt
from tests import rk4_accuracy_cases as rc
from tests import rk4_twin as tw
from tests import test_rk4_twin as t0      # its scalar mpmath restatement of RK4Integrator.m:28-121
from tests.accuracy_check import FLOOR, K

DPS = 50
LD_EPS = 2.0 ** -64
CASES = cs.all_cases()
IDS = [cs.case_id(c) for c in CASES]


@pytest.fixture(scope="module")
def ocs():
    import __graft_entry__ as g
    g.build()
    return g.load_package()


# ---- the twin against mpmath ----------------------------------------------------------------------------------------------
def _mp_basis(kind, t, n):
    """PWLinearControl.m:31-50, PWConstantControl.m:41-50, ChebyshevControl.m:21-31 on mpf scalars; t and the break points fp64"""
    tm = t0._mpf(t)
    nT = len(tm)
    B = [[mp.mpf(0)] * nT for _ in range(n)]
    if kind == "PWLinearControl":
        p = t0._mpf(nt.linspace(t[0], t[-1], n))
        for j, q in enumerate(tm):
            for i in range(n):
                if i > 0 and p[i - 1] <= q <= p[i]:
                    B[i][j] = (q - p[i - 1]) / (p[i] - p[i - 1])
                elif i < n - 1 and p[i] <= q <= p[i + 1]:
                    B[i][j] = 1 - (q - p[i]) / (p[i + 1] - p[i])
    elif kind == "PWConstantControl":
        s = t0._mpf(nt.linspace(t[0], t[-1], n + 1))
        for j, q in enumerate(tm):
            for i in range(n):
                if q >= s[i] and (i == n - 1 or q < s[i + 1]):
                    B[i][j] = mp.mpf(1)
    else:
        for j, q in enumerate(tm):
            x = 2 * (q - tm[0]) / (tm[-1] - tm[0]) - 1
            B[0][j] = mp.mpf(1)
            if n > 1:
                B[1][j] = x
            for i in range(2, n):
                B[i][j] = 2 * x * B[i - 1][j] - B[i - 2][j]
    return B


REDUCED = [("PWLinearControl", 6), ("PWConstantControl", 4), ("ChebyshevControl", 9)]
_TWIN_ERR = {}


def _twin_against_mpmath(oracle, regime, kind, nB):
    """On the reduced shape (nS = 2, N = 12, 2 trajectories, free initial states [2, 1]): the twin's error against mpmath for B
    (relative to the row's max |B|), u (rk4_twin.err restated), dJdv (windowed, and on the condition scale), lam0 and J; and the
    oracle's error against the twin on the same inputs."""
    key = (regime, kind, nB)
    if key in _TWIN_ERR:
        return _TWIN_ERR[key]
    c = cs.Case(regime, kind, nB, 2, 12, 2, True)
    par, tspan, x0, v, cc, Bt, ref = cs.reference(c)
    free = cs.free_states(c)
    t = tw.grid(tspan)[0]
    nT = t.size
    with mp.workdps(DPS):
        Bm = _mp_basis(kind, t, nB)
        eB = max(float(abs(t0._mpl(Bt[i, j]) - Bm[i][j]) / max(abs(x) for x in Bm[i])) for i in range(nB) for j in range(nT))
        e = {"B": eB, "u": 0.0, "dJdv": 0.0, "dJdv_cond": 0.0, "lam0": 0.0, "J": 0.0}
        for b in range(c.batch):
            vm = t0._mpf(v[:nB, b])
            um = [sum(vm[k] * Bm[k][j] for k in range(nB)) for j in range(nT)]
            x0m = x0[:, b].copy()
            for f, s in enumerate(free):
                x0m[s - 1] = v[nB + f, b]
            fns = t0._mp_logistic(dict(par, c=float(cc[b])))
            x, lam, dJdu = _mp_passes_mpf_u(fns, tspan, x0m, um)
            dm = [sum(Bm[k][j] * dJdu[0][j] for j in range(nT)) for k in range(nB)]
            cond = [sum(abs(Bm[k][j] * dJdu[0][j]) for j in range(nT)) for k in range(nB)]
            au = [abs(a) for a in um]
            for j in range(nT):
                s = max(au[max(0, j - tw.WINDOW):j + tw.WINDOW + 1])
                e["u"] = max(e["u"], float(abs(t0._mpl(ref["u"][0, j, b]) - um[j]) / s))
            ad = [abs(a) for a in dm]
            for k in range(nB):
                d = abs(t0._mpl(ref["dJdv"][k, b]) - dm[k])
                e["dJdv"] = max(e["dJdv"], float(d / max(ad[max(0, k - tw.WINDOW):k + tw.WINDOW + 1])))
                e["dJdv_cond"] = max(e["dJdv_cond"], float(d / cond[k]))
            for f, s in enumerate(free):
                e["lam0"] = max(e["lam0"], float(abs(t0._mpl(ref["lam0"][f, b]) - lam[s - 1][0]) / abs(lam[s - 1][0])))
            e["J"] = max(e["J"], float(abs(t0._mpl(ref["J"][b]) - x[-1][-1]) / abs(x[-1][-1])))
    _TWIN_ERR[key] = (e, {k: float(np.max(a)) for k, a in cs.oracle_errors(oracle, c).items()})
    return _TWIN_ERR[key]


def _mp_passes_mpf_u(fns, tspan, x0, um):
    """t0._mp_passes with the control given as mpf samples: the twin's u = v B is not fp64 data, so it must not be rounded"""
    return t0._mp_passes(fns, tspan, x0, np.array(um, dtype=object).reshape(1, -1), None)


@pytest.mark.parametrize("kind,nB", REDUCED, ids=[k[:-7] for k, _ in REDUCED])
@pytest.mark.parametrize("regime", cs.REGIMES)
def test_twin_against_mpmath(oracle, regime, kind, nB):
    """The twin's own error against 50 digits.  Bounds from the format and the operation counts, not from a run: B is one
    division and a subtraction per tent (4 * 2^-64), or a recurrence of nB - 2 = 7 steps whose error grows like k^2 (64 * 2^-64);
    u adds nB products; the pass pair over 12 steps is within test_rk4_twin's 64 * 2^-64; dJdv on the condition scale
    sum_j |B_kj dJdu_j| adds 25 products and sums to it: 128 * 2^-64 in all.  The windowed dJdv error is printed (the table of
    NOTES.md); the oracle's error on the same inputs must be finite."""
    e, orc = _twin_against_mpmath(oracle, regime, kind, nB)
    print("TWIN", regime, kind, nB, {k: f"{v:.1e}" for k, v in e.items()}, "ORACLE", {k: f"{v:.1e}" for k, v in orc.items()})
    assert e["B"] <= 64 * LD_EPS and e["u"] <= 64 * LD_EPS
    assert e["J"] <= 64 * LD_EPS and e["lam0"] <= 64 * LD_EPS
    assert e["dJdv_cond"] <= 128 * LD_EPS
    assert e["dJdv"] <= FLOOR / 16, "the twin's windowed error must stay an order below the floor of the statement"
    for k, v in orc.items():
        assert np.isfinite(v), k


# ---- the twin against the oracle, the cases' non-vacuity --------------------------------------------------------------------
@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_twin_matches_oracle_by_the_old_measure(oracle, c):
    """The whole twin against the oracle by the parity tests' measure at 1e-12 (J relative), and the oracle's error by the
    new measure, printed: the oracle-against-twin table of NOTES.md."""
    ref, orc = cs.reference(c)[-1], cs.oracle_objective(oracle, c)
    full = np.vstack([ref["dJdv"], ref["lam0"]]).astype(np.float64)
    assert tw.relerr_old(orc["dJdv"], full) < 1e-12
    assert np.max(tw.err_J(orc["J"], ref["J"])) < 1e-12
    assert tw.relerr_old(orc["u"], ref["u"].astype(np.float64)) < 1e-12
    e = cs.oracle_errors(oracle, c)
    print("ORACLE", cs.case_id(c), " ".join(f"{k}={float(np.max(a)):.1e}" for k, a in e.items()))
    assert all(np.all(np.isfinite(a)) for a in e.values())


@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_case_is_not_vacuous(oracle, c):
    """Each case proves its regime with the oracle and the twin alone, every property an assertion on the case itself:

    * the states stay positive, and grow at every stage in B; the control stays inside its bounds [0, 1];
    * every Chebyshev case has a row with |dJdv_k| < 1e-3 sum_j |B_kj dJdu_j| -- cancellation, which the cases build in through
      c on their first two trajectories (nlp_accuracy_cases.CANCELLING) -- and both of those trajectories show it;
    * under r = 3 the smallest |dJdv| row is at least six orders below the largest: on every trajectory of a piecewise basis
      with at least 10 functions (the late hats), and on the cancelling trajectories of a Chebyshev case.  PWLinear with two
      control points is not claimed: both hats span the whole horizon."""
    par, tspan, x0, v, cc, Bt, ref = cs.reference(c)
    orc = cs.oracle_objective(oracle, c)
    assert np.all(orc["x"][:-1] > 0) and np.all(ref["x"] > 0)
    if c.regime == "B":
        rc.assert_growing(par, ref, ref["u"])
        assert np.all(np.diff(orc["x"][:-1], axis=1) > 0)
    assert np.all(orc["u"] >= cs.BOUNDS[0][0]) and np.all(orc["u"] <= cs.BOUNDS[0][1])
    d = np.abs(orc["dJdv"][:c.nB])
    if c.kind == "ChebyshevControl":
        cond = nt.condition_scale(orc["B"], orc["dJdu"]).astype(np.float64)
        ratio = np.min(d / cond, axis=0)
        print("CANCEL", cs.case_id(c), f"min |dJdv_k| / sum_j |B_kj dJdu_j| = {ratio[0]:.1e}, {ratio[1]:.1e}; others {np.min(ratio[2:]):.1e}")
        assert np.all(ratio[:cs.CANCELLING] < 1e-3), ratio[:cs.CANCELLING]
        if c.regime == "C-r3":
            assert np.all(np.min(d, axis=0)[:cs.CANCELLING] <= 1e-6 * np.max(d, axis=0)[:cs.CANCELLING])
    elif c.regime == "C-r3" and c.nB >= 10:
        assert np.all(np.min(d, axis=0) <= 1e-6 * np.max(d, axis=0))


# ---- the measure ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_reordered_contraction_is_within_K(oracle, c):
    """The condition of the measure: the oracle's own fp64 dJdu and B, contracted in two other legitimate orders (the grid
    points from last to first; tiles of 16 columns summed pairwise), must satisfy the statement of the GPU test against the
    oracle's own error.  A measure under which they did not would reject correct kernels for their summation order."""
    ref, orc, eo = cs.reference(c)[-1], cs.oracle_objective(oracle, c), cs.oracle_errors(oracle, c)
    yard = max(float(np.max(eo["dJdv"])), FLOOR)
    for order in ("reversed", "tiles"):
        e = nt.err_dJdv(nt.contract_reordered(orc["B"], orc["dJdu"], order), ref["dJdv"])
        print("REORDER", cs.case_id(c), order, f"ratio={float(np.max(e)) / yard:.2f}")
        assert np.all(e <= K * yard), (order, float(np.max(e)), yard)


def test_err_dJdv_sees_what_relerr_cannot(oracle):
    """A relative 1e-9 in the last hat function's row under r = 3 (the row is below 1e-9): about 1e-9 by err_dJdv, a pass by
    the parity tests' max |a - b| / max(1, |b|)."""
    c = cs.Case("C-r3", "PWLinearControl", 21, 1, 72, 70, True)
    ref = cs.reference(c)[-1]
    clean = np.vstack([ref["dJdv"], ref["lam0"]]).astype(np.float64)
    planted = clean.copy()
    planted[20, 5] *= 1 + 1e-9
    assert abs(clean[20, 5]) < 1e-9
    e = nt.errors({"J": ref["J"].astype(np.float64), "dJdv": planted}, ref)["dJdv"]
    expected = 1e-9 * abs(clean[20, 5]) / np.max(np.abs(clean[16:21, 5]))     # the row against the largest of its neighbours
    assert 1e-13 < expected <= 1e-9
    assert abs(e[5] - expected) < 1e-3 * expected + 4 * tw.EPS and np.max(np.delete(e, 5)) < 4 * tw.EPS
    assert tw.relerr_old(planted, clean) < 1e-12


# ---- the library's host code --------------------------------------------------------------------------------------------------
def _row_error(B, Bt):
    """max |B - Bt| relative to the row's max |Bt|; a row no grid point touches (all zero in the twin) must be zero exactly"""
    d, scale = np.abs(np.asarray(B).astype(nt.L) - Bt), np.max(np.abs(Bt), axis=1, keepdims=True)
    assert np.all(d[scale[:, 0] == 0] == 0)
    return float(np.max(d / np.where(scale > 0, scale, 1)))


@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_host_built_basis_under_the_measure(ocs, oracle, c):
    """ocs_control_basis (the library's host-built B, which creating a handle computes without a device) and the oracle's B
    against the twin's, relative to the row's max |B|: the library within K of the oracle."""
    par, tspan, x0, v, cc, Bt, ref = cs.reference(c)
    t = tw.grid(tspan)[0]
    lib = getattr(ocs, c.kind)(t, c.nB, 1).B
    el, eo = _row_error(lib, Bt), _row_error(cs.oracle_objective(oracle, c)["B"], Bt)
    print("BASIS", cs.case_id(c), f"library={el:.2e} oracle={eo:.2e}")
    assert el <= K * max(eo, FLOOR)
    if c.kind == "PWConstantControl":
        assert el == 0.0


def test_every_family_is_reached_in_every_regime(ocs):
    """The plan of tests/test_gpu_nlp_accuracy.py, from the restated dispatch: in each regime every kernel family is reached
    by at least one (case, fusion mode); the cases without free initial states reach every family once."""
    def reached(cases):
        got = set()
        for c in cases:
            B = getattr(ocs, c.kind)(tw.grid(cs.inputs(c)[1])[0], c.nB, 1).B
            got |= {cs.family(c, m, B) for m in cs.modes(c, B)}
        return got
    for regime in cs.REGIMES:
        assert reached([c for c in CASES if c.regime == regime and c.free]) == set(cs.FAMILIES), regime
    no_free = reached(cs.NO_FREE)
    assert no_free == set(cs.FAMILIES), no_free
