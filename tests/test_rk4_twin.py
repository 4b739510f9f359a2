"""CPU tests that pin the instrument of tests/test_gpu_rk4_accuracy.py: the extended-precision twin (tests/rk4_twin.py) against
an mpmath restatement at 50 digits, the non-vacuity of the oracle's error as a yardstick, and the error measure itself.

The mpmath restatement is scalar, one trajectory at a time, RK4Integrator.m:28-121 line by line on Python lists; it runs at
the smallest shapes only (Logistic nS = 1, 2, 4 with N = 24 and 3 trajectories per regime; LQ nS = 5, nC = 2, N = 16 and 2
trajectories).  Non-vacuity: on every regime and shape of the GPU test the oracle's error against the twin is at least 16
times the twin's own error against mpmath, so the ratios formed there compare rounding errors of fp64 programs, not the
noise of the reference."""
import numpy as np
import pytest
from mpmath import mp   # (comes with sympy, which tests/test_symbolic.py needs already)

from tests import rk4_accuracy_cases as cs
from tests import rk4_twin as tw

DPS = 50

_TWIN_ERR = {}   # (family, regime) -> {output: the twin's error against mpmath}, filled once


def _mpf(a):
    return [mp.mpf(float(v)) for v in np.ravel(a)]


def _mpl(v):
    """a long double as the exact mpf: its fp64 head plus the remainder (both conversions are exact)"""
    hi = float(v)
    return mp.mpf(hi) + mp.mpf(float(v - np.longdouble(hi)))


def _mp_logistic(par):
    m, c, r = _mpf(par["m"]), mp.mpf(par["c"]), mp.mpf(par["r"])
    nS = len(m)

    def F(t, y, u):
        e = mp.exp(-r * t)
        return [y[k] * (m[k] - y[k]) - u[0] for k in range(nS)] + [e * (sum(y[k] * y[k] for k in range(nS)) + c * u[0] * u[0])]

    def dFdx(t, y, u, v):
        e = mp.exp(-r * t)
        return [(m[k] - 2 * y[k]) * v[k] + e * 2 * y[k] * v[nS] for k in range(nS)] + [mp.mpf(0)]

    def dFdu(t, y, u, v):
        return [-sum(v[k] for k in range(nS)) + mp.exp(-r * t) * 2 * c * u[0] * v[nS]]
    return F, dFdx, dFdu


def _mp_lq(par):
    A, Bu = np.asarray(par["A"]), np.asarray(par["Bu"])
    nS, nC = Bu.shape
    Am = [[mp.mpf(float(A[i, j])) for j in range(nS)] for i in range(nS)]
    Bm = [[mp.mpf(float(Bu[i, j])) for j in range(nC)] for i in range(nS)]
    q, rd, r = _mpf(par["q"]), _mpf(par["rdiag"]), mp.mpf(par["r"])

    def F(t, y, u):
        top = [sum(Am[i][j] * y[j] for j in range(nS)) + sum(Bm[i][j] * u[j] for j in range(nC)) for i in range(nS)]
        return top + [mp.exp(-r * t) * (sum(q[k] * y[k] * y[k] for k in range(nS)) + sum(rd[k] * u[k] * u[k] for k in range(nC)))]

    def dFdx(t, y, u, v):
        e = mp.exp(-r * t)
        return [sum(Am[j][i] * v[j] for j in range(nS)) + e * 2 * q[i] * y[i] * v[nS] for i in range(nS)] + [mp.mpf(0)]

    def dFdu(t, y, u, v):
        e = mp.exp(-r * t)
        return [sum(Bm[j][i] * v[j] for j in range(nS)) + e * 2 * rd[i] * u[i] * v[nS] for i in range(nC)]
    return F, dFdx, dFdu


def _mp_passes(fns, tspan, x0, u, lamT):
    """RK4Integrator.m:28-121 for one trajectory: x0 [nS], u [nC][2N+1], lamT [nS+1] or None -> x, lam [nS+1][N+1], dJdu"""
    F, dFdx, dFdu = fns
    tg, hg = tw.grid(tspan)
    t, h = _mpf(tg), _mpf(hg)
    N, nA, nC = len(h), len(x0) + 1, u.shape[0]
    # (u: fp64 samples, or mpf samples as they are -- tests/test_nlp_twin.py hands over a control that is not fp64 data)
    uc = [[u[c, j] if isinstance(u[c, j], mp.mpf) else mp.mpf(float(u[c, j])) for c in range(nC)] for j in range(2 * N + 1)]
    axpy = lambda y, a, f: [y[k] + a * f[k] for k in range(nA)]
    xK = [[None] * 4 for _ in range(N + 1)]
    xK[0][0] = _mpf(x0) + [mp.mpf(0)]
    for i in range(N):
        y1 = xK[i][0]
        F1 = F(t[2 * i], y1, uc[2 * i])
        xK[i][1] = axpy(y1, h[i] / 2, F1)
        F2 = F(t[2 * i + 1], xK[i][1], uc[2 * i + 1])
        xK[i][2] = axpy(y1, h[i] / 2, F2)
        F3 = F(t[2 * i + 1], xK[i][2], uc[2 * i + 1])
        xK[i][3] = axpy(y1, h[i], F3)
        F4 = F(t[2 * i + 2], xK[i][3], uc[2 * i + 2])
        xK[i + 1][0] = [y1[k] + h[i] / 6 * (F1[k] + 2 * F2[k] + 2 * F3[k] + F4[k]) for k in range(nA)]
    lam = [None] * (N + 1)
    lam[N] = [mp.mpf(0)] * (nA - 1) + [mp.mpf(1)] if lamT is None else _mpf(lamT)
    dJdk = [[None] * 4 for _ in range(N)]
    for i in range(N - 1, -1, -1):
        ln = lam[i + 1]
        dJdk[i][3] = [h[i] / 6 * v for v in ln]
        d3 = dFdx(t[2 * i + 2], xK[i][3], uc[2 * i + 2], dJdk[i][3])
        dJdk[i][2] = [h[i] / 3 * ln[k] + h[i] * d3[k] for k in range(nA)]
        d2 = dFdx(t[2 * i + 1], xK[i][2], uc[2 * i + 1], dJdk[i][2])
        dJdk[i][1] = [h[i] / 3 * ln[k] + h[i] / 2 * d2[k] for k in range(nA)]
        d1 = dFdx(t[2 * i + 1], xK[i][1], uc[2 * i + 1], dJdk[i][1])
        dJdk[i][0] = [h[i] / 6 * ln[k] + h[i] / 2 * d1[k] for k in range(nA)]
        d0 = dFdx(t[2 * i], xK[i][0], uc[2 * i], dJdk[i][0])
        lam[i] = [ln[k] + d1[k] + d2[k] + d3[k] + d0[k] for k in range(nA)]
    dJdu = [None] * (2 * N + 1)
    dJdu[0] = dFdu(t[0], xK[0][0], uc[0], dJdk[0][0])
    for i in range(N):
        a, b = dFdu(t[2 * i + 1], xK[i][1], uc[2 * i + 1], dJdk[i][1]), dFdu(t[2 * i + 1], xK[i][2], uc[2 * i + 1], dJdk[i][2])
        dJdu[2 * i + 1] = [a[c] + b[c] for c in range(nC)]
    for i in range(1, N):
        a, b = dFdu(t[2 * i], xK[i][0], uc[2 * i], dJdk[i][0]), dFdu(t[2 * i], xK[i - 1][3], uc[2 * i], dJdk[i - 1][3])
        dJdu[2 * i] = [a[c] + b[c] for c in range(nC)]
    dJdu[2 * N] = dFdu(t[2 * N], xK[N - 1][3], uc[2 * N], dJdk[N - 1][3])
    cols = lambda rows, n: [[rows[j][k] for j in range(len(rows))] for k in range(n)]
    return cols([xK[i][0] for i in range(N + 1)], nA), cols(lam, nA), cols(dJdu, nC)


def _twin_error_against_mpmath(*args):
    with mp.workdps(DPS):   # (local: the working precision of mpmath is global state that sympy shares)
        return _twin_error_at_working_precision(*args)


def _twin_error_at_working_precision(fns, prob, tspan, x0, u, lamT):
    """err of every output of the twin with the mpmath result as the reference, maximum over the trajectories.  The twin's
    longdouble arrays are compared in mpmath (nothing is rounded to fp64 on the way): the measure of rk4_twin.err, restated."""
    ref = tw.passes(prob, tspan, x0, u, lamT)
    worst = {k: 0.0 for k in tw.OUTPUTS}

    def local(v, r):          # v: longdouble [rows][cols], r: mpf [rows][cols]
        rows, n = len(r), len(r[0])
        a = [max(abs(r[k][j]) for k in range(rows)) for j in range(n)]
        e = mp.mpf(0)
        for j in range(n):
            s = max(a[max(0, j - tw.WINDOW):j + tw.WINDOW + 1])
            for k in range(rows):
                d = abs(_mpl(v[k][j]) - r[k][j])
                assert s > 0 or d == 0
                if s > 0:
                    e = max(e, d / s)
        return float(e)
    for b in range(x0.shape[1]):
        x, lam, dJdu = _mp_passes(fns, tspan, x0[:, b], u[:, :, b], None)
        _, lam2, d2 = _mp_passes(fns, tspan, x0[:, b], u[:, :, b], lamT[:, b])
        nS = x0.shape[0]
        got = {"x": local(ref["x"][:, :, b], x[:nS]), "cost": local(ref["cost"][:, :, b], x[nS:]),
               "J": float(abs(_mpl(ref["J"][b]) - x[nS][-1]) / abs(x[nS][-1])),
               "lam": local(ref["lam"][:nS, :, b], lam[:nS]), "lam2": local(ref["lam2"][:nS, :, b], lam2[:nS]),
               "dJdu": local(ref["dJdu"][:, :, b], dJdu), "d2": local(ref["d2"][:, :, b], d2)}
        assert all(ref["lam"][nS, j, b] == 1 for j in range(len(lam[0]))) and all(v == lamT[nS, b] for v in ref["lam2"][nS, :, b])
        worst = {k: max(worst[k], got[k]) for k in worst}
    return worst


def _twin_err(oracle, family, regime):
    """the twin's error against mpmath on the reduced shapes of a regime (maximum over them), and the oracle's on the same inputs"""
    key = (family, regime)
    if key not in _TWIN_ERR:
        worst, orc_err = {k: 0.0 for k in tw.OUTPUTS}, []
        if family == "logistic":
            for nS in (1, 2, 4):
                par, tspan, x0, u, lamT = cs.logistic_regime(regime, nS, 24, batch=3)
                e = _twin_error_against_mpmath(_mp_logistic(par), tw.LogisticK(par["m"], par["c"], par["r"]), tspan, x0, u, lamT)
                worst = {k: max(worst[k], e[k]) for k in worst}
                po = oracle.LogisticProblem(par["m"], par["c"], par["r"], [[0.0, 1.0]])
                ref = tw.passes(tw.LogisticK(par["m"], par["c"], par["r"]), tspan, x0, u, lamT)
                orc_err.append(tw.errors(cs.oracle_passes(oracle, po, tspan, x0, u, lamT), ref))
        else:
            par, tspan, x0, u, lamT = cs.lq_regime(regime, 5, 2, N=16, batch=2)
            prob = tw.LQ(par["A"], par["Bu"], par["q"], par["rdiag"], par["r"])
            worst = _twin_error_against_mpmath(_mp_lq(par), prob, tspan, x0, u, lamT)
            po = oracle.LQProblem(par["A"], par["Bu"], par["q"], par["rdiag"], par["r"], [[-1.0, 1.0]] * 2)
            orc_err.append(tw.errors(cs.oracle_passes(oracle, po, tspan, x0, u, lamT), tw.passes(prob, tspan, x0, u, lamT)))
        _TWIN_ERR[key] = (worst, orc_err)
    return _TWIN_ERR[key]


ALL_REGIMES = [("logistic", r) for r in cs.LOGISTIC_REGIMES] + [("lq", r) for r in cs.LQ_REGIMES]


@pytest.mark.parametrize("family,regime", ALL_REGIMES, ids=[f"{f}-{r}" for f, r in ALL_REGIMES])
def test_twin_against_mpmath(oracle, family, regime):
    """The twin's own error, by its own measure, against 50 digits: a few units of the long double's round-off (2^-64 = 5.4e-20)
    accumulated over the steps -- bounded here by 64 * 2^-64 = 3.5e-18 (a bound from the format and the step count of 24,
    not from a run), more than an order below fp64's 2^-53.  On the same reduced inputs the oracle's error is never exactly
    zero over a whole case."""
    worst, orc_err = _twin_err(oracle, family, regime)
    print("TWIN", family, regime, {k: f"{v:.1e}" for k, v in worst.items()})
    assert max(worst.values()) < 64 * 2.0 ** -64, worst
    for e in orc_err:
        for k, v in e.items():
            assert np.all(np.isfinite(v)) and np.max(v) > 0, (k, v)


def _full_shapes(family):
    if family == "logistic":
        return [(nS, N) for nS in (1, 2, 3, 4) for N in (72, 200)]
    return list(cs.LQ_SHAPES)


@pytest.mark.parametrize("family,regime", ALL_REGIMES, ids=[f"{f}-{r}" for f, r in ALL_REGIMES])
def test_oracle_against_twin_is_a_yardstick(oracle, family, regime):
    """The oracle against the twin on the full shapes of tests/test_gpu_rk4_accuracy.py: every error finite (printed per
    regime and shape: the table of NOTES.md) and at least 16 times the twin's error against mpmath in that regime
    (non-vacuity).  A regime that fails this has inputs that are too easy or too short: change the inputs, not the factor."""
    twin, _ = _twin_err(oracle, family, regime)
    for shape in _full_shapes(family):
        case = cs.logistic_case(oracle, regime, *shape) if family == "logistic" else cs.lq_case(oracle, regime, *shape)
        e = {k: float(np.max(v)) for k, v in case[-1].items()}
        print("ORACLE", family, regime, shape, " ".join(f"{k}={v:.1e}" for k, v in e.items()))
        for k, v in e.items():
            assert np.isfinite(v), (shape, k)
            assert v >= 16 * twin[k], (shape, k, v, twin[k])


def test_twin_takes_parameters_per_trajectory():
    """One batch with r (and c, m) per trajectory equals, bit for bit, the shared-parameter runs of its parts."""
    nS, N = 2, 24
    par, tspan, x0, u, lamT = cs.logistic_regime("C-r3", nS, N, batch=6)
    rs = np.array([0.05, 1.0, 3.0, 0.05, 1.0, 3.0])
    ms = np.array(par["m"])[:, None] * np.array([1.0, 1.0, 1.0, 0.9, 0.9, 0.9])[None, :]
    whole = tw.passes(tw.LogisticK(ms, par["c"], rs), tspan, x0, u, lamT)
    for b in range(6):
        one = tw.passes(tw.LogisticK(ms[:, b], par["c"], rs[b]), tspan, x0[:, b:b + 1], u[:, :, b:b + 1], lamT[:, b:b + 1])
        for k in tw.OUTPUTS:
            assert np.array_equal(whole[k][..., b], one[k][..., 0]), (b, k)
    parq, tspan, x0, u, lamT = cs.lq_regime("Lb", 5, 2, N=8, batch=4)
    rs, qs = np.array([0.05, 3.0, 0.05, 3.0]), parq["q"][:, None] * np.array([1.0, 1.0, 2.0, 2.0])[None, :]
    whole = tw.passes(tw.LQ(parq["A"], parq["Bu"], qs, parq["rdiag"], rs), tspan, x0, u, lamT)
    for b in range(4):
        one = tw.passes(tw.LQ(parq["A"], parq["Bu"], qs[:, b], parq["rdiag"], rs[b]), tspan, x0[:, b:b + 1], u[:, :, b:b + 1],
                        lamT[:, b:b + 1])
        for k in tw.OUTPUTS:
            assert np.array_equal(whole[k][..., b], one[k][..., 0]), (b, k)


def test_err_sees_what_relerr_cannot(oracle):
    """Why the measure exists: a relative perturbation of 1e-9 in ONE late dJdu entry of the strong-discount regime (r = 3,
    T = 8: the entry is of order 1e-12) is reported as about 1e-9 by err and as less than 1e-12 -- a pass -- by the parity
    tests' max |a - b| / max(1, |b|)."""
    par, tspan, x0, u, lamT, ref, orc, _ = cs.logistic_case(oracle, "C-r3", 2, 72)
    clean = np.asarray(ref["dJdu"], dtype=np.float64)
    col, b = 2 * 72 - 5, 17
    planted = clean.copy()
    planted[0, col, b] *= 1.0 + 1e-9
    assert abs(clean[0, col, b]) < 1e-9
    e = tw.err(planted, ref["dJdu"])
    window = np.max(np.abs(clean[0, col - tw.WINDOW:col + tw.WINDOW + 1, b]))
    expected = 1e-9 * abs(clean[0, col, b]) / window       # the entry against the largest of its +-4 neighbours
    assert 0.1e-9 < expected <= 1e-9
    assert abs(e[b] - expected) < 1e-3 * expected + 4 * tw.EPS
    assert np.max(np.delete(e, b)) < 4 * tw.EPS            # rounding the twin to fp64, nothing else
    assert tw.relerr_old(planted, clean) < 1e-12
