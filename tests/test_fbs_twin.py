"""CPU tests that pin the instrument of tests/test_gpu_fbs_accuracy.py: the extended-precision twin of the sweep
(tests/fbs_twin.py) against mpmath at 50 digits (its pchip: everything else is rk4_twin's arithmetic, pinned in
tests/test_rk4_twin.py, or a clamp and a quotient) and against the oracle's compute_x_lam and fb_sweep, and the non-vacuity of
every case of tests/fbs_accuracy_cases.py for the oracle alone."""
import numpy as np
import pytest
from mpmath import mp   # (comes with sympy, which tests/test_symbolic.py needs already)

from tests import fbs_accuracy_cases as fc
from tests import fbs_twin as ft
from tests import rk4_accuracy_cases as rc
from tests import rk4_twin as tw
from tests.test_rk4_twin import DPS, _mpl

L = np.longdouble


def _mp_sgn(v):
    return (v > 0) - (v < 0)


def _mp_pchip_slopes(x, y):
    """MATLAB's pchip slopes (the piece oracle/ocs_oracle.c ocs_or_pchip_slopes restates), scalar, on lists of mpf"""
    n = len(x)
    h = [x[i + 1] - x[i] for i in range(n - 1)]
    dl = [(y[i + 1] - y[i]) / h[i] for i in range(n - 1)]
    if n == 2:
        return [dl[0], dl[0]]
    d = [mp.mpf(0)] * n
    for k in range(n - 2):
        if _mp_sgn(dl[k]) * _mp_sgn(dl[k + 1]) > 0:
            hs = h[k] + h[k + 1]
            w1, w2 = (h[k] + hs) / (3 * hs), (hs + h[k + 1]) / (3 * hs)
            dmax, dmin = max(abs(dl[k]), abs(dl[k + 1])), min(abs(dl[k]), abs(dl[k + 1]))
            d[k + 1] = dmin / (w1 * (dl[k] / dmax) + w2 * (dl[k + 1] / dmax))

    def end(ha, hb, da, db):
        e = ((2 * ha + hb) * da - ha * db) / (ha + hb)
        if _mp_sgn(e) != _mp_sgn(da):
            return mp.mpf(0)
        if _mp_sgn(da) != _mp_sgn(db) and abs(e) > abs(3 * da):
            return 3 * da
        return e
    d[0], d[n - 1] = end(h[0], h[1], dl[0], dl[1]), end(h[n - 2], h[n - 3], dl[n - 2], dl[n - 3])
    return d


def _mp_pchip_eval(x, y, q):
    n, d = len(x), _mp_pchip_slopes(x, y)
    out = []
    for t in q:
        k = 0 if t <= x[0] else (n - 2 if t >= x[n - 1] else max(i for i in range(n - 1) if x[i] <= t))
        h = x[k + 1] - x[k]
        dl = (y[k + 1] - y[k]) / h
        a, b = (dl - d[k]) / h, (d[k + 1] - dl) / h
        s = t - x[k]
        out.append(y[k] + s * (d[k] + s * ((2 * a - b) + s * ((b - a) / h))))
    return out


_RNG = np.random.default_rng(20261021)
_NONUNIFORM = np.concatenate([[0.0], np.sort(_RNG.uniform(0.0, 3.0, 9)), [3.0]])
PCHIP_CASES = {
    "nonuniform-monotone": (_NONUNIFORM, np.cumsum(_RNG.uniform(0.1, 2.0, 11))),
    "secant-sign-change": (_NONUNIFORM, np.sin(2.5 * _NONUNIFORM) * np.exp(-_NONUNIFORM)),
    "flat-piece": (_NONUNIFORM, np.array([0.0, 0.3, 0.9, 0.9, 0.9, 1.4, 1.1, 1.1, 0.2, -0.5, -0.5])),
    "end-clamps": (np.array([0.0, 0.1, 1.0, 1.2, 2.0]), np.array([1.0, 0.0, 0.05, 3.0, 2.9])),
    "n2": (np.array([0.25, 1.75]), np.array([1.0e-9, -3.0])),
    "n3": (np.array([0.0, 0.4, 1.0]), np.array([2.0, 1.0, 1.5])),
}


@pytest.mark.parametrize("name", sorted(PCHIP_CASES))
def test_pchip_against_mpmath(name):
    """Midpoints and point evaluation (on nodes, between them, at both ends) against the scalar restatement at 50 digits: a
    few units of the long double's round-off, 16 * 2^-64 relative to the largest node value (the Hermite form divides three
    times by h and sums four terms; a bound from the format, not from a run).  The flat pieces must come out exactly flat."""
    x, y = PCHIP_CASES[name]
    ys = np.stack([y, -0.5 * y[::-1]])[:, :, None]                 # two rows, one trajectory
    q = np.concatenate([x, (x[:-1] + x[1:]) / 2, x[0] + (x[-1] - x[0]) * _RNG.uniform(0, 1, 23)])
    got = ft.pchip_eval(x, ys, q)
    t, _ = tw.grid(x)
    mid = ft.pchip_mid(x, ys)
    with mp.workdps(DPS):
        xm, qm, tm = [mp.mpf(float(v)) for v in x], [mp.mpf(float(v)) for v in q], [mp.mpf(float(v)) for v in t[1::2]]
        for row in range(2):
            ym = [mp.mpf(float(v)) for v in ys[row, :, 0]]
            scale = max(abs(v) for v in ym)
            for ref, val in ((_mp_pchip_eval(xm, ym, qm), got[row, :, 0]), (_mp_pchip_eval(xm, ym, tm), mid[row, :, 0])):
                worst = max(abs(_mpl(v) - r) for v, r in zip(val, ref)) / scale
                assert worst < 16 * 2.0 ** -64, (name, row, float(worst))
    if name == "flat-piece":
        assert np.all(mid[0, 2:4, 0] == L(0.9)) and mid[0, 6, 0] == L(1.1) and mid[0, 9, 0] == L(-0.5)
        assert np.all(ft.pchip_slopes(x, ys)[0, 2:5, 0] == 0)
    if name == "n2":
        assert np.all(ft.pchip_slopes(x, ys)[:, 0] == ft.pchip_slopes(x, ys)[:, 1])


def test_pchip_slopes_equal_the_oracles(oracle):
    """the slope rule, every branch, against oracle.pchip_slopes to fp64 round-off"""
    for name, (x, y) in PCHIP_CASES.items():
        d = ft.pchip_slopes(x, y[None, :, None])[0, :, 0].astype(np.float64)
        do = oracle.pchip_slopes(x, y)
        assert np.max(np.abs(d - do)) <= 1e-14 * max(1.0, np.max(np.abs(do))), name
        assert np.array_equal(d == 0, do == 0), name


X_LAM_KEYS = ([("logistic", r, nS, N, b, "own") for r in fc.LOGISTIC_REGIMES for nS, N, b in fc.LOGISTIC_SHAPES] +
              [("lq", r, s, rc.LQ_N, rc.LQ_BATCH, "own") for r in fc.LQ_REGIMES for s in fc.LQ_MC_SHAPES + (fc.LQ_LANE_SHAPE,)])


@pytest.mark.parametrize("key", X_LAM_KEYS, ids=lambda k: "-".join(map(str, k)).replace(" ", ""))
def test_compute_x_lam_against_oracle(oracle, key):
    """twin and oracle agree to 1e-12 by the parity tests' measure on every case of test_compute_x_lam_error"""
    *_, ref, orc, e = fc.x_lam_case(oracle, *key)
    for k in ("x", "lam", "J"):
        assert tw.relerr_old(orc[k], np.asarray(ref[k], dtype=np.float64)) < 1e-12, k
        assert np.all(np.isfinite(e[k])) and np.max(e[k]) > 0, k


def _inside(u, bounds):
    """fraction of the grid nodes on which every control is strictly inside its bounds, per trajectory"""
    b = np.asarray(bounds, dtype=np.float64)
    u = np.asarray(u, dtype=np.float64)[:, 0::2]
    return np.all((u > b[:, 0][:, None, None]) & (u < b[:, 1][:, None, None]), axis=0).mean(axis=0)


@pytest.mark.parametrize("key", fc.sweep_keys(), ids=lambda k: "-".join(map(str, k)).replace(" ", ""))
def test_sweeps_against_oracle_and_non_vacuity(oracle, key):
    """Every case of test_sweep_error, every k it runs:
    * twin and oracle agree to 1e-12 by the parity tests' measure (maxChange relative to its value);
    * no instance converges: the oracle's fb_sweep returns 0 and its maxChange[j] > 2 for every j < k;
    * discounted regimes: min |lam| over the entries with lam != 0 is below 1e-8 max |lam|;
    * growth regime: x (m - x) - u > 0 at every stage state of every sweep;
    * the control that sweeps 2 and 3 integrate (what sweeps 1 and 2 leave on the grid) is strictly inside its bounds on
      at least a quarter of the nodes of every trajectory."""
    family, regime, shape, N, batch, grid, kmax, nE = key
    for k in range(1, kmax + 1):
        par, tspan, x0, ref, orc, e = fc.sweep_case(oracle, family, regime, shape, N, batch, grid, k, nE)
        for name in ("x", "lam", "J"):
            assert tw.relerr_old(orc[name], np.asarray(ref[name], dtype=np.float64)) < 1e-12, (k, name)
        for n, u in ref["u"].items():
            assert tw.relerr_old(orc["u"][n], np.asarray(u, dtype=np.float64)) < 1e-12, (k, n)
        print("ORACLE", key, "k", k, " ".join(
            f"{a}={np.max(max(v.values(), key=np.max) if isinstance(v, dict) else v):.1e}" for a, v in e.items()))
        assert np.all(orc["sweeps"] == 0) and np.all(orc["maxChange"] > 2), (k, float(np.min(orc["maxChange"])))
        # (once the change is a difference of nearly equal controls its relative error is that difference's: 1e-7 at most here)
        assert np.max(fc.err_max_change(orc["maxChange"], ref["maxChange"])) < 1e-6
        lam = np.abs(np.asarray(ref["lam"], dtype=np.float64))
        if regime in fc.DISCOUNTED:
            assert np.min(lam[lam > 0]) < 1e-8 * np.max(lam), k
        if regime == "B":
            rc.assert_growing(par, ref, np.asarray(ref["ugrid_in"]))
        if k < kmax or kmax == 1:
            frac = _inside(ref["ugrid"], fc.bounds_of(family, par))
            assert np.min(frac) >= 0.25, (k, float(np.min(frac)))
