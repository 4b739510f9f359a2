"""Regimes, shapes and shared references of the sweep's accuracy tests (tests/test_fbs_twin.py on the CPU,
tests/test_gpu_fbs_accuracy.py on the GPU): where compute_x_lam_J and fb_sweep are run to measure their rounding error against
tests/fbs_twin.py.  The regimes are those of tests/rk4_accuracy_cases.py (its x0, its benign controls for compute_x_lam, its
grids), with what the sweep needs changed and written down here:

    grids     "own" is the regime's grid (A: random non-uniform, B: uniform, C: jittered by up to 0.35 h, D: uniform);
              "uniform" is linspace(0, T, N + 1) on the same horizon.  The error points are linspace(T0, TF, nERROR_PTS)
              (fb_sweep.m:69), so they lie on the nodes -- the condition of the sweep loops 4 and 2 -- on a uniform grid only:
              loops 4 and 2 run on "uniform", loops 1 and 5 on "own" (C's jittered grid is the non-uniform one of the sweep).
    B         c = 2e7 instead of 1.5.  The costate of a growing state grows backwards like e^{m t} to ~1e4 at t = 0; with
              c = 1.5 ControlChar = sum(lam) e^{rt} / (2c) is clamped to 1 there, the second sweep harvests a state of 1e-3 at
              rate 1 and the regime leaves the growth it is named for (x (m - x) - u < 0: the blow-up that
              test_blow_up_trajectories_agree owns).  With c = 2e7 the control of every sweep stays below x (m - x) and
              strictly inside (0, 1) (asserted: assert_growing on the twin's stage states of every sweep).
              At N = 13 the horizon is 3 instead of 6: a step of 6/13 overshoots the saturated state.
    A, C      c = 40 instead of 1.5: with c = 1.5 the control of sweep 2 sits on its upper bound 1 on most of the horizon (a
              clamped control tests nothing) and, being above the largest sustainable yield m^2 / 4 of the rows with m <= 2,
              sends their states through zero.  With c = 40 it is strictly inside (0, 1) on more than 9 nodes in 10.
    tols      uRelTol = uAbsTol = 1e-10 (1e-16 in B, whose control is of order 1e-5) instead of 1e-7: the sweep contracts fast
              at these cost weights and the one-state instances would converge in sweep 3.
    D-r3      rdiag 20 times the regime's (else the control is clamped on 3 nodes in 4), and time rescaled: A -> s A,
              tspan -> tspan / s with s = T / 8, so h max|eig A| = 2.5 as before and T = 8:
              e^{-rT} = 4e-11.  On the pass pair's horizon (T = 0.24 at N = 96) r = 3 discounts by e^{-0.72}: nothing falls.
    options   u0 = lower bound (fb_sweep.m:23), bounds [0, 1] (logistic), [-1, 1] (LQ).

No instance converges within the k <= 3 sweeps of a test (tests/test_fbs_twin.py asserts the oracle's maxChange > 2 on every
instance and sweep), so the sweep takes no discrete decision inside a test."""
import numpy as np

from tests import fbs_twin as ft
from tests import rk4_accuracy_cases as rc
from tests import rk4_twin as tw

L = np.longdouble
LOGISTIC_BOUNDS = [[0.0, 1.0]]
B_COST = 2.0e7
AC_COST = 40.0
D3_R_SCALE = 20.0


def tolerances(regime):
    """(uRelTol, uAbsTol) of a regime (module docstring)"""
    return (1e-16, 1e-16) if regime == "B" else (1e-10, 1e-10)


N_OFF_NODES = 41            # nERROR_PTS of the loop-5 runs: off the nodes of every grid here
N_INTERP_OFF = 37           # nINTERP_PTS off the nodes (the other parametrisation is 2N + 1: nodes and middles)
LOGISTIC_REGIMES = ("A", "B", "C-r0.05", "C-r3")
LQ_REGIMES = ("D-r0.05", "D-r3")
DISCOUNTED = ("C-r3", "D-r3")                                   # min |lam| < 1e-8 max |lam| (tests/test_fbs_twin.py)
# (nS, N, batch): the wave-specialised kernels on a whole tile and a ragged even one (70 = 64 + 6, 2 * 32 + 6, 4 * 16 + 6); on
# whole tiles alone (64); the lane kernels k_costate + k_pchip_mid (N % 8 != 0; batch 69 is odd as well, which keeps the state
# pass on the lane kernel too: tile_ok)
LOGISTIC_SHAPES = [(nS, 72, 70) for nS in (1, 2, 4)] + [(nS, 72, 64) for nS in (1, 2, 4)] + [(nS, 13, 69) for nS in (1, 2, 4)]
SCAN_LIMIT_WG = 128         # costate_scan_ok (csrc/ocs_scan_kernels.hip): batch / (64 / nS) <= 128 workgroups
BIG_N = 16
LQ_MC_SHAPES = ((12, 2), (32, 4))
LQ_LANE_SHAPE = (5, 2)


def big_batch(nS):
    """one batch beyond the scan's limit: 129 tiles and two instances (ragged, even)"""
    return (SCAN_LIMIT_WG + 1) * 64 // nS + 2


def tile_ok(batch, tile):
    """csrc/ocs_internal.hpp: whole tiles, or at least one tile and an even batch (the ragged tile overlaps its neighbour)"""
    return batch % tile == 0 or (batch > tile and batch % 2 == 0)


def linspace(a, b, n):
    """MATLAB's linspace in fp64 (oracle/ocs_oracle.c ocs_or_linspace, sweep.matlab_linspace): data of every implementation"""
    y = a + (np.arange(n, dtype=np.float64) * (b - a)) / (n - 1)
    y[0], y[-1] = a, b
    return y


def logistic_inputs(name, nS, N, batch, grid):
    """(params, tspan, x0, u): rk4_accuracy_cases.logistic_regime with the changes of the module docstring"""
    par, tspan, x0, u, _ = rc.logistic_regime(name, nS, N, max(batch, rc.LOGISTIC_BATCH))   # (64, 69 and 70: the same draws)
    x0, u = x0[:, :batch], np.asfortranarray(u[:, :, :batch])
    par = dict(par, c=B_COST if name == "B" else AC_COST)
    if name == "B" and N < 72:
        tspan = tspan * 0.5
    if grid == "uniform":
        tspan = linspace(0.0, tspan[-1], N + 1)
        if name != "B":    # the benign controls are a function of t: sampled on the new grid (B's grid is uniform already)
            u = np.asfortranarray(rc._benign_controls(np.random.default_rng(rc._seed(name + "u", nS, N)), tspan, batch))
    else:
        assert grid == "own"
    return par, tspan, x0, u


def lq_inputs(name, nS, nC, N=rc.LQ_N, batch=rc.LQ_BATCH):
    par, tspan, x0, u, _ = rc.lq_regime(name, nS, nC, N, batch)
    tspan = linspace(0.0, tspan[-1], N + 1)    # (h * arange differs from it in the last bit of some nodes)
    if name == "D-r3":
        s = tspan[-1] / 8.0
        par, tspan = dict(par, A=par["A"] * s, rdiag=par["rdiag"] * D3_R_SCALE), linspace(0.0, 8.0, N + 1)
    return par, tspan, x0, u


def twin_problem(family, par):
    if family == "logistic":
        return tw.LogisticK(par["m"], par["c"], par["r"])
    return tw.LQ(par["A"], par["Bu"], par["q"], par["rdiag"], par["r"])


def oracle_problem(oracle, family, par, bounds):
    if family == "logistic":
        return oracle.LogisticProblem(par["m"], par["c"], par["r"], bounds)
    return oracle.LQProblem(par["A"], par["Bu"], par["q"], par["rdiag"], par["r"], bounds)


def bounds_of(family, par):
    return LOGISTIC_BOUNDS if family == "logistic" else [[-1.0, 1.0]] * np.atleast_2d(par["Bu"]).shape[1]


def inputs(family, regime, shape, N, batch, grid):
    if family == "logistic":
        return logistic_inputs(regime, shape, N, batch, grid)
    return lq_inputs(regime, *shape, N=N, batch=batch)


# ---- the oracle, trajectory by trajectory --------------------------------------------------------------------------------
def oracle_compute_x_lam(oracle, po, tspan, x0, u):
    go = oracle.RK4Integrator(tspan)
    xs, ls, Js = [], [], []
    for b in range(x0.shape[1]):
        x, lam, J = oracle.compute_x_lam(go, po, x0[:, b], u[:, :, b], want_J=True)
        xs.append(x), ls.append(lam), Js.append(J)
    return {"x": np.stack(xs, axis=-1), "lam": np.stack(ls, axis=-1), "J": np.array(Js)}


def oracle_sweeps(oracle, po, tspan, x0, k, nE, nIs, tol=(1e-7, 1e-7)):
    """The oracle's fb_sweep with nSWEEPS = k on every trajectory.  An instance that does not converge returns nothing but its
    maxChange history (fb_sweep.m:77), so x, J, lam of sweep k and ControlChar of them at the interpolation points are taken
    from the same functions the oracle's loop calls, in its order (ocs_or_fb_sweep: compute_x_lam, control_from_x_lam on the
    grid); maxChange is the loop's own, and `sweeps` its return value (0 = not converged)."""
    go = oracle.RK4Integrator(tspan)
    T0, TF = go.t[0], go.t[-1]
    opts = {"nSWEEPS": k, "nERROR_PTS": nE, "nINTERP_PTS": 2, "uRelTol": tol[0], "uAbsTol": tol[1]}
    out = {"x": [], "lam": [], "J": [], "maxChange": [], "sweeps": [], "u": {n: [] for n in nIs}}
    lb = po.ControlBounds[:, 0:1]
    for b in range(x0.shape[1]):
        r = oracle.fb_sweep(po, x0[:, b], tspan, opts)
        out["sweeps"].append(r["_sweeps"]), out["maxChange"].append(r["_maxChange"])
        u = lb @ np.ones((1, go.t.size))
        for _ in range(k):
            x, lam, J = oracle.compute_x_lam(go, po, x0[:, b], u, want_J=True)
            u = oracle.control_from_x_lam(go, po, x, lam, go.t)
        out["x"].append(x), out["lam"].append(lam), out["J"].append(J)
        for n in nIs:
            out["u"][n].append(oracle.control_from_x_lam(go, po, x, lam, oracle.linspace(T0, TF, n)))
    return {"x": np.stack(out["x"], axis=-1), "lam": np.stack(out["lam"], axis=-1), "J": np.array(out["J"]),
            "maxChange": np.stack(out["maxChange"], axis=-1), "sweeps": np.array(out["sweeps"]),
            "u": {n: np.stack(v, axis=-1) for n, v in out["u"].items()}}


# ---- the error measure: rk4_twin's, with two entries more ------------------------------------------------------------------
def err_max_change(mc, ref):
    """|maxChange - ref| / |ref| per sweep, the largest over the sweeps -> [B]"""
    return np.max(np.stack([tw.err_J(mc[j], ref[j]) for j in range(ref.shape[0])]), axis=0)


def errors(got, ref, nI=None):
    """err per output and trajectory.  x, lam (and cost, where `got` has the row) by rk4_twin.err, J by err_J; u by err on its
    own local scale, like lam; maxChange relative to the twin's value."""
    out = {"x": tw.err(got["x"], ref["x"]), "J": tw.err_J(got["J"], ref["J"]), "lam": tw.err(got["lam"], ref["lam"])}
    if "cost" in got:
        out["cost"] = tw.err(got["cost"], ref["cost"])
    if "u" in got:
        out["u"] = tw.err(got["u"][nI] if isinstance(got["u"], dict) else got["u"], ref["u"][nI])
        out["maxChange"] = err_max_change(got["maxChange"], ref["maxChange"])
    return out


_CASES = {}   # computed once per key, shared by the tests that need it, never written again


def x_lam_case(oracle, family, regime, shape, N, batch, grid="own"):
    """compute_x_lam_J on the regime's controls: (par, tspan, x0, u, ref, orc, err_oracle)"""
    key = ("xlam", family, regime, shape, N, batch, grid)
    if key not in _CASES:
        par, tspan, x0, u = inputs(family, regime, shape, N, batch, grid)
        x, cost, J, lam = ft.compute_x_lam(twin_problem(family, par), tspan, x0, u)
        ref = {"x": x, "cost": cost, "J": J, "lam": lam}
        orc = oracle_compute_x_lam(oracle, oracle_problem(oracle, family, par, bounds_of(family, par)), tspan, x0, u)
        _CASES[key] = (par, tspan, x0, u, ref, orc, errors(orc, ref))
    return _CASES[key]


def sweep_case(oracle, family, regime, shape, N, batch, grid, k, nE):
    """k sweeps with nERROR_PTS = nE: (par, tspan, x0, ref, orc, err_oracle); ref["u"], orc["u"] and err_oracle["u"] are dicts
    over nINTERP_PTS in (2N + 1, 37)."""
    key = ("sweep", family, regime, shape, N, batch, grid, k, nE)
    if key not in _CASES:
        par, tspan, x0, _ = inputs(family, regime, shape, N, batch, grid)
        nIs = (2 * N + 1, N_INTERP_OFF)
        bounds = bounds_of(family, par)
        T0, TF = tspan[0], tspan[-1]
        pts = np.concatenate([linspace(T0, TF, n) for n in nIs])
        tol = tolerances(regime)
        ref = ft.sweeps(twin_problem(family, par), tspan, x0, k, linspace(T0, TF, nE), pts, bounds, *tol)
        ref["u"] = {nIs[0]: ref["u"][:, :nIs[0]], nIs[1]: ref["u"][:, nIs[0]:]}
        orc = oracle_sweeps(oracle, oracle_problem(oracle, family, par, bounds), tspan, x0, k, nE, nIs, tol)
        e = errors({k_: v for k_, v in orc.items() if k_ != "u"}, ref)
        e["u"] = {n: tw.err(orc["u"][n], ref["u"][n]) for n in nIs}
        e["maxChange"] = err_max_change(orc["maxChange"], ref["maxChange"])
        _CASES[key] = (par, tspan, x0, ref, orc, e)
    return _CASES[key]


# every (family, regime, shape, N, batch, grid, kmax, nE) the GPU test runs; the CPU test proves each non-vacuous
def sweep_keys():
    keys = []
    for regime in LOGISTIC_REGIMES:
        for nS, N, batch in LOGISTIC_SHAPES:
            kmax = 3 if N == 72 else 2
            keys.append(("logistic", regime, nS, N, batch, "uniform", kmax, N + 1))
            keys.append(("logistic", regime, nS, N, batch, "own", kmax, N + 1))
            keys.append(("logistic", regime, nS, N, batch, "own", kmax, N_OFF_NODES))
    for nS in (1, 2, 4):
        keys.append(("logistic", "C-r3", nS, BIG_N, big_batch(nS), "uniform", 2, BIG_N + 1))
    for regime in LQ_REGIMES:
        for shape in LQ_MC_SHAPES + (LQ_LANE_SHAPE,):
            kmax = 3 if shape == (12, 2) else 2
            keys.append(("lq", regime, shape, rc.LQ_N, rc.LQ_BATCH, "own", kmax, rc.LQ_N + 1))
            keys.append(("lq", regime, shape, rc.LQ_N, rc.LQ_BATCH, "own", kmax, N_OFF_NODES))
    return sorted(set(keys), key=str)
