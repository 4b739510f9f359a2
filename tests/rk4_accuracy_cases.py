"""Regimes, shapes and shared references of the accuracy tests (tests/test_rk4_twin.py on the CPU, tests/test_gpu_rk4_accuracy.py
on the GPU): where the RK4 pass pair is run to measure its rounding error against tests/rk4_twin.py.

Each regime is a function returning (problem parameters, tspan, x0, u, lamT) from a fixed seed:

    A    benign (the parity tests' inputs): x0 in [0.8, 2.5], u in [0.05, 0.45], r = 0.05, T = 0.03 N, non-uniform grid
    B    growth, then saturation: x0 in [1e-3, 1e-2], u in [0, 1e-4] falling over time, m = [3, 2.5, 2, 1.5], T = 6, uniform
         grid; Bn: the same on a non-uniform grid.  x (m - x) - u stays positive (asserted on the twin's stage states)
    C    strong discount: A's states and controls on T = 8, r one of 0.05, 1, 3 (lam and dJdu fall through ten orders)
    D    LQ, stiff and near the stability limit: A = -diag(logspace(0, 3, nS)) + 0.1 randn, h max|eig A| = 2.5, r 0.05 or 3
    Lb   LQ, benign: lq_matrices on a non-uniform grid over [0, 1.5], r = 0.05

One r per problem: r feeds the time-coefficient table of the registry problems and ocs_problem_set_batch_params refuses it
per trajectory (tests/test_gpu_batch_params.py::test_refusal_clear_and_mismatch pins that), so a regime with several r is
run once per value, every trajectory at every value.  The twin itself takes r per trajectory (tests/test_rk4_twin.py)."""
import numpy as np

from tests import rk4_twin as tw
from tests.user_problems import lq_matrices

M4 = [3.0, 2.5, 2.0, 1.5]
C_COST = 1.5
LOGISTIC_REGIMES = ("A", "B", "Bn", "C-r0.05", "C-r1", "C-r3")
LQ_REGIMES = ("D-r0.05", "D-r3", "Lb")
LOGISTIC_BATCH = 70      # lane / row-split / scan / auto take the first 69 (a whole tile of 64, 32 or 16 and a ragged one), the
                         # pipeline pair the first 64 (whole tiles only), the pipeline state pass all 70 (ragged, even)
LQ_SHAPES = ((12, 2), (32, 4))
LQ_N, LQ_BATCH = 96, 37


def _random_grid(rng, T, N):
    return np.concatenate([[0.0], np.sort(rng.uniform(0.0, T, N - 1)), [T]])


def _jittered_grid(rng, T, N):
    """nodes of the uniform grid moved by up to 0.35 h: steps between 0.3 h and 1.7 h"""
    tspan = np.linspace(0.0, T, N + 1)
    tspan[1:-1] += 0.35 * (T / N) * rng.uniform(-1.0, 1.0, N - 1)
    return tspan


def _seed(name, nS, N):
    return [sum(map(ord, name)), nS, N]


def _benign_controls(rng, tspan, batch):
    t, _ = tw.grid(tspan)
    f, ph = rng.uniform(0, 1, batch), rng.uniform(0, 2 * np.pi, batch)
    return (0.25 + 0.2 * np.sin(2 * np.pi * f[None, :] * t[:, None] + ph[None, :]))[None]


def logistic_regime(name, nS, N, batch=LOGISTIC_BATCH):
    """(params, tspan, x0, u, lamT); params = dict(m, c, r) of ocs.LogisticProblem / oracle.LogisticProblem / tw.LogisticK"""
    rng = np.random.default_rng(_seed(name, nS, N))
    m = M4[:nS]
    if name == "A":
        tspan, r = _random_grid(rng, 0.03 * N, N), 0.05
        u = _benign_controls(rng, tspan, batch)
        x0 = rng.uniform(0.8, 2.5, (nS, batch))
    elif name in ("B", "Bn"):
        T, r = 6.0, 0.05
        tspan = np.linspace(0.0, T, N + 1) if name == "B" else _jittered_grid(rng, T, N)
        t, _ = tw.grid(tspan)
        # falling in time: the equilibrium the state chases rises, so the state stays below it and keeps growing
        u = (1e-4 * rng.uniform(0.2, 1.0, batch)[None, :] * np.exp(-rng.uniform(0.1, 1.0, batch)[None, :] * t[:, None]))[None]
        x0 = rng.uniform(1e-3, 1e-2, (nS, batch))
    elif name.startswith("C-r"):
        tspan, r = _jittered_grid(rng, 8.0, N), float(name[3:])
        u = _benign_controls(rng, tspan, batch)
        x0 = rng.uniform(0.8, 2.5, (nS, batch))
    else:
        raise KeyError(name)
    lamT = rng.normal(size=(nS + 1, batch))
    return {"m": m, "c": C_COST, "r": r}, tspan, x0, np.asfortranarray(u), lamT


def lq_regime(name, nS, nC, N=LQ_N, batch=LQ_BATCH):
    """(params, tspan, x0, u, lamT); params = dict(A, Bu, q, rdiag, r)"""
    rng = np.random.default_rng(_seed(name, nS, N))
    if name.startswith("D-r"):
        # the matrix of test_bl5_full_size_properties (tests/test_gpu_lq.py) at this nS
        A = -np.diag(np.logspace(0, 3, nS)) + 0.1 * rng.normal(size=(nS, nS))
        Bu = rng.normal(size=(nS, nC))
        q, rdiag, r = rng.uniform(0.5, 1.5, nS), rng.uniform(1, 2, nC), float(name[3:])
        h = 2.5 / np.abs(np.linalg.eigvals(A)).max()
        tspan = h * np.arange(N + 1)
    elif name == "Lb":
        A, Bu, q, rdiag = lq_matrices(nS, nC)
        r, tspan = 0.05, _random_grid(rng, 1.5, N)
    else:
        raise KeyError(name)
    u = rng.uniform(-1, 1, (nC, 2 * N + 1, batch))
    x0 = rng.normal(size=(nS, batch))
    lamT = rng.normal(size=(nS + 1, batch))
    return {"A": A, "Bu": Bu, "q": q, "rdiag": rdiag, "r": r}, tspan, x0, u, lamT


def assert_growing(par, ref, u):
    """regime B: x (m - x) - u > 0 at every stage state of the twin -- the regime never drifts into the blow-up (harvest beyond
    the sustainable yield) that test_blow_up_trajectories_agree owns"""
    m = np.asarray(par["m"], dtype=np.longdouble)[:, None]
    for i, stages in enumerate(ref["xK"]):
        for y, col in zip(stages, (2 * i, 2 * i + 1, 2 * i + 1, 2 * i + 2)):
            x = y[:-1]
            assert np.all(x * (m - x) - u[0, col] > 0), ("regime B stopped growing at step", i)


def oracle_passes(oracle, po, tspan, x0, u, lamT):
    """The plain serial fp64 recursion (oracle/ocs_oracle.c) on every trajectory: the yardstick.  Host shapes."""
    go = oracle.RK4Integrator(tspan)
    out = {k: [] for k in ("x", "J", "lam", "dJdu", "lam2", "d2")}
    for b in range(x0.shape[1]):
        xo, Jo = go.compute_states(po, x0[:, b], u[:, :, b])
        lamo, do = go.compute_adjoints(po, u[:, :, b])
        l2, d2 = go.compute_adjoints(po, u[:, :, b], lamT[:, b])
        for k, v in zip(out, (xo, Jo, lamo, do, l2, d2)):
            out[k].append(v)
    return {k: (np.array(v) if k == "J" else np.stack(v, axis=-1)) for k, v in out.items()}


_CASES = {}   # computed once per (family, regime, shape), shared by the tests that need it, never written again


def logistic_case(oracle, name, nS, N):
    """inputs, the twin's passes and the oracle's error against it (per output and trajectory)"""
    key = ("logistic", name, nS, N)
    if key not in _CASES:
        par, tspan, x0, u, lamT = logistic_regime(name, nS, N)
        ref = tw.passes(tw.LogisticK(par["m"], par["c"], par["r"]), tspan, x0, u, lamT)
        if name in ("B", "Bn"):
            assert_growing(par, ref, u)
        po = oracle.LogisticProblem(par["m"], par["c"], par["r"], [[0.0, 1.0]])
        orc = oracle_passes(oracle, po, tspan, x0, u, lamT)
        _CASES[key] = (par, tspan, x0, u, lamT, ref, orc, tw.errors(orc, ref))
    return _CASES[key]


def lq_case(oracle, name, nS, nC):
    key = ("lq", name, nS, nC)
    if key not in _CASES:
        par, tspan, x0, u, lamT = lq_regime(name, nS, nC)
        ref = tw.passes(tw.LQ(par["A"], par["Bu"], par["q"], par["rdiag"], par["r"]), tspan, x0, u, lamT)
        po = oracle.LQProblem(par["A"], par["Bu"], par["q"], par["rdiag"], par["r"], [[-1.0, 1.0]] * nC)
        orc = oracle_passes(oracle, po, tspan, x0, u, lamT)
        _CASES[key] = (par, tspan, x0, u, lamT, ref, orc, tw.errors(orc, ref))
    return _CASES[key]
