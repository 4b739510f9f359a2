"""The instances on which the bvp_solver's Newton iteration is pinned to its NumPy twin (tests/bvp_twin.py), shared by the
CPU checks of the twin (tests/test_bvp_twin.py: every case is shown to be able to tell a right step from a wrong one) and
the GPU tests (tests/test_gpu_bvp_iteration.py: the device takes the twin's steps).  No test module: nothing is collected here.

The one-step bound.  The device and the twin evaluate the same expressions in another order and with contracted
multiply-adds; the forward-difference quotient of optSys divides such last-bit differences by sqrt(eps) max(1, |y|).
bvp_twin.step_noise measures what ONE last-bit change of the step's input does to the twin's own step; the device differs
in roughly three evaluations of optSys per quotient, at every node, so the bound allows MARGIN of those plus four units in
the last place of y:   |y_device - y_twin| <= MARGIN step_noise + 4 eps max(1, |y|)   per instance and step.
MARGIN began at 16 and holds on all steps but three first steps from the constant guess (measured 7.6, 9.8 and 61 on the
MI355X, every other step below 3), where step_noise under-samples the twin's sensitivity: the twin answers random +-1-ulp
changes of those starts with 7 to 16 step_noise (NOTES.md).  128 covers the measured 61; the wrong Newton matrices of
tests/test_bvp_twin.py stay at least 1.6e3 bounds away (100 is asked), so the margin is not raised further."""
import numpy as np

from tests import bvp_twin as bt

EPS = float(np.finfo(np.float64).eps)
TOL = 1e-10                                                           # NewtonTol (the default)
MARGIN = 128.0
BOUNDS = [[0.0, 1.0]]
BL3 = {"c": 1.5, "m": 3.0, "r": 0.05}
LOGISTIC_M = [3.0, 2.5, 2.0, 2.8]
NONUNIFORM = 10.0 * np.linspace(0.0, 1.0, 38) ** 1.3                  # N = 37: no multiple of the interval chunk (8)
EDGE_GRID = 10.0 * np.linspace(0.0, 1.0, 18) ** 1.3                   # its first N + 1 points: the grids of EDGE_N
EDGE_N = (1, 2, 7, 8, 9, 16, 17)                                      # below one chunk, one and two chunks exactly, one over


def wavy_guess(x0, tspan):
    """A start with nothing round in it.  From the constant guess [x0; 0] the first step computes with lam = 0 and the same
    few values at every node: on a grid of a few intervals step_noise then samples next to no rounding at all (it comes out
    at 0 to 1e-16 of the step, where 1e-9 to 1e-8 is the rule) and says nothing about the step's sensitivity."""
    x0, t = np.asarray(x0, dtype=np.float64)[:, None], np.asarray(tspan)[None, :]
    k = np.arange(x0.size)[:, None]
    return np.vstack([x0 * (1 + 0.05 * np.sin(3 * t + k)), 0.3 * (1.0 - t / t[0, -1]) + 0.02 * np.cos(2 * t + k)])


class Case:
    """One instance: the BL-3 problem (kind "bl3": c and the control's upper bound may be the instance's own) or the
    logistic family (kind "logistic", nS = len(x0)) from x0 on tspan, started from the constant guess or, with `wavy`, from
    wavy_guess.  `steps`: how many iterations of the twin's trace the one-step test takes (None: all of them)."""

    def __init__(self, family, kind, x0, tspan, c=1.5, ub=1.0, steps=None, wavy=False):
        self.family, self.kind, self.x0, self.tspan, self.c, self.ub, self.steps = family, kind, list(x0), tspan, c, ub, steps
        self.nS = len(self.x0)
        self.y0 = wavy_guess(self.x0, tspan) if wavy else None
        self.name = f"{family}: {kind} x0 {self.x0} c {c} ub {ub} N {len(tspan) - 1}" + (" wavy guess" if wavy else "")
        self.memo = {}

    def group(self):
        """Instances of one group run in one device call (same kernels, same grid)."""
        return (self.family, self.kind, self.nS, len(self.tspan))

    def problem(self, oracle):
        if self.kind == "bl3":
            return oracle.TestOCProblem(dict(BL3, c=self.c), [[0.0, self.ub]])
        return oracle.LogisticProblem(LOGISTIC_M[:self.nS], self.c, 0.05, [[0.0, self.ub]])

    def solve(self, oracle, **options):
        """The twin's solve with its trace, once per set of options; do not write into the result."""
        key = tuple(sorted(options.items()))
        if key not in self.memo:
            self.memo[key] = bt.solve(self.problem(oracle), self.x0, self.tspan, y0=self.y0, trace=True, **options)
        return self.memo[key]

    def step_records(self, oracle, **options):
        """The steps the one-step test takes: for iteration k of the twin's trace the start y_{k-1}, the twin's y_k, alpha_k,
        ||Phi(y_k)||_inf, the verdict of a solve that may take this one iteration only, and step_noise at y_{k-1}."""
        key = ("records",) + tuple(sorted(options.items()))
        if key not in self.memo:
            tw, prob = self.solve(oracle, **options), self.problem(oracle)
            out, prev = [], tw["start"]["y"]
            for k, s in enumerate(tw["trace"][:self.steps], 1):
                out.append({"k": k, "from": prev, "y": s["y"], "alpha": s["alpha"], "resinf": s["resinf"],
                            "converged": s["alpha"] > 0 and s["resinf"] <= TOL,
                            "noise": bt.step_noise(prob, self.x0, self.tspan, prev, **options)})
                prev = s["y"]
            self.memo[key] = out
        return self.memo[key]


def step_bound(noise, y, margin=MARGIN):
    return margin * noise + 4 * EPS * np.maximum(1.0, np.abs(y))


def eligible_for_counts(trace):
    """No iterate's ||Phi||_inf within a factor 30 of NewtonTol, on either side: the device, whose residual differs from
    the twin's by rounding, then stops at the same iteration."""
    return all(not (TOL / 30 <= s["resinf"] <= 30 * TOL) for s in trace)


# starts on the edge grids whose trace from wavy_guess keeps ||Phi||_inf away from NewtonTol (found with the twin)
EDGE_X0 = {1: ([2.15], [2.2], [2.35, 2.15, 2.0], [2.49, 2.15, 2.16]), 2: ([2.0], [2.05], [2.04, 2.12, 2.4], [2.29, 2.05, 2.22]),
           7: ([2.35], [2.4], [2.04, 2.12, 2.4], [2.29, 2.05, 2.22]), 8: ([2.05], [2.1], [2.04, 2.12, 2.4], [2.29, 2.05, 2.22]),
           9: ([2.05], [2.1], [2.04, 2.12, 2.4], [2.29, 2.05, 2.22]), 16: ([2.05], [2.1], [2.29, 2.05, 2.22], [2.24, 2.08, 2.37]),
           17: ([2.05], [2.1], [2.29, 2.05, 2.22], [2.24, 2.08, 2.37])}


def _edge_cases():
    return [Case(f"edge grid N = {N}", "bl3" if len(x0) == 1 else "logistic", x0, EDGE_GRID[:N + 1], steps=1, wavy=True)
            for N in EDGE_N for x0 in EDGE_X0[N]]


# the damped instances (found with the twin; tests/test_bvp_twin.py asserts their step lengths): BL-3 on NONUNIFORM from the
# constant guess takes alpha = 1/4, 1/2 from x0 = 1.8 (first stage of the device's line search: trials 1, 1/2, 1/4) and
# 1/4, 1/16 from x0 = 1.75, 1/4, 1/16, 1/8, 1/32, 1/2 from x0 = 1.6 (second stage)
DAMPED_ALPHAS = {1.8: [0.25, 0.5, 1.0, 1.0, 1.0, 1.0], 1.75: [0.25, 0.0625, 1.0, 1.0, 1.0, 1.0, 1.0],
                 1.6: [0.25, 0.0625, 0.125, 0.03125, 0.5, 1.0, 1.0, 1.0, 1.0]}
DAMPED = [Case("damped", "bl3", [x0], NONUNIFORM) for x0 in DAMPED_ALPHAS]
FULL = [Case("BL-3", "bl3", [x0], NONUNIFORM) for x0 in (2.0, 2.5)]
NOT_CONVERGING = Case("BL-3", "bl3", [0.5], NONUNIFORM)               # (no step case: its line searches end in failure)
LOGISTIC = [Case("logistic", "logistic", x0, NONUNIFORM) for x0 in
            ([2.39, 2.22], [2.43, 2.35], [2.38, 2.13, 2.21], [2.23, 2.48, 2.45], [2.34, 2.31, 2.48, 2.21], [2.08, 2.43, 2.08, 2.17])]
PER_TRAJECTORY = [Case("per-trajectory c and bounds", "bl3", [x0], NONUNIFORM, c=c, ub=ub)
                  for c, ub, x0 in ((1.5, 0.3, 2.0), (1.7, 0.3, 2.3), (1.9, 0.5, 2.5), (1.7, 1.0, 2.1), (1.9, 0.5, 2.3))]
EDGE = _edge_cases()
STEP_CASES = FULL + LOGISTIC + PER_TRAJECTORY + DAMPED + EDGE
# whole solves whose iteration count is compared with the twin's (each is shown eligible on the CPU)
COUNT_CASES = FULL + LOGISTIC + DAMPED
# tests/symbolic_test2.m's problem and grid for the count test only (its mutant gaps are 1e-5: no step case); the script's own
# x0 = .1 passes ||Phi||_inf = 1.7e-9 and x0 = .2 ends at 3.0e-11, within the factor 30 of NewtonTol, so neighbours stand in
SYMBOLIC_TEST2 = {"par": {"c": 4.0, "m": 0.5, "r": 0.0}, "T": 5.0, "N": 200, "x0": [0.15, 0.3, 0.35, 0.45]}
