"""GPU tests of the bvp_solver's Newton ITERATION (csrc/ocs_bvp_device.hpp, ocs_bvp_kernels.hip, ocs_bvp.cpp) against its
NumPy twin: tests/test_gpu_bvp_solver.py looks at the end of a solve, which a wrong Newton matrix reaches as well (a few
iterations later); here the device takes the twin's steps one at a time, needs the twin's number of them, follows the
twin's line search and treats an instance the same in any batch.

Bounds (tests/bvp_cases.py).  One step from the twin's iterate: MARGIN step_noise + 4 eps max(1, |y|), step_noise being the
twin's own answer to a last-bit change of that iterate; tests/test_bvp_twin.py shows for every case used here that three
wrong Newton matrices miss this bound by a factor > 1e3, that no ||Phi||_inf of its trace is within a factor 30 of
NewtonTol (so counts are not decided by rounding) and that no step starts on a kink of the control's clamp.
resnorm against the twin's residual of the device's y: RES_ULPS eps max(1, |y|, |optSys|) -- an entry of Phi is a sum of
about ten terms of that size, each behind some thirty roundings of optSys and one exp of either library."""
import numpy as np
import pytest

from tests import bvp_cases as bc
from tests import bvp_twin as bt
from tests.test_gpu_bvp_solver import Twins, check_instances, relerr

pytestmark = pytest.mark.gpu
TOL = bc.TOL
RES_ULPS = 64


@pytest.fixture(scope="module")
def ocs():
    import torch
    assert torch.cuda.is_available()
    import __graft_entry__ as g
    return g.load_package()


def device_problem(ocs, cases):
    """The device problem of a batch whose instance b is cases[b] (one kind and nS): c and the upper bound per trajectory
    where they differ within the batch."""
    first = cases[0]
    assert all(c.kind == first.kind and c.nS == first.nS for c in cases)
    if first.kind == "logistic":
        assert all(c.c == 1.5 and c.ub == 1.0 for c in cases)
        return ocs.LogisticProblem(bc.LOGISTIC_M[:first.nS], 1.5, 0.05, bc.BOUNDS)
    pr = ocs.TestOCProblem(bc.BL3, bc.BOUNDS)
    if any((c.c, c.ub) != (1.5, 1.0) for c in cases):
        pr.set_batch_params([0], np.array([[c.c for c in cases]]))
        pr.set_batch_bounds(np.zeros((1, len(cases))), np.array([[c.ub for c in cases]]))
    return pr


def solve_batch(ocs, cases, options=None, y0=None):
    X0 = np.array([c.x0 for c in cases]).T
    o = dict({"nINTERP_PTS": 11}, **(options or {}))
    if y0 is not None:
        o["y0"] = np.stack(y0, axis=2)
    return ocs.bvp_solver_batch(device_problem(ocs, cases), X0, cases[0].tspan, o)


def start_of(case, oracle):
    return case.y0 if case.y0 is not None else bt.constant_guess(case.problem(oracle), case.x0, case.tspan)


def check_steps(ocs, oracle, cases, batch=None, **options):
    """Every step of the cases' traces in one call: instance = (case, iteration k), started from the twin's y_{k-1}, one
    iteration allowed.  Returns the largest gap / step_noise."""
    inst = [(c, r) for c in cases for r in c.step_records(oracle, **options)]
    inst = [inst[b % len(inst)] for b in range(batch or len(inst))]
    assert len(inst) <= 130
    res = solve_batch(ocs, [c for c, _ in inst], dict(options, MaxIter=1), [r["from"] for _, r in inst])
    worst = 0.0
    for b, (c, r) in enumerate(inst):
        y = res["y"][:, :, b]
        gap = np.abs(y - r["y"])
        ratio = float(gap.max() / r["noise"])
        worst = max(worst, ratio)
        _, f, _, fm = bt.residual(c.problem(oracle), c.x0, c.tspan, y, parts=True)
        phi = float(np.max(np.abs(bt.residual(c.problem(oracle), c.x0, c.tspan, y))))
        scale = max(1.0, float(np.abs(y).max()), float(np.abs(f).max()), float(np.abs(fm).max()))
        print(f"{c.name} k {r['k']} alpha {r['alpha']}: gap {gap.max():.2e} = {ratio:.2f} step_noise, "
              f"resnorm {res['resnorm'][b]:.3e} (twin's of this y {phi:.3e}), ||Phi||_inf of the twin's y_k {r['resinf']:.3e}")
        assert res["iterations"][b] == 1, (c.name, r["k"])
        assert (gap <= bc.step_bound(r["noise"], r["y"])).all(), (c.name, r["k"], float(gap.max()), r["noise"], ratio)
        assert abs(res["resnorm"][b] - phi) <= RES_ULPS * bc.EPS * scale, (c.name, r["k"], res["resnorm"][b], phi)
        assert bool(res["converged"][b]) == r["converged"], (c.name, r["k"], res["resnorm"][b], r["resinf"])
    assert res["status"] == (0 if all(r["converged"] for _, r in inst) else 2)
    print(f"largest gap / step_noise: {worst:.2f} (margin {bc.MARGIN})")
    return worst


def groups(cases):
    out = {}
    for c in cases:
        out.setdefault(c.group(), []).append(c)
    return out


STEP_GROUPS = groups(bc.FULL + bc.LOGISTIC + bc.PER_TRAJECTORY + bc.DAMPED)


@pytest.mark.parametrize("group", list(STEP_GROUPS), ids=lambda g: f"{g[0]}-nS{g[2]}")
def test_one_step_at_a_time(ocs, oracle, group):
    """3a: BL-3 from x0 = 2 and 2.5, the logistic family with 2, 3, 4 states, c and an active upper bound per trajectory, and
    the damped instances (accepted alpha 1/2 ... 1/32), every iteration of the twin's trace."""
    check_steps(ocs, oracle, STEP_GROUPS[group])


def check_counts(ocs, oracle, cases, **options):
    """Whole solves: the verdict and the iteration count of the twin under the same options, per instance; an instance that
    ran out of iterations or step lengths reports a residual above NewtonTol and the call OCS_NUM_NOT_CONVERGED."""
    res = solve_batch(ocs, cases, options)
    failed = False
    for b, c in enumerate(cases):
        tw = c.solve(oracle, **options)
        assert (bool(res["converged"][b]), res["iterations"][b]) == (tw["converged"], tw["iterations"]), \
            (c.name, options, res["converged"][b], res["iterations"][b], tw["converged"], tw["iterations"], tw["why"])
        if not tw["converged"]:
            failed = True
            assert res["resnorm"][b] > TOL, (c.name, options, res["resnorm"][b])
        else:
            assert res["resnorm"][b] <= TOL, (c.name, options, res["resnorm"][b])
    assert res["status"] == (2 if failed else 0)
    return res


COUNT_GROUPS = groups(bc.COUNT_CASES)


@pytest.mark.parametrize("group", list(COUNT_GROUPS), ids=lambda g: f"{g[0]}-nS{g[2]}")
def test_whole_solves_take_the_twins_number_of_iterations(ocs, oracle, group):
    """3b: default options, then MaxIter = the twin's count (converged at exactly the last allowed iteration) and one less
    (failed: iterations == MaxIter, status 2, resnorm > NewtonTol) for every count in the batch."""
    cases = COUNT_GROUPS[group]
    cases = [cases[b % len(cases)] for b in range(max(len(cases), 9))]
    res = check_counts(ocs, oracle, cases)
    counts = sorted(set(res["iterations"].tolist()))
    print(f"{group}: iterations {counts}")
    for m in sorted(set(counts) | {n - 1 for n in counts}):
        lim = check_counts(ocs, oracle, cases, MaxIter=m)
        short = res["iterations"] > m
        assert (lim["iterations"][short] == m).all() and not lim["converged"][short].any()
        assert np.array_equal(lim["iterations"][~short], res["iterations"][~short]) and lim["converged"][~short].all()


def test_reference_script_grid_takes_the_twins_number_of_iterations(ocs, oracle):
    """3b on tests/symbolic_test2.m's problem and grid (N = 200), from starts whose trace is eligible."""
    so = bc.SYMBOLIC_TEST2
    pr, po = ocs.TestOCProblem(so["par"], bc.BOUNDS), oracle.TestOCProblem(so["par"], bc.BOUNDS)
    ts = oracle.linspace(0, so["T"], so["N"] + 1)
    X0 = np.array([so["x0"] * 4])
    tw = {x0: bt.solve(po, [x0], ts) for x0 in so["x0"]}
    want = np.array([tw[x0]["iterations"] for x0 in X0[0]])
    for m in (40, int(want.max()), int(want.max()) - 1):
        res = ocs.bvp_solver_batch(pr, X0, ts, {"nINTERP_PTS": 11, "MaxIter": m})
        assert np.array_equal(res["iterations"], np.minimum(want, m)), (m, res["iterations"], want)
        assert np.array_equal(res["converged"], want <= m) and res["status"] == (0 if (want <= m).all() else 2)


@pytest.mark.parametrize("maxBacktracks", [0, 2, 3, 12])
def test_line_search_follows_the_twin(ocs, oracle, maxBacktracks):
    """3c: the damped instances (first stage: alpha 1/4, 1/2; second stage, after the host's first read of the counts: 1/16,
    1/8, 1/32), full-step instances and the non-converging x0 = .5 in one batch.  maxBacktracks = 2 makes the first stage
    final, 3 leaves one trial (1/8, which x0 = .5 accepts in its second iteration) to the second stage, 0 allows the full
    step only.  The one-step bound on the damped steps themselves: test_one_step_at_a_time[damped]."""
    cases = bc.DAMPED + bc.FULL + [bc.NOT_CONVERGING]
    cases = [cases[b % len(cases)] for b in range(65)]
    res = check_counts(ocs, oracle, cases, maxBacktracks=maxBacktracks)
    print(f"maxBacktracks {maxBacktracks}: iterations {res['iterations'][:6].tolist()}, converged {res['converged'][:6].tolist()}")
    if maxBacktracks in (3, 12):   # x0 = .5 at its second iteration: the step of length 1/8 is the device's, too
        c = bc.NOT_CONVERGING
        tw = c.solve(oracle, maxBacktracks=maxBacktracks)
        assert tw["trace"][1]["alpha"] == 0.125
        one = solve_batch(ocs, [c], {"MaxIter": 1, "maxBacktracks": maxBacktracks}, [tw["trace"][0]["y"]])
        noise = bt.step_noise(c.problem(oracle), c.x0, c.tspan, tw["trace"][0]["y"], maxBacktracks=maxBacktracks)
        gap = np.abs(one["y"][:, :, 0] - tw["trace"][1]["y"])
        print(f"x0 = .5, k 2, alpha 1/8: gap {gap.max():.2e} = {gap.max() / noise:.2f} step_noise")
        assert one["iterations"][0] == 1 and (gap <= bc.step_bound(noise, tw["trace"][1]["y"])).all()


@pytest.mark.parametrize("kind", ["bl3", "logistic"])
@pytest.mark.parametrize("N", bc.EDGE_N)
def test_edge_grids(ocs, oracle, N, kind):
    """3d: N = 1 (the first chunk is the last: both boundary rows in one partial), 2, 7 (below one chunk of 8), 8, 16 (ending
    on a chunk), 9, 17 -- the first N + 1 points of a non-uniform grid, batch 65: whole solves from the constant guess
    against the twin's, and the first step from a guess with nothing round in it (bvp_cases.wavy_guess)."""
    cases = [c for c in bc.EDGE if c.kind == kind and len(c.tspan) == N + 1]
    ts, ring = cases[0].tspan, [cases[b % len(cases)] for b in range(65)]
    res = solve_batch(ocs, ring)
    twins = Twins(lambda i: (cases[i].problem(oracle), cases[i].x0), ts)
    assert check_instances(res, [b % len(cases) for b in range(65)], twins, f"{kind}, N = {N}").all() and res["status"] == 0
    check_steps(ocs, oracle, cases, batch=65)


def test_an_instance_does_not_see_its_batch(ocs, oracle):
    """3e: 130 instances cycling through fast and slow converging ones, the damped ones, x0 = .5 and one that starts on the
    converged root of an earlier solve; each then alone at batch 1.  y, iterations, converged, resnorm: the same bits (one
    instance per lane, reductions in a fixed order); u, x, lam, J: 1e-11 relative (other pass kernels at batch 1)."""
    cases = bc.FULL + bc.DAMPED + [bc.NOT_CONVERGING]
    rooted = bc.Case("BL-3", "bl3", [2.2], bc.NONUNIFORM)
    root = solve_batch(ocs, [rooted])
    assert root["converged"][0]
    starts = [start_of(c, oracle) for c in cases] + [root["y"][:, :, 0].copy()]
    cases = cases + [rooted]
    tw = bt.solve(rooted.problem(oracle), rooted.x0, rooted.tspan, y0=starts[-1])
    n = len(cases)
    res = solve_batch(ocs, [cases[b % n] for b in range(130)], y0=[starts[b % n] for b in range(130)])
    assert (bool(res["converged"][n - 1]), res["iterations"][n - 1]) == (tw["converged"], tw["iterations"]) and tw["iterations"] <= 1
    print(f"from the root: {tw['why']}, iterations {tw['iterations']}; batch of 130: iterations {res['iterations'][:n].tolist()}")
    for i, c in enumerate(cases):
        alone = solve_batch(ocs, [c], y0=[starts[i]])
        for b in range(i, 130, n):
            for k in ("y", "iterations", "converged", "resnorm"):
                assert np.array_equal(res[k][..., b], alone[k][..., 0]), (c.name, b, k)
            for k in ("u", "x", "lam", "J"):
                assert relerr(res[k][..., b], alone[k][..., 0]) < 1e-11, (c.name, b, k)
    assert res["status"] == 2


def test_a_nonfinite_start_fails_alone(ocs, oracle):
    """An instance whose y0 holds a NaN is reported failed before its first iteration (k_bvp_accept: !isfinite -> 2); its
    neighbours' y, iterations and resnorm are the bits of the same batch with a finite guess in that slot."""
    cases = bc.FULL + bc.DAMPED
    ring = [cases[b % len(cases)] for b in range(65)]
    starts = [start_of(c, oracle) for c in ring]
    good = solve_batch(ocs, ring, y0=starts)
    bad_at = 7
    starts[bad_at] = starts[bad_at].copy()
    starts[bad_at][1, 5] = np.nan
    res = solve_batch(ocs, ring, y0=starts)
    assert not res["converged"][bad_at] and res["iterations"][bad_at] == 0 and res["status"] == 2
    others = np.arange(65) != bad_at
    assert good["converged"].all() and res["converged"][others].all()
    for k in ("y", "iterations", "resnorm"):
        assert np.array_equal(res[k][..., others], good[k][..., others]), k


def test_time_tables_on_the_control_side(ocs, oracle):
    """3f: the row-function logistic plugin whose ocs_ControlChar takes e^{rt} from the TU tables (OCS_USER_CC_TCOEF; BvpRhs
    reads TU at 2 i + 1 on the middles) against the registry problem on the non-uniform grid, two and four states (row functions take nS in {1, 2, 4}): equal
    iterations, y and J to 1e-11.  (The proportional-harvest plugin has no twin with a ControlChar in the oracle: left out.)"""
    from tests.user_problems import LOGISTIC_ROWS_CCT_SRC
    for nS in (2, 4):
        m, c, r = bc.LOGISTIC_M[:nS], 1.5, 0.05
        X0 = np.random.default_rng(7 + nS).uniform(2.0, 2.5, (nS, 24))
        pu = ocs.UserProblem(LOGISTIC_ROWS_CCT_SRC, nS, 1, [c, r] + m, bc.BOUNDS, has_control_char=True, row_separable=True)
        a = ocs.bvp_solver_batch(pu, X0, bc.NONUNIFORM, {"nINTERP_PTS": 75})
        b = ocs.bvp_solver_batch(ocs.LogisticProblem(m, c, r, bc.BOUNDS), X0, bc.NONUNIFORM, {"nINTERP_PTS": 75})
        assert a["converged"].all() and np.array_equal(a["iterations"], b["iterations"])
        assert relerr(a["y"], b["y"]) < 1e-11 and relerr(a["J"], b["J"]) < 1e-11
