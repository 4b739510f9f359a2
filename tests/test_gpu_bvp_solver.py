"""GPU tests of the batched bvp_solver (functions/bvp_solver.m; csrc/ocs_bvp_device.hpp, ocs_bvp_kernels.hip, ocs_bvp.cpp)
against its NumPy twin (tests/bvp_twin.py: same residual, dense Newton system) instance by instance.

Bounds.  Device and twin both stop at ||Phi||_inf <= NewtonTol on the same residual, so their roots differ by at most
||J^{-1}||_inf (tol + tol) to first order: the tests allow 4 ||J^{-1}||_inf NewtonTol per instance, ||J^{-1}||_inf taken
from the twin's dense Jacobian at its root, and ask the twin's own residual function of the device's y for <= 2 NewtonTol."""
import numpy as np
import pytest

from tests import bvp_twin as bt

pytestmark = pytest.mark.gpu
BOUNDS = [[0.0, 1.0]]
TOL = 1e-10          # NewtonTol (the default)
BL3 = {"c": 1.5, "m": 3.0, "r": 0.05}


@pytest.fixture(scope="module")
def ocs():
    import torch
    assert torch.cuda.is_available()
    import __graft_entry__ as g
    return g.load_package()


def relerr(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.max(np.abs(a - b) / np.maximum(1.0, np.abs(b))))


class Twins:
    """Twin solutions keyed by what distinguishes an instance; `make(key)` gives (oracle problem, x0) of that instance."""

    def __init__(self, make, ts):
        self.make, self.ts, self.memo = make, ts, {}

    def __call__(self, key):
        if key not in self.memo:
            prob, x0 = self.make(key)
            r = bt.solve(prob, x0, self.ts)
            r["inv"] = bt.inverse_norm(prob, x0, self.ts, r["y"]) if r["converged"] else np.nan
            self.memo[key] = (prob, x0, r)
        return self.memo[key]


def check_instances(res, keys, twins, what=""):
    """Every instance against its twin: same verdict; where converged, the twin's residual of the device's y and the
    distance of the two roots within the bounds of the module docstring.  Returns the converged mask of the twin."""
    conv = []
    worst_res = worst_gap = 0.0
    for b, key in enumerate(keys):
        prob, x0, tw = twins(key)
        conv.append(tw["converged"])
        assert bool(res["converged"][b]) == tw["converged"], (what, b, key, res["iterations"][b], tw["iterations"], tw["why"])
        if not tw["converged"]:
            continue
        y = res["y"][:, :, b]
        phi = float(np.max(np.abs(bt.residual(prob, x0, twins.ts, y))))
        gap = float(np.max(np.abs(y - tw["y"])))
        worst_res, worst_gap = max(worst_res, phi), max(worst_gap, gap / (tw["inv"] * TOL))
        assert res["resnorm"][b] <= TOL and phi <= 2 * TOL, (what, b, key, res["resnorm"][b], phi)
        assert gap <= 4 * tw["inv"] * TOL, (what, b, key, gap, tw["inv"])
    print(f"{what}: {len(keys)} instances, {int(np.sum(conv))} converged; worst twin residual of the device's y {worst_res:.2e}, "
          f"worst root distance {worst_gap:.2e} x ||J^-1|| NewtonTol; iterations {sorted(set(res['iterations'].tolist()))}")
    return np.array(conv)


def test_reference_script_case_converges_where_the_sweep_does_not(ocs, oracle):
    """tests/symbolic_test2.m solves [0, 5] from x0 = .1 with bvp_solver: TestOCProblem{c 4, m .5, r 0}, N = 200.  Every
    instance converges in <= 10 Newton iterations; fb_sweep_batch on the same inputs does not settle, as before."""
    par = {"c": 4.0, "m": 0.5, "r": 0.0}
    pr, ts = ocs.TestOCProblem(par, BOUNDS), oracle.linspace(0, 5, 201)
    X0 = np.array([[0.1, 0.3, 0.2, 0.45] * 16])
    res = ocs.bvp_solver_batch(pr, X0, ts, {"nINTERP_PTS": 101})
    assert res["status"] == 0 and res["converged"].all() and res["iterations"].max() <= 10, res["iterations"]
    sw = ocs.fb_sweep_batch(pr, X0, ts, {"nERROR_PTS": 201, "nINTERP_PTS": 101})
    assert sw["status"] == 2 and not (sw["sweeps"] > 0).all() and sw["sweeps"][0] == 0
    twins = Twins(lambda x0: (oracle.TestOCProblem(par, BOUNDS), [x0]), ts)
    check_instances(res, X0[0].tolist(), twins, "symbolic_test2 on [0, 5]")
    assert np.isfinite(res["J"]).all() and relerr(res["x"][:, 0, :], X0) < 1e-15
    # the post-processing is what it says: u = ControlChar(interpPts, pchip y), x of compute_x_lam_J under it near y's state
    po = oracle.TestOCProblem(par, BOUNDS)
    for b in (0, 1, 63):
        yq = oracle.vector_interp(ts, res["y"][:, :, b], oracle.INTERP_PCHIP, res["interpPts"])
        assert relerr(res["u"][:, :, b], po.ControlChar(res["interpPts"], yq[:1], yq[1:])) < 1e-12
        assert np.max(np.abs(res["x"][:, :, b] - res["y"][:1, :, b])) < 1e-6


def test_agrees_with_the_sweep_where_the_sweep_converges(ocs, oracle):
    """The same problem on [0, 2], where fb_sweep converges: J and u of the two drivers agree.  Bound on u: twice the twin's
    own difference between N and 2N (the discretisation) plus the sweep's stopping tolerance uRelTol |u| + uAbsTol; on J the
    largest such bound times max(1, |J|) (J is stationary in u at the solution)."""
    par = {"c": 4.0, "m": 0.5, "r": 0.0}
    pr, po = ocs.TestOCProblem(par, BOUNDS), oracle.TestOCProblem(par, BOUNDS)
    N = 200
    ts, ts2 = oracle.linspace(0, 2, N + 1), oracle.linspace(0, 2, 2 * N + 1)
    x0s = [0.1, 0.3, 0.2, 0.45]
    X0 = np.array([x0s * 16])
    res = ocs.bvp_solver_batch(pr, X0, ts, {"nINTERP_PTS": N + 1})
    sw = ocs.fb_sweep_batch(pr, X0, ts, {"nERROR_PTS": N + 1, "nINTERP_PTS": N + 1})
    assert res["converged"].all() and (sw["sweeps"] > 0).all()
    refine = 0.0
    for x0 in x0s:
        a, b = bt.solve(po, [x0], ts), bt.solve(po, [x0], ts2)
        assert a["converged"] and b["converged"]
        refine = max(refine, float(np.max(np.abs(a["y"] - b["y"][:, ::2]))))
    bound_u = 2 * refine + 1e-7 * np.abs(sw["u"]) + 1e-7
    du, dJ = np.abs(res["u"] - sw["u"]), np.abs(res["J"] - sw["J"])
    print(f"[0, 2]: twin refinement {refine:.2e}; |u_bvp - u_sweep| max {du.max():.2e} (bound {bound_u.max():.2e}), "
          f"|J_bvp - J_sweep| max {dJ.max():.2e}; sweeps {sorted(set(sw['sweeps'].tolist()))}")
    assert (du <= bound_u).all()
    assert (dJ <= bound_u.max() * np.maximum(1.0, np.abs(sw["J"]))).all()


def test_failed_instances_are_reported_and_leave_their_neighbours_alone(ocs, oracle):
    """BL-3 problem on [0, 10]: x0 = .5 does not converge from the constant guess (neither does the twin, nor solve_bvp);
    the call returns OCS_NUM_NOT_CONVERGED, the converged set is the twin's, the neighbours meet the usual bounds."""
    pr, ts = ocs.TestOCProblem(BL3, BOUNDS), oracle.linspace(0, 10, 101)
    x0s = [2.0, 2.5, 0.5, 2.2, 1.8, 2.8, 3.0, 2.4]
    X0 = np.array([x0s * 4])
    res = ocs.bvp_solver_batch(pr, X0, ts, {"nINTERP_PTS": 101})
    twins = Twins(lambda x0: (oracle.TestOCProblem(BL3, BOUNDS), [x0]), ts)
    conv = check_instances(res, X0[0].tolist(), twins, "BL-3 on [0, 10]")
    assert conv.mean() >= 0.75 and not conv.all()
    assert res["status"] == 2                                         # OCS_NUM_NOT_CONVERGED
    assert (res["iterations"][~conv] >= 1).all() and (res["resnorm"][~conv] > TOL).all()


NONUNIFORM = 10.0 * np.linspace(0.0, 1.0, 38) ** 1.3                  # N = 37: no multiple of the interval chunk (8)


@pytest.mark.parametrize("batch", [1, 63, 65, 300])
def test_batch_shapes_on_a_nonuniform_grid(ocs, oracle, batch):
    pr = ocs.TestOCProblem(BL3, BOUNDS)
    x0s = np.linspace(2.0, 2.5, 7)
    X0 = x0s[np.arange(batch) % 7][None, :]
    res = ocs.bvp_solver_batch(pr, X0, NONUNIFORM, {"nINTERP_PTS": 75})
    twins = Twins(lambda x0: (oracle.TestOCProblem(BL3, BOUNDS), [x0]), NONUNIFORM)
    assert check_instances(res, X0[0].tolist(), twins, f"batch {batch}, N = 37 non-uniform").all() and res["status"] == 0


@pytest.mark.parametrize("nS", [2, 4])
def test_logistic_family(ocs, oracle, nS):
    m = [3.0, 2.5, 2.0, 2.8][:nS]
    pr = ocs.LogisticProblem(m, 1.5, 0.05, BOUNDS)
    rng = np.random.default_rng(40 + nS)
    starts = rng.uniform(2.0, 2.5, (5, nS))
    batch = 65
    X0 = starts[np.arange(batch) % 5].T
    res = ocs.bvp_solver_batch(pr, X0, NONUNIFORM, {"nINTERP_PTS": 75})
    twins = Twins(lambda k: (oracle.LogisticProblem(m, 1.5, 0.05, BOUNDS), starts[k]), NONUNIFORM)
    assert check_instances(res, (np.arange(batch) % 5).tolist(), twins, f"Logistic nS = {nS}").all() and res["status"] == 0


def test_per_trajectory_parameters_and_bounds(ocs, oracle):
    """c of its own per trajectory (set_batch_params) and control bounds of its own (set_batch_bounds) with an upper bound
    that is active along most of the horizon: every instance against the twin of ITS problem."""
    batch = 65
    cs, ubs, x0s = [1.5, 1.7, 1.9], [0.3, 0.5, 1.0], [2.0, 2.3, 2.5, 2.1]
    keys = [(cs[b % 3], ubs[(b // 3) % 3], x0s[b % 4]) for b in range(batch)]
    pr = ocs.TestOCProblem(BL3, BOUNDS)
    pr.set_batch_params([0], np.array([[k[0] for k in keys]]))
    pr.set_batch_bounds(np.zeros((1, batch)), np.array([[k[1] for k in keys]]))
    X0 = np.array([[k[2] for k in keys]])
    res = ocs.bvp_solver_batch(pr, X0, NONUNIFORM, {"nINTERP_PTS": 75})
    twins = Twins(lambda k: (oracle.TestOCProblem({"c": k[0], "m": 3.0, "r": 0.05}, [[0.0, k[1]]]), [k[2]]), NONUNIFORM)
    assert check_instances(res, keys, twins, "per-trajectory c and bounds").all()
    active = [b for b, k in enumerate(keys) if k[1] == 0.3]
    assert active and all((res["u"][:, :, b] == 0.3).sum() > 30 and res["u"][:, :, b].max() <= 0.3 for b in active)
    assert any(res["u"][:, :, b].max() > 0.5 for b, k in enumerate(keys) if k[1] == 1.0)


def test_plugins_give_the_registry_problems_solution(ocs, oracle):
    """The make_from_symbolic plugin of tests/symbolic_test2.m and the row-function logistic plugin run the hipRTC instances
    of the same kernels: y and J of the registry problem to 1e-11 relative, the same iteration counts."""
    import importlib
    from tests.test_symbolic import reference_symbolic_test2
    from tests.user_problems import LOGISTIC_ROWS_CC_SRC
    sym = importlib.import_module("ocs_amd.symbolic")
    g, f, vals, bounds = reference_symbolic_test2(sym)
    ts = oracle.linspace(0, 5, 201)
    X0 = np.array([[0.1, 0.3, 0.2, 0.45] * 4])
    a = ocs.bvp_solver_batch(ocs.make_from_symbolic(g, f, 1, 1, vals, bounds), X0, ts, {"nINTERP_PTS": 101})
    b = ocs.bvp_solver_batch(ocs.TestOCProblem({"c": 4.0, "m": 0.5, "r": 0.0}, bounds), X0, ts, {"nINTERP_PTS": 101})
    assert a["converged"].all() and np.array_equal(a["iterations"], b["iterations"])
    assert relerr(a["y"], b["y"]) < 1e-11 and relerr(a["J"], b["J"]) < 1e-11

    m, c, r = [3.0, 2.5], 1.5, 0.05
    X0 = np.random.default_rng(7).uniform(2.0, 2.5, (2, 24))
    pu = ocs.UserProblem(LOGISTIC_ROWS_CC_SRC, 2, 1, [c, r] + m, BOUNDS, has_control_char=True, row_separable=True)
    a = ocs.bvp_solver_batch(pu, X0, NONUNIFORM, {"nINTERP_PTS": 75})
    b = ocs.bvp_solver_batch(ocs.LogisticProblem(m, c, r, BOUNDS), X0, NONUNIFORM, {"nINTERP_PTS": 75})
    assert a["converged"].all() and np.array_equal(a["iterations"], b["iterations"])
    assert relerr(a["y"], b["y"]) < 1e-11 and relerr(a["J"], b["J"]) < 1e-11


def test_guesses_reach_the_default_guess_root(ocs, oracle):
    """options y0 (samples on the nodes, and a callable) and u0 (a control guess: the start is compute_x_lam under it)
    converge to the root the constant guess finds (bvp_solver.m:87-98)."""
    pr, ts = ocs.TestOCProblem(BL3, BOUNDS), oracle.linspace(0, 10, 101)
    x0s = [2.0, 2.2, 2.5]
    X0 = np.array([x0s * 3])
    twins = Twins(lambda x0: (oracle.TestOCProblem(BL3, BOUNDS), [x0]), ts)
    base = ocs.bvp_solver_batch(pr, X0, ts, {"nINTERP_PTS": 101})
    ypert = base["y"] * (1.0 + 0.05 * np.sin(ts)[None, :, None])
    runs = {"y0 samples": {"y0": ypert},
            "y0 callable": {"y0": lambda t: np.vstack([2.2 * np.ones_like(t), 0.1 * (10.0 - t)])},
            "u0": {"u0": lambda t: 0.4 + 0.0 * t}}
    for name, o in runs.items():
        res = ocs.bvp_solver_batch(pr, X0, ts, dict(o, nINTERP_PTS=101))
        assert check_instances(res, X0[0].tolist(), twins, name).all()
        assert relerr(res["J"], base["J"]) < 1e-9
    with pytest.warns(RuntimeWarning, match="bvpRelTol"):
        ocs.bvp_solver_batch(pr, X0, ts, {"nINTERP_PTS": 101, "bvpRelTol": 1e-6, "MAX_MESH_SIZE": 1000})


def test_handle_reuse_and_refusals(ocs, oracle):
    """A second call on the same integrator after a call with another batch returns the bits of a fresh handle; the LQ
    problem and a six-state plugin are refused with OCS_ERR_UNSUPPORTED."""
    from tests.user_problems import lq_matrices, lq_source
    pr, ts = ocs.TestOCProblem(BL3, BOUNDS), oracle.linspace(0, 10, 101)
    Xa, Xb = np.array([[2.0, 2.5, 0.5, 2.2, 1.8, 2.8, 3.0, 2.4]]), np.array([[2.1, 2.6, 1.9, 2.45, 2.3]])
    gi = ocs.RK4Integrator(ts)
    ocs.bvp_solver_batch(pr, Xa, ts, {"nINTERP_PTS": 101}, integrator=gi)
    again = ocs.bvp_solver_batch(pr, Xb, ts, {"nINTERP_PTS": 101}, integrator=gi)
    fresh = ocs.bvp_solver_batch(pr, Xb, ts, {"nINTERP_PTS": 101}, integrator=ocs.RK4Integrator(ts))
    for k in ("y", "x", "lam", "u", "J", "iterations", "converged", "resnorm"):
        assert np.array_equal(again[k], fresh[k]), k
    assert again["converged"].all()
    A, Bu, q, rd = lq_matrices(6, 1)
    refused = [ocs.LQProblem(A, Bu, q, rd, 0.05, [[-5.0, 5.0]]),
               ocs.UserProblem(lq_source(6, 1), 6, 1, np.concatenate([[0.05], A.ravel(order="F"), Bu.ravel(order="F"), q, rd]),
                               [[-5.0, 5.0]])]
    for prob in refused:
        with pytest.raises(ocs.OcsError) as e:
            ocs.bvp_solver_batch(prob, np.ones((6, 4)), ts)
        assert e.value.code == -6, e.value                              # OCS_ERR_UNSUPPORTED
