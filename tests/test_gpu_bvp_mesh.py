"""GPU tests of the mesh side of the batched bvp_solver: ocs_bvp_rms (k_bvp_rms and its reduction), ocs_bvp_prolong and the
loop bvp_solver_adaptive_batch around them, against tests/bvp_mesh_twin.py.

The statement on ocs_bvp_rms and ocs_bvp_prolong is the one of tests/accuracy_check.py, with the float64 twin in the
oracle's place and absolute errors (an rms is a residual: it has no scale of its own):

    |v_device - v_longdouble| <= K max(|v_float64twin - v_longdouble|, 8 eps),   K = 8, eps = 2^-53

per interval (or inserted node and component) and instance, the float64 twin's error taken at that same entry.  The loop is held to the twin's loop on the cases of
tests/bvp_mesh_cases.py, whose residuals stay a factor two away from every threshold (tests/test_bvp_mesh_twin.py)."""
import numpy as np
import pytest

from tests import bvp_cases as bc
from tests import bvp_mesh_cases as mc
from tests import bvp_mesh_twin as mt
from tests import bvp_twin as bt
from tests.accuracy_check import FLOOR, K
from tests.test_gpu_bvp_iteration import device_problem
from tests.test_gpu_bvp_solver import relerr

pytestmark = pytest.mark.gpu
L = np.longdouble


@pytest.fixture(scope="module")
def ocs():
    import torch
    assert torch.cuda.is_available()
    import __graft_entry__ as g
    return g.load_package()


# ---- the instances ocs_bvp_rms is given: the twin's converged iterate and a start with nothing small in its residual ----
def instances(kind, tspan, oracle, memo={}):
    """[(Case, y)]: per Case of the kind on tspan its converged iterate (where the twin converges) and wavy_guess moved by a
    few per cent; the longdouble and float64 estimates are computed once per (kind, grid)."""
    key = (kind, len(tspan))
    if key not in memo:
        if kind == "bl3":
            cases = [bc.Case("rms", "bl3", [x0], tspan) for x0 in (2.0, 2.5)]
        elif kind == "per-trajectory":
            cases = [bc.Case("rms", "bl3", [x0], tspan, c=c, ub=ub) for c, ub, x0 in ((1.5, 0.3, 2.0), (1.7, 0.3, 2.3), (1.9, 0.5, 2.5))]
        else:
            cases = [bc.Case("rms", "logistic", x0, tspan) for x0 in ([2.39, 2.22], [2.38, 2.13, 2.21], [2.34, 2.31, 2.48, 2.21])
                     if f"logistic{len(x0)}" == kind]
        out = []
        for c in cases:
            ys = [bc.wavy_guess(c.x0, tspan) * (1 + 0.03 * np.cos(5 * np.asarray(tspan)))[None, :]]
            tw = bt.solve(c.problem(oracle), c.x0, tspan)
            if tw["converged"]:
                ys.append(tw["y"])
            for y in ys:
                o = mt.optsys_of(c)
                out.append((c, y, mt.rms(o, tspan, y, L), mt.rms(o, tspan, y)))
        memo[key] = out
    return memo[key]


def check_rms(ocs, oracle, kind, tspan, batch, prob=None, what=""):
    inst = instances(kind, tspan, oracle)
    ring = [inst[b % len(inst)] for b in range(batch)]
    pr = prob or device_problem(ocs, [c for c, _, _, _ in ring])
    y = np.stack([y for _, y, _, _ in ring], axis=2)
    res = ocs.bvp_residuals(pr, tspan, y)
    worst = 0.0
    for b, (c, _, ld, f64) in enumerate(ring):
        yard = np.maximum(np.abs(f64.astype(L) - ld).astype(np.float64), FLOOR)
        e = np.abs(res["rms"][:, b].astype(L) - ld).astype(np.float64)
        worst = max(worst, float(np.max(e / yard)))
        assert (e <= K * yard).all(), (what, kind, len(tspan) - 1, batch, b, c.name, float(np.max(e / yard)))
    print(f"ACCURACY rms {what}{kind} N {len(tspan) - 1} batch {batch}: worst err / max(err_twin, 8 eps) = {worst:.2f}; "
          f"rms {res['rms'].min():.2e} .. {res['rms'].max():.2e}")
    assert np.array_equal(res["rmsmax"], res["rms"].max(axis=1)) and np.array_equal(res["rmsinst"], res["rms"].max(axis=0))
    return res, y, pr


GRIDS = [bc.EDGE_GRID[:N + 1] for N in (1, 2, 7, 8, 9, 17)] + [bc.NONUNIFORM]


@pytest.mark.parametrize("kind", ["bl3", "logistic2", "logistic3", "logistic4", "per-trajectory"])
def test_rms_against_the_longdouble_twin(ocs, oracle, kind):
    """Every grid (the chunk-of-8 edges N = 1, 2, 7, 8, 9, 17 and the non-uniform N = 37) at every batch (1, 3, 64, 65, 130)."""
    for ts in GRIDS:
        for batch in (1, 3, 64, 65, 130):
            check_rms(ocs, oracle, kind, ts, batch)


def test_rms_of_a_plugin_is_the_registry_problems(ocs, oracle):
    """The symbolic logistic problem (make_from_symbolic of tests/symbolic_test2.m's expressions: no discount, r = 0, with
    BL-3's c and m) runs the hipRTC instances of k_bvp_rms and k_bvp_prolong: the same bound against the longdouble twin of
    that problem as the registry problem with r = 0, whose bits it may or may not give."""
    import importlib
    from tests.test_symbolic import reference_symbolic_test2
    sym = importlib.import_module("ocs_amd.symbolic")
    g, f, vals, bounds = reference_symbolic_test2(sym)
    par = dict(bc.BL3, r=0.0)
    pu = ocs.make_from_symbolic(g, f, 1, 1, {k: par[str(k)] for k in vals}, bc.BOUNDS)
    reg = ocs.TestOCProblem(par, bc.BOUNDS)
    osys = mt.OptSys([par["m"]], par["c"], 0.0, 0.0, 1.0)
    for ts, batch in ((bc.NONUNIFORM, 65), (bc.EDGE_GRID[:10], 3)):
        inst = instances("bl3", ts, oracle)
        ring = [inst[b % len(inst)][1] for b in range(batch)]
        y = np.stack(ring, axis=2)
        got = {name: ocs.bvp_residuals(p, ts, y)["rms"] for name, p in (("plugin", pu), ("registry", reg))}
        new = mt.refine(ts, np.array([2.0, 200.0] * len(ts))[:len(ts) - 1], 1.0, 100.0)
        pro = {name: ocs.bvp_prolong(p, ts, y, new) for name, p in (("plugin", pu), ("registry", reg))}
        for b in range(min(batch, len(inst))):
            for what, twin, dev in (("rms", lambda d: mt.rms(osys, ts, ring[b], d), {k: v[:, b] for k, v in got.items()}),
                                    ("prolong", lambda d: mt.prolong(osys, ts, ring[b], new, d), {k: v[:, :, b] for k, v in pro.items()})):
                ld = twin(L)
                yard = np.maximum(np.abs(twin(np.float64).astype(L) - ld).astype(np.float64), FLOOR)
                for name, v in dev.items():
                    e = np.abs(v.astype(L) - ld).astype(np.float64)
                    assert (e <= K * yard).all(), (what, name, len(ts) - 1, b, float(np.max(e / yard)))
        print(f"plugin, N {len(ts) - 1}: the registry problem's bits: rms {np.array_equal(got['plugin'], got['registry'])}, "
              f"prolong {np.array_equal(pro['plugin'], pro['registry'])}")


def check_reductions(ocs, pr, ts, y, use, bad, at):
    """rmsmax / rmsinst are NumPy's maxima of the device's own rms; `use` masks instances out of rmsmax only; a NaN in
    instance `bad` at node `at` shows as inf in its own rmsinst and, where in use, in rmsmax -- not in its neighbours'
    rmsinst; the same call twice gives the same bits."""
    batch = y.shape[2]
    res = ocs.bvp_residuals(pr, ts, y)
    assert np.array_equal(res["rmsmax"], res["rms"].max(axis=1)) and np.array_equal(res["rmsinst"], res["rms"].max(axis=0))
    again = ocs.bvp_residuals(pr, ts, y)
    for k in ("rms", "rmsmax", "rmsinst"):
        assert np.array_equal(res[k], again[k]), k
    masked = ocs.bvp_residuals(pr, ts, y, use=use)
    assert np.array_equal(masked["rms"], res["rms"]) and np.array_equal(masked["rmsinst"], res["rmsinst"])
    assert np.array_equal(masked["rmsmax"], res["rms"][:, use].max(axis=1))
    assert not np.array_equal(masked["rmsmax"], res["rmsmax"])
    none = ocs.bvp_residuals(pr, ts, y, use=np.zeros(batch))
    assert (none["rmsmax"] == 0).all() and np.array_equal(none["rmsinst"], res["rmsinst"])
    yn = y.copy()
    yn[1, at, bad] = np.nan
    nan = ocs.bvp_residuals(pr, ts, yn)
    others = np.arange(batch) != bad
    assert np.array_equal(nan["rms"][:, others], res["rms"][:, others]) and np.array_equal(nan["rmsinst"][others], res["rmsinst"][others])
    assert np.isnan(nan["rms"][at - 1:at + 1, bad]).all() and nan["rmsinst"][bad] == np.inf
    want = res["rmsmax"].copy()
    want[at - 1:at + 1] = np.inf
    assert np.array_equal(nan["rmsmax"], want)
    out = ocs.bvp_residuals(pr, ts, yn, use=others)
    assert np.array_equal(out["rmsmax"], res["rms"][:, others].max(axis=1)) and out["rmsinst"][bad] == np.inf


def test_reductions(ocs, oracle):
    """batch 130 on the non-uniform grid; the mask keeps one member of the ring of four, a converged iterate alone; the NaN at
    node 20: intervals 19 and 20 (chunk 2)"""
    ts, batch = bc.NONUNIFORM, 130
    _, y, pr = check_rms(ocs, oracle, "bl3", ts, batch)
    check_reductions(ocs, pr, ts, y, np.arange(batch) % 4 == 1, 70, 20)


def test_reductions_past_one_stride(ocs, oracle):
    """batch 321 = 256 + 64 + 1, N 9: the row loop's second stride and the second workgroup of the per-instance half with its
    partly filled last wave; two chunks, the second a one-interval tail.  The NaN in instance 300 (second stride) at node 8:
    intervals 7 and 8, one in either chunk.  (Every instance is scaled on its own: the ring alone has four different rms.)"""
    ts, batch = bc.EDGE_GRID[:10], 321
    _, y, pr = check_rms(ocs, oracle, "bl3", ts, batch)
    y = y * (1 + 0.01 * np.cos(np.arange(batch)))[None, None, :]
    check_reductions(ocs, pr, ts, y, np.arange(batch) % 3 == 1, 300, 8)


@pytest.mark.parametrize("kind", ["bl3", "logistic2", "logistic4", "per-trajectory"])
def test_prolong(ocs, oracle, kind):
    """Meshes with one insert per interval, two, a mix and none: old nodes come back bit for bit, inserted nodes within the
    K = 8 rule of the longdouble twin."""
    for ts, batch in ((bc.NONUNIFORM, 65), (bc.EDGE_GRID[:10], 130), (bc.EDGE_GRID[:2], 3)):
        inst = instances(kind, ts, oracle)
        ring = [inst[b % len(inst)] for b in range(batch)]
        pr = device_problem(ocs, [c for c, _, _, _ in ring])
        y = np.stack([y for _, y, _, _ in ring], axis=2)
        n = len(ts) - 1
        for name, r in (("one", np.full(n, 2.0)), ("two", np.full(n, 200.0)), ("mixed", np.array([0.1, 2.0, 200.0] * n)[:n]),
                        ("none", np.zeros(n))):
            new = mt.refine(ts, r, 1.0, 100.0)
            old = np.isin(new, ts)
            assert old.sum() == n + 1 and new.size == n + 1 + int((r == 2.0).sum()) + 2 * int((r == 200.0).sum())
            got = ocs.bvp_prolong(pr, ts, y, new)
            assert got.shape == (y.shape[0], new.size, batch) and np.array_equal(got[:, old, :], y), (kind, name)
            worst = 0.0
            for b, (c, yb, _, _) in enumerate(ring[:len(inst)]):
                o = mt.optsys_of(c)
                ld, f64 = mt.prolong(o, ts, yb, new, L), mt.prolong(o, ts, yb, new)
                yard = np.maximum(np.abs(f64.astype(L) - ld).astype(np.float64), FLOOR)
                e = np.abs(got[:, :, b].astype(L) - ld).astype(np.float64)
                worst = max(worst, float(np.max(e / yard)))
                assert (e <= K * yard).all(), (kind, name, b, float(np.max(e / yard)))
                for b2 in range(b + len(inst), batch, len(inst)):
                    assert np.array_equal(got[:, :, b2], got[:, :, b])
            print(f"ACCURACY prolong {kind} N {n} {name} batch {batch}: worst err / max(err_twin, 8 eps) = {worst:.2f}")


# ---- the loop ----
def run_case(ocs, case):
    X0 = np.array([c.x0 for c in case.cases]).T
    return ocs.bvp_solver_adaptive_batch(device_problem(ocs, case.cases), X0, case.mesh[[0, -1]],
                                         dict({"InitMesh": case.mesh, "bvpRelTol": case.tol, "MAX_MESH_SIZE": case.max_nodes,
                                               "nINTERP_PTS": 41}, **case.options))


@pytest.mark.parametrize("case", mc.CASES, ids=lambda c: c.name)
def test_adaptive_loop_takes_the_twins_meshes(ocs, oracle, case):
    """meshes, the final mesh, mesh_status, rms_ok and converged are the twin's; y within 4 ||J^-1|| NewtonTol of the twin's
    root on the final mesh (the bound of tests/test_gpu_bvp_solver.py), rms within what that distance of the roots can move a
    residual; the post-processing on the final mesh as tests/test_gpu_bvp_solver.py and the smoke test hold it: u is ControlChar
    of the pchip of y at interpPts to 1e-12, x, lam and J are the oracle's compute_x_lam_J under the pchip of that u to 1e-11,
    and J is the J of the twin's root under the same post-processing to 1e-9, what test_gpu_bvp_solver.py allows between the J of
    two roots that both meet NewtonTol (test_guesses_reach_the_default_guess_root)."""
    tw = case.twin(oracle)
    res = run_case(ocs, case)
    print(f"{case.name}: meshes {res['meshes']} (twin {tw['meshes']}), status {res['mesh_status']}, converged {res['converged'].tolist()}, "
          f"rms_ok {res['rms_ok'].tolist()}, largest rms / tol {np.nanmax(res['rms']) / case.tol:.3f}")
    assert res["meshes"] == tw["meshes"] and np.array_equal(res["mesh"], tw["mesh"]) and np.array_equal(res["tspan"], tw["mesh"])
    assert res["mesh_status"] == tw["mesh_status"]
    assert np.array_equal(res["converged"], tw["converged"]) and np.array_equal(res["rms_ok"], tw["rms_ok"])
    assert res["rms"].shape == tw["rms"].shape
    for b, c in enumerate(case.cases):
        if not tw["converged"][b]:
            continue
        prob = c.problem(oracle)
        inv = bt.inverse_norm(prob, c.x0, tw["mesh"], tw["y"][b])
        gap = float(np.max(np.abs(res["y"][:, :, b] - tw["y"][b])))
        assert gap <= 4 * inv * bc.TOL, (case.name, b, gap, inv)
        assert float(np.max(np.abs(bt.residual(prob, c.x0, tw["mesh"], res["y"][:, :, b])))) <= 2 * bc.TOL
        # a root moved by gap moves S' - f by at most (3 / h + |df/dy| (1 + h |df/dy| / 4)) gap; |df/dy| <= m + 2 |x| + 2 < 16 here
        hmin = float(np.min(np.diff(tw["mesh"])))
        assert np.max(np.abs(res["rms"][:, b] - tw["rms"][:, b])) <= (3 / hmin + 16 * (1 + 4 * hmin)) * 4 * inv * bc.TOL, (case.name, b)
        # u, x, lam, J of the final mesh
        pts, integ = res["interpPts"], oracle.RK4Integrator(tw["mesh"])
        post = {}
        for who, y in (("device", res["y"][:, :, b]), ("twin", tw["y"][b])):
            yq = oracle.vector_interp(tw["mesh"], y, oracle.INTERP_PCHIP, pts)
            u = prob.ControlChar(pts, yq[:c.nS], yq[c.nS:])
            post[who] = (u,) + oracle.compute_x_lam(integ, prob, c.x0, oracle.vector_interp(pts, u, oracle.INTERP_PCHIP, integ.t), want_J=True)
        u, x, lam, J = post["device"]
        assert relerr(res["u"][:, :, b], u) < 1e-12, (case.name, b)
        ud = res["u"][:, :, b]
        xo, lo, Jo = oracle.compute_x_lam(integ, prob, c.x0, oracle.vector_interp(pts, ud, oracle.INTERP_PCHIP, integ.t), want_J=True)
        assert relerr(res["x"][:, :, b], xo) < 1e-11 and relerr(res["lam"][:, :, b], lo) < 1e-11 and relerr(res["J"][b], Jo) < 1e-11
        print(f"  instance {b}: J {res['J'][b]:.12g}, twin's post-processing {post['twin'][3]:.12g}, oracle under the device's u {Jo:.12g}")
        assert relerr(res["J"][b], post["twin"][3]) < 1e-9, (case.name, b)


@pytest.mark.parametrize("case", [c for c in mc.CASES if len(c.cases) == 1 and c.max_nodes >= 1000], ids=lambda c: c.name)
def test_single_instances_against_solve_bvp(ocs, oracle, case):
    """scipy.integrate.solve_bvp from the same first mesh and guess at the same tol: y at the common nodes and J (scipy's
    from a cost row added to its system) within 10 tol."""
    from scipy.integrate import solve_bvp
    c = case.cases[0]
    o, nS = mt.optsys_of(c), c.nS
    x0 = np.array(c.x0)

    def fun(t, y):
        u = o.control(t, y[:2 * nS])
        return np.vstack([o(t, y[:2 * nS]), np.exp(-o.r * t) * (np.sum(y[:nS] ** 2, axis=0) + o.c * u ** 2)])

    guess = np.vstack([bt.constant_guess(c.problem(oracle), c.x0, case.mesh), np.zeros((1, case.mesh.size))])
    sol = solve_bvp(fun, lambda ya, yb: np.concatenate([ya[:nS] - x0, yb[nS:2 * nS], ya[2 * nS:]]), case.mesh, guess, tol=case.tol,
                    max_nodes=1000)
    assert sol.status == 0
    res = run_case(ocs, case)
    assert res["mesh_status"] == 0 and res["rms_ok"].all()
    common = np.intersect1d(res["mesh"], sol.x)
    assert common.size >= case.mesh.size
    dy = float(np.max(np.abs(res["y"][:, np.isin(res["mesh"], common), 0] - sol.y[:2 * nS, np.isin(sol.x, common)])))
    dJ = abs(float(res["J"][0]) - float(sol.y[-1, -1]))
    print(f"{case.name}: {common.size} common nodes (ours {res['mesh'].size}, scipy's {sol.x.size}); |y - y_scipy| {dy:.3e}, "
          f"|J - J_scipy| {dJ:.3e}, 10 tol {10 * case.tol:.1e}")
    assert dy <= 10 * case.tol and dJ <= 10 * case.tol


def test_host_helpers_are_the_twins(ocs):
    """the package's statement of the refinement rule and of the prolongation map against the twin's (which
    tests/test_bvp_mesh_twin.py holds against scipy's modify_mesh)"""
    from ocs_amd import mesh
    rng = np.random.default_rng(5)
    for _ in range(100):
        n = int(rng.integers(1, 40))
        x = np.sort(rng.uniform(0.0, 10.0, n + 1))
        tol = float(10 ** rng.uniform(-6, -2))
        r = tol * 10 ** rng.uniform(-3, 4, n)
        r[rng.uniform(size=n) < 0.1] = tol
        r[rng.uniform(size=n) < 0.1] = 100 * tol
        r[rng.uniform(size=n) < 0.05] = np.nan
        new = mt.refine(x, r, tol, 100 * tol)
        assert np.array_equal(mesh.refine_mesh(x, r, tol, 100 * tol), new)
        idx, theta = mesh._prolong_map(x, new)
        ti, tt = mt.locate(x, new)
        assert np.array_equal(idx, ti) and np.array_equal(theta, tt) and theta[-1] == 1.0 and (theta[np.isin(new, x)][:-1] == 0.0).all()


# ---- what does not change ----
def test_solver_is_untouched_by_the_mesh_calls(ocs, oracle):
    """bvp_solver_batch before and after bvp_residuals / bvp_prolong on the same handle: the same bits; it still warns on
    bvpRelTol."""
    cases = bc.FULL + bc.DAMPED
    pr, X0 = device_problem(ocs, cases), np.array([c.x0 for c in cases]).T
    gi = ocs.RK4Integrator(bc.NONUNIFORM)
    before = ocs.bvp_solver_batch(pr, X0, bc.NONUNIFORM, {"nINTERP_PTS": 41}, integrator=gi)
    ocs.bvp_residuals(pr, bc.NONUNIFORM, before["y"], integrator=gi)
    ocs.bvp_prolong(pr, bc.NONUNIFORM, before["y"], mt.refine(bc.NONUNIFORM, np.full(37, 2.0), 1.0, 100.0), integrator=gi)
    after = ocs.bvp_solver_batch(pr, X0, bc.NONUNIFORM, {"nINTERP_PTS": 41}, integrator=gi)
    for k in ("y", "x", "lam", "u", "J", "iterations", "converged", "resnorm"):
        assert np.array_equal(before[k], after[k]), k
    with pytest.warns(RuntimeWarning, match="bvpRelTol"):
        ocs.bvp_solver_batch(pr, X0, bc.NONUNIFORM, {"nINTERP_PTS": 41, "bvpRelTol": 1e-6, "MAX_MESH_SIZE": 1000})
    with pytest.warns(RuntimeWarning, match="bvpAbsTol"):
        ocs.bvp_solver_adaptive_batch(pr, X0, [0.0, 2.0], {"nINTERP_PTS": 41, "bvpRelTol": 1e-2, "bvpAbsTol": 1e-6, "InitMesh": [0.0, 1.0, 2.0]})


def test_refusals(ocs, oracle):
    """LQ, nS > 4, the tiled layout and an RK4InfiniteIntegrator grid: OCS_ERR_UNSUPPORTED from both entry points, with the
    messages of ocs_bvp_solver; a prolongation map that leaves the old mesh: OCS_ERR_INVALID."""
    from tests.user_problems import lq_matrices, lq_source
    ts = bc.EDGE_GRID[:10]
    A, Bu, q, rd = lq_matrices(6, 1)
    big = [ocs.LQProblem(A, Bu, q, rd, 0.05, [[-5.0, 5.0]]),
           ocs.UserProblem(lq_source(6, 1), 6, 1, np.concatenate([[0.05], A.ravel(order="F"), Bu.ravel(order="F"), q, rd]), [[-5.0, 5.0]])]
    pr = ocs.TestOCProblem(bc.BL3, bc.BOUNDS)
    y1 = np.ones((2, 10, 4))
    calls = [(p, ocs.RK4Integrator(ts), "bvp_solver") for p in big]
    calls.append((pr, ocs.RK4Integrator(ts).set_layout("tiled"), "tiled layout"))
    calls.append((pr, ocs.RK4InfiniteIntegrator(ts, np.linspace(ts[-1], ts[-1] + 2, 5), [0.4]), "RK4Integrator grid"))
    for p, gi, msg in calls:
        y = np.ones((2 * p.nS, gi.nSTEPS + 1, 4))
        for f in (lambda: ocs.bvp_residuals(p, gi.tspan, y, integrator=gi), lambda: ocs.bvp_prolong(p, gi.tspan, y, ts, integrator=gi)):
            with pytest.raises(ocs.OcsError) as e:
                f()
            assert e.value.code == -6 and msg in str(e.value), e.value
    with pytest.raises(ocs.OcsError) as e:
        ocs.bvp_prolong(pr, ts, y1, np.append(ts, ts[-1] + 1.0))
    assert e.value.code == -1, e.value
