"""CPU checks of tests/bvp_mesh_twin.py, the yardstick of tests/test_gpu_bvp_mesh.py: its residual estimate, refinement rule
and prolongation against scipy.integrate.solve_bvp's own (both reference-side), its optSys against the oracle's, and the
adaptive cases of tests/bvp_mesh_cases.py: robust against last-bit differences, and each showing what it is there for."""
import numpy as np
import pytest
from scipy.integrate import solve_bvp
from scipy.integrate._bvp import modify_mesh

from tests import bvp_cases as bc
from tests import bvp_mesh_cases as mc
from tests import bvp_mesh_twin as mt
from tests import bvp_twin as bt

EPS = 2.0 ** -53
# largest |rms_twin - sol.rms_residuals| / max(sol.rms_residuals) measured over the three problems below (NOTES.md): the two
# evaluate the same interpolant in another basis, the difference is the rounding of S' - f (O(1) terms, eps each) seen from
# an rms of 1e-4
MEASURED = 9.5e-12
PROBLEMS = [("BL-3", [3.0], [2.0]), ("logistic 2", bc.LOGISTIC_M[:2], [2.39, 2.22]), ("logistic 4", bc.LOGISTIC_M, [2.34, 2.31, 2.48, 2.21])]


def scipy_solution(m, x0, memo={}):
    key = tuple(m)
    if key not in memo:
        osys, nS = mt.OptSys(m, 1.5, 0.05, 0.0, 1.0), len(m)
        x = np.linspace(0.0, 10.0, 11)
        guess = np.vstack([np.repeat(np.array(x0)[:, None], x.size, axis=1), np.zeros((nS, x.size))])
        sol = solve_bvp(lambda t, y: osys(t, y), lambda ya, yb: np.concatenate([ya[:nS] - x0, yb[nS:]]), x, guess, tol=1e-4)
        assert sol.status == 0 and sol.x.size > 30
        memo[key] = (osys, sol)
    return memo[key]


@pytest.mark.parametrize("name,m,x0", PROBLEMS, ids=[p[0] for p in PROBLEMS])
def test_optsys_is_the_oracles(oracle, name, m, x0):
    """float64 OptSys against the oracle's adapter (stateRHS, adjointRHS under ControlChar) at random points, clamped ones
    included: a few roundings of terms up to m |x| + x^2 apart."""
    osys, prob = mt.OptSys(m, 1.5, 0.05, 0.0, 1.0), oracle.LogisticProblem(m, 1.5, 0.05, [[0.0, 1.0]])
    rng = np.random.default_rng(2)
    y, t = rng.uniform(-0.5, 3.0, (2 * len(m), 400)), rng.uniform(0.0, 10.0, 400)
    a, b = osys(t, y), bt.optsys(prob, t, y)
    u = osys.control(t, y)
    assert (u == 0.0).any() and (u == 1.0).any() and ((u > 0.0) & (u < 1.0)).any()
    assert np.max(np.abs(a - b) / np.maximum(1.0, np.abs(y[:len(m)]) * (np.array(m)[:, None] + np.abs(y[:len(m)]))).max(axis=0)) <= 16 * EPS


@pytest.mark.parametrize("name,m,x0", PROBLEMS, ids=[p[0] for p in PROBLEMS])
def test_rms_is_scipys_estimate(name, m, x0):
    osys, sol = scipy_solution(m, x0)
    r = mt.rms(osys, sol.x, sol.y)
    top = float(np.max(sol.rms_residuals))
    rel = float(np.max(np.abs(r - sol.rms_residuals))) / top
    print(f"{name}: {sol.x.size} nodes, largest rms {top:.3e}, |twin - scipy| / largest rms = {rel:.3e}")
    assert rel <= min(16 * MEASURED, 1e-8)
    rl = mt.rms(osys, sol.x, sol.y, mt.L)
    assert rl.dtype == mt.L and float(np.max(np.abs(rl - r))) / top <= min(16 * MEASURED, 1e-8)


def test_refine_is_scipys_modify_mesh():
    rng = np.random.default_rng(5)
    for _ in range(200):
        n = int(rng.integers(1, 40))
        x = np.sort(rng.uniform(0.0, 10.0, n + 1))
        tol = float(10 ** rng.uniform(-6, -2))
        r = tol * 10 ** rng.uniform(-3, 4, n)
        r[rng.uniform(size=n) < 0.1] = tol                             # on the threshold: neither rule inserts
        r[rng.uniform(size=n) < 0.1] = 100 * tol                       # two nodes
        i1, = np.nonzero((r > tol) & (r < 100 * tol))
        i2, = np.nonzero(r >= 100 * tol)
        want = modify_mesh(x, i1, i2)
        assert np.array_equal(mt.refine(x, r, tol, 100 * tol), want)
    assert mt.refine([0.0, 1.0, 2.0], [np.nan, 0.0], 1.0, 100.0).size == 5


@pytest.mark.parametrize("name,m,x0", PROBLEMS, ids=[p[0] for p in PROBLEMS])
def test_prolong_is_scipys_spline(name, m, x0):
    """sol.sol is the cubic through (y_i, fun(x_i, y_i)): the same interpolant in PPoly's basis.  Between two evaluations of a
    cubic with terms of size |y| + h |f|: 16 eps of that."""
    osys, sol = scipy_solution(m, x0)
    q = np.sort(np.concatenate([sol.x, np.random.default_rng(1).uniform(0.0, 10.0, 80)]))
    p = mt.prolong(osys, sol.x, sol.y, q)
    assert np.array_equal(p[:, np.isin(q, sol.x)], sol.y)
    scale = np.max(np.abs(sol.y)) + np.max(np.diff(sol.x)) * np.max(np.abs(osys(sol.x, sol.y)))
    assert np.max(np.abs(p - sol.sol(q))) <= 16 * EPS * scale
    pl = mt.prolong(osys, sol.x, sol.y, q, mt.L)
    assert pl.dtype == mt.L and np.max(np.abs(pl - p)) <= 16 * EPS * scale


def outside_bands(r, tol):
    return not np.any(((r >= tol / 2) & (r <= 2 * tol)) | ((r >= 50 * tol) & (r <= 200 * tol)))


@pytest.mark.parametrize("case", mc.CASES, ids=lambda c: c.name)
def test_cases_are_robust(oracle, case):
    tw = case.twin(oracle)
    for k, r in enumerate(tw["rounds"]):
        print(f"{case.name} round {k + 1}: {r['mesh'].size} nodes, converged {r['converged'].tolist()}, rmsmax / tol "
              f"{np.array2string(r['rmsmax'] / case.tol, precision=3)}")
        assert outside_bands(r["rmsmax"], case.tol), (case.name, k)
    assert len(tw["rounds"]) == len(tw["meshes"]) and tw["mesh"].size == tw["meshes"][-1]


def test_cases_show_what_they_are_there_for(oracle):
    three = mc.THREE_ROUNDS.twin(oracle)
    assert len(three["meshes"]) >= 3 and three["mesh_status"] == 0 and three["rms_ok"].all()
    assert len(mc.THREE_ROUNDS_LOGISTIC.twin(oracle)["meshes"]) >= 3
    two = mc.TWO_NODES.twin(oracle)
    r0 = two["rounds"][0]
    assert (r0["rmsmax"] >= 100 * mc.TWO_NODES.tol).any() and two["meshes"][1] == two["meshes"][0] + 2 * int((r0["rmsmax"] >= 100 * mc.TWO_NODES.tol).sum())
    assert two["mesh_status"] == 2 and not two["converged"].any()      # (and ends where no instance converges on the new mesh)
    full = mc.MESH_FULL.twin(oracle)
    assert full["mesh_status"] == 1 and full["meshes"] == three["meshes"][:len(full["meshes"])] and full["meshes"][-1] <= 3
    assert len(full["meshes"]) >= 2 and not full["rms_ok"].all()
    rec = mc.FAILED_RECOVERS.twin(oracle)
    assert mc.FAILED_RECOVERS.cases[1].x0 == bc.NOT_CONVERGING.x0 and mc.FAILED_RECOVERS.options == {}
    assert [r["converged"].tolist() for r in rec["rounds"]] == [[True, False, True], [True, True, True], [True, True, True]]
    assert rec["rounds"][0]["solves"][1]["why"] == "line search" and np.isfinite(rec["rounds"][0]["solves"][1]["y"]).all()
    assert rec["meshes"] == [2, 4, 7] and rec["mesh_status"] == 1
    # the failed instance is masked: its own residual alone would ask for another mesh than the one taken
    r0 = rec["rounds"][0]
    assert np.array_equal(r0["rmsmax"], np.max(r0["rms"][:, [0, 2]], axis=1))
    stay = mc.FAILED_STAYS.twin(oracle)
    assert mc.FAILED_STAYS.cases[2].x0 == bc.NOT_CONVERGING.x0 and mc.FAILED_STAYS.options == {}
    assert [r["converged"].tolist() for r in stay["rounds"]] == [[True, True, False], [True, True, False]]
    assert stay["meshes"] == [2, 4] and stay["mesh_status"] == 1
    assert np.isfinite(stay["y"][2]).all() and not stay["rms_ok"][2]
    un = mc.UNION.twin(oracle)
    assert mc.UNION.cases[1].x0 == bc.NOT_CONVERGING.x0
    differs = False
    for r in un["rounds"][:-1]:
        both = mt.refine(r["mesh"], r["rmsmax"], mc.UNION.tol, 100 * mc.UNION.tol)
        own = [mt.refine(r["mesh"], r["rms"][:, b], mc.UNION.tol, 100 * mc.UNION.tol) for b in np.nonzero(r["converged"])[0]]
        differs = differs or (len(own) >= 2 and all(not np.array_equal(o, both) for o in own))
    assert differs
