"""GPU tests of fb_sweep_adaptive_batch against the twin's loop (tests/xlam_err_twin.py solve_adaptive on the cases of
tests/xlam_err_cases.py): the meshes bit for bit -- nodes are float64 mesh arithmetic alone, so they agree as long as every
refinement decision does, which the cases' distance from the thresholds guarantees -- and x, lam, J on the last mesh at the
tolerance of tests/test_gpu_fb_sweep.py."""
import warnings

import numpy as np
import pytest

from tests import xlam_err_cases as xc
from tests.test_gpu_fb_sweep import RTOL, relerr

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ocs():
    import torch
    assert torch.cuda.is_available()
    import __graft_entry__ as g
    return g.load_package()


def run(ocs, case, **extra):
    opts = dict(xc.OPTIONS, InitMesh=xc.MESH0, RelTol=xc.TOL, AbsTol=xc.TOL, **extra)
    with warnings.catch_warnings():
        warnings.simplefilter("error")                    # RelTol / AbsTol raise no warning here
        return ocs.fb_sweep_adaptive_batch(case.device_problem(ocs), case.x0, xc.MESH0[[0, -1]], opts)


@pytest.mark.parametrize("case", xc.CASES, ids=lambda c: c.name)
def test_adaptive_loop_takes_the_twins_meshes(ocs, oracle, case):
    tw = case.twin(oracle)
    assert xc.margin(tw) > 1e-6
    res = run(ocs, case)
    print(f"{case.name}: meshes {res['meshes']} (twin {tw['meshes']}), status {res['mesh_status']}, sweeps {res['sweeps'].tolist()}, "
          f"largest ratio {max(np.max(res['rx']), np.max(res['rl'])):.3f}, threshold margin of the twin {xc.margin(tw):.2e}")
    assert res["meshes"] == tw["meshes"] and np.array_equal(res["mesh"], tw["mesh"]) and np.array_equal(res["tspan"], tw["mesh"])
    assert np.array_equal(res["sweeps"], tw["sweeps"])
    assert res["mesh_status"] == 0 and res["err_ok"].all() and res["mesh"].size > xc.MESH0.size
    n = res["mesh"].size
    assert res["rx"].shape == (n - 1, 5) and res["ugrid"].shape == (1, 2 * n - 1, 5)
    for b in range(5):
        assert relerr(res["x"][:, :, b], tw["x"][:, :, b]) < RTOL and relerr(res["lam"][:, :, b], tw["lam"][:, :, b]) < RTOL
        assert abs(res["J"][b] - tw["J"][b]) < RTOL * abs(tw["J"][b])
    Jref = xc.j_reference(case, oracle, res["u"], res["mesh"], res["interpPts"])
    ratio = np.abs(res["J"] - Jref) / np.abs(res["errJ"])
    print(f"  |J - J_ref| / |errJ| = {np.array2string(ratio, precision=3)}; errJ {np.array2string(res['errJ'], precision=3)}")
    assert (np.abs(res["J"] - Jref) <= 10 * np.abs(res["errJ"]) + 1e-12 * np.abs(Jref)).all()


def test_max_mesh_size_stops_the_loop(ocs, oracle):
    case = xc.CASES[0]
    res = run(ocs, case, MAX_MESH_SIZE=15)
    assert res["mesh_status"] == 1 and res["meshes"] == [11] and np.array_equal(res["mesh"], xc.MESH0)
    assert res["x"].shape == (1, 11, 5) and res["rx"].shape == (10, 5) and not res["err_ok"].all()


def test_an_instance_that_never_converges_does_not_steer_the_mesh(ocs, oracle):
    """nSWEEPS = 1: nobody of the first case converges, mesh_status 2 on the first mesh.  Four instances whose control costs
    c = 1e12, so that ControlChar stays within uAbsTol of the start and they converge in their first sweep, beside one with
    c = 1.5 that cannot: the meshes are those of the four alone and of the twin, err_ok is false for the fifth."""
    case = xc.CASES[0]
    res = run(ocs, case, nSWEEPS=1)
    assert res["mesh_status"] == 2 and res["meshes"] == [11] and not res["err_ok"].any() and (res["sweeps"] == 0).all()
    hard = xc.Case("one-fails", 1, case.x0, [1e12] * 4 + [1.5])
    alone = xc.Case("four", 1, case.x0[:, :4], [1e12] * 4)
    tw = hard.twin(oracle, options={"nSWEEPS": 1})
    assert xc.margin(tw) > 1e-6
    r5, r4 = run(ocs, hard, nSWEEPS=1), run(ocs, alone, nSWEEPS=1)
    print(f"sweeps {r5['sweeps'].tolist()}, meshes {r5['meshes']} / without the failing instance {r4['meshes']}")
    assert r5["sweeps"].tolist() == [1, 1, 1, 1, 0] and r5["meshes"] == tw["meshes"] and np.array_equal(r5["mesh"], tw["mesh"])
    assert r5["meshes"] == r4["meshes"] and np.array_equal(r5["mesh"], r4["mesh"])
    assert r5["err_ok"].tolist() == [True, True, True, True, False] and r5["mesh_status"] == 0


def test_fb_sweep_batch_is_untouched(ocs, oracle):
    """fb_sweep_batch still warns on RelTol / AbsTol, and gives the same bits before and after an adaptive run and an estimate
    on the same handle"""
    case = xc.CASES[1]
    pr = case.device_problem(ocs)
    ts = np.linspace(0.0, 10.0, 41)
    gi = ocs.RK4Integrator(ts)
    before = ocs.fb_sweep_batch(pr, case.x0, ts, xc.OPTIONS, integrator=gi)
    ocs.fb_sweep_adaptive_batch(pr, case.x0, ts, dict(xc.OPTIONS, RelTol=1e-3, AbsTol=1e-3))
    ug = np.full((1, 81, 5), 0.3)
    ocs.x_lam_error(pr, ts, ug, before["x"], before["lam"], 1e-6, 1e-6, integrator=gi)
    with pytest.warns(RuntimeWarning, match="RelTol, AbsTol"):
        after = ocs.fb_sweep_batch(pr, case.x0, ts, dict(xc.OPTIONS, RelTol=1e-6, AbsTol=1e-6), integrator=gi)
    for k in ("x", "lam", "u", "J", "sweeps", "maxChange"):
        assert np.array_equal(before[k], after[k], equal_nan=True), k
