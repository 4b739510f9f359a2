"""The batches tests/test_gpu_fb_sweep_adaptive.py runs through fb_sweep_adaptive_batch, with the twin's loop
(tests/xlam_err_twin.py solve_adaptive, the oracle's fb_sweep as the sweep) computed once per case.  Chosen on the CPU so that
in the twin no interval's rmax of any round lies within a relative 1e-3 of 1 or 32 (the test asserts 1e-6): `margin` reports
the distance.  (On the first mesh of logistic1 four of the five instances use up their 50 sweeps: the mesh of that round
follows the fifth alone.)"""
import numpy as np

from tests import rk4_twin as tw
from tests import xlam_err_twin as xt

BOUNDS = [[0.0, 1.0]]
R = 0.05
M = [3.0, 2.5]
TOL = 1e-5
MESH0 = np.linspace(0.0, 10.0, 11)
OPTIONS = {"nERROR_PTS": 101, "nINTERP_PTS": 201}


class Case:
    def __init__(self, name, nS, x0, c):
        self.name, self.nS = name, nS
        self.x0, self.c = np.asarray(x0, dtype=np.float64), np.asarray(c, dtype=np.float64)
        self._twin = {}

    def oracle_problems(self, oracle):
        return [oracle.LogisticProblem(M[:self.nS], c, R, BOUNDS) for c in self.c]

    def twin_problems(self):
        return [tw.LogisticK(M[:self.nS], c, R) for c in self.c]

    def device_problem(self, ocs):
        p = ocs.LogisticProblem(M[:self.nS], 1.5, R, BOUNDS)
        p.set_batch_params([0], self.c[None, :])
        return p

    def twin(self, oracle, options=None, max_nodes=20000):
        key = (tuple(sorted((options or {}).items())), max_nodes)
        if key not in self._twin:
            self._twin[key] = xt.solve_adaptive(oracle, self.oracle_problems(oracle), self.twin_problems(), self.x0, MESH0, TOL, TOL,
                                                dict(OPTIONS, **(options or {})), max_nodes)
        return self._twin[key]


CASES = [
    Case("logistic1", 1, [[0.6, 1.1, 1.6, 2.1, 2.4]], [1.1, 1.3, 1.5, 1.7, 1.9]),
    Case("logistic2", 2, [[0.6, 1.1, 1.6, 2.1, 2.4], [2.2, 1.8, 1.2, 0.9, 0.7]], [1.1, 1.3, 1.5, 1.7, 1.9]),
]


def margin(tw_result):
    """the smallest relative distance of any round's rmax from the thresholds 1 and 32"""
    r = np.concatenate([rd["rmax"] for rd in tw_result["rounds"]])
    r = r[np.isfinite(r) & (r > 0)]
    if r.size == 0:
        return np.inf
    return float(min(np.min(np.abs(r - 1.0)), np.min(np.abs(r - 32.0) / 32.0)))


def j_reference(case, oracle, res_u, mesh, interp_pts):
    """J_ref per instance: the twin's compute_x_lam on `mesh` with every interval split in four, ugrid the pchip of the
    returned u (res_u [nC][nI][B] on interp_pts)"""
    fine = np.unique(np.concatenate([mesh] + [mesh[:-1] + k * np.diff(mesh) / 4 for k in (1, 2, 3)]))
    t, _ = tw.grid(fine)
    out = []
    for b, p in enumerate(case.twin_problems()):
        ug = oracle.vector_interp(interp_pts, res_u[:, :, b], oracle.INTERP_PCHIP, t)
        out.append(float(tw.compute_states(p, fine, case.x0[:, b:b + 1], ug[:, :, None])[1][0]))
    return np.array(out)
