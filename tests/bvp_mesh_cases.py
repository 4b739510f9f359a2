"""The batches on which bvp_solver_adaptive_batch is held to the twin's loop (tests/bvp_mesh_twin.py solve_adaptive), shared
by tests/test_bvp_mesh_twin.py (CPU: every case is robust and shows what it is there for) and tests/test_gpu_bvp_mesh.py.
No test module: nothing is collected here.

Robust: in every round and on every interval the twin's rmsmax lies outside [tol / 2, 2 tol] and outside [50 tol, 200 tol],
so a difference in the last bits between the device's estimate and the twin's cannot move a node.  The residual estimates
of a mesh spread over decades, so this holds only on small meshes and for a tol picked between the values: the first meshes
have one to three intervals and the tolerances are coarse.  Found by a random search with the twin over x0, the horizon, the
first mesh T linspace(0, 1, n + 1)^power and tol.

BL-3 from x0 = .5 (bvp_cases.NOT_CONVERGING's instance) beside solvable neighbours, default Newton options: in FAILED_RECOVERS
its line search fails on the first mesh, it is masked out of rmsmax, prolonged as it stands and converges on the second mesh; in
FAILED_STAYS it fails on both meshes.  Their residuals keep the margins above for the rounds that run; MAX_MESH_SIZE ends
both loops where a later round would not (mesh_status 1).  It is also in the UNION batch, on whose horizon it converges.
"""
import numpy as np

from tests import bvp_cases as bc
from tests import bvp_mesh_twin as mt


class MeshCase:
    """instances: (kind, x0, c, ub) as tests/bvp_cases.py Case takes them, from the constant guess; the first mesh is
    T linspace(0, 1, n0 + 1)^power; options: those of the Newton solve (MaxIter, maxBacktracks), for the twin and the device"""

    def __init__(self, name, instances, T, n0, tol, power=1.0, max_nodes=1000, options=None):
        self.name, self.tol, self.max_nodes, self.options = name, tol, max_nodes, dict(options or {})
        self.mesh = T * np.linspace(0.0, 1.0, n0 + 1) ** power
        self.cases = [bc.Case(name, kind, x0, self.mesh, c=c, ub=ub) for kind, x0, c, ub in instances]
        self.memo = None

    def twin(self, oracle):
        """the twin's loop, once; do not write into the result"""
        if self.memo is None:
            self.memo = mt.solve_adaptive(self.cases, oracle, self.mesh, self.tol, self.max_nodes, **self.options)
        return self.memo


NOT_CONVERGING_X0 = bc.NOT_CONVERGING.x0                              # BL-3 from x0 = .5

THREE_ROUNDS = MeshCase("three rounds", [("bl3", [2.37], 1.5, 1.0)], 1.0, 1, 0.00662)
THREE_ROUNDS_LOGISTIC = MeshCase("three rounds, two states", [("logistic", [2.42, 1.8], 1.5, 1.0)], 1.0, 1, 0.00878)
TWO_NODES = MeshCase("two nodes in an interval", [("bl3", [2.17], 1.7, 0.3), ("bl3", [1.87], 1.7, 0.3)], 10.0, 1, 0.00064)
MESH_FULL = MeshCase("MAX_MESH_SIZE 3", [("bl3", [2.37], 1.5, 1.0)], 1.0, 1, 0.00662, max_nodes=3)
UNION = MeshCase("union of the instances' needs", [("bl3", [1.88], 1.5, 1.0), ("bl3", NOT_CONVERGING_X0, 1.5, 1.0), ("bl3", [2.18], 1.5, 1.0)],
                 1.0, 2, 0.00867, power=1.26)
FAILED_RECOVERS = MeshCase("a failed instance recovers", [("bl3", [2.48], 1.5, 1.0), ("bl3", NOT_CONVERGING_X0, 1.5, 1.0), ("bl3", [1.83], 1.5, 1.0)],
                           2.0, 1, 0.00102, max_nodes=7)
FAILED_STAYS = MeshCase("a failed instance stays failed", [("bl3", [1.93], 1.5, 1.0), ("bl3", [2.56], 1.5, 1.0), ("bl3", NOT_CONVERGING_X0, 1.5, 1.0)],
                        6.0, 1, 0.000127, max_nodes=4)
CASES = [FAILED_RECOVERS, FAILED_STAYS, THREE_ROUNDS, THREE_ROUNDS_LOGISTIC, TWO_NODES, MESH_FULL, UNION]
