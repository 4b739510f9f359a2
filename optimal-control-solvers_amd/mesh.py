"""Mesh adaptation shared by the error-controlled drivers (solvers.bvp_solver_adaptive_batch, sweep.fb_sweep_adaptive_batch):
the refinement rule, the loop around a round of solving and estimating, where the nodes of one mesh lie on another, and the
argument shaping the drivers and their estimates have in common.  It imports neither of the two modules."""
from __future__ import annotations

import numpy as np

from ._lib import ip
from .integrator import RK4Integrator
from .problem import _f


def refine_mesh(mesh, r, lo, hi):
    """One node in the middle of the intervals with lo < r < hi, two at the thirds of those with r >= hi (a NaN counts as
    such).  r: one ratio per interval.  The bvp driver passes (tol, 100 tol), solve_bvp's rule and its modify_mesh; the sweep
    driver (1, 32): the local error of an RK4 step falls by 32 when the step is halved.  Returns the new mesh, sorted; nodes are
    only added."""
    mesh, r = np.asarray(mesh, dtype=np.float64), np.asarray(r, dtype=np.float64)
    r = np.where(np.isnan(r), np.inf, r)
    i1, = np.nonzero((r > lo) & (r < hi))
    i2, = np.nonzero(r >= hi)
    return np.sort(np.hstack((mesh, 0.5 * (mesh[i1] + mesh[i1 + 1]), (2 * mesh[i2] + mesh[i2 + 1]) / 3,
                              (mesh[i2] + 2 * mesh[i2 + 1]) / 3)))


def adapt_mesh(mesh, max_nodes, lo, hi, solve_round):
    """The loop of both drivers.  solve_round(mesh, integ) solves and estimates on `mesh` (integ = RK4Integrator(mesh)) and
    returns (res, conv, rmax, restart): the round's result dict, the instances that converged, the largest ratio per interval
    over them, and restart(new), which makes the next round start from this one's solution on the mesh `new`.  The batch shares
    the mesh.  Returns the last round's res with meshes (the node count of every round) and mesh_status -- 2: no instance
    converged on a mesh; 0: refine_mesh(mesh, rmax, lo, hi) adds nothing; 1: the next mesh would exceed max_nodes."""
    meshes = []
    while True:
        integ = RK4Integrator(mesh)
        res, conv, rmax, restart = solve_round(mesh, integ)
        meshes.append(int(mesh.size))
        if not conv.any():
            status = 2
            break
        new = refine_mesh(mesh, rmax, lo, hi)
        if new.size == mesh.size:
            status = 0
            break
        if new.size > max_nodes:
            status = 1
            break
        restart(new)
        del integ, restart                           # (the handle's workspace goes with it: restart may hold it too)
        mesh = new
    res.update(meshes=meshes, mesh_status=status)
    return res


def _prolong_map(old, new):
    """Where the nodes of `new` lie on the mesh `old`: (idx int32, theta) with new = old[idx] + theta (old[idx + 1] - old[idx]),
    0 <= theta <= 1; a node of `old` has theta 0 (the last one: theta 1 in the last interval)."""
    old, new = np.asarray(old, dtype=np.float64), np.asarray(new, dtype=np.float64)
    idx = np.clip(np.searchsorted(old, new, side="right") - 1, 0, old.size - 2)
    theta = (new - old[idx]) / (old[idx + 1] - old[idx])
    return np.ascontiguousarray(idx, dtype=np.int32), np.ascontiguousarray(theta)


def use_flags(use, batch):
    """The `use` argument of the estimates (batch flags, or None: all) as (int32 array, its ctypes pointer) or (None, None)"""
    if use is None:
        return None, None
    use = np.ascontiguousarray(np.asarray(use).ravel() != 0, dtype=np.int32)
    if use.size != batch:
        raise ValueError(f"use: expected {batch} flags, got {use.size}")
    return use, use.ctypes.data_as(ip)


def x0_batch(prob, x0):
    """x0 of the batch drivers (nS values, nS x batch, or anything that reshapes to it) as an nS x batch Fortran array"""
    x0 = _f(np.atleast_2d(np.asarray(x0, dtype=np.float64)))
    if x0.shape[0] != prob.nS:
        x0 = _f(x0.reshape(prob.nS, -1))
    return x0
