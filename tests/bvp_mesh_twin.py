"""NumPy twin of the mesh side of the batched bvp_solver (csrc/ocs_bvp_device.hpp k_bvp_rms, k_bvp_prolong; solvers.py
bvp_solver_adaptive_batch): the residual estimate of a nodal solution, the refinement rule, the prolongation to the refined
mesh and the loop around tests/bvp_twin.py's Newton solve.  What it restates is scipy.integrate.solve_bvp's
estimate_rms_residuals / modify_mesh / its cubic spline; tests/test_bvp_mesh_twin.py holds it against those.

The residual estimate and the prolongation exist in float64 and in np.longdouble (`dtype`): the longdouble result is the
yardstick of the GPU tests, the float64 one says how far a float64 implementation may be from it.  What counts as data (the
same bits for every implementation, as in tests/rk4_twin.py): the mesh, h = diff(mesh), the interval middles, the Lobatto
times t_m -/+ (h/2) sqrt(3/7) formed in float64, y and the parameters.  Everything from there on is carried in `dtype`.

optSys is written here, not taken from the oracle (C, float64 only): OptSys below is the logistic family through the
adapter of functions/bvp_solver.m:105-109; test_bvp_mesh_twin.py checks its float64 form against the oracle's."""
import numpy as np

from tests import bvp_cases as bc
from tests import bvp_twin as bt

L = np.longdouble
assert np.finfo(L).nmant >= 63, "tests/bvp_mesh_twin.py needs an extended-precision long double (>= 64-bit significand)"


class OptSys:
    """y' = optSys(t, y), y = [x; lam], of  x_k' = x_k (m_k - x_k) - u,  cost' = e^{-rt} (sum x_k^2 + c u^2):
    u = clamp(sum(lam) e^{rt} / (2 c), lb, ub),  lam_k' = -((m_k - 2 x_k) lam_k + 2 e^{-rt} x_k)."""

    def __init__(self, m, c, r, lb, ub):
        self.m, self.c, self.r, self.lb, self.ub = [float(v) for v in m], float(c), float(r), float(lb), float(ub)
        self.nS = len(self.m)

    def control(self, t, y, dtype=np.float64):
        t, lam = np.asarray(t, dtype=np.float64).astype(dtype), y[self.nS:]
        s = lam[0]
        for k in range(1, self.nS):
            s = s + lam[k]
        return np.minimum(dtype(self.ub), np.maximum(dtype(self.lb), s * np.exp(dtype(self.r) * t) / (2 * dtype(self.c))))

    def __call__(self, t, y, dtype=np.float64):
        """t: k times (float64 data), y: 2nS x k in dtype"""
        y = np.asarray(y, dtype=dtype)
        td = np.asarray(t, dtype=np.float64).astype(dtype)
        m = np.array(self.m, dtype=dtype)[:, None]
        x, lam = y[:self.nS], y[self.nS:]
        u = self.control(t, y, dtype)
        return np.vstack([x * (m - x) - u, -((m - 2 * x) * lam + 2 * np.exp(-dtype(self.r) * td) * x)])


def optsys_of(case):
    """OptSys of a tests/bvp_cases.py Case"""
    m = [bc.BL3["m"]] if case.kind == "bl3" else bc.LOGISTIC_M[:case.nS]
    return OptSys(m, case.c, bc.BL3["r"], 0.0, case.ub)


def lobatto_times(tspan):
    """(t_-, t_+) [N] each, float64: t_m -/+ (h/2) sqrt(3/7)"""
    _, tm, h = bt.grid(tspan)
    d = h / 2 * np.sqrt(3.0 / 7.0)
    return tm - d, tm + d


def hermite_weights(th):
    """S = y_l + w (y_r - y_l) + h (a f_l - b f_r),  S' = dw (y_r - y_l) / h + da f_l + db f_r  at theta"""
    return (th * th * (3 - 2 * th), th * (1 - th) * (1 - th), th * th * (1 - th),
            6 * th * (1 - th), (1 - th) * (1 - 3 * th), th * (3 * th - 2))


def rms(osys, tspan, y, dtype=np.float64):
    """estimate_rms_residuals of solve_bvp for the nodal solution y (2nS x (N+1)) on tspan: [N] in dtype"""
    tn, tm, h64 = bt.grid(tspan)
    tlo, thi = lobatto_times(tspan)
    y, h = np.asarray(y, dtype=np.float64).astype(dtype), h64.astype(dtype)
    f = osys(tn, y, dtype)
    yl, yr, fl, fr = y[:, :-1], y[:, 1:], f[:, :-1], f[:, 1:]
    slope = (yr - yl) / h

    def norm2(sp, fs):
        q = (sp - fs) / (1 + np.abs(fs))
        return np.sum(q * q, axis=0)

    fm = osys(tm, dtype(0.5) * (yl + yr) + h / 8 * (fl - fr), dtype)
    rm = norm2(dtype(1.5) * slope - dtype(0.25) * (fl + fr), fm)
    s = np.sqrt(dtype(3) / dtype(7)) / 2
    rpm = 0
    for th, t in ((dtype(0.5) - s, tlo), (dtype(0.5) + s, thi)):
        w, a, b, dw, da, db = hermite_weights(th)
        fs = osys(t, yl + w * (yr - yl) + h * (a * fl - b * fr), dtype)
        rpm = rpm + norm2(dw * slope + da * fl + db * fr, fs)
    return np.sqrt(dtype(0.5) * (dtype(32) / dtype(45) * rm + dtype(49) / dtype(90) * rpm))


def refine(mesh, r, lo, hi):
    """One node in the middle of the intervals with lo < r < hi, two at the thirds of those with r >= hi; a NaN counts as the
    latter.  (tol, 100 tol) on the rms residuals: solve_bvp's rule and its modify_mesh; (1, 32) on the ratios of
    tests/xlam_err_twin.py."""
    x, r = np.asarray(mesh, dtype=np.float64), np.asarray(r, dtype=np.float64)
    r = np.where(np.isnan(r), np.inf, r)
    one = [i for i in range(r.size) if lo < r[i] < hi]
    two = [i for i in range(r.size) if r[i] >= hi]
    new = list(x) + [0.5 * (x[i] + x[i + 1]) for i in one] + [(2 * x[i] + x[i + 1]) / 3 for i in two] + \
        [(x[i] + 2 * x[i + 1]) / 3 for i in two]
    return np.array(sorted(new))


def locate(old, new):
    """interval index and theta = (t - t_i) / h_i (float64 data) of the points `new` on the mesh `old`; nodes of `old` get
    theta 0 (the last one theta 1 in the last interval)"""
    old, new = np.asarray(old, dtype=np.float64), np.asarray(new, dtype=np.float64)
    idx = np.array([min(max(int(np.sum(old <= t)) - 1, 0), old.size - 2) for t in new])
    return idx, (new - old[idx]) / (old[idx + 1] - old[idx])


def prolong(osys, tspan, y, new, dtype=np.float64):
    """The cubic Hermite interpolant of y (2nS x (N+1)) on tspan with the slopes optSys(t_i, y_i), at the points `new`:
    2nS x len(new) in dtype; old nodes are copied."""
    tn, _, h64 = bt.grid(tspan)
    idx, theta = locate(tspan, new)
    y = np.asarray(y, dtype=np.float64).astype(dtype)
    f = osys(tn, y, dtype)
    out = np.empty((y.shape[0], idx.size), dtype=dtype)
    for j, (i, th) in enumerate(zip(idx, theta)):
        if th == 0.0 or th == 1.0:
            out[:, j] = y[:, i if th == 0.0 else i + 1]
            continue
        w, a, b, _, _, _ = hermite_weights(dtype(th))
        out[:, j] = y[:, i] + w * (y[:, i + 1] - y[:, i]) + dtype(h64[i]) * (a * f[:, i] - b * f[:, i + 1])
    return out


def solve_adaptive(cases, oracle, mesh, tol, max_nodes=1000, **options):
    """The loop of bvp_solver_adaptive_batch on the instances `cases` (tests/bvp_cases.py Case: problem, x0, start; their
    tspan is not used) from the mesh `mesh`: solve every instance with bvp_twin.solve, estimate, refine where any converged
    instance asks for it, prolong every instance (the failed ones too), again.  Returns a dict: mesh, mesh_status (0 the
    tolerance holds, 1 the next mesh would exceed max_nodes, 2 no instance converged), meshes (node counts), y [2nS x (N+1)]
    per instance, converged, rms (N x batch), rms_ok, and rounds: per round its mesh, rmsmax, rms, the solves."""
    mesh = np.asarray(mesh, dtype=np.float64)
    osys = [optsys_of(c) for c in cases]
    start = [None if c.y0 is None else c.y0 for c in cases]
    rounds = []
    while True:
        sol = [bt.solve(c.problem(oracle), c.x0, mesh, y0=s, trace=True, **options) for c, s in zip(cases, start)]
        conv = np.array([s["converged"] for s in sol])
        with np.errstate(all="ignore"):
            r = np.stack([rms(o, mesh, s["y"]) for o, s in zip(osys, sol)], axis=1)
        rinf = np.where(np.isnan(r), np.inf, r)
        rmsmax = np.max(rinf[:, conv], axis=1) if conv.any() else np.zeros(mesh.size - 1)
        rounds.append({"mesh": mesh, "rms": r, "rmsmax": rmsmax, "solves": sol, "converged": conv})
        if not conv.any():
            status = 2
            break
        new = refine(mesh, rmsmax, tol, 100 * tol)
        if new.size == mesh.size:
            status = 0
            break
        if new.size > max_nodes:
            status = 1
            break
        with np.errstate(all="ignore"):
            start = [prolong(o, mesh, s["y"], new) for o, s in zip(osys, sol)]
        mesh = new
    return {"mesh": mesh, "mesh_status": status, "meshes": [r["mesh"].size for r in rounds], "y": [s["y"] for s in sol],
            "converged": conv, "rms": r, "rms_ok": conv & (np.max(rinf, axis=0) <= tol), "rounds": rounds}
