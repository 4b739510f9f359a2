"""NumPy twin of the batched bvp_solver (csrc/ocs_bvp_device.hpp, ocs_bvp.cpp), one instance at a time.

The same optSys (functions/bvp_solver.m:105-109 through the Gen-2 -> Gen-1 adapter, from the oracle's problem twins), the
same Simpson / Lobatto-IIIa residual with the boundary rows x_0 - x0 and lam_N, the same forward-difference Jacobian of
optSys and the same damping rule -- but the Newton system is assembled DENSE and solved with LAPACK, where the device
eliminates block by block over time: the two share no linear algebra."""
import numpy as np

SQRT_EPS = float(np.sqrt(np.finfo(np.float64).eps))


def grid(tspan):
    """Nodes and interval middles as RK4Integrator.m:21-24 lays them out: (tn [N+1], tm [N], h [N])."""
    tn = np.asarray(tspan, dtype=np.float64).ravel()
    h = np.diff(tn)
    return tn, tn[:-1] + h / 2, h


def optsys(prob, t, y):
    """value = optSys(t, y) for k columns: y is 2nS x k, t has k entries."""
    nS = prob.nS
    x, lam = y[:nS], y[nS:]
    u = prob.ControlChar(t, x, lam)
    return np.vstack([prob.stateRHS(t, x, u), prob.adjointRHS(t, x, lam, u)])


def fd_jacobian(prob, t, y, f):
    """J[r, c, j] = d optSys_r / d y_c at column j, forward differences with step sqrt(eps) max(1, |y_c|)."""
    nY, k = y.shape
    J = np.empty((nY, nY, k))
    for c in range(nY):
        step = SQRT_EPS * np.maximum(1.0, np.abs(y[c]))
        yp = y.copy()
        yp[c] = y[c] + step
        J[:, c, :] = (optsys(prob, t, yp) - f) / step
    return J


def residual(prob, x0, tspan, y, parts=False):
    """Phi(y): [x_0 - x0; Phi_0; ...; Phi_{N-1}; lam_N], y is 2nS x (N+1)."""
    nS = prob.nS
    tn, tm, h = grid(tspan)
    f = optsys(prob, tn, y)
    ym = 0.5 * (y[:, :-1] + y[:, 1:]) + h / 8 * (f[:, :-1] - f[:, 1:])
    fm = optsys(prob, tm, ym)
    phi = y[:, 1:] - y[:, :-1] - h / 6 * (f[:, :-1] + 4 * fm + f[:, 1:])
    r = np.concatenate([y[:nS, 0] - np.asarray(x0, dtype=np.float64).ravel(), phi.T.ravel(), y[nS:, -1]])
    return (r, f, ym, fm) if parts else r


def jacobian(prob, x0, tspan, y):
    """Dense dPhi/dy, unknowns ordered node by node, by the chain rule through y_m."""
    nS = prob.nS
    nY = 2 * nS
    tn, tm, h = grid(tspan)
    N = h.size
    _, f, ym, fm = residual(prob, x0, tspan, y, parts=True)
    Jn = fd_jacobian(prob, tn, y, f)
    Jm = fd_jacobian(prob, tm, ym, fm)
    n = nY * (N + 1)
    D = np.zeros((n, n))
    I = np.eye(nY)
    D[:nS, :nS] = np.eye(nS)
    for i in range(N):
        Jl, Jr, Jc = Jn[:, :, i], Jn[:, :, i + 1], Jm[:, :, i]
        L = -I - h[i] / 6 * (Jl + 4 * Jc @ (0.5 * I + h[i] / 8 * Jl))
        R = I - h[i] / 6 * (Jr + 4 * Jc @ (0.5 * I - h[i] / 8 * Jr))
        r0 = nS + nY * i
        D[r0:r0 + nY, nY * i:nY * (i + 1)] = L
        D[r0:r0 + nY, nY * (i + 1):nY * (i + 2)] = R
    D[n - nS:, n - nS:] = np.eye(nS)
    return D


def inverse_norm(prob, x0, tspan, y):
    """||J^{-1}||_inf of the Newton matrix at y: what a residual of size eps moves the root by, at most."""
    return float(np.linalg.norm(np.linalg.inv(jacobian(prob, x0, tspan, y)), np.inf))


def constant_guess(prob, x0, tspan):
    """bvpinit's constant guess [x0; 0] on the nodes (bvp_solver.m:87-89)."""
    n = np.asarray(tspan).size
    x0 = np.asarray(x0, dtype=np.float64).ravel()
    return np.vstack([np.repeat(x0[:, None], n, axis=1), np.zeros((prob.nS, n))])


def solve(prob, x0, tspan, y0=None, NewtonTol=1e-10, MaxIter=40, maxBacktracks=12, trace=False, jacobian=jacobian):
    """Damped Newton from y0 (default: the constant guess).  Returns a dict: y, converged, iterations, resnorm
    (||Phi||_inf of y) and why it stopped.  With `trace` also "trace": one dict per iteration with the iterate y after it,
    the accepted step length alpha (0.0 where the iteration failed and left y as it was) and resinf, res2 = ||Phi(y)||_inf,
    ||Phi(y)||_2; and "start": the same of y0 (alpha None).  `jacobian` replaces the Newton matrix (the tests of the twin
    pass deliberately wrong ones to show that their bounds notice)."""
    nY = 2 * prob.nS
    y = constant_guess(prob, x0, tspan) if y0 is None else np.array(y0, dtype=np.float64).reshape(nY, -1)
    r = residual(prob, x0, tspan, y)
    nrm = float(np.sqrt(np.sum(r * r)))
    out = {"iterations": 0, "converged": False, "why": "MaxIter"}
    steps = []

    def note(alpha):
        return {"y": y.copy(), "alpha": alpha, "resinf": float(np.max(np.abs(r))), "res2": nrm}

    start = note(None)
    if not np.isfinite(nrm):
        out["why"] = "non-finite start"
    elif np.max(np.abs(r)) <= NewtonTol:
        out["converged"], out["why"] = True, "start"
    else:
        for it in range(1, MaxIter + 1):
            out["iterations"] = it
            try:
                with np.errstate(all="ignore"):
                    d = np.linalg.solve(jacobian(prob, x0, tspan, y), -r)
            except np.linalg.LinAlgError:
                out["why"] = "singular"
                steps.append(note(0.0))
                break
            if not np.all(np.isfinite(d)):
                out["why"] = "non-finite step"
                steps.append(note(0.0))
                break
            d = d.reshape(-1, nY).T
            a, taken = 1.0, False
            for _ in range(maxBacktracks + 1):
                with np.errstate(all="ignore"):
                    rt = residual(prob, x0, tspan, y + a * d)
                    nt = float(np.sqrt(np.sum(rt * rt)))
                if np.isfinite(nt) and nt < (1.0 - 1e-4 * a) * nrm:
                    y, r, nrm, taken = y + a * d, rt, nt, True
                    break
                a *= 0.5
            steps.append(note(a if taken else 0.0))
            if not taken:
                out["why"] = "line search"
                break
            if np.max(np.abs(r)) <= NewtonTol:
                out["converged"], out["why"] = True, "NewtonTol"
                break
    out["y"], out["resnorm"] = y, float(np.max(np.abs(r)))
    if trace:
        out["trace"], out["start"] = steps, start
    return out


def step_noise(prob, x0, tspan, y, **options):
    """The twin's own sensitivity to a last-bit change of its input: one damped Newton step (solve with MaxIter = 1) from y
    and one from nextafter(y, inf); the largest difference of the two results.  The forward-difference quotient divides
    rounding errors of optSys by sqrt(eps) max(1, |y|), so this is far above one ulp, and no comparison of two float64
    implementations of the step can ask for less."""
    y = np.asarray(y, dtype=np.float64)
    a = solve(prob, x0, tspan, y0=y, **dict(options, MaxIter=1))["y"]
    b = solve(prob, x0, tspan, y0=np.nextafter(y, np.inf), **dict(options, MaxIter=1))["y"]
    return float(np.max(np.abs(a - b)))
