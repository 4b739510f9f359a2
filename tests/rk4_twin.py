"""Extended-precision twin of the RK4 pass pair (RK4Integrator.m:28-121), NumPy longdouble, vectorised over the batch.

A third statement of the recursion beside the oracle's C and the kernels, written from the reference's MATLAB text and
DESIGN.md in the plainest order: the state pass on the augmented state [x; running cost] with J = x(end, end) (:28-56), the
discrete adjoint with the default lamT = [0; ...; 0; 1] or a given one (:59-94), and dJdu with the reference's node /
midpoint split (:97-121).  Two right-hand sides:

    LogisticK (nS = 1..4)   x_k' = x_k (m_k - x_k) - u,      cost' = e^{-rt} (sum_k x_k^2 + c u^2)
    LQ                      x'   = A x + Bu u,               cost' = e^{-rt} (x'Qx + u'Ru),   Q = diag(q), R = diag(rdiag)

Every parameter but A and Bu may be given per trajectory (a trailing batch axis), so one batch can hold several r.

What counts as data and what as arithmetic: the grid t (nodes and interval middles) and h = diff(tspan) are formed in fp64
exactly as the constructor does (:16-25) -- they are inputs of the recursion, the same bits for every implementation -- and
x0, u, lamT and the parameters are the given fp64 numbers.  Everything from there on (h/2, h/6, h/3, e^{-rt}, the stages, the
sums) is carried in longdouble, which must have at least a 64-bit significand: a 53-bit "twin" would make every error
ratio formed against it meaningless, so the module refuses to import instead of skipping.

Arrays use the host shapes of the package: x0 [nS][B], u [nC][2N+1][B], x and lam [nS+1][N+1][B], dJdu [nC][2N+1][B], J [B].

`err` is the error measure of tests/test_gpu_rk4_accuracy.py and tests/test_rk4_twin.py (see its docstring)."""
import numpy as np

L = np.longdouble
assert np.finfo(L).nmant >= 63, (
    "tests/rk4_twin.py needs an extended-precision long double (>= 64-bit significand); this platform's has "
    f"{np.finfo(L).nmant + 1} bits")

EPS = 2.0 ** -53     # unit round-off of fp64
WINDOW = 4           # nodes either side: one chunk of the lane and scan kernels, half a pipeline block


def _ld(a):
    """fp64 data as longdouble; an array that is longdouble already (the control between two sweeps of tests/fbs_twin.py) as it is"""
    a = np.asarray(a)
    return a if a.dtype == L else a.astype(np.float64).astype(L)


def _per_traj(a, rows=None):
    """a shared scalar / vector or its per-trajectory form -> an array that broadcasts against [rows][B] (rows given) or [B]"""
    a = _ld(a)
    if rows is None:
        return a                                   # () or [B]
    if a.ndim == 0:
        a = np.full(rows, a, dtype=L)
    assert a.shape[0] == rows, (a.shape, rows)
    return a[:, None] if a.ndim == 1 else a        # [rows][1] or [rows][B]


class LogisticK:
    """tests/TestOCProblem.m:22-38 generalised to nS rows sharing one control (nS = 1 is TestOCProblem itself)."""

    def __init__(self, m, c, r):
        m = np.atleast_1d(np.asarray(m, dtype=np.float64))
        self.nS, self.nC = m.shape[0], 1
        self.m, self.c, self.r = _per_traj(m, self.nS), _per_traj(c), _per_traj(r)

    def disc(self, t):
        return np.exp(-self.r * L(t))

    def F(self, t, y, u):
        x, u = y[:-1], u[0]
        cost = self.disc(t) * (np.sum(x * x, axis=0) + self.c * u * u)
        return np.concatenate([x * (self.m - x) - u, np.broadcast_to(cost, (1,) + x.shape[1:])])

    def dFdx_times_vec(self, t, y, u, v):
        x = y[:-1]
        top = (self.m - 2 * x) * v[:-1] + self.disc(t) * (2 * x) * v[-1]
        return np.concatenate([top, np.zeros((1,) + x.shape[1:], dtype=L)])

    def dFdu_times_vec(self, t, y, u, v):
        return (-np.sum(v[:-1], axis=0) + self.disc(t) * (2 * self.c * u[0]) * v[-1])[None]


class LQ:
    """F = [A x + Bu u ; e^{-rt} (x'Qx + u'Ru)] with a shared Jacobian; q, rdiag and r may be per trajectory."""

    def __init__(self, A, Bu, q, rdiag, r):
        self.A, self.Bu = _ld(A), _ld(np.atleast_2d(Bu))
        self.nS, self.nC = self.Bu.shape
        self.q, self.rd, self.r = _per_traj(q, self.nS), _per_traj(rdiag, self.nC), _per_traj(r)

    def disc(self, t):
        return np.exp(-self.r * L(t))

    def F(self, t, y, u):
        x = y[:-1]
        cost = self.disc(t) * (np.sum(self.q * x * x, axis=0) + np.sum(self.rd * u * u, axis=0))
        return np.concatenate([self.A @ x + self.Bu @ u, np.broadcast_to(cost, (1,) + x.shape[1:])])

    def dFdx_times_vec(self, t, y, u, v):
        top = self.A.T @ v[:-1] + self.disc(t) * (2 * self.q * y[:-1]) * v[-1]
        return np.concatenate([top, np.zeros((1,) + top.shape[1:], dtype=L)])

    def dFdu_times_vec(self, t, y, u, v):
        return self.Bu.T @ v[:-1] + self.disc(t) * (2 * self.rd * u) * v[-1]


def grid(tspan):
    """RK4Integrator.m:16-25 in fp64: t (nodes and interval middles, 2N+1) and h = diff(tspan)."""
    tspan = np.asarray(tspan, dtype=np.float64).ravel()
    t = np.zeros(2 * tspan.size - 1)
    t[0::2] = tspan
    t[1::2] = (tspan[:-1] + tspan[1:]) / 2
    return t, np.diff(tspan)


def compute_states(prob, tspan, x0, u):
    """RK4Integrator.m:28-56.  Returns (x [nS+1][N+1][B], J [B], xK): xK[i] holds the four stage states of step i."""
    t, h = grid(tspan)
    x0, u = _ld(np.atleast_2d(x0)), _ld(u)
    N, B = h.size, x0.shape[1]
    x = np.empty((prob.nS + 1, N + 1, B), dtype=L)
    x[:-1, 0], x[-1, 0] = x0, 0
    xK = []
    for i in range(N):
        hi = L(h[i])
        y1 = x[:, i]
        F1 = prob.F(t[2 * i], y1, u[:, 2 * i])
        y2 = y1 + hi / 2 * F1
        F2 = prob.F(t[2 * i + 1], y2, u[:, 2 * i + 1])
        y3 = y1 + hi / 2 * F2
        F3 = prob.F(t[2 * i + 1], y3, u[:, 2 * i + 1])
        y4 = y1 + hi * F3
        F4 = prob.F(t[2 * i + 2], y4, u[:, 2 * i + 2])
        x[:, i + 1] = y1 + hi / 6 * (F1 + 2 * F2 + 2 * F3 + F4)
        xK.append((y1, y2, y3, y4))
    return x, x[-1, -1].copy(), xK


def compute_adjoints(prob, tspan, u, xK, lamT=None):
    """RK4Integrator.m:59-121 on the stage states of compute_states.  Returns (lam [nS+1][N+1][B], dJdu [nC][2N+1][B])."""
    t, h = grid(tspan)
    u = _ld(u)
    N, B = h.size, u.shape[2]
    lam = np.empty((prob.nS + 1, N + 1, B), dtype=L)
    if lamT is None:
        lam[:, N] = 0
        lam[-1, N] = 1
    else:
        lam[:, N] = _ld(lamT)
    dJdu = np.zeros((prob.nC, 2 * N + 1, B), dtype=L)
    k1_of_next = None                              # dFdu'k1 of step i + 1: the other half of node column 2(i + 1)
    for i in range(N - 1, -1, -1):
        hi = L(h[i])
        y1, y2, y3, y4 = xK[i]
        tA, tM, tB = t[2 * i], t[2 * i + 1], t[2 * i + 2]
        uA, uM, uB = u[:, 2 * i], u[:, 2 * i + 1], u[:, 2 * i + 2]
        ln = lam[:, i + 1]
        k4 = hi / 6 * ln
        d3 = prob.dFdx_times_vec(tB, y4, uB, k4)
        k3 = hi / 3 * ln + hi * d3
        d2 = prob.dFdx_times_vec(tM, y3, uM, k3)
        k2 = hi / 3 * ln + hi / 2 * d2
        d1 = prob.dFdx_times_vec(tM, y2, uM, k2)
        k1 = hi / 6 * ln + hi / 2 * d1
        lam[:, i] = ln + d1 + d2 + d3 + prob.dFdx_times_vec(tA, y1, uA, k1)
        # :97-121 -- middles: k2 and k3 of the step; inner nodes: k1 of the step that starts there + k4 of the one that ends there
        dJdu[:, 2 * i + 1] = prob.dFdu_times_vec(tM, y2, uM, k2) + prob.dFdu_times_vec(tM, y3, uM, k3)
        right = prob.dFdu_times_vec(tB, y4, uB, k4)
        dJdu[:, 2 * i + 2] = right if k1_of_next is None else k1_of_next + right
        k1_of_next = prob.dFdu_times_vec(tA, y1, uA, k1)
    dJdu[:, 0] = k1_of_next
    return lam, dJdu


def passes(prob, tspan, x0, u, lamT):
    """Both passes, the adjoint with the default and with the explicit lamT: a dict of longdouble arrays
    x [nS][N+1][B], cost [1][N+1][B], J [B], lam, lam2 [nS+1][N+1][B], dJdu, d2 [nC][2N+1][B], and xK (the stage states)."""
    x, J, xK = compute_states(prob, tspan, x0, u)
    lam, dJdu = compute_adjoints(prob, tspan, u, xK)
    lam2, d2 = compute_adjoints(prob, tspan, u, xK, lamT)
    return {"x": x[:-1], "cost": x[-1:], "J": J, "lam": lam, "dJdu": dJdu, "lam2": lam2, "d2": d2, "xK": xK}


def err(v, ref):
    """The local error of v [rows][cols][B] against ref (longdouble), one number per trajectory:

        err[i] = |v_i - ref_i| / max_{|j - i| <= 4} |ref_j|        i over the time axis, maximum over i and the rows

    The scale of an entry is the largest reference magnitude within +-4 columns of it, over the rows of the array: local in
    time, so the small part of a trajectory (a discounted tail, the start of a growing state) is held to its own size, but not
    componentwise across rows -- rows that are coupled through the dynamics are judged on their common scale, which is all any
    algorithm delivers.  Where the scale is 0 the entry must be exactly equal (else inf).  Non-finite values give inf."""
    ref = np.asarray(ref, dtype=L)
    d = np.abs(np.asarray(v).astype(L) - ref)
    a = np.max(np.abs(ref), axis=0)                             # [cols][B]
    n = a.shape[0]
    pad = np.concatenate([np.zeros((WINDOW,) + a.shape[1:], dtype=L), a, np.zeros((WINDOW,) + a.shape[1:], dtype=L)])
    scale = np.max(np.stack([pad[k:k + n] for k in range(2 * WINDOW + 1)]), axis=0)
    d = np.max(d, axis=0)
    with np.errstate(divide="ignore", invalid="ignore"):
        e = np.where(scale > 0, d / scale, np.where(d == 0, L(0), L(np.inf)))
    e = np.where(np.isfinite(e), e, L(np.inf))
    return np.max(e, axis=0).astype(np.float64)                 # [B]


def err_J(J, ref):
    """|J - ref| / |ref| per trajectory."""
    ref = np.asarray(ref, dtype=L)
    e = np.abs(np.asarray(J).astype(L) - ref) / np.abs(ref)
    return np.where(np.isfinite(e), e, L(np.inf)).astype(np.float64)


OUTPUTS = ("x", "cost", "J", "lam", "dJdu", "lam2", "d2")


def errors(got, ref):
    """err of every output of a pass pair, per trajectory: got holds fp64 arrays x [nS+1][N+1][B] (cost row last), J, lam,
    dJdu, lam2, d2 in the package's host shapes; ref is the dict of passes().  Returns {output: [B]}.  The last row of lam is the
    multiplier of the cost row, constant in time (dF/dy has a zero last column, :86): it must equal lamT's entry exactly and
    stays out of the scale of the state rows, which it would otherwise pin at 1."""
    x = np.asarray(got["x"])
    out = {"x": err(x[:-1], ref["x"]), "cost": err(x[-1:], ref["cost"]), "J": err_J(got["J"], ref["J"])}
    for k in ("lam", "lam2"):
        lam = np.asarray(got[k])
        exact = np.all(lam[-1] == ref[k][-1].astype(np.float64), axis=0)
        out[k] = np.where(exact, err(lam[:-1], ref[k][:-1]), np.inf)
    for k in ("dJdu", "d2"):
        out[k] = err(got[k], ref[k])
    return out


def relerr_old(a, b):
    """The measure of the parity tests (tests/test_gpu_rk4_parity.py): max |a - b| / max(1, |b|)."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.max(np.abs(a - b) / np.maximum(1.0, np.abs(b))))
