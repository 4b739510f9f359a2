"""Extended-precision twin of the grid forward-backward sweep (fb_sweep.m, compute_x_lam.m, compute_x_lam_J.m with odevr7 ->
RK4 on the grid), NumPy longdouble, vectorised over the batch.  Built on tests/rk4_twin.py: its problems (LogisticK, LQ), its
grid, its state pass and its error measure are used as they are.

Restated here, each from the reference lines the oracle (oracle/ocs_oracle.c) cites for the same piece:

    pchip_slopes, pchip_eval, pchip_mid   MATLAB's pchip (Moler, NCM pchiptx; vectorInterpolant.m:1-12): interior slopes the
                                          weighted harmonic mean, 0 where the secants differ in sign or vanish; end slopes the
                                          three-point formula with its two clamps; n = 2 linear; the Hermite cubic in s = q - t_k
    costate_pass                          compute_x_lam.m:4, :11-14: RK4 from node i+1 to node i with lam(TF) = 0 * x0,
                                          adjointRHS = -dFdx_times_vec(t, [x; 0], u, [lam; 1]) (make_from_symbolic.m:11-14), x at
                                          the nodes and at the pchip midpoints (compute_x_lam.m:9), u from the 2N+1 grid
    control_char                          make_from_symbolic.m:17-23, :111: the root of dHdu in u, clamped to the bounds
                                          (logistic: sum(lam) e^{rt} / (2c); LQ: -(Bu' lam) e^{rt} / (2 R))
    weighted_change                       fb_sweep.m:107-108
    compute_x_lam                         compute_x_lam_J.m:6-15 (the state pass on [x; running objective]) + the above
    sweeps                                fb_sweep.m:76-96 for exactly k sweeps from u0 = lower bound (:23): no convergence test
                                          (:110), no freezing

Data and arithmetic as in rk4_twin: the grid t, h = diff(tspan), the error and interpolation points, x0, u, the bounds, the
tolerances and the parameters are the given fp64 numbers; everything computed from them (node differences of pchip, secants,
slopes, e^{rt}, the stages) is carried in longdouble.

Shapes: x0 [nS][B], ugrid [nC][2N+1][B], x, lam [nS][N+1][B], cost [1][N+1][B], J [B], u at points [nC][nq][B],
maxChange [k][B]."""
import numpy as np

from tests import rk4_twin as tw
from tests.rk4_twin import EPS, LQ, WINDOW, L, LogisticK, compute_states, err, err_J, grid   # noqa: F401  (the twin's own)


_ld = tw._ld


def _sgn(v):
    return np.sign(v)


def pchip_slopes(t, y):
    """Slopes d [rows][n][B] of MATLAB's pchip through (t [n] fp64, y [rows][n][B])."""
    t, y = _ld(t), np.asarray(y, dtype=L)
    n = t.size
    h = np.diff(t)[None, :, None]
    dl = np.diff(y, axis=1) / h
    d = np.zeros_like(y)
    if n == 2:
        d[:, 0] = d[:, 1] = dl[:, 0]
        return d
    h0, h1 = h[:, :-1], h[:, 1:]
    d0, d1 = dl[:, :-1], dl[:, 1:]
    hs = h0 + h1
    w1, w2 = (h0 + hs) / (3 * hs), (hs + h1) / (3 * hs)
    a0, a1 = np.abs(d0), np.abs(d1)
    dmax, dmin = np.maximum(a0, a1), np.minimum(a0, a1)
    same = _sgn(d0) * _sgn(d1) > 0
    with np.errstate(divide="ignore", invalid="ignore"):
        inner = dmin / (w1 * (d0 / dmax) + w2 * (d1 / dmax))
    d[:, 1:-1] = np.where(same, inner, L(0))

    def end(ha, hb, da, db):       # ha, da: the end interval; hb, db: its neighbour
        e = ((2 * ha + hb) * da - ha * db) / (ha + hb)
        e = np.where(_sgn(e) != _sgn(da), L(0), e)
        return np.where((_sgn(e) == _sgn(da)) & (_sgn(da) != _sgn(db)) & (np.abs(e) > np.abs(3 * da)), 3 * da, e)
    d[:, 0] = end(h[:, 0], h[:, 1], dl[:, 0], dl[:, 1])
    d[:, -1] = end(h[:, -1], h[:, -2], dl[:, -1], dl[:, -2])
    return d


def pchip_eval(t, y, tq):
    """The pchip interpolant of (t, y [rows][n][B]) at tq [nq] fp64 -> [rows][nq][B].  Interval k with t_k <= q < t_{k+1},
    clamped to 0 .. n-2 (the end intervals extrapolate, as griddedInterpolant does)."""
    tf = np.asarray(t, dtype=np.float64)
    tq = np.atleast_1d(np.asarray(tq, dtype=np.float64))
    y = np.asarray(y, dtype=L)
    d = pchip_slopes(tf, y)
    k = np.clip(np.searchsorted(tf, tq, side="right") - 1, 0, tf.size - 2)
    tl = _ld(tf)
    h = (tl[k + 1] - tl[k])[None, :, None]
    s = (_ld(tq) - tl[k])[None, :, None]
    yk, dk, dk1 = y[:, k], d[:, k], d[:, k + 1]
    dl = (y[:, k + 1] - yk) / h
    dzzdx, dzdxdx = (dl - dk) / h, (dk1 - dl) / h
    c3, c2 = (dzdxdx - dzzdx) / h, 2 * dzzdx - dzdxdx
    return yk + s * (dk + s * (c2 + s * c3))


def pchip_mid(tspan, y):
    """pchip of the node values y [rows][N+1][B] at the interval middles of the grid (fp64 (t_i + t_{i+1}) / 2) -> [rows][N][B]"""
    t, _ = grid(tspan)
    return pchip_eval(t[0::2], y, t[1::2])


def adjoint_rhs(prob, t, x, lam, u):
    """-dFdx_times_vec(t, [x; 0], u, [lam; 1])(1:nS)"""
    y = np.concatenate([x, np.zeros((1,) + x.shape[1:], dtype=L)])
    v = np.concatenate([lam, np.ones((1,) + lam.shape[1:], dtype=L)])
    return -prob.dFdx_times_vec(t, y, u, v)[:-1]


def costate_pass(prob, tspan, x, xmid, ugrid):
    """lam [nS][N+1][B] from x [nS][N+1][B] at the nodes, xmid [nS][N][B] at the middles and ugrid [nC][2N+1][B]."""
    t, h = grid(tspan)
    x, xmid, u = np.asarray(x, dtype=L), np.asarray(xmid, dtype=L), _ld(ugrid)
    N = h.size
    lam = np.empty_like(x)
    lam[:, N] = 0
    for i in range(N - 1, -1, -1):
        hi = -L(h[i])
        tA, tM, tB = t[2 * i], t[2 * i + 1], t[2 * i + 2]
        uA, uM, uB = u[:, 2 * i], u[:, 2 * i + 1], u[:, 2 * i + 2]
        l = lam[:, i + 1]
        k1 = adjoint_rhs(prob, tB, x[:, i + 1], l, uB)
        k2 = adjoint_rhs(prob, tM, xmid[:, i], l + hi / 2 * k1, uM)
        k3 = adjoint_rhs(prob, tM, xmid[:, i], l + hi / 2 * k2, uM)
        k4 = adjoint_rhs(prob, tA, x[:, i], l + hi * k3, uA)
        lam[:, i] = l + hi / 6 * (k1 + 2 * k2 + 2 * k3 + k4)
    return lam


def control_char(prob, tq, lam, bounds):
    """ControlChar at the points tq [nq] for lam [nS][nq][B] -> [nC][nq][B], clamped to bounds [nC][2]."""
    lam = np.asarray(lam, dtype=L)
    e = np.exp(prob.r * _ld(tq)[:, None])[None]           # [1][nq][1 or B]
    if isinstance(prob, LogisticK):
        u = (np.sum(lam, axis=0) * e[0] / (2 * prob.c))[None]
    else:
        u = -np.einsum("sc,sqb->cqb", prob.Bu, lam) * e / (2 * prob.rd[:, None, :])     # rd [nC][1 or B]
    b = _ld(bounds).reshape(prob.nC, 2)
    return np.minimum(b[:, 1][:, None, None], np.maximum(b[:, 0][:, None, None], u))


def weighted_change(unew, u, rel_tol, abs_tol):
    """max over the controls and the error points of |uNew - u| / (uRelTol |u| + uAbsTol) -> [B]"""
    w = np.abs(unew - u) / (L(rel_tol) * np.abs(u) + L(abs_tol))
    return np.max(w, axis=(0, 1))


def compute_x_lam(prob, tspan, x0, ugrid):
    """(x [nS][N+1][B], cost [1][N+1][B], J [B], lam [nS][N+1][B]) for the control samples ugrid on the 2N+1 grid."""
    xa, J, _ = compute_states(prob, tspan, x0, ugrid)
    x = xa[:-1]
    lam = costate_pass(prob, tspan, x, pchip_mid(tspan, x), ugrid)
    return x, xa[-1:], J, lam


def control_from_x_lam(prob, tspan, lam, tq, bounds):
    """uNew(tq) = ControlChar(tq, x(tq), lam(tq)) with the pchip of the node values (fb_sweep.m:96); neither problem's
    ControlChar reads x."""
    nodes = np.asarray(tspan, dtype=np.float64).ravel()
    return control_char(prob, tq, pchip_eval(nodes, lam, tq), bounds)


def sweeps(prob, tspan, x0, k, error_pts, interp_pts, bounds, rel_tol=1e-7, abs_tol=1e-7):
    """Exactly k sweeps from u0 = lower bound.  Returns a dict: x, J, lam of sweep k (computed from the control of sweep
    k - 1), u = ControlChar of them at interp_pts, maxChange [k][B]; and for the tests of the regimes xK, the stage states of
    sweep k's state pass, ugrid_in, the control that pass integrated, and ugrid, the control sweep k leaves on the grid."""
    t, _ = grid(tspan)
    x0 = np.atleast_2d(np.asarray(x0, dtype=np.float64))
    B = x0.shape[1]
    lb = _ld(bounds).reshape(prob.nC, 2)[:, 0]
    u = np.broadcast_to(lb[:, None, None], (prob.nC, t.size, B)).astype(L)
    ue = np.broadcast_to(lb[:, None, None], (prob.nC, np.size(error_pts), B)).astype(L)
    mc = np.empty((k, B), dtype=L)
    for j in range(k):
        uin = u
        xa, J, xK = compute_states(prob, tspan, x0, u)     # (u stays longdouble from sweep to sweep: rk4_twin._ld keeps it)
        x = xa[:-1]
        lam = costate_pass(prob, tspan, x, pchip_mid(tspan, x), u)
        unew = control_from_x_lam(prob, tspan, lam, t, bounds)
        uenew = control_from_x_lam(prob, tspan, lam, error_pts, bounds)
        mc[j] = weighted_change(uenew, ue, rel_tol, abs_tol)
        u, ue = unew, uenew
    return {"x": x, "J": J, "lam": lam, "u": control_from_x_lam(prob, tspan, lam, interp_pts, bounds), "maxChange": mc,
            "xK": xK, "ugrid_in": uin, "ugrid": u}
