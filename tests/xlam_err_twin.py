"""NumPy twin of the error estimate of the sweep's pass pair (csrc/ocs_xlam_err_device.hpp k_xlam_err and its reduction;
include/ocs.h ocs_x_lam_err) and of the loop fb_sweep_adaptive_batch (sweep.py) around it.

The estimate exists in float64 and in np.longdouble (`dtype`): the longdouble result is the yardstick of the GPU tests, the
float64 one says how far a float64 implementation may be from it.  Built on tests/rk4_twin.py and tests/fbs_twin.py: their
grid, their problems (LogisticK, LQ) and, in tests/test_xlam_err_twin.py, their pchip, state pass and costate pass, to which
the pieces restated here in `dtype` are held.  What counts as data (the same bits for every implementation, as in
rk4_twin): the grid t, h = diff(tspan), the spacings diff(t) of the 2N+1 grid, the quarter points t_i + h/4, t_i + 3h/4 and
their local coordinates, t_mid - t_i, all formed in float64; ugrid, x, lam, the tolerances and the parameters.  Everything
from there on is carried in `dtype`.

Shapes as in fbs_twin: ugrid [nC][2N+1][B], x, lam [nS][N+1][B]; rx, rl [N][B]."""
import copy

import numpy as np

from tests import fbs_twin as ft
from tests import rk4_twin as tw
from tests.bvp_mesh_twin import refine

L = tw.L
CHUNK = 8            # intervals per partial sum of errJ (kErrChunk)


def as_dtype(prob, dtype):
    """the rk4_twin problem itself (longdouble), or a copy that computes in float64: parameters cast back to the float64 they
    were given as, e^{-rt} in float64"""
    if dtype is L:
        return prob
    q = copy.copy(prob)
    for k, v in vars(prob).items():
        if isinstance(v, np.ndarray) and v.dtype == L:
            setattr(q, k, v.astype(np.float64))
    q.disc = lambda t: np.exp(-q.r * np.float64(t))
    return q


def slopes(h, y, dtype):
    """fbs_twin.pchip_slopes in dtype, with the spacings h [n-1] given (float64 data): d [rows][n][B]"""
    y = np.asarray(y, dtype=dtype)
    n = y.shape[1]
    h = np.asarray(h, dtype=np.float64).astype(dtype)[None, :, None]
    dl = np.diff(y, axis=1) / h
    d = np.zeros_like(y)
    if n == 2:
        d[:, 0] = d[:, 1] = dl[:, 0]
        return d
    h0, h1, d0, d1 = h[:, :-1], h[:, 1:], dl[:, :-1], dl[:, 1:]
    hs = h0 + h1
    w1, w2 = (h0 + hs) / (3 * hs), (hs + h1) / (3 * hs)
    a0, a1 = np.abs(d0), np.abs(d1)
    dmax, dmin = np.maximum(a0, a1), np.minimum(a0, a1)
    with np.errstate(divide="ignore", invalid="ignore"):
        inner = dmin / (w1 * (d0 / dmax) + w2 * (d1 / dmax))
    d[:, 1:-1] = np.where(np.sign(d0) * np.sign(d1) > 0, inner, dtype(0))

    def end(ha, hb, da, db):
        e = ((2 * ha + hb) * da - ha * db) / (ha + hb)
        e = np.where(np.sign(e) != np.sign(da), dtype(0), e)
        return np.where((np.sign(e) == np.sign(da)) & (np.sign(da) != np.sign(db)) & (np.abs(e) > np.abs(3 * da)), 3 * da, e)
    d[:, 0] = end(h[:, 0], h[:, 1], dl[:, 0], dl[:, 1])
    d[:, -1] = end(h[:, -1], h[:, -2], dl[:, -1], dl[:, -2])
    return d


def piece(v0, v1, dk, dk1, h, s):
    """the cubic Hermite piece of fbs_twin.pchip_eval on an interval of length h at the local coordinate s"""
    dl = (v1 - v0) / h
    dzzdx, dzdxdx = (dl - dk) / h, (dk1 - dl) / h
    c3, c2 = (dzdxdx - dzzdx) / h, 2 * dzzdx - dzdxdx
    return v0 + s * (dk + s * (c2 + s * c3))


def quarter_points(tspan):
    """(tq [2N], sq [2N]) float64: t_i + h/4 and t_i + 3h/4, and their local coordinates in the grid intervals 2i, 2i+1"""
    t, h = tw.grid(tspan)
    tq = np.empty(2 * h.size)
    tq[0::2], tq[1::2] = t[0:-1:2] + 0.25 * h, t[0:-1:2] + 0.75 * h
    sq = np.empty_like(tq)
    sq[0::2], sq[1::2] = tq[0::2] - t[0:-1:2], tq[1::2] - t[1::2]
    return tq, sq


def control_quarters(tspan, ugrid, dtype=L):
    """the pchip of the 2N+1 samples on the grid t at the quarter points: (u1, u3) [nC][N][B] each"""
    t, _ = tw.grid(tspan)
    _, sq = quarter_points(tspan)
    u = np.asarray(ugrid, dtype=np.float64).astype(dtype)
    hg = np.diff(t)
    du = slopes(hg, u, dtype)
    hg, sq = hg.astype(dtype)[None, :, None], sq.astype(dtype)[None, :, None]
    u1 = piece(u[:, 0:-1:2], u[:, 1::2], du[:, 0:-1:2], du[:, 1::2], hg[:, 0::2], sq[:, 0::2])
    u3 = piece(u[:, 1::2], u[:, 2::2], du[:, 1::2], du[:, 2::2], hg[:, 1::2], sq[:, 1::2])
    return u1, u3


def state_step(P, y, hs, F1, tM, uM, tB, uB, dtype):
    """one RK4 step of the augmented state over hs whose first stage is given"""
    c = lambda v: np.asarray(v).astype(dtype)
    F2 = c(P.F(tM, y + hs / 2 * F1, uM))
    F3 = c(P.F(tM, y + hs / 2 * F2, uM))
    F4 = c(P.F(tB, y + hs * F3, uB))
    return y + hs / 6 * (F1 + 2 * F2 + 2 * F3 + F4)


def costate_step(P, l, hs, B, M, A, dtype):
    """one RK4 step of the costate backward over hs: B, M, A = (t, x, u) at the start, the middle and the end of the step"""
    def rhs(p, lam):
        t, x, u = p
        return np.asarray(ft.adjoint_rhs(P, t, x, lam, u)).astype(dtype)
    k1 = rhs(B, l)
    k2 = rhs(M, l - hs / 2 * k1)
    k3 = rhs(M, l - hs / 2 * k2)
    k4 = rhs(A, l - hs * k3)
    return l - hs / 6 * (k1 + 2 * k2 + 2 * k3 + k4)


def estimate(prob, tspan, ugrid, x, lam, rtol, atol, dtype=L, hermite=True):
    """The estimate of ocs_x_lam_err.  Returns a dict in dtype: ex, el [nS][N][B] (16/15 |fine - coarse| per row), dJ [N][B],
    rx, rl [N][B], errJ [B], and for the tests the scales sx, sl [N][B] (max over the rows of max(|v_i|, |v_{i+1}|)) and the
    smallest denominators denx, denl [N][B].  hermite = False takes the states of the fine costate steps from the pchip of the
    node values instead (what the estimate would be blind to)."""
    t, h64 = tw.grid(tspan)
    tq, _ = quarter_points(tspan)
    N = h64.size
    P = as_dtype(prob, dtype)
    c = lambda v: np.asarray(v).astype(dtype)
    u = np.asarray(ugrid, dtype=np.float64).astype(dtype)
    x, lam = np.asarray(x, dtype=np.float64).astype(dtype), np.asarray(lam, dtype=np.float64).astype(dtype)
    u1, u3 = control_quarters(tspan, ugrid, dtype)
    dx = slopes(h64, x, dtype)
    B = x.shape[2]
    zero = np.zeros((1, B), dtype=dtype)
    ex, el, dJ = np.empty((x.shape[0], N, B), dtype=dtype), np.empty((x.shape[0], N, B), dtype=dtype), np.empty((N, B), dtype=dtype)
    for i in range(N):
        h = dtype(h64[i])
        tA, tM, tB, t1, t3 = t[2 * i], t[2 * i + 1], t[2 * i + 2], tq[2 * i], tq[2 * i + 1]
        uA, uM, uB = u[:, 2 * i], u[:, 2 * i + 1], u[:, 2 * i + 2]
        xA, xB = x[:, i], x[:, i + 1]
        yA = np.concatenate([xA, zero])
        fA = c(P.F(tA, yA, uA))
        yc = state_step(P, yA, h, fA, tM, uM, tB, uB, dtype)
        ym = state_step(P, yA, h / 2, fA, t1, u1[:, i], tM, uM, dtype)
        fm = c(P.F(tM, ym, uM))
        yf = state_step(P, ym, h / 2, fm, t3, u3[:, i], tB, uB, dtype)
        fB = c(P.F(tB, np.concatenate([xB, zero]), uB))
        ex[:, i] = dtype(16) / 15 * np.abs(yf[:-1] - yc[:-1])
        dJ[i] = dtype(16) / 15 * ((yc[-1] - yf[-1]) + np.sum(lam[:, i + 1] * (yc[:-1] - yf[:-1]), axis=0))
        xm = ym[:-1]
        xM = piece(xA, xB, dx[:, i], dx[:, i + 1], h, dtype(t[2 * i + 1] - t[2 * i]))
        if hermite:
            x1 = (xA + xm) / 2 + h / 16 * (fA[:-1] - fm[:-1])
            x3 = (xm + xB) / 2 + h / 16 * (fm[:-1] - fB[:-1])
            xmf = xm
        else:        # the pchip of the node values everywhere between the nodes
            x1 = piece(xA, xB, dx[:, i], dx[:, i + 1], h, dtype(tq[2 * i] - t[2 * i]))
            x3 = piece(xA, xB, dx[:, i], dx[:, i + 1], h, dtype(tq[2 * i + 1] - t[2 * i]))
            xmf = xM
        lB = lam[:, i + 1]
        lc = costate_step(P, lB, h, (tB, xB, uB), (tM, xM, uM), (tA, xA, uA), dtype)
        lm = costate_step(P, lB, h / 2, (tB, xB, uB), (t3, x3, u3[:, i]), (tM, xmf, uM), dtype)
        lf = costate_step(P, lm, h / 2, (tM, xmf, uM), (t1, x1, u1[:, i]), (tA, xA, uA), dtype)
        el[:, i] = dtype(16) / 15 * np.abs(lf - lc)
    rt, at = dtype(rtol), dtype(atol)
    out = {"ex": ex, "el": el, "dJ": dJ}
    for name, e, v in (("x", ex, x), ("l", el, lam)):
        sc = np.maximum(np.abs(v[:, :-1]), np.abs(v[:, 1:]))
        den = at + rt * sc
        out["r" + name], out["s" + name], out["den" + name] = np.max(e / den, axis=0), np.max(sc, axis=0), np.min(den, axis=0)
    out["errJ"] = sum_in_order(np.stack([sum_in_order(dJ[k:k + CHUNK]) for k in range(0, N, CHUNK)]))
    return out


def sum_in_order(a):
    """a[0] + a[1] + ... from 0.0, left to right"""
    s = np.zeros(a.shape[1:], dtype=a.dtype)
    for row in a:
        s = s + row
    return s


def reductions(rx, rl, use=None):
    """(rmax [N], rinst [B]) of ocs_x_lam_err from the ratios: a NaN counts as inf; rmax over the instances in use (none: 0)"""
    r = np.maximum(np.asarray(rx, dtype=np.float64), np.asarray(rl, dtype=np.float64))
    r = np.where(np.isnan(r), np.inf, r)
    use = np.ones(r.shape[1], dtype=bool) if use is None else np.asarray(use).astype(bool)
    rmax = np.max(r[:, use], axis=1) if use.any() else np.zeros(r.shape[0])
    return rmax, np.max(r, axis=0)


def solve_adaptive(oracle, oprobs, tprobs, x0, mesh, rtol, atol, options, max_nodes=20000):
    """The loop of fb_sweep_adaptive_batch with the oracle's fb_sweep as the sweep: oprobs / tprobs the oracle's and the twin's
    problem of every instance, x0 [nS][B].  Returns a dict: mesh, mesh_status, meshes, sweeps [B], x, lam [nS][N+1][B], J,
    errJ [B], u [nC][nI][B], ugrid, rx, rl, err_ok, and rounds: per round its mesh, rmax, sweeps."""
    mesh = np.asarray(mesh, dtype=np.float64)
    x0 = np.asarray(x0, dtype=np.float64)
    nB = x0.shape[1]
    start = [None] * nB
    rounds = []
    while True:
        integ = oracle.RK4Integrator(mesh)
        sol, per = [], []
        for b in range(nB):
            opt = dict(options)
            if start[b] is not None:
                pts, ub = start[b]
                opt["u0"] = lambda tq, pts=pts, ub=ub: oracle.vector_interp(pts, ub, oracle.INTERP_PCHIP, tq)
            s = oracle.fb_sweep(oprobs[b], x0[:, b], mesh, opt)
            sol.append(s)
            pts = s["_interpPts"]
            # (an instance that did not converge has no u: its passes run under the lower bound, whatever -- it is not in use)
            ub = s["u"] if s["_sweeps"] > 0 else np.repeat(oprobs[b].ControlBounds[:, 0:1], pts.size, axis=1)
            ug = oracle.vector_interp(pts, ub, oracle.INTERP_PCHIP, integ.t)
            xb, lb, Jb = oracle.compute_x_lam(integ, oprobs[b], x0[:, b], ug, want_J=True)
            e = estimate(tprobs[b], mesh, ug[:, :, None], xb[:, :, None], lb[:, :, None], rtol, atol, np.float64)
            per.append((ub, ug, xb, lb, Jb, e))
        sweeps = np.array([s["_sweeps"] for s in sol])
        conv = sweeps > 0
        rx = np.stack([p[5]["rx"][:, 0] for p in per], axis=1)
        rl = np.stack([p[5]["rl"][:, 0] for p in per], axis=1)
        rmax, rinst = reductions(rx, rl, conv)
        rounds.append({"mesh": mesh, "rmax": rmax, "sweeps": sweeps})
        if not conv.any():
            status = 2
            break
        new = refine(mesh, rmax, 1, 32)
        if new.size == mesh.size:
            status = 0
            break
        if new.size > max_nodes:
            status = 1
            break
        start = [(sol[b]["_interpPts"], sol[b]["u"]) if conv[b] else None for b in range(nB)]
        mesh = new
    return {"mesh": mesh, "mesh_status": status, "meshes": [r["mesh"].size for r in rounds], "sweeps": sweeps,
            "x": np.stack([p[2] for p in per], axis=2), "lam": np.stack([p[3] for p in per], axis=2),
            "J": np.array([p[4] for p in per]), "errJ": np.array([float(p[5]["errJ"][0]) for p in per]),
            "u": np.stack([p[0] for p in per], axis=2), "ugrid": np.stack([p[1] for p in per], axis=2), "rx": rx, "rl": rl,
            "err_ok": conv & (rinst <= 1), "rounds": rounds}
