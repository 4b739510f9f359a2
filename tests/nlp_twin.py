"""Extended-precision twin of the single-shooting objective [J, dJdv] = nlpObjective(v) (single_shooting.m:137-150) and of the
three control bases under it, NumPy longdouble on top of tests/rk4_twin.py, vectorised over the batch only.

A third statement beside the oracle's C and the kernels, from the reference's MATLAB text:

    PWLinearControl.m:13-18, :31-50      controlPts = linspace(t(1), t(end), n); tents by griddedInterpolant('linear', 'nearest')
    PWConstantControl.m:11-17, :41-50    intervalStarts = linspace(t(1), t(end), n + 1)(1:n); B(i,:) = t >= s_i & t < s_{i+1}
    ChebyshevControl.m:21-31             tTrans = 2 (t - t(1)) / (t(end) - t(1)) - 1; B(1) = 1, B(2) = tTrans, three-term recurrence
    compute_u / compute_dJdv             u = reshape(v, nC, []) * B;  dJdv = reshape(dJdu * B', [], 1)   (control index fastest)
    single_shooting.m:137-150            x0(FreeInitStates) = v(nV+1:end); u; compute_states; compute_adjoints; dJdv; lam(Free, 1)

What counts as data and what as arithmetic: the grid t is formed in fp64 exactly as RK4Integrator.m:16-25 forms it
(rk4_twin.grid), and so are the break points that linspace puts on it (controlPts, intervalStarts: MATLAB's linspace in fp64).
They are inputs -- the break points decide which interval a grid point lies in, a discrete fact that every implementation must
share.  Everything formed FROM them is arithmetic and carried in longdouble: the tent weights (q - x_k) / (x_{k+1} - x_k), tTrans
and the Chebyshev recurrence, the products with v and dJdu and their sums.  So the host code that builds B in fp64
(ocs_control_create, the oracle's twin of it) is under the same measure as the kernels.

Shapes: v [nC nB + nFree][batch], x0 [nS][batch], u and dJdu [nC][2N+1][batch], B [nB][2N+1], dJdv [nC nB][batch] (the basis
rows alone), lam0 [nFree][batch].

The error measure (tests/test_gpu_nlp_accuracy.py, tests/test_nlp_twin.py):

    J       rk4_twin.err_J
    u       rk4_twin.err (local in time, +-4 grid points)
    dJdv    per control c:  |d_k - ref_k| / max_{|i - k| <= 4} |ref_i|   over the basis index k: rk4_twin.err with the window over
            the basis index.  A hat function late in a discounted horizon is held to its own size; a Chebyshev coefficient to
            the largest of its nine neighbours in degree (the coefficients of one expansion, formed from the same dJdu).
    lam0    each free-initial-state row relative to its own reference value, |l - ref| / |ref|

The windowed scale is kept for the Chebyshev rows as well: tests/test_nlp_twin.py::test_reordered_contraction_is_within_K
shows that two other legitimate fp64 summation orders stay within K of the oracle's error on every case under it, so the
condition scale sum_j |B_kj| |dJdu_j| (returned as "cond" for the non-vacuity assertions) is not needed as a replacement."""
import numpy as np

from tests import rk4_twin as tw

L = tw.L
KINDS = ("PWLinearControl", "PWConstantControl", "ChebyshevControl")


def linspace(a, b, n):
    """MATLAB's linspace in fp64 (oracle/ocs_oracle.c ocs_or_linspace): data of every implementation"""
    if n == 1:
        return np.array([b], dtype=np.float64)
    y = a + (np.arange(n, dtype=np.float64) * (b - a)) / (n - 1)
    y[0], y[-1] = a, b
    return y


def _tent(x, vals, q):
    """griddedInterpolant(x, vals, 'linear', 'nearest')(q), PWLinearControl.m:35: x fp64 break points (data), the weight in
    longdouble.  One query at a time."""
    n = len(x)
    if q < x[0]:
        return L(vals[0])
    if q > x[n - 1]:
        return L(vals[n - 1])
    k = 0
    while k < n - 2 and q >= x[k + 1]:      # x[k] <= q < x[k+1]; the last interval is closed
        k += 1
    w = (L(q) - L(x[k])) / (L(x[k + 1]) - L(x[k]))
    return L(vals[k]) + (L(vals[k + 1]) - L(vals[k])) * w


def basis(kind, t, n):
    """The basis matrix B [n][len(t)] in longdouble from the fp64 grid t (module docstring)."""
    t = np.asarray(t, dtype=np.float64).ravel()
    nT = t.size
    B = np.zeros((n, nT), dtype=L)
    if kind == "PWLinearControl":
        pts = linspace(t[0], t[-1], n)                                    # :16
        for j in range(nT):
            B[0, j] = _tent(pts[0:2], [1, 0], t[j])                       # :35-37
            for i in range(1, n - 1):                                     # :40-44
                B[i, j] = _tent(pts[i - 1:i + 2], [0, 1, 0], t[j])
            B[n - 1, j] = _tent(pts[n - 2:n], [0, 1], t[j])               # :47-49
    elif kind == "PWConstantControl":
        starts = linspace(t[0], t[-1], n + 1)[:-1]                        # :14-15
        for i in range(n - 1):                                            # :43-47
            B[i] = ((t >= starts[i]) & (t < starts[i + 1])).astype(L)
        B[n - 1] = (t >= starts[n - 1]).astype(L)                         # :49
    elif kind == "ChebyshevControl":
        tT = 2 * (L(1) * t - L(t[0])) / (L(t[-1]) - L(t[0])) - 1          # :23
        B[0] = 1
        if n > 1:
            B[1] = tT
        for i in range(2, n):                                             # :28-30
            B[i] = 2 * tT * B[i - 1] - B[i - 2]
    else:
        raise KeyError(kind)
    return B


def compute_u(B, v, nC):
    """u = reshape(v, nC, []) * B: v [nC nB][batch] (control index fastest) -> u [nC][nT][batch], summed over k in order"""
    B, v = tw._ld(B), tw._ld(v)
    nB, nT = B.shape
    u = np.zeros((nC, nT, v.shape[1]), dtype=L)
    for c in range(nC):
        for k in range(nB):
            u[c] += B[k][:, None] * v[c + nC * k][None, :]
    return u


def compute_dJdv(B, dJdu):
    """dJdv = reshape(dJdu * B', [], 1): dJdu [nC][nT][batch] -> [nC nB][batch], summed over the grid points in order"""
    B, dJdu = tw._ld(B), tw._ld(dJdu)
    nB, nT = B.shape
    nC = dJdu.shape[0]
    out = np.zeros((nC * nB, dJdu.shape[2]), dtype=L)
    for c in range(nC):
        for k in range(nB):
            for j in range(nT):
                out[c + nC * k] += B[k, j] * dJdu[c, j]
    return out


def condition_scale(B, dJdu):
    """sum_j |B_kj| |dJdu_cj|, shaped like dJdv: what any summation order of row k is conditioned on"""
    return compute_dJdv(np.abs(tw._ld(B)), np.abs(tw._ld(dJdu)))


def nlp_objective(prob, tspan, B, x0, v, free=()):
    """single_shooting.m:137-150.  prob: rk4_twin.LogisticK / LQ; B: basis(kind, rk4_twin.grid(tspan)[0], n); free: 1-based
    state indices (FreeInitStates).  Returns a dict of longdouble arrays: u, x [nS][N+1][batch], J [batch], lam, dJdu, dJdv
    (basis rows), lam0 [len(free)][batch], cond (condition_scale), x0 (after :146) and xK (the stage states)."""
    nC, nV = prob.nC, prob.nC * B.shape[0]
    x0 = np.array(np.atleast_2d(x0), dtype=np.float64)
    v = np.asarray(v, dtype=np.float64)
    assert v.shape[0] == nV + len(free)
    for f, s in enumerate(free):                                          # :146
        x0[s - 1] = v[nV + f]
    u = compute_u(B, v[:nV], nC)                                          # :139 / :145
    lamT = np.zeros((prob.nS + 1, x0.shape[1]))
    lamT[-1] = 1                                                          # the default of RK4Integrator.m:62-64
    p = tw.passes(prob, tspan, x0, u, lamT)                               # :140-141 / :147-148
    dJdv = compute_dJdv(B, p["dJdu"])                                     # :142 / :149
    lam0 = np.stack([p["lam"][s - 1, 0] for s in free]) if len(free) else np.zeros((0, x0.shape[1]), dtype=L)
    return {"u": u, "x": p["x"], "J": p["J"], "lam": p["lam"], "dJdu": p["dJdu"], "dJdv": dJdv, "lam0": lam0,
            "cond": condition_scale(B, p["dJdu"]), "x0": x0, "xK": p["xK"]}


def by_control(d, nC):
    """[nC nB][batch] (control index fastest) -> [nC][nB][batch]"""
    d = np.asarray(d)
    return d.reshape(d.shape[0] // nC, nC, d.shape[1]).transpose(1, 0, 2)


def err_dJdv(d, ref, nC=1):
    """The windowed error of the basis rows per trajectory (module docstring): each control's rows on their own."""
    d, ref = by_control(d, nC), by_control(ref, nC)
    return np.max(np.stack([tw.err(d[c:c + 1], ref[c:c + 1]) for c in range(nC)]), axis=0)


def err_lam0(l, ref):
    """|l - ref| / |ref| per free initial state, maximum over them, per trajectory; [0][batch] gives zeros"""
    ref = np.asarray(ref, dtype=L)
    if ref.shape[0] == 0:
        return np.zeros(ref.shape[1])
    e = np.abs(np.asarray(l).astype(L) - ref) / np.abs(ref)
    return np.max(np.where(np.isfinite(e), e, L(np.inf)), axis=0).astype(np.float64)


def errors(got, ref, nC=1):
    """got: fp64 J [batch], dJdv [nC nB + nFree][batch] as nlp_objective of the package / the oracle returns it (free rows last)
    and, where present, u; ref: the dict of nlp_objective above.  Returns {output: [batch]}; lam0 only with free states."""
    nV = ref["dJdv"].shape[0]
    d = np.asarray(got["dJdv"])
    out = {"J": tw.err_J(got["J"], ref["J"]), "dJdv": err_dJdv(d[:nV], ref["dJdv"], nC)}
    if ref["lam0"].shape[0]:
        out["lam0"] = err_lam0(d[nV:], ref["lam0"])
    if "u" in got:
        out["u"] = tw.err(got["u"], ref["u"])
    return out


def contract_reordered(B, dJdu, order):
    """A second fp64 statement of dJdv = dJdu B' with another legitimate summation order (B, dJdu fp64): "reversed" sums the
    grid points from the last to the first, "tiles" sums tiles of 16 columns pairwise (a binary tree inside the tile) and the
    tile sums pairwise again.  Test instrument of the measure, not a reference."""
    B, dJdu = np.asarray(B, dtype=np.float64), np.asarray(dJdu, dtype=np.float64)
    nB, nT = B.shape
    nC, _, batch = dJdu.shape

    def tree(terms):
        while len(terms) > 1:
            terms = [terms[i] + terms[i + 1] if i + 1 < len(terms) else terms[i] for i in range(0, len(terms), 2)]
        return terms[0]
    out = np.zeros((nC * nB, batch))
    for c in range(nC):
        for k in range(nB):
            if order == "reversed":
                s = np.zeros(batch)
                for j in range(nT - 1, -1, -1):
                    s = s + B[k, j] * dJdu[c, j]
            else:
                assert order == "tiles"
                s = tree([tree([B[k, j] * dJdu[c, j] for j in range(j0, min(j0 + 16, nT))]) for j0 in range(0, nT, 16)])
            out[c + nC * k] = s
    return out
