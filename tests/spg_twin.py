"""The iteration of the batched shooting driver in plain NumPy (a helper module, not a test file).

`spg_twin` restates ocs_single_shooting_batch_dev (csrc/ocs_shooting.cpp:98-115) and the five k_spg_* kernels
(csrc/ocs_shooting_kernels.hip) statement by statement, every instance a column of [rows][B] arrays, no Python loop
over instances.  The objective and its gradient come from a callback, so the same twin runs on the CPU oracle
(tests/test_spg_twin.py) and on the library's own nlp_objective_dev (tests/test_gpu_shooting_driver.py), where it
then sees the very bits the driver sees and only the bookkeeping is under test.

`CASES` / `make_inputs` is the one table of cases and seeds both files use; `check_purpose` asserts on a twin run
what makes a case non-vacuous."""
from types import SimpleNamespace

import numpy as np

P = {"c": 1.5, "m": 3.0, "r": 0.05}
DECISIVE_MARGIN = 1e-9      # three orders above the 1e-12 parity of the evaluations
INDECISIVE_CAP = 0.05       # of the batch


def _proj(w, lb, ub):                                   # spg_proj, kernels.hip:12
    return np.fmin(np.fmax(w, lb[:, None]), ub[:, None])


def _pgn(v, g, lb, ub):                                 # kernels.hip:19-23, :37-41, :119-123
    return np.fmax.reduce(np.abs(_proj(v - g, lb, ub) - v), axis=0, initial=0.0)


def _rel(a, b):
    a, b = np.broadcast_arrays(np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64))
    r = np.abs(a - b) / np.maximum(np.maximum(np.abs(a), np.abs(b)), 1e-300)
    return np.where(np.isnan(r), np.inf, r)             # a NaN side decides the comparison whatever the other is


def _dot(a, b):                                         # the kernels' running sums, row after row (:52-58, :94-99)
    s = np.zeros(a.shape[1])
    for i in range(a.shape[0]):
        s = s + a[i] * b[i]
    return s


def spg_twin(evaluate, v0, Lb, Ub, TolX, TolFun, MaxIter, memory, maxBacktracks, ulp_seed=None):
    """evaluate(V [nV][B]) -> (J [B], G [nV][B]), always called on the whole batch.  With `ulp_seed` every computed
    direction d and step length alpha is moved by one ulp in a seeded random direction (the sensitivity probe of the
    GPU test).  Returns v, J, iterations, converged, pgn, and per instance: backtracks [iterations run][B], nonmonotone
    (an accepted step had Jt > J), margin (smallest relative distance over every comparison that decided something);
    `snap[k]` is the state a call with MaxIter = k returns (k = 0..MaxIter), `steps[it]` the record of iteration it."""
    v = np.array(v0, dtype=np.float64, copy=True)
    nV, B = v.shape
    lb = np.full(nV, -np.inf) if Lb is None else np.asarray(Lb, dtype=np.float64).ravel()      # cpp:58-60
    ub = np.full(nV, np.inf) if Ub is None else np.asarray(Ub, dtype=np.float64).ravel()
    rng = None if ulp_seed is None else np.random.default_rng(ulp_seed)

    def bump(x):
        if rng is None:
            return x
        return np.nextafter(x, np.where(rng.integers(0, 2, size=x.shape) == 1, np.inf, -np.inf))

    margin = np.full(B, np.inf)

    def decide(mask, a, b):                             # the instances of `mask` take the comparison a ? b
        margin[mask] = np.minimum(margin, _rel(a, b))[mask]

    snap, steps = [], []

    def snapshot():                                     # k_spg_finish, kernels.hip:115-126 (cpp:115)
        pgn = _pgn(v, g, lb, ub)
        snap.append(SimpleNamespace(v=v.copy(), J=J.copy(), iterations=iters.copy(), active=active.copy(), pgn=pgn,
                                    converged=pgn <= 10.0 * TolFun,
                                    margin=np.minimum(margin, _rel(pgn, 10.0 * TolFun))))

    with np.errstate(all="ignore"):
        J, g = evaluate(v)                              # cpp:98
        J, g = np.array(J, dtype=np.float64), np.array(g, dtype=np.float64)
        # k_spg_init, kernels.hip:15-28
        alpha = bump(1.0 / np.fmax(_pgn(v, g, lb, ub), 1e-12))
        hist = np.tile(J, (memory, 1))
        active = np.ones(B, dtype=bool)
        iters = np.zeros(B, dtype=np.int64)
        nonmonotone = np.zeros(B, dtype=bool)
        snapshot()
        for it in range(MaxIter):                       # cpp:100
            # k_spg_direction, kernels.hip:31-66
            pgn = _pgn(v, g, lb, ub)
            decide(active, pgn, TolFun)
            active = active & (pgn > TolFun)            # :42  !(pgn > TolFun) stops, a NaN norm too
            accepted = np.where(active, 0, 1)           # :46, :64
            d = bump(_proj(v - alpha * g, lb, ub) - v)  # :54
            d = np.where(active, d, 0.0)
            vt = np.where(active, _proj(v + d, lb, ub), v)   # :47 a finished instance's trial point is its v; :56
            gtd = _dot(g, d)                            # :57
            fmx = hist[0].copy()                        # :59-60
            for m in range(1, memory):
                fmx = np.fmax(fmx, hist[m])
            lam = np.ones(B)                            # :63
            if not active.any():                        # cpp:103
                break
            started = active.copy()
            nbt = np.zeros(B, dtype=np.int64)
            lhs, rhs_at, Jt0 = np.full(B, np.nan), np.full(B, np.nan), None
            for ls in range(maxBacktracks):             # cpp:104
                Jt, gt = evaluate(vt)                   # cpp:105
                Jt, gt = np.array(Jt, dtype=np.float64), np.array(gt, dtype=np.float64)
                Jt0 = Jt.copy() if ls == 0 else Jt0
                # k_spg_accept, kernels.hip:70-83
                pending = accepted == 0                 # :72
                rhs = fmx + 1e-4 * lam * gtd            # :75
                decide(pending, Jt, rhs)
                ok = pending & (Jt <= rhs)              # a NaN Jt is a rejection
                accepted[ok] = 2                        # :76
                lhs[ok], rhs_at[ok] = Jt[ok], rhs[ok]
                rej = pending & ~ok
                lam = np.where(rej, 0.5 * lam, lam)     # :79-80
                vt = np.where(rej, _proj(v + lam * d, lb, ub), vt)     # :81
                nbt += rej
                if not rej.any():                       # cpp:108
                    break
            # k_spg_update, kernels.hip:86-112
            iters += active                             # :91 (a failed line search counts too)
            take = active & (accepted == 2)             # :92
            s, y = vt - v, gt - g                       # :96
            sty, sts = _dot(s, y), _dot(s, s)           # :97-98
            smax = np.fmax.reduce(np.abs(s), axis=0, initial=0.0)   # :99
            nonmonotone |= take & (Jt > J)
            v = np.where(take, vt, v)                   # :100
            g = np.where(take, gt, g)                   # :101
            J = np.where(take, Jt, J)                   # :103
            decide(take, sty, 0.0)
            # |sty - 0| / max(|sty|, 0) is 1 for every sty != 0: measure the sign of sty on the scale of its terms as well
            with_scale = np.abs(sty) / np.fmax(_dot(np.abs(s), np.abs(y)), 1e-300)
            margin[take] = np.minimum(margin, np.where(np.isnan(with_scale), np.inf, with_scale))[take]
            an = np.where(sty > 0.0, sts / np.fmax(sty, 1e-300), 1e3)       # :104
            alpha = np.where(take, bump(np.fmin(np.fmax(an, 1e-10), 1e10)), alpha)   # :105
            decide(take, smax, TolX)
            tolx = take & (smax <= TolX)                # :106
            active = take & ~tolx                       # :106, :108 a failed line search stops where it is
            hist[it % memory] = J                       # :111 every instance, every iteration
            steps.append(SimpleNamespace(started=started, accepted=take, failed=started & ~take, tolx=tolx,
                                         backtracks=nbt, Jt=lhs, rhs=rhs_at, lam=lam.copy(), Jt0=Jt0))
            snapshot()
        while len(snap) < MaxIter + 1:                  # the loop ended early (cpp:103): later calls return the same
            snapshot()
    last = snap[-1]
    return SimpleNamespace(v=last.v, J=last.J, iterations=last.iterations, converged=last.converged, pgn=last.pgn,
                           backtracks=np.array([s.backtracks for s in steps]).reshape(len(steps), B),
                           nonmonotone=nonmonotone, margin=last.margin, active=last.active, snap=snap, steps=steps)


# ---------------------------------------------------------------------------------------------------------------
# the one table of cases: shapes, options and seeds of tests/test_spg_twin.py and tests/test_gpu_shooting_driver.py
# problem "testoc": TestOCProblem, per-instance c ~ U(1, 2), x0 ~ U(0.6, 2.4); "logistic": LogisticProblem(m)
_BLOCKS = dict(problem="testoc", basis="pwl", nB=7, N=40, T=4.0, start=(0.0, 1.0), memory=3, K=8, TolFun=1e-6,
               TolX=1e-10, maxBacktracks=25, free=(), fsb=None, fusion=None)
# a long horizon and a start next to the upper bound: the first step (length 1 / pgn) overshoots for most instances
# the last `blowup` instances have m = 1.5 and start in [0, 0.5]: their first trial point P(v - g / pgn) drives the state
# through zero, J is not finite there, and halving brings them back
_BACK = dict(_BLOCKS, batch=130, T=20.0, start=(0.8, 1.0), memory=10, TolFun=1e-9, TolX=2e-3, seed=31, blowup=40)
CASES = {
    "blocks257": dict(_BLOCKS, batch=257, seed=11),
    "blocks600": dict(_BLOCKS, batch=600, seed=12),
    "backtrack": dict(_BACK),
    "exhausted1": dict(_BACK, maxBacktracks=1),
    "exhausted2": dict(_BACK, maxBacktracks=2),
    "tolx": dict(_BLOCKS, batch=70, memory=10, TolX=1e-1, TolFun=1e-9, seed=41),
    "zero": dict(_BLOCKS, batch=70, K=0, seed=51),
    "free": dict(_BLOCKS, problem="logistic", m=(3.0, 2.5), nB=6, batch=65, memory=10, start=(0.1, 0.5), free=(2,),
                 fsb=((0.45, 2.5),), crange=(0.2, 8.0), seed=61),
    "cheb64on": dict(_BLOCKS, problem="logistic", m=(3.0,), basis="cheb", nB=5, N=48, batch=64, memory=10, K=6,
                     fusion="on", seed=71),
    "cheb64off": dict(_BLOCKS, problem="logistic", m=(3.0,), basis="cheb", nB=5, N=48, batch=64, memory=10, K=6,
                      fusion="off", seed=71),
    "cheb70on": dict(_BLOCKS, problem="logistic", m=(3.0,), basis="cheb", nB=5, N=48, batch=70, memory=10, K=6,
                     fusion="on", seed=72),
    "cheb70off": dict(_BLOCKS, problem="logistic", m=(3.0,), basis="cheb", nB=5, N=48, batch=70, memory=10, K=6,
                      fusion="off", seed=72),
}
BOUNDS = [[0.0, 1.0]]


def make_inputs(name, **over):
    """The numbers of a case (`over` replaces entries of its row): per-instance c, m and x0, the start v0 [nB][B]
    (without the free initial states)."""
    c = SimpleNamespace(name=name, **dict(CASES[name], **over))
    rng = np.random.default_rng(c.seed)
    B = c.batch
    c.nS = 1 if c.problem == "testoc" else len(c.m)
    c.cs = rng.uniform(*getattr(c, "crange", (1.0, 2.0)), B)
    c.x0 = rng.uniform(0.6, 2.4, (c.nS, B)) if c.problem == "testoc" else rng.uniform(0.95, 2.4, (c.nS, B))
    if c.basis == "cheb":                               # decaying coefficients around a constant, no bounds
        c.v0 = 0.05 * rng.normal(size=(c.nB, B)) / np.arange(1, c.nB + 1)[:, None]
        c.v0[0] += 0.4
    else:                                               # u0 per instance: a constant control
        c.v0 = np.repeat(rng.uniform(c.start[0], c.start[1], (1, B)), c.nB, axis=0)
    c.ms = np.full(B, P["m"])
    nb = getattr(c, "blowup", 0)
    if nb:
        c.ms[B - nb:] = 1.5
        c.v0[:, B - nb:] = np.repeat(rng.uniform(0.0, 0.5, (1, nb)), c.nB, axis=0)
    c.opts = dict(TolX=c.TolX, TolFun=c.TolFun, memory=c.memory, maxBacktracks=c.maxBacktracks)
    return c


def full_start(c, Lb, Ub):
    """v0 with x0(FreeInitStates) at its tail and the bounds with FreeStateBounds (single_shooting.m:84, :91-94);
    Lb = Ub = None for a basis without compute_nlp_bounds."""
    nV = c.v0.shape[0]
    Lb = np.full(nV, -np.inf) if Lb is None else np.asarray(Lb, dtype=np.float64)
    Ub = np.full(nV, np.inf) if Ub is None else np.asarray(Ub, dtype=np.float64)
    v0 = c.v0
    if c.free:
        idx = [k - 1 for k in c.free]
        fsb = np.asarray(c.fsb, dtype=np.float64)
        v0 = np.vstack([v0, c.x0[idx, :]])
        Lb, Ub = np.concatenate([Lb, fsb[:, 0]]), np.concatenate([Ub, fsb[:, 1]])
    return np.ascontiguousarray(v0), Lb, Ub


def oracle_setup(oracle, c):
    """evaluate, v0, Lb, Ub of a case on the CPU oracle (one nlp_objective call per instance)."""
    go = oracle.RK4Integrator(oracle.linspace(0, c.T, c.N + 1))
    if c.problem == "testoc":
        probs = [oracle.TestOCProblem({"c": cb, "m": mb, "r": P["r"]}, BOUNDS) for cb, mb in zip(c.cs, c.ms)]
    else:
        probs = [oracle.LogisticProblem(list(c.m), cb, P["r"], BOUNDS) for cb in c.cs]
    co = (oracle.ChebyshevControl if c.basis == "cheb" else oracle.PWLinearControl)(go.t, c.nB, 1)
    v0, Lb, Ub = full_start(c, *((None, None) if c.basis == "cheb" else co.compute_nlp_bounds(BOUNDS)))
    free = list(c.free)

    def evaluate(V):
        J, G = np.empty(V.shape[1]), np.empty(V.shape)
        for b in range(V.shape[1]):
            J[b], G[:, b], _ = oracle.nlp_objective(go, probs[b], co, c.x0[:, b], V[:, b], FreeInitStates=free)
        return J, G
    return evaluate, v0, Lb, Ub


def decisive_mask(tw, k=None):
    s = tw.snap[-1 if k is None else k]
    return s.margin >= DECISIVE_MARGIN


def check_invariants(c, tw, Lb, Ub):
    """What holds in every run: v inside the bounds, an accepted step satisfies its Armijo inequality, iterations <= MaxIter,
    a stopped instance does not move."""
    K = len(tw.snap) - 1
    for k, s in enumerate(tw.snap):
        assert np.all(s.v >= Lb[:, None]) and np.all(s.v <= Ub[:, None]), (c.name, k)
        assert np.all(s.iterations <= k)
    assert np.all(tw.iterations <= K)
    for it, st in enumerate(tw.steps):
        a = st.accepted
        assert np.all(st.Jt[a] <= st.rhs[a]) and not np.isnan(st.Jt[a]).any(), (c.name, it)
        assert np.all(st.backtracks <= c.maxBacktracks)
        stopped = ~tw.snap[it].active
        assert np.array_equal(tw.snap[it + 1].v[:, stopped], tw.snap[it].v[:, stopped]), (c.name, it)
        assert np.array_equal(tw.snap[it + 1].J[stopped], tw.snap[it].J[stopped])
        assert np.array_equal(tw.snap[it + 1].iterations[stopped], tw.snap[it].iterations[stopped])
        assert not (st.started & stopped).any()


def check_purpose(c, tw, dec, Lb, Ub):
    """The case's purpose occurs among the decisive instances `dec` of the twin run `tw` (so no test of it passes empty)."""
    name, B = c.name, c.batch
    assert np.count_nonzero(~dec) <= INDECISIVE_CAP * B, (name, "indecisive", int(np.count_nonzero(~dec)), B)
    moved = np.zeros(B, dtype=bool)
    for st in tw.steps:
        moved |= st.accepted
    if name.startswith("blocks"):
        assert (dec & moved)[256:512].any() and B % 256 != 0, "second workgroup, ragged last one"
        if B > 512:
            assert (dec & moved)[512:].any(), "third workgroup"
        late = [st.accepted & dec for st in tw.steps[c.memory:]]
        assert late and np.count_nonzero(np.any(late, axis=0)) >= B // 2, "the history ring wraps under moving instances"
        assert (tw.nonmonotone & dec).any(), "a step with Jt > J is accepted"
        on = ((tw.v == Lb[:, None]) | (tw.v == Ub[:, None]))[:, dec]
        assert on.any() and (~on).any() and (on.any(axis=0) & (~on).any(axis=0)).any(), "active and inactive bounds"
    if name == "backtrack":
        assert np.count_nonzero(dec & (tw.backtracks >= 2).any(axis=0)) >= 10, "two backtracks in one iteration"
        done = dec & ~tw.active
        assert len(set(tw.iterations[done].tolist())) >= 2, "instances finish in different iterations"
        assert (dec & tw.active).any()
        nan_then_ok = np.any([~np.isfinite(st.Jt0) & st.accepted for st in tw.steps], axis=0)
        assert np.count_nonzero(dec & nan_then_ok) >= 5, "a non-finite first trial, rejected, and a later accepted step"
    if name.startswith("exhausted"):
        failed = np.any([st.failed for st in tw.steps], axis=0)
        assert np.count_nonzero(dec & failed) >= 5, "failed line searches"
        first = min(it for it, st in enumerate(tw.steps) if (st.failed & dec).any())
        assert any((st.accepted & dec).any() for st in tw.steps[first + 1:]), "the rest of the batch continues"
    if name == "tolx":
        tolx = np.any([st.tolx for st in tw.steps], axis=0)
        assert (dec & tolx & ~tw.converged).any(), "a stop on the step size far from the optimum"
    if name == "free":
        # below x = 0.5 the second state collapses under a strong harvest: where the control is cheap (small c) the free
        # state stays inside its bounds, where it is dear the state ends on the lower bound
        tail = tw.v[-1]
        onb = (tail == Lb[-1]) | (tail == Ub[-1])
        assert np.count_nonzero(dec & onb) >= 5 and np.count_nonzero(dec & ~onb & moved) >= 5, "free state on its bound and inside"
    if name.startswith("cheb"):
        assert np.isinf(Lb).all() and np.isinf(Ub).all() and np.count_nonzero(dec & moved) >= B // 2


# ---------------------------------------------------------------------------------------------------------------
# driver against twin: `runs[k]` is what the driver returned with MaxIter = k (v, J, iterations, converged, pgn)
def _moved(snaps):
    return np.array([np.any(snaps[k + 1].v != snaps[k].v, axis=0) for k in range(len(snaps) - 1)]).reshape(len(snaps) - 1, -1)


def _same_discrete(a, b):
    """per instance: iterations, converged and the set of iterations in which it moved agree at every k"""
    same = np.all(_moved(a) == _moved(b), axis=0) if len(a) > 1 else np.ones(a[0].J.shape, dtype=bool)
    for sa, sb in zip(a, b):
        same &= (sa.iterations == sb.iterations) & (np.asarray(sa.converged, dtype=bool) == np.asarray(sb.converged, dtype=bool))
    return same


def _spread(a, b, mask):
    """largest difference of v, J and the projected gradient norm over every k, relative to max(1, |.|)"""
    worst = 0.0
    if not mask.any():
        return worst
    for sa, sb in zip(a, b):
        for x, y in ((sa.v[:, mask], sb.v[:, mask]), (sa.J[mask], sb.J[mask]), (sa.pgn[mask], sb.pgn[mask])):
            worst = max(worst, float(np.max(np.abs(x - y) / np.maximum(1.0, np.abs(y)))))
    return worst


def measured_tolerance(tw, tw2):
    """decisive instances and the tolerance of the comparison, from the twin run `tw` and its rerun `tw2` with every d and
    alpha moved by one ulp: an instance is decisive if no comparison of either run came closer than DECISIVE_MARGIN and the
    two runs agree in everything discrete; the tolerance is 16 x the largest difference between the runs, at least 1e-13."""
    dec = _same_discrete(tw.snap, tw2.snap)
    for s in tw.snap + tw2.snap:
        dec &= s.margin >= DECISIVE_MARGIN
    spread = _spread(tw.snap, tw2.snap, dec)
    return dec, spread, max(16.0 * spread, 1e-13)


def compare_with_twin(runs, tw, dec, tol):
    """every decisive instance at every k: iterations, converged and the moving set equal, v, J, pgn within tol"""
    assert len(runs) == len(tw.snap)
    same = _same_discrete(runs, tw.snap)
    assert same[dec].all(), ("discrete results differ at instances", np.flatnonzero(dec & ~same)[:10].tolist())
    worst = _spread(runs, tw.snap, dec)
    assert worst <= tol, ("v, J or the projected gradient differ by", worst, "allowed", tol)
    return worst
