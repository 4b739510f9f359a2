"""The iteration of the batched shooting driver in plain NumPy (a helper module, not a test file).

`spg_twin` restates ocs_single_shooting_batch_dev (csrc/ocs_shooting.cpp) and the five k_spg_* kernels
(csrc/ocs_shooting_kernels.hip) statement by statement, every instance a column of [rows][B] arrays, no Python loop
over instances.  The objective and its gradient come from a callback, so the same twin runs on the CPU oracle
(tests/test_spg_twin.py) and on the library's own nlp_objective_dev (tests/test_gpu_shooting_driver.py), where it
then sees the very bits the driver sees and only the bookkeeping is under test.

The driver's loop is `run_twin`, once for both algorithms (the other is tests/lbfgs_twin.py): an algorithm is its phases
direction / accept / update, plain functions on the state `st` of a run.  The kernels' shared helpers are restated once.

`CASES` / `make_inputs` is the one table of cases and seeds both files use; `check_purpose` asserts on a twin run
what makes a case non-vacuous."""
from types import SimpleNamespace

import numpy as np

P = {"c": 1.5, "m": 3.0, "r": 0.05}
DECISIVE_MARGIN = 1e-9      # three orders above the 1e-12 parity of the evaluations
INDECISIVE_CAP = 0.05       # of the batch


def _proj(w, lb, ub):                                   # proj
    return np.fmin(np.fmax(w, lb[:, None]), ub[:, None])


def _pgn(v, g, lb, ub):                                 # pg_norm
    return np.fmax.reduce(np.abs(_proj(v - g, lb, ub) - v), axis=0, initial=0.0)


def _rel(a, b):
    a, b = np.broadcast_arrays(np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64))
    r = np.abs(a - b) / np.maximum(np.maximum(np.abs(a), np.abs(b)), 1e-300)
    return np.where(np.isnan(r), np.inf, r)             # a NaN side decides the comparison whatever the other is


def _dot(a, b, fr=None):                                # the kernels' running sums, row after row (over the rows `fr`)
    s = np.zeros(a.shape[1])
    for i in range(a.shape[0]):
        s = s + (a[i] * b[i] if fr is None else np.where(fr[i], a[i] * b[i], 0.0))
    return s


def note(st, what, mask, r):                            # the instances of `mask` decided something at relative distance r
    st.margin[mask] = np.minimum(st.margin, r)[mask]
    m = st.margins.setdefault(what, np.full(st.margin.shape, np.inf))   # the same per kind of decision (for the reader
    m[mask] = np.minimum(m, r)[mask]                                    # of a failing case)


def decide(st, what, mask, a, b):                       # the instances of `mask` take the comparison a ? b
    note(st, what, mask, _rel(a, b))


def decide_sign(st, what, mask, value, scale):          # the sign of `value`, measured on the scale of its terms
    r = np.abs(value) / np.fmax(scale, 1e-300)          # (|x - 0| / max(|x|, 0) is 1 for every x != 0)
    note(st, what, mask, np.where(np.isnan(r), np.inf, r))


def goes_on(st):                                        # goes_on: the stopping test of both direction kernels
    pgn = _pgn(st.v, st.g, st.lb, st.ub)
    decide(st, "pgn <= TolFun", st.active, pgn, st.TolFun)
    st.active = st.active & (pgn > st.TolFun)           # !(pgn > TolFun) stops, a NaN norm too
    st.accepted = np.where(st.active, 0, 1)             # a finished instance's trial point is its v (the callers' where)


def halve_step(st, rej):                                # halve_step
    st.lam = np.where(rej, 0.5 * st.lam, st.lam)
    st.vt = np.where(rej, _proj(st.v + st.lam * st.d, st.lb, st.ub), st.vt)


def take_step(st, take):
    """step_rows with `take` and step_taken: v, g, J move to the accepted point, Barzilai-Borwein step length of the next
    iteration, stop on a small step.  Returns s, y, s'y and the instances stopped by TolX."""
    s, y = st.vt - st.v, st.gt - st.g
    sty, sts = _dot(s, y), _dot(s, s)
    smax = np.fmax.reduce(np.abs(s), axis=0, initial=0.0)
    st.v = np.where(take, st.vt, st.v)
    st.g = np.where(take, st.gt, st.g)
    st.J = np.where(take, st.Jt, st.J)
    decide(st, "s'y > 0", take, sty, 0.0)
    decide_sign(st, "s'y > 0", take, sty, _dot(np.abs(s), np.abs(y)))
    an = np.where(sty > 0.0, sts / np.fmax(sty, 1e-300), 1e3)
    st.alpha = np.where(take, st.bump(np.fmin(np.fmax(an, 1e-10), 1e10)), st.alpha)
    decide(st, "step <= TolX", take, smax, st.TolX)
    return s, y, sty, take & (smax <= st.TolX)


def run_twin(evaluate, v0, Lb, Ub, TolX, TolFun, MaxIter, maxBacktracks, ulp_seed, phases, **own):
    """ocs_single_shooting_batch_dev: the loop of both algorithms on the state `st` (`own`: the algorithm's options), phases
    = (start, direction, accept, update).  start(st) adds the algorithm's state after k_spg_init; direction(st) is the
    Direction phase; accept(st, pending) the Accept phase on the instances still waiting: it returns (accepted now, the
    right-hand side of their test) and gives the others their next trial point; update(st, started) the Update phase: it
    returns (step taken, stopped by TolX, the algorithm's entries of the step record).  Returns the result and `st`."""
    start, direction, accept, update = phases
    st = SimpleNamespace(v=np.array(v0, dtype=np.float64, copy=True), TolX=TolX, TolFun=TolFun, margins={}, **own)
    nV, B = st.v.shape
    st.lb = np.full(nV, -np.inf) if Lb is None else np.asarray(Lb, dtype=np.float64).ravel()
    st.ub = np.full(nV, np.inf) if Ub is None else np.asarray(Ub, dtype=np.float64).ravel()
    rng = None if ulp_seed is None else np.random.default_rng(ulp_seed)
    one_ulp = lambda x: np.nextafter(x, np.where(rng.integers(0, 2, size=x.shape) == 1, np.inf, -np.inf))
    st.bump = bump = (lambda x: x) if rng is None else one_ulp
    st.margin, snap, steps = np.full(B, np.inf), [], []
    arrays = lambda Jg: (np.array(Jg[0], dtype=np.float64), np.array(Jg[1], dtype=np.float64))

    def snapshot():                                     # k_spg_finish
        pgn = _pgn(st.v, st.g, st.lb, st.ub)
        snap.append(SimpleNamespace(v=st.v.copy(), J=st.J.copy(), iterations=st.iters.copy(), active=st.active.copy(),
                                    pgn=pgn, converged=pgn <= 10.0 * TolFun,
                                    margin=np.minimum(st.margin, _rel(pgn, 10.0 * TolFun))))

    with np.errstate(all="ignore"):
        st.J, st.g = arrays(evaluate(st.v))
        # k_spg_init
        st.alpha = bump(1.0 / np.fmax(_pgn(st.v, st.g, st.lb, st.ub), 1e-12))
        st.active = np.ones(B, dtype=bool)
        st.iters = np.zeros(B, dtype=np.int64)
        start(st)
        snapshot()
        for it in range(MaxIter):
            st.it = it
            direction(st)
            if not st.active.any():                     # nactive == 0
                break
            started = st.active.copy()
            nbt = np.zeros(B, dtype=np.int64)
            lhs, rhs_at, Jt0 = np.full(B, np.nan), np.full(B, np.nan), None
            for ls in range(maxBacktracks):
                st.Jt, st.gt = arrays(evaluate(st.vt))
                Jt0 = st.Jt.copy() if ls == 0 else Jt0
                pending = st.accepted == 0              # the accept kernels return on accepted[b] != 0
                ok, rhs = accept(st, pending)
                st.accepted[ok] = 2
                lhs[ok], rhs_at[ok] = st.Jt[ok], rhs[ok]
                nbt += pending & ~ok
                if not (pending & ~ok).any():           # nrejected == 0
                    break
            take, tolx, rec = update(st, started)
            steps.append(SimpleNamespace(started=started, accepted=take, failed=started & ~take, tolx=tolx, backtracks=nbt,
                                         Jt=lhs, rhs=rhs_at, lam=st.lam.copy(), Jt0=Jt0, **rec))
            snapshot()
        while len(snap) < MaxIter + 1:                  # the loop ended early: later calls return the same
            snapshot()
    backtracks = np.array([s.backtracks for s in steps]).reshape(len(steps), B)
    return SimpleNamespace(**vars(snap[-1]), backtracks=backtracks, snap=snap, steps=steps), st   # v, J, ... of the last k


def _spg_start(st):                                     # k_spg_init: the history
    st.hist = np.tile(st.J, (st.memory, 1))
    st.nonmonotone = np.zeros(st.J.shape, dtype=bool)


def _spg_direction(st):                                 # k_spg_direction
    goes_on(st)
    d = st.bump(_proj(st.v - st.alpha * st.g, st.lb, st.ub) - st.v)    # spg_direction, SPG's form
    st.d = np.where(st.active, d, 0.0)
    st.vt = np.where(st.active, _proj(st.v + st.d, st.lb, st.ub), st.v)
    st.gtd = _dot(st.g, st.d)
    st.fmx = st.hist[0].copy()
    for m in range(1, st.memory):
        st.fmx = np.fmax(st.fmx, st.hist[m])
    st.lam = np.ones(st.J.shape)


def _spg_accept(st, pending):                           # k_spg_accept
    rhs = st.fmx + 1e-4 * st.lam * st.gtd
    decide(st, "Armijo", pending, st.Jt, rhs)
    ok = pending & (st.Jt <= rhs)                       # a NaN Jt is a rejection
    halve_step(st, pending & ~ok)
    return ok, rhs


def _spg_update(st, started):                           # k_spg_update
    st.iters += st.active                               # a failed line search counts too
    take = st.active & (st.accepted == 2)
    st.nonmonotone |= take & (st.Jt > st.J)
    tolx = take_step(st, take)[3]
    st.active = take & ~tolx                            # a failed line search stops where it is
    st.hist[st.it % st.memory] = st.J                   # every instance, every iteration
    return take, tolx, {}


def spg_twin(evaluate, v0, Lb, Ub, TolX, TolFun, MaxIter, memory, maxBacktracks, ulp_seed=None):
    """evaluate(V [nV][B]) -> (J [B], G [nV][B]), always called on the whole batch.  With `ulp_seed` every computed
    direction d and step length alpha is moved by one ulp in a seeded random direction (the sensitivity probe of the
    GPU test).  Returns v, J, iterations, converged, pgn, and per instance: backtracks [iterations run][B], nonmonotone
    (an accepted step had Jt > J), margin (smallest relative distance over every comparison that decided something);
    `snap[k]` is the state a call with MaxIter = k returns (k = 0..MaxIter), `steps[it]` the record of iteration it."""
    r, st = run_twin(evaluate, v0, Lb, Ub, TolX, TolFun, MaxIter, maxBacktracks, ulp_seed,
                     (_spg_start, _spg_direction, _spg_accept, _spg_update), memory=memory)
    r.nonmonotone = st.nonmonotone
    return r


# ---------------------------------------------------------------------------------------------------------------
# the one table of cases: shapes, options and seeds of tests/test_spg_twin.py and tests/test_gpu_shooting_driver.py
# problem "testoc": TestOCProblem, per-instance c ~ U(1, 2), x0 ~ U(0.6, 2.4); "logistic": LogisticProblem(m)
_BLOCKS = dict(problem="testoc", basis="pwl", nB=7, N=40, T=4.0, start=(0.0, 1.0), memory=3, K=8, TolFun=1e-6,
               TolX=1e-10, maxBacktracks=25, free=(), fsb=None, fusion=None)
# a long horizon and a start next to the upper bound: the first step (length 1 / pgn) overshoots for most instances
# the last `blowup` instances have m = 1.5 and start in [0, 0.5]: their first trial point P(v - g / pgn) drives the state
# through zero, J is not finite there, and halving brings them back
_BACK = dict(_BLOCKS, batch=130, T=20.0, start=(0.8, 1.0), memory=10, TolFun=1e-9, TolX=2e-3, seed=31, blowup=40)
_CHEB = dict(_BLOCKS, problem="logistic", m=(3.0,), basis="cheb", nB=5, N=48, memory=10, K=6)
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
    "cheb64on": dict(_CHEB, batch=64, fusion="on", seed=71),
    "cheb64off": dict(_CHEB, batch=64, fusion="off", seed=71),
    "cheb70on": dict(_CHEB, batch=70, fusion="on", seed=72),
    "cheb70off": dict(_CHEB, batch=70, fusion="off", seed=72),
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


def device_setup(ocs, oracle, c):
    """handles of a case on the GPU library `ocs`, v0, Lb, Ub, evaluate (its nlp_objective_dev on these handles, the whole
    batch in one call) and solve(k, **options): what single_shooting_batch returns with MaxIter = k"""
    import torch
    tspan = oracle.linspace(0, c.T, c.N + 1)
    integ = ocs.RK4Integrator(tspan)
    if c.problem == "testoc":                           # parameter block [c m r]: c and m per trajectory
        prob = ocs.TestOCProblem(P, BOUNDS)
        prob.set_batch_params([0, 1], np.vstack([c.cs, c.ms]))
    else:
        prob = ocs.LogisticProblem(list(c.m), P["c"], P["r"], BOUNDS)
        prob.set_batch_params([0], c.cs[None, :])
    ctrl = (ocs.ChebyshevControl if c.basis == "cheb" else ocs.PWLinearControl)(integ.t, c.nB, 1)
    if c.fusion:
        ctrl.set_fusion(c.fusion)
    v0, Lb, Ub = full_start(c, *((None, None) if c.basis == "cheb" else ctrl.compute_nlp_bounds(prob.ControlBounds)))

    def evaluate(V, want_x0=False):
        x0d = torch.tensor(c.x0, device="cuda:0").contiguous()
        J, G = ocs.nlp_objective_dev(integ, prob, ctrl, x0d, torch.tensor(np.ascontiguousarray(V), device="cuda:0"),
                                      FreeInitStates=list(c.free))
        torch.cuda.synchronize()
        return (J.cpu().numpy(), G.cpu().numpy()) + ((x0d.cpu().numpy(),) if want_x0 else ())

    def solve(k, **kw):
        r = ocs.single_shooting_batch(prob, c.x0, tspan, c.nB, Control=ctrl, Integrator=integ, v0=c.v0, MaxIter=k,
                                      FreeInitStates=list(c.free), FreeStateBounds=c.fsb, constraints="ignore", **dict(c.opts, **kw))
        torch.cuda.synchronize()
        return SimpleNamespace(keys=sorted(r), pgn=r["projected_gradient"].cpu().numpy(),
                               **{k: r[k].cpu().numpy() for k in ("v", "J", "iterations", "converged", "x0")})
    return SimpleNamespace(c=c, v0=v0, Lb=Lb, Ub=Ub, evaluate=evaluate, solve=solve, integ=integ, prob=prob, ctrl=ctrl)


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
