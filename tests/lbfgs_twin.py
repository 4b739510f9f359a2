"""The projected L-BFGS iteration of the batched shooting driver in plain NumPy (a helper module, not a test file).

`lbfgs_twin` restates ocs_single_shooting_batch_dev with algorithm = OCS_SS_LBFGS (csrc/ocs_shooting.cpp) and the
k_lbfgs_* kernels (csrc/ocs_shooting_kernels.hip) statement by statement, in the style of tests/spg_twin.py: every instance
a column of [rows][B] arrays, no Python loop over instances, objective and gradient from a callback.  It is the
specification of the iteration; where the outline left a choice the choice is made and commented here:

  * order in one iteration: stopping test on the projected gradient, active set, direction, safeguard, line search, update.
  * every pass of an active instance through the outer loop counts as an iteration: one whose line search failed on a
    quasi-Newton direction (the pairs are dropped, the instance goes on with SPG's direction) and one in which the
    safeguard replaced the direction count like any other.
  * the inner products of the two-loop recursion and of the initial scaling s'y / y'y run over the free coefficients of
    the current iterate; rho of a pair is 1 / s'y of the whole pair, from the moment it was stored.  With any rho > 0 the
    matrix of the recursion stays positive definite on the free coefficients (V'HV + rho ss'), so g'd < 0 holds in exact
    arithmetic; a scaling that is not positive or not finite shows in g'd and is caught by the safeguard.
  * Armijo uses the projected displacement, J + 1e-4 g'(vt - v).  A quasi-Newton direction can be clipped by the
    projection until g'(vt - v) is no longer negative; such a trial point is a rejection whatever its objective, so J never
    increases.  On SPG's direction v + lam d stays inside the box and g'(vt - v) = lam g'd < 0 always.
  * the Barzilai-Borwein step length alpha is updated after every accepted step exactly as in SPG, whether or not the pair
    is stored; a pair is stored iff s'y > 2.2e-16 y'y (a NaN fails the test).
  * the first trial point on SPG's direction is P(v - alpha g) itself, so a coefficient that reaches a bound is on it
    exactly and the equality tests of the active set mean what they say.
  * `memory` (SPG's non-monotone history) has no meaning here: the line search is monotone."""
import numpy as np

from tests.spg_twin import (INDECISIVE_CAP, _dot, _proj, _rel, decide, decide_sign, goes_on, halve_step, make_inputs, note,
                            run_twin, take_step)

EPS_PAIR = 2.2e-16


def _col(A, slot):                                      # A [pairs][...][B], slot [B] -> A[slot[b], ..., b]
    return np.take_along_axis(A, slot.reshape((1,) * (A.ndim - 1) + (-1,)), axis=0)[0]


def _lands(st, who, w):     # trial point P(w): a coefficient that moves and lands next to a bound decides whether it is on it
    near = np.minimum(_rel(w, st.lb[:, None]), _rel(w, st.ub[:, None]))
    near = np.where((st.lam * st.d != 0.0) & np.isfinite(w), near, np.inf).min(axis=0)
    note(st, "lands on a bound", who, near)


def _lbfgs_start(st):                                   # the pair rings are empty
    nV, B = st.v.shape
    st.S, st.Y = np.zeros((st.pairs, nV, B)), np.zeros((st.pairs, nV, B))
    st.rho = np.zeros((st.pairs, B))
    st.head, st.count = np.zeros(B, dtype=np.int64), np.zeros(B, dtype=np.int64)


def _lbfgs_direction(st):                               # k_lbfgs_direction
    v, g, lb, ub, pairs, head = st.v, st.g, st.lb, st.ub, st.pairs, st.head
    goes_on(st)
    # active set: on a bound with the gradient pushing outward
    onl, onu = v == lb[:, None], v == ub[:, None]
    fr = ~((onl & (g > 0.0)) | (onu & (g < 0.0)))
    gmax = np.fmax.reduce(np.abs(g), axis=0, initial=0.0)
    decide_sign(st, "active set", st.active, np.where(onl | onu, np.abs(g), np.inf).min(axis=0), gmax)
    # two-loop recursion on the free coefficients, newest pair first (lbfgs_slot)
    qn = st.active & (st.count > 0)
    q = np.where(fr, g, 0.0)
    al = np.zeros((pairs, v.shape[1]))
    for j in range(pairs):
        use = qn & (j < st.count)
        slot = (head + pairs - 1 - j) % pairs
        sj, yj = _col(st.S, slot), _col(st.Y, slot)
        a = _col(st.rho, slot) * _dot(sj, q, fr)
        al[j] = a
        q = np.where(use & fr, q - a * yj, q)
    slot = (head + pairs - 1) % pairs
    s0, y0 = _col(st.S, slot), _col(st.Y, slot)
    gamma = _dot(s0, y0, fr) / _dot(y0, y0, fr)
    r = gamma * q
    for j in range(pairs - 1, -1, -1):
        use = qn & (j < st.count)
        slot = (head + pairs - 1 - j) % pairs
        sj, yj = _col(st.S, slot), _col(st.Y, slot)
        beta = _col(st.rho, slot) * _dot(yj, r, fr)
        r = np.where(use & fr, r + sj * (al[j] - beta), r)
    dq = st.bump(np.where(fr, -r, 0.0))
    dq = np.where(fr, dq, 0.0)                          # the probe leaves the zeros of the active set alone
    gtd = _dot(g, dq)
    # safeguard: not a finite descent direction -> drop the pairs, SPG's direction
    decide_sign(st, "g'd < 0", qn, gtd, _dot(np.abs(g), np.abs(dq)))
    st.reset = qn & ~((gtd < 0.0) & np.isfinite(gtd))
    st.count = np.where(st.reset, 0, st.count)
    st.qn = qn & ~st.reset
    ds = st.bump(_proj(v - st.alpha * g, lb, ub) - v)   # spg_direction
    st.d = np.where(st.active, np.where(st.qn, dq, ds), 0.0)
    st.lam = np.ones(v.shape[1])
    w = np.where(st.qn, v + st.d, v - st.alpha * g)     # spg_direction, L-BFGS's form: the projection itself (see above)
    st.vt = np.where(st.active, _proj(w, lb, ub), v)    # a finished instance's trial point is its v
    _lands(st, st.active, w)
    st.gts = _dot(g, st.vt - v)                         # lbfgs_gts


def _lbfgs_accept(st, pending):                         # k_lbfgs_accept
    rhs = st.J + 1e-4 * st.gts
    decide_sign(st, "g'(vt - v) < 0", pending, st.gts, _dot(np.abs(st.g), np.abs(st.vt - st.v)))
    decide(st, "Armijo", pending & (st.gts < 0.0), st.Jt, rhs)
    ok = pending & (st.gts < 0.0) & (st.Jt <= rhs)      # a NaN Jt is a rejection
    rej = pending & ~ok
    halve_step(st, rej)
    _lands(st, rej, st.v + st.lam * st.d)
    st.gts = np.where(rej, _dot(st.g, st.vt - st.v), st.gts)
    return ok, rhs


def _lbfgs_update(st, started):                         # k_lbfgs_update
    pairs, head, qn = st.pairs, st.head, st.qn
    st.iters += st.active
    take = st.active & (st.accepted == 2)
    s, y, sty, tolx = take_step(st, take)
    yty = _dot(y, y)                                    # step_rows' first pass, with y'y
    decide(st, "pair stored", take, sty, EPS_PAIR * yty)
    store = take & (sty > EPS_PAIR * yty)               # a NaN fails the test
    at = (head[None, None, :] == np.arange(pairs)[:, None, None]) & store[None, None, :]
    st.S = np.where(at, s[None], st.S)
    st.Y = np.where(at, y[None], st.Y)
    st.rho = np.where(at[:, 0, :], (1.0 / sty)[None], st.rho)
    st.head = np.where(store, (head + 1) % pairs, head)
    st.count = np.where(store, np.minimum(st.count + 1, pairs), st.count)
    failed = started & ~take
    st.count = np.where(failed & qn, 0, st.count)       # a failed search on a quasi-Newton direction: drop the pairs, go on
    st.active = (take & ~tolx) | (failed & qn)          # on SPG's direction the instance stops where it is
    return take, tolx, dict(qn=qn.copy(), reset=st.reset, stored=store, skipped=take & ~store, sty=sty, count=st.count.copy())


def lbfgs_twin(evaluate, v0, Lb, Ub, TolX, TolFun, MaxIter, maxBacktracks, pairs=8, memory=None, ulp_seed=None):
    """evaluate(V [nV][B]) -> (J [B], G [nV][B]), always called on the whole batch.  With `ulp_seed` every computed
    direction d and step length alpha is moved by one ulp in a seeded random direction.  Returns what spg_twin returns
    (v, J, iterations, converged, pgn, backtracks, margin, active, snap, steps) and margins (margin per kind of decision); a
    step record has in addition qn (the direction was a quasi-Newton one), reset (the safeguard dropped the pairs), stored /
    skipped (the pair of an accepted step was stored / failed its test), sty, count (pairs held after the iteration)."""
    r, st = run_twin(evaluate, v0, Lb, Ub, TolX, TolFun, MaxIter, maxBacktracks, ulp_seed,
                     (_lbfgs_start, _lbfgs_direction, _lbfgs_accept, _lbfgs_update), pairs=pairs)
    r.margins = st.margins
    return r


def counted(evaluate):
    """evaluate with a call counter: batch evaluations are what the GPU pays for"""
    def ev(V):
        ev.calls += 1
        return evaluate(V)
    ev.calls = 0
    return ev


def check_lbfgs_invariants(tw):
    """beyond spg_twin.check_invariants: J never increases, every stored pair has s'y > 0"""
    for k in range(len(tw.snap) - 1):
        assert np.all(tw.snap[k + 1].J <= tw.snap[k].J), k
    for it, st in enumerate(tw.steps):
        assert np.all(st.sty[st.stored] > 0.0), it
        assert not (st.stored & ~st.accepted).any()


# ---------------------------------------------------------------------------------------------------------------
# the table of cases of tests/test_lbfgs_twin.py and tests/test_gpu_shooting_lbfgs.py: a row of spg_twin.CASES with
# entries replaced (make_inputs draws the numbers), plus `pairs`
LCASES = {
    # TolFun of the bounded cases is 3e-3: with J near 100 an instance that goes on to a smaller projected gradient takes
    # steps whose decrease is below 1e-9 J, and every Armijo test of such a step counts as indecisive (DECISIVE_MARGIN)
    # (a), (b), (c) the ring of 3 pairs wraps, active bounds at the solution, safeguard resets; two workgroups with a last
    # one of one thread
    "ring257": ("blocks257", dict(nB=15, T=20.0, TolFun=3e-3, K=12, pairs=3, seed=111)),
    "ring600": ("blocks600", dict(nB=11, T=12.0, TolFun=3e-3, K=10, pairs=8, seed=112)),
    # (c), (d) instances next to a non-finite trial point and three evaluations per line search: pairs that fail their
    # test, failed searches on a quasi-Newton direction that go on with an accepted step on SPG's
    "fail257": ("exhausted2", dict(batch=257, nB=11, K=12, pairs=3, blowup=80, TolX=2e-3, TolFun=3e-3, maxBacktracks=3,
                                   seed=131)),
    # (e) a free initial state inside FreeStateBounds
    "free257": ("free", dict(batch=257, nB=11, K=10, pairs=4, seed=161)),
    # (f) Chebyshev, no bounds
    "cheb257": ("cheb64on", dict(batch=257, nB=11, N=48, K=10, pairs=8, fusion=None, seed=171)),
}
# the purpose at GPU-test size: the defaults of single_shooting.m on a long horizon, run until every instance has stopped
PURPOSE_GPU = ("blocks257", dict(nB=21, N=60, T=50.0, K=120, pairs=8, TolFun=3e-4, TolX=1e-5, memory=10, seed=181))
# and on the CPU oracle: 41 control points, a grid of 200 steps
PURPOSE_CPU = ("blocks257", dict(batch=16, nB=41, N=200, T=40.0, K=500, pairs=8, TolFun=3e-4, TolX=1e-5, memory=10, seed=5))


def make_case(name):
    base, over = name if isinstance(name, tuple) else LCASES[name]
    over = dict(over)
    pairs = over.pop("pairs")
    c = make_inputs(base, **over)
    c.name, c.pairs = (name if isinstance(name, str) else "purpose"), pairs
    return c


def check_case_purpose(c, tw, dec, Lb, Ub):
    """what the case was made for occurs among the decisive instances `dec` of the twin run `tw`"""
    name, B = c.name, c.batch
    assert np.count_nonzero(~dec) <= INDECISIVE_CAP * B, (name, "indecisive", int(np.count_nonzero(~dec)), B)
    moved = np.any([st.accepted for st in tw.steps], axis=0)
    qn_moved = np.any([st.accepted & st.qn for st in tw.steps], axis=0)
    stored = np.sum([st.stored for st in tw.steps], axis=0)
    on = (tw.v == Lb[:, None]) | (tw.v == Ub[:, None])
    assert np.count_nonzero(dec & qn_moved) >= B // 2, "accepted steps on quasi-Newton directions"
    assert B % 256 != 0 and (dec & moved)[256:].any(), "second workgroup, ragged last one"
    if name.startswith("ring"):
        assert np.count_nonzero(dec & (stored > c.pairs)) >= (B // 4 if c.pairs == 3 else 1), "(b) the ring wraps"
        held = on.any(axis=0) & (~on).any(axis=0) & ~tw.active
        assert np.count_nonzero(dec & held) >= B // 4, "(a) a non-empty active set at the solution"
        assert np.any([st.reset & dec for st in tw.steps]) or np.any([st.skipped & dec for st in tw.steps]), "(c)"
        if B > 512:
            assert (dec & qn_moved)[512:].any(), "third workgroup"
    if name == "fail257":
        assert sum(np.count_nonzero(st.skipped & dec) for st in tw.steps) >= 5, "(c) pairs that fail s'y > eps y'y"
        then_spg = [a.failed & a.qn & b.accepted & ~b.qn & dec for a, b in zip(tw.steps[:-1], tw.steps[1:])]
        assert np.count_nonzero(np.any(then_spg, axis=0)) >= 5, "(d) a failed quasi-Newton search, then an accepted SPG step"
        for a, b in zip(tw.steps[:-1], tw.steps[1:]):
            f = a.failed & a.qn
            assert np.all(a.count[f] == 0) and not b.qn[f].any() and b.started[f].all()
        assert np.any([~np.isfinite(st.Jt0) & st.started & dec for st in tw.steps]), "a non-finite trial point"
    if name == "free257":
        tail = tw.v[-1]
        onb = (tail == Lb[-1]) | (tail == Ub[-1])
        assert np.isfinite([Lb[-1], Ub[-1]]).all()
        assert np.count_nonzero(dec & onb) >= 5 and np.count_nonzero(dec & ~onb & qn_moved) >= 5, "(e) free state on its bound and inside"
    if name == "cheb257":
        assert np.isinf(Lb).all() and np.isinf(Ub).all(), "(f)"
