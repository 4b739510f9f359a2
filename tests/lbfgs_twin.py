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
from types import SimpleNamespace

import numpy as np

from tests.spg_twin import _dot, _pgn, _proj, _rel

EPS_PAIR = 2.2e-16


def _dotf(a, b, fr):                                    # running sum over the free rows only, row after row
    s = np.zeros(a.shape[1])
    for i in range(a.shape[0]):
        s = s + np.where(fr[i], a[i] * b[i], 0.0)
    return s


def _col(A, slot):                                      # A [pairs][...][B], slot [B] -> A[slot[b], ..., b]
    return np.take_along_axis(A, slot.reshape((1,) * (A.ndim - 1) + (-1,)), axis=0)[0]


def lbfgs_twin(evaluate, v0, Lb, Ub, TolX, TolFun, MaxIter, maxBacktracks, pairs=8, memory=None, ulp_seed=None):
    """evaluate(V [nV][B]) -> (J [B], G [nV][B]), always called on the whole batch.  With `ulp_seed` every computed
    direction d and step length alpha is moved by one ulp in a seeded random direction.  Returns what spg_twin returns
    (v, J, iterations, converged, pgn, backtracks, margin, active, snap, steps); a step record has in addition qn (the
    direction was a quasi-Newton one), reset (the safeguard dropped the pairs), stored / skipped (the pair of an accepted
    step was stored / failed its test), sty, count (pairs held after the iteration)."""
    v = np.array(v0, dtype=np.float64, copy=True)
    nV, B = v.shape
    lb = np.full(nV, -np.inf) if Lb is None else np.asarray(Lb, dtype=np.float64).ravel()
    ub = np.full(nV, np.inf) if Ub is None else np.asarray(Ub, dtype=np.float64).ravel()
    rng = None if ulp_seed is None else np.random.default_rng(ulp_seed)

    def bump(x):
        if rng is None:
            return x
        return np.nextafter(x, np.where(rng.integers(0, 2, size=x.shape) == 1, np.inf, -np.inf))

    margin = np.full(B, np.inf)
    margins = {}                                        # the same per kind of decision (for the reader of a failing case)

    def note(what, mask, r):
        margin[mask] = np.minimum(margin, r)[mask]
        m = margins.setdefault(what, np.full(B, np.inf))
        m[mask] = np.minimum(m, r)[mask]

    def decide(what, mask, a, b):                       # the instances of `mask` take the comparison a ? b
        note(what, mask, _rel(a, b))

    def decide_sign(what, mask, value, scale):          # the sign of `value`, measured on the scale of its terms
        r = np.abs(value) / np.fmax(scale, 1e-300)
        note(what, mask, np.where(np.isnan(r), np.inf, r))

    def trial(lam, d, who, vt_old, full_spg):
        """vt = P(v + lam d) for the instances `who`; a coefficient that moves and lands next to a bound decides whether
        it is on it (active-set membership of the next iterate).  SPG's full step is P(v - alpha g) itself, not
        P(v + d): v + ((ub - v) rounded) can end one ulp inside the box, and the active set asks for equality"""
        w = np.where(full_spg, v - alpha * g, v + lam * d)
        vt = _proj(w, lb, ub)
        near = np.minimum(_rel(w, lb[:, None]), _rel(w, ub[:, None]))
        near = np.where((lam * d != 0.0) & np.isfinite(w), near, np.inf).min(axis=0)
        note("lands on a bound", who, near)
        return np.where(who, vt, vt_old)

    snap, steps = [], []

    def snapshot():                                     # k_spg_finish
        pgn = _pgn(v, g, lb, ub)
        snap.append(SimpleNamespace(v=v.copy(), J=J.copy(), iterations=iters.copy(), active=active.copy(), pgn=pgn,
                                    converged=pgn <= 10.0 * TolFun,
                                    margin=np.minimum(margin, _rel(pgn, 10.0 * TolFun))))

    with np.errstate(all="ignore"):
        J, g = evaluate(v)
        J, g = np.array(J, dtype=np.float64), np.array(g, dtype=np.float64)
        # k_spg_init: the first step length; the pair rings are empty
        alpha = bump(1.0 / np.fmax(_pgn(v, g, lb, ub), 1e-12))
        active = np.ones(B, dtype=bool)
        iters = np.zeros(B, dtype=np.int64)
        S, Y = np.zeros((pairs, nV, B)), np.zeros((pairs, nV, B))
        rho = np.zeros((pairs, B))
        head, count = np.zeros(B, dtype=np.int64), np.zeros(B, dtype=np.int64)
        snapshot()
        for it in range(MaxIter):
            # k_lbfgs_direction: stopping test
            pgn = _pgn(v, g, lb, ub)
            decide("pgn <= TolFun", active, pgn, TolFun)
            active = active & (pgn > TolFun)
            accepted = np.where(active, 0, 1)
            # active set: on a bound with the gradient pushing outward
            onl, onu = v == lb[:, None], v == ub[:, None]
            fr = ~((onl & (g > 0.0)) | (onu & (g < 0.0)))
            gmax = np.fmax.reduce(np.abs(g), axis=0, initial=0.0)
            decide_sign("active set", active, np.where(onl | onu, np.abs(g), np.inf).min(axis=0), gmax)
            # two-loop recursion on the free coefficients, newest pair first
            qn = active & (count > 0)
            q = np.where(fr, g, 0.0)
            al = np.zeros((pairs, B))
            for j in range(pairs):
                use = qn & (j < count)
                slot = (head + pairs - 1 - j) % pairs
                sj, yj = _col(S, slot), _col(Y, slot)
                a = _col(rho, slot) * _dotf(sj, q, fr)
                al[j] = a
                q = np.where(use & fr, q - a * yj, q)
            slot = (head + pairs - 1) % pairs
            s0, y0 = _col(S, slot), _col(Y, slot)
            gamma = _dotf(s0, y0, fr) / _dotf(y0, y0, fr)
            r = gamma * q
            for j in range(pairs - 1, -1, -1):
                use = qn & (j < count)
                slot = (head + pairs - 1 - j) % pairs
                sj, yj = _col(S, slot), _col(Y, slot)
                beta = _col(rho, slot) * _dotf(yj, r, fr)
                r = np.where(use & fr, r + sj * (al[j] - beta), r)
            dq = bump(np.where(fr, -r, 0.0))
            dq = np.where(fr, dq, 0.0)                  # the probe leaves the zeros of the active set alone
            gtd = _dot(g, dq)
            # safeguard: not a finite descent direction -> drop the pairs, SPG's direction
            decide_sign("g'd < 0", qn, gtd, _dot(np.abs(g), np.abs(dq)))
            reset = qn & ~((gtd < 0.0) & np.isfinite(gtd))
            count = np.where(reset, 0, count)
            qn = qn & ~reset
            ds = bump(_proj(v - alpha * g, lb, ub) - v)
            d = np.where(qn, dq, ds)
            d = np.where(active, d, 0.0)
            lam = np.ones(B)
            vt = trial(lam, d, active, v, ~qn)             # a finished instance's trial point is its v
            gts = _dot(g, vt - v)
            if not active.any():
                break
            started = active.copy()
            nbt = np.zeros(B, dtype=np.int64)
            lhs, rhs_at, Jt0 = np.full(B, np.nan), np.full(B, np.nan), None
            for ls in range(maxBacktracks):
                Jt, gt = evaluate(vt)
                Jt, gt = np.array(Jt, dtype=np.float64), np.array(gt, dtype=np.float64)
                Jt0 = Jt.copy() if ls == 0 else Jt0
                # k_lbfgs_accept
                pending = accepted == 0
                rhs = J + 1e-4 * gts
                decide_sign("g'(vt - v) < 0", pending, gts, _dot(np.abs(g), np.abs(vt - v)))
                decide("Armijo", pending & (gts < 0.0), Jt, rhs)
                ok = pending & (gts < 0.0) & (Jt <= rhs)    # a NaN Jt is a rejection
                accepted[ok] = 2
                lhs[ok], rhs_at[ok] = Jt[ok], rhs[ok]
                rej = pending & ~ok
                lam = np.where(rej, 0.5 * lam, lam)
                vt = trial(lam, d, rej, vt, np.zeros(B, dtype=bool))
                gts = np.where(rej, _dot(g, vt - v), gts)
                nbt += rej
                if not rej.any():
                    break
            # k_lbfgs_update
            iters += active
            take = active & (accepted == 2)
            s, y = vt - v, gt - g
            sty, sts, yty = _dot(s, y), _dot(s, s), _dot(y, y)
            smax = np.fmax.reduce(np.abs(s), axis=0, initial=0.0)
            v = np.where(take, vt, v)
            g = np.where(take, gt, g)
            J = np.where(take, Jt, J)
            decide("s'y > 0", take, sty, 0.0)
            decide_sign("s'y > 0", take, sty, _dot(np.abs(s), np.abs(y)))
            an = np.where(sty > 0.0, sts / np.fmax(sty, 1e-300), 1e3)
            alpha = np.where(take, bump(np.fmin(np.fmax(an, 1e-10), 1e10)), alpha)
            decide("pair stored", take, sty, EPS_PAIR * yty)
            store = take & (sty > EPS_PAIR * yty)
            at = (head[None, None, :] == np.arange(pairs)[:, None, None]) & store[None, None, :]
            S = np.where(at, s[None], S)
            Y = np.where(at, y[None], Y)
            rho = np.where(at[:, 0, :], (1.0 / sty)[None], rho)
            head = np.where(store, (head + 1) % pairs, head)
            count = np.where(store, np.minimum(count + 1, pairs), count)
            decide("step <= TolX", take, smax, TolX)
            tolx = take & (smax <= TolX)
            failed = started & ~take
            count = np.where(failed & qn, 0, count)     # a failed search on a quasi-Newton direction: drop the pairs, go on
            active = (take & ~tolx) | (failed & qn)     # on SPG's direction the instance stops where it is
            steps.append(SimpleNamespace(started=started, accepted=take, failed=failed, tolx=tolx, backtracks=nbt, Jt=lhs,
                                         rhs=rhs_at, lam=lam.copy(), Jt0=Jt0, qn=qn.copy(), reset=reset, stored=store,
                                         skipped=take & ~store, sty=sty, count=count.copy()))
            snapshot()
        while len(snap) < MaxIter + 1:
            snapshot()
    last = snap[-1]
    return SimpleNamespace(v=last.v, J=last.J, iterations=last.iterations, converged=last.converged, pgn=last.pgn,
                           backtracks=np.array([s.backtracks for s in steps]).reshape(len(steps), B),
                           margin=last.margin, margins=margins, active=last.active, snap=snap, steps=steps)


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
    from tests.spg_twin import make_inputs
    base, over = name if isinstance(name, tuple) else LCASES[name]
    over = dict(over)
    pairs = over.pop("pairs")
    c = make_inputs(base, **over)
    c.name, c.pairs = (name if isinstance(name, str) else "purpose"), pairs
    return c


def check_case_purpose(c, tw, dec, Lb, Ub):
    """what the case was made for occurs among the decisive instances `dec` of the twin run `tw`"""
    from tests.spg_twin import INDECISIVE_CAP
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
