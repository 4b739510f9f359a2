"""The opt-in tiled device layout (include/ocs.h, ocs_integrator_set_layout) on the GPU: converters, the pass pair, pad lanes
and bounds, refusals, handle reuse.

Every comparison between layouts is np.array_equal: a trajectory's arithmetic does not depend on where its operands live, so
a difference of one ulp is a defect.  The batch-minor reference runs the kernels the tiled layout runs: the pipeline state pass
and the scan adjoint pass forced, the lane kernels where N is below a block (8) / a chunk (4) -- the tiled layout takes them
for exactly those steps -- and, where the batch-minor pipeline kernel refuses the batch (below a tile of 64 / nS trajectories,
or odd), at that tile's batch with the trajectories repeated: the project pins these kernels bit for bit across batch sizes.
Oracle tolerance: 1e-12 relative against max(1, |ref|), the bar of tests/test_gpu_rk4_parity.py for every mapping."""

import numpy as np
import pytest

from tests.user_problems import LOGISTIC_ROWS_SRC, lq_matrices

pytestmark = pytest.mark.gpu

C_, R_ = 1.5, 0.05
M4 = [3.0, 2.5, 2.0, 1.5]
BOUNDS = [[0.0, 1.0]]
RTOL = 1e-12
SHAPES = [(nS, N, B) for nS in (1, 2, 4) for N in (1, 8, 11, 13, 37) for B in (1, 70, 128)] + [(4, 16, 4112)]
CONV = [(rows, cols, B) for rows in (1, 5) for cols in (1, 9) for B in (1, 15, 16, 17, 70)]
GUARD = 4096   # doubles of sentinel on either side: more than a whole tile of the largest array guarded (38 x 5 x 16)
SENT = -7.25e77


@pytest.fixture(scope="module")
def ocs():
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    import __graft_entry__ as g
    return g.load_package()


def relerr(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    if not (np.isfinite(a).all() and np.isfinite(b).all()):
        return float("inf")
    return float(np.max(np.abs(a - b) / np.maximum(1.0, np.abs(b))))


def _tspan(N, grid):
    s = np.arange(N + 1) / N
    if grid == "nonuniform":
        s = s ** 1.5
    return 0.01 * N * s   # steps of about 0.01, BL-2's


def _inputs(nS, N, B, seed):
    rng = np.random.default_rng(seed)
    f, ph = rng.uniform(0, 1, B), rng.uniform(0, 2 * np.pi, B)
    t = np.linspace(0.0, 0.01 * N, 2 * N + 1)
    u = np.clip(0.25 + 0.2 * np.sin(2 * np.pi * f[None, :] * t[:, None] + ph[None, :]), 0, 1)[:, None, :]   # [2N+1][1][B]
    x0 = rng.uniform(0.8, 2.5, (nS, B))
    lamT = rng.normal(size=(nS + 1, B))
    return np.ascontiguousarray(x0), np.ascontiguousarray(u), np.ascontiguousarray(lamT)


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _prob(ocs, nS):
    return ocs.LogisticProblem(M4[:nS], C_, R_, BOUNDS)


def _ref_batch(nS, N, B):
    """the batch the batch-minor reference runs at: B where its pipeline kernel takes it (ocs_internal.hpp, tile_ok)"""
    tpw = 64 // nS
    if N < 8 or B % tpw == 0 or (B > tpw and B % 2 == 0):
        return B
    return -(-B // tpw) * tpw


def run_default(ocs, nS, N, B, grid, x0, u, lamT, g=None):
    """x, J, and the three adjoint cases in the batch-minor layout (numpy, [cols][rows][B])"""
    import torch
    Br = _ref_batch(nS, N, B)
    rep = np.arange(Br) % B
    x0r, ur, lTr = x0[:, rep], u[:, :, rep], lamT[:, rep]
    p = _prob(ocs, nS)
    g = g or ocs.RK4Integrator(_tspan(N, grid))
    g.set_layout("batch_minor")
    dx0, du, dlT = _dev(x0r), _dev(ur), _dev(lTr)
    x = torch.empty((N + 1, nS + 1, Br), dtype=torch.float64, device="cuda")
    g.set_mapping("pipeline" if N >= 8 else "lane")
    _, J = g.compute_states_dev(p, dx0, du, x)
    g.set_mapping("scan" if N >= 4 else "lane")
    out = {"x": x.cpu().numpy()[:, :, :B], "J": J.cpu().numpy()[:B]}
    for case in ("both", "lam", "lamT"):
        lam = torch.empty((N + 1, nS + 1, Br), dtype=torch.float64, device="cuda")
        dJ = None if case == "lam" else torch.empty((2 * N + 1, 1, Br), dtype=torch.float64, device="cuda")
        g.compute_adjoints_dev(p, du, dlT if case == "lamT" else None, lam, dJ)
        out[case] = (lam.cpu().numpy()[:, :, :B], None if dJ is None else dJ.cpu().numpy()[:, :, :B])
    g.set_mapping("auto")
    return out


def run_tiled(ocs, nS, N, B, grid, x0, u, lamT, g=None):
    """the same through tiled arrays, converted back"""
    import torch
    p = _prob(ocs, nS)
    g = g or ocs.RK4Integrator(_tspan(N, grid))
    g.set_layout("tiled")
    dx0, dlT = _dev(x0), _dev(lamT)
    ut = ocs.to_tiled(_dev(u))
    xt = torch.empty(ocs.tiled_doubles(nS + 1, N + 1, B), dtype=torch.float64, device="cuda")
    _, J = g.compute_states_dev(p, dx0, ut, xt)
    out = {"x": ocs.from_tiled(xt, nS + 1, N + 1, B).cpu().numpy(), "J": J.cpu().numpy()}
    for case in ("both", "lam", "lamT"):
        lam = torch.empty_like(xt)
        dJ = None if case == "lam" else torch.empty_like(ut)
        g.compute_adjoints_dev(p, ut, dlT if case == "lamT" else None, lam, dJ, batch=B)
        out[case] = (ocs.from_tiled(lam, nS + 1, N + 1, B).cpu().numpy(),
                     None if dJ is None else ocs.from_tiled(dJ, 1, 2 * N + 1, B).cpu().numpy())
    g.set_layout("batch_minor")
    return out


_CACHE = {}


def both(ocs, nS, N, B, grid):
    """reference and tiled results of a shape, computed once and shared by the tests that read them"""
    key = (nS, N, B, grid)
    if key not in _CACHE:
        x0, u, lamT = _inputs(nS, N, B, seed=1000 * nS + 10 * N + B % 7)
        _CACHE[key] = (x0, u, lamT, run_default(ocs, nS, N, B, grid, x0, u, lamT), run_tiled(ocs, nS, N, B, grid, x0, u, lamT))
    return _CACHE[key]


# ---- 1. converters ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows,cols,B", CONV)
def test_converters_follow_the_index_map(ocs, rows, cols, B):
    rng = np.random.default_rng(rows * 100 + cols * 10 + B)
    a = rng.normal(size=(cols, rows, B))
    t = ocs.to_tiled(_dev(a)).cpu().numpy()
    ix = ocs.tiled_index(rows, cols, B)
    assert t.size == ocs.tiled_doubles(rows, cols, B)
    assert np.array_equal(t[ix], a)
    # pad lanes: copies of the last trajectory
    tiles = -(-B // 16)
    full = t.reshape(tiles, cols, rows, 16)
    for l in range(B - (tiles - 1) * 16, 16):
        assert np.array_equal(full[-1, :, :, l], a[:, :, B - 1])
    back = ocs.from_tiled(_dev(t), rows, cols, B).cpu().numpy()
    assert np.array_equal(back, a)


# ---- 2. state pass ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("grid", ["linspace", "nonuniform"])
@pytest.mark.parametrize("nS,N,B", SHAPES)
def test_state_pass_same_bits_in_both_layouts(ocs, oracle, nS, N, B, grid):
    x0, u, _, d, t = both(ocs, nS, N, B, grid)
    assert np.array_equal(t["x"], d["x"])
    assert np.array_equal(t["J"], d["J"])
    sel = sorted({0, B // 2, B - 1})
    po = oracle.LogisticProblem(M4[:nS], C_, R_, BOUNDS)
    ref = oracle.batch_states_adjoints(po, _tspan(N, grid), x0[:, sel], np.asfortranarray(u[:, :, sel].transpose(1, 0, 2)),
                                       want=("x", "J"))
    assert relerr(t["x"][:, :, sel].transpose(1, 0, 2), ref["x"]) < RTOL
    assert relerr(t["J"][sel], ref["J"]) < RTOL


# ---- 3. adjoint pass -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["both", "lam", "lamT"])
@pytest.mark.parametrize("nS,N,B", SHAPES)
def test_adjoint_pass_same_bits_in_both_layouts(ocs, nS, N, B, case):
    _, _, _, d, t = both(ocs, nS, N, B, "linspace")
    assert np.array_equal(t[case][0], d[case][0])
    if case != "lam":
        assert np.array_equal(t[case][1], d[case][1])


# ---- 4. pad lanes and bounds ----------------------------------------------------------------------------------------
def _guarded(n, fill=None):
    """a flat array of n doubles between two sentinel guards (fill: a numpy array to start from, returned in its shape)"""
    import torch
    big = torch.full((n + 2 * GUARD,), SENT, dtype=torch.float64, device="cuda")
    mid = big[GUARD:GUARD + n]
    if fill is not None:
        mid.copy_(_dev(fill).reshape(-1))
        mid = mid.view(fill.shape)
    return big, mid


def _guards_intact(big):
    h = big.cpu().numpy()
    return bool(np.all(h[:GUARD] == SENT) and np.all(h[-GUARD:] == SENT))


def _pad_positions(ocs, rows, cols, B):
    import torch
    n = ocs.tiled_doubles(rows, cols, B)
    return torch.from_numpy(np.setdiff1d(np.arange(n), ocs.tiled_index(rows, cols, B).ravel())).cuda()


@pytest.mark.parametrize("nS,N", [(1, 13), (2, 37), (4, 11), (4, 8)])
def test_pad_lanes_and_bounds(ocs, nS, N):
    import torch
    B = 70   # 10 pad lanes in the fifth tile; with nS = 1, 2 the second workgroup's tiles reach past the arrays
    x0, u, lamT, d, _ = both(ocs, nS, N, B, "linspace")
    p, g = _prob(ocs, nS), ocs.RK4Integrator(_tspan(N, "linspace")).set_layout("tiled")
    nx, nu = ocs.tiled_doubles(nS + 1, N + 1, B), ocs.tiled_doubles(1, 2 * N + 1, B)
    bu, ut = _guarded(nu)
    ocs.to_tiled(_dev(u), out=ut)
    ut[_pad_positions(ocs, 1, 2 * N + 1, B)] = float("nan")
    bx, xt = _guarded(nx)
    b0, dx0 = _guarded(x0.size, x0)     # the untiled arrays are guarded too: nothing outside [0, B) of them
    bT, dlT = _guarded(lamT.size, lamT)
    bJ, J = _guarded(B)
    g.compute_states_dev(p, dx0, ut, xt, J)
    Jh = J.cpu().numpy()
    assert np.isfinite(Jh).all() and np.array_equal(Jh, d["J"])
    assert np.array_equal(ocs.from_tiled(xt.clone(), nS + 1, N + 1, B).cpu().numpy(), d["x"])
    xt[_pad_positions(ocs, nS + 1, N + 1, B)] = float("nan")   # checkpoint input of the adjoint pass
    for case in ("both", "lam", "lamT"):
        bl, lam = _guarded(nx)
        bd, dJ = _guarded(nu) if case != "lam" else (None, None)
        g.compute_adjoints_dev(p, ut, dlT if case == "lamT" else None, lam, dJ, batch=B)
        assert np.array_equal(ocs.from_tiled(lam.clone(), nS + 1, N + 1, B).cpu().numpy(), d[case][0])
        assert _guards_intact(bl)
        if dJ is not None:
            assert np.array_equal(ocs.from_tiled(dJ.clone(), 1, 2 * N + 1, B).cpu().numpy(), d[case][1])
            assert _guards_intact(bd)
    assert _guards_intact(bu) and _guards_intact(bx) and _guards_intact(b0) and _guards_intact(bT) and _guards_intact(bJ)
    assert np.array_equal(dx0.cpu().numpy(), x0) and np.array_equal(dlT.cpu().numpy(), lamT)   # inputs are inputs


# ---- 5. refusals -----------------------------------------------------------------------------------------------------
def _refused(ocs, fn, word):
    with pytest.raises(ocs._lib.OcsError) as e:
        fn()
    assert e.value.code == -6 and word in str(e.value), str(e.value)


def test_refusals_name_the_reason(ocs):
    import torch
    nS, N, B = 2, 16, 64
    x0, u, lamT = _inputs(nS, N, B, seed=5)
    ts = _tspan(N, "linspace")
    g = ocs.RK4Integrator(ts).set_layout("tiled")
    dx0, ut = _dev(x0), ocs.to_tiled(_dev(u))
    xt = torch.empty(ocs.tiled_doubles(nS + 1, N + 1, B), dtype=torch.float64, device="cuda")

    def states(gg, p, nS_=nS, nC=1):
        n = ocs.tiled_doubles(nS_ + 1, N + 1, B)
        gg.compute_states_dev(p, torch.ones((nS_, B), dtype=torch.float64, device="cuda"),
                              torch.zeros(ocs.tiled_doubles(nC, 2 * N + 1, B), dtype=torch.float64, device="cuda"),
                              torch.empty(n, dtype=torch.float64, device="cuda"))

    A, Bu, q, rdiag = lq_matrices(16, 4)
    _refused(ocs, lambda: states(g, ocs.LQProblem(A, Bu, q, rdiag, R_, [[-1.0, 1.0]] * 4), 16, 4), "LQ")
    _refused(ocs, lambda: states(g, ocs.UserProblem(LOGISTIC_ROWS_SRC, 2, 1, [C_, R_] + M4[:2], BOUNDS, row_separable=True)),
             "plugin")
    _refused(ocs, lambda: states(g, _prob(ocs, 3), 3), "nS = 3")
    pb = _prob(ocs, nS)
    pb.set_batch_params([0], np.linspace(2.0, 3.0, B)[None, :])
    _refused(ocs, lambda: states(g, pb), "per-trajectory")
    gi = ocs.RK4InfiniteIntegrator(ts, ts[-1] + ts[:9], [0.4]).set_layout("tiled")
    _refused(ocs, lambda: states(gi, _prob(ocs, nS)), "RK4InfiniteIntegrator")
    p = _prob(ocs, nS)
    for m in ("lane", "rowsplit"):
        g.set_mapping(m)
        _refused(ocs, lambda: states(g, p), "mapping")
    g.set_mapping("auto")
    # ... and at compute_adjoints_dev: a state pass that the tiled layout takes, then a setting it does not cover
    g.compute_states_dev(p, dx0, ut, xt)
    lamt = torch.empty_like(xt)
    for m in ("lane", "rowsplit"):
        g.set_mapping(m)
        _refused(ocs, lambda: g.compute_adjoints_dev(p, ut, None, lamt, None, batch=B), "mapping")
    g.set_mapping("auto")
    pb.set_batch_params([], None)
    g.compute_states_dev(pb, dx0, ut, xt)
    pb.set_batch_params([0], np.linspace(2.0, 3.0, B)[None, :])
    _refused(ocs, lambda: g.compute_adjoints_dev(pb, ut, None, lamt, None, batch=B), "per-trajectory")
    # entry points that know the batch-minor layout only
    uh = np.asfortranarray(u.transpose(1, 0, 2))
    _refused(ocs, lambda: g.compute_states(p, x0, uh), "tiled layout")
    _refused(ocs, lambda: g.compute_adjoints(p, uh), "tiled layout")
    ctrl = ocs.PWLinearControl(g.t, 5, 1)
    v = np.full((5, B), 0.3)
    _refused(ocs, lambda: ocs.nlp_objective(g, p, ctrl, x0, v), "tiled layout")
    _refused(ocs, lambda: ocs.nlp_objective_dev(g, p, ctrl, dx0.clone(), _dev(v)), "tiled layout")
    _refused(ocs, lambda: ocs.fb_sweep_dev(p, g, dx0), "tiled layout")
    _refused(ocs, lambda: ocs.compute_x_lam(p, x0, ts, uh, integrator=g), "tiled layout")
    md = ocs.MultiDevice([0])
    _refused(ocs, lambda: md.compute_states(([g]), [p], x0, uh), "tiled layout")
    # the handle works in the tiled layout, and gives the batch-minor bits again afterwards
    g.compute_states_dev(p, dx0, ut, xt)
    want = run_default(ocs, nS, N, B, "linspace", x0, u, lamT)
    got = run_default(ocs, nS, N, B, "linspace", x0, u, lamT, g=g)
    assert np.array_equal(got["x"], want["x"]) and np.array_equal(got["J"], want["J"])
    assert np.array_equal(got["both"][0], want["both"][0]) and np.array_equal(got["both"][1], want["both"][1])
    # checkpoints written in one layout are not read in the other
    g.set_layout("tiled")
    with pytest.raises(ocs._lib.OcsError) as e:
        g.compute_adjoints_dev(p, ut, None, torch.empty_like(xt), None, batch=B)
    assert e.value.code != 0 and "layout" in str(e.value)


# ---- 6. handle reuse -------------------------------------------------------------------------------------------------
def test_one_handle_through_both_layouts_and_two_batches(ocs):
    nS, N = 4, 13
    g = ocs.RK4Integrator(_tspan(N, "linspace"))
    for run, B in ((run_default, 70), (run_tiled, 70), (run_default, 70), (run_tiled, 128)):
        x0, u, lamT, d, t = both(ocs, nS, N, B, "linspace")
        fresh = d if run is run_default else t
        got = run(ocs, nS, N, B, "linspace", x0, u, lamT, g=g)
        assert np.array_equal(got["x"], fresh["x"]) and np.array_equal(got["J"], fresh["J"])
        for case in ("both", "lam", "lamT"):
            assert np.array_equal(got[case][0], fresh[case][0])
            if case != "lam":
                assert np.array_equal(got[case][1], fresh[case][1])
