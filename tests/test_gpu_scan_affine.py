"""GPU: the adjoint scan of the registry problems (k_backward_scan, ocs_scan_kernel.hpp), whose phase 3 evaluates lam and
the dJdu columns of every step from affine records kept by phase 1, against the lane mapping (the serial recursion) and
the CPU oracle, and its lam-only / dJdu-only / combined variants against each other, with and without an explicit lamT."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

C, R = 1.5, 0.05
BOUNDS = [[0.0, 1.0]]
RTOL = 1e-12


def relerr(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    assert np.all(np.isfinite(a)) and np.all(np.isfinite(b))
    return float(np.max(np.abs(a - b) / np.maximum(1.0, np.abs(b))))


@pytest.fixture(scope="module")
def ocs():
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    import __graft_entry__ as g
    return g.load_package()


def _case(oracle, nS, N, batch, seed, T):
    rng = np.random.default_rng(seed)
    tspan = np.sort(np.concatenate([[0.0, T], rng.uniform(0, T, N - 1)]))
    u = np.asfortranarray(rng.uniform(0.05, 0.45, (1, 2 * N + 1, batch)))
    x0 = rng.uniform(0.8, 2.5, (nS, batch))
    lamT = rng.normal(size=(nS + 1, batch))
    m = [3.0, 2.5, 2.0, 1.5][:nS]
    return tspan, x0, u, lamT, m


@pytest.mark.parametrize("nS,N,batch", [(1, 37, 50), (2, 70, 33), (4, 131, 23), (4, 64, 17), (2, 8, 40), (1, 250, 65)])
def test_scan_matches_lane_and_oracle(ocs, oracle, nS, N, batch):
    # ragged batches (not a multiple of the 64 / nS trajectories of a workgroup), step counts around the superblock
    # (16 chunks of 4 steps) and not a multiple of the chunk, default and explicit lamT
    tspan, x0, u, lamT, m = _case(oracle, nS, N, batch, seed=31 * nS + N, T=0.02 * N)
    pg = ocs.LogisticProblem(m, C, R, BOUNDS)
    po = oracle.LogisticProblem(m, C, R, BOUNDS)
    out = {}
    for mapping in ("scan", "lane"):
        g = ocs.RK4Integrator(tspan).set_mapping(mapping)
        g.compute_states(pg, x0, u)
        out[mapping] = (g.compute_adjoints(pg, u), g.compute_adjoints(pg, u, lamT))
    for k in range(2):
        for j in range(2):   # lam, dJdu
            assert relerr(out["scan"][k][j], out["lane"][k][j]) < RTOL, (k, j)
    ref = oracle.batch_states_adjoints(po, tspan, x0, u)
    assert relerr(out["scan"][0][0], ref["lam"]) < RTOL and relerr(out["scan"][0][1], ref["dJdu"]) < RTOL
    go = oracle.RK4Integrator(tspan)
    for b in sorted({0, batch // 2, batch - 1}):
        go.compute_states(po, x0[:, b], u[:, :, b])
        lo, do = go.compute_adjoints(po, u[:, :, b], lamT[:, b])
        assert relerr(out["scan"][1][0][:, :, b], lo) < RTOL and relerr(out["scan"][1][1][:, :, b], do) < RTOL


@pytest.mark.parametrize("nS,N,batch", [(1, 64, 70), (2, 68, 33), (4, 200, 23)])
def test_scan_variants_bit_identical(ocs, oracle, nS, N, batch):
    # lam only, dJdu only and both: one arithmetic path, the same bits -- with and without an explicit lamT
    import torch
    tspan, x0, u, lamT, m = _case(oracle, nS, N, batch, seed=57 * nS + N, T=0.03 * N)
    pg = ocs.LogisticProblem(m, C, R, BOUNDS)
    g = ocs.RK4Integrator(tspan).set_mapping("scan")
    dev = torch.device("cuda:0")
    x0d = torch.tensor(np.ascontiguousarray(x0), device=dev)
    ud = torch.tensor(np.ascontiguousarray(np.transpose(u, (1, 0, 2))), device=dev)
    xd = torch.empty((N + 1, nS + 1, batch), dtype=torch.float64, device=dev)
    g.compute_states_dev(pg, x0d, ud, xd)
    for lt in (None, torch.tensor(lamT, device=dev)):
        lam, dd = torch.empty_like(xd), torch.empty_like(ud)
        g.compute_adjoints_dev(pg, ud, lt, lam, dd)
        lam_only, d_only = torch.empty_like(xd), torch.empty_like(ud)
        g.compute_adjoints_dev(pg, ud, lt, lam_only, None)
        g.compute_adjoints_dev(pg, ud, lt, None, d_only)
        torch.cuda.synchronize()
        assert torch.equal(lam, lam_only) and torch.equal(dd, d_only)
        assert bool(torch.isfinite(lam).all()) and bool(torch.isfinite(dd).all())
