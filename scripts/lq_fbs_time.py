"""fb_sweep on the LQ problem by state count: python scripts/lq_fbs_time.py

From eight states on the state and costate passes run on the matrix-core kernels (`mc 1` in the output; OCS_LQ_SWEEP=0
keeps them on the hipRTC plugin twin's lane kernels); the control update and the bookkeeping are the twin's in both cases.
Environment: N (steps, 400), BATCH (1024), NS (comma-separated state counts, default 4,5,8,16,32), OCS_TREE (root of another
checkout of this repository whose package and library are timed instead: A/B runs; a tree without the flag prints `mc n/a`)."""
import os, sys, time, numpy as np, torch
ROOT = os.environ.get("OCS_TREE") or os.path.join(os.path.dirname(os.path.abspath(__file__)), '..')
sys.path.insert(0, ROOT)
import __graft_entry__ as g
ocs = g.load_package()
dev = torch.device('cuda:0')
N, batch = int(os.environ.get("N", "400")), int(os.environ.get("BATCH", "1024"))
NC = {4: 2, 5: 2, 8: 2, 16: 4, 32: 4}
for nS in (int(v) for v in os.environ.get("NS", "4,5,8,16,32").split(",")):
    nC = NC.get(nS, 2)
    rng = np.random.default_rng(nS)
    A = -np.diag(np.linspace(0.5, 3.0, nS)) + 0.1 * rng.normal(size=(nS, nS))
    Bu = rng.normal(size=(nS, nC)); q, rd = rng.uniform(0.5, 1.5, nS), rng.uniform(1, 2, nC)
    prob = ocs.LQProblem(A, Bu, q, rd, 0.05, [[-1.0, 1.0]] * nC)
    integ = ocs.RK4Integrator(ocs.linspace(0, 2, N + 1))
    x0 = torch.tensor(rng.normal(size=(nS, batch)), device=dev)
    opts = {"nERROR_PTS": N + 1, "nINTERP_PTS": 41, "nSWEEPS": 30, "uRelax": 0.5}
    t0 = time.perf_counter(); r = ocs.fb_sweep_dev(prob, integ, x0, opts); torch.cuda.synchronize(); first = time.perf_counter() - t0
    t0 = time.perf_counter()
    for _ in range(2): r = ocs.fb_sweep_dev(prob, integ, x0, opts)
    torch.cuda.synchronize(); dt = (time.perf_counter() - t0) / 2
    sw = r["sweeps"].cpu().numpy(); ns = max(int(sw.max()), 1) if (sw > 0).any() else 30
    mc = ocs.fb_sweep_matrix_core(integ) if hasattr(ocs, "fb_sweep_matrix_core") else "n/a"
    print(f"LQ nS={nS} nC={nC} batch={batch} N={N}: solve {dt*1e3:.2f} ms, sweeps {sw.min()}..{sw.max()}, ~{dt/ns*1e6:.0f} us per sweep, first call (hipRTC) {first:.1f} s, path {ocs.fb_sweep_path(integ)}, mc {mc}", flush=True)
