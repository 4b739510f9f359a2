#!/usr/bin/env python3
"""bench.py -- headline benchmark of the RK4 state + discrete-adjoint hot path on MI355X.

Workload (BASELINE.json configs[1]): LogisticK with nS = 4 (nAug = 5,
nC = 1), N = 1000 RK4 steps on linspace(0, 10, 1001), batch = 4096 control candidates per
GPU, fp64, full-output mode (x, J, lam, dJdu all written).  One "step" of this script is one
pass of the hot path over the batch: compute_states followed by compute_adjoints, i.e.
batch * N fused RK4 state+costate steps.  Inputs are synthetic and already resident in HBM.

  python bench.py --gpus 1 --steps 20 --warmup 3
  python bench.py --gpus 1 --steps 20 --warmup 3 --full
  python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 \
         --master-port P bench.py --gpus N --steps K --warmup W

A plain run sets up, pre-warms, runs the W warm-up steps, times the K steps and prints the headline line; with
--dump-outputs DIR it also writes the outputs of the last timed step as DIR/<name>.npy (see dump_outputs).  --full adds
everything else this script measures: the PMC traffic collected in child processes, the per-kernel HIP-event timings and
roofline of the headline kernels, the secondary legs and the CPU baseline with its parity check.

Multi-GPU: the batch axis shards with no data-path exchange; the only collective is the all-reduce(SUM) of the
objective sum over ranks (north_star), 8 bytes per step, issued asynchronously so that it overlaps the next step's
kernels.  --scaling weak (default): 4096 trajectories per GPU; --scaling strong: --batch is the TOTAL, split into
contiguous blocks.  The secondary legs shard as BASELINE.json names them: configs[3] (65 536 Chebyshev candidates,
8192 per GPU at N = 8, J all-gathered, best candidate selected) and configs[4] (8192 LQ32 trajectories, 1024 per GPU
at N = 8); fb_sweep (configs[2]) shards its 16 384 instances the same way.  Every rank runs every leg.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

NS, NC, NSTEPS, BATCH = 4, 1, 1000, 4096
M, C_PAR, R_PAR = [3.0, 2.5, 2.0, 1.5], 1.5, 0.05
T_END = 10.0
HBM_PEAK_GBPS = 8000.0  # MI355X_MICROARCH.md: HBM3E 8.0 TB/s spec


def make_inputs(batch, device, seed):
    """SURVEY BL-2 candidates u_b(t) = clamp(a + A sin(2 pi f_b t + phi_b), 0, 1), seeded; amplitude
    (a, A) = (0.25, 0.2) instead of the survey's (0.5, 0.4), which drives the m = 1.5 state to -inf."""
    rng = np.random.default_rng(seed)
    tspan = np.linspace(0.0, T_END, NSTEPS + 1)
    t = np.zeros(2 * NSTEPS + 1)
    t[0::2] = tspan
    t[1::2] = (tspan[:-1] + tspan[1:]) / 2
    f, ph = rng.uniform(0, 1, batch), rng.uniform(0, 2 * np.pi, batch)
    u = np.clip(0.25 + 0.2 * np.sin(2 * np.pi * f[None, :] * t[:, None] + ph[None, :]), 0.0, 1.0)
    u = np.ascontiguousarray(u[:, None, :])                      # [2N+1][nC][B] batch-minor
    x0 = np.ones((NS, batch))
    return tspan, x0, u


def cpu_baseline(tspan, x0, u, target_seconds=8.0):
    """Times the CPU oracle (the C restatement of RK4Integrator.m) on the same workload, kind 'port': (a) OpenMP over
    the batch on all host cores, whole-batch passes for ~target_seconds; (b) one thread, on the first 256
    trajectories of the same batch for ~4 s (SURVEY 8(d) asks for both)."""
    from oracle import oracle as orc
    orc.build()
    try:
        cores = len(os.sched_getaffinity(0))
    except AttributeError:
        cores = os.cpu_count() or 1
    try:  # cgroup quota of the GPU box (16 CPUs for one GPU)
        q, p = open("/sys/fs/cgroup/cpu.max").read().split()
        if q != "max":
            cores = max(1, min(cores, int(int(q) / int(p))))
    except Exception:
        pass
    cores = min(cores, orc.max_threads())
    prob = orc.LogisticProblem(M, C_PAR, R_PAR, [[0.0, 1.0]])
    u_m = np.asfortranarray(u.transpose(1, 0, 2))               # nC x (2N+1) x B, MATLAB shape
    out = orc.batch_states_adjoints(prob, tspan, x0, u_m, nthreads=cores)  # warm-up, touches outputs
    t0 = time.perf_counter()
    passes = 0
    while True:
        orc.batch_states_adjoints(prob, tspan, x0, u_m, nthreads=cores, out=out)
        passes += 1
        dt = time.perf_counter() - t0
        if dt >= target_seconds or passes >= 200:
            break
    batch = x0.shape[1]
    # one thread
    b1 = min(256, batch)
    x1, u1 = np.ascontiguousarray(x0[:, :b1]), np.asfortranarray(u_m[:, :, :b1])
    o1 = orc.batch_states_adjoints(prob, tspan, x1, u1, nthreads=1)
    t1 = time.perf_counter()
    p1 = 0
    while True:
        orc.batch_states_adjoints(prob, tspan, x1, u1, nthreads=1, out=o1)
        p1 += 1
        d1 = time.perf_counter() - t1
        if d1 >= 4.0 or p1 >= 200:
            break
    literal = {"value": batch * NSTEPS * passes / dt, "unit": "RK4 state+costate steps/s", "cores": cores,
               "sample": f"{passes} full passes of the bench workload (batch {batch} x {NSTEPS} steps, "
                         f"x/J/lam/dJdu written) in {dt:.1f} s, oracle/ocs_oracle.c (the line-by-line restatement of "
                         "RK4Integrator.m: one trajectory per call, xK cached, a call per stage) with OpenMP over the batch",
               "one_thread": {"value": b1 * NSTEPS * p1 / d1, "unit": "RK4 state+costate steps/s", "cores": 1,
                              "sample": f"{p1} passes over the first {b1} trajectories of the same batch in {d1:.1f} s"}}
    # the same arithmetic written for the host's vector units (oracle/ocs_cpu_fast.c: batch-minor arrays, unit-stride loops
    # over blocks of 64 trajectories, stage states recomputed, FMA on): what the GPU figure is fairly compared with
    ub = np.ascontiguousarray(u[:, 0, :])
    of = orc.fast_logistic_pair(M, C_PAR, R_PAR, tspan, x0, ub, nthreads=cores)
    errf = float(np.max(np.abs(of["J"] - out["J"]) / np.maximum(1.0, np.abs(out["J"]))))
    tf0, pf = time.perf_counter(), 0
    while True:
        orc.fast_logistic_pair(M, C_PAR, R_PAR, tspan, x0, ub, nthreads=cores, out=of)
        pf += 1
        df = time.perf_counter() - tf0
        if df >= 6.0 or pf >= 400:
            break
    o1 = orc.fast_logistic_pair(M, C_PAR, R_PAR, tspan, x1, np.ascontiguousarray(ub[:, :b1]), nthreads=1)
    t1f, p1f = time.perf_counter(), 0
    while True:
        orc.fast_logistic_pair(M, C_PAR, R_PAR, tspan, x1, np.ascontiguousarray(ub[:, :b1]), nthreads=1, out=o1)
        p1f += 1
        d1f = time.perf_counter() - t1f
        if d1f >= 2.0 or p1f >= 400:
            break
    return {"value": batch * NSTEPS * pf / df, "unit": "RK4 state+costate steps/s", "cores": cores, "kind": "port",
            "sample": f"{pf} full passes of the bench workload (batch {batch} x {NSTEPS} steps, x/J/lam/dJdu written) in {df:.1f} s, "
                      "oracle/ocs_cpu_fast.c: the restatement's arithmetic tuned for the host (vector loops over blocks of 64 "
                      "trajectories, batch-minor arrays as the GPU gets them, stage states recomputed, FMA), OpenMP over the blocks; "
                      f"J agrees with the literal restatement to {errf:.1e}",
            "one_thread": {"value": b1 * NSTEPS * p1f / d1f, "unit": "RK4 state+costate steps/s", "cores": 1,
                           "sample": f"{p1f} passes over the first {b1} trajectories in {d1f:.1f} s"},
            "literal_restatement": literal}, out


def live_traffic(timeout_s=150):
    """HBM bytes per launch of the headline kernels from the PMC counters, COLLECTED BY THIS RUN: two child processes
    (rocprofv3 --pmc FETCH_SIZE / --pmc WRITE_SIZE in separate passes, as MI355X_MICROARCH.md prescribes; kernel trace only)
    over scripts/traffic_once.py -- the same kernels on the same shapes -- started before this process touches the GPU.
    Counters are KiB; both are corrected by the factor the same passes measure on a copy of known size with this path's
    access width (8 B per lane: FETCH_SIZE x 2.0 on gfx950, WRITE_SIZE x 1.0).  Returns None if rocprofv3 is missing or a
    pass fails (the line then carries the replayed figure of profiles/, labelled as such)."""
    import csv
    import glob
    import shutil
    import subprocess
    import tempfile
    if shutil.which("rocprofv3") is None:
        return None
    # under a profiler the preloaded tool library has already initialised the GPU in THIS process: it must not start
    # children that exec (and a profile of bench.py is about the timed loops anyway)
    if "rocprof" in os.environ.get("LD_PRELOAD", "").lower() or any(k.startswith(("ROCPROF", "ROCP_")) for k in os.environ):
        return None
    work = tempfile.mkdtemp(prefix="ocs_traffic_", dir="/tmp")
    env = dict(os.environ, TMPDIR="/tmp")
    per = {}
    try:
        for counter in ("FETCH_SIZE", "WRITE_SIZE"):
            out = os.path.join(work, counter)
            r = subprocess.run(["rocprofv3", "--pmc", counter, "--kernel-trace", "--output-format", "csv", "-d", out, "--",
                                sys.executable, os.path.join(ROOT, "scripts", "traffic_once.py")],
                               cwd="/tmp", env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=timeout_s)
            files = glob.glob(os.path.join(out, "**", "*counter_collection.csv"), recursive=True)
            if r.returncode != 0 or not files:
                return None
            cal_bytes = None
            for ln in r.stdout.decode(errors="replace").splitlines():
                if ln.startswith("calibration bytes per launch"):
                    cal_bytes = float(ln.split(":")[1])
            rows = {}
            with open(max(files, key=os.path.getmtime)) as fh:
                for row in csv.DictReader(fh):
                    if row["Counter_Name"] != counter:
                        continue
                    nm = row["Kernel_Name"]
                    key = ("copy" if "k_copy8" in nm else "fwd" if "k_forward_p2" in nm else "bwd" if "k_backward_scan" in nm else
                           "fcc" if "k_forward_cc" in nm else "cst" if "k_costate" in nm else None)
                    if key:
                        rows.setdefault(key, []).append((int(row["Dispatch_Id"]), float(row["Counter_Value"]) * 1024.0))
            if cal_bytes is None or "copy" not in rows or len(rows.get("bwd", [])) < 17 or len(rows.get("fwd", [])) < 17:
                return None
            for k in rows:
                rows[k] = [v for _, v in sorted(rows[k])]
            fac = cal_bytes / (sum(rows["copy"]) / len(rows["copy"]))
            mean = lambda v: sum(v) / len(v)
            per[counter] = {"factor": fac,
                            "fwd_one_set": mean(rows["fwd"][4:8]) * fac, "bwd_one_set": mean(rows["bwd"][4:8]) * fac,
                            "fwd_rotating": mean(rows["fwd"][11:17]) * fac, "bwd_rotating": mean(rows["bwd"][11:17]) * fac}
            for k in ("fcc", "cst"):   # live launches of the sweep only (a gated-off launch moves nothing)
                if k in rows and max(rows[k]) > 0:
                    live = [v for v in rows[k] if v > 0.05 * max(rows[k])]
                    per[counter][k] = mean(live) * fac
        f, w = per["FETCH_SIZE"], per["WRITE_SIZE"]
        res = {"source": "collected by this run: rocprofv3 --pmc FETCH_SIZE and --pmc WRITE_SIZE (separate passes, kernel trace "
                         "only) over scripts/traffic_once.py before the timed loops; bytes = counter x 1024 x the factor the same "
                         "pass measures on ocs_copy_dev (8 B per lane, known byte count)",
               "fetch_factor": f["factor"], "write_factor": w["factor"]}
        for k in ("fwd_one_set", "bwd_one_set", "fwd_rotating", "bwd_rotating", "fcc", "cst"):
            if k in f and k in w:
                res[k] = {"fetch": f[k], "write": w[k], "hbm_bytes_per_launch": f[k] + w[k]}
        return res
    except Exception:
        return None
    finally:
        shutil.rmtree(work, ignore_errors=True)


def _shard(ocs, total):
    world, rank = ocs.distributed.world_info()
    lo, hi = ocs.distributed.shard_bounds(total, world, rank)
    return world, rank, lo, hi


def _sync():
    torch.cuda.synchronize()


def fb_sweep_metric(ocs, dev, batch=16384, reps=20, shard=True, prewarm_s=0.3):
    """Second half of BASELINE.json's metric: fb_sweep iters/sec on configs[2] (SURVEY BL-3):
    TestOCProblem through the A9 adapter, T=10, N=1000 forward + 1000 backward, batch=16384 instances with
    x0 ~ U(0.5,2.5), c ~ U(1,2) (seed 20260402), u0 = lower bound, default tolerances, <= 50 sweeps.
    One iter = forward + costate + control update + convergence reduction for one instance; converged
    instances stop counting (the whole batch still runs until the last one is done).  Under world > 1 the instances
    shard into contiguous blocks (no exchange; the count of iterations is all-reduced).
    Timing: >= prewarm_s seconds of untimed solves (the leg's own work, like the headline's pre-warm), then `reps`
    solves timed one by one (sync on both sides of each); `value` follows the MEDIAN, and min / max / the per-rep
    list are in the line.  The output tensors are allocated once and written by every solve (`out=`)."""
    world, rank, lo, hi = _shard(ocs, batch) if shard else (1, 0, 0, batch)
    rng = np.random.default_rng(20260402)
    tspan = ocs.linspace(0.0, T_END, NSTEPS + 1)  # MATLAB's linspace, as fb_sweep.m:69-70 builds its point sets
    x0 = torch.tensor(np.ascontiguousarray(rng.uniform(0.5, 2.5, (1, batch))[:, lo:hi]), device=dev)
    cs = rng.uniform(1.0, 2.0, batch)[lo:hi]
    prob = ocs.TestOCProblem({"c": 1.5, "m": 3.0, "r": 0.05}, [[0.0, 1.0]])
    prob.set_batch_params([0], cs[None, :])
    integ = ocs.RK4Integrator(tspan)
    res = {"r": ocs.fb_sweep_dev(prob, integ, x0)}   # first call: allocations, tables

    def solve():
        res["r"] = ocs.fb_sweep_dev(prob, integ, x0, out=res["r"])
    n_warm = ocs.distributed.prewarm(solve, prewarm_s, _sync)
    per_rep = ocs.distributed.timed_reps_max_over_ranks(solve, reps, _sync)
    sp, dt = ocs.distributed.spread(per_rep)
    sw = res["r"]["sweeps"].cpu().numpy()
    tot = torch.tensor([float(np.where(sw > 0, sw, 50).sum()), float((sw > 0).sum()), float(sw.max())],
                       dtype=torch.float64, device=dev)
    if shard and ocs.distributed.collectives_on():
        import torch.distributed as dist
        mx = tot[2:].clone()
        dist.all_reduce(tot[:2])
        dist.all_reduce(mx, op=dist.ReduceOp.MAX)
        tot[2] = mx[0]
    iters, nconv, smax = float(tot[0]), float(tot[1]), float(tot[2])
    # Algorithmic bytes per (instance, step) of one sweep.
    #  * the reference's data flow (compute_x_lam -> ControlChar on the grid): x write + read, lam write + read, u (two
    #    samples per step) write + read = 8 (4 nS + 4 nC) - 8 = 72 B at nS = nC = 1 as SURVEY 8(d) counts it (round 1's figure);
    #  * what the folded kernels of this build move: state pass reads lam (8 nS) and writes x (8 nS); costate pass reads
    #    x (8 nS) and the costate it replaces (8 nS) and writes lam (8 nS) = 40 nS: the control samples never reach memory.
    n_local = hi - lo
    bytes_sweep_ref = 72.0 * n_local * NSTEPS
    bytes_sweep_fold = 40.0 * n_local * NSTEPS
    bsps = float(sw.max()) / dt
    # HBM bytes of a sweep (both kernels) from the PMC passes of scripts/profile_fbs_traffic.sh: replayed, not collected here
    fb_traffic, fb_traffic_source = None, None
    try:
        tr = json.load(open(os.path.join(ROOT, "profiles", "fb_traffic_latest.json")))
        if n_local == 16384 and NSTEPS == 1000:
            fb_traffic = tr["hbm_bytes_per_batch_sweep"]
            fb_traffic_source = (f"profiles/{tr['tag']}_fb_sweep_traffic.json (rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE passes, "
                                 "k_forward_cc + the costate kernel per live launch; replayed from that file, not collected by this run)")
    except Exception:
        fb_traffic = None
    return {"value": iters / dt, "unit": "fb_sweep iters/s (instance-sweeps)", "batch": batch, "n_steps": NSTEPS,
            "batch_per_gpu": hi - lo, "seconds_per_solve": dt, "ms_per_solve": sp,
            "timing": f"median of {reps} solves timed one by one after {n_warm} untimed solves (>= {prewarm_s} s); "
                      "outputs allocated once",
            "sweeps_min": int(sw[sw > 0].min()) if (sw > 0).any() else 0,
            "sweeps_max": int(smax), "fraction_converged": nconv / batch,
            "batch_sweeps_per_s": bsps,
            "sweep_loop": ocs.fb_sweep_path(integ),
            "roofline": {"bound": "hbm", "kernel": "one sweep of the local batch: state pass with the control update "
                                                   "folded in (k_forward_cc) + costate pass with the convergence test "
                                                   "(k_costate_plx, MET)",
                         "achieved": bytes_sweep_fold * bsps / 1e9, "peak": HBM_PEAK_GBPS, "unit": "GB/s",
                         "frac": bytes_sweep_fold * bsps / 1e9 / HBM_PEAK_GBPS, "traffic": fb_traffic,
                         "traffic_source": fb_traffic_source,
                         "algorithmic_bytes_per_batch_sweep": bytes_sweep_fold,
                         "bytes_per_instance_step": 40.0,
                         "note": "the two kernels of a sweep are marching kernels (one recursion wave per 64 instances, "
                                 "bound by its dependent fp64 chain and by the LDS pipe), not HBM-bound; with round 1's "
                                 "72 B per instance-step (control samples through memory) the same rate reads "
                                 "frac_round1_definition",
                         "frac_round1_definition": bytes_sweep_ref * bsps / 1e9 / HBM_PEAK_GBPS}}


FP64_PEAK_TFLOPS = 78.6   # MI355X fp64 peak, vector = matrix (public spec); the two share one datapath per SIMD
                          # (scripts/probe/mfma_valu_overlap.hip), so this is the fp64 roofline whatever the mix


def bl4_metric(ocs, dev, batch=65536, reps=12, shard=True):
    """BASELINE configs[3] (SURVEY BL-4): single_shooting objective + gradient (single_shooting.m:137-150) with a
    Chebyshev basis of 16 coefficients, TestOCProblem, N = 1000, batch = 65536 coefficient vectors (seed 20260403),
    sharded into contiguous blocks (8192 per GPU at 8 GPUs) through distributed.sharded_objective_eval: one evaluation
    = u = v*B, forward, adjoint, dJdv = dJdu*B' for the local block, then the all-gather of J, the best candidate and
    the ensemble mean (the only collectives; KBs).  shard=False: the whole `batch` on this rank (the per-GPU shard of a
    larger job, measured on one GPU).

    Rooflines.  HBM: objective+gradient-only mode moves the checkpoint of every step once out and once in; SURVEY 8(d)
    counts 8*2*nAug = 32 B per (trajectory, step) (this build checkpoints the state rows only: 16 B).  fp64: u and dJdu
    never reach memory, so the pass is arithmetic: per (trajectory, step) the three products with the basis matrix
    (expansion in both passes, contraction) are 3 * 2 samples * 2 nBasis = 192 flop; the RK4 state pass of TestOCProblem
    52 flop (four F of 8 flop, RK4Integrator.m:39-48; the three stage states and the update of :50-51: 20); the discrete
    adjoint with compute_dJdu 76 flop (four dFdx_times_vec of 7, :74-88; k1..k4 and the lam update: 26; four
    dFdu_times_vec of 5 and the two column sums, :97-121: 22) -- the stage recomputation of this build is not counted:
    320 flop."""
    world, rank, lo, hi = _shard(ocs, batch) if shard else (1, 0, 0, batch)
    rng = np.random.default_rng(20260403)
    V = 0.05 * rng.normal(size=(16, batch)) / np.arange(1, 17)[:, None]
    V[0] += 0.5
    integ = ocs.RK4Integrator(np.linspace(0.0, T_END, NSTEPS + 1))
    prob = ocs.TestOCProblem({"c": 1.5, "m": 3.0, "r": 0.05}, [[0.0, 1.0]])
    ctrl = ocs.ChebyshevControl(integ.t, 16, 1)
    Vg = torch.tensor(V, device=dev)
    nloc = hi - lo
    x0 = torch.ones((1, nloc), dtype=torch.float64, device=dev)
    J = torch.empty(nloc, dtype=torch.float64, device=dev)
    G = torch.empty((16, nloc), dtype=torch.float64, device=dev)

    def eval_local(Vl):
        ocs.nlp_objective_dev(integ, prob, ctrl, x0, Vl, (), J, G)
        return J, G
    out = {}
    Vl = Vg[:, lo:hi].contiguous()

    def one():
        out["r"] = ocs.distributed.sharded_objective_eval(eval_local, Vg) if shard else None
    eval_local(Vl)
    one()
    # `value`: the evaluations themselves (the data path), max over ranks; >= 0.3 s of untimed evaluations first, then
    # `reps` groups of 5 evaluations timed one group at a time (median); the KB-size post-reductions (J all-gather, best
    # candidate, ensemble mean; each ends in a host read) are timed with them once more and reported beside it
    ocs.distributed.prewarm(lambda: eval_local(Vl), 0.3, _sync, chunk=10)
    sp, dt = ocs.distributed.spread(ocs.distributed.timed_reps_max_over_ranks(lambda: eval_local(Vl), reps, _sync, inner=5))
    res = {"value": batch * NSTEPS / dt, "unit": "RK4 state+costate steps/s inside objective+gradient evaluations",
           "batch": batch, "batch_per_gpu": nloc, "n_basis": 16, "ms_per_batch_evaluation": dt * 1e3,
           "ms_per_batch_evaluation_spread": sp,
           "evaluations_per_s": batch / dt, "finite": bool(torch.isfinite(G).all().item())}
    if shard:
        dt_red = ocs.distributed.timed_max_over_ranks(one, 5, _sync)
        r = out["r"]
        res.update({"ms_per_evaluation_with_post_reductions": dt_red * 1e3,
                    "best_candidate": {"J": r["best"][0], "index": r["best"][1]}, "J_all_gathered": int(r["J_all"].numel())})
    wave = nloc <= 32768 and nloc % 64 == 0
    bytes_eval = 32.0 * nloc * NSTEPS
    flops_eval = 320.0 * nloc * NSTEPS
    tr = _replayed_traffic("bl4_traffic_latest.json", nloc)
    res["roofline"] = {"bound": "mfma", "note": "fp64 arithmetic (vector + matrix instructions on one datapath): 320 flop per "
                                                 "(trajectory, step), see the docstring",
                       "kernel": ("k_forward_p2<NKS=4> + k_backward_fcs (wave-specialised state pass, adjoint scan, basis products "
                                  "on v_mfma_f64_16x16x4_f64)" if wave else
                                  "k_forward_fc + k_backward_fc (lane per trajectory, basis products as v_fmac_f64_dpp)") + ", local block",
                       "achieved": flops_eval / dt / 1e12, "peak": FP64_PEAK_TFLOPS, "unit": "TFLOP/s",
                       "frac": flops_eval / dt / 1e12 / FP64_PEAK_TFLOPS, "traffic": tr[0], "traffic_source": tr[1],
                       "algorithmic_flops_per_evaluation": flops_eval}
    res["roofline_hbm"] = {"bound": "hbm", "achieved": bytes_eval / dt / 1e9, "peak": HBM_PEAK_GBPS, "unit": "GB/s",
                           "frac": bytes_eval / dt / 1e9 / HBM_PEAK_GBPS, "algorithmic_bytes_per_evaluation": bytes_eval}
    return res


def _replayed_traffic(name, nloc):
    """HBM bytes per evaluation (both kernels) from the committed rocprofv3 PMC summary under profiles/ (scripts/profile_r03.sh
    + summarize_r03.py; replayed, not collected by this run), if one was taken at this local batch."""
    try:
        tr = json.load(open(os.path.join(ROOT, "profiles", name)))["entries"].get(str(nloc))
        if tr:
            return tr["hbm_bytes_per_evaluation"], f"{tr['source']} (rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE passes; replayed)"
    except Exception:
        pass
    return None, None


def _replayed_variant_traffic(key):
    """HBM bytes per pass pair of a secondary BL-2 entry from profiles/bl2_variants_traffic_latest.json
    (scripts/profile_variants.sh + summarize_variants.py; replayed, not collected by this run)."""
    try:
        tr = json.load(open(os.path.join(ROOT, "profiles", "bl2_variants_traffic_latest.json")))["entries"].get(key)
        if tr:
            return tr["hbm_bytes_per_pass_pair"], f"{tr['source']} (rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE passes; replayed)"
    except Exception:
        pass
    return None, None


def _pair_buffers(ocs, dev, nS, batch, seed, nsets=1):
    tspan, x0_h, u_h = make_inputs(batch, dev, seed)
    x0 = torch.tensor(np.ascontiguousarray(x0_h[:nS]), device=dev)
    sets = []
    for k in range(nsets):
        u = torch.tensor(u_h, device=dev) if k == 0 else sets[0][0].clone()
        x = torch.empty((NSTEPS + 1, nS + 1, batch), dtype=torch.float64, device=dev)
        sets.append((u, x, torch.empty_like(x), torch.empty_like(u)))
    J = torch.empty(batch, dtype=torch.float64, device=dev)
    return tspan, x0, sets, J


def pair_time(ocs, dev, nS, batch, reps=12, seed=20260410, spread=False):
    """ms per pass pair (compute_states + compute_adjoints, full output, automatic mapping) of the BL-2 problem family:
    >= 0.2 s of untimed pairs, then `reps` groups of 10 pairs (5 above batch 8192) timed group by group; the median."""
    tspan, x0, sets, J = _pair_buffers(ocs, dev, nS, batch, seed)
    u, x, lam, dJdu = sets[0]
    prob = ocs.LogisticProblem(M[:nS], C_PAR, R_PAR, [[0.0, 1.0]])
    integ = ocs.RK4Integrator(tspan)

    def pair():
        integ.compute_states_dev(prob, x0, u, x, J)
        integ.compute_adjoints_dev(prob, u, None, lam, dJdu)
    ocs.distributed.prewarm(pair, 0.2, _sync, chunk=10)
    sp, med = ocs.distributed.spread(ocs.distributed.timed_reps_max_over_ranks(pair, reps, _sync, inner=10 if batch <= 8192 else 5))
    return (med * 1e3, sp) if spread else med * 1e3


def bl2_rotated_metric(ocs, dev, batch=BATCH, nsets=3, reps=20):
    """The BL-2 pass pair with NO reuse of a buffer from one step to the next: `nsets` complete buffer sets (u, x, lam,
    dJdu: 458 MB each at batch 4096, so three of them are 5.4 x the 256 MiB Infinity Cache) are used round-robin, one set
    per step; a set is touched again only after all the others.  The headline loop re-uses ONE set, whose u (65 MB) and x
    (164 MB) can stay in the memory-side cache between steps -- this entry is the figure with every byte coming from and
    going to HBM.  Same kernels, same roofline arithmetic; per-kernel times from HIP events on the launch stream in
    a separate untimed loop."""
    nS = NS
    tspan, x0, sets, J = _pair_buffers(ocs, dev, nS, batch, 20260401, nsets)
    prob = ocs.LogisticProblem(M, C_PAR, R_PAR, [[0.0, 1.0]])
    integ = ocs.RK4Integrator(tspan)
    state = {"k": 0}

    def step():
        u, x, lam, dJdu = sets[state["k"] % nsets]
        state["k"] += 1
        integ.compute_states_dev(prob, x0, u, x, J)
        integ.compute_adjoints_dev(prob, u, None, lam, dJdu)
    # (the steady state of this memory-bound loop takes ~30 ms to settle after any gap -- the first repetitions after the
    #  pre-warm of an earlier version ran 0.158 .. 0.150 ms on their way to 0.145: the pre-warm is long, the repetitions follow
    #  it directly, and the event-bracketed steps for the per-kernel times come last)
    ocs.distributed.prewarm(step, 0.6, _sync, chunk=nsets * 20)
    sp, dt = ocs.distributed.spread(ocs.distributed.timed_reps_max_over_ranks(step, reps, _sync, inner=nsets * 10))
    nev = 30
    ev = [[torch.cuda.Event(enable_timing=True) for _ in range(3)] for _ in range(nev)]
    for k in range(nev):
        u, x, lam, dJdu = sets[k % nsets]
        ev[k][0].record()
        integ.compute_states_dev(prob, x0, u, x, J)
        ev[k][1].record()
        integ.compute_adjoints_dev(prob, u, None, lam, dJdu)
        ev[k][2].record()
    torch.cuda.synchronize()
    t_f = float(np.median([e[0].elapsed_time(e[1]) for e in ev])) * 1e-3
    t_b = float(np.median([e[1].elapsed_time(e[2]) for e in ev])) * 1e-3
    nA = nS + 1
    b_f, b_b = 8 * (nA + 2 * NC) * batch * NSTEPS, 8 * (2 * nA + 4 * NC) * batch * NSTEPS
    return {"value": batch * NSTEPS / dt, "unit": "RK4 state+costate steps/s", "batch": batch, "buffer_sets": nsets,
            "bytes_per_buffer_set": int(sum(t.numel() * 8 for t in sets[0])), "ms_per_pass_pair": dt * 1e3,
            "ms_per_pass_pair_spread": sp,
            "roofline": {"bound": "hbm", "kernel": "k_forward_p2 + k_backward_scan, pass pair, rotating buffer sets",
                         "achieved": (b_f + b_b) / dt / 1e9, "peak": HBM_PEAK_GBPS, "unit": "GB/s",
                         "frac": (b_f + b_b) / dt / 1e9 / HBM_PEAK_GBPS, "traffic": None,
                         "algorithmic_bytes_per_pass_pair": b_f + b_b},
            "kernels": {"k_forward": {"median_s": t_f, "GBps": b_f / t_f / 1e9},
                        "k_backward": {"median_s": t_b, "GBps": b_b / t_b / 1e9, "frac": b_b / t_b / 1e9 / HBM_PEAK_GBPS}},
            "finite": bool(torch.isfinite(J).all().item())}


def strong_scaling_readiness(ocs, dev):
    """The path has no exchange step, so the time of an N-GPU job is the one-GPU time at the shard size (plus a
    latency-bound 8-byte all-reduce that overlaps the next step).  Measured here on ONE GPU: every BASELINE config at its
    total size B and at its 8-GPU shard B / 8, the predicted strong-scaling efficiency at 8 GPUs  t(B) / (8 t(B / 8)),
    and the BL-2 pass pair over batch 512 ... 65 536 (across the switches of the automatic mapping)."""
    out = {"definition": "predicted_efficiency_8gpu = t(B) / (8 * t(B/8)), both measured on one GPU; the data path has no collective"}
    sweep = {}
    for b in (512, 1024, 2048, 4096, 8192, 16384, 32768, 65536):
        sweep[str(b)] = pair_time(ocs, dev, NS, b, reps=12 if b <= 8192 else 6)
    out["BL-2 pass pair ms by batch (LogisticK nS=4, N=1000, automatic mapping)"] = sweep
    out["BL-2"] = {"B": 4096, "ms_B": sweep["4096"], "ms_shard": sweep["512"],
                   "predicted_efficiency_8gpu": sweep["4096"] / (8 * sweep["512"])}
    f_full, f_shard = fb_sweep_metric(ocs, dev, 16384, shard=False), fb_sweep_metric(ocs, dev, 2048, shard=False)
    out["BL-3 fb_sweep"] = {"B": 16384, "ms_solve_B": f_full["seconds_per_solve"] * 1e3,
                            "ms_solve_shard": f_shard["seconds_per_solve"] * 1e3,
                            "batch_sweeps_per_s_shard": f_shard["batch_sweeps_per_s"],
                            "predicted_efficiency_8gpu": f_full["seconds_per_solve"] / (8 * f_shard["seconds_per_solve"])}
    b4f, b4s = bl4_metric(ocs, dev, 65536, shard=False), bl4_metric(ocs, dev, 8192, shard=False)
    out["BL-4"] = {"B": 65536, "ms_B": b4f["ms_per_batch_evaluation"], "ms_shard": b4s["ms_per_batch_evaluation"],
                   "predicted_efficiency_8gpu": b4f["ms_per_batch_evaluation"] / (8 * b4s["ms_per_batch_evaluation"]),
                   "shard": b4s}
    b5f, b5s = bl5_metric(ocs, dev, 8192, shard=False), bl5_metric(ocs, dev, 1024, shard=False)
    out["BL-5"] = {"B": 8192, "ms_B": b5f["ms_pass_pair_max_over_ranks"], "ms_shard": b5s["ms_pass_pair_max_over_ranks"],
                   "predicted_efficiency_8gpu": b5f["ms_pass_pair_max_over_ranks"] / (8 * b5s["ms_pass_pair_max_over_ranks"]),
                   "shard_roofline": b5s["roofline"]}
    return out


def bl2_large_batch_metric(ocs, dev, batch=65536, reps=8):
    """The BL-2 problem in the HBM-bound regime (the lane-per-trajectory mapping at batch 65 536, full output; its adjoint kernel
    reads one checkpoint in four and re-integrates the others): the figure DESIGN.md quotes for "what the passes reach once the
    chip is full".  `achieved` counts the algorithmic 168 B per trajectory-step, `traffic` what the counters saw."""
    tspan, x0_h, u_h = make_inputs(batch, dev, 20260409)
    prob = ocs.LogisticProblem(M, C_PAR, R_PAR, [[0.0, 1.0]])
    integ = ocs.RK4Integrator(tspan).set_mapping("lane")
    x0, u = torch.tensor(x0_h, device=dev), torch.tensor(u_h, device=dev)
    x = torch.empty((NSTEPS + 1, NS + 1, batch), dtype=torch.float64, device=dev)
    lam, dJdu = torch.empty_like(x), torch.empty_like(u)
    J = torch.empty(batch, dtype=torch.float64, device=dev)

    def pair():
        integ.compute_states_dev(prob, x0, u, x, J)
        integ.compute_adjoints_dev(prob, u, None, lam, dJdu)
    ocs.distributed.prewarm(pair, 0.2, _sync, chunk=5)
    sp, dt = ocs.distributed.spread(ocs.distributed.timed_reps_max_over_ranks(pair, reps, _sync, inner=3))
    nbytes = 8.0 * (3 * (NS + 1) + 6 * NC) * batch * NSTEPS
    tr = _replayed_variant_traffic(f"lane_{NS}_{batch}")
    return {"value": batch * NSTEPS / dt, "unit": "RK4 state+costate steps/s", "batch": batch, "mapping": "lane",
            "ms_per_pass_pair": dt * 1e3, "ms_per_pass_pair_spread": sp,
            "roofline": {"bound": "hbm", "kernel": "k_forward + k_backward<XRC> (lane per trajectory; the adjoint re-integrates 3 of 4 checkpoints), pass pair",
                         "achieved": nbytes / dt / 1e9, "peak": HBM_PEAK_GBPS, "unit": "GB/s",
                         "frac": nbytes / dt / 1e9 / HBM_PEAK_GBPS, "traffic": tr[0], "traffic_source": tr[1]}}


def bl2_single_state_metric(ocs, dev, batch=4096, reps=12):
    """"reduces to TestOCProblem when nS = 1 -- also benchmark that nAug = 2 case": the same grid,
    batch and candidates with one state (96 B per trajectory-step), automatic mapping (k_forward_p2 + k_backward_scan)."""
    tspan, _, u_h = make_inputs(batch, dev, 20260401)
    prob = ocs.TestOCProblem({"c": C_PAR, "m": 3.0, "r": R_PAR}, [[0.0, 1.0]])
    integ = ocs.RK4Integrator(tspan)
    x0, u = torch.ones((1, batch), dtype=torch.float64, device=dev), torch.tensor(u_h, device=dev)
    x = torch.empty((NSTEPS + 1, 2, batch), dtype=torch.float64, device=dev)
    lam, dJdu = torch.empty_like(x), torch.empty_like(u)
    J = torch.empty(batch, dtype=torch.float64, device=dev)

    def pair():
        integ.compute_states_dev(prob, x0, u, x, J)
        integ.compute_adjoints_dev(prob, u, None, lam, dJdu)
    ocs.distributed.prewarm(pair, 0.2, _sync, chunk=10)
    sp, dt = ocs.distributed.spread(ocs.distributed.timed_reps_max_over_ranks(pair, reps, _sync, inner=10))
    nbytes = 8.0 * (3 * 2 + 6 * 1) * batch * NSTEPS
    tr = _replayed_variant_traffic(f"auto_1_{batch}")
    return {"value": batch * NSTEPS / dt, "unit": "RK4 state+costate steps/s", "batch": batch, "nS": 1,
            "ms_per_pass_pair": dt * 1e3, "ms_per_pass_pair_spread": sp,
            "roofline": {"bound": "hbm (at 64 workgroups on 256 CUs the passes are bound by their serial chains: a quarter "
                                  "of the chip is in use)",
                         "kernel": "k_forward_p2 + k_backward_scan, pass pair", "achieved": nbytes / dt / 1e9,
                         "peak": HBM_PEAK_GBPS, "unit": "GB/s", "frac": nbytes / dt / 1e9 / HBM_PEAK_GBPS,
                         "traffic": tr[0], "traffic_source": tr[1]},
            "finite": bool(torch.isfinite(J).all().item())}


FP64_MFMA_PEAK_TFLOPS = FP64_PEAK_TFLOPS


def bl5_metric(ocs, dev, batch=8192, nsteps=4000, reps=2, shard=True):
    """BASELINE configs[4] (SURVEY BL-5): build-defined LQ32 (nS = 32, nC = 4, A = -diag(logspace(0,3,32)) + 0.1 G,
    seed 20260405), RK4InfiniteIntegrator with N2 = N = 4000 tail steps (|lambda_max| h = 2.5), uStar = 0,
    batch 8192 in total (sharded: 1024 per GPU at 8 GPUs -- 64 groups of 16 trajectories, i.e. 128 waves of the
    two-wave kernels on 1024 SIMDs: that leg is latency-bound by design of the config), full output.  The stage
    products A*Y / A'*k run on v_mfma_f64_16x16x4_f64 (csrc/ocs_lq_kernels.hip); fp64-compute-bound, so the roofline
    is the fp64 matrix peak."""
    world, rank, lo, hi = _shard(ocs, batch) if shard else (1, 0, 0, batch)
    nloc = hi - lo
    nS, nC, T = 32, 4, 10.0
    rng = np.random.default_rng(20260405)
    A = -np.diag(np.logspace(0, 3, nS)) + 0.1 * rng.normal(size=(nS, nS))
    Bu = rng.normal(size=(nS, nC))
    q, rd = rng.uniform(0.5, 1.5, nS), rng.uniform(1, 2, nC)
    prob = ocs.LQProblem(A, Bu, q, rd, 0.05, [[-1.0, 1.0]] * nC)
    N = nsteps
    integ = ocs.RK4InfiniteIntegrator(np.linspace(0, T, N + 1), np.linspace(T, 2 * T, N + 1), np.zeros(nC))
    g = torch.Generator(device=dev).manual_seed(20260405 + rank)
    u = torch.rand((2 * N + 1, nC, nloc), dtype=torch.float64, device=dev, generator=g) * 2 - 1
    x0 = torch.randn((nS, nloc), dtype=torch.float64, device=dev, generator=g)
    x = torch.empty((N + 1, nS + 1, nloc), dtype=torch.float64, device=dev)
    lam = torch.empty_like(x)
    dJdu = torch.empty_like(u)
    _, J = integ.compute_states_dev(prob, x0, u, x)
    integ.compute_adjoints_dev(prob, u, None, lam, dJdu)
    torch.cuda.synchronize()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
    tf = tb = 0.0
    for _ in range(reps):
        ev[0].record()
        integ.compute_states_dev(prob, x0, u, x, J)
        ev[1].record()
        integ.compute_adjoints_dev(prob, u, None, lam, dJdu)
        ev[2].record()
        torch.cuda.synchronize()
        tf += ev[0].elapsed_time(ev[1]) * 1e-3 / reps
        tb += ev[1].elapsed_time(ev[2]) * 1e-3 / reps

    def pair():
        integ.compute_states_dev(prob, x0, u, x, J)
        integ.compute_adjoints_dev(prob, u, None, lam, dJdu)
    sp5, dt = ocs.distributed.spread(ocs.distributed.timed_reps_max_over_ranks(pair, max(reps, 3), _sync))  # whole job: max over ranks, median
    steps_local = nloc * 2 * N                # RK4 steps of both legs (main + tail) on this rank
    # algorithmic flops per (trajectory, step): 4 F + 3 recomputed F + 4 A'k products of 2 nS^2, the Bu u / Bu' k
    # products, O(nS) axpys not counted (12 mat-vecs, here 11 because F4 is not needed in the adjoint)
    fl_fwd = 4 * 2 * nS * nS + 3 * 2 * nS * nC
    fl_bwd = 7 * 2 * nS * nS + 2 * 2 * nS * nC + 2 * 2 * nS * nC
    tfl_b = steps_local * fl_bwd / tb / 1e12
    tr5 = (None, None)
    try:   # HBM bytes of the adjoint kernels of a pass pair, replayed from the committed PMC summary
        t5 = json.load(open(os.path.join(ROOT, "profiles", "bl5_traffic_latest.json")))
        if t5.get("batch") == nloc and N == 4000:
            kb = sum(v["hbm_bytes_per_launch"] for k, v in t5["kernels"].items() if "backward" in k)
            tr5 = (kb, f"{t5['source']} (rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE passes, k_lq2_backward of both legs; replayed)")
    except Exception:
        pass
    try:   # ... of the chunked passes of the 1024-trajectory shard (scripts/profile_r04.sh + summarize_r04.py)
        t5s = json.load(open(os.path.join(ROOT, "profiles", "bl5_shard_traffic_latest.json")))
        if tr5[0] is None and t5s.get("batch") == nloc and N == 4000:
            tr5 = (t5s["hbm_bytes_adjoint_kernels_per_pass_pair"],
                   f"{t5s['source']} (rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE passes, the k_lq_backward launches of a pass pair; replayed)")
    except Exception:
        pass
    return {"value": batch * 2 * N / dt, "unit": "RK4 state+costate steps/s (both legs of RK4InfiniteIntegrator)",
            "batch": batch, "batch_per_gpu": nloc, "n_steps": N, "n_tail_steps": N, "ms_forward": tf * 1e3,
            "ms_adjoint": tb * 1e3, "ms_pass_pair_max_over_ranks": dt * 1e3, "ms_pass_pair_spread": sp5,
            "roofline": {"bound": "mfma", "kernel": ("k_lq_backward in time-parallel chunks (pass Z + carries + pass X, both legs; one wave "
                                                     "per 16 trajectories and chunk; 14 stage products per step instead of 7 -- "
                                                     "the flops counted are the algorithm's 7), this rank" if nloc <= 4096 else
                                                     "k_lq2_backward (adjoint + dJdu, both legs; two waves per 16 "
                                                     "trajectories), this rank") if nloc <= 8192 else
                                                    "k_lq_backward (adjoint + dJdu, both legs; one wave per 16 trajectories), this rank",
                         "achieved": tfl_b, "peak": FP64_MFMA_PEAK_TFLOPS, "unit": "TFLOP/s",
                         "frac": tfl_b / FP64_MFMA_PEAK_TFLOPS, "traffic": tr5[0], "traffic_source": tr5[1],
                         "algorithmic_flops_per_trajectory_step": fl_bwd},
            "pass_pair_TFLOPs": steps_local * (fl_fwd + fl_bwd) / (tf + tb) / 1e12,
            "finite": bool(torch.isfinite(lam[0]).all().item()) and bool(torch.isfinite(J).all().item())}


DUMP_TRAJECTORIES = 256      # trajectories of x / lam / dJdu written by --dump-outputs (~25 MB at N = 1000, nS = 4)
DUMP_J_MAX = 1 << 20         # entries of J written by --dump-outputs (all of them up to this batch)


def dump_outputs(out_dir, x, J, lam, dJdu):
    """Writes what the headline pass pair hands its caller -- x [N+1][nS+1][B], J [B], lam [N+1][nS+1][B],
    dJdu [2N+1][nC][B] -- as out_dir/<name>.npy in float64.  x, lam and dJdu are written for a fixed, seeded sample of
    DUMP_TRAJECTORIES trajectories (sorted batch indices, the same for every run with the same --batch), J for a sample
    of up to DUMP_J_MAX trajectories (the whole batch below that), so the files stay well under 64 MB."""
    os.makedirs(out_dir, exist_ok=True)
    batch = J.shape[0]
    rng = np.random.default_rng(20260416)
    cols = torch.tensor(np.sort(rng.choice(batch, min(batch, DUMP_TRAJECTORIES), replace=False)), device=J.device)
    jcols = torch.tensor(np.sort(rng.choice(batch, min(batch, DUMP_J_MAX), replace=False)), device=J.device)
    for name, t in (("x", x.index_select(2, cols)), ("J", J.index_select(0, jcols)),
                    ("lam", lam.index_select(2, cols)), ("dJdu", dJdu.index_select(2, cols))):
        np.save(os.path.join(out_dir, name + ".npy"), np.ascontiguousarray(t.cpu().numpy(), dtype=np.float64))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=BATCH,
                    help="trajectories per GPU (weak scaling, default: BASELINE config) / in total (strong scaling)")
    ap.add_argument("--scaling", choices=("weak", "strong"), default="weak",
                    help="weak: --batch per GPU (the driver's contract); strong: --batch is the total, split over the GPUs")
    ap.add_argument("--prewarm", type=float, default=1.0,
                    help="seconds of untimed passes before the W warm-up steps: the clocks of an idle GPU take a few "
                         "hundred ms to come up, and the K timed steps last only a few ms")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write x, J, lam and dJdu of the last timed step (a fixed, seeded sample of trajectories) as "
                         "DIR/<name>.npy, float64")
    ap.add_argument("--full", action="store_true",
                    help="also run everything beyond the headline figure: live PMC traffic, per-kernel event timings and "
                         "roofline, the secondary legs, the CPU baseline and its parity check")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="with --full: skip the CPU baseline")
    ap.add_argument("--no-live-traffic", action="store_true",
                    help="with --full: do not collect the PMC traffic counters in child processes first (roofline.traffic "
                         "is then the figure replayed from profiles/)")
    ap.add_argument("--no-fb-sweep", action="store_true",
                    help="with --full: skip the secondary legs (fb_sweep, BL-4, BL-5, large batch)")
    args = ap.parse_args()
    if args.steps < 1 or args.warmup < 0:
        ap.error("--steps must be >= 1 and --warmup >= 0")

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if args.gpus > 1 and world != args.gpus:
        raise SystemExit(f"--gpus {args.gpus} needs torch.distributed.run with --nproc-per-node {args.gpus}")
    import torch.distributed as dist
    LIVE = (live_traffic() if (args.full and world == 1 and not args.no_live_traffic and "RANK" not in os.environ)
            else None)
    # OCS_FORCE_COLLECTIVES=1 under torch.distributed.run with ONE process: the process group is created and every
    # collective of the N-rank path (asynchronous objective all-reduce and its drain, barriers, max over ranks, the
    # gathers of the secondary legs) executes on RCCL with world size 1 -- the rehearsal a one-GPU box allows
    use_dist = world > 1 or (os.environ.get("OCS_FORCE_COLLECTIVES") == "1" and "RANK" in os.environ)
    # OCS_BENCH_REHEARSAL=1: the N-rank code paths on a box with fewer GPUs than ranks -- ranks share the devices there are and
    # the process group runs on gloo (RCCL refuses two ranks on one device).  The line carries "rehearsal": true; its numbers
    # mean nothing (the ranks compete for one GPU).
    rehearsal = os.environ.get("OCS_BENCH_REHEARSAL") == "1" and world > 1
    ndev = max(torch.cuda.device_count(), 1)
    if use_dist:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        if rehearsal:
            torch.cuda.set_device(local_rank % ndev)
            dist.init_process_group("gloo")
        else:
            torch.cuda.set_device(local_rank)
            dist.init_process_group("nccl", device_id=torch.device("cuda", local_rank))
    dev = torch.device("cuda", (local_rank % ndev if rehearsal else local_rank) if world > 1 else 0)
    torch.cuda.set_device(dev)

    import __graft_entry__ as ge
    ocs = ge.load_package()  # raises if libocs.so is missing: no fallback path

    if args.scaling == "strong":
        lo, hi = ocs.distributed.shard_bounds(args.batch, world, rank)
        batch, total_batch = hi - lo, args.batch
    else:
        batch, total_batch = args.batch, args.batch * world
    tspan, x0_h, u_h = make_inputs(batch, dev, 20260401 + rank)
    prob = ocs.LogisticProblem(M, C_PAR, R_PAR, [[0.0, 1.0]])
    integ = ocs.RK4Integrator(tspan)
    x0 = torch.tensor(x0_h, device=dev)
    u = torch.tensor(u_h, device=dev)
    x = torch.empty((NSTEPS + 1, NS + 1, batch), dtype=torch.float64, device=dev)
    lam = torch.empty_like(x)
    dJdu = torch.empty_like(u)
    J = torch.empty(batch, dtype=torch.float64, device=dev)
    # one 8-byte buffer per step of a phase: the objective all-reduce of step k overlaps the kernels of step k+1
    Jsums = torch.zeros((max(args.steps, args.warmup, 1), 1), dtype=torch.float64, device=dev)
    pending = []

    ev = [[torch.cuda.Event(enable_timing=True) for _ in range(3)] for _ in range(args.steps)] if args.full else []

    def one_step(i, k=None):
        if k is not None:
            ev[k][0].record()
        integ.compute_states_dev(prob, x0, u, x, J)
        if k is not None:
            ev[k][1].record()
        integ.compute_adjoints_dev(prob, u, None, lam, dJdu)
        if k is not None:
            ev[k][2].record()
        if use_dist:
            # the one collective of the path: all-reduce(SUM) of the objective over the shards, 8 bytes; issued
            # asynchronously on RCCL's stream so that its latency hides under the next step's kernels
            torch.sum(J, dim=0, keepdim=True, out=Jsums[i])
            pending.append(dist.all_reduce(Jsums[i], async_op=True))

    def drain():
        for w in pending:
            w.wait()
        pending.clear()

    # steady state first: an idle GPU sits at low clocks; W = 3..5 steps (< 1 ms) do not bring them up
    tw = time.perf_counter()
    while time.perf_counter() - tw < args.prewarm:
        for _ in range(20):
            integ.compute_states_dev(prob, x0, u, x, J)
            integ.compute_adjoints_dev(prob, u, None, lam, dJdu)
        torch.cuda.synchronize()
    for i in range(args.warmup):
        one_step(i)
    drain()
    torch.cuda.synchronize()
    if use_dist:
        dist.barrier()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for k in range(args.steps):
        one_step(k)
    drain()  # every step's objective sum has arrived before the clock stops
    if use_dist:
        dist.barrier()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, x, J, lam, dJdu)
    if args.full:
        # per-kernel durations (roofline): K more steps, untimed, with HIP events between the two kernels (an event record
        # between kernels costs a few us of GPU idle time, so the timed steps above carry none, and these come after them)
        for k in range(args.steps):
            one_step(k, k)
        drain()
        torch.cuda.synchronize()
    if use_dist:
        tmax = torch.tensor([dt], dtype=torch.float64, device=dev)
        dist.all_reduce(tmax, op=dist.ReduceOp.MAX)
        dt = float(tmax.item())
    ok = bool(torch.isfinite(J).all().item()) and bool(torch.isfinite(dJdu).all().item())

    line = None
    if rank == 0:
        steps_total = total_batch * NSTEPS * args.steps
        line = {
            "metric": "RK4 state+costate steps/sec (batch*nSteps)",
            "value": steps_total / dt,
            "unit": "steps/s",
            "n_gpus": world,
            "collectives_executed": bool(use_dist),
            **({"rehearsal": True} if rehearsal else {}),
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": dt / args.steps * 1e3,
            "higher_is_better": True,
            "prewarm_s": args.prewarm,
            "scaling": args.scaling,
            "vs_baseline": None,
            "dtype": "f64",
            "data": "synthetic",
            "config": {"workload": "BL-2: LogisticK nS=4 (nAug=5, nC=1), 1000 RK4 steps, "
                                   f"batch={batch} control candidates per GPU, full output (x,J,lam,dJdu)",
                       "problem": "LogisticK(m=[3,2.5,2,1.5], c=1.5, r=0.05)", "n_steps": NSTEPS,
                       "batch_per_gpu": batch, "batch_total": total_batch, "parallelism": f"batch-sharded x{world}",
                       "mapping": "automatic: compute_states k_forward_p2 (wave-specialised, minimal recursion wave), "
                                  "compute_adjoints k_backward_scan (scan over time)"},
            "finite": ok,
        }
    if rank == 0 and args.full:
        # per-kernel durations from HIP events on the launch stream (torch's current stream)
        t_fwd = float(np.mean([e[0].elapsed_time(e[1]) for e in ev])) * 1e-3
        t_bwd = float(np.mean([e[1].elapsed_time(e[2]) for e in ev])) * 1e-3
        ev_f = sorted(e[0].elapsed_time(e[1]) * 1e3 for e in ev)
        ev_b = sorted(e[1].elapsed_time(e[2]) * 1e3 for e in ev)
        nA = NS + 1
        bytes_fwd = 8 * (nA + 2 * NC) * batch * NSTEPS           # write x, read u (2 new samples/step)
        bytes_bwd = 8 * (2 * nA + 4 * NC) * batch * NSTEPS       # read x, write lam, read u, write dJdu
        # HBM bytes per launch of the dominant kernel from rocprofv3 PMC passes (FETCH_SIZE / WRITE_SIZE, separate
        # passes, calibrated on a copy of known size); NOT measured by this run: replayed from the named
        # profile of the same kernels, or null
        traffic, traffic_source = None, None
        tr_path = os.path.join(ROOT, "profiles", "traffic_latest.json")
        if os.path.exists(tr_path):
            try:
                tr = json.load(open(tr_path))
                if tr.get("batch") == batch and tr.get("kernel") == "k_backward":
                    traffic = tr.get("hbm_bytes_per_launch")
                    traffic_source = (f"{tr.get('source')} (rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE passes of these kernels; "
                                      "replayed from that file, not collected by this run)")
            except Exception:
                traffic = None
        if LIVE and "bwd_one_set" in LIVE and batch == BATCH:
            traffic = LIVE["bwd_one_set"]["hbm_bytes_per_launch"]
            traffic_source = LIVE["source"]
        line.update({
            "roofline": {"bound": "hbm", "kernel": "k_backward_scan (compute_adjoints + compute_dJdu)",
                         "achieved": bytes_bwd / t_bwd / 1e9, "peak": HBM_PEAK_GBPS, "unit": "GB/s",
                         "frac": bytes_bwd / t_bwd / 1e9 / HBM_PEAK_GBPS, "traffic": traffic,
                         "traffic_source": traffic_source,
                         "algorithmic_bytes_per_launch": bytes_bwd, "avg_launch_s": t_bwd},
            "kernels": {"k_forward": {"avg_s": t_fwd, "alg_bytes": bytes_fwd,
                                      "GBps": bytes_fwd / t_fwd / 1e9,
                                      "bound": "dependent chain of the state recursion (8 fp64 operations per step)"},
                        "k_backward": {"avg_s": t_bwd, "alg_bytes": bytes_bwd,
                                       "GBps": bytes_bwd / t_bwd / 1e9},
                        "event_us_min_median_max": {"k_forward": [round(ev_f[0], 2), round(ev_f[len(ev_f) // 2], 2), round(ev_f[-1], 2)],
                                                    "k_backward": [round(ev_b[0], 2), round(ev_b[len(ev_b) // 2], 2), round(ev_b[-1], 2)]},
                        # the pass pair over the timed (event-free) steps of this rank
                        "pass_pair_GBps": (bytes_fwd + bytes_bwd) * args.steps / dt / 1e9,
                        "pass_pair_frac": (bytes_fwd + bytes_bwd) * args.steps / dt / 1e9 / HBM_PEAK_GBPS},
        })
        if LIVE:
            line["traffic_collected_by_this_run"] = LIVE
    # secondary legs: every rank runs them on its shard (collectives inside)
    if args.full and not args.no_fb_sweep:
        fb = fb_sweep_metric(ocs, dev)
        b4 = bl4_metric(ocs, dev)
        b5 = bl5_metric(ocs, dev)
        big = bl2_large_batch_metric(ocs, dev) if world == 1 else None
        one = bl2_single_state_metric(ocs, dev) if world == 1 else None
        rot = bl2_rotated_metric(ocs, dev, batch) if world == 1 else None
        ssr = strong_scaling_readiness(ocs, dev) if world == 1 and not use_dist else None
        if rank == 0:
            line["fb_sweep"] = fb
            line["other_configs"] = {"BL-4 chebyshev16 objective+gradient": b4,
                                     "BL-5 LQ32 + RK4InfiniteIntegrator (matrix cores)": b5}
            if big:
                line["other_configs"]["BL-2 problem at batch 65536 (lane mapping, HBM-bound regime)"] = big
            if one:
                line["other_configs"]["BL-2 shapes with one state (TestOCProblem, nAug = 2)"] = one
            if rot:
                if LIVE and "bwd_rotating" in LIVE and batch == BATCH:
                    rot["roofline"]["traffic"] = LIVE["fwd_rotating"]["hbm_bytes_per_launch"] + LIVE["bwd_rotating"]["hbm_bytes_per_launch"]
                    rot["roofline"]["traffic_source"] = LIVE["source"]
                line["other_configs"]["BL-2 pass pair over 3 rotating buffer sets (no reuse across steps: HBM, not Infinity Cache)"] = rot
            if LIVE and "fcc" in LIVE and "cst" in LIVE and fb["batch_per_gpu"] == 16384:
                fb["roofline"]["traffic"] = LIVE["fcc"]["hbm_bytes_per_launch"] + LIVE["cst"]["hbm_bytes_per_launch"]
                fb["roofline"]["traffic_source"] = LIVE["source"]
            if ssr:
                line["other_configs"]["strong-scaling readiness (8-GPU shard sizes on one GPU)"] = ssr
    if rank == 0:
        if args.full and not args.no_cpu_baseline and world == 1:
            cb, ref = cpu_baseline(tspan, x0_h, u_h)
            line["cpu_baseline"] = cb
            # the baseline run doubles as a parity check of the timed buffers
            err = float(np.max(np.abs(J.cpu().numpy() - ref["J"]) / np.maximum(1.0, np.abs(ref["J"]))))
            line["parity_J_max_rel_err_vs_oracle"] = err
        print(json.dumps(line), flush=True)
    if use_dist:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
