// ocs_bvp.cpp -- batched bvp_solver driver (functions/bvp_solver.m): damped Newton on the Simpson / Lobatto-IIIa
// collocation of the optimality system on the integrator grid, every instance with its own step length, line search and
// stopping test; the batch advances iteration by iteration until no instance is active (one host round trip each, a second
// one when a line search needs more than its first three step lengths).
#include "ocs_trace.hpp"
#include "ocs_handles.hpp"
#include "ocs_matlab.hpp"

#include <algorithm>

using namespace ocs;

struct ocs_bvp_state {
  // Newton workspace.  The step maps [A_i | b_i] of all intervals are kept and the forward substitution reads them again: the
  // sweep kernel then does not see the problem functor.  Storing only [P_i | p_i] would mean a second assembly in the forward
  // pass -- about 5 % of an iteration at one state, where the sweep is 84 % (NOTES.md), so time does not decide it there; four
  // states are unmeasured.  2 nS (2 nS + 1) doubles per interval and instance: DESIGN.md 3f has the footprint.
  DevBuf AB, PP, d, SS, MX, status, search, alpha, nrm2, cnt;
  // post-processing: the costate half of y, the interpolation points, the control on the 2N+1 grid
  DevBuf lamn, ugrid, KI, SI, TI, TUI;
  int nint = 0;
  const ocs_problem_s* tu_prob = nullptr;
  unsigned long long tu_version = 0;
  // the u0 start: x, lam of compute_x_lam under it
  DevBuf gx, gl;
  // host entry point
  DevBuf x0, y0, u0, y, xaug, lam, uint_, J, iters, conv, res, stage;
  // the mesh side (ocs_bvp_rms, ocs_bvp_prolong): rms [N][B] where the caller wants none, its chunk maxima, the Lobatto
  // points of the grid with their time coefficients, the prolongation map
  DevBuf rms, PM, pidx, ptheta;
  TcoefAt lobatto;
  // ... and their host entry points
  DevBuf use, rmsmax, rmsinst, ynew;
};
void ocs_bvp_state_free(ocs_bvp_state* s) { delete s; }

// what the driver does not take, checked before anything is uploaded or allocated (both entry points)
static int bvp_refuse(const ocs_integrator_s* g, const ocs_problem_s* p, const ocs_bvp_options* opt) {
  if (g->kind != 0) return fail(OCS_ERR_UNSUPPORTED, "bvp_solver needs an RK4Integrator grid");
  if (p->functor == Functor::LQ)
    return fail(OCS_ERR_UNSUPPORTED, "bvp_solver: the LQ problem is not supported (registry logistic family and plugins with nS <= 4, nC <= 2)");
  if (p->nS > 4 || p->nC > 2)
    return fail(OCS_ERR_UNSUPPORTED, "bvp_solver: nS = %d, nC = %d is beyond its kernels (nS <= 4, nC <= 2)", p->nS, p->nC);
  if (p->user && !p->user->has_cc)
    return fail(OCS_ERR_UNSUPPORTED, "bvp_solver needs ocs_ControlChar in the user problem source (has_control_char)");
  if (g->N + 1 > 65535)   // (the node index of the packing kernels and the chunk index of the assembly are grid dimensions)
    return fail(OCS_ERR_UNSUPPORTED, "bvp_solver: %d steps are beyond its kernels (at most 65534)", g->N);
  if (!(opt->NewtonTol > 0.0) || opt->MaxIter < 1 || opt->maxBacktracks < 0 || opt->maxBacktracks > 60 || opt->nINTERP_PTS < 2)
    return fail(OCS_ERR_INVALID, "bad options");
  return OCS_OK;
}

// the same refusals for the entry points that take no options (the mesh side)
static int bvp_refuse(const ocs_integrator_s* g, const ocs_problem_s* p) {
  ocs_bvp_options o;
  ocs_bvp_default_options(&o);
  return bvp_refuse(g, p, &o);
}

extern "C" {

int ocs_bvp_default_options(ocs_bvp_options* o) {
  if (!o) return fail(OCS_ERR_INVALID, "null argument");
  o->NewtonTol = 1e-10;
  o->MaxIter = 40;
  o->maxBacktracks = 12;
  o->nINTERP_PTS = 1001;   // bvp_solver.m:20
  o->cost_row = 0;
  return OCS_OK;
}

int ocs_bvp_solver_dev(ocs_integrator g, ocs_problem p, int batch, const double* x0, const ocs_bvp_options* opt,
                       const double* y0, const double* u0grid, double* ynodes, double* xaug, double* lam,
                       double* uInterp, double* J, int* iterations, int* converged, double* resnorm, void* stream) {
  OCS_TRY(refuse_tiled(g, "ocs_bvp_solver"));
  OCS_TRACE("ocs_bvp_solver_dev");
  if (!g || !p || !x0 || !opt || !ynodes || !xaug || !lam || !uInterp || !J || !iterations || !converged || !resnorm ||
      batch < 1)
    return fail(OCS_ERR_INVALID, "bad argument");
  OCS_TRY(bvp_refuse(g, p, opt));
  hipStream_t s = (hipStream_t)stream;
  OCS_TRY(bind_problem(g, p, batch, s));
  OCS_TRY(fbs_ensure_tables(g));
  if (!g->bvp) g->bvp = new ocs_bvp_state();
  ocs_bvp_state* f = g->bvp;
  const int N = g->N, nS = p->nS, nC = p->nC, nY = 2 * nS, nAug = nS + 1, nT = 2 * N + 1, nI = opt->nINTERP_PTS;
  const size_t B = (size_t)batch;
  const int nparts = bvp_chunks(N), nbt = opt->maxBacktracks;
  OCS_TRY(f->AB.ensure(sizeof(double) * (size_t)N * nY * (nY + 1) * B));
  OCS_TRY(f->PP.ensure(sizeof(double) * (size_t)(N + 1) * nS * (nS + 1) * B));
  OCS_TRY(f->d.ensure(sizeof(double) * (size_t)(N + 1) * nY * B));
  OCS_TRY(f->SS.ensure(sizeof(double) * (size_t)nparts * B));
  OCS_TRY(f->MX.ensure(sizeof(double) * (size_t)nparts * B));
  OCS_TRY(f->status.ensure(sizeof(int) * B));
  OCS_TRY(f->search.ensure(sizeof(int) * B));
  OCS_TRY(f->alpha.ensure(sizeof(double) * B));
  OCS_TRY(f->nrm2.ensure(sizeof(double) * B));
  OCS_TRY(f->cnt.ensure(sizeof(int) * (size_t)(nbt + 3)));
  int* status = (int*)f->status.p;
  int* search = (int*)f->search.p;
  int* cnt = (int*)f->cnt.p;   // [0 .. nbt]: instances still searching after trial t; [nbt + 1], [nbt + 2]: still active after the first / second stage of the iteration
  const ProblemDesc pd = describe(p);
  const GridDesc gd = describe(g);

  // ---- the start (bvp_solver.m:87-98) ----
  if (y0) {
    HIP_TRY(hipMemcpyAsync(ynodes, y0, sizeof(double) * (size_t)(N + 1) * nY * B, hipMemcpyDeviceToDevice, s));
  } else if (u0grid) {
    OCS_TRY(f->gx.ensure(sizeof(double) * (size_t)(N + 1) * nAug * B));
    OCS_TRY(f->gl.ensure(sizeof(double) * (size_t)(N + 1) * nS * B));
    OCS_TRY(ocs_compute_x_lam_dev(g, p, batch, x0, u0grid, f->gx.d(), f->gl.d(), nullptr, s));
    LAUNCH_TRY(launch_bvp_pack(N + 1, nS, batch, f->gx.d(), nAug, true, f->gl.d(), ynodes, s));
  } else {
    LAUNCH_TRY(launch_bvp_pack(N + 1, nS, batch, x0, nS, false, nullptr, ynodes, s));
  }
  LAUNCH_TRY(launch_bvp_init(batch, status, search, iterations, f->alpha.d(), s));
  BvpIterate it{batch, x0, ynodes, ynodes, 0.0, status, search, f->AB.d(), f->SS.d(), f->MX.d(), nullptr};
  BvpVerdictArgs va{batch, nparts, f->SS.d(), f->MX.d(), opt->NewtonTol, search, status, f->nrm2.d(), resnorm, f->alpha.d(), nullptr};
  LAUNCH_TRY(launch_bvp_norm(pd, gd, it, s));   // (alpha = 0: the residual of the start itself)
  LAUNCH_TRY(launch_bvp_accept(va, true, 0.0, nullptr, s));
  it.d = f->d.d();

  // ---- Newton iterations: assembly, block elimination, line search, update; then the host reads the count ----
  // The trials of a line search are enqueued without asking the host; each looks first at the device count of instances the
  // trial before left searching.  Most iterations accept the full step, so only the first kHead trials go out with the
  // iteration; the host reads their count together with the count of active instances (one wait), and only if some instance
  // is still searching do the remaining trials follow, with a second update and the final bookkeeping.
  constexpr int kHead = 3;
  int counts[2];
  int nactive = batch;
  for (int k = 1; k <= opt->MaxIter && nactive > 0; ++k) {
    HIP_TRY(hipMemsetAsync(cnt, 0, sizeof(int) * (size_t)(nbt + 3), s));
    it.gate = nullptr;
    LAUNCH_TRY(launch_bvp_assemble(pd, gd, it, s));
    const BvpSweepArgs sw{N, batch, k, f->AB.d(), f->PP.d(), ynodes, x0, f->d.d(), status, search, iterations, f->alpha.d()};
    LAUNCH_TRY(launch_bvp_sweep(nS, sw, s));
    auto trials = [&](int t0, int t1) -> int {
      for (int t = t0; t <= t1; ++t) {
        it.gate = t > 0 ? cnt + (t - 1) : nullptr;
        it.alpha = std::ldexp(1.0, -t);
        LAUNCH_TRY(launch_bvp_norm(pd, gd, it, s));
        va.slot = cnt + t;
        LAUNCH_TRY(launch_bvp_accept(va, false, it.alpha, it.gate, s));
      }
      return OCS_OK;
    };
    const int head = std::min(kHead - 1, nbt);   // last trial of the first stage
    OCS_TRY(trials(0, head));
    LAUNCH_TRY(launch_bvp_update((N + 1) * nY, batch, f->alpha.d(), f->d.d(), ynodes, s));
    va.slot = cnt + (nbt + 1);
    LAUNCH_TRY(launch_bvp_finish(va, k, opt->MaxIter, head == nbt, s));
    HIP_TRY(hipMemcpyAsync(&counts[0], cnt + head, sizeof(int), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(&counts[1], cnt + (nbt + 1), sizeof(int), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    nactive = counts[1];
    if (head < nbt && counts[0] > 0) {
      OCS_TRY(trials(head + 1, nbt));
      LAUNCH_TRY(launch_bvp_update((N + 1) * nY, batch, f->alpha.d(), f->d.d(), ynodes, s));
      va.slot = cnt + (nbt + 2);
      LAUNCH_TRY(launch_bvp_finish(va, k, opt->MaxIter, true, s));
      HIP_TRY(hipMemcpyAsync(&nactive, cnt + (nbt + 2), sizeof(int), hipMemcpyDeviceToHost, s));
      HIP_TRY(hipStreamSynchronize(s));
    }
  }
  LAUNCH_TRY(launch_bvp_converged(batch, status, converged, s));
  int nfailed = 0;
  {   // (MaxIter iterations leave no instance active: what is not converged has failed)
    std::vector<int> st(B);
    HIP_TRY(hipMemcpyAsync(st.data(), status, sizeof(int) * B, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    for (int v : st) nfailed += v != 1;
  }

  // ---- post-processing (bvp_solver.m:124-132) ----
  // uInterp = ControlChar(interpPts, x(interpPts), lam(interpPts)), x and lam the pchip interpolants of the nodal solution
  if (f->nint != nI) {
    OCS_TRY(fbs_build_points(g, nI, f->KI, f->SI, f->TI));
    f->nint = nI;
    f->tu_prob = nullptr;
  }
  if (f->tu_prob != p || f->tu_version != p->version) {
    OCS_TRY(f->TUI.ensure(sizeof(double) * (size_t)nI * std::max(1, functor_ntu(p->functor, p->nS))));
    LAUNCH_TRY(launch_tu_at(pd, nI, f->TI.d(), f->TUI.d(), s));
    f->tu_prob = p;
    f->tu_version = p->version;
  }
  OCS_TRY(f->lamn.ensure(sizeof(double) * (size_t)(N + 1) * nS * B));
  LAUNCH_TRY(launch_bvp_costate_rows(N + 1, nS, batch, ynodes, f->lamn.d(), s));
  LAUNCH_TRY(launch_control_pts(pd, fbs_tables(g), nI, (const int*)f->KI.p, f->SI.d(), f->TUI.d(), batch, ynodes, nY,
                                f->lamn.d(), uInterp, nullptr, 0, nullptr, nullptr, 0.0, 0.0, s));
  // soln.u = pchip of those samples (:126), sampled on the 2N+1 grid; [soln.x, soln.lam, soln.J] = compute_x_lam_J under it (:132)
  OCS_TRY(f->ugrid.ensure(sizeof(double) * (size_t)nT * nC * B));
  {
    std::vector<double> pts(nI);
    matlab_linspace(g->t.front(), g->t.back(), nI, pts.data());   // :99
    OCS_TRY(ocs_interp_dev(OCS_INTERP_PCHIP, nC, nI, pts.data(), uInterp, nT, g->t.data(), f->ugrid.d(), batch, s));
  }
  OCS_TRY(ocs_compute_x_lam_dev(g, p, batch, x0, f->ugrid.d(), xaug, lam, J, s));
  return nfailed > 0 ? OCS_NUM_NOT_CONVERGED : OCS_OK;
}

int ocs_bvp_solver(ocs_integrator g, ocs_problem p, int batch, const double* x0, const ocs_bvp_options* opt,
                   const double* y0, const double* u0grid, double* ynodes, double* x, double* lam, double* uInterp,
                   double* J, int* iterations, int* converged, double* resnorm) {
  OCS_TRACE("ocs_bvp_solver");
  if (!g || !p || !x0 || !opt || !ynodes || !x || !lam || !uInterp || !J || !iterations || !converged || !resnorm || batch < 1)
    return fail(OCS_ERR_INVALID, "bad argument");
  OCS_TRY(bvp_refuse(g, p, opt));
  OCS_TRY(upload_grid(g));
  if (!g->bvp) g->bvp = new ocs_bvp_state();
  ocs_bvp_state* f = g->bvp;
  const int N = g->N, nS = p->nS, nC = p->nC, nY = 2 * nS, nAug = nS + 1, nT = 2 * N + 1, nI = opt->nINTERP_PTS;
  const size_t B = (size_t)batch;
  hipStream_t s = g->stream;
  HIP_TRY(hipStreamSynchronize(s));   // (before every stage_in here: the stage buffer may still be in use)
  OCS_TRY(stage_in(f->stage, f->x0, x0, nS, batch, s));
  if (y0) {
    HIP_TRY(hipStreamSynchronize(s));
    OCS_TRY(stage_in(f->stage, f->y0, y0, nY * (N + 1), batch, s));
  } else if (u0grid) {
    HIP_TRY(hipStreamSynchronize(s));
    OCS_TRY(stage_in(f->stage, f->u0, u0grid, nC * nT, batch, s));
  }
  OCS_TRY(f->y.ensure(sizeof(double) * (size_t)(N + 1) * nY * B));
  OCS_TRY(f->xaug.ensure(sizeof(double) * (size_t)(N + 1) * nAug * B));
  OCS_TRY(f->lam.ensure(sizeof(double) * (size_t)(N + 1) * nS * B));
  OCS_TRY(f->uint_.ensure(sizeof(double) * (size_t)nI * nC * B));
  OCS_TRY(f->J.ensure(sizeof(double) * B));
  OCS_TRY(f->iters.ensure(sizeof(int) * B));
  OCS_TRY(f->conv.ensure(sizeof(int) * B));
  OCS_TRY(f->res.ensure(sizeof(double) * B));
  const int st = ocs_bvp_solver_dev(g, p, batch, f->x0.d(), opt, y0 ? f->y0.d() : nullptr, (!y0 && u0grid) ? f->u0.d() : nullptr,
                                    f->y.d(), f->xaug.d(), f->lam.d(), f->uint_.d(), f->J.d(), (int*)f->iters.p,
                                    (int*)f->conv.p, f->res.d(), s);
  if (st < 0) return st;
  OCS_TRY(stage_out(f->stage, f->y.d(), ynodes, (N + 1) * nY, batch, s));
  {   // soln.x: the nS state rows of xaug
    std::vector<double> tmp((size_t)(N + 1) * nAug * B);
    OCS_TRY(stage_out(f->stage, f->xaug.d(), tmp.data(), (N + 1) * nAug, batch, s));
    for (size_t b = 0; b < B; ++b)
      for (int i = 0; i <= N; ++i)
        for (int k = 0; k < nS; ++k) x[(b * (N + 1) + i) * nS + k] = tmp[(b * (N + 1) + i) * nAug + k];
  }
  OCS_TRY(stage_out(f->stage, f->lam.d(), lam, (N + 1) * nS, batch, s));
  OCS_TRY(stage_out(f->stage, f->uint_.d(), uInterp, nI * nC, batch, s));
  HIP_TRY(hipMemcpy(J, f->J.p, sizeof(double) * B, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(iterations, f->iters.p, sizeof(int) * B, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(converged, f->conv.p, sizeof(int) * B, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(resnorm, f->res.p, sizeof(double) * B, hipMemcpyDeviceToHost));
  return st;
}

// ---- the mesh side: residual estimate of a nodal solution, prolongation to another mesh ----
int ocs_bvp_rms_dev(ocs_integrator g, ocs_problem p, int batch, const double* ynodes, const int* use, double* rms,
                    double* rmsmax, double* rmsinst, void* stream) {
  OCS_TRY(refuse_tiled(g, "ocs_bvp_rms"));
  OCS_TRACE("ocs_bvp_rms_dev");
  if (!g || !p || !ynodes || !rmsmax || !rmsinst || batch < 1) return fail(OCS_ERR_INVALID, "bad argument");
  OCS_TRY(bvp_refuse(g, p));
  hipStream_t s = (hipStream_t)stream;
  OCS_TRY(bind_problem(g, p, batch, s));
  if (!g->bvp) g->bvp = new ocs_bvp_state();
  ocs_bvp_state* f = g->bvp;
  const int N = g->N;
  const size_t B = (size_t)batch;
  std::vector<double> tl;
  if (!f->lobatto.T.p) {   // t_m -/+ (h/2) sqrt(3/7) in fp64, like the grid itself: the same numbers for every implementation
    tl.resize((size_t)2 * N);
    const double s37 = std::sqrt(3.0 / 7.0);
    for (int i = 0; i < N; ++i) {
      const double d = g->h[i] / 2 * s37;
      tl[2 * (size_t)i] = g->t[2 * (size_t)i + 1] - d;
      tl[2 * (size_t)i + 1] = g->t[2 * (size_t)i + 1] + d;
    }
  }
  OCS_TRY(f->lobatto.ensure(p, 2 * N, tl.data(), s));
  if (!rms) {
    OCS_TRY(f->rms.ensure(sizeof(double) * (size_t)N * B));
    rms = f->rms.d();
  }
  const int nparts = bvp_chunks(N);
  OCS_TRY(f->PM.ensure(sizeof(double) * (size_t)nparts * B));
  LAUNCH_TRY(launch_bvp_rms(describe(p), describe(g), batch, f->lobatto.TC.d(), f->lobatto.TU.d(), ynodes, rms, f->PM.d(), s));
  LAUNCH_TRY(launch_interval_reduce(N, batch, nparts, rms, nullptr, f->PM.d(), nullptr, use, rmsmax, rmsinst, nullptr, s));
  return OCS_OK;
}

int ocs_bvp_rms(ocs_integrator g, ocs_problem p, int batch, const double* ynodes, const int* use, double* rms,
                double* rmsmax, double* rmsinst) {
  OCS_TRACE("ocs_bvp_rms");
  if (!g || !p || !ynodes || !rmsmax || !rmsinst || batch < 1) return fail(OCS_ERR_INVALID, "bad argument");
  OCS_TRY(refuse_tiled(g, "ocs_bvp_rms"));
  OCS_TRY(bvp_refuse(g, p));
  OCS_TRY(upload_grid(g));
  if (!g->bvp) g->bvp = new ocs_bvp_state();
  ocs_bvp_state* f = g->bvp;
  const int N = g->N, nY = 2 * p->nS;
  const size_t B = (size_t)batch;
  hipStream_t s = g->stream;
  HIP_TRY(hipStreamSynchronize(s));   // (the stage buffer may still be in use)
  OCS_TRY(stage_in(f->stage, f->y, ynodes, nY * (N + 1), batch, s));
  const int* duse;
  OCS_TRY(stage_flags(f->use, use, batch, s, &duse));
  OCS_TRY(f->rms.ensure(sizeof(double) * (size_t)N * B));
  OCS_TRY(f->rmsmax.ensure(sizeof(double) * (size_t)N));
  OCS_TRY(f->rmsinst.ensure(sizeof(double) * B));
  OCS_TRY(ocs_bvp_rms_dev(g, p, batch, f->y.d(), duse, f->rms.d(), f->rmsmax.d(), f->rmsinst.d(), s));
  if (rms) OCS_TRY(stage_out(f->stage, f->rms.d(), rms, N, batch, s));
  return fetch({{rmsmax, f->rmsmax, (size_t)N}, {rmsinst, f->rmsinst, B}}, s);
}

int ocs_bvp_prolong_dev(ocs_integrator g_old, ocs_problem p, int batch, const double* ynodes_old, int nnew, const int* idx,
                        const double* theta, double* ynew, void* stream) {
  ocs_integrator g = g_old;
  OCS_TRY(refuse_tiled(g, "ocs_bvp_prolong"));
  OCS_TRACE("ocs_bvp_prolong_dev");
  if (!g || !p || !ynodes_old || !idx || !theta || !ynew || batch < 1 || nnew < 1) return fail(OCS_ERR_INVALID, "bad argument");
  OCS_TRY(bvp_refuse(g, p));
  if (nnew > 65535) return fail(OCS_ERR_UNSUPPORTED, "bvp_solver: %d steps are beyond its kernels (at most 65534)", nnew - 1);
  for (int j = 0; j < nnew; ++j)
    if (idx[j] < 0 || idx[j] >= g->N || !(theta[j] >= 0.0 && theta[j] <= 1.0))
      return fail(OCS_ERR_INVALID, "ocs_bvp_prolong: node %d lies outside the old mesh (interval %d of %d, theta %g)", j, idx[j],
                  g->N, theta[j]);
  hipStream_t s = (hipStream_t)stream;
  OCS_TRY(bind_problem(g, p, batch, s));
  if (!g->bvp) g->bvp = new ocs_bvp_state();
  ocs_bvp_state* f = g->bvp;
  HIP_TRY(hipStreamSynchronize(s));   // (a map of an earlier call may still be read)
  OCS_TRY(f->pidx.ensure(sizeof(int) * (size_t)nnew));
  OCS_TRY(f->ptheta.ensure(sizeof(double) * (size_t)nnew));
  HIP_TRY(hipMemcpyAsync(f->pidx.p, idx, sizeof(int) * (size_t)nnew, hipMemcpyHostToDevice, s));
  HIP_TRY(hipMemcpyAsync(f->ptheta.p, theta, sizeof(double) * (size_t)nnew, hipMemcpyHostToDevice, s));
  LAUNCH_TRY(launch_bvp_prolong(describe(p), describe(g), batch, ynodes_old, nnew, (const int*)f->pidx.p, f->ptheta.d(), ynew, s));
  HIP_TRY(hipStreamSynchronize(s));   // (idx and theta are the caller's again)
  return OCS_OK;
}

int ocs_bvp_prolong(ocs_integrator g_old, ocs_problem p, int batch, const double* ynodes_old, int nnew, const int* idx,
                    const double* theta, double* ynew) {
  ocs_integrator g = g_old;
  OCS_TRACE("ocs_bvp_prolong");
  if (!g || !p || !ynodes_old || !idx || !theta || !ynew || batch < 1 || nnew < 1) return fail(OCS_ERR_INVALID, "bad argument");
  OCS_TRY(refuse_tiled(g, "ocs_bvp_prolong"));
  OCS_TRY(bvp_refuse(g, p));
  OCS_TRY(upload_grid(g));
  if (!g->bvp) g->bvp = new ocs_bvp_state();
  ocs_bvp_state* f = g->bvp;
  const int N = g->N, nY = 2 * p->nS;
  hipStream_t s = g->stream;
  HIP_TRY(hipStreamSynchronize(s));
  OCS_TRY(stage_in(f->stage, f->y, ynodes_old, nY * (N + 1), batch, s));
  OCS_TRY(f->ynew.ensure(sizeof(double) * (size_t)nnew * nY * batch));
  OCS_TRY(ocs_bvp_prolong_dev(g, p, batch, f->y.d(), nnew, idx, theta, f->ynew.d(), s));
  OCS_TRY(stage_out(f->stage, f->ynew.d(), ynew, nnew * nY, batch, s));
  return OCS_OK;
}

}  // extern "C"
