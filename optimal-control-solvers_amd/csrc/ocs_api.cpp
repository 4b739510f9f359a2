// ocs_api.cpp -- the C-ABI of libocs.so (include/ocs.h): handle bookkeeping, argument
// validation, host<->device staging and layout conversion around the gfx950 kernels.
// No compute happens on the host here; if no MI355X is usable every compute entry point
// fails with OCS_ERR_NO_DEVICE.
#include "ocs_trace.hpp"
#include "ocs_handles.hpp"

#include <memory>

using namespace ocs;

// ------------------------------------------------------------------------------------
// library
// ------------------------------------------------------------------------------------
extern "C" {

const char* ocs_version(void) { return "ocs-mi355x 0.1 (gfx950, fp64)"; }
const char* ocs_last_error(void) { return err_string().c_str(); }

int ocs_device_count(int* count) {
  if (!count) return fail(OCS_ERR_INVALID, "count is NULL");
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) n = 0;
  *count = n;
  return OCS_OK;
}
int ocs_set_device(int device) {
  OCS_TRY(require_device());
  HIP_TRY(hipSetDevice(device));
  return OCS_OK;
}
int ocs_synchronize(void) {
  OCS_TRY(require_device());
  HIP_TRY(hipDeviceSynchronize());
  return OCS_OK;
}

// ------------------------------------------------------------------------------------
// OCProblem
// ------------------------------------------------------------------------------------
int ocs_problem_create(ocs_problem* out, int problem_id, int nS, int nC, const double* params, int nparams,
                       const double* control_bounds) {
  if (!out || !params || !control_bounds) return fail(OCS_ERR_INVALID, "null argument");
  *out = nullptr;
  std::unique_ptr<ocs_problem_s> p(new ocs_problem_s());
  p->id = problem_id;
  p->nS = nS;
  p->nC = nC;
  if (problem_id == OCS_PROBLEM_TEST) {
    // tests/TestOCProblem.m:16-20, params [c m r] -> LogisticK<1> block [c r m]
    if (nS != 1 || nC != 1 || nparams != 3)
      return fail(OCS_ERR_SHAPE, "TestOCProblem needs nS=1, nC=1, params [c m r]");
    p->functor = Functor::Logistic;
    p->par = {params[0], params[2], params[1]};
    p->user2func = {0, 2, 1};
  } else if (problem_id == OCS_PROBLEM_LOGISTIC) {
    if (nS < 1 || nC != 1 || nparams != 2 + nS)
      return fail(OCS_ERR_SHAPE, "LogisticK needs nC=1 and params [c r m_1..m_nS]");
    p->functor = Functor::Logistic;
    p->par.assign(params, params + nparams);
    p->user2func.resize(nparams);
    for (int k = 0; k < nparams; ++k) p->user2func[k] = k;
  } else if (problem_id == OCS_PROBLEM_LQ) {
    // build-defined linear-quadratic problem: params [r | A | Bu | q | rdiag]
    if (nS < 1 || nC < 1 || nparams != 1 + nS * nS + nS * nC + nS + nC)
      return fail(OCS_ERR_SHAPE, "LQ needs params [r | A (nS x nS) | Bu (nS x nC) | q (nS) | rdiag (nC)]");
    p->functor = Functor::LQ;
    p->par.assign(params, params + nparams);
    p->user2func.resize(nparams);
    for (int k = 0; k < nparams; ++k) p->user2func[k] = k;
  } else {
    return fail(OCS_ERR_UNSUPPORTED, "unknown problem id %d", problem_id);
  }
  if (!functor_supported(p->functor, nS, nC))
    return fail(OCS_ERR_UNSUPPORTED, "no kernel instantiated for nS=%d nC=%d", nS, nC);
  p->bounds.assign(control_bounds, control_bounds + 2 * nC);
  p->version = next_version();
  *out = p.release();
  return OCS_OK;
}

int ocs_problem_destroy(ocs_problem p) {
  delete p;   // (~ocs_problem_s: the shadow problem and the hipRTC module, then the buffers)
  return OCS_OK;
}

int ocs_problem_dims(ocs_problem p, int* nS, int* nC) {
  if (!p) return fail(OCS_ERR_INVALID, "null problem");
  if (nS) *nS = p->nS;
  if (nC) *nC = p->nC;
  return OCS_OK;
}

int ocs_problem_set_batch_params(ocs_problem p, int batch, const int* param_index, int nidx,
                                 const double* values) {
  if (!p) return fail(OCS_ERR_INVALID, "null problem");
  if (nidx == 0) {  // clear
    p->pmask = 0;
    p->has_w = false;
    p->pb_batch = 0;
    p->version = next_version();
    return OCS_OK;
  }
  if (!param_index || !values || batch < 1 || nidx < 0) return fail(OCS_ERR_INVALID, "bad argument");
  OCS_TRY(upload_problem(p));
  const int npar = (int)p->par.size();
  if (p->functor == Functor::LQ) {
    // The cost weights q and rdiag (the tail of [r | A | Bu | q | rdiag]) are per-lane registers of the matrix-core kernels and
    // may differ per trajectory; an index set inside that range goes to a dense array of its own, W [nS + nC][batch], which
    // holds every trajectory's full q and rdiag (rows not named: the shared values).  Any other set takes the mask path below.
    const int w0 = 1 + p->nS * p->nS + p->nS * p->nC, nW = p->nS + p->nC;
    bool weights_only = true;
    for (int q = 0; q < nidx; ++q) weights_only = weights_only && param_index[q] >= w0 && param_index[q] < npar;
    if (weights_only) {
      std::vector<double> W((size_t)nW * batch);
      for (int r = 0; r < nW; ++r)
        for (int b = 0; b < batch; ++b) W[(size_t)r * batch + b] = p->par[w0 + r];
      for (int q = 0; q < nidx; ++q)
        for (int b = 0; b < batch; ++b) W[(size_t)(param_index[q] - w0) * batch + b] = values[(size_t)b * nidx + q];
      OCS_TRY(p->d_w.ensure(sizeof(double) * W.size()));
      HIP_TRY(hipMemcpy(p->d_w.p, W.data(), sizeof(double) * W.size(), hipMemcpyHostToDevice));
      p->pmask = 0;
      p->has_w = true;
      p->pb_batch = batch;
      p->version = next_version();
      return OCS_OK;
    }
  }
  if (npar > 32) return fail(OCS_ERR_UNSUPPORTED, "per-trajectory parameters need <= 32 parameters");
  if (p->user && (npar > 16 || user_rowsep(p->user)))
    return fail(OCS_ERR_UNSUPPORTED, "user problems with more than 16 parameters or given as row functions read the "
                                     "shared parameter block only: no per-trajectory parameters");
  if (p->user && p->user->tcoef_hooks)
    return fail(OCS_ERR_UNSUPPORTED, "the problem source defines ocs_tcoef / ocs_cc_tcoef, whose values are tabulated once per "
                                     "grid point from the SHARED parameter block: no per-trajectory parameters");
  const unsigned tcmask = functor_tc_param_mask(p->functor, p->nS);
  unsigned mask = 0;
  std::vector<double> pb((size_t)npar * batch, 0.0);
  for (int q = 0; q < nidx; ++q) {
    const int ui = param_index[q];
    if (ui < 0 || ui >= npar) return fail(OCS_ERR_INVALID, "parameter index %d out of range", ui);
    const int fi = p->user2func[ui];
    if ((tcmask >> fi) & 1u)
      return fail(OCS_ERR_UNSUPPORTED,
                  "parameter %d feeds the time-coefficient table and must be batch-uniform", ui);
    mask |= 1u << fi;
    for (int b = 0; b < batch; ++b) pb[(size_t)fi * batch + b] = values[(size_t)b * nidx + q];
  }
  OCS_TRY(p->d_pb.ensure(sizeof(double) * pb.size()));
  HIP_TRY(hipMemcpy(p->d_pb.p, pb.data(), sizeof(double) * pb.size(), hipMemcpyHostToDevice));
  p->pmask = mask;
  p->has_w = false;
  p->pb_batch = batch;
  p->version = next_version();
  return OCS_OK;
}

int ocs_problem_set_batch_bounds(ocs_problem p, int batch, const double* lb, const double* ub) {
  if (!p) return fail(OCS_ERR_INVALID, "null problem");
  if (!lb && !ub) {  // clear
    p->bb_batch = 0;
    p->bb.clear();
    p->version = next_version();
    return OCS_OK;
  }
  if (!lb || !ub) return fail(OCS_ERR_INVALID, "give both lb and ub, or neither to clear");
  if (batch < 1) return fail(OCS_ERR_INVALID, "batch must be >= 1");
  const int nC = p->nC;
  std::vector<double> m(2 * (size_t)nC * batch);   // nC x batch column-major -> [nC][batch]
  double* um = m.data() + (size_t)nC * batch;
  for (int b = 0; b < batch; ++b)
    for (int c = 0; c < nC; ++c) {
      const double lo = lb[(size_t)b * nC + c], hi = ub[(size_t)b * nC + c];
      if (!(lo <= hi)) return fail(OCS_ERR_INVALID, "lb > ub (or NaN) at control %d of trajectory %d", c, b);
      m[(size_t)c * batch + b] = lo;
      um[(size_t)c * batch + b] = hi;
    }
  return set_batch_bounds_minor(p, batch, m.data(), um);
}

static int eval_common(ocs_problem p, int which, int k, const double* t, const double* y, const double* u,
                       const double* v, double* out) {
  if (!p || !t || !y || !u || !out || (which != 0 && !v) || k < 1) return fail(OCS_ERR_INVALID, "bad argument");
  if (p->has_w)
    return fail(OCS_ERR_UNSUPPORTED, "F / dFdx_times_vec / dFdu_times_vec: per-trajectory cost weights have no meaning for k free columns");
  OCS_TRY(upload_problem(p));
  const int nAug = p->nS + 1, nC = p->nC;
  const int nout = (which == 2) ? nC : nAug;
  DevBuf dt, dy, du, dv, dout;
  OCS_TRY(dt.ensure(sizeof(double) * k));
  OCS_TRY(dy.ensure(sizeof(double) * (size_t)nAug * k));
  OCS_TRY(du.ensure(sizeof(double) * (size_t)nC * k));
  OCS_TRY(dv.ensure(sizeof(double) * (size_t)nAug * k));
  OCS_TRY(dout.ensure(sizeof(double) * (size_t)nout * k));
  HIP_TRY(hipMemcpy(dt.p, t, sizeof(double) * k, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(dy.p, y, sizeof(double) * (size_t)nAug * k, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(du.p, u, sizeof(double) * (size_t)nC * k, hipMemcpyHostToDevice));
  if (which != 0) HIP_TRY(hipMemcpy(dv.p, v, sizeof(double) * (size_t)nAug * k, hipMemcpyHostToDevice));
  LAUNCH_TRY(launch_eval(describe(p), which, k, dt.d(), dy.d(), du.d(), dv.d(), dout.d(), nullptr));
  HIP_TRY(hipMemcpy(out, dout.p, sizeof(double) * (size_t)nout * k, hipMemcpyDeviceToHost));
  return OCS_OK;
}
int ocs_problem_F(ocs_problem p, int k, const double* t, const double* y, const double* u, double* out) {
  return eval_common(p, 0, k, t, y, u, nullptr, out);
}
int ocs_problem_dFdx_times_vec(ocs_problem p, int k, const double* t, const double* y, const double* u,
                               const double* v, double* out) {
  return eval_common(p, 1, k, t, y, u, v, out);
}
int ocs_problem_dFdu_times_vec(ocs_problem p, int k, const double* t, const double* y, const double* u,
                               const double* v, double* out) {
  return eval_common(p, 2, k, t, y, u, v, out);
}

// compute_equilibrium.m:1-34, batched (k_equilibrium)
static int equilibrium_check(ocs_problem p, int batch) {
  if (!p || batch < 1) return fail(OCS_ERR_INVALID, "bad argument");
  if (p->functor == Functor::LQ) return fail(OCS_ERR_UNSUPPORTED, "compute_equilibrium: not instantiated for the LQ problem");
  if (p->functor == Functor::User && 2 * p->nS + p->nC > 24)
    return fail(OCS_ERR_UNSUPPORTED, "compute_equilibrium: at most 24 unknowns per instance");
  if (p->pmask && p->pb_batch != batch)
    return fail(OCS_ERR_SHAPE, "problem has per-trajectory parameters for batch %d, call has batch %d", p->pb_batch, batch);
  return OCS_OK;
}
int ocs_compute_equilibrium_dev(ocs_problem p, int batch, double r, const double* yGuess, const double* lb,
                                const double* ub, double* y, double* resnorm, double* residual, int* exitflag,
                                void* stream) {
  OCS_TRACE("ocs_compute_equilibrium_dev");
  if (!yGuess || !lb || !ub || !y || !resnorm || !exitflag) return fail(OCS_ERR_INVALID, "null argument");
  OCS_TRY(equilibrium_check(p, batch));
  OCS_TRY(upload_problem(p));
  // 4000 iterations is lsqnonlin's MaxIter in the reference (:24); the residual tolerance is round-off level
  LAUNCH_TRY(launch_equilibrium(describe(p), batch, r, yGuess, lb, ub, y, resnorm, residual, exitflag, 4000, 1e-15,
                                (hipStream_t)stream));
  return OCS_OK;
}
int ocs_compute_equilibrium(ocs_problem p, int batch, double r, const double* yGuess, const double* lb,
                            const double* ub, double* y, double* resnorm, double* residual, int* exitflag) {
  OCS_TRACE("ocs_compute_equilibrium");
  if (!yGuess || !lb || !ub || !y || !resnorm || !exitflag) return fail(OCS_ERR_INVALID, "null argument");
  OCS_TRY(equilibrium_check(p, batch));
  const int n = 2 * p->nS + p->nC;
  const size_t nb = (size_t)n * batch;
  DevBuf dg, dl, du, dy, dr, dres, df, dst;
  OCS_TRY(dst.ensure(sizeof(double) * nb));
  OCS_TRY(dg.ensure(sizeof(double) * nb));
  OCS_TRY(dy.ensure(sizeof(double) * nb));
  OCS_TRY(dres.ensure(sizeof(double) * nb));
  OCS_TRY(dl.ensure(sizeof(double) * n));
  OCS_TRY(du.ensure(sizeof(double) * n));
  OCS_TRY(dr.ensure(sizeof(double) * batch));
  OCS_TRY(df.ensure(sizeof(int) * batch));
  HIP_TRY(hipMemcpy(dst.p, yGuess, sizeof(double) * nb, hipMemcpyHostToDevice));
  LAUNCH_TRY(launch_to_batch_minor(dst.d(), dg.d(), n, batch, nullptr));
  HIP_TRY(hipMemcpy(dl.p, lb, sizeof(double) * n, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(du.p, ub, sizeof(double) * n, hipMemcpyHostToDevice));
  OCS_TRY(ocs_compute_equilibrium_dev(p, batch, r, dg.d(), dl.d(), du.d(), dy.d(), dr.d(), dres.d(), (int*)df.p, nullptr));
  OCS_TRY(stage_out(dst, dy.d(), y, n, batch, nullptr));
  if (residual) OCS_TRY(stage_out(dst, dres.d(), residual, n, batch, nullptr));
  HIP_TRY(hipMemcpy(resnorm, dr.p, sizeof(double) * batch, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(exitflag, df.p, sizeof(int) * batch, hipMemcpyDeviceToHost));
  for (int b = 0; b < batch; ++b)
    if (exitflag[b] < 0) return OCS_NUM_NONFINITE;   // (a numerical condition: the outputs of the other instances stand)
  return OCS_OK;
}

// ------------------------------------------------------------------------------------
// Integrator
// ------------------------------------------------------------------------------------
int ocs_rk4_create(ocs_integrator* out, const double* tspan, int npts) {
  if (!out || !tspan) return fail(OCS_ERR_INVALID, "null argument");
  *out = nullptr;
  if (npts < 2) return fail(OCS_ERR_SHAPE, "tspan needs at least 2 points");
  std::unique_ptr<ocs_integrator_s> g(new ocs_integrator_s());
  const int N = npts - 1;
  g->N = N;
  g->tspan.assign(tspan, tspan + npts);
  g->h.resize(N);
  g->t.resize(2 * (size_t)N + 1);
  for (int i = 0; i < N; ++i) g->h[i] = tspan[i + 1] - tspan[i];                  // RK4Integrator.m:17
  for (int i = 0; i <= N; ++i) g->t[2 * (size_t)i] = tspan[i];                    // :22
  for (int i = 0; i < N; ++i) g->t[2 * (size_t)i + 1] = (tspan[i] + tspan[i + 1]) / 2;  // :23
  for (int i = 0; i < N; ++i)
    if (!(g->h[i] > 0) || !std::isfinite(g->h[i])) return fail(OCS_ERR_INVALID, "tspan must be finite and strictly increasing");
  *out = g.release();
  return OCS_OK;
}

/* obj = RK4InfiniteIntegrator(tspan, tspanExtra, uStar)   Integrator/RK4InfiniteIntegrator.m:12-17 */
int ocs_rk4inf_create(ocs_integrator* out, const double* tspan, int npts, const double* tspanExtra,
                      int nptsExtra, const double* uStar, int nC) {
  if (!out || !tspan || !tspanExtra || !uStar) return fail(OCS_ERR_INVALID, "null argument");
  *out = nullptr;
  if (nC < 1) return fail(OCS_ERR_SHAPE, "uStar needs nC >= 1 entries");
  ocs_integrator g1 = nullptr, g2 = nullptr;
  OCS_TRY(ocs_rk4_create(&g1, tspan, npts));
  std::unique_ptr<ocs_integrator_s> leg1(g1);
  OCS_TRY(ocs_rk4_create(&g2, tspanExtra, nptsExtra));
  leg1->kind = 1;
  leg1->leg2 = g2;
  leg1->ustar.assign(uStar, uStar + nC);
  *out = leg1.release();
  return OCS_OK;
}

// which uStar the tail leg of (g, batch) runs under; refuses a batch other than the per-trajectory uStar's
static int tail_ustar(const ocs_integrator_s* g, int batch, const double** u, bool* per_traj) {
  if (g->ustar_batch && g->ustar_batch != batch)
    return fail(OCS_ERR_SHAPE, "integrator has a per-trajectory uStar for batch %d, call has batch %d", g->ustar_batch, batch);
  *per_traj = g->ustar_batch != 0;
  *u = *per_traj ? g->d_ustar_b.d() : g->d_ustar.d();
  return OCS_OK;
}
static int batch_ustar_check(ocs_integrator g, int batch) {
  if (!g) return fail(OCS_ERR_INVALID, "null integrator");
  if (g->kind != 1) return fail(OCS_ERR_INVALID, "a per-trajectory uStar needs an RK4InfiniteIntegrator");
  if (batch < 0) return fail(OCS_ERR_SHAPE, "batch must be >= 0");
  return OCS_OK;
}
// every set and clear: a new version, and the checkpoints of a state pass under the earlier uStar no longer serve an adjoint pass
static void batch_ustar_changed(ocs_integrator g) {
  g->ustar_batch = 0;
  g->ustar_version = next_version();
  g->ck = nullptr;
  g->leg2->ck = nullptr;
}
static int batch_ustar_clear(ocs_integrator g) {
  batch_ustar_changed(g);
  return OCS_OK;
}
int ocs_rk4inf_set_batch_ustar_dev(ocs_integrator g, int batch, const double* uStar, void* stream) {
  OCS_TRY(batch_ustar_check(g, batch));
  if (batch == 0 || !uStar) return batch_ustar_clear(g);
  OCS_TRY(upload_grid(g));
  const size_t bytes = sizeof(double) * g->ustar.size() * (size_t)batch;
  batch_ustar_changed(g);   // (and not set if the copy below fails)
  OCS_TRY(g->d_ustar_b.ensure(bytes));
  HIP_TRY(hipMemcpyAsync(g->d_ustar_b.p, uStar, bytes, hipMemcpyDeviceToDevice, (hipStream_t)stream));
  g->ustar_batch = batch;
  return OCS_OK;
}
int ocs_rk4inf_set_batch_ustar(ocs_integrator g, int batch, const double* uStar) {
  OCS_TRY(batch_ustar_check(g, batch));
  if (batch == 0 || !uStar) return batch_ustar_clear(g);
  OCS_TRY(upload_grid(g));
  batch_ustar_changed(g);
  HIP_TRY(hipStreamSynchronize(g->stream));   // (the stage buffer may be in use by a host call's copies)
  OCS_TRY(stage_in(g->d_stage, g->d_ustar_b, uStar, (int)g->ustar.size(), batch, g->stream));
  HIP_TRY(hipStreamSynchronize(g->stream));   // complete before a _dev call on any other stream
  g->ustar_batch = batch;
  return OCS_OK;
}

int ocs_integrator_destroy(ocs_integrator g) {
  delete g;   // (~ocs_integrator_s: event, tail leg, sweep and LQ workspaces, stream, then the buffers)
  return OCS_OK;
}
int ocs_integrator_set_mapping(ocs_integrator g, int mapping) {
  if (!g) return fail(OCS_ERR_INVALID, "null integrator");
  if (mapping < MAP_AUTO || mapping > MAP_SCAN) return fail(OCS_ERR_INVALID, "mapping must be 0..4");
  g->mapping = mapping;
  if (g->leg2) g->leg2->mapping = mapping;
  return OCS_OK;
}
int ocs_integrator_set_layout(ocs_integrator g, int layout) {
  if (!g) return fail(OCS_ERR_INVALID, "null integrator");
  if (layout != OCS_LAYOUT_BATCH_MINOR && layout != OCS_LAYOUT_TILED) return fail(OCS_ERR_INVALID, "layout must be 0 or 1");
  g->layout = layout;   // (what the tiled layout does not cover is refused at the compute call, as for set_mapping)
  return OCS_OK;
}
int ocs_integrator_layout(ocs_integrator g) { return g ? g->layout : fail(OCS_ERR_INVALID, "null integrator"); }
// what the tiled layout covers: the registry logistic family with 1, 2 or 4 states and shared parameters, on an RK4Integrator,
// in the automatic / pipeline / scan mappings (pipeline + scan at every batch, remainder steps on the lane kernels)
static int tiled_check(const ocs_integrator_s* g, const ocs_problem_s* p) {
  if (g->layout != LAYOUT_TILED) return OCS_OK;
  const char* why = nullptr;
  if (g->kind != 0) why = "RK4InfiniteIntegrator";
  else if (p->functor == Functor::LQ) why = "the LQ problem";
  else if (p->functor == Functor::User) why = "hipRTC plugin problems";
  else if (p->nS == 3) why = "nS = 3 (the wave-specialised kernels take 1, 2 or 4 states)";
  else if (p->pmask || p->has_w) why = "per-trajectory parameters";
  else if (g->mapping != MAP_AUTO && g->mapping != MAP_PIPELINE && g->mapping != MAP_SCAN)
    why = "the lane and row-split mappings (automatic, pipeline or scan only)";
  else if (!tiled_supported(describe(p))) why = "this problem";
  if (why) return fail(OCS_ERR_UNSUPPORTED, "tiled layout: not instantiated for %s", why);
  return OCS_OK;
}
int ocs_integrator_nsteps(ocs_integrator g, int* nsteps) {
  if (!g || !nsteps) return fail(OCS_ERR_INVALID, "null argument");
  *nsteps = g->N;
  return OCS_OK;
}
int ocs_integrator_t(ocs_integrator g, double* t) {
  if (!g || !t) return fail(OCS_ERR_INVALID, "null argument");
  memcpy(t, g->t.data(), sizeof(double) * g->t.size());
  return OCS_OK;
}
int ocs_integrator_h(ocs_integrator g, double* h) {
  if (!g || !h) return fail(OCS_ERR_INVALID, "null argument");
  memcpy(h, g->h.data(), sizeof(double) * g->h.size());
  return OCS_OK;
}

// one RK4 leg, forward.  ck receives the checkpoints (x itself when the caller wants x).
static int leg_forward(ocs_integrator_s* g, ocs_problem_s* p, int batch, const double* x0, const double* u,
                       double* x, double* J, const FwdOpts& o, hipStream_t s) {
  OCS_TRY(tiled_check(g, p));
  OCS_TRY(bind_problem(g, p, batch, s));
  const size_t ckdbl = g->layout == LAYOUT_TILED ? tiled_doubles_host((size_t)p->nS + 1, (size_t)g->N + 1, (size_t)batch)
                                                 : (size_t)(p->nS + 1) * (g->N + 1) * batch;
  double* ck = x;
  if (!ck && (g->kind == 1 || o.uconst || g->want_ck)) {
    // checkpoints go to handle-owned scratch so the adjoint pass can still run
    OCS_TRY(g->d_ck.ensure(sizeof(double) * ckdbl));
    ck = g->d_ck.d();
  }
  g->ck = nullptr;
  FwdOpts om = o;
  om.mapping = g->mapping;
  om.layout = g->layout;
  LAUNCH_TRY(launch_forward(describe(p), describe(g), batch, x0, u, ck, J, om, s));
  g->ck = ck;
  g->ck_batch = batch;
  g->ck_layout = g->layout;
  g->ck_prob = p;
  return OCS_OK;
}

int ocs_compute_states_dev(ocs_integrator g, ocs_problem p, int batch, const double* x0, const double* u,
                           double* x, double* J, void* stream) {
  OCS_TRACE("ocs_compute_states_dev");
  if (!g || !p || !x0 || !u || !J) return fail(OCS_ERR_INVALID, "null argument");
  if (batch < 1) return fail(OCS_ERR_SHAPE, "batch must be >= 1");
  hipStream_t s = (hipStream_t)stream;
  g->want_ck = true;
  if (g->kind == 0) return leg_forward(g, p, batch, x0, u, x, J, FwdOpts(), s);
  // RK4InfiniteIntegrator.m:20-24: [x,J1] = leg1(x0,u); [~,J2] = leg2(x(1:end-1,end), uStar); J = J1 + J2
  if ((int)g->ustar.size() != p->nC) return fail(OCS_ERR_SHAPE, "uStar has %d entries, problem has nC=%d",
                                                 (int)g->ustar.size(), p->nC);
  const double* us = nullptr;
  bool us_batch = false;
  OCS_TRY(upload_grid(g));   // (d_ustar exists from here on)
  OCS_TRY(tail_ustar(g, batch, &us, &us_batch));
  OCS_TRY(leg_forward(g, p, batch, x0, u, x, J, FwdOpts(), s));
  const double* xT = g->ck + (size_t)g->N * (p->nS + 1) * batch;  // x(1:nS, end): rows are contiguous [nS][B]
  ocs_integrator_s* g2 = g->leg2;
  OCS_TRY(g2->d_ck.ensure(sizeof(double) * (size_t)(p->nS + 1) * (g2->N + 1) * batch));
  // The tail leg has a constant control.  The lane kernels take it as a parameter and read nothing (the mapping for a full
  // chip); where the wave-specialised kernels would be chosen (small batches: the lane kernels are chain-bound, 650 against
  // 125 us for the tail at batch 4096) the tail runs on them, on SAMPLES of the constant control kept with the handle.
  OCS_TRY(bind_problem(g2, p, batch, s));
  g2->tail_wave = g2->mapping == MAP_AUTO && tail_leg_wave_ok(describe(p), describe(g2), batch);
  if (g2->tail_wave) {
    const size_t nU = (size_t)(2 * g2->N + 1) * p->nC * batch;
    OCS_TRY(g2->d_utail.ensure(sizeof(double) * nU));
    if (g2->utail_batch != batch || g2->utail_version != g->ustar_version) {
      LAUNCH_TRY(launch_fill_rows(2 * g2->N + 1, p->nC, batch, us, g2->d_utail.d(), s, us_batch));
      g2->utail_batch = batch;
      g2->utail_version = g->ustar_version;
    }
    OCS_TRY(g2->d_J2.ensure(sizeof(double) * (size_t)batch));
    OCS_TRY(leg_forward(g2, p, batch, xT, g2->d_utail.d(), g2->d_ck.d(), g2->d_J2.d(), FwdOpts(), s));
    LAUNCH_TRY(launch_add_vec(batch, J, g2->d_J2.d(), J, s));   // J = J1 + J2   :24
    return OCS_OK;
  }
  FwdOpts o2;
  o2.uconst = true;
  o2.uconst_batch = us_batch;
  o2.uversion = g->ustar_version;
  o2.Jadd = J;
  OCS_TRY(leg_forward(g2, p, batch, xT, us, g2->d_ck.d(), J, o2, s));
  return OCS_OK;
}

int ocs_compute_adjoints_dev(ocs_integrator g, ocs_problem p, int batch, const double* u, const double* lamT,
                             double* lam, double* dJdu, void* stream) {
  OCS_TRACE("ocs_compute_adjoints_dev");
  if (!g || !p || !u) return fail(OCS_ERR_INVALID, "null argument");
  if (!lam && !dJdu) return fail(OCS_ERR_INVALID, "at least one of lam, dJdu must be requested");
  if (!g->ck || g->ck_prob != p || g->ck_batch != batch || g->ck_layout != g->layout)
    return fail(OCS_ERR_ORDER, "compute_adjoints needs compute_states first on the same handle/problem/batch/layout");
  hipStream_t s = (hipStream_t)stream;
  OCS_TRY(tiled_check(g, p));
  OCS_TRY(bind_problem(g, p, batch, s));
  BwdOpts o;
  o.mapping = g->mapping;
  o.layout = g->layout;
  o.lam0 = g->want_lam0;
  if (!lam) {
    OCS_TRY(g->d_split.ensure(sizeof(double) * (size_t)(p->nS + 1) * batch));
    o.split_scratch = g->d_split.d();
  }
  if (g->kind == 1) {
    // RK4InfiniteIntegrator.m:27-30: lam2 = leg2.adjoints(uStar); [lam,dJdu] = leg1.adjoints(u, lam2(:,1))
    if (lamT) return fail(OCS_ERR_INVALID, "RK4InfiniteIntegrator.compute_adjoints takes no lamT");
    ocs_integrator_s* g2 = g->leg2;
    if (!g2->ck || g2->ck_prob != p || g2->ck_batch != batch)
      return fail(OCS_ERR_ORDER, "tail leg has no forward pass");
    OCS_TRY(bind_problem(g2, p, batch, s));
    OCS_TRY(g->d_lam2.ensure(sizeof(double) * (size_t)(p->nS + 1) * batch));
    const double* us = nullptr;
    bool us_batch = false;
    OCS_TRY(tail_ustar(g, batch, &us, &us_batch));
    if (g2->tail_wave && g2->utail_batch == batch && g2->utail_version == g->ustar_version) {   // (the state pass of the tail ran on the sampled control: so does this)
      OCS_TRY(g2->d_lamtail.ensure(sizeof(double) * (size_t)(g2->N + 1) * (p->nS + 1) * batch));
      BwdOpts o2;
      o2.mapping = g2->mapping;
      LAUNCH_TRY(launch_backward(describe(p), describe(g2), batch, g2->ck, g2->d_utail.d(), nullptr, g2->d_lamtail.d(),
                                 nullptr, o2, s));
      lamT = g2->d_lamtail.d();   // lam2(:, 1): the first column
    } else {
      BwdOpts o2;
      o2.mapping = g2->mapping;
      o2.uconst = true;
      o2.uconst_batch = us_batch;
      o2.lam0 = g->d_lam2.d();
      LAUNCH_TRY(launch_backward(describe(p), describe(g2), batch, g2->ck, us, nullptr, nullptr, nullptr,
                                 o2, s));
      lamT = g->d_lam2.d();
    }
  }
  LAUNCH_TRY(launch_backward(describe(p), describe(g), batch, g->ck, u, lamT, lam, dJdu, o, s));
  return OCS_OK;
}

int ocs_compute_states(ocs_integrator g, ocs_problem p, int batch, const double* x0, const double* u,
                       double* x, double* J) {
  OCS_TRACE("ocs_compute_states");
  if (!g || !p || !x0 || !u || !J) return fail(OCS_ERR_INVALID, "null argument");
  if (batch < 1) return fail(OCS_ERR_SHAPE, "batch must be >= 1");
  OCS_TRY(refuse_tiled(g, "ocs_compute_states (host arrays)"));
  OCS_TRY(upload_grid(g));
  const int nAug = p->nS + 1, nC = p->nC, N = g->N;
  HIP_TRY(hipStreamSynchronize(g->stream));
  OCS_TRY(stage_in(g->d_stage, g->d_x0, x0, p->nS, batch, g->stream));
  HIP_TRY(hipStreamSynchronize(g->stream));
  OCS_TRY(stage_in(g->d_stage, g->d_u, u, nC * (2 * N + 1), batch, g->stream));
  OCS_TRY(g->d_x.ensure(sizeof(double) * (size_t)nAug * (N + 1) * batch));
  OCS_TRY(g->d_J.ensure(sizeof(double) * batch));
  OCS_TRY(ocs_compute_states_dev(g, p, batch, g->d_x0.d(), g->d_u.d(), g->d_x.d(), g->d_J.d(), g->stream));
  HIP_TRY(hipMemcpyAsync(J, g->d_J.p, sizeof(double) * batch, hipMemcpyDeviceToHost, g->stream));
  if (x) {
    OCS_TRY(stage_out(g->d_stage, g->d_x.d(), x, nAug * (N + 1), batch, g->stream));
  } else {
    HIP_TRY(hipStreamSynchronize(g->stream));
  }
  g->traj_status.assign(batch, 0);
  int rc = OCS_OK;
  for (int b = 0; b < batch; ++b)
    if (!std::isfinite(J[b])) {
      g->traj_status[b] = OCS_NUM_NONFINITE;
      rc = OCS_NUM_NONFINITE;
    }
  return rc;
}

int ocs_integrator_trajectory_status(ocs_integrator g, int batch, int* status) {
  if (!g || !status) return fail(OCS_ERR_INVALID, "null argument");
  if ((int)g->traj_status.size() != batch)
    return fail(OCS_ERR_ORDER, "no host compute call with batch %d has run on this handle", batch);
  for (int b = 0; b < batch; ++b) status[b] = g->traj_status[b];
  return OCS_OK;
}
int ocs_trajectory_status_dev(int batch, const double* J, int* status, void* stream) {
  if (!J || !status || batch < 1) return fail(OCS_ERR_INVALID, "bad argument");
  OCS_TRY(require_device());
  LAUNCH_TRY(launch_traj_status(J, batch, status, (hipStream_t)stream));
  return OCS_OK;
}
int ocs_tracing_enabled(void) { return roctx_available() ? 1 : 0; }

int ocs_compute_adjoints(ocs_integrator g, ocs_problem p, int batch, const double* u, const double* lamT,
                         double* lam, double* dJdu) {
  OCS_TRACE("ocs_compute_adjoints");
  if (!g || !p || !u || !lam) return fail(OCS_ERR_INVALID, "null argument");
  OCS_TRY(refuse_tiled(g, "ocs_compute_adjoints (host arrays)"));
  if (!g->ck || g->ck != g->d_x.d() || g->ck_prob != p || g->ck_batch != batch)
    return fail(OCS_ERR_ORDER, "compute_adjoints needs compute_states first on the same handle/problem/batch");
  const int nAug = p->nS + 1, nC = p->nC, N = g->N;
  HIP_TRY(hipStreamSynchronize(g->stream));
  OCS_TRY(stage_in(g->d_stage, g->d_u, u, nC * (2 * N + 1), batch, g->stream));
  if (lamT) {
    HIP_TRY(hipStreamSynchronize(g->stream));
    OCS_TRY(stage_in(g->d_stage, g->d_lamT, lamT, nAug, batch, g->stream));
  }
  OCS_TRY(g->d_lam.ensure(sizeof(double) * (size_t)nAug * (N + 1) * batch));
  if (dJdu) OCS_TRY(g->d_dJdu.ensure(sizeof(double) * (size_t)nC * (2 * N + 1) * batch));
  OCS_TRY(ocs_compute_adjoints_dev(g, p, batch, g->d_u.d(), lamT ? g->d_lamT.d() : nullptr, g->d_lam.d(),
                                   dJdu ? g->d_dJdu.d() : nullptr, g->stream));
  OCS_TRY(stage_out(g->d_stage, g->d_lam.d(), lam, nAug * (N + 1), batch, g->stream));
  if (dJdu) OCS_TRY(stage_out(g->d_stage, g->d_dJdu.d(), dJdu, nC * (2 * N + 1), batch, g->stream));
  return OCS_OK;
}

int ocs_device_malloc(void** ptr, unsigned long bytes) {
  if (!ptr || bytes == 0) return fail(OCS_ERR_INVALID, "bad argument");
  OCS_TRY(require_device());
  *ptr = nullptr;
  HIP_TRY(hipMalloc(ptr, (size_t)bytes));
  return OCS_OK;
}
int ocs_device_free(void* ptr) {
  if (ptr) HIP_TRY(hipFree(ptr));
  return OCS_OK;
}
int ocs_device_upload(void* dst, const void* src, unsigned long bytes, void* stream) {
  if (!dst || !src) return fail(OCS_ERR_INVALID, "bad argument");
  OCS_TRY(require_device());
  if (stream) HIP_TRY(hipMemcpyAsync(dst, src, (size_t)bytes, hipMemcpyHostToDevice, (hipStream_t)stream));
  else HIP_TRY(hipMemcpy(dst, src, (size_t)bytes, hipMemcpyHostToDevice));
  return OCS_OK;
}
int ocs_device_download(void* dst, const void* src, unsigned long bytes, void* stream) {
  if (!dst || !src) return fail(OCS_ERR_INVALID, "bad argument");
  OCS_TRY(require_device());
  if (stream) HIP_TRY(hipMemcpyAsync(dst, src, (size_t)bytes, hipMemcpyDeviceToHost, (hipStream_t)stream));
  else HIP_TRY(hipMemcpy(dst, src, (size_t)bytes, hipMemcpyDeviceToHost));
  return OCS_OK;
}

int ocs_copy_dev(const double* src, double* dst, long n, void* stream) {
  if (!src || !dst || n < 1) return fail(OCS_ERR_INVALID, "bad argument");
  OCS_TRY(require_device());
  LAUNCH_TRY(launch_copy8(src, dst, (size_t)n, (hipStream_t)stream));
  return OCS_OK;
}
int ocs_to_batch_minor_dev(const double* src, double* dst, int per_traj, int batch, void* stream) {
  if (!src || !dst || per_traj < 1 || batch < 1) return fail(OCS_ERR_INVALID, "bad argument");
  OCS_TRY(require_device());
  LAUNCH_TRY(launch_to_batch_minor(src, dst, per_traj, batch, (hipStream_t)stream));
  return OCS_OK;
}
int ocs_to_tiled_dev(const double* src, double* dst, int rows, int cols, int batch, void* stream) {
  if (!src || !dst || rows < 1 || cols < 1 || batch < 1) return fail(OCS_ERR_INVALID, "bad argument");
  OCS_TRY(require_device());
  LAUNCH_TRY(launch_tiled_convert(true, src, dst, (size_t)rows * cols, batch, (hipStream_t)stream));
  return OCS_OK;
}
int ocs_from_tiled_dev(const double* src, double* dst, int rows, int cols, int batch, void* stream) {
  if (!src || !dst || rows < 1 || cols < 1 || batch < 1) return fail(OCS_ERR_INVALID, "bad argument");
  OCS_TRY(require_device());
  LAUNCH_TRY(launch_tiled_convert(false, src, dst, (size_t)rows * cols, batch, (hipStream_t)stream));
  return OCS_OK;
}
long ocs_tiled_doubles(int rows, int cols, int batch) {
  if (rows < 1 || cols < 1 || batch < 1) return fail(OCS_ERR_INVALID, "bad argument");
  return (long)tiled_doubles_host((size_t)rows, (size_t)cols, (size_t)batch);
}
int ocs_to_traj_major_dev(const double* src, double* dst, int per_traj, int batch, void* stream) {
  if (!src || !dst || per_traj < 1 || batch < 1) return fail(OCS_ERR_INVALID, "bad argument");
  OCS_TRY(require_device());
  LAUNCH_TRY(launch_to_traj_major(src, dst, per_traj, batch, (hipStream_t)stream));
  return OCS_OK;
}

}  // extern "C"
