// ocs_shooting.cpp -- batched direct single shooting on the device: B independent NLPs
//   min_v J_b(v),  Lb <= v <= Ub        (single_shooting.m:69-115; one per column of x0 / per parameter set)
// solved together.  The reference hands one problem to fmincon('sqp') (:114), a MATLAB toolbox; the outer iteration
// here is a spectral projected gradient (Birgin-Martinez-Raydan: Barzilai-Borwein step length, projection on the
// bounds of compute_nlp_bounds, non-monotone Armijo back-tracking) in which every instance keeps its own step
// length, line search and stopping test, and every objective / gradient evaluation is one call of the hot path
// (nlpObjective, :137-150) over the whole batch.  Iterates differ from fmincon's; the KKT point is the same.
// ocs_ss_options.algorithm = OCS_SS_LBFGS selects a second outer iteration with the same evaluations, stopping tests and
// outputs: a projected limited-memory BFGS per instance (two-loop recursion on the coefficients that are not held on a
// bound, monotone Armijo search along the projected path, SPG's direction while no pair is held); tests/lbfgs_twin.py
// states it step by step.
#include "ocs_trace.hpp"
#include "ocs_handles.hpp"

#include <initializer_list>
#include <limits>
#include <utility>
#include <vector>

using namespace ocs;

// `fields` = (pointer to set, rows): [rows][B] arrays laid side by side in one device buffer, in this order
template <class T>
static int carve(DevBuf& buf, size_t B, std::initializer_list<std::pair<T**, size_t>> fields) {
  size_t rows = 0;
  for (const auto& f : fields) rows += f.second;
  OCS_TRY(buf.ensure(sizeof(T) * rows * B));
  T* at = (T*)buf.p;
  for (const auto& f : fields) {
    *f.first = at;
    at += f.second * B;
  }
  return OCS_OK;
}

// The solve of both entry points.  per_instance false: Lb, Ub are HOST vectors [nV + nFree] shared by the batch; true: DEVICE
// arrays [nV + nFree][B], bounds of its own per instance.  Either may be NULL (unbounded).
static int shooting_solve(const char* what, ocs_integrator g, ocs_problem p, ocs_control c, int batch, double* x0, double* v,
                          int nFree, const int* FreeInitStates, const double* Lb, const double* Ub, bool per_instance,
                          const ocs_ss_options* opt, double* J, int* iterations, int* converged, double* pgnorm,
                          void* stream);

extern "C" {

int ocs_ss_default_options(ocs_ss_options* o) {
  if (!o) return fail(OCS_ERR_INVALID, "null argument");
  o->TolX = 1e-5;     // single_shooting.m:20
  o->TolFun = 3e-4;   // :21
  o->MaxIter = 500;
  o->memory = 10;
  o->maxBacktracks = 25;
  o->algorithm = OCS_SS_SPG;
  o->pairs = 8;
  return OCS_OK;
}

// device: x0 [nS][B] (overwritten at FreeInitStates, :146), v [nV+nFree][B] start -> solution; host: Lb, Ub
// [nV+nFree] or NULL (unbounded); outputs J [B], iterations int[B], converged int[B], pgnorm [B] (any may be NULL
// except J).  Returns OCS_NUM_NOT_CONVERGED if an instance did not reach 10 TolFun.
int ocs_single_shooting_batch_dev(ocs_integrator g, ocs_problem p, ocs_control c, int batch, double* x0, double* v,
                                  int nFree, const int* FreeInitStates, const double* Lb, const double* Ub,
                                  const ocs_ss_options* opt, double* J, int* iterations, int* converged,
                                  double* pgnorm, void* stream) {
  return shooting_solve("ocs_single_shooting_batch_dev", g, p, c, batch, x0, v, nFree, FreeInitStates, Lb, Ub, false, opt, J,
                        iterations, converged, pgnorm, stream);
}

// the same with bounds of its own per instance: Lb, Ub DEVICE arrays [nV+nFree][B], batch-minor, or NULL (unbounded)
int ocs_single_shooting_batch_bounds_dev(ocs_integrator g, ocs_problem p, ocs_control c, int batch, double* x0, double* v,
                                         int nFree, const int* FreeInitStates, const double* Lb, const double* Ub,
                                         const ocs_ss_options* opt, double* J, int* iterations, int* converged,
                                         double* pgnorm, void* stream) {
  return shooting_solve("ocs_single_shooting_batch_bounds_dev", g, p, c, batch, x0, v, nFree, FreeInitStates, Lb, Ub, true, opt,
                        J, iterations, converged, pgnorm, stream);
}

}  // extern "C"

static int shooting_solve(const char* what, ocs_integrator g, ocs_problem p, ocs_control c, int batch, double* x0, double* v,
                          int nFree, const int* FreeInitStates, const double* Lb, const double* Ub, bool per_instance,
                          const ocs_ss_options* opt, double* J, int* iterations, int* converged, double* pgnorm,
                          void* stream) {
  OCS_TRY(refuse_tiled(g, "ocs_single_shooting"));
  OCS_TRACE(what);
  if (!g || !p || !c || !x0 || !v || !opt || !J || batch < 1 || nFree < 0) return fail(OCS_ERR_INVALID, "bad argument");
  if (opt->MaxIter < 0 || opt->memory < 1 || opt->maxBacktracks < 1 || !(opt->TolFun > 0))
    return fail(OCS_ERR_INVALID, "bad options");
  if (opt->algorithm != OCS_SS_SPG && opt->algorithm != OCS_SS_LBFGS)
    return fail(OCS_ERR_INVALID, "algorithm %d: expected OCS_SS_SPG or OCS_SS_LBFGS", opt->algorithm);
  if (opt->algorithm == OCS_SS_LBFGS && (opt->pairs < 1 || opt->pairs > 16))
    return fail(OCS_ERR_INVALID, "pairs %d: expected 1..16", opt->pairs);
  hipStream_t s = (hipStream_t)stream;
  int nB = 0, nC = 0, nT = 0;
  OCS_TRY(ocs_control_dims(c, &nB, &nC, &nT));
  const int nV = nB * nC + nFree;
  const size_t B = (size_t)batch, vb = sizeof(double) * (size_t)nV * B;
  DevBuf gbuf, dbuf, vtbuf, gtbuf, sc, hist, flags, lbub, counter, conv, ring, coef, lflags;
  OCS_TRY(gbuf.ensure(vb));
  OCS_TRY(dbuf.ensure(vb));
  OCS_TRY(vtbuf.ensure(vb));
  OCS_TRY(gtbuf.ensure(vb));
  OCS_TRY(hist.ensure(sizeof(double) * (size_t)opt->memory * B));
  OCS_TRY(lbub.ensure(sizeof(double) * 2 * (size_t)nV * (per_instance ? B : 1)));
  OCS_TRY(counter.ensure(sizeof(int)));
  OCS_TRY(conv.ensure(sizeof(int) * B));
  if (per_instance) {   // the same refusal, counted on the device
    int bad = 0;
    HIP_TRY(hipMemsetAsync(counter.p, 0, sizeof(int), s));
    LAUNCH_TRY(launch_ss_bounds(nV, batch, Lb, Ub, lbub.d(), lbub.d() + (size_t)nV * B, (int*)counter.p, s));
    HIP_TRY(hipMemcpyAsync(&bad, counter.p, sizeof(int), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    if (bad) return fail(OCS_ERR_INVALID, "Lb > Ub at %d coefficient(s) of the per-instance bounds", bad);
  } else {
    std::vector<double> h(2 * (size_t)nV);
    const double inf = std::numeric_limits<double>::infinity();
    for (int i = 0; i < nV; ++i) {
      h[i] = Lb ? Lb[i] : -inf;
      h[nV + i] = Ub ? Ub[i] : inf;
      if (!(h[i] <= h[nV + i])) return fail(OCS_ERR_INVALID, "Lb > Ub at coefficient %d", i);
    }
    HIP_TRY(hipMemcpyAsync(lbub.p, h.data(), sizeof(double) * h.size(), hipMemcpyHostToDevice, s));
    HIP_TRY(hipStreamSynchronize(s));
  }
  ShootingArgs r = {};
  LbfgsArgs& l = r.l;
  SpgArgs& a = l.a;
  r.algorithm = opt->algorithm;
  r.pgnorm = pgnorm;
  r.converged = (int*)conv.p;
  a.batch = batch;
  a.nV = nV;
  a.memory = opt->memory;
  a.TolFun = opt->TolFun;
  a.TolX = opt->TolX;
  a.lb = lbub.d();
  a.ub = lbub.d() + (size_t)nV * (per_instance ? B : 1);
  a.bstride = per_instance ? batch : 0;
  a.v = v;
  a.g = gbuf.d();
  a.d = dbuf.d();
  a.vt = vtbuf.d();
  a.gt = gtbuf.d();
  a.J = J;
  a.hist = hist.d();
  a.counter = (int*)counter.p;
  OCS_TRY(carve<double>(sc, B, {{&a.Jt, 1}, {&a.alpha, 1}, {&a.lam, 1}, {&a.gtd, 1}, {&a.fmax, 1}}));
  OCS_TRY(carve<int>(flags, B, {{&a.active, 1}, {&a.accepted, 1}, {&a.iters, 1}}));
  if (opt->algorithm == OCS_SS_LBFGS) {  // the ring of (s, y) pairs of every instance, empty at the start
    const size_t m = (size_t)opt->pairs;
    l.pairs = opt->pairs;
    OCS_TRY(carve<double>(ring, B, {{&l.S, m * nV}, {&l.Y, m * nV}}));
    OCS_TRY(carve<double>(coef, B, {{&l.rho, m}, {&l.al, m}}));
    OCS_TRY(carve<int>(lflags, B, {{&l.head, 1}, {&l.count, 1}, {&l.qn, 1}, {&l.fr, (size_t)nV}}));
    HIP_TRY(hipMemsetAsync(l.head, 0, sizeof(int) * (size_t)(l.fr - l.head), s));  // head, count, qn
  }
  auto launch = [&](SsPhase phase) -> int {
    LAUNCH_TRY(launch_shooting(phase, r, s));
    return OCS_OK;
  };
  auto count_after = [&](SsPhase phase, int* n) -> int {  // the instances the phase counted (SpgArgs.counter)
    HIP_TRY(hipMemsetAsync(counter.p, 0, sizeof(int), s));
    OCS_TRY(launch(phase));
    HIP_TRY(hipMemcpyAsync(n, counter.p, sizeof(int), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    return OCS_OK;
  };
  OCS_TRY(ocs_nlp_objective_dev(g, p, c, batch, x0, v, nFree, FreeInitStates, J, a.g, stream));
  OCS_TRY(launch(SsPhase::Init));
  for (r.it = 0; r.it < opt->MaxIter; ++r.it) {
    int nactive = 0;
    OCS_TRY(count_after(SsPhase::Direction, &nactive));
    if (nactive == 0) break;
    for (int ls = 0; ls < opt->maxBacktracks; ++ls) {
      OCS_TRY(ocs_nlp_objective_dev(g, p, c, batch, x0, a.vt, nFree, FreeInitStates, a.Jt, a.gt, stream));
      int nrejected = 0;
      OCS_TRY(count_after(SsPhase::Accept, &nrejected));
      if (nrejected == 0) break;
    }
    OCS_TRY(launch(SsPhase::Update));
  }
  // x0 at FreeInitStates follows the last evaluated trial point: make it (and J, g) those of the returned v
  if (nFree > 0) OCS_TRY(ocs_nlp_objective_dev(g, p, c, batch, x0, v, nFree, FreeInitStates, J, a.g, stream));
  OCS_TRY(launch(SsPhase::Finish));
  std::vector<int> hc(B);
  HIP_TRY(hipMemcpyAsync(hc.data(), conv.p, sizeof(int) * B, hipMemcpyDeviceToHost, s));
  if (converged) HIP_TRY(hipMemcpyAsync(converged, conv.p, sizeof(int) * B, hipMemcpyDeviceToDevice, s));
  if (iterations) HIP_TRY(hipMemcpyAsync(iterations, a.iters, sizeof(int) * B, hipMemcpyDeviceToDevice, s));
  HIP_TRY(hipStreamSynchronize(s));
  for (size_t b = 0; b < B; ++b)
    if (!hc[b]) return OCS_NUM_NOT_CONVERGED;
  return OCS_OK;
}
