// ocs_shooting_kernels.hip -- per-instance bookkeeping of the batched single-shooting driver (ocs_shooting.cpp):
// spectral projected gradient on  min_v J_b(v), Lb <= v <= Ub  for B independent instances.  The objective and its
// gradient come from the hot path (nlpObjective, single_shooting.m:137-150); these kernels are the outer iteration
// that fmincon('sqp') performs in the reference (single_shooting.m:114), one thread per instance, every array
// [rows][B] so that a wave reads consecutive instances.
#include "ocs_device_common.hpp"
#include "ocs_internal.hpp"
#include "../../include/ocs.h"

namespace ocs {

// ---- the pieces both algorithms are made of, each over (args, instance b), every loop row after row

// projection of coefficient i of instance b on its bounds (shared, or the instance's own: SpgArgs::bstride)
__device__ static inline double proj(const SpgArgs& a, int i, int b, double w) {
  return fmin(fmax(w, bound_at(a.lb, i, a.bstride, b)), bound_at(a.ub, i, a.bstride, b));
}

// ||P(v - g) - v||_inf
__device__ static inline double pg_norm(const SpgArgs& a, int b) {
  const size_t B = (size_t)a.batch;
  double pgn = 0.0;
  for (int i = 0; i < a.nV; ++i) {
    const double v = a.v[i * B + b], g = a.g[i * B + b];
    pgn = fmax(pgn, fabs(proj(a, i, b, v - g) - v));
  }
  return pgn;
}

// stopping test: whether the instance goes on (a NaN norm stops it too)
__device__ static inline bool goes_on(const SpgArgs& a, int b) {
  const size_t B = (size_t)a.batch;
  int act = a.active[b];
  if (act) {
    if (!(pg_norm(a, b) > a.TolFun)) act = 0;
    a.active[b] = act;
  }
  if (!act) {  // finished: its trial point stays its solution, so that the batch evaluation leaves it alone
    a.accepted[b] = 1;
    for (int i = 0; i < a.nV; ++i) a.vt[i * B + b] = a.v[i * B + b];
  }
  return act;
}

// SPG's direction d = P(v - alpha g) - v with its first trial point; returns g'd.  SPG takes vt = P(v + d): v + (lb - v)
// can round to one ulp outside the box.  L-BFGS (on_bound) takes the projection itself, so that a coefficient that
// reaches a bound is on it exactly (its active set tests equality)
__device__ static inline double spg_direction(const SpgArgs& a, int b, bool on_bound) {
  const size_t B = (size_t)a.batch;
  const double alpha = a.alpha[b];
  double gtd = 0.0;
  for (int i = 0; i < a.nV; ++i) {
    const double v = a.v[i * B + b], g = a.g[i * B + b], w = proj(a, i, b, v - alpha * g);
    const double d = w - v;
    a.d[i * B + b] = d;
    a.vt[i * B + b] = on_bound ? w : proj(a, i, b, v + d);
    gtd += g * d;
  }
  return gtd;
}

// a rejected trial point: half the step, vt = P(v + lam d)
__device__ static inline void halve_step(const SpgArgs& a, int b) {
  const size_t B = (size_t)a.batch;
  const double half = 0.5 * a.lam[b];
  a.lam[b] = half;
  for (int i = 0; i < a.nV; ++i) a.vt[i * B + b] = proj(a, i, b, a.v[i * B + b] + half * a.d[i * B + b]);
}

// the accepted step: one pass over s = vt - v, y = gt - g with s'y, s's and max |s|; `row(i, s, y)` is what the algorithm
// adds to a row; with `take` the pass moves v, g to the accepted point
struct StepSums { double sty, sts, smax; };
template <class Row>
__device__ static inline StepSums step_rows(const SpgArgs& a, int b, bool take, Row row) {
  const size_t B = (size_t)a.batch;
  StepSums r = {0.0, 0.0, 0.0};
  for (int i = 0; i < a.nV; ++i) {
    const double vn = a.vt[i * B + b], gn = a.gt[i * B + b];
    const double s = vn - a.v[i * B + b], y = gn - a.g[i * B + b];
    r.sty += s * y;
    r.sts += s * s;
    r.smax = fmax(r.smax, fabs(s));
    row(i, s, y);
    if (take) {
      a.v[i * B + b] = vn;
      a.g[i * B + b] = gn;
    }
  }
  return r;
}
// and what follows it: the objective, the Barzilai-Borwein step length of the next iteration, the stop on a small step
__device__ static inline void step_taken(const SpgArgs& a, int b, const StepSums& r) {
  a.J[b] = a.Jt[b];
  const double an = r.sty > 0.0 ? r.sts / fmax(r.sty, 1e-300) : 1e3;
  a.alpha[b] = fmin(fmax(an, 1e-10), 1e10);
  if (r.smax <= a.TolX) a.active[b] = 0;
}

// ---- spectral projected gradient

// first evaluation done: step length 1 / ||P(v - g) - v||_inf, objective history filled with J
__global__ __launch_bounds__(256) void k_spg_init(SpgArgs a) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= a.batch) return;
  const size_t B = (size_t)a.batch;
  a.alpha[b] = 1.0 / fmax(pg_norm(a, b), 1e-12);
  for (int m = 0; m < a.memory; ++m) a.hist[m * B + b] = a.J[b];
  a.active[b] = 1;
  a.iters[b] = 0;
}

// stopping test, search direction, g'd, the non-monotone reference value, first trial point
__global__ __launch_bounds__(256) void k_spg_direction(SpgArgs a) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= a.batch || !goes_on(a, b)) return;
  const size_t B = (size_t)a.batch;
  const double gtd = spg_direction(a, b, false);
  double fmx = a.hist[b];
  for (int m = 1; m < a.memory; ++m) fmx = fmax(fmx, a.hist[m * B + b]);
  a.gtd[b] = gtd;
  a.fmax[b] = fmx;
  a.lam[b] = 1.0;
  a.accepted[b] = 0;
  atomicAdd(a.counter, 1);
}

// Armijo test of the trial point against the non-monotone reference; a rejected instance halves its step and gets
// its next trial point
__global__ __launch_bounds__(256) void k_spg_accept(SpgArgs a) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= a.batch || a.accepted[b]) return;
  if (a.Jt[b] <= a.fmax[b] + 1e-4 * a.lam[b] * a.gtd[b]) {
    a.accepted[b] = 2;  // accepted in this iteration
    return;
  }
  halve_step(a, b);
  atomicAdd(a.counter, 1);
}

// take the accepted point (a failed line search stops the instance where it is), history slot of iteration it
__global__ __launch_bounds__(256) void k_spg_update(SpgArgs a, int it) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= a.batch) return;
  const size_t B = (size_t)a.batch;
  if (a.active[b]) {
    a.iters[b] += 1;
    if (a.accepted[b] == 2) step_taken(a, b, step_rows(a, b, true, [](int, double, double) {}));
    else a.active[b] = 0;
  }
  a.hist[(size_t)(it % a.memory) * B + b] = a.J[b];
}

// ||P(v - g) - v||_inf of the result and the verdict (both algorithms)
__global__ __launch_bounds__(256) void k_spg_finish(SpgArgs a, double* pgnorm, int* converged) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= a.batch) return;
  const double pgn = pg_norm(a, b);
  if (pgnorm) pgnorm[b] = pgn;
  if (converged) converged[b] = pgn <= 10.0 * a.TolFun;
}

// ---- projected L-BFGS (ocs_ss_options.algorithm = OCS_SS_LBFGS): the same phases, one fused launch each; init and
// verdict are SPG's.  The iteration is specified statement by statement in tests/lbfgs_twin.py.

// slot of the j-th newest pair in the ring (j = 0 the newest)
__device__ static inline int lbfgs_slot(int head, int pairs, int j) { return (head + pairs - 1 - j) % pairs; }

// g'(vt - v) of the current trial point
__device__ static inline double lbfgs_gts(const SpgArgs& a, int b) {
  const size_t B = (size_t)a.batch;
  double gts = 0.0;
  for (int i = 0; i < a.nV; ++i) gts += a.g[i * B + b] * (a.vt[i * B + b] - a.v[i * B + b]);
  return gts;
}

// stopping test, active set, two-loop recursion on the free coefficients (SPG's direction while no pair is held or when
// the safeguard drops the pairs), first trial point and its g'(vt - v)
__global__ __launch_bounds__(256) void k_lbfgs_direction(LbfgsArgs l) {
  const SpgArgs& a = l.a;
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= a.batch || !goes_on(a, b)) return;
  const size_t B = (size_t)a.batch, nVB = (size_t)a.nV * B;
  const int pairs = l.pairs, head = l.head[b];
  int cnt = l.count[b];
  int qn = cnt > 0;
  if (qn) {
    // q = g on the free coefficients (kept in d), 0 on the active set
    for (int i = 0; i < a.nV; ++i) {
      const double v = a.v[i * B + b], g = a.g[i * B + b];
      const int fr = !((v == bound_at(a.lb, i, a.bstride, b) && g > 0.0) || (v == bound_at(a.ub, i, a.bstride, b) && g < 0.0));
      l.fr[i * B + b] = fr;
      a.d[i * B + b] = fr ? g : 0.0;
    }
    for (int j = 0; j < cnt; ++j) {
      const size_t o = (size_t)lbfgs_slot(head, pairs, j);
      const double *S = l.S + o * nVB, *Y = l.Y + o * nVB;
      double sq = 0.0;
      for (int i = 0; i < a.nV; ++i) sq += l.fr[i * B + b] ? S[i * B + b] * a.d[i * B + b] : 0.0;
      const double al = l.rho[o * B + b] * sq;
      l.al[(size_t)j * B + b] = al;
      for (int i = 0; i < a.nV; ++i)
        if (l.fr[i * B + b]) a.d[i * B + b] = a.d[i * B + b] - al * Y[i * B + b];
    }
    {
      const size_t o = (size_t)lbfgs_slot(head, pairs, 0);
      const double *S = l.S + o * nVB, *Y = l.Y + o * nVB;
      double sy = 0.0, yy = 0.0;
      for (int i = 0; i < a.nV; ++i) sy += l.fr[i * B + b] ? S[i * B + b] * Y[i * B + b] : 0.0;
      for (int i = 0; i < a.nV; ++i) yy += l.fr[i * B + b] ? Y[i * B + b] * Y[i * B + b] : 0.0;
      const double gamma = sy / yy;
      for (int i = 0; i < a.nV; ++i) a.d[i * B + b] = gamma * a.d[i * B + b];
    }
    for (int j = cnt - 1; j >= 0; --j) {
      const size_t o = (size_t)lbfgs_slot(head, pairs, j);
      const double *S = l.S + o * nVB, *Y = l.Y + o * nVB;
      double yr = 0.0;
      for (int i = 0; i < a.nV; ++i) yr += l.fr[i * B + b] ? Y[i * B + b] * a.d[i * B + b] : 0.0;
      const double c = l.al[(size_t)j * B + b] - l.rho[o * B + b] * yr;
      for (int i = 0; i < a.nV; ++i)
        if (l.fr[i * B + b]) a.d[i * B + b] = a.d[i * B + b] + S[i * B + b] * c;
    }
    double gtd = 0.0;
    for (int i = 0; i < a.nV; ++i) {
      const double d = l.fr[i * B + b] ? -a.d[i * B + b] : 0.0;
      a.d[i * B + b] = d;
      gtd += a.g[i * B + b] * d;
    }
    if (gtd < 0.0 && gtd >= -1.7976931348623157e308) {
      for (int i = 0; i < a.nV; ++i) a.vt[i * B + b] = proj(a, i, b, a.v[i * B + b] + a.d[i * B + b]);
    } else {  // not a finite descent direction: drop the pairs
      qn = 0;
      l.count[b] = 0;
    }
  }
  if (!qn) spg_direction(a, b, true);
  l.qn[b] = qn;
  a.gtd[b] = lbfgs_gts(a, b);
  a.lam[b] = 1.0;
  a.accepted[b] = 0;
  atomicAdd(a.counter, 1);
}

// monotone Armijo test on the projected displacement; a rejected instance halves its step along the projected path
__global__ __launch_bounds__(256) void k_lbfgs_accept(LbfgsArgs l) {
  const SpgArgs& a = l.a;
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= a.batch || a.accepted[b]) return;
  const double gts = a.gtd[b];
  if (gts < 0.0 && a.Jt[b] <= a.J[b] + 1e-4 * gts) {
    a.accepted[b] = 2;  // accepted in this iteration
    return;
  }
  halve_step(a, b);
  a.gtd[b] = lbfgs_gts(a, b);
  atomicAdd(a.counter, 1);
}

// take the accepted point and store the pair if s'y > 2.2e-16 y'y; a line search that failed on a quasi-Newton direction
// drops the pairs and goes on, one that failed on SPG's direction stops.  Two passes of step_rows: slot `head` may hold
// the oldest pair, which stays in use unless the sums of the whole step let the new one in
__global__ __launch_bounds__(256) void k_lbfgs_update(LbfgsArgs l) {
  const SpgArgs& a = l.a;
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= a.batch || !a.active[b]) return;
  const size_t B = (size_t)a.batch, nVB = (size_t)a.nV * B;
  a.iters[b] += 1;
  if (a.accepted[b] != 2) {
    if (l.qn[b]) l.count[b] = 0;
    else a.active[b] = 0;
    return;
  }
  double yty = 0.0;
  const StepSums r = step_rows(a, b, false, [&](int, double, double y) { yty += y * y; });
  const int store = r.sty > 2.2e-16 * yty, head = l.head[b];
  double *S = l.S + (size_t)head * nVB, *Y = l.Y + (size_t)head * nVB;
  step_rows(a, b, true, [&](int i, double s, double y) {
    if (store) {
      S[i * B + b] = s;
      Y[i * B + b] = y;
    }
  });
  if (store) {
    l.rho[(size_t)head * B + b] = 1.0 / r.sty;
    l.head[b] = (head + 1) % l.pairs;
    l.count[b] = min(l.count[b] + 1, l.pairs);
  }
  step_taken(a, b, r);
}

// Lb / Ub of a solve with bounds per instance: copies them into the driver's own arrays (a NULL side: unbounded) and counts the
// entries with Lb > Ub (or NaN) into *bad, which refuses the solve
__global__ __launch_bounds__(256) void k_ss_bounds(size_t n, const double* __restrict__ Lb, const double* __restrict__ Ub,
                                                   double* __restrict__ lb, double* __restrict__ ub, int* __restrict__ bad) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const double lo = Lb ? Lb[i] : -__builtin_inf(), hi = Ub ? Ub[i] : __builtin_inf();
  lb[i] = lo;
  ub[i] = hi;
  if (!(lo <= hi)) atomicAdd(bad, 1);
}
int launch_ss_bounds(int nV, int batch, const double* Lb, const double* Ub, double* lb, double* ub, int* bad, hipStream_t s) {
  const size_t n = (size_t)nV * batch;
  k_ss_bounds<<<dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s>>>(n, Lb, Ub, lb, ub, bad);
  return hip_rc(hipGetLastError());
}

int launch_shooting(SsPhase phase, const ShootingArgs& r, hipStream_t s) {
  const LbfgsArgs& l = r.l;
  const SpgArgs& a = l.a;
  const dim3 grid((a.batch + 255) / 256), block(256);
  const bool lbfgs = r.algorithm == OCS_SS_LBFGS;
  switch (phase) {
    case SsPhase::Init: k_spg_init<<<grid, block, 0, s>>>(a); break;
    case SsPhase::Direction:
      if (lbfgs) k_lbfgs_direction<<<grid, block, 0, s>>>(l);
      else k_spg_direction<<<grid, block, 0, s>>>(a);
      break;
    case SsPhase::Accept:
      if (lbfgs) k_lbfgs_accept<<<grid, block, 0, s>>>(l);
      else k_spg_accept<<<grid, block, 0, s>>>(a);
      break;
    case SsPhase::Update:
      if (lbfgs) k_lbfgs_update<<<grid, block, 0, s>>>(l);
      else k_spg_update<<<grid, block, 0, s>>>(a, r.it);
      break;
    case SsPhase::Finish: k_spg_finish<<<grid, block, 0, s>>>(a, r.pgnorm, r.converged); break;
  }
  return hip_rc(hipGetLastError());
}

}  // namespace ocs
