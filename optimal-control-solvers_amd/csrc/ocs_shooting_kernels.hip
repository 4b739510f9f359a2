// ocs_shooting_kernels.hip -- per-instance bookkeeping of the batched single-shooting driver (ocs_shooting.cpp):
// spectral projected gradient on  min_v J_b(v), Lb <= v <= Ub  for B independent instances.  The objective and its
// gradient come from the hot path (nlpObjective, single_shooting.m:137-150); these kernels are the outer iteration
// that fmincon('sqp') performs in the reference (single_shooting.m:114), one thread per instance, every array
// [rows][B] so that a wave reads consecutive instances.
#include "ocs_device_common.hpp"
#include "ocs_internal.hpp"

namespace ocs {


__device__ static inline double spg_proj(double w, double lb, double ub) { return fmin(fmax(w, lb), ub); }

// first evaluation done: step length 1 / ||P(v - g) - v||_inf, objective history filled with J
__global__ __launch_bounds__(256) void k_spg_init(SpgArgs a) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= a.batch) return;
  const size_t B = (size_t)a.batch;
  double pgn = 0.0;
  for (int i = 0; i < a.nV; ++i) {
    const double v = a.v[i * B + b], g = a.g[i * B + b];
    pgn = fmax(pgn, fabs(spg_proj(v - g, a.lb[i], a.ub[i]) - v));
  }
  a.alpha[b] = 1.0 / fmax(pgn, 1e-12);
  for (int m = 0; m < a.memory; ++m) a.hist[m * B + b] = a.J[b];
  a.active[b] = 1;
  a.iters[b] = 0;
}

// stopping test, search direction d = P(v - alpha g) - v, g'd, the non-monotone reference value, first trial point
__global__ __launch_bounds__(256) void k_spg_direction(SpgArgs a) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= a.batch) return;
  const size_t B = (size_t)a.batch;
  int act = a.active[b];
  if (act) {
    double pgn = 0.0;
    for (int i = 0; i < a.nV; ++i) {
      const double v = a.v[i * B + b], g = a.g[i * B + b];
      pgn = fmax(pgn, fabs(spg_proj(v - g, a.lb[i], a.ub[i]) - v));
    }
    if (!(pgn > a.TolFun)) act = 0;
    a.active[b] = act;
  }
  if (!act) {  // finished: its trial point stays its solution, so that the batch evaluation leaves it alone
    a.accepted[b] = 1;
    for (int i = 0; i < a.nV; ++i) a.vt[i * B + b] = a.v[i * B + b];
    return;
  }
  const double alpha = a.alpha[b];
  double gtd = 0.0;
  for (int i = 0; i < a.nV; ++i) {
    const double v = a.v[i * B + b], g = a.g[i * B + b];
    const double d = spg_proj(v - alpha * g, a.lb[i], a.ub[i]) - v;
    a.d[i * B + b] = d;
    a.vt[i * B + b] = spg_proj(v + d, a.lb[i], a.ub[i]);  // v + (lb - v) can round to one ulp outside the box
    gtd += g * d;
  }
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
  const size_t B = (size_t)a.batch;
  const double lam = a.lam[b];
  if (a.Jt[b] <= a.fmax[b] + 1e-4 * lam * a.gtd[b]) {
    a.accepted[b] = 2;  // accepted in this iteration
    return;
  }
  const double half = 0.5 * lam;
  a.lam[b] = half;
  for (int i = 0; i < a.nV; ++i) a.vt[i * B + b] = spg_proj(a.v[i * B + b] + half * a.d[i * B + b], a.lb[i], a.ub[i]);
  atomicAdd(a.counter, 1);
}

// take the accepted point, Barzilai-Borwein step length for the next iteration, history, stopping on a small step
__global__ __launch_bounds__(256) void k_spg_update(SpgArgs a, int it) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= a.batch) return;
  const size_t B = (size_t)a.batch;
  if (a.active[b]) {
    a.iters[b] += 1;
    if (a.accepted[b] == 2) {
      double sty = 0.0, sts = 0.0, smax = 0.0;
      for (int i = 0; i < a.nV; ++i) {
        const double vn = a.vt[i * B + b], gn = a.gt[i * B + b];
        const double s = vn - a.v[i * B + b], y = gn - a.g[i * B + b];
        sty += s * y;
        sts += s * s;
        smax = fmax(smax, fabs(s));
        a.v[i * B + b] = vn;
        a.g[i * B + b] = gn;
      }
      a.J[b] = a.Jt[b];
      const double an = sty > 0.0 ? sts / fmax(sty, 1e-300) : 1e3;
      a.alpha[b] = fmin(fmax(an, 1e-10), 1e10);
      if (smax <= a.TolX) a.active[b] = 0;
    } else {
      a.active[b] = 0;  // the line search failed: the instance stops where it is
    }
  }
  a.hist[(size_t)(it % a.memory) * B + b] = a.J[b];
}

// ||P(v - g) - v||_inf of the result and the verdict
__global__ __launch_bounds__(256) void k_spg_finish(SpgArgs a, double* pgnorm, int* converged) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= a.batch) return;
  const size_t B = (size_t)a.batch;
  double pgn = 0.0;
  for (int i = 0; i < a.nV; ++i) {
    const double v = a.v[i * B + b], g = a.g[i * B + b];
    pgn = fmax(pgn, fabs(spg_proj(v - g, a.lb[i], a.ub[i]) - v));
  }
  if (pgnorm) pgnorm[b] = pgn;
  if (converged) converged[b] = pgn <= 10.0 * a.TolFun;
}

int launch_spg(int which, const SpgArgs& a, int it, double* pgnorm, int* converged, hipStream_t s) {
  const dim3 grid((a.batch + 255) / 256), block(256);
  switch (which) {
    case 0: k_spg_init<<<grid, block, 0, s>>>(a); break;
    case 1: k_spg_direction<<<grid, block, 0, s>>>(a); break;
    case 2: k_spg_accept<<<grid, block, 0, s>>>(a); break;
    case 3: k_spg_update<<<grid, block, 0, s>>>(a, it); break;
    case 4: k_spg_finish<<<grid, block, 0, s>>>(a, pgnorm, converged); break;
    default: return -1;
  }
  return hip_rc(hipGetLastError());
}

// ---- projected L-BFGS (ocs_ss_options.algorithm = OCS_SS_LBFGS): the same phases as SPG, one fused launch each.
// k_spg_init and k_spg_finish are shared; the iteration is specified statement by statement in tests/lbfgs_twin.py.

// slot of the j-th newest pair in the ring (j = 0 the newest)
__device__ static inline int lbfgs_slot(int head, int pairs, int j) { return (head + pairs - 1 - j) % pairs; }

// g'(vt - v) of the current trial point, row after row
__device__ static inline double lbfgs_gts(const LbfgsArgs& l, int b) {
  const SpgArgs& a = l.a;
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
  if (b >= a.batch) return;
  const size_t B = (size_t)a.batch, nVB = (size_t)a.nV * B;
  int act = a.active[b];
  if (act) {
    double pgn = 0.0;
    for (int i = 0; i < a.nV; ++i) {
      const double v = a.v[i * B + b], g = a.g[i * B + b];
      pgn = fmax(pgn, fabs(spg_proj(v - g, a.lb[i], a.ub[i]) - v));
    }
    if (!(pgn > a.TolFun)) act = 0;
    a.active[b] = act;
  }
  if (!act) {  // finished: its trial point stays its solution, so that the batch evaluation leaves it alone
    a.accepted[b] = 1;
    for (int i = 0; i < a.nV; ++i) a.vt[i * B + b] = a.v[i * B + b];
    return;
  }
  const int pairs = l.pairs, head = l.head[b];
  int cnt = l.count[b];
  int qn = cnt > 0;
  if (qn) {
    // q = g on the free coefficients (kept in d), 0 on the active set
    for (int i = 0; i < a.nV; ++i) {
      const double v = a.v[i * B + b], g = a.g[i * B + b];
      const int fr = !((v == a.lb[i] && g > 0.0) || (v == a.ub[i] && g < 0.0));
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
      for (int i = 0; i < a.nV; ++i) a.vt[i * B + b] = spg_proj(a.v[i * B + b] + a.d[i * B + b], a.lb[i], a.ub[i]);
    } else {  // not a finite descent direction: drop the pairs
      qn = 0;
      l.count[b] = 0;
    }
  }
  if (!qn) {  // the trial point is the projection itself: a coefficient that reaches a bound is on it exactly
    const double alpha = a.alpha[b];
    for (int i = 0; i < a.nV; ++i) {
      const double v = a.v[i * B + b], w = spg_proj(v - alpha * a.g[i * B + b], a.lb[i], a.ub[i]);
      a.d[i * B + b] = w - v;
      a.vt[i * B + b] = w;
    }
  }
  l.qn[b] = qn;
  a.gtd[b] = lbfgs_gts(l, b);
  a.lam[b] = 1.0;
  a.accepted[b] = 0;
  atomicAdd(a.counter, 1);
}

// monotone Armijo test on the projected displacement; a rejected instance halves its step along the projected path
__global__ __launch_bounds__(256) void k_lbfgs_accept(LbfgsArgs l) {
  const SpgArgs& a = l.a;
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= a.batch || a.accepted[b]) return;
  const size_t B = (size_t)a.batch;
  const double gts = a.gtd[b];
  if (gts < 0.0 && a.Jt[b] <= a.J[b] + 1e-4 * gts) {
    a.accepted[b] = 2;  // accepted in this iteration
    return;
  }
  const double half = 0.5 * a.lam[b];
  a.lam[b] = half;
  for (int i = 0; i < a.nV; ++i) a.vt[i * B + b] = spg_proj(a.v[i * B + b] + half * a.d[i * B + b], a.lb[i], a.ub[i]);
  a.gtd[b] = lbfgs_gts(l, b);
  atomicAdd(a.counter, 1);
}

// take the accepted point, Barzilai-Borwein step length as in SPG, store the pair if s'y > 2.2e-16 y'y; a line search
// that failed on a quasi-Newton direction drops the pairs and goes on, one that failed on SPG's direction stops
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
  double sty = 0.0, sts = 0.0, yty = 0.0, smax = 0.0;
  for (int i = 0; i < a.nV; ++i) {
    const double s = a.vt[i * B + b] - a.v[i * B + b], y = a.gt[i * B + b] - a.g[i * B + b];
    sty += s * y;
    sts += s * s;
    yty += y * y;
    smax = fmax(smax, fabs(s));
  }
  const int store = sty > 2.2e-16 * yty, head = l.head[b];
  double *S = l.S + (size_t)head * nVB, *Y = l.Y + (size_t)head * nVB;
  for (int i = 0; i < a.nV; ++i) {
    const double vn = a.vt[i * B + b], gn = a.gt[i * B + b];
    if (store) {
      S[i * B + b] = vn - a.v[i * B + b];
      Y[i * B + b] = gn - a.g[i * B + b];
    }
    a.v[i * B + b] = vn;
    a.g[i * B + b] = gn;
  }
  if (store) {
    l.rho[(size_t)head * B + b] = 1.0 / sty;
    l.head[b] = (head + 1) % l.pairs;
    l.count[b] = min(l.count[b] + 1, l.pairs);
  }
  a.J[b] = a.Jt[b];
  const double an = sty > 0.0 ? sts / fmax(sty, 1e-300) : 1e3;
  a.alpha[b] = fmin(fmax(an, 1e-10), 1e10);
  if (smax <= a.TolX) a.active[b] = 0;
}

int launch_lbfgs(int which, const LbfgsArgs& l, hipStream_t s) {
  const dim3 grid((l.a.batch + 255) / 256), block(256);
  switch (which) {
    case 1: k_lbfgs_direction<<<grid, block, 0, s>>>(l); break;
    case 2: k_lbfgs_accept<<<grid, block, 0, s>>>(l); break;
    case 3: k_lbfgs_update<<<grid, block, 0, s>>>(l); break;
    default: return -1;
  }
  return hip_rc(hipGetLastError());
}

}  // namespace ocs
