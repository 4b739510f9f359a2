// ocs_xlam_err_device.hpp -- kernel template of the error estimate of the sweep's pass pair (ocs_x_lam_err): how far are
// x and lam of compute_x_lam, fixed-step RK4 on the grid under the control samples ugrid, from the continuous problem under
// that control?  Step doubling, per interval i and instance.  Shared by ocs_xlam_err_kernels.hip (registry problems) and the
// hipRTC path for user problems; device code only.
//
//   control   between its 2N+1 samples the pchip interpolant of them on the grid t (pchip_slope_at / pchip_piece), at the
//             quarter points t_i + h/4 and t_i + 3h/4: five values per interval with the three samples
//   state     from y_i = [x_i; 0]: one RK4 step of h with the three samples (the pass's step), two of h/2 with the five
//             values;  ex = 16/15 |fine - coarse| per state row;  dJ = 16/15 ((coarse - fine) of the cost row + lam_{i+1}'
//             (coarse - fine) of the state rows), signed: the step's share of J(grid) - J(continuous) to first order (lam is
//             the derivative of the rest of the objective by the state)
//   costate   from lam_{i+1} backward: one RK4 step of h as the pass does it (x at the nodes and at the pchip midpoint of
//             the node values), two of h/2 with x at the nodes, the fine state x^_m after its first half step at the middle
//             and, at the quarter points, the cubic Hermite interpolant through (x_i, f_i), (x^_m, f^_m), (x_{i+1},
//             f_{i+1}) at the middle of each half -- f the state right-hand side there (f_i and f^_m are the first stages of
//             the two fine state steps).  The pass's midpoint state is the pchip of the nodes, the fine steps' is not: the
//             difference is the coupling error of the pass;  el = 16/15 |fine - coarse| per row
//   ratios    rx = max_k ex_k / (AbsTol + RelTol max(|x_{i,k}|, |x_{i+1,k}|)),  rl the same with el and lam
//
// The mapping of k_bvp_rms: one thread per (instance, chunk of kErrChunk intervals), batch-minor loads; the right node's f,
// the pchip slopes of u and of x there become the next interval's left ones.  Only F and dFdx_times_vec are evaluated
// (the A9 adapter's adjointRHS); ControlChar is never called.  PM: the chunk's largest ratio, a NaN counted as +inf; PJ:
// the chunk's sum of dJ in interval order.
#pragma once
#include "ocs_device_common.hpp"

namespace ocs {

constexpr int kErrChunk = 8;   // intervals per thread

// the larger of two numbers, NaN if either is one
__device__ static inline double nan_max(double a, double b) { return (a != a || b != b) ? a + b : fmax(a, b); }

struct XlamErrArgs {
  int N, batch;
  const double* HT;    // [N][4] = {h, h/2, h/6, h/3}
  const double* TC;    // [2N+1][NTC] F-side time coefficients of the grid points
  const double* TCQ;   // [2N][NTC] ... of the quarter points: 2 i at t_i + h/4, 2 i + 1 at t_i + 3h/4
  const double* SQ;    // [2N] their local coordinates in the grid intervals 2 i and 2 i + 1 (t_q - t[2 i], t_q - t[2 i + 1])
  PchipTab TG;         // the grid t (2N+1 points): pchip of the control samples
  PchipTab TX;         // the nodes (N+1 points): pchip of the node states
  const double* TM;    // [N] interval middles
  const double* ps;
  const double* pb;
  unsigned pmask;
  const double* u;     // [2N+1][nC][B]
  const double* x;     // [N+1][ldx][B], rows 0 .. nS-1
  int ldx;
  const double* lam;   // [N+1][nS][B]
  double rtol, atol;
  double* rx;          // [N][B]
  double* rl;          // [N][B]
  double* PM;          // [chunks][B]
  double* PJ;          // [chunks][B]
};

template <class P>
__global__ __launch_bounds__(64) void k_xlam_err(const XlamErrArgs a) {
  constexpr int NS = P::NS, NC = P::NC, NA = P::NS + 1, NTC = P::NTC;
  const int b = blockIdx.x * 64 + threadIdx.x;
  const int i0 = blockIdx.y * kErrChunk;
  if (b >= a.batch || i0 >= a.N) return;
  const size_t B = (size_t)a.batch;
  const typename P::Par p = P::load(ParamSrc{as_uniform(a.ps), a.pb, a.pmask, B, b});
  const uniform_ptr HT = as_uniform(a.HT), TC = as_uniform(a.TC), TCQ = as_uniform(a.TCQ), SQ = as_uniform(a.SQ),
                    TM = as_uniform(a.TM), TN = as_uniform(a.TX.TN);
  const size_t ldU = (size_t)NC * B, ldX = (size_t)a.ldx * B;
  const double* up = a.u + b;
  const double* xp = a.x + b;
  const double* lp = a.lam + b;

  auto tcs = [&](uniform_ptr tab, int j, double* tc) OCS_INLINE {
#pragma unroll
    for (int k = 0; k < NTC; ++k) tc[k] = tab[(size_t)j * NTC + k];
  };
  // adjointRHS(t, x, lam, u) = -dFdx_times_vec(t, [x; 0], u, [lam; 1])(1:nS)
  auto arhs = [&](const double* tc, const double* x, const double* l, const double* u, double* out) OCS_INLINE {
    double v[NA], g[NS];
#pragma unroll
    for (int k = 0; k < NS; ++k) v[k] = l[k];
    v[NS] = 1.0;
    P::dFdxT(tc, x, u, p, v, g);
#pragma unroll
    for (int k = 0; k < NS; ++k) out[k] = -g[k];
  };
  // y + c f on the NA rows (F reads the NS state rows only)
  auto axpy = [&](const double* y, double c, const double* f, double* out) OCS_INLINE {
#pragma unroll
    for (int k = 0; k < NA; ++k) out[k] = __builtin_fma(c, f[k], y[k]);
  };
  // one RK4 step of the augmented state from y over hs, its first stage F1 given: F at (tcM, uM) twice and at (tcB, uB)
  auto state_step = [&](const double* y, double hs, const double* F1, const double* tcM, const double* uM, const double* tcB,
                        const double* uB, double* out) OCS_INLINE {
    double ys[NA], F2[NA], F3[NA], F4[NA];
    axpy(y, 0.5 * hs, F1, ys);
    P::F(tcM, ys, uM, p, F2);
    axpy(y, 0.5 * hs, F2, ys);
    P::F(tcM, ys, uM, p, F3);
    axpy(y, hs, F3, ys);
    P::F(tcB, ys, uB, p, F4);
#pragma unroll
    for (int k = 0; k < NA; ++k) out[k] = __builtin_fma(hs / 6.0, (F1[k] + 2.0 * F2[k]) + (2.0 * F3[k] + F4[k]), y[k]);
  };
  // one RK4 step of the costate backward over hs from l: (tcB, xB, uB) -> (tcM, xM, uM) twice -> (tcA, xA, uA)
  auto costate_step = [&](const double* l, double hs, const double* tcB, const double* xB, const double* uB, const double* tcM,
                          const double* xM, const double* uM, const double* tcA, const double* xA, const double* uA,
                          double* out) OCS_INLINE {
    double k1[NS], k2[NS], k3[NS], k4[NS], ls[NS];
    arhs(tcB, xB, l, uB, k1);
#pragma unroll
    for (int k = 0; k < NS; ++k) ls[k] = __builtin_fma(-0.5 * hs, k1[k], l[k]);
    arhs(tcM, xM, ls, uM, k2);
#pragma unroll
    for (int k = 0; k < NS; ++k) ls[k] = __builtin_fma(-0.5 * hs, k2[k], l[k]);
    arhs(tcM, xM, ls, uM, k3);
#pragma unroll
    for (int k = 0; k < NS; ++k) ls[k] = __builtin_fma(-hs, k3[k], l[k]);
    arhs(tcA, xA, ls, uA, k4);
#pragma unroll
    for (int k = 0; k < NS; ++k) out[k] = __builtin_fma(-hs / 6.0, (k1[k] + 2.0 * k2[k]) + (2.0 * k3[k] + k4[k]), l[k]);
  };

  // the left node of the chunk: x, lam, u, f, and the pchip slopes of u (grid point 2 i0) and of x (node i0)
  double yA[NA], lA[NS], uA[NC], fA[NA], duA[NC], dxA[NS], tcA[NTC];
  tcs(TC, 2 * i0, tcA);
#pragma unroll
  for (int k = 0; k < NS; ++k) {
    yA[k] = xp[((size_t)i0 * a.ldx + k) * B];
    lA[k] = lp[((size_t)i0 * NS + k) * B];
    dxA[k] = pchip_slope_at(a.TX, xp + (size_t)k * B, ldX, i0);
  }
  yA[NS] = 0.0;
#pragma unroll
  for (int c = 0; c < NC; ++c) {
    uA[c] = up[((size_t)(2 * i0) * NC + c) * B];
    duA[c] = pchip_slope_at(a.TG, up + (size_t)c * B, ldU, 2 * i0);
  }
  P::F(tcA, yA, uA, p, fA);

  double pm = 0.0, pj = 0.0;
  const int iend = i0 + kErrChunk < a.N ? i0 + kErrChunk : a.N;
#pragma unroll 1
  for (int i = i0; i < iend; ++i) {
    const double h = HT[4 * (size_t)i], hh = 0.5 * h;
    double yB[NA], lB[NS], uM[NC], uB[NC], u1[NC], u3[NC], duB[NC], dxB[NS], tcM[NTC], tcB[NTC], tc1[NTC], tc3[NTC];
    tcs(TC, 2 * i + 1, tcM);
    tcs(TC, 2 * i + 2, tcB);
    tcs(TCQ, 2 * i, tc1);
    tcs(TCQ, 2 * i + 1, tc3);
#pragma unroll
    for (int k = 0; k < NS; ++k) {
      yB[k] = xp[((size_t)(i + 1) * a.ldx + k) * B];
      lB[k] = lp[((size_t)(i + 1) * NS + k) * B];
      dxB[k] = pchip_slope_at(a.TX, xp + (size_t)k * B, ldX, i + 1);
    }
    yB[NS] = 0.0;
    // the control: samples at the middle and the right node, pchip at the quarter points
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      const double* uc = up + (size_t)c * B;
      uM[c] = uc[(size_t)(2 * i + 1) * ldU];
      uB[c] = uc[(size_t)(2 * i + 2) * ldU];
      const double duM = pchip_slope_at(a.TG, uc, ldU, 2 * i + 1);
      duB[c] = pchip_slope_at(a.TG, uc, ldU, 2 * i + 2);
      u1[c] = pchip_piece(uA[c], uM[c], duA[c], duM, a.TG.HN[2 * i], SQ[2 * (size_t)i]);
      u3[c] = pchip_piece(uM[c], uB[c], duM, duB[c], a.TG.HN[2 * i + 1], SQ[2 * (size_t)i + 1]);
    }
    // ---- state: coarse, fine ----
    double yc[NA], ym[NA], yf[NA], fm[NA], fB[NA];
    state_step(yA, h, fA, tcM, uM, tcB, uB, yc);
    state_step(yA, hh, fA, tc1, u1, tcM, uM, ym);
    P::F(tcM, ym, uM, p, fm);
    state_step(ym, hh, fm, tc3, u3, tcB, uB, yf);
    P::F(tcB, yB, uB, p, fB);
    // ---- the states of the costate steps: pchip midpoint of the nodes (coarse), Hermite quarter points (fine) ----
    double xM[NS], x1[NS], x3[NS];
    const double sm = TM[i] - TN[i], h16 = 0.0625 * h;
#pragma unroll
    for (int k = 0; k < NS; ++k) {
      xM[k] = pchip_piece(yA[k], yB[k], dxA[k], dxB[k], a.TX.HN[i], sm);
      x1[k] = __builtin_fma(h16, fA[k] - fm[k], 0.5 * (yA[k] + ym[k]));
      x3[k] = __builtin_fma(h16, fm[k] - fB[k], 0.5 * (ym[k] + yB[k]));
    }
    // ---- costate: coarse, fine ----
    double lc[NS], lm[NS], lf[NS];
    costate_step(lB, h, tcB, yB, uB, tcM, xM, uM, tcA, yA, uA, lc);
    costate_step(lB, hh, tcB, yB, uB, tc3, x3, u3, tcM, ym, uM, lm);
    costate_step(lm, hh, tcM, ym, uM, tc1, x1, u1, tcA, yA, uA, lf);
    // ---- ratios (maxima that keep a NaN: fmax alone would drop it) ----
    double rx = 0.0, rl = 0.0;
#pragma unroll
    for (int k = 0; k < NS; ++k) {
      const double qx = (16.0 / 15.0) * fabs(yf[k] - yc[k]) / __builtin_fma(a.rtol, nan_max(fabs(yA[k]), fabs(yB[k])), a.atol);
      const double ql = (16.0 / 15.0) * fabs(lf[k] - lc[k]) / __builtin_fma(a.rtol, nan_max(fabs(lA[k]), fabs(lB[k])), a.atol);
      rx = nan_max(rx, qx);
      rl = nan_max(rl, ql);
    }
    a.rx[(size_t)i * B + b] = rx;
    a.rl[(size_t)i * B + b] = rl;
    const double r = (rx == rx && rl == rl) ? fmax(rx, rl) : __builtin_inf();
    pm = fmax(pm, r);
    // the step's share of J(grid) - J(continuous), to first order: its own cost error and what its state error does to the
    // cost of the rest of the horizon, lam_{i+1}' (x_coarse - x_fine) -- lam is dJ/dx of that rest (lam(TF) = 0)
    double dj = yc[NS] - yf[NS];
#pragma unroll
    for (int k = 0; k < NS; ++k) dj = __builtin_fma(lB[k], yc[k] - yf[k], dj);
    pj += (16.0 / 15.0) * dj;
    // the right node becomes the left one
#pragma unroll
    for (int k = 0; k < NS; ++k) {
      yA[k] = yB[k];
      lA[k] = lB[k];
      dxA[k] = dxB[k];
    }
#pragma unroll
    for (int k = 0; k < NA; ++k) fA[k] = fB[k];
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      uA[c] = uB[c];
      duA[c] = duB[c];
    }
#pragma unroll
    for (int k = 0; k < NTC; ++k) tcA[k] = tcB[k];
  }
  a.PM[(size_t)blockIdx.y * B + b] = pm;
  a.PJ[(size_t)blockIdx.y * B + b] = pj;
}

}  // namespace ocs
