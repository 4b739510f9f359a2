// ocs_bvp_device.hpp -- kernel templates of the batched bvp_solver (functions/bvp_solver.m): damped Newton on the
// Simpson / Lobatto-IIIa collocation of the optimality system y' = optSys(t, y), y = [x; lam] (bvp_solver.m:105-109) on the
// integrator's node grid.  Shared by ocs_bvp_kernels.hip (registry problems) and the hipRTC path for user problems; device
// code only.
//
//   f(t, y)  = [F(1:nS); -dFdx_times_vec(t, [x;0], u, [lam;1])(1:nS)],  u = ControlChar(t, x, lam)   (the A9 adapter)
//   y_m      = (y_i + y_{i+1})/2 + h/8 (f_i - f_{i+1})
//   Phi_i    = y_{i+1} - y_i - h/6 (f_i + 4 f(t_i + h/2, y_m) + f_{i+1})
//   df/dy    by forward differences, column by column, step sqrt(eps) max(1, |y_k|): ControlChar's clamp is differentiated
//            as it stands
// k_bvp_assemble turns every interval into the step map  dy_{i+1} = A_i dy_i + b_i  of the Newton system
// (dPhi_i/dy_{i+1}) dy_{i+1} + (dPhi_i/dy_i) dy_i = -Phi_i;  k_bvp_norm evaluates Phi alone at a line-search trial point.
//
// The mesh side (bvp4c / solve_bvp's error control): with S the cubic Hermite interpolant of a nodal solution through
// (y_i, f_i), (y_{i+1}, f_{i+1}), k_bvp_rms estimates the residual S' - optSys(t, S) of every interval by the five-point
// Lobatto rule (zero at the nodes: the middle and t_m -/+ (h/2) sqrt(3/7) remain); k_bvp_prolong evaluates S at the nodes of
// another mesh.
#pragma once
#include "ocs_device_common.hpp"

namespace ocs {

constexpr int kBvpChunk = 8;   // intervals per thread of the assembly and the residual kernel (one partial norm per chunk)

struct BvpArgs {
  int N, batch;
  const double* HT;    // [N][4] = {h, h/2, h/6, h/3}
  const double* TC;    // [2N+1][NTC] F-side time coefficients of the grid points
  const double* TU;    // [2N+1][NTU] ControlChar-side
  const double* ps;
  const double* pb;
  unsigned pmask;
  const double* lb;
  const double* ub;
  int bstride;         // 0: lb / ub are [NC], shared; batch: [NC][batch], the instance's own (bound_at)
  const double* x0;    // [nS][B]
  const double* y;     // [N+1][2 nS][B] the iterate
  const double* d;     // [N+1][2 nS][B] the Newton step (k_bvp_norm: the trial point is y + alpha d)
  double alpha;
  const int* status;   // k_bvp_assemble: instances with status != 0 (finished) are skipped
  const int* search;   // k_bvp_norm: instances with search == 0 (step accepted, or finished) are skipped
  double* AB;          // k_bvp_assemble: [N][2 nS (2 nS + 1)][B] rows of [A_i | b_i]
  double* SS;          // k_bvp_norm: [chunks][B] sum of squares of the chunk's residuals ...
  double* MX;          //             ... and their largest magnitude
  const int* gate;     // optional: the launch does nothing if *gate == 0
};

// In-place Gauss-Jordan elimination with partial pivoting on M = [S | C] (S: NR x NR, C: NR x NCOL): C becomes S^{-1} C.
// Every index is a compile-time constant (rows are exchanged by selects), so M lives in registers.  A zero or non-finite
// pivot leaves non-finite values in C: the caller's instance fails its finiteness test, nothing is aborted.
template <int NR, int NCOL>
__device__ static inline void bvp_gauss_jordan(double (&M)[NR][NR + NCOL]) {
  constexpr int W = NR + NCOL;
#pragma unroll
  for (int k = 0; k < NR; ++k) {
    int piv = k;
    double best = fabs(M[k][k]);
#pragma unroll
    for (int r = k + 1; r < NR; ++r) {
      const double a = fabs(M[r][k]);
      if (a > best) {
        best = a;
        piv = r;
      }
    }
#pragma unroll
    for (int r = k + 1; r < NR; ++r) {
      const bool sw = piv == r;
#pragma unroll
      for (int c = k; c < W; ++c) {
        const double top = M[k][c], low = M[r][c];
        M[k][c] = sw ? low : top;
        M[r][c] = sw ? top : low;
      }
    }
    const double inv = 1.0 / M[k][k];
#pragma unroll
    for (int c = k + 1; c < W; ++c) M[k][c] *= inv;
#pragma unroll
    for (int r = 0; r < NR; ++r) {
      if (r == k) continue;
      const double fct = M[r][k];
#pragma unroll
      for (int c = k + 1; c < W; ++c) M[r][c] = __builtin_fma(-fct, M[k][c], M[r][c]);
    }
  }
}

// optSys of one instance at the grid points of the integrator (bvp_solver.m:105-109 through the A9 adapter)
template <class P>
struct BvpRhs {
  static constexpr int NS = P::NS, NC = P::NC, NY = 2 * P::NS;
  typename P::Par p;
  double lb[NC], ub[NC];
  uniform_ptr TC, TU;
  template <class Args>   // (BvpArgs, BvpRmsArgs, BvpProlongArgs: the same member names)
  __device__ inline BvpRhs(const Args& a, int b)
      : p(P::load(ParamSrc{as_uniform(a.ps), a.pb, a.pmask, (size_t)a.batch, b})), TC(as_uniform(a.TC)), TU(as_uniform(a.TU)) {
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      lb[c] = bound_at(a.lb, c, a.bstride, b);
      ub[c] = bound_at(a.ub, c, a.bstride, b);
    }
  }
  // f = optSys(t_j, y), j = grid point (2 i: node i, 2 i + 1: the middle of interval i)
  __device__ inline OCS_INLINE void operator()(int j, const double* y, double* f) const {
    at(TC + (size_t)j * P::NTC, TU + (size_t)j * P::NTU, y, f);
  }
  // f = optSys(t, y) at a time with the coefficients tcp [NTC], tup [NTU] (a row of a table of its own: the Lobatto points)
  __device__ inline OCS_INLINE void at(uniform_ptr tcp, uniform_ptr tup, const double* y, double* f) const {
    double tc[P::NTC], tu[P::NTU], u[NC], F[NS + 1], v[NS + 1], g[NS];
#pragma unroll
    for (int k = 0; k < P::NTC; ++k) tc[k] = tcp[k];
#pragma unroll
    for (int k = 0; k < P::NTU; ++k) tu[k] = tup[k];
    P::control_char(tu, y, y + NS, p, lb, ub, u);
    P::F(tc, y, u, p, F);
#pragma unroll
    for (int k = 0; k < NS; ++k) v[k] = y[NS + k];
    v[NS] = 1.0;
    P::dFdxT(tc, y, u, p, v, g);
#pragma unroll
    for (int k = 0; k < NS; ++k) {
      f[k] = F[k];
      f[NS + k] = -g[k];
    }
  }
  // J[r][k] = d f_r / d y_k by forward differences (f = optSys(t_j, y) is given)
  __device__ inline OCS_INLINE void jac(int j, const double* y, const double* f, double (&J)[NY][NY]) const {
#pragma unroll
    for (int k = 0; k < NY; ++k) {
      double yp[NY], fp[NY];
#pragma unroll
      for (int r = 0; r < NY; ++r) yp[r] = y[r];
      const double step = 1.4901161193847656e-08 * fmax(1.0, fabs(y[k]));   // sqrt(eps) max(1, |y_k|)
      yp[k] = y[k] + step;
      (*this)(j, yp, fp);
      const double inv = 1.0 / step;
#pragma unroll
      for (int r = 0; r < NY; ++r) J[r][k] = (fp[r] - f[r]) * inv;
    }
  }
};

// Phi of interval i from the end values and their right-hand sides; ym, fm: the collocation point and optSys there
template <class P>
__device__ static inline OCS_INLINE void bvp_residual(const BvpRhs<P>& rhs, int i, double h6, double h8, const double* yl,
                                                      const double* fl, const double* yr, const double* fr, double* ym,
                                                      double* fm, double* phi) {
  constexpr int NY = 2 * P::NS;
#pragma unroll
  for (int r = 0; r < NY; ++r) ym[r] = __builtin_fma(h8, fl[r] - fr[r], 0.5 * (yl[r] + yr[r]));
  rhs(2 * i + 1, ym, fm);
#pragma unroll
  for (int r = 0; r < NY; ++r) phi[r] = (yr[r] - yl[r]) - h6 * (fl[r] + 4.0 * fm[r] + fr[r]);
}

// ---------------------------------------------------------------------------------------
// assembly: one thread per (instance, chunk of kBvpChunk intervals); the right node of an interval (optSys and its
// Jacobian there) is the left node of the next.  blockIdx.y = chunk.
// ---------------------------------------------------------------------------------------
template <class P>
__global__ __launch_bounds__(64) void k_bvp_assemble(const BvpArgs a) {
  constexpr int NY = 2 * P::NS, NE = NY * (NY + 1);
  if (a.gate && *a.gate == 0) return;
  const int b = blockIdx.x * 64 + threadIdx.x;
  const int i0 = blockIdx.y * kBvpChunk;
  if (b >= a.batch || i0 >= a.N || a.status[b] != 0) return;
  const size_t B = (size_t)a.batch;
  const BvpRhs<P> rhs(a, b);
  const uniform_ptr HT = as_uniform(a.HT);
  double yl[NY], fl[NY], Jl[NY][NY];
#pragma unroll
  for (int r = 0; r < NY; ++r) yl[r] = a.y[((size_t)i0 * NY + r) * B + b];
  rhs(2 * i0, yl, fl);
  rhs.jac(2 * i0, yl, fl, Jl);
  const int iend = i0 + kBvpChunk < a.N ? i0 + kBvpChunk : a.N;
#pragma unroll 1
  for (int i = i0; i < iend; ++i) {
    const double h = HT[4 * (size_t)i], h6 = HT[4 * (size_t)i + 2], h8 = 0.125 * h;
    double yr[NY], fr[NY], Jr[NY][NY], ym[NY], fm[NY], phi[NY], Jm[NY][NY];
#pragma unroll
    for (int r = 0; r < NY; ++r) yr[r] = a.y[((size_t)(i + 1) * NY + r) * B + b];
    rhs(2 * i + 2, yr, fr);
    rhs.jac(2 * i + 2, yr, fr, Jr);
    bvp_residual<P>(rhs, i, h6, h8, yl, fl, yr, fr, ym, fm, phi);
    rhs.jac(2 * i + 1, ym, fm, Jm);
    // M = [dPhi/dy_{i+1} | dPhi/dy_i | Phi]:  with Dl = dy_m/dy_i = I/2 + h/8 Jl, Dr = dy_m/dy_{i+1} = I/2 - h/8 Jr
    //   dPhi/dy_i = -I - h/6 (Jl + 4 Jm Dl),  dPhi/dy_{i+1} = I - h/6 (Jr + 4 Jm Dr)
    double M[NY][2 * NY + 1];
#pragma unroll
    for (int r = 0; r < NY; ++r) {
#pragma unroll
      for (int c = 0; c < NY; ++c) {
        double sl = 0.0, sr = 0.0;
#pragma unroll
        for (int q = 0; q < NY; ++q) {
          sl = __builtin_fma(Jm[r][q], (q == c ? 0.5 : 0.0) + h8 * Jl[q][c], sl);
          sr = __builtin_fma(Jm[r][q], (q == c ? 0.5 : 0.0) - h8 * Jr[q][c], sr);
        }
        M[r][c] = (r == c ? 1.0 : 0.0) - h6 * (Jr[r][c] + 4.0 * sr);
        M[r][NY + c] = (r == c ? -1.0 : 0.0) - h6 * (Jl[r][c] + 4.0 * sl);
      }
      M[r][2 * NY] = phi[r];
    }
    bvp_gauss_jordan<NY, NY + 1>(M);
    double* dst = a.AB + (size_t)i * NE * B + b;
#pragma unroll
    for (int r = 0; r < NY; ++r)
#pragma unroll
      for (int c = 0; c <= NY; ++c) dst[(size_t)(r * (NY + 1) + c) * B] = -M[r][NY + c];
#pragma unroll
    for (int r = 0; r < NY; ++r) {
      yl[r] = yr[r];
      fl[r] = fr[r];
#pragma unroll
      for (int c = 0; c < NY; ++c) Jl[r][c] = Jr[r][c];
    }
  }
}

// ---------------------------------------------------------------------------------------
// residual at a trial point y + alpha d: per chunk of intervals the sum of squares and the largest magnitude of Phi (the
// first chunk adds the boundary rows x_0 - x0, the last one lam_N, bvp_solver.m:66); reduced in chunk order by k_bvp_accept.
// ---------------------------------------------------------------------------------------
template <class P>
__global__ __launch_bounds__(64) void k_bvp_norm(const BvpArgs a) {
  constexpr int NS = P::NS, NY = 2 * P::NS;
  if (a.gate && *a.gate == 0) return;
  const int b = blockIdx.x * 64 + threadIdx.x;
  const int i0 = blockIdx.y * kBvpChunk;
  if (b >= a.batch || i0 >= a.N || a.search[b] == 0) return;
  const size_t B = (size_t)a.batch;
  const BvpRhs<P> rhs(a, b);
  const uniform_ptr HT = as_uniform(a.HT);
  auto trial = [&](int i, double* y) OCS_INLINE {
#pragma unroll
    for (int r = 0; r < NY; ++r) {
      const size_t at = ((size_t)i * NY + r) * B + b;
      y[r] = __builtin_fma(a.alpha, a.d[at], a.y[at]);
    }
  };
  double ss = 0.0, mx = 0.0;
  auto take = [&](double v) OCS_INLINE {
    ss = __builtin_fma(v, v, ss);
    mx = fmax(mx, fabs(v));
  };
  double yl[NY], fl[NY];
  trial(i0, yl);
  rhs(2 * i0, yl, fl);
  if (i0 == 0) {
#pragma unroll
    for (int k = 0; k < NS; ++k) take(yl[k] - a.x0[(size_t)k * B + b]);
  }
  const int iend = i0 + kBvpChunk < a.N ? i0 + kBvpChunk : a.N;
#pragma unroll 1
  for (int i = i0; i < iend; ++i) {
    const double h = HT[4 * (size_t)i], h6 = HT[4 * (size_t)i + 2], h8 = 0.125 * h;
    double yr[NY], fr[NY], ym[NY], fm[NY], phi[NY];
    trial(i + 1, yr);
    rhs(2 * i + 2, yr, fr);
    bvp_residual<P>(rhs, i, h6, h8, yl, fl, yr, fr, ym, fm, phi);
#pragma unroll
    for (int r = 0; r < NY; ++r) {
      take(phi[r]);
      yl[r] = yr[r];
      fl[r] = fr[r];
    }
  }
  if (iend == a.N) {
#pragma unroll
    for (int k = 0; k < NS; ++k) take(yl[NS + k]);
  }
  a.SS[(size_t)blockIdx.y * B + b] = ss;
  a.MX[(size_t)blockIdx.y * B + b] = mx;
}

// ---------------------------------------------------------------------------------------
// residual estimate of a nodal solution (estimate_rms_residuals of scipy's solve_bvp; Kierzenka & Shampine's bvp4c): per
// interval and instance
//   rms_i = sqrt( 1/2 ( 32/45 |r_m|^2 + 49/90 (|r_+|^2 + |r_-|^2) ) ),   r = (S' - optSys(t, S)) / (1 + |optSys(t, S)|)
// componentwise, at t_m and t_m -/+ (h/2) sqrt(3/7).  With theta = (t - t_i) / h = 1/2 -/+ s, s = sqrt(3/7) / 2, and
// theta (1 - theta) = 1/7 the Hermite weights are constants:
//   S  = y_i + w (y_{i+1} - y_i) + h (a f_i - b f_{i+1}),   w = (9 theta - 1) / 7,  a = (1 - theta) / 7,  b = theta / 7
//   S' = 6/7 (y_{i+1} - y_i) / h + (4/7 - theta) f_i + (theta - 3/7) f_{i+1}
// The mapping of k_bvp_norm: one thread per (instance, chunk of kBvpChunk intervals), the right node's optSys kept as the
// next left node's.  PM: the chunk's largest rms, a NaN counted as +inf.
// ---------------------------------------------------------------------------------------
struct BvpRmsArgs {
  int N, batch;
  const double* HT;
  const double* TC;
  const double* TU;
  const double* TCL;   // [2N][NTC] time coefficients of the Lobatto points: 2 i at t_m - (h/2) sqrt(3/7), 2 i + 1 at t_m + ...
  const double* TUL;   // [2N][NTU]
  const double* ps;
  const double* pb;
  unsigned pmask;
  const double* lb;
  const double* ub;
  int bstride;
  const double* y;     // [N+1][2 nS][B]
  double* rms;         // [N][B]
  double* PM;          // [chunks][B]
};

constexpr double kLobS = 0.32732683535398857;   // sqrt(3/7) / 2

template <class P>
__global__ __launch_bounds__(64) void k_bvp_rms(const BvpRmsArgs a) {
  constexpr int NY = 2 * P::NS;
  const int b = blockIdx.x * 64 + threadIdx.x;
  const int i0 = blockIdx.y * kBvpChunk;
  if (b >= a.batch || i0 >= a.N) return;
  const size_t B = (size_t)a.batch;
  const BvpRhs<P> rhs(a, b);
  const uniform_ptr HT = as_uniform(a.HT), TCL = as_uniform(a.TCL), TUL = as_uniform(a.TUL);
  double yl[NY], fl[NY];
#pragma unroll
  for (int r = 0; r < NY; ++r) yl[r] = a.y[((size_t)i0 * NY + r) * B + b];
  rhs(2 * i0, yl, fl);
  double pm = 0.0;
  const int iend = i0 + kBvpChunk < a.N ? i0 + kBvpChunk : a.N;
#pragma unroll 1
  for (int i = i0; i < iend; ++i) {
    const double h = HT[4 * (size_t)i], h8 = 0.125 * h;
    double yr[NY], fr[NY], dy[NY], sl[NY], ys[NY], fs[NY];
#pragma unroll
    for (int r = 0; r < NY; ++r) yr[r] = a.y[((size_t)(i + 1) * NY + r) * B + b];
    rhs(2 * i + 2, yr, fr);
#pragma unroll
    for (int r = 0; r < NY; ++r) {
      dy[r] = yr[r] - yl[r];
      sl[r] = dy[r] / h;
    }
    // |r|^2 of one point from S' there (sp) and optSys at S (fs)
    auto norm2 = [&](const double* sp) OCS_INLINE {
      double acc = 0.0;
#pragma unroll
      for (int r = 0; r < NY; ++r) {
        const double q = (sp[r] - fs[r]) / (1.0 + fabs(fs[r]));
        acc = __builtin_fma(q, q, acc);
      }
      return acc;
    };
    // the middle: S and S' are the collocation point and the collocation residual of the Simpson formula
    double sp[NY];
#pragma unroll
    for (int r = 0; r < NY; ++r) {
      ys[r] = __builtin_fma(h8, fl[r] - fr[r], 0.5 * (yl[r] + yr[r]));
      sp[r] = 1.5 * sl[r] - 0.25 * (fl[r] + fr[r]);
    }
    rhs(2 * i + 1, ys, fs);
    const double rm = norm2(sp);
    double rpm = 0.0;
#pragma unroll
    for (int side = 0; side < 2; ++side) {
      const double th = side ? 0.5 + kLobS : 0.5 - kLobS;
      const double w = (9.0 * th - 1.0) / 7.0, ca = (1.0 - th) / 7.0, cb = th / 7.0, da = 4.0 / 7.0 - th, db = th - 3.0 / 7.0;
#pragma unroll
      for (int r = 0; r < NY; ++r) {
        ys[r] = yl[r] + w * dy[r] + h * (ca * fl[r] - cb * fr[r]);
        sp[r] = (6.0 / 7.0) * sl[r] + da * fl[r] + db * fr[r];
      }
      rhs.at(TCL + (size_t)(2 * i + side) * P::NTC, TUL + (size_t)(2 * i + side) * P::NTU, ys, fs);
      rpm += norm2(sp);
    }
    const double v = sqrt(0.5 * ((32.0 / 45.0) * rm + (49.0 / 90.0) * rpm));
    a.rms[(size_t)i * B + b] = v;
    pm = fmax(pm, v == v ? v : __builtin_inf());
#pragma unroll
    for (int r = 0; r < NY; ++r) {
      yl[r] = yr[r];
      fl[r] = fr[r];
    }
  }
  a.PM[(size_t)blockIdx.y * B + b] = pm;
}

// ---------------------------------------------------------------------------------------
// S of a nodal solution on the mesh of the integrator at the nodes of another mesh: new node j lies in interval idx[j] at
// theta[j] = (t - t_i) / h in [0, 1].  theta == 0 and theta == 1 are the old nodes idx and idx + 1: copied, not evaluated
// (the same bits).  One thread per (instance, new node); ynew [nnew][2 nS][B].
// ---------------------------------------------------------------------------------------
struct BvpProlongArgs {
  int N, batch, nnew;
  const double* HT;
  const double* TC;
  const double* TU;
  const double* ps;
  const double* pb;
  unsigned pmask;
  const double* lb;
  const double* ub;
  int bstride;
  const double* y;       // [N+1][2 nS][B]
  const int* idx;        // [nnew], 0 .. N-1
  const double* theta;   // [nnew]
  double* ynew;
};

template <class P>
__global__ __launch_bounds__(64) void k_bvp_prolong(const BvpProlongArgs a) {
  constexpr int NY = 2 * P::NS;
  const int b = blockIdx.x * 64 + threadIdx.x;
  const int j = blockIdx.y;
  if (b >= a.batch || j >= a.nnew) return;
  const size_t B = (size_t)a.batch;
  const int i = a.idx[j];
  const double th = a.theta[j];
  if (i < 0 || i >= a.N) return;   // (the host has checked: nothing is read or written out of bounds whatever it passes)
  double* dst = a.ynew + (size_t)j * NY * B + b;
  if (th == 0.0 || th == 1.0) {
    const double* src = a.y + (size_t)(th == 0.0 ? i : i + 1) * NY * B + b;
#pragma unroll
    for (int r = 0; r < NY; ++r) dst[(size_t)r * B] = src[(size_t)r * B];
    return;
  }
  const BvpRhs<P> rhs(a, b);
  double yl[NY], yr[NY], fl[NY], fr[NY];
#pragma unroll
  for (int r = 0; r < NY; ++r) {
    yl[r] = a.y[((size_t)i * NY + r) * B + b];
    yr[r] = a.y[((size_t)(i + 1) * NY + r) * B + b];
  }
  rhs(2 * i, yl, fl);
  rhs(2 * i + 2, yr, fr);
  const double h = as_uniform(a.HT)[4 * (size_t)i];
  const double w = th * th * (3.0 - 2.0 * th), ca = th * (1.0 - th) * (1.0 - th), cb = th * th * (1.0 - th);
#pragma unroll
  for (int r = 0; r < NY; ++r) dst[(size_t)r * B] = yl[r] + w * (yr[r] - yl[r]) + h * (ca * fl[r] - cb * fr[r]);
}

}  // namespace ocs
