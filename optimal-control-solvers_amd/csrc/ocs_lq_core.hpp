// ocs_lq_core.hpp -- what the matrix-core kernels of the shared-Jacobian linear-quadratic problem have in common
// (ocs_lq_kernels.hip: the integrator passes, the one-wave state pass being fb_sweep's too; ocs_lq_sweep_kernels.hip: the
// costate pass of fb_sweep and the launchers of both sweep passes): the MFMA wrapper, the A-operand fragments of a matrix,
// the products on them and the problem's parameter block.
// Mapping "M" (one wave per 16 trajectories) is described at the top of ocs_lq_kernels.hip.
#pragma once
#include "ocs_device_common.hpp"

namespace ocs {

typedef double d4 __attribute__((ext_vector_type(4)));

// time coefficients of the LQ problem for the shared table builders (k_tcoef / k_build_rec)
struct LQTime {
  static constexpr int NTC = 1, NTU = 1, NSC = 0;
  __device__ static inline void tcoef(double t, const double* ps, double* tc, double* tu) {
    tc[0] = exp(-ps[0] * t);
    tu[0] = exp(ps[0] * t);
  }
  __device__ static inline void step_consts(double, double, const double*, const double*, const double*, double*) {}
};

struct LQArgs {
  int N, batch, nS, nC;
  const double* REC;
  const double* ps;     // [r | A nS x nS col-major | Bu nS x nC | q nS | rdiag nC]
  const double* x0;     // forward: [nS][B]
  const double* xck;    // backward: checkpoints [N+1][nAug][B]
  const double* u;      // [2N+1][nC][B]; UCONST: [nC], or [nC][B] with `ub`
  double* x;            // forward out [N+1][nAug][B] or null
  double* J;            // forward out [B]
  const double* Jadd;   // optional [B]
  const double* lamT;   // backward: [nAug][B] or null (default e_last, RK4Integrator.m:63-66)
  double* lam;          // [N+1][nAug][B] or null
  double* dJdu;         // [2N+1][nC][B] or null
  double* lam0;         // [nAug][B] or null
  // fb_sweep's state pass (k_lq_forward with SWEEP; not read by the integrator's passes)
  const int* frozen;    // optional [B]: instances with frozen[b] != 0 store nothing
  const int* gate;      // optional: the launch does nothing if *gate == 0
  // time-parallel passes (k_lq_forward / k_lq_backward with CH != 0): blockIdx.y = chunk c, steps [c L, min(N, (c+1) L))
  int L;                // steps per chunk
  const double* cs;     // chunk start values [C][nS][B]: the state at the chunk's first node / the costate at its last node
  double* ce;           // CH = 1: chunk end values [C][nS][B] (state at the last node from cs / costate at the first node from 0)
  double* cj;           // CH = 2: forward: chunk objective sums [C][B]; adjoint: k1 half of the chunk's first node column [C][nC][B]
  // per-trajectory cost weights (ocs_problem_set_batch_params on the weight range; read by the PW instantiations of the
  // integrator passes only): [nS + nC][B], rows 0 .. nS-1 = q, rows nS .. nS+nC-1 = rdiag; null: the shared block's
  const double* W;
  // UCONST only: 0 (u is [nC], shared), or B when u is [nC][B]: every trajectory under a constant control of its own
  // (ocs_rk4inf_set_batch_ustar)
  int ub;
};
// UCONST: control row g of the lane that holds trajectory b (b < B also for the lanes past a ragged batch end, which are clamped)
__device__ static inline double lq_uconst(const LQArgs& a, int g, int b) {
  return a.ub ? a.u[(size_t)g * a.ub + b] : a.u[g];
}
// k_lq_forward<RT, true, false, 0, false, SWEEP = true> on `a`, RT by a.nS (ocs_lq_kernels.hip)
void lq_forward_one_wave(const LQArgs& a, hipStream_t s);

// D = A(16x4) * B(4x16) + C on one wave; a: lane (g,i) holds A[i][g]; b: lane (g,n) holds B[g][n];
// c/d: lane (g,n) holds rows g + 4j of column n.
__device__ static inline d4 mma(double a, double b, d4 c) {
  return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0);
}

template <int RT>
struct LQMat {
  static constexpr int KS = 4 * RT;
  double f[RT][KS];
};

// fragments of M (rows x cols, column-major with leading dimension ld, zero outside) as the A operand:
// tile rt, k-step kk: lane (g,i) <- M[16 rt + i][4 kk + g];  TRANS reads M' instead.
template <int RT, bool TRANS>
__device__ static inline void load_frags(LQMat<RT>& o, const double* M, int ld, int rows, int cols, int g, int i) {
#pragma unroll
  for (int rt = 0; rt < RT; ++rt)
#pragma unroll
    for (int kk = 0; kk < 4 * RT; ++kk) {
      const int r = 16 * rt + i, c = 4 * kk + g;
      const int rr = TRANS ? c : r, cc = TRANS ? r : c;
      o.f[rt][kk] = (rr < rows && cc < cols) ? M[rr + (size_t)ld * cc] : 0.0;
    }
}

// acc (tile rt, reg j) <-> row 4 (4 rt + j) + g, i.e. per-lane value index m = 4 rt + j
template <int RT>
__device__ static inline void matvec(const LQMat<RT>& A, const double (&v)[4 * RT], d4 (&acc)[RT]) {
  if constexpr (RT == 1) {  // a single tile: two independent accumulation chains instead of one dependent one
    d4 alt = {0.0, 0.0, 0.0, 0.0};
    acc[0] = mma(A.f[0][0], v[0], acc[0]);
    alt = mma(A.f[0][1], v[1], alt);
    acc[0] = mma(A.f[0][2], v[2], acc[0]);
    alt = mma(A.f[0][3], v[3], alt);
    acc[0] += alt;
  } else {
#pragma unroll
    for (int kk = 0; kk < 4 * RT; ++kk)
#pragma unroll
      for (int rt = 0; rt < RT; ++rt) acc[rt] = mma(A.f[rt][kk], v[kk], acc[rt]);
  }
}

template <int RT>
__device__ static inline void unpack(const d4 (&acc)[RT], double (&f)[4 * RT]) {
#pragma unroll
  for (int rt = 0; rt < RT; ++rt) {
    f[4 * rt + 0] = acc[rt].x;
    f[4 * rt + 1] = acc[rt].y;
    f[4 * rt + 2] = acc[rt].z;
    f[4 * rt + 3] = acc[rt].w;
  }
}

// sum over the four lanes (g = 0..3) that share a trajectory
__device__ static inline double sum_over_g(double v) {
  v += __shfl_xor(v, 16);
  v += __shfl_xor(v, 32);
  return v;
}

template <int RT>
struct LQCore {
  static constexpr int KS = 4 * RT;
  LQMat<RT> A;
  double Bu[RT];   // A-operand fragments of Bu (nS x nC, K = 4 >= nC): lane (g,i) <- Bu[16 rt + i][g]
  double q[KS];    // q[4m + g]
  double R;        // rdiag[g] (0 for g >= nC)

  __device__ inline void load(const double* ps, int nS, int nC, int g, int i) {
    load_frags<RT, false>(A, ps + 1, nS, nS, nS, g, i);
    const double* bu = ps + 1 + (size_t)nS * nS;
#pragma unroll
    for (int rt = 0; rt < RT; ++rt) {
      const int r = 16 * rt + i;
      Bu[rt] = (r < nS && g < nC) ? bu[r + (size_t)nS * g] : 0.0;
    }
    const double* qq = bu + (size_t)nS * nC;
#pragma unroll
    for (int m = 0; m < KS; ++m) q[m] = (4 * m + g < nS) ? qq[4 * m + g] : 0.0;
    R = (g < nC) ? qq[nS + g] : 0.0;
  }
  // q and R of trajectory b (the column this lane holds the B operand and the accumulators of) in place of the shared ones
  __device__ inline void load_weights(const double* W, size_t B, int b, int nS, int nC, int g) {
#pragma unroll
    for (int m = 0; m < KS; ++m) q[m] = (4 * m + g < nS) ? W[(size_t)(4 * m + g) * B + b] : 0.0;
    R = (g < nC) ? W[(size_t)(nS + g) * B + b] : 0.0;
  }
  // Bu * u for 16 trajectories (lane (g,n) holds u_g of trajectory n)
  __device__ inline void bu_times(double u, d4 (&o)[RT]) const {
#pragma unroll
    for (int rt = 0; rt < RT; ++rt) {
      const d4 z = {0.0, 0.0, 0.0, 0.0};
      o[rt] = mma(Bu[rt], u, z);
    }
  }
  // state rows of F: A Y + Bu u (bu = Bu u precomputed)
  __device__ inline void Fx(const double (&Y)[KS], const d4 (&bu)[RT], double (&f)[KS]) const {
    d4 acc[RT];
#pragma unroll
    for (int rt = 0; rt < RT; ++rt) acc[rt] = bu[rt];
    matvec<RT>(A, Y, acc);
    unpack<RT>(acc, f);
  }
  // this lane's share of the objective integrand e^{-rt}(sum q x^2 + sum R u^2)
  __device__ inline double cost_part(const double (&Y)[KS], double u, double e) const {
    double s = R * (u * u);
#pragma unroll
    for (int m = 0; m < KS; ++m) s = __builtin_fma(q[m], Y[m] * Y[m], s);
    return e * s;
  }
};

}  // namespace ocs
