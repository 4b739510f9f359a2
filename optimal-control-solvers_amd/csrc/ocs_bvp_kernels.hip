// ocs_bvp_kernels.hip -- batched bvp_solver (functions/bvp_solver.m): the kernels of one damped Newton iteration on the
// collocated optimality system.  Assembly and residual are templates over the problem functor (ocs_bvp_device.hpp; hipRTC
// instances for user problems); the block elimination, the line-search verdict and the bookkeeping do not see the problem.
#include "ocs_bvp_device.hpp"
#include "ocs_internal.hpp"
#include "ocs_jit.hpp"
#include "ocs_problems.hpp"

namespace ocs {

// ---------------------------------------------------------------------------------------
// separated-boundary sweep, one instance per lane: with the step maps dy_{i+1} = A_i dy_i + b_i, dy = [dx; dl],
//   backward from dl_N = -lam_N:   dl_i = P_i dx_i + p_i,   (All - P_{i+1} Axl) [P_i | p_i] = [P_{i+1} Axx - Alx | P_{i+1} bx + p_{i+1} - bl]
//   forward from dx_0 = x0 - x_0:  dx_{i+1} = Axx dx_i + Axl dl_i + bx,   dl_{i+1} = P_{i+1} dx_{i+1} + p_{i+1}
// (one NS x NS pivoted solve per node; the products of the A_i are never formed: the optimality system has growing and
// decaying modes).  A step with a non-finite entry -- a singular pivot here or in the assembly -- marks the instance failed.
// ---------------------------------------------------------------------------------------
template <int NS>
__global__ __launch_bounds__(64) void k_bvp_sweep(BvpSweepArgs a) {
  constexpr int NY = 2 * NS, NE = NY * (NY + 1), NP = NS * (NS + 1);
  const int b = blockIdx.x * 64 + threadIdx.x;
  if (b >= a.batch || a.status[b] != 0) return;
  const size_t B = (size_t)a.batch;
  const int N = a.N;
  double P[NS][NS], p[NS];
#pragma unroll
  for (int r = 0; r < NS; ++r) {
#pragma unroll
    for (int c = 0; c < NS; ++c) P[r][c] = 0.0;
    p[r] = -a.y[((size_t)N * NY + NS + r) * B + b];
  }
  auto store_pp = [&](int i) OCS_INLINE {
    double* dst = a.PP + (size_t)i * NP * B + b;
#pragma unroll
    for (int r = 0; r < NS; ++r) {
#pragma unroll
      for (int c = 0; c < NS; ++c) dst[(size_t)(r * (NS + 1) + c) * B] = P[r][c];
      dst[(size_t)(r * (NS + 1) + NS) * B] = p[r];
    }
  };
  store_pp(N);
#pragma unroll 1
  for (int i = N - 1; i >= 0; --i) {
    double A[NY][NY + 1];
    const double* src = a.AB + (size_t)i * NE * B + b;
#pragma unroll
    for (int r = 0; r < NY; ++r)
#pragma unroll
      for (int c = 0; c <= NY; ++c) A[r][c] = src[(size_t)(r * (NY + 1) + c) * B];
    double M[NS][2 * NS + 1];
#pragma unroll
    for (int r = 0; r < NS; ++r) {
#pragma unroll
      for (int c = 0; c < NS; ++c) {
        double m = A[NS + r][NS + c], q = -A[NS + r][c];
#pragma unroll
        for (int k = 0; k < NS; ++k) {
          m = __builtin_fma(-P[r][k], A[k][NS + c], m);
          q = __builtin_fma(P[r][k], A[k][c], q);
        }
        M[r][c] = m;
        M[r][NS + c] = q;
      }
      double v = p[r] - A[NS + r][NY];
#pragma unroll
      for (int k = 0; k < NS; ++k) v = __builtin_fma(P[r][k], A[k][NY], v);
      M[r][2 * NS] = v;
    }
    bvp_gauss_jordan<NS, NS + 1>(M);
#pragma unroll
    for (int r = 0; r < NS; ++r) {
#pragma unroll
      for (int c = 0; c < NS; ++c) P[r][c] = M[r][NS + c];
      p[r] = M[r][2 * NS];
    }
    store_pp(i);
  }
  double dx[NS], dl[NS];
  bool ok = true;
  auto emit = [&](int i) OCS_INLINE {
    double* dst = a.d + (size_t)i * NY * B + b;
#pragma unroll
    for (int k = 0; k < NS; ++k) {
      dst[(size_t)k * B] = dx[k];
      dst[(size_t)(NS + k) * B] = dl[k];
      ok = ok && isfinite(dx[k]) && isfinite(dl[k]);
    }
  };
#pragma unroll
  for (int k = 0; k < NS; ++k) dx[k] = a.x0[(size_t)k * B + b] - a.y[(size_t)k * B + b];
#pragma unroll
  for (int r = 0; r < NS; ++r) {   // (P, p are those of node 0)
    double v = p[r];
#pragma unroll
    for (int k = 0; k < NS; ++k) v = __builtin_fma(P[r][k], dx[k], v);
    dl[r] = v;
  }
  emit(0);
#pragma unroll 1
  for (int i = 0; i < N; ++i) {
    const double* src = a.AB + (size_t)i * NE * B + b;
    const double* pp = a.PP + (size_t)(i + 1) * NP * B + b;
    double dn[NS];
#pragma unroll
    for (int r = 0; r < NS; ++r) {
      double v = src[(size_t)(r * (NY + 1) + NY) * B];
#pragma unroll
      for (int k = 0; k < NS; ++k) {
        v = __builtin_fma(src[(size_t)(r * (NY + 1) + k) * B], dx[k], v);
        v = __builtin_fma(src[(size_t)(r * (NY + 1) + NS + k) * B], dl[k], v);
      }
      dn[r] = v;
    }
#pragma unroll
    for (int r = 0; r < NS; ++r) {
      double v = pp[(size_t)(r * (NS + 1) + NS) * B];
#pragma unroll
      for (int k = 0; k < NS; ++k) v = __builtin_fma(pp[(size_t)(r * (NS + 1) + k) * B], dn[k], v);
      dl[r] = v;
    }
#pragma unroll
    for (int k = 0; k < NS; ++k) dx[k] = dn[k];
    emit(i + 1);
  }
  // this instance's iteration `it`: the line search looks at it unless the step is unusable
  a.iters[b] = a.it;
  a.alpha[b] = 0.0;
  a.search[b] = ok ? 1 : 0;
  if (!ok) a.status[b] = 2;
}

int launch_bvp_sweep(int nS, const BvpSweepArgs& a, hipStream_t s) {
  const dim3 grid((a.batch + 63) / 64), block(64);
  switch (nS) {
    case 1: k_bvp_sweep<1><<<grid, block, 0, s>>>(a); break;
    case 2: k_bvp_sweep<2><<<grid, block, 0, s>>>(a); break;
    case 3: k_bvp_sweep<3><<<grid, block, 0, s>>>(a); break;
    case 4: k_bvp_sweep<4><<<grid, block, 0, s>>>(a); break;
    default: return -1;
  }
  return hip_rc(hipGetLastError());
}

// ---------------------------------------------------------------------------------------
// verdict of one line-search trial (or, with init, of the start point), one thread per instance: the chunk partials are
// summed in chunk order -- no floating-point atomics, the same call gives the same bits.  Armijo rule on the residual:
// accept the first finite trial with ||Phi(y + a d)||_2 < (1 - 1e-4 a) ||Phi(y)||_2; converged at ||Phi||_inf <= tol.
// *slot counts the instances that go on searching.
// ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void k_bvp_accept(BvpVerdictArgs a, int init, double step, const int* gate) {
  if (gate && *gate == 0) return;
  const int b = blockIdx.x * 64 + threadIdx.x;
  const size_t B = (size_t)a.batch;
  bool still = false;
  if (b < a.batch && a.search[b] != 0) {
    double ss = 0.0, mx = 0.0;
    for (int q = 0; q < a.nparts; ++q) {
      ss += a.SS[(size_t)q * B + b];
      mx = fmax(mx, a.MX[(size_t)q * B + b]);
    }
    const double nt = sqrt(ss);
    if (init) {
      a.nrm2[b] = nt;
      a.resinf[b] = mx;
      a.search[b] = 0;
      a.status[b] = !isfinite(nt) ? 2 : (mx <= a.tol ? 1 : 0);
    } else if (isfinite(nt) && nt < (1.0 - 1e-4 * step) * a.nrm2[b]) {
      a.nrm2[b] = nt;
      a.resinf[b] = mx;
      a.alpha[b] = step;
      a.search[b] = 0;
      if (mx <= a.tol) a.status[b] = 1;
    } else {
      still = true;
    }
  }
  const unsigned long long m = __ballot(still);
  if ((threadIdx.x & 63) == 0 && m && a.slot) atomicAdd(a.slot, __popcll(m));
}
int launch_bvp_accept(const BvpVerdictArgs& a, bool init, double step, const int* gate, hipStream_t s) {
  k_bvp_accept<<<dim3((a.batch + 63) / 64), dim3(64), 0, s>>>(a, init ? 1 : 0, step, gate);
  return hip_rc(hipGetLastError());
}

// end of iteration `it` (final), or of its first few line-search trials (!final: instances still searching stay as they
// are, the remaining trials follow): an instance whose line search ran out of step lengths, or that is still active after
// max_iter iterations, has failed; *slot counts the instances that go on
__global__ __launch_bounds__(64) void k_bvp_finish(BvpVerdictArgs a, int it, int max_iter, int final) {
  const int b = blockIdx.x * 64 + threadIdx.x;
  bool still = false;
  if (b < a.batch) {
    const bool searching = a.search[b] != 0;
    if (searching && final) {
      a.search[b] = 0;
      a.status[b] = 2;
    }
    if (a.status[b] == 0 && it >= max_iter && !(searching && !final)) a.status[b] = 2;
    a.alpha[b] = 0.0;
    still = a.status[b] == 0;
  }
  const unsigned long long m = __ballot(still);
  if ((threadIdx.x & 63) == 0 && m) atomicAdd(a.slot, __popcll(m));
}
int launch_bvp_finish(const BvpVerdictArgs& a, int it, int max_iter, bool final, hipStream_t s) {
  k_bvp_finish<<<dim3((a.batch + 63) / 64), dim3(64), 0, s>>>(a, it, max_iter, final ? 1 : 0);
  return hip_rc(hipGetLastError());
}

// y += alpha[b] d for the instances whose line search accepted a step (alpha != 0); the expression of k_bvp_norm's trial point
constexpr int kBvpRows = 16;
__global__ __launch_bounds__(256) void k_bvp_update(int rows, int batch, const double* __restrict__ alpha,
                                                    const double* __restrict__ d, double* __restrict__ y) {
  const int b = blockIdx.x * 256 + threadIdx.x;
  if (b >= batch) return;
  const double al = alpha[b];
  if (al == 0.0) return;
  const size_t B = (size_t)batch;
  for (int r0 = blockIdx.y * kBvpRows; r0 < rows; r0 += gridDim.y * kBvpRows) {
    const int r1 = r0 + kBvpRows < rows ? r0 + kBvpRows : rows;
    for (int r = r0; r < r1; ++r) {
      const size_t at = (size_t)r * B + b;
      y[at] = __builtin_fma(al, d[at], y[at]);
    }
  }
}
int launch_bvp_update(int rows, int batch, const double* alpha, const double* d, double* y, hipStream_t s) {
  const int parts = (rows + kBvpRows - 1) / kBvpRows;
  k_bvp_update<<<dim3((batch + 255) / 256, parts < 65535 ? parts : 65535), dim3(256), 0, s>>>(rows, batch, alpha, d, y);
  return hip_rc(hipGetLastError());
}

// start of a solve: every instance active and waiting for the verdict on its start point
__global__ void k_bvp_init(int batch, int* status, int* search, int* iters, double* alpha) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= batch) return;
  status[b] = 0;
  search[b] = 1;
  iters[b] = 0;
  alpha[b] = 0.0;
}
int launch_bvp_init(int batch, int* status, int* search, int* iters, double* alpha, hipStream_t s) {
  k_bvp_init<<<dim3((batch + 255) / 256), dim3(256), 0, s>>>(batch, status, search, iters, alpha);
  return hip_rc(hipGetLastError());
}

// y [npts][2 nS][B] from its halves: rows 0 .. nS-1 from xs (node i: xs[(i ldx + k) B + b]; xs_nodes == 0: the one column
// x0 [nS][B] for every node, bvpinit's constant guess), rows nS .. from lam [npts][nS][B] (NULL: zeros)
__global__ __launch_bounds__(256) void k_bvp_pack(int npts, int nS, int batch, const double* __restrict__ xs, int ldx,
                                                  int xs_nodes, const double* __restrict__ lam, double* __restrict__ y) {
  const int b = blockIdx.x * 256 + threadIdx.x;
  const int i = blockIdx.y;
  if (b >= batch || i >= npts) return;
  const size_t B = (size_t)batch;
  for (int k = 0; k < nS; ++k) {
    y[((size_t)i * 2 * nS + k) * B + b] = xs[((size_t)(xs_nodes ? i : 0) * ldx + k) * B + b];
    y[((size_t)i * 2 * nS + nS + k) * B + b] = lam ? lam[((size_t)i * nS + k) * B + b] : 0.0;
  }
}
int launch_bvp_pack(int npts, int nS, int batch, const double* xs, int ldx, bool xs_nodes, const double* lam, double* y,
                    hipStream_t s) {
  if (npts > 65535) return -1;
  k_bvp_pack<<<dim3((batch + 255) / 256, npts), dim3(256), 0, s>>>(npts, nS, batch, xs, ldx, xs_nodes ? 1 : 0, lam, y);
  return hip_rc(hipGetLastError());
}
// the costate half of y as an array of its own [npts][nS][B] (the layout the control-at-points kernels read)
__global__ __launch_bounds__(256) void k_bvp_costate_rows(int npts, int nS, int batch, const double* __restrict__ y,
                                                          double* __restrict__ lam) {
  const int b = blockIdx.x * 256 + threadIdx.x;
  const int i = blockIdx.y;
  if (b >= batch || i >= npts) return;
  const size_t B = (size_t)batch;
  for (int k = 0; k < nS; ++k) lam[((size_t)i * nS + k) * B + b] = y[((size_t)i * 2 * nS + nS + k) * B + b];
}
int launch_bvp_costate_rows(int npts, int nS, int batch, const double* y, double* lam, hipStream_t s) {
  if (npts > 65535) return -1;
  k_bvp_costate_rows<<<dim3((batch + 255) / 256, npts), dim3(256), 0, s>>>(npts, nS, batch, y, lam);
  return hip_rc(hipGetLastError());
}
__global__ void k_bvp_converged(int batch, const int* __restrict__ status, int* __restrict__ converged) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b < batch) converged[b] = status[b] == 1 ? 1 : 0;
}
int launch_bvp_converged(int batch, const int* status, int* converged, hipStream_t s) {
  k_bvp_converged<<<dim3((batch + 255) / 256), dim3(256), 0, s>>>(batch, status, converged);
  return hip_rc(hipGetLastError());
}

// ---------------------------------------------------------------------------------------
// the two kernels that see the problem
// ---------------------------------------------------------------------------------------
bool bvp_supported(const ProblemDesc& p) {
  if (p.nS < 1 || p.nS > 4 || p.nC < 1 || p.nC > 2) return false;
  return p.functor == Functor::Logistic || p.functor == Functor::User;
}
int bvp_chunks(int N) { return (N + kBvpChunk - 1) / kBvpChunk; }

template <class P>
static void run_bvp(bool assemble, const BvpArgs& a, dim3 grid, hipStream_t s) {
  if (assemble) k_bvp_assemble<P><<<grid, dim3(64), 0, s>>>(a);
  else k_bvp_norm<P><<<grid, dim3(64), 0, s>>>(a);
}
static int launch_bvp(bool assemble, const ProblemDesc& p, const GridDesc& g, const BvpIterate& it, hipStream_t s) {
  if (!bvp_supported(p) || bvp_chunks(g.N) > 65535) return -1;
  const BvpArgs a{g.N, it.batch, g.HT, g.TC, g.TU, p.ps, p.pb, p.pmask, p.lb, p.ub, p.bstride, it.x0, it.y, it.d, it.alpha,
                  it.status, it.search, it.AB, it.SS, it.MX, it.gate};
  const dim3 grid((a.batch + 63) / 64, bvp_chunks(g.N));
  if (p.functor == Functor::User) {
    void* args[] = {(void*)&a};
    return jit_launch(p.user, assemble ? UK_BVP_ASSEMBLE : UK_BVP_NORM, grid, dim3(64), args, s);
  }
  if (!for_logistic<1, 2, 3, 4>(p.nS, [&](auto P) { run_bvp<decltype(P)>(assemble, a, grid, s); })) return -1;
  return hip_rc(hipGetLastError());
}
int launch_bvp_assemble(const ProblemDesc& p, const GridDesc& g, const BvpIterate& a, hipStream_t s) {
  return launch_bvp(true, p, g, a, s);
}
int launch_bvp_norm(const ProblemDesc& p, const GridDesc& g, const BvpIterate& a, hipStream_t s) {
  return launch_bvp(false, p, g, a, s);
}

// ---------------------------------------------------------------------------------------
// the mesh side: residual estimate (its two maxima: launch_interval_reduce, ocs_kernels.hip), prolongation
// ---------------------------------------------------------------------------------------
int launch_bvp_rms(const ProblemDesc& p, const GridDesc& g, int batch, const double* TCL, const double* TUL, const double* y,
                   double* rms, double* PM, hipStream_t s) {
  if (!bvp_supported(p) || bvp_chunks(g.N) > 65535) return -1;
  const BvpRmsArgs a{g.N, batch, g.HT, g.TC, g.TU, TCL, TUL, p.ps, p.pb, p.pmask, p.lb, p.ub, p.bstride, y, rms, PM};
  const dim3 grid((batch + 63) / 64, bvp_chunks(g.N));
  if (p.functor == Functor::User) {
    void* args[] = {(void*)&a};
    return jit_launch(p.user, UK_BVP_RMS, grid, dim3(64), args, s);
  }
  if (!for_logistic<1, 2, 3, 4>(p.nS, [&](auto P) { k_bvp_rms<decltype(P)><<<grid, dim3(64), 0, s>>>(a); })) return -1;
  return hip_rc(hipGetLastError());
}

int launch_bvp_prolong(const ProblemDesc& p, const GridDesc& g, int batch, const double* y, int nnew, const int* idx,
                       const double* theta, double* ynew, hipStream_t s) {
  if (!bvp_supported(p) || nnew < 1 || nnew > 65535) return -1;
  const BvpProlongArgs a{g.N, batch, nnew, g.HT, g.TC, g.TU, p.ps, p.pb, p.pmask, p.lb, p.ub, p.bstride, y, idx, theta, ynew};
  const dim3 grid((batch + 63) / 64, nnew);
  if (p.functor == Functor::User) {
    void* args[] = {(void*)&a};
    return jit_launch(p.user, UK_BVP_PROLONG, grid, dim3(64), args, s);
  }
  if (!for_logistic<1, 2, 3, 4>(p.nS, [&](auto P) { k_bvp_prolong<decltype(P)><<<grid, dim3(64), 0, s>>>(a); })) return -1;
  return hip_rc(hipGetLastError());
}

}  // namespace ocs
