// ocs_xlam_err_kernels.hip -- error estimate of the sweep's pass pair (ocs_x_lam_err): the registry instances of k_xlam_err
// (ocs_xlam_err_device.hpp; hipRTC instances for user problems) and the reduction of its ratios, which does not see the
// problem.
#include "ocs_xlam_err_device.hpp"
#include "ocs_internal.hpp"
#include "ocs_jit.hpp"
#include "ocs_problems.hpp"

namespace ocs {

bool xlam_err_supported(const ProblemDesc& p) {
  if (!vector_shape_ok(p.nS, p.nC)) return false;
  return p.functor == Functor::Logistic || p.functor == Functor::User;
}
int xlam_err_chunks(int N) { return (N + kErrChunk - 1) / kErrChunk; }

int launch_xlam_err(const ProblemDesc& p, const GridDesc& g, const FbsTables& tx, const XlamErrTables& tq, int batch,
                    const double* u, const double* x, int ldx, const double* lam, double rtol, double atol, double* rx,
                    double* rl, double* PM, double* PJ, hipStream_t s) {
  if (!xlam_err_supported(p) || xlam_err_chunks(g.N) > 65535) return -1;
  const PchipTab TG{2 * g.N + 1, g.T, tq.HG, tq.W1G, tq.W2G, nullptr};
  const PchipTab TX{tx.n, tx.TN, tx.HN, tx.W1, tx.W2, tx.IH};
  const XlamErrArgs a{g.N, batch, g.HT, g.TC, tq.TCQ, tq.SQ, TG, TX, tx.TM, p.ps, p.pb, p.pmask, u, x, ldx, lam, rtol, atol,
                      rx, rl, PM, PJ};
  const dim3 grid((batch + 63) / 64, xlam_err_chunks(g.N));
  if (p.functor == Functor::User) {
    void* args[] = {(void*)&a};
    return jit_launch(p.user, UK_XLAM_ERR, grid, dim3(64), args, s);
  }
  if (!for_logistic<1, 2, 3, 4>(p.nS, [&](auto P) { k_xlam_err<decltype(P)><<<grid, dim3(64), 0, s>>>(a); })) return -1;
  return hip_rc(hipGetLastError());
}

// Workgroups 0 .. N-1: rmax[i] = the largest of rx[i][b], rl[i][b] over the instances with use[b] != 0 (use == NULL: all;
// none: 0).  The workgroups behind them, one thread per instance: rinst[b] = the largest of the instance's chunk maxima PM,
// errJ[b] = the sum of its chunk sums PJ in chunk order.  A NaN counts as +inf in both maxima; an instance's NaN reaches
// rmax only where it is in use, and never another instance's rinst or errJ.  Maxima, and one thread's sum in a fixed order: no
// floating-point atomics, the order of the reduction does not show.
__global__ __launch_bounds__(256) void k_xlam_err_reduce(int N, int batch, int nparts, const double* __restrict__ rx,
                                                         const double* __restrict__ rl, const double* __restrict__ PM,
                                                         const double* __restrict__ PJ, const int* __restrict__ use,
                                                         double* __restrict__ rmax, double* __restrict__ rinst,
                                                         double* __restrict__ errJ) {
  const size_t B = (size_t)batch;
  if ((int)blockIdx.x >= N) {
    const int b = (blockIdx.x - N) * 256 + threadIdx.x;
    if (b >= batch) return;
    double m = 0.0, sj = 0.0;
    for (int q = 0; q < nparts; ++q) {
      m = fmax(m, PM[(size_t)q * B + b]);
      sj += PJ[(size_t)q * B + b];
    }
    rinst[b] = m;
    errJ[b] = sj;
    return;
  }
  __shared__ double part[4];
  const double* rowx = rx + (size_t)blockIdx.x * B;
  const double* rowl = rl + (size_t)blockIdx.x * B;
  double m = 0.0;
  for (int b = threadIdx.x; b < batch; b += 256) {
    if (use && use[b] == 0) continue;
    const double vx = rowx[b], vl = rowl[b];
    m = fmax(m, (vx == vx && vl == vl) ? fmax(vx, vl) : __builtin_inf());
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) m = fmax(m, __shfl_xor(m, o, 64));
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = m;
  __syncthreads();
  if (threadIdx.x == 0) rmax[blockIdx.x] = fmax(fmax(part[0], part[1]), fmax(part[2], part[3]));
}
int launch_xlam_err_reduce(int N, int batch, const double* rx, const double* rl, const double* PM, const double* PJ,
                           const int* use, double* rmax, double* rinst, double* errJ, hipStream_t s) {
  k_xlam_err_reduce<<<dim3(N + (batch + 255) / 256), dim3(256), 0, s>>>(N, batch, xlam_err_chunks(N), rx, rl, PM, PJ, use, rmax,
                                                                        rinst, errJ);
  return hip_rc(hipGetLastError());
}

}  // namespace ocs
