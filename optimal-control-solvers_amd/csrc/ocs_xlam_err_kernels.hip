// ocs_xlam_err_kernels.hip -- error estimate of the sweep's pass pair (ocs_x_lam_err): the registry instances of k_xlam_err
// (ocs_xlam_err_device.hpp; hipRTC instances for user problems).  The reduction of its ratios does not see the problem:
// launch_interval_reduce, ocs_kernels.hip.
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

}  // namespace ocs
