// ocs_lq_sweep_kernels.hip -- the costate pass of the forward-backward sweep (functions/fb_sweep.m, compute_x_lam.m) for the
// build-defined LQ problem on the gfx950 matrix cores, and the launchers of both of the sweep's passes.  Its state pass is
// the integrator's one-wave kernel, k_lq_forward<RT, true, false> of ocs_lq_kernels.hip (compute_x_lam_J.m:6-15 on the grid
// is RK4Integrator.m:28-56), in the instantiation that honours the sweep's frozen and gate (SWEEP).
//
// Mapping "M" of ocs_lq_kernels.hip: one wave per 16 trajectories, lane (g, n) = (lane >> 4, lane & 15) owns rows
// {4m + g} of trajectory n for the whole pass; A' sits in registers as A-operand fragments of v_mfma_f64_16x16x4_f64, the
// stage vector is the B operand, and the C/D layout of one product is the B-operand layout of the next.  RT = 1 row tile
// for nS <= 16, RT = 2 for nS <= 32.
//
// What the sweep asks of a pass beyond the integrator's: a device gate (a sweep enqueued ahead of the host's knowledge
// that the one before it left no instance active does nothing), and frozen instances (converged in an earlier sweep:
// integrated along, nothing stored).  A lane is switched off for stores by a buffer offset past num_records (kOffDrop),
// so neither needs a branch in the recursion nor a scratch array for the stores of frozen instances.
//
// The control-update, error-point and bookkeeping kernels of the sweep stay those of the problem's plugin twin
// (ocs_fbs.cpp sweep_problem).
#include "ocs_device_common.hpp"
#include "ocs_internal.hpp"
#include "ocs_lq_core.hpp"
#include "ocs_scan_kernel.hpp"   // Buf: raw buffer accesses with scalar offsets

namespace ocs {

struct LQSweepArgs {
  int N, batch, nS, nC;
  const double* REC;     // StepRec<1> records of the LQ problem: e^{-rt} at A / M / B
  const double* ps;      // [r | A nS x nS col-major | Bu nS x nC | q nS | rdiag nC]
  const double* x;       // [N+1][ldx][B]
  int ldx;               // rows per column of x (nS + 1)
  const double* xmid;    // pchip midpoints of x [N][nS][B] (launch_pchip_mid)
  double* lam;           // out [N+1][nS][B]
  const int* frozen;     // optional [B]: instances with frozen[b] != 0 store nothing
  const int* gate;       // optional: the launch does nothing if *gate == 0
};

// ---------------------------------------------------------------------------------------
// costate pass   compute_x_lam.m:4,11-14: lam' = -(A' lam + 2 e^{-rt} q .* x), lam(TF) = 0
// ---------------------------------------------------------------------------------------
// Classical RK4 with step -h from node i+1 to node i; stage order, FMA forms and the constants {h, h/2, h/6} are those
// of k_costate (ocs_fbs_device.hpp): k1 at (tB, xB, l), k2 and k3 at (tM, xM, .), k4 at (tA, xA, .).  The kernel carries
// G = A' L + 2 e^{-rt} q .* x = -k, an exact negation, so  L = fma(-h/2, k1, l) = fma(h/2, G1, l)  bit for bit, and
// the same for the step's sum.  The forcing term is the accumulator's start value, as Bu u is in LQCore::Fx; k2 and k3
// share theirs.  dFdx of this problem has no u in it: the control samples are not read.
template <int RT>
__global__ __launch_bounds__(64) void k_lq_sweep_costate(const LQSweepArgs a) {
  if (a.gate && *a.gate == 0) return;
  constexpr int KS = 4 * RT;
  using Rec = StepRec<1>;
  const int lane = threadIdx.x, g = lane >> 4, n = lane & 15;
  const int b0 = blockIdx.x * 16 + n;
  const int b = b0 < a.batch ? b0 : a.batch - 1;  // lanes past the batch recompute the last trajectory
  const size_t B = (size_t)a.batch;
  const int nS = a.nS, N = a.N;
  const size_t xcol = (size_t)a.ldx * B, lcol = (size_t)nS * B;
  const bool keep = b0 < a.batch && !(a.frozen && a.frozen[b] != 0);

  LQMat<RT> AT;  // fragments of A'
  load_frags<RT, true>(AT, a.ps + 1, nS, nS, nS, g, n);
  double q[KS];  // q[4m + g]
  {
    const double* qq = a.ps + 1 + (size_t)nS * nS + (size_t)nS * a.nC;
#pragma unroll
    for (int m = 0; m < KS; ++m) q[m] = (4 * m + g < nS) ? qq[4 * m + g] : 0.0;
  }
  // per-lane byte offset of (row 4m + g, trajectory b) inside a column of x, xmid or lam: loads of padded rows are
  // dropped (they return 0), stores also those of frozen instances and of lanes past the batch
  unsigned vld[KS], vst[KS];
#pragma unroll
  for (int m = 0; m < KS; ++m) {
    vld[m] = (4 * m + g < nS) ? (unsigned)(((size_t)(4 * m + g) * B + b) * 8) : kOffDrop;
    vst[m] = keep ? vld[m] : kOffDrop;
  }
  // G = A' L + 2 e (q .* x)
  auto rhs = [&](const double (&L)[KS], const double (&x)[KS], double e, double (&G)[KS]) OCS_INLINE {
    const double e2 = 2.0 * e;
    d4 acc[RT];
#pragma unroll
    for (int rt = 0; rt < RT; ++rt) {
      acc[rt].x = (e2 * q[4 * rt + 0]) * x[4 * rt + 0];
      acc[rt].y = (e2 * q[4 * rt + 1]) * x[4 * rt + 1];
      acc[rt].z = (e2 * q[4 * rt + 2]) * x[4 * rt + 2];
      acc[rt].w = (e2 * q[4 * rt + 3]) * x[4 * rt + 3];
    }
    matvec<RT>(AT, L, acc);
    unpack<RT>(acc, G);
  };

  double l[KS], xB[KS], xM[KS], xA[KS];
  {
    const Buf bl = Buf::make(a.lam + (size_t)N * lcol);
    const Buf bxB = Buf::make(a.x + (size_t)N * xcol), bxA = Buf::make(a.x + (size_t)(N - 1) * xcol);
    const Buf bxM = Buf::make(a.xmid + (size_t)(N - 1) * lcol);
#pragma unroll
    for (int m = 0; m < KS; ++m) {
      l[m] = 0.0;  // lam0 = 0*x0   compute_x_lam.m:4
      bl.st0(0.0, vst[m], 0);
      xB[m] = bxB.ld(vld[m], 0);
      xM[m] = bxM.ld(vld[m], 0);
      xA[m] = bxA.ld(vld[m], 0);
    }
  }
  const double* recp = a.REC + (size_t)(N - 1) * rec_stride(1);
  Rec cur = load_rec<1>(recp);
  for (int i = N - 1; i >= 0; --i) {
    // the record and the states of step i-1 are requested now and consumed a step later
    recp -= rec_stride(1);
    const Rec nxt = load_rec<1>(recp);  // the table is padded before step 0
    const int ip = i > 0 ? i - 1 : 0;
    const Buf bxA = Buf::make(a.x + (size_t)ip * xcol), bxM = Buf::make(a.xmid + (size_t)ip * lcol);
    double xAn[KS], xMn[KS];
#pragma unroll
    for (int m = 0; m < KS; ++m) {
      xAn[m] = bxA.ld(vld[m], 0);
      xMn[m] = bxM.ld(vld[m], 0);
    }
    double G1[KS], G2[KS], G3[KS], G4[KS], L[KS];
    rhs(l, xB, cur.tcB[0], G1);
#pragma unroll
    for (int m = 0; m < KS; ++m) L[m] = __builtin_fma(cur.hh, G1[m], l[m]);
    rhs(L, xM, cur.tcM[0], G2);
#pragma unroll
    for (int m = 0; m < KS; ++m) L[m] = __builtin_fma(cur.hh, G2[m], l[m]);
    rhs(L, xM, cur.tcM[0], G3);
#pragma unroll
    for (int m = 0; m < KS; ++m) L[m] = __builtin_fma(cur.h, G3[m], l[m]);
    rhs(L, xA, cur.tcA[0], G4);
#pragma unroll
    for (int m = 0; m < KS; ++m)
      l[m] = __builtin_fma(cur.h6, __builtin_fma(2.0, G3[m], __builtin_fma(2.0, G2[m], G1[m])) + G4[m], l[m]);
    const Buf bl = Buf::make(a.lam + (size_t)i * lcol);
#pragma unroll
    for (int m = 0; m < KS; ++m) {
      bl.st0(l[m], vst[m], 0);
      xB[m] = xA[m];
      xA[m] = xAn[m];
      xM[m] = xMn[m];
    }
    cur = nxt;
  }
}

// ---------------------------------------------------------------------------------------
// launchers
// ---------------------------------------------------------------------------------------
static bool lq_sweep_shape_ok(const ProblemDesc& p, const GridDesc& g, int batch) {
  // (32-bit byte offsets from a buffer base: one column of x is (nS + 1) batch doubles; the state pass reaches three grid
  //  columns of u, 3 nC batch doubles, from the base of the first)
  const size_t rows = (size_t)(p.nS + 1) > (size_t)(3 * p.nC) ? (size_t)(p.nS + 1) : (size_t)(3 * p.nC);
  return p.functor == Functor::LQ && lq_supported(p.nS, p.nC) && !p.pmask && g.N >= 1 && g.REC && batch >= 1 &&
         rows * (size_t)batch * 8 < (size_t)kNumRec;
}

int launch_sweep_forward_lq(const ProblemDesc& p, const GridDesc& g, int batch, const double* x0, const double* u,
                            double* x, double* J, const int* frozen, const int* gate, hipStream_t s) {
  if (!lq_sweep_shape_ok(p, g, batch) || !x0 || !u || !x || !J) return -1;
  LQArgs a{};
  a.N = g.N; a.batch = batch; a.nS = p.nS; a.nC = p.nC; a.REC = g.REC; a.ps = p.ps;
  a.x0 = x0; a.u = u; a.x = x; a.J = J; a.frozen = frozen; a.gate = gate;
  lq_forward_one_wave(a, s);
  return hip_rc(hipGetLastError());
}

int launch_sweep_costate_lq(const ProblemDesc& p, const GridDesc& g, int batch, const double* x, int ldx,
                            const double* xmid, const int* frozen, double* lam, const int* gate, hipStream_t s) {
  if (!lq_sweep_shape_ok(p, g, batch) || !x || !xmid || !lam || ldx != p.nS + 1) return -1;
  LQSweepArgs a{};
  a.N = g.N; a.batch = batch; a.nS = p.nS; a.nC = p.nC; a.REC = g.REC; a.ps = p.ps;
  a.x = x; a.ldx = ldx; a.xmid = xmid; a.lam = lam; a.frozen = frozen; a.gate = gate;
  const dim3 grid((batch + 15) / 16), block(64);
  if (p.nS <= 16)
    k_lq_sweep_costate<1><<<grid, block, 0, s>>>(a);
  else
    k_lq_sweep_costate<2><<<grid, block, 0, s>>>(a);
  return hip_rc(hipGetLastError());
}

}  // namespace ocs
