// ocs_lq_kernels.hip -- gfx950 matrix-core kernels for problems whose dynamics are linear with a
// Jacobian shared by the whole batch (the build-defined LQ problem of BASELINE config 5):
//
//   F(t,[x;.],u) = [ A x + Bu u ;  e^{-rt} ( sum_k q_k x_k^2 + sum_c R_c u_c^2 ) ]
//   dFdx_times_vec = [ A' v_x + 2 e^{-rt} (q .* x) v_last ; 0 ]
//   dFdu_times_vec =   Bu' v_x + 2 e^{-rt} (R .* u) v_last
//
// (the OCProblem plugin contract of OCProblem/OCProblem.m:8-21; same parameter block
// [r | A | Bu | q | rdiag] as oracle/ocs_oracle.c).  The RK4 recursion and its discrete adjoint are
// those of Integrator/RK4Integrator.m:28-56, :59-94, :97-121.
//
// Mapping ("M"): one wave integrates 16 trajectories.  Every stage evaluation A*Y is a
// (16 RT x 16 RT) x (16 RT x 16) product done with v_mfma_f64_16x16x4_f64: A sits in registers as
// MFMA A-operand fragments for the whole kernel (RT * 4RT fragments, one double per lane each), the
// stage state Y is the B operand.  The C/D layout of that instruction (lane (g, n) = (lane>>4, lane&15)
// holds rows g + 4j of column n) is exactly its B-operand layout for k-step j, so the result of one
// stage feeds the next stage's product without leaving the registers: lane (g, n) owns rows
// {4m + g} of trajectory n for the whole pass.  Bu*u is one more k-step (nC <= 4 = K).
// The adjoint pass recomputes Y2..Y4 from the checkpoint y_i with the same instruction sequence
// (bit-identical to the forward pass) and runs the four A'k products on the transposed fragments.
#include "ocs_device_common.hpp"
#include "ocs_internal.hpp"
#include "ocs_lq_core.hpp"       // mma, LQMat, load_frags, matvec, LQCore, LQArgs, LQTime
#include "ocs_rk4_kernels.hpp"
#include "ocs_scan_kernel.hpp"   // Buf: raw buffer accesses with scalar offsets
#include <cstdlib>
#include <vector>

namespace ocs {

int launch_tcoef_lq(const ProblemDesc& p, const GridDesc& g, hipStream_t s) {
  const int nT = 2 * g.N + 1;
  k_tcoef<LQTime><<<dim3((nT + 255) / 256), dim3(256), 0, s>>>(nT, g.T, p.ps, g.TC, g.TU);
  k_build_rec<LQTime><<<dim3((g.N + 2 * kRecPad + 255) / 256), dim3(256), 0, s>>>(g.N, g.HT, g.TC, g.REC);
  return hip_rc(hipGetLastError());
}

// ---------------------------------------------------------------------------------------
// forward pass   RK4Integrator.m:28-56
// ---------------------------------------------------------------------------------------
// CH (time-parallel passes, see "chunked passes" below): 0 the whole horizon from x0; 1 the chunk blockIdx.y from the
// start state cs[c], no objective, no trajectory: only the state at the chunk's last node -> ce[c]; 2 the chunk from
// cs[c] with every output of its steps, the running objective counted from the chunk's first node (its total -> cj[c]).
// PW (every integrator pass below): q and rdiag are this lane's trajectory's own, read from a.W in the prologue
// (ocs_problem_set_batch_params on the weight range); the time loop is the same.
// SWEEP: fb_sweep's state pass (lq_forward_one_wave), which honours a.gate and a.frozen (ocs_lq_sweep_kernels.hip says what
// they ask); a lane is switched off for stores by a buffer offset past num_records (kOffDrop): no branch in the recursion.
// The integrator's instantiations do not read the two: with the tests in them the one-wave state pass at batch 16 384
// (2 x 4000 steps) took 19.5 ms instead of 18.9, the time loop the same instructions in another order.
template <int RT, bool OUT_X, bool UCONST, int CH = 0, bool PW = false, bool SWEEP = false>
__global__ __launch_bounds__(64) void k_lq_forward(const LQArgs a) {
  if constexpr (SWEEP) {
    if (a.gate && *a.gate == 0) return;
  }
  constexpr int KS = 4 * RT;
  using Rec = StepRec<1>;
  const int lane = threadIdx.x, g = lane >> 4, n = lane & 15;
  const int b0 = blockIdx.x * 16 + n;
  const int b = b0 < a.batch ? b0 : a.batch - 1;  // lanes past the batch recompute the last trajectory
  const size_t B = (size_t)a.batch;
  const int nS = a.nS, nC = a.nC, N = a.N;
  const size_t nAugB = (size_t)(nS + 1) * B;
  const int ch = CH ? (int)blockIdx.y : 0;
  const int i0 = CH ? ch * a.L : 0, i1 = CH ? (i0 + a.L < N ? i0 + a.L : N) : N;
  // this lane's trajectory is stored (the integrator also stores what tail lanes recompute: the same values)
  const bool keep = !SWEEP || (b0 < a.batch && !(a.frozen && a.frozen[b] != 0));

  LQCore<RT> P;
  P.load(a.ps, nS, nC, g, n);
  if constexpr (PW) P.load_weights(a.W, B, b, nS, nC, g);

  double y[KS], yc = 0.0;  // xK(:,1,1) = [x0; 0]   :33
  {
    const double* ys = CH ? a.cs + (size_t)ch * nS * B : a.x0;
#pragma unroll
    for (int m = 0; m < KS; ++m) y[m] = (4 * m + g < nS) ? ys[(size_t)(4 * m + g) * B + b] : 0.0;
  }

  // (global accesses through raw buffer descriptors built per column on the scalar unit, per-lane byte offsets fixed for
  //  the pass: no 64-bit vector address arithmetic on the pipe the matrix instructions need -- see k_lq2_forward)
  unsigned vrow[KS];
#pragma unroll
  for (int m = 0; m < KS; ++m) vrow[m] = (keep && 4 * m + g < nS) ? (unsigned)(((size_t)(4 * m + g) * B + b) * 8) : kOffDrop;
  const unsigned vcost = (keep && g == 0) ? (unsigned)(((size_t)nS * B + b) * 8) : kOffDrop;
  auto store_x = [&](int col) OCS_INLINE {
    if (!OUT_X) return;
    const Buf bx = Buf::make(a.x + (size_t)col * nAugB);
#pragma unroll
    for (int m = 0; m < KS; ++m) bx.st0(y[m], vrow[m], 0);
    bx.st0(yc, vcost, 0);
  };
  if (!CH || ch == 0) store_x(0);

  const bool uact = g < nC;
  const size_t ustride = (size_t)nC * B;
  const double* up = a.u + (UCONST ? 0 : (size_t)(2 * i0) * ustride) + (size_t)(uact ? g : 0) * B + b;  // u(:, 2 i0 + 1) of this lane's control row
  const unsigned vu = (unsigned)(((size_t)(uact ? g : 0) * B + b) * 8), us8 = (unsigned)(ustride * 8);
  double uA = UCONST ? (uact ? lq_uconst(a, g, b) : 0.0) : (uact ? *up : 0.0);
  d4 buA[RT], buM[RT], buB[RT];
  P.bu_times(uA, buA);
  if (UCONST) {
#pragma unroll
    for (int rt = 0; rt < RT; ++rt) buM[rt] = buB[rt] = buA[rt];
  }

  const double* recp = a.REC + (size_t)i0 * rec_stride(1);
  Rec cur = load_rec<1>(recp);
  double uM = uA, uB = uA;
  if (!UCONST) {
    uM = uact ? up[ustride] : 0.0;
    uB = uact ? up[2 * ustride] : 0.0;
  }
  for (int i = i0; i < i1; ++i) {
    // next step's uniform record and control samples are requested now and consumed a step later
    recp += rec_stride(1);
    const Rec nxt = load_rec<1>(recp);  // the table is padded past step N-1
    double uMn = uM, uBn = uB;
    if (!UCONST) {
      const int in = i + 1 < N ? i + 1 : i;
      const Buf bu = Buf::make(a.u + (size_t)(2 * in) * ustride);
      const double vM = bu.ld(vu, us8), vB = bu.ld(vu, 2 * us8);  // unused control rows read row 0 and are zeroed
      uMn = uact ? vM : 0.0;
      uBn = uact ? vB : 0.0;
      P.bu_times(uM, buM);
      P.bu_times(uB, buB);
    }
    double F1[KS], F2[KS], F3[KS], F4[KS], Y[KS];
    P.Fx(y, buA, F1);                                                         // :37
    double cs = 0.0;
    if (CH != 1) cs = P.cost_part(y, uA, cur.tcA[0]);
#pragma unroll
    for (int m = 0; m < KS; ++m) Y[m] = __builtin_fma(cur.hh, F1[m], y[m]);   // :40
    P.Fx(Y, buM, F2);                                                         // :41
    if (CH != 1) cs += 2.0 * P.cost_part(Y, uM, cur.tcM[0]);
#pragma unroll
    for (int m = 0; m < KS; ++m) Y[m] = __builtin_fma(cur.hh, F2[m], y[m]);   // :44
    P.Fx(Y, buM, F3);                                                         // :45
    if (CH != 1) cs += 2.0 * P.cost_part(Y, uM, cur.tcM[0]);
#pragma unroll
    for (int m = 0; m < KS; ++m) Y[m] = __builtin_fma(cur.h, F3[m], y[m]);    // :48
    P.Fx(Y, buB, F4);                                                         // :49
    if (CH != 1) cs += P.cost_part(Y, uB, cur.tcB[0]);
#pragma unroll
    for (int m = 0; m < KS; ++m)                                              // :50
      y[m] = __builtin_fma(cur.h6, (F1[m] + 2.0 * F2[m]) + (2.0 * F3[m] + F4[m]), y[m]);
    if (CH != 1) yc = __builtin_fma(cur.h6, sum_over_g(cs), yc);
    store_x(i + 1);
    cur = nxt;
    uA = uB;
    uM = uMn;
    uB = uBn;
#pragma unroll
    for (int rt = 0; rt < RT; ++rt) buA[rt] = buB[rt];
  }
  if (CH == 0) {
    if (keep && g == 0) a.J[b] = a.Jadd ? a.Jadd[b] + yc : yc;  // J = x(end,end)   :55
  } else if (CH == 1) {
    double* ye = a.ce + (size_t)ch * nS * B;
#pragma unroll
    for (int m = 0; m < KS; ++m)
      if (4 * m + g < nS && b0 < a.batch) ye[(size_t)(4 * m + g) * B + b] = y[m];
  } else {
    if (g == 0 && b0 < a.batch) a.cj[(size_t)ch * B + b] = yc;
  }
}

// ---------------------------------------------------------------------------------------
// adjoint pass   RK4Integrator.m:59-121
// ---------------------------------------------------------------------------------------
// CH: 0 the whole horizon from lamT; 1 the chunk blockIdx.y from a zero costate at its last node (the objective row keeps
// its constant value), no outputs but the costate at the chunk's first node -> ce[c] (the part of the affine chunk map
// lam_lo = M' lam_hi + b that does not depend on lam_hi); 2 the chunk from cs[c] with every output of its steps; the k1
// half of its first node column of dJdu, which belongs to the column the chunk below writes, goes to cj[c].
template <int RT, bool OUT_LAM, bool OUT_DJDU, bool UCONST, int CH = 0, bool PW = false>
__global__ __launch_bounds__(64) void k_lq_backward(const LQArgs a) {
  constexpr int KS = 4 * RT;
  using Rec = StepRec<1>;
  const int lane = threadIdx.x, g = lane >> 4, n = lane & 15;
  const int b0 = blockIdx.x * 16 + n;
  const int b = b0 < a.batch ? b0 : a.batch - 1;
  const size_t B = (size_t)a.batch;
  const int nS = a.nS, nC = a.nC;
  const int ch = CH ? (int)blockIdx.y : 0;
  const int i0 = CH ? ch * a.L : 0;
  const int N = CH ? (i0 + a.L < a.N ? i0 + a.L : a.N) : a.N;   // the last node of the pass / of the chunk
  const size_t nAugB = (size_t)(nS + 1) * B;

  LQCore<RT> P;
  P.load(a.ps, nS, nC, g, n);
  if constexpr (PW) P.load_weights(a.W, B, b, nS, nC, g);
  LQMat<RT> AT;  // fragments of A'
  load_frags<RT, true>(AT, a.ps + 1, nS, nS, nS, g, n);
  double BuT[KS];  // A-operand fragments of Bu' (nC x nS, rows padded to 16): lane (g,i) <- Bu[4 kk + g][i]
  {
    const double* bu = a.ps + 1 + (size_t)nS * nS;
#pragma unroll
    for (int kk = 0; kk < KS; ++kk) BuT[kk] = (4 * kk + g < nS && n < nC) ? bu[(4 * kk + g) + (size_t)nS * n] : 0.0;
  }
  // (Bu' v)_g of trajectory n lands in register 0 of lane (g, n)
  auto but_times = [&](const double (&v)[KS]) OCS_INLINE {
    d4 acc = {0.0, 0.0, 0.0, 0.0}, alt = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int kk = 0; kk < KS; kk += 2) {
      acc = mma(BuT[kk], v[kk], acc);
      alt = mma(BuT[kk + 1], v[kk + 1], alt);
    }
    return acc.x + alt.x;
  };
  // A' k + 2 e (q .* Y) k_last
  auto ATx = [&](const double (&k)[KS], const double (&Y)[KS], double e2kl, double (&gout)[KS]) OCS_INLINE {
    d4 acc[RT];
#pragma unroll
    for (int rt = 0; rt < RT; ++rt) {
      acc[rt].x = P.q[4 * rt + 0] * Y[4 * rt + 0] * e2kl;
      acc[rt].y = P.q[4 * rt + 1] * Y[4 * rt + 1] * e2kl;
      acc[rt].z = P.q[4 * rt + 2] * Y[4 * rt + 2] * e2kl;
      acc[rt].w = P.q[4 * rt + 3] * Y[4 * rt + 3] * e2kl;
    }
    matvec<RT>(AT, k, acc);
    unpack<RT>(acc, gout);
  };

  double lam[KS], lamc;  // lam(:,end) = lamT   :69; the last row of dFdx_times_vec is 0, so lam(end,:) is constant
  if (CH == 2) {
    const double* ls = a.cs + (size_t)ch * nS * B;
#pragma unroll
    for (int m = 0; m < KS; ++m) lam[m] = (4 * m + g < nS) ? ls[(size_t)(4 * m + g) * B + b] : 0.0;
  } else {
#pragma unroll
    for (int m = 0; m < KS; ++m) lam[m] = (CH == 0 && a.lamT && 4 * m + g < nS) ? a.lamT[(size_t)(4 * m + g) * B + b] : 0.0;
  }
  lamc = a.lamT ? a.lamT[(size_t)nS * B + b] : 1.0;

  unsigned vrow[KS];   // (raw buffer descriptors per column: see k_lq_forward)
#pragma unroll
  for (int m = 0; m < KS; ++m) vrow[m] = (4 * m + g < nS) ? (unsigned)(((size_t)(4 * m + g) * B + b) * 8) : kOffDrop;
  const unsigned vlamc = (g == 0) ? (unsigned)(((size_t)nS * B + b) * 8) : kOffDrop;
  auto store_lam = [&](int col) OCS_INLINE {
    if (!OUT_LAM) return;
    const Buf bl = Buf::make(a.lam + (size_t)col * nAugB);
#pragma unroll
    for (int m = 0; m < KS; ++m) bl.st0(lam[m], vrow[m], 0);
    bl.st0(lamc, vlamc, 0);
  };
  if (!CH || N == a.N) store_lam(N);

  const bool uact = g < nC;
  const size_t ustride = (size_t)nC * B;
  const size_t uoff = (size_t)(uact ? g : 0) * B + b;
  const double* up = a.u + uoff;
  double* dq = a.dJdu + uoff;
  const unsigned vu = (unsigned)(uoff * 8), us8 = (unsigned)(ustride * 8), vdq = uact ? vu : kOffDrop;
  double uB = UCONST ? (uact ? lq_uconst(a, g, b) : 0.0) : (uact ? up[(size_t)(2 * N) * ustride] : 0.0);
  double uA = uB, uM = uB;
  d4 buA[RT], buM[RT];
  P.bu_times(uB, buA);
#pragma unroll
  for (int rt = 0; rt < RT; ++rt) buM[rt] = buA[rt];

  double k1c[KS], k1lc = 0.0;  // k1 of step i+1 (the other half of the node column of dJdu, :108-112)
#pragma unroll
  for (int m = 0; m < KS; ++m) k1c[m] = 0.0;

  const double* recp = a.REC + (size_t)(N - 1) * rec_stride(1);
  const double* ckp = a.xck + (size_t)(N - 1) * nAugB + (size_t)g * B + b;
  Rec cur = load_rec<1>(recp);
  double y[KS];
#pragma unroll
  for (int m = 0; m < KS; ++m) y[m] = (4 * m + g < nS) ? ckp[(size_t)(4 * m) * B] : 0.0;
  if (!UCONST) {
    uA = uact ? up[(size_t)(2 * N - 2) * ustride] : 0.0;
    uM = uact ? up[(size_t)(2 * N - 1) * ustride] : 0.0;
  }
  double eA0 = cur.tcA[0];

  for (int i = N - 1; i >= i0; --i) {
    // requests for step i-1 (consumed at the end of this iteration)
    recp -= rec_stride(1);
    const Rec nxt = load_rec<1>(recp);  // the table is padded before step 0
    const int ip = i > 0 ? i - 1 : 0;
    const Buf bc = Buf::make(a.xck + (size_t)ip * nAugB);   // (a dropped access returns 0: the padded rows)
    double yn[KS];
#pragma unroll
    for (int m = 0; m < KS; ++m) yn[m] = bc.ld(vrow[m], 0);
    double uAn = uA, uMn = uM;
    if (!UCONST) {
      const Buf bu = Buf::make(a.u + (size_t)(2 * ip) * ustride);
      const double vA = bu.ld(vu, 0), vM = bu.ld(vu, us8);
      uAn = uact ? vA : 0.0;
      uMn = uact ? vM : 0.0;
      P.bu_times(uA, buA);
      P.bu_times(uM, buM);
    }
    // recompute the stage states (same instruction sequence as the forward pass)
    double F[KS], Y2[KS], Y3[KS], Y4[KS];
    P.Fx(y, buA, F);
#pragma unroll
    for (int m = 0; m < KS; ++m) Y2[m] = __builtin_fma(cur.hh, F[m], y[m]);
    P.Fx(Y2, buM, F);
#pragma unroll
    for (int m = 0; m < KS; ++m) Y3[m] = __builtin_fma(cur.hh, F[m], y[m]);
    P.Fx(Y3, buM, F);
#pragma unroll
    for (int m = 0; m < KS; ++m) Y4[m] = __builtin_fma(cur.h, F[m], y[m]);

    double k4[KS], k3[KS], k2[KS], k1[KS], g3[KS], g2[KS], g1[KS], g0[KS];
    const double k4l = cur.h6 * lamc, k3l = cur.h3 * lamc, k2l = k3l, k1l = k4l;
#pragma unroll
    for (int m = 0; m < KS; ++m) k4[m] = cur.h6 * lam[m];                              // :73
    ATx(k4, Y4, 2.0 * cur.tcB[0] * k4l, g3);                                            // :74
#pragma unroll
    for (int m = 0; m < KS; ++m) k3[m] = __builtin_fma(cur.h, g3[m], cur.h3 * lam[m]);  // :77
    ATx(k3, Y3, 2.0 * cur.tcM[0] * k3l, g2);                                            // :78
#pragma unroll
    for (int m = 0; m < KS; ++m) k2[m] = __builtin_fma(cur.hh, g2[m], cur.h3 * lam[m]); // :81
    ATx(k2, Y2, 2.0 * cur.tcM[0] * k2l, g1);                                            // :82
#pragma unroll
    for (int m = 0; m < KS; ++m) k1[m] = __builtin_fma(cur.hh, g1[m], cur.h6 * lam[m]); // :85
    ATx(k1, y, 2.0 * cur.tcA[0] * k1l, g0);                                             // :86-88

    if (OUT_DJDU) {
      // dFdu_times_vec is linear in v and does not read y for this problem, so the two terms of a
      // column (:104-106 midpoint, :108-112 node) are one product of the summed multipliers
      double v[KS];
#pragma unroll
      for (int m = 0; m < KS; ++m) v[m] = k4[m] + k1c[m];
      const double dn = but_times(v) + 2.0 * cur.tcB[0] * P.R * uB * (k4l + k1lc);
#pragma unroll
      for (int m = 0; m < KS; ++m) v[m] = k2[m] + k3[m];
      const double dm = but_times(v) + 2.0 * cur.tcM[0] * P.R * uM * (k2l + k3l);
      const Buf bd = Buf::make(a.dJdu + (size_t)(2 * i + 1) * ustride);
      bd.st0(dn, vdq, us8);
      bd.st0(dm, vdq, 0);
#pragma unroll
      for (int m = 0; m < KS; ++m) k1c[m] = k1[m];
      k1lc = k1l;
    }
#pragma unroll
    for (int m = 0; m < KS; ++m) lam[m] = (((lam[m] + g1[m]) + g2[m]) + g3[m]) + g0[m];  // :86-88
    store_lam(i);

    eA0 = cur.tcA[0];
    cur = nxt;
    uB = uA;
    uA = uAn;
    uM = uMn;
#pragma unroll
    for (int m = 0; m < KS; ++m) y[m] = yn[m];
  }
  if (OUT_DJDU) {  // first column: B(t_1, y_1, u_1)' k1_1   :100-101   (uB now holds u(:,1))
    const double d0 = but_times(k1c) + 2.0 * eA0 * P.R * uB * k1lc;
    if (CH == 2 && ch > 0) {   // the k1 half of column 2 i0: the chunk below writes that column (its k4 half)
      if (uact && b0 < a.batch) a.cj[((size_t)ch * nC + g) * B + b] = d0;
    } else if (uact) {
      dq[0] = d0;
    }
  }
  if (CH == 1) {
    double* le = a.ce + (size_t)ch * nS * B;
#pragma unroll
    for (int m = 0; m < KS; ++m)
      if (4 * m + g < nS && b0 < a.batch) le[(size_t)(4 * m + g) * B + b] = lam[m];
  }
  if (a.lam0 && CH != 1 && (CH == 0 || ch == 0)) {
#pragma unroll
    for (int m = 0; m < KS; ++m)
      if (4 * m + g < nS) a.lam0[(size_t)(4 * m + g) * B + b] = lam[m];
    if (g == 0) a.lam0[(size_t)nS * B + b] = lamc;
  }
}

// ---------------------------------------------------------------------------------------
// Mapping "M2": two waves per 16 trajectories (17 <= nS <= 32)
// ---------------------------------------------------------------------------------------
// With one wave per 16 trajectories a batch of 8192 occupies 512 of the 1024 SIMDs.  Here a pair of waves
// shares 16 trajectories (a 256-thread workgroup holds two independent pairs, so that one workgroup
// spreads over the four SIMDs of a CU: two 128-thread workgroups on a CU were observed to share
// SIMDs 0 and 1).  Wave w of a pair owns row tile w of every product: its accumulator holds rows 16w + g + 4j, it
// keeps only its half of the stage state up to date and receives the partner's half through LDS
// (4 doubles per lane per stage, two ping-pong slots, one s_barrier per exchange).  The k-steps that
// multiply the wave's own half are issued between posting it and fetching the partner's, so the LDS
// round trip runs under matrix-core work.  The adjoint needs the partner's half of Y2, Y3 (recompute)
// and of k3, k2, k1, lam; A'k's elementwise term 2 e^{-rt} (q .* Y) k_last and the Bu'k products only
// touch own rows (the latter are K-split: each wave contracts its 16 rows, wave 0 adds the two parts).
typedef double d2 __attribute__((ext_vector_type(2)));
constexpr int kX2Pair = 64, kX2Wave = 3 * kX2Pair, kX2Slot = 2 * kX2Wave;  // d2 units

__device__ static inline void lq_lds_barrier() {
  __builtin_amdgcn_sched_barrier(0);
  lds_barrier();
  __builtin_amdgcn_sched_barrier(0);
}

struct LQ2Pending {
  d2 a, b, c;
};
struct LQ2X {
  d2* mine;
  const d2* theirs;
  int tog;
  __device__ inline void init(d2* xb, int w, int lane) {
    mine = xb + w * kX2Wave + lane;
    theirs = xb + (1 - w) * kX2Wave + lane;
    tog = 0;
  }
  // An exchange is three calls with matrix-core work in between, so that the LDS round trip never has the
  // matrix pipe idle: post (ds_write) -> [first product of the own half] -> sync (barrier + ds_read issue)
  // -> [rest of the own half, any independent vector work] -> take (the partner's values).
  template <bool EXTRA>
  __device__ inline void post(const double (&own)[4], double e0 = 0.0, double e1 = 0.0) {
    d2* p = mine + tog;
    p[0] = d2{own[0], own[1]};
    p[kX2Pair] = d2{own[2], own[3]};
    if (EXTRA) p[2 * kX2Pair] = d2{e0, e1};
    __builtin_amdgcn_sched_barrier(0);
  }
  template <bool EXTRA>
  __device__ inline LQ2Pending sync() {
    lq_lds_barrier();
    const d2* p = theirs + tog;
    LQ2Pending r;
    r.a = p[0];
    r.b = p[kX2Pair];
    r.c = EXTRA ? p[2 * kX2Pair] : d2{0.0, 0.0};
    tog = kX2Slot - tog;
    __builtin_amdgcn_sched_barrier(0);
    return r;
  }
  __device__ static inline void take(const LQ2Pending& r, double (&oth)[4]) {
    oth[0] = r.a.x; oth[1] = r.a.y; oth[2] = r.b.x; oth[3] = r.b.y;
  }
};

// product of this wave's row tile with a vector whose own half is known and whose other half arrives
// through the exchange; `mid` is independent work placed behind the own half
// NMID: matrix instructions inside `mid` (they take part in the issue pattern below)
template <bool EXTRA, int NMID = 0, class Mid>
__device__ static inline LQ2Pending xmv(LQ2X& X, const double (&Fo)[4], const double (&Fx)[4], const double (&vo)[4],
                                        d4 init, double (&vx)[4], double (&f)[4], double e0, double e1, Mid&& mid) {
  X.post<EXTRA>(vo, e0, e1);
  // two products ahead of the barrier: the wave blocks on the second until the first has left the pipe
  // (~70 cycles), which is about when its LDS writes have landed; the other two cover the read latency
  // One accumulation chain: a dependent v_mfma_f64_16x16x4_f64 issues as soon as its predecessor leaves the pipe, so two
  // chains gain nothing and their final addition (4 v_add_f64 behind the last result) only lengthens the stage's tail:
  // state pass 11.79 -> 11.44 ms, adjoint 20.13 -> 19.77 ms at BL-5.
  d4 acc = mma(Fo[0], vo[0], init);
  acc = mma(Fo[1], vo[1], acc);
  const LQ2Pending r = X.sync<EXTRA>();
  acc = mma(Fo[2], vo[2], acc);
  acc = mma(Fo[3], vo[3], acc);
  mid();
  LQ2X::take(r, vx);
  acc = mma(Fx[0], vx[0], acc);
  acc = mma(Fx[1], vx[1], acc);
  acc = mma(Fx[2], vx[2], acc);
  acc = mma(Fx[3], vx[3], acc);
  f[0] = acc.x; f[1] = acc.y; f[2] = acc.z; f[3] = acc.w;
  // Issue order of this region (from the barrier to the next post): one matrix instruction, then a few of the
  // independent vector / memory instructions (`mid`, address arithmetic, the step's loads and stores), and so
  // on.  A wave issues in order and blocks on a matrix instruction while the pipe is busy (~70 cycles), so
  // independent work placed BEHIND the last product would run with the pipe idle.
#pragma unroll
  for (int k = 0; k < 6 + NMID; ++k) {
    __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);  // MFMA
    __builtin_amdgcn_sched_group_barrier(0x002, 6, 0);  // VALU
    __builtin_amdgcn_sched_group_barrier(0x060, 2, 0);  // VMEM read / write
  }
  return r;
}
// the same product when both halves are already known (no exchange)
__device__ static inline void mv2(const double (&Fo)[4], const double (&Fx)[4], const double (&vo)[4],
                                  const double (&vx)[4], d4 init, double (&f)[4]) {
  d4 acc = mma(Fo[0], vo[0], init);
  acc = mma(Fo[1], vo[1], acc);
  acc = mma(Fo[2], vo[2], acc);
  acc = mma(Fo[3], vo[3], acc);
  acc = mma(Fx[0], vx[0], acc);
  acc = mma(Fx[1], vx[1], acc);
  acc = mma(Fx[2], vx[2], acc);
  acc = mma(Fx[3], vx[3], acc);
  f[0] = acc.x; f[1] = acc.y; f[2] = acc.z; f[3] = acc.w;
}

struct LQ2Core {
  double Ao[4], Ax[4];  // fragments of A, row tile w: own k-steps (kk = 4w + j) and the partner's (kk = 4(1-w) + j)
  double Bu;            // fragment of Bu, row tile w
  double q[4];          // q[16w + 4j + g]
  double R;             // rdiag[g] on wave 0, 0 on wave 1 (each control's cost is counted once)
  __device__ inline void load(const double* ps, int nS, int nC, int w, int g, int i) {
    const double* A = ps + 1;
    const int r = 16 * w + i;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int co = 4 * (4 * w + j) + g, cx = 4 * (4 * (1 - w) + j) + g;
      Ao[j] = (r < nS && co < nS) ? A[r + (size_t)nS * co] : 0.0;
      Ax[j] = (r < nS && cx < nS) ? A[r + (size_t)nS * cx] : 0.0;
    }
    const double* bu = A + (size_t)nS * nS;
    Bu = (r < nS && g < nC) ? bu[r + (size_t)nS * g] : 0.0;
    const double* qq = bu + (size_t)nS * nC;
#pragma unroll
    for (int j = 0; j < 4; ++j) q[j] = (16 * w + 4 * j + g < nS) ? qq[16 * w + 4 * j + g] : 0.0;
    R = (w == 0 && g < nC) ? qq[nS + g] : 0.0;
  }
  // q and R of trajectory b in place of the shared ones (LQCore::load_weights)
  __device__ inline void load_weights(const double* W, size_t B, int b, int nS, int nC, int w, int g) {
#pragma unroll
    for (int j = 0; j < 4; ++j) q[j] = (16 * w + 4 * j + g < nS) ? W[(size_t)(16 * w + 4 * j + g) * B + b] : 0.0;
    R = (w == 0 && g < nC) ? W[(size_t)(nS + g) * B + b] : 0.0;
  }
  __device__ inline d4 bu_times(double u) const {
    const d4 z = {0.0, 0.0, 0.0, 0.0};
    return mma(Bu, u, z);
  }
  __device__ inline double cost_part(const double (&Yo)[4], double u, double e) const {
    double s = R * (u * u);
#pragma unroll
    for (int j = 0; j < 4; ++j) s = __builtin_fma(q[j], Yo[j] * Yo[j], s);
    return e * s;
  }
};

template <bool OUT_X, bool UCONST, bool PW = false>
__global__ __launch_bounds__(256) void k_lq2_forward(const LQArgs a) {
  using Rec = StepRec<1>;
  __shared__ d2 xb2[2][2 * kX2Slot];
  const int pair = threadIdx.x >> 7, w = (threadIdx.x >> 6) & 1, lane = threadIdx.x & 63, g = lane >> 4, n = lane & 15;
  d2* xb = xb2[pair];
  const int b0 = (blockIdx.x * 2 + pair) * 16 + n;
  const int b = b0 < a.batch ? b0 : a.batch - 1;
  const size_t B = (size_t)a.batch;
  const int nS = a.nS, nC = a.nC, N = a.N;
  const size_t nAugB = (size_t)(nS + 1) * B;
  LQ2X X;
  X.init(xb, w, lane);
  LQ2Core P;
  P.load(a.ps, nS, nC, w, g, n);
  if constexpr (PW) P.load_weights(a.W, B, b, nS, nC, w, g);

  // own rows 16w + 4j + g, partner rows 16(1-w) + 4j + g
  double yo[4], yx[4], yc = 0.0;  // yc: this wave's share of the running cost
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int ro = 16 * w + 4 * j + g, rx = 16 * (1 - w) + 4 * j + g;
    yo[j] = ro < nS ? a.x0[(size_t)ro * B + b] : 0.0;
    yx[j] = rx < nS ? a.x0[(size_t)rx * B + b] : 0.0;
  }
  // Outputs and control samples go through raw buffer descriptors rebuilt per step on the scalar unit (base of the
  // column) with a per-lane byte offset fixed for the whole pass: 64-bit pointer arithmetic per access was ~36 vector
  // instructions per step, on the pipe the matrix instructions need.
  unsigned vrow[4];   // byte offset of row 16w + 4j + g of this lane's trajectory inside a column (dropped if padded)
#pragma unroll
  for (int j = 0; j < 4; ++j)
    vrow[j] = (16 * w + 4 * j + g < nS) ? (unsigned)(((size_t)(16 * w + 4 * j + g) * B + b) * 8) : kOffDrop;
  const unsigned vcost = (w == 0 && g == 0) ? (unsigned)(((size_t)nS * B + b) * 8) : kOffDrop;
  if (OUT_X) {
    const Buf bx0 = Buf::make(a.x);
#pragma unroll
    for (int j = 0; j < 4; ++j) bx0.st0(yo[j], vrow[j], 0);
  }

  const bool uact = g < nC;
  const size_t ustride = (size_t)nC * B;
  const unsigned us8 = (unsigned)(ustride * 8);
  const double* up = a.u + (size_t)(uact ? g : 0) * B + b;
  const unsigned vu = (unsigned)(((size_t)(uact ? g : 0) * B + b) * 8);
  double uA = UCONST ? (uact ? lq_uconst(a, g, b) : 0.0) : (uact ? *up : 0.0);
  double uM = uA, uB = uA;
  if (!UCONST) {
    uM = uact ? up[ustride] : 0.0;
    uB = uact ? up[2 * ustride] : 0.0;
  }
  d4 buA = P.bu_times(uA), buM = buA, buB = buA;
  double F1[4];
  mv2(P.Ao, P.Ax, yo, yx, buA, F1);  // stage 1 of step 0 (later steps: under the y exchange of the step before)

  // Per-step inputs (uniform record, two control samples) are requested TWO steps ahead into two slots that the
  // steps use alternately.  vmcnt counts loads and stores in order, so with a lead of one step the wait for
  // step i+1's inputs would also be a wait for the stores of step i; the loop is unrolled by the two slots (and
  // the odd last step peeled) so that no register copy of a freshly requested value and no branch sits in a step.
  struct Slot {
    Rec r;
    double uM, uB;  // raw loads; unused control rows are zeroed when the slot is consumed
  };
  auto request = [&](int i, Slot& q) OCS_INLINE {
    q.r = load_rec<1>(a.REC + (size_t)i * rec_stride(1));  // the table is padded past step N-1
    if (!UCONST) {
      const int ic = i < N ? i : N - 1;
      const Buf bu = Buf::make(a.u + (size_t)(2 * ic) * ustride);
      q.uM = bu.ld(vu, us8);
      q.uB = bu.ld(vu, 2 * us8);
    }
  };
  auto step = [&](int i, Slot& q) OCS_INLINE {
    const Rec cur = q.r;
    if (!UCONST) {
      uM = uact ? q.uM : 0.0;
      uB = uact ? q.uB : 0.0;
    }
    request(i + 2, q);
    if (!UCONST) {
      buM = P.bu_times(uM);
      buB = P.bu_times(uB);
    }
    double F2[4], F3[4], F4[4], Yo[4], Yx[4];
    double cs = 0.0;
#pragma unroll
    for (int j = 0; j < 4; ++j) Yo[j] = __builtin_fma(cur.hh, F1[j], yo[j]);  // :40
    // this exchange also carries the wave's share of the running cost up to x(:, i) (reduced over g under
    // the previous exchange); wave 0 then completes the cost row of column i
    const LQ2Pending r2 = xmv<true>(X, P.Ao, P.Ax, Yo, buM, Yx, F2, yc, 0.0, [&]() OCS_INLINE {   // :41
      cs = P.cost_part(yo, uA, cur.tcA[0]) + 2.0 * P.cost_part(Yo, uM, cur.tcM[0]);
    });
    const double ctot = yc + r2.c.x;  // x(end, i)
#pragma unroll
    for (int j = 0; j < 4; ++j) Yo[j] = __builtin_fma(cur.hh, F2[j], yo[j]);  // :44
    xmv<false>(X, P.Ao, P.Ax, Yo, buM, Yx, F3, 0.0, 0.0, [&]() OCS_INLINE {                       // :45
      cs += 2.0 * P.cost_part(Yo, uM, cur.tcM[0]);
    });
#pragma unroll
    for (int j = 0; j < 4; ++j) Yo[j] = __builtin_fma(cur.h, F3[j], yo[j]);   // :48
    xmv<false>(X, P.Ao, P.Ax, Yo, buB, Yx, F4, 0.0, 0.0, [&]() OCS_INLINE {                       // :49
      cs += P.cost_part(Yo, uB, cur.tcB[0]);
    });
#pragma unroll
    for (int j = 0; j < 4; ++j)                                               // :50
      yo[j] = __builtin_fma(cur.h6, (F1[j] + 2.0 * F2[j]) + (2.0 * F3[j] + F4[j]), yo[j]);
    // y exchange; stage 1 of the next step is the product that runs under it
    xmv<false>(X, P.Ao, P.Ax, yo, buB, yx, F1, 0.0, 0.0, [&]() OCS_INLINE {                       // :37
      yc = __builtin_fma(cur.h6, sum_over_g(cs), yc);
    });
    if (OUT_X) {
      const Buf bx = Buf::make(a.x + (size_t)i * nAugB);   // column i: its cost row; column i + 1: the state rows
      bx.st0(ctot, vcost, 0);
      const unsigned col8 = (unsigned)(nAugB * 8);
#pragma unroll
      for (int j = 0; j < 4; ++j) bx.st0(yo[j], vrow[j], col8);
    }
    uA = uB;
    buA = buB;
  };
  Slot sa, sb;
  request(0, sa);
  request(1, sb);
  int i = 0;
  for (; i + 1 < N; i += 2) {
    step(i, sa);
    step(i + 1, sb);
  }
  if (i < N) step(i, sa);
  {  // the partner's share of the final cost
    X.post<true>(yo, yc, 0.0);
    const LQ2Pending r = X.sync<true>();
    if (w == 0 && g == 0) {
      const double Jt = yc + r.c.x;
      if (OUT_X) a.x[(size_t)N * nAugB + (size_t)nS * B + b] = Jt;
      a.J[b] = a.Jadd ? a.Jadd[b] + Jt : Jt;  // J = x(end,end)   :55
    }
  }
}

template <bool OUT_LAM, bool OUT_DJDU, bool UCONST, bool PW = false>
__global__ __launch_bounds__(256) void k_lq2_backward(const LQArgs a) {
  using Rec = StepRec<1>;
  __shared__ d2 xb2[2][2 * kX2Slot];
  const int pair = threadIdx.x >> 7, w = (threadIdx.x >> 6) & 1, lane = threadIdx.x & 63, g = lane >> 4, n = lane & 15;
  d2* xb = xb2[pair];
  const int b0 = (blockIdx.x * 2 + pair) * 16 + n;
  const int b = b0 < a.batch ? b0 : a.batch - 1;
  const size_t B = (size_t)a.batch;
  const int nS = a.nS, nC = a.nC, N = a.N;
  const size_t nAugB = (size_t)(nS + 1) * B;
  LQ2X X;
  X.init(xb, w, lane);
  LQ2Core P;
  P.load(a.ps, nS, nC, w, g, n);
  if constexpr (PW) P.load_weights(a.W, B, b, nS, nC, w, g);
  const double Rall = (g < nC) ? (PW ? a.W[(size_t)(nS + g) * B + b] : a.ps[1 + (size_t)nS * nS + (size_t)nS * nC + nS + g]) : 0.0;
  double ATo[4], ATx[4], BuT[4];  // fragments of A' (row tile w) and of Bu' restricted to this wave's rows
  {
    const double* A = a.ps + 1;
    const double* bu = A + (size_t)nS * nS;
    const int r = 16 * w + n;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int co = 4 * (4 * w + j) + g, cx = 4 * (4 * (1 - w) + j) + g;
      ATo[j] = (r < nS && co < nS) ? A[co + (size_t)nS * r] : 0.0;
      ATx[j] = (r < nS && cx < nS) ? A[cx + (size_t)nS * r] : 0.0;
      BuT[j] = (co < nS && n < nC) ? bu[co + (size_t)nS * n] : 0.0;
    }
  }
  // this wave's part of (Bu' v)_g: the contraction over its own 16 rows
  auto but_part = [&](const double (&vo)[4]) OCS_INLINE {
    const d4 z = {0.0, 0.0, 0.0, 0.0};
    d4 acc = mma(BuT[0], vo[0], z), alt = mma(BuT[1], vo[1], z);
    acc = mma(BuT[2], vo[2], acc);
    alt = mma(BuT[3], vo[3], alt);
    return acc.x + alt.x;
  };
  auto qy = [&](const double (&Yo)[4], double e2kl) OCS_INLINE {
    return d4{P.q[0] * Yo[0] * e2kl, P.q[1] * Yo[1] * e2kl, P.q[2] * Yo[2] * e2kl, P.q[3] * Yo[3] * e2kl};
  };

  double lo_[4], lx_[4], lamc;  // lam own / partner rows
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int ro = 16 * w + 4 * j + g, rx = 16 * (1 - w) + 4 * j + g;
    lo_[j] = (a.lamT && ro < nS) ? a.lamT[(size_t)ro * B + b] : 0.0;
    lx_[j] = (a.lamT && rx < nS) ? a.lamT[(size_t)rx * B + b] : 0.0;
  }
  lamc = a.lamT ? a.lamT[(size_t)nS * B + b] : 1.0;
  // raw buffer descriptors per column (scalar unit) + per-lane byte offsets fixed for the pass: see k_lq2_forward
  unsigned vown[4], vpar[4];   // rows 16w + 4j + g and 16(1-w) + 4j + g of this lane's trajectory (dropped if padded)
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int ro = 16 * w + 4 * j + g, rx = 16 * (1 - w) + 4 * j + g;
    vown[j] = (ro < nS) ? (unsigned)(((size_t)ro * B + b) * 8) : kOffDrop;
    vpar[j] = (rx < nS) ? (unsigned)(((size_t)rx * B + b) * 8) : kOffDrop;
  }
  const unsigned vlamc = (w == 0 && g == 0) ? (unsigned)(((size_t)nS * B + b) * 8) : kOffDrop;
  auto store_lam = [&](int col) OCS_INLINE {
    if (!OUT_LAM) return;
    const Buf bl = Buf::make(a.lam + (size_t)col * nAugB);
#pragma unroll
    for (int j = 0; j < 4; ++j) bl.st0(lo_[j], vown[j], 0);
    bl.st0(lamc, vlamc, 0);
  };
  store_lam(N);

  const bool uact = g < nC;
  const size_t ustride = (size_t)nC * B;
  const size_t uoff = (size_t)(uact ? g : 0) * B + b;
  const double* up = a.u + uoff;
  double* dq = a.dJdu + uoff;
  const unsigned vu = (unsigned)(uoff * 8), us8 = (unsigned)(ustride * 8);
  const unsigned vdq = (w == 0 && uact) ? vu : kOffDrop;
  double uB = UCONST ? (uact ? lq_uconst(a, g, b) : 0.0) : (uact ? up[(size_t)(2 * N) * ustride] : 0.0);
  double uA = uB, uM = uB;
  if (!UCONST) {
    uA = uact ? up[(size_t)(2 * N - 2) * ustride] : 0.0;
    uM = uact ? up[(size_t)(2 * N - 1) * ustride] : 0.0;
  }
  d4 buA = P.bu_times(uA), buM = P.bu_times(uM);
  double k1co[4] = {0.0, 0.0, 0.0, 0.0}, k1lc = 0.0;

  auto load_ck = [&](int i, double (&o)[4], double (&x)[4]) OCS_INLINE {
    const Buf bc = Buf::make(a.xck + (size_t)i * nAugB);   // (a dropped access returns 0: the padded rows)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      o[j] = bc.ld(vown[j], 0);
      x[j] = bc.ld(vpar[j], 0);
    }
  };
  // Per-step inputs (uniform record, checkpoint y_i, two control samples) are requested two steps ahead into
  // two alternating slots, as in the forward pass (k_lq2_forward explains why).
  struct Slot {
    Rec r;
    double yo[4], yx[4];
    double uA, uM;  // raw loads
  };
  auto request = [&](int i, Slot& q) OCS_INLINE {
    q.r = load_rec<1>(a.REC + (long long)i * rec_stride(1));  // the table is padded before step 0
    const int ic = i > 0 ? i : 0;
    load_ck(ic, q.yo, q.yx);
    if (!UCONST) {
      const Buf bu = Buf::make(a.u + (size_t)(2 * ic) * ustride);
      q.uA = bu.ld(vu, 0);
      q.uM = bu.ld(vu, us8);
    }
  };
  double yo[4], F[4];
  double eA0 = 0.0;
  auto nothing = []() {};

  // step i reads its record and controls from `q`, then refills `q` for step i-2; `qn` holds step i-1, whose
  // checkpoint is consumed at the end of this step (its first stage runs under the lam exchange)
  auto step = [&](int i, Slot& q, Slot& qn) OCS_INLINE {
    const Rec cur = q.r;
    if (!UCONST) {
      uA = uact ? q.uA : 0.0;
      uM = uact ? q.uM : 0.0;
    }
    request(i - 2, q);
    // k4 = h/6 lam is known when the step starts (both halves), so the matrix part of its product A'k4 runs inside
    // the two exchanges of the recompute chain below, where the matrix pipe would wait for the partner's values;
    // the elementwise term of :74, which needs Y4, is added when Y4 exists
    const double k4l = cur.h6 * lamc, k3l = cur.h3 * lamc, k2l = k3l, k1l = k4l;
    double k4o[4], k4x[4], k3o[4], k2o[4], k1o[4], kx[4], g3[4], g2[4], g1[4], g0[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {                                                         // :73
      k4o[j] = cur.h6 * lo_[j];
      k4x[j] = cur.h6 * lx_[j];
    }
    const d4 z4 = {0.0, 0.0, 0.0, 0.0};
    d4 g3a = z4, g3b = z4;
    // recompute the stage states (same products as the forward pass); only F2 and F3 need the partner's half
    double Y2o[4], Y3o[4], Y4o[4], Yx[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) Y2o[j] = __builtin_fma(cur.hh, F[j], yo[j]);
    xmv<false, 4>(X, P.Ao, P.Ax, Y2o, buM, Yx, F, 0.0, 0.0, [&]() OCS_INLINE {
      g3a = mma(ATo[0], k4o[0], g3a);
      g3b = mma(ATo[1], k4o[1], g3b);
      g3a = mma(ATo[2], k4o[2], g3a);
      g3b = mma(ATo[3], k4o[3], g3b);
    });
#pragma unroll
    for (int j = 0; j < 4; ++j) Y3o[j] = __builtin_fma(cur.hh, F[j], yo[j]);
    xmv<false, 4>(X, P.Ao, P.Ax, Y3o, buM, Yx, F, 0.0, 0.0, [&]() OCS_INLINE {
      g3a = mma(ATx[0], k4x[0], g3a);
      g3b = mma(ATx[1], k4x[1], g3b);
      g3a = mma(ATx[2], k4x[2], g3a);
      g3b = mma(ATx[3], k4x[3], g3b);
    });
#pragma unroll
    for (int j = 0; j < 4; ++j) Y4o[j] = __builtin_fma(cur.h, F[j], yo[j]);
    {                                                                                     // :74
      const d4 e = qy(Y4o, 2.0 * cur.tcB[0] * k4l), t = (g3a + g3b) + e;
      g3[0] = t.x; g3[1] = t.y; g3[2] = t.z; g3[3] = t.w;
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) k3o[j] = __builtin_fma(cur.h, g3[j], cur.h3 * lo_[j]);    // :77
    xmv<false>(X, ATo, ATx, k3o, qy(Y3o, 2.0 * cur.tcM[0] * k3l), kx, g2, 0.0, 0.0, nothing);  // :78
#pragma unroll
    for (int j = 0; j < 4; ++j) k2o[j] = __builtin_fma(cur.hh, g2[j], cur.h3 * lo_[j]);   // :81
    double pm = 0.0, pn = 0.0;
    xmv<false>(X, ATo, ATx, k2o, qy(Y2o, 2.0 * cur.tcM[0] * k2l), kx, g1, 0.0, 0.0, [&]() OCS_INLINE {  // :82
      if (OUT_DJDU) {  // midpoint column, this wave's rows   :104-106
        double v[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = k2o[j] + k3o[j];
        pm = but_part(v);
      }
    });
#pragma unroll
    for (int j = 0; j < 4; ++j) k1o[j] = __builtin_fma(cur.hh, g1[j], cur.h6 * lo_[j]);   // :85
    const LQ2Pending rm = xmv<OUT_DJDU>(X, ATo, ATx, k1o, qy(yo, 2.0 * cur.tcA[0] * k1l), kx, g0, pm, 0.0,
                                        [&]() OCS_INLINE {                                // :86-88
      if (OUT_DJDU) {  // node column, this wave's rows   :108-112
        double v[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = k4o[j] + k1co[j];
        pn = but_part(v);
      }
    });
#pragma unroll
    for (int j = 0; j < 4; ++j) lo_[j] = (((lo_[j] + g1[j]) + g2[j]) + g3[j]) + g0[j];
    // lam exchange; the next step's first stage does not depend on lam and runs under it
    X.post<OUT_DJDU>(lo_, pn, 0.0);
    d4 buAn = buA, buMn = buM;
    if (!UCONST) {
      buAn = P.bu_times(uact ? qn.uA : 0.0);
      buMn = P.bu_times(uact ? qn.uM : 0.0);
    }
    const LQ2Pending rl = X.sync<OUT_DJDU>();
    mv2(P.Ao, P.Ax, qn.yo, qn.yx, buAn, F);
    LQ2X::take(rl, lx_);
    store_lam(i);
    if (OUT_DJDU) {
      const Buf bd = Buf::make(a.dJdu + (size_t)(2 * i + 1) * ustride);
      bd.st0((pn + rl.c.x) + 2.0 * cur.tcB[0] * Rall * uB * (k4l + k1lc), vdq, us8);
      bd.st0((pm + rm.c.x) + 2.0 * cur.tcM[0] * Rall * uM * (k2l + k3l), vdq, 0);
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      k1co[j] = k1o[j];
      yo[j] = qn.yo[j];
    }
    k1lc = k1l;
    eA0 = cur.tcA[0];
    uB = uA;
    buA = buAn;
    buM = buMn;
  };
  Slot sa, sb;
  request(N - 1, sa);
  request(N - 2, sb);
  {  // F1 of the first step (later steps: computed under the lam exchange of the step before)
#pragma unroll
    for (int j = 0; j < 4; ++j) yo[j] = sa.yo[j];
    mv2(P.Ao, P.Ax, sa.yo, sa.yx, buA, F);
  }
  int i = N - 1;
  for (; i >= 1; i -= 2) {
    step(i, sa, sb);
    step(i - 1, sb, sa);
  }
  if (i == 0) step(0, sa, sb);
  if (OUT_DJDU) {  // first column: B(t_1, y_1, u_1)' k1_1   :100-101
    const double p0 = but_part(k1co);
    X.post<true>(k1co, p0, 0.0);
    const LQ2Pending r0 = X.sync<true>();
    if (w == 0 && uact) dq[0] = (p0 + r0.c.x) + 2.0 * eA0 * Rall * uB * k1lc;
  }
  if (a.lam0) {
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (16 * w + 4 * j + g < nS) a.lam0[(size_t)(16 * w + 4 * j + g) * B + b] = lo_[j];
    if (w == 0 && g == 0) a.lam0[(size_t)nS * B + b] = lamc;
  }
}

// ---------------------------------------------------------------------------------------
// Mapping "M4": four waves per 16 trajectories (17 <= nS <= 32), the products split over K as well
// ---------------------------------------------------------------------------------------
// Wave (w, h) = (wave >> 1, wave & 1) of a 256-thread workgroup computes the PARTIAL product of row tile w over the
// K half h (k-steps 4h .. 4h+3: four matrix instructions where a wave of M2 issues eight) and keeps the state rows of
// tile h -- the B operand of exactly those k-steps -- up to date.  What goes through LDS is therefore not the stage
// state (M2) but the partial products: every wave posts its 4 doubles per lane, one s_barrier, and wave (w, h) reads
// and adds the two partials of tile h, P(h, 0) + P(h, 1) (the Bu u term rides in P(., 0)'s accumulator).  Both waves
// that keep tile h form the same sums in the same order, so their copies of the state agree bit for bit.
// A batch of 8192 puts two such waves (of different trajectory groups) on every SIMD: one group's exchange runs under
// the other's matrix instructions; a batch of 1024 (the 8-GPU shard of BASELINE configs[4]) still spreads over 256
// SIMDs with half the dependent matrix instructions per stage.
// Adjoint pass: five exchanges per step -- (A Y2 | A'k4), A Y3, A'k3, A'k2, (A'k1 | A y_{i-1}); the contraction
// Bu'(k2 + k3) of the midpoint column is done by the waves (0, h) and Bu'(k4 + k1) of the node column by the waves
// (1, h) over the rows of their tile h, the two halves meet in the spare row of the last exchange.
constexpr int kX4Row = 64, kX4Rows = 5, kX4Wave = kX4Rows * kX4Row, kX4Slot = 4 * kX4Wave;  // d2 units

struct LQ4X {
  d2* mine;
  const d2* src;   // slot of wave (h, 0); wave (h, 1)'s follows it
  int tog;
  __device__ inline void init(d2* xb, int wv, int h, int lane) {
    mine = xb + wv * kX4Wave + lane;
    src = xb + (2 * h) * kX4Wave + lane;
    tog = 0;
  }
  template <int NP, bool EXTRA>
  __device__ inline void post(const d4 (&P)[NP], double e0 = 0.0, double e1 = 0.0) {
    d2* p = mine + tog;
#pragma unroll
    for (int q = 0; q < NP; ++q) {
      p[(2 * q) * kX4Row] = d2{P[q].x, P[q].y};
      p[(2 * q + 1) * kX4Row] = d2{P[q].z, P[q].w};
    }
    if (EXTRA) p[4 * kX4Row] = d2{e0, e1};
    __builtin_amdgcn_sched_barrier(0);
  }
  // the sums of the two partials of this wave's tile; ex0 / ex1: the spare rows of waves (h, 0) and (h, 1)
  template <int NP, bool EXTRA>
  __device__ inline void fetch(d4 (&S)[NP], d2& ex0, d2& ex1) {
    lq_lds_barrier();
    const d2* p0 = src + tog;
    const d2* p1 = p0 + kX4Wave;
    d2 lo0[NP], hi0[NP], lo1[NP], hi1[NP];
#pragma unroll
    for (int q = 0; q < NP; ++q) {
      lo0[q] = p0[(2 * q) * kX4Row];
      hi0[q] = p0[(2 * q + 1) * kX4Row];
      lo1[q] = p1[(2 * q) * kX4Row];
      hi1[q] = p1[(2 * q + 1) * kX4Row];
    }
    if (EXTRA) {
      ex0 = p0[4 * kX4Row];
      ex1 = p1[4 * kX4Row];
    }
#pragma unroll
    for (int q = 0; q < NP; ++q) S[q] = d4{lo0[q].x + lo1[q].x, lo0[q].y + lo1[q].y, hi0[q].x + hi1[q].x, hi0[q].y + hi1[q].y};
    tog = kX4Slot - tog;
    __builtin_amdgcn_sched_barrier(0);
  }
};

// four k-steps of one row tile
__device__ static inline d4 mv4(const double (&Fr)[4], const double (&v)[4], d4 init) {
  d4 acc = mma(Fr[0], v[0], init);
  acc = mma(Fr[1], v[1], acc);
  acc = mma(Fr[2], v[2], acc);
  acc = mma(Fr[3], v[3], acc);
  return acc;
}
__device__ static inline void d4_to(const d4 v, double (&f)[4]) { f[0] = v.x; f[1] = v.y; f[2] = v.z; f[3] = v.w; }

template <bool OUT_X, bool UCONST, bool PW = false>
__global__ __launch_bounds__(256) void k_lq4_forward(const LQArgs a) {
  using Rec = StepRec<1>;
  __shared__ d2 xb[2 * kX4Slot];
  const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), w = wv >> 1, h = wv & 1;
  const int lane = threadIdx.x & 63, g = lane >> 4, n = lane & 15;
  const int b0 = blockIdx.x * 16 + n;
  const int b = b0 < a.batch ? b0 : a.batch - 1;
  const size_t B = (size_t)a.batch;
  const int nS = a.nS, nC = a.nC, N = a.N;
  const size_t nAugB = (size_t)(nS + 1) * B;
  LQ4X X;
  X.init(xb, wv, h, lane);
  const d4 z4 = {0.0, 0.0, 0.0, 0.0};

  double Aw[4], Bu, q[4], R;   // A[16w + n][4(4h + j) + g]; Bu[16w + n][g] (waves h == 0); q of the rows of tile h
  {
    const double* A = a.ps + 1;
    const double* bu = A + (size_t)nS * nS;
    const double* qq = bu + (size_t)nS * nC;
    const int r = 16 * w + n;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int c = 4 * (4 * h + j) + g;
      Aw[j] = (r < nS && c < nS) ? A[r + (size_t)nS * c] : 0.0;
      q[j] = (16 * h + 4 * j + g < nS) ? qq[16 * h + 4 * j + g] : 0.0;
    }
    Bu = (r < nS && g < nC) ? bu[r + (size_t)nS * g] : 0.0;
    R = (wv == 0 && g < nC) ? qq[nS + g] : 0.0;   // each control's cost is counted once
    if constexpr (PW) {   // this lane's trajectory's own weights
#pragma unroll
      for (int j = 0; j < 4; ++j) q[j] = (16 * h + 4 * j + g < nS) ? a.W[(size_t)(16 * h + 4 * j + g) * B + b] : 0.0;
      R = (wv == 0 && g < nC) ? a.W[(size_t)(nS + g) * B + b] : 0.0;
    }
  }
  auto bu_times = [&](double u) OCS_INLINE { return h == 0 ? mma(Bu, u, z4) : z4; };   // (wave-uniform)
  auto cost_part = [&](const double (&Y)[4], double u, double e) OCS_INLINE {
    double s = R * (u * u);
#pragma unroll
    for (int j = 0; j < 4; ++j) s = __builtin_fma(q[j], Y[j] * Y[j], s);
    return e * s;
  };
  const bool costw = w == 0;   // the waves (0, h) integrate the objective over the rows of tile h

  double y[4], yc = 0.0;   // rows 16h + 4j + g; yc: this wave's share of the running cost
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int r = 16 * h + 4 * j + g;
    y[j] = r < nS ? a.x0[(size_t)r * B + b] : 0.0;
  }
  const bool storew = w == 1;   // the waves (1, h) store the rows of tile h
  // (raw buffer descriptors per column, per-lane byte offsets fixed for the pass: see k_lq2_forward)
  unsigned vrow[4];
#pragma unroll
  for (int j = 0; j < 4; ++j)
    vrow[j] = (storew && 16 * h + 4 * j + g < nS) ? (unsigned)(((size_t)(16 * h + 4 * j + g) * B + b) * 8) : kOffDrop;
  const unsigned vcost = (wv == 0 && g == 0) ? (unsigned)(((size_t)nS * B + b) * 8) : kOffDrop;
  if (OUT_X) {
    const Buf bx0 = Buf::make(a.x);
#pragma unroll
    for (int j = 0; j < 4; ++j) bx0.st0(y[j], vrow[j], 0);
  }
  const bool uact = g < nC;
  const size_t ustride = (size_t)nC * B;
  const double* up = a.u + (size_t)(uact ? g : 0) * B + b;
  const unsigned vu = (unsigned)(((size_t)(uact ? g : 0) * B + b) * 8), us8 = (unsigned)(ustride * 8);
  double uA = UCONST ? (uact ? lq_uconst(a, g, b) : 0.0) : (uact ? *up : 0.0);
  double uM = uA, uB = uA;
  d4 buA = bu_times(uA), buM = buA, buB = buA;
  double F1[4];
  d2 e0, e1;
  {  // stage 1 of step 0 (later steps: the exchange at the end of the step before)
    d4 P[1] = {mv4(Aw, y, buA)}, S[1];
    X.post<1, false>(P);
    X.fetch<1, false>(S, e0, e1);
    d4_to(S[0], F1);
  }
  struct Slot {
    Rec r;
    double uM, uB;
  };
  auto request = [&](int i, Slot& s) OCS_INLINE {
    s.r = load_rec<1>(a.REC + (size_t)i * rec_stride(1));  // the table is padded past step N-1
    if (!UCONST) {
      const int ic = i < N ? i : N - 1;
      const Buf bu = Buf::make(a.u + (size_t)(2 * ic) * ustride);
      s.uM = bu.ld(vu, us8);
      s.uB = bu.ld(vu, 2 * us8);
    }
  };
  auto step = [&](int i, Slot& sl) OCS_INLINE {
    const Rec cur = sl.r;
    if (!UCONST) {
      uM = uact ? sl.uM : 0.0;
      uB = uact ? sl.uB : 0.0;
    }
    request(i + 2, sl);
    if (!UCONST) {
      buM = bu_times(uM);
      buB = bu_times(uB);
    }
    double F2[4], F3[4], F4[4], Y[4];
    double cs = 0.0;
    d4 P[1], S[1];
#pragma unroll
    for (int j = 0; j < 4; ++j) Y[j] = __builtin_fma(cur.hh, F1[j], y[j]);   // :40
    P[0] = mv4(Aw, Y, buM);                                                   // :41
    X.post<1, true>(P, yc, 0.0);   // ... with the wave's share of the running cost up to x(:, i)
    if (costw) cs = cost_part(y, uA, cur.tcA[0]) + 2.0 * cost_part(Y, uM, cur.tcM[0]);
    X.fetch<1, true>(S, e0, e1);
    d4_to(S[0], F2);
    const double ctot = e0.x + e1.x;   // wave 0: x(end, i)
#pragma unroll
    for (int j = 0; j < 4; ++j) Y[j] = __builtin_fma(cur.hh, F2[j], y[j]);   // :44
    P[0] = mv4(Aw, Y, buM);                                                   // :45
    X.post<1, false>(P);
    if (costw) cs += 2.0 * cost_part(Y, uM, cur.tcM[0]);
    X.fetch<1, false>(S, e0, e1);
    d4_to(S[0], F3);
#pragma unroll
    for (int j = 0; j < 4; ++j) Y[j] = __builtin_fma(cur.h, F3[j], y[j]);    // :48
    P[0] = mv4(Aw, Y, buB);                                                   // :49
    X.post<1, false>(P);
    if (costw) cs += cost_part(Y, uB, cur.tcB[0]);
    X.fetch<1, false>(S, e0, e1);
    d4_to(S[0], F4);
#pragma unroll
    for (int j = 0; j < 4; ++j)                                               // :50
      y[j] = __builtin_fma(cur.h6, (F1[j] + 2.0 * F2[j]) + (2.0 * F3[j] + F4[j]), y[j]);
    P[0] = mv4(Aw, y, buB);   // stage 1 of the next step   :37
    X.post<1, false>(P);
    if (costw) yc = __builtin_fma(cur.h6, sum_over_g(cs), yc);
    if (OUT_X) {
      const Buf bx = Buf::make(a.x + (size_t)i * nAugB);   // column i: its cost row; column i + 1: the state rows
      bx.st0(ctot, vcost, 0);
      const unsigned col8 = (unsigned)(nAugB * 8);
#pragma unroll
      for (int j = 0; j < 4; ++j) bx.st0(y[j], vrow[j], col8);
    }
    X.fetch<1, false>(S, e0, e1);
    d4_to(S[0], F1);
    uA = uB;
    buA = buB;
  };
  Slot sa, sb;
  request(0, sa);
  request(1, sb);
  int i = 0;
  for (; i + 1 < N; i += 2) {
    step(i, sa);
    step(i + 1, sb);
  }
  if (i < N) step(i, sa);
  {  // the two shares of the final cost
    d4 P[1] = {z4}, S[1];
    X.post<1, true>(P, yc, 0.0);
    X.fetch<1, true>(S, e0, e1);
    if (wv == 0 && g == 0) {
      const double Jt = e0.x + e1.x;
      if (OUT_X) a.x[(size_t)N * nAugB + (size_t)nS * B + b] = Jt;
      a.J[b] = a.Jadd ? a.Jadd[b] + Jt : Jt;  // J = x(end,end)   :55
    }
  }
}

template <bool OUT_LAM, bool OUT_DJDU, bool UCONST, bool PW = false>
__global__ __launch_bounds__(256) void k_lq4_backward(const LQArgs a) {
  using Rec = StepRec<1>;
  __shared__ d2 xb[2 * kX4Slot];
  const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), w = wv >> 1, h = wv & 1;
  const int lane = threadIdx.x & 63, g = lane >> 4, n = lane & 15;
  const int b0 = blockIdx.x * 16 + n;
  const int b = b0 < a.batch ? b0 : a.batch - 1;
  const size_t B = (size_t)a.batch;
  const int nS = a.nS, nC = a.nC, N = a.N;
  const size_t nAugB = (size_t)(nS + 1) * B;
  LQ4X X;
  X.init(xb, wv, h, lane);
  const d4 z4 = {0.0, 0.0, 0.0, 0.0};

  // A and A' fragments of (row tile w, K half h); Bu (waves h == 0); Bu' over the rows of tile h; q of tile h
  double Aw[4], ATw[4], BuT[4], Bu, q[4];
  {
    const double* A = a.ps + 1;
    const double* bu = A + (size_t)nS * nS;
    const double* qq = bu + (size_t)nS * nC;
    const int r = 16 * w + n;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int c = 4 * (4 * h + j) + g;
      Aw[j] = (r < nS && c < nS) ? A[r + (size_t)nS * c] : 0.0;
      ATw[j] = (r < nS && c < nS) ? A[c + (size_t)nS * r] : 0.0;
      BuT[j] = (c < nS && n < nC) ? bu[c + (size_t)nS * n] : 0.0;
      q[j] = (16 * h + 4 * j + g < nS) ? qq[16 * h + 4 * j + g] : 0.0;
    }
    Bu = (r < nS && g < nC) ? bu[r + (size_t)nS * g] : 0.0;
    if constexpr (PW) {   // this lane's trajectory's own weights
#pragma unroll
      for (int j = 0; j < 4; ++j) q[j] = (16 * h + 4 * j + g < nS) ? a.W[(size_t)(16 * h + 4 * j + g) * B + b] : 0.0;
    }
  }
  const double Rall = (g < nC) ? (PW ? a.W[(size_t)(nS + g) * B + b] : a.ps[1 + (size_t)nS * nS + (size_t)nS * nC + nS + g]) : 0.0;
  auto bu_times = [&](double u) OCS_INLINE { return h == 0 ? mma(Bu, u, z4) : z4; };
  auto but_part = [&](const double (&v)[4]) OCS_INLINE {   // (Bu' v)_g over the rows of tile h
    d4 acc = mma(BuT[0], v[0], z4), alt = mma(BuT[1], v[1], z4);
    acc = mma(BuT[2], v[2], acc);
    alt = mma(BuT[3], v[3], alt);
    return acc.x + alt.x;
  };
  auto qy = [&](const double (&Y)[4], double e2kl, const d4 lin, double (&o)[4]) OCS_INLINE {   // :74 elementwise term
    o[0] = __builtin_fma(q[0] * Y[0], e2kl, lin.x);
    o[1] = __builtin_fma(q[1] * Y[1], e2kl, lin.y);
    o[2] = __builtin_fma(q[2] * Y[2], e2kl, lin.z);
    o[3] = __builtin_fma(q[3] * Y[3], e2kl, lin.w);
  };

  double lam[4], lamc;   // rows of tile h
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int r = 16 * h + 4 * j + g;
    lam[j] = (a.lamT && r < nS) ? a.lamT[(size_t)r * B + b] : 0.0;
  }
  lamc = a.lamT ? a.lamT[(size_t)nS * B + b] : 1.0;
  const bool storew = w == 1;   // the waves (1, h) store lam of tile h
  unsigned vrow[4], vst[4];   // rows of tile h of this lane's trajectory: loads (every wave), stores (waves (1, h))
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    vrow[j] = (16 * h + 4 * j + g < nS) ? (unsigned)(((size_t)(16 * h + 4 * j + g) * B + b) * 8) : kOffDrop;
    vst[j] = storew ? vrow[j] : kOffDrop;
  }
  const unsigned vlamc = (wv == 2 && g == 0) ? (unsigned)(((size_t)nS * B + b) * 8) : kOffDrop;
  auto store_lam = [&](int col) OCS_INLINE {
    if (!OUT_LAM) return;
    const Buf bl = Buf::make(a.lam + (size_t)col * nAugB);
#pragma unroll
    for (int j = 0; j < 4; ++j) bl.st0(lam[j], vst[j], 0);
    bl.st0(lamc, vlamc, 0);
  };
  store_lam(N);

  const bool uact = g < nC;
  const size_t ustride = (size_t)nC * B;
  const size_t uoff = (size_t)(uact ? g : 0) * B + b;
  const double* up = a.u + uoff;
  double* dq = a.dJdu + uoff;
  const unsigned vu = (unsigned)(uoff * 8), us8 = (unsigned)(ustride * 8);
  double uB = UCONST ? (uact ? lq_uconst(a, g, b) : 0.0) : (uact ? up[(size_t)(2 * N) * ustride] : 0.0);
  double uA = uB, uM = uB;
  if (!UCONST) {
    uA = uact ? up[(size_t)(2 * N - 2) * ustride] : 0.0;
    uM = uact ? up[(size_t)(2 * N - 1) * ustride] : 0.0;
  }
  d4 buA = bu_times(uA), buM = bu_times(uM);
  double k1c[4] = {0.0, 0.0, 0.0, 0.0}, k1lc = 0.0;

  auto load_ck = [&](int i, double (&o)[4]) OCS_INLINE {
    const Buf bc = Buf::make(a.xck + (size_t)i * nAugB);   // (a dropped access returns 0: the padded rows)
#pragma unroll
    for (int j = 0; j < 4; ++j) o[j] = bc.ld(vrow[j], 0);
  };
  struct Slot {
    Rec r;
    double y[4];
    double uA, uM;
  };
  auto request = [&](int i, Slot& s) OCS_INLINE {
    s.r = load_rec<1>(a.REC + (long long)i * rec_stride(1));  // the table is padded before step 0
    const int ic = i > 0 ? i : 0;
    load_ck(ic, s.y);
    if (!UCONST) {
      const Buf bu = Buf::make(a.u + (size_t)(2 * ic) * ustride);
      s.uA = bu.ld(vu, 0);
      s.uM = bu.ld(vu, us8);
    }
  };
  double yo[4], F[4];
  double eA0 = 0.0;
  d2 e0, e1;

  auto step = [&](int i, Slot& sl, Slot& sn) OCS_INLINE {
    const Rec cur = sl.r;
    if (!UCONST) {
      uA = uact ? sl.uA : 0.0;
      uM = uact ? sl.uM : 0.0;
    }
    request(i - 2, sl);
    const double k4l = cur.h6 * lamc, k3l = cur.h3 * lamc, k2l = k3l, k1l = k4l;
    double k4[4], k3[4], k2[4], k1[4], g3[4], g2[4], g1[4], g0[4], Y2[4], Y3[4], Y4[4];
    double pm = 0.0, pn = 0.0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      k4[j] = cur.h6 * lam[j];                                                            // :73
      Y2[j] = __builtin_fma(cur.hh, F[j], yo[j]);
    }
    d4 P2[2], S2[2], P1[1], S1[1];
    P2[0] = mv4(Aw, Y2, buM);     // recompute   A Y2
    P2[1] = mv4(ATw, k4, z4);     // matrix part of A'k4   :74
    X.post<2, false>(P2);
    if (OUT_DJDU && w == 1) {     // node column over the rows of tile h   :108-112
      double v[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) v[j] = k4[j] + k1c[j];
      pn = but_part(v);
    }
    X.fetch<2, false>(S2, e0, e1);
    d4_to(S2[0], F);
    const d4 G3 = S2[1];
#pragma unroll
    for (int j = 0; j < 4; ++j) Y3[j] = __builtin_fma(cur.hh, F[j], yo[j]);
    P1[0] = mv4(Aw, Y3, buM);
    X.post<1, false>(P1);
    d4 buAn = buA, buMn = buM;
    if (!UCONST) {
      buAn = bu_times(uact ? sn.uA : 0.0);
      buMn = bu_times(uact ? sn.uM : 0.0);
    }
    X.fetch<1, false>(S1, e0, e1);
    d4_to(S1[0], F);
#pragma unroll
    for (int j = 0; j < 4; ++j) Y4[j] = __builtin_fma(cur.h, F[j], yo[j]);
    qy(Y4, 2.0 * cur.tcB[0] * k4l, G3, g3);                                                // :74
#pragma unroll
    for (int j = 0; j < 4; ++j) k3[j] = __builtin_fma(cur.h, g3[j], cur.h3 * lam[j]);      // :77
    P1[0] = mv4(ATw, k3, z4);                                                              // :78
    X.post<1, false>(P1);
    X.fetch<1, false>(S1, e0, e1);
    qy(Y3, 2.0 * cur.tcM[0] * k3l, S1[0], g2);
#pragma unroll
    for (int j = 0; j < 4; ++j) k2[j] = __builtin_fma(cur.hh, g2[j], cur.h3 * lam[j]);     // :81
    P1[0] = mv4(ATw, k2, z4);                                                              // :82
    X.post<1, false>(P1);
    if (OUT_DJDU && w == 0) {     // midpoint column over the rows of tile h   :104-106
      double v[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) v[j] = k2[j] + k3[j];
      pm = but_part(v);
    }
    X.fetch<1, false>(S1, e0, e1);
    qy(Y2, 2.0 * cur.tcM[0] * k2l, S1[0], g1);
#pragma unroll
    for (int j = 0; j < 4; ++j) k1[j] = __builtin_fma(cur.hh, g1[j], cur.h6 * lam[j]);     // :85
    P2[0] = mv4(ATw, k1, z4);                                                              // :86-88
    P2[1] = mv4(Aw, sn.y, buAn);  // stage 1 of step i-1 from its checkpoint
    X.post<2, OUT_DJDU>(P2, w == 0 ? pm : pn, 0.0);
    X.fetch<2, OUT_DJDU>(S2, e0, e1);
    qy(yo, 2.0 * cur.tcA[0] * k1l, S2[0], g0);
    d4_to(S2[1], F);
#pragma unroll
    for (int j = 0; j < 4; ++j) lam[j] = (((lam[j] + g1[j]) + g2[j]) + g3[j]) + g0[j];
    store_lam(i);
    if (OUT_DJDU) {
      // wave 0 = (0, 0) has read the midpoint parts of the waves (0, 0), (0, 1); wave 3 = (1, 1) the node parts of (1, 0), (1, 1)
      const Buf bd = Buf::make(a.dJdu + (size_t)(2 * i + 1) * ustride);
      bd.st0((e0.x + e1.x) + 2.0 * cur.tcB[0] * Rall * uB * (k4l + k1lc), (wv == 3 && uact) ? vu : kOffDrop, us8);
      bd.st0((e0.x + e1.x) + 2.0 * cur.tcM[0] * Rall * uM * (k2l + k3l), (wv == 0 && uact) ? vu : kOffDrop, 0);
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      k1c[j] = k1[j];
      yo[j] = sn.y[j];
    }
    k1lc = k1l;
    eA0 = cur.tcA[0];
    uB = uA;
    buA = buAn;
    buM = buMn;
  };
  Slot sa, sb;
  request(N - 1, sa);
  request(N - 2, sb);
  {  // F1 of the first step (later steps: the last exchange of the step before)
#pragma unroll
    for (int j = 0; j < 4; ++j) yo[j] = sa.y[j];
    d4 P[1] = {mv4(Aw, sa.y, buA)}, S[1];
    X.post<1, false>(P);
    X.fetch<1, false>(S, e0, e1);
    d4_to(S[0], F);
  }
  int i = N - 1;
  for (; i >= 1; i -= 2) {
    step(i, sa, sb);
    step(i - 1, sb, sa);
  }
  if (i == 0) step(0, sa, sb);
  if (OUT_DJDU) {  // first column: B(t_1, y_1, u_1)' k1_1   :100-101
    const double p0 = w == 0 ? but_part(k1c) : 0.0;
    d4 P[1] = {z4}, S[1];
    X.post<1, true>(P, p0, 0.0);
    X.fetch<1, true>(S, e0, e1);
    if (wv == 0 && uact) dq[0] = (e0.x + e1.x) + 2.0 * eA0 * Rall * uB * k1lc;
  }
  if (a.lam0 && storew) {
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (16 * h + 4 * j + g < nS) a.lam0[(size_t)(16 * h + 4 * j + g) * B + b] = lam[j];
    if (wv == 2 && g == 0) a.lam0[(size_t)nS * B + b] = lamc;
  }
}

// ---------------------------------------------------------------------------------------
// plugin evaluation (ocs_problem_F / dFdx_times_vec / dFdu_times_vec): one thread per column
// ---------------------------------------------------------------------------------------
__global__ void k_lq_eval(int which, int k, int nS, int nC, const double* __restrict__ t,
                          const double* __restrict__ y, const double* __restrict__ u, const double* __restrict__ v,
                          const double* __restrict__ ps, double* __restrict__ out) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= k) return;
  const int nAug = nS + 1;
  const double *A = ps + 1, *Bu = A + (size_t)nS * nS, *q = Bu + (size_t)nS * nC, *R = q + nS;
  const double* yj = y + (size_t)j * nAug;
  const double* uj = u + (size_t)j * nC;
  const double e = exp(-ps[0] * t[j]);
  if (which == 0) {
    double* o = out + (size_t)j * nAug;
    double s = 0.0;
    for (int i = 0; i < nS; ++i) {
      double acc = 0.0;
      for (int l = 0; l < nS; ++l) acc += A[i + (size_t)l * nS] * yj[l];
      for (int l = 0; l < nC; ++l) acc += Bu[i + (size_t)l * nS] * uj[l];
      o[i] = acc;
      s += q[i] * (yj[i] * yj[i]);
    }
    for (int l = 0; l < nC; ++l) s += R[l] * (uj[l] * uj[l]);
    o[nS] = e * s;
  } else if (which == 1) {
    const double* vj = v + (size_t)j * nAug;
    double* o = out + (size_t)j * nAug;
    for (int i = 0; i < nS; ++i) {
      double acc = 0.0;
      for (int l = 0; l < nS; ++l) acc += A[l + (size_t)i * nS] * vj[l];
      o[i] = acc + 2 * e * q[i] * yj[i] * vj[nS];
    }
    o[nS] = 0.0;
  } else {
    const double* vj = v + (size_t)j * nAug;
    double* o = out + (size_t)j * nC;
    for (int l = 0; l < nC; ++l) {
      double acc = 0.0;
      for (int i = 0; i < nS; ++i) acc += Bu[i + (size_t)l * nS] * vj[i];
      o[l] = acc + 2 * e * R[l] * uj[l] * vj[nS];
    }
  }
}

// ---------------------------------------------------------------------------------------
// chunked ("time-parallel") passes for small batches
// ---------------------------------------------------------------------------------------
// The dynamics are linear with a Jacobian shared by the batch, so the RK4 step of Integrator/RK4Integrator.m:35-52 is an
// affine map x_{i+1} = P_i x_i + g_i(u) whose matrix P_i = sum_{k<=4} (h_i A)^k / k! depends on the grid alone, and the
// discrete adjoint of :72-89 is lam_i = P_i' lam_{i+1} + c_i (c_i: the objective row's share, which reads the stage
// states and the constant lam(end)).  A small batch (BASELINE configs[4] gives each of 8 GPUs 1024 trajectories = 64
// groups of 16) leaves most SIMDs without a wave and is bound by the 2 N dependent steps of a lone wave.  Here the horizon
// is cut into C chunks of L steps, and a wave integrates ONE chunk of one group:
//   pass Z   every chunk from a zero start (state pass: with its controls; adjoint pass: with the objective's share) ->
//            the constant z_c of the chunk map  x_hi = M_c x_lo + z_c  /  lam_lo = M_c' lam_hi + b_c;   M_c = prod P_i
//   carry    x at every chunk's first node: x_{c+1} = M_c x_c + z_c, C small matrix-vector products per trajectory
//   pass X   every chunk from its true start, with all outputs of its steps -- RK4Integrator.m's lines as in the serial kernel
//   fix-up   the running objective restarts at every chunk: the sums of the chunks below are added to the cost row; a node
//            column of dJdu at a chunk boundary is the sum of a k4 half (chunk below) and a k1 half (chunk above)
// M_c is not formed from powers of A: pass Z runs once per (grid, problem) on the unit vectors with zero control
// (the same instruction sequence the trajectories see).  Work per step doubles, the dependent chain shrinks C-fold; used
// while groups x C <= one wave per SIMD.  Any grid (the h_i enter through the step records as everywhere else).
struct LqWorkspace {
  // chunk matrices of one (grid, problem): MT [C][nS][nU] with M_c[r][k] at (c nS + r) nU + k
  const double* key_ps = nullptr;
  const double* key_rec = nullptr;
  unsigned long long key_version = 0;
  int key_C = 0, key_N = 0, key_nS = 0;
  double* MT = nullptr;
  size_t MT_cap = 0;
  // per-call scratch: cs, ce [C][nS][B]; cj [C][max(1, nC)][B]; off [C + 1][B]
  double *cs = nullptr, *ce = nullptr, *cj = nullptr, *off = nullptr, *zero_u = nullptr, *unit = nullptr;
  size_t cs_cap = 0, ce_cap = 0, cj_cap = 0, off_cap = 0, unit_cap = 0;
  // state pass under a CONSTANT control (the tail leg of RK4InfiniteIntegrator.m:20-24): the zero-start response of a chunk
  // does not depend on the trajectory -- one group of 16 identical trajectories, once per (matrices, control vector)
  double *zc = nullptr, *zz = nullptr;   // [C][nS][16]: the responses; zeros (their start states)
  size_t zc_cap = 0, zz_cap = 0;
  const double* zc_key_u = nullptr;
  unsigned long long zc_key_uversion = 0;   // FwdOpts::uversion the responses were formed under
  bool zc_valid = false;
};
void lq_workspace_free(LqWorkspace* w) {
  if (!w) return;
  for (double* q : {w->MT, w->cs, w->ce, w->cj, w->off, w->zero_u, w->unit, w->zc, w->zz})
    if (q) (void)hipFree(q);
  delete w;
}
static int lq_ensure(double*& q, size_t& cap, size_t n) {
  if (n <= cap) return 0;
  if (q) (void)hipFree(q);
  q = nullptr;
  cap = 0;
  const hipError_t e = hipMalloc((void**)&q, n * sizeof(double));
  if (e != hipSuccess) return (int)e;
  cap = n;
  return 0;
}

// carries through the chunk maps.  Thread (b, rg) owns rows 8 rg .. 8 rg + 7 of trajectory b (block: 64 x 4).
// TRANS = false (state pass):   out[0] = start; out[c+1] = M_c out[c] + add[c], c = 0 .. C-2
// TRANS = true  (adjoint pass): out[C-1] = start (or zero); out[c-1] = M_c' out[c] + add[c], c = C-1 .. 1;
//                               last (optional, [nS][B]) = M_0' out[0] + add[0]
// addB: trajectories in `add` ([C][nS][addB]); addB != B: one column for everybody (column 0)
template <bool TRANS>
__global__ __launch_bounds__(256) void k_lq_carry(int nS, int nU, int B, int C, const double* __restrict__ MT,
                                                  const double* __restrict__ start, const double* __restrict__ add,
                                                  double* out, double* last, int addB) {
  // the chunk matrix and the block's 64 current vectors live in LDS: an iteration is one round of global loads (the
  // next matrix, the next constants) and 32 x 8 multiply-adds per thread from LDS, not 32 dependent global round trips
  __shared__ double Ms[32 * 32];
  __shared__ double xs[32 * 64];
  const int tl = threadIdx.x & 63, rg = threadIdx.x >> 6;
  const int b = blockIdx.x * 64 + tl;
  const bool live = b < B;
  const size_t SB = (size_t)nS * B;
  const int first = TRANS ? C - 1 : 0;
  for (int r = 8 * rg; r < 8 * rg + 8; ++r) {
    const double v = (live && r < nS && start) ? start[(size_t)r * B + b] : 0.0;
    xs[r * 64 + tl] = v;
    if (live && r < nS) out[(size_t)first * SB + (size_t)r * B + b] = v;
  }
  const int nsteps = TRANS ? (last ? C : C - 1) : C - 1;
  // the matrix and the constants of iteration it + 1 are requested while iteration it computes (registers, then LDS)
  double mreg[4], areg[8];
  auto fetch = [&](int it) {
    const int c = TRANS ? C - 1 - it : it;
    const double* M = MT + (size_t)c * nS * nU;
#pragma unroll
    for (int j = 0; j < 4; ++j) {   // Ms[r][k] = M_c[r][k] (TRANS: M_c[k][r]), zero outside nS x nS
      const int e = threadIdx.x + 256 * j, r = e >> 5, k = e & 31;
      mreg[j] = (r < nS && k < nS) ? (TRANS ? M[(size_t)k * nU + r] : M[(size_t)r * nU + k]) : 0.0;
    }
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      const int r = 8 * rg + q;
      areg[q] = (live && r < nS) ? add[((size_t)c * nS + r) * addB + (addB == B ? b : 0)] : 0.0;
    }
  };
  if (nsteps > 0) fetch(0);
  for (int it = 0; it < nsteps; ++it) {
    const int c = TRANS ? C - 1 - it : it;           // the chunk whose map is applied
    const int dst = TRANS ? c - 1 : c + 1;           // (-1: `last`)
    double acc[8];
#pragma unroll
    for (int j = 0; j < 4; ++j) Ms[threadIdx.x + 256 * j] = mreg[j];
#pragma unroll
    for (int q = 0; q < 8; ++q) acc[q] = areg[q];
    __syncthreads();   // Ms and xs complete
    if (it + 1 < nsteps) fetch(it + 1);
#pragma unroll 8
    for (int k = 0; k < 32; ++k) {
      const double xk = xs[k * 64 + tl];
#pragma unroll
      for (int q = 0; q < 8; ++q) acc[q] = __builtin_fma(Ms[(8 * rg + q) * 32 + k], xk, acc[q]);
    }
    __syncthreads();   // everybody has read xs and Ms
    double* o = dst >= 0 ? out + (size_t)dst * SB : last;
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      const int r = 8 * rg + q;
      xs[r * 64 + tl] = (r < nS) ? acc[q] : 0.0;
      if (live && r < nS) o[(size_t)r * B + b] = acc[q];
    }
  }
}

// off[0] = 0, off[c+1] = off[c] + cj[c]; J = (Jadd +) off[C]  -- the value the cost row's last entry gets below
__global__ void k_lq_cost_prefix(int B, int C, const double* __restrict__ cj, double* __restrict__ off,
                                 const double* __restrict__ Jadd, double* __restrict__ J) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  double s = 0.0;
  off[b] = 0.0;
  for (int c = 0; c < C; ++c) {
    s += cj[(size_t)c * B + b];
    off[(size_t)(c + 1) * B + b] = s;
  }
  J[b] = Jadd ? Jadd[b] + s : s;
}
// x(end, col) += off[chunk of col] for the columns above the first chunk (blockIdx.y + L + 1 = col)
__global__ void k_lq_cost_fix(int B, int nS, int N, int L, const double* __restrict__ off, double* __restrict__ x) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  const int col = blockIdx.y + L + 1;
  if (b >= B || col > N) return;
  const int c = (col - 1) / L;
  double* q = x + ((size_t)col * (nS + 1) + nS) * B + b;
  // (the last column: off[c] + local is the sum k_lq_cost_prefix formed for J, bit for bit)
  *q = off[(size_t)c * B + b] + *q;
}
// dJdu(:, 2 c L + 1) += the k1 half the chunk above left in cj[c], c = 1 .. C-1
__global__ void k_lq_djdu_fix(int B, int nC, int L, int C, const double* __restrict__ cj, double* __restrict__ dJdu) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  const int c = blockIdx.y + 1, g = blockIdx.z;
  if (b >= B || c >= C) return;
  double* q = dJdu + ((size_t)(2 * c * L) * nC + g) * B + b;
  *q += cj[((size_t)c * nC + g) * B + b];
}

__global__ void k_lq_set_row(int B, double* __restrict__ dst, const double* __restrict__ src) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b < B) dst[b] = src ? src[b] : 1.0;
}

static int lq_env_map() {
  static const int env = [] {
    const char* e = getenv("OCS_LQ_MAP");
    return e ? atoi(e) : 0;
  }();
  return env;
}
// how many chunks: groups x C = 2048 waves, two per SIMD (measured at 1024 trajectories, 2 x 4000 steps, pass pair: 1024 waves
// 7.8 ms, 2048 6.6 ms, 4096 6.6 ms; the X passes hold at most two waves per SIMD in registers); at most 64 chunks; chunks of
// at least 32 steps when chosen automatically (2 when the mapping is requested: tests, tuning).  OCS_LQ_CHUNK_WAVES
// overrides the wave target.
static bool lq_chunk_forced(int mapping) { return mapping == MAP_SCAN || (mapping == MAP_AUTO && lq_env_map() == 5); }
static int lq_chunks(int batch, int N, int mapping) {
  static const int target = [] {
    const char* e = getenv("OCS_LQ_CHUNK_WAVES");
    const int v = e ? atoi(e) : 0;
    return v > 0 ? v : 2048;
  }();
  const int groups = (batch + 15) / 16, minlen = lq_chunk_forced(mapping) ? 2 : 32;
  int C = target / groups;
  if (C > 64) C = 64;
  if (C > N / minlen) C = N / minlen;
  return C < 2 ? 1 : C;
}

template <int RT>
static int lq_chunk_matrices(LqWorkspace* w, const ProblemDesc& p, const GridDesc& g, int C, int L, hipStream_t s) {
  const int nS = p.nS, nU = 16 * RT;
  if (w->MT && w->key_ps == p.ps && w->key_version == p.version && w->key_rec == g.REC && w->key_C == C && w->key_N == g.N &&
      w->key_nS == nS)
    return 0;
  int rc;
  if ((rc = lq_ensure(w->MT, w->MT_cap, (size_t)C * nS * nU))) return rc;
  if ((rc = lq_ensure(w->unit, w->unit_cap, (size_t)C * nS * nU))) return rc;
  if (!w->zero_u) {
    if (hipMalloc((void**)&w->zero_u, 8 * sizeof(double)) != hipSuccess) return (int)hipErrorOutOfMemory;
    (void)hipMemsetAsync(w->zero_u, 0, 8 * sizeof(double), s);
  }
  // start states: the unit vectors, for every chunk ([C][nS][nU], trajectory j starts at e_j)
  std::vector<double> I((size_t)C * nS * nU, 0.0);
  for (int c = 0; c < C; ++c)
    for (int r = 0; r < nS; ++r) I[((size_t)c * nS + r) * nU + r] = 1.0;
  if (hipMemcpyAsync(w->unit, I.data(), I.size() * sizeof(double), hipMemcpyHostToDevice, s) != hipSuccess) return (int)hipErrorUnknown;
  if (hipStreamSynchronize(s) != hipSuccess) return (int)hipErrorUnknown;   // (I is a host temporary)
  LQArgs a{};
  a.N = g.N; a.batch = nU; a.nS = nS; a.nC = p.nC; a.REC = g.REC; a.ps = p.ps;
  a.u = w->zero_u; a.L = L; a.cs = w->unit; a.ce = w->MT;
  k_lq_forward<RT, false, true, 1><<<dim3(nU / 16, C), dim3(64), 0, s>>>(a);
  w->key_ps = p.ps; w->key_version = p.version; w->key_rec = g.REC; w->key_C = C; w->key_N = g.N; w->key_nS = nS;
  w->zc_valid = false;
  return hip_rc(hipGetLastError());
}

template <int RT, bool PW>
static int lq_forward_chunked(const ProblemDesc& p, const GridDesc& g, int batch, const double* x0, const double* u,
                              double* x, double* J, const FwdOpts& o, hipStream_t s) {
  LqWorkspace*& w = *g.lqws;
  if (!w) w = new LqWorkspace();
  const int N = g.N, nS = p.nS, nC = p.nC, nU = 16 * RT;
  const int C0 = lq_chunks(batch, N, o.mapping), L = (N + C0 - 1) / C0, C = (N + L - 1) / L;
  const size_t B = (size_t)batch;
  int rc;
  if ((rc = lq_chunk_matrices<RT>(w, p, g, C, L, s))) return rc;
  if ((rc = lq_ensure(w->cs, w->cs_cap, (size_t)C * nS * B))) return rc;
  if ((rc = lq_ensure(w->ce, w->ce_cap, (size_t)C * nS * B))) return rc;
  if ((rc = lq_ensure(w->cj, w->cj_cap, (size_t)C * (nC > 1 ? nC : 1) * B))) return rc;
  if ((rc = lq_ensure(w->off, w->off_cap, (size_t)(C + 1) * B))) return rc;
  LQArgs a{};
  a.N = N; a.batch = batch; a.nS = nS; a.nC = nC; a.REC = g.REC; a.ps = p.ps;
  a.x0 = x0; a.u = u; a.x = x; a.J = J; a.Jadd = o.Jadd; a.L = L; a.W = p.W;
  a.ub = o.uconst && o.uconst_batch ? batch : 0;
  const dim3 grid((batch + 15) / 16, C), block(64);
  // pass Z: every chunk from a zero state (cs of the carries is not read: zeros through a memset); it forms no objective, so
  // it reads no weights and is the same kernel with and without per-trajectory weights, like the chunk matrices
  if (hipMemsetAsync(w->cs, 0, (size_t)C * nS * B * sizeof(double), s) != hipSuccess) return (int)hipErrorUnknown;
  a.cs = w->cs; a.ce = w->ce;
  if (o.uconst && o.uconst_batch) {
    // a constant control of its own per trajectory: so is the zero-start response -- pass Z over the real batch, as below
    k_lq_forward<RT, false, true, 1><<<grid, block, 0, s>>>(a);
    k_lq_carry<false><<<dim3((batch + 63) / 64), dim3(256), 0, s>>>(nS, nU, batch, C, w->MT, x0, w->ce, w->cs, nullptr, batch);
  } else if (o.uconst) {
    // constant control: the zero-start response is one vector per chunk for the whole batch; kept with the matrices
    if (!w->zc_valid || w->zc_key_u != u || w->zc_key_uversion != o.uversion) {
      if ((rc = lq_ensure(w->zc, w->zc_cap, (size_t)C * nS * 16))) return rc;
      if ((rc = lq_ensure(w->zz, w->zz_cap, (size_t)C * nS * 16))) return rc;
      if (hipMemsetAsync(w->zz, 0, (size_t)C * nS * 16 * sizeof(double), s) != hipSuccess) return (int)hipErrorUnknown;
      LQArgs z = a;
      z.batch = 16; z.x = nullptr; z.J = nullptr; z.Jadd = nullptr; z.cs = w->zz; z.ce = w->zc;
      k_lq_forward<RT, false, true, 1><<<dim3(1, C), block, 0, s>>>(z);
      w->zc_key_u = u;
      w->zc_key_uversion = o.uversion;
      w->zc_valid = true;
    }
    k_lq_carry<false><<<dim3((batch + 63) / 64), dim3(256), 0, s>>>(nS, nU, batch, C, w->MT, x0, w->zc, w->cs, nullptr, 16);
  } else {
    k_lq_forward<RT, false, false, 1><<<grid, block, 0, s>>>(a);
    k_lq_carry<false><<<dim3((batch + 63) / 64), dim3(256), 0, s>>>(nS, nU, batch, C, w->MT, x0, w->ce, w->cs, nullptr, batch);
  }
  // pass X
  a.cj = w->cj; a.ce = nullptr;
  if (o.uconst) k_lq_forward<RT, true, true, 2, PW><<<grid, block, 0, s>>>(a);
  else if (x) k_lq_forward<RT, true, false, 2, PW><<<grid, block, 0, s>>>(a);
  else k_lq_forward<RT, false, false, 2, PW><<<grid, block, 0, s>>>(a);
  k_lq_cost_prefix<<<dim3((batch + 255) / 256), dim3(256), 0, s>>>(batch, C, w->cj, w->off, o.Jadd, J);
  if (x && N > L) k_lq_cost_fix<<<dim3((batch + 255) / 256, N - L), dim3(256), 0, s>>>(batch, nS, N, L, w->off, x);
  return hip_rc(hipGetLastError());
}

template <int RT, bool PW>
static int lq_backward_chunked(const ProblemDesc& p, const GridDesc& g, int batch, const double* xck, const double* u,
                               const double* lamT, double* lam, double* dJdu, const BwdOpts& o, hipStream_t s) {
  LqWorkspace*& w = *g.lqws;
  if (!w) w = new LqWorkspace();
  const int N = g.N, nS = p.nS, nC = p.nC, nU = 16 * RT;
  const int C0 = lq_chunks(batch, N, o.mapping), L = (N + C0 - 1) / C0, C = (N + L - 1) / L;
  const size_t B = (size_t)batch;
  int rc;
  if ((rc = lq_chunk_matrices<RT>(w, p, g, C, L, s))) return rc;
  if ((rc = lq_ensure(w->cs, w->cs_cap, (size_t)C * nS * B))) return rc;
  if ((rc = lq_ensure(w->ce, w->ce_cap, (size_t)C * nS * B))) return rc;
  if ((rc = lq_ensure(w->cj, w->cj_cap, (size_t)C * (nC > 1 ? nC : 1) * B))) return rc;
  LQArgs a{};
  a.N = N; a.batch = batch; a.nS = nS; a.nC = nC; a.REC = g.REC; a.ps = p.ps;
  a.xck = xck; a.u = u; a.lamT = lamT; a.L = L; a.W = p.W;
  a.ub = o.uconst && o.uconst_batch ? batch : 0;
  const dim3 grid((batch + 15) / 16, C), block(64);
  // pass Z: the objective's share of every chunk map (zero costate at the chunk's last node) -- with the trajectory's own q
  a.ce = w->ce;
  if (o.uconst) k_lq_backward<RT, false, false, true, 1, PW><<<grid, block, 0, s>>>(a);
  else k_lq_backward<RT, false, false, false, 1, PW><<<grid, block, 0, s>>>(a);
  // carries from the last node down; with a constant control (the tail leg of RK4InfiniteIntegrator.m:27-30) only
  // lam(:,1) is wanted, which is the carry below the first chunk
  double* last = nullptr;
  if (o.uconst) last = o.lam0;
  k_lq_carry<true><<<dim3((batch + 63) / 64), dim3(256), 0, s>>>(nS, nU, batch, C, w->MT, lamT, w->ce, w->cs, last, batch);
  if (o.uconst) {   // the constant objective row of lam(:,1)
    k_lq_set_row<<<dim3((batch + 255) / 256), dim3(256), 0, s>>>(batch, o.lam0 + (size_t)nS * B, lamT ? lamT + (size_t)nS * B : nullptr);
    return hip_rc(hipGetLastError());
  }
  a.ce = nullptr; a.cs = w->cs; a.cj = w->cj; a.lam = lam; a.dJdu = dJdu; a.lam0 = o.lam0;
  if (lam && dJdu) k_lq_backward<RT, true, true, false, 2, PW><<<grid, block, 0, s>>>(a);
  else if (lam) k_lq_backward<RT, true, false, false, 2, PW><<<grid, block, 0, s>>>(a);
  else k_lq_backward<RT, false, true, false, 2, PW><<<grid, block, 0, s>>>(a);
  if (dJdu && C > 1) k_lq_djdu_fix<<<dim3((batch + 255) / 256, C - 1, nC), dim3(256), 0, s>>>(batch, nC, L, C, w->cj, dJdu);
  return hip_rc(hipGetLastError());
}

// ---------------------------------------------------------------------------------------
// launchers
// ---------------------------------------------------------------------------------------
bool lq_supported(int nS, int nC) { return nS >= 1 && nS <= 32 && nC >= 1 && nC <= 4; }
// Which mapping a pass takes; m: the request (ocs_integrator_set_mapping), E: OCS_LQ_MAP (A/B timing).
// Chunks, automatic: up to 4096 trajectories (C >= 8).  Measured, nS = 32, nC = 4, 2 x 4000 steps, pass pair: 1024 trajectories
// 6.6 ms (four-wave kernels 28.5), 2048: ~12 (28.6), 4096: 21-23 (28.6); at 8192 the doubled work costs what the shorter chains
// gain (two-wave kernels 30.3 ms).  uconst (the tail leg of RK4InfiniteIntegrator.m:20-30): the state pass needs no pass Z of
// its own (the zero-start responses are one vector per chunk for the whole batch) and the adjoint wants nothing but lam2(:,1),
// the value at the far end of the horizon -- pass Z and the carries ARE that pass, there is no pass X; no doubled work, so
// chunks pay as soon as there are two of them (8192 trajectories: 4 chunks, 2048 one-wave groups instead of 1024 exchanging pairs).
// With a uStar per trajectory (FwdOpts::uconst_batch) the responses differ per trajectory and the state pass runs a real pass Z
// over the batch; the threshold is the shared form's (pass pair at 8192 trajectories 27.8 -> 34.8 ms, NOTES.md; not re-tuned).
// Four waves per 16 trajectories (K-split): E = 4 always, E = 2 never; request 3 forces it.  Automatic: while the four waves
// of a group still find SIMDs of their own (<= 4096 trajectories = 1024 waves).  Measured, nS = 32, nC = 4, 2 x 4000 steps, ms
// state pass / adjoint pass, two waves -> four waves:
//   batch 1024: 11.61 / 19.93 -> 11.02 / 18.08    2048: 11.61 / 19.99 -> 11.01 / 18.11    4096: 11.63 / 19.96 -> 11.12 / 18.26
//   8192 (two waves of different groups per SIMD): 11.77 / 20.04 -> 16.80 / 32.88
// A stage of M4 is 4 dependent matrix instructions + one LDS exchange of ~580 cycles that nothing of the same group can
// run under (every partial product is needed before the post); a stage of M2 is 8 matrix instructions with the exchange
// under the first four.  So M4 shortens the chain of a lone group by 5-9 % only, and two groups sharing a SIMD collide at
// the barriers instead of interleaving.  What bounds BL-5 at batch 8192 is the dependent tail of each stage (result
// latency of the last matrix instruction + the stage's vector update, ~200 of 730 cycles): with one independent wave per
// SIMD there is nothing to fill it with; the one-wave mapping at batch 16 384 (no exchange, one wave per SIMD) runs the
// adjoint pass at 58.6 TFLOP/s = 0.75 of the nominal peak.
// Two waves: request 2; automatic while that still leaves at most one wave per SIMD (1024 waves); beyond, the single-wave
// mapping has less overhead.
enum class LqMap { OneWave, TwoWaves, FourWaves, Chunks };
static LqMap lq_mapping(const GridDesc& g, int nS, int batch, int m, bool uconst) {
  const int E = lq_env_map();
  if (g.lqws) {
    if (lq_chunk_forced(m)) {
      if (lq_chunks(batch, g.N, m) >= 2) return LqMap::Chunks;
    } else if (m == MAP_AUTO && E == 0 && lq_chunks(batch, g.N, m) >= (uconst ? 2 : 8)) {
      return LqMap::Chunks;
    }
  }
  if (nS <= 16) return LqMap::OneWave;
  if (!(m == MAP_LANE || m == MAP_ROWSPLIT || E == 2) && (m == MAP_PIPELINE || E == 4 || batch <= 4096)) return LqMap::FourWaves;
  if (m != MAP_LANE && (m == MAP_ROWSPLIT || batch <= 8192)) return LqMap::TwoWaves;
  return LqMap::OneWave;
}

// the kernel families: trajectories and threads per workgroup, the instantiation of a pass for an output variant
template <int RT>
struct LqM1 {
  static constexpr int traj = 16, threads = 64;
  template <bool OUT_X, bool UCONST, bool PW> static constexpr auto forward = k_lq_forward<RT, OUT_X, UCONST, 0, PW>;
  template <bool OUT_LAM, bool OUT_DJDU, bool UCONST, bool PW> static constexpr auto backward = k_lq_backward<RT, OUT_LAM, OUT_DJDU, UCONST, 0, PW>;
};
struct LqM2 {
  static constexpr int traj = 32, threads = 256;
  template <bool OUT_X, bool UCONST, bool PW> static constexpr auto forward = k_lq2_forward<OUT_X, UCONST, PW>;
  template <bool OUT_LAM, bool OUT_DJDU, bool UCONST, bool PW> static constexpr auto backward = k_lq2_backward<OUT_LAM, OUT_DJDU, UCONST, PW>;
};
struct LqM4 {
  static constexpr int traj = 16, threads = 256;
  template <bool OUT_X, bool UCONST, bool PW> static constexpr auto forward = k_lq4_forward<OUT_X, UCONST, PW>;
  template <bool OUT_LAM, bool OUT_DJDU, bool UCONST, bool PW> static constexpr auto backward = k_lq4_backward<OUT_LAM, OUT_DJDU, UCONST, PW>;
};

// K: the kernel family; PW: per-trajectory cost weights (p.W)
template <class K, bool PW>
static void run_lq_forward(const LQArgs& a, bool uconst, hipStream_t s) {
  const dim3 grid((a.batch + K::traj - 1) / K::traj), block(K::threads);
  if (uconst)
    K::template forward<true, true, PW><<<grid, block, 0, s>>>(a);
  else if (a.x)
    K::template forward<true, false, PW><<<grid, block, 0, s>>>(a);
  else
    K::template forward<false, false, PW><<<grid, block, 0, s>>>(a);
}
template <bool PW>
static int lq_forward_dispatch(const ProblemDesc& p, const GridDesc& g, int batch, const double* x0, const double* u,
                               double* x, double* J, const FwdOpts& o, hipStream_t s) {
  LQArgs a{};
  a.N = g.N; a.batch = batch; a.nS = p.nS; a.nC = p.nC; a.REC = g.REC; a.ps = p.ps;
  a.x0 = x0; a.u = u; a.x = x; a.J = J; a.Jadd = o.Jadd; a.W = p.W;
  a.ub = o.uconst && o.uconst_batch ? batch : 0;
  switch (lq_mapping(g, p.nS, batch, o.mapping, o.uconst)) {
    case LqMap::Chunks:
      return p.nS <= 16 ? lq_forward_chunked<1, PW>(p, g, batch, x0, u, x, J, o, s) : lq_forward_chunked<2, PW>(p, g, batch, x0, u, x, J, o, s);
    case LqMap::OneWave:
      p.nS <= 16 ? run_lq_forward<LqM1<1>, PW>(a, o.uconst, s) : run_lq_forward<LqM1<2>, PW>(a, o.uconst, s);
      break;
    case LqMap::TwoWaves: run_lq_forward<LqM2, PW>(a, o.uconst, s); break;
    case LqMap::FourWaves: run_lq_forward<LqM4, PW>(a, o.uconst, s); break;
  }
  return hip_rc(hipGetLastError());
}
// fb_sweep's state pass (launch_sweep_forward_lq): the one-wave pass with every output, SWEEP
void lq_forward_one_wave(const LQArgs& a, hipStream_t s) {
  const dim3 grid((a.batch + 15) / 16), block(64);
  if (a.nS <= 16)
    k_lq_forward<1, true, false, 0, false, true><<<grid, block, 0, s>>>(a);
  else
    k_lq_forward<2, true, false, 0, false, true><<<grid, block, 0, s>>>(a);
}
// p.pmask: per-trajectory r, A or Bu -- no kernel reads them (the Jacobian is the shared A operand of the matrix instruction);
// p.W: per-trajectory q and rdiag for exactly `p.Wbatch` trajectories
int launch_forward_lq(const ProblemDesc& p, const GridDesc& g, int batch, const double* x0, const double* u,
                      double* x, double* J, const FwdOpts& o, hipStream_t s) {
  if (!lq_supported(p.nS, p.nC) || p.pmask || o.frozen || (o.uconst && !x)) return -1;
  if (p.W && p.Wbatch != batch) return -1;
  return p.W ? lq_forward_dispatch<true>(p, g, batch, x0, u, x, J, o, s) : lq_forward_dispatch<false>(p, g, batch, x0, u, x, J, o, s);
}

template <class K, bool PW>
static void run_lq_backward(const LQArgs& a, bool uconst, hipStream_t s) {
  const dim3 grid((a.batch + K::traj - 1) / K::traj), block(K::threads);
  if (uconst)
    K::template backward<false, false, true, PW><<<grid, block, 0, s>>>(a);
  else if (a.lam && a.dJdu)
    K::template backward<true, true, false, PW><<<grid, block, 0, s>>>(a);
  else if (a.lam)
    K::template backward<true, false, false, PW><<<grid, block, 0, s>>>(a);
  else
    K::template backward<false, true, false, PW><<<grid, block, 0, s>>>(a);
}
template <bool PW>
static int lq_backward_dispatch(const ProblemDesc& p, const GridDesc& g, int batch, const double* xck, const double* u,
                                const double* lamT, double* lam, double* dJdu, const BwdOpts& o, hipStream_t s) {
  LQArgs a{};
  a.N = g.N; a.batch = batch; a.nS = p.nS; a.nC = p.nC; a.REC = g.REC; a.ps = p.ps;
  a.xck = xck; a.u = u; a.lamT = lamT; a.lam = lam; a.dJdu = dJdu; a.lam0 = o.lam0; a.W = p.W;
  a.ub = o.uconst && o.uconst_batch ? batch : 0;
  switch (lq_mapping(g, p.nS, batch, o.mapping, o.uconst)) {
    case LqMap::Chunks:
      return p.nS <= 16 ? lq_backward_chunked<1, PW>(p, g, batch, xck, u, lamT, lam, dJdu, o, s)
                        : lq_backward_chunked<2, PW>(p, g, batch, xck, u, lamT, lam, dJdu, o, s);
    case LqMap::OneWave:
      p.nS <= 16 ? run_lq_backward<LqM1<1>, PW>(a, o.uconst, s) : run_lq_backward<LqM1<2>, PW>(a, o.uconst, s);
      break;
    case LqMap::TwoWaves: run_lq_backward<LqM2, PW>(a, o.uconst, s); break;
    case LqMap::FourWaves: run_lq_backward<LqM4, PW>(a, o.uconst, s); break;
  }
  return hip_rc(hipGetLastError());
}
int launch_backward_lq(const ProblemDesc& p, const GridDesc& g, int batch, const double* xck, const double* u,
                       const double* lamT, double* lam, double* dJdu, const BwdOpts& o, hipStream_t s) {
  if (!lq_supported(p.nS, p.nC) || p.pmask) return -1;
  if (p.W && p.Wbatch != batch) return -1;
  if (o.uconst ? (lam || dJdu || !o.lam0) : (!lam && !dJdu)) return -1;
  return p.W ? lq_backward_dispatch<true>(p, g, batch, xck, u, lamT, lam, dJdu, o, s)
             : lq_backward_dispatch<false>(p, g, batch, xck, u, lamT, lam, dJdu, o, s);
}

int launch_eval_lq(const ProblemDesc& p, int which, int k, const double* t, const double* y, const double* u,
                   const double* v, double* out, hipStream_t s) {
  if (p.W) return -1;   // k free columns have no trajectory index
  k_lq_eval<<<dim3((k + 127) / 128), dim3(128), 0, s>>>(which, k, p.nS, p.nC, t, y, u, v, p.ps, out);
  return hip_rc(hipGetLastError());
}

}  // namespace ocs
