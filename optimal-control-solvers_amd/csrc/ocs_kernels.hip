// ocs_kernels.hip -- gfx950 (MI355X) kernels for the batched RK4 state pass and its exact
// discrete adjoint.  fp64 throughout.
//
// Mapping ("L", lane-per-trajectory): one lane integrates one trajectory; a 64-lane wave
// (= one workgroup) owns 64 consecutive trajectories.  All per-step quantities that do not
// depend on the trajectory (step sizes, time coefficients) are wave-uniform and come from
// scalar loads.  Arrays are batch-minor ([time][row][batch]) so every vector load/store of a
// wave is one contiguous 512-B segment: coalescing needs no LDS staging in this mapping.
// The time recursion is serial, so at small batch the passes are bound by fp64 issue on one
// wave per SIMD, not by HBM; control samples and checkpoints are
// software-prefetched CH steps ahead in registers so that HBM latency stays off the chain.
//
// Reference semantics: Integrator/RK4Integrator.m:28-56 (compute_states), :59-94
// (compute_adjoints), :97-121 (compute_dJdu).  The reference caches all four stage states
// (xK); here only y_i is checkpointed and Y2..Y4 are recomputed in the adjoint pass (same
// arithmetic, deterministic => same values), which cuts checkpoint traffic 4x.
#include "ocs_device_common.hpp"
#include "ocs_internal.hpp"
#include "ocs_jit.hpp"
#include "ocs_problems.hpp"
#include "ocs_rk4_kernels.hpp"

namespace ocs {


// ---------------------------------------------------------------------------------------
// layout helpers: 64x64 LDS-tiled transposes between [batch][per] and [per][batch]
// ---------------------------------------------------------------------------------------
// src is R x Cc row-major (R rows of Cc), dst is Cc x R row-major.
__global__ __launch_bounds__(256) void k_transpose(const double* __restrict__ src, double* __restrict__ dst,
                                                   int R, int Cc) {
  __shared__ double tile[64][65];
  const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;  // 64 x 4
  const int c0 = blockIdx.x * 64, r0 = blockIdx.y * 64;
  for (int rr = ty; rr < 64; rr += 4) {
    const int r = r0 + rr, c = c0 + tx;
    if (r < R && c < Cc) tile[rr][tx] = src[(size_t)r * Cc + c];
  }
  __syncthreads();
  for (int cc = ty; cc < 64; cc += 4) {
    const int c = c0 + cc, r = r0 + tx;
    if (r < R && c < Cc) dst[(size_t)c * R + r] = tile[tx][cc];
  }
}

// straight 8-byte-per-lane copy: the known-byte-count reference for calibrating the HBM counters
__global__ __launch_bounds__(256) void k_copy8(const double* __restrict__ src, double* __restrict__ dst, size_t n) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) dst[i] = src[i];
}
int launch_copy8(const double* src, double* dst, size_t n, hipStream_t s) {
  k_copy8<<<dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s>>>(src, dst, n);
  return hip_rc(hipGetLastError());
}

__global__ void k_count_nonfinite(const double* __restrict__ v, int n, int* __restrict__ count) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  const bool bad = (i < n) && !isfinite(v[i]);
  const unsigned long long m = __ballot(bad);
  if ((threadIdx.x & 63) == 0 && m) atomicAdd(count, __popcll(m));
}

// ---------------------------------------------------------------------------------------
// dispatch
// ---------------------------------------------------------------------------------------

bool functor_supported(Functor f, int nS, int nC) {
  if (f == Functor::User) return true;
  if (f == Functor::LQ) return lq_supported(nS, nC);
  if (f == Functor::Logistic) return nS >= 1 && nS <= 4 && nC == 1;
  return false;
}
int functor_ntc(Functor f, int nS) {
  (void)nS;
  if (f == Functor::User || f == Functor::LQ) return 1;
  if (f == Functor::Logistic) return LogisticK<1>::NTC;
  return 0;
}
int functor_ntu(Functor f, int nS) {
  (void)nS;
  if (f == Functor::User || f == Functor::LQ) return 1;
  if (f == Functor::Logistic) return LogisticK<1>::NTU;
  return 0;
}
unsigned functor_tc_param_mask(Functor f, int nS) {
  (void)nS;
  if (f == Functor::User) return 0u;
  if (f == Functor::LQ) return 1u;  // r feeds the e^{-rt} table
  if (f == Functor::Logistic) return LogisticK<1>::TC_PARAM_MASK;
  return 0;
}

template <class P>
static void run_tcoef(const ProblemDesc& p, const GridDesc& g, hipStream_t s) {
  const int nT = 2 * g.N + 1;
  k_tcoef<P><<<dim3((nT + 255) / 256), dim3(256), 0, s>>>(nT, g.T, p.ps, g.TC, g.TU);
  k_build_rec<P><<<dim3((g.N + 2 * kRecPad + 255) / 256), dim3(256), 0, s>>>(g.N, g.HT, g.TC, g.REC);
}
int launch_tcoef(const ProblemDesc& p, const GridDesc& g, hipStream_t s) {
  if (p.functor == Functor::User) {
    int nT = 2 * g.N + 1, N = g.N;
    const double *T = g.T, *ps = p.ps, *HT = g.HT;
    double *TC = g.TC, *TU = g.TU, *REC = g.REC;
    void* a1[] = {&nT, &T, &ps, &TC, &TU};
    int rc = jit_launch(p.user, UK_TCOEF, dim3((nT + 255) / 256), dim3(256), a1, s);
    if (rc) return rc;
    const double* TCc = g.TC;
    void* a2[] = {&N, &HT, &TCc, &REC};
    return jit_launch(p.user, UK_BUILD_REC, dim3((N + 2 * kRecPad + 255) / 256), dim3(256), a2, s);
  }
  if (p.functor == Functor::LQ) return launch_tcoef_lq(p, g, s);
  if (!for_logistic<1, 2, 3, 4>(p.nS, [&](auto P) { run_tcoef<decltype(P)>(p, g, s); })) return -1;
  return hip_rc(hipGetLastError());
}
// the same two tables at nq times of the caller's (no step records): TCQ [nq][NTC], TUQ [nq][NTU]
int launch_tcoef_at(const ProblemDesc& p, int nq, const double* tq, double* TCQ, double* TUQ, hipStream_t s) {
  const dim3 grid((nq + 255) / 256), block(256);
  if (p.functor == Functor::User) {
    const double* ps = p.ps;
    void* args[] = {&nq, &tq, &ps, &TCQ, &TUQ};
    return jit_launch(p.user, UK_TCOEF, grid, block, args, s);
  }
  if (p.functor != Functor::Logistic) return -1;
  if (!for_logistic<1, 2, 3, 4>(p.nS, [&](auto P) { k_tcoef<decltype(P)><<<grid, block, 0, s>>>(nq, tq, p.ps, TCQ, TUQ); }))
    return -1;
  return hip_rc(hipGetLastError());
}
int rec_stride_host(int ntc) { return rec_stride(ntc); }
int rec_sc_offset_host(int ntc) { return rec_sc_offset(ntc); }
int rec_pad_host() { return kRecPad; }

constexpr int kChunk = 4;
// step records in flight: a divisor of 2*kChunk so the ring needs no register rotation at the loop
// back-edge; deeper for the small problems, whose register budget is loose and which run with few waves
template <class P>
constexpr int pf_of() { return P::NS <= 2 ? 4 : 3; }

// the lane adjoint kernel with checkpoint re-integration (k_backward<..., XRC>): where the launch fills the chip and the pass is
// HBM-bound (OCS_LANE_XRC_MIN: batch from which it is taken; 0 = never)
static int lane_xrc_min_batch() {
  static const int v = [] {
    const char* e = getenv("OCS_LANE_XRC_MIN");
    return e ? atoi(e) : 32768;
  }();
  return v;
}
template <class P>
static void run_forward(const FwdArgs& a, bool uconst, hipStream_t s) {
  const dim3 grid((a.batch + 63) / 64), block(64);
  if (uconst)
    k_forward<P, kChunk, pf_of<P>(), true, true><<<grid, block, 0, s>>>(a);
  else if (a.x && lane_xrc_min_batch() > 0 && a.batch >= lane_xrc_min_batch())
    k_forward<P, kChunk, pf_of<P>(), true, false, true><<<grid, block, 0, s>>>(a);   // (non-temporal stores of x)
  else if (a.x)
    k_forward<P, kChunk, pf_of<P>(), true, false><<<grid, block, 0, s>>>(a);
  else
    k_forward<P, kChunk, pf_of<P>(), false, false><<<grid, block, 0, s>>>(a);
}
// Mapping selection, measured on MI355X with the kernels of round 4 (LogisticK, N = 1000; us per pass; scripts/pair_loop.py,
// profiles/r04_pair_by_batch_mapping.log) by workgroups of the wave-specialised kernels (one per 64/nS trajectories):
//   workgroups      state pass: lane / pipeline            adjoint pass: lane / scan
//                   nS = 1      nS = 2      nS = 4          nS = 1        nS = 2       nS = 4
//      512         256 / 267   209 / 131   297 / 124       351 / 300     296 / 205    439 / 166
//     1024         434 / 545   285 / 267   342 / 241       647 / 630     429 / 416    466 / 370
//     2048         837 / 1026  499 / 553   452 / 500      1297 / 1191    791 / 825    639 / 737
//     4096        1762 / 2046 1004 / 1052  673 / 892      2736 / 2438   1598 / 1628  1172 / 1435
// The wave-specialised kernels win while the serial chain sets the time -- up to 1024 workgroups (512 with one state, where a
// lane kernel already has a wave per row) --; beyond that the lane kernels have the fewest instructions per trajectory and both
// passes are HBM-bound (only the one-state scan still matches its lane kernel).  Row-split: while the lane mapping would leave most
// SIMDs idle and the pipeline does not apply.
// The pipeline kernels take whole blocks of 8 steps.  Other step counts are split: the first 8*floor(N/8) steps
// go through the pipeline kernel, the remaining (< 8) through the lane kernel, which continues from / hands over
// the boundary column (running objective, lamT, the k1 half of the boundary column of dJdu), so the result is
// the one-kernel result bit for bit.  splits(): 0 = no pipeline, else the number of pipeline steps.
static int pipeline_steps(const ProblemDesc& p, int N, int batch, bool backward) {
  const int D = pipeline_block_steps(), N1 = (N / D) * D;
  // (user problems given as row functions have the state-pass kernel only: their adjoint pass is the scan)
  if (backward ? !pipeline_supported(p.functor, p.nS, p.nC) : !pipeline_problem_ok(p)) {
    // any other problem with nS <= 4, nC <= 2: the vector-lane state pass (whole tiles of 64 trajectories)
    if (!backward && vector_problem_ok(p) && N1 >= D && batch >= 64 && tile_ok(batch, 64)) return N1;
    return 0;
  }
  if (N1 < D || !pipeline_shape_ok(p.nS, N1, batch, backward)) return 0;
  return N1;
}
static bool forward_is_vector(const ProblemDesc& p) { return !pipeline_problem_ok(p) && vector_problem_ok(p); }
// boundary: the caller's output arrays can carry the hand-over column of a split pass (x forward, lam backward)
// Accuracy: MAP_PIPELINE's state pass rounds at the size of m_r/2 (recursion on z = y - m_r/2); states orders of magnitude below
// that lose relative precision there and not on MAP_LANE / MAP_ROWSPLIT.  The choice below cannot see the states: DESIGN.md 3.
static int choose_mapping(const ProblemDesc& p, int N, int batch, int requested, bool plain, bool backward,
                          bool boundary) {
  if (requested != MAP_AUTO) return requested;
  const int N1 = plain ? pipeline_steps(p, N, batch, backward) : 0;
  const int tpw = (!backward && forward_is_vector(p)) ? 64 : 64 / p.nS;
  const int wgmax = (p.nS == 1 || tpw == 64 || backward) ? 512 : 1024;
  if (N1 > 0 && (N1 == N || boundary) && batch / tpw <= wgmax) return MAP_PIPELINE;
  if (plain && rowsplit_supported(p.functor, p.nS, p.nC) && batch <= 8192) return MAP_ROWSPLIT;
  return MAP_LANE;
}

// Scan against the serial mappings: the scan does ~2x the arithmetic of a serial adjoint step but has no
// dependent chain over time; it wins wherever the serial kernels are latency-bound (every batch measured so far).
// ... wherever the serial kernels are latency-bound: up to 1024 workgroups (table above); with one state at every batch.
// Beyond that the lane kernel re-integrates three of four checkpoints (k_backward<..., XRC>, from batch 32768) and wins with two
// and four states: adjoint pass at batch 65536, scan / lane / lane with re-integration: nS = 4 1435 / 1185 / 903 us, nS = 2
// 825 / 811 / 720; nS = 1 at 131072: 1191 / 1327 / 1167 (level: the scan stays).
static bool scan_pays(int nS, int N, int batch) {
  return N >= 8 && (nS == 1 || batch / (64 / nS) <= 1024);
}

// the wave-specialised state passes on whole horizons (the two-kernel sweep and the fused control update are built on them)
int fold_wg_limit() {
  static const int v = [] {
    const char* e = getenv("OCS_FOLD_MAX_WG");
    const int n = e ? atoi(e) : 0;
    return n > 0 ? n : (1 << 30);   // no limit: at 1024-4096 workgroups the folded sweep is 1.3-2.2x faster than the lane sequence
                                    // (profiles/r04_fbs_by_batch_fold_limit.log; until round 4 the limit was 512)
  }();
  return v;
}
bool forward_gate_supported(const ProblemDesc& p, const GridDesc& g, int batch) {
  if (p.functor == Functor::LQ) return false;
  const int tpw = forward_is_vector(p) ? 64 : 64 / p.nS;
  return pipeline_steps(p, g.N, batch, false) == g.N && g.N > 0 && batch / tpw <= fold_wg_limit();
}
bool tail_leg_wave_ok(const ProblemDesc& p, const GridDesc& g, int batch) {
  if (p.functor == Functor::LQ) return false;
  return choose_mapping(p, g.N, batch, MAP_AUTO, true, false, true) == MAP_PIPELINE;
}
// ---------------------------------------------------------------------------------------
// the pass pair on tiled arrays: pipeline + scan at every batch, the steps past the last whole block / chunk on the lane kernels
// ---------------------------------------------------------------------------------------
bool tiled_supported(const ProblemDesc& p) {
  return pipeline_supported(p.functor, p.nS, p.nC) && scan_supported(p.functor, p.nS, p.nC) && !p.pb;
}
template <class P>
static void run_forward_tiled(const FwdArgsTiled& t, hipStream_t s) {
  const dim3 grid((t.a.batch + 63) / 64), block(64);
  if (t.a.x)
    k_forward_tiled<P, kChunk, pf_of<P>(), true><<<grid, block, 0, s>>>(t);
  else
    k_forward_tiled<P, kChunk, pf_of<P>(), false><<<grid, block, 0, s>>>(t);
}
template <class P>
static void run_backward_tiled(const BwdArgsTiled& t, hipStream_t s) {
  const dim3 grid((t.a.batch + 63) / 64), block(64);
  if (t.a.lam && t.a.dJdu)
    k_backward_tiled<P, kChunk, pf_of<P>(), true, true><<<grid, block, 0, s>>>(t);
  else if (t.a.lam)
    k_backward_tiled<P, kChunk, pf_of<P>(), true, false><<<grid, block, 0, s>>>(t);
  else
    k_backward_tiled<P, kChunk, pf_of<P>(), false, true><<<grid, block, 0, s>>>(t);
}
static int launch_forward_tiled(const ProblemDesc& p, const GridDesc& g, int batch, const double* x0, const double* u,
                                double* x, double* J, const FwdOpts& o, hipStream_t s) {
  const bool map_ok = o.mapping == MAP_AUTO || o.mapping == MAP_PIPELINE || o.mapping == MAP_SCAN;
  if (!tiled_supported(p) || !map_ok || o.uconst || o.Jadd || o.frozen || o.gate || g.N < 1 || batch < 1) return -1;
  const int D = pipeline_block_steps(), N1 = (g.N / D) * D, nodes = g.N + 1;
  if (N1 > 0 && N1 < g.N && !x) return -1;   // the split needs the boundary column in memory
  if (N1 > 0) {
    GridDesc g1 = g;
    g1.N = N1;
    const int rc = launch_forward_p2_tiled(p, g1, nodes, batch, x0, u, x, J, s);
    if (rc || N1 == g.N) return rc;
  }
  // steps N1 .. N-1 on the lane kernel, continuing from column N1 of the tiled x (N1 = 0: the whole pass, from x0)
  const size_t xrow = kTile, xcol = (size_t)(p.nS + 1) * kTile, ucol = (size_t)p.nC * kTile;
  double* xb = x ? x + (size_t)N1 * xcol : nullptr;
  const FwdArgs a{g.N - N1, batch, g.REC + (size_t)N1 * rec_stride_host(functor_ntc(p.functor, p.nS)), p.ps, nullptr, 0u,
                  N1 > 0 ? xb : x0, u + (size_t)(2 * N1) * ucol, xb, J, nullptr, nullptr, nullptr,
                  N1 > 0 ? xb + (size_t)p.nS * xrow : nullptr};
  const FwdArgsTiled t{a, nodes, N1 > 0 ? 1 : 0};
  if (!for_logistic<1, 2, 4>(p.nS, [&](auto P) { run_forward_tiled<decltype(P)>(t, s); })) return -1;
  return hip_rc(hipGetLastError());
}
static int launch_backward_tiled(const ProblemDesc& p, const GridDesc& g, int batch, const double* xck, const double* u,
                                 const double* lamT, double* lam, double* dJdu, const BwdOpts& o, hipStream_t s) {
  const bool map_ok = o.mapping == MAP_AUTO || o.mapping == MAP_PIPELINE || o.mapping == MAP_SCAN;
  if (!tiled_supported(p) || !map_ok || o.uconst || (!lam && !dJdu) || g.N < 1 || batch < 1) return -1;
  const int Ls = scan_chunk_steps(), N1 = (g.N / Ls) * Ls, nodes = g.N + 1;
  if (N1 == g.N) return launch_backward_scan_tiled(p, g, nodes, batch, xck, u, lamT, false, lam, dJdu, o.lam0, nullptr, s);
  if (N1 > 0 && !lam && !o.split_scratch) return -1;
  // steps N-1 .. N1 first, on the lane kernel (as split_at of launch_backward): lam columns N1 .. N, dJdu columns 2 N1 .. 2 N
  const size_t xcol = (size_t)(p.nS + 1) * kTile, ucol = (size_t)p.nC * kTile;
  double* lamb = lam ? lam + (size_t)N1 * xcol : o.split_scratch;   // lam(:, N1): a tiled column, or a [nAug][B] vector
  double* db = dJdu ? dJdu + (size_t)(2 * N1) * ucol : nullptr;
  const BwdArgs a{g.N - N1, batch, g.REC + (size_t)N1 * rec_stride_host(functor_ntc(p.functor, p.nS)), p.ps, nullptr, 0u,
                  xck + (size_t)N1 * xcol, u + (size_t)(2 * N1) * ucol, lamT, lam ? lamb : nullptr, db,
                  N1 == 0 ? o.lam0 : (lam ? nullptr : lamb)};
  const BwdArgsTiled t{a, nodes};
  if (!for_logistic<1, 2, 4>(p.nS, [&](auto P) { run_backward_tiled<decltype(P)>(t, s); })) return -1;
  const int rc = hip_rc(hipGetLastError());
  if (rc || N1 == 0) return rc;
  GridDesc g1 = g;
  g1.N = N1;
  return launch_backward_scan_tiled(p, g1, nodes, batch, xck, u, lamb, lam != nullptr, lam, dJdu, o.lam0, db, s);
}

// FwdOpts::gate: honoured by any state pass the sweep launches with `frozen` set (pipeline kernels, split passes, the lane
// kernel), refused on the LQ functor (the sweep runs that problem's plugin twin or its own matrix-core passes)
int launch_forward(const ProblemDesc& p, const GridDesc& g, int batch, const double* x0, const double* u,
                   double* x, double* J, const FwdOpts& o, hipStream_t s) {
  if (o.layout == LAYOUT_TILED) return launch_forward_tiled(p, g, batch, x0, u, x, J, o, s);
  if (o.gate && (o.mapping != MAP_AUTO || o.uconst || o.Jadd || p.functor == Functor::LQ || !o.frozen)) return -1;
  if (p.functor == Functor::LQ) return launch_forward_lq(p, g, batch, x0, u, x, J, o, s);
  const bool plain = !o.uconst && !o.Jadd;
  // (MAP_SCAN names the adjoint kernel; the state pass of such an integrator is chosen automatically)
  int map = choose_mapping(p, g.N, batch, o.mapping == MAP_SCAN ? MAP_AUTO : o.mapping, plain, false, x != nullptr);
  if (map == MAP_ROWSPLIT && o.frozen && o.mapping == MAP_AUTO) map = MAP_LANE;  // not in that kernel
  if (map == MAP_PIPELINE) {
    const int N1 = plain ? pipeline_steps(p, g.N, batch, false) : 0;
    if (N1 == 0 || (N1 < g.N && !x)) return -1;  // the split needs the boundary column in memory
    GridDesc g1 = g;
    g1.N = N1;
    // (a split pass hands the running objective to the lane kernel through the boundary column: keep the row then)
    int rc;
    if (forward_is_vector(p)) {
      rc = launch_forward_pv(p, g1, batch, x0, u, x, J, s, o.no_cost_row && N1 == g.N, o.gate, o.frozen);
    } else {
      if (o.frozen && !o.dump) return -1;  // the lane kernel that finishes a split pass stores to dump
      rc = launch_forward_p2(p, g1, batch, x0, u, x, J, o.frozen, s, o.no_cost_row && N1 == g.N, o.gate);
    }
    if (rc || N1 == g.N) return rc;
    // remaining steps N1 .. N-1 on the lane kernel, continuing from column N1 (state rows and running objective)
    const size_t col = (size_t)(p.nS + 1) * batch, ucol = (size_t)p.nC * batch;
    double* xb = x + (size_t)N1 * col;
    FwdArgs a{g.N - N1, batch, g.REC + (size_t)N1 * rec_stride_host(functor_ntc(p.functor, p.nS)), p.ps, p.pb,
              p.pmask, xb, u + (size_t)(2 * N1) * ucol, xb, J, nullptr, o.frozen, o.dump, xb + (size_t)p.nS * batch};
    a.gate = o.gate;
    if (p.functor == Functor::User) {
      void* args[] = {(void*)&a};
      return jit_launch(p.user, UK_FWD_X, dim3((batch + 63) / 64), dim3(64), args, s);
    }
    if (!for_logistic<1, 2, 3, 4>(p.nS, [&](auto P) { run_forward<decltype(P)>(a, false, s); })) return -1;
    return hip_rc(hipGetLastError());
  }
  if (map == MAP_ROWSPLIT) {
    if (!plain || o.frozen || !rowsplit_supported(p.functor, p.nS, p.nC)) return -1;
    return launch_forward_rs(p, g, batch, x0, u, x, J, s);
  }
  if (o.uconst && !x) return -1;
  FwdArgs a{g.N, batch, g.REC, p.ps, p.pb, p.pmask, x0, u, x, J, o.Jadd, o.frozen, o.dump, nullptr};
  a.gate = o.gate;
  a.ub = o.uconst && o.uconst_batch ? batch : 0;
  if (p.functor == Functor::User) {
    void* args[] = {(void*)&a};
    const int kid = o.uconst ? UK_FWD_UCONST : (x ? UK_FWD_X : UK_FWD_J);
    return jit_launch(p.user, kid, dim3((batch + 63) / 64), dim3(64), args, s);
  }
  if (!for_logistic<1, 2, 3, 4>(p.nS, [&](auto P) { run_forward<decltype(P)>(a, o.uconst, s); })) return -1;
  return hip_rc(hipGetLastError());
}

template <class P>
static void run_backward(const BwdArgs& a, bool uconst, hipStream_t s) {
  const dim3 grid((a.batch + 63) / 64), block(64);
  const int xmin = lane_xrc_min_batch();
  if (!uconst && xmin > 0 && a.batch >= xmin && a.N >= kChunk) {
    if (a.lam && a.dJdu)
      k_backward<P, kChunk, kChunk, true, true, false, true><<<grid, block, 0, s>>>(a);
    else if (a.lam)
      k_backward<P, kChunk, kChunk, true, false, false, true><<<grid, block, 0, s>>>(a);
    else
      k_backward<P, kChunk, kChunk, false, true, false, true><<<grid, block, 0, s>>>(a);
    return;
  }
  if (uconst)
    k_backward<P, kChunk, pf_of<P>(), false, false, true><<<grid, block, 0, s>>>(a);
  else if (a.lam && a.dJdu)
    k_backward<P, kChunk, pf_of<P>(), true, true, false><<<grid, block, 0, s>>>(a);
  else if (a.lam)
    k_backward<P, kChunk, pf_of<P>(), true, false, false><<<grid, block, 0, s>>>(a);
  else
    k_backward<P, kChunk, pf_of<P>(), false, true, false><<<grid, block, 0, s>>>(a);
}
int launch_backward(const ProblemDesc& p, const GridDesc& g, int batch, const double* xck, const double* u,
                    const double* lamT, double* lam, double* dJdu, const BwdOpts& o, hipStream_t s) {
  if (o.layout == LAYOUT_TILED) return launch_backward_tiled(p, g, batch, xck, u, lamT, lam, dJdu, o, s);
  if (p.functor == Functor::LQ) return launch_backward_lq(p, g, batch, xck, u, lamT, lam, dJdu, o, s);
  const bool plain = !o.uconst;
  int map = choose_mapping(p, g.N, batch, o.mapping, plain, true, lam != nullptr);
  // the adjoint pass as a scan over time: whenever the problem is row-separable (any N, any batch); the serial
  // mappings remain selectable
  // The scan takes whole chunks of L steps; other step counts are split as for the pipeline mapping: steps N1..N-1
  // first on the lane kernel (which hands lam(:, N1) and the k1 half of column 2 N1 over through the output arrays),
  // so a split pass needs the lam array.
  const int Ls = scan_chunk_steps(), Ns = (g.N / Ls) * Ls;
  const bool scan_ok = plain && g.RECS && scan_problem_ok(p) && Ns >= Ls && (Ns == g.N || lam || o.split_scratch);
  if (o.mapping == MAP_AUTO && scan_ok && scan_pays(p.nS, g.N, batch)) map = MAP_SCAN;
  // any other problem with nS <= 4, nC <= 2: the scan with dense step maps, while the lane kernel would leave most of
  // the chip idle (it does (nS + 2) times the arithmetic of a serial step)
  const bool vscan = !scan_ok && plain && g.RECS && vector_problem_ok(p) && Ns >= Ls && (Ns == g.N || lam || o.split_scratch);
  // (measured again with round 4's kernels, us per adjoint pass, dense-map scan / lane kernel: nS = 1 at batch 16384 176 / 236,
  //  32768 365 / 365, 49152 556 / 510; nS = 2 at 16384 271 / 447, 24576 470 / 486, 32768 540 / 496; nS = 4 at 8192 381 / 422,
  //  16384 415 / 428, 24576 775 / 520 -- profiles/r04_user_vector_pair_by_batch_mapping.log)
  if (o.mapping == MAP_AUTO && vscan && g.N >= 8 && batch <= 16384 * 6 / (p.nS + 2)) map = MAP_SCAN;
  auto scan_launch = [&](const GridDesc& gg, const double* lT, const double* pend0) {
    return vscan ? launch_backward_vscan(p, gg, batch, xck, u, lT, lam, dJdu, o.lam0, pend0, s)
                 : launch_backward_scan(p, gg, batch, xck, u, lT, lam, dJdu, o.lam0, pend0, s);
  };
  // A split pass: steps N-1 .. N1 first, on the lane kernel -- lam columns N1..N, dJdu columns 2 N1 .. 2 N (column 2 N1 holds
  // the k1 half only, RK4Integrator.m:108-112) -- then whole(g1, lamb, db): the whole blocks or chunks below, started from
  // lam(:, N1) and adding their k4 half to column 2 N1.
  auto split_at = [&](int N1, auto&& whole) -> int {
    const size_t col = (size_t)(p.nS + 1) * batch, ucol = (size_t)p.nC * batch;
    double* lamb = lam ? lam + (size_t)N1 * col : o.split_scratch;   // lam(:, N1): in the output array, or as lam0
    double* db = dJdu ? dJdu + (size_t)(2 * N1) * ucol : nullptr;
    const BwdArgs a{g.N - N1, batch, g.REC + (size_t)N1 * rec_stride_host(functor_ntc(p.functor, p.nS)), p.ps, p.pb,
                    p.pmask, xck + (size_t)N1 * col, u + (size_t)(2 * N1) * ucol, lamT, lam ? lamb : nullptr, db,
                    lam ? nullptr : lamb};
    int rc;
    if (p.functor == Functor::User) {
      void* args[] = {(void*)&a};
      rc = jit_launch(p.user, a.lam && a.dJdu ? UK_BWD_LAM_DJDU : (a.lam ? UK_BWD_LAM : UK_BWD_DJDU),
                      dim3((batch + 63) / 64), dim3(64), args, s);
    } else {
      if (!for_logistic<1, 2, 3, 4>(p.nS, [&](auto P) { run_backward<decltype(P)>(a, false, s); })) return -1;
      rc = hip_rc(hipGetLastError());
    }
    if (rc) return rc;
    GridDesc g1 = g;
    g1.N = N1;
    return whole(g1, lamb, db);
  };
  if (map == MAP_SCAN) {
    if (!scan_ok && !vscan) return -1;
    if (Ns == g.N) return scan_launch(g, lamT, nullptr);
    return split_at(Ns, scan_launch);
  }
  if (map == MAP_PIPELINE) {
    const int N1 = plain ? pipeline_steps(p, g.N, batch, true) : 0;
    if (N1 == 0 || (N1 < g.N && !lam)) return -1;  // the split hands lam(:, N1) over through memory
    if (N1 == g.N) return launch_backward_pl(p, g, batch, xck, u, lamT, lam, dJdu, o.lam0, nullptr, s);
    return split_at(N1, [&](const GridDesc& g1, const double* lamb, const double* db) {
      return launch_backward_pl(p, g1, batch, xck, u, lamb, lam, dJdu, o.lam0, db, s);
    });
  }
  if (map == MAP_ROWSPLIT) {
    if (!plain || !rowsplit_supported(p.functor, p.nS, p.nC)) return -1;
    return launch_backward_rs(p, g, batch, xck, u, lamT, lam, dJdu, o.lam0, s);
  }
  if (o.uconst ? (lam || dJdu || !o.lam0) : (!lam && !dJdu)) return -1;
  const BwdArgs a{g.N, batch, g.REC, p.ps, p.pb, p.pmask, xck, u, lamT, lam, dJdu, o.lam0,
                  o.uconst && o.uconst_batch ? batch : 0};
  if (p.functor == Functor::User) {
    void* args[] = {(void*)&a};
    int kid = o.uconst ? UK_BWD_UCONST : (lam && dJdu ? UK_BWD_LAM_DJDU : (lam ? UK_BWD_LAM : UK_BWD_DJDU));
    const int xmin = lane_xrc_min_batch();   // (as for the registry problems: re-integration where the launch is HBM-bound)
    if (kid == UK_BWD_LAM_DJDU && xmin > 0 && batch >= xmin && g.N >= 4 && p.nS <= 4) kid = UK_BWD_LAM_DJDU_XRC;
    return jit_launch(p.user, kid, dim3((batch + 63) / 64), dim3(64), args, s);
  }
  if (!for_logistic<1, 2, 3, 4>(p.nS, [&](auto P) { run_backward<decltype(P)>(a, o.uconst, s); })) return -1;
  return hip_rc(hipGetLastError());
}

template <class P>
static void run_eval(const ProblemDesc& p, int which, int k, const double* t, const double* y, const double* u,
                     const double* v, double* out, hipStream_t s) {
  k_eval<P><<<dim3((k + 127) / 128), dim3(128), 0, s>>>(which, k, t, y, u, v, p.ps, out, p.lb, p.ub);
}
int launch_eval(const ProblemDesc& p, int which, int k, const double* t, const double* y, const double* u,
                const double* v, double* out, hipStream_t s) {
  if (p.functor == Functor::User) {
    const double *ps = p.ps, *lb = p.lb, *ub = p.ub;
    void* args[] = {&which, &k, &t, &y, &u, &v, &ps, &out, &lb, &ub};
    return jit_launch(p.user, UK_EVAL, dim3((k + 127) / 128), dim3(128), args, s);
  }
  if (p.functor == Functor::LQ) return which == 3 ? -1 : launch_eval_lq(p, which, k, t, y, u, v, out, s);   // (ControlChar: its plugin twin)
  if (!for_logistic<1, 2, 3, 4>(p.nS, [&](auto P) { run_eval<decltype(P)>(p, which, k, t, y, u, v, out, s); })) return -1;
  return hip_rc(hipGetLastError());
}

template <class P>
static void run_equilibrium(const EqArgs& a, hipStream_t s) {
  k_equilibrium<P><<<dim3((a.batch + 63) / 64), dim3(64), 0, s>>>(a);
}
int launch_equilibrium(const ProblemDesc& p, int batch, double r, const double* y0, const double* lb, const double* ub,
                       double* y, double* resnorm, double* residual, int* exitflag, int max_iter, double tol,
                       hipStream_t s) {
  const EqArgs a{batch, r, p.ps, p.pb, p.pmask, y0, lb, ub, y, resnorm, residual, exitflag, max_iter, tol};
  if (p.functor == Functor::User) {
    void* args[] = {(void*)&a};
    return jit_launch(p.user, UK_EQUILIBRIUM, dim3((batch + 63) / 64), dim3(64), args, s);
  }
  if (p.functor != Functor::Logistic) return -1;
  if (!for_logistic<1, 2, 3, 4>(p.nS, [&](auto P) { run_equilibrium<decltype(P)>(a, s); })) return -1;
  return hip_rc(hipGetLastError());
}

// traj-major [batch][per]  ->  batch-minor [per][batch]
int launch_to_batch_minor(const double* src, double* dst, int per, int batch, hipStream_t s) {
  hipLaunchKernelGGL(k_transpose, dim3((per + 63) / 64, (batch + 63) / 64), dim3(256), 0, s, src, dst, batch,
                     per);
  return hip_rc(hipGetLastError());
}
// batch-minor [per][batch]  ->  traj-major [batch][per]
int launch_to_traj_major(const double* src, double* dst, int per, int batch, hipStream_t s) {
  hipLaunchKernelGGL(k_transpose, dim3((batch + 63) / 64, (per + 63) / 64), dim3(256), 0, s, src, dst, per,
                     batch);
  return hip_rc(hipGetLastError());
}

// batch-minor [nR][batch] (nR = cols * rows) <-> tiled [tiles][nR][16] (ocs_device_common.hpp).  A workgroup moves 64 rows of
// four tiles through LDS: on the batch-minor side a wave touches 64 consecutive trajectories of a row (512 bytes), on the
// tiled side the 64 rows of a tile in one run (8 KiB).  TO: the pad lanes of the last tile get the last trajectory.
template <bool TO>
__global__ __launch_bounds__(256) void k_tiled_convert(const double* __restrict__ src, double* __restrict__ dst, int nR,
                                                       int batch) {
  __shared__ double tile[64][65];
  const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
  const int R0 = blockIdx.x * 64, b0 = blockIdx.y * 64;
  const int ntiles = (int)tiled_tiles((size_t)batch);
  const size_t ts = (size_t)nR * kTile;
  if (TO) {
    const int b = b0 + tx < batch ? b0 + tx : batch - 1;
    for (int rr = ty; rr < 64; rr += 4)
      if (R0 + rr < nR) tile[rr][tx] = src[(size_t)(R0 + rr) * batch + b];
  } else {
    for (int k = threadIdx.x; k < 4 * 64 * kTile; k += 256) {
      const int tq = k / (64 * kTile), rr = (k / kTile) % 64, l = k % kTile, t = b0 / kTile + tq;
      if (t < ntiles && R0 + rr < nR) tile[rr][tq * kTile + l] = src[(size_t)t * ts + (size_t)(R0 + rr) * kTile + l];
    }
  }
  __syncthreads();
  if (TO) {
    for (int k = threadIdx.x; k < 4 * 64 * kTile; k += 256) {
      const int tq = k / (64 * kTile), rr = (k / kTile) % 64, l = k % kTile, t = b0 / kTile + tq;
      if (t < ntiles && R0 + rr < nR) dst[(size_t)t * ts + (size_t)(R0 + rr) * kTile + l] = tile[rr][tq * kTile + l];
    }
  } else {
    for (int rr = ty; rr < 64; rr += 4)
      if (R0 + rr < nR && b0 + tx < batch) dst[(size_t)(R0 + rr) * batch + b0 + tx] = tile[rr][tx];
  }
}
int launch_tiled_convert(bool to_tiled, const double* src, double* dst, size_t nR, int batch, hipStream_t s) {
  const dim3 grid((unsigned)((nR + 63) / 64), (unsigned)((batch + 63) / 64));
  if (nR > 0x7fffffff || grid.y > 65535) return -1;
  if (to_tiled)
    k_tiled_convert<true><<<grid, dim3(256), 0, s>>>(src, dst, (int)nR, batch);
  else
    k_tiled_convert<false><<<grid, dim3(256), 0, s>>>(src, dst, (int)nR, batch);
  return hip_rc(hipGetLastError());
}
size_t tiled_doubles_host(size_t rows, size_t cols, size_t batch) { return tiled_doubles(rows, cols, batch); }

__global__ void k_traj_status(const double* __restrict__ J, int n, int* __restrict__ status) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) status[i] = isfinite(J[i]) ? 0 : 1;   // OCS_NUM_NONFINITE
}
int launch_traj_status(const double* J, int n, int* status, hipStream_t s) {
  hipLaunchKernelGGL(k_traj_status, dim3((n + 255) / 256), dim3(256), 0, s, J, n, status);
  return hip_rc(hipGetLastError());
}

// The reduction behind the per-interval estimates of the mesh drivers (ocs_bvp_rms: one ratio array, no sum; ocs_x_lam_err: two
// and the sum).  Workgroups 0 .. N-1: rmax[i] = the largest of r0[i][b] (and r1[i][b]) over the instances with use[b] != 0
// (use == NULL: all; none: 0).  The workgroups behind them, one thread per instance: rinst[b] = the largest of the instance's
// chunk maxima PM, sum[b] = its chunk sums PS added in chunk order.  A NaN counts as +inf in both maxima ("exceeds every
// tolerance"); an instance's NaN reaches rmax only where it is in use, and never another instance's rinst or sum.  Maxima, and
// one thread's sum in a fixed order: no floating-point atomics, the order of the reduction does not show.  The per-instance
// threads walk their chunks one load latency at a time and are the last to finish: the sum rides in the loop of the maximum.
template <bool Two, bool Sum>
__global__ __launch_bounds__(256) void k_interval_reduce(int N, int batch, int nparts, const double* __restrict__ r0,
                                                         const double* __restrict__ r1, const double* __restrict__ PM,
                                                         const double* __restrict__ PS, const int* __restrict__ use,
                                                         double* __restrict__ rmax, double* __restrict__ rinst,
                                                         double* __restrict__ sum) {
  const size_t B = (size_t)batch;
  if ((int)blockIdx.x >= N) {
    const int b = (blockIdx.x - N) * 256 + threadIdx.x;
    if (b >= batch) return;
    double m = 0.0, sj = 0.0;
    for (int q = 0; q < nparts; ++q) {
      m = fmax(m, PM[(size_t)q * B + b]);
      if (Sum) sj += PS[(size_t)q * B + b];
    }
    rinst[b] = m;
    if (Sum) sum[b] = sj;
    return;
  }
  __shared__ double part[4];
  const double* row0 = r0 + (size_t)blockIdx.x * B;
  const double* row1 = Two ? r1 + (size_t)blockIdx.x * B : row0;
  double m = 0.0;
  for (int b = threadIdx.x; b < batch; b += 256) {
    if (use && use[b] == 0) continue;
    const double v0 = row0[b], v1 = Two ? row1[b] : v0;
    m = fmax(m, (v0 == v0 && v1 == v1) ? fmax(v0, v1) : __builtin_inf());
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) m = fmax(m, __shfl_xor(m, o, 64));
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = m;
  __syncthreads();
  if (threadIdx.x == 0) rmax[blockIdx.x] = fmax(fmax(part[0], part[1]), fmax(part[2], part[3]));
}
int launch_interval_reduce(int N, int batch, int nparts, const double* r0, const double* r1, const double* PM,
                           const double* PS, const int* use, double* rmax, double* rinst, double* sum, hipStream_t s) {
  const dim3 grid(N + (batch + 255) / 256), block(256);
  if (r1 && PS)
    k_interval_reduce<true, true><<<grid, block, 0, s>>>(N, batch, nparts, r0, r1, PM, PS, use, rmax, rinst, sum);
  else if (!r1 && !PS)
    k_interval_reduce<false, false><<<grid, block, 0, s>>>(N, batch, nparts, r0, r1, PM, PS, use, rmax, rinst, sum);
  else
    return -1;   // (instantiated for the two estimates there are)
  return hip_rc(hipGetLastError());
}

// one workgroup: the post-reductions of a shard's objectives (ocs_multi.cpp)
// (mask: optional, entries <= 0 are left out -- the sweep index of fb_sweep, 0 = not converged)
__global__ __launch_bounds__(256) void k_objective_stats(const double* __restrict__ J, int n, int lo, double* __restrict__ out,
                                                         const int* __restrict__ mask) {
  __shared__ double ss[256], sc[256], sm[256], si[256];
  double sum = 0.0, cnt = 0.0, mn = INFINITY, am = -1.0;
  for (int i = threadIdx.x; i < n; i += 256) {
    const double v = J[i];
    if (isfinite(v) && (!mask || mask[i] > 0)) {
      sum += v;
      cnt += 1.0;
      if (v < mn) {
        mn = v;
        am = (double)(lo + i);
      }
    }
  }
  ss[threadIdx.x] = sum; sc[threadIdx.x] = cnt; sm[threadIdx.x] = mn; si[threadIdx.x] = am;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) {
      ss[threadIdx.x] += ss[threadIdx.x + w];
      sc[threadIdx.x] += sc[threadIdx.x + w];
      const double m2 = sm[threadIdx.x + w], i2 = si[threadIdx.x + w];
      // the smaller value; of equal values the smaller index (deterministic whatever the thread count)
      if (m2 < sm[threadIdx.x] || (m2 == sm[threadIdx.x] && i2 >= 0.0 && (si[threadIdx.x] < 0.0 || i2 < si[threadIdx.x]))) {
        sm[threadIdx.x] = m2;
        si[threadIdx.x] = i2;
      }
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    out[0] = ss[0];
    out[1] = sc[0];
    out[2] = sm[0];
    out[3] = si[0];
  }
}
int launch_objective_stats(const double* J, int n, int lo, double* out, hipStream_t s, const int* mask) {
  hipLaunchKernelGGL(k_objective_stats, dim3(1), dim3(256), 0, s, J, n, lo, out, mask);
  return hip_rc(hipGetLastError());
}

int launch_count_nonfinite(const double* v, int n, int* count, hipStream_t s) {
  hipLaunchKernelGGL(k_count_nonfinite, dim3((n + 255) / 256), dim3(256), 0, s, v, n, count);
  return hip_rc(hipGetLastError());
}

}  // namespace ocs
