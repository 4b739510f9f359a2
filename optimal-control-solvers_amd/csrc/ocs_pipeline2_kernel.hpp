// ocs_pipeline2_kernel.hpp -- state pass (RK4Integrator.m:28-56) for row-separable problems, wave-specialised
// with a MINIMAL recursion wave.
//
// The pass has one inherently serial part, the state recursion y_{i+1} = Phi_i(y_i): eight dependent fp64
// operations per step and row.  Everything else -- the objective integrand at the four stage states, its
// quadrature, the stores of the trajectory -- only needs y_i and is independent from step to step.  A lone wave
// issues one instruction per ~6 cycles whatever it is, so the pass runs at (instructions of the recursion wave
// per step) x 6 cycles x N.  Here the recursion wave S executes per step: one 16-byte LDS read (the two new
// prepared control terms), the eleven arithmetic instructions of the step, one 8-byte LDS write (y_i).  All other
// work is time-parallel and spread over the other SIMDs of the CU:
//
//   wave M/P  streams control samples and step records HBM -> LDS (LDS-DMA, 1 KiB per instruction, Q blocks
//             ahead, the only wave that waits for memory) and prepares the control terms of the NEXT block for S
//             (P::row_vertex: m_r^2/4 - u, so that a stage evaluation of S is one fused multiply-add);
//   wave S    the recursion, on z = y - m_r/2 (P::row_f_shifted);
//   waves C   (2 or 4) take the steps of the block S finished in the previous interval: recompute the stage
//             states from y_i (three more F evaluations per step: cheaper than a second LDS write on S), form the
//             objective increment d_i, store x(t_i).  A lane takes all rows of one (trajectory, step), so row
//             sums need no cross-lane traffic; lanes are trajectory-fastest, so every quad stores into one line;
//   wave J    prefix-sums the objective increments of the block before that, stores the cost row and J.
//
// One LDS-only barrier per block of D = 8 steps.  Interval k (between barriers k and k+1):
//   M: issues block k+1+Q, waits for block k+2    P: prepares block k+1    S: block k    C: block k-1    J: block k-2
// Results: a step is the recursion on z and the objective summed over rows before the quadrature weights (DESIGN.md,
// Numerics; generic row functions: the reference's sum, RK4Integrator.m:50) -- to round-off the lane kernels' and the
// oracle's where the states are of the size of m_r/2.  The recursion on z rounds at the size of m_r/2, not of y: on a state
// far below m_r/2 the relative error is up to (1 + m_r / (2 |y|)) times the plain recursion's ("Rounding error
// per mapping"; tests/test_gpu_rk4_accuracy.py).  The state pass of the folded sweep (ocs_fold_kernel.hpp) repeats this arithmetic.
// This header holds the kernel template only (also compiled by hipRTC for user problems given as row functions); the
// launchers are in ocs_pipeline2_kernels.hip.  Registry problems use the shifted form of their rows (HAS_SHIFT), user
// problems the generic g_row_f / g_row_q.
#pragma once
#include "ocs_device_common.hpp"

namespace ocs {

#ifdef OCS_P2_STAMPS
__device__ static long long g_p2_stamp[16 * 4];   // per wave role: {barrier wait, total, -, -} of workgroup 0
__device__ static long long g_p2_wg[1024 * 4];    // per workgroup: S wave {start, end, barrier wait, xcc}
#define P2_BARRIER() do { const long long t0_ = __builtin_amdgcn_s_memtime(); lds_barrier(); tbar_ += __builtin_amdgcn_s_memtime() - t0_; } while (0)
#define P2_BEGIN() long long tbar_ = 0; const long long tstart_ = __builtin_amdgcn_s_memtime(); const long long rstart_ = __builtin_amdgcn_s_memrealtime()
#define P2_END(w) do { if (blockIdx.x == 0 && lane == 0) { g_p2_stamp[(w) * 4] = tbar_; g_p2_stamp[(w) * 4 + 1] = __builtin_amdgcn_s_memtime() - tstart_; } if ((w) == 1 && lane == 0 && blockIdx.x < 1024) { g_p2_wg[blockIdx.x * 4] = tstart_; g_p2_wg[blockIdx.x * 4 + 1] = __builtin_amdgcn_s_memtime(); g_p2_wg[blockIdx.x * 4 + 2] = rstart_; g_p2_wg[blockIdx.x * 4 + 3] = __builtin_amdgcn_s_memrealtime() - rstart_; } } while (0)
#else
#define P2_BARRIER() lds_barrier()
#define P2_BEGIN()
#define P2_END(w)
#endif
// wait until at most `blocks` * LPB of this wave's vector-memory operations are outstanding (blocks is wave-uniform)
template <int LPB, int QMAX>
__device__ static inline void wait_blocks_p2(int blocks) {
  static_assert(QMAX * LPB <= 63 && QMAX <= 8, "vmcnt is a 6-bit counter");
#define OCS_WB(n) case n: if (n <= QMAX) asm volatile("s_waitcnt vmcnt(%0)" ::"n"((n <= QMAX ? n : 0) * LPB) : "memory"); break;
  switch (blocks < 0 ? 0 : blocks) {
    OCS_WB(0) OCS_WB(1) OCS_WB(2) OCS_WB(3) OCS_WB(4) OCS_WB(5) OCS_WB(6) OCS_WB(7) OCS_WB(8)
    default: asm volatile("s_waitcnt vmcnt(%0)" ::"n"(QMAX * LPB) : "memory"); break;
  }
#undef OCS_WB
}
typedef unsigned v2u_p2 __attribute__((ext_vector_type(2)));
constexpr unsigned kDropP2 = 0xFFFFFFF0u;
constexpr int kNumRecP2 = 0x7FFFFFF0;
struct BufP2 {
  __amdgpu_buffer_rsrc_t r;
  __device__ static inline BufP2 make(double* p) {
    return BufP2{__builtin_amdgcn_make_buffer_rsrc(p, 0, kNumRecP2, 0x00020000)};
  }
  // plain (cached): the state rows of x, which the adjoint pass reads next (non-temporal and sc1 measured: NOTES.md)
  __device__ inline void st(double v, unsigned voff, unsigned soff) const {
    __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(v2u_p2, v), r, voff, soff, 0);
  }
  // non-temporal: for rows nobody reads back soon (the running-objective row: the adjoint pass reads the state rows only)
  __device__ inline void st_nt(double v, unsigned voff, unsigned soff) const {
    __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(v2u_p2, v), r, voff, soff, 2);
  }
};

// NKS > 0: the control samples are not read from memory but expanded in the kernel from the coefficients of a dense
// basis, u(:, j) = sum_k v_k B(k, j) (Control/ChebyshevControl.m:35-38), by NUW waves on the matrix cores: NKS k-steps of
// v_mfma_f64_16x16x4_f64 per tile of 16 samples x 16 trajectories (role U below).  Only the step records are streamed then.
// TPW_: trajectories per workgroup, 64 / G by default (every lane of the recursion wave owns one state row).  Half of
// that (G = 1, TPW_ = 32: the upper half of the recursion wave repeats the lower) halves everything a workgroup does
// besides the recursion -- for batches that leave CUs idle, where the other waves of the CU set the pace.
template <int G, int NKS = 0, int TPW_ = 64 / G>
struct P2Cfg {
  static constexpr int D = 8;                        // steps per block
  static constexpr int TPW = TPW_;                   // trajectories per workgroup
  static constexpr int GS = 64 / TPW;                // lane groups of a wave (objective waves: steps per pass)
  static_assert(GS * TPW == 64 && GS % G == 0 && GS <= 4, "lane groups");
  static constexpr int Q = NKS > 0 ? 2 : (G == 1) ? 6 : 8;   // blocks the DMA runs ahead of the preparation (an interval is
                                                     // ~0.3 us: HBM latency needs several; vmcnt counts to 63; the record
                                                     // table alone is shared by all workgroups and sits in L2)
  static constexpr int NSLOT = Q + 3;                // input ring (block j: prepared in interval j-1, read by C in j+1)
  static constexpr int RS = rec_stride(1), SCO = rec_sc_offset(1);
  static constexpr int REC_DBL = D * RS, NREC = REC_DBL / 128;
  static constexpr int U_DBL = 2 * D * TPW, NU = U_DBL / 128;
  static constexpr int SLOT = REC_DBL + U_DBL;
  static constexpr int LPB = NREC + (NKS > 0 ? 0 : NU);
  static constexpr int NCW = (GS == 4) ? 2 : 4;      // objective/store waves
  static constexpr int SPW = D / NCW;                // steps per such wave and block
  static constexpr int NPASS = SPW / GS > 0 ? SPW / GS : 1;
  static constexpr int NT = TPW / 16;                // tiles of 16 trajectories (NKS > 0)
  static constexpr int NUW = NKS > 0 ? (NT >= 2 ? 2 : 1) : 0;   // expansion waves
  static constexpr int TW = NKS > 0 ? NT / NUW : 0;  // tiles per expansion wave
  static constexpr int NWAVE = 4 + NCW + NUW;        // M, S, C.., J, P (, U..)
  static_assert(REC_DBL % 128 == 0 && U_DBL % 128 == 0 && (SPW % GS == 0 || GS > SPW), "block shapes");
  static_assert(NKS == 0 || (2 * D == 16 && NT >= 1 && NKS <= 8), "a block of samples is one 16-row tile");
  // role of a wave (0 M, 1 S, 2.. C, 2 + NCW J, 3 + NCW P, 4 + NCW.. U).  A workgroup's waves are dealt to the four
  // SIMDs in turn (wave w and w + 4 share one): with the expansion waves present the recursion wave gets the SIMD of
  // the nearly idle M wave, the matrix work goes beside the objective waves.
  __device__ static constexpr int role(int w) {
    if (NKS == 0) return w;
    constexpr int M_ = 0, S_ = 1, C_ = 2, J_ = 2 + NCW, P_ = 3 + NCW, U_ = 4 + NCW;
    // (a matrix instruction occupies the SIMD's fp64 datapath for its 64 cycles: an expansion wave gets ONE objective
    //  wave beside it, the two remaining objective waves share the fourth SIMD)
    if (NWAVE == 10) { constexpr int r[10] = {U_, U_ + 1, S_, C_ + 2, C_, C_ + 1, M_, C_ + 3, J_, P_}; return r[w]; }
    constexpr int r[7] = {U_, C_, S_, C_ + 1, J_, P_, M_};
    return r[w];
  }
};
typedef double d4_p2 __attribute__((ext_vector_type(4)));

struct FwdArgsP2 {
  int N, batch;
  const double* REC;
  const double* ps;
  const double* pb;
  unsigned pmask;
  const double* x0;
  const double* u;
  double* x;
  double* J;
  const int* frozen;   // optional [B]: trajectories with frozen[b] != 0 store nothing
  int nocost;          // leave the running-objective row of x unwritten (J only)
  const int* gate;     // optional: the launch does nothing if *gate == 0
  // NKS > 0 (u expanded in the kernel; `u` is not read):
  const double* BT = nullptr;   // [2N+1][ldbt]: transposed basis, zero-padded to 4 NKS functions
  const double* v = nullptr;    // [nBasis][B] coefficients (one control)
  int nBasis = 0, ldbt = 0;
};

// The kernel body is ONE text, ocs_pipeline2_body.inc, included into k_forward_p2 and into k_forward_p2_tiled below.  The spots
// that depend on the device layout are OCS_P2_ macros, defined before each #include and gone after it:
//   OCS_P2_DECL_BW             declares bw, the workgroup's first trajectory
//   OCS_P2_DECL_LAYOUT         declarations only the tiled kernel needs
//   OCS_P2_B(tl), _POS(tl)     index of the workgroup's trajectory tl for the per-trajectory vectors; tiled: declares its Pos ps_
//   OCS_P2_RX, _X0W            x: row stride, the workgroup's part of an index with its "+" (batch-minor: nothing)
//   OCS_P2_LX, _LX_SZ          x: the trajectory's part of an index, as it stands and as a size_t
//   OCS_P2_URS, _UL(tl)        control part of an input slot: row stride, place of trajectory tl in a row
//   OCS_P2_U0(b, lu)           index of a trajectory's sample 0 in u: b, or its tiled place lu past the workgroup's
//   OCS_P2_DMA_U(j, q, dst)    chunk q (16 bytes per lane) of the LDS-DMA of block j's control samples into slot dst
//   OCS_P2_DROP(c)             condition for a dropped store offset: c, tiled also for a tile that does not exist
//   OCS_P2_IF_TILE(c), _IF_TRAJ(c)   condition of a plain store: c, tiled only into a tile / for a trajectory that exists
// The batch-minor definitions are, token for token, what k_forward_p2 held at these spots before the body was shared, so its
// device code does not depend on the tiled kernel existing.  Not a template parameter and not a __device__ function: both were
// built and changed the code of the batch-minor instances (NOTES.md, "Tiled device layout").  An edit of either kernel is an
// edit of the body file; a new spot that depends on the layout gets a macro in BOTH blocks.

// UNI: uniform grid -- the step sizes are the same for every step and stay in registers
// bw: a batch that is not a multiple of the tile: the LAST workgroup takes the last TPW trajectories, overlapping its neighbour --
// the overlap is computed twice with the same operations and stored twice with the same values (nothing of this kernel is
// accumulated across trajectories).  The launcher asks for it only with batch >= TPW and an even batch (the 16-byte
// DMA chunks stay aligned).
template <class P, bool OUT_X, bool FRZ, bool UNI, int NKS = 0, int TPW_ = 64 / P::NS>
__global__ __launch_bounds__((P2Cfg<P::NS, NKS, TPW_>::NWAVE * 64)) void k_forward_p2(const FwdArgsP2 a) {
#define OCS_P2_DECL_BW              \
  const int bw_ = blockIdx.x * TPW; \
  const int bw = bw_ + TPW <= a.batch ? bw_ : a.batch - TPW;
#define OCS_P2_DECL_LAYOUT
#define OCS_P2_B(tl) bw + tl
#define OCS_P2_POS(tl)
#define OCS_P2_RX B
#define OCS_P2_X0W
#define OCS_P2_LX b
#define OCS_P2_LX_SZ (size_t)b
#define OCS_P2_URS TPW
#define OCS_P2_UL(tl) tl
#define OCS_P2_U0(b, lu) b
#define OCS_P2_DMA_U(j, q, dst)                                  \
  const int e = q * 128 + 2 * lane, row = e / TPW, t2 = e % TPW; \
  dma16(a.u + ((size_t)(2 * D * j + 1 + row)) * B + bw + t2, dst + C_::REC_DBL + q * 128);
#define OCS_P2_DROP(c) (c)
#define OCS_P2_IF_TILE(c) c
#define OCS_P2_IF_TRAJ(c) c
#include "ocs_pipeline2_body.inc"
#undef OCS_P2_DECL_BW
#undef OCS_P2_DECL_LAYOUT
#undef OCS_P2_B
#undef OCS_P2_POS
#undef OCS_P2_RX
#undef OCS_P2_X0W
#undef OCS_P2_LX
#undef OCS_P2_LX_SZ
#undef OCS_P2_URS
#undef OCS_P2_UL
#undef OCS_P2_U0
#undef OCS_P2_DMA_U
#undef OCS_P2_DROP
#undef OCS_P2_IF_TILE
#undef OCS_P2_IF_TRAJ
}

// The same pass on tiled x and u (OCS_LAYOUT_TILED; DevLayout, ocs_device_common.hpp), for the plain case (control samples from
// memory, nothing frozen: the body's expansion-wave branch is discarded with NKS = 0).  nodes: the columns N + 1 of the WHOLE x
// array, a.N being the steps of this launch.  A workgroup's TPW trajectories are 1, 2 or 4 whole tiles, no workgroup overlaps
// another: ragged and odd batches end in pad lanes.  A block of 16 samples of one tile is 2 KiB in one run, so the DMA copies it
// as it lies: the control part of an input slot is [tile][sample][16] here ([sample][TPW] in k_forward_p2).  A tile of the
// workgroup past the last tile of the arrays loads that last tile and stores nothing; a pad lane of a tile that exists runs on
// whatever the pad lane of u holds -- nothing of this kernel crosses trajectories -- with the last trajectory's x0, and stores
// into its own pad lane of x only.
// OCS_P2_DECL_LAYOUT: x (NAUG rows) and u (one row) have the row strides RX, RU and the workgroup's part of an index x0w, u0w.
// pos(tl), trajectory tl of the workgroup: bc its index for the per-trajectory vectors, bv whether it is one of the batch, tv
// whether its tile exists, lx / lu its part of an index into x / u (relative to the workgroup's first tile; of the last tile of
// the arrays if its own does not exist; `left`: the tiles of the arrays from the workgroup's first on, >= 1).
// OCS_P2_DMA_U: tile tq's samples 2 D j + 1 .. 2 D j + 2 D are 2 D 16 doubles in one run.
struct FwdArgsP2Tiled {
  FwdArgsP2 a;
  int nodes;   // N + 1 of the whole pass
};
template <class P, bool OUT_X, bool UNI>
__global__ __launch_bounds__((P2Cfg<P::NS>::NWAVE * 64)) void k_forward_p2_tiled(const FwdArgsP2Tiled t) {
  constexpr bool FRZ = false;
  // NKS: 0, written so that it depends on P -- the body's expansion-wave branch (arrays of NKS elements) is then discarded at
  // instantiation instead of being checked with NKS = 0 where the template is defined
  constexpr int NKS = 0 * P::NS, TPW_ = 64 / P::NS;
  static_assert(TPW_ % kTile == 0, "whole tiles");
  const FwdArgsP2& a = t.a;
  const int nodes = t.nodes;
#define OCS_P2_DECL_BW const int bw = blockIdx.x * TPW;
#define OCS_P2_DECL_LAYOUT                                                                                             \
  const DevLayout<true> LX = DevLayout<true>::make(B, NAUG, nodes), LU = DevLayout<true>::make(B, 1, 2 * nodes - 1); \
  const size_t RX = LX.row(), RU = LU.row();                                                                          \
  const size_t x0w = LX.at(bw), u0w = LU.at(bw);                                                                      \
  constexpr int URS = kTile;                                                                                          \
  auto ul = [](int tl) OCS_INLINE { return (tl / kTile) * (2 * D * kTile) + tl % kTile; };                            \
  struct Pos { int bc; bool bv, tv; size_t lx, lu; };                                                                 \
  auto pos = [&](int tl) OCS_INLINE {                                                                                 \
    const int b = bw + tl;                                                                                            \
    const int left = (int)tiled_tiles(B) - bw / kTile;                                                                \
    const bool tv = tl / kTile < left;                                                                                \
    const size_t bl = (size_t)bw + (tv ? tl : (left - 1) * kTile + tl % kTile);                                       \
    return Pos{b < a.batch ? b : a.batch - 1, b < a.batch, tv, LX.at(bl, bw), LU.at(bl, bw)};                         \
  };
#define OCS_P2_B(tl) pos(tl).bc
#define OCS_P2_POS(tl) const Pos ps_ = pos(tl);
#define OCS_P2_RX RX
#define OCS_P2_X0W x0w +
#define OCS_P2_LX ps_.lx
#define OCS_P2_LX_SZ ps_.lx
#define OCS_P2_URS URS
#define OCS_P2_UL(tl) ul(tl)
#define OCS_P2_U0(b, lu) u0w + lu
#define OCS_P2_DMA_U(j, q, dst)                                                                    \
  const int e = q * 128 + 2 * lane;                                                                \
  const int tq = e / (2 * D * kTile);                                                              \
  dma16(a.u + u0w + pos(tq * kTile).lu + (size_t)(2 * D * j + 1) * kTile + e % (2 * D * kTile), \
           dst + C_::REC_DBL + q * 128);
#define OCS_P2_DROP(c) (c || !ps_.tv)
#define OCS_P2_IF_TILE(c) c && ps_.tv
#define OCS_P2_IF_TRAJ(c) c && ps_.bv
#include "ocs_pipeline2_body.inc"
#undef OCS_P2_DECL_BW
#undef OCS_P2_DECL_LAYOUT
#undef OCS_P2_B
#undef OCS_P2_POS
#undef OCS_P2_RX
#undef OCS_P2_X0W
#undef OCS_P2_LX
#undef OCS_P2_LX_SZ
#undef OCS_P2_URS
#undef OCS_P2_UL
#undef OCS_P2_U0
#undef OCS_P2_DMA_U
#undef OCS_P2_DROP
#undef OCS_P2_IF_TILE
#undef OCS_P2_IF_TRAJ
}


}  // namespace ocs
