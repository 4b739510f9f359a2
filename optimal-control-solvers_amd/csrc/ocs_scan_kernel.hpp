// ocs_scan_kernel.hpp -- the discrete-adjoint pass (RK4Integrator.m:59-121) as a scan over time, for
// row-separable problems.
//
// The adjoint recursion is linear in lam: for a problem whose state rows are uncoupled (row r of F reads y_r
// and u only, ocs_problems.hpp ROW_SEPARABLE) and whose cost row of lam is constant (last row of
// dFdx_times_vec is zero, OCProblem.m:14-15), every step is a scalar affine map per row,
//     lam_i = alpha_i lam_{i+1} + beta_i,
// whose coefficients depend on the stage states Y1..Y4 of step i only -- and those are recomputed from the
// checkpoint x(t_i) and the control samples, independently for every step.  So the 1000-step serial chain of
// the pass disappears:
//
//   phase 1  (time-parallel)  wave w of a workgroup takes a chunk of L consecutive steps of the workgroup's
//            64 (trajectory, row) lanes, recomputes Y2..Y4, forms (alpha_i, beta_i) by pushing the pair
//            (coefficient of lam, constant) through RK4Integrator.m:73-88, and composes them into the chunk
//            map (A_w, B_w):  lam_lo = A_w lam_hi+1 + B_w.
//   phase 2  (W-term scan)    the W chunk maps of a superblock (W chunks = W L steps) go through LDS; every
//            wave composes them in time order on top of the carry (lam at the top of the superblock), which
//            gives it lam at the top of its own chunk and the next carry.  One LDS barrier per superblock.
//   phase 3  (time-parallel)  with the true lam at the top of its chunk a wave walks down its L steps, stores lam and
//            assembles the dJdu columns (:97-121).  Where (dF/du)'v does not read y (!P::DFDU_READS_Y: the registry
//            problems) everything a step stores is affine in lam_{i+1} as well -- lam_i, and this row's shares of the
//            midpoint column (B'k2 + B'k3) and of the two node columns (B'k1, B'k4) -- and phase 1 keeps those
//            coefficients in registers in place of the stage states: a step of phase 3 is four FMAs and the row sums,
//            with no stage state and no row function.  For the other problems (user problems given as row functions,
//            ocs_user_functor.hpp) phase 3 forms the stage states once more and runs :73-88 as the reference writes
//            them (inside a chunk the arithmetic is the serial kernels').
//
// Superblocks are taken from the end of the horizon; the loads of superblock k+1 are issued before superblock k
// is processed (two register sets), so HBM latency lies under a whole superblock of arithmetic and the pass
// streams: per (trajectory, step) it reads x (nS doubles) and two new control samples and writes lam (nAug)
// and two dJdu columns.  Steps below 0 in the last superblock run as exact identity maps (records with
// h = 0 on clamped inputs), so any N works; stores are predicated, so any batch works.
//
// Differences to the serial kernels: lam at the chunk boundaries comes from composed maps, and (registry problems) lam
// and dJdu inside a chunk from the per-step affine forms, i.e. a different association of the same products and sums
// (round-off level; tolerance 1e-12 as for the other mappings).  The lam-only, dJdu-only and combined instances share
// one arithmetic path and store the same bits.
// The composed products prod(alpha) must stay inside the fp64 range.
// This header holds the kernel template only (it is also compiled by hipRTC for user problems given as row functions,
// csrc/ocs_user_functor.hpp); the launchers are in ocs_scan_kernels.hip.  Functor interface: the g_* names of
// ocs_problems.hpp ("generic row-separable interface").
#pragma once
#include "ocs_device_common.hpp"

namespace ocs {

// Lane layout: lane = r * (64/G) + tl, the trajectory index fastest.  The 64/G lanes of a state row read and
// write one contiguous segment, and above all the four lanes of every quad touch ONE cache line: the texture
// addresser works through a wave's addresses a quad at a time, and with the row index fastest (lane = tl G + r,
// the layout of the row-split / pipeline kernels) every quad spans G lines -- measured 3.5 TB/s against 6 TB/s
// for the same bytes.  The price: sums over the rows of a trajectory cross lanes 16 or 32 apart, which DPP
// cannot reach; they use the row-swapping permlane instructions of gfx950 (swap_add16 / swap_add32 below).
// v_permlane16_swap(vdst, src): the odd 16-lane rows of vdst trade places with the even rows of src;
// v_permlane32_swap: the upper half of vdst with the lower half of src.  With (a, b) in, the two results added give
// per row [a0+a1, b0+b1, a2+a3, b2+b3] -- a transposing pair reduction in two instructions per 32-bit half, in the
// vector pipe (ds_bpermute, the alternative, parks the wave for an LDS round trip: 13 % of its cycles were measured).
__device__ static inline double swap_add16(double a, double b) {
  const auto lo = __builtin_amdgcn_permlane16_swap((unsigned)__double2loint(a), (unsigned)__double2loint(b), false, false);
  const auto hi = __builtin_amdgcn_permlane16_swap((unsigned)__double2hiint(a), (unsigned)__double2hiint(b), false, false);
  return __hiloint2double((int)hi[0], (int)lo[0]) + __hiloint2double((int)hi[1], (int)lo[1]);
}
__device__ static inline double swap_add32(double a, double b) {
  const auto lo = __builtin_amdgcn_permlane32_swap((unsigned)__double2loint(a), (unsigned)__double2loint(b), false, false);
  const auto hi = __builtin_amdgcn_permlane32_swap((unsigned)__double2hiint(a), (unsigned)__double2hiint(b), false, false);
  return __hiloint2double((int)hi[0], (int)lo[0]) + __hiloint2double((int)hi[1], (int)lo[1]);
}
// sum over the G rows of a trajectory (lanes r TPW + tl), in every lane
template <int G>
__device__ static inline double group_sum_sc(double v) {
  static_assert(G == 1 || G == 2 || G == 4, "group size");
  if (G == 4) v = swap_add16(v, v);
  if (G >= 2) v = swap_add32(v, v);
  return v;
}
// two sums at once: lanes of even row r get sum_r a, lanes of odd row r get sum_r b
template <int G>
__device__ static inline double pair_sum_sc(double a, double b) {
  static_assert(G == 1 || G == 2 || G == 4, "group size");
  if (G == 1) return a;   // (not used: one lane per trajectory has nothing to sum)
  if (G == 4) {
    const double s = swap_add16(a, b);   // rows: [a0+a1, b0+b1, a2+a3, b2+b3]
    return swap_add32(s, s);             //       [sum a, sum b, sum a, sum b]
  }
  return swap_add32(a, b);               // halves (= rows): [a0+a1, b0+b1]
}

struct BwdArgsScan {
  int N, batch;          // N: a multiple of L (the launcher gives the remainder to the lane kernel)
  const double* RECS;    // step records (kScanRec doubles each), zero records around [0, N)
  const double* ps;
  const double* pb;
  unsigned pmask;
  const double* xck;
  const double* u;
  const double* lamT;
  double* lam;
  double* dJdu;
  double* lam0;
  const double* pend0;   // optional [B]: the k1 half of column 2N when the steps above N were done by another kernel
};

// Buffer addressing (raw SRSRC, 32-bit per-lane voffset + scalar soffset): a lane's part of every address
// ((row r, trajectory b) of a column) is fixed for the whole kernel and lives in one VGPR per array; the
// column (time) part is wave-uniform and goes through the scalar offset, so address arithmetic costs no vector
// registers or instructions.  A lane is switched off without a branch by an offset beyond num_records (the
// range check of a raw buffer compares the vector offset only and drops the access), a whole chunk by a
// descriptor with num_records = 0.
typedef unsigned v2u_sc __attribute__((ext_vector_type(2)));
constexpr unsigned kOffDrop = 0xFFFFFFF0u;  // >= num_records of every descriptor below
constexpr int kNumRec = 0x7FFFFFF0;
struct Buf {
  __amdgpu_buffer_rsrc_t r;
  __device__ static inline Buf make(const double* p, int nrec = kNumRec) {
    return Buf{__builtin_amdgcn_make_buffer_rsrc(const_cast<double*>(p), 0, nrec, 0x00020000)};
  }
  __device__ inline double ld(unsigned voff, unsigned soff) const {
    return __builtin_bit_cast(double, __builtin_amdgcn_raw_buffer_load_b64(r, voff, soff, 0));
  }
  __device__ inline void st0(double v, unsigned voff, unsigned soff) const {   // plain (cached) store
    __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(v2u_sc, v), r, voff, soff, 0);
  }
  __device__ inline void st(double v, unsigned voff, unsigned soff) const {   // non-temporal (aux 2; measured: NOTES.md)
    __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(v2u_sc, v), r, voff, soff, 2);
  }
};

constexpr int kScanRec = 16;       // doubles per record: {h, h/2, h/6, h/3 | s4, s3, s1, 0 | tcA, tcM, tcB, 0 | pad}
constexpr int kScanPadFront = 136; // zero records before step 0 (>= the steps of a superblock + 1: 16 x 4 in
                                   // k_backward_scan, 8 x 4 x 4 in k_backward_fcs)
constexpr int kScanPadBack = 8;    // and after step N-1 (a wave copies 8 records per chunk)
// Checkpoints of a chunk's upper L - 1 steps integrated again from the first instead of read (k_backward_scan): 8 nS / L
// bytes of checkpoint traffic per (trajectory, step) instead of 8 nS, for four more evaluations of the row's right-hand
// side.  Measured at BL-2 (batch 4096, nS = 4): buffers that rotate through HBM 94.5 -> 89.2 us, one buffer set re-used
// from the memory-side cache 79.9 -> 81.0 us; nS = 1: 70.3 -> 66.8 / 69.2 -> 66.7 us (profiles/r04f_xrc.log; NOTES.md).

// Chunk of wave `wave` in superblock sb of a scan over time: steps lo .. lo + L - 1, superblocks counted from the end of the
// horizon.  Below step 0 a chunk is dead as a whole (N % L == 0).  Used by k_backward_scan(_tiled) and k_backward_vscan; the
// costate scans keep a lambda with the same line, and the rest of what the four kernels have in common -- the phase 2 carry,
// the dense map algebra, the pchip block, the clamped loads -- is the same text in each of them ON PURPOSE: as shared
// functions each of these changed the kernels' code (NOTES.md, "Scan kernels: wave primitives once").
template <int W, int L>
__device__ constexpr int scan_chunk_lo(int N, int sb, int wave) { return N - (sb * W + wave + 1) * L; }

// The kernel body is ONE text, ocs_scan_body.inc, included into k_backward_scan and into k_backward_scan_tiled below.  The spots
// that depend on the device layout are OCS_SC_ macros, defined before each #include and gone after it:
//   OCS_SC_PROLOGUE          declarations only the tiled kernel needs
//   OCS_SC_RX, OCS_SC_RU     row stride of x / lam and of u / dJdu
//   OCS_SC_X0W, OCS_SC_U0W   the workgroup's part of an index into them, with its "+" (batch-minor: nothing)
//   OCS_SC_LX, OCS_SC_LU     the lane's part of such an index
//   OCS_SC_LAMT(row)         lamT of the lane's trajectory, OCS_SC_PEND0 its pend0
// The batch-minor definitions are, token for token, what k_backward_scan held at these spots before the body was shared, so its
// device code does not depend on the tiled kernel existing.  Not a template parameter and not a __device__ function: both were
// built and changed the code of the batch-minor instances (NOTES.md, "Tiled device layout").  An edit of either kernel is an
// edit of the body file; a new spot that depends on the layout gets a macro in BOTH blocks.

// W waves per workgroup (chunks per superblock), L steps per chunk
template <class P, int W, int L, bool OUT_LAM, bool OUT_DJDU, bool LT>
__global__ __launch_bounds__(W * 64) void k_backward_scan(const BwdArgsScan a) {
#define OCS_SC_PROLOGUE
#define OCS_SC_RX B
#define OCS_SC_RU B
#define OCS_SC_X0W
#define OCS_SC_U0W
#define OCS_SC_LX b
#define OCS_SC_LU (size_t)b
#define OCS_SC_LAMT(row) a.lamT[(size_t)row * B + b]
#define OCS_SC_PEND0 a.pend0[b]
#include "ocs_scan_body.inc"
#undef OCS_SC_PROLOGUE
#undef OCS_SC_RX
#undef OCS_SC_RU
#undef OCS_SC_X0W
#undef OCS_SC_U0W
#undef OCS_SC_LX
#undef OCS_SC_LU
#undef OCS_SC_LAMT
#undef OCS_SC_PEND0
}

// The same pass on tiled checkpoints, u, lam and dJdu (OCS_LAYOUT_TILED; DevLayout, ocs_device_common.hpp): the same body with
// the tiled row strides and offsets in every address.  nodes: the columns N + 1 of the WHOLE checkpoint / lam arrays, a.N being
// the steps of this launch.  A workgroup's 64 / G trajectories are whole tiles; the part of every address that belongs to the
// workgroup's first tile (x0w, u0w) is wave-uniform and goes into the descriptors' base, so the 32-bit lane offsets (from lx, lu)
// span at most four tiles whatever the batch.  Lanes past the batch are clamped for loads and dropped for stores as in
// k_backward_scan, so pad lanes are neither read nor written.  colT: lamT points into a column of the tiled lam (the hand-over
// column of a split pass; VT, vt: its row stride and the lane's index either way); pend0 is a column of the tiled dJdu wherever
// it is given.
struct BwdArgsScanTiled {
  BwdArgsScan a;
  int nodes;   // N + 1 of the whole pass
  int colT;    // lamT is a column of the tiled lam
};
template <class P, int W, int L, bool OUT_LAM, bool OUT_DJDU, bool LT>
__global__ __launch_bounds__(W * 64) void k_backward_scan_tiled(const BwdArgsScanTiled t) {
  const BwdArgsScan& a = t.a;
  const int nodes = t.nodes;
  const bool colT = t.colT != 0;
#define OCS_SC_PROLOGUE                                                                                                \
  const DevLayout<true> LX = DevLayout<true>::make(B, NAUG, nodes), LU = DevLayout<true>::make(B, 1, 2 * nodes - 1); \
  const size_t RX = LX.row(), RU = LU.row(), bw = (size_t)blockIdx.x * TPW;                                           \
  const size_t x0w = LX.at(bw), u0w = LU.at(bw);                                                                      \
  const size_t lx = LX.at(b, bw), lu = LU.at(b, bw);                                                                  \
  const size_t VT = colT ? RX : B, vt = colT ? LX.at(b) : (size_t)b;
#define OCS_SC_RX RX
#define OCS_SC_RU RU
#define OCS_SC_X0W x0w +
#define OCS_SC_U0W u0w +
#define OCS_SC_LX lx
#define OCS_SC_LU lu
#define OCS_SC_LAMT(row) a.lamT[(size_t)row * VT + vt]
#define OCS_SC_PEND0 a.pend0[LU.at(b)]
#include "ocs_scan_body.inc"
#undef OCS_SC_PROLOGUE
#undef OCS_SC_RX
#undef OCS_SC_RU
#undef OCS_SC_X0W
#undef OCS_SC_U0W
#undef OCS_SC_LX
#undef OCS_SC_LU
#undef OCS_SC_LAMT
#undef OCS_SC_PEND0
}

}  // namespace ocs
