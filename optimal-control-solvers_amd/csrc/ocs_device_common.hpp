// ocs_device_common.hpp -- device helpers shared by the kernel translation units.
#pragma once
#include <hip/hip_runtime.h>

namespace ocs {

// The wave that carries a kernel's dependent chain (state / costate recursion) does NOT ask the SIMD's arbiter for priority
// over the helper waves it shares the SIMD with: s_setprio 3 on it measured slower (NOTES.md, "Tuning switches taken out") --
// the chain waits for its own results (8 dependent fp64 operations per step), not for issue slots.

#define OCS_INLINE __attribute__((always_inline))

// ---------------------------------------------------------------------------------------
// wave primitives: THE copy for every kernel translation unit and the hipRTC header set
// ---------------------------------------------------------------------------------------
// Hand-off barrier: only LDS traffic has to be complete.  __syncthreads() would also drain vmcnt,
// i.e. every global store still in flight.
__device__ static inline void lds_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }
// 16-byte-per-lane LDS-DMA: lane l copies src_l[0..1] to lds_base[2l..2l+1]
__device__ static inline void dma16(const double* src, double* lds_base) {
  __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)src,
                                   (__attribute__((address_space(3))) void*)lds_base, 16, 0, 0);
}
// fp64 cross-lane move inside a quad (DPP quad_perm on the two 32-bit halves)
template <int CTRL>
__device__ static inline double dpp_quad(double v) {
  const int lo = __double2loint(v), hi = __double2hiint(v);
  const int lo2 = __builtin_amdgcn_mov_dpp(lo, CTRL, 0xF, 0xF, true);
  const int hi2 = __builtin_amdgcn_mov_dpp(hi, CTRL, 0xF, 0xF, true);
  return __hiloint2double(hi2, lo2);
}

// First trajectory of a workgroup's tile of TPW trajectories.  A batch that is not a multiple of the tile: the LAST workgroup takes
// the last TPW trajectories, overlapping its neighbour -- the overlap is computed twice with the same operations (the tiled
// kernels accumulate nothing across trajectories).  A kernel that writes only arrays it does not read (the state passes: x, J from
// x0, u or lam; the plain costate passes: lam from x) stores the overlap twice with the same values.  A kernel that reads an array
// it also writes must NOT: nothing orders the two workgroups, and the later one would read what the earlier one stored.  The costate
// passes that carry the sweep's convergence test (k_costate_scan<MET>, k_costate_plx<MET>: lam replaced in place, status, maxChange,
// the counter of active instances) give an overlapped trajectory ONE owner -- the lanes with b < block * TPW of the last workgroup are
// the neighbour's and store nothing.  Launchers ask for the overlap with batch > TPW and an even batch (16-byte DMA chunks).
__device__ static inline int tile_base(int block, int TPW, int batch) {
  const int b0 = block * TPW;
  return b0 + TPW <= batch ? b0 : batch - TPW;
}

// ---------------------------------------------------------------------------------------
// device layouts of the per-step arrays (x / checkpoints, u, lam, dJdu): THE copy of the index arithmetic
// ---------------------------------------------------------------------------------------
// An array of `cols` columns (time) x `rows` rows x `batch` trajectories lives either batch-minor, element (i, r, b) at
// (i rows + r) batch + b, or tiled (OCS_LAYOUT_TILED): trajectories in tiles of kTile = 16, one row of a tile one 128-byte
// line, element (i, r, b) at ((b / 16) cols + i) rows 16 + r 16 + b % 16 -- everything a workgroup streams over time is one
// sequential run of rows * 128 bytes per column.  In both layouts the rows of consecutive columns follow each other at one
// stride, row(), so the kernels walk an array row by row with one pointer whatever the column; what differs is the stride
// and the trajectory's part of the index, at(b).  A tiled array holds whole tiles: ceil(batch / 16) * 16 trajectories.
// Per-trajectory vectors (x0, J, lamT, lam0) are [rows][batch] in both layouts.
constexpr int kTile = 16;
__host__ __device__ constexpr size_t tiled_tiles(size_t batch) { return (batch + kTile - 1) / kTile; }
__host__ __device__ constexpr size_t tiled_tile_doubles(size_t rows, size_t cols) { return cols * rows * kTile; }
__host__ __device__ constexpr size_t tiled_doubles(size_t rows, size_t cols, size_t batch) {
  return tiled_tiles(batch) * tiled_tile_doubles(rows, cols);
}
__host__ __device__ constexpr size_t tiled_index(size_t rows, size_t cols, size_t i, size_t r, size_t b) {
  return ((b / kTile) * cols + i) * rows * kTile + r * kTile + b % kTile;
}
template <bool TILED>
struct DevLayout {
  size_t s;   // batch-minor: the batch; tiled: doubles per tile, cols * rows * 16
  // cols: the columns of the WHOLE array, also where a launch is handed a pointer to one of its later columns
  __host__ __device__ static inline DevLayout make(size_t batch, size_t rows, size_t cols) {
    return DevLayout{TILED ? tiled_tile_doubles(rows, cols) : batch};
  }
  __host__ __device__ inline size_t row() const { return TILED ? (size_t)kTile : s; }
  __host__ __device__ inline size_t at(size_t b) const { return TILED ? (b / kTile) * s + b % kTile : b; }
  // the same relative to trajectory b0 (a multiple of 16: the first of a workgroup): the part of a workgroup's lanes, small
  // enough for the 32-bit lane offsets of the raw buffer accesses whatever the batch
  __host__ __device__ inline size_t at(size_t b, size_t b0) const { return at(b) - at(b0); }
};

// Wave-uniform read-only tables (step sizes, time coefficients, shared parameters) are read
// through the constant address space so the backend emits scalar (s_load) instead of
// per-lane vector loads: `__restrict__` on struct members does not reach alias analysis.
typedef const double __attribute__((address_space(4))) * uniform_ptr;
__device__ static inline uniform_ptr as_uniform(const double* p) { return (uniform_ptr)p; }
#define PSU(p) as_uniform(p)

// Where a trajectory's parameters come from: the shared block `ps` (uniform, scalar loads) or, for the
// parameters whose bit is set in `pmask`, the per-trajectory array pb[k][batch].
struct ParamSrc {
  uniform_ptr ps;
  const double* pb;
  unsigned pmask;
  size_t B;
  int b;
  __device__ inline double operator()(int k) const {
    return ((pmask >> k) & 1u) ? pb[(size_t)k * B + b] : ps[k];
  }
};

// Bound c of trajectory b: from the shared vector [nC] (bstride 0: the plain load of before) or from the per-trajectory array
// [nC][bstride] with bstride = batch (ProblemDesc::bb)
__device__ static inline double bound_at(const double* v, int c, int bstride, int b) {
  return bstride ? v[(size_t)c * bstride + b] : v[c];
}

// ---------------------------------------------------------------------------------------
// per-step record table
// ---------------------------------------------------------------------------------------
// Everything wave-uniform that step i needs sits in one 64-byte-aligned record:
//   REC[i] = { h, h/2, h/6, h/3, tc(t_2i)[NTC], tc(t_2i+1)[NTC], tc(t_2i+2)[NTC], pad | sc[8] }
__host__ __device__ constexpr int rec_sc_offset(int ntc) { return ((4 + 3 * ntc + 7) / 8) * 8; }
// ... followed by a block of 8 problem-defined step constants (P::step_consts; used by the pipeline kernels)
__host__ __device__ constexpr int rec_stride(int ntc) { return rec_sc_offset(ntc) + 8; }
// The table carries kRecPad extra records before step 0 and after step N-1 (copies of the edge
// records) so that the kernels can keep a ring of prefetched records in flight by just walking a
// pointer, without clamping the index at either end.
constexpr int kRecPad = 4;

template <int NTC>
struct StepRec {
  double h, hh, h6, h3;
  double tcA[NTC], tcM[NTC], tcB[NTC];
};
// Records are read through the VECTOR memory path (every lane loads the same address): vector
// loads return in order, so a ring of RD records can be kept in flight with counted vmcnt
// waits.  Scalar loads return out of order, every wait is lgkmcnt(0), and the newest
// prefetch would always be waited for together with the record that is needed (measured:
// +40 % time per step).
template <int NTC>
__device__ static inline StepRec<NTC> load_rec(const double* q) {
  StepRec<NTC> r;
  r.h = q[0];
  r.hh = q[1];
  r.h6 = q[2];
  r.h3 = q[3];
#pragma unroll
  for (int k = 0; k < NTC; ++k) {
    r.tcA[k] = q[4 + k];
    r.tcM[k] = q[4 + NTC + k];
    r.tcB[k] = q[4 + 2 * NTC + k];
  }
  return r;
}

// Ring of PF prefetched step records, the one every lane kernel walks the table with.  `Rec rq[PF]` and the table pointer
// `recp` are the caller's locals, and the caller fills the ring with its own loop (why: NOTES.md, "Lane RK4 kernels").
// DIR is the direction of that loop and has to match it: +1 where it steps `recp += rec_stride(NTC)` up from step 0,
// -1 where it steps `recp -= rec_stride(NTC)` down from step N-1.  rec_ring_next hands out the oldest record, rq[0], and
// requests one more; until then rq[q] is the record that the q-th call from now returns.  The table is padded by kRecPad
// records at either end, so the ring never clamps.  PF steps of lead, not one: a step is shorter than the L2 round trip
// of a new record.
template <int NTC, int PF, int DIR>
__device__ inline OCS_INLINE StepRec<NTC> rec_ring_next(StepRec<NTC> (&rq)[PF], const double*& recp) {
  static_assert(PF <= kRecPad, "record ring deeper than the table padding");
  static_assert(DIR == 1 || DIR == -1, "walking direction");
  const StepRec<NTC> cur = rq[0];
#pragma unroll
  for (int q = 0; q + 1 < PF; ++q) rq[q] = rq[q + 1];
  rq[PF - 1] = load_rec<NTC>(recp);
  recp += DIR * rec_stride(NTC);
  return cur;
}

// ---------------------------------------------------------------------------------------
// one RK4 step of a lane (= trajectory), forward and reverse: THE copy of the lane kernels' arithmetic
// ---------------------------------------------------------------------------------------
// compute_states, RK4Integrator.m:36-51: y (and the running objective yc) from node i to i+1, controls at grid points
// 2i (uA), 2i+1 (uM), 2i+2 (uB).  COST = false is the same step on the state rows only (P::Fx; yc untouched): the
// adjoint kernel's re-integration of checkpoints, which has to reproduce the state pass bit for bit.
template <class P, bool COST = true>
__device__ inline OCS_INLINE void lane_state_step(const StepRec<P::NTC>& r, double* y, double& yc, const double* uA,
                                                  const double* uM, const double* uB, const typename P::Par& p) {
  constexpr int NS = P::NS, NF = COST ? NS + 1 : NS;
  auto rhs = [&](const double* tc, const double* x, const double* u, double* f) OCS_INLINE {
    if constexpr (COST) P::F(tc, x, u, p, f);
    else P::Fx(tc, x, u, p, f);
  };
  double F1[NF], F2[NF], F3[NF], F4[NF], Y[NS];
  rhs(r.tcA, y, uA, F1);                                                 // :39
#pragma unroll
  for (int k = 0; k < NS; ++k) Y[k] = __builtin_fma(r.hh, F1[k], y[k]);  // :40
  rhs(r.tcM, Y, uM, F2);                                                 // :42
#pragma unroll
  for (int k = 0; k < NS; ++k) Y[k] = __builtin_fma(r.hh, F2[k], y[k]);  // :43
  rhs(r.tcM, Y, uM, F3);                                                 // :45
#pragma unroll
  for (int k = 0; k < NS; ++k) Y[k] = __builtin_fma(r.h, F3[k], y[k]);   // :46
  rhs(r.tcB, Y, uB, F4);                                                 // :48
#pragma unroll
  for (int k = 0; k < NS; ++k)                                           // :50-51
    y[k] = __builtin_fma(r.h6, __builtin_fma(2.0, F3[k], __builtin_fma(2.0, F2[k], F1[k])) + F4[k], y[k]);
  if constexpr (COST)
    yc = __builtin_fma(r.h6, __builtin_fma(2.0, F3[NS], __builtin_fma(2.0, F2[NS], F1[NS])) + F4[NS], yc);
}
template <class P>
__device__ inline OCS_INLINE void lane_state_rows_step(const StepRec<P::NTC>& r, double* y, const double* uA,
                                                       const double* uM, const double* uB, const typename P::Par& p) {
  double none = 0.0;
  lane_state_step<P, false>(r, y, none, uA, uM, uB, p);
}

// compute_adjoints, RK4Integrator.m:73-88, with compute_dJdu :97-121 fused in: the reverse of step i from the checkpoint
// xi = y_i.  lam(1:nS) is updated in place; lamc = lam(end,:) is constant (the last row of dFdx_times_vec is 0,
// OCProblem.m:14-15).  With DJDU the two columns of dJdu that this step finishes are handed to columns(dn, dm) -- dn is
// column 2i+2 (k4 of this step plus pend, the k1-term of step i+1), dm column 2i+1 -- before pend becomes this step's
// k1-term and lam is updated: the caller stores or folds them at the place where every lane kernel always did (after
// the step instead, the fused kernels spill).  Without DJDU the dFduT calls vanish and columns is never called.
template <class P, bool DJDU, class Columns>
__device__ inline OCS_INLINE void lane_adjoint_step(const StepRec<P::NTC>& r, const double* xi, const double* uA,
                                                    const double* uM, const double* uB, const typename P::Par& p,
                                                    double* lam, const double lamc, double* pend, Columns&& columns) {
  constexpr int NS = P::NS, NC = P::NC, NAUG = P::NAUG;
  // stage states xK(:,i,2:4), recomputed (compute_states :39-46)
  double f[NS], Y2[NS], Y3[NS], Y4[NS];
  P::Fx(r.tcA, xi, uA, p, f);
#pragma unroll
  for (int k = 0; k < NS; ++k) Y2[k] = __builtin_fma(r.hh, f[k], xi[k]);
  P::Fx(r.tcM, Y2, uM, p, f);
#pragma unroll
  for (int k = 0; k < NS; ++k) Y3[k] = __builtin_fma(r.hh, f[k], xi[k]);
  P::Fx(r.tcM, Y3, uM, p, f);
#pragma unroll
  for (int k = 0; k < NS; ++k) Y4[k] = __builtin_fma(r.h, f[k], xi[k]);
  // dJdk(:,i,4..1) and the dJdx terms   :73-88
  double k4[NAUG], k3[NAUG], k2[NAUG], k1[NAUG], g3[NS], g2[NS], g1[NS], g0[NS];
#pragma unroll
  for (int k = 0; k < NS; ++k) k4[k] = r.h6 * lam[k];                             // :73
  k4[NS] = r.h6 * lamc;
  P::dFdxT(r.tcB, Y4, uB, p, k4, g3);                                             // :74-75
#pragma unroll
  for (int k = 0; k < NS; ++k) k3[k] = __builtin_fma(r.h, g3[k], r.h3 * lam[k]);  // :77
  k3[NS] = r.h3 * lamc;
  P::dFdxT(r.tcM, Y3, uM, p, k3, g2);                                             // :78-79
#pragma unroll
  for (int k = 0; k < NS; ++k) k2[k] = __builtin_fma(r.hh, g2[k], r.h3 * lam[k]); // :81
  k2[NS] = r.h3 * lamc;
  P::dFdxT(r.tcM, Y2, uM, p, k2, g1);                                             // :82-83
#pragma unroll
  for (int k = 0; k < NS; ++k) k1[k] = __builtin_fma(r.hh, g1[k], r.h6 * lam[k]); // :85
  k1[NS] = r.h6 * lamc;
  P::dFdxT(r.tcA, xi, uA, p, k1, g0);                                             // :87-88
  if constexpr (DJDU) {  // compute_dJdu :97-121: column 2i+2 pairs k4 of step i with k1 of step i+1
    double d4[NC], d3[NC], d2[NC];
    P::dFduT(r.tcB, Y4, uB, p, k4, d4);
    P::dFduT(r.tcM, Y3, uM, p, k3, d3);
    P::dFduT(r.tcM, Y2, uM, p, k2, d2);
    double dn[NC], dm[NC];
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      dn[c] = pend[c] + d4[c];  // column 2i+2  :112-116 (:119-120 at i = N-1)
      dm[c] = d2[c] + d3[c];    // column 2i+1  :105-109
    }
    columns(dn, dm);
    P::dFduT(r.tcA, xi, uA, p, k1, pend);
  }
#pragma unroll
  for (int k = 0; k < NS; ++k) lam[k] = (((lam[k] + g1[k]) + g2[k]) + g3[k]) + g0[k];  // :86-88
}

// pchip (Fritsch-Carlson / MATLAB pchipslopes) interior slope of a node between secants del0, del1 with weights w1, w2:
// with ONE division: |del0 del1| / (w1 |del0| + w2 |del1|) (pchip_interior's harmonic mean multiplied
// through by dmax; round-off level difference to the two-division form of the midpoint kernel)
__device__ static inline double pchip_interior1(double del0, double del1, double w1, double w2) {
  const bool same = (del0 > 0.0 && del1 > 0.0) || (del0 < 0.0 && del1 < 0.0);
  const double a0 = fabs(del0), a1 = fabs(del1);
  double d = (a0 * a1) / __builtin_fma(w1, a0, w2 * a1);
  asm("" : "+v"(d));  // opaque: keeps the division out of a divergent branch (0/0 lanes are discarded below); not
                      // volatile, so that the divisions of neighbouring nodes still overlap
  return same ? (del0 > 0.0 ? d : -d) : 0.0;
}

// the same slope from the signed secants: del0 del1 / (w1 del0 + w2 del1) -- the quotient of the absolute values with the
// common sign of the secants, bit for bit, in fewer instructions (k_forward_cc's control waves are VALU-bound)
__device__ static inline double pchip_interior_s(double del0, double del1, double w1, double w2) {
  const double pr = del0 * del1;
  double d = pr / __builtin_fma(w1, del0, w2 * del1);
  asm("" : "+v"(d));
  return pr > 0.0 ? d : 0.0;
}

// ... and with the quotient by reciprocal + Newton steps instead of the IEEE division sequence (no scaling: the secants of
// a costate are far from the ends of the exponent range; at most an ulp from the correctly rounded quotient)
// (v_rcp_f64 is good to 2^29 ulp, i.e. ~1e-7 relative; one Newton step on the reciprocal takes that to ~1e-14, and the
//  correction of the quotient multiplies the two errors: full precision in six operations)
__device__ static inline double fast_div(double n, double d) {
  double r = __builtin_amdgcn_rcp(d);
  r = __builtin_fma(__builtin_fma(-d, r, 1.0), r, r);
  const double q = n * r;
  return __builtin_fma(__builtin_fma(-d, q, n), r, q);
}
__device__ static inline double pchip_interior_f(double del0, double del1, double w1, double w2) {
  const double pr = del0 * del1;
  const double d = fast_div(pr, __builtin_fma(w1, del0, w2 * del1));
  return pr > 0.0 ? d : 0.0;
}

// per-interval pchip records of the node grid (built by k_pchip_records, streamed by k_costate_plx / k_forward_cc):
// doubles per interval i: {h(i-1), h(i), h(i+1), 1/h(i-1), 1/h(i), 1/h(i+1), W1(i), W2(i), W1(i+1), W2(i+1), tmid_i - t_i, h(i)/8, pad}
// pchip at the MIDDLE of an interval (all the sweep kernels need) is the Hermite cubic's closed form there,
// (y0 + y1)/2 + h/8 (d0 - d1): four operations instead of the ten of the general evaluation; tmid_i is the rounded
// (t_i + t_i+1)/2, so this differs from evaluating at tmid_i by round-off
constexpr int kPRec = 16;
// pchip end slope (MATLAB pchipslopes' three-point formula with its two shape-preserving corrections)
__device__ static inline double pchip_end_pl(double h0, double h1, double del0, double del1) {
  double d = ((2.0 * h0 + h1) * del0 - h0 * del1) / (h0 + h1);
  const bool s0 = (d > 0.0) == (del0 > 0.0) && (d < 0.0) == (del0 < 0.0);
  const bool s1 = (del0 > 0.0) == (del1 > 0.0) && (del0 < 0.0) == (del1 < 0.0);
  if (!s0)
    d = 0.0;
  else if (!s1 && fabs(d) > fabs(3.0 * del0))
    d = 3.0 * del0;
  return d;
}

// The record table is written by another kernel and is cold in this XCD's L2: a scalar load
// that misses to the Infinity Cache / HBM costs more than a whole RK4 step.  Every wave
// therefore sweeps the table once with wide vector loads (1 KiB per instruction) before the
// recursion starts, so the per-step scalar loads that follow are L2 hits.
__device__ static inline double warm_table(const double* tab, size_t ndoubles) {
  typedef double double2v __attribute__((ext_vector_type(2)));
  const double2v* q = reinterpret_cast<const double2v*>(tab);
  const size_t n2 = ndoubles / 2;
  double acc = 0.0;
  size_t k = threadIdx.x & 63;
  for (; k + 15 * 64 < n2; k += 16 * 64) {
    double2v v[16];
#pragma unroll
    for (int j = 0; j < 16; ++j) v[j] = q[k + (size_t)j * 64];
#pragma unroll
    for (int j = 0; j < 16; ++j) acc += v[j].x + v[j].y;
  }
  for (; k < n2; k += 64) acc += q[k].x + q[k].y;
  return acc;  // the caller keeps it alive behind a never-taken branch
}

// ---------------------------------------------------------------------------------------
// pchip (Fritsch-Carlson slopes as in MATLAB pchip / Moler's pchiptx), per lane
// ---------------------------------------------------------------------------------------
__device__ static inline int dsgn(double v) { return (v > 0.0) - (v < 0.0); }

// interior node: weighted harmonic mean of the neighbouring secants, 0 at a local extremum
__device__ static inline double pchip_interior(double del0, double del1, double w1, double w2) {
  if (dsgn(del0) * dsgn(del1) <= 0) return 0.0;
  const double a0 = fabs(del0), a1 = fabs(del1);
  const double dmax = fmax(a0, a1), dmin = fmin(a0, a1);
  return dmin / (w1 * (del0 / dmax) + w2 * (del1 / dmax));
}
// end node: non-centred three-point formula with the two shape-preserving corrections
__device__ static inline double pchip_end(double h0, double h1, double del0, double del1) {
  double d = ((2.0 * h0 + h1) * del0 - h0 * del1) / (h0 + h1);
  if (dsgn(d) != dsgn(del0))
    d = 0.0;
  else if (dsgn(del0) != dsgn(del1) && fabs(d) > fabs(3.0 * del0))
    d = 3.0 * del0;
  return d;
}

// Node tables (uniform): TN[0..n-1] node times, HN[0..n-2] spacings, W1/W2[1..n-2] slope weights, IH = 1./HN.
struct PchipTab {
  int n;
  const double* TN;
  const double* HN;
  const double* W1;
  const double* W2;
  const double* IH;  // 1 ./ HN
};

// slope at node k of the samples v(k) = V[(k*ld + row)*B + b]
__device__ static inline double pchip_slope_at(const PchipTab& T, const double* V, size_t ldB, int k) {
  const int n = T.n;
  auto val = [&](int j) OCS_INLINE { return V[(size_t)j * ldB]; };
  if (n == 2) return (val(1) - val(0)) / T.HN[0];
  if (k == 0) {
    const double d0 = (val(1) - val(0)) / T.HN[0], d1 = (val(2) - val(1)) / T.HN[1];
    return pchip_end(T.HN[0], T.HN[1], d0, d1);
  }
  if (k == n - 1) {
    const double d0 = (val(n - 1) - val(n - 2)) / T.HN[n - 2], d1 = (val(n - 2) - val(n - 3)) / T.HN[n - 3];
    return pchip_end(T.HN[n - 2], T.HN[n - 3], d0, d1);
  }
  const double d0 = (val(k) - val(k - 1)) / T.HN[k - 1], d1 = (val(k + 1) - val(k)) / T.HN[k];
  return pchip_interior(d0, d1, T.W1[k], T.W2[k]);
}
// cubic Hermite piece on an interval of length h with end values v0, v1 and end slopes dk, dk1 (pwch + ppval)
__device__ static inline double pchip_piece(double v0, double v1, double dk, double dk1, double h, double s) {
  const double del = (v1 - v0) / h;
  const double dzzdx = (del - dk) / h, dzdxdx = (dk1 - del) / h;
  const double c3 = (dzdxdx - dzzdx) / h, c2 = 2.0 * dzzdx - dzdxdx;
  return v0 + s * (dk + s * (c2 + s * c3));
}


}  // namespace ocs
