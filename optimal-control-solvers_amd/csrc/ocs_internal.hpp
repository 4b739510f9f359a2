// ocs_internal.hpp -- launcher interface between the C-ABI layer (ocs_api.cpp) and the
// gfx950 kernels (ocs_kernels.hip).  Not part of the public boundary.
#pragma once
#include <cstdlib>
#include <hip/hip_runtime.h>
#include <stddef.h>

namespace ocs {

// what a launcher returns: 0, or the HIP error as it is
inline int hip_rc(hipError_t e) { return e == hipSuccess ? 0 : (int)e; }

// Which device functor a problem handle resolves to.
enum class Functor : int { Logistic = 1, LQ = 3, User = 100 };
struct UserModule;  // hipRTC-compiled user problem (ocs_jit.hpp)

struct LqWorkspace;   // chunk matrices and scratch of the time-parallel LQ passes (ocs_lq_kernels.hip), owned by an integrator
void lq_workspace_free(LqWorkspace* w);

struct ProblemDesc {
  Functor functor;
  int nS, nC;
  int npar;
  const double* ps;   // device: shared parameter block [npar]
  const double* pb;   // device: per-trajectory overrides [npar][batch] or nullptr
  unsigned pmask;     // bit k set -> parameter k is read from pb
  // Functor::LQ only: per-trajectory cost weights [nS + nC][Wbatch] (rows 0 .. nS-1 = q, then rdiag; rows that were not
  // overridden hold the shared block's values), or nullptr.  The parameter block of that problem has up to 1189 entries, so
  // a mask word cannot name them; never set together with pmask.
  const double* W = nullptr;
  int Wbatch = 0;
  const double* lb;   // device: control lower bounds [nC], or row 0 of bb
  const double* ub;   // device: control upper bounds [nC], or row nC of bb
  // per-trajectory control bounds [2 nC][bstride] (lower rows, then upper rows) or nullptr; bstride 0: lb / ub are the shared
  // [nC] vectors, bstride = batch: bound c of trajectory b is lb[c * bstride + b] (bound_at, ocs_device_common.hpp)
  const double* bb = nullptr;
  int bstride = 0;
  const UserModule* user = nullptr;  // set for Functor::User
  unsigned long long version = 0;    // of the handle's device-visible parameters (cache key of tables derived from them)
};

struct GridDesc {
  int N;              // nSTEPS
  const double* HT;   // device: [N][4] = {h, h/2, h/6, h/3} (host IEEE divisions, RK4Integrator.m:40,50,73,77)
  const double* T;    // device: [2N+1] grid times (obj.t)
  double* TC;         // device: [2N+1][NTC] time coefficients of the bound problem (F side)
  double* TU;         // device: [2N+1][NTU] time coefficients of its ControlChar
  double* REC;        // device: [N][rec_stride(NTC)] per-step records {h,h/2,h/6,h/3,tcA,tcM,tcB}
  double* RECS = nullptr;  // device: compact zero-padded records of the scan kernels (record of step 0), or nullptr
  bool uniform = false;    // every step has the same size (bitwise): kernels may keep h, h/2, h/6, h/3 in registers
  LqWorkspace** lqws = nullptr;  // where the integrator keeps the workspace of the time-parallel LQ passes (created on first use)
};

// Device-native layouts (batch-minor): x0 [nS][B], u [2N+1][nC][B], x [N+1][nAug][B],
// lam [N+1][nAug][B], dJdu [2N+1][nC][B], J [B], lamT [nAug][B].
int launch_tcoef(const ProblemDesc& p, const GridDesc& g, hipStream_t s);
// mapping of the serial RK4 kernels: lane-per-trajectory (ocs_kernels.hip) or row-split
// (ocs_rowsplit_kernels.hip, row-separable problems only)
enum Mapping : int { MAP_AUTO = 0, MAP_LANE = 1, MAP_ROWSPLIT = 2, MAP_PIPELINE = 3, MAP_SCAN = 4 };
// adjoint pass as a scan over time (ocs_scan_kernels.hip): row-separable problems, any N, any batch
bool scan_supported(Functor f, int nS, int nC);
// the same for a bound problem: registry problems as above, user problems if given as row functions (hipRTC instances)
bool user_rowsep(const UserModule* m);
bool scan_problem_ok(const ProblemDesc& p);
bool pipeline_problem_ok(const ProblemDesc& p);
// any OCProblem with nS <= 4, nC <= 2 (coupled rows, several controls): the vector-lane state pass
// (ocs_pipelinev_kernel.hpp; whole blocks of 8 steps, whole tiles of 64 trajectories) and the scan adjoint pass with
// dense step maps (ocs_vscan_kernel.hpp; N a multiple of scan_chunk_steps())
bool user_vector(const UserModule* m);
// a user problem given as row functions whose ocs_ControlChar reads the costate alone and whose ocs_row_dFdy does not
// read u (flag bit 2): the folded sweep of fb_sweep is instantiated for it
bool user_fold(const UserModule* m);
bool vector_problem_ok(const ProblemDesc& p);
int launch_forward_pv(const ProblemDesc& p, const GridDesc& g, int batch, const double* x0, const double* u, double* x,
                      double* J, hipStream_t s, bool no_cost_row, const int* gate, const int* frozen = nullptr);
int launch_backward_vscan(const ProblemDesc& p, const GridDesc& g, int batch, const double* xck, const double* u,
                          const double* lamT, double* lam, double* dJdu, double* lam0, const double* pend0,
                          hipStream_t s);
// N a multiple of scan_chunk_steps(); pend0 as for launch_backward_pl
int scan_chunk_steps();
int launch_backward_scan(const ProblemDesc& p, const GridDesc& g, int batch, const double* xck, const double* u,
                         const double* lamT, double* lam, double* dJdu, double* lam0, const double* pend0,
                         hipStream_t s);
// the scan kernels' record table: scan_recs_doubles(N) doubles at RECS_base, built from REC (stride rs, step
// constants at sco); GridDesc::RECS = RECS_base + scan_recs_front()
size_t scan_recs_doubles(int N);
size_t scan_recs_front();
int launch_build_recs(int N, int rs, int sco, const double* REC, double* RECS_base, hipStream_t s);
bool pipeline_supported(Functor f, int nS, int nC);
// tiles of `tile` trajectories: whole, or with a ragged last tile taken by a workgroup that overlaps its neighbour (tile_base,
// ocs_device_common.hpp): more than one tile and an even batch
// (odd batches were tried: with four states the overlapped instances of the sweep kernels then differ at 1e-8 between the two
//  workgroups that compute them -- rows start at odd multiples of 8 bytes and the kernels pair trajectories in 16-byte accesses;
//  one and two states were clean.  Even batches only.)
inline bool tile_ok(int batch, int tile) { return batch % tile == 0 || (batch > tile && batch % 2 == 0); }
inline int tile_count(int batch, int tile) { return (batch + tile - 1) / tile; }
bool pipeline_shape_ok(int nS, int N, int batch, bool backward);  // nSTEPS multiple of the block, batch of the tile
int pipeline_block_steps();  // the pipeline kernels take whole blocks of this many steps
// wave-specialised costate pass of the sweep (registry problems whose adjoint right-hand side does not read u)
bool costate_pl_ok(Functor f, int nS, int nC, int N, int batch);
// the same forming the pchip midpoints of x itself (no xmid array); PR: [N][costate_prec()] interval records
int costate_prec();
int launch_costate_plx(const ProblemDesc& p, const GridDesc& g, int batch, const double* x, int ldx, const double* PR,
                       const int* frozen, double* dump, double* lam, hipStream_t s, const int* gate = nullptr);
// the same pass as a scan over time (ocs_costate_scan_kernel.hpp); _met: with the convergence test of the folded sweep
bool costate_scan_ok(const ProblemDesc& p, const GridDesc& g, int batch);
bool costate_scan_u_ok(const ProblemDesc& p, const GridDesc& g, int batch);
// any user problem with nS <= 4, nC <= 2 given as full-vector methods: the costate pass as a scan with dense step maps
bool costate_vscan_ok(const ProblemDesc& p, const GridDesc& g, int batch);
int launch_costate_vscan(const ProblemDesc& p, const GridDesc& g, int batch, const double* x, int ldx, const double* PR,
                         const double* u, const int* frozen, double* lam, hipStream_t s, const int* gate);
int launch_costate_scan_u(const ProblemDesc& p, const GridDesc& g, int batch, const double* x, int ldx, const double* PR,
                          const double* u, const int* frozen, double* lam, hipStream_t s, const int* gate);
int launch_costate_scan(const ProblemDesc& p, const GridDesc& g, int batch, const double* x, int ldx, const double* PR,
                        const int* frozen, double* lam, hipStream_t s, const int* gate);
int launch_costate_scan_met(const ProblemDesc& p, const GridDesc& g, int batch, const double* x, int ldx, const double* PR,
                            const double* lb, const double* ub, double relTol, double absTol, int sweep, int* status,
                            double* maxChange, int* nactive, double* lam, hipStream_t s, const int* gate);
int launch_costate_pl(const ProblemDesc& p, const GridDesc& g, int batch, const double* x, int ldx, const double* xmid,
                      const int* frozen, double* dump, double* lam, hipStream_t s);
// pend0: optional [B], the k1 half of column 2N of dJdu when the steps above N were integrated by another kernel
int launch_backward_pl(const ProblemDesc& p, const GridDesc& g, int batch, const double* xck, const double* u,
                       const double* lamT, double* lam, double* dJdu, double* lam0, const double* pend0,
                       hipStream_t s);
// the same pass with a minimal recursion wave (ocs_pipeline2_kernels.hip)
int launch_forward_p2(const ProblemDesc& p, const GridDesc& g, int batch, const double* x0, const double* u,
                      double* x, double* J, const int* frozen, hipStream_t s, bool no_cost_row, const int* gate);
// whether launch_forward with these shapes runs the one kernel that honours FwdOpts::gate
bool forward_gate_supported(const ProblemDesc& p, const GridDesc& g, int batch);
// workgroups (of 64/nS trajectories) up to which fb_sweep takes its wave-specialised kernels (the folded two-kernel sweep, the
// costate kernels that form the midpoints of x); OCS_FOLD_MAX_WG overrides (tuning)
int fold_wg_limit();
bool rowsplit_supported(Functor f, int nS, int nC);
int launch_forward_rs(const ProblemDesc& p, const GridDesc& g, int batch, const double* x0, const double* u,
                      double* x, double* J, hipStream_t s);
int launch_backward_rs(const ProblemDesc& p, const GridDesc& g, int batch, const double* xck, const double* u,
                       const double* lamT, double* lam, double* dJdu, double* lam0, hipStream_t s);

// the pass pair on tiled arrays (OCS_LAYOUT_TILED; index map: ocs_device_common.hpp): registry logistic problems with 1, 2 or 4
// states and shared parameters.  g.N: the steps of this launch, whole blocks (8) / chunks (scan_chunk_steps()) from step 0;
// nodes: N + 1 of the whole pass; x / u / xck / lam / dJdu: the whole tiled arrays
int launch_forward_p2_tiled(const ProblemDesc& p, const GridDesc& g, int nodes, int batch, const double* x0,
                            const double* u, double* x, double* J, hipStream_t s);
int launch_backward_scan_tiled(const ProblemDesc& p, const GridDesc& g, int nodes, int batch, const double* xck,
                               const double* u, const double* lamT, bool lamT_col, double* lam, double* dJdu, double* lam0,
                               const double* pend0, hipStream_t s);
// batch-minor [nR][batch] <-> tiled, nR = cols * rows
int launch_tiled_convert(bool to_tiled, const double* src, double* dst, size_t nR, int batch, hipStream_t s);
size_t tiled_doubles_host(size_t rows, size_t cols, size_t batch);
bool tiled_supported(const ProblemDesc& p);
enum Layout : int { LAYOUT_BATCH_MINOR = 0, LAYOUT_TILED = 1 };
struct FwdOpts;
struct BwdOpts;
// matrix-core kernels of the shared-Jacobian linear-quadratic problem (ocs_lq_kernels.hip)
bool lq_supported(int nS, int nC);
int launch_tcoef_lq(const ProblemDesc& p, const GridDesc& g, hipStream_t s);
int launch_forward_lq(const ProblemDesc& p, const GridDesc& g, int batch, const double* x0, const double* u,
                      double* x, double* J, const FwdOpts& o, hipStream_t s);
int launch_backward_lq(const ProblemDesc& p, const GridDesc& g, int batch, const double* xck, const double* u,
                       const double* lamT, double* lam, double* dJdu, const BwdOpts& o, hipStream_t s);
// fb_sweep's state and costate passes of the same problem on the matrix cores (ocs_lq_sweep_kernels.hip), one wave per
// 16 trajectories.  g.REC: the LQ problem's own step records (launch_tcoef_lq), not those of the integrator's bound
// problem.  frozen / gate as FwdOpts; stores of frozen instances are dropped, no scratch array.  x [N+1][ldx][B] with
// ldx = nS + 1, xmid [N][nS][B] (launch_pchip_mid), lam [N+1][nS][B].  The costate pass reads no control samples.
int launch_sweep_forward_lq(const ProblemDesc& p, const GridDesc& g, int batch, const double* x0, const double* u,
                            double* x, double* J, const int* frozen, const int* gate, hipStream_t s);
int launch_sweep_costate_lq(const ProblemDesc& p, const GridDesc& g, int batch, const double* x, int ldx,
                            const double* xmid, const int* frozen, double* lam, const int* gate, hipStream_t s);
// 'nearest' / 'next' of griddedInterpolant: index of the sample a query point takes, -1 = NaN (ocs_control.cpp)
int interp_sample_index(int method, int n, const double* x, double q);
int launch_eval_lq(const ProblemDesc& p, int which, int k, const double* t, const double* y, const double* u,
                   const double* v, double* out, hipStream_t s);

struct FwdOpts {
  int mapping = MAP_AUTO;
  bool uconst = false;          // u is a device [nC] vector shared by all grid points and trajectories
  bool uconst_batch = false;    // with uconst: u is [nC][B], one constant control per trajectory (ocs_rk4inf_set_batch_ustar)
  unsigned long long uversion = 0;  // with uconst: bumps whenever the values behind u change (what is cached per u follows it)
  const double* Jadd = nullptr; // J = Jadd + x(end,end)
  const int* frozen = nullptr;  // [B]: trajectories with frozen[b] != 0 store nothing (fb_sweep: converged instances)
  double* dump = nullptr;       // [B] scratch the stores of frozen trajectories go to
  const int* gate = nullptr;    // device flag: the launch does nothing if *gate == 0 (only where
                                // forward_gate_supported says so; otherwise the call fails)
  bool no_cost_row = false;     // the running-objective row of x may be left unwritten (only J is wanted); honoured
                                // where it saves traffic (the pipeline kernel), ignored elsewhere
  int layout = LAYOUT_BATCH_MINOR;  // of x and u; tiled: plain passes only (none of the options above), pipeline + lane remainder
};
struct BwdOpts {
  int mapping = MAP_AUTO;
  bool uconst = false;
  bool uconst_batch = false;    // as FwdOpts
  double* lam0 = nullptr;       // [nAug][B]: lam(:,1)
  double* split_scratch = nullptr;  // [nAug][B]: hand-over column of a split pass when no lam array is requested
  int layout = LAYOUT_BATCH_MINOR;  // of xck, u, lam and dJdu; tiled: plain passes only, scan + lane remainder
};
int launch_forward(const ProblemDesc& p, const GridDesc& g, int batch, const double* x0, const double* u,
                   double* x, double* J, const FwdOpts& o, hipStream_t s);
int launch_backward(const ProblemDesc& p, const GridDesc& g, int batch, const double* xck, const double* u,
                    const double* lamT, double* lam, double* dJdu, const BwdOpts& o, hipStream_t s);
// which: 0 F, 1 dFdx_times_vec, 2 dFdu_times_vec; column-major device arrays with k columns.
int launch_eval(const ProblemDesc& p, int which, int k, const double* t, const double* y, const double* u,
                const double* v, double* out, hipStream_t s);
// batched compute_equilibrium (k_equilibrium, ocs_rk4_kernels.hpp): y0 / y / residual [2 nS + nC][B], lb / ub [2 nS + nC]
int launch_equilibrium(const ProblemDesc& p, int batch, double r, const double* y0, const double* lb, const double* ub,
                       double* y, double* resnorm, double* residual, int* exitflag, int max_iter, double tol,
                       hipStream_t s);
// layout helpers; per = doubles per trajectory
int launch_to_batch_minor(const double* src, double* dst, int per, int batch, hipStream_t s);
int launch_to_traj_major(const double* src, double* dst, int per, int batch, hipStream_t s);
int launch_copy8(const double* src, double* dst, size_t n, hipStream_t s);
// number of non-finite entries of v[0..n) is added to *count (device int)
int launch_count_nonfinite(const double* v, int n, int* count, hipStream_t s);
// out[0..3] = {sum of the finite J[i], their number, min J, lo + index of the minimum (-1 if none is finite)}
int launch_objective_stats(const double* J, int n, int lo, double* out, hipStream_t s, const int* mask = nullptr);
// status[i] = OCS_NUM_NONFINITE if J[i] is NaN/Inf, else 0
int launch_traj_status(const double* J, int n, int* status, hipStream_t s);

// control bases (ocs_control_kernels.hip); v [nBasis][nC][B], u / dJdu [nT][nC][B]
int launch_basis_expand(int nT, int nC, int batch, const int* colptr, const int* row, const double* val,
                        const double* v, double* u, hipStream_t s);
int launch_basis_contract(int nBasis, int nC, int batch, const int* rowptr, const int* col, const double* val,
                          const double* dJdu, double* dJdv, hipStream_t s);
bool basis_dense_supported(int nBasis);
int launch_basis_dense(bool expand, int nBasis, int nT, int nC, int batch, const double* BT, const double* in,
                       double* out, hipStream_t s);
// out[j][c][b] = val[c], or val[c][b] with per_traj (val is [nC][batch])
int launch_fill_rows(int ncols, int nC, int batch, const double* val, double* out, hipStream_t s, bool per_traj = false);
// out[i] = a[i] + b[i]
int launch_add_vec(int n, const double* a, const double* b, double* out, hipStream_t s);
// RK4InfiniteIntegrator's tail leg (constant control): true where the wave-specialised state pass would be chosen for this grid
// and batch -- the tail then runs on samples of the constant control instead of the lane kernels (ocs_api.cpp)
bool tail_leg_wave_ok(const ProblemDesc& p, const GridDesc& g, int batch);
int launch_gather_rows(int nrows, int batch, const int* idx, const double* src, double* dst, hipStream_t s);
int launch_scatter_rows(int nrows, int batch, const int* idx, const double* src, double* dst, hipStream_t s);

// shooting objective + gradient with the (dense, <= 32 functions) control basis fused into the RK4 kernels
// (ocs_fused_control_kernels.hip).  BT16: transposed basis [2N+1][16 or 32], zero-padded (16 when nBasis <= 16)
bool fused_control_supported(Functor f, int nS, int nC, int nBasis);
int launch_forward_fc(const ProblemDesc& p, const GridDesc& g, int batch, int nBasis, const double* BT16,
                      const double* v, const double* x0, double* ck, double* J, hipStream_t s);
int launch_backward_fc(const ProblemDesc& p, const GridDesc& g, int batch, int nBasis, const double* BT16,
                       const double* v, const double* ck, double* dJdv, double* lam0, hipStream_t s);

// the same on the wave-specialised state pass and the adjoint scan, both basis products on the matrix cores
// (ocs_fused_wave_kernels.hip); BT: [2N+1][ldbt] as BT16
bool fused_wave_supported(Functor f, int nS, int nC, int nBasis, int N, int batch);
int launch_forward_fcw(const ProblemDesc& p, const GridDesc& g, int batch, int nBasis, int ldbt, const double* BT,
                       const double* v, const double* x0, double* ck, double* J, hipStream_t s);
int launch_backward_fcs(const ProblemDesc& p, const GridDesc& g, int batch, int nBasis, int ldbt, const double* BT,
                        const double* v, const double* ck, double* dJdv, double* lam0, hipStream_t s);

// the same for a banded basis (PWLinear, PWConstant; ocs_fused_banded_kernels.hip).  CT: column table
// [2N+1][fused_banded_rec()] = {w0, w1, adv, pad}, r0 the first row of column 0; dJdv must be zero-filled
bool fused_banded_supported(Functor f, int nS, int nC);
int fused_banded_rec();
int launch_forward_fb(const ProblemDesc& p, const GridDesc& g, int batch, int nBasis, int r0, const double* CT,
                      const double* v, const double* x0, double* ck, double* J, hipStream_t s);
int launch_backward_fb(const ProblemDesc& p, const GridDesc& g, int batch, int nBasis, int r0, const double* CT,
                       const double* v, const double* ck, double* dJdv, double* lam0, hipStream_t s);

// forward-backward sweep (ocs_fbs_kernels.hip)
struct FbsTables {   // pchip node tables of an integrator grid, device pointers
  int n;             // number of nodes N+1
  const double* TN;  // [n] node times
  const double* HN;  // [n-1] spacings
  const double* W1;  // [n] interior slope weights (entries 1..n-2 used)
  const double* W2;
  const double* TM;  // [n-1] interval midpoints
  const double* IH;  // [n-1] reciprocal spacings
  const double* PR;  // [n-1][costate_prec()] per-interval pchip records (launch_costate_plx)
};
int launch_pchip_mid(const FbsTables& t, int nrows, int ld, int batch, const double* V, double* out, hipStream_t s,
                     const int* gate = nullptr);
bool costate_forms_midpoints(const ProblemDesc& p, int N, int batch);
// fb_sweep with the control update folded into the state pass (ocs_fold_kernel.hpp) and the convergence test into the
// costate pass (k_costate_plx, MET): sweeps >= 2 are two kernels
bool fold_supported(const ProblemDesc& p, const GridDesc& g, int batch);
int launch_forward_cc(const ProblemDesc& p, const GridDesc& g, int batch, const double* PR, const double* lb,
                      const double* ub, const double* x0, const double* lam, double* x, double* J, const int* frozen,
                      bool no_cost_row, const int* gate, bool first_sweep, hipStream_t s);
int launch_costate_met(const ProblemDesc& p, const GridDesc& g, int batch, const double* x, int ldx, const double* PR,
                       const double* lb, const double* ub, double relTol, double absTol, int sweep, int* status,
                       double* maxChange, int* nactive, double* lam, hipStream_t s, const int* gate);
int launch_costate(const ProblemDesc& p, const GridDesc& g, int batch, const double* x, int ldx, const double* xmid,
                   const double* u, const int* frozen, double* dump, double* lam, hipStream_t s,
                   const double* PR = nullptr,   // xmid == NULL with PR: the kernel forms the midpoints (see below)
                   const int* gate = nullptr);
// metric (optional): [control_grid_parts(N)][B] partial maxima of the weighted change at the grid nodes (error points
// == nodes), for launch_fbs_advance
// batched single shooting (ocs_shooting.cpp): per-instance state of the spectral projected gradient iteration,
// every array [rows][B]
struct SpgArgs {
  int batch, nV, memory;
  double TolFun, TolX;
  const double *lb, *ub;      // [nV], or [nV][B] with bstride = B: bounds of its own per instance
  int bstride;
  double *v, *g, *d, *vt, *gt;  // [nV][B]: iterate, its gradient, direction, trial point, its gradient
  double *J, *Jt, *alpha, *lam, *gtd, *fmax;  // [B]
  double* hist;               // [memory][B] last objective values (non-monotone line search)
  int *active, *accepted, *iters;  // [B]
  int* counter;               // instances still active (Direction) / rejected by the line search (Accept)
};
// projected L-BFGS on the same state (alpha, the trial point and the flags are SPG's; hist and fmax are unused; gtd holds
// g'(vt - v) of the current trial point): per-instance ring of (s, y) pairs
struct LbfgsArgs {
  SpgArgs a;
  int pairs;
  double *S, *Y;      // [pairs][nV][B]
  double *rho, *al;   // [pairs][B]: 1 / s'y of the stored pair; first-loop coefficients, newest pair first
  int *fr;            // [nV][B] free coefficients of the current iterate
  int *head, *count, *qn;  // [B] next slot, pairs held, the direction of this iteration is a quasi-Newton one
};
// the phases of one solve: first evaluation done; stopping test + direction + first trial point; Armijo test + next trial
// point; take the step; verdict.  Init and Finish are common to both algorithms
enum class SsPhase { Init, Direction, Accept, Update, Finish };
struct ShootingArgs {
  int algorithm;      // OCS_SS_SPG (l.a alone is filled) or OCS_SS_LBFGS
  LbfgsArgs l;
  int it;             // Update: the iteration in progress (SPG's slot in hist)
  double* pgnorm;     // Finish: [B] or NULL, ||P(v - g) - v||_inf of the result
  int* converged;     // Finish: [B] or NULL, its verdict
};
int launch_shooting(SsPhase phase, const ShootingArgs& r, hipStream_t s);
// bounds per instance: Lb, Ub [nV][B] or NULL (unbounded) -> lb, ub [nV][B]; *bad (device, zeroed by the caller) counts Lb > Ub
int launch_ss_bounds(int nV, int batch, const double* Lb, const double* Ub, double* lb, double* ub, int* bad, hipStream_t s);
int control_grid_parts(int N);
// batched vectorInterpolant: V [n][nComp][B] -> out [nq][nComp][B]; method as OCS_INTERP_*; t: tables of the sample grid
int launch_interp(int method, const FbsTables& t, int nComp, int nq, const int* KQ, const double* SQ, int batch,
                  const double* V, double* out, hipStream_t s);
// 'pchip' with the query points sorted by interval (QS [n], QI [nq], SS [nq]: ocs_fbs_device.hpp k_interp_pchip_sorted)
int launch_interp_pchip_sorted(const FbsTables& t, int nComp, const int* QS, const int* QI, const double* SS, int batch,
                               const double* V, double* out, hipStream_t s);
int launch_control_grid(const ProblemDesc& p, const GridDesc& g, const FbsTables& t, int batch, const double* x, int ldx,
                        const double* xmid, const double* lam, double* u, const int* status, double* metric,
                        double relTol, double absTol, hipStream_t s, const int* gate = nullptr, double relax = 1.0);
int launch_control_pts(const ProblemDesc& p, const FbsTables& t, int nq, const int* KQ, const double* SQ,
                       const double* TUQ, int batch, const double* x, int ldx, const double* lam, double* out,
                       const int* usel, long long odelta, double* metric, int* anyvalid, double relTol,
                       double absTol, hipStream_t s, double relax = 1.0, const int* gate = nullptr);
// error-point mode on points sorted by interval (QS [n]: offsets per interval): registry problems; parts = control_pts_run_parts(N)
int control_pts_run_parts(int N);
bool control_pts_sorted_ok(const ProblemDesc& p);
int launch_control_pts_sorted(const ProblemDesc& p, const FbsTables& t, int nq, const int* QS, const double* SQ,
                              const double* TUQ, int batch, const double* x, int ldx, const double* lam, double* out,
                              double* metric, double relTol, double absTol, hipStream_t s, double relax = 1.0,
                              const int* gate = nullptr);
int launch_tu_at(const ProblemDesc& p, int nq, const double* tq, double* TUQ, hipStream_t s);
int control_pts_parts(int nq);  // rows of the partial-maximum array `metric` [parts][B] that launch_control_pts fills
int launch_fbs_init(int batch, int nsweeps, int* usel, int* status, double* maxChange, hipStream_t s);
int launch_fbs_advance(int batch, int sweep, int nparts, const double* metric, int* anyvalid, int* usel, int* status,
                       double* maxChange, int* nactive, hipStream_t s, const int* gate = nullptr);

// batched bvp_solver (ocs_bvp_kernels.hip): damped Newton on the collocated optimality system, y = [x; lam] [N+1][2 nS][B]
bool bvp_supported(const ProblemDesc& p);   // registry logistic family and user problems, nS <= 4, nC <= 2
int bvp_chunks(int N);                      // rows of the partial-norm arrays SS, MX [chunks][B]
struct BvpIterate {
  int batch;
  const double* x0;    // [nS][B]
  const double* y;     // the iterate
  const double* d;     // the Newton step (launch_bvp_norm: the residual is taken at y + alpha d)
  double alpha;
  const int* status;   // [B] 0 active, 1 converged, 2 failed: launch_bvp_assemble skips the finished instances
  const int* search;   // [B] launch_bvp_norm skips instances with search == 0
  double* AB;          // [N][2 nS (2 nS + 1)][B] step maps [A_i | b_i] (launch_bvp_assemble)
  double* SS;          // [chunks][B] partial sums of squares of the residual (launch_bvp_norm) ...
  double* MX;          //             ... and partial maxima of its magnitude
  const int* gate;     // optional device flag: the launch does nothing if *gate == 0
};
int launch_bvp_assemble(const ProblemDesc& p, const GridDesc& g, const BvpIterate& a, hipStream_t s);
int launch_bvp_norm(const ProblemDesc& p, const GridDesc& g, const BvpIterate& a, hipStream_t s);
struct BvpSweepArgs {
  int N, batch, it;
  const double* AB;
  double* PP;          // [N+1][nS (nS + 1)][B] rows of [P_i | p_i]
  const double* y;
  const double* x0;
  double* d;           // [N+1][2 nS][B]
  int* status;         // a non-finite step: 2
  int* search;         // 1 for the instances whose step the line search is to try
  int* iters;          // = it for every instance the sweep ran for
  double* alpha;       // = 0
};
int launch_bvp_sweep(int nS, const BvpSweepArgs& a, hipStream_t s);
struct BvpVerdictArgs {
  int batch, nparts;
  const double* SS;
  const double* MX;
  double tol;          // NewtonTol
  int* search;
  int* status;
  double* nrm2;        // [B] ||Phi||_2 of the iterate
  double* resinf;      // [B] ||Phi||_inf of the iterate
  double* alpha;       // [B] accepted step length of this iteration, 0: none (yet)
  int* slot;           // device counter of the instances that go on (searching / iterating); zeroed by the caller
};
int launch_bvp_accept(const BvpVerdictArgs& a, bool init, double step, const int* gate, hipStream_t s);
int launch_bvp_finish(const BvpVerdictArgs& a, int it, int max_iter, bool final, hipStream_t s);
int launch_bvp_update(int rows, int batch, const double* alpha, const double* d, double* y, hipStream_t s);
int launch_bvp_init(int batch, int* status, int* search, int* iters, double* alpha, hipStream_t s);
int launch_bvp_pack(int npts, int nS, int batch, const double* xs, int ldx, bool xs_nodes, const double* lam, double* y,
                    hipStream_t s);
int launch_bvp_costate_rows(int npts, int nS, int batch, const double* y, double* lam, hipStream_t s);
int launch_bvp_converged(int batch, const int* status, int* converged, hipStream_t s);
// the mesh side.  Residual estimate of a nodal solution y (k_bvp_rms, ocs_bvp_device.hpp): rms [N][B] and the chunk maxima
// PM [bvp_chunks(N)][B]; TCL [2N][NTC], TUL [2N][NTU]: time coefficients of the Lobatto points (launch_tcoef_at)
int launch_tcoef_at(const ProblemDesc& p, int nq, const double* tq, double* TCQ, double* TUQ, hipStream_t s);
int launch_bvp_rms(const ProblemDesc& p, const GridDesc& g, int batch, const double* TCL, const double* TUL, const double* y,
                   double* rms, double* PM, hipStream_t s);
// the Hermite interpolant of y on the grid of g at nnew points (interval idx, position theta in it): ynew [nnew][2 nS][B]
int launch_bvp_prolong(const ProblemDesc& p, const GridDesc& g, int batch, const double* y, int nnew, const int* idx,
                       const double* theta, double* ynew, hipStream_t s);

// error estimate of the sweep's pass pair by step doubling (ocs_xlam_err_kernels.hip, k_xlam_err in ocs_xlam_err_device.hpp)
struct XlamErrTables {   // device; what the estimate needs beside the integrator's and the sweep's tables
  const double* HG;      // [2N] spacings of the grid t (nodes and middles): pchip of the control samples
  const double* W1G;     // [2N+1] its interior slope weights (entries 1 .. 2N-1 used)
  const double* W2G;
  const double* SQ;      // [2N] local coordinates of the quarter points t_i + h/4, t_i + 3h/4 in their grid intervals
  const double* TCQ;     // [2N][NTC] F-side time coefficients of the quarter points (launch_tcoef_at)
};
bool xlam_err_supported(const ProblemDesc& p);   // registry logistic family and user problems, nS <= 4, nC <= 2
int xlam_err_chunks(int N);                      // rows of PM, PJ [chunks][B]
// u [2N+1][nC][B], x [N+1][ldx][B], lam [N+1][nS][B] -> the ratios rx, rl [N][B], PM (largest per chunk, NaN as +inf), PJ
// (sum of the cost row's signed estimate per chunk)
int launch_xlam_err(const ProblemDesc& p, const GridDesc& g, const FbsTables& tx, const XlamErrTables& tq, int batch,
                    const double* u, const double* x, int ldx, const double* lam, double rtol, double atol, double* rx,
                    double* rl, double* PM, double* PJ, hipStream_t s);

// what both estimates reduce their ratios [N][B] and chunk partials [nparts][B] with (ocs_kernels.hip), use [B] or NULL (all):
// rmax[i]  = max over instances in use of max(r0[i][b], r1 ? r1[i][b] : r0[i][b]), NaN -> +inf, none in use -> 0
// rinst[b] = max over chunks of PM[q][b];   sum[b] = PS[q][b] added from 0.0 in chunk order (PS, sum may be NULL together)
// Instantiated for the two forms in use: r0 alone without a sum, r0 and r1 with it (any other: -1).
int launch_interval_reduce(int N, int batch, int nparts, const double* r0, const double* r1, const double* PM,
                           const double* PS, const int* use, double* rmax, double* rinst, double* sum, hipStream_t s);

// registry queries (host)
bool functor_supported(Functor f, int nS, int nC);
int functor_ntc(Functor f, int nS);
int functor_ntu(Functor f, int nS);
int rec_stride_host(int ntc);
int rec_sc_offset_host(int ntc);
int rec_pad_host();
unsigned functor_tc_param_mask(Functor f, int nS);

}  // namespace ocs
