// ocs_handles.hpp -- private: handle structs, error plumbing and staging helpers shared by
// the C-ABI translation units (ocs_api.cpp, ocs_control.cpp, ocs_fbs.cpp, ocs_shooting.cpp, ocs_multi.cpp, ocs_jit.cpp).
// Ownership: a DevBuf frees its memory when it goes out of scope, a handle struct destroys what it owns in its destructor
// (streams and events in the body, i.e. before its member buffers go); the ocs_*_destroy entry points are `delete`.
#pragma once
#include "../../include/ocs.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <initializer_list>
#include <mutex>
#include <string>
#include <vector>

#include "ocs_internal.hpp"
#include "ocs_jit.hpp"

namespace ocs {

// ------------------------------------------------------------------------------------
// errors
// ------------------------------------------------------------------------------------
inline std::string& err_string() {
  static thread_local std::string s;
  return s;
}

inline int fail(int code, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  err_string() = buf;
  return code;
}
#define HIP_TRY(expr)                                                                       \
  do {                                                                                      \
    hipError_t e_ = (expr);                                                                 \
    if (e_ != hipSuccess) return fail(OCS_ERR_HIP, "%s: %s", #expr, hipGetErrorString(e_)); \
  } while (0)
#define LAUNCH_TRY(expr)                                                                    \
  do {                                                                                      \
    int rc_ = (expr);                                                                       \
    if (rc_ < 0) return fail(OCS_ERR_UNSUPPORTED, "%s: no kernel for this problem", #expr); \
    if (rc_ > 0) return fail(OCS_ERR_HIP, "%s: %s", #expr, hipGetErrorString((hipError_t)rc_)); \
  } while (0)
#define OCS_TRY(expr)         \
  do {                        \
    int rc_ = (expr);         \
    if (rc_ < 0) return rc_;  \
  } while (0)

inline int require_device() {
  static std::once_flag once;   // (reachable from the worker threads of ocs_multi_*)
  static int state = -1;        // 1 ok, -1 none
  std::call_once(once, [] {
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    state = (e == hipSuccess && n > 0) ? 1 : -1;
  });
  if (state < 0)
    return fail(OCS_ERR_NO_DEVICE, "no HIP device: libocs has no CPU fallback, an MI355X is required");
  return OCS_OK;
}

// ------------------------------------------------------------------------------------
// device buffers
// ------------------------------------------------------------------------------------
// Owns its memory: freed by the destructor (hipFree waits for the device, so work in flight on the buffer is finished).
// No object of this type, and no handle that has one, may have static or thread-local storage: its destructor would run at
// thread or process exit, possibly after the HIP runtime has shut down.
struct DevBuf {
  void* p = nullptr;
  size_t cap = 0;
  DevBuf() = default;
  ~DevBuf() { release(); }
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  DevBuf(DevBuf&& o) noexcept : p(o.p), cap(o.cap) { o.detach(); }
  DevBuf& operator=(DevBuf&& o) noexcept {
    if (this != &o) {
      release();
      cap = o.cap;
      p = o.detach();
    }
    return *this;
  }
  int ensure(size_t bytes) {
    if (bytes <= cap) return OCS_OK;
    if (p) (void)hipFree(p);
    p = nullptr;
    cap = 0;
    HIP_TRY(hipMalloc(&p, bytes));
    cap = bytes;
    return OCS_OK;
  }
  void release() {   // (for a buffer dropped early on purpose; cleanup is the destructor's)
    if (p) (void)hipFree(p);
    p = nullptr;
    cap = 0;
  }
  void* detach() {   // hands the memory to the caller: this object forgets it
    void* q = p;
    p = nullptr;
    cap = 0;
    return q;
  }
  double* d() const { return static_cast<double*>(p); }
};

// a host table to a buffer of its size (never an empty one); returns when the copy is done
inline int upload(DevBuf& d, const void* src, size_t bytes) {
  OCS_TRY(d.ensure(bytes ? bytes : 8));
  if (bytes) HIP_TRY(hipMemcpy(d.p, src, bytes, hipMemcpyHostToDevice));
  return OCS_OK;
}

// Host staging: a MATLAB-shaped host array (`per` doubles per trajectory, trajectory-major) to / from a batch-minor device
// array, through the caller's ONE stage buffer on the caller's stream.  stage_out waits for the stream: the host array is
// complete and the stage buffer free again on return.  stage_in does not wait; a caller whose stage buffer may still be in
// use waits for its stream first.
inline int stage_in(DevBuf& stage, DevBuf& dst, const double* host, int per, int batch, hipStream_t s) {
  const size_t bytes = sizeof(double) * (size_t)per * batch;
  OCS_TRY(stage.ensure(bytes));
  OCS_TRY(dst.ensure(bytes));
  HIP_TRY(hipMemcpyAsync(stage.p, host, bytes, hipMemcpyHostToDevice, s));
  LAUNCH_TRY(launch_to_batch_minor(stage.d(), dst.d(), per, batch, s));
  return OCS_OK;
}
inline int stage_out(DevBuf& stage, const double* src, double* host, int per, int batch, hipStream_t s) {
  const size_t bytes = sizeof(double) * (size_t)per * batch;
  OCS_TRY(stage.ensure(bytes));
  LAUNCH_TRY(launch_to_traj_major(src, stage.d(), per, batch, s));
  HIP_TRY(hipMemcpyAsync(host, stage.p, bytes, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  return OCS_OK;
}
// The caller's batch flags (`use` of the estimates) to the device on s: *dev is the device copy, NULL for use == NULL.
inline int stage_flags(DevBuf& dst, const int* use, int batch, hipStream_t s, const int** dev) {
  *dev = nullptr;
  if (!use) return OCS_OK;
  OCS_TRY(dst.ensure(sizeof(int) * (size_t)batch));
  HIP_TRY(hipMemcpyAsync(dst.p, use, sizeof(int) * (size_t)batch, hipMemcpyHostToDevice, s));
  *dev = (const int*)dst.p;
  return OCS_OK;
}
// Small result vectors (n doubles each, no layout to change) back to the host on s; waits for the stream like stage_out.
struct Fetch {
  double* host;
  const DevBuf& dev;
  size_t n;
};
inline int fetch(std::initializer_list<Fetch> vectors, hipStream_t s) {
  for (const Fetch& v : vectors) HIP_TRY(hipMemcpyAsync(v.host, v.dev.p, sizeof(double) * v.n, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  return OCS_OK;
}

// ------------------------------------------------------------------------------------
// handles
// ------------------------------------------------------------------------------------
// Globally unique: the integrator tables are cached under (problem pointer, version), and problems are created and
// re-parametrised concurrently from the worker threads of ocs_multi_*.
inline unsigned long long next_version() {
  static std::atomic<unsigned long long> c{1};
  return c.fetch_add(1, std::memory_order_relaxed);
}

// The HIP current device is per host thread.  Every handle records the device it was created on; entry points that
// switch devices (ocs_multi_*) restore the caller's on every return path through this guard.
struct DeviceGuard {
  int prev = -1;
  DeviceGuard() {
    if (hipGetDevice(&prev) != hipSuccess) prev = -1;
  }
  ~DeviceGuard() {
    if (prev >= 0) (void)hipSetDevice(prev);
  }
  DeviceGuard(const DeviceGuard&) = delete;
  DeviceGuard& operator=(const DeviceGuard&) = delete;
};

inline int current_device_or(int dflt) {
  int d = dflt;
  return hipGetDevice(&d) == hipSuccess ? d : dflt;
}

}  // namespace ocs

struct ocs_problem_s {
  using DevBuf = ocs::DevBuf;
  using Functor = ocs::Functor;
  int id = 0, nS = 0, nC = 0;
  int device = -1;              // HIP device current when the handle was created (-1: created without a device)
  Functor functor = Functor::Logistic;
  ocs::UserModule* user = nullptr;  // hipRTC module of a user-supplied problem
  std::vector<double> par;      // functor order
  std::vector<int> user2func;   // user parameter index -> functor parameter index
  std::vector<double> bounds;   // nC x 2
  DevBuf d_ps, d_pb, d_lb, d_ub;
  unsigned pmask = 0;
  int pb_batch = 0;             // batch of the per-trajectory parameters (d_pb under pmask, or d_w)
  // OCS_PROBLEM_LQ only: per-trajectory cost weights [nS + nC][pb_batch] (ProblemDesc::W); never together with pmask
  DevBuf d_w;
  bool has_w = false;
  // control bounds of its own per trajectory (ocs_problem_set_batch_bounds): device [2 nC][bb_batch], batch-minor, rows
  // 0 .. nC-1 the lower bounds, then the upper ones; bb_batch == 0: not set, the shared d_lb / d_ub are read.  `bb`: the same
  // values on the host (the LQ problem hands them to its shadow, ocs_fbs.cpp sweep_problem)
  DevBuf d_bb;
  std::vector<double> bb;
  int bb_batch = 0;
  unsigned long long version = 0;  // bumps whenever device-visible parameters change
  bool uploaded = false;
  // OCS_PROBLEM_LQ only: the same problem as generated device source (hipRTC), built on first use by the
  // forward-backward-sweep entry points, whose kernels are instantiated per functor (ocs_fbs.cpp: lq_shadow)
  ocs_problem_s* shadow = nullptr;
  unsigned long long shadow_version = 0;
  ~ocs_problem_s() {
    delete shadow;
    if (user) ocs::jit_free(user);
  }
};

struct ocs_fbs_state;  // forward-backward-sweep workspace (ocs_fbs.cpp)
void ocs_fbs_state_free(ocs_fbs_state* s);

struct ocs_bvp_state;  // bvp_solver workspace (ocs_bvp.cpp)
void ocs_bvp_state_free(ocs_bvp_state* s);

struct ocs_integrator_s {
  using DevBuf = ocs::DevBuf;
  ocs_fbs_state* fbs = nullptr;
  ocs_bvp_state* bvp = nullptr;
  ocs::LqWorkspace* lqws = nullptr;   // time-parallel LQ passes: chunk matrices of the bound problem + scratch
  int device = -1;   // HIP device current when the handle was created
  int rec_stride = 8;  // doubles per step record of the bound problem
  bool uniform = false;  // all steps of the grid have the same size
  hipEvent_t tc_event = nullptr;   // recorded behind the kernels that build TC / TU / REC / RECS ...
  hipStream_t tc_stream = nullptr; // ... on this stream: a call on another stream waits for it first
  std::vector<int> traj_status;    // per-trajectory flags of the last host compute_states / nlp_objective
  int mapping = 0;  // ocs::Mapping requested through ocs_integrator_set_mapping (0 = automatic)
  int layout = 0;   // ocs::Layout of the per-step device arrays of the _dev compute calls (ocs_integrator_set_layout)
  int kind = 0;  // 0 RK4Integrator, 1 RK4InfiniteIntegrator (then `leg2` and `ustar` are set)
  ocs_integrator_s* leg2 = nullptr;   // integrator2 of RK4InfiniteIntegrator.m:13-14
  std::vector<double> ustar;          // uStar (nC)
  DevBuf d_ustar, d_lam2;             // device uStar [nC]; lam2(:,1) [nAug][B]
  // a uStar of its own per trajectory (ocs_rk4inf_set_batch_ustar): [nC][ustar_batch], handle-owned; ustar_batch == 0: not
  // set, the tail leg runs under the shared d_ustar.  ustar_version bumps at every set and clear: what is cached per uStar
  // (d_utail below, the chunk responses of the LQ tail) is keyed on it, the buffer's address says nothing
  DevBuf d_ustar_b;
  int ustar_batch = 0;
  unsigned long long ustar_version = 0;
  // tail leg of RK4InfiniteIntegrator on the wave-specialised kernels (small batches): the constant control as samples
  // [2N+1][nC][B], the tail's lam [N+1][nAug][B] (its first column is the main leg's lamT), the tail's objective [B]
  DevBuf d_utail, d_lamtail, d_J2;
  int utail_batch = 0;
  unsigned long long utail_version = 0;   // ustar_version of the main leg the samples were filled under
  bool tail_wave = false;
  int N = 0;
  std::vector<double> tspan, t, h;
  DevBuf d_HT, d_T, d_TC, d_TU, d_REC, d_RECS, d_split;
  bool grid_uploaded = false;
  unsigned long long tc_version = 0;  // version of the problem TC was built for
  const ocs_problem_s* tc_prob = nullptr;
  bool want_ck = true;          // keep checkpoints of J-only forward passes (adjoint may follow)
  double* want_lam0 = nullptr;  // if set, the next adjoint pass also writes lam(:,1) here ([nAug][B])
  // state of the last forward pass (the xK contract of RK4Integrator.m:10,32)
  const double* ck = nullptr;
  int ck_batch = 0;
  int ck_layout = 0;            // the layout the checkpoints were written in
  const ocs_problem_s* ck_prob = nullptr;
  // staging for the host entry points
  hipStream_t stream = nullptr;
  DevBuf d_x0, d_u, d_x, d_J, d_lam, d_dJdu, d_lamT, d_stage, d_ck;
  ~ocs_integrator_s() {
    if (tc_event) (void)hipEventDestroy(tc_event);
    delete leg2;
    if (fbs) ocs_fbs_state_free(fbs);
    if (bvp) ocs_bvp_state_free(bvp);
    if (lqws) ocs::lq_workspace_free(lqws);
    if (stream) (void)hipStreamDestroy(stream);
  }
};

struct ocs_control_s;
const double* ocs_control_device_J(const ocs_control_s* c);   // ocs_control.cpp
int ocs_control_device_id(const ocs_control_s* c);             // device owning the handle's memory, -1 before the first use

namespace ocs {

// Entry points that read or write per-step arrays in the batch-minor layout only: refused on a handle set to the tiled layout
inline int refuse_tiled(const ocs_integrator_s* g, const char* what) {
  if (g && g->layout != LAYOUT_BATCH_MINOR)
    return fail(OCS_ERR_UNSUPPORTED, "%s: the integrator is set to the tiled layout, which only ocs_compute_states_dev / "
                "ocs_compute_adjoints_dev read and write (ocs_integrator_set_layout)", what);
  return OCS_OK;
}

inline int upload_problem(ocs_problem_s* p) {
  if (p->uploaded) return OCS_OK;
  OCS_TRY(require_device());
  if (p->device < 0) p->device = current_device_or(-1);   // the device that owns the handle's memory from here on
  OCS_TRY(p->d_ps.ensure(sizeof(double) * p->par.size()));
  HIP_TRY(hipMemcpy(p->d_ps.p, p->par.data(), sizeof(double) * p->par.size(), hipMemcpyHostToDevice));
  OCS_TRY(p->d_lb.ensure(sizeof(double) * p->nC));
  OCS_TRY(p->d_ub.ensure(sizeof(double) * p->nC));
  HIP_TRY(hipMemcpy(p->d_lb.p, p->bounds.data(), sizeof(double) * p->nC, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(p->d_ub.p, p->bounds.data() + p->nC, sizeof(double) * p->nC, hipMemcpyHostToDevice));
  p->uploaded = true;
  return OCS_OK;
}

// per-trajectory control bounds from host arrays that are batch-minor already: lbm, ubm [nC][batch] (validated by the caller)
inline int set_batch_bounds_minor(ocs_problem_s* p, int batch, const double* lbm, const double* ubm) {
  OCS_TRY(upload_problem(p));
  const size_t half = (size_t)p->nC * batch;
  std::vector<double> bb(2 * half);
  memcpy(bb.data(), lbm, sizeof(double) * half);
  memcpy(bb.data() + half, ubm, sizeof(double) * half);
  OCS_TRY(p->d_bb.ensure(sizeof(double) * bb.size()));
  HIP_TRY(hipMemcpy(p->d_bb.p, bb.data(), sizeof(double) * bb.size(), hipMemcpyHostToDevice));
  p->bb.swap(bb);
  p->bb_batch = batch;
  p->version = next_version();
  return OCS_OK;
}

inline ProblemDesc describe(const ocs_problem_s* p) {
  ProblemDesc d;
  d.functor = p->functor;
  d.nS = p->nS;
  d.nC = p->nC;
  d.npar = (int)p->par.size();
  d.ps = p->d_ps.d();
  d.pb = p->pmask ? p->d_pb.d() : nullptr;
  d.pmask = p->pmask;
  d.W = p->has_w ? p->d_w.d() : nullptr;
  d.Wbatch = p->has_w ? p->pb_batch : 0;
  d.bb = p->bb_batch ? p->d_bb.d() : nullptr;
  d.bstride = p->bb_batch;
  d.lb = d.bb ? d.bb : p->d_lb.d();
  d.ub = d.bb ? d.bb + (size_t)p->nC * p->bb_batch : p->d_ub.d();
  d.user = p->user;
  d.version = p->version;
  return d;
}

// The time coefficients of a problem at n extra times of a grid (launch_tcoef_at): TC [n][NTC], TU [n][NTU].  The times are a
// property of the grid and go up once per handle; the tables follow (problem, version) like the integrator's own (bind_problem).
struct TcoefAt {
  DevBuf T, TC, TU;
  const ocs_problem_s* prob = nullptr;
  unsigned long long version = 0;
  // times: n host values, read only while T is empty; the tables are rebuilt on s
  int ensure(const ocs_problem_s* p, int n, const double* times, hipStream_t s) {
    if (!T.p) {
      OCS_TRY(upload(T, times, sizeof(double) * (size_t)n));
      prob = nullptr;
    }
    if (prob != p || version != p->version) {
      OCS_TRY(TC.ensure(sizeof(double) * (size_t)n * std::max(1, functor_ntc(p->functor, p->nS))));
      OCS_TRY(TU.ensure(sizeof(double) * (size_t)n * std::max(1, functor_ntu(p->functor, p->nS))));
      LAUNCH_TRY(launch_tcoef_at(describe(p), n, T.d(), TC.d(), TU.d(), s));
      prob = p;
      version = p->version;
    }
    return OCS_OK;
  }
};

inline int upload_grid(ocs_integrator_s* g) {
  if (g->grid_uploaded) return OCS_OK;
  OCS_TRY(require_device());
  if (g->device < 0) g->device = current_device_or(-1);
  const int N = g->N;
  std::vector<double> HT((size_t)4 * N);
  for (int i = 0; i < N; ++i) {  // the divisions the reference performs per step, done once in IEEE fp64
    HT[4 * i + 0] = g->h[i];
    HT[4 * i + 1] = g->h[i] / 2;  // RK4Integrator.m:40
    HT[4 * i + 2] = g->h[i] / 6;  // :50, :73
    HT[4 * i + 3] = g->h[i] / 3;  // :77
  }
  g->uniform = true;
  for (int i = 1; i < N; ++i) g->uniform = g->uniform && g->h[i] == g->h[0];
  OCS_TRY(g->d_HT.ensure(sizeof(double) * HT.size()));
  HIP_TRY(hipMemcpy(g->d_HT.p, HT.data(), sizeof(double) * HT.size(), hipMemcpyHostToDevice));
  OCS_TRY(g->d_T.ensure(sizeof(double) * g->t.size()));
  HIP_TRY(hipMemcpy(g->d_T.p, g->t.data(), sizeof(double) * g->t.size(), hipMemcpyHostToDevice));
  if (!g->stream) HIP_TRY(hipStreamCreate(&g->stream));
  if (g->kind == 1) {
    OCS_TRY(g->d_ustar.ensure(sizeof(double) * g->ustar.size()));
    HIP_TRY(hipMemcpy(g->d_ustar.p, g->ustar.data(), sizeof(double) * g->ustar.size(), hipMemcpyHostToDevice));
  }
  g->grid_uploaded = true;
  return OCS_OK;
}

inline GridDesc describe(const ocs_integrator_s* g) {
  GridDesc d;
  d.N = g->N;
  d.HT = g->d_HT.d();
  d.T = g->d_T.d();
  d.TC = g->d_TC.d();
  d.TU = g->d_TU.d();
  d.REC = g->d_REC.d() ? g->d_REC.d() + (size_t)rec_pad_host() * g->rec_stride : nullptr;
  d.RECS = g->d_RECS.d() ? g->d_RECS.d() + scan_recs_front() : nullptr;
  d.uniform = g->uniform;
  d.lqws = const_cast<LqWorkspace**>(&g->lqws);
  return d;
}

// pieces of the sweep's workspace that bvp_solver's post-processing shares (ocs_fbs.cpp): the pchip node tables of the grid,
// and interval index / local coordinate / time of the points linspace(T0, TF, nq)
int fbs_ensure_tables(ocs_integrator_s* g);
FbsTables fbs_tables(const ocs_integrator_s* g);
int fbs_build_points(ocs_integrator_s* g, int nq, DevBuf& K, DevBuf& S, DevBuf& T);

// make sure the time-coefficient table of (g, p) is current; enqueued on `s`
inline int bind_problem(ocs_integrator_s* g, ocs_problem_s* p, int batch, hipStream_t s) {
  OCS_TRY(upload_problem(p));
  OCS_TRY(upload_grid(g));
  if ((p->pmask || p->has_w) && p->pb_batch != batch)
    return fail(OCS_ERR_SHAPE, "problem has per-trajectory parameters for batch %d, call has batch %d",
                p->pb_batch, batch);
  if (p->bb_batch && p->bb_batch != batch)
    return fail(OCS_ERR_SHAPE, "problem has per-trajectory control bounds for batch %d, call has batch %d",
                p->bb_batch, batch);
  if (g->tc_prob != p || g->tc_version != p->version) {
    const int ntc = functor_ntc(p->functor, p->nS);
    const int ntu = functor_ntu(p->functor, p->nS);
    OCS_TRY(g->d_TC.ensure(sizeof(double) * (size_t)(2 * g->N + 1) * ntc));
    // (+128: the fold kernels stream this table in 1 KiB pieces, the last of which reaches past the horizon)
    OCS_TRY(g->d_TU.ensure(sizeof(double) * ((size_t)(2 * g->N + 1) * (ntu > 0 ? ntu : 1) + 128)));
    g->rec_stride = rec_stride_host(ntc);
    OCS_TRY(g->d_REC.ensure(sizeof(double) * (size_t)(g->N + 2 * rec_pad_host()) * g->rec_stride));
    LAUNCH_TRY(launch_tcoef(describe(p), describe(g), s));
    if (scan_problem_ok(describe(p)) || vector_problem_ok(describe(p))) {
      OCS_TRY(g->d_RECS.ensure(sizeof(double) * scan_recs_doubles(g->N)));
      LAUNCH_TRY(launch_build_recs(g->N, g->rec_stride, rec_sc_offset_host(ntc), describe(g).REC, g->d_RECS.d(), s));
    }
    g->tc_prob = p;
    g->tc_version = p->version;
    // the tables are valid for every later call on this stream; a call on another stream must wait for them
    if (!g->tc_event) HIP_TRY(hipEventCreateWithFlags(&g->tc_event, hipEventDisableTiming));
    HIP_TRY(hipEventRecord(g->tc_event, s));
    g->tc_stream = s;
  } else if (g->tc_event && s != g->tc_stream) {
    HIP_TRY(hipStreamWaitEvent(s, g->tc_event, 0));
  }
  return OCS_OK;
}


}  // namespace ocs
