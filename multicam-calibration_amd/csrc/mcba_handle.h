// mcba_handle.h -- what the translation units of the C ABI (mcba_api.hip, mcba_lm_api.hip, mcba_prefilter_api.hip, mcba_calib_api.hip,
// mcba_geom_api.hip, mcba_comm_api.hip, mcba_cov_api.hip, mcba_tricov_api.hip, mcba_kpba_api.hip, mcba_flat.hip, mcba_detect.hip) share: the handle, the error plumbing, the buffer pool, profiling scopes and the launch helpers of the solver chain.
// Private to the library: not installed, not part of include/mcba.h.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <rccl/rccl.h>
#include <string>
#include <vector>

#include "../../include/mcba.h"
#include "mcba_kernels.h"
#include "mcba_math.h"

namespace mcba_internal {

extern thread_local std::string g_err;  // what mcba_last_error() returns (mcba_api.hip)

enum KernelId { K_TRANSPOSE = 0, K_GRAM, K_COST, K_SYRK, K_REDUCE, K_BACKSUB, K_SUM_TRIAL, K_JACOBIAN, K_DECIDE, K_SOLVE,
                K_SP_FACTOR, K_SP_PAIRS, K_SP_SOLVE_PRE, K_SP_POTRF, K_SP_TRSM, K_SP_UPDATE, K_SP_FINISH, K_COUNT };
// (sparse-Schur handle: k_sp_factor = k_sp_factor + k_sp_y, k_sp_pairs = k_sp_pairs + k_sp_assemble, k_sp_solve_pre = k_sp_solve_pre + k_sp_load)
constexpr const char* kKernelNames = "k_transpose_obs\nk_gram\nk_cost\nk_syrk\nk_reduce_system\nk_backsub\nk_sum_trial\nk_jacobian\nk_decide\nk_solve_cam"
                                     "\nk_sp_factor\nk_sp_pairs\nk_sp_solve_pre\nk_sp_potrf\nk_sp_trsm\nk_sp_update\nk_sp_finish";
constexpr int kRing = 16;  // host-mapped LM state slots (device-resident loop): the host may run at most kRing - 1 ticks ahead

struct EvRec { int kid; hipEvent_t a, b; };
struct DevBuf { void** slot; size_t bytes; };  // a pooled device buffer of a handle: where its pointer lives, its size

}  // namespace mcba_internal

struct mcba_handle {
  int C = 0, F = 0, N = 0, Fpad = 0, nfb = 0, n = 0;
  int device = 0;
  hipStream_t stream = nullptr;
  int loss = MCBA_LOSS_SOFT_L1;
  double f_scale = 1.0;
  bool have_obs = false, have_lin = false, have_red = false, have_jac = false;
  // device buffers
  double *obs_t = nullptr, *obs_raw = nullptr, *obj = nullptr, *x[2] = {nullptr, nullptr};
  double *rec2[2] = {nullptr, nullptr}, *gpart2[2] = {nullptr, nullptr}, *fbuf = nullptr, *fpart = nullptr;
  int lin = 0;          // which of the two linearisation buffers holds the accepted point
  bool have_spec = false;  // the other one holds a speculative linearisation of the last trial point
  double *spart = nullptr, *cpart = nullptr, *bpart = nullptr;
  double *red_own = nullptr, *red = nullptr;
  double *jac = nullptr, *res = nullptr;
  double *err = nullptr, *dmean = nullptr, *dfull = nullptr, *repro = nullptr, *trans = nullptr, *und = nullptr;  // pre-filter / diagnostics (lazy)
  mcba::SelState* sel = nullptr;   // the radix select's states (two per camera: per-camera medians)
  unsigned char* fmask = nullptr;
  // mcba_prefilter (the selection on the device): scratch state, per-frame status / worst mean error, the packed result and its pinned landing place
  unsigned char *pf_state = nullptr, *pf_status = nullptr, *pf_packed = nullptr, *pf_host = nullptr;
  double* pf_worst = nullptr;
  size_t pf_host_bytes = 0;
  double* core_arena = nullptr;            // mcba_create: x[0] | x[1] | obj
  unsigned char* solver_arena = nullptr;   // ensure_solver: the one allocation the solver buffers below are pieces of
  int* sub_frames = nullptr;   // mcba_create_subset: the frame indices on the device (kept with the handle: no synchronisation to free them)
  double* cov_work = nullptr;  // mcba_covariance: factor, inverse factor and Sigma_cc (ld x ld each), scales, sums, flags, the frame blocks [F][36] (lazy)
  double* outbuf = nullptr;    // mcba_lm_result: [x | gradient] packed for one device-to-host copy
  // calibrate() on the device (mcba_calib_*): intrinsics [C][9], every view's board pose [C][6][Fpad] (NaN = none), per-view flags, and
  // scratch that grows with the call (view lists, outputs, pairwise transforms, select states, world-frame poses)
  double *cal_intr = nullptr, *cal_poses_t = nullptr, *cal_out = nullptr, *cal_rel = nullptr, *cal_world = nullptr;
  unsigned char *cal_valid = nullptr, *cal_nit = nullptr;
  mcba::SelState* cal_sel = nullptr;
  int* cal_views = nullptr;
  size_t cal_out_cap = 0, cal_rel_cap = 0, cal_sel_cap = 0, cal_views_cap = 0;
  bool have_cal_poses = false;
  double* obj_host = nullptr;  // board points as uploaded (diagnostics normalise them on the host)
  int planar = 0;              // every board point has z = 0 exactly (the fused k_gram then runs its planar instance)
  int *tile_i = nullptr, *tile_j = nullptr;
  int NT = 0, NP = 0, G = 0, sq = 0, sr = 0, FS = 0, ppw = 4, nfblocks = 0, nbblocks = 0, nch = 1;  // k_syrk: G workgroups, sq stages of FS frames each, the first sr one more
  mcba::GramPlan gram;       // which launches linearise this shard (mcba_gram_plan.h; derive_geometry)
  double* gchunk = nullptr;  // gram.chunk_doubles() of raw sums: the point-chunk tail's scratch
  double curv_floor = 1.0;  // curvature weight of the NEXT linearisations: max(Triggs, curv_floor rho') -- 1 = IRLS (mcba_set_curvature_floor; csrc/mcba_math.h)
  int cw = 12;         // camera block width: 12, or 6 = the intrinsics of every camera are held fixed (mcba_set_camera_block; BASELINE configs[1]): n = cw C
  size_t nx = 0, nsys = 0;
  double* pinned = nullptr;  // nsys + 8 doubles, + 12C for dc
  ncclComm_t comm = nullptr;  // direct RCCL communicator (optional)
  // device-resident LM loop (mcba_lm_auto_*)
  double *dcbuf = nullptr, *swork = nullptr;
  double* dscale = nullptr;   // numeric x_scale (least_squares): D = 1 / x_scale^2 in the layout of x; have_xscale says whether it is in use
  bool have_xscale = false;   // the XS kernel instances run: a numeric x_scale and / or frozen coordinates are in `dscale`
  std::vector<double> xs_host;             // numeric x_scale as D = 1 / x_scale^2 (nx entries; empty = 'jac')
  std::vector<unsigned char> frozen_host;  // coordinates taken out of the system (mcba_set_frozen; empty = none)
  double *blo = nullptr, *bhi = nullptr;   // box constraints (mcba_set_bounds), in the layout of x
  bool have_bounds = false;
  double* loss_tab = nullptr;   // loss == LOSS_TABLE (mcba_set_loss_table): [3][C][N][Fpad] (u, v) pairs, laid out as obs_t
  int fuse_max_polls = 200000;
  bool strict_sync = true;    // the fused back-substitution's readers ACQUIRE the release word with an agent-scope fence: the HIP memory model's form, the default since round 6 (MCBA_STRICT_SYNC=0 / mcba_set_strict_sync(h, 0): relaxed loads + gfx950's in-order issue, ~1.3 us per iteration faster)
  unsigned char* fixed = nullptr;
  bool have_fixed = false, auto_ready = false;
  bool speculate = true;       // frame-sharded ticks: one collective (speculative Schur reduction) instead of two
  double* ring = nullptr;      // kRing x MCBA_LMS doubles, host-coherent pinned memory the GPU writes directly
  double* ring_dev = nullptr;  // the same memory as the device sees it
  int npad = 0, solve_lds = 0;
  // k_solve_backsub (single-GPU ticks, factor in LDS): the solve's launch also runs the back-substitution of the NEXT trial step;
  // trial_ready = the last tick did so, the next one must not back-substitute again.  The flag word sits behind the camera step.
  bool fuse_backsub = false, trial_ready = false;
  unsigned long long last_solve_seq = 0;  // sequence number of the last mcba_lm_auto_solve / tick (what a timed-out back-substitution of that launch stamps)
  unsigned long long waited_seq = 0;      // the last tick whose posted state the host has read (mcba_lm_auto_wait): equal to last_solve_seq = nothing posts into the ring any more
  unsigned long long solve_launches = 0;  // k_solve_cam launches so far (SolveArgs.stage_tag)
  int ncu = 256, lds_optin = 160 * 1024;  // compute units and the LDS a workgroup may ask for (hipGetDeviceProperties at create; MI355X: 256 / 160 KiB)
  bool spec_copy_ready = false;  // the last k_reduce_system was a speculative one: the pre-decision state copy is in place
  double ftol = 1e-8, xtol = 1e-8, gtol = 1e-8, lam_min = 1e-12, lam_max = 1e12;
  double dec_floor = 0.0;      // floor of Nielsen's damping factor on accepted steps (0 = the classical 1/3): mcba_lm_set_decrease_floor
  // profiling
  bool prof = false;
  unsigned prof_mask = ~0u;
  int prof_stride = 1;             // bracket every prof_stride-th launch of a selected kernel
  bool prof_exact = false;         // k_gram: events on the dispatch itself (mcba_profile_exact)
  unsigned prof_count[32] = {};
  std::vector<mcba_internal::EvRec> evs;
  std::vector<hipEvent_t> pool;
  std::vector<mcba_internal::DevBuf> bufs;  // every pooled device buffer (mcba_destroy parks them)
  std::vector<double> hist;        // mcba_lm_run: the state every retired tick posted (MCBA_LMS doubles each; row 0 = the solve of the start point)
  bool have_solver = false;        // solver buffers are allocated on first use (ensure_solver): a pre-filter handle never needs them
  size_t ring_bytes = 0, pinned_bytes = 0;
  unsigned ring_flags = 0;
  // sparse-Schur handle (mcba_create_sparse; mcba_sparse_api.hip): the visibility index of the uploaded observations (built on first use
  // after an upload), Y_cf of every seen (camera, frame), the pair-chunk sums, and the blocked solve's matrix, damping and control words
  bool sparse = false, sp_ready = false;
  int sp_nent = 0, sp_npairs = 0, sp_nchunks = 0;
  int *sp_index = nullptr, *sp_frame_off = nullptr, *sp_ent_cam = nullptr, *sp_ent_frame = nullptr, *sp_items = nullptr, *sp_chunks = nullptr, *sp_pair_map = nullptr, *sp_pair_chunks = nullptr;
  int* sp_ctl = nullptr;
  double *sp_Y = nullptr, *sp_part = nullptr, *sp_A = nullptr, *sp_damp = nullptr, *sp_y = nullptr;
  size_t sp_index_ints = 0, sp_Y_count = 0, sp_part_count = 0;
};

// a device array that outlives its handle (mcba_residuals_detach, mcba_lm_result)
struct mcba_buffer { double* dev; size_t count; int device; hipStream_t stream; double* base; size_t base_count; };  // dev / count: what a download delivers; base / base_count: the pooled allocation it lies in

namespace mcba_internal {

#define HIPCHK(expr)                                                                                     \
  do {                                                                                                   \
    hipError_t e_ = (expr);                                                                              \
    if (e_ != hipSuccess) {                                                                              \
      mcba_internal::g_err = std::string(#expr) + ": " + hipGetErrorString(e_);                          \
      return MCBA_ERR_HIP;                                                                               \
    }                                                                                                    \
  } while (0)

inline int fail(int code, const char* msg) { g_err = msg; return code; }

inline int check_launch() {
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) { g_err = std::string("kernel launch: ") + hipGetErrorString(e); return MCBA_ERR_HIP; }
  return MCBA_OK;
}

inline hipEvent_t get_event(mcba_handle* h) {
  if (!h->pool.empty()) { hipEvent_t e = h->pool.back(); h->pool.pop_back(); return e; }
  hipEvent_t e;
  (void)hipEventCreate(&e);
  return e;
}

struct Scope {  // brackets one launch with events when profiling
  mcba_handle* h; int kid; hipEvent_t a{}, b{};
  bool on, exact;
  Scope(mcba_handle* h_, int k) : h(h_), kid(k), on(h_->prof && ((h_->prof_mask >> k) & 1u) && (h_->prof_count[k]++ % (unsigned)h_->prof_stride) == 0), exact(false) {
    if (!on) return;
    a = get_event(h); b = get_event(h);
    // k_gram with exact timing asked for (mcba_profile_exact): the events ride on the kernel's dispatch (its own begin / end timestamps,
    // what rocprofv3 reports); everything else: event records around the launch (which read ~2.5 us more than the kernel takes)
    exact = h->prof_exact && k == K_GRAM;
    if (exact) mcba::gram_time_next_launch(a, b);
    else (void)hipEventRecord(a, h->stream);
  }
  ~Scope() {
    if (!on) return;
    if (exact && mcba::gram_time_pending()) {   // another launch variant than the fused kernel ran: no exact timing for it
      mcba::gram_time_next_launch(nullptr, nullptr);
      h->pool.push_back(a); h->pool.push_back(b);
      return;
    }
    if (!exact) (void)hipEventRecord(b, h->stream);
    h->evs.push_back({kid, a, b});
  }
};

// ---- buffer pool (mcba_api.hip): freed device / pinned host buffers are parked per (device, size) and handed out again
hipError_t pool_malloc(void** p, size_t bytes, int device, hipStream_t stream = nullptr, bool any_stream = false);
void pool_free(void* p, size_t bytes, int device, hipStream_t stream = nullptr, bool busy = false);
hipError_t pool_host_malloc(void** p, size_t bytes, unsigned flags);
void pool_host_free(void* p, size_t bytes, unsigned flags);
int poison_byte();  // MCBA_POISON (tests): the byte buffers handed out without a zero fill are filled with, 0 = none

// zero-filled device buffer from the pool, registered with the handle (mcba_destroy parks it again).  The fill is
// enqueued on the handle's stream (no host synchronisation); `zero = false` for buffers a kernel overwrites completely
// before anything reads them (observation layouts, Jacobian blocks).
template <class T>
int dalloc(mcba_handle* h, T** p, size_t count, bool zero = true) {
  const size_t bytes = std::max<size_t>(count, 1) * sizeof(T);
  HIPCHK(pool_malloc(reinterpret_cast<void**>(p), bytes, h->device, h->stream));
  h->bufs.push_back({reinterpret_cast<void**>(p), bytes});
  if (zero) HIPCHK(hipMemsetAsync(*p, 0, bytes, h->stream));
  else if (int pz = poison_byte()) HIPCHK(hipMemsetAsync(*p, pz, bytes, h->stream));  // (tests: whatever relies on a fill that is no longer made shows)
  return MCBA_OK;
}

// RCCL entry points resolved at run time from the copy already loaded in the process (torch's librccl.so):
// loaded on first use by mcba_comm_api.hip, which alone defines the table
struct RcclApi {
  bool ok = false;
  ncclResult_t (*GetUniqueId)(ncclUniqueId*) = nullptr;
  ncclResult_t (*CommInitRank)(ncclComm_t*, int, ncclUniqueId, int) = nullptr;
  ncclResult_t (*AllReduce)(const void*, void*, size_t, ncclDataType_t, ncclRedOp_t, ncclComm_t, hipStream_t) = nullptr;
  ncclResult_t (*CommDestroy)(ncclComm_t) = nullptr;
  ncclResult_t (*CommCount)(const ncclComm_t, int*) = nullptr;
  const char* (*GetErrorString)(ncclResult_t) = nullptr;
};
extern RcclApi g_rccl;

// the device of a stateless entry point: checked, then made current.  who != nullptr prefixes the out-of-range message
inline int stateless_device(int device, const char* who = nullptr) {
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return fail(MCBA_ERR_NODEVICE, "no HIP device visible");
  if (device < 0 || device >= ndev) { g_err = who ? std::string(who) + ": device ordinal out of range" : "device ordinal out of range"; return MCBA_ERR_ARG; }
  HIPCHK(hipSetDevice(device));
  return MCBA_OK;
}

// the LDS a workgroup of this device may ask for (dynamic, after opting in): at most 160 KiB; 64 KiB where the device does not say
inline int lds_optin_of(int device) {
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, device) == hipSuccess && prop.sharedMemPerBlockOptin > 0) return (int)std::min<size_t>(prop.sharedMemPerBlockOptin, 160 * 1024);
  return 64 * 1024;
}

// the device buffers and events of one stateless call (null stream), released on every path out.  upload / scratch / put / download return
// an MCBA_* code with g_err set; counts are elements of T, the type of both the host and the device side; start / stop time the call's kernels
struct StatelessCall {
  std::vector<void*> bufs;
  hipEvent_t e0 = nullptr, e1 = nullptr, e2 = nullptr;
  ~StatelessCall() {
    for (void* b : bufs) (void)hipFree(b);
    for (hipEvent_t e : {e0, e1, e2})
      if (e) (void)hipEventDestroy(e);
  }
  template <class T>
  int alloc(T** p, size_t count, bool poison) {
    const size_t bytes = count * sizeof(T) > 0 ? count * sizeof(T) : 16;
    void* v = nullptr;
    HIPCHK(hipMalloc(&v, bytes));
    bufs.push_back(v);
    *p = static_cast<T*>(v);
    if (int pz = poison ? poison_byte() : 0) HIPCHK(hipMemset(v, pz, bytes));
    return MCBA_OK;
  }
  // a buffer that a kernel writes before anything reads it, outputs included: filled with the MCBA_POISON byte when that mode is on (tests:
  // whatever reads an element nobody wrote shows).  Inputs go through upload(); only a slab that holds inputs and scratch in one allocation,
  // or a staging buffer refilled per chunk, is made here and has its input slices filled by put() or the caller's own copies
  template <class T>
  int scratch(T** p, size_t count) { return alloc(p, count, true); }
  template <class T>
  int put(T* dst, const T* host, size_t count) {
    HIPCHK(hipMemcpy(dst, host, count * sizeof(T), hipMemcpyHostToDevice));
    return MCBA_OK;
  }
  // a buffer holding `count` elements of a host array
  template <class T>
  int upload(T** p, const T* host, size_t count) {
    if (int rc = alloc(p, count, false)) return rc;
    return put(*p, host, count);
  }
  template <class T>
  int download(T* host, const T* src, size_t count) {
    HIPCHK(hipMemcpy(host, src, count * sizeof(T), hipMemcpyDeviceToHost));
    return MCBA_OK;
  }
  // ---- timed brackets of a call with many of them (e0 and e1 created by the call): open() before the launches; close() checks them, waits for
  // them and adds their time to sum.  A bracket whose last part is timed on its own has mark() between the parts -- or a launcher that records
  // e1 there itself -- and closes with close_split(), which adds the time after the mark to part as well; e2, its end, is made by the first
  // open(true), ahead of the bracket, so that nothing but the launches lies between its events
  int open(bool split = false) {
    if (split && !e2) HIPCHK(hipEventCreate(&e2));
    HIPCHK(hipEventRecord(e0, nullptr));
    return MCBA_OK;
  }
  int mark() { HIPCHK(hipEventRecord(e1, nullptr)); return MCBA_OK; }
  int close(double& sum) {
    if (int rc = mark_launches(e1)) return rc;
    return add_ms(e0, e1, sum);
  }
  int close_split(double& sum, double& part) {
    if (int rc = mark_launches(e2)) return rc;
    if (int rc = add_ms(e0, e2, sum)) return rc;
    return add_ms(e1, e2, part);
  }
  hipError_t start() {
    hipError_t e = hipEventCreate(&e0);
    if (e == hipSuccess) e = hipEventCreate(&e1);
    if (e == hipSuccess) e = hipEventRecord(e0, nullptr);
    return e;
  }
  hipError_t stop(double* kernel_ms) {
    hipError_t e = hipEventRecord(e1, nullptr);
    if (e == hipSuccess) e = hipEventSynchronize(e1);
    if (e == hipSuccess && kernel_ms) {
      float ms = 0.f;
      e = hipEventElapsedTime(&ms, e0, e1);
      *kernel_ms = ms;
    }
    return e;
  }

 private:
  int mark_launches(hipEvent_t end) {
    if (int rc = check_launch()) return rc;
    HIPCHK(hipEventRecord(end, nullptr));
    HIPCHK(hipEventSynchronize(end));
    return MCBA_OK;
  }
  int add_ms(hipEvent_t from, hipEvent_t to, double& sum) {
    float ms = 0.f;
    HIPCHK(hipEventElapsedTime(&ms, from, to));
    sum += ms;
    return MCBA_OK;
  }
};

// The N events that separate the N + 1 stages of a stateless call between its start() and its stop(), released on every path out:
// create() before start(), mark() after each stage but the last, fill() after stop()
template <int N>
struct StageEvents {
  hipEvent_t ev[N] = {};
  int marked = 0;
  ~StageEvents() { for (hipEvent_t e : ev) if (e) (void)hipEventDestroy(e); }
  hipError_t create() {
    hipError_t e = hipSuccess;
    for (int i = 0; i < N && e == hipSuccess; ++i) e = hipEventCreate(&ev[i]);
    return e;
  }
  hipError_t mark() { return hipEventRecord(ev[marked++], nullptr); }
  // kernel_ms[0] = total, kernel_ms[1 .. N + 1] = the stages, from e0 over the marks to e1; nothing is written unless every span was read
  hipError_t fill(const StatelessCall& call, double total, double* kernel_ms) const {
    double ms[N + 2] = {total};
    for (int i = 0; i <= N; ++i) {
      float span = 0.f;
      hipError_t e = hipEventElapsedTime(&span, i == 0 ? call.e0 : ev[i - 1], i == N ? call.e1 : ev[i]);
      if (e != hipSuccess) return e;
      ms[1 + i] = span;
    }
    for (int i = 0; i < N + 2; ++i) kernel_ms[i] = ms[i];
    return hipSuccess;
  }
};

// The per-detection weights of a stateless keypoint call, count = C P of them, as the kernels read them: the plane of
// sqrt(w), 0 for a zero or NaN weight (the detection is unseen), uploaded once beside the detections.  weights NULL: *d_sw = nullptr, the
// unweighted kernels.  check_weights (before the device is touched, with the other arguments): MCBA_ERR_ARG for a negative or infinite weight.
inline int check_weights(const char* who, const double* weights, size_t count) {
  if (!weights) return MCBA_OK;
  for (size_t i = 0; i < count; ++i)
    if (weights[i] < 0.0 || weights[i] > 1.7976931348623157e308) {
      g_err = std::string(who) + ": weights must be finite and not negative (0 or NaN = the detection is unseen)";
      return MCBA_ERR_ARG;
    }
  return MCBA_OK;
}
inline int upload_sqrt_weights(StatelessCall& call, const double* weights, size_t count, double** d_sw) {
  *d_sw = nullptr;
  if (!weights) return MCBA_OK;
  std::vector<double> sq(count);
  for (size_t i = 0; i < count; ++i) sq[i] = weights[i] > 0.0 ? sqrt(weights[i]) : 0.0;
  return call.upload(d_sw, sq.data(), count);
}

// the camera table of the keypoint kernels (mcba_keypoint_math.h: KpCam, one per camera of cam12 and dist5 or NULL) in device memory (mcba_geom_api.hip)
int upload_kp_cams(StatelessCall& call, int n_cameras, const double* cam12, const double* dist5, mcba::KpCam** d_cams);

// The argument checks that the calls on detections of tracks and skeletons (mcba_traj_refine_api.hip, mcba_skeltraj_api.hip,
// mcba_skeleton_api.hip) make alike.  Each is a run of checks that stands at the same place in every caller's order, so the message of the
// first thing wrong is the same as if the caller had written them out; what differs between the callers is checked by them, through bad()
struct DetectionChecks {
  const char* who;
  int bad(const char* what) const { g_err = std::string(who) + ": " + what; return MCBA_ERR_ARG; }
  static bool finite(double v) { return v - v == 0.0; }
  // k_max, c_max: SK_MAX_K and kKpMaxCams, the 64 of the messages
  int frames_keypoints(size_t T, int K, int k_max) const {
    if (T < 1 || T > ((size_t)1 << 31)) return bad("1 .. 2^31 frames required");
    if (K < 1 || K > k_max) return bad("1 .. 64 keypoints required");
    return MCBA_OK;
  }
  // arrays: every input array that may not be NULL is there
  int cameras_arrays(int C, int c_max, bool arrays) const {
    if (C < 1 || C > c_max) return bad("1 .. 64 cameras required");
    if (!arrays) return bad("non-NULL arrays (but dist5 and weights) required");
    return MCBA_OK;
  }
  int convex_loss(int loss) const {
    if (loss < mcba::LOSS_LINEAR || loss > mcba::LOSS_HUBER) return bad("loss must be linear, soft_l1 or huber (0 .. 2)");
    return MCBA_OK;
  }
  int loop(double f_scale, int max_iterations, double xtol) const {
    if (!(f_scale > 0.0) || !finite(f_scale)) return bad("f_scale must be positive and finite");
    if (max_iterations < 1) return bad("max_iterations >= 1");
    if (!(xtol >= 0.0)) return bad("xtol >= 0");
    return MCBA_OK;
  }
  int pixel_std(const double* std, int C) const {
    for (int c = 0; c < C; ++c)
      if (!(std[c] > 0.0) || !finite(std[c]) || !finite(1.0 / std[c])) return bad("pixel_std must be positive and finite (and its inverse too)");
    return MCBA_OK;
  }
  // rc: what skel_plan (mcba_skeleton_math.h) returned for the forest
  int forest(int rc) const {
    switch (rc) {
      case 0: return MCBA_OK;
      case 2: return bad("a parent outside -1 .. K - 1, or a keypoint that is its own parent");
      case 3: return bad("the parents form a cycle: the skeleton must be a forest");
      default: return bad("bone_length and bone_std must be positive and finite for every keypoint with a parent");
    }
  }
};

// info8 and *kernel_ms (or NULL) of a trajectory or skeleton call, slot by slot
inline void fill_info8(double* info8, double* kernel_ms, double levels, double width, double s2, double s3, double ms, double s5, double device_bytes, double s7) {
  const double v[8] = {levels, width, s2, s3, ms, s5, device_bytes, s7};
  for (int i = 0; i < 8; ++i) info8[i] = v[i];
  if (kernel_ms) *kernel_ms = ms;
}

inline int slot_ok(const mcba_handle* h, int slot) { return h && (slot == 0 || slot == 1); }

int create_impl(mcba_handle** out, int C, int F, int N, int device, bool sparse);   // mcba_create / mcba_create_sparse (mcba_api.hip)
// solver buffers on first use (mcba_api.hip)
int ensure_solver(mcba_handle* h);
#define NEED_SOLVER(h) do { int rc_ = mcba_internal::ensure_solver(h); if (rc_) return rc_; } while (0)
int upload_impl(mcba_handle* h, const double* uvs, const double* objpoints, bool sync);

// ---- selectors of the solver kernels' operands
inline mcba::Sel host_sel(int idx, double lam = 0.0) { return mcba::Sel{nullptr, idx, lam, 0, 0.0}; }
inline mcba::Sel dev_sel(const mcba_handle* h, int flip) { return mcba::Sel{h->red + h->nsys + 8, flip, 0.0, 0, 0.0}; }  // LM state lives behind the trial scalars
inline mcba::Sel spec_sel(const mcba_handle* h) { return mcba::Sel{h->red + h->nsys + 8, 0, h->lam_min, 1, h->dec_floor}; }
// the state AFTER the decision k_syrk took itself (single-GPU ticks): a second buffer behind the first
inline double* post_state(const mcba_handle* h) { return h->red + h->nsys + 8 + MCBA_LMS; }
inline mcba::Sel post_sel(const mcba_handle* h) { return mcba::Sel{post_state(h), 0, 0.0, 0, 0.0}; }
inline double* timeout_word(const mcba_handle* h) { return h->dcbuf + h->n + 1; }  // behind the camera step and the release word
inline mcba::SyrkFuse no_fuse() { mcba::SyrkFuse z{}; return z; }

// ---- the solver chain's launches (mcba_api.hip): the operands that come from the handle filled in once; each one is bracketed
// for profiling and checked.  la / lb: the linearisation buffers (rec2 / gpart2) in positions 0 / 1; xa / xb: the parameter slots.
int gram_launch(mcba_handle* h, mcba::Sel sel, const double* xa, const double* xb, int la, int lb);   // k_gram, with the handle's curvature floor
int trial_sum(mcba_handle* h, mcba::Sel sel, int la, int lb, const mcba::DecideArgs& da);            // k_sum_trial over k_gram's per-block sums
int backsub_launch(mcba_handle* h, mcba::Sel sel, int la, int lb, int xa, int xb, const double* delta_cam);  // delta_cam NULL: the camera step on the device (dcbuf)
int syrk_launch(mcba_handle* h, mcba::Sel sel, const mcba::SyrkFuse& fz);
int reduce_launch(mcba_handle* h, mcba::Sel sel, int rank_slot, bool spec);   // spec: + the trial scalars and the pre-decision state copy

// ---- the sparse-Schur handle (mcba_sparse_api.hip).  syrk_launch / reduce_launch / backsub_launch and the device-resident solve route here
// when h->sparse: frame factors + co-visible pairs + assembly, the tail of k_reduce_system, the blocked solve.
int sparse_build(mcba_handle* h, mcba::Sel sel);      // frame factors, Y, pair chunks, S0 and rhs into h->red
int sparse_solve(mcba_handle* h, const mcba::SolveArgs& a);
void sparse_forget(mcba_handle* h);                   // mcba_trim released the buffers

}  // namespace mcba_internal
