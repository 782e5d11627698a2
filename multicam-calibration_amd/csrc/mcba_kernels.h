// mcba_kernels.h -- launch wrappers of mcba_kernels.hip and the device buffer record sizes.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>

#include <type_traits>

#define MCBA_REC 100  // per (frame, camera) record: W 72 | V 21 | g_f 6 | pad
#define MCBA_GP 92    // k_gram per-wavefront sums, stored [camera][k][frame block]: k = U 78 | g_c 12 | cost | pairs with data
#define MCBA_FB 40    // per frame: L 21 (diagonal slots hold 1 / L_ii) | z 6 | g_f 6 | D_f 6 | pad

#include "mcba_gram_plan.h"
#include "mcba_lm_state.h"
#include "mcba_math.h"

namespace mcba {
// ---- run-time values to template arguments (host side).  A launcher computes its grid and LDS size, then makes one nested call whose
// innermost generic lambda names the kernel: with_loss(loss, [&](auto L) { ... k_x<decltype(L)::value> ... return 0; }).
// with_int: f(std::integral_constant<int, V>{}) for the V of the list equal to v; 1, without calling f, when there is none
template <int... Vs, class F>
int with_int(int v, F&& f) {
  int rc = 1;
  (void)((v == Vs && ((rc = f(std::integral_constant<int, Vs>{})), true)) || ...);
  return rc;
}
// for_each_int: f(std::integral_constant<int, V>{}) for every V of the list, in order -- with_int's twin for the launchers whose kernels
// need an opt-in to their LDS: the launcher and the opt-in name ONE list (an IntList), so no instance the launcher can reach is left out
template <int... Vs>
struct IntList {};
template <int... Vs, class F>
int with_int(IntList<Vs...>, int v, F&& f) { return with_int<Vs...>(v, f); }
template <int... Vs, class F>
void for_each_int(IntList<Vs...>, F&& f) { (f(std::integral_constant<int, Vs>{}), ...); }
// one kernel per loss: loss_weights takes it as a template argument.  1 for anything but the five losses
using LossList = IntList<LOSS_LINEAR, LOSS_SOFT_L1, LOSS_HUBER, LOSS_CAUCHY, LOSS_ARCTAN>;
template <class F>
int with_loss(int loss, F&& f) { return with_int(LossList{}, loss, f); }
template <class F>
int with_bool(bool b, F&& f) { return b ? f(std::true_type{}) : f(std::false_type{}); }
template <class F>
void for_each_bool(F&& f) { f(std::false_type{}); f(std::true_type{}); }
// sw != nullptr: the weighted instantiation
template <class F>
int with_weights(const double* sw, F&& f) { return with_bool(sw != nullptr, f); }
// the launch as an expression (0), for the innermost lambda of such a call
template <class... P, class... A>
int launch(void (*kernel)(P...), dim3 grid, dim3 block, size_t lds, hipStream_t st, const A&... args) {
  hipLaunchKernelGGL(kernel, grid, block, lds, st, args...);
  return 0;
}
// opt in to more than 64 KiB of dynamic LDS where the launch asks for it, then launch (256 threads)
template <class... P, class... A>
int launch_with_lds(void (*kernel)(P...), dim3 grid, size_t lds, hipStream_t st, A... args) {
  if (lds > 64 * 1024 && hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess) return 1;
  return launch(kernel, grid, dim3(256), lds, st, args...);
}

// Double-buffered operands (parameter slots, linearisation records) and the damping are chosen either from host
// values (lms == nullptr: idx / lam as given) or from the device-resident LM state (idx is XORed with state[3],
// lam = state[1]) -- so a whole LM iteration can be enqueued without knowing whether its trial step is accepted.
// Camera step handed to k_backsub through the kernel-argument segment (no H2D copy): 12 x C doubles, C <= 40.
struct CamStep {
  double v[480];
};

struct Sel {
  const double* lms;
  int idx;
  double lam;   // host value of the damping (lms == nullptr); lambda_min when spec != 0
  int spec;     // speculative Schur reduction of the trial linearisation (see sel_spec in mcba_kernels.hip)
  double dec;   // spec != 0: floor of Nielsen's factor the prediction assumes (mcba_lm.h: lm_spec_lambda)
  double cfl = 1.0;  // k_gram only: curvature floor of this linearisation (mcba_math.h: lm_weight) -- 1 = the IRLS weight rho', 0.1 = Triggs with a floor
};
// k_syrk's fused decision prologue (single-GPU ticks of the device-resident loop; see k_syrk in mcba_kernels.hip)
struct SyrkFuse {
  int decide;          // != 0: every workgroup sums the trial scalars and takes the accept / reject decision itself
  const double* cp0;   // per-wavefront cost sums of the two linearisation buffers (gpart + 90 nfb) ...
  const double* cp1;
  int cinner;          // ... element idx of `ncp` lives at (idx / cinner) * couter + (idx % cinner) * cstride
  int cstride;         // 4: k_gram leaves the cost of a whole workgroup (four frame blocks) in its first wavefront's slot, zeros in the others
  int cdense;          // ... up to idx % cinner == cdense; from there on every slot holds a value (k_gram_psplit ran on those frame blocks): slot = cdense cstride + (idx % cinner - cdense)
  size_t couter;
  int ncp;
  const double* bpart; // k_backsub's per-block sums (3 per block)
  int nbp;
  double* trial_out;   // 4 trial scalars for the host (cost, pred_f, |d_f|^2, |x_f|^2)
  double* lms_post;    // the state AFTER the decision (workgroup 0 writes it; later kernels of the tick read it)
  DecideArgs da;       // lam_min, lam_max, ftol, xtol
  const double* timeout_word;  // device word a back-substitution workgroup of k_solve_backsub stamps with its tick's number when its poll ran out
  double seq_prev;             // the previous tick's number: found in the word, this tick's trial point is stale -> rebuild only
};
// k_solve_cam (mcba_solve.hip): reduced camera system factorised and solved by one workgroup
struct SolveArgs {
  const double* red;         // S0 (n x n) | rhs | diag U | g_c | 16 scalars
  const double* lms_in;      // device LM state as the tick's decision left it (== lms unless k_syrk took the decision)
  double* lms;               // device LM state the NEXT tick starts from (written back here)
  double* work;              // npad x npad scratch (used when the factor does not fit LDS)
  double* dc;                // n doubles: the camera step
  const double* x0;          // parameter slots (camera block first)
  const double* x1;
  const unsigned char* fixed;  // n flags (1 = parameter held fixed) or nullptr
  const double* dscale;      // numeric x_scale: D_c = dscale[0 .. n) instead of diag(U), or nullptr
  double* host_state;        // host-mapped ring slot of MCBA_LMS doubles, or nullptr
  double* flag;              // k_solve_backsub: device word released with `seq` when the camera step is in place (else nullptr)
  const double* timeout_word;  // see SyrkFuse (one-collective ticks: the decision taken here checks it); may be nullptr
  double seq;
  double gtol, lam_max;
  int n, npad, use_lds;
  int cw;                    // camera block width: 12, or 6 = the intrinsics of every camera are held fixed (row i of the system is parameter 6 + i % 6 of camera i / 6)
  // decide != 0 (frame-sharded ticks with one collective): the all-reduced trial scalars sit behind the system and the
  // accept/reject decision is taken HERE, then checked against the prediction the speculative Schur reduction was built on
  int decide;
  double lam_min, ftol, xtol;
  double dec_floor;          // floor of Nielsen's damping factor (0 = 1/3): used by the decision taken here and to check the prediction
  double stage_tag;          // > 9 cameras: this launch's number in the handle's life (never repeats: the stager workgroups release it, workgroup 0 waits for it)
};
void launch_transpose_obs(hipStream_t st, const double* raw, double* obs_t, int C, int F, int N, int Fpad);
// executes a plan (mcba_gram_plan.h) over C cameras x Fpad / 64 frame blocks.  planar: every board point has z = 0 exactly (with f_scale = 1 the FAST
// instances run); chunk: plan.chunk_doubles() of scratch; ltab (loss == LOSS_TABLE): three planes [C][N][Fpad] of (u, v) pairs -- 0.5 f_scale^2 rho,
// rho', J_scale^2 (mcba_set_loss_table)
void launch_gram(hipStream_t st, int loss, double f_scale, const double* obs_t, const double* obj, Sel s, const double* x0, const double* x1, double* rec0, double* rec1, double* gp0, double* gp1, int C, int N, int Fpad,
                 const GramPlan& plan, int planar = 0, double* chunk = nullptr, const double* ltab = nullptr);
void gram_time_next_launch(hipEvent_t start, hipEvent_t stop);  // measurement: the next fused k_gram launch of this thread carries the events on its dispatch (the kernel's own begin / end)
bool gram_time_pending();                                       // ... still pending after the launch: another variant ran, bracket it the usual way
int gram_psplit_set_lds_limit();             // raises the dynamic-LDS limit of the point split's instances to kGramPsplitLdsMax (0 = ok)
void launch_cost(hipStream_t st, int loss, double f_scale, const double* obs_t, const double* obj, const double* x, double* cpart, double* res, int C, int F, int N, int Fpad, int nch,
                 double fill = 0.0);   // what the residual vector holds where a scalar is missing: 0, or NaN (then the vector carries its own row mask)
size_t syrk_lds_bytes(int C, int FS, int cw = 12);
void launch_syrk(hipStream_t st, Sel s, const SyrkFuse& fz, const double* rec0, const double* rec1, double* fbuf, double* fpart, const int* tile_i, const int* tile_j, double* spart, int C, int F, int Fpad, int NT, int NP, int G, int sq, int sr, int FS, int ppw,
                 const double* dscale = nullptr,   // dscale: D = 1 / x_scale^2 in the layout of x (numeric x_scale), nullptr: D = diag(J^T J)
                 int cw = 12);                     // camera block width (6: intrinsics held fixed; the 4-tile variant only)
int syrk_items_per_thread();
// bpart != nullptr (speculative frame-sharded ticks): the trial scalars are summed here as well (red + nsys .. + 8) and the LM
// state is copied to state_copy (MCBA_LMS doubles)
void launch_reduce_system(hipStream_t st, Sel s, const double* gp0, const double* gp1, const double* spart, const double* fpart, const int* tile_i, const int* tile_j, double* red, int C, int nfb, int G, int NT, int NP, int nfblocks, int rank_slot,
                          const double* bpart = nullptr, int nbp = 0, double* state_copy = nullptr, int cw = 12,
                          const double* timeout_word = nullptr, double seq_prev = 0.0);  // (speculative ticks: trial scalar 5 = the previous fused back-substitution of this shard gave up)
void launch_backsub(hipStream_t st, Sel s, const double* rec0, const double* rec1, const double* fbuf, const CamStep& dc, double* x0, double* x1, double* bpart, int C, int F, int Fpad, int cw = 12);
void launch_backsub_dev(hipStream_t st, Sel s, const double* rec0, const double* rec1, const double* fbuf, const double* dc_dev, double* x0, double* x1, double* bpart, int C, int F, int Fpad, int cw = 12);
size_t solve_lds_bytes(int npad, int use_lds);
int solve_fits_lds(int npad, int lds_limit);
int solve_set_lds_limit(int npad, int use_lds);
void launch_solve_cam(hipStream_t st, const SolveArgs& a);
// solve + the back-substitution of the next trial step in one launch (a.use_lds variants, a.flag set); early_state = the LM state
// the tick's decision left (final as far as the slot bit goes), or -- spec != 0, the solve decides -- a copy of the state before it
int solve_backsub_set_lds_limit(int npad, int cw = 12);
void launch_solve_backsub(hipStream_t st, const SolveArgs& a, Sel sl, const double* rec0, const double* rec1, const double* fbuf, double* x0, double* x1, double* bpart, int C, int F, int Fpad,
                          const double* early_state, int max_polls, int spec, double* timeout_dev, double* timeout_host,   // (a.cw selects the camera block width)
                          int strict = 0);  // != 0: the waiting workgroups acquire the release word with an agent-scope fence (mcba_backsub.h: release_word_acquired)
void launch_sum_trial(hipStream_t st, Sel s, const double* cp0, const double* cp1, int cstride, int cinner, size_t couter, int ncp, const double* bpart, int nbp, double* out, DecideArgs da);
void launch_decide(hipStream_t st, const double* trial8, DecideArgs da);
void launch_lm_init(hipStream_t st, const double* red_scal, double* lms, double lam0, int sel, double cfl, double cfl_switch, double* clear8 = nullptr);  // mcba_lm_run: the start state, on the device
void launch_pack_result(hipStream_t st, const double* x, const double* gc, const double* fbuf, const unsigned char* fixed, double* out, int C, int F, int cw);  // mcba_lm_result
void launch_jacobian(hipStream_t st, int loss, double f_scale, const double* obs_raw, const double* obj, const double* x, double* jac, double* res, int C, int F, int N, int Fpad, int robust);
int syrk_set_lds_limit(size_t bytes);
// the sparse-Schur handle (mcba_sparse.hip): visibility, frame factors + Y_cf, co-visible pair chunks + assembly of S0 / rhs, the blocked reduced solve
void launch_sp_seen(hipStream_t st, const double* obs_raw, unsigned char* seen, int C, int F, int N);
void launch_sp_factor(hipStream_t st, Sel s, const double* rec0, const double* rec1, double* fbuf, double* fpart, const int* frame_off, const int* ent_cam, const int* ent_frame, int nent,
                      double* Y, const double* dscale, int C, int F, int Fpad, int cw);
void launch_sp_pairs(hipStream_t st, Sel s, const double* Y, const double* fbuf, const int* items, const int* chunks, int nchunks, double* part, const double* gp0, const double* gp1,
                     const int* pair_map, const int* pair_chunks, double* red, int C, int nfb, int cw);
int sp_npad(int n);                // rows of the blocked factorisation: n + 1 rounded up to its block
// bracket(ctx, stage, begin): profiling hook around each stage (0 prologue + load, 1 diagonal blocks, 2 panels, 3 trailing updates, 4 backward sweep + state)
void launch_sp_solve(hipStream_t st, const SolveArgs& a, int* ctl, double* damp, double* A, double* y, void (*bracket)(void*, int, int), void* ctx);   // y: npad doubles of scratch
// pre-filter, frame subsets, undistortion, reprojection diagnostics (mcba_diag.hip)
void launch_frame_err(hipStream_t st, const double* obs_t, const double* obj, const double* x, double* err, double* mean_cf, double* full_cf, int C, int F, int N, int Fpad,
                      void* prefilter_state = nullptr);   // non-NULL: the launch also zeroes the selection's state (launch_prefilter_select(..., state_cleared = true) follows)
// exact order statistics by radix select (mcba_diag.hip): one state per wanted rank, eight passes of one byte over the bit patterns
struct SelState {
  unsigned long long prefix;   // the leading 8 x pass bits of the selected value's key
  unsigned long long rank;     // the wanted rank among the group's non-NaN values (set at pass 0), then inside the prefix's bin
  unsigned long long count;    // non-NaN values of the group
  unsigned long long value;    // bit pattern of the selected double (after the last pass)
  unsigned int hist[256];      // the pass' histogram (cleared by the pick)
};
constexpr int kSelMaxRanks = 8;   // states per group
MCBA_HD double sel_value(const SelState& s) { return __builtin_bit_cast(double, s.value); }
// np.median from the states of the two middle ranks: the mean of the two middle values; NaN for a group without values
MCBA_HD double sel_median(const SelState& lo, const SelState& hi) {
  const double m = 0.5 * (sel_value(lo) + sel_value(hi));
  return lo.count ? m : __builtin_nan("");
}
// `groups` equal slices of v (per_group doubles each; frame = index % Fpad for fmask, which may be nullptr), NaNs skipped.  Group g owns
// the states sel[g * nranks .. (g + 1) * nranks) (nranks <= kSelMaxRanks); state j of a group selects rank ranks[j] -- ranks == nullptr:
// medians, two states per group for the lower and the upper middle rank.  After the call every state's count and value are valid.
void launch_select(hipStream_t st, const double* v, const unsigned char* fmask, size_t per_group, int groups, int Fpad, SelState* sel,
                   int skey,   // != 0: values of either sign (compared through an order-preserving key); 0: values >= +0 (the pre-filter's errors)
                   const unsigned long long* ranks = nullptr, int nranks = 0);
int launch_select_hist(hipStream_t st, const double* v, const unsigned char* fmask, size_t per_group, int Fpad, SelState* sel, unsigned long long prefix, int pass, unsigned int* hist256);
// the pre-filter's selection on the device (mcba_prefilter): see mcba_diag.hip
size_t prefilter_state_bytes();
void launch_prefilter_select(hipStream_t st, const double* err, const double* mean_cf, const double* full_cf, unsigned char* fmask, unsigned char* status, double* worst, void* state,
                             unsigned char* packed, int C, int F, int N, int Fpad, double threshold, bool state_cleared = false);
void launch_prefilter_status(hipStream_t st, unsigned char* status, const double* worst, void* state, unsigned char* packed, int F, double threshold, int from_state);
void launch_gather_params(hipStream_t st, const double* x_src, const int* frames, double* x_dst, int C, int Fdst);
void launch_clip(hipStream_t st, double* x, const double* lo, const double* hi, size_t n);  // x <- min(max(x, lo), hi): the trial point of a bounded step
bool launch_store_small(hipStream_t st, double* dst, const double* src_host, size_t n);  // <= 480 doubles through the kernel-argument segment (no blocking copy); false: too many
double measure_fp64_issue_rate(int ncu);  // TFLOP/s of independent v_fma_f64 at one wavefront per SIMD on `ncu` compute units (measurement aid)
void launch_gather_frames(hipStream_t st, const double* src_raw, const int* frames, double* dst_raw, int C, int Fsrc, int Fdst, int N,
                          const int* only_cam = nullptr);   // non-NULL: destination frame j keeps the detection of camera only_cam[j] alone (NaN for the others)
void launch_seen_bits(hipStream_t st, const double* obs_raw, size_t count, unsigned long long* words);  // words: ceil(count / 64) of them
void launch_undistort(hipStream_t st, const double* uv, double* out, size_t n, const double* K4, const double* dist5, int iters);
void launch_reproj_diag(hipStream_t st, const double* obs_t, const double* obj, const double* x, const double* dist5, const double* bn, double* und, double* repro, double* trans, double* err, int C, int F, int N,
                        int Fpad, int iters, int lm_iters);
// calibrate()'s per-view work and pose graph (mcba_pnp.hip).  mode 0: homographies of the listed views (out: nviews x 9); mode 1: board poses --
// views != nullptr: of the listed (camera, frame) views (out: nviews x 6), else of every (camera, frame) (out (C,F,6) and / or poses_t [C][6][Fpad])
void launch_view_complete(hipStream_t st, const double* obs_t, unsigned char* out, int C, int F, int N, int Fpad);
void launch_pnp(hipStream_t st, int mode, const double* obs_t, const double* obj, const double* intr9, const int* views, int nviews, const double* bn3, int C, int F, int N, int Fpad, int und_iters, int lm_iters,
                double* out, double* poses_t, unsigned char* valid, unsigned char* nit);
// poses addressed as p[c * sc + f * sf + k * sk]; rel [n_edges][6][Fpad]; world [C][6][Fpad] scratch; out (F, 6)
void launch_zhang(hipStream_t st, const double* H, const unsigned char* ok, const int* views, int nviews, const double* sizes, int C, double* intr9, unsigned char* closed);
void launch_pose_pairs(hipStream_t st, const double* poses, size_t sc, size_t sf, size_t sk, const int* edges, int n_edges, int F, int Fpad, double* rel);
void launch_pose_chain(hipStream_t st, const SelState* sel, const int* edges, int n_edges, int root, int C, double* ext, double* transforms, double* counts);   // sel: the medians of launch_select
void launch_pose_consensus(hipStream_t st, const double* poses, size_t sc, size_t sf, size_t sk, const double* ext, int C, int F, int Fpad, double* world, double* out);
// triangulation (mcba_triangulate.hip): up to 8 cameras; P = K [R | t] row-major 3x4, K = (fx, fy, cx, cy), dist = (k1 k2 p1 p2 k3)
struct TriCams {
  double P[8][12];
  double K[8][4];
  double dist[8][5];
};
// single-camera calibration with the 5-coefficient model (mcba_calib.hip): per view the 15 x 15 Gauss-Newton block (upper triangle, 120), the gradient (15), the cost
void launch_calib_views(hipStream_t st, const double* uvs, const double* obj, const double* intr9, const double* poses, int V, int N, double* out);
int launch_triangulate(hipStream_t st, int C, const double* uvs, const TriCams& cams, double* out, size_t npts, int iters);
// 9 .. 64 cameras: cams_dev = C x {P[12], K[4], dist[5]} doubles in device memory; one wavefront per point
int launch_triangulate_wave(hipStream_t st, int C, const double* uvs, const void* cams_dev, double* out, size_t npts, int iters);
// keypoint projection, reprojection errors and per-point refinement (mcba_keypoints.hip).  cams: C <= kKpMaxCams (64) entries of the camera
// table (KpCam, mcba_keypoint_math.h) in device memory -- callers with more cameras launch per group.  Non-zero: arguments out of range.
struct KpCam;
struct TcCam;   // (mcba_tricov_math.h: a KpCam and the nine doubles behind it)
// mode 0: k1, k2 model, 1: five coefficients -- out (C, P, 2); mode 2: the rigid transform of cams[0] -- out (P, 3)
int launch_project(hipStream_t st, int mode, const double* pts, size_t npts, const KpCam* cams, int C, double* out);
// uvs (C, P, 2); err rows (C, npad) doubles, NaN where unseen and in the padding p >= npts
int launch_keypoint_errors(hipStream_t st, const double* pts, const double* uvs, size_t npts, size_t npad, const KpCam* cams, int C, double* err);
// How the kernels that form a residual read one point's detections: element p of the (C, P) double2 planes and -- WEIGHTED (SURVEY.md section
// 8f-13) -- of the (C, P) plane sw of sqrt(weight), a detection counting only where sw > 0.  The observation functor of the math headers:
// three arguments without weights, four with them (mcba_keypoint_math.h: kp_observe).
template <bool WEIGHTED>
struct KpDetections;
template <>
struct KpDetections<false> {
  const double2* det;
  size_t npts;
  __device__ KpDetections(const double2* uvs, const double*, size_t npts_, size_t p) : det(uvs + p), npts(npts_) {}
  __host__ __device__ void operator()(int c, double& ou, double& ov) const {
    const double2 o = det[(size_t)c * npts];
    ou = o.x; ov = o.y;
  }
};
template <>
struct KpDetections<true> {
  const double2* det;
  const double* sq;
  size_t npts;
  __device__ KpDetections(const double2* uvs, const double* sw, size_t npts_, size_t p) : det(uvs + p), sq(sw + p), npts(npts_) {}
  __host__ __device__ void operator()(int c, double& ou, double& ov, double& s) const {
    const double2 o = det[(size_t)c * npts];
    ou = o.x; ov = o.y;
    s = sq[(size_t)c * npts];
  }
};
// The camera table into LDS, once per workgroup: the 21 doubles of every KpCam, from a KpCam table or from the KpCam part of a TcCam table
// (mcba_tricov_math.h: 30 doubles per entry).  Every thread of the workgroup calls this (one barrier).
template <int SRC_STRIDE>
__device__ __forceinline__ void stage_cam_doubles(KpCam* s_cam, const double* __restrict__ src, int C) {
  double* dst = reinterpret_cast<double*>(s_cam);
  for (int i = threadIdx.x; i < 21 * C; i += blockDim.x) dst[i] = SRC_STRIDE == 21 ? src[i] : src[SRC_STRIDE * (i / 21) + i % 21];
  __syncthreads();
}
__device__ __forceinline__ void stage_cams(KpCam* s_cam, const KpCam* __restrict__ cams, int C) { stage_cam_doubles<21>(s_cam, reinterpret_cast<const double*>(cams), C); }
__device__ __forceinline__ void stage_cams(KpCam* s_cam, const TcCam* __restrict__ cams, int C) { stage_cam_doubles<30>(s_cam, reinterpret_cast<const double*>(cams), C); }
// sw, here and below: nullptr, or the (C, P) plane of sqrt(weight) in device memory (0 = the detection is unseen) -- the weighted instantiations
// start / out (P, 3), info (P, 4) = (cost, cost at the start, iterations, status) or nullptr; loss: enum Loss, LOSS_LINEAR .. LOSS_ARCTAN
int launch_tri_refine(hipStream_t st, int loss, const double* uvs, const double* start, size_t npts, const KpCam* cams, int C, double f_scale, int max_iterations, double* out, double* info,
                      const double* sw = nullptr);
// consensus triangulation (mcba_consensus.hip): 2 <= C <= kKpMaxCams.  out (P, 3), mask (P) inlier words, info (P, 8) = (inliers, pair i, pair j,
// hypothesis cost, refit cost, refit cost at the start, iterations, status) or nullptr; hyp (P, 2): scratch between the search and the refit of
// the two-launch forms (may be nullptr for CONSENSUS_LANE).  form: CONSENSUS_AUTO picks by camera count.
enum ConsensusForm { CONSENSUS_AUTO = -1, CONSENSUS_LANE = 0, CONSENSUS_WAVE = 1, CONSENSUS_LANE_SEARCH = 2 };
int launch_consensus(hipStream_t st, int form, int loss, const double* uvs, size_t npts, const KpCam* cams, int C, double threshold, int min_views, int und_iters, double f_scale,
                     int max_iterations, double* out, unsigned long long* mask, double* hyp, double* info);
// hypothesis scoring (mcba_hyp_score.h): the one launch shape of the two RANSAC pipelines below, and the finish kernel they share
constexpr int kHypThreads = 256, kHypPPT = 4, kHypPoints = kHypThreads * kHypPPT;   // k_hyp_score: points per lane and per workgroup
constexpr int kHypChunk = 64;                                                        // hypotheses that one workgroup of k_hyp_score holds in LDS
inline size_t hyp_score_blocks(size_t n) { return (n + kHypPoints - 1) / kHypPoints; }     // workgroups of k_hyp_score per camera
inline size_t hyp_point_blocks(size_t n) { return (n + kHypThreads - 1) / kHypThreads; }   // workgroups of a lane = point kernel per camera
// part_c, part_n (C, nblk, H) -> cost (C, H; +inf for a void hypothesis: status != 1), count (C, H)
void launch_hyp_finish(hipStream_t st, const double* part_c, const unsigned* part_n, size_t nblk, int C, int H, const int* status, double* cost, unsigned* count);
// two-view RANSAC (mcba_twoview.hip): the device side of mcba_two_view_ransac, one launcher per stage, every buffer the
// caller's.  M >= 8 common points, 1 <= H <= MCBA_TWOVIEW_MAX_HYPOTHESES.  Nothing is accumulated with atomics: the results depend on (M, H) alone.
struct TvCams { double ka[4], da[5], kb[4], db[5]; };   // (fx fy cx cy), (k1 k2 p1 p2 k3) of camera a and of camera b
// prep: 8 planes of M doubles (undistorted pixels a.x a.y b.x b.y, normalised a.x a.y b.x b.y)
void launch_tv_prepare(hipStream_t st, const double* uv_a, const double* uv_b, size_t M, const TvCams& cams, int und_iters, double* prep);
// E, F (H, 9), status (H).  e_in (H, 9) or nullptr: the generator is skipped, E = e_in (void where not finite)
void launch_tv_hypotheses(hipStream_t st, const double* prep, size_t M, const int* samples, int H, const double* e_in, const TvCams& cams, double* E, double* F, int* status);
// part_c, part_n: hyp_score_blocks(M) x H per-workgroup partial costs and inlier counts
void launch_tv_score(hipStream_t st, const double* prep, size_t M, const double* F, int H, double threshold, double* part_c, unsigned* part_n);
// cost (H; +inf for a void hypothesis), count (H); then the winner: win_idx[0], best4[0 .. 2] = (index, cost, inliers), cand (4 x 12) = its four (R, t)
void launch_tv_finish(hipStream_t st, const double* part_c, const unsigned* part_n, size_t nblk, int H, const double* E, const int* status, double* cost, unsigned* count, int* win_idx, double* best4,
                      double* cand);
// inliers (M bytes), part_f: hyp_point_blocks(M) x 4 in-front counts; then win_idx[1] = the candidate, best4[3] = its count, rt12; points (M, 3), NaN for non-inliers
void launch_tv_pose(hipStream_t st, const double* prep, size_t M, const double* F, const int* status, double threshold, const double* cand, unsigned* part_f, int* win_idx, double* best4, double* rt12,
                    unsigned char* inliers, double* points);
// the five-point generator (mcba_fivepoint.hip): 1 <= H <= MCBA_TWOVIEW5_MAX_SAMPLES samples of five correspondences.  E10, F10
// (10 H, 9), status10 (10 H): the candidate table in slot order; Ep, Fp (10 H rows of room), stp, map: its live rows packed in index order, map[i] =
// 10 sample + slot, n_packed[0] of them (at least 1: a void row 0 where nothing is live) -- the table launch_tv_score .. launch_tv_pose take
void launch_tv5_hypotheses(hipStream_t st, const double* prep, size_t M, const int* samples, int H, const TvCams& cams, double* E10, double* F10, int* status10, double* Ep, double* Fp, int* stp,
                           int* map, int* n_packed);
// camera resection (mcba_resect.hip): the device side of mcba_resect_ransac and mcba_resect_refine, one launcher per stage,
// every buffer the caller's.  C cameras (the grid's last dimension) of at least 6 usable points each, 1 <= H <= MCBA_RESECT_MAX_HYPOTHESES per camera.
// Nothing is accumulated with atomics: the results depend on (P, H) alone.
// points (P, 3), uvs (C, P, 2), cams (C, 9) = fx fy cx cy k1 k2 p1 p2 k3.  prep: per camera 4 planes of P doubles (undistorted u, v; normalised x, y); usable (C, P)
void launch_rs_prepare(hipStream_t st, const double* points, const double* uvs, size_t P, int C, const double* cams, int und_iters, double* prep, unsigned char* usable);
// pose, KP (C, H, 12), status (C, H).  pose_in (C, H, 12) or nullptr: the generator is skipped, pose = pose_in (void where not finite)
void launch_rs_hypotheses(hipStream_t st, const double* points, const double* prep, size_t P, int C, const int* samples, int H, const double* pose_in, const double* cams, double* pose, double* KP,
                          int* status);
// the P3P generator (mcba_resect_p3p.hip): samples (C, H, 3), 1 <= H <= MCBA_RESECT_P3P_MAX_SAMPLES; pose, KP (C, 4 H, 12),
// status (C, 4 H): the candidates of sample h in slots 4 h .. 4 h + 3, void slots included -- the table launch_rs_score .. launch_rs_mask take with 4 H for H
void launch_rs3_hypotheses(hipStream_t st, const double* points, const double* prep, size_t P, int C, const int* samples, int H, const double* cams, double* pose, double* KP, int* status);
// part_c, part_n: (C, hyp_score_blocks(P), H) per-workgroup partial costs and inlier counts
void launch_rs_score(hipStream_t st, const double* points, const double* prep, const unsigned char* usable, size_t P, int C, const double* KP, int H, double threshold, double* part_c,
                     unsigned* part_n);
// cost (C, H; +inf for a void hypothesis), count (C, H); then per camera the winner: win_idx (C), best4 (C, 4)[0 .. 2] = (index, cost, inliers), rt12 (C, 12) = its pose
void launch_rs_finish(hipStream_t st, const double* part_c, const unsigned* part_n, size_t nblk, int C, int H, const double* pose, const int* status, double* cost, unsigned* count, int* win_idx,
                      double* best4, double* rt12);
// inliers (C, P) bytes: the winner's
void launch_rs_mask(hipStream_t st, const double* points, const double* prep, const unsigned char* usable, size_t P, int C, const double* KP, const int* status, int H, double threshold,
                    const int* win_idx, unsigned char* inliers);
// the polish, one evaluation of n listed problems: ids (n) = the row of uvs / mask, tcs (n) = the camera at the pose to evaluate; part (n, hyp_point_blocks(P), 29);
// sys (n, 29) = upper triangle of J^T W J | gradient | robust cost | detections used; cost_only: the last two alone, the others 0.  Non-zero: an unknown loss.
int launch_rs_normal(hipStream_t st, int loss, bool cost_only, const double* points, const double* uvs, const unsigned char* mask, size_t P, int n, const int* ids, const TcCam* tcs, double f_scale,
                     double* part, double* sys);
// calibration uncertainty (mcba_cov.hip).  Non-zero: arguments out of range.
// part: 2 x 1024 doubles of scratch; out[0] = sum rho' f^2, out[1] = present scalars of the residual vector res (NaN = missing)
int launch_cov_wss(hipStream_t st, int loss, double f_scale, const double* res, size_t count, double* part, double* out);
// flag[f]: 0 = V_f positive definite, 1 = a frame without data, 2 = not positive definite with data; counts[0] += flags != 0, counts[1] += flags == 2
void launch_cov_check(hipStream_t st, const double* rec, unsigned char* flag, int* counts, int C, int F, int Fpad);
// S0 (n x n) -> Sig (ld x ld, ld = ceil(n / 64) 64, zero outside the free n x n) = sigma2 S_g^-1; R, M: ld x ld scratch, isd: n; *pivot (preset to -1) = the first failing pivot
void launch_cov_cam(hipStream_t st, const double* S0, int n, int cw, int gauge, double sigma2, double* R, double* M, double* isd, double* Sig, int ld, int* pivot);
int cov_frames_group(int n, int lds_limit, int force_g);   // frames per workgroup of k_cov_frames (8 or 4; 0: no shape fits)
int launch_cov_frames(hipStream_t st, const double* rec, const double* fbuf, const unsigned char* flag, const double* Sig, int ld, double sigma2, double* out, int C, int F, int Fpad, int cw, int G);

// ---- triangulation uncertainty (mcba_tricov.hip).  uvs (C, P, 2) raw detections (NaN = unseen), pts (P, 3), cams: the
// table of mcba_tricov_math.h (TcCam) in device memory, 2 <= C <= 64.  Non-zero: arguments out of range.
int tricov_point_blocks(size_t npts);   // workgroups of k_tricov_point: part holds 4 doubles for each
// hinv (P, 6) = H^-1 packed (NaN unless status is 1), views / status (P); then info[0 .. 4] = sigma2 (sigma2_in, or -- NaN -- pooled in a fixed
// order), present scalars m and 3 P_u of the points of status 1, points of status -1, points of status -2
int launch_tricov_point(hipStream_t st, int loss, const double* uvs, const double* pts, size_t npts, const TcCam* cams, int C, double f_scale, double sigma2_in, double* hinv, int* views, int* status,
                        double* part, double* info, const double* sw = nullptr);
void launch_tricov_scale(hipStream_t st, const double* hinv, const int* status, const double* info, size_t npts, double* det6);   // det6 = info[0] hinv
int tricov_group(int n, int lds_limit, int force_g);   // points per workgroup of k_tricov_cal (16, 10 or 5; 0: no shape fits)
// det6 = sigma2 H^-1 and cal6 = G Sig G^T (both (P, 6) packed), Sig the zero-padded ld x ld camera covariance (ld a multiple of 64, >= 12 C rounded up to 32)
int launch_tricov_cal(hipStream_t st, int loss, const double* uvs, const double* pts, size_t npts, const TcCam* cams, int C, double f_scale, const double* hinv, const int* status, const double* Sig,
                      int ld, const double* info, double* det6, double* cal6, int G, const double* sw = nullptr);

// ---- trajectory smoothing (mcba_smooth.hip).  SmLevel, SmData: mcba_smooth_math.h.  A chunk of K tracks, (T, K, .) planes
struct SmLevel;
struct SmData;
// p, winv, w from the raw points, packed covariances and start weights (w_in NULL: 1); n_usable (K)
void launch_smooth_prepare(hipStream_t st, size_t T, int K, const double* pts, const double* cov6, const double* w_in, double* p, double* winv, double* w, int* n_usable);
// the elimination alone, every level up, of the nact tracks of list; bad (K) is set to 1 where a pivot was refused
int launch_smooth_reduce(hipStream_t st, const SmLevel* lv, int levels, const SmData& td, int K, const int* list, int nact, int* bad, bool rhs = false);
// the back-substitution alone, every level down.  rhs (both): level 0 in the right-hand-side mode of mcba_smooth_math.h (SmData::rhs)
int launch_smooth_backsub(hipStream_t st, const SmLevel* lv, int levels, const SmData& td, int K, const int* list, int nact, bool rhs = false);
// after launch_smooth_reduce(rhs = true): the forward pass again for the right-hand side td.rhs holds now, from the stored factors; done: null or a
// device word that, non-zero, makes the launches return at once.  launch_smooth_backsub(rhs = true) follows
int launch_smooth_resolve(hipStream_t st, const SmLevel* lv, int levels, const SmData& td, int K, const int* list, int nact, const int* done);
// one linear solve (launch_smooth_reduce, then every level down) of the nact tracks of list, then res (nact, 4) = objective, step, max |x|, 0
int launch_smooth_solve(hipStream_t st, const SmLevel* lv, int levels, const SmData& td, int K, const int* list, int nact, int* bad, double* part, double* res);

// ---- trajectory uncertainty (mcba_smooth_cov.hip).  After launch_smooth_reduce: the selected inversion, every level
// down: z[l] = the SM_ZC planes of level l >= 1 (mcba_smooth_cov_math.h), cov6 (T, K, 6), lag9 (T - 1, K, 9) or null
int launch_smooth_selinv(hipStream_t st, const SmLevel* lv, int levels, const SmData& td, double* const* z, double* cov6, double* lag9, int K, const int* list, int nact);

// ---- the smoother's evidence (mcba_smooth_evidence.hip).  After launch_smooth_reduce and launch_smooth_backsub of the nact
// tracks of list: res (nact, 4) = sum w d^2, sum |second difference|^2, the sum of log over the stored pivot reciprocals of every factorised block,
// and 1 where bad (launch_smooth_reduce's flags, K) is set.
// part: 2 smooth_eval_blocks(T) nact doubles, lane: evidence_lanes() nact doubles of scratch; mark: null or an event recorded ahead of the
// log-determinant kernels
int launch_smooth_evidence(hipStream_t st, const SmLevel* lv, int levels, const SmData& td, int K, const int* list, int nact, const int* bad, double* part, double* lane, double* res, hipEvent_t mark);

// ---- trajectory refinement (mcba_traj_refine.hip).  TrData: mcba_traj_refine_math.h, the planes of a chunk of K tracks;
// cams: a KpCam table in device memory, 1 <= C <= kKpMaxCams; loss: linear, soft_l1 or huber.  Non-zero: arguments out of range
struct TrData;
// per track its usable frames (two cameras or more), its single ones (exactly one) and the non-finite coordinates of its start (K each)
int launch_traj_count(hipStream_t st, const TrData& rd, int C, int K, int* n_usable, int* n_single, int* n_bad);
// H and G at x for the tracks with run[k] != 0
int launch_traj_linearise(hipStream_t st, int loss, const TrData& rd, const KpCam* cams, int C, int K, const int* run);
// res (nact, TR_SUMS) of the nact tracks of list from x and d; part: TR_SUMS smooth_eval_blocks(T) nact doubles of scratch
int launch_traj_trial(hipStream_t st, int loss, const TrData& rd, const KpCam* cams, int C, int K, const int* list, int nact, double* part, double* res);
// x <- x + alpha[k] d for every track of the chunk (alpha 0: untouched)
int launch_traj_apply(hipStream_t st, const TrData& rd, int K, const double* alpha);

// ---- skeleton-constrained keypoint refinement (mcba_skeleton.hip).  SkArgs, SkPlan: mcba_skeleton_math.h -- the planes of
// a launch (device memory) and the forest plan (plan_dev: a copy in device memory); cams: a KpCam table in device memory, 1 <= C <= kKpMaxCams;
// loss: LOSS_LINEAR .. LOSS_ARCTAN.  Non-zero: arguments out of range
struct SkArgs;
struct SkPlan;
// every frame of a.T: the loop (a.system == 0; with a.cov the marginal covariance at the result) or one evaluation laid open (a.system != 0)
int launch_skel_refine(hipStream_t st, int loss, const SkArgs& a, const SkPlan* plan_dev, int K, const KpCam* cams, int C);
// dist (E, T): the distance between the two ends of bone e = bones[2 e], bones[2 e + 1] in frame t of pts (T, K, 3), NaN where an end has a NaN
int launch_skel_dist(hipStream_t st, const double* pts, const int* bones, size_t T, int K, int E, double* dist);
// dist <- |dist - the median of its bone| with sel the states of launch_select over dist (two per bone)
int launch_skel_absdev(hipStream_t st, double* dist, const SelState* sel, size_t T, int E);

// ---- skeleton trajectories (mcba_skeltraj.hip).  SktData: mcba_skeltraj_math.h, the planes of the call over K <= 64
// tracks, its active forest (device memory) and run (K).  Every launch is flat over (frame, keypoint) and takes part: one double per workgroup
// of 256 lanes (SKT_SUMS for the trial).  Non-zero: arguments out of range
struct SktData;
// after launch_traj_linearise: the bones' gradient into G, q = G, dir and bres
int launch_skt_linearise(hipStream_t st, const SktData& sd, int K);
// after the first solve M z = -G: p = z, d = 0, sc (CG_DOUBLES) and w (CG_INTS) set for a new solve
int launch_skt_cg_start(hipStream_t st, const SktData& sd, int K, double* part, double* sc, int* w);
// one iteration of the preconditioned recurrence: operator, step, the re-solve of td (rhs = q, x = z) from the factors in lv, direction.  Every
// kernel of it but the back-substitution returns at once when w[CG_DONE] is set; the last iteration sets it (tol2 = cg_tol^2, cg_max)
int launch_skt_cg_iteration(hipStream_t st, const SktData& sd, int K, const SmLevel* lv, int levels, const SmData& td, const int* list, int nact, double tol2, int cg_max, double* part,
                            double* sc, int* w);
// res (SKT_SUMS) of the whole call from x and d
int launch_skt_trial(hipStream_t st, int loss, const SktData& sd, const KpCam* cams, int C, int K, double* part, double* res);

// ---- free-point bundle adjustment of the extrinsics (mcba_kpba.hip).  uvs (C, P, 2) raw detections (NaN = unseen), pts
// (P, 3), cams: TcCam table in device memory, 2 <= C <= 24, held (C): bit i = scalar i of the camera is not free.  Non-zero: arguments out of range.
int kpba_group(int C, int lds_limit, int force_g);   // points per group of k_kpba_reduce (64, 32 or 16; 0: no shape fits)
int kpba_groups(size_t npts);                        // workgroups of a pass: that many partial systems
size_t kpba_partial_size(int C);                     // doubles of one (partial) system: NP NP + 33 C + 4, NP = 6 C rounded up to 16
// wide (here and in launch_kpba_step): the instantiation whose camera tables hold kKtMaxCams, for the tiled reduction
int launch_kpba_status(hipStream_t st, const double* uvs, const double* pts, size_t npts, const TcCam* cams, int C, int* status, const double* sw = nullptr, bool wide = false);
// sys = Y Y^T (NP, NP) | per camera U_c packed lower, g_c, sum Y z (C, 33) | cost, present scalars, max |g_p|, 0; part: kpba_groups() partial systems
int launch_kpba_reduce(hipStream_t st, int loss, const double* uvs, const double* pts, const int* status, size_t npts, const TcCam* cams, const int* held, int C, double f_scale, double lam, int G,
                       double* part, double* sys, const double* sw = nullptr);
// cams2: the current table and behind it the trial one; trial (P, 3) the trial points; out4 = trial cost, sum dX^2, 0, sum X^2; part4: 4 kpba_groups()
int launch_kpba_step(hipStream_t st, int loss, const double* uvs, const double* pts, double* trial, const int* status, size_t npts, const TcCam* cams2, const double* dtheta, int C, double f_scale,
                     double lam, double* part4, double* out4, const double* sw = nullptr, bool wide = false);
void launch_kpba_finish(hipStream_t st, const double* part, int nwg, int C, double* sys);   // k_kpba_finish: nwg partial systems in order -> sys
void launch_kpba_finish_sized(hipStream_t st, const double* part, int nwg, int NP, int nacc, double* sys);   // the same kernel for a system of NP NP + nacc + 4 doubles
// ---- free-point bundle adjustment of the cameras, intrinsics free (mcba_kpcam.hip): the calls above with 12 scalars
// per camera, 2 <= C <= 12, held (C): 12 bits in theta_c order.  k_kpba_status and k_kpba_finish are the ones above.
int kpcam_group(int C, int lds_limit, int force_g);   // points per group of k_kpcam_reduce (64, 32 or 16; 0: no shape fits)
size_t kpcam_partial_size(int C);                     // doubles of one (partial) system: NP NP + 102 C + 4, NP = 12 C rounded up to 16
size_t kpcam_reduce_lds(int C, int G);                // dynamic LDS of k_kpcam_reduce
// sys = Y Y^T (NP, NP) | per camera U_c packed lower (78), g_c (12), sum Y z (12) | cost, present scalars, max |g_p|, 0; part: kpba_groups() partial systems
int launch_kpcam_reduce(hipStream_t st, int loss, const double* uvs, const double* pts, const int* status, size_t npts, const TcCam* cams, const int* held, int C, double f_scale, double lam, int G,
                        double* part, double* sys, const double* sw = nullptr);
// cams2: the current table and behind it the trial one; dtheta (C, 12); out4 = trial cost, sum dX^2, 0, sum X^2; part4: 4 kpba_groups()
int launch_kpcam_step(hipStream_t st, int loss, const double* uvs, const double* pts, double* trial, const int* status, size_t npts, const TcCam* cams2, const double* dtheta, int C, double f_scale,
                      double lam, double* part4, double* out4, const double* sw = nullptr);
// ---- the tiled reduction (mcba_kpba_tiled.hip): the same system for 2 <= C <= 64, camera bands of kKtBand, groups of kKtGroup points.
constexpr int kKtMaxCams = 64, kKtBand = 16, kKtGroup = 16;
int kpba_tiled_groups(int C, size_t npts);   // workgroups along the points = partial systems: all of them within the resident path's largest allocation
int kpba_tiled_pairs(int C);                 // band pairs (I >= J)
size_t kpba_tiled_lds();                     // dynamic LDS of k_kpba_reduce_tiled, the same for every C
// fac: (P, 13) point factors, written by k_kpba_factors and read by k_kpba_reduce_tiled; part: kpba_tiled_groups() partial systems
int launch_kpba_reduce_tiled(hipStream_t st, int loss, const double* uvs, const double* pts, const int* status, size_t npts, const TcCam* cams, const int* held, int C, double f_scale, double lam,
                             double* fac, double* part, double* sys, const double* sw = nullptr);
}  // namespace mcba
