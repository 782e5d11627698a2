// mcba_skeleton_api.hip -- the stateless skeleton calls of include/mcba.h (host arrays in, host arrays out, a device ordinal, no handle), in the
// idiom of mcba_traj_refine_api.hip.  Frames are independent, so a call runs them in chunks of whole frames under a device-memory budget; the
// forest plan (order, levels, child lists) is derived and checked here, before a device is touched, by skel_plan (mcba_skeleton_math.h).  One
// launch per chunk: the whole Levenberg-Marquardt loop of a frame runs inside k_skel_refine.
#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "mcba_handle.h"
#include "mcba_kernels.h"
#include "mcba_skeleton_math.h"

using namespace mcba_internal;

namespace {

constexpr double SK_BUDGET_BYTES = 2048.0 * 1048576.0;   // device memory of one chunk of frames

struct SkelIn {
  size_t T;
  int K, C;
  const double *uvs, *cam12, *dist5, *weights, *pixel_std, *start;
  const int* parent;
  const double *bone_length, *bone_std;
  int loss;
  double f_scale;
  int max_iterations;
  double xtol, lam;
  int device;
};
// system: one evaluation at the points (gradient, step, the costs); otherwise the loop
struct SkelOut {
  bool system;
  double* points;
  int *kstatus, *fstatus, *nit;
  double *cost, *cost0, *bone_res, *cov6, *info6, *dir, *grad, *step, *data_cost, *bone_cost, *trial_cost;
  double *info8, *kernel_ms;
};

int skel_check(const char* who, const SkelIn& in, mcba::SkPlan& plan) {
  auto bad = [&](const char* what) { g_err = std::string(who) + ": " + what; return MCBA_ERR_ARG; };
  if (in.T < 1 || in.T > ((size_t)1 << 31)) return bad("1 .. 2^31 frames required");
  if (in.K < 1 || in.K > mcba::SK_MAX_K) return bad("1 .. 64 keypoints required");
  if (in.C < 1 || in.C > mcba::kKpMaxCams) return bad("1 .. 64 cameras required");
  if (!in.uvs || !in.cam12 || !in.pixel_std || !in.start || !in.parent || !in.bone_length || !in.bone_std) return bad("non-NULL arrays (but dist5 and weights) required");
  if (in.loss < mcba::LOSS_LINEAR || in.loss > mcba::LOSS_ARCTAN) return bad("loss must be one of linear, soft_l1, huber, cauchy, arctan (0 .. 4)");
  if (!(in.f_scale > 0.0) || !mcba::sk_finite(in.f_scale)) return bad("f_scale must be positive and finite");
  if (in.max_iterations < 1) return bad("max_iterations >= 1");
  if (!(in.xtol >= 0.0)) return bad("xtol >= 0");
  if (!(in.lam >= 0.0) || !mcba::sk_finite(in.lam)) return bad("the damping must be finite and not negative");
  for (int c = 0; c < in.C; ++c)
    if (!(in.pixel_std[c] > 0.0) || !mcba::sk_finite(in.pixel_std[c]) || !mcba::sk_finite(1.0 / in.pixel_std[c])) return bad("pixel_std must be positive and finite (and its inverse too)");
  switch (mcba::skel_plan(in.K, in.parent, in.bone_length, in.bone_std, plan)) {
    case 0: break;
    case 2: return bad("a parent outside -1 .. K - 1, or a keypoint that is its own parent");
    case 3: return bad("the parents form a cycle: the skeleton must be a forest");
    default: return bad("bone_length and bone_std must be positive and finite for every keypoint with a parent");
  }
  return check_weights(who, in.weights, (size_t)in.C * in.T * in.K);
}

// device doubles (ints counted as doubles) one frame needs
size_t skel_frame_doubles(int K, int C, bool system, bool cov) {
  return (size_t)K * (3 * (size_t)C + 3 + 3 + 1 + 1 + (system ? 6 + 3 + 3 + 3 : cov ? 6 + 6 + 3 : 0)) + 8;
}

int skel_run(const char* who, const SkelIn& in, const SkelOut& out, const mcba::SkPlan& plan) {
  (void)who;
  const size_t T = in.T, K = (size_t)in.K;
  const int C = in.C;
  const bool cov = out.cov6 != nullptr, wide = out.system || cov;
  const size_t per_frame = skel_frame_doubles(in.K, C, out.system, cov) * sizeof(double);
  const size_t Tc = std::min<size_t>(T, std::max<size_t>(1, (size_t)(SK_BUDGET_BYTES / (double)per_frame)));
  const size_t nchunks = (T + Tc - 1) / Tc, TK = Tc * K;

  StatelessCall call;
  mcba::KpCam* d_cams = nullptr;
  mcba::SkPlan* d_plan = nullptr;
  std::vector<mcba::KpCam> tab((size_t)C);
  for (int c = 0; c < C; ++c) mcba::make_kp_cam(in.cam12 + 12 * c, in.dist5 ? in.dist5 + 5 * c : nullptr, tab[c]);
  if (int rc = call.upload(&d_cams, tab.data(), tab.size())) return rc;
  if (int rc = call.upload(&d_plan, &plan, 1)) return rc;
  double *d_det = nullptr, *d_sw = nullptr, *d_x = nullptr, *d_pts = nullptr, *d_cost = nullptr, *d_cost0 = nullptr, *d_bres = nullptr, *d_cov = nullptr, *d_info = nullptr, *d_dir = nullptr,
         *d_grad = nullptr, *d_step = nullptr, *d_dc = nullptr, *d_bc = nullptr, *d_tc = nullptr;
  int *d_kst = nullptr, *d_fst = nullptr, *d_nit = nullptr;
  if (int rc = call.scratch(&d_det, 2 * C * TK)) return rc;
  if (int rc = call.scratch(&d_sw, C * TK)) return rc;
  if (int rc = call.scratch(&d_x, 3 * TK)) return rc;
  if (int rc = call.scratch(&d_kst, TK)) return rc;
  if (int rc = call.scratch(&d_fst, Tc)) return rc;
  if (out.system) {
    if (int rc = call.scratch(&d_grad, 3 * TK)) return rc;
    if (int rc = call.scratch(&d_step, 3 * TK)) return rc;
    if (int rc = call.scratch(&d_dc, Tc)) return rc;
    if (int rc = call.scratch(&d_bc, Tc)) return rc;
    if (int rc = call.scratch(&d_tc, Tc)) return rc;
  } else {
    if (int rc = call.scratch(&d_pts, 3 * TK)) return rc;
    if (int rc = call.scratch(&d_nit, Tc)) return rc;
    if (int rc = call.scratch(&d_cost, Tc)) return rc;
    if (int rc = call.scratch(&d_cost0, Tc)) return rc;
    if (int rc = call.scratch(&d_bres, TK)) return rc;
    if (cov) if (int rc = call.scratch(&d_cov, 6 * TK)) return rc;
  }
  if (wide) {
    if (int rc = call.scratch(&d_info, 6 * TK)) return rc;
    if (int rc = call.scratch(&d_dir, 3 * TK)) return rc;
  }
  HIPCHK(hipEventCreate(&call.e0));
  HIPCHK(hipEventCreate(&call.e1));

  std::vector<double> h_sw;
  double ms_total = 0.0;
  int most = 0;
  for (size_t c0 = 0; c0 < nchunks; ++c0) {
    const size_t t0 = c0 * Tc, tc = std::min(Tc, T - t0), tk = tc * K;
    // the chunk's planes: detections (C, tc K) pairs, sqrt(w) / pixel_std beside them, the start
    h_sw.resize(C * tk);
    for (int cc = 0; cc < C; ++cc) {
      const double ips = 1.0 / in.pixel_std[cc];
      for (size_t i = 0; i < tk; ++i) {
        const double w = in.weights ? in.weights[(cc * T + t0) * K + i] : 1.0;
        h_sw[cc * tk + i] = w > 0.0 ? sqrt(w) * ips : 0.0;   // (a zero or NaN weight: unseen)
      }
    }
    HIPCHK(hipMemcpy2D(d_det, 2 * tk * sizeof(double), in.uvs + 2 * t0 * K, 2 * T * K * sizeof(double), 2 * tk * sizeof(double), (size_t)C, hipMemcpyHostToDevice));
    if (int rc = call.put(d_sw, h_sw.data(), C * tk)) return rc;
    if (int rc = call.put(d_x, in.start + 3 * t0 * K, 3 * tk)) return rc;
    mcba::SkArgs a{};
    a.T = tc; a.det = d_det; a.sw = d_sw; a.start = d_x;
    a.fs2 = in.f_scale * in.f_scale; a.inv_fs2 = 1.0 / a.fs2; a.lam0 = in.lam; a.xtol = in.xtol;
    a.max_iterations = out.system ? 1 : in.max_iterations; a.system = out.system ? 1 : 0; a.cov = cov ? 1 : 0;
    a.points = d_pts; a.kstatus = d_kst; a.fstatus = d_fst; a.nit = d_nit; a.cost = d_cost; a.cost0 = d_cost0; a.bone_res = d_bres; a.info6 = d_info; a.dir = d_dir; a.cov6 = d_cov;
    a.grad = d_grad; a.step = d_step; a.data_cost = d_dc; a.bone_cost = d_bc; a.trial_cost = d_tc;
    HIPCHK(hipEventRecord(call.e0, nullptr));
    if (mcba::launch_skel_refine(nullptr, in.loss, a, d_plan, in.K, d_cams, C) != 0) return fail(MCBA_ERR_ARG, "skeleton refinement: bad launch");
    if (int rc = check_launch()) return rc;
    HIPCHK(hipEventRecord(call.e1, nullptr));
    HIPCHK(hipEventSynchronize(call.e1));
    float ms = 0.f;
    HIPCHK(hipEventElapsedTime(&ms, call.e0, call.e1));
    ms_total += ms;
    if (int rc = call.download(out.kstatus + t0 * K, d_kst, tk)) return rc;
    if (int rc = call.download(out.fstatus + t0, d_fst, tc)) return rc;
    if (out.system) {
      if (int rc = call.download(out.grad + 3 * t0 * K, d_grad, 3 * tk)) return rc;
      if (int rc = call.download(out.step + 3 * t0 * K, d_step, 3 * tk)) return rc;
      if (int rc = call.download(out.data_cost + t0, d_dc, tc)) return rc;
      if (int rc = call.download(out.bone_cost + t0, d_bc, tc)) return rc;
      if (int rc = call.download(out.trial_cost + t0, d_tc, tc)) return rc;
    } else {
      if (int rc = call.download(out.points + 3 * t0 * K, d_pts, 3 * tk)) return rc;
      if (int rc = call.download(out.nit + t0, d_nit, tc)) return rc;
      if (int rc = call.download(out.cost + t0, d_cost, tc)) return rc;
      if (int rc = call.download(out.cost0 + t0, d_cost0, tc)) return rc;
      if (int rc = call.download(out.bone_res + t0 * K, d_bres, tk)) return rc;
      if (cov) if (int rc = call.download(out.cov6 + 6 * t0 * K, d_cov, 6 * tk)) return rc;
      for (size_t t = 0; t < tc; ++t) most = std::max(most, out.nit[t0 + t]);
    }
    if (wide) {
      if (int rc = call.download(out.info6 + 6 * t0 * K, d_info, 6 * tk)) return rc;
      if (int rc = call.download(out.dir + 3 * t0 * K, d_dir, 3 * tk)) return rc;
    }
  }
  double* info8 = out.info8;
  info8[0] = plan.levels; info8[1] = mcba::skel_frames_per_group(in.K); info8[2] = (double)Tc; info8[3] = (double)nchunks; info8[4] = ms_total; info8[5] = out.system ? 1 : most;
  info8[6] = (double)per_frame * (double)Tc; info8[7] = 0.0;
  if (out.kernel_ms) *out.kernel_ms = ms_total;
  return MCBA_OK;
}

}  // namespace

extern "C" {

int mcba_refine_skeleton(size_t n_frames, int n_keypoints, int n_cameras, const double* uvs, const double* cam12, const double* dist5, const double* weights, const double* pixel_std,
                         const double* start, const int* parent, const double* bone_length, const double* bone_std, int loss, double f_scale, int max_iterations, double xtol, int device,
                         double* out_points, int* keypoint_status, int* frame_status, int* n_iterations, double* cost, double* cost_start, double* bone_residual, double* out_cov6,
                         double* information, double* direction, double* info8, double* kernel_ms) {
  const char* who = "mcba_refine_skeleton";
  const SkelIn in{n_frames, n_keypoints, n_cameras, uvs, cam12, dist5, weights, pixel_std, start, parent, bone_length, bone_std, loss, f_scale, max_iterations, xtol, mcba::SK_LAM_START, device};
  mcba::SkPlan plan;
  if (int rc = skel_check(who, in, plan)) return rc;
  if (!out_points || !keypoint_status || !frame_status || !n_iterations || !cost || !cost_start || !bone_residual || !info8 || (out_cov6 && (!information || !direction)) ||
      (!out_cov6 && (information || direction)))
    return fail(MCBA_ERR_ARG, "mcba_refine_skeleton: non-NULL outputs required (out_cov6, information and direction: all three or none)");
  if (int rc = stateless_device(device, who)) return rc;
  const SkelOut out{false, out_points, keypoint_status, frame_status, n_iterations, cost, cost_start, bone_residual, out_cov6, information, direction, nullptr, nullptr, nullptr, nullptr, nullptr,
                    info8, kernel_ms};
  return skel_run(who, in, out, plan);
}

int mcba_refine_skeleton_system(size_t n_frames, int n_keypoints, int n_cameras, const double* uvs, const double* cam12, const double* dist5, const double* weights, const double* pixel_std,
                                const double* points, const int* parent, const double* bone_length, const double* bone_std, int loss, double f_scale, double lam, int device, double* information,
                                double* gradient, double* direction, double* step, int* keypoint_status, int* frame_status, double* data_cost, double* bone_cost, double* trial_cost,
                                double* info8, double* kernel_ms) {
  const char* who = "mcba_refine_skeleton_system";
  const SkelIn in{n_frames, n_keypoints, n_cameras, uvs, cam12, dist5, weights, pixel_std, points, parent, bone_length, bone_std, loss, f_scale, 1, 0.0, lam, device};
  mcba::SkPlan plan;
  if (int rc = skel_check(who, in, plan)) return rc;
  if (!information || !gradient || !direction || !step || !keypoint_status || !frame_status || !data_cost || !bone_cost || !trial_cost || !info8)
    return fail(MCBA_ERR_ARG, "mcba_refine_skeleton_system: non-NULL outputs required");
  if (int rc = stateless_device(device, who)) return rc;
  const SkelOut out{true, nullptr, keypoint_status, frame_status, nullptr, nullptr, nullptr, nullptr, nullptr, information, direction, gradient, step, data_cost, bone_cost, trial_cost, info8, kernel_ms};
  return skel_run(who, in, out, plan);
}

int mcba_bone_lengths(size_t n_frames, int n_keypoints, const double* points, int n_bones, const int* bones, int device, double* length, double* std, int* count, double* kernel_ms) {
  const char* who = "mcba_bone_lengths";
  if (n_frames < 1 || n_frames > ((size_t)1 << 31) || n_keypoints < 1 || n_bones < 1 || n_bones > 65535 || !points || !bones || !length || !std || !count)
    return fail(MCBA_ERR_ARG, "mcba_bone_lengths: 1 .. 2^31 frames, at least one keypoint, 1 .. 65535 bones and non-NULL arrays required");
  for (int e = 0; e < 2 * n_bones; ++e)
    if (bones[e] < 0 || bones[e] >= n_keypoints) return fail(MCBA_ERR_ARG, "mcba_bone_lengths: a bone's keypoint outside 0 .. K - 1");
  if (int rc = stateless_device(device, who)) return rc;
  const size_t T = n_frames, E = (size_t)n_bones;
  StatelessCall call;
  double *d_pts = nullptr, *d_dist = nullptr;
  int* d_bones = nullptr;
  mcba::SelState *d_sel = nullptr, *d_sel2 = nullptr;   // the states of the two selections: lengths, then absolute deviations
  std::vector<mcba::SelState> sel(2 * E), sel2(2 * E);
  if (int rc = call.upload(&d_pts, points, 3 * T * n_keypoints)) return rc;
  if (int rc = call.upload(&d_bones, bones, 2 * E)) return rc;
  if (int rc = call.scratch(&d_dist, E * T)) return rc;
  if (int rc = call.scratch(&d_sel, 2 * E)) return rc;
  if (int rc = call.scratch(&d_sel2, 2 * E)) return rc;
  HIPCHK(call.start());
  if (mcba::launch_skel_dist(nullptr, d_pts, d_bones, T, n_keypoints, n_bones, d_dist) != 0) return fail(MCBA_ERR_ARG, "mcba_bone_lengths: bad launch");
  if (int rc = check_launch()) return rc;
  mcba::launch_select(nullptr, d_dist, nullptr, T, n_bones, 1 /* no frame mask */, d_sel, 0 /* distances are >= +0 */);
  if (int rc = check_launch()) return rc;
  if (mcba::launch_skel_absdev(nullptr, d_dist, d_sel, T, n_bones) != 0) return fail(MCBA_ERR_ARG, "mcba_bone_lengths: bad launch");
  if (int rc = check_launch()) return rc;
  mcba::launch_select(nullptr, d_dist, nullptr, T, n_bones, 1, d_sel2, 0);
  if (int rc = check_launch()) return rc;
  HIPCHK(call.stop(kernel_ms));
  if (int rc = call.download(sel.data(), d_sel, sel.size())) return rc;
  if (int rc = call.download(sel2.data(), d_sel2, sel2.size())) return rc;
  for (size_t e = 0; e < E; ++e) {
    length[e] = mcba::sel_median(sel[2 * e], sel[2 * e + 1]);
    std[e] = 1.4826 * mcba::sel_median(sel2[2 * e], sel2[2 * e + 1]);
    count[e] = (int)sel[2 * e].count;
  }
  return MCBA_OK;
}

}  // extern "C"
