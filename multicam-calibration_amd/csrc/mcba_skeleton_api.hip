// mcba_skeleton_api.hip -- the stateless skeleton calls of include/mcba.h (host arrays in, host arrays out, a device ordinal, no handle), in the
// idiom of mcba_traj_refine_api.hip.  Frames are independent, so a call runs them in chunks of whole frames under a device-memory budget; the
// forest plan (order, levels, child lists) is derived and checked here, before a device is touched, by skel_plan (mcba_skeleton_math.h).  One
// launch per chunk: the whole Levenberg-Marquardt loop of a frame runs inside k_skel_refine.  The argument checks it has in common with the
// trajectory calls, the camera table and the timed bracket are those of mcba_handle.h; the weight plane is kp_weight_box (mcba_keypoint_math.h).
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
  const DetectionChecks ck{who};
  if (int rc = ck.frames_keypoints(in.T, in.K, mcba::SK_MAX_K)) return rc;
  if (int rc = ck.cameras_arrays(in.C, mcba::kKpMaxCams, in.uvs && in.cam12 && in.pixel_std && in.start && in.parent && in.bone_length && in.bone_std)) return rc;
  if (in.loss < mcba::LOSS_LINEAR || in.loss > mcba::LOSS_ARCTAN) return ck.bad("loss must be one of linear, soft_l1, huber, cauchy, arctan (0 .. 4)");
  if (int rc = ck.loop(in.f_scale, in.max_iterations, in.xtol)) return rc;
  if (!(in.lam >= 0.0) || !mcba::sk_finite(in.lam)) return ck.bad("the damping must be finite and not negative");
  if (int rc = ck.pixel_std(in.pixel_std, in.C)) return rc;
  if (int rc = ck.forest(mcba::skel_plan(in.K, in.parent, in.bone_length, in.bone_std, plan))) return rc;
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
  if (int rc = upload_kp_cams(call, C, in.cam12, in.dist5, &d_cams)) return rc;
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
    mcba::kp_weight_box(in.weights, in.pixel_std, C, T, K, t0, tc, 0, K, h_sw.data());
    HIPCHK(hipMemcpy2D(d_det, 2 * tk * sizeof(double), in.uvs + 2 * t0 * K, 2 * T * K * sizeof(double), 2 * tk * sizeof(double), (size_t)C, hipMemcpyHostToDevice));
    if (int rc = call.put(d_sw, h_sw.data(), C * tk)) return rc;
    if (int rc = call.put(d_x, in.start + 3 * t0 * K, 3 * tk)) return rc;
    mcba::SkArgs a{};
    a.T = tc; a.det = d_det; a.sw = d_sw; a.start = d_x;
    a.fs2 = in.f_scale * in.f_scale; a.inv_fs2 = 1.0 / a.fs2; a.lam0 = in.lam; a.xtol = in.xtol;
    a.max_iterations = out.system ? 1 : in.max_iterations; a.system = out.system ? 1 : 0; a.cov = cov ? 1 : 0;
    a.points = d_pts; a.kstatus = d_kst; a.fstatus = d_fst; a.nit = d_nit; a.cost = d_cost; a.cost0 = d_cost0; a.bone_res = d_bres; a.info6 = d_info; a.dir = d_dir; a.cov6 = d_cov;
    a.grad = d_grad; a.step = d_step; a.data_cost = d_dc; a.bone_cost = d_bc; a.trial_cost = d_tc;
    if (int rc = call.open()) return rc;
    if (mcba::launch_skel_refine(nullptr, in.loss, a, d_plan, in.K, d_cams, C) != 0) return fail(MCBA_ERR_ARG, "skeleton refinement: bad launch");
    if (int rc = call.close(ms_total)) return rc;
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
  fill_info8(out.info8, out.kernel_ms, plan.levels, mcba::skel_frames_per_group(in.K), (double)Tc, (double)nchunks, ms_total, out.system ? 1 : most, (double)per_frame * (double)Tc, 0.0);
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
