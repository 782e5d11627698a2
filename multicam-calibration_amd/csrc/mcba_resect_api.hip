// mcba_resect_api.hip -- mcba_resect_ransac, mcba_resect_ransac_p3p and mcba_resect_refine of include/mcba.h (SURVEY.md sections 8f-16, 8f-18):
// stateless, host arrays in and out, a device ordinal, no handle.  The points, the detections and the samples go up once; the stages of
// csrc/mcba_resect.hip run on that copy, each between two events; the two RANSAC entries are one body (resect_ransac) that differs in the
// generator it launches: k_rs_hypotheses, or k_rs3_hypotheses of csrc/mcba_resect_p3p.hip with four table rows per sample.
// Cameras with fewer than six usable points are left out before anything is uploaded: the kernels see the others, packed.
// The polish's loop is rs_lm of mcba_resect_math.h, driven here against the kernels: one launch pair and one small copy back per evaluation.
#include "mcba_handle.h"
#include "mcba_ransac_host.h"
#include "mcba_resect_math.h"

using namespace mcba_internal;

namespace {

// one evaluation of the listed cameras on the device (rs_lm's back end)
struct ResectBackEnd {
  StatelessCall& call;
  int loss;
  size_t P;
  double f_scale;
  const double *cam12, *dist5;
  const double *d_pts, *d_uv;
  const unsigned char* d_mask;
  int* d_ids;
  mcba::TcCam* d_tcs;
  double *d_part, *d_sys;
  int evaluations = 0;
  std::vector<mcba::TcCam> tcs;
  std::vector<double> sys;

  int evaluate(bool cost_only, int n, const int* ids, const double* poses6) {
    tcs.resize((size_t)n);
    for (int k = 0; k < n; ++k) {
      double cam[12];
      for (int i = 0; i < 6; ++i) { cam[i] = cam12[12 * (size_t)ids[k] + i]; cam[6 + i] = poses6[6 * k + i]; }
      mcba::make_tc_cam(cam, dist5 + 5 * (size_t)ids[k], tcs[(size_t)k]);
    }
    if (int rc = call.put(d_ids, ids, (size_t)n)) return rc;
    if (int rc = call.put(d_tcs, tcs.data(), (size_t)n)) return rc;
    if (mcba::launch_rs_normal(nullptr, loss, cost_only, d_pts, d_uv, d_mask, P, n, d_ids, d_tcs, f_scale, d_part, d_sys) != 0) return fail(MCBA_ERR_ARG, "mcba_resect_refine: unknown loss");
    if (int rc = check_launch()) return rc;
    sys.resize((size_t)n * mcba::kRsSys);
    ++evaluations;
    return call.download(sys.data(), d_sys, (size_t)n * mcba::kRsSys);
  }
  int normal(int n, const int* ids, const double* poses6, double* out) {
    if (int rc = evaluate(false, n, ids, poses6)) return rc;
    for (size_t i = 0; i < sys.size(); ++i) out[i] = sys[i];
    return 0;
  }
  int trial(int n, const int* ids, const double* poses6, double* cost) {
    if (int rc = evaluate(true, n, ids, poses6)) return rc;
    for (int k = 0; k < n; ++k) cost[k] = sys[(size_t)k * mcba::kRsSys + 27];
    return 0;
  }
};

constexpr mcba::Generator kDlt6{"mcba_resect_ransac", MCBA_RESECT_SAMPLE, 1, MCBA_RESECT_MAX_HYPOTHESES, ": 1 .. MCBA_RESECT_MAX_HYPOTHESES (4096) hypotheses required"};
constexpr mcba::Generator kP3p{"mcba_resect_ransac_p3p", MCBA_RESECT_P3P_SAMPLE, MCBA_RESECT_P3P_SLOTS, MCBA_RESECT_P3P_MAX_SAMPLES, ": 1 .. MCBA_RESECT_P3P_MAX_SAMPLES (1024) samples required"};

// The body of mcba_resect_ransac and mcba_resect_ransac_p3p: the checks, the upload, the stages between their events, the download.
// n_hypotheses counts samples; the table that the scorer sees has H = n_hypotheses g.slots rows per camera.
int resect_ransac(const mcba::Generator& g, int n_cameras, size_t n_points, const double* points, const double* uvs, const double* cam12, const double* dist5, int n_hypotheses, const int* samples,
                  const double* poses_in, double threshold, int undistort_iterations, int device, double* rt12, double* best4, unsigned char* inliers, double* pose_out, double* cost_out,
                  unsigned* count_out, int* status_out, double* kernel_ms) {
  auto bad = [&](const char* what) { return fail(MCBA_ERR_ARG, (std::string(g.who) + what).c_str()); };
  if (!points || !uvs || !cam12 || !dist5 || !rt12 || !best4 || !inliers || (!samples && !poses_in) || undistort_iterations < 0)
    return bad(g.slots == 1 ? ": non-NULL arrays (samples or poses_in), undistort_iterations >= 0 required" : ": non-NULL arrays, undistort_iterations >= 0 required");
  if (n_cameras < 1 || n_cameras > MCBA_RESECT_MAX_CAMERAS) return bad(": 1 .. MCBA_RESECT_MAX_CAMERAS (64) cameras required");
  if (n_points < 1) return bad(": at least one point required");
  if (n_hypotheses < 1 || n_hypotheses > g.max_h) return bad(g.range);
  if (!(threshold > 0.0)) return bad(": threshold (pixels) must be positive");
  const int C = n_cameras, S = n_hypotheses, H = S * g.slots;
  const size_t P = n_points;
  // the usable points of every camera; the cameras that take part
  std::vector<unsigned char> use((size_t)C * P);
  std::vector<size_t> n_use((size_t)C, 0);
  std::vector<int> act;
  for (int c = 0; c < C; ++c) {
    for (size_t p = 0; p < P; ++p) {
      const bool ok = mcba::rs_usable(points[3 * p], points[3 * p + 1], points[3 * p + 2], uvs[2 * ((size_t)c * P + p)], uvs[2 * ((size_t)c * P + p) + 1]);
      use[(size_t)c * P + p] = ok;
      n_use[c] += ok;
    }
    if (n_use[c] >= (size_t)MCBA_RESECT_SAMPLE) act.push_back(c);
  }
  std::string msg;
  if (!poses_in)
    for (int c : act)
      if (!mcba::samples_ok(g.who, samples + (size_t)g.size * S * c, (size_t)S, g.size, P, use.data() + (size_t)c * P, &msg)) return fail(MCBA_ERR_ARG, msg.c_str());
  if (int rc = stateless_device(device)) return rc;
  const double nan = __builtin_nan("");
  for (int c = 0; c < C; ++c) {
    for (int i = 0; i < 12; ++i) rt12[12 * (size_t)c + i] = nan;
    best4[4 * (size_t)c] = -1.0; best4[4 * (size_t)c + 1] = nan; best4[4 * (size_t)c + 2] = 0.0; best4[4 * (size_t)c + 3] = (double)n_use[c];
    for (size_t p = 0; p < P; ++p) inliers[(size_t)c * P + p] = 0;
    for (size_t i = (size_t)c * H; i < (size_t)(c + 1) * H; ++i) {
      if (pose_out) for (int k = 0; k < 12; ++k) pose_out[12 * i + k] = nan;
      if (cost_out) cost_out[i] = nan;
      if (count_out) count_out[i] = 0u;
      if (status_out) status_out[i] = mcba::RS_VOID;
    }
  }
  if (kernel_ms) for (int i = 0; i < 6; ++i) kernel_ms[i] = 0.0;
  const int Ca = (int)act.size();
  if (Ca == 0) return MCBA_OK;
  // the cameras that take part, packed
  std::vector<double> cams9((size_t)Ca * 9);
  for (int a = 0; a < Ca; ++a) {
    for (int i = 0; i < 4; ++i) cams9[9 * (size_t)a + i] = cam12[12 * (size_t)act[a] + i];
    for (int i = 0; i < 5; ++i) cams9[9 * (size_t)a + 4 + i] = dist5[5 * (size_t)act[a] + i];
  }
  const size_t nblk = mcba::hyp_score_blocks(P);
  StatelessCall call;
  double *d_pts = nullptr, *d_uv = nullptr, *d_cams = nullptr, *d_pin = nullptr, *d_prep = nullptr, *d_pose = nullptr, *d_KP = nullptr, *d_pc = nullptr, *d_cost = nullptr, *d_best = nullptr,
         *d_rt = nullptr;
  int *d_smp = nullptr, *d_st = nullptr, *d_win = nullptr;
  unsigned *d_pn = nullptr, *d_cnt = nullptr;
  unsigned char *d_use = nullptr, *d_inl = nullptr;
  if (int rc = call.upload(&d_pts, points, 3 * P)) return rc;
  if (int rc = call.scratch(&d_uv, 2 * P * Ca)) return rc;
  for (int a = 0; a < Ca; ++a)
    if (int rc = call.put(d_uv + 2 * P * a, uvs + 2 * P * (size_t)act[a], 2 * P)) return rc;
  if (int rc = call.upload(&d_cams, cams9.data(), cams9.size())) return rc;
  const size_t HH = (size_t)H;
  if (poses_in) {
    if (int rc = call.scratch(&d_pin, 12 * HH * Ca)) return rc;
    for (int a = 0; a < Ca; ++a)
      if (int rc = call.put(d_pin + 12 * HH * a, poses_in + 12 * HH * act[a], 12 * HH)) return rc;
  } else {
    const size_t per = (size_t)g.size * S;   // indices per camera
    if (int rc = call.scratch(&d_smp, per * Ca)) return rc;
    for (int a = 0; a < Ca; ++a)
      if (int rc = call.put(d_smp + per * a, samples + per * act[a], per)) return rc;
  }
  if (int rc = call.scratch(&d_prep, 4 * P * Ca)) return rc;
  if (int rc = call.scratch(&d_use, P * Ca)) return rc;
  if (int rc = call.scratch(&d_pose, 12 * HH * Ca)) return rc;
  if (int rc = call.scratch(&d_KP, 12 * HH * Ca)) return rc;
  if (int rc = call.scratch(&d_st, HH * Ca)) return rc;
  if (int rc = call.scratch(&d_pc, nblk * HH * Ca)) return rc;
  if (int rc = call.scratch(&d_pn, nblk * HH * Ca)) return rc;
  if (int rc = call.scratch(&d_cost, HH * Ca)) return rc;
  if (int rc = call.scratch(&d_cnt, HH * Ca)) return rc;
  if (int rc = call.scratch(&d_win, (size_t)Ca)) return rc;
  if (int rc = call.scratch(&d_best, (size_t)4 * Ca)) return rc;
  if (int rc = call.scratch(&d_rt, (size_t)12 * Ca)) return rc;
  if (int rc = call.scratch(&d_inl, P * Ca)) return rc;
  StageEvents<4> stages;   // the call's own events bracket the whole; four more separate the stages
  HIPCHK(stages.create());
  HIPCHK(call.start());
  mcba::launch_rs_prepare(nullptr, d_pts, d_uv, P, Ca, d_cams, undistort_iterations, d_prep, d_use);
  if (int rc = check_launch()) return rc;
  HIPCHK(stages.mark());
  if (g.slots == 1) mcba::launch_rs_hypotheses(nullptr, d_pts, d_prep, P, Ca, d_smp, H, d_pin, d_cams, d_pose, d_KP, d_st);
  else mcba::launch_rs3_hypotheses(nullptr, d_pts, d_prep, P, Ca, d_smp, S, d_cams, d_pose, d_KP, d_st);
  if (int rc = check_launch()) return rc;
  HIPCHK(stages.mark());
  mcba::launch_rs_score(nullptr, d_pts, d_prep, d_use, P, Ca, d_KP, H, threshold, d_pc, d_pn);
  if (int rc = check_launch()) return rc;
  HIPCHK(stages.mark());
  mcba::launch_rs_finish(nullptr, d_pc, d_pn, nblk, Ca, H, d_pose, d_st, d_cost, d_cnt, d_win, d_best, d_rt);
  if (int rc = check_launch()) return rc;
  HIPCHK(stages.mark());
  mcba::launch_rs_mask(nullptr, d_pts, d_prep, d_use, P, Ca, d_KP, d_st, H, threshold, d_win, d_inl);
  if (int rc = check_launch()) return rc;
  double total = 0.0;
  HIPCHK(call.stop(&total));
  if (kernel_ms) HIPCHK(stages.fill(call, total, kernel_ms));
  for (int a = 0; a < Ca; ++a) {
    const size_t c = (size_t)act[a];
    double b4[4];
    if (int rc = call.download(rt12 + 12 * c, d_rt + 12 * a, (size_t)12)) return rc;
    if (int rc = call.download(b4, d_best + 4 * a, (size_t)4)) return rc;
    for (int i = 0; i < 3; ++i) best4[4 * c + i] = b4[i];
    if (int rc = call.download(inliers + c * P, d_inl + P * a, P)) return rc;
    if (pose_out)
      if (int rc = call.download(pose_out + 12 * HH * c, d_pose + 12 * HH * a, 12 * HH)) return rc;
    if (cost_out)
      if (int rc = call.download(cost_out + HH * c, d_cost + HH * a, HH)) return rc;
    if (count_out)
      if (int rc = call.download(count_out + HH * c, d_cnt + HH * a, HH)) return rc;
    if (status_out)
      if (int rc = call.download(status_out + HH * c, d_st + HH * a, HH)) return rc;
  }
  return MCBA_OK;
}

}  // namespace

extern "C" {

int mcba_resect_ransac(int n_cameras, size_t n_points, const double* points, const double* uvs, const double* cam12, const double* dist5, int n_hypotheses, const int* samples,
                       const double* poses_in, double threshold, int undistort_iterations, int device, double* rt12, double* best4, unsigned char* inliers, double* pose_out, double* cost_out,
                       unsigned* count_out, int* status_out, double* kernel_ms) {
  return resect_ransac(kDlt6, n_cameras, n_points, points, uvs, cam12, dist5, n_hypotheses, samples, poses_in, threshold, undistort_iterations, device, rt12, best4, inliers, pose_out, cost_out,
                       count_out, status_out, kernel_ms);
}

int mcba_resect_ransac_p3p(int n_cameras, size_t n_points, const double* points, const double* uvs, const double* cam12, const double* dist5, int n_hypotheses, const int* samples,
                           double threshold, int undistort_iterations, int device, double* rt12, double* best4, unsigned char* inliers, double* pose_out, double* cost_out, unsigned* count_out,
                           int* status_out, double* kernel_ms) {
  return resect_ransac(kP3p, n_cameras, n_points, points, uvs, cam12, dist5, n_hypotheses, samples, nullptr, threshold, undistort_iterations, device, rt12, best4, inliers, pose_out, cost_out,
                       count_out, status_out, kernel_ms);
}

int mcba_resect_refine(int n_cameras, size_t n_points, const double* points, const double* uvs, const unsigned char* mask, const double* cam12, const double* dist5, const int* active, int loss,
                       double f_scale, double ftol, double xtol, double gtol, int max_nfev, int device, double* extrinsics_out, double* result, double* system_out, double* kernel_ms) {
  if (!points || !uvs || !mask || !cam12 || !dist5 || !extrinsics_out || !result) return fail(MCBA_ERR_ARG, "mcba_resect_refine: non-NULL arrays required");
  if (n_cameras < 1 || n_cameras > MCBA_RESECT_MAX_CAMERAS) return fail(MCBA_ERR_ARG, "mcba_resect_refine: 1 .. MCBA_RESECT_MAX_CAMERAS (64) cameras required");
  if (n_points < 1) return fail(MCBA_ERR_ARG, "mcba_resect_refine: at least one point required");
  if (loss < mcba::LOSS_LINEAR || loss > mcba::LOSS_ARCTAN) return fail(MCBA_ERR_ARG, "mcba_resect_refine: loss must be one of linear, soft_l1, huber, cauchy, arctan (0 .. 4)");
  if (!(f_scale > 0.0)) return fail(MCBA_ERR_ARG, "mcba_resect_refine: f_scale must be positive");
  if (max_nfev < 1) return fail(MCBA_ERR_ARG, "mcba_resect_refine: max_nfev must be at least 1");
  if (int rc = stateless_device(device)) return rc;
  const int C = n_cameras;
  const size_t P = n_points, nblk = mcba::hyp_point_blocks(P);
  std::vector<mcba::RsCamera> cams((size_t)C);
  int n_act = 0;
  for (int c = 0; c < C; ++c) {
    for (int i = 0; i < 6; ++i) cams[c].pose[i] = cam12[12 * (size_t)c + 6 + i];
    for (int i = 0; i < mcba::kRsSys; ++i) cams[c].sys[i] = __builtin_nan("");
    cams[c].status = (!active || active[c]) ? -1 : -2;   // (-2: takes no part)
    n_act += cams[c].status == -1;
  }
  double span = 0.0;
  int evaluations = 0;
  if (n_act > 0) {
    StatelessCall call;
    double *d_pts = nullptr, *d_uv = nullptr, *d_part = nullptr, *d_sys = nullptr;
    unsigned char* d_mask = nullptr;
    int* d_ids = nullptr;
    mcba::TcCam* d_tcs = nullptr;
    if (int rc = call.upload(&d_pts, points, 3 * P)) return rc;
    if (int rc = call.upload(&d_uv, uvs, 2 * P * C)) return rc;
    if (int rc = call.upload(&d_mask, mask, P * C)) return rc;
    if (int rc = call.scratch(&d_ids, (size_t)C)) return rc;
    if (int rc = call.scratch(&d_tcs, (size_t)C)) return rc;
    if (int rc = call.scratch(&d_part, nblk * mcba::kRsSys * C)) return rc;
    if (int rc = call.scratch(&d_sys, (size_t)mcba::kRsSys * C)) return rc;
    ResectBackEnd be{call, loss, P, f_scale, cam12, dist5, d_pts, d_uv, d_mask, d_ids, d_tcs, d_part, d_sys};
    const mcba::KbOptions opt{ftol, xtol, gtol, max_nfev};
    HIPCHK(call.start());
    if (int rc = mcba::rs_lm(be, C, cams.data(), opt)) return rc;
    HIPCHK(call.stop(&span));
    evaluations = be.evaluations;
  }
  const double nan = __builtin_nan("");
  for (int c = 0; c < C; ++c) {
    const mcba::RsCamera& cm = cams[c];
    const bool on = cm.status != -2;
    for (int i = 0; i < 6; ++i) extrinsics_out[6 * (size_t)c + i] = cm.pose[i];
    double* r = result + 8 * (size_t)c;
    r[0] = on ? cm.cost0 : nan; r[1] = on ? cm.cost : nan; r[2] = on ? cm.optimality : nan; r[3] = on ? cm.nfev : nan; r[4] = on ? cm.njev : nan;
    r[5] = on ? cm.status : nan; r[6] = on ? cm.sys[28] : nan; r[7] = on ? cm.lam : nan;
    if (system_out)
      for (int i = 0; i < mcba::kRsSys; ++i) system_out[(size_t)mcba::kRsSys * c + i] = cm.sys[i];
  }
  if (kernel_ms) { kernel_ms[0] = span; kernel_ms[1] = (double)evaluations; }
  return MCBA_OK;
}

}  // extern "C"
