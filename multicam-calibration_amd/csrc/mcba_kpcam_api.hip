// mcba_kpcam_api.hip -- the stateless camera-refinement call of include/mcba.h, in the idiom of mcba_kpba_api.hip: host
// arrays in, host arrays out, a device ordinal, no handle; one upload of the detections and their weights, then the whole Levenberg-Marquardt loop
// (kpcam_lm, mcba_kpcam_math.h) with the kernels of mcba_kpcam.hip as its back end.  Per evaluation the camera tables go up (60 C doubles, rebuilt
// from the 12 scalars of every camera: trial intrinsics and extrinsics alike) and the reduced system comes down (NP^2 + 102 C + 4 doubles); the
// dense solve and the prior on the intrinsics are the host's.  The loop ends at the first HIP error and starts nothing after it.
// mcba_refine_cameras_system is one evaluation of that loop laid open: the same refusals, set-up and back end, and what the kernels wrote
// handed back as it is.
#include "mcba_handle.h"
#include "mcba_kpcam_math.h"

using namespace mcba_internal;

namespace {

struct CameraBackEnd {
  StatelessCall& call;
  const char* who;   // the entry point, for messages
  int C, loss, G;
  size_t P;
  double f_scale;
  const double* dist5;   // p1, p2, k3 of every camera (or NULL: zero); k1, k2 come with the 12 scalars
  double* d_uv = nullptr;
  double* d_sw = nullptr;   // the plane of sqrt(weight), or nullptr: the unweighted kernels
  double* d_pts[2] = {nullptr, nullptr};
  int* d_status = nullptr;
  int* d_held = nullptr;
  mcba::TcCam* d_cams = nullptr;   // current table | trial table
  double *d_dth = nullptr, *d_part = nullptr, *d_sys = nullptr, *d_part4 = nullptr, *d_out4 = nullptr;
  int cur = 0;
  std::vector<mcba::TcCam> tab;   // 2 C
  std::vector<double> host_sys;   // the system of the last reduce, as k_kpba_finish left it
  double out4[4] = {0.0, 0.0, 0.0, 0.0};   // the four scalars of the last step, likewise
  double status_ms = 0.0, reduce_ms = 0.0, step_ms = 0.0;
  int n_reduce = 0, n_step = 0;

  int launch_failed(const char* what) const {
    g_err = std::string(who) + ": " + what;
    return MCBA_ERR_HIP;
  }
  int timed(double* ms_sum) {   // after a launch between the two records
    HIPCHK(hipEventRecord(call.e1, nullptr));
    HIPCHK(hipEventSynchronize(call.e1));
    if (int rc = check_launch()) return rc;
    float ms = 0.f;
    HIPCHK(hipEventElapsedTime(&ms, call.e0, call.e1));
    *ms_sum += ms;
    return MCBA_OK;
  }
  int reduce(const double* theta, double lam, mcba::KcSystem& sys) {
    mcba::kpcam_table(C, theta, dist5, tab.data());
    if (int rc = call.put(d_cams, tab.data(), (size_t)C)) return rc;
    HIPCHK(hipEventRecord(call.e0, nullptr));
    if (mcba::launch_kpcam_reduce(nullptr, loss, d_uv, d_pts[cur], d_status, P, d_cams, d_held, C, f_scale, lam, G, d_part, d_sys, d_sw) != 0) return launch_failed("k_kpcam_reduce could not be launched");
    if (int rc = timed(&reduce_ms)) return rc;
    ++n_reduce;
    const size_t PS = mcba::kpcam_partial_size(C);
    host_sys.resize(PS);
    if (int rc = call.download(host_sys.data(), d_sys, PS)) return rc;
    sys.shape(C);
    const size_t nyy = (size_t)sys.NP * sys.NP;
    std::copy(host_sys.begin(), host_sys.begin() + nyy, sys.YY.begin());
    std::copy(host_sys.begin() + nyy, host_sys.begin() + nyy + sys.acc.size(), sys.acc.begin());
    sys.cost = host_sys[PS - 4]; sys.count = host_sys[PS - 3]; sys.gmax = host_sys[PS - 2];
    return MCBA_OK;
  }
  int step(const double* theta_trial, const double* dtheta, double lam, double out[3]) {
    mcba::kpcam_table(C, theta_trial, dist5, tab.data() + C);
    if (int rc = call.put(d_cams + C, tab.data() + C, (size_t)C)) return rc;
    if (int rc = call.put(d_dth, dtheta, (size_t)mcba::kKcRows * C)) return rc;
    HIPCHK(hipEventRecord(call.e0, nullptr));
    if (mcba::launch_kpcam_step(nullptr, loss, d_uv, d_pts[cur], d_pts[1 - cur], d_status, P, d_cams, d_dth, C, f_scale, lam, d_part4, d_out4, d_sw) != 0)
      return launch_failed("k_kpcam_step could not be launched");
    if (int rc = timed(&step_ms)) return rc;
    ++n_step;
    if (int rc = call.download(out4, d_out4, (size_t)4)) return rc;
    out[0] = out4[0]; out[1] = out4[1]; out[2] = out4[3];
    return MCBA_OK;
  }
  void accept() { cur = 1 - cur; }
  // the detections, their weights (or NULL), both point buffers and the camera tables (at theta) up, the scratch of a pass, then k_kpba_status: point_status (P) on the host
  int setup(const double* uvs, const double* weights, const double* points, const double* theta, int* point_status) {
    tab.resize((size_t)2 * C);
    mcba::kpcam_table(C, theta, dist5, tab.data());
    mcba::kpcam_table(C, theta, dist5, tab.data() + C);
    const int nwg = mcba::kpba_groups(P);
    if (int rc = call.upload(&d_uv, uvs, (size_t)2 * C * P)) return rc;
    if (int rc = upload_sqrt_weights(call, weights, (size_t)C * P, &d_sw)) return rc;
    if (int rc = call.upload(&d_pts[0], points, 3 * P)) return rc;
    if (int rc = call.upload(&d_pts[1], points, 3 * P)) return rc;
    if (int rc = call.upload(&d_cams, tab.data(), tab.size())) return rc;
    if (int rc = call.scratch(&d_status, P)) return rc;
    if (int rc = call.scratch(&d_held, (size_t)C)) return rc;
    if (int rc = call.scratch(&d_dth, (size_t)mcba::kKcRows * C)) return rc;
    if (int rc = call.scratch(&d_part, (size_t)nwg * mcba::kpcam_partial_size(C))) return rc;
    if (int rc = call.scratch(&d_sys, mcba::kpcam_partial_size(C))) return rc;
    if (int rc = call.scratch(&d_part4, (size_t)4 * nwg)) return rc;
    if (int rc = call.scratch(&d_out4, (size_t)4)) return rc;
    HIPCHK(call.start());
    if (mcba::launch_kpba_status(nullptr, d_uv, d_pts[0], P, d_cams, C, d_status, d_sw, false) != 0) {
      g_err = std::string(who) + ": bad launch (k_kpba_status)";
      return MCBA_ERR_ARG;
    }
    if (int rc = timed(&status_ms)) return rc;
    return call.download(point_status, d_status, P);
  }
};

// what both entry points refuse alike
int kpcam_refuse(const char* who, int n_cameras, size_t n_points, int loss, double f_scale) {
  const char* why = nullptr;
  if (n_cameras < 2 || n_cameras > mcba::kKcMaxCams)
    why = "2 to 12 cameras (12 scalars per camera hold the reduced system to 144 rows: nine matrix-core tiles; mcba_refine_extrinsics_reduction with MCBA_KPBA_TILED takes up to 64 for the extrinsics alone)";
  else if (loss < mcba::LOSS_LINEAR || loss > mcba::LOSS_ARCTAN) why = "loss must be one of linear, soft_l1, huber, cauchy, arctan (0 .. 4)";
  else if (!(f_scale > 0.0)) why = "f_scale must be positive";
  else if (n_points == 0) why = "no points";
  if (!why) return MCBA_OK;
  g_err = std::string(who) + ": " + why;
  return MCBA_ERR_ARG;
}

// points per group of k_kpcam_reduce on this device; MCBA_KPCAM_G (test knob) forces the smaller groups at any size
int kpcam_pick_group(const char* who, int C, int device, int* G) {
  int force_g = 0;
  if (const char* e = getenv("MCBA_KPCAM_G")) force_g = atoi(e);
  *G = mcba::kpcam_group(C, lds_optin_of(device), force_g);
  if (*G) return MCBA_OK;
  g_err = std::string(who) + ": k_kpcam_reduce does not fit the LDS of this device";
  return MCBA_ERR_HIP;
}

// the 12 scalars of every camera as the loop moves them: cam12 with k1, k2 from dist5 where it is given (as make_kp_cam reads them)
void kpcam_theta(int C, const double* cam12, const double* dist5, std::vector<double>& theta) {
  theta.assign(cam12, cam12 + (size_t)12 * C);
  if (dist5)
    for (int c = 0; c < C; ++c) { theta[12 * c + 4] = dist5[5 * c]; theta[12 * c + 5] = dist5[5 * c + 1]; }
}

}  // namespace

extern "C" {

int mcba_refine_cameras(int n_cameras, size_t n_points, const double* uvs, const double* weights, const double* cam12, const double* dist5, const double* points, int* held, const double* prior_weight,
                        int gauge_camera, int scale_camera, int loss, double f_scale, double ftol, double xtol, double gtol, int max_nfev, int device, double* cameras_out, double* points_out,
                        int* point_status, double* result16, double* history, int history_rows) {
  const char* who = "mcba_refine_cameras";
  if (int rc = kpcam_refuse(who, n_cameras, n_points, loss, f_scale)) return rc;
  if (!uvs || !cam12 || !points || !held || !cameras_out || !points_out || !point_status || !result16 || (history_rows > 0 && !history))
    return fail(MCBA_ERR_ARG, "mcba_refine_cameras: non-NULL arrays required");
  if (gauge_camera < 0 || gauge_camera >= n_cameras || scale_camera < 0 || scale_camera >= n_cameras || gauge_camera == scale_camera)
    return fail(MCBA_ERR_ARG, "mcba_refine_cameras: gauge_camera and scale_camera must be two different cameras of the rig");
  if (max_nfev < 2) return fail(MCBA_ERR_ARG, "mcba_refine_cameras: max_nfev must be at least 2 (the start and one trial)");
  if (!(ftol >= 0.0 && xtol >= 0.0 && gtol >= 0.0)) return fail(MCBA_ERR_ARG, "mcba_refine_cameras: ftol, xtol, gtol must not be negative");
  const int C = n_cameras;
  const size_t P = n_points;
  if (prior_weight)
    for (int k = 0; k < 6 * C; ++k)
      if (!(prior_weight[k] >= 0.0 && prior_weight[k] <= 1.79e308)) return fail(MCBA_ERR_ARG, "mcba_refine_cameras: prior_weight (1 / std^2) must be finite and not negative (0: no prior on that scalar)");
  if (int rc = check_weights(who, weights, (size_t)C * P)) return rc;
  for (int i = 0; i < 16; ++i) result16[i] = 0.0;
  if (int rc = stateless_device(device)) return rc;
  int G = 0;
  if (int rc = kpcam_pick_group(who, C, device, &G)) return rc;

  StatelessCall call;
  CameraBackEnd be{call, who, C, loss, G, P, f_scale, dist5};
  std::vector<double> theta;
  kpcam_theta(C, cam12, dist5, theta);
  if (int rc = be.setup(uvs, weights, points, theta.data(), point_status)) return rc;
  for (int c = 0; c < C; ++c) {   // a camera that no used point sees (with a positive weight) is held whole, all 12 scalars
    bool seen = false;
    const double* u = uvs + (size_t)2 * c * P;
    const double* w = weights ? weights + (size_t)c * P : nullptr;
    for (size_t p = 0; p < P && !seen; ++p) seen = point_status[p] == mcba::KB_USED && u[2 * p] == u[2 * p] && u[2 * p + 1] == u[2 * p + 1] && (!w || w[p] > 0.0);
    if (!seen) held[c] = mcba::kKcHeldAll;
    held[c] &= mcba::kKcHeldAll;
  }
  if ((held[scale_camera] & 0xFC0) == 0xFC0) return fail(MCBA_ERR_ARG, "mcba_refine_cameras: scale_camera sees no used point (or its extrinsics are held whole): nothing fixes the scale of the rig");
  held[gauge_camera] |= 0xFC0;
  if (int rc = call.put(be.d_held, held, (size_t)C)) return rc;

  const double baseline = mcba::kpcam_baseline(C, theta.data(), gauge_camera, scale_camera);
  const mcba::KbOptions opt{ftol, xtol, gtol, max_nfev};
  mcba::KcResult res;
  if (int rc = mcba::kpcam_lm(be, C, held, theta.data(), prior_weight, opt, res, history, history_rows)) return rc;

  if (int rc = call.download(points_out, be.d_pts[be.cur], 3 * P)) return rc;
  const double nan = __builtin_nan("");
  for (size_t p = 0; p < P; ++p)
    if (point_status[p] != mcba::KB_USED) points_out[3 * p] = points_out[3 * p + 1] = points_out[3 * p + 2] = nan;
  const double s = mcba::kpcam_rescale(C, held, theta.data(), P, points_out, gauge_camera, scale_camera, baseline);
  for (int k = 0; k < 12 * C; ++k) cameras_out[k] = theta[k];
  result16[0] = res.cost; result16[1] = res.cost0; result16[2] = res.optimality; result16[3] = res.nfev; result16[4] = res.njev; result16[5] = res.status; result16[6] = s;
  result16[7] = res.nhist; result16[8] = be.status_ms + be.reduce_ms + be.step_ms; result16[9] = be.reduce_ms; result16[10] = be.n_reduce; result16[11] = be.step_ms; result16[12] = be.n_step;
  result16[13] = G; result16[14] = res.prior_cost;
  return MCBA_OK;
}

int mcba_refine_cameras_system(int n_cameras, size_t n_points, const double* uvs, const double* weights, const double* cam12, const double* dist5, const double* points, const int* held, int loss,
                               double f_scale, double lam, int device, const double* cameras_trial, const double* dtheta, int* point_status, double* system, double* trial_points, double* step4,
                               double* info4) {
  const char* who = "mcba_refine_cameras_system";
  if (int rc = kpcam_refuse(who, n_cameras, n_points, loss, f_scale)) return rc;
  const bool stepping = cameras_trial || dtheta;
  if (!uvs || !cam12 || !points || !held || !point_status || !system || !info4 || (stepping && (!cameras_trial || !dtheta || !trial_points || !step4)))
    return fail(MCBA_ERR_ARG, "mcba_refine_cameras_system: non-NULL arrays required (cameras_trial and dtheta both or neither; with them trial_points and step4)");
  if (!(lam >= 0.0 && lam < mcba::KB_LAMBDA_MAX)) return fail(MCBA_ERR_ARG, "mcba_refine_cameras_system: lam must be in [0, 1e12)");
  if (int rc = check_weights(who, weights, (size_t)n_cameras * n_points)) return rc;
  if (int rc = stateless_device(device)) return rc;
  const int C = n_cameras;
  const size_t P = n_points;
  int G = 0;
  if (int rc = kpcam_pick_group(who, C, device, &G)) return rc;

  StatelessCall call;
  CameraBackEnd be{call, who, C, loss, G, P, f_scale, dist5};
  std::vector<double> theta;
  kpcam_theta(C, cam12, dist5, theta);
  if (int rc = be.setup(uvs, weights, points, theta.data(), point_status)) return rc;
  std::vector<int> h(held, held + C);
  for (int& v : h) v &= mcba::kKcHeldAll;
  if (int rc = call.put(be.d_held, h.data(), (size_t)C)) return rc;   // (as given: no gauge, no scale, no blind-camera rule here)
  mcba::KcSystem sys;
  if (int rc = be.reduce(theta.data(), lam, sys)) return rc;
  std::copy(be.host_sys.begin(), be.host_sys.end(), system);
  if (stepping) {
    double out[3];
    if (int rc = be.step(cameras_trial, dtheta, lam, out)) return rc;
    if (int rc = call.download(trial_points, be.d_pts[1 - be.cur], 3 * P)) return rc;
    for (int k = 0; k < 4; ++k) step4[k] = be.out4[k];
  }
  info4[0] = G; info4[1] = mcba::kpba_groups(P); info4[2] = sys.NP; info4[3] = be.status_ms + be.reduce_ms + be.step_ms;
  return MCBA_OK;
}

}  // extern "C"
