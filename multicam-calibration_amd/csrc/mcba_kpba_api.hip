// mcba_kpba_api.hip -- the stateless extrinsics-refinement call of include/mcba.h (host arrays in, host arrays out, a device ordinal, no handle),
// in the idiom of mcba_geom_api.hip: one upload of the detections, then the whole Levenberg-Marquardt loop (kpba_lm, mcba_kpba_math.h) with the
// kernels of mcba_kpba.hip -- or, with reduction = MCBA_KPBA_TILED, the reduce of mcba_kpba_tiled.hip (2 to 64 cameras) -- as its back end.  Per
// evaluation the camera tables go up (60 C doubles) and the reduced system comes down (NP^2 + 33 C + 4 doubles); the dense solve is the host's.  The loop ends at the first HIP error and starts nothing after it.
// mcba_refine_extrinsics_system is one evaluation of that loop laid open: the same refusals, set-up and back end (kpba_refuse, kpba_pick_group,
// DeviceBackEnd::setup / reduce / step below), and what the kernels wrote handed back as it is.
#include "mcba_handle.h"
#include "mcba_kpba_math.h"

using namespace mcba_internal;

namespace {

struct DeviceBackEnd {
  StatelessCall& call;
  const char* who;   // the entry point, for messages
  int C, loss, G;
  bool tiled;   // the reduce of mcba_kpba_tiled.hip and the 64-camera tables of k_kpba_status and k_kpba_step
  size_t P;
  double f_scale;
  const double* cam12;
  const double* dist5;
  double* d_uv = nullptr;
  double* d_sw = nullptr;   // the plane of sqrt(weight), or nullptr: the unweighted kernels
  double* d_pts[2] = {nullptr, nullptr};
  int* d_status = nullptr;
  int* d_held = nullptr;
  mcba::TcCam* d_cams = nullptr;   // current table | trial table
  double *d_dth = nullptr, *d_part = nullptr, *d_sys = nullptr, *d_part4 = nullptr, *d_out4 = nullptr, *d_fac = nullptr;
  int cur = 0;
  std::vector<mcba::TcCam> tab;   // 2 C
  std::vector<double> host_sys;   // the system of the last reduce, as k_kpba_finish left it
  double out4[4] = {0.0, 0.0, 0.0, 0.0};   // the four scalars of the last step, likewise
  double status_ms = 0.0, reduce_ms = 0.0, step_ms = 0.0;
  int n_reduce = 0, n_step = 0;

  void table(const double* ext, mcba::TcCam* t) const {
    for (int c = 0; c < C; ++c) {
      double q[12];
      for (int k = 0; k < 6; ++k) { q[k] = cam12[12 * c + k]; q[6 + k] = ext[6 * c + k]; }
      mcba::make_tc_cam(q, dist5 ? dist5 + 5 * c : nullptr, t[c]);
    }
  }
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
  int reduce(const double* ext, double lam, mcba::KbSystem& sys) {
    table(ext, tab.data());
    if (int rc = call.put(d_cams, tab.data(), (size_t)C)) return rc;
    HIPCHK(hipEventRecord(call.e0, nullptr));
    if ((tiled ? mcba::launch_kpba_reduce_tiled(nullptr, loss, d_uv, d_pts[cur], d_status, P, d_cams, d_held, C, f_scale, lam, d_fac, d_part, d_sys, d_sw)
               : mcba::launch_kpba_reduce(nullptr, loss, d_uv, d_pts[cur], d_status, P, d_cams, d_held, C, f_scale, lam, G, d_part, d_sys, d_sw)) != 0)
      return launch_failed(tiled ? "k_kpba_reduce_tiled could not be launched" : "k_kpba_reduce could not be launched");
    if (int rc = timed(&reduce_ms)) return rc;
    ++n_reduce;
    const size_t PS = mcba::kpba_partial_size(C);
    host_sys.resize(PS);
    if (int rc = call.download(host_sys.data(), d_sys, PS)) return rc;
    sys.shape(C);
    const size_t nyy = (size_t)sys.NP * sys.NP;
    std::copy(host_sys.begin(), host_sys.begin() + nyy, sys.YY.begin());
    std::copy(host_sys.begin() + nyy, host_sys.begin() + nyy + sys.acc.size(), sys.acc.begin());
    sys.cost = host_sys[PS - 4]; sys.count = host_sys[PS - 3]; sys.gmax = host_sys[PS - 2];
    return MCBA_OK;
  }
  int step(const double* ext_trial, const double* dtheta, double lam, double out[3]) {
    table(ext_trial, tab.data() + C);
    if (int rc = call.put(d_cams + C, tab.data() + C, (size_t)C)) return rc;
    if (int rc = call.put(d_dth, dtheta, (size_t)6 * C)) return rc;
    HIPCHK(hipEventRecord(call.e0, nullptr));
    if (mcba::launch_kpba_step(nullptr, loss, d_uv, d_pts[cur], d_pts[1 - cur], d_status, P, d_cams, d_dth, C, f_scale, lam, d_part4, d_out4, d_sw, tiled) != 0)
      return launch_failed("k_kpba_step could not be launched");
    if (int rc = timed(&step_ms)) return rc;
    ++n_step;
    if (int rc = call.download(out4, d_out4, (size_t)4)) return rc;
    out[0] = out4[0]; out[1] = out4[1]; out[2] = out4[3];
    return MCBA_OK;
  }
  void accept() { cur = 1 - cur; }
  int partials() const { return tiled ? mcba::kpba_tiled_groups(C, P) : mcba::kpba_groups(P); }   // partial systems of a reduce
  // the detections, their weights (or NULL), both point buffers and the camera tables (at ext) up, the scratch of a pass, then k_kpba_status: point_status (P) on the host
  int setup(const double* uvs, const double* weights, const double* points, const double* ext, int* point_status) {
    tab.resize((size_t)2 * C);
    table(ext, tab.data());
    table(ext, tab.data() + C);
    const int nwg = mcba::kpba_groups(P);
    if (int rc = call.upload(&d_uv, uvs, (size_t)2 * C * P)) return rc;
    if (int rc = upload_sqrt_weights(call, weights, (size_t)C * P, &d_sw)) return rc;
    if (int rc = call.upload(&d_pts[0], points, 3 * P)) return rc;
    if (int rc = call.upload(&d_pts[1], points, 3 * P)) return rc;
    if (int rc = call.upload(&d_cams, tab.data(), tab.size())) return rc;
    if (int rc = call.scratch(&d_status, P)) return rc;
    if (int rc = call.scratch(&d_held, (size_t)C)) return rc;
    if (int rc = call.scratch(&d_dth, (size_t)6 * C)) return rc;
    if (int rc = call.scratch(&d_part, (size_t)partials() * mcba::kpba_partial_size(C))) return rc;
    if (tiled)
      if (int rc = call.scratch(&d_fac, (size_t)13 * P)) return rc;
    if (int rc = call.scratch(&d_sys, mcba::kpba_partial_size(C))) return rc;
    if (int rc = call.scratch(&d_part4, (size_t)4 * nwg)) return rc;
    if (int rc = call.scratch(&d_out4, (size_t)4)) return rc;
    HIPCHK(call.start());
    if (mcba::launch_kpba_status(nullptr, d_uv, d_pts[0], P, d_cams, C, d_status, d_sw, tiled) != 0) {
      g_err = std::string(who) + ": bad launch (k_kpba_status)";
      return MCBA_ERR_ARG;
    }
    if (int rc = timed(&status_ms)) return rc;
    return call.download(point_status, d_status, P);
  }
};

// what both entry points refuse alike
int kpba_refuse(const char* who, int n_cameras, size_t n_points, int loss, double f_scale, int reduction) {
  const char* why = nullptr;
  if (reduction != MCBA_KPBA_RESIDENT && reduction != MCBA_KPBA_TILED) why = "reduction must be MCBA_KPBA_RESIDENT (0) or MCBA_KPBA_TILED (1)";
  else if (reduction == MCBA_KPBA_TILED && (n_cameras < 2 || n_cameras > mcba::kKtMaxCams)) why = "2 to 64 cameras (the tiled reduction: four bands of 16 cameras)";
  else if (reduction == MCBA_KPBA_RESIDENT && (n_cameras < 2 || n_cameras > mcba::kKbMaxCams))
    why = "2 to 24 cameras (the resident reduction holds the reduced system to 144 rows: nine matrix-core tiles; reduction = MCBA_KPBA_TILED takes up to 64)";
  else if (loss < mcba::LOSS_LINEAR || loss > mcba::LOSS_ARCTAN) why = "loss must be one of linear, soft_l1, huber, cauchy, arctan (0 .. 4)";
  else if (!(f_scale > 0.0)) why = "f_scale must be positive";
  else if (n_points == 0) why = "no points";
  if (!why) return MCBA_OK;
  g_err = std::string(who) + ": " + why;
  return MCBA_ERR_ARG;
}

// points per group of k_kpba_reduce on this device; MCBA_KPBA_G (test knob) forces the smaller groups at any size
int kpba_pick_group(const char* who, int C, int device, int reduction, int* G) {
  if (reduction == MCBA_KPBA_TILED) {   // one shape for every C
    *G = mcba::kKtGroup;
    if (mcba::kpba_tiled_lds() + 8 * 1024 <= (size_t)lds_optin_of(device)) return MCBA_OK;
    g_err = std::string(who) + ": k_kpba_reduce_tiled does not fit the LDS of this device";
    return MCBA_ERR_HIP;
  }
  int force_g = 0;
  if (const char* e = getenv("MCBA_KPBA_G")) force_g = atoi(e);
  *G = mcba::kpba_group(C, lds_optin_of(device), force_g);
  if (*G) return MCBA_OK;
  g_err = std::string(who) + ": k_kpba_reduce does not fit the LDS of this device";
  return MCBA_ERR_HIP;
}

}  // namespace

extern "C" {

int mcba_refine_extrinsics(int n_cameras, size_t n_points, const double* uvs, const double* cam12, const double* dist5, const double* points, int* held, int gauge_camera, int scale_camera, int loss,
                           double f_scale, double ftol, double xtol, double gtol, int max_nfev, int device, double* extrinsics_out, double* points_out, int* point_status, double* result16,
                           double* history, int history_rows) {
  return mcba_refine_extrinsics_reduction(n_cameras, n_points, uvs, nullptr, MCBA_KPBA_RESIDENT, cam12, dist5, points, held, gauge_camera, scale_camera, loss, f_scale, ftol, xtol, gtol, max_nfev, device,
                                          extrinsics_out, points_out, point_status, result16, history, history_rows);
}

// weights NULL: the call above, launch for launch.  Otherwise the plane of sqrt(w) goes up once beside the detections and the weighted kernels run.
int mcba_refine_extrinsics_weighted(int n_cameras, size_t n_points, const double* uvs, const double* weights, const double* cam12, const double* dist5, const double* points, int* held,
                                    int gauge_camera, int scale_camera, int loss, double f_scale, double ftol, double xtol, double gtol, int max_nfev, int device, double* extrinsics_out,
                                    double* points_out, int* point_status, double* result16, double* history, int history_rows) {
  return mcba_refine_extrinsics_reduction(n_cameras, n_points, uvs, weights, MCBA_KPBA_RESIDENT, cam12, dist5, points, held, gauge_camera, scale_camera, loss, f_scale, ftol, xtol, gtol, max_nfev, device,
                                          extrinsics_out, points_out, point_status, result16, history, history_rows);
}

// reduction MCBA_KPBA_TILED: the reduce of mcba_kpba_tiled.hip and the wide tables; everything else is the same text
int mcba_refine_extrinsics_reduction(int n_cameras, size_t n_points, const double* uvs, const double* weights, int reduction, const double* cam12, const double* dist5, const double* points, int* held,
                                     int gauge_camera, int scale_camera, int loss, double f_scale, double ftol, double xtol, double gtol, int max_nfev, int device, double* extrinsics_out,
                                     double* points_out, int* point_status, double* result16, double* history, int history_rows) {
  const char* who = weights ? "mcba_refine_extrinsics_weighted" : "mcba_refine_extrinsics";
  if (int rc = kpba_refuse(who, n_cameras, n_points, loss, f_scale, reduction)) return rc;
  if (!uvs || !cam12 || !points || !held || !extrinsics_out || !points_out || !point_status || !result16 || (history_rows > 0 && !history))
    return fail(MCBA_ERR_ARG, "mcba_refine_extrinsics: non-NULL arrays required");
  if (gauge_camera < 0 || gauge_camera >= n_cameras || scale_camera < 0 || scale_camera >= n_cameras || gauge_camera == scale_camera)
    return fail(MCBA_ERR_ARG, "mcba_refine_extrinsics: gauge_camera and scale_camera must be two different cameras of the rig");
  if (max_nfev < 2) return fail(MCBA_ERR_ARG, "mcba_refine_extrinsics: max_nfev must be at least 2 (the start and one trial)");
  if (!(ftol >= 0.0 && xtol >= 0.0 && gtol >= 0.0)) return fail(MCBA_ERR_ARG, "mcba_refine_extrinsics: ftol, xtol, gtol must not be negative");
  if (int rc = check_weights(who, weights, (size_t)n_cameras * n_points)) return rc;
  for (int i = 0; i < 16; ++i) result16[i] = 0.0;
  if (int rc = stateless_device(device)) return rc;
  const int C = n_cameras;
  const size_t P = n_points;
  int G = 0;
  if (int rc = kpba_pick_group(who, C, device, reduction, &G)) return rc;

  StatelessCall call;
  DeviceBackEnd be{call, who, C, loss, G, reduction == MCBA_KPBA_TILED, P, f_scale, cam12, dist5};
  std::vector<double> ext((size_t)6 * C);
  for (int c = 0; c < C; ++c)
    for (int k = 0; k < 6; ++k) ext[6 * c + k] = cam12[12 * c + 6 + k];
  if (int rc = be.setup(uvs, weights, points, ext.data(), point_status)) return rc;
  for (int c = 0; c < C; ++c) {   // a camera that no used point sees (with a positive weight) is held whole
    bool seen = false;
    const double* u = uvs + (size_t)2 * c * P;
    const double* w = weights ? weights + (size_t)c * P : nullptr;
    for (size_t p = 0; p < P && !seen; ++p) seen = point_status[p] == mcba::KB_USED && u[2 * p] == u[2 * p] && u[2 * p + 1] == u[2 * p + 1] && (!w || w[p] > 0.0);
    if (!seen) held[c] = 63;
  }
  if (held[scale_camera] == 63) return fail(MCBA_ERR_ARG, "mcba_refine_extrinsics: scale_camera sees no used point (or is held whole): nothing fixes the scale of the rig");
  held[gauge_camera] = 63;
  if (int rc = call.put(be.d_held, held, (size_t)C)) return rc;

  const double baseline = mcba::kpba_baseline(ext.data(), gauge_camera, scale_camera);
  const mcba::KbOptions opt{ftol, xtol, gtol, max_nfev};
  mcba::KbResult res;
  if (int rc = mcba::kpba_lm(be, C, held, ext.data(), opt, res, history, history_rows)) return rc;

  if (int rc = call.download(points_out, be.d_pts[be.cur], 3 * P)) return rc;
  const double nan = __builtin_nan("");
  for (size_t p = 0; p < P; ++p)
    if (point_status[p] != mcba::KB_USED) points_out[3 * p] = points_out[3 * p + 1] = points_out[3 * p + 2] = nan;
  const double s = mcba::kpba_rescale(C, held, ext.data(), P, points_out, gauge_camera, scale_camera, baseline);
  for (int k = 0; k < 6 * C; ++k) extrinsics_out[k] = ext[k];
  result16[0] = res.cost; result16[1] = res.cost0; result16[2] = res.optimality; result16[3] = res.nfev; result16[4] = res.njev; result16[5] = res.status; result16[6] = s;
  result16[7] = res.nhist; result16[8] = be.status_ms + be.reduce_ms + be.step_ms; result16[9] = be.reduce_ms; result16[10] = be.n_reduce; result16[11] = be.step_ms; result16[12] = be.n_step;
  result16[13] = G;
  if (be.tiled) { result16[14] = mcba::kKtBand; result16[15] = mcba::kpba_tiled_pairs(C); }
  return MCBA_OK;
}

int mcba_refine_extrinsics_system(int n_cameras, size_t n_points, const double* uvs, const double* cam12, const double* dist5, const double* points, const int* held, int loss, double f_scale,
                                  double lam, int device, const double* ext_trial, const double* dtheta, int* point_status, double* system, double* trial_points, double* step4, double* info4) {
  return mcba_refine_extrinsics_system_weighted(n_cameras, n_points, uvs, nullptr, cam12, dist5, points, held, loss, f_scale, lam, device, ext_trial, dtheta, point_status, system, trial_points, step4,
                                                info4);
}

int mcba_refine_extrinsics_system_weighted(int n_cameras, size_t n_points, const double* uvs, const double* weights, const double* cam12, const double* dist5, const double* points, const int* held,
                                           int loss, double f_scale, double lam, int device, const double* ext_trial, const double* dtheta, int* point_status, double* system, double* trial_points,
                                           double* step4, double* info4) {
  if (!info4) return fail(MCBA_ERR_ARG, "mcba_refine_extrinsics_system: non-NULL arrays required (ext_trial and dtheta both or neither; with them trial_points and step4)");
  double info8[8];
  const int rc = mcba_refine_extrinsics_system_reduction(n_cameras, n_points, uvs, weights, MCBA_KPBA_RESIDENT, cam12, dist5, points, held, loss, f_scale, lam, device, ext_trial, dtheta, point_status,
                                                         system, trial_points, step4, info8);
  if (rc == MCBA_OK)
    for (int k = 0; k < 4; ++k) info4[k] = info8[k];
  return rc;
}

int mcba_refine_extrinsics_system_reduction(int n_cameras, size_t n_points, const double* uvs, const double* weights, int reduction, const double* cam12, const double* dist5, const double* points,
                                            const int* held, int loss, double f_scale, double lam, int device, const double* ext_trial, const double* dtheta, int* point_status, double* system,
                                            double* trial_points, double* step4, double* info8) {
  const char* who = weights ? "mcba_refine_extrinsics_system_weighted" : "mcba_refine_extrinsics_system";
  if (int rc = kpba_refuse(who, n_cameras, n_points, loss, f_scale, reduction)) return rc;
  const bool stepping = ext_trial || dtheta;
  if (!uvs || !cam12 || !points || !held || !point_status || !system || !info8 || (stepping && (!ext_trial || !dtheta || !trial_points || !step4)))
    return fail(MCBA_ERR_ARG, "mcba_refine_extrinsics_system: non-NULL arrays required (ext_trial and dtheta both or neither; with them trial_points and step4)");
  if (!(lam >= 0.0 && lam < mcba::KB_LAMBDA_MAX)) return fail(MCBA_ERR_ARG, "mcba_refine_extrinsics_system: lam must be in [0, 1e12)");
  if (int rc = check_weights(who, weights, (size_t)n_cameras * n_points)) return rc;
  if (int rc = stateless_device(device)) return rc;
  const int C = n_cameras;
  const size_t P = n_points;
  int G = 0;
  if (int rc = kpba_pick_group(who, C, device, reduction, &G)) return rc;

  StatelessCall call;
  DeviceBackEnd be{call, who, C, loss, G, reduction == MCBA_KPBA_TILED, P, f_scale, cam12, dist5};
  std::vector<double> ext((size_t)6 * C);
  for (int c = 0; c < C; ++c)
    for (int k = 0; k < 6; ++k) ext[6 * c + k] = cam12[12 * c + 6 + k];
  if (int rc = be.setup(uvs, weights, points, ext.data(), point_status)) return rc;
  if (int rc = call.put(be.d_held, held, (size_t)C)) return rc;   // (as given: no gauge, no scale, no blind-camera rule here)
  mcba::KbSystem sys;
  if (int rc = be.reduce(ext.data(), lam, sys)) return rc;
  std::copy(be.host_sys.begin(), be.host_sys.end(), system);
  if (stepping) {
    double out[3];
    if (int rc = be.step(ext_trial, dtheta, lam, out)) return rc;
    if (int rc = call.download(trial_points, be.d_pts[1 - be.cur], 3 * P)) return rc;
    for (int k = 0; k < 4; ++k) step4[k] = be.out4[k];
  }
  info8[0] = G; info8[1] = be.partials(); info8[2] = sys.NP; info8[3] = be.status_ms + be.reduce_ms + be.step_ms;
  info8[4] = be.tiled ? mcba::kKtBand : 0; info8[5] = be.tiled ? mcba::kpba_tiled_pairs(C) : 0; info8[6] = reduction; info8[7] = 0.0;
  return MCBA_OK;
}

}  // extern "C"
