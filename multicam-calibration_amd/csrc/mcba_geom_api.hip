// mcba_geom_api.hip -- the stateless geometry calls of include/mcba.h (host arrays in, host arrays out, a device ordinal, no handle):
// undistort_points, robust triangulation, its refinement and its consensus form, keypoint projection, rigid transforms and reprojection errors.
#include "mcba_handle.h"
#include "mcba_keypoint_math.h"   // KpCam, make_kp_cam: the camera table of the keypoint kernels

using namespace mcba_internal;

// the camera table of the keypoint kernels in device memory: for the calls of this file and every other stateless call on keypoints (mcba_handle.h)
int mcba_internal::upload_kp_cams(StatelessCall& call, int n_cameras, const double* cam12, const double* dist5, mcba::KpCam** d_cams) {
  std::vector<mcba::KpCam> tab((size_t)n_cameras);
  for (int c = 0; c < n_cameras; ++c) mcba::make_kp_cam(cam12 + 12 * c, dist5 ? dist5 + 5 * c : nullptr, tab[c]);
  return call.upload(d_cams, tab.data(), tab.size());
}

extern "C" {

// undistort_points (reference geometry.py:328-358): stateless; host arrays in, host array out
int mcba_undistort_points(size_t n_points, const double* uvs, const double* K4, const double* dist5, int iterations, int device, double* out) {
  if (!uvs || !K4 || !out || iterations < 0) return fail(MCBA_ERR_ARG, "mcba_undistort_points: bad argument");
  if (n_points == 0) return MCBA_OK;
  if (int rc = stateless_device(device)) return rc;
  StatelessCall call;
  double *d_in = nullptr, *d_out = nullptr;
  if (int rc = call.upload(&d_in, uvs, 2 * n_points)) return rc;
  if (int rc = call.scratch(&d_out, 2 * n_points)) return rc;
  mcba::launch_undistort(nullptr, d_in, d_out, n_points, K4, dist5, iterations);
  if (int rc = check_launch()) return rc;
  return call.download(out, d_out, 2 * n_points);
}

// ---------------------------------------------------------------------------------------------------------
// Robust triangulation (reference geometry.py:361-433): stateless; host arrays in, host array out.
// The median-of-pairs kernels' camera operands: per camera {P = K [R | t] (12), K (4), dist (5)} -- kernel arguments for the register path
// (<= 8 cameras), a device array for the wavefront-per-point path
struct TriOperands {
  bool reg_path = true;
  mcba::TriCams cams;
  double* d_cams = nullptr;
};
static int tri_operands(StatelessCall& call, int n_cameras, const double* cam12, const double* dist5, TriOperands& op) {
  std::vector<double> cam21((size_t)21 * n_cameras, 0.0);
  for (int c = 0; c < n_cameras; ++c) {
    const double* q = cam12 + 12 * c;
    double* P = cam21.data() + (size_t)21 * c;
    double R[9];
    mcba::rot_only(q + 6, R);
    const double fx = q[0], fy = q[1], cx = q[2], cy = q[3];
    for (int j = 0; j < 3; ++j) {
      P[j] = fx * R[j] + cx * R[6 + j];
      P[4 + j] = fy * R[3 + j] + cy * R[6 + j];
      P[8 + j] = R[6 + j];
    }
    P[3] = fx * q[9] + cx * q[11];
    P[7] = fy * q[10] + cy * q[11];
    P[11] = q[11];
    P[12] = fx; P[13] = fy; P[14] = cx; P[15] = cy;
    if (dist5) for (int k = 0; k < 5; ++k) P[16 + k] = dist5[5 * c + k];
    else { P[16] = q[4]; P[17] = q[5]; }
  }
  op.reg_path = n_cameras <= 8;
  memset(&op.cams, 0, sizeof(op.cams));
  if (!op.reg_path) return call.upload(&op.d_cams, cam21.data(), cam21.size());
  for (int c = 0; c < n_cameras; ++c) {
    memcpy(op.cams.P[c], cam21.data() + (size_t)21 * c, 12 * sizeof(double));
    memcpy(op.cams.K[c], cam21.data() + (size_t)21 * c + 12, 4 * sizeof(double));
    memcpy(op.cams.dist[c], cam21.data() + (size_t)21 * c + 16, 5 * sizeof(double));
  }
  return MCBA_OK;
}
static int tri_launch(const TriOperands& op, int n_cameras, const double* d_uv, double* d_out, size_t n_points, int iterations) {
  return op.reg_path ? mcba::launch_triangulate(nullptr, n_cameras, d_uv, op.cams, d_out, n_points, iterations)
                     : mcba::launch_triangulate_wave(nullptr, n_cameras, d_uv, op.d_cams, d_out, n_points, iterations);
}

int mcba_triangulate(int n_cameras, size_t n_points, const double* uvs, const double* cam12, const double* dist5, int iterations, int device, double* out, double* kernel_ms) {
  if (n_cameras < 2 || n_cameras > 64 || !uvs || !cam12 || !out || iterations < 0) return fail(MCBA_ERR_ARG, "mcba_triangulate: 2..64 cameras, non-NULL arrays, iterations >= 0 required");
  if (n_points == 0) return MCBA_OK;
  if (int rc = stateless_device(device)) return rc;
  StatelessCall call;
  double *d_uv = nullptr, *d_out = nullptr;
  const size_t nin = (size_t)2 * n_cameras * n_points;
  if (int rc = call.upload(&d_uv, uvs, nin)) return rc;
  if (int rc = call.scratch(&d_out, 3 * n_points)) return rc;
  TriOperands op;
  if (int rc = tri_operands(call, n_cameras, cam12, dist5, op)) return rc;
  HIPCHK(call.start());
  if (tri_launch(op, n_cameras, d_uv, d_out, n_points, iterations) != 0) return fail(MCBA_ERR_ARG, "mcba_triangulate: unsupported camera count");
  if (int rc = check_launch()) return rc;
  HIPCHK(call.stop(kernel_ms));
  return call.download(out, d_out, 3 * n_points);
}

// ---------------------------------------------------------------------------------------------------------
// Keypoints through a calibration (reference geometry.py:128-152 apply_rigid_transform, :277-325 project_points): stateless; host arrays in and out.
// (the camera table of the keypoint kernels: upload_kp_cams, above)

int mcba_project_points(int n_cameras, size_t n_points, const double* points, const double* cam12, const double* dist5, int device, double* uvs_out, double* kernel_ms) {
  if (n_cameras < 1 || !points || !cam12 || !uvs_out) return fail(MCBA_ERR_ARG, "mcba_project_points: cameras >= 1, non-NULL arrays required");
  if (n_points == 0) return MCBA_OK;
  if (int rc = stateless_device(device)) return rc;
  StatelessCall call;
  double *d_pts = nullptr, *d_out = nullptr;
  mcba::KpCam* d_cams = nullptr;
  const size_t nout = (size_t)2 * n_cameras * n_points;
  if (int rc = call.upload(&d_pts, points, 3 * n_points)) return rc;
  if (int rc = call.scratch(&d_out, nout)) return rc;
  if (int rc = upload_kp_cams(call, n_cameras, cam12, dist5, &d_cams)) return rc;
  HIPCHK(call.start());
  for (int c0 = 0; c0 < n_cameras; c0 += mcba::kKpMaxCams) {   // the table of one launch holds kKpMaxCams cameras
    const int nc = std::min(mcba::kKpMaxCams, n_cameras - c0);
    if (mcba::launch_project(nullptr, dist5 ? 1 : 0, d_pts, n_points, d_cams + c0, nc, d_out + (size_t)2 * c0 * n_points) != 0) return fail(MCBA_ERR_ARG, "mcba_project_points: bad launch");
  }
  if (int rc = check_launch()) return rc;
  HIPCHK(call.stop(kernel_ms));
  return call.download(uvs_out, d_out, nout);
}

int mcba_rigid_transform(size_t n_points, const double* points, const double* T12, int device, double* out) {
  if (!points || !T12 || !out) return fail(MCBA_ERR_ARG, "mcba_rigid_transform: non-NULL arrays required");
  if (n_points == 0) return MCBA_OK;
  if (int rc = stateless_device(device)) return rc;
  mcba::KpCam kc;
  memset(&kc, 0, sizeof(kc));
  memcpy(kc.pc.Rcf, T12, 9 * sizeof(double));
  memcpy(kc.pc.tcf, T12 + 9, 3 * sizeof(double));
  StatelessCall call;
  double *d_pts = nullptr, *d_out = nullptr;
  mcba::KpCam* d_cams = nullptr;
  if (int rc = call.upload(&d_pts, points, 3 * n_points)) return rc;
  if (int rc = call.scratch(&d_out, 3 * n_points)) return rc;
  if (int rc = call.upload(&d_cams, &kc, 1)) return rc;
  if (mcba::launch_project(nullptr, 2, d_pts, n_points, d_cams, 1, d_out) != 0) return fail(MCBA_ERR_ARG, "mcba_rigid_transform: bad launch");
  if (int rc = check_launch()) return rc;
  return call.download(out, d_out, 3 * n_points);
}

int mcba_keypoint_errors(int n_cameras, size_t n_points, const double* points, const double* uvs, const double* cam12, const double* dist5, int device, double* errors_out, double* median_out,
                         double* kernel_ms) {
  if (n_cameras < 1 || !points || !uvs || !cam12 || !median_out) return fail(MCBA_ERR_ARG, "mcba_keypoint_errors: cameras >= 1, non-NULL arrays required");
  if (n_points == 0) {
    for (int c = 0; c < n_cameras; ++c) median_out[c] = __builtin_nan("");
    return MCBA_OK;
  }
  if (int rc = stateless_device(device)) return rc;
  const size_t npad = (n_points + 63) / 64 * 64, nuv = (size_t)2 * n_cameras * n_points;
  StatelessCall call;
  double *d_pts = nullptr, *d_uv = nullptr, *d_err = nullptr;
  mcba::KpCam* d_cams = nullptr;
  mcba::SelState* d_sel = nullptr;
  std::vector<mcba::SelState> sel((size_t)2 * n_cameras);
  if (int rc = call.upload(&d_pts, points, 3 * n_points)) return rc;
  if (int rc = call.upload(&d_uv, uvs, nuv)) return rc;
  if (int rc = call.scratch(&d_err, (size_t)n_cameras * npad)) return rc;
  if (int rc = call.scratch(&d_sel, sel.size())) return rc;
  if (int rc = upload_kp_cams(call, n_cameras, cam12, dist5, &d_cams)) return rc;
  HIPCHK(call.start());
  for (int c0 = 0; c0 < n_cameras; c0 += mcba::kKpMaxCams) {
    const int nc = std::min(mcba::kKpMaxCams, n_cameras - c0);
    if (mcba::launch_keypoint_errors(nullptr, d_pts, d_uv + (size_t)2 * c0 * n_points, n_points, npad, d_cams + c0, nc, d_err + (size_t)c0 * npad) != 0)
      return fail(MCBA_ERR_ARG, "mcba_keypoint_errors: bad launch");
  }
  if (int rc = check_launch()) return rc;
  mcba::launch_select(nullptr, d_err, nullptr, npad, n_cameras, 1 /* no frame mask */, d_sel, 0 /* errors are >= +0 */);   // per-camera medians: two states per camera
  if (int rc = check_launch()) return rc;
  HIPCHK(call.stop(kernel_ms));
  if (int rc = call.download(sel.data(), d_sel, sel.size())) return rc;
  for (int c = 0; c < n_cameras; ++c) median_out[c] = mcba::sel_median(sel[2 * c], sel[2 * c + 1]);
  if (errors_out)
    HIPCHK(hipMemcpy2D(errors_out, n_points * sizeof(double), d_err, npad * sizeof(double), n_points * sizeof(double), (size_t)n_cameras, hipMemcpyDeviceToHost));
  return MCBA_OK;
}

int mcba_triangulate_refine(int n_cameras, size_t n_points, const double* uvs, const double* cam12, const double* dist5, const double* points_in, int undistort_iterations, int loss, double f_scale,
                            int max_iterations, int device, double* points_out, double* info_out, double* kernel_ms) {
  return mcba_triangulate_refine_weighted(n_cameras, n_points, uvs, nullptr, cam12, dist5, points_in, undistort_iterations, loss, f_scale, max_iterations, device, points_out, info_out, kernel_ms);
}

// weights NULL: the call above, launch for launch.  Otherwise the plane of sqrt(w) goes up once beside the detections; the detections of zero or
// NaN weight go up as NaN, so that the median of pairs (which stays unweighted) does not see them either.
int mcba_triangulate_refine_weighted(int n_cameras, size_t n_points, const double* uvs, const double* weights, const double* cam12, const double* dist5, const double* points_in,
                                     int undistort_iterations, int loss, double f_scale, int max_iterations, int device, double* points_out, double* info_out, double* kernel_ms) {
  if (n_cameras < 2 || n_cameras > 64 || !uvs || !cam12 || !points_out || undistort_iterations < 0 || max_iterations < 0)
    return fail(MCBA_ERR_ARG, "mcba_triangulate_refine: 2..64 cameras, non-NULL arrays, iterations >= 0 required");
  if (loss < mcba::LOSS_LINEAR || loss > mcba::LOSS_ARCTAN) return fail(MCBA_ERR_ARG, "mcba_triangulate_refine: loss must be one of linear, soft_l1, huber, cauchy, arctan (0 .. 4)");
  if (!(f_scale > 0.0)) return fail(MCBA_ERR_ARG, "mcba_triangulate_refine: f_scale must be positive");
  if (int rc = check_weights("mcba_triangulate_refine_weighted", weights, (size_t)n_cameras * n_points)) return rc;
  if (n_points == 0) return MCBA_OK;
  if (int rc = stateless_device(device)) return rc;
  StatelessCall call;
  double *d_uv = nullptr, *d_start = nullptr, *d_out = nullptr, *d_info = nullptr, *d_sw = nullptr;
  mcba::KpCam* d_cams = nullptr;
  const size_t nuv = (size_t)2 * n_cameras * n_points;
  if (int rc = upload_sqrt_weights(call, weights, nuv / 2, &d_sw)) return rc;
  if (weights) {
    const double nan = __builtin_nan("");
    std::vector<double> masked(uvs, uvs + nuv);
    for (size_t i = 0; i < nuv / 2; ++i)
      if (!(weights[i] > 0.0)) masked[2 * i] = masked[2 * i + 1] = nan;
    if (int rc = call.upload(&d_uv, masked.data(), nuv)) return rc;
  } else if (int rc = call.upload(&d_uv, uvs, nuv)) return rc;   // the detections go up once, for the start and for the refinement
  if (int rc = points_in ? call.upload(&d_start, points_in, 3 * n_points) : call.scratch(&d_start, 3 * n_points)) return rc;
  if (int rc = call.scratch(&d_out, 3 * n_points)) return rc;
  if (info_out)
    if (int rc = call.scratch(&d_info, 4 * n_points)) return rc;
  if (int rc = upload_kp_cams(call, n_cameras, cam12, dist5, &d_cams)) return rc;
  TriOperands op;
  if (!points_in)
    if (int rc = tri_operands(call, n_cameras, cam12, dist5, op)) return rc;
  HIPCHK(call.start());
  if (!points_in) {   // start from the median of pairs
    if (tri_launch(op, n_cameras, d_uv, d_start, n_points, undistort_iterations) != 0) return fail(MCBA_ERR_ARG, "mcba_triangulate_refine: unsupported camera count");
    if (int rc = check_launch()) return rc;
  }
  if (mcba::launch_tri_refine(nullptr, loss, d_uv, d_start, n_points, d_cams, n_cameras, f_scale, max_iterations, d_out, d_info, d_sw) != 0) return fail(MCBA_ERR_ARG, "mcba_triangulate_refine: bad launch");
  if (int rc = check_launch()) return rc;
  HIPCHK(call.stop(kernel_ms));
  if (int rc = call.download(points_out, d_out, 3 * n_points)) return rc;
  return info_out ? call.download(info_out, d_info, 4 * n_points) : MCBA_OK;
}

// Consensus triangulation (csrc/mcba_consensus.hip): the detections go up once; the search, the refit and the optional errors at the
// final point run on that copy.  The projection matrices of the hypotheses are derived on the device from the one camera table (upload_kp_cams).
int mcba_triangulate_consensus(int n_cameras, size_t n_points, const double* uvs, const double* cam12, const double* dist5, double threshold, int min_views, int undistort_iterations, int loss,
                               double f_scale, int max_iterations, int device, double* points_out, unsigned long long* inliers_out, double* info_out, double* errors_out, double* kernel_ms) {
  if (n_cameras < 2 || n_cameras > 64 || !uvs || !cam12 || !points_out || !inliers_out || undistort_iterations < 0 || max_iterations < 0)
    return fail(MCBA_ERR_ARG, "mcba_triangulate_consensus: 2..64 cameras, non-NULL arrays, iterations >= 0 required");
  if (!(threshold > 0.0)) return fail(MCBA_ERR_ARG, "mcba_triangulate_consensus: threshold (pixels) must be positive");
  if (min_views < 2) return fail(MCBA_ERR_ARG, "mcba_triangulate_consensus: min_views must be at least 2");
  if (loss < mcba::LOSS_LINEAR || loss > mcba::LOSS_ARCTAN) return fail(MCBA_ERR_ARG, "mcba_triangulate_consensus: loss must be one of linear, soft_l1, huber, cauchy, arctan (0 .. 4)");
  if (!(f_scale > 0.0)) return fail(MCBA_ERR_ARG, "mcba_triangulate_consensus: f_scale must be positive");
  if (n_points == 0) return MCBA_OK;
  if (int rc = stateless_device(device)) return rc;
  StatelessCall call;
  double *d_uv = nullptr, *d_out = nullptr, *d_hyp = nullptr, *d_info = nullptr, *d_err = nullptr;
  unsigned long long* d_mask = nullptr;
  mcba::KpCam* d_cams = nullptr;
  const size_t nuv = (size_t)2 * n_cameras * n_points;
  if (int rc = call.upload(&d_uv, uvs, nuv)) return rc;
  if (int rc = call.scratch(&d_out, 3 * n_points)) return rc;
  if (int rc = call.scratch(&d_mask, n_points)) return rc;
  if (int rc = call.scratch(&d_hyp, 2 * n_points)) return rc;
  if (info_out)
    if (int rc = call.scratch(&d_info, 8 * n_points)) return rc;
  if (errors_out)
    if (int rc = call.scratch(&d_err, (size_t)n_cameras * n_points)) return rc;
  if (int rc = upload_kp_cams(call, n_cameras, cam12, dist5, &d_cams)) return rc;
  HIPCHK(call.start());
  if (mcba::launch_consensus(nullptr, mcba::CONSENSUS_AUTO, loss, d_uv, n_points, d_cams, n_cameras, threshold, min_views, undistort_iterations, f_scale, max_iterations, d_out, d_mask, d_hyp, d_info) != 0)
    return fail(MCBA_ERR_ARG, "mcba_triangulate_consensus: bad launch (MCBA_CONSENSUS_FORM, if set, must be lane, wave or lane2)");
  if (int rc = check_launch()) return rc;
  if (errors_out) {
    if (mcba::launch_keypoint_errors(nullptr, d_out, d_uv, n_points, n_points, d_cams, n_cameras, d_err) != 0) return fail(MCBA_ERR_ARG, "mcba_triangulate_consensus: bad launch");
    if (int rc = check_launch()) return rc;
  }
  HIPCHK(call.stop(kernel_ms));
  if (int rc = call.download(points_out, d_out, 3 * n_points)) return rc;
  if (int rc = call.download(inliers_out, d_mask, n_points)) return rc;
  if (info_out)
    if (int rc = call.download(info_out, d_info, 8 * n_points)) return rc;
  return errors_out ? call.download(errors_out, d_err, (size_t)n_cameras * n_points) : MCBA_OK;
}

}  // extern "C"
