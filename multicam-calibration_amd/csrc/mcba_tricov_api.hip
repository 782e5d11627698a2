// mcba_tricov_api.hip -- the stateless triangulation-uncertainty call of include/mcba.h (host arrays in, host arrays out, a device ordinal, no
// handle), in the idiom of mcba_geom_api.hip: one upload of the detections, the kernels of mcba_tricov.hip back to back on it.
#include "mcba_handle.h"
#include "mcba_tricov_math.h"   // TcCam, make_tc_cam: the camera table of the kernels

using namespace mcba_internal;

extern "C" {

int mcba_triangulation_covariance(int n_cameras, size_t n_points, const double* points, const double* uvs, const double* cam12, const double* dist5, const double* cam_cov, int loss, double f_scale,
                                  double sigma2_in, int device, double* det6, double* cal6, int* views_out, int* status_out, double* info8, double* kernel_ms) {
  return mcba_triangulation_covariance_weighted(n_cameras, n_points, points, uvs, nullptr, cam12, dist5, cam_cov, loss, f_scale, sigma2_in, device, det6, cal6, views_out, status_out, info8, kernel_ms);
}

// weights NULL: the call above, launch for launch.  Otherwise the plane of sqrt(w) goes up once beside the detections and the weighted kernels run.
int mcba_triangulation_covariance_weighted(int n_cameras, size_t n_points, const double* points, const double* uvs, const double* weights, const double* cam12, const double* dist5,
                                           const double* cam_cov, int loss, double f_scale, double sigma2_in, int device, double* det6, double* cal6, int* views_out, int* status_out, double* info8,
                                           double* kernel_ms) {
  if (n_cameras < 2 || n_cameras > 64 || !points || !uvs || !cam12 || !det6 || !views_out || !status_out || !info8)
    return fail(MCBA_ERR_ARG, "mcba_triangulation_covariance: 2..64 cameras, non-NULL arrays required");
  if ((cam_cov != nullptr) != (cal6 != nullptr)) return fail(MCBA_ERR_ARG, "mcba_triangulation_covariance: cal6 is required exactly when cam_cov is given");
  if (loss < mcba::LOSS_LINEAR || loss > mcba::LOSS_ARCTAN) return fail(MCBA_ERR_ARG, "mcba_triangulation_covariance: loss must be one of linear, soft_l1, huber, cauchy, arctan (0 .. 4)");
  if (!(f_scale > 0.0)) return fail(MCBA_ERR_ARG, "mcba_triangulation_covariance: f_scale must be positive");
  if (!(sigma2_in != sigma2_in) && !(sigma2_in >= 0.0)) return fail(MCBA_ERR_ARG, "mcba_triangulation_covariance: sigma2 >= 0, or NaN to estimate it");
  if (int rc = check_weights("mcba_triangulation_covariance_weighted", weights, (size_t)n_cameras * n_points)) return rc;
  for (int i = 0; i < 8; ++i) info8[i] = 0.0;
  info8[0] = sigma2_in;
  if (kernel_ms) *kernel_ms = 0.0;
  if (n_points == 0) return MCBA_OK;
  if (int rc = stateless_device(device)) return rc;

  const int n = 12 * n_cameras, ld = (n + 63) / 64 * 64;
  int G = 0;
  if (cam_cov) {
    int force_g = 0;
    if (const char* e = getenv("MCBA_TRICOV_G")) force_g = atoi(e);   // test knob: the smaller shapes of k_tricov_cal at any size
    G = mcba::tricov_group(n, lds_optin_of(device), force_g);
    if (!G) return fail(MCBA_ERR_HIP, "mcba_triangulation_covariance: k_tricov_cal does not fit the LDS of this device");
  }

  StatelessCall call;
  double *d_uv = nullptr, *d_pts = nullptr, *d_hinv = nullptr, *d_det = nullptr, *d_cal = nullptr, *d_part = nullptr, *d_info = nullptr, *d_sig = nullptr, *d_sw = nullptr;
  int *d_views = nullptr, *d_status = nullptr;
  mcba::TcCam* d_cams = nullptr;
  std::vector<mcba::TcCam> tab((size_t)n_cameras);
  for (int c = 0; c < n_cameras; ++c) mcba::make_tc_cam(cam12 + 12 * c, dist5 ? dist5 + 5 * c : nullptr, tab[c]);
  if (int rc = call.upload(&d_uv, uvs, (size_t)2 * n_cameras * n_points)) return rc;
  if (int rc = upload_sqrt_weights(call, weights, (size_t)n_cameras * n_points, &d_sw)) return rc;
  if (int rc = call.upload(&d_pts, points, 3 * n_points)) return rc;
  if (int rc = call.upload(&d_cams, tab.data(), tab.size())) return rc;
  if (int rc = call.scratch(&d_hinv, 6 * n_points)) return rc;
  if (int rc = call.scratch(&d_det, 6 * n_points)) return rc;
  if (int rc = call.scratch(&d_views, n_points)) return rc;
  if (int rc = call.scratch(&d_status, n_points)) return rc;
  if (int rc = call.scratch(&d_part, (size_t)4 * mcba::tricov_point_blocks(n_points))) return rc;
  if (int rc = call.scratch(&d_info, (size_t)8)) return rc;
  if (cam_cov) {
    std::vector<double> sig((size_t)ld * ld, 0.0);   // zero-padded to ld x ld: the kernel's panel fetches never leave it
    for (int i = 0; i < n; ++i) memcpy(sig.data() + (size_t)i * ld, cam_cov + (size_t)i * n, n * sizeof(double));
    if (int rc = call.upload(&d_sig, sig.data(), sig.size())) return rc;
    if (int rc = call.scratch(&d_cal, 6 * n_points)) return rc;
  }
  HIPCHK(call.start());
  if (mcba::launch_tricov_point(nullptr, loss, d_uv, d_pts, n_points, d_cams, n_cameras, f_scale, sigma2_in, d_hinv, d_views, d_status, d_part, d_info, d_sw) != 0)
    return fail(MCBA_ERR_ARG, "mcba_triangulation_covariance: bad launch");
  if (int rc = check_launch()) return rc;
  if (cam_cov) {
    if (mcba::launch_tricov_cal(nullptr, loss, d_uv, d_pts, n_points, d_cams, n_cameras, f_scale, d_hinv, d_status, d_sig, ld, d_info, d_det, d_cal, G, d_sw) != 0)
      return fail(MCBA_ERR_ARG, "mcba_triangulation_covariance: bad launch (k_tricov_cal)");
  } else {
    mcba::launch_tricov_scale(nullptr, d_hinv, d_status, d_info, n_points, d_det);
  }
  if (int rc = check_launch()) return rc;
  double ms = 0.0;
  HIPCHK(call.stop(&ms));
  if (kernel_ms) *kernel_ms = ms;
  if (int rc = call.download(info8, d_info, (size_t)5)) return rc;
  info8[5] = ms; info8[6] = G; info8[7] = ld;
  if (int rc = call.download(det6, d_det, 6 * n_points)) return rc;
  if (int rc = call.download(views_out, d_views, n_points)) return rc;
  if (int rc = call.download(status_out, d_status, n_points)) return rc;
  return cal6 ? call.download(cal6, d_cal, 6 * n_points) : MCBA_OK;
}

}  // extern "C"
