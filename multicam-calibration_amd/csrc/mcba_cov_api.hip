// mcba_cov_api.hip -- mcba_covariance (include/mcba.h): the covariance of the cameras and of the frame poses at x[slot], from one
// linearisation with the IRLS weight and the Schur reduction with lambda = 0 (kernels: mcba_cov.hip).
#include "mcba_handle.h"

using namespace mcba_internal;

namespace {

// the pieces of h->cov_work, in doubles
struct CovWork {
  size_t ld, R, M, Sig, isd, part, scal, ints, flag, fout, total;
  explicit CovWork(const mcba_handle* h) {
    ld = ((size_t)h->n + 63) / 64 * 64;
    size_t o = 0;
    auto take = [&](size_t count) { const size_t at = o; o += (count + 31) / 32 * 32; return at; };
    R = take(ld * ld); M = take(ld * ld); Sig = take(ld * ld); isd = take(ld); part = take(2 * 1024); scal = take(8); ints = take(4);
    flag = take(((size_t)h->Fpad + 7) / 8); fout = take((size_t)h->F * 36);
    total = o;
  }
};

}  // namespace

extern "C" {

int mcba_covariance(mcba_handle* h, int slot, int gauge_camera, double sigma2_in, double* cam_cov, double* frame_cov, double* info8) {
  if (!slot_ok(h, slot) || !info8) return fail(MCBA_ERR_ARG, "mcba_covariance: bad handle/slot/pointer");
  if (h->sparse) return fail(MCBA_ERR_ARG, "mcba_covariance: the sparse-Schur handle is not covered yet (dense handles: at most 40 cameras)");
  if (gauge_camera < 0 || gauge_camera >= h->C) return fail(MCBA_ERR_ARG, "mcba_covariance: gauge_camera out of range");
  if (!h->have_obs) return fail(MCBA_ERR_ARG, "mcba_covariance: upload observations first");
  if (h->loss == mcba::LOSS_TABLE) return fail(MCBA_ERR_ARG, "mcba_covariance: named losses only (a tabulated loss is set)");
  if (h->have_xscale) return fail(MCBA_ERR_ARG, "mcba_covariance: a numeric x_scale or frozen coordinates are set on this handle");
  if (!(sigma2_in != sigma2_in) && !(sigma2_in >= 0.0)) return fail(MCBA_ERR_ARG, "mcba_covariance: sigma2 >= 0, or NaN to estimate it");
  HIPCHK(hipSetDevice(h->device));
  NEED_SOLVER(h);
  int force_g = 0;
  if (const char* e = getenv("MCBA_COV_FRAMES_G")) force_g = atoi(e);   // test knob: the 4-frame shape of k_cov_frames at any size
  const int G = mcba::cov_frames_group(h->n, h->lds_optin, force_g);
  if (frame_cov && !G) return fail(MCBA_ERR_HIP, "mcba_covariance: k_cov_frames does not fit the LDS of this device");
  const CovWork cw(h);
  int rc;
  if (!h->cov_work && (rc = dalloc(h, &h->cov_work, cw.total, false))) return rc;
  if (!h->res && (rc = dalloc(h, &h->res, (size_t)2 * h->C * h->F * h->N, false))) return rc;
  double* W = h->cov_work;
  int* ints = reinterpret_cast<int*>(W + cw.ints);   // first failing pivot, degenerate frames, degenerate frames with data
  unsigned char* flag = reinterpret_cast<unsigned char*>(W + cw.flag);

  // ---- linearise x[slot] with the IRLS weight into the handle's own buffers, reduce with lambda = 0 (k_syrk adds lambda D to the diagonal
  // of V_f and k_reduce_system leaves the damping to the solve: lambda = 0 takes the same path as any other value); the caller's
  // linearisation is gone afterwards, its curvature floor is not
  const double floor_was = h->curv_floor;
  h->curv_floor = 1.0;
  rc = gram_launch(h, host_sel(0), h->x[slot], h->x[slot], h->lin, h->lin);
  h->curv_floor = floor_was;
  h->have_lin = h->have_red = h->have_spec = false;
  if (rc) return rc;
  if ((rc = syrk_launch(h, host_sel(h->lin, 0.0), no_fuse()))) return rc;
  if ((rc = reduce_launch(h, host_sel(h->lin), 0, false))) return rc;

  // ---- the noise scale's sums and the frames' verdicts
  mcba::launch_cost(h->stream, h->loss, h->f_scale, h->obs_t, h->obj, h->x[slot], h->cpart, h->res, h->C, h->F, h->N, h->Fpad, h->nch, NAN);
  if ((rc = check_launch())) return rc;
  if (mcba::launch_cov_wss(h->stream, h->loss, h->f_scale, h->res, (size_t)2 * h->C * h->F * h->N, W + cw.part, W + cw.scal)) return fail(MCBA_ERR_ARG, "mcba_covariance: unknown loss");
  if ((rc = check_launch())) return rc;
  const int ints0[4] = {-1, 0, 0, 0};
  HIPCHK(hipMemcpyAsync(ints, ints0, sizeof(ints0), hipMemcpyHostToDevice, h->stream));
  mcba::launch_cov_check(h->stream, h->rec2[h->lin], flag, ints + 1, h->C, h->F, h->Fpad);
  if ((rc = check_launch())) return rc;
  double sums[2];
  int counts[4];
  HIPCHK(hipMemcpyAsync(sums, W + cw.scal, sizeof(sums), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipMemcpyAsync(counts, ints, sizeof(counts), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  h->have_jac = false;   // (the residual buffer now holds NaN where a scalar is missing)
  if (!isfinite(sums[0])) return fail(MCBA_ERR_NONFINITE, "Residuals are not finite");
  const int ndeg = counts[1];
  if (counts[2] > 0) {
    g_err = "mcba_covariance: " + std::to_string(counts[2]) + " frame(s) hold data but their V_f is not positive definite: leave them out (they reached the Schur complement)";
    return MCBA_ERR_ARG;
  }
  const double m = sums[1], p = (double)(h->n - 6) + 6.0 * (h->F - ndeg);
  const bool given = sigma2_in == sigma2_in;
  const double sigma2 = given ? sigma2_in : (m > p ? sums[0] / (m - p) : NAN);

  // ---- Sigma_cc, then the frame blocks
  hipEvent_t e0 = get_event(h), e1 = get_event(h);
  auto done = [&](int code) { h->pool.push_back(e0); h->pool.push_back(e1); return code; };
  const int ld = (int)cw.ld;
  (void)hipEventRecord(e0, h->stream);
  mcba::launch_cov_cam(h->stream, h->red, h->n, h->cw, gauge_camera, sigma2, W + cw.R, W + cw.M, W + cw.isd, W + cw.Sig, ld, ints);
  if ((rc = check_launch())) return done(rc);
  if (frame_cov) {
    if (mcba::launch_cov_frames(h->stream, h->rec2[h->lin], h->fbuf, flag, W + cw.Sig, ld, sigma2, W + cw.fout, h->C, h->F, h->Fpad, h->cw, G)) return done(fail(MCBA_ERR_HIP, "mcba_covariance: cannot launch k_cov_frames"));
    if ((rc = check_launch())) return done(rc);
  }
  (void)hipEventRecord(e1, h->stream);
  int pivot = -1;
  hipError_t e = hipMemcpyAsync(&pivot, ints, sizeof(int), hipMemcpyDeviceToHost, h->stream);
  if (e == hipSuccess && cam_cov) e = hipMemcpy2DAsync(cam_cov, (size_t)h->n * sizeof(double), W + cw.Sig, (size_t)ld * sizeof(double), (size_t)h->n * sizeof(double), h->n, hipMemcpyDeviceToHost, h->stream);
  if (e == hipSuccess && frame_cov) e = hipMemcpyAsync(frame_cov, W + cw.fout, (size_t)h->F * 36 * sizeof(double), hipMemcpyDeviceToHost, h->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
  float ms = 0.f;
  if (e == hipSuccess) e = hipEventElapsedTime(&ms, e0, e1);
  if (e != hipSuccess) { g_err = std::string("mcba_covariance: ") + hipGetErrorString(e); return done(MCBA_ERR_HIP); }
  info8[0] = sigma2; info8[1] = m; info8[2] = p; info8[3] = ndeg; info8[4] = pivot; info8[5] = ms; info8[6] = frame_cov ? G : 0; info8[7] = ld;
  if (pivot >= 0) {
    const int cam = pivot / h->cw, par = pivot % h->cw + (12 - h->cw);
    g_err = "mcba_covariance: the gauge-fixed Schur complement is not positive definite: pivot " + std::to_string(pivot) + " (camera " + std::to_string(cam) + ", parameter " + std::to_string(par) + ")";
    return done(MCBA_ERR_NONFINITE);
  }
  return done(MCBA_OK);
}

}  // extern "C"
