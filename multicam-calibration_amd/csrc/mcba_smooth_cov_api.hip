// mcba_smooth_cov_api.hip -- the stateless trajectory-uncertainty call of include/mcba.h (host arrays in, host arrays out, a device ordinal, no
// handle), in the idiom of mcba_smooth_api.hip: tracks run in the same chunks under the same device-memory budget (SmoothChunks of
// mcba_smooth_host.h).  Per chunk: prepare and count, the smoother's elimination of every level, the selected inversion of every level
// (mcba_smooth_cov.hip), one download.
#include "mcba_smooth_host.h"
#include "mcba_smooth_cov_math.h"

using namespace mcba_internal;

extern "C" {

int mcba_smooth_covariance(size_t n_frames, int n_tracks, const double* points, const double* cov6, const double* accel_std, const double* weights, int segment, int device, double* out_cov6,
                           double* out_lag9, int* status, int* n_usable, double* info8, double* kernel_ms) {
  const char* who = "mcba_smooth_covariance";
  if (n_frames < 1 || n_frames > ((size_t)1 << 31) || n_tracks < 1 || !points || !cov6 || !accel_std || !out_cov6 || !status || !n_usable || !info8)
    return fail(MCBA_ERR_ARG, "mcba_smooth_covariance: 1 .. 2^31 frames, at least one track, non-NULL arrays (but weights and out_lag9) required");
  const size_t T = n_frames, K = (size_t)n_tracks;
  if (int rc = smooth_check_common(who, "weights", T, n_tracks, accel_std, weights, segment)) return rc;
  if (int rc = stateless_device(device, who)) return rc;
  if (segment == 0) segment = mcba::SM_SEGMENT_DEFAULT;
  const bool lag = out_lag9 != nullptr;

  const double nan = __builtin_nan("");
  double ms_selinv = 0.0;

  SmoothChunks ch;
  StatelessCall& call = ch.call;
  if (int rc = ch.setup(who, T, K, segment, points, cov6, accel_std, weights, mcba::smooth_cov_chunk_doubles(T, 1, segment, lag), mcba::SM_ZC)) return rc;
  const int Kc = ch.Kc;
  double *d_oc = nullptr, *d_ol = nullptr;
  if (int rc = call.scratch(&d_oc, 6 * T * Kc)) return rc;
  if (lag) if (int rc = call.scratch(&d_ol, 9 * (T - 1) * Kc)) return rc;

  std::vector<double> h_oc, h_ol;
  std::vector<int> h_bad;
  for (int c = 0; c < ch.nchunks; ++c) {
    if (int rc = ch.begin(c)) return rc;
    const size_t tk = ch.tk, lk = (T - 1) * ch.kc;
    const int kc = ch.kc;
    // (ch.td has no x, d2, dx: the elimination reads p, winv, w and 1 / a^2 only: there is no solution, and the loss plays no part)
    h_bad.assign(kc, 0);
    h_oc.resize(6 * tk);
    if (lag) h_ol.resize(9 * lk);
    if (!ch.h_list.empty()) {
      const int nact = (int)ch.h_list.size();
      if (int rc = call.put(ch.d_list, ch.h_list.data(), (size_t)nact)) return rc;
      if (int rc = ch.open(true)) return rc;
      if (mcba::launch_smooth_reduce(nullptr, ch.lv, ch.levels, ch.td, kc, ch.d_list, nact, ch.d_bad) != 0) return fail(MCBA_ERR_ARG, "mcba_smooth_covariance: bad launch");
      if (int rc = check_launch()) return rc;
      if (int rc = ch.mark()) return rc;
      if (mcba::launch_smooth_selinv(nullptr, ch.lv, ch.levels, ch.td, ch.aux, d_oc, lag ? d_ol : nullptr, kc, ch.d_list, nact) != 0) return fail(MCBA_ERR_ARG, "mcba_smooth_covariance: bad launch");
      if (int rc = ch.close_split(ms_selinv)) return rc;
      if (int rc = call.download(h_bad.data(), ch.d_bad, (size_t)kc)) return rc;
      if (int rc = call.download(h_oc.data(), d_oc, 6 * tk)) return rc;
      if (lag && lk) if (int rc = call.download(h_ol.data(), d_ol, 9 * lk)) return rc;
    }
    for (int k = 0; k < kc; ++k) {
      const int st = ch.h_nus[k] < 2 ? mcba::SM_TOO_FEW_FRAMES : h_bad[k] ? mcba::SM_PIVOT : mcba::SM_OK;
      status[ch.k0 + k] = st;
      n_usable[ch.k0 + k] = ch.h_nus[k];
      ch.scatter(k, st == mcba::SM_OK, h_oc.data(), 6, out_cov6, nan);
      if (lag) ch.scatter(k, st == mcba::SM_OK, h_ol.data(), 9, out_lag9, nan, T - 1);
    }
  }
  ch.info(info8, kernel_ms, Kc, ch.nchunks, 1.0, (double)mcba::smooth_cov_chunk_doubles(T, Kc, segment, lag) * sizeof(double), ms_selinv);
  return MCBA_OK;
}

}  // extern "C"
