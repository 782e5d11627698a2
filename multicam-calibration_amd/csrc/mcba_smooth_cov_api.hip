// mcba_smooth_cov_api.hip -- the stateless trajectory-uncertainty call of include/mcba.h (host arrays in, host arrays out, a device ordinal, no
// handle), in the idiom of mcba_smooth_api.hip: tracks run in chunks that fit the same device-memory budget, each chunk gathered on the host
// into (T, Kc, .) planes.  Per chunk: prepare and count, the elimination of every level, the selected inversion of every level
// (mcba_smooth_cov.hip), one download.
#include "mcba_handle.h"
#include "mcba_smooth_cov_math.h"

using namespace mcba_internal;

namespace {

// device doubles (and ints, counted as doubles) one chunk of K tracks needs
size_t smooth_cov_chunk_doubles(size_t T, int K, int segment, bool lag) {
  mcba::SmLevel lv[mcba::SM_MAX_LEVELS];
  const int levels = mcba::smooth_plan(T, segment, K, lv);
  size_t n = (size_t)T * K * (20 + 6 + (lag ? 9 : 0)) + (size_t)K * 4;
  for (int l = 0; l < levels; ++l) n += lv[l].NS * (mcba::SM_FAC + (l ? mcba::SM_SEP + mcba::SM_ZC : 0));
  return n;
}

}  // namespace

extern "C" {

int mcba_smooth_covariance(size_t n_frames, int n_tracks, const double* points, const double* cov6, const double* accel_std, const double* weights, int segment, int device, double* out_cov6,
                           double* out_lag9, int* status, int* n_usable, double* info8, double* kernel_ms) {
  const char* who = "mcba_smooth_covariance";
  if (n_frames < 1 || n_frames > ((size_t)1 << 31) || n_tracks < 1 || !points || !cov6 || !accel_std || !out_cov6 || !status || !n_usable || !info8)
    return fail(MCBA_ERR_ARG, "mcba_smooth_covariance: 1 .. 2^31 frames, at least one track, non-NULL arrays (but weights and out_lag9) required");
  if (segment != 0 && (segment < mcba::SM_SEGMENT_MIN || segment > mcba::SM_SEGMENT_MAX)) return fail(MCBA_ERR_ARG, "mcba_smooth_covariance: segment must be 0 (the default) or 2 .. 64");
  for (int k = 0; k < n_tracks; ++k)
    if (!(accel_std[k] > 0.0) || !mcba::sm_finite(accel_std[k]) || !mcba::sm_finite(1.0 / (accel_std[k] * accel_std[k])) || !(1.0 / (accel_std[k] * accel_std[k]) > 0.0))
      return fail(MCBA_ERR_ARG, "mcba_smooth_covariance: accel_std must be positive and finite (and its inverse square too)");
  const size_t T = n_frames, K = (size_t)n_tracks;
  if (weights)
    for (size_t i = 0; i < T * K; ++i)
      if (!(weights[i] >= 0.0) || !mcba::sm_finite(weights[i])) return fail(MCBA_ERR_ARG, "mcba_smooth_covariance: weights must be finite and not negative");
  if (int rc = stateless_device(device, who)) return rc;
  if (segment == 0) segment = mcba::SM_SEGMENT_DEFAULT;
  const bool lag = out_lag9 != nullptr;

  // tracks per chunk from the smoother's budget (MCBA_SMOOTH_BUDGET_MB), at least one
  double budget_mb = 8192.0;
  if (const char* e = getenv("MCBA_SMOOTH_BUDGET_MB")) { const double v = atof(e); if (v > 0.0) budget_mb = v; }
  const double per_track = (double)smooth_cov_chunk_doubles(T, 1, segment, lag) * sizeof(double);
  const int Kc = (int)std::min<double>((double)K, std::max(1.0, floor(budget_mb * 1048576.0 / per_track)));
  const int nchunks = (int)((K + Kc - 1) / Kc);

  const double nan = __builtin_nan("");
  double ms_total = 0.0, ms_selinv = 0.0;
  int levels = 0;

  StatelessCall call;
  mcba::SmLevel lv[mcba::SM_MAX_LEVELS];
  double* zc[mcba::SM_MAX_LEVELS];
  const size_t TK = T * Kc, LK = (T - 1) * Kc;   // (the buffers are sized for the widest chunk: a narrower last one re-plans its levels inside them)
  double *d_pts = nullptr, *d_cov = nullptr, *d_win = nullptr, *d_p = nullptr, *d_winv = nullptr, *d_w = nullptr, *d_ia2 = nullptr, *d_lev = nullptr, *d_oc = nullptr, *d_ol = nullptr;
  int *d_nus = nullptr, *d_list = nullptr, *d_bad = nullptr;
  if (int rc = call.scratch(&d_pts, 3 * TK)) return rc;
  if (int rc = call.scratch(&d_cov, 6 * TK)) return rc;
  if (weights) if (int rc = call.scratch(&d_win, TK)) return rc;
  if (int rc = call.scratch(&d_p, 3 * TK)) return rc;
  if (int rc = call.scratch(&d_winv, 6 * TK)) return rc;
  if (int rc = call.scratch(&d_w, TK)) return rc;
  if (int rc = call.scratch(&d_ia2, (size_t)Kc)) return rc;
  if (int rc = call.scratch(&d_nus, (size_t)Kc)) return rc;
  if (int rc = call.scratch(&d_list, (size_t)Kc)) return rc;
  if (int rc = call.scratch(&d_bad, (size_t)Kc)) return rc;
  if (int rc = call.scratch(&d_oc, 6 * TK)) return rc;
  if (lag) if (int rc = call.scratch(&d_ol, 9 * LK)) return rc;
  size_t lev_doubles = 0;
  {
    const int L = mcba::smooth_plan(T, segment, Kc, lv);
    if (L < 1) return fail(MCBA_ERR_ARG, "mcba_smooth_covariance: too many levels");
    for (int l = 0; l < L; ++l) lev_doubles += lv[l].NS * (mcba::SM_FAC + (l ? mcba::SM_SEP + mcba::SM_ZC : 0));
  }
  if (int rc = call.scratch(&d_lev, lev_doubles)) return rc;
  hipEvent_t ev0 = nullptr, ev1 = nullptr, ev2 = nullptr;
  struct Events {
    hipEvent_t *a, *b, *c;
    ~Events() { if (*a) (void)hipEventDestroy(*a); if (*b) (void)hipEventDestroy(*b); if (*c) (void)hipEventDestroy(*c); }
  } events{&ev0, &ev1, &ev2};
  HIPCHK(hipEventCreate(&ev0));
  HIPCHK(hipEventCreate(&ev1));
  HIPCHK(hipEventCreate(&ev2));

  std::vector<double> h_pts, h_cov, h_win, h_ia2, h_oc, h_ol;
  std::vector<int> h_nus, h_list, h_bad;
  for (int c = 0; c < nchunks; ++c) {
    const size_t k0 = (size_t)c * Kc;
    const int kc = (int)std::min<size_t>(Kc, K - k0);
    const size_t tk = T * kc, lk = (T - 1) * kc;
    levels = mcba::smooth_plan(T, segment, kc, lv);
    {
      double* cur = d_lev;
      for (int l = 0; l < levels; ++l) {
        lv[l].fac = cur; cur += lv[l].NS * mcba::SM_FAC;
        zc[l] = nullptr;
        if (l) { lv[l].sep = cur; cur += lv[l].NS * mcba::SM_SEP; zc[l] = cur; cur += lv[l].NS * mcba::SM_ZC; }
      }
    }
    // gather the chunk's tracks (all of them: the arrays as they are)
    const double *s_pts = points, *s_cov = cov6, *s_win = weights;
    if (kc != (int)K) {
      h_pts.resize(3 * tk); h_cov.resize(6 * tk);
      if (weights) h_win.resize(tk);
      for (size_t t = 0; t < T; ++t) {
        memcpy(h_pts.data() + 3 * t * kc, points + 3 * (t * K + k0), 3 * kc * sizeof(double));
        memcpy(h_cov.data() + 6 * t * kc, cov6 + 6 * (t * K + k0), 6 * kc * sizeof(double));
        if (weights) memcpy(h_win.data() + t * kc, weights + t * K + k0, kc * sizeof(double));
      }
      s_pts = h_pts.data(); s_cov = h_cov.data(); s_win = weights ? h_win.data() : nullptr;
    }
    h_ia2.resize(kc);
    for (int k = 0; k < kc; ++k) h_ia2[k] = 1.0 / (accel_std[k0 + k] * accel_std[k0 + k]);
    if (int rc = call.put(d_pts, s_pts, 3 * tk)) return rc;
    if (int rc = call.put(d_cov, s_cov, 6 * tk)) return rc;
    if (s_win) if (int rc = call.put(d_win, s_win, tk)) return rc;
    if (int rc = call.put(d_ia2, h_ia2.data(), (size_t)kc)) return rc;
    HIPCHK(hipMemset(d_bad, 0, kc * sizeof(int)));

    // (the elimination reads p, winv, w and 1 / a^2 only: there is no solution, and the loss plays no part)
    mcba::SmData td{T, d_p, d_winv, d_w, d_ia2, nullptr, nullptr, nullptr, mcba::SM_LOSS_LINEAR, 1.0, 1.0};
    HIPCHK(hipEventRecord(ev0, nullptr));
    mcba::launch_smooth_prepare(nullptr, T, kc, d_pts, d_cov, s_win ? d_win : nullptr, d_p, d_winv, d_w, d_nus);
    if (int rc = check_launch()) return rc;
    HIPCHK(hipEventRecord(ev1, nullptr));
    HIPCHK(hipEventSynchronize(ev1));
    float ms = 0.f;
    HIPCHK(hipEventElapsedTime(&ms, ev0, ev1));
    ms_total += ms;
    h_nus.resize(kc); h_bad.assign(kc, 0);
    if (int rc = call.download(h_nus.data(), d_nus, (size_t)kc)) return rc;
    h_list.clear();
    for (int k = 0; k < kc; ++k)
      if (h_nus[k] >= 2) h_list.push_back(k);   // (the others are never launched)
    h_oc.resize(6 * tk);
    if (lag) h_ol.resize(9 * lk);
    if (!h_list.empty()) {
      const int nact = (int)h_list.size();
      if (int rc = call.put(d_list, h_list.data(), (size_t)nact)) return rc;
      HIPCHK(hipEventRecord(ev0, nullptr));
      if (mcba::launch_smooth_cov_reduce(nullptr, lv, levels, td, kc, d_list, nact, d_bad) != 0) return fail(MCBA_ERR_ARG, "mcba_smooth_covariance: bad launch");
      if (int rc = check_launch()) return rc;
      HIPCHK(hipEventRecord(ev1, nullptr));
      if (mcba::launch_smooth_selinv(nullptr, lv, levels, td, zc, d_oc, lag ? d_ol : nullptr, kc, d_list, nact) != 0) return fail(MCBA_ERR_ARG, "mcba_smooth_covariance: bad launch");
      if (int rc = check_launch()) return rc;
      HIPCHK(hipEventRecord(ev2, nullptr));
      HIPCHK(hipEventSynchronize(ev2));
      HIPCHK(hipEventElapsedTime(&ms, ev0, ev2));
      ms_total += ms;
      HIPCHK(hipEventElapsedTime(&ms, ev1, ev2));
      ms_selinv += ms;
      if (int rc = call.download(h_bad.data(), d_bad, (size_t)kc)) return rc;
      if (int rc = call.download(h_oc.data(), d_oc, 6 * tk)) return rc;
      if (lag && lk) if (int rc = call.download(h_ol.data(), d_ol, 9 * lk)) return rc;
    }
    for (int k = 0; k < kc; ++k) {
      const int st = h_nus[k] < 2 ? mcba::SM_TOO_FEW_FRAMES : h_bad[k] ? mcba::SM_PIVOT : mcba::SM_OK;
      const bool ok = st == mcba::SM_OK;
      status[k0 + k] = st;
      n_usable[k0 + k] = h_nus[k];
      for (size_t t = 0; t < T; ++t) {
        const size_t src = t * kc + k, dst = t * K + k0 + k;
        for (int e = 0; e < 6; ++e) out_cov6[6 * dst + e] = ok ? h_oc[6 * src + e] : nan;
        if (lag && t + 1 < T)
          for (int e = 0; e < 9; ++e) out_lag9[9 * dst + e] = ok ? h_ol[9 * src + e] : nan;
      }
    }
  }
  info8[0] = levels; info8[1] = segment; info8[2] = Kc; info8[3] = nchunks; info8[4] = ms_total; info8[5] = 1.0;
  info8[6] = (double)smooth_cov_chunk_doubles(T, Kc, segment, lag) * sizeof(double); info8[7] = ms_selinv;
  if (kernel_ms) *kernel_ms = ms_total;
  return MCBA_OK;
}

}  // extern "C"
