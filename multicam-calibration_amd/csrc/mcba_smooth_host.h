// mcba_smooth_host.h -- the host side that the calls on the smoother's elimination share (mcba_smooth_api.hip, mcba_smooth_cov_api.hip,
// mcba_smooth_evidence_api.hip; through mcba_traj_host.h: mcba_traj_refine_api.hip, mcba_skeltraj_api.hip; host only): the argument checks
// they make alike, and the walk over chunks of tracks.  Tracks are independent: they run in chunks that fit a fixed device-memory budget
// (MCBA_SMOOTH_BUDGET_MB: a test and tuning knob), each chunk gathered on the host into (T, kc, .) planes, prepared and counted here; what is
// done with the running tracks of a chunk -- the IRLS loop, the selected inversion, the candidates of the evidence -- is the entry point's
// own.  Plan, carve and chunk rule: mcba_smooth_math.h.  The timed brackets are StatelessCall's (mcba_handle.h).
#pragma once
#include "mcba_handle.h"
#include "mcba_smooth_math.h"

namespace mcba_internal {

// the weights of a smoother's call (count of them, or NULL); weights_name: the parameter
inline int smooth_check_weights(const char* who, const char* weights_name, const double* weights, size_t count) {
  if (weights)
    for (size_t i = 0; i < count; ++i)
      if (!(weights[i] >= 0.0) || !mcba::sm_finite(weights[i])) { g_err = std::string(who) + ": " + weights_name + " must be finite and not negative"; return MCBA_ERR_ARG; }
  return MCBA_OK;
}

// segment, accel_std (K) and the weights (T K of them, or NULL), checked in this order after the entry's own checks
inline int smooth_check_common(const char* who, const char* weights_name, size_t T, int K, const double* accel_std, const double* weights, int segment) {
  if (segment != 0 && (segment < mcba::SM_SEGMENT_MIN || segment > mcba::SM_SEGMENT_MAX)) { g_err = std::string(who) + ": segment must be 0 (the default) or 2 .. 64"; return MCBA_ERR_ARG; }
  for (int k = 0; k < K; ++k)
    if (!(accel_std[k] > 0.0) || !mcba::sm_finite(accel_std[k]) || !mcba::sm_finite(1.0 / (accel_std[k] * accel_std[k])) || !(1.0 / (accel_std[k] * accel_std[k]) > 0.0)) {
      g_err = std::string(who) + ": accel_std must be positive and finite (and its inverse square too)";
      return MCBA_ERR_ARG;
    }
  return smooth_check_weights(who, weights_name, weights, T * (size_t)K);
}

// the device-memory budget of one chunk in bytes: MCBA_SMOOTH_BUDGET_MB, 8192 where it is unset or not positive
inline double smooth_budget_bytes() {
  double budget_mb = 8192.0;
  if (const char* e = getenv("MCBA_SMOOTH_BUDGET_MB")) { const double v = atof(e); if (v > 0.0) budget_mb = v; }
  return budget_mb * 1048576.0;
}

// tracks k0 .. k0 + kc - 1 of a (lead, T, K, n) array as (lead, T, kc, n): the array as it is where they are all of it, else gathered into buf
inline const double* gather_tracks(const double* src, size_t lead, size_t T, size_t K, size_t k0, size_t kc, size_t n, std::vector<double>& buf) {
  if (kc == K) return src;
  buf.resize(lead * T * kc * n);
  for (size_t r = 0; r < lead * T; ++r) memcpy(buf.data() + r * kc * n, src + (r * K + k0) * n, kc * n * sizeof(double));
  return buf.data();
}

// One call's walk over its chunks.  setup() once, then per chunk c < nchunks: begin(c), the entry's own launches on list, scatter() per output.
// What every trajectory call shares is setup_shared() / begin_shared(): the budget and the chunk width, the levels, 1 / a^2, the list, d_bad, the
// events.  setup() / begin() add the data planes of the calls that take points and covariances (upload, prepare, count); a call with data
// planes of its own (TrackFit, mcba_traj_host.h) uses the shared pair and fills h_list itself
struct SmoothChunks {
  StatelessCall call;   // every device buffer of the call, and the events of its brackets
  const char* who = nullptr;
  size_t T = 0, K = 0;
  int segment = 0, extra = 0, Kc = 0, nchunks = 0;
  const double *points = nullptr, *cov6 = nullptr, *weights = nullptr;
  const double* accel_std = nullptr;   // (K); NULL: the call has no value per track to begin with and sets every candidate itself (set_accel)
  double *d_pts = nullptr, *d_cov = nullptr, *d_win = nullptr, *d_p = nullptr, *d_winv = nullptr, *d_w = nullptr, *d_ia2 = nullptr, *d_lev = nullptr;
  int *d_nus = nullptr, *d_list = nullptr, *d_bad = nullptr;
  double ms_total = 0.0;   // kernel time so far: begin() adds its prepare, close() what the entry brackets
  // the chunk begin(c) left: tracks k0 .. k0 + kc - 1, tk = T kc, its levels carved into d_lev (aux[l]: the `extra` plane of level l >= 1),
  // td = (T, p, winv, w, 1 / a^2) for the entry to complete, n_usable per track and the list of tracks that run (two usable frames or more)
  size_t k0 = 0, tk = 0;
  int kc = 0, levels = 0;
  mcba::SmLevel lv[mcba::SM_MAX_LEVELS];
  double* aux[mcba::SM_MAX_LEVELS];
  mcba::SmData td{};
  std::vector<double> h_pts, h_cov, h_win, h_ia2;
  std::vector<int> h_nus, h_list;

  // per_track: the device doubles one track takes (the entry's *_chunk_doubles at K = 1); extra: doubles per separator node beyond fac and sep.
  // The buffers are sized for the widest chunk: a narrower last one re-plans its levels inside them
  int setup_shared(const char* who_, size_t T_, size_t K_, int segment_, const double* accel_std_, size_t per_track, int extra_) {
    who = who_; T = T_; K = K_; segment = segment_; accel_std = accel_std_; extra = extra_;
    Kc = mcba::smooth_chunk_tracks(smooth_budget_bytes(), per_track, K, nchunks);
    if (int rc = call.scratch(&d_ia2, (size_t)Kc)) return rc;
    if (int rc = call.scratch(&d_nus, (size_t)Kc)) return rc;
    if (int rc = call.scratch(&d_list, (size_t)Kc)) return rc;
    if (int rc = call.scratch(&d_bad, (size_t)Kc)) return rc;
    const size_t lev_doubles = mcba::smooth_carve(T, segment, Kc, lv, extra, nullptr, nullptr);
    if (lev_doubles == 0) { g_err = std::string(who) + ": too many levels"; return MCBA_ERR_ARG; }
    if (int rc = call.scratch(&d_lev, lev_doubles)) return rc;
    HIPCHK(hipEventCreate(&call.e0));
    HIPCHK(hipEventCreate(&call.e1));
    return MCBA_OK;
  }
  int setup(const char* who_, size_t T_, size_t K_, int segment_, const double* points_, const double* cov6_, const double* accel_std_, const double* weights_, size_t per_track, int extra_) {
    points = points_; cov6 = cov6_; weights = weights_;
    if (int rc = setup_shared(who_, T_, K_, segment_, accel_std_, per_track, extra_)) return rc;
    const size_t TK = T * Kc;
    if (int rc = call.scratch(&d_pts, 3 * TK)) return rc;
    if (int rc = call.scratch(&d_cov, 6 * TK)) return rc;
    if (weights) if (int rc = call.scratch(&d_win, TK)) return rc;
    if (int rc = call.scratch(&d_p, 3 * TK)) return rc;
    if (int rc = call.scratch(&d_winv, 6 * TK)) return rc;
    if (int rc = call.scratch(&d_w, TK)) return rc;
    return MCBA_OK;
  }

  // a timed bracket of launches whose time goes to ms_total; close_split: the time after the mark to part as well (StatelessCall)
  int open(bool split = false) { return call.open(split); }
  int mark() { return call.mark(); }
  int close() { return call.close(ms_total); }
  int close_split(double& part) { return call.close_split(ms_total, part); }

  int tracks_of(int c) const { return (int)std::min<size_t>(Kc, K - (size_t)c * Kc); }   // (the last chunk may be narrower)

  // 1 / a^2 of the chunk's tracks (a: kc values) on the device and d_bad cleared, ahead of an elimination.  The kernels read 1 / a^2 at the
  // tracks of their list only (k = list[..] in smooth_reduce_lane, smooth_resolve_lane and smooth_backsub_lane), so at a track that does not
  // run any value of a will do
  int set_accel(const double* a) {
    h_ia2.resize(kc);
    for (int k = 0; k < kc; ++k) h_ia2[k] = 1.0 / (a[k] * a[k]);
    if (int rc = call.put(d_ia2, h_ia2.data(), (size_t)kc)) return rc;
    HIPCHK(hipMemset(d_bad, 0, kc * sizeof(int)));
    return MCBA_OK;
  }

  // the chunk's tracks and its levels; with one accel_std per track: set_accel
  int begin_shared(int c) {
    k0 = (size_t)c * Kc;
    kc = tracks_of(c);
    tk = T * kc;
    mcba::smooth_carve(T, segment, kc, lv, extra, d_lev, aux, &levels);
    return accel_std ? set_accel(accel_std + k0) : MCBA_OK;
  }

  int begin(int c) {
    if (int rc = begin_shared(c)) return rc;
    const double* s_pts = gather_tracks(points, 1, T, K, k0, kc, 3, h_pts);
    const double* s_cov = gather_tracks(cov6, 1, T, K, k0, kc, 6, h_cov);
    const double* s_win = weights ? gather_tracks(weights, 1, T, K, k0, kc, 1, h_win) : nullptr;
    if (int rc = call.put(d_pts, s_pts, 3 * tk)) return rc;
    if (int rc = call.put(d_cov, s_cov, 6 * tk)) return rc;
    if (s_win) if (int rc = call.put(d_win, s_win, tk)) return rc;
    td = mcba::SmData{T, d_p, d_winv, d_w, d_ia2, nullptr, nullptr, nullptr, mcba::SM_LOSS_LINEAR, 1.0, 1.0};
    if (int rc = open()) return rc;
    mcba::launch_smooth_prepare(nullptr, T, kc, d_pts, d_cov, s_win ? d_win : nullptr, d_p, d_winv, d_w, d_nus);
    if (int rc = close()) return rc;
    h_nus.resize(kc);
    if (int rc = call.download(h_nus.data(), d_nus, (size_t)kc)) return rc;
    h_list.clear();
    for (int k = 0; k < kc; ++k)
      if (h_nus[k] >= 2) h_list.push_back(k);   // (the others are never launched)
    return MCBA_OK;
  }

  // info8 and *kernel_ms of the call: the levels, the segment and the kernel time from here, the other slots as the entry has them
  void info(double* info8, double* kernel_ms, double s2, double s3, double s5, double device_bytes, double s7) const {
    fill_info8(info8, kernel_ms, levels, segment, s2, s3, ms_total, s5, device_bytes, s7);
  }

  // one output plane of track k of the chunk: src (T, kc, n) -> dst (T, K, n), the first `rows` frames of it (all, by default); a track that
  // is not SM_OK gets `off` throughout
  void scatter(int k, bool ok, const double* src, int n, double* dst, double off, size_t rows = (size_t)-1) const {
    for (size_t t = 0; t < std::min(rows, T); ++t)
      for (int e = 0; e < n; ++e) dst[n * (t * K + k0 + k) + e] = ok ? src[n * (t * kc + k) + e] : off;
  }
};

}  // namespace mcba_internal
