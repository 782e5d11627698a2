// mcba_smooth_host.h -- the host side that mcba_smooth_api.hip and mcba_smooth_cov_api.hip share (host only): the argument checks both make, and
// the walk over chunks of tracks.  Tracks are independent: they run in chunks that fit a fixed device-memory budget (MCBA_SMOOTH_BUDGET_MB: a
// test and tuning knob), each chunk gathered on the host into (T, kc, .) planes, prepared and counted here; what is done with the running
// tracks of a chunk -- the IRLS loop, the selected inversion -- is the entry point's own.  Plan, carve and chunk rule: mcba_smooth_math.h.
#pragma once
#include "mcba_handle.h"
#include "mcba_smooth_math.h"

namespace mcba_internal {

// segment, accel_std (K) and the weights (T K of them, or NULL), checked in this order after the entry's own checks; weights_name: the parameter
inline int smooth_check_common(const char* who, const char* weights_name, size_t T, int K, const double* accel_std, const double* weights, int segment) {
  if (segment != 0 && (segment < mcba::SM_SEGMENT_MIN || segment > mcba::SM_SEGMENT_MAX)) { g_err = std::string(who) + ": segment must be 0 (the default) or 2 .. 64"; return MCBA_ERR_ARG; }
  for (int k = 0; k < K; ++k)
    if (!(accel_std[k] > 0.0) || !mcba::sm_finite(accel_std[k]) || !mcba::sm_finite(1.0 / (accel_std[k] * accel_std[k])) || !(1.0 / (accel_std[k] * accel_std[k]) > 0.0)) {
      g_err = std::string(who) + ": accel_std must be positive and finite (and its inverse square too)";
      return MCBA_ERR_ARG;
    }
  if (weights)
    for (size_t i = 0; i < T * (size_t)K; ++i)
      if (!(weights[i] >= 0.0) || !mcba::sm_finite(weights[i])) { g_err = std::string(who) + ": " + weights_name + " must be finite and not negative"; return MCBA_ERR_ARG; }
  return MCBA_OK;
}

// the device-memory budget of one chunk in bytes: MCBA_SMOOTH_BUDGET_MB, 8192 where it is unset or not positive
inline double smooth_budget_bytes() {
  double budget_mb = 8192.0;
  if (const char* e = getenv("MCBA_SMOOTH_BUDGET_MB")) { const double v = atof(e); if (v > 0.0) budget_mb = v; }
  return budget_mb * 1048576.0;
}

// One call's walk over its chunks.  setup() once, then per chunk c < nchunks: begin(c), the entry's own launches on list, scatter() per output.
// What every trajectory call shares is setup_shared() / begin_shared(): the budget and the chunk width, the levels, 1 / a^2, the list, d_bad, the
// events.  setup() / begin() add the data planes of the two calls that take points and covariances (upload, prepare, count); a call with data
// planes of its own (mcba_traj_refine_api.hip) uses the shared pair and fills h_list itself
struct SmoothChunks {
  StatelessCall call;        // every device buffer of the call, and the events e0, e1 around its launches
  hipEvent_t e2 = nullptr;   // a third event for a call that times a part of its bracket: created by that call, released here
  const char* who = nullptr;
  size_t T = 0, K = 0;
  int segment = 0, extra = 0, Kc = 0, nchunks = 0;
  const double *points = nullptr, *cov6 = nullptr, *accel_std = nullptr, *weights = nullptr;
  double *d_pts = nullptr, *d_cov = nullptr, *d_win = nullptr, *d_p = nullptr, *d_winv = nullptr, *d_w = nullptr, *d_ia2 = nullptr, *d_lev = nullptr;
  int *d_nus = nullptr, *d_list = nullptr, *d_bad = nullptr;
  double ms_total = 0.0;   // kernel time so far: begin() adds its prepare, add_ms() what the entry brackets
  // the chunk begin(c) left: tracks k0 .. k0 + kc - 1, tk = T kc, its levels carved into d_lev (aux[l]: the `extra` plane of level l >= 1),
  // td = (T, p, winv, w, 1 / a^2) for the entry to complete, n_usable per track and the list of tracks that run (two usable frames or more)
  size_t k0 = 0, tk = 0;
  int kc = 0, levels = 0;
  mcba::SmLevel lv[mcba::SM_MAX_LEVELS];
  double* aux[mcba::SM_MAX_LEVELS];
  mcba::SmData td{};
  std::vector<double> h_pts, h_cov, h_win, h_ia2;
  std::vector<int> h_nus, h_list;

  ~SmoothChunks() { if (e2) (void)hipEventDestroy(e2); }

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

  // the time between two recorded events, the later one complete, added to sum
  int add_ms(hipEvent_t from, hipEvent_t to, double& sum) {
    float ms = 0.f;
    HIPCHK(hipEventElapsedTime(&ms, from, to));
    sum += ms;
    return MCBA_OK;
  }

  int tracks_of(int c) const { return (int)std::min<size_t>(Kc, K - (size_t)c * Kc); }   // (the last chunk may be narrower)

  // the chunk's tracks, its levels, 1 / a^2 on the device, d_bad cleared
  int begin_shared(int c) {
    k0 = (size_t)c * Kc;
    kc = tracks_of(c);
    tk = T * kc;
    mcba::smooth_carve(T, segment, kc, lv, extra, d_lev, aux, &levels);
    h_ia2.resize(kc);
    for (int k = 0; k < kc; ++k) h_ia2[k] = 1.0 / (accel_std[k0 + k] * accel_std[k0 + k]);
    if (int rc = call.put(d_ia2, h_ia2.data(), (size_t)kc)) return rc;
    HIPCHK(hipMemset(d_bad, 0, kc * sizeof(int)));
    return MCBA_OK;
  }

  int begin(int c) {
    if (int rc = begin_shared(c)) return rc;
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
    if (int rc = call.put(d_pts, s_pts, 3 * tk)) return rc;
    if (int rc = call.put(d_cov, s_cov, 6 * tk)) return rc;
    if (s_win) if (int rc = call.put(d_win, s_win, tk)) return rc;
    td = mcba::SmData{T, d_p, d_winv, d_w, d_ia2, nullptr, nullptr, nullptr, mcba::SM_LOSS_LINEAR, 1.0, 1.0};
    HIPCHK(hipEventRecord(call.e0, nullptr));
    mcba::launch_smooth_prepare(nullptr, T, kc, d_pts, d_cov, s_win ? d_win : nullptr, d_p, d_winv, d_w, d_nus);
    if (int rc = check_launch()) return rc;
    HIPCHK(hipEventRecord(call.e1, nullptr));
    HIPCHK(hipEventSynchronize(call.e1));
    if (int rc = add_ms(call.e0, call.e1, ms_total)) return rc;
    h_nus.resize(kc);
    if (int rc = call.download(h_nus.data(), d_nus, (size_t)kc)) return rc;
    h_list.clear();
    for (int k = 0; k < kc; ++k)
      if (h_nus[k] >= 2) h_list.push_back(k);   // (the others are never launched)
    return MCBA_OK;
  }

  // one output plane of track k of the chunk: src (T, kc, n) -> dst (T, K, n), the first `rows` frames of it (all, by default); a track that
  // is not SM_OK gets `off` throughout
  void scatter(int k, bool ok, const double* src, int n, double* dst, double off, size_t rows = (size_t)-1) const {
    for (size_t t = 0; t < std::min(rows, T); ++t)
      for (int e = 0; e < n; ++e) dst[n * (t * K + k0 + k) + e] = ok ? src[n * (t * kc + k) + e] : off;
  }
};

}  // namespace mcba_internal
