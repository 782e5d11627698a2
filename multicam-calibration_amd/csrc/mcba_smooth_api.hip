// mcba_smooth_api.hip -- the stateless trajectory-smoothing call of include/mcba.h (host arrays in, host arrays out, a device ordinal, no handle),
// in the idiom of mcba_tricov_api.hip.  Tracks are independent: they are solved in chunks that fit a fixed device-memory budget, each chunk
// gathered on the host into (T, Kc, .) planes.  The IRLS loop is here: per iteration the kernels of mcba_smooth.hip back to back and one small
// download (four doubles and a flag per running track), as mcba_refine_extrinsics does.
#include "mcba_handle.h"
#include "mcba_smooth_math.h"

using namespace mcba_internal;

namespace {

// device doubles (and ints, counted as doubles) one chunk of K tracks needs
size_t smooth_chunk_doubles(size_t T, int K, int segment) {
  mcba::SmLevel lv[mcba::SM_MAX_LEVELS];
  const int levels = mcba::smooth_plan(T, segment, K, lv);
  size_t n = (size_t)T * K * 24 + (size_t)K * 8 + (size_t)4 * mcba::smooth_eval_blocks(T) * K;
  for (int l = 0; l < levels; ++l) n += lv[l].NS * (mcba::SM_FAC + (l ? mcba::SM_SEP + 6 : 0));
  return n;
}

}  // namespace

extern "C" {

int mcba_smooth_trajectories(size_t n_frames, int n_tracks, const double* points, const double* cov6, const double* accel_std, const double* weights_in, int loss, double f_scale,
                             int max_iterations, double xtol, int segment, int device, double* out_points, double* out_weights, double* out_d2, int* status, int* n_usable, int* n_iterations,
                             double* history, double* info8, double* kernel_ms) {
  const char* who = "mcba_smooth_trajectories";
  if (n_frames < 1 || n_frames > ((size_t)1 << 31) || n_tracks < 1 || !points || !cov6 || !accel_std || !out_points || !out_weights || !out_d2 || !status || !n_usable || !n_iterations || !history || !info8)
    return fail(MCBA_ERR_ARG, "mcba_smooth_trajectories: 1 .. 2^31 frames, at least one track, non-NULL arrays required");
  if (loss < mcba::SM_LOSS_LINEAR || loss > mcba::SM_LOSS_HUBER)
    return fail(MCBA_ERR_ARG, "mcba_smooth_trajectories: loss must be linear, soft_l1 or huber (0 .. 2): the IRLS loop is a majorise-minimise scheme for convex losses only");
  if (!(f_scale > 0.0) || !mcba::sm_finite(f_scale)) return fail(MCBA_ERR_ARG, "mcba_smooth_trajectories: f_scale must be positive and finite");
  if (max_iterations < 1) return fail(MCBA_ERR_ARG, "mcba_smooth_trajectories: max_iterations >= 1");
  if (!(xtol >= 0.0)) return fail(MCBA_ERR_ARG, "mcba_smooth_trajectories: xtol >= 0");
  if (segment != 0 && (segment < mcba::SM_SEGMENT_MIN || segment > mcba::SM_SEGMENT_MAX)) return fail(MCBA_ERR_ARG, "mcba_smooth_trajectories: segment must be 0 (the default) or 2 .. 64");
  for (int k = 0; k < n_tracks; ++k)
    if (!(accel_std[k] > 0.0) || !mcba::sm_finite(accel_std[k]) || !mcba::sm_finite(1.0 / (accel_std[k] * accel_std[k])) || !(1.0 / (accel_std[k] * accel_std[k]) > 0.0))
      return fail(MCBA_ERR_ARG, "mcba_smooth_trajectories: accel_std must be positive and finite (and its inverse square too)");
  const size_t T = n_frames, K = (size_t)n_tracks;
  if (weights_in)
    for (size_t i = 0; i < T * K; ++i)
      if (!(weights_in[i] >= 0.0) || !mcba::sm_finite(weights_in[i])) return fail(MCBA_ERR_ARG, "mcba_smooth_trajectories: weights_in must be finite and not negative");
  if (int rc = stateless_device(device, who)) return rc;
  if (segment == 0) segment = mcba::SM_SEGMENT_DEFAULT;

  // tracks per chunk from the budget (MCBA_SMOOTH_BUDGET_MB: a test and tuning knob), at least one
  double budget_mb = 8192.0;
  if (const char* e = getenv("MCBA_SMOOTH_BUDGET_MB")) { const double v = atof(e); if (v > 0.0) budget_mb = v; }
  const double per_track = (double)smooth_chunk_doubles(T, 1, segment) * sizeof(double);
  int Kc = (int)std::min<double>((double)K, std::max(1.0, floor(budget_mb * 1048576.0 / per_track)));
  const int nchunks = (int)((K + Kc - 1) / Kc);

  const double nan = __builtin_nan("");
  for (size_t i = 0; i < (size_t)max_iterations * K * 2; ++i) history[i] = nan;
  double ms_total = 0.0;
  int levels = 0, most_solves = 0;

  StatelessCall call;
  mcba::SmLevel lv[mcba::SM_MAX_LEVELS];
  const size_t TK = T * Kc;   // (the buffers are sized for the widest chunk: a narrower last one re-plans its levels inside them)
  const int nblk = mcba::smooth_eval_blocks(T);
  double *d_pts = nullptr, *d_cov = nullptr, *d_win = nullptr, *d_p = nullptr, *d_winv = nullptr, *d_w = nullptr, *d_x = nullptr, *d_d2 = nullptr, *d_dx = nullptr, *d_ia2 = nullptr, *d_part = nullptr,
         *d_res = nullptr, *d_lev = nullptr;
  int *d_nus = nullptr, *d_list = nullptr, *d_bad = nullptr;
  if (int rc = call.scratch(&d_pts, 3 * TK)) return rc;
  if (int rc = call.scratch(&d_cov, 6 * TK)) return rc;
  if (weights_in) if (int rc = call.scratch(&d_win, TK)) return rc;
  if (int rc = call.scratch(&d_p, 3 * TK)) return rc;
  if (int rc = call.scratch(&d_winv, 6 * TK)) return rc;
  if (int rc = call.scratch(&d_w, TK)) return rc;
  if (int rc = call.scratch(&d_x, 3 * TK)) return rc;
  if (int rc = call.scratch(&d_d2, TK)) return rc;
  if (int rc = call.scratch(&d_dx, TK)) return rc;
  if (int rc = call.scratch(&d_ia2, (size_t)Kc)) return rc;
  if (int rc = call.scratch(&d_part, (size_t)4 * nblk * Kc)) return rc;
  if (int rc = call.scratch(&d_res, (size_t)4 * Kc)) return rc;
  if (int rc = call.scratch(&d_nus, (size_t)Kc)) return rc;
  if (int rc = call.scratch(&d_list, (size_t)Kc)) return rc;
  if (int rc = call.scratch(&d_bad, (size_t)Kc)) return rc;
  size_t lev_doubles = 0;
  {
    const int L = mcba::smooth_plan(T, segment, Kc, lv);
    if (L < 1) return fail(MCBA_ERR_ARG, "mcba_smooth_trajectories: too many levels");
    for (int l = 0; l < L; ++l) lev_doubles += lv[l].NS * (mcba::SM_FAC + (l ? mcba::SM_SEP + 6 : 0));
  }
  if (int rc = call.scratch(&d_lev, lev_doubles)) return rc;
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  HIPCHK(hipEventCreate(&ev0));
  if (hipEventCreate(&ev1) != hipSuccess) { (void)hipEventDestroy(ev0); return fail(MCBA_ERR_HIP, "mcba_smooth_trajectories: hipEventCreate"); }
  struct Events { hipEvent_t a, b; ~Events() { (void)hipEventDestroy(a); (void)hipEventDestroy(b); } } events{ev0, ev1};

  std::vector<double> h_pts, h_cov, h_win, h_x, h_w, h_d2, h_ia2, h_res;
  std::vector<int> h_nus, h_list, h_bad, h_stat, h_nit;
  for (int c = 0; c < nchunks; ++c) {
    const size_t k0 = (size_t)c * Kc;
    const int kc = (int)std::min<size_t>(Kc, K - k0);
    const size_t tk = T * kc;
    levels = mcba::smooth_plan(T, segment, kc, lv);
    {
      double* cur = d_lev;
      for (int l = 0; l < levels; ++l) {
        lv[l].fac = cur; cur += lv[l].NS * mcba::SM_FAC;
        if (l) { lv[l].sep = cur; cur += lv[l].NS * mcba::SM_SEP; lv[l].x = cur; cur += lv[l].NS * 6; }
      }
    }
    // gather the chunk's tracks (all of them: the arrays as they are)
    const double *s_pts = points, *s_cov = cov6, *s_win = weights_in;
    if (kc != (int)K) {
      h_pts.resize(3 * tk); h_cov.resize(6 * tk);
      if (weights_in) h_win.resize(tk);
      for (size_t t = 0; t < T; ++t) {
        memcpy(h_pts.data() + 3 * t * kc, points + 3 * (t * K + k0), 3 * kc * sizeof(double));
        memcpy(h_cov.data() + 6 * t * kc, cov6 + 6 * (t * K + k0), 6 * kc * sizeof(double));
        if (weights_in) memcpy(h_win.data() + t * kc, weights_in + t * K + k0, kc * sizeof(double));
      }
      s_pts = h_pts.data(); s_cov = h_cov.data(); s_win = weights_in ? h_win.data() : nullptr;
    }
    h_ia2.resize(kc);
    for (int k = 0; k < kc; ++k) h_ia2[k] = 1.0 / (accel_std[k0 + k] * accel_std[k0 + k]);
    if (int rc = call.put(d_pts, s_pts, 3 * tk)) return rc;
    if (int rc = call.put(d_cov, s_cov, 6 * tk)) return rc;
    if (s_win) if (int rc = call.put(d_win, s_win, tk)) return rc;
    if (int rc = call.put(d_ia2, h_ia2.data(), (size_t)kc)) return rc;
    HIPCHK(hipMemset(d_x, 0, 3 * tk * sizeof(double)));   // (the first solve's step is measured against it and never used)
    HIPCHK(hipMemset(d_d2, 0, tk * sizeof(double)));
    HIPCHK(hipMemset(d_bad, 0, kc * sizeof(int)));

    mcba::SmData td{T, d_p, d_winv, d_w, d_ia2, d_x, d_d2, d_dx, loss, f_scale * f_scale, 1.0 / (f_scale * f_scale)};
    HIPCHK(hipEventRecord(ev0, nullptr));
    mcba::launch_smooth_prepare(nullptr, T, kc, d_pts, d_cov, s_win ? d_win : nullptr, d_p, d_winv, d_w, d_nus);
    if (int rc = check_launch()) return rc;
    HIPCHK(hipEventRecord(ev1, nullptr));
    HIPCHK(hipEventSynchronize(ev1));
    float ms = 0.f;
    HIPCHK(hipEventElapsedTime(&ms, ev0, ev1));
    ms_total += ms;
    h_nus.resize(kc); h_stat.assign(kc, mcba::SM_OK); h_nit.assign(kc, 0); h_bad.resize(kc); h_res.resize((size_t)4 * kc);
    if (int rc = call.download(h_nus.data(), d_nus, (size_t)kc)) return rc;
    h_list.clear();
    for (int k = 0; k < kc; ++k) {
      if (h_nus[k] < 2) h_stat[k] = mcba::SM_TOO_FEW_FRAMES;   // never launched
      else h_list.push_back(k);
    }
    for (int it = 0; it < max_iterations && !h_list.empty(); ++it) {
      const int nact = (int)h_list.size();
      if (int rc = call.put(d_list, h_list.data(), (size_t)nact)) return rc;
      HIPCHK(hipEventRecord(ev0, nullptr));
      if (mcba::launch_smooth_solve(nullptr, lv, levels, td, kc, d_list, nact, d_bad, d_part, d_res) != 0) return fail(MCBA_ERR_ARG, "mcba_smooth_trajectories: bad launch");
      if (int rc = check_launch()) return rc;
      HIPCHK(hipEventRecord(ev1, nullptr));
      HIPCHK(hipEventSynchronize(ev1));
      HIPCHK(hipEventElapsedTime(&ms, ev0, ev1));
      ms_total += ms;
      if (int rc = call.download(h_res.data(), d_res, (size_t)4 * nact)) return rc;
      if (int rc = call.download(h_bad.data(), d_bad, (size_t)kc)) return rc;
      most_solves = std::max(most_solves, it + 1);
      std::vector<int> next;
      for (int kk = 0; kk < nact; ++kk) {
        const int k = h_list[kk];
        const double obj = h_res[4 * kk], step = it == 0 ? HUGE_VAL : h_res[4 * kk + 1], xmax = h_res[4 * kk + 2];
        h_nit[k] = it + 1;
        history[((size_t)it * K + k0 + k) * 2] = obj;
        history[((size_t)it * K + k0 + k) * 2 + 1] = step;
        if (h_bad[k]) { h_stat[k] = mcba::SM_PIVOT; continue; }
        if (!mcba::smooth_stops(loss, it, max_iterations, step, xmax, xtol)) next.push_back(k);
      }
      h_list.swap(next);
    }
    h_x.resize(3 * tk); h_w.resize(tk); h_d2.resize(tk);
    if (int rc = call.download(h_x.data(), d_x, 3 * tk)) return rc;
    if (int rc = call.download(h_w.data(), d_w, tk)) return rc;
    if (int rc = call.download(h_d2.data(), d_d2, tk)) return rc;
    for (int k = 0; k < kc; ++k) {
      const bool ok = h_stat[k] == mcba::SM_OK;
      status[k0 + k] = h_stat[k];
      n_usable[k0 + k] = h_nus[k];
      n_iterations[k0 + k] = h_nit[k];
      for (size_t t = 0; t < T; ++t) {
        const size_t src = t * kc + k, dst = t * K + k0 + k;
        for (int e = 0; e < 3; ++e) out_points[3 * dst + e] = ok ? h_x[3 * src + e] : nan;
        out_weights[dst] = ok ? h_w[src] : 0.0;
        out_d2[dst] = ok ? h_d2[src] : nan;
      }
    }
  }
  info8[0] = levels; info8[1] = segment; info8[2] = Kc; info8[3] = nchunks; info8[4] = ms_total; info8[5] = most_solves;
  info8[6] = (double)smooth_chunk_doubles(T, Kc, segment) * sizeof(double); info8[7] = 0.0;
  if (kernel_ms) *kernel_ms = ms_total;
  return MCBA_OK;
}

}  // extern "C"
