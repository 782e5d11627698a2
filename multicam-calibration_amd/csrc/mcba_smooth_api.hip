// mcba_smooth_api.hip -- the stateless trajectory-smoothing call of include/mcba.h (host arrays in, host arrays out, a device ordinal, no handle),
// in the idiom of mcba_tricov_api.hip.  The walk over chunks of tracks and the timed brackets are SmoothChunks of mcba_smooth_host.h.  The
// IRLS loop is here: per iteration the kernels of mcba_smooth.hip back to back and one small download (four doubles and a flag per running
// track), as mcba_refine_extrinsics does.
#include "mcba_smooth_host.h"

using namespace mcba_internal;

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
  const size_t T = n_frames, K = (size_t)n_tracks;
  if (int rc = smooth_check_common(who, "weights_in", T, n_tracks, accel_std, weights_in, segment)) return rc;
  if (int rc = stateless_device(device, who)) return rc;
  if (segment == 0) segment = mcba::SM_SEGMENT_DEFAULT;

  const double nan = __builtin_nan("");
  for (size_t i = 0; i < (size_t)max_iterations * K * 2; ++i) history[i] = nan;
  int most_solves = 0;

  SmoothChunks ch;
  StatelessCall& call = ch.call;
  if (int rc = ch.setup(who, T, K, segment, points, cov6, accel_std, weights_in, mcba::smooth_chunk_doubles(T, 1, segment), 6)) return rc;
  const int Kc = ch.Kc, nblk = mcba::smooth_eval_blocks(T);
  const size_t TK = T * Kc;
  double *d_x = nullptr, *d_d2 = nullptr, *d_dx = nullptr, *d_part = nullptr, *d_res = nullptr;
  if (int rc = call.scratch(&d_x, 3 * TK)) return rc;
  if (int rc = call.scratch(&d_d2, TK)) return rc;
  if (int rc = call.scratch(&d_dx, TK)) return rc;
  if (int rc = call.scratch(&d_part, (size_t)4 * nblk * Kc)) return rc;
  if (int rc = call.scratch(&d_res, (size_t)4 * Kc)) return rc;

  std::vector<double> h_x, h_w, h_d2, h_res;
  std::vector<int> h_bad, h_stat, h_nit;
  for (int c = 0; c < ch.nchunks; ++c) {
    const int kc = ch.tracks_of(c);
    const size_t k0 = (size_t)c * Kc, tk = T * kc;
    HIPCHK(hipMemset(d_x, 0, 3 * tk * sizeof(double)));   // (the first solve's step is measured against it and never used)
    HIPCHK(hipMemset(d_d2, 0, tk * sizeof(double)));
    if (int rc = ch.begin(c)) return rc;
    for (int l = 1; l < ch.levels; ++l) ch.lv[l].x = ch.aux[l];
    mcba::SmData td = ch.td;
    td.x = d_x; td.d2 = d_d2; td.dx = d_dx; td.loss = loss; td.f2 = f_scale * f_scale; td.inv_f2 = 1.0 / (f_scale * f_scale);
    h_stat.resize(kc); h_nit.assign(kc, 0); h_bad.resize(kc); h_res.resize((size_t)4 * kc);
    for (int k = 0; k < kc; ++k) h_stat[k] = ch.h_nus[k] < 2 ? mcba::SM_TOO_FEW_FRAMES : mcba::SM_OK;   // (too few: never launched)
    std::vector<int>& h_list = ch.h_list;
    for (int it = 0; it < max_iterations && !h_list.empty(); ++it) {
      const int nact = (int)h_list.size();
      if (int rc = call.put(ch.d_list, h_list.data(), (size_t)nact)) return rc;
      if (int rc = ch.open()) return rc;
      if (mcba::launch_smooth_solve(nullptr, ch.lv, ch.levels, td, kc, ch.d_list, nact, ch.d_bad, d_part, d_res) != 0) return fail(MCBA_ERR_ARG, "mcba_smooth_trajectories: bad launch");
      if (int rc = ch.close()) return rc;
      if (int rc = call.download(h_res.data(), d_res, (size_t)4 * nact)) return rc;
      if (int rc = call.download(h_bad.data(), ch.d_bad, (size_t)kc)) return rc;
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
    if (int rc = call.download(h_w.data(), ch.d_w, tk)) return rc;
    if (int rc = call.download(h_d2.data(), d_d2, tk)) return rc;
    for (int k = 0; k < kc; ++k) {
      const bool ok = h_stat[k] == mcba::SM_OK;
      status[k0 + k] = h_stat[k];
      n_usable[k0 + k] = ch.h_nus[k];
      n_iterations[k0 + k] = h_nit[k];
      ch.scatter(k, ok, h_x.data(), 3, out_points, nan);
      ch.scatter(k, ok, h_w.data(), 1, out_weights, 0.0);
      ch.scatter(k, ok, h_d2.data(), 1, out_d2, nan);
    }
  }
  ch.info(info8, kernel_ms, Kc, ch.nchunks, most_solves, (double)mcba::smooth_chunk_doubles(T, Kc, segment) * sizeof(double), 0.0);
  return MCBA_OK;
}

}  // extern "C"
