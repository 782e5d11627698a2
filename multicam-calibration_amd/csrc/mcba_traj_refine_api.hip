// mcba_traj_refine_api.hip -- the stateless trajectory-refinement calls of include/mcba.h (host arrays in, host arrays out, a device ordinal, no
// handle), in the idiom of mcba_smooth_api.hip: tracks run in chunks under the same device-memory budget (the shared part of SmoothChunks,
// mcba_smooth_host.h); the data planes of a chunk -- detections, sqrt(w) / pixel_std, the points --, its count and the opening of an iteration
// are TrackFit's (mcba_traj_host.h), shared with mcba_skeltraj_api.hip.  The Gauss-Newton loop is here: per iteration the kernels of
// mcba_traj_refine.hip and the smoother's elimination back to back and one small download (TR_SUMS doubles and a flag per running track).
// mcba_refine_trajectories_system is the first iteration of that loop laid open, before anything is accepted.
#include "mcba_traj_host.h"

using namespace mcba_internal;

namespace {

struct TrajIn {
  size_t T;
  int K, C;
  const double *uvs, *cam12, *dist5, *weights, *pixel_std, *start, *accel_std;
  int loss;
  double f_scale;
  int max_iterations;
  double xtol;
  int segment, device;
};
// system: one evaluation at the start (gradient, step, the costs); otherwise the loop (n_iterations, cost, history, cov6, lag9)
struct TrajOut {
  bool system;
  double *points, *information;
  int *status, *n_usable, *n_single, *n_iterations;
  double *cost, *history, *cov6, *lag9;
  double *gradient, *step, *data_cost, *penalty_cost, *trial_costs;
  double *info8, *kernel_ms;
};

int traj_check(const char* who, const TrajIn& in) {
  const DetectionChecks ck{who};
  if (in.T < 1 || in.T > ((size_t)1 << 31) || in.K < 1) return ck.bad("1 .. 2^31 frames and at least one track required");
  if (int rc = ck.cameras_arrays(in.C, mcba::kKpMaxCams, in.uvs && in.cam12 && in.pixel_std && in.start && in.accel_std)) return rc;
  if (int rc = ck.convex_loss(in.loss)) return rc;
  if (int rc = ck.loop(in.f_scale, in.max_iterations, in.xtol)) return rc;
  if (int rc = ck.pixel_std(in.pixel_std, in.C)) return rc;
  if (int rc = check_weights(who, in.weights, (size_t)in.C * in.T * in.K)) return rc;
  return smooth_check_common(who, "weights", in.T, in.K, in.accel_std, nullptr, in.segment);
}

int traj_run(const char* who, const TrajIn& in, const TrajOut& out) {
  const size_t T = in.T, K = (size_t)in.K;
  const int C = in.C, loss = in.loss, max_iterations = out.system ? 1 : in.max_iterations;
  const int segment = in.segment == 0 ? mcba::SM_SEGMENT_DEFAULT : in.segment;
  const bool cov = out.cov6 != nullptr, lag = out.lag9 != nullptr;
  const double nan = __builtin_nan("");
  if (out.history)
    for (size_t i = 0; i < (size_t)max_iterations * K * 3; ++i) out.history[i] = nan;
  int most = 0;
  double ms_cov = 0.0;

  SmoothChunks ch;
  StatelessCall& call = ch.call;
  if (int rc = ch.setup_shared(who, T, K, segment, in.accel_std, mcba::traj_refine_chunk_doubles(T, 1, C, segment, cov, lag), cov ? mcba::SM_ZC : 6)) return rc;
  const int Kc = ch.Kc, nblk = mcba::smooth_eval_blocks(T);
  const size_t TK = T * Kc;
  TrackFit fit{ch, "trajectory refinement", C, in.uvs, in.weights, in.pixel_std, in.start, in.f_scale};
  if (int rc = fit.setup(in.cam12, in.dist5)) return rc;
  double *d_part = nullptr, *d_res = nullptr, *d_oc = nullptr, *d_ol = nullptr;
  if (int rc = call.scratch(&d_part, (size_t)mcba::TR_SUMS * nblk * Kc)) return rc;
  if (int rc = call.scratch(&d_res, (size_t)mcba::TR_SUMS * Kc)) return rc;
  if (cov) if (int rc = call.scratch(&d_oc, 6 * TK)) return rc;
  if (lag) if (int rc = call.scratch(&d_ol, 9 * (T - 1) * Kc)) return rc;
  mcba::KpCam* const d_cams = fit.d_cams;
  double *const d_x = fit.d_x, *const d_d = fit.d_d, *const d_H = fit.d_H, *const d_G = fit.d_G;
  int* const d_run = fit.d_run;

  std::vector<double> h_x, h_H, h_G, h_d, h_res, h_alpha, h_cost, h_oc, h_ol;
  std::vector<int> h_bad, h_nit;
  std::vector<int>&h_stat = fit.h_stat, &h_run = fit.h_run, &h_nus = fit.h_nus, &h_nsg = fit.h_nsg;
  for (int c = 0; c < ch.nchunks; ++c) {
    if (int rc = ch.begin_shared(c)) return rc;
    if (int rc = fit.begin()) return rc;
    const int kc = ch.kc;
    const size_t k0 = ch.k0, tk = ch.tk;
    for (int l = 1; l < ch.levels; ++l) ch.lv[l].x = ch.aux[l];   // (with cov: the first six of the SM_ZC planes)
    const mcba::TrData& rd = fit.rd;
    // level 0 of the elimination: H as the diagonal blocks, -G as the right-hand side, d as the solution
    mcba::SmData td{T, nullptr, d_H, nullptr, ch.d_ia2, d_d, nullptr, nullptr, mcba::SM_LOSS_LINEAR, 1.0, 1.0, d_G};
    h_nit.assign(kc, 0); h_bad.assign(kc, 0); h_res.assign((size_t)mcba::TR_SUMS * kc, nan); h_alpha.assign(kc, 0.0); h_cost.assign(kc, nan);
    std::vector<int>& h_list = ch.h_list;
    std::vector<int> ran = h_list, sys_pos(kc, -1);
    bool pending = false;   // accepted steps not yet applied: the next bracket starts with them
    for (int it = 0; it < max_iterations && !h_list.empty(); ++it) {
      const int nact = (int)h_list.size();
      std::fill(h_run.begin(), h_run.end(), 0);
      for (int k : h_list) h_run[k] = 1;
      if (int rc = call.put(ch.d_list, h_list.data(), (size_t)nact)) return rc;
      if (int rc = call.put(d_run, h_run.data(), (size_t)kc)) return rc;
      if (int rc = fit.open_linearised(loss, pending, h_alpha)) return rc;
      int lrc = mcba::launch_smooth_reduce(nullptr, ch.lv, ch.levels, td, kc, ch.d_list, nact, ch.d_bad, true);
      lrc = lrc || mcba::launch_smooth_backsub(nullptr, ch.lv, ch.levels, td, kc, ch.d_list, nact, true);
      lrc = lrc || mcba::launch_traj_trial(nullptr, loss, rd, d_cams, C, kc, ch.d_list, nact, d_part, d_res);
      if (lrc) return fit.bad_launch();
      if (int rc = ch.close()) return rc;
      if (int rc = call.download(h_res.data(), d_res, (size_t)mcba::TR_SUMS * nact)) return rc;
      if (int rc = call.download(h_bad.data(), ch.d_bad, (size_t)kc)) return rc;
      most = std::max(most, it + 1);
      if (out.system) {
        for (int kk = 0; kk < nact; ++kk) sys_pos[h_list[kk]] = kk;
        break;
      }
      std::vector<int> next;
      std::fill(h_alpha.begin(), h_alpha.end(), 0.0);
      pending = false;
      for (int kk = 0; kk < nact; ++kk) {
        const int k = h_list[kk];
        const double* res = h_res.data() + (size_t)mcba::TR_SUMS * kk;
        h_nit[k] = it + 1;
        if (h_bad[k]) { h_stat[k] = mcba::TR_PIVOT; continue; }
        double alpha, cost;
        const bool stops = mcba::traj_decide(res, in.xtol, it, max_iterations, alpha, cost);
        double* h = out.history + ((size_t)it * K + k0 + k) * 3;
        h[0] = cost; h[1] = alpha * res[mcba::TR_DMAX]; h[2] = alpha;
        h_alpha[k] = alpha;
        h_cost[k] = cost;
        pending = pending || alpha != 0.0;
        if (!stops) next.push_back(k);
      }
      h_list.swap(next);
    }

    h_x.resize(3 * tk); h_H.resize(6 * tk);
    if (out.system) {
      h_G.resize(3 * tk); h_d.resize(3 * tk);
      if (int rc = call.download(h_G.data(), d_G, 3 * tk)) return rc;
      if (int rc = call.download(h_d.data(), d_d, 3 * tk)) return rc;
    } else {
      // the returned point: the last accepted steps, its linearisation and, on request, the band of the inverse of its Gauss-Newton matrix
      h_list.clear();
      std::fill(h_run.begin(), h_run.end(), 0);
      for (int k : ran)
        if (h_stat[k] == mcba::TR_OK) { h_list.push_back(k); h_run[k] = 1; }
      if (!h_list.empty()) {
        const int nact = (int)h_list.size();
        if (int rc = call.put(ch.d_list, h_list.data(), (size_t)nact)) return rc;
        if (int rc = call.put(d_run, h_run.data(), (size_t)kc)) return rc;
        if (int rc = fit.open_linearised(loss, pending, h_alpha, true)) return rc;
        if (int rc = ch.mark()) return rc;
        if (cov) {
          int lrc = mcba::launch_smooth_reduce(nullptr, ch.lv, ch.levels, td, kc, ch.d_list, nact, ch.d_bad, true);
          lrc = lrc || mcba::launch_smooth_selinv(nullptr, ch.lv, ch.levels, td, ch.aux, d_oc, d_ol, kc, ch.d_list, nact);
          if (lrc) return fit.bad_launch();
        }
        if (int rc = ch.close_split(ms_cov)) return rc;
        if (cov) {
          if (int rc = call.download(h_bad.data(), ch.d_bad, (size_t)kc)) return rc;
          for (int k : h_list)
            if (h_bad[k]) h_stat[k] = mcba::TR_PIVOT;
          h_oc.resize(6 * tk);
          if (int rc = call.download(h_oc.data(), d_oc, 6 * tk)) return rc;
          if (lag && T > 1) {
            h_ol.resize(9 * (T - 1) * kc);
            if (int rc = call.download(h_ol.data(), d_ol, 9 * (T - 1) * kc)) return rc;
          }
        }
      }
    }
    if (int rc = call.download(h_x.data(), d_x, 3 * tk)) return rc;
    if (int rc = call.download(h_H.data(), d_H, 6 * tk)) return rc;
    for (int k = 0; k < kc; ++k) {
      if (out.system && h_stat[k] == mcba::TR_OK && h_bad[k]) h_stat[k] = mcba::TR_PIVOT;
      const bool ok = h_stat[k] == mcba::TR_OK;
      out.status[k0 + k] = h_stat[k];
      out.n_usable[k0 + k] = h_nus[k];
      out.n_single[k0 + k] = h_nsg[k];
      ch.scatter(k, ok, h_H.data(), 6, out.information, nan);
      if (out.system) {
        const double* res = h_res.data() + (size_t)mcba::TR_SUMS * (sys_pos[k] < 0 ? 0 : sys_pos[k]);
        const bool have = ok && sys_pos[k] >= 0;
        ch.scatter(k, ok, h_G.data(), 3, out.gradient, nan);
        ch.scatter(k, ok, h_d.data(), 3, out.step, nan);
        out.data_cost[k0 + k] = have ? res[mcba::TR_DATA] : nan;
        out.penalty_cost[k0 + k] = have ? res[mcba::TR_PEN] : nan;
        for (int a = 0; a < mcba::TR_TRIALS; ++a) out.trial_costs[mcba::TR_TRIALS * (k0 + k) + a] = have ? res[1 + a] : nan;
      } else {
        ch.scatter(k, ok, h_x.data(), 3, out.points, nan);
        out.n_iterations[k0 + k] = h_nit[k];
        out.cost[k0 + k] = ok ? h_cost[k] : nan;
        if (cov) ch.scatter(k, ok, h_oc.data(), 6, out.cov6, nan);
        if (lag) ch.scatter(k, ok, h_ol.data(), 9, out.lag9, nan, T - 1);
      }
    }
  }
  ch.info(out.info8, out.kernel_ms, Kc, ch.nchunks, most, (double)mcba::traj_refine_chunk_doubles(T, Kc, C, segment, cov, lag) * sizeof(double), ms_cov);
  return MCBA_OK;
}

}  // namespace

extern "C" {

int mcba_refine_trajectories(size_t n_frames, int n_tracks, int n_cameras, const double* uvs, const double* cam12, const double* dist5, const double* weights, const double* pixel_std,
                             const double* start, const double* accel_std, int loss, double f_scale, int max_iterations, double xtol, int segment, int device, double* out_points,
                             double* information, int* status, int* n_usable, int* n_single, int* n_iterations, double* cost, double* history, double* out_cov6, double* out_lag9, double* info8,
                             double* kernel_ms) {
  const char* who = "mcba_refine_trajectories";
  const TrajIn in{n_frames, n_tracks, n_cameras, uvs, cam12, dist5, weights, pixel_std, start, accel_std, loss, f_scale, max_iterations, xtol, segment, device};
  if (int rc = traj_check(who, in)) return rc;
  if (!out_points || !information || !status || !n_usable || !n_single || !n_iterations || !cost || !history || !info8 || (out_lag9 && !out_cov6))
    return fail(MCBA_ERR_ARG, "mcba_refine_trajectories: non-NULL outputs (but out_cov6 and out_lag9, the second only with the first) required");
  if (int rc = stateless_device(device, who)) return rc;
  const TrajOut out{false, out_points, information, status, n_usable, n_single, n_iterations, cost, history, out_cov6, out_lag9, nullptr, nullptr, nullptr, nullptr, nullptr, info8, kernel_ms};
  return traj_run(who, in, out);
}

int mcba_refine_trajectories_system(size_t n_frames, int n_tracks, int n_cameras, const double* uvs, const double* cam12, const double* dist5, const double* weights, const double* pixel_std,
                                    const double* points, const double* accel_std, int loss, double f_scale, int segment, int device, double* information, double* gradient, double* step,
                                    int* status, int* n_usable, int* n_single, double* data_cost, double* penalty_cost, double* trial_costs, double* info8, double* kernel_ms) {
  const char* who = "mcba_refine_trajectories_system";
  const TrajIn in{n_frames, n_tracks, n_cameras, uvs, cam12, dist5, weights, pixel_std, points, accel_std, loss, f_scale, 1, 0.0, segment, device};
  if (int rc = traj_check(who, in)) return rc;
  if (!information || !gradient || !step || !status || !n_usable || !n_single || !data_cost || !penalty_cost || !trial_costs || !info8)
    return fail(MCBA_ERR_ARG, "mcba_refine_trajectories_system: non-NULL outputs required");
  if (int rc = stateless_device(device, who)) return rc;
  const TrajOut out{true, nullptr, information, status, n_usable, n_single, nullptr, nullptr, nullptr, nullptr, nullptr, gradient, step, data_cost, penalty_cost, trial_costs, info8, kernel_ms};
  return traj_run(who, in, out);
}

}  // extern "C"
