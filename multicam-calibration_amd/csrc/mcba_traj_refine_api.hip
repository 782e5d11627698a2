// mcba_traj_refine_api.hip -- the stateless trajectory-refinement calls of include/mcba.h (host arrays in, host arrays out, a device ordinal, no
// handle), in the idiom of mcba_smooth_api.hip: tracks run in chunks under the same device-memory budget (the shared part of SmoothChunks,
// mcba_smooth_host.h); the data planes of a chunk -- detections, sqrt(w) / pixel_std, the points -- are this file's own.  The Gauss-Newton loop is
// here: per iteration the kernels of mcba_traj_refine.hip and the smoother's elimination back to back and one small download (TR_SUMS doubles and a
// flag per running track).  mcba_refine_trajectories_system is the first iteration of that loop laid open, before anything is accepted.
#include "mcba_smooth_host.h"
#include "mcba_traj_refine_math.h"

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
  auto bad = [&](const char* what) { g_err = std::string(who) + ": " + what; return MCBA_ERR_ARG; };
  if (in.T < 1 || in.T > ((size_t)1 << 31) || in.K < 1) return bad("1 .. 2^31 frames and at least one track required");
  if (in.C < 1 || in.C > mcba::kKpMaxCams) return bad("1 .. 64 cameras required");
  if (!in.uvs || !in.cam12 || !in.pixel_std || !in.start || !in.accel_std) return bad("non-NULL arrays (but dist5 and weights) required");
  if (in.loss < mcba::SM_LOSS_LINEAR || in.loss > mcba::SM_LOSS_HUBER) return bad("loss must be linear, soft_l1 or huber (0 .. 2)");
  if (!(in.f_scale > 0.0) || !mcba::sm_finite(in.f_scale)) return bad("f_scale must be positive and finite");
  if (in.max_iterations < 1) return bad("max_iterations >= 1");
  if (!(in.xtol >= 0.0)) return bad("xtol >= 0");
  for (int c = 0; c < in.C; ++c)
    if (!(in.pixel_std[c] > 0.0) || !mcba::sm_finite(in.pixel_std[c]) || !mcba::sm_finite(1.0 / in.pixel_std[c])) return bad("pixel_std must be positive and finite (and its inverse too)");
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
  double *d_det = nullptr, *d_sw = nullptr, *d_x = nullptr, *d_d = nullptr, *d_H = nullptr, *d_G = nullptr, *d_part = nullptr, *d_res = nullptr, *d_alpha = nullptr, *d_oc = nullptr, *d_ol = nullptr;
  int *d_nsg = nullptr, *d_nbs = nullptr, *d_run = nullptr;
  mcba::KpCam* d_cams = nullptr;
  std::vector<mcba::KpCam> tab((size_t)C);
  for (int c = 0; c < C; ++c) mcba::make_kp_cam(in.cam12 + 12 * c, in.dist5 ? in.dist5 + 5 * c : nullptr, tab[c]);
  if (int rc = call.upload(&d_cams, tab.data(), tab.size())) return rc;
  if (int rc = call.scratch(&d_det, 2 * C * TK)) return rc;
  if (int rc = call.scratch(&d_sw, C * TK)) return rc;
  if (int rc = call.scratch(&d_x, 3 * TK)) return rc;
  if (int rc = call.scratch(&d_d, 3 * TK)) return rc;
  if (int rc = call.scratch(&d_H, 6 * TK)) return rc;
  if (int rc = call.scratch(&d_G, 3 * TK)) return rc;
  if (int rc = call.scratch(&d_part, (size_t)mcba::TR_SUMS * nblk * Kc)) return rc;
  if (int rc = call.scratch(&d_res, (size_t)mcba::TR_SUMS * Kc)) return rc;
  if (int rc = call.scratch(&d_alpha, (size_t)Kc)) return rc;
  if (int rc = call.scratch(&d_nsg, (size_t)Kc)) return rc;
  if (int rc = call.scratch(&d_nbs, (size_t)Kc)) return rc;
  if (int rc = call.scratch(&d_run, (size_t)Kc)) return rc;
  if (cov) if (int rc = call.scratch(&d_oc, 6 * TK)) return rc;
  if (lag) if (int rc = call.scratch(&d_ol, 9 * (T - 1) * Kc)) return rc;
  HIPCHK(hipEventCreate(&ch.e2));

  std::vector<double> h_det, h_sw, h_x, h_H, h_G, h_d, h_res, h_alpha, h_cost, h_oc, h_ol;
  std::vector<int> h_nus, h_nsg, h_nbs, h_bad, h_stat, h_nit, h_run;
  for (int c = 0; c < ch.nchunks; ++c) {
    if (int rc = ch.begin_shared(c)) return rc;
    const int kc = ch.kc;
    const size_t k0 = ch.k0, tk = ch.tk;
    // gather the chunk's planes: detections (C, T kc) pairs, sqrt(w) / pixel_std beside them, the start
    h_sw.resize(C * tk);
    const double *s_det = in.uvs, *s_x = in.start;
    if (kc != (int)K) {
      h_det.resize(2 * C * tk); h_x.resize(3 * tk);
      for (int cc = 0; cc < C; ++cc)
        for (size_t t = 0; t < T; ++t) memcpy(h_det.data() + 2 * (cc * tk + t * kc), in.uvs + 2 * ((cc * T + t) * K + k0), 2 * kc * sizeof(double));
      for (size_t t = 0; t < T; ++t) memcpy(h_x.data() + 3 * t * kc, in.start + 3 * (t * K + k0), 3 * kc * sizeof(double));
      s_det = h_det.data(); s_x = h_x.data();
    }
    for (int cc = 0; cc < C; ++cc) {
      const double ips = 1.0 / in.pixel_std[cc];
      for (size_t t = 0; t < T; ++t)
        for (int k = 0; k < kc; ++k) {
          const double w = in.weights ? in.weights[(cc * T + t) * K + k0 + k] : 1.0;
          h_sw[cc * tk + t * kc + k] = w > 0.0 ? sqrt(w) * ips : 0.0;   // (a zero or NaN weight: unseen)
        }
    }
    if (int rc = call.put(d_det, s_det, 2 * C * tk)) return rc;
    if (int rc = call.put(d_sw, h_sw.data(), C * tk)) return rc;
    if (int rc = call.put(d_x, s_x, 3 * tk)) return rc;
    for (int l = 1; l < ch.levels; ++l) ch.lv[l].x = ch.aux[l];   // (with cov: the first six of the SM_ZC planes)
    const mcba::TrData rd{T, d_det, d_sw, d_x, d_d, d_H, d_G, ch.d_ia2, in.f_scale * in.f_scale, 1.0 / (in.f_scale * in.f_scale)};
    // level 0 of the elimination: H as the diagonal blocks, -G as the right-hand side, d as the solution
    mcba::SmData td{T, nullptr, d_H, nullptr, ch.d_ia2, d_d, nullptr, nullptr, mcba::SM_LOSS_LINEAR, 1.0, 1.0, d_G};

    HIPCHK(hipEventRecord(call.e0, nullptr));
    if (mcba::launch_traj_count(nullptr, rd, C, kc, ch.d_nus, d_nsg, d_nbs) != 0) return fail(MCBA_ERR_ARG, "trajectory refinement: bad launch");
    if (int rc = check_launch()) return rc;
    HIPCHK(hipEventRecord(call.e1, nullptr));
    HIPCHK(hipEventSynchronize(call.e1));
    if (int rc = ch.add_ms(call.e0, call.e1, ch.ms_total)) return rc;
    h_nus.resize(kc); h_nsg.resize(kc); h_nbs.resize(kc);
    if (int rc = call.download(h_nus.data(), ch.d_nus, (size_t)kc)) return rc;
    if (int rc = call.download(h_nsg.data(), d_nsg, (size_t)kc)) return rc;
    if (int rc = call.download(h_nbs.data(), d_nbs, (size_t)kc)) return rc;
    h_stat.resize(kc); h_nit.assign(kc, 0); h_bad.assign(kc, 0); h_res.assign((size_t)mcba::TR_SUMS * kc, nan); h_alpha.assign(kc, 0.0); h_cost.assign(kc, nan); h_run.assign(kc, 0);
    std::vector<int>& h_list = ch.h_list;
    h_list.clear();
    for (int k = 0; k < kc; ++k) {
      h_stat[k] = h_nus[k] < 2 ? mcba::TR_TOO_FEW_FRAMES : h_nbs[k] ? mcba::TR_BAD_START : mcba::TR_OK;   // (neither is ever launched)
      if (h_stat[k] == mcba::TR_OK) h_list.push_back(k);
    }
    std::vector<int> ran = h_list, sys_pos(kc, -1);
    bool pending = false;   // accepted steps not yet applied: the next bracket starts with them
    for (int it = 0; it < max_iterations && !h_list.empty(); ++it) {
      const int nact = (int)h_list.size();
      std::fill(h_run.begin(), h_run.end(), 0);
      for (int k : h_list) h_run[k] = 1;
      if (int rc = call.put(ch.d_list, h_list.data(), (size_t)nact)) return rc;
      if (int rc = call.put(d_run, h_run.data(), (size_t)kc)) return rc;
      if (pending) if (int rc = call.put(d_alpha, h_alpha.data(), (size_t)kc)) return rc;
      HIPCHK(hipEventRecord(call.e0, nullptr));
      int lrc = pending ? mcba::launch_traj_apply(nullptr, rd, kc, d_alpha) : 0;
      lrc = lrc || mcba::launch_traj_linearise(nullptr, loss, rd, d_cams, C, kc, d_run);
      lrc = lrc || mcba::launch_smooth_reduce(nullptr, ch.lv, ch.levels, td, kc, ch.d_list, nact, ch.d_bad, true);
      lrc = lrc || mcba::launch_smooth_backsub(nullptr, ch.lv, ch.levels, td, kc, ch.d_list, nact, true);
      lrc = lrc || mcba::launch_traj_trial(nullptr, loss, rd, d_cams, C, kc, ch.d_list, nact, d_part, d_res);
      if (lrc) return fail(MCBA_ERR_ARG, "trajectory refinement: bad launch");
      if (int rc = check_launch()) return rc;
      HIPCHK(hipEventRecord(call.e1, nullptr));
      HIPCHK(hipEventSynchronize(call.e1));
      if (int rc = ch.add_ms(call.e0, call.e1, ch.ms_total)) return rc;
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
        if (pending) if (int rc = call.put(d_alpha, h_alpha.data(), (size_t)kc)) return rc;
        HIPCHK(hipEventRecord(call.e0, nullptr));
        int lrc = pending ? mcba::launch_traj_apply(nullptr, rd, kc, d_alpha) : 0;
        lrc = lrc || mcba::launch_traj_linearise(nullptr, loss, rd, d_cams, C, kc, d_run);
        HIPCHK(hipEventRecord(call.e1, nullptr));
        if (cov) {
          lrc = lrc || mcba::launch_smooth_reduce(nullptr, ch.lv, ch.levels, td, kc, ch.d_list, nact, ch.d_bad, true);
          lrc = lrc || mcba::launch_smooth_selinv(nullptr, ch.lv, ch.levels, td, ch.aux, d_oc, d_ol, kc, ch.d_list, nact);
        }
        if (lrc) return fail(MCBA_ERR_ARG, "trajectory refinement: bad launch");
        if (int rc = check_launch()) return rc;
        HIPCHK(hipEventRecord(ch.e2, nullptr));
        HIPCHK(hipEventSynchronize(ch.e2));
        if (int rc = ch.add_ms(call.e0, ch.e2, ch.ms_total)) return rc;
        if (int rc = ch.add_ms(call.e1, ch.e2, ms_cov)) return rc;
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
  double* info8 = out.info8;
  info8[0] = ch.levels; info8[1] = segment; info8[2] = Kc; info8[3] = ch.nchunks; info8[4] = ch.ms_total; info8[5] = most;
  info8[6] = (double)mcba::traj_refine_chunk_doubles(T, Kc, C, segment, cov, lag) * sizeof(double); info8[7] = ms_cov;
  if (out.kernel_ms) *out.kernel_ms = ch.ms_total;
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
