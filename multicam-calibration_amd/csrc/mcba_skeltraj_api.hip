// mcba_skeltraj_api.hip -- the stateless skeleton-trajectory calls of include/mcba.h (host arrays in, host arrays out, a device ordinal, no handle),
// in the idiom of mcba_traj_refine_api.hip: the reprojection planes, the count and the opening of an iteration are TrackFit's
// (mcba_traj_host.h), shared with it.  Bones couple the tracks, so the call is one chunk: it must fit the smoother's device-memory budget
// (MCBA_SMOOTH_BUDGET_MB) whole and is refused otherwise, before anything is allocated.  The Gauss-Newton loop is here: per outer iteration the
// two linearisations, one elimination, the conjugate-gradient iterations (launch_skt_cg_iteration; the done word is read every
// SKT_HOST_READS_EVERY of them, nothing else synchronises inside a solve) and the trial with one small download.
// mcba_refine_skeleton_trajectories_system is the first iteration of that loop laid open, before anything is accepted.
#include "mcba_traj_host.h"
#include "mcba_skeltraj_math.h"

using namespace mcba_internal;

namespace {

struct SktIn {
  size_t T;
  int K, C;
  const double *uvs, *cam12, *dist5, *weights, *pixel_std, *start, *accel_std;
  const int* parent;
  const double *bone_length, *bone_std;
  int loss;
  double f_scale;
  int max_iterations;
  double xtol, cg_tol;
  int cg_max, segment, device;
};
// system: one evaluation at the start; otherwise the loop
struct SktOut {
  bool system;
  double *points, *information;
  int *status, *n_usable, *n_single, *converged, *n_iterations;
  double *cost, *cost_start, *history, *bone_residual, *direction;
  double *gradient, *step;
  int* cg_iterations;
  double *cg_residual, *data_cost, *penalty_cost, *bone_cost, *trial_costs;
  double* resolve_check;   // system, or null: (2, T, K, 3) -- M z = -G by the elimination, and again by the re-solve from its stored factors
  double *info8, *kernel_ms;
};

int skt_check(const char* who, const SktIn& in) {
  const DetectionChecks ck{who};
  if (int rc = ck.frames_keypoints(in.T, in.K, mcba::SK_MAX_K)) return rc;
  if (int rc = ck.cameras_arrays(in.C, mcba::kKpMaxCams, in.uvs && in.cam12 && in.pixel_std && in.start && in.accel_std && in.parent && in.bone_length && in.bone_std)) return rc;
  if (int rc = ck.convex_loss(in.loss)) return rc;
  if (int rc = ck.loop(in.f_scale, in.max_iterations, in.xtol)) return rc;
  if (!(in.cg_tol > 0.0 && in.cg_tol < 1.0)) return ck.bad("cg_tol must lie inside (0, 1)");
  if (in.cg_max < 1) return ck.bad("cg_max >= 1");
  if (int rc = ck.pixel_std(in.pixel_std, in.C)) return rc;
  mcba::SkPlan plan;
  if (int rc = ck.forest(mcba::skel_plan(in.K, in.parent, in.bone_length, in.bone_std, plan))) return rc;
  if (int rc = check_weights(who, in.weights, (size_t)in.C * in.T * in.K)) return rc;
  if (int rc = smooth_check_common(who, "weights", in.T, in.K, in.accel_std, nullptr, in.segment)) return rc;
  const int segment = in.segment == 0 ? mcba::SM_SEGMENT_DEFAULT : in.segment;
  if ((double)mcba::skeltraj_chunk_doubles(in.T, in.K, in.C, segment) * sizeof(double) > smooth_budget_bytes())
    return ck.bad("the call does not fit the device-memory budget MCBA_SMOOTH_BUDGET_MB (bones couple the tracks: it cannot run in chunks)");
  return MCBA_OK;
}

int skt_run(const char* who, const SktIn& in, const SktOut& out) {
  const size_t T = in.T, K = (size_t)in.K, TK = T * K;
  const int C = in.C, Ki = in.K, loss = in.loss, max_iterations = out.system ? 1 : in.max_iterations;
  const int segment = in.segment == 0 ? mcba::SM_SEGMENT_DEFAULT : in.segment;
  const double nan = __builtin_nan(""), tol2 = in.cg_tol * in.cg_tol;
  const size_t total = mcba::skeltraj_chunk_doubles(T, Ki, C, segment);
  if (out.history)
    for (size_t i = 0; i < (size_t)max_iterations * 4; ++i) out.history[i] = nan;

  SmoothChunks ch;
  StatelessCall& call = ch.call;
  if (int rc = ch.setup_shared(who, T, K, segment, in.accel_std, total / K, 6)) return rc;
  if (ch.nchunks != 1) return fail(MCBA_ERR_ARG, "skeleton trajectories: the call must be one chunk");
  const unsigned nblk = (unsigned)((TK + 255) / 256);
  TrackFit fit{ch, "skeleton trajectories", C, in.uvs, in.weights, in.pixel_std, in.start, in.f_scale};
  if (int rc = fit.setup(in.cam12, in.dist5)) return rc;
  double *d_q = nullptr, *d_p = nullptr, *d_y = nullptr, *d_z = nullptr, *d_dir = nullptr, *d_bres = nullptr, *d_part = nullptr, *d_res = nullptr, *d_sc = nullptr;
  int* d_w = nullptr;
  mcba::SkPlan* d_plan = nullptr;
  if (int rc = call.scratch(&d_plan, 1)) return rc;
  for (double** p3 : {&d_q, &d_p, &d_y, &d_z, &d_dir})
    if (int rc = call.scratch(p3, 3 * TK)) return rc;
  if (int rc = call.scratch(&d_bres, TK)) return rc;
  if (int rc = call.scratch(&d_part, (size_t)mcba::SKT_SUMS * nblk)) return rc;
  if (int rc = call.scratch(&d_res, (size_t)mcba::SKT_SUMS)) return rc;
  if (int rc = call.scratch(&d_sc, (size_t)mcba::CG_DOUBLES)) return rc;
  if (int rc = call.scratch(&d_w, (size_t)mcba::CG_INTS)) return rc;
  mcba::KpCam* const d_cams = fit.d_cams;
  double *const d_x = fit.d_x, *const d_d = fit.d_d, *const d_H = fit.d_H, *const d_G = fit.d_G;
  int* const d_run = fit.d_run;

  if (int rc = ch.begin_shared(0)) return rc;
  if (int rc = fit.begin()) return rc;
  for (int l = 1; l < ch.levels; ++l) ch.lv[l].x = ch.aux[l];
  const mcba::TrData& rd = fit.rd;
  const mcba::SktData sd{rd, d_q, d_p, d_y, d_z, d_dir, d_bres, d_plan, d_run};
  // level 0 of the elimination and of every re-solve: H as the diagonal blocks, -q as the right-hand side (q = G at the elimination), z as the solution
  const mcba::SmData td{T, nullptr, d_H, nullptr, ch.d_ia2, d_z, nullptr, nullptr, mcba::SM_LOSS_LINEAR, 1.0, 1.0, d_q};

  std::vector<int>&h_nus = fit.h_nus, &h_nsg = fit.h_nsg, &h_stat = fit.h_stat, &h_run = fit.h_run, &h_list = ch.h_list;
  std::vector<int> h_bad(K, 0), h_par(K, -1);
  // the active forest: a bone stays when both its tracks run
  for (int k = 0; k < Ki; ++k) h_par[k] = h_run[k] && in.parent[k] >= 0 && h_run[in.parent[k]] ? in.parent[k] : -1;
  mcba::SkPlan plan;
  if (mcba::skel_plan(Ki, h_par.data(), in.bone_length, in.bone_std, plan) != 0) return fail(MCBA_ERR_ARG, "skeleton trajectories: bad plan");
  if (int rc = call.put(d_plan, &plan, 1)) return rc;
  if (int rc = call.put(d_run, h_run.data(), K)) return rc;
  const int nact = (int)h_list.size();
  if (nact) if (int rc = call.put(ch.d_list, h_list.data(), (size_t)nact)) return rc;

  std::vector<double> h_alpha(K, 0.0);
  double res[mcba::SKT_SUMS], sc[mcba::CG_DOUBLES];
  int w[mcba::CG_INTS] = {0, 0};
  for (int e = 0; e < mcba::SKT_SUMS; ++e) res[e] = nan;
  for (int e = 0; e < mcba::CG_DOUBLES; ++e) sc[e] = nan;
  bool pending = false, stopped = nact == 0, converged = false, have = false;
  int n_it = 0, cg_total = 0;
  double cost = nan, cost_start = nan;
  for (int it = 0; it < max_iterations && !stopped; ++it) {
    if (int rc = fit.open_linearised(loss, pending, h_alpha)) return rc;
    int lrc = mcba::launch_skt_linearise(nullptr, sd, Ki);
    lrc = lrc || mcba::launch_smooth_reduce(nullptr, ch.lv, ch.levels, td, Ki, ch.d_list, nact, ch.d_bad, true);
    lrc = lrc || mcba::launch_smooth_backsub(nullptr, ch.lv, ch.levels, td, Ki, ch.d_list, nact, true);
    if (lrc) return fit.bad_launch();
    if (out.system && out.resolve_check) {
      // the re-solve held against the elimination on the same right-hand side: z is kept, the right-hand-side halves of every stored record,
      // every level's solution and z are overwritten with NaN (all bits set), and the re-solve with the same back-substitution makes z again
      if (int rc = ch.close()) return rc;
      if (int rc = call.download(out.resolve_check, d_z, 3 * TK)) return rc;
      for (int l = 0; l < ch.levels; ++l) {
        const size_t NS = ch.lv[l].NS, six = 6 * NS * sizeof(double);
        HIPCHK(hipMemset(ch.lv[l].fac + 57 * NS, 0xff, six));
        if (l) {
          HIPCHK(hipMemset(ch.lv[l].sep + 21 * NS, 0xff, six));
          HIPCHK(hipMemset(ch.lv[l].sep + 48 * NS, 0xff, six));
          HIPCHK(hipMemset(ch.lv[l].x, 0xff, six));
        }
      }
      HIPCHK(hipMemset(d_z, 0xff, 3 * TK * sizeof(double)));
      if (int rc = ch.open()) return rc;
      if (mcba::launch_smooth_resolve(nullptr, ch.lv, ch.levels, td, Ki, ch.d_list, nact, nullptr) || mcba::launch_smooth_backsub(nullptr, ch.lv, ch.levels, td, Ki, ch.d_list, nact, true))
        return fit.bad_launch();
      if (int rc = ch.close()) return rc;
      if (int rc = call.download(out.resolve_check + 3 * TK, d_z, 3 * TK)) return rc;
      if (int rc = ch.open()) return rc;
    }
    if (mcba::launch_skt_cg_start(nullptr, sd, Ki, d_part, d_sc, d_w)) return fit.bad_launch();
    for (int launched = 0;;) {
      for (int i = 0; i < mcba::SKT_HOST_READS_EVERY && launched < in.cg_max; ++i, ++launched)
        if (mcba::launch_skt_cg_iteration(nullptr, sd, Ki, ch.lv, ch.levels, td, ch.d_list, nact, tol2, in.cg_max, d_part, d_sc, d_w)) return fit.bad_launch();
      if (int rc = ch.close()) return rc;
      if (int rc = call.download(w, d_w, (size_t)mcba::CG_INTS)) return rc;
      if (int rc = ch.open()) return rc;
      if (w[mcba::CG_DONE] || launched >= in.cg_max) break;
    }
    if (mcba::launch_skt_trial(nullptr, loss, sd, d_cams, C, Ki, d_part, d_res)) return fit.bad_launch();
    if (int rc = ch.close()) return rc;
    if (int rc = call.download(res, d_res, (size_t)mcba::SKT_SUMS)) return rc;
    if (int rc = call.download(sc, d_sc, (size_t)mcba::CG_DOUBLES)) return rc;
    if (int rc = call.download(h_bad.data(), ch.d_bad, K)) return rc;
    pending = false;
    have = true;
    bool pivot = false;
    for (int k : h_list)
      if (h_bad[k]) { h_stat[k] = mcba::TR_PIVOT; pivot = true; }
    if (it == 0) {
      cost_start = cost = res[0];
      if (!pivot && !mcba::sm_finite(res[0]))   // (a bone of zero length, or an overflow: no start to descend from)
        for (int k : h_list) h_stat[k] = mcba::TR_BAD_START;
    }
    if (out.system) { n_it = 1; cg_total = w[mcba::CG_ITERATIONS]; }
    // (an iteration that ends on a refused pivot or a non-finite objective accepts nothing and is not counted: no history row, no share of the CG total)
    if (pivot || !mcba::sm_finite(res[0]) || out.system) break;
    n_it = it + 1;
    cg_total += w[mcba::CG_ITERATIONS];
    double alpha;
    stopped = mcba::traj_decide(res, in.xtol, it, max_iterations, alpha, cost);
    converged = mcba::skt_converged(res, in.xtol, alpha);
    double* h = out.history + (size_t)it * 4;
    h[0] = cost; h[1] = alpha * res[mcba::TR_DMAX]; h[2] = alpha; h[3] = w[mcba::CG_ITERATIONS];
    for (int k : h_list) h_alpha[k] = alpha;
    pending = alpha != 0.0;
  }

  bool any_ok = false;
  for (int k = 0; k < Ki; ++k) any_ok = any_ok || h_stat[k] == mcba::TR_OK;
  std::vector<double> h_x(3 * TK), h_H(6 * TK), h_dir(3 * TK), h_bres(TK), h_G, h_d;
  if (any_ok && !out.system) {
    // the returned point: the last accepted step, and its linearisation
    if (int rc = fit.open_linearised(loss, pending, h_alpha)) return rc;
    if (mcba::launch_skt_linearise(nullptr, sd, Ki)) return fit.bad_launch();
    if (int rc = ch.close()) return rc;
  }
  if (any_ok) {
    if (int rc = call.download(h_x.data(), d_x, 3 * TK)) return rc;
    if (int rc = call.download(h_H.data(), d_H, 6 * TK)) return rc;
    if (int rc = call.download(h_dir.data(), d_dir, 3 * TK)) return rc;
    if (int rc = call.download(h_bres.data(), d_bres, TK)) return rc;
    if (out.system) {
      h_G.resize(3 * TK); h_d.resize(3 * TK);
      if (int rc = call.download(h_G.data(), d_G, 3 * TK)) return rc;
      if (int rc = call.download(h_d.data(), d_d, 3 * TK)) return rc;
    }
  }
  for (int k = 0; k < Ki; ++k) {
    const bool ok = h_stat[k] == mcba::TR_OK, bone = ok && h_par[k] >= 0 && h_stat[h_par[k]] == mcba::TR_OK;
    out.status[k] = h_stat[k];
    out.n_usable[k] = h_nus[k];
    out.n_single[k] = h_nsg[k];
    ch.scatter(k, ok, h_H.data(), 6, out.information, nan);
    ch.scatter(k, bone, h_dir.data(), 3, out.direction, nan);
    if (out.system) {
      ch.scatter(k, ok, h_G.data(), 3, out.gradient, nan);
      ch.scatter(k, ok, h_d.data(), 3, out.step, nan);
    } else {
      ch.scatter(k, ok, h_x.data(), 3, out.points, nan);
      ch.scatter(k, bone, h_bres.data(), 1, out.bone_residual, nan);
    }
  }
  if (out.system) {
    const bool ok = any_ok && have;
    *out.cg_iterations = ok ? w[mcba::CG_ITERATIONS] : 0;
    *out.cg_residual = ok ? (sc[mcba::CG_RZ0] > 0.0 ? sqrt(fmax(sc[mcba::CG_RZ], 0.0) / sc[mcba::CG_RZ0]) : 0.0) : nan;
    *out.data_cost = ok ? res[mcba::TR_DATA] : nan;
    *out.penalty_cost = ok ? res[mcba::TR_PEN] : nan;
    *out.bone_cost = ok ? res[mcba::SKT_BONE] : nan;
    for (int a = 0; a < mcba::TR_TRIALS; ++a) out.trial_costs[a] = ok ? res[1 + a] : nan;
  } else {
    *out.converged = any_ok && converged ? 1 : 0;
    *out.n_iterations = n_it;
    *out.cost = any_ok ? cost : nan;
    *out.cost_start = any_ok ? cost_start : nan;
  }
  ch.info(out.info8, out.kernel_ms, nact, cg_total, n_it, (double)total * sizeof(double), 0.0);
  return MCBA_OK;
}

}  // namespace

extern "C" {

int mcba_refine_skeleton_trajectories(size_t n_frames, int n_keypoints, int n_cameras, const double* uvs, const double* cam12, const double* dist5, const double* weights,
                                      const double* pixel_std, const double* start, const double* accel_std, const int* parent, const double* bone_length, const double* bone_std, int loss,
                                      double f_scale, int max_iterations, double xtol, double cg_tol, int cg_max, int segment, int device, double* out_points, double* information, int* status,
                                      int* n_usable, int* n_single, int* converged, int* n_iterations, double* cost, double* cost_start, double* history, double* bone_residual,
                                      double* direction, double* info8, double* kernel_ms) {
  const char* who = "mcba_refine_skeleton_trajectories";
  const SktIn in{n_frames, n_keypoints, n_cameras, uvs, cam12, dist5, weights, pixel_std, start, accel_std, parent, bone_length, bone_std, loss, f_scale, max_iterations, xtol, cg_tol, cg_max,
                 segment, device};
  if (int rc = skt_check(who, in)) return rc;
  if (!out_points || !information || !status || !n_usable || !n_single || !converged || !n_iterations || !cost || !cost_start || !history || !bone_residual || !direction || !info8)
    return fail(MCBA_ERR_ARG, "mcba_refine_skeleton_trajectories: non-NULL outputs required");
  if (int rc = stateless_device(device, who)) return rc;
  const SktOut out{false, out_points, information, status, n_usable, n_single, converged, n_iterations, cost, cost_start, history, bone_residual, direction, nullptr, nullptr, nullptr, nullptr,
                   nullptr, nullptr, nullptr, nullptr, nullptr, info8, kernel_ms};
  return skt_run(who, in, out);
}

int mcba_refine_skeleton_trajectories_system(size_t n_frames, int n_keypoints, int n_cameras, const double* uvs, const double* cam12, const double* dist5, const double* weights,
                                             const double* pixel_std, const double* points, const double* accel_std, const int* parent, const double* bone_length, const double* bone_std,
                                             int loss, double f_scale, double cg_tol, int cg_max, int segment, int device, double* information, double* gradient, double* direction,
                                             double* step, int* status, int* n_usable, int* n_single, int* cg_iterations, double* cg_residual, double* data_cost, double* penalty_cost,
                                             double* bone_cost, double* trial_costs, double* resolve_check, double* info8, double* kernel_ms) {
  const char* who = "mcba_refine_skeleton_trajectories_system";
  const SktIn in{n_frames, n_keypoints, n_cameras, uvs, cam12, dist5, weights, pixel_std, points, accel_std, parent, bone_length, bone_std, loss, f_scale, 1, 0.0, cg_tol, cg_max, segment, device};
  if (int rc = skt_check(who, in)) return rc;
  if (!information || !gradient || !direction || !step || !status || !n_usable || !n_single || !cg_iterations || !cg_residual || !data_cost || !penalty_cost || !bone_cost || !trial_costs || !info8)
    return fail(MCBA_ERR_ARG, "mcba_refine_skeleton_trajectories_system: non-NULL outputs required");
  if (int rc = stateless_device(device, who)) return rc;
  const SktOut out{true, nullptr, information, status, n_usable, n_single, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, direction, gradient, step, cg_iterations, cg_residual, data_cost,
                   penalty_cost, bone_cost, trial_costs, resolve_check, info8, kernel_ms};
  return skt_run(who, in, out);
}

}  // extern "C"
