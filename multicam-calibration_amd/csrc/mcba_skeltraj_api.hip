// mcba_skeltraj_api.hip -- the stateless skeleton-trajectory calls of include/mcba.h (host arrays in, host arrays out, a device ordinal, no handle),
// in the idiom of mcba_traj_refine_api.hip.  Bones couple the tracks, so the call is one chunk: it must fit the smoother's device-memory budget
// (MCBA_SMOOTH_BUDGET_MB) whole and is refused otherwise, before anything is allocated.  The Gauss-Newton loop is here: per outer iteration the
// two linearisations, one elimination, the conjugate-gradient iterations (launch_skt_cg_iteration; the done word is read every
// SKT_HOST_READS_EVERY of them, nothing else synchronises inside a solve) and the trial with one small download.
// mcba_refine_skeleton_trajectories_system is the first iteration of that loop laid open, before anything is accepted.
#include "mcba_smooth_host.h"
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
  auto bad = [&](const char* what) { g_err = std::string(who) + ": " + what; return MCBA_ERR_ARG; };
  if (in.T < 1 || in.T > ((size_t)1 << 31)) return bad("1 .. 2^31 frames required");
  if (in.K < 1 || in.K > mcba::SK_MAX_K) return bad("1 .. 64 keypoints required");
  if (in.C < 1 || in.C > mcba::kKpMaxCams) return bad("1 .. 64 cameras required");
  if (!in.uvs || !in.cam12 || !in.pixel_std || !in.start || !in.accel_std || !in.parent || !in.bone_length || !in.bone_std) return bad("non-NULL arrays (but dist5 and weights) required");
  if (in.loss < mcba::SM_LOSS_LINEAR || in.loss > mcba::SM_LOSS_HUBER) return bad("loss must be linear, soft_l1 or huber (0 .. 2)");
  if (!(in.f_scale > 0.0) || !mcba::sm_finite(in.f_scale)) return bad("f_scale must be positive and finite");
  if (in.max_iterations < 1) return bad("max_iterations >= 1");
  if (!(in.xtol >= 0.0)) return bad("xtol >= 0");
  if (!(in.cg_tol > 0.0 && in.cg_tol < 1.0)) return bad("cg_tol must lie inside (0, 1)");
  if (in.cg_max < 1) return bad("cg_max >= 1");
  for (int c = 0; c < in.C; ++c)
    if (!(in.pixel_std[c] > 0.0) || !mcba::sm_finite(in.pixel_std[c]) || !mcba::sm_finite(1.0 / in.pixel_std[c])) return bad("pixel_std must be positive and finite (and its inverse too)");
  mcba::SkPlan plan;
  switch (mcba::skel_plan(in.K, in.parent, in.bone_length, in.bone_std, plan)) {
    case 0: break;
    case 2: return bad("a parent outside -1 .. K - 1, or a keypoint that is its own parent");
    case 3: return bad("the parents form a cycle: the skeleton must be a forest");
    default: return bad("bone_length and bone_std must be positive and finite for every keypoint with a parent");
  }
  if (int rc = check_weights(who, in.weights, (size_t)in.C * in.T * in.K)) return rc;
  if (int rc = smooth_check_common(who, "weights", in.T, in.K, in.accel_std, nullptr, in.segment)) return rc;
  const int segment = in.segment == 0 ? mcba::SM_SEGMENT_DEFAULT : in.segment;
  if ((double)mcba::skeltraj_chunk_doubles(in.T, in.K, in.C, segment) * sizeof(double) > smooth_budget_bytes())
    return bad("the call does not fit the device-memory budget MCBA_SMOOTH_BUDGET_MB (bones couple the tracks: it cannot run in chunks)");
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
  double *d_det = nullptr, *d_sw = nullptr, *d_x = nullptr, *d_d = nullptr, *d_H = nullptr, *d_G = nullptr, *d_q = nullptr, *d_p = nullptr, *d_y = nullptr, *d_z = nullptr, *d_dir = nullptr,
         *d_bres = nullptr, *d_part = nullptr, *d_res = nullptr, *d_alpha = nullptr, *d_sc = nullptr;
  int *d_nsg = nullptr, *d_nbs = nullptr, *d_run = nullptr, *d_w = nullptr;
  mcba::KpCam* d_cams = nullptr;
  mcba::SkPlan* d_plan = nullptr;
  std::vector<mcba::KpCam> tab((size_t)C);
  for (int c = 0; c < C; ++c) mcba::make_kp_cam(in.cam12 + 12 * c, in.dist5 ? in.dist5 + 5 * c : nullptr, tab[c]);
  if (int rc = call.upload(&d_cams, tab.data(), tab.size())) return rc;
  if (int rc = call.scratch(&d_plan, 1)) return rc;
  if (int rc = call.scratch(&d_det, 2 * C * TK)) return rc;
  if (int rc = call.scratch(&d_sw, C * TK)) return rc;
  for (double** p3 : {&d_x, &d_d, &d_G, &d_q, &d_p, &d_y, &d_z, &d_dir})
    if (int rc = call.scratch(p3, 3 * TK)) return rc;
  if (int rc = call.scratch(&d_H, 6 * TK)) return rc;
  if (int rc = call.scratch(&d_bres, TK)) return rc;
  if (int rc = call.scratch(&d_part, (size_t)mcba::SKT_SUMS * nblk)) return rc;
  if (int rc = call.scratch(&d_res, (size_t)mcba::SKT_SUMS)) return rc;
  if (int rc = call.scratch(&d_alpha, K)) return rc;
  if (int rc = call.scratch(&d_sc, (size_t)mcba::CG_DOUBLES)) return rc;
  if (int rc = call.scratch(&d_w, (size_t)mcba::CG_INTS)) return rc;
  if (int rc = call.scratch(&d_nsg, K)) return rc;
  if (int rc = call.scratch(&d_nbs, K)) return rc;
  if (int rc = call.scratch(&d_run, K)) return rc;

  if (int rc = ch.begin_shared(0)) return rc;
  std::vector<double> h_sw(C * TK);
  for (int cc = 0; cc < C; ++cc) {
    const double ips = 1.0 / in.pixel_std[cc];
    for (size_t i = 0; i < TK; ++i) {
      const double w = in.weights ? in.weights[cc * TK + i] : 1.0;
      h_sw[cc * TK + i] = w > 0.0 ? sqrt(w) * ips : 0.0;   // (a zero or NaN weight: unseen)
    }
  }
  if (int rc = call.put(d_det, in.uvs, 2 * C * TK)) return rc;
  if (int rc = call.put(d_sw, h_sw.data(), C * TK)) return rc;
  if (int rc = call.put(d_x, in.start, 3 * TK)) return rc;
  for (int l = 1; l < ch.levels; ++l) ch.lv[l].x = ch.aux[l];
  const mcba::TrData rd{T, d_det, d_sw, d_x, d_d, d_H, d_G, ch.d_ia2, in.f_scale * in.f_scale, 1.0 / (in.f_scale * in.f_scale)};
  const mcba::SktData sd{rd, d_q, d_p, d_y, d_z, d_dir, d_bres, d_plan, d_run};
  // level 0 of the elimination and of every re-solve: H as the diagonal blocks, -q as the right-hand side (q = G at the elimination), z as the solution
  const mcba::SmData td{T, nullptr, d_H, nullptr, ch.d_ia2, d_z, nullptr, nullptr, mcba::SM_LOSS_LINEAR, 1.0, 1.0, d_q};

  // one bracket of launches: e0 was recorded before them; waits for them and adds their time
  auto close_bracket = [&]() -> int {
    if (int rc = check_launch()) return rc;
    HIPCHK(hipEventRecord(call.e1, nullptr));
    HIPCHK(hipEventSynchronize(call.e1));
    return ch.add_ms(call.e0, call.e1, ch.ms_total);
  };

  HIPCHK(hipEventRecord(call.e0, nullptr));
  if (mcba::launch_traj_count(nullptr, rd, C, Ki, ch.d_nus, d_nsg, d_nbs) != 0) return fail(MCBA_ERR_ARG, "skeleton trajectories: bad launch");
  if (int rc = close_bracket()) return rc;
  std::vector<int> h_nus(K), h_nsg(K), h_nbs(K), h_stat(K), h_run(K, 0), h_bad(K, 0), h_par(K, -1);
  if (int rc = call.download(h_nus.data(), ch.d_nus, K)) return rc;
  if (int rc = call.download(h_nsg.data(), d_nsg, K)) return rc;
  if (int rc = call.download(h_nbs.data(), d_nbs, K)) return rc;
  std::vector<int>& h_list = ch.h_list;
  h_list.clear();
  for (int k = 0; k < Ki; ++k) {
    h_stat[k] = h_nus[k] < 2 ? mcba::TR_TOO_FEW_FRAMES : h_nbs[k] ? mcba::TR_BAD_START : mcba::TR_OK;
    if (h_stat[k] == mcba::TR_OK) { h_list.push_back(k); h_run[k] = 1; }
  }
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
    if (pending) if (int rc = call.put(d_alpha, h_alpha.data(), K)) return rc;
    HIPCHK(hipEventRecord(call.e0, nullptr));
    int lrc = pending ? mcba::launch_traj_apply(nullptr, rd, Ki, d_alpha) : 0;
    lrc = lrc || mcba::launch_traj_linearise(nullptr, loss, rd, d_cams, C, Ki, d_run);
    lrc = lrc || mcba::launch_skt_linearise(nullptr, sd, Ki);
    lrc = lrc || mcba::launch_smooth_reduce(nullptr, ch.lv, ch.levels, td, Ki, ch.d_list, nact, ch.d_bad, true);
    lrc = lrc || mcba::launch_smooth_backsub(nullptr, ch.lv, ch.levels, td, Ki, ch.d_list, nact, true);
    if (lrc) return fail(MCBA_ERR_ARG, "skeleton trajectories: bad launch");
    if (out.system && out.resolve_check) {
      // the re-solve held against the elimination on the same right-hand side: z is kept, the right-hand-side halves of every stored record,
      // every level's solution and z are overwritten with NaN (all bits set), and the re-solve with the same back-substitution makes z again
      if (int rc = close_bracket()) return rc;
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
      HIPCHK(hipEventRecord(call.e0, nullptr));
      if (mcba::launch_smooth_resolve(nullptr, ch.lv, ch.levels, td, Ki, ch.d_list, nact, nullptr) || mcba::launch_smooth_backsub(nullptr, ch.lv, ch.levels, td, Ki, ch.d_list, nact, true))
        return fail(MCBA_ERR_ARG, "skeleton trajectories: bad launch");
      if (int rc = close_bracket()) return rc;
      if (int rc = call.download(out.resolve_check + 3 * TK, d_z, 3 * TK)) return rc;
      HIPCHK(hipEventRecord(call.e0, nullptr));
    }
    if (mcba::launch_skt_cg_start(nullptr, sd, Ki, d_part, d_sc, d_w)) return fail(MCBA_ERR_ARG, "skeleton trajectories: bad launch");
    for (int launched = 0;;) {
      for (int i = 0; i < mcba::SKT_HOST_READS_EVERY && launched < in.cg_max; ++i, ++launched)
        if (mcba::launch_skt_cg_iteration(nullptr, sd, Ki, ch.lv, ch.levels, td, ch.d_list, nact, tol2, in.cg_max, d_part, d_sc, d_w)) return fail(MCBA_ERR_ARG, "skeleton trajectories: bad launch");
      if (int rc = close_bracket()) return rc;
      if (int rc = call.download(w, d_w, (size_t)mcba::CG_INTS)) return rc;
      HIPCHK(hipEventRecord(call.e0, nullptr));
      if (w[mcba::CG_DONE] || launched >= in.cg_max) break;
    }
    if (mcba::launch_skt_trial(nullptr, loss, sd, d_cams, C, Ki, d_part, d_res)) return fail(MCBA_ERR_ARG, "skeleton trajectories: bad launch");
    if (int rc = close_bracket()) return rc;
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
    if (pending) if (int rc = call.put(d_alpha, h_alpha.data(), K)) return rc;
    HIPCHK(hipEventRecord(call.e0, nullptr));
    int lrc = pending ? mcba::launch_traj_apply(nullptr, rd, Ki, d_alpha) : 0;
    lrc = lrc || mcba::launch_traj_linearise(nullptr, loss, rd, d_cams, C, Ki, d_run);
    lrc = lrc || mcba::launch_skt_linearise(nullptr, sd, Ki);
    if (lrc) return fail(MCBA_ERR_ARG, "skeleton trajectories: bad launch");
    if (int rc = close_bracket()) return rc;
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
  double* info8 = out.info8;
  info8[0] = ch.levels; info8[1] = segment; info8[2] = nact; info8[3] = cg_total; info8[4] = ch.ms_total; info8[5] = n_it;
  info8[6] = (double)total * sizeof(double); info8[7] = 0.0;
  if (out.kernel_ms) *out.kernel_ms = ch.ms_total;
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
