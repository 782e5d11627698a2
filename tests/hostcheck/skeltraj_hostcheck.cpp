// Host build of csrc/mcba_skeltraj_math.h -- the per-lane text of csrc/mcba_skeltraj.hip -- and of smooth_resolve_lane of csrc/mcba_smooth_math.h,
// for g++: serial loops over the lanes in the kernels' order (flat over (frame, keypoint), sums as a tree over 256 lanes and then over the
// partials), the conjugate-gradient recurrence and the Gauss-Newton loop of mcba_skeltraj_api.hip around them.
// tests/test_hostcheck_skeltraj.py compiles this as a shared library (plain -O2) and holds it to the GPU tier's rules.
#include <cmath>
#include <cstddef>
#include <cstring>
#include <type_traits>
#include <vector>
#include "../../multicam-calibration_amd/csrc/mcba_skeltraj_math.h"

using namespace mcba;

namespace {

template <class F>
void with_loss3(int loss, F&& f) {
  if (loss == LOSS_LINEAR) f(std::integral_constant<int, LOSS_LINEAR>{});
  else if (loss == LOSS_SOFT_L1) f(std::integral_constant<int, LOSS_SOFT_L1>{});
  else f(std::integral_constant<int, LOSS_HUBER>{});
}

enum Pass { REDUCE, RESOLVE };
void forward(Pass pass, const SmLevel* lv, int levels, const SmData& td, int K, const std::vector<int>& list, int* bad) {
  const SmLevel none{};
  const int nact = (int)list.size();
  for (int l = 0; l < levels; ++l) {
    const int nq = smooth_lanes(lv[l]);
    const SmLevel& nx = l + 1 < levels ? lv[l + 1] : none;
    for (size_t gid = 0; gid < (size_t)nq * nact; ++gid) {
      const int k = list[gid % nact], q = (int)(gid / nact);
      if (pass == REDUCE && l == 0) smooth_reduce_lane<true, true>(lv[0], nx, td, K, k, q, bad);
      else if (pass == REDUCE) smooth_reduce_lane<false>(lv[l], nx, td, K, k, q, bad);
      else if (l == 0) smooth_resolve_lane<true>(lv[0], nx, td, K, k, q);
      else smooth_resolve_lane<false>(lv[l], nx, td, K, k, q);
    }
  }
}

void substitute(const SmLevel* lv, int levels, const SmData& td, int K, const std::vector<int>& list) {
  const SmLevel none{};
  const int nact = (int)list.size();
  for (int l = levels - 1; l >= 0; --l) {
    const int nq = smooth_lanes(lv[l]);
    const SmLevel& up = l + 1 < levels ? lv[l + 1] : none;
    for (size_t gid = 0; gid < (size_t)nq * nact; ++gid) {
      if (l == 0) smooth_backsub_lane<true, true>(lv[0], up, td, K, list[gid % nact], (int)(gid / nact));
      else smooth_backsub_lane<false>(lv[l], up, td, K, list[gid % nact], (int)(gid / nact));
    }
  }
}

// the sums of a flat launch in the kernels' order: per workgroup a tree over its 256 lanes, then one workgroup over the partials.  lane(i, acc)
// adds lane i's share to acc (N doubles, zero on entry); is_max marks the sums that are maxima
template <int N, class F>
void flat_sums(size_t lanes, const bool* is_max, double* out, F&& lane) {
  const size_t nblk = (lanes + 255) / 256;
  std::vector<double> part(N * nblk);
  auto tree = [&](double (*s)[256]) {
    for (int h = 128; h > 0; h >>= 1)
      for (int i = 0; i < h; ++i)
        for (int e = 0; e < N; ++e) s[e][i] = is_max[e] ? fmax(s[e][i], s[e][i + h]) : s[e][i] + s[e][i + h];
  };
  for (size_t b = 0; b < nblk; ++b) {
    double s[N][256];
    for (int i = 0; i < 256; ++i) {
      double acc[N];
      for (int e = 0; e < N; ++e) acc[e] = 0.0;
      const size_t idx = b * 256 + i;
      if (idx < lanes) lane(idx, acc);
      for (int e = 0; e < N; ++e) s[e][i] = acc[e];
    }
    tree(s);
    for (int e = 0; e < N; ++e) part[N * b + e] = s[e][0];
  }
  double s[N][256];
  for (int i = 0; i < 256; ++i) {
    for (int e = 0; e < N; ++e) s[e][i] = 0.0;
    for (size_t b = i; b < nblk; b += 256)
      for (int e = 0; e < N; ++e) s[e][i] = is_max[e] ? fmax(s[e][i], part[N * b + e]) : s[e][i] + part[N * b + e];
  }
  tree(s);
  for (int e = 0; e < N; ++e) out[e] = s[e][0];
}

}  // namespace

// the arguments of mcba_refine_skeleton_trajectories (system == 0) or mcba_refine_skeleton_trajectories_system (system != 0); outputs of the other
// mode may be null.  resolve_check (2 T K 3, or null; system only): the solution of M z = -G by the re-solve from the stored factors, after the
// right-hand-side halves of every record were overwritten with NaN, beside the fresh elimination's
extern "C" int hc_refine_skeleton_trajectories(int system, size_t T, int K, int C, const double* uvs, const double* cam12, const double* dist5, const double* weights, const double* pixel_std,
                                               const double* start, const double* accel_std, const int* parent, const double* bone_length, const double* bone_std, int loss, double f_scale,
                                               int max_iterations, double xtol, double cg_tol, int cg_max, int segment, double* out_points, double* information, int* status, int* n_usable,
                                               int* n_single, int* converged_out, int* n_iterations, double* cost_out, double* cost_start_out, double* history, double* bone_residual,
                                               double* direction, double* gradient, double* step, int* cg_iterations, double* cg_residual, double* data_cost, double* penalty_cost,
                                               double* bone_cost, double* trial_costs, double* info8, double* resolve_check) {
  if (T < 1 || K < 1 || K > SK_MAX_K || C < 1 || C > kKpMaxCams || loss < 0 || loss > 2 || !(f_scale > 0.0) || (segment != 0 && (segment < SM_SEGMENT_MIN || segment > SM_SEGMENT_MAX))) return 1;
  if (system) max_iterations = 1;
  if (max_iterations < 1 || !(cg_tol > 0.0 && cg_tol < 1.0) || cg_max < 1) return 1;
  if (segment == 0) segment = SM_SEGMENT_DEFAULT;
  const double nan = std::nan(""), tol2 = cg_tol * cg_tol;
  const size_t TK = T * K;
  SmLevel lv[SM_MAX_LEVELS];
  double* aux[SM_MAX_LEVELS];
  int levels = 0;
  std::vector<double> store(smooth_carve(T, segment, K, lv, 6, nullptr, nullptr), nan);   // NaN-filled: whatever reads a word nobody wrote shows
  if (store.empty()) return 1;
  smooth_carve(T, segment, K, lv, 6, store.data(), aux, &levels);
  for (int l = 1; l < levels; ++l) lv[l].x = aux[l];
  std::vector<KpCam> cams(C);
  for (int c = 0; c < C; ++c) make_kp_cam(cam12 + 12 * c, dist5 ? dist5 + 5 * c : nullptr, cams[c]);
  std::vector<double> sw((size_t)C * TK), x(start, start + 3 * TK), d(3 * TK, nan), H(6 * TK, nan), G(3 * TK, nan), q(3 * TK, nan), p(3 * TK, nan), y(3 * TK, nan), z(3 * TK, nan), dir(3 * TK, nan),
      bres(TK, nan), ia2(K);
  kp_weight_box(weights, pixel_std, C, T, K, 0, T, 0, K, sw.data());
  for (int k = 0; k < K; ++k) ia2[k] = 1.0 / (accel_std[k] * accel_std[k]);
  const TrData rd{T, uvs, sw.data(), x.data(), d.data(), H.data(), G.data(), ia2.data(), f_scale * f_scale, 1.0 / (f_scale * f_scale)};
  const SmData td{T, nullptr, H.data(), nullptr, ia2.data(), z.data(), nullptr, nullptr, SM_LOSS_LINEAR, 1.0, 1.0, q.data()};
  std::vector<int> bad(K, 0), list, stat(K), run(K, 0), par(K, -1);
  for (int k = 0; k < K; ++k) {
    double acc[3] = {0.0, 0.0, 0.0};
    for (size_t t = 0; t < T; ++t) traj_count_frame(rd, C, K, k, t, acc);
    n_usable[k] = (int)acc[0]; n_single[k] = (int)acc[1];
    stat[k] = traj_start_status(n_usable[k], acc[2] != 0.0);
    if (stat[k] == TR_OK) { list.push_back(k); run[k] = 1; }
  }
  for (int k = 0; k < K; ++k) par[k] = run[k] && parent[k] >= 0 && run[parent[k]] ? parent[k] : -1;
  SkPlan plan;
  if (skel_plan(K, par.data(), bone_length, bone_std, plan) != 0) return 1;
  const SktData sd{rd, q.data(), p.data(), y.data(), z.data(), dir.data(), bres.data(), &plan, run.data()};
  if (history)
    for (size_t i = 0; i < (size_t)max_iterations * 4; ++i) history[i] = nan;
  const bool one_sum[1] = {false};
  bool trial_max[SKT_SUMS];
  for (int e = 0; e < SKT_SUMS; ++e) trial_max[e] = e == TR_DMAX || e == TR_XMAX;
  auto linearise = [&]() {
    with_loss3(loss, [&](auto L) {
      for (size_t i = 0; i < TK; ++i)
        if (run[i % K]) traj_linearise_lane<decltype(L)::value>(cams.data(), C, rd, K, (int)(i % K), i / K);
    });
    for (size_t i = 0; i < TK; ++i) skt_linearise_lane(sd, K, (int)(i % K), i / K);
  };
  double alpha = 0.0, res[SKT_SUMS], sc[CG_DOUBLES], cost = nan, cost_start = nan;
  int w[CG_INTS] = {0, 0}, n_it = 0, cg_total = 0;
  bool stopped = list.empty(), converged = false;
  for (int e = 0; e < SKT_SUMS; ++e) res[e] = nan;
  for (int it = 0; it < max_iterations && !stopped; ++it) {
    for (size_t i = 0; i < TK; ++i) traj_apply_lane(rd, i, run[i % K] ? alpha : 0.0);
    linearise();
    forward(REDUCE, lv, levels, td, K, list, bad.data());
    substitute(lv, levels, td, K, list);
    if (resolve_check && system) {
      memcpy(resolve_check, z.data(), 3 * TK * sizeof(double));
      for (int l = 0; l < levels; ++l) {
        for (size_t i = 0; i < 6 * lv[l].NS; ++i) lv[l].fac[57 * lv[l].NS + i] = nan;
        if (l)
          for (size_t i = 0; i < 6 * lv[l].NS; ++i) lv[l].sep[21 * lv[l].NS + i] = lv[l].sep[48 * lv[l].NS + i] = lv[l].x[i] = nan;
      }
      std::fill(z.begin(), z.end(), nan);
      forward(RESOLVE, lv, levels, td, K, list, nullptr);
      substitute(lv, levels, td, K, list);
      memcpy(resolve_check + 3 * TK, z.data(), 3 * TK * sizeof(double));
    }
    double sum;
    flat_sums<1>(TK, one_sum, &sum, [&](size_t i, double* acc) { if (run[i % K]) acc[0] = skt_start_lane(sd, i); });
    skt_scalars(CG_START, sum, tol2, cg_max, sc, w);
    for (int launched = 0; launched < cg_max && !w[CG_DONE]; ++launched) {
      flat_sums<1>(TK, one_sum, &sum, [&](size_t i, double* acc) { if (run[i % K]) acc[0] = skt_operator_lane(sd, K, (int)(i % K), i / K); });
      skt_scalars(CG_AFTER_OPERATOR, sum, tol2, cg_max, sc, w);
      if (w[CG_DONE]) break;
      for (size_t i = 0; i < TK; ++i)
        if (run[i % K]) skt_step_lane(sd, i, sc[CG_ALPHA]);
      forward(RESOLVE, lv, levels, td, K, list, nullptr);
      substitute(lv, levels, td, K, list);
      flat_sums<1>(TK, one_sum, &sum, [&](size_t i, double* acc) { if (run[i % K]) acc[0] = skt_dot_lane(sd, i); });
      skt_scalars(CG_AFTER_DOT, sum, tol2, cg_max, sc, w);
      if (w[CG_DONE]) break;
      for (size_t i = 0; i < TK; ++i)
        if (run[i % K]) skt_direction_lane(sd, i, sc[CG_BETA]);
    }
    with_loss3(loss, [&](auto L) {
      flat_sums<SKT_SUMS>(TK, trial_max, res, [&](size_t i, double* acc) { if (run[i % K]) skt_trial_lane<decltype(L)::value>(cams.data(), C, sd, K, (int)(i % K), i / K, acc); });
    });
    alpha = 0.0;
    bool pivot = false;
    for (int k : list)
      if (bad[k]) { stat[k] = TR_PIVOT; pivot = true; }
    if (it == 0) {
      cost_start = cost = res[0];
      if (!pivot && !sm_finite(res[0]))
        for (int k : list) stat[k] = TR_BAD_START;
    }
    if (system) { n_it = 1; cg_total = w[CG_ITERATIONS]; }
    if (pivot || !sm_finite(res[0]) || system) break;   // (such an iteration accepts nothing and is not counted)
    n_it = it + 1;
    cg_total += w[CG_ITERATIONS];
    stopped = traj_decide(res, xtol, it, max_iterations, alpha, cost);
    converged = skt_converged(res, xtol, alpha);
    double* h = history + (size_t)it * 4;
    h[0] = cost; h[1] = alpha * res[TR_DMAX]; h[2] = alpha; h[3] = w[CG_ITERATIONS];
  }
  bool any_ok = false;
  for (int k = 0; k < K; ++k) any_ok = any_ok || stat[k] == TR_OK;
  if (any_ok && !system) {
    for (size_t i = 0; i < TK; ++i) traj_apply_lane(rd, i, run[i % K] ? alpha : 0.0);
    linearise();
  }
  for (int k = 0; k < K; ++k) {
    const bool ok = stat[k] == TR_OK, bone = ok && par[k] >= 0 && stat[par[k]] == TR_OK;
    status[k] = stat[k];
    for (size_t t = 0; t < T; ++t) {
      const size_t i = t * K + k;
      for (int e = 0; e < 6; ++e) information[6 * i + e] = ok ? H[6 * i + e] : nan;
      for (int e = 0; e < 3; ++e) {
        direction[3 * i + e] = bone ? dir[3 * i + e] : nan;
        if (system) { gradient[3 * i + e] = ok ? G[3 * i + e] : nan; step[3 * i + e] = ok ? d[3 * i + e] : nan; }
        else out_points[3 * i + e] = ok ? x[3 * i + e] : nan;
      }
      if (!system) bone_residual[i] = bone ? bres[i] : nan;
    }
  }
  if (system) {
    *cg_iterations = any_ok ? w[CG_ITERATIONS] : 0;
    *cg_residual = any_ok ? (sc[CG_RZ0] > 0.0 ? sqrt(fmax(sc[CG_RZ], 0.0) / sc[CG_RZ0]) : 0.0) : nan;
    *data_cost = any_ok ? res[TR_DATA] : nan;
    *penalty_cost = any_ok ? res[TR_PEN] : nan;
    *bone_cost = any_ok ? res[SKT_BONE] : nan;
    for (int a = 0; a < TR_TRIALS; ++a) trial_costs[a] = any_ok ? res[1 + a] : nan;
  } else {
    *converged_out = any_ok && converged ? 1 : 0;
    *n_iterations = n_it;
    *cost_out = any_ok ? cost : nan;
    *cost_start_out = any_ok ? cost_start : nan;
  }
  for (int i = 0; i < 8; ++i) info8[i] = 0.0;
  info8[0] = levels; info8[1] = segment; info8[2] = (double)list.size(); info8[3] = cg_total; info8[5] = n_it;
  info8[6] = (double)skeltraj_chunk_doubles(T, K, C, segment) * sizeof(double);
  return 0;
}
