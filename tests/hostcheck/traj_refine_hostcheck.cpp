// Host build of csrc/mcba_traj_refine_math.h -- the per-lane text of csrc/mcba_traj_refine.hip (k_traj_count, k_traj_linearise, k_traj_trial,
// k_traj_apply) -- and of the right-hand-side mode of csrc/mcba_smooth_math.h, for g++: serial loops over the lanes in the kernels' order, the
// Gauss-Newton loop of mcba_traj_refine_api.hip around them with its accept and stop rule, the selected inversion at the returned points.
// tests/test_hostcheck_traj_refine.py compiles this as a shared library (plain -O2) and holds it to the GPU tier's rules.
#include <cmath>
#include <cstddef>
#include <cstring>
#include <type_traits>
#include <vector>
#include "../../multicam-calibration_amd/csrc/mcba_traj_refine_math.h"

using namespace mcba;

namespace {

template <class F>
void with_loss3(int loss, F&& f) {
  if (loss == LOSS_LINEAR) f(std::integral_constant<int, LOSS_LINEAR>{});
  else if (loss == LOSS_SOFT_L1) f(std::integral_constant<int, LOSS_SOFT_L1>{});
  else f(std::integral_constant<int, LOSS_HUBER>{});
}

void eliminate(const SmLevel* lv, int levels, const SmData& td, int K, const std::vector<int>& list, int* bad) {
  const SmLevel none{};
  const int nact = (int)list.size();
  for (int l = 0; l < levels; ++l) {
    const int nq = smooth_lanes(lv[l]);
    const SmLevel& nx = l + 1 < levels ? lv[l + 1] : none;
    for (size_t gid = 0; gid < (size_t)nq * nact; ++gid) {
      if (l == 0) smooth_reduce_lane<true, true>(lv[0], nx, td, K, list[gid % nact], (int)(gid / nact), bad);
      else smooth_reduce_lane<false>(lv[l], nx, td, K, list[gid % nact], (int)(gid / nact), bad);
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

void invert(const SmLevel* lv, int levels, const SmData& td, double* const* z, double* cov6, double* lag9, int K, const std::vector<int>& list) {
  const SmLevel none{};
  const int nact = (int)list.size();
  for (int l = levels - 1; l >= 0; --l) {
    const int nq = smooth_lanes(lv[l]);
    const SmLevel& up = l + 1 < levels ? lv[l + 1] : none;
    const double* zup = l + 1 < levels ? z[l + 1] : nullptr;
    for (size_t gid = 0; gid < (size_t)nq * nact; ++gid) {
      if (l == 0) smooth_selinv_lane<true>(lv[0], up, td, nullptr, zup, cov6, lag9, K, list[gid % nact], (int)(gid / nact));
      else smooth_selinv_lane<false>(lv[l], up, td, z[l], zup, nullptr, nullptr, K, list[gid % nact], (int)(gid / nact));
    }
  }
}

}  // namespace

// the arguments of mcba_refine_trajectories (system == 0) or mcba_refine_trajectories_system (system != 0: max_iterations and xtol unused, points
// = where to evaluate); one chunk of all K tracks.  Outputs of the other mode may be null
extern "C" int hc_refine_trajectories(int system, size_t T, int K, int C, const double* uvs, const double* cam12, const double* dist5, const double* weights, const double* pixel_std,
                                      const double* start, const double* accel_std, int loss, double f_scale, int max_iterations, double xtol, int segment, double* out_points, double* information,
                                      int* status, int* n_usable, int* n_single, int* n_iterations, double* cost, double* history, double* out_cov6, double* out_lag9, double* gradient, double* step,
                                      double* data_cost, double* penalty_cost, double* trial_costs, double* info8) {
  if (T < 1 || K < 1 || C < 1 || C > kKpMaxCams || loss < 0 || loss > 2 || !(f_scale > 0.0) || (segment != 0 && (segment < SM_SEGMENT_MIN || segment > SM_SEGMENT_MAX))) return 1;
  if (system) max_iterations = 1;
  if (max_iterations < 1) return 1;
  if (segment == 0) segment = SM_SEGMENT_DEFAULT;
  const bool cov = out_cov6 != nullptr;
  const double nan = std::nan("");
  const size_t TK = T * K;
  SmLevel lv[SM_MAX_LEVELS];
  double* aux[SM_MAX_LEVELS];
  int levels = 0;
  const int extra = cov ? SM_ZC : 6;
  std::vector<double> store(smooth_carve(T, segment, K, lv, extra, nullptr, nullptr), nan);   // NaN-filled: whatever reads a word nobody wrote shows
  if (store.empty()) return 1;
  smooth_carve(T, segment, K, lv, extra, store.data(), aux, &levels);
  for (int l = 1; l < levels; ++l) lv[l].x = aux[l];
  std::vector<KpCam> cams(C);
  for (int c = 0; c < C; ++c) make_kp_cam(cam12 + 12 * c, dist5 ? dist5 + 5 * c : nullptr, cams[c]);
  std::vector<double> sw((size_t)C * TK), x(start, start + 3 * TK), d(3 * TK, nan), H(6 * TK, nan), G(3 * TK, nan), ia2(K), oc(cov ? 6 * TK : 0, nan), ol(out_lag9 ? 9 * (T - 1) * K : 0, nan);
  kp_weight_box(weights, pixel_std, C, T, K, 0, T, 0, K, sw.data());
  for (int k = 0; k < K; ++k) ia2[k] = 1.0 / (accel_std[k] * accel_std[k]);
  const TrData rd{T, uvs, sw.data(), x.data(), d.data(), H.data(), G.data(), ia2.data(), f_scale * f_scale, 1.0 / (f_scale * f_scale)};
  SmData td{T, nullptr, H.data(), nullptr, ia2.data(), d.data(), nullptr, nullptr, SM_LOSS_LINEAR, 1.0, 1.0, G.data()};
  std::vector<int> bad(K, 0), list, stat(K), nit(K, 0);
  std::vector<double> alpha(K, 0.0), fcost(K, nan), res((size_t)TR_SUMS * K, nan);
  for (int k = 0; k < K; ++k) {
    double acc[3] = {0.0, 0.0, 0.0};
    for (size_t t = 0; t < T; ++t) traj_count_frame(rd, C, K, k, t, acc);
    n_usable[k] = (int)acc[0]; n_single[k] = (int)acc[1];
    stat[k] = traj_start_status(n_usable[k], acc[2] != 0.0);
    if (stat[k] == TR_OK) list.push_back(k);
  }
  const std::vector<int> ran = list;
  if (history)
    for (size_t i = 0; i < (size_t)max_iterations * K * 3; ++i) history[i] = nan;
  auto apply = [&]() {
    for (size_t i = 0; i < TK; ++i) traj_apply_lane(rd, i, alpha[i % K]);
  };
  auto linearise = [&](const std::vector<int>& tracks) {
    std::vector<int> run(K, 0);
    for (int k : tracks) run[k] = 1;
    with_loss3(loss, [&](auto L) {
      for (size_t i = 0; i < TK; ++i)
        if (run[i % K]) traj_linearise_lane<decltype(L)::value>(cams.data(), C, rd, K, (int)(i % K), i / K);
    });
  };
  int most = 0;
  for (int it = 0; it < max_iterations && !list.empty(); ++it) {
    apply();
    linearise(list);
    eliminate(lv, levels, td, K, list, bad.data());
    substitute(lv, levels, td, K, list);
    std::vector<int> next;
    most = it + 1;
    for (int kk = 0; kk < (int)list.size(); ++kk) {
      const int k = list[kk];
      // the sums in the kernels' order: per workgroup of 256 frames a tree over its lanes, then the workgroups in order
      double* r = res.data() + (size_t)TR_SUMS * k;
      const int nblk = smooth_eval_blocks(T);
      std::vector<double> part((size_t)TR_SUMS * nblk, 0.0);
      with_loss3(loss, [&](auto L) {
        for (int b = 0; b < nblk; ++b) {
          double s[TR_SUMS][256];
          for (int i = 0; i < 256; ++i) {
            double acc[TR_SUMS];
            for (int e = 0; e < TR_SUMS; ++e) acc[e] = 0.0;
            const size_t t = (size_t)b * 256 + i;
            if (t < T) traj_trial_lane<decltype(L)::value>(cams.data(), C, rd, K, k, t, acc);
            for (int e = 0; e < TR_SUMS; ++e) s[e][i] = acc[e];
          }
          for (int h = 128; h > 0; h >>= 1)
            for (int i = 0; i < h; ++i)
              for (int e = 0; e < TR_SUMS; ++e) s[e][i] = e >= TR_DMAX ? fmax(s[e][i], s[e][i + h]) : s[e][i] + s[e][i + h];
          for (int e = 0; e < TR_SUMS; ++e) part[(size_t)TR_SUMS * b + e] = s[e][0];
        }
      });
      {
        double s[TR_SUMS][256];
        for (int i = 0; i < 256; ++i) {
          for (int e = 0; e < TR_SUMS; ++e) s[e][i] = 0.0;
          for (int b = i; b < nblk; b += 256)
            for (int e = 0; e < TR_SUMS; ++e) s[e][i] = e >= TR_DMAX ? fmax(s[e][i], part[(size_t)TR_SUMS * b + e]) : s[e][i] + part[(size_t)TR_SUMS * b + e];
        }
        for (int h = 128; h > 0; h >>= 1)
          for (int i = 0; i < h; ++i)
            for (int e = 0; e < TR_SUMS; ++e) s[e][i] = e >= TR_DMAX ? fmax(s[e][i], s[e][i + h]) : s[e][i] + s[e][i + h];
        for (int e = 0; e < TR_SUMS; ++e) r[e] = e == TR_PEN ? 0.5 * ia2[k] * s[e][0] : s[e][0];
      }
    }
    if (system) break;
    std::fill(alpha.begin(), alpha.end(), 0.0);
    for (int k : list) {
      const double* r = res.data() + (size_t)TR_SUMS * k;
      nit[k] = it + 1;
      if (bad[k]) { stat[k] = TR_PIVOT; continue; }
      double a, c;
      const bool stops = traj_decide(r, xtol, it, max_iterations, a, c);
      double* h = history + ((size_t)it * K + k) * 3;
      h[0] = c; h[1] = a * r[TR_DMAX]; h[2] = a;
      alpha[k] = a;
      fcost[k] = c;
      if (!stops) next.push_back(k);
    }
    list.swap(next);
  }
  if (!system) {
    list.clear();
    for (int k : ran)
      if (stat[k] == TR_OK) list.push_back(k);
    if (!list.empty()) {
      apply();
      linearise(list);
      if (cov) {
        eliminate(lv, levels, td, K, list, bad.data());
        invert(lv, levels, td, aux, oc.data(), out_lag9 ? ol.data() : nullptr, K, list);
        for (int k : list)
          if (bad[k]) stat[k] = TR_PIVOT;
      }
    }
  }
  for (int k = 0; k < K; ++k) {
    if (system && stat[k] == TR_OK && bad[k]) stat[k] = TR_PIVOT;
    const bool ok = stat[k] == TR_OK;
    status[k] = stat[k];
    for (size_t t = 0; t < T; ++t) {
      const size_t i = t * K + k;
      for (int e = 0; e < 6; ++e) information[6 * i + e] = ok ? H[6 * i + e] : nan;
      for (int e = 0; e < 3; ++e) {
        if (system) { gradient[3 * i + e] = ok ? G[3 * i + e] : nan; step[3 * i + e] = ok ? d[3 * i + e] : nan; }
        else out_points[3 * i + e] = ok ? x[3 * i + e] : nan;
      }
      if (cov)
        for (int e = 0; e < 6; ++e) out_cov6[6 * i + e] = ok ? oc[6 * i + e] : nan;
      if (out_lag9 && t + 1 < T)
        for (int e = 0; e < 9; ++e) out_lag9[9 * i + e] = ok ? ol[9 * i + e] : nan;
    }
    const double* r = res.data() + (size_t)TR_SUMS * k;
    if (system) {
      data_cost[k] = ok ? r[TR_DATA] : nan;
      penalty_cost[k] = ok ? r[TR_PEN] : nan;
      for (int a = 0; a < TR_TRIALS; ++a) trial_costs[TR_TRIALS * k + a] = ok ? r[1 + a] : nan;
    } else {
      n_iterations[k] = nit[k];
      cost[k] = ok ? fcost[k] : nan;
    }
  }
  for (int i = 0; i < 8; ++i) info8[i] = 0.0;
  info8[0] = levels; info8[1] = segment; info8[2] = K; info8[3] = 1; info8[5] = most;
  return 0;
}

// the weight plane of the detection calls, one sub-box of it: kp_weight_box (mcba_keypoint_math.h) as the C calls use it
extern "C" void hc_weight_box(const double* weights, const double* pixel_std, int C, size_t T, size_t K, size_t t0, size_t tc, size_t k0, size_t kc, double* out) {
  kp_weight_box(weights, pixel_std, C, T, K, t0, tc, k0, kc, out);
}

// the chunk rule of the C call: out4 = tracks per chunk, chunks, device bytes, levels
extern "C" int hc_refine_chunks(size_t T, int K, int C, int segment, int cov, int lag, double budget_mb, double* out4) {
  if (segment == 0) segment = SM_SEGMENT_DEFAULT;
  int nchunks = 0, levels = 0;
  const int Kc = smooth_chunk_tracks(budget_mb * 1048576.0, traj_refine_chunk_doubles(T, 1, C, segment, cov != 0, lag != 0), (size_t)K, nchunks);
  SmLevel lv[SM_MAX_LEVELS];
  smooth_carve(T, segment, Kc, lv, cov ? SM_ZC : 6, nullptr, nullptr, &levels);
  out4[0] = Kc; out4[1] = nchunks; out4[2] = (double)traj_refine_chunk_doubles(T, Kc, C, segment, cov != 0, lag != 0) * sizeof(double); out4[3] = levels;
  return 0;
}
