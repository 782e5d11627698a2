// mcba_traj_refine_math.h -- the per-lane arithmetic of csrc/mcba_traj_refine.hip: keypoint tracks refined on the detections.
// Per track, frames t = 0 .. T-1, unknowns x_t in R^3:
//   minimise 0.5 sum_t sum_{c sees (t, k)} f^2 [rho(ru^2 / f^2) + rho(rv^2 / f^2)] + 0.5 / a^2 sum_{t=1}^{T-2} |x_{t-1} - 2 x_t + x_{t+1}|^2,
//   (ru, rv) = sw (detection - project5_c(x_t)),  sw = sqrt(w) / pixel_std_c
// by Gauss-Newton in step form with a backtracking trial: per iteration
//   linearise  H_t, g_t of the data term (keypoint_linearise, its curvature weights), G_t = g_t + a^-2 (D2^T D2 x)_t          traj_linearise_lane
//   solve      (blockdiag(H_t) + a^-2 D2^T D2 (x) I3) d = -G: the smoother's elimination, level 0 in its right-hand-side mode   mcba_smooth_math.h
//   trial      the objective at x + alpha d, alpha = 0, 1, 1/2, 1/4, 1/8, the detections read once; max |d|, max |x|             traj_trial_lane
//   accept     the largest alpha whose objective is not above the one at alpha = 0 (NaN compares false); stop or go on           traj_decide
// A frame is usable when two cameras or more see it, single when exactly one does (a detection is seen under the rule of kp_observe); a track
// runs with two usable frames and a finite start.  Detections lie as (C, T K) pairs, tracks fastest, sw beside them as (C, T K).
// The same text is compiled with g++ into tests/hostcheck/traj_refine_hostcheck.cpp (tests/test_hostcheck_traj_refine.py).
#pragma once
#include "mcba_keypoint_math.h"
#include "mcba_smooth_cov_math.h"

namespace mcba {

// status of a track
constexpr int TR_OK = 1, TR_TOO_FEW_FRAMES = -1, TR_PIVOT = -2, TR_BAD_START = -3;
constexpr int TR_TRIALS = 4;   // alpha = 1, 1/2, 1/4, 1/8
// the sums of one track: the objective at alpha = 0 and at the trials | the data cost at x | sum |second difference|^2 at x | max |d| | max |x|
constexpr int TR_SUMS = TR_TRIALS + 5, TR_DATA = TR_TRIALS + 1, TR_PEN = TR_TRIALS + 2, TR_DMAX = TR_TRIALS + 3, TR_XMAX = TR_TRIALS + 4;
MCBA_HD double traj_alpha(int a) { return a == 0 ? 0.0 : a == 1 ? 1.0 : a == 2 ? 0.5 : a == 3 ? 0.25 : 0.125; }

// the detections of one (frame, track): element c of a plane lies `stride` = T K further
struct TrObs {
  const double* det;
  const double* sw;
  size_t stride;
  MCBA_HD void operator()(int c, double& ou, double& ov, double& s) const {
    const size_t i = (size_t)c * stride;
    ou = det[2 * i]; ov = det[2 * i + 1];
    s = sw[i];
  }
};

// the planes of one chunk of K tracks
struct TrData {
  size_t T;
  const double* det;   // (C, T K, 2)
  const double* sw;    // (C, T K)
  double* x;           // (T, K, 3): the points
  double* d;           // (T, K, 3): the step
  double* H;           // (T, K, 6): packed 00 01 02 11 12 22, as SmData::winv
  double* G;           // (T, K, 3): the gradient of the whole objective
  const double* ia2;   // (K)
  double fs2, inv_fs2;
};

MCBA_HD TrObs traj_obs(const TrData& rd, int K, int k, size_t t) {
  const size_t idx = t * K + k;
  return TrObs{rd.det + 2 * idx, rd.sw + idx, rd.T * (size_t)K};
}

// device doubles (and ints, counted as doubles) one chunk of K tracks needs: the detection and weight planes (3 C per frame), x, d, H, G (15),
// the covariance planes on request, the per-track words, the partial sums, the levels (their extra plane holds the solution of a level, or
// with cov the SM_ZC planes whose first six hold it)
inline size_t traj_refine_chunk_doubles(size_t T, int K, int C, int segment, bool cov, bool lag) {
  SmLevel lv[SM_MAX_LEVELS];
  return (size_t)T * K * (3 * (size_t)C + 15 + (cov ? 6 : 0) + (lag ? 9 : 0)) + (size_t)K * (8 + TR_SUMS) + (size_t)TR_SUMS * smooth_eval_blocks(T) * K +
         smooth_carve(T, segment, K, lv, cov ? SM_ZC : 6, nullptr, nullptr);
}

// ---- count: one (frame, track): acc = (usable, single, a non-finite coordinate of the start)
MCBA_HD void traj_count_frame(const TrData& rd, int C, int K, int k, size_t t, double* acc) {
  TrObs obs = traj_obs(rd, K, k, t);
  int views = 0;
  for (int c = 0; c < C; ++c) {
    double ou, ov, sw;
    if (kp_observe(obs, c, ou, ov, sw, 0)) ++views;
  }
  acc[0] += views >= 2 ? 1.0 : 0.0;
  acc[1] += views == 1 ? 1.0 : 0.0;
  const size_t idx = t * K + k;
  acc[2] += sm_finite(rd.x[3 * idx]) && sm_finite(rd.x[3 * idx + 1]) && sm_finite(rd.x[3 * idx + 2]) ? 0.0 : 1.0;
}

// ---- linearise: one (frame, track) at x: H_t and the gradient of the whole objective.  The stencil of D2^T D2 is the elimination's own
// (sm_pen_diag, sm_pen_off1, sm_pen_off2): a neighbour outside the track has a zero coefficient and is not read
template <int LOSS>
MCBA_HD void traj_linearise_lane(const KpCam* cams, int C, const TrData& rd, int K, int k, size_t t) {
  const size_t idx = t * K + k;
  const long long tt = (long long)t;
  const double X[3] = {rd.x[3 * idx], rd.x[3 * idx + 1], rd.x[3 * idx + 2]};
  TrObs obs = traj_obs(rd, K, k, t);
  double H[6], g[3], cost;
  keypoint_linearise<LOSS>(cams, C, obs, X, rd.fs2, rd.inv_fs2, H, g, cost);
  const double ia2 = rd.ia2[k];
  const double c0 = sm_pen_diag(tt, rd.T), cp1 = sm_pen_off1(tt, rd.T), cm1 = sm_pen_off1(tt - 1, rd.T), cp2 = sm_pen_off2(tt, rd.T), cm2 = sm_pen_off2(tt - 2, rd.T);
#pragma unroll
  for (int e = 0; e < 3; ++e) {
    double s = c0 * X[e];
    if (cp1 != 0.0) s = fma(cp1, rd.x[3 * (idx + K) + e], s);
    if (cm1 != 0.0) s = fma(cm1, rd.x[3 * (idx - K) + e], s);
    if (cp2 != 0.0) s = fma(cp2, rd.x[3 * (idx + 2 * (size_t)K) + e], s);
    if (cm2 != 0.0) s = fma(cm2, rd.x[3 * (idx - 2 * (size_t)K) + e], s);
    rd.G[3 * idx + e] = fma(ia2, s, g[e]);
  }
#pragma unroll
  for (int e = 0; e < 6; ++e) rd.H[6 * idx + e] = H[e];
}

// ---- trial: one (frame, track): acc[a] += the frame's share of the objective at x + alpha_a d (a = 0: at x), acc[TR_DATA ..] as TR_SUMS says.
// The point and its two neighbours are formed per alpha as fma(alpha, d, x): exactly what traj_apply_lane stores for the accepted one
template <int LOSS>
MCBA_HD void traj_trial_lane(const KpCam* cams, int C, const TrData& rd, int K, int k, size_t t, double* acc) {
  const size_t idx = t * K + k;
  const bool pen = t >= 1 && t + 2 <= rd.T;
  double x[3][3], d[3][3];   // [neighbour: t - 1, t, t + 1][coordinate]
#pragma unroll
  for (int n = 0; n < 3; ++n) {
    const bool in = n == 1 || pen;
    const size_t j = in ? idx + (size_t)n * K - K : idx;
#pragma unroll
    for (int e = 0; e < 3; ++e) { x[n][e] = rd.x[3 * j + e]; d[n][e] = rd.d[3 * j + e]; }
  }
  double data[TR_TRIALS + 1];
#pragma unroll
  for (int a = 0; a <= TR_TRIALS; ++a) data[a] = 0.0;
  TrObs obs = traj_obs(rd, K, k, t);
  for (int c = 0; c < C; ++c) {
    double ou, ov, sw;
    if (kp_observe(obs, c, ou, ov, sw, 0)) {
#pragma unroll
      for (int a = 0; a <= TR_TRIALS; ++a) {
        const double al = traj_alpha(a);
        const double X[3] = {fma(al, d[1][0], x[1][0]), fma(al, d[1][1], x[1][1]), fma(al, d[1][2], x[1][2])};
        double u, v;
        project5<false>(cams[c], X, u, v);
        const double fu = sw * (ou - u), fv = sw * (ov - v);
        double rhu, rhv, gw, w2;
        loss_weights<LOSS>(fu, rd.fs2, rd.inv_fs2, rhu, gw, w2);
        loss_weights<LOSS>(fv, rd.fs2, rd.inv_fs2, rhv, gw, w2);
        data[a] += rhu + rhv;
      }
    }
  }
  const double hia2 = 0.5 * rd.ia2[k];
#pragma unroll
  for (int a = 0; a <= TR_TRIALS; ++a) {
    const double al = traj_alpha(a);
    double q = 0.0;
    if (pen) {
#pragma unroll
      for (int e = 0; e < 3; ++e) {
        const double s = fma(al, d[0][e], x[0][e]) - 2.0 * fma(al, d[1][e], x[1][e]) + fma(al, d[2][e], x[2][e]);
        q = fma(s, s, q);
      }
    }
    acc[a] += fma(hia2, q, data[a]);
    if (a == 0) { acc[TR_DATA] += data[0]; acc[TR_PEN] += q; }
  }
  acc[TR_DMAX] = fmax(acc[TR_DMAX], fmax(fabs(d[1][0]), fmax(fabs(d[1][1]), fabs(d[1][2]))));
  acc[TR_XMAX] = fmax(acc[TR_XMAX], fmax(fabs(x[1][0]), fmax(fabs(x[1][1]), fabs(x[1][2]))));
}

// ---- apply: one (frame, track): x <- x + alpha d for the track's accepted alpha (0: untouched, whatever d holds)
MCBA_HD void traj_apply_lane(const TrData& rd, size_t idx, double alpha) {
  if (alpha == 0.0) return;
#pragma unroll
  for (int e = 0; e < 3; ++e) rd.x[3 * idx + e] = fma(alpha, rd.d[3 * idx + e], rd.x[3 * idx + e]);
}

// ---- the status a track starts with, from its counts (traj_count_frame): one that is not TR_OK is never launched
MCBA_HD int traj_start_status(int n_usable, bool bad_start) { return n_usable < 2 ? TR_TOO_FEW_FRAMES : bad_start ? TR_BAD_START : TR_OK; }

// ---- the loop's decision for one track after iteration `it` (0-based) from its sums res (TR_SUMS): the accepted alpha -- the largest trial
// whose objective is not above the one at x, 0 when there is none -- the objective after it, and true = the track stops: nothing accepted (the
// minimiser to the cost's resolution), the last iteration, or a step alpha max |d| below xtol max |x|
MCBA_HD bool traj_decide(const double* res, double xtol, int it, int max_iterations, double& alpha, double& cost) {
  alpha = 0.0;
  cost = res[0];
  for (int a = 1; a <= TR_TRIALS; ++a)
    if (res[a] <= res[0]) {   // (NaN compares false)
      alpha = traj_alpha(a);
      cost = res[a];
      break;
    }
  return alpha == 0.0 || it + 1 >= max_iterations || alpha * res[TR_DMAX] < xtol * res[TR_XMAX];
}

}  // namespace mcba
