// mcba_consensus_math.h -- the per-lane arithmetic of csrc/mcba_consensus.hip: consensus triangulation of one point.
// Every camera pair that sees the point gives a hypothesis (the two-view DLT point of mcba_geom_math.h from the undistorted detections); a
// hypothesis is scored against the RAW detections of every camera that sees the point with the truncated (MSAC) cost of the forward
// five-coefficient reprojection error; the cheapest hypothesis names the inlier cameras, and the point is refitted on those alone by the
// Levenberg-Marquardt of mcba_keypoint_math.h.  Nothing here is new arithmetic where the library had it: undistort_px, triangulate_pair,
// keypoint_error, rigid_point, refine_point.  The enumeration is exhaustive and deterministic; an exact tie goes to the lowest pair index.
// The same text is compiled with g++ into tests/hostcheck/consensus_hostcheck.cpp (tests/test_hostcheck_consensus.py, also under ASan + UBSan).
#pragma once
#include "mcba_geom_math.h"
#include "mcba_keypoint_math.h"

namespace mcba {

constexpr int KP_NO_CONSENSUS = -2;     // status: the winning hypothesis has fewer than min_views inliers (KP_TOO_FEW_VIEWS: no hypothesis at all)
constexpr int kConsNone = 0x7fffffff;   // pair index of "no hypothesis yet": loses the (cost, k) comparison to every real one

// P = K [R | t], row-major 3 x 4, of one entry of the camera table (what triangulate_pair takes)
MCBA_HD void cons_projection(const KpCam& kc, double* P) {
  const double* R = kc.pc.Rcf;
  const double* t = kc.pc.tcf;
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    P[j] = fma(kc.K.fx, R[j], kc.K.cx * R[6 + j]);
    P[4 + j] = fma(kc.K.fy, R[3 + j], kc.K.cy * R[6 + j]);
    P[8 + j] = R[6 + j];
  }
  P[3] = fma(kc.K.fx, t[0], kc.K.cx * t[2]);
  P[7] = fma(kc.K.fy, t[1], kc.K.cy * t[2]);
  P[11] = t[2];
}

// pair k -> (i, j), i < j, in the order (0,1), (0,2), ..., (0,C-1), (1,2), ... (k_triangulate_wave's)
MCBA_HD void cons_pair(int k, int C, int& i, int& j) {
  i = 0;
  while (k >= C - 1 - i) { k -= C - 1 - i; ++i; }
  j = i + 1 + k;
}

// hypothesis of the pair (i, j): the DLT point of the two detections, undistorted with und_iters rounds.  false: void (a camera of the pair does
// not see the point, or triangulate_pair does not keep the result: non-finite, a point at infinity).  proj: C x 12, cons_projection per camera.
template <class Obs>
MCBA_HD bool consensus_hypothesis(const KpCam* cams, const double* proj, int i, int j, Obs& observation, int und_iters, double X[3]) {
  double ui, vi, uj, vj;
  observation(i, ui, vi);
  observation(j, uj, vj);
  if (!(ui == ui && vi == vi && uj == uj && vj == vj)) return false;
  const KpCam &a = cams[i], &b = cams[j];
  const double ka[5] = {a.K.k1, a.K.k2, a.p1, a.p2, a.k3}, kb[5] = {b.K.k1, b.K.k2, b.p1, b.p2, b.k3};
  double xi, yi, xj, yj;
  undistort_px(ui, vi, a.K.fx, a.K.fy, a.K.cx, a.K.cy, ka, und_iters, xi, yi);
  undistort_px(uj, vj, b.K.fx, b.K.fy, b.K.cx, b.K.cy, kb, und_iters, xj, yj);
  return triangulate_pair(xi, yi, proj + 12 * i, xj, yj, proj + 12 * j, true, X[0], X[1], X[2]);
}

// truncated cost of the hypothesis X over the cameras that see the point: e^2 for an inlier (in front of the camera, e <= threshold; a NaN
// compares false), threshold^2 otherwise.  mask: bit c = camera c is an inlier.
template <class Obs>
MCBA_HD double consensus_score(const KpCam* cams, int C, Obs& observation, const double X[3], double threshold, unsigned long long& mask) {
  const double t2 = threshold * threshold;
  double cost = 0.0;
  mask = 0ull;
  for (int c = 0; c < C; ++c) {
    double ou, ov;
    observation(c, ou, ov);
    if (ou == ou && ov == ov) {
      const double e = keypoint_error(cams[c], X, ou, ov);
      double Xc[3];
      rigid_point(cams[c].pc, X, Xc);
      const bool inlier = Xc[2] > 0.0 && e <= threshold;
      cost = inlier ? fma(e, e, cost) : cost + t2;
      mask |= inlier ? 1ull << c : 0ull;
    }
  }
  return cost;
}

// the running best: lowest (cost, k), compared lexicographically
struct ConsBest {
  double cost;
  int k;
  double X[3];
  unsigned long long mask;
};
MCBA_HD void cons_best_init(ConsBest& b) {
  b.cost = __builtin_inf();
  b.k = kConsNone;
  b.X[0] = b.X[1] = b.X[2] = __builtin_nan("");
  b.mask = 0ull;
}
MCBA_HD bool cons_before(double cost_a, int k_a, double cost_b, int k_b) { return cost_a < cost_b || (cost_a == cost_b && k_a < k_b); }
MCBA_HD void cons_offer(ConsBest& b, double cost, int k, const double X[3], unsigned long long mask) {
  const bool take = cons_before(cost, k, b.cost, b.k);
  b.cost = take ? cost : b.cost;
  b.k = take ? k : b.k;
  b.X[0] = take ? X[0] : b.X[0]; b.X[1] = take ? X[1] : b.X[1]; b.X[2] = take ? X[2] : b.X[2];
  b.mask = take ? mask : b.mask;
}

// the pairs k0, k0 + stride, ... of one point into `best` (lane = point: k0 = 0, stride = 1; wavefront = point: k0 = lane, stride = 64)
template <class Obs>
MCBA_HD void consensus_search(const KpCam* cams, const double* proj, int C, Obs& observation, double threshold, int und_iters, int k0, int stride, ConsBest& best) {
  const int NP = C * (C - 1) / 2;
  int i = 0, rem = k0;
  for (int k = k0; k < NP; k += stride, rem += stride) {
    while (rem >= C - 1 - i) { rem -= C - 1 - i; ++i; }
    double X[3];
    if (consensus_hypothesis(cams, proj, i, i + 1 + rem, observation, und_iters, X)) {
      unsigned long long mask;
      const double cost = consensus_score(cams, C, observation, X, threshold, mask);
      cons_offer(best, cost, k, X, mask);
    }
  }
}

// outcome of the search: the refit on the inlier views from the winner's X (refine_point sees NaN for every other camera), or no point.
// info = (inliers, pair i, pair j, hypothesis cost, refit cost, refit cost at the start, iterations, status); the mask is not re-voted.
template <int LOSS, class Obs>
MCBA_HD void consensus_finish(const KpCam* cams, int C, Obs& observation, const ConsBest& best, int min_views, double f_scale, int max_iterations, double Xout[3], double info[8]) {
  const double nan = __builtin_nan("");
  const bool any = best.k != kConsNone;
  const int n = __builtin_popcountll(best.mask);
  int pi = -1, pj = -1;
  if (any) cons_pair(best.k, C, pi, pj);
  info[0] = (double)n; info[1] = (double)pi; info[2] = (double)pj; info[3] = any ? best.cost : nan;
  if (any && n >= min_views) {
    const unsigned long long mask = best.mask;
    auto inlier_observation = [&](int c, double& ou, double& ov) {
      ou = ov = nan;
      if ((mask >> c) & 1ull) observation(c, ou, ov);
    };
    refine_point<LOSS>(cams, C, inlier_observation, best.X, f_scale, max_iterations, Xout, info + 4);
  } else {
    Xout[0] = Xout[1] = Xout[2] = nan;
    info[4] = info[5] = nan;
    info[6] = 0.0;
    info[7] = (double)(any ? KP_NO_CONSENSUS : KP_TOO_FEW_VIEWS);
  }
}

// the whole point, as one lane runs it
template <int LOSS, class Obs>
MCBA_HD void consensus_point(const KpCam* cams, const double* proj, int C, Obs& observation, double threshold, int min_views, int und_iters, double f_scale, int max_iterations, double Xout[3],
                             unsigned long long& mask, double info[8]) {
  ConsBest best;
  cons_best_init(best);
  consensus_search(cams, proj, C, observation, threshold, und_iters, 0, 1, best);
  consensus_finish<LOSS>(cams, C, observation, best, min_views, f_scale, max_iterations, Xout, info);
  mask = best.mask;
}

}  // namespace mcba
