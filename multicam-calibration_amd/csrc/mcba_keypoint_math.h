// mcba_keypoint_math.h -- the per-lane arithmetic of csrc/mcba_keypoints.hip: projecting 3-D keypoints into calibrated
// cameras (reference geometry.py:277-325 `project_points`), the distance between a detection and that projection, and the per-point
// Levenberg-Marquardt refinement of a triangulated point on the robust reprojection cost.  One lane = one point; the kernels own the staging of
// the camera table in LDS and the loads.  Nothing here is new arithmetic where the library had it already: the k1, k2 projection is
// project_only (mcba_math.h), the five-coefficient forward model and its derivative distort5 (mcba_pnp_math.h), the robust weights loss_weights /
// lm_weight (mcba_math.h), the 3 x 3 solve chol3 / fwd3 / bwd3 (mcba_pnp_math.h).  The same text is compiled with g++ into
// tests/hostcheck/keypoints_hostcheck.cpp, where tests/test_hostcheck_keypoints.py runs the GPU tier's gates in the GPU-less tier.
#pragma once
#include "mcba_pnp_math.h"

namespace mcba {

// one camera of the table, 21 doubles: X_c = Rcf X + tcf (world -> camera), fx fy cx cy k1 k2, p1 p2 k3
struct KpCam {
  PairConst pc;
  Intr K;
  double p1, p2, k3;
};
static_assert(sizeof(KpCam) == 21 * sizeof(double), "the camera table is 21 doubles per camera");
constexpr int kKpMaxCams = 64;   // cameras of one launch (the table staged in LDS: 10.5 KB)

// cam12 = (fx fy cx cy k1 k2 | rotation vector | translation), the parameter layout of include/mcba.h; dist5 = (k1 k2 p1 p2 k3) replaces k1, k2, or NULL
MCBA_HD void make_kp_cam(const double* cam12, const double* dist5, KpCam& kc) {
  rot_only(cam12 + 6, kc.pc.Rcf);
  kc.pc.tcf[0] = cam12[9]; kc.pc.tcf[1] = cam12[10]; kc.pc.tcf[2] = cam12[11];
  kc.K.fx = cam12[0]; kc.K.fy = cam12[1]; kc.K.cx = cam12[2]; kc.K.cy = cam12[3];
  kc.K.k1 = dist5 ? dist5[0] : cam12[4];
  kc.K.k2 = dist5 ? dist5[1] : cam12[5];
  kc.p1 = dist5 ? dist5[2] : 0.0;
  kc.p2 = dist5 ? dist5[3] : 0.0;
  kc.k3 = dist5 ? dist5[4] : 0.0;
}

MCBA_HD void rigid_point(const PairConst& pc, const double X[3], double Xc[3]) {
  Xc[0] = fma(pc.Rcf[0], X[0], fma(pc.Rcf[1], X[1], fma(pc.Rcf[2], X[2], pc.tcf[0])));
  Xc[1] = fma(pc.Rcf[3], X[0], fma(pc.Rcf[4], X[1], fma(pc.Rcf[5], X[2], pc.tcf[1])));
  Xc[2] = fma(pc.Rcf[6], X[0], fma(pc.Rcf[7], X[1], fma(pc.Rcf[8], X[2], pc.tcf[2])));
}

// what the five-coefficient projection passes through on its way: the normalised point (x, y) = (Xc / Zc, Yc / Zc) and 1 / Zc, the distorted
// point (xd, yd) and, with LIN, the rows Pu, Pv of P = d(u, v)/dX_c (project5<false> leaves Pu, Pv unwritten: undefined there) -- for callers
// that differentiate with respect to the camera as well (mcba_tricov_math.h)
struct Proj5Parts {
  double x, y, xd, yd, Pu[3], Pv[3];
};

// five-coefficient projection of the world point X; LIN: also Ju, Jv = d(u, v)/dX (rows of P R, P = d(u, v)/dX_c); parts: the intermediates
template <bool LIN>
MCBA_HD void project5(const KpCam& kc, const double X[3], double& u, double& v, double* Ju = nullptr, double* Jv = nullptr, Proj5Parts* parts = nullptr) {
  double Xc[3];
  rigid_point(kc.pc, X, Xc);
  const double iz = fast_rcp(Xc[2]);
  const double x = Xc[0] * iz, y = Xc[1] * iz;
  const Cam9 cam{kc.K.fx, kc.K.fy, kc.K.cx, kc.K.cy, kc.K.k1, kc.K.k2, kc.p1, kc.p2, kc.k3};
  double xd, yd, axx, axy, ayy;
  distort5(cam, x, y, xd, yd, axx, axy, ayy);
  u = fma(cam.fx, xd, cam.cx);
  v = fma(cam.fy, yd, cam.cy);
  if (LIN) {
    const double P0[3] = {cam.fx * axx * iz, cam.fx * axy * iz, -cam.fx * (axx * x + axy * y) * iz};
    const double P1[3] = {cam.fy * axy * iz, cam.fy * ayy * iz, -cam.fy * (axy * x + ayy * y) * iz};
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      Ju[j] = fma(P0[0], kc.pc.Rcf[j], fma(P0[1], kc.pc.Rcf[3 + j], P0[2] * kc.pc.Rcf[6 + j]));
      Jv[j] = fma(P1[0], kc.pc.Rcf[j], fma(P1[1], kc.pc.Rcf[3 + j], P1[2] * kc.pc.Rcf[6 + j]));
    }
    if (parts) {
#pragma unroll
      for (int j = 0; j < 3; ++j) { parts->Pu[j] = P0[j]; parts->Pv[j] = P1[j]; }
    }
  }
  if (parts) { parts->x = x; parts->y = y; parts->xd = xd; parts->yd = yd; }
}

// |detection - projection| in pixels; NaN where the camera does not see the point (a NaN coordinate in the detection) or the point has a NaN
MCBA_HD double keypoint_error(const KpCam& kc, const double X[3], double ou, double ov) {
  double u, v;
  project5<false>(kc, X, u, v);
  const double du = ou - u, dv = ov - v;
  return sqrt(fma(du, du, dv * dv));
}

// ---- per-detection confidence weights.  A detection of weight w enters every cost as if it and fx, fy, cx, cy of its
// camera had been multiplied by sqrt(w): its residual and every derivative of its projection are scaled by sw = sqrt(w) before the loss sees
// them.  The rows of the Jacobians are not touched for that: the factor goes into what multiplies them -- the curvature weight of a scalar
// times w (two rows meet in every product), rho' f times sw once more (one row).  An observation functor of four arguments,
// observation(c, ou, ov, sw), hands out sw beside the detection; one of three arguments is the unweighted problem, and what is compiled for
// it has no trace of sw.  A detection is seen when neither coordinate is NaN and, weighted, sw > 0 (a zero or NaN weight: unseen, exactly
// like a NaN detection).
template <class Obs>
MCBA_HD auto kp_observe(Obs& observation, int c, double& ou, double& ov, double& sw, int) -> decltype(observation(c, ou, ov, sw), bool()) {
  observation(c, ou, ov, sw);
  return ou == ou && ov == ov && sw > 0.0;
}
template <class Obs>
MCBA_HD bool kp_observe(Obs& observation, int c, double& ou, double& ov, double& sw, long) {
  observation(c, ou, ov);
  sw = 1.0;
  return ou == ou && ov == ov;
}
template <class Obs>
struct KpWeighted {   // value: the functor takes the fourth argument.  (MCBA_HD throughout: a device-only functor is callable from these alone)
  template <class T>
  MCBA_HD static T& ref();
  template <class O>
  MCBA_HD static auto test(int) -> decltype(ref<O>()(0, ref<double>(), ref<double>(), ref<double>()), char());
  template <class O>
  MCBA_HD static long test(long);
  static constexpr bool value = sizeof(test<Obs>(0)) == sizeof(char);
};
// WEIGHTED: the pair of a detection's two scalars (residuals, weights, gradient factors) times s
template <bool WEIGHTED>
MCBA_HD void kp_scale_pair(double s, double& a, double& b) {
  if (WEIGHTED) { a *= s; b *= s; }
}

// The weight plane of the calls that take a pixel_std per camera (host only): what those kernels read as sw beside a detection is
// sqrt(w) / pixel_std[c], 0 for a zero or NaN weight (unseen).  One sub-box of the (C, T, K) array weights (NULL: every w = 1) -- frames
// t0 .. t0 + tc - 1, tracks k0 .. k0 + kc - 1 -- into out (C, tc, kc).  1 / pixel_std[c] is formed first and then multiplied
inline void kp_weight_box(const double* weights, const double* pixel_std, int C, size_t T, size_t K, size_t t0, size_t tc, size_t k0, size_t kc, double* out) {
  for (int c = 0; c < C; ++c) {
    const double ips = 1.0 / pixel_std[c];
    for (size_t t = 0; t < tc; ++t)
      for (size_t k = 0; k < kc; ++k) {
        const double w = weights ? weights[((size_t)c * T + t0 + t) * K + k0 + k] : 1.0;
        out[((size_t)c * tc + t) * kc + k] = w > 0.0 ? sqrt(w) * ips : 0.0;
      }
  }
}

// ---- refinement of one point: minimise 0.5 sum rho(f^2) over X, f = the 2 (cameras that see it) scalars detection - projection (pixels), rho and
// f_scale scipy's (loss_weights).  observation(c, ou, ov) hands out the point's detection in camera c (with a fourth argument: and sqrt(w)).
// One linearisation at X: packed Gauss-Newton matrix H (00 01 02 11 12 22) with the curvature weights of the bundle-adjustment tick
// (lm_weight: Triggs' weight floored at MCBA_CURV_FLOOR_TRIGGS rho'), gradient g of the cost, the robust cost.  Returns the number of views.
template <int LOSS, class Obs>
MCBA_HD int keypoint_linearise(const KpCam* cams, int C, Obs& observation, const double X[3], double fs2, double inv_fs2, double* H, double* g, double& cost) {
#pragma unroll
  for (int i = 0; i < 6; ++i) H[i] = 0.0;
  g[0] = g[1] = g[2] = 0.0;
  cost = 0.0;
  int views = 0;
  for (int c = 0; c < C; ++c) {
    double ou, ov, sw;
    if (kp_observe(observation, c, ou, ov, sw, 0)) {
      ++views;
      double u, v, Ju[3], Jv[3];
      project5<true>(cams[c], X, u, v, Ju, Jv);
      double fu = ou - u, fv = ov - v;
      kp_scale_pair<KpWeighted<Obs>::value>(sw, fu, fv);
      double rhu, gwu, w2u, rhv, gwv, w2v;
      loss_weights<LOSS>(fu, fs2, inv_fs2, rhu, gwu, w2u);
      loss_weights<LOSS>(fv, fs2, inv_fs2, rhv, gwv, w2v);
      cost += rhu + rhv;
      double wu = lm_weight(gwu, w2u, MCBA_CURV_FLOOR_TRIGGS), wv = lm_weight(gwv, w2v, MCBA_CURV_FLOOR_TRIGGS);
      double gu = gwu * fu, gv = gwv * fv;   // (df/dX = -J)
      kp_scale_pair<KpWeighted<Obs>::value>(sw * sw, wu, wv);
      kp_scale_pair<KpWeighted<Obs>::value>(sw, gu, gv);
      int k = 0;
#pragma unroll
      for (int i = 0; i < 3; ++i) {
        const double a = wu * Ju[i], b = wv * Jv[i];
#pragma unroll
        for (int j = i; j < 3; ++j, ++k) H[k] = fma(a, Ju[j], fma(b, Jv[j], H[k]));
        g[i] -= fma(gu, Ju[i], gv * Jv[i]);
      }
    }
  }
  return views;
}

// status of a refined point
constexpr int KP_CONVERGED = 1, KP_ITERATION_LIMIT = 0, KP_TOO_FEW_VIEWS = -1;
// convergence tests (scipy's three, at tight tolerances: the result is compared with an optimum known to 5e-7 mm):
//   step      max |dX| <= KP_XTOL (1 + max |X|)       (1e-9 mm at a point a metre from the origin)
//   cost      an accepted step gained <= KP_FTOL cost  (at the cost's own rounding level: the decrease left cannot be told from round-off)
//   gradient  max |g| <= KP_GTOL
constexpr double KP_XTOL = 1e-12, KP_FTOL = 1e-15, KP_GTOL = 1e-12;

// Levenberg-Marquardt with Marquardt's damping lam diag(H): a trial point is accepted when its robust cost is not larger (so the result is never
// worse than the start: if nothing is accepted the start comes back), the damping falls tenfold on acceptance and rises tenfold on rejection.
// A lane that is done leaves the loop; on the GPU the wavefront leaves it when its last lane has (the loop's exit is the hardware's vote).
// Out: Xout (NaN for fewer than two views or a NaN start), info = (cost, cost at the start, iterations, status).
template <int LOSS, class Obs>
MCBA_HD void refine_point(const KpCam* cams, int C, Obs& observation, const double X0[3], double f_scale, int max_iterations, double Xout[3], double info[4]) {
  const double fs2 = f_scale * f_scale, inv_fs2 = 1.0 / fs2;
  double X[3] = {X0[0], X0[1], X0[2]}, H[6], g[3], cost;
  const int views = keypoint_linearise<LOSS>(cams, C, observation, X, fs2, inv_fs2, H, g, cost);
  const bool usable = views >= 2 && X[0] == X[0] && X[1] == X[1] && X[2] == X[2];
  const double cost0 = cost;
  double lam = 1e-4;
  int it = 0, status = KP_ITERATION_LIMIT;
  bool done = !usable;
  if (!done && fmax(fabs(g[0]), fmax(fabs(g[1]), fabs(g[2]))) <= KP_GTOL) { done = true; status = KP_CONVERGED; }
  while (!done && it < max_iterations) {
    ++it;
    double A[6] = {H[0], H[1], H[2], H[3], H[4], H[5]}, L[6], b[3] = {-g[0], -g[1], -g[2]}, z[3], d[3];
    A[0] = fma(lam, H[0], H[0]); A[3] = fma(lam, H[3], H[3]); A[5] = fma(lam, H[5], H[5]);
    chol3(A, 0.0, L);
    fwd3(L, b, z);
    bwd3(L, z, d);
    const double Xt[3] = {X[0] + d[0], X[1] + d[1], X[2] + d[2]};
    double Ht[6], gt[3], ct;
    keypoint_linearise<LOSS>(cams, C, observation, Xt, fs2, inv_fs2, Ht, gt, ct);
    const double dmax = fmax(fabs(d[0]), fmax(fabs(d[1]), fabs(d[2]))), xmax = fmax(fabs(X[0]), fmax(fabs(X[1]), fabs(X[2])));
    const bool small_step = dmax <= KP_XTOL * (1.0 + xmax);
    if (ct <= cost) {   // (NaN compares false)
      const double gain = cost - ct;
#pragma unroll
      for (int i = 0; i < 6; ++i) H[i] = Ht[i];
#pragma unroll
      for (int i = 0; i < 3; ++i) { X[i] = Xt[i]; g[i] = gt[i]; }
      cost = ct;
      lam = fmax(0.1 * lam, 1e-12);
      const double gmax = fmax(fabs(g[0]), fmax(fabs(g[1]), fabs(g[2])));
      if (small_step || gain <= KP_FTOL * cost || gmax <= KP_GTOL) { done = true; status = KP_CONVERGED; }
    } else {
      lam *= 10.0;
      if (small_step || !(lam < 1e12)) { done = true; status = KP_CONVERGED; }   // no point nearby is better: the minimiser to the cost's resolution
    }
  }
  const double nan = __builtin_nan("");
#pragma unroll
  for (int i = 0; i < 3; ++i) Xout[i] = usable ? X[i] : nan;
  info[0] = usable ? cost : nan;
  info[1] = usable ? cost0 : nan;
  info[2] = (double)it;
  info[3] = (double)(usable ? status : KP_TOO_FEW_VIEWS);
}

}  // namespace mcba
