// mcba_kpba_math.h -- the arithmetic of csrc/mcba_kpba.hip and csrc/mcba_kpba_api.hip: free-point bundle adjustment of the
// camera extrinsics on raw keypoint detections.  Unknowns: the rotation vector and translation of every camera (intrinsics fixed) and every point.
//   per point p over the cameras that see it   H_p = sum A^T w A,  g_p = -sum A^T rho' f,  W_cp = B_c^T w A_c (6 x 3)
//   per camera c                               U_c = sum_p B^T w B,  g_c = -sum_p B^T rho' f
//   reduced system                             S = U + lam diag(U) - sum_p Y_p Y_p^T,   rhs = -g_c + sum_p Y_p z_p
//                                              Y_cp = W_cp D L^-T,  z_p = L^-1 D g_p,  L L^T = D (H_p + lam diag H_p) D,  D = diag(H_p)^-1/2
//   back-substitution                          dX_p = -D L^-T L^-1 D (g_p + sum_c W_cp^T dtheta_c)
// f = detection - projection, A = d(u, v)/dX (project5<true>), B = columns 6 .. 11 of tricov_cam_rows (rotation vector, translation), w the
// curvature weight of the bundle-adjustment tick (lm_weight, Triggs floored), rho' in the gradient.  What a lane (or a (camera, point) item) does
// is here, and so is everything the host does per evaluation: the Jacobi-scaled dense Cholesky of the reduced system, the Levenberg-Marquardt loop
// (kpba_lm, written against a back end: the kernels in mcba_kpba_api.hip, plain loops in tests/hostcheck/kpba_hostcheck.cpp), the closing rescale.
#pragma once
#include <cstddef>
#include <vector>

#include "mcba_tricov_math.h"

namespace mcba {

constexpr int KB_USED = 1, KB_TOO_FEW_VIEWS = -1, KB_ZERO_DIAGONAL = -2;   // status of a point
constexpr int kKbMaxCams = 24;                                             // 6 C <= 144: nine 16-row tiles
constexpr int kKbAcc = 33;                                                 // per camera: U_c packed lower (21) | g_c (6) | sum_p Y_cp z_p (6)
constexpr double KB_LAMBDA0 = 1e-4, KB_LAMBDA_MIN = 1e-12, KB_LAMBDA_MAX = 1e12;

// ---- one point at X: packed H (00 01 02 11 12 22), gradient g, robust cost, views; with dtheta (6 per camera, or NULL) also q = sum_c W_cp^T dtheta_c.
// An observation functor of four arguments also hands out sqrt(w) of the detection (mcba_keypoint_math.h): f, A and B as if times it, unseen unless it is > 0.
struct KbPoint {
  double H[6], g[3], q[3], cost;
  int views;
};

template <int LOSS, class Obs>
MCBA_HD void kpba_point(const TcCam* cams, int C, Obs& observation, const double X[3], double fs2, double inv_fs2, const double* dtheta, KbPoint& pt) {
#pragma unroll
  for (int i = 0; i < 6; ++i) pt.H[i] = 0.0;
#pragma unroll
  for (int i = 0; i < 3; ++i) pt.g[i] = pt.q[i] = 0.0;
  pt.cost = 0.0;
  pt.views = 0;
  for (int c = 0; c < C; ++c) {
    double ou, ov, sw;
    if (!kp_observe(observation, c, ou, ov, sw, 0)) continue;
    ++pt.views;
    double u, v, Ju[3], Jv[3], Bu[12], Bv[12];
    if (dtheta) tricov_cam_rows(cams[c], X, u, v, Ju, Jv, Bu, Bv);
    else project5<true>(cams[c].kc, X, u, v, Ju, Jv);
    double fu = ou - u, fv = ov - v;
    kp_scale_pair<KpWeighted<Obs>::value>(sw, fu, fv);
    double rhu, gwu, w2u, rhv, gwv, w2v;
    loss_weights<LOSS>(fu, fs2, inv_fs2, rhu, gwu, w2u);
    loss_weights<LOSS>(fv, fs2, inv_fs2, rhv, gwv, w2v);
    pt.cost += rhu + rhv;
    double wu = lm_weight(gwu, w2u, MCBA_CURV_FLOOR_TRIGGS), wv = lm_weight(gwv, w2v, MCBA_CURV_FLOOR_TRIGGS);
    double gu = gwu * fu, gv = gwv * fv;   // (df/dX = -A)
    kp_scale_pair<KpWeighted<Obs>::value>(sw * sw, wu, wv);
    kp_scale_pair<KpWeighted<Obs>::value>(sw, gu, gv);
    double bu = 0.0, bv = 0.0;                    // B_c dtheta_c, per scalar
    if (dtheta) {
#pragma unroll
      for (int i = 0; i < 6; ++i) {
        bu = fma(Bu[6 + i], dtheta[6 * c + i], bu);
        bv = fma(Bv[6 + i], dtheta[6 * c + i], bv);
      }
      bu *= wu; bv *= wv;
    }
    int k = 0;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      const double a = wu * Ju[i], b = wv * Jv[i];
#pragma unroll
      for (int j = i; j < 3; ++j, ++k) pt.H[k] = fma(a, Ju[j], fma(b, Jv[j], pt.H[k]));
      pt.g[i] -= fma(gu, Ju[i], gv * Jv[i]);
      pt.q[i] = fma(bu, Ju[i], fma(bv, Jv[i], pt.q[i]));
    }
  }
}

MCBA_HD int kpba_status(int views, const double X[3], const double* H) {
  if (!(views >= 2 && X[0] == X[0] && X[1] == X[1] && X[2] == X[2])) return KB_TOO_FEW_VIEWS;
  return (H[0] > 0.0 && H[3] > 0.0 && H[5] > 0.0) ? KB_USED : KB_ZERO_DIAGONAL;
}

// ---- the Cholesky factor of the damped, Jacobi-scaled block.  false: a diagonal entry that is not positive (the point then contributes nothing)
struct KbFactor {
  double L[6], d[3];
};
MCBA_HD bool kpba_factor(const double* H, double lam, KbFactor& f) {
  if (!(H[0] > 0.0 && H[3] > 0.0 && H[5] > 0.0)) {
#pragma unroll
    for (int i = 0; i < 6; ++i) f.L[i] = 0.0;
    f.d[0] = f.d[1] = f.d[2] = 0.0;
    return false;
  }
  f.d[0] = 1.0 / sqrt(H[0]); f.d[1] = 1.0 / sqrt(H[3]); f.d[2] = 1.0 / sqrt(H[5]);
  const double A[6] = {1.0 + lam, H[1] * f.d[0] * f.d[1], H[2] * f.d[0] * f.d[2], 1.0 + lam, H[4] * f.d[1] * f.d[2], 1.0 + lam};
  chol3(A, 0.0, f.L);
  return true;
}
MCBA_HD void kpba_fwd(const KbFactor& f, const double* v, double* z) {   // z = L^-1 D v
  const double s[3] = {f.d[0] * v[0], f.d[1] * v[1], f.d[2] * v[2]};
  fwd3(f.L, s, z);
}
MCBA_HD void kpba_bwd(const KbFactor& f, const double* z, double* x) {   // x = D L^-T z
  double y[3];
  bwd3(f.L, z, y);
  x[0] = f.d[0] * y[0]; x[1] = f.d[1] * y[1]; x[2] = f.d[2] * y[2];
}
// dX = -(H + lam diag H)^-1 (g + q)
MCBA_HD void kpba_point_step(const KbFactor& f, const double* g, const double* q, double* dX) {
  const double b[3] = {-(g[0] + q[0]), -(g[1] + q[1]), -(g[2] + q[2])};
  double z[3];
  kpba_fwd(f, b, z);
  kpba_bwd(f, z, dX);
}

// ---- one (camera, point) item, the camera seeing the point: the rows Y_cp (6 x 3, row-major; a row whose bit in `held` is set is zero) and the
// camera's sums acc[kKbAcc] = U_c packed lower (i, j <= i) | g_c | Y_cp z_p
// WEIGHTED: the detection has the weight sw^2 > 0 (the residual times sw; the curvature weights times sw^2, rho' f once more times sw)
template <int LOSS, bool WEIGHTED>
MCBA_HD void kpba_item_w(const TcCam& tc, const double X[3], double ou, double ov, double sw, double fs2, double inv_fs2, const KbFactor& f, const double* zp, int held, double* Y, double* acc) {
  double u, v, Ju[3], Jv[3], Bu[12], Bv[12];
  tricov_cam_rows(tc, X, u, v, Ju, Jv, Bu, Bv);
  double fu = ou - u, fv = ov - v;
  kp_scale_pair<WEIGHTED>(sw, fu, fv);
  double rh, gwu, w2u, gwv, w2v;
  loss_weights<LOSS>(fu, fs2, inv_fs2, rh, gwu, w2u);
  loss_weights<LOSS>(fv, fs2, inv_fs2, rh, gwv, w2v);
  double wu = lm_weight(gwu, w2u, MCBA_CURV_FLOOR_TRIGGS), wv = lm_weight(gwv, w2v, MCBA_CURV_FLOOR_TRIGGS);
  double gu = gwu * fu, gv = gwv * fv;
  kp_scale_pair<WEIGHTED>(sw * sw, wu, wv);
  kp_scale_pair<WEIGHTED>(sw, gu, gv);
  int k = 0;
#pragma unroll
  for (int i = 0; i < 6; ++i) {
    const double a = wu * Bu[6 + i], b = wv * Bv[6 + i];
#pragma unroll
    for (int j = 0; j <= i; ++j, ++k) acc[k] = fma(a, Bu[6 + j], b * Bv[6 + j]);
    acc[21 + i] = -fma(gu, Bu[6 + i], gv * Bv[6 + i]);
    const double w[3] = {fma(a, Ju[0], b * Jv[0]), fma(a, Ju[1], b * Jv[1]), fma(a, Ju[2], b * Jv[2])};   // row i of W_cp
    double y[3];
    kpba_fwd(f, w, y);
    const bool off = (held >> i) & 1;
#pragma unroll
    for (int j = 0; j < 3; ++j) Y[3 * i + j] = off ? 0.0 : y[j];
    acc[27 + i] = off ? 0.0 : fma(y[0], zp[0], fma(y[1], zp[1], y[2] * zp[2]));
  }
}
template <int LOSS>
MCBA_HD void kpba_item(const TcCam& tc, const double X[3], double ou, double ov, double fs2, double inv_fs2, const KbFactor& f, const double* zp, int held, double* Y, double* acc) {
  kpba_item_w<LOSS, false>(tc, X, ou, ov, 1.0, fs2, inv_fs2, f, zp, held, Y, acc);
}
template <int LOSS>
MCBA_HD void kpba_item(const TcCam& tc, const double X[3], double ou, double ov, double sw, double fs2, double inv_fs2, const KbFactor& f, const double* zp, int held, double* Y, double* acc) {
  kpba_item_w<LOSS, true>(tc, X, ou, ov, sw, fs2, inv_fs2, f, zp, held, Y, acc);
}

// ================================================================ host side
// ---- A x = b for the symmetric positive definite n x n A (row-major, overwritten) through the Cholesky factor of its Jacobi-scaled form.
// false: a diagonal entry or a pivot that is not positive.
inline bool kpba_dense_solve(int n, double* A, const double* b, double* x) {
  std::vector<double> s((size_t)n);
  for (int i = 0; i < n; ++i) {
    if (!(A[(size_t)i * n + i] > 0.0)) return false;
    s[i] = 1.0 / sqrt(A[(size_t)i * n + i]);
  }
  for (int i = 0; i < n; ++i)
    for (int j = 0; j <= i; ++j) A[(size_t)i * n + j] *= s[i] * s[j];
  for (int j = 0; j < n; ++j) {
    double d = A[(size_t)j * n + j];
    for (int k = 0; k < j; ++k) d -= A[(size_t)j * n + k] * A[(size_t)j * n + k];
    if (!(d > 1e-14)) return false;   // (the scaled diagonal is 1: the pivot is what the elimination left of it)
    const double l = sqrt(d);
    A[(size_t)j * n + j] = l;
    for (int i = j + 1; i < n; ++i) {
      double v = A[(size_t)i * n + j];
      for (int k = 0; k < j; ++k) v -= A[(size_t)i * n + k] * A[(size_t)j * n + k];
      A[(size_t)i * n + j] = v / l;
    }
  }
  for (int i = 0; i < n; ++i) {
    double v = s[i] * b[i];
    for (int k = 0; k < i; ++k) v -= A[(size_t)i * n + k] * x[k];
    x[i] = v / A[(size_t)i * n + i];
  }
  for (int i = n - 1; i >= 0; --i) {
    double v = x[i];
    for (int k = i + 1; k < n; ++k) v -= A[(size_t)k * n + i] * x[k];
    x[i] = v / A[(size_t)i * n + i];
  }
  for (int i = 0; i < n; ++i) x[i] *= s[i];
  return true;
}

// ---- what one linearisation hands to the host: YY = sum_p Y_p Y_p^T (NP x NP, NP = 6 C rounded up to 16), acc (C x kKbAcc), the robust cost,
// the present scalars and max |g_p| of the used points
struct KbSystem {
  int C = 0, NP = 0;
  std::vector<double> YY, acc;
  double cost = 0.0, count = 0.0, gmax = 0.0;
  void shape(int C_) {
    C = C_; NP = (6 * C + 15) / 16 * 16;
    YY.assign((size_t)NP * NP, 0.0);
    acc.assign((size_t)C * kKbAcc, 0.0);
  }
  double U(int c, int i, int j) const { return acc[(size_t)c * kKbAcc + (i >= j ? i * (i + 1) / 2 + j : j * (j + 1) / 2 + i)]; }
};

inline void kpba_centre(const double* ext6, double* c) {   // c = -R^T t
  double R[9];
  rot_only(ext6, R);
  for (int j = 0; j < 3; ++j) c[j] = -(R[j] * ext6[3] + R[3 + j] * ext6[4] + R[6 + j] * ext6[5]);
}
inline void kpba_set_centre(double* ext6, const double* c) {   // t = -R c
  double R[9];
  rot_only(ext6, R);
  for (int i = 0; i < 3; ++i) ext6[3 + i] = -(R[3 * i] * c[0] + R[3 * i + 1] * c[1] + R[3 * i + 2] * c[2]);
}
inline double kpba_baseline(const double* ext, int gauge, int scale_cam) {
  double c0[3], cj[3];
  kpba_centre(ext + 6 * gauge, c0);
  kpba_centre(ext + 6 * scale_cam, cj);
  return sqrt((cj[0] - c0[0]) * (cj[0] - c0[0]) + (cj[1] - c0[1]) * (cj[1] - c0[1]) + (cj[2] - c0[2]) * (cj[2] - c0[2]));
}
// The closing step: camera centres and points about the gauge camera's centre by s = baseline / |c_j - c_0|; every projection is unchanged.
// A camera held whole (the gauge camera; one that no used point sees and so has no projection) keeps its extrinsics as they are.
inline double kpba_rescale(int C, const int* held, double* ext, size_t P, double* pts, int gauge, int scale_cam, double baseline) {
  const double now = kpba_baseline(ext, gauge, scale_cam);
  const double s = now > 0.0 ? baseline / now : 1.0;
  double c0[3];
  kpba_centre(ext + 6 * gauge, c0);
  for (int c = 0; c < C; ++c) {
    if (c == gauge || held[c] == 63) continue;
    double cc[3];
    kpba_centre(ext + 6 * c, cc);
    for (int j = 0; j < 3; ++j) cc[j] = c0[j] + s * (cc[j] - c0[j]);
    kpba_set_centre(ext + 6 * c, cc);
  }
  for (size_t p = 0; p < P; ++p)
    for (int j = 0; j < 3; ++j) pts[3 * p + j] = c0[j] + s * (pts[3 * p + j] - c0[j]);   // (NaN rows stay NaN)
  return s;
}

struct KbOptions {
  double ftol, xtol, gtol;
  int max_nfev;
};
struct KbResult {
  double cost = 0.0, cost0 = 0.0, optimality = 0.0;
  int nfev = 0, njev = 0, status = 0, nhist = 0;
};

// ---- Levenberg-Marquardt with Marquardt's damping lam diag(.) on cameras and points alike.  A trial is accepted when the robust cost does not
// rise (the result is never worse than the start); the damping falls tenfold on acceptance, rises tenfold on rejection, and the system is then
// rebuilt at the same point.  Termination: scipy's status values -- 1 gtol (inf-norm of the gradient over the free parameters), 2 ftol (an
// accepted step gained less than ftol cost), 3 xtol (|step| < xtol (xtol + |x|), or the damping ran out of range), 0 max_nfev.
// The back end:  int reduce(const double* ext, double lam, KbSystem&)         linearise at (ext, current points)
//                int step(const double* ext_trial, const double* dtheta, double lam, double out[3])
//                                                trial points into the second buffer; out = trial cost, sum dX^2, sum X^2 (used points)
//                void accept()                   the trial points become the current ones
// A non-zero return of the back end ends the loop at once and is returned.  held[c]: bit i set = scalar i of camera c is not free.
// hist: (cap, 3) rows of (cost, damping, accepted) per evaluation.
template <class BackEnd>
int kpba_lm(BackEnd& be, int C, const int* held, double* ext, const KbOptions& opt, KbResult& res, double* hist, int hist_cap) {
  std::vector<int> idx;
  for (int c = 0; c < C; ++c)
    for (int i = 0; i < 6; ++i)
      if (!((held[c] >> i) & 1)) idx.push_back(6 * c + i);
  const int n = (int)idx.size();
  KbSystem sys;
  sys.shape(C);
  std::vector<double> A((size_t)n * n), b((size_t)n), x((size_t)n), dth((size_t)6 * C), trial((size_t)6 * C);
  auto record = [&](double cost, double lam, bool accepted) {
    if (res.nhist < hist_cap) { hist[3 * res.nhist] = cost; hist[3 * res.nhist + 1] = lam; hist[3 * res.nhist + 2] = accepted ? 1.0 : 0.0; }
    ++res.nhist;
  };
  auto gradient = [&]() {
    double g = sys.gmax;
    for (int a = 0; a < n; ++a) g = fmax(g, fabs(sys.acc[(size_t)(idx[a] / 6) * kKbAcc + 21 + idx[a] % 6]));
    return g;
  };
  double lam = KB_LAMBDA0;
  if (int rc = be.reduce(ext, lam, sys)) return rc;
  double cost = sys.cost;
  res.cost0 = cost;
  res.nfev = res.njev = 1;
  record(cost, lam, true);
  res.optimality = gradient();
  int status = res.optimality <= opt.gtol ? 1 : -1;
  while (status == -1) {
    if (res.nfev >= opt.max_nfev) { status = 0; break; }
    for (int a = 0; a < n; ++a) {
      const int ca = idx[a] / 6, ia = idx[a] % 6;
      for (int k = 0; k < n; ++k) {
        const int ck = idx[k] / 6, ik = idx[k] % 6;
        double v = ca == ck ? sys.U(ca, ia, ik) : 0.0;
        if (a == k) v = fma(lam, v, v);
        A[(size_t)a * n + k] = v - sys.YY[(size_t)idx[a] * sys.NP + idx[k]];
      }
      b[a] = sys.acc[(size_t)ca * kKbAcc + 27 + ia] - sys.acc[(size_t)ca * kKbAcc + 21 + ia];
    }
    if (!kpba_dense_solve(n, A.data(), b.data(), x.data())) {   // not positive definite at this damping: more of it
      lam *= 10.0;
      if (!(lam < KB_LAMBDA_MAX)) { status = 3; break; }
      if (int rc = be.reduce(ext, lam, sys)) return rc;
      continue;
    }
    double step2 = 0.0, x2 = 0.0;
    for (int k = 0; k < 6 * C; ++k) { dth[k] = 0.0; trial[k] = ext[k]; }
    for (int a = 0; a < n; ++a) {
      dth[idx[a]] = x[a];
      trial[idx[a]] = ext[idx[a]] + x[a];
      step2 += x[a] * x[a];
      x2 += ext[idx[a]] * ext[idx[a]];
    }
    double out[3];
    if (int rc = be.step(trial.data(), dth.data(), lam, out)) return rc;
    ++res.nfev;
    const double xn = sqrt(x2 + out[2]);
    const bool small = sqrt(step2 + out[1]) < opt.xtol * (opt.xtol + xn);
    if (out[0] <= cost) {   // (NaN compares false)
      const double gain = cost - out[0];
      be.accept();
      for (int k = 0; k < 6 * C; ++k) ext[k] = trial[k];
      cost = out[0];
      record(cost, lam, true);
      lam = fmax(0.1 * lam, KB_LAMBDA_MIN);
      if (int rc = be.reduce(ext, lam, sys)) return rc;
      ++res.njev;
      res.optimality = gradient();
      if (res.optimality <= opt.gtol) status = 1;
      else if (gain <= opt.ftol * cost) status = 2;
      else if (small) status = 3;
    } else {
      record(out[0], lam, false);
      lam *= 10.0;
      if (small || !(lam < KB_LAMBDA_MAX)) { status = 3; break; }
      if (int rc = be.reduce(ext, lam, sys)) return rc;
    }
  }
  res.cost = cost;
  res.status = status;
  return 0;
}
}  // namespace mcba
