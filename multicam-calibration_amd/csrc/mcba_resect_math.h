// mcba_resect_math.h -- the per-lane arithmetic of csrc/mcba_resect.hip and the host loop of csrc/mcba_resect_api.hip:
// camera resection, the pose of one camera from known 3-D points and its own 2-D detections of them.  A hypothesis is the 6-point DLT of six
// index-selected points, projected onto a rotation and settled by ten Gauss-Newton iterations on the same six points (normalised coordinates);
// it is scored over all usable points with the truncated (MSAC) squared reprojection error of the undistorted pixels; the winner is polished
// by a pose-only Levenberg-Marquardt on the raw detections (rs_lm, written against a back end like kpba_lm).
// Reused, not restated: undistort_px and chol_solve (mcba_geom_math.h), det::hartley (mcba_detect_math.h), tv_svd3 and tv_before
// (mcba_twoview_math.h), tricov_cam_rows (mcba_tricov_math.h), loss_weights / lm_weight (mcba_math.h), kpba_dense_solve (mcba_kpba_math.h).
// New: a cyclic Jacobi for 12 x 12 (rs_jacobi_smallest12), rs_dlt, rs_gauss_newton, rs_error2, rs_normal_item, rs_lm.
// Conventions: x_cam = R X + t; a pose is 12 doubles, R row-major then t.
// The same text is compiled with g++ into tests/hostcheck/resection_hostcheck.cpp (tests/test_hostcheck_resection.py).
#pragma once
#include "mcba_twoview_math.h"
#include "mcba_kpba_math.h"

#if defined(__clang__)
#pragma clang fp contract(off)
#endif

namespace mcba {

constexpr int RS_OK = 1, RS_VOID = -1;   // status of a hypothesis
constexpr int kRsSample = 6;             // points of a sample
constexpr int kRsGnIterations = 10;      // Gauss-Newton iterations of a hypothesis (the share not settled by then)
constexpr int kRsSys = 29;               // per camera: upper triangle of J^T W J (21, row-major) | gradient (6) | robust cost | detections used
constexpr double RS_FINITE_MAX = 1.7976931348623157e308;
// The smallest eigen-gap lambda_2 / lambda_12 (ascending eigenvalues of the normalised 12 x 12 normal matrix) at which a DLT start is still
// defined: the null vector is known to about EPS / gap, so below 1e-10 not even its sixth digit is -- the vector is then whatever the rounding
// of the eigen-solver makes of a null space of more than one dimension, and two correct implementations disagree on it.  Six coplanar points
// are the case in point (every multiple of the plane in each of the three rows is a null vector: gap at rounding level, 1e-15); the smallest
// gap of a sample of the test scenes is 1.6e-7.  Such a hypothesis is void.
constexpr double RS_DLT_GAP_MIN = 1e-10;

MCBA_HD bool rs_finite(double x) { return fabs(x) <= RS_FINITE_MAX; }   // (NaN compares false)

// the eigenvector of the smallest eigenvalue of the symmetric 12 x 12 S (row-major, destroyed); V: 144 doubles of work space.  Returns the
// eigen-gap lambda_2 / lambda_12: the second smallest eigenvalue over the largest (0 when the largest is not positive)
MCBA_HD double rs_jacobi_smallest12(double* S, double* V, double* vec) {
  for (int i = 0; i < 144; ++i) V[i] = (i % 13 == 0) ? 1.0 : 0.0;
  for (int sweep = 0; sweep < 30; ++sweep) {
    double off = 0.0, dn = 0.0;
    for (int p = 0; p < 12; ++p) {
      for (int q = p + 1; q < 12; ++q) off += S[p * 12 + q] * S[p * 12 + q];
      dn += S[p * 12 + p] * S[p * 12 + p];
    }
    if (!(off > 1e-32 * dn)) break;   // off-diagonal at rounding level of the largest eigenvalue (or not finite)
    for (int p = 0; p < 12; ++p)
      for (int q = p + 1; q < 12; ++q) {
        const double apq = S[p * 12 + q];
        if (apq == 0.0) continue;
        const double theta = (S[q * 12 + q] - S[p * 12 + p]) / (2.0 * apq);
        const double t = (theta >= 0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
        const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
        for (int k = 0; k < 12; ++k) {  // S <- S J (columns p, q)
          const double skp = S[k * 12 + p], skq = S[k * 12 + q];
          S[k * 12 + p] = c * skp - s * skq;
          S[k * 12 + q] = s * skp + c * skq;
        }
        for (int k = 0; k < 12; ++k) {  // S <- J^T S (rows p, q)
          const double spk = S[p * 12 + k], sqk = S[q * 12 + k];
          S[p * 12 + k] = c * spk - s * sqk;
          S[q * 12 + k] = s * spk + c * sqk;
        }
        for (int k = 0; k < 12; ++k) {
          const double vkp = V[k * 12 + p], vkq = V[k * 12 + q];
          V[k * 12 + p] = c * vkp - s * vkq;
          V[k * 12 + q] = s * vkp + c * vkq;
        }
      }
  }
  int m = 0;
  for (int i = 1; i < 12; ++i)
    if (S[i * 12 + i] < S[m * 12 + m]) m = i;
  for (int k = 0; k < 12; ++k) vec[k] = V[k * 12 + m];
  int m2 = m == 0 ? 1 : 0, top = 0;
  for (int i = 0; i < 12; ++i) {
    if (i != m && S[i * 12 + i] < S[m2 * 12 + m2]) m2 = i;
    if (S[i * 12 + i] > S[top * 12 + top]) top = i;
  }
  return S[top * 12 + top] > 0.0 ? S[m2 * 12 + m2] / S[top * 12 + top] : 0.0;
}

// The 6-point DLT pose of the world points X (6 x 3) seen at the normalised coordinates x (6 x 2): Hartley normalisation of either set (3-D:
// centroid, mean distance sqrt 3; 2-D: sqrt 2), the smallest eigenvector of the 12 x 12 normal matrix of the rows [X 1 0 -uX -u],
// [0 X 1 -vX -v], de-normalised, the sign that makes det of the left 3 x 3 block positive, R = U V^T of that block, t = p_4 over the mean
// singular value.  S, V: 144 doubles of work space each (the caller places them).  pose: R row-major, then t.  false: something is not finite,
// or the eigen-gap is below RS_DLT_GAP_MIN (the start is not defined: coplanar sample points).
MCBA_HD bool rs_dlt(const double* X, const double* x, double* S, double* V, double* pose) {
  double c3[3] = {0.0, 0.0, 0.0};
  for (int k = 0; k < 6; ++k)
    for (int j = 0; j < 3; ++j) c3[j] += X[3 * k + j];
  for (int j = 0; j < 3; ++j) c3[j] /= 6.0;
  double d3 = 0.0;
  for (int k = 0; k < 6; ++k) {
    const double a = X[3 * k] - c3[0], b = X[3 * k + 1] - c3[1], c = X[3 * k + 2] - c3[2];
    d3 += sqrt(a * a + b * b + c * c);
  }
  d3 /= 6.0;
  const double s3 = d3 > 0 ? 1.7320508075688772 / d3 : 1.0;
  double mx, my, s2;
  det::hartley(x, 6, mx, my, s2);
  for (int i = 0; i < 144; ++i) S[i] = 0.0;
  for (int k = 0; k < 6; ++k) {
    const double a = s3 * (X[3 * k] - c3[0]), b = s3 * (X[3 * k + 1] - c3[1]), c = s3 * (X[3 * k + 2] - c3[2]);
    const double u = s2 * (x[2 * k] - mx), v = s2 * (x[2 * k + 1] - my);
    const double r0[12] = {a, b, c, 1.0, 0.0, 0.0, 0.0, 0.0, -u * a, -u * b, -u * c, -u};
    const double r1[12] = {0.0, 0.0, 0.0, 0.0, a, b, c, 1.0, -v * a, -v * b, -v * c, -v};
    for (int i = 0; i < 12; ++i)
      for (int j = i; j < 12; ++j) S[12 * i + j] = fma(r0[i], r0[j], fma(r1[i], r1[j], S[12 * i + j]));
  }
  for (int i = 0; i < 12; ++i)
    for (int j = 0; j < i; ++j) S[12 * i + j] = S[12 * j + i];
  double p[12];
  const double gap = rs_jacobi_smallest12(S, V, p);
  // P = T2^-1 Pn T3, T3 = [[s3 I, -s3 c3], [0, 1]], T2^-1 = [[1 / s2, 0, mx], [0, 1 / s2, my], [0, 0, 1]]
  double M[12], P[12];
  for (int r = 0; r < 3; ++r) {
    M[4 * r] = p[4 * r] * s3; M[4 * r + 1] = p[4 * r + 1] * s3; M[4 * r + 2] = p[4 * r + 2] * s3;
    M[4 * r + 3] = p[4 * r + 3] - (M[4 * r] * c3[0] + M[4 * r + 1] * c3[1] + M[4 * r + 2] * c3[2]);
  }
  for (int j = 0; j < 4; ++j) {
    P[j] = M[j] / s2 + mx * M[8 + j];
    P[4 + j] = M[4 + j] / s2 + my * M[8 + j];
    P[8 + j] = M[8 + j];
  }
  const double dt = P[0] * (P[5] * P[10] - P[6] * P[9]) - P[1] * (P[4] * P[10] - P[6] * P[8]) + P[2] * (P[4] * P[9] - P[5] * P[8]);
  const double sg = dt < 0.0 ? -1.0 : 1.0;
  double a[3][3], v[3][3];
#pragma unroll
  for (int c = 0; c < 3; ++c)
#pragma unroll
    for (int r = 0; r < 3; ++r) a[c][r] = sg * P[4 * r + c];
  tv_svd3(a, v);
  double sv[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) sv[c] = sqrt(fma(a[c][0], a[c][0], fma(a[c][1], a[c][1], a[c][2] * a[c][2])));
  const double mean = (sv[0] + sv[1] + sv[2]) / 3.0;
  bool ok = sv[0] > 0.0 && sv[1] > 0.0 && sv[2] > 0.0 && gap >= RS_DLT_GAP_MIN;   // (a NaN gap compares false)
#pragma unroll
  for (int r = 0; r < 3; ++r) {
#pragma unroll
    for (int c = 0; c < 3; ++c) pose[3 * r + c] = (a[0][r] / sv[0]) * v[0][c] + (a[1][r] / sv[1]) * v[1][c] + (a[2][r] / sv[2]) * v[2][c];
    pose[9 + r] = sg * P[4 * r + 3] / mean;
  }
#pragma unroll
  for (int i = 0; i < 12; ++i) ok = ok && rs_finite(pose[i]);
  return ok;
}

MCBA_HD void rs_camera_point(const double* pose, const double* X, double* Xc) {
  Xc[0] = fma(pose[0], X[0], fma(pose[1], X[1], fma(pose[2], X[2], pose[9])));
  Xc[1] = fma(pose[3], X[0], fma(pose[4], X[1], fma(pose[5], X[2], pose[10])));
  Xc[2] = fma(pose[6], X[0], fma(pose[7], X[1], fma(pose[8], X[2], pose[11])));
}

// One Gauss-Newton iteration on N sample points (6: a DLT hypothesis; 3: a P3P candidate, mcba_resect_p3p_math.h): residuals pi(R X + t) - x
// in normalised coordinates (2 N), unknowns (omega, delta) of the left-multiplicative update R <- exp(omega) R, t <- exp(omega) t + delta, the
// 6 x 6 normal equations solved by chol_solve<6>.  step6: the step taken (tests: how far the last one still moved).
template <int N>
MCBA_HD void rs_gauss_newton_step(const double* X, const double* x, double* pose, double* step6) {
  double A[21], g[6];
#pragma unroll
  for (int i = 0; i < 21; ++i) A[i] = 0.0;
#pragma unroll
  for (int i = 0; i < 6; ++i) g[i] = 0.0;
  for (int k = 0; k < N; ++k) {
    double Xc[3];
    rs_camera_point(pose, X + 3 * k, Xc);
    const double iz = 1.0 / Xc[2], px = Xc[0] * iz, py = Xc[1] * iz;
    const double ru = px - x[2 * k], rv = py - x[2 * k + 1];
    const double au[3] = {iz, 0.0, -px * iz}, av[3] = {0.0, iz, -py * iz};
    // a . (omega x Xc) = omega . (Xc x a)
    const double ju[6] = {Xc[1] * au[2] - Xc[2] * au[1], Xc[2] * au[0] - Xc[0] * au[2], Xc[0] * au[1] - Xc[1] * au[0], au[0], au[1], au[2]};
    const double jv[6] = {Xc[1] * av[2] - Xc[2] * av[1], Xc[2] * av[0] - Xc[0] * av[2], Xc[0] * av[1] - Xc[1] * av[0], av[0], av[1], av[2]};
    int e = 0;
#pragma unroll
    for (int i = 0; i < 6; ++i) {
#pragma unroll
      for (int j = i; j < 6; ++j, ++e) A[e] = fma(ju[i], ju[j], fma(jv[i], jv[j], A[e]));
      g[i] = fma(ju[i], ru, fma(jv[i], rv, g[i]));
    }
  }
#pragma unroll
  for (int i = 0; i < 6; ++i) g[i] = -g[i];
  chol_solve<6>(A, g);
  double E[9], R[9], t[3];
  rot_only(g, E);
  mm33(E, pose, R);
  mv3(E, pose + 9, t);
#pragma unroll
  for (int i = 0; i < 9; ++i) pose[i] = R[i];
#pragma unroll
  for (int i = 0; i < 3; ++i) pose[9 + i] = t[i] + g[3 + i];
#pragma unroll
  for (int i = 0; i < 6; ++i) step6[i] = g[i];
}

// A hypothesis: rs_dlt, then exactly kRsGnIterations Gauss-Newton iterations.  RS_VOID (pose all NaN) when anything is not finite, when the
// DLT start is not defined (rs_dlt) or when a sample point ends with z <= 0.  step6: the last step.
MCBA_HD int rs_hypothesis(const double* X, const double* x, double* S, double* V, double* pose, double* step6) {
  bool ok = rs_dlt(X, x, S, V, pose);
  for (int i = 0; i < 6; ++i) step6[i] = 0.0;
  for (int it = 0; it < kRsGnIterations; ++it) rs_gauss_newton_step<kRsSample>(X, x, pose, step6);
#pragma unroll
  for (int i = 0; i < 12; ++i) ok = ok && rs_finite(pose[i]);
  for (int k = 0; k < 6; ++k) {
    double Xc[3];
    rs_camera_point(pose, X + 3 * k, Xc);
    ok = ok && Xc[2] > 0.0;
  }
  if (!ok) {
#pragma unroll
    for (int i = 0; i < 12; ++i) pose[i] = __builtin_nan("");
  }
  return ok ? RS_OK : RS_VOID;
}

// K [R | t] row-major (3 x 4) for undistorted pixels; k4 = (fx, fy, cx, cy)
MCBA_HD void rs_pixel_matrix(const double* pose, const double* k4, double* KP) {
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const double r0 = j < 3 ? pose[j] : pose[9], r1 = j < 3 ? pose[3 + j] : pose[10], r2 = j < 3 ? pose[6 + j] : pose[11];
    KP[j] = fma(k4[0], r0, k4[2] * r2);
    KP[4 + j] = fma(k4[1], r1, k4[3] * r2);
    KP[8 + j] = r2;
  }
}

// squared reprojection error in px^2 of the world point (X, Y, Z) against the undistorted pixel (u, v) under KP; +inf for a point that is not
// in front of the camera (z <= 0), NaN where something is NaN -- which no comparison takes for an inlier
MCBA_HD double rs_error2(const double* KP, double X, double Y, double Z, double u, double v) {
  const double a = fma(KP[0], X, fma(KP[1], Y, fma(KP[2], Z, KP[3])));
  const double b = fma(KP[4], X, fma(KP[5], Y, fma(KP[6], Z, KP[7])));
  const double z = fma(KP[8], X, fma(KP[9], Y, fma(KP[10], Z, KP[11])));
  const double iz = fast_rcp(z);
  const double du = fma(a, iz, -u), dv = fma(b, iz, -v);
  const double e2 = fma(du, du, dv * dv);
  return z <= 0.0 ? __builtin_inf() : e2;
}
// the truncated cost term and the inlier test of one point (tv_cost_term / tv_inlier: a NaN or +inf is not an inlier and costs the full threshold^2)

// one usable point through k_rs_prepare: the detection undistorted (pixels) and normalised.  k4 = (fx, fy, cx, cy), d5 = (k1 k2 p1 p2 k3)
MCBA_HD void rs_prepare(double u, double v, const double* k4, const double* d5, int und_iters, double out4[4]) {
  undistort_px(u, v, k4[0], k4[1], k4[2], k4[3], d5, und_iters, out4[0], out4[1]);
  out4[2] = (out4[0] - k4[2]) / k4[0];
  out4[3] = (out4[1] - k4[3]) / k4[1];
}
MCBA_HD bool rs_usable(double X, double Y, double Z, double u, double v) { return rs_finite(X) && rs_finite(Y) && rs_finite(Z) && rs_finite(u) && rs_finite(v); }

// ---- the polish: one detection's share of a camera's normal system.  f = detection - projection of the five-coefficient model on the RAW
// detection, B = columns 6 .. 11 of tricov_cam_rows (rotation vector, translation), the curvature weights of the extrinsics refinement
// (lm_weight, Triggs floored), rho' in the gradient.  acc[kRsSys]: upper triangle of B^T w B | gradient -B^T rho' f | robust cost | 1.
template <int LOSS>
MCBA_HD void rs_normal_item(const TcCam& tc, const double X[3], double ou, double ov, double fs2, double inv_fs2, double* acc) {
  double u, v, Ju[3], Jv[3], Bu[12], Bv[12];
  tricov_cam_rows(tc, X, u, v, Ju, Jv, Bu, Bv);
  const double fu = ou - u, fv = ov - v;
  double rhu, gwu, w2u, rhv, gwv, w2v;
  loss_weights<LOSS>(fu, fs2, inv_fs2, rhu, gwu, w2u);
  loss_weights<LOSS>(fv, fs2, inv_fs2, rhv, gwv, w2v);
  const double wu = lm_weight(gwu, w2u, MCBA_CURV_FLOOR_TRIGGS), wv = lm_weight(gwv, w2v, MCBA_CURV_FLOOR_TRIGGS);
  const double gu = gwu * fu, gv = gwv * fv;
  int k = 0;
#pragma unroll
  for (int i = 0; i < 6; ++i) {
    const double a = wu * Bu[6 + i], b = wv * Bv[6 + i];
#pragma unroll
    for (int j = i; j < 6; ++j, ++k) acc[k] = fma(a, Bu[6 + j], b * Bv[6 + j]);
    acc[21 + i] = -fma(gu, Bu[6 + i], gv * Bv[6 + i]);
  }
  acc[27] = rhu + rhv;
  acc[28] = 1.0;
}
// the robust cost of one detection alone (a trial pose)
template <int LOSS>
MCBA_HD double rs_cost_item(const TcCam& tc, const double X[3], double ou, double ov, double fs2, double inv_fs2) {
  double u, v;
  project5<false>(tc.kc, X, u, v);
  double rhu, rhv, gw, w2;
  loss_weights<LOSS>(ou - u, fs2, inv_fs2, rhu, gw, w2);
  loss_weights<LOSS>(ov - v, fs2, inv_fs2, rhv, gw, w2);
  return rhu + rhv;
}

// ================================================================ host side
struct RsCamera {   // one camera of rs_lm
  double pose[6];   // rotation vector, translation: the start on entry, the result on exit
  double sys[kRsSys];
  double lam = KB_LAMBDA0, cost = 0.0, cost0 = 0.0, optimality = 0.0;
  int nfev = 0, njev = 0, status = -1;
};

// ---- Pose-only Levenberg-Marquardt over fixed points, every camera a problem of its own: Marquardt's damping lam diag(.) with kpba_lm's
// tenfold rule (down on acceptance, up on rejection), a trial accepted when the robust cost does not rise (the result is never worse than the
// start), scipy's status values -- 1 gtol (inf-norm of the gradient), 2 ftol (an accepted step gained no more than ftol cost), 3 xtol
// (|step| < xtol (xtol + |x|), or the damping ran out of range), 0 max_nfev.  A stopped camera is not evaluated again and no longer moves.
// The back end:  int normal(int n, const int* ids, const double* poses6, double* sys)    n cameras ids[k] at poses6[6 k ..]: sys[kRsSys k ..]
//                int trial(int n, const int* ids, const double* poses6, double* cost)     the robust cost alone
// One call of either per evaluation, whatever the number of cameras still running.  A non-zero return ends the loop and is returned.
template <class BackEnd>
int rs_lm(BackEnd& be, int C, RsCamera* cams, const KbOptions& opt) {
  std::vector<int> ids;
  std::vector<double> poses, out;
  auto gather = [&](auto&& pick) {
    ids.clear(); poses.clear();
    for (int c = 0; c < C; ++c)
      if (pick(c)) ids.push_back(c);
  };
  auto grad = [](const RsCamera& cm) {
    double g = 0.0;
    for (int i = 0; i < 6; ++i) g = fmax(g, fabs(cm.sys[21 + i]));
    return g;
  };
  auto linearise = [&]() -> int {   // the cameras in ids, at their own poses
    if (ids.empty()) return 0;
    poses.resize(6 * ids.size());
    out.resize((size_t)kRsSys * ids.size());
    for (size_t k = 0; k < ids.size(); ++k)
      for (int i = 0; i < 6; ++i) poses[6 * k + i] = cams[ids[k]].pose[i];
    if (int rc = be.normal((int)ids.size(), ids.data(), poses.data(), out.data())) return rc;
    for (size_t k = 0; k < ids.size(); ++k) {
      RsCamera& cm = cams[ids[k]];
      for (int i = 0; i < kRsSys; ++i) cm.sys[i] = out[(size_t)kRsSys * k + i];
      ++cm.njev;
      cm.optimality = grad(cm);
    }
    return 0;
  };
  gather([&](int c) { return cams[c].status == -1; });
  if (int rc = linearise()) return rc;
  for (int c : ids) {
    RsCamera& cm = cams[c];
    cm.cost = cm.cost0 = cm.sys[27];
    cm.nfev = 1;
    cm.lam = KB_LAMBDA0;
    if (cm.optimality <= opt.gtol) cm.status = 1;
  }
  std::vector<double> trial((size_t)6 * C), gain((size_t)C);
  std::vector<char> small((size_t)C), accepted((size_t)C);
  for (;;) {
    for (int c = 0; c < C; ++c) {
      RsCamera& cm = cams[c];
      if (cm.status != -1) continue;
      if (cm.nfev >= opt.max_nfev) { cm.status = 0; continue; }
      double A[36], b[6], x[6];
      for (;;) {   // (the system does not depend on the damping: more of it costs no evaluation)
        int e = 0;
        for (int i = 0; i < 6; ++i)
          for (int j = i; j < 6; ++j, ++e) A[6 * i + j] = A[6 * j + i] = cm.sys[e];
        for (int i = 0; i < 6; ++i) { A[7 * i] = fma(cm.lam, A[7 * i], A[7 * i]); b[i] = -cm.sys[21 + i]; }
        if (kpba_dense_solve(6, A, b, x)) break;
        cm.lam *= 10.0;
        if (!(cm.lam < KB_LAMBDA_MAX)) { cm.status = 3; break; }
      }
      if (cm.status != -1) continue;
      double step2 = 0.0, x2 = 0.0;
      for (int i = 0; i < 6; ++i) {
        trial[6 * c + i] = cm.pose[i] + x[i];
        step2 += x[i] * x[i];
        x2 += cm.pose[i] * cm.pose[i];
      }
      small[c] = sqrt(step2) < opt.xtol * (opt.xtol + sqrt(x2));
    }
    gather([&](int c) { return cams[c].status == -1; });
    if (ids.empty()) break;
    poses.resize(6 * ids.size());
    out.resize(ids.size());
    for (size_t k = 0; k < ids.size(); ++k)
      for (int i = 0; i < 6; ++i) poses[6 * k + i] = trial[6 * ids[k] + i];
    if (int rc = be.trial((int)ids.size(), ids.data(), poses.data(), out.data())) return rc;
    for (size_t k = 0; k < ids.size(); ++k) {
      const int c = ids[k];
      RsCamera& cm = cams[c];
      ++cm.nfev;
      accepted[c] = out[k] <= cm.cost;   // (NaN compares false)
      if (accepted[c]) {
        gain[c] = cm.cost - out[k];
        cm.cost = out[k];
        for (int i = 0; i < 6; ++i) cm.pose[i] = trial[6 * c + i];
        cm.lam = fmax(0.1 * cm.lam, KB_LAMBDA_MIN);
      } else {
        cm.lam *= 10.0;
        if (small[c] || !(cm.lam < KB_LAMBDA_MAX)) cm.status = 3;
      }
    }
    gather([&](int c) { return cams[c].status == -1 && accepted[c]; });
    if (int rc = linearise()) return rc;
    for (int c : ids) {
      RsCamera& cm = cams[c];
      if (cm.optimality <= opt.gtol) cm.status = 1;
      else if (gain[c] <= opt.ftol * cm.cost) cm.status = 2;
      else if (small[c]) cm.status = 3;
    }
  }
  return 0;
}

}  // namespace mcba
