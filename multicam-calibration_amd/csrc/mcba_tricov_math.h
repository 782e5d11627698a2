// mcba_tricov_math.h -- the per-lane arithmetic of csrc/mcba_tricov.hip: how well a triangulated point is known.
//   H = sum_c A_c^T W_c A_c        A_c = d(u, v)/dX of the five-coefficient model in camera c, W_c = diag(rho'((f / f_scale)^2)) per scalar
//   Sigma_det = sigma2 H^-1         H inverted through its Jacobi-scaled 3 x 3 Cholesky factor; a pivot whose square is below 1e-12 = degenerate
//   Sigma_cal = G Sigma_cc G^T      G = [G_0 .. G_{C-1}], G_c = H^-1 A_c^T W_c B_c, B_c = d(u, v)/d(theta_c), theta_c the camera's 12 parameters
// The Gauss-Newton, IRLS-weighted convention of mcba_cov_math.h.  What a lane does is here; what the lanes do together (the matrix-core product
// Z = G Sigma_cc, the fixed-order sums behind sigma2) is the kernels'.  Nothing here is new arithmetic where the library had it: project5 (with its
// intermediates) and make_kp_cam (mcba_keypoint_math.h), chol3, fwd3, bwd3, sym3 (mcba_pnp_math.h), rot_and_jr and loss_weights (mcba_math.h).
// The same text is compiled with g++ into tests/hostcheck/tricov_hostcheck.cpp (tests/test_hostcheck_tricov.py).
#pragma once
#include "mcba_keypoint_math.h"

namespace mcba {

// status of a point
constexpr int TC_OK = 1, TC_TOO_FEW_VIEWS = -1, TC_DEGENERATE = -2;
// the smallest square of a pivot of the Jacobi-scaled H that is still factorised: beyond a scaled condition number of roughly 1e12 nothing is left
constexpr double TC_PIVOT2_MIN = 1e-12;

// one camera of the table, 30 doubles: the keypoint kernels' camera and the right Jacobian of its rotation vector (d R(r) X / dr_k = R (Jr e_k x X))
struct TcCam {
  KpCam kc;
  double Jr[9];
};
static_assert(sizeof(TcCam) == 30 * sizeof(double), "the camera table is 30 doubles per camera");

MCBA_HD void make_tc_cam(const double* cam12, const double* dist5, TcCam& tc) {
  make_kp_cam(cam12, dist5, tc.kc);
  double R[9];
  rot_and_jr(cam12 + 6, R, tc.Jr);
}

// ---- the rho'-weighted linearisation at X: packed H (00 01 02 11 12 22) and wss = sum w f^2 over the cameras that see the point.  Returns the
// number of views (the point's present scalars are twice that).  observation(c, ou, ov) hands out the point's detection in camera c; with a
// fourth argument also sw = sqrt(w) of the detection (mcba_keypoint_math.h: the residual times sw, rho' times w, unseen unless sw > 0).
template <int LOSS, class Obs>
MCBA_HD int tricov_linearise(const KpCam* cams, int C, Obs& observation, const double X[3], double fs2, double inv_fs2, double* H, double& wss) {
#pragma unroll
  for (int i = 0; i < 6; ++i) H[i] = 0.0;
  wss = 0.0;
  int views = 0;
  for (int c = 0; c < C; ++c) {
    double ou, ov, sw;
    if (kp_observe(observation, c, ou, ov, sw, 0)) {
      ++views;
      double u, v, Ju[3], Jv[3];
      project5<true>(cams[c], X, u, v, Ju, Jv);
      double fu = ou - u, fv = ov - v;
      kp_scale_pair<KpWeighted<Obs>::value>(sw, fu, fv);
      double rh, wu, wv, w2;
      loss_weights<LOSS>(fu, fs2, inv_fs2, rh, wu, w2);
      loss_weights<LOSS>(fv, fs2, inv_fs2, rh, wv, w2);
      wss += fma(wu, fu * fu, wv * (fv * fv));
      kp_scale_pair<KpWeighted<Obs>::value>(sw * sw, wu, wv);
      int k = 0;
#pragma unroll
      for (int i = 0; i < 3; ++i) {
        const double a = wu * Ju[i], b = wv * Jv[i];
#pragma unroll
        for (int j = i; j < 3; ++j, ++k) H[k] = fma(a, Ju[j], fma(b, Jv[j], H[k]));
      }
    }
  }
  return views;
}

// ---- H^-1 (packed, unscaled) through the Cholesky factor of D H D, D = diag(H)^-1/2.  false = degenerate (a diagonal entry that is not
// positive, or a pivot whose square is below TC_PIVOT2_MIN), Hi then NaN.
MCBA_HD bool tricov_inv3(const double* H, double* Hi) {
  const double nan = __builtin_nan("");
#pragma unroll
  for (int i = 0; i < 6; ++i) Hi[i] = nan;
  if (!(H[0] > 0.0 && H[3] > 0.0 && H[5] > 0.0)) return false;
  const double d[3] = {1.0 / sqrt(H[0]), 1.0 / sqrt(H[3]), 1.0 / sqrt(H[5])};
  const double A[6] = {1.0, H[1] * d[0] * d[1], H[2] * d[0] * d[2], 1.0, H[4] * d[1] * d[2], 1.0};
  double L[6];
  chol3(A, 0.0, L);   // (a pivot that is not positive comes back as 1e-150: far below the threshold)
  if (!(L[0] * L[0] >= TC_PIVOT2_MIN && L[3] * L[3] >= TC_PIVOT2_MIN && L[5] * L[5] >= TC_PIVOT2_MIN)) return false;
#pragma unroll
  for (int j = 0; j < 3; ++j) {   // column j of the scaled inverse; its entries i <= j are the packed row i
    const double e[3] = {j == 0 ? 1.0 : 0.0, j == 1 ? 1.0 : 0.0, j == 2 ? 1.0 : 0.0};
    double z[3], y[3];
    fwd3(L, e, z);
    bwd3(L, z, y);
#pragma unroll
    for (int i = 0; i <= j; ++i) Hi[i == 0 ? j : (i == 1 ? 2 + j : 5)] = (d[i] * d[j]) * y[i];
  }
  return true;
}

// ---- one point: status, views, packed H^-1 (NaN unless the status is TC_OK) and its share wss of sum w f^2
template <int LOSS, class Obs>
MCBA_HD int tricov_point(const KpCam* cams, int C, Obs& observation, const double X[3], double f_scale, double* Hi, int& views, double& wss) {
  const double fs2 = f_scale * f_scale, inv_fs2 = 1.0 / fs2;
  double H[6];
  views = tricov_linearise<LOSS>(cams, C, observation, X, fs2, inv_fs2, H, wss);
  if (!(views >= 2 && X[0] == X[0] && X[1] == X[1] && X[2] == X[2])) {
    const double nan = __builtin_nan("");
#pragma unroll
    for (int i = 0; i < 6; ++i) Hi[i] = nan;
    return TC_TOO_FEW_VIEWS;
  }
  return tricov_inv3(H, Hi) ? TC_OK : TC_DEGENERATE;
}

// ---- the rows of one camera at X: the projection (u, v), A_c = (Ju; Jv) and B_c = (Bu; Bv), 12 columns in the order of theta_c =
// (fx fy cx cy k1 k2 | rotation vector | translation); p1, p2, k3 are constants
MCBA_HD void tricov_cam_rows(const TcCam& tc, const double X[3], double& u, double& v, double* Ju, double* Jv, double* Bu, double* Bv) {
  const KpCam& kc = tc.kc;
  Proj5Parts q;
  project5<true>(kc, X, u, v, Ju, Jv, &q);
  const double fx = kc.K.fx, fy = kc.K.fy, x = q.x, y = q.y, r2 = x * x + y * y;
  Bu[0] = q.xd; Bv[0] = 0.0;
  Bu[1] = 0.0;  Bv[1] = q.yd;
  Bu[2] = 1.0; Bv[2] = 0.0;
  Bu[3] = 0.0; Bv[3] = 1.0;
  Bu[4] = fx * x * r2;      Bv[4] = fy * y * r2;
  Bu[5] = fx * x * r2 * r2; Bv[5] = fy * y * r2 * r2;
#pragma unroll
  for (int k = 0; k < 3; ++k) {   // d X_c / dr_k = R (j_k x X), j_k = column k of Jr; (Ju; Jv) = P R already
    const double j0 = tc.Jr[k], j1 = tc.Jr[3 + k], j2 = tc.Jr[6 + k];
    const double cr[3] = {j1 * X[2] - j2 * X[1], j2 * X[0] - j0 * X[2], j0 * X[1] - j1 * X[0]};
    Bu[6 + k] = fma(Ju[0], cr[0], fma(Ju[1], cr[1], Ju[2] * cr[2]));
    Bv[6 + k] = fma(Jv[0], cr[0], fma(Jv[1], cr[1], Jv[2] * cr[2]));
  }
#pragma unroll
  for (int j = 0; j < 3; ++j) { Bu[9 + j] = q.Pu[j]; Bv[9 + j] = q.Pv[j]; }   // d X_c / dt = I: the rows of P = d(u, v)/dX_c
}

// ---- one row block G_c = H^-1 (Ju^T wu Bu + Jv^T wv Bv): g[3][12] row-major
MCBA_HD void tricov_g_rows(const double* Hi, const double* Ju, const double* Jv, double wu, double wv, const double* Bu, const double* Bv, double* g) {
  double au[3], av[3];
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    au[i] = wu * fma(sym3(Hi, i, 0), Ju[0], fma(sym3(Hi, i, 1), Ju[1], sym3(Hi, i, 2) * Ju[2]));
    av[i] = wv * fma(sym3(Hi, i, 0), Jv[0], fma(sym3(Hi, i, 1), Jv[1], sym3(Hi, i, 2) * Jv[2]));
  }
#pragma unroll
  for (int i = 0; i < 3; ++i) {
#pragma unroll
    for (int j = 0; j < 12; ++j) g[12 * i + j] = fma(au[i], Bu[j], av[i] * Bv[j]);
  }
}

// G_c of the point X for the detection (ou, ov) of camera tc, present; WEIGHTED: of weight sw^2 > 0 (the residual times sw, rho' times sw^2
// for A_c and B_c)
template <int LOSS, bool WEIGHTED>
MCBA_HD void tricov_g_block_w(const TcCam& tc, const double X[3], double ou, double ov, double sw, const double* Hi, double fs2, double inv_fs2, double* g) {
  double u, v, Ju[3], Jv[3], Bu[12], Bv[12];
  tricov_cam_rows(tc, X, u, v, Ju, Jv, Bu, Bv);
  double fu = ou - u, fv = ov - v;
  kp_scale_pair<WEIGHTED>(sw, fu, fv);
  double rh, wu, wv, w2;
  loss_weights<LOSS>(fu, fs2, inv_fs2, rh, wu, w2);
  loss_weights<LOSS>(fv, fs2, inv_fs2, rh, wv, w2);
  kp_scale_pair<WEIGHTED>(sw * sw, wu, wv);
  tricov_g_rows(Hi, Ju, Jv, wu, wv, Bu, Bv, g);
}
template <int LOSS>
MCBA_HD void tricov_g_block(const TcCam& tc, const double X[3], double ou, double ov, const double* Hi, double fs2, double inv_fs2, double* g) {
  tricov_g_block_w<LOSS, false>(tc, X, ou, ov, 1.0, Hi, fs2, inv_fs2, g);
}
template <int LOSS>
MCBA_HD void tricov_g_block(const TcCam& tc, const double X[3], double ou, double ov, double sw, const double* Hi, double fs2, double inv_fs2, double* g) {
  tricov_g_block_w<LOSS, true>(tc, X, ou, ov, sw, Hi, fs2, inv_fs2, g);
}

// ---- the packed output blocks (00 01 02 11 12 22).  entry e -> (k, l), k <= l
MCBA_HD void tricov_tri3_pair(int e, int& k, int& l) {
  k = e < 3 ? 0 : (e < 5 ? 1 : 2);
  l = e < 3 ? e : (e < 5 ? e - 2 : 2);
}
// one entry of the detection term sigma2 H^-1 and of the calibration term (G Sigma_cc G^T)_kl = sum_j Z_kj G_lj; NaN unless the point is TC_OK
MCBA_HD double tricov_det_entry(double hi, double sigma2, bool ok) { return ok ? sigma2 * hi : __builtin_nan(""); }
MCBA_HD double tricov_cal_entry(double zg, bool ok) { return ok ? zg : __builtin_nan(""); }

// the pooled noise scale: sum w f^2 / (m - 3 P_u), NaN unless m > 3 P_u
MCBA_HD double tricov_sigma2(double wss, double m, double nfree) { return m > nfree ? wss / (m - nfree) : __builtin_nan(""); }

}  // namespace mcba
