// mcba_kpcam_math.h -- the arithmetic of csrc/mcba_kpcam.hip and csrc/mcba_kpcam_api.hip: free-point bundle adjustment of
// the cameras on raw keypoint detections, intrinsics among the unknowns.  mcba_kpba_math.h with 12 rows per camera where it has 6:
//   theta_c = (fx fy cx cy k1 k2 | rotation vector | translation), B = all 12 columns of tricov_cam_rows; p1, p2, k3 stay constants
//   per point p   H_p, g_p as there (they do not depend on which camera scalars are free),  W_cp = B_c^T w A_c (12 x 3)
//   per camera c  acc[kKcAcc] = U_c packed lower (78) | g_c (12) | sum_p Y_cp z_p (12)
//   reduced       S = U + diag(1 / std^2) + lam diag(.) - sum_p Y_p Y_p^T,   rhs = -g_c - (theta - theta_0) / std^2 + sum_p Y_p z_p
// held: 12 bits per camera in theta_c order; bits 6 .. 11 mean what the bits 0 .. 5 of refine_extrinsics mean.
// The 3 x 3 point block is mcba_kpba_math.h's (kpba_factor, kpba_fwd, kpba_bwd, kpba_point_step, kpba_status), and so are the dense solve, the
// options and the result of the loop.  The Gaussian prior on the intrinsics is the host's alone (kpcam_lm): no kernel sees it.
// An item of the reduction is (camera, half, point): HALF 0 the rows 0 .. 5 (intrinsics), HALF 1 the rows 6 .. 11 (extrinsics) of Y_cp, of
// the lower triangle of U_c, of g_c and of Y_cp z_p -- 18 + 33 doubles and 18 + 69, not 36 + 102 at once.
#pragma once
#include "mcba_kpba_math.h"

namespace mcba {

constexpr int kKcRows = 12;       // scalars per camera
constexpr int kKcMaxCams = 12;    // 12 C <= 144: nine 16-row tiles
constexpr int kKcAcc = 102;       // per camera: U_c packed lower (78) | g_c (12) | sum_p Y_cp z_p (12)
constexpr int kKcG = 78, kKcYz = 90;
constexpr int kKcHeldAll = 0xFFF;

// ---- one point at X: kpba_point with q = sum_c W_cp^T dtheta_c over all 12 columns (dtheta: 12 per camera, or NULL)
template <int LOSS, class Obs>
MCBA_HD void kpcam_point(const TcCam* cams, int C, Obs& observation, const double X[3], double fs2, double inv_fs2, const double* dtheta, KbPoint& pt) {
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
      for (int i = 0; i < kKcRows; ++i) {
        bu = fma(Bu[i], dtheta[kKcRows * c + i], bu);
        bv = fma(Bv[i], dtheta[kKcRows * c + i], bv);
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

// ---- one (camera, half, point) item, the camera seeing the point.  Y: the rows 6 HALF .. 6 HALF + 5 of Y_cp (6 x 3, row-major; a row whose bit
// in `held` is set is zero).  a: the rows' share of the camera's sums, kpcam_half_size(HALF) doubles = the rows of the lower triangle of U_c
// (row i: columns 0 .. i; 21 doubles for HALF 0, 57 for HALF 1) | g_c (6) | Y_cp z_p (6); kpcam_half_slot maps them into acc[kKcAcc].
MCBA_HD constexpr int kpcam_half_tri(int half) { return half ? 57 : 21; }
MCBA_HD constexpr int kpcam_half_size(int half) { return kpcam_half_tri(half) + 12; }
MCBA_HD constexpr int kpcam_half_slot(int half, int k) {
  return k < kpcam_half_tri(half) ? (half ? 21 + k : k) : (k < kpcam_half_tri(half) + 6 ? kKcG + 6 * half + (k - kpcam_half_tri(half)) : kKcYz + 6 * half + (k - kpcam_half_tri(half) - 6));
}
template <int LOSS, bool WEIGHTED, int HALF>
MCBA_HD void kpcam_item_w(const TcCam& tc, const double X[3], double ou, double ov, double sw, double fs2, double inv_fs2, const KbFactor& f, const double* zp, int held, double* Y, double* a) {
  constexpr int R0 = 6 * HALF, NT = kpcam_half_tri(HALF);
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
  for (int r = 0; r < 6; ++r) {
    const int i = R0 + r;
    const double p = wu * Bu[i], q = wv * Bv[i];
#pragma unroll
    for (int j = 0; j <= i; ++j, ++k) a[k] = fma(p, Bu[j], q * Bv[j]);
    a[NT + r] = -fma(gu, Bu[i], gv * Bv[i]);
    const double w[3] = {fma(p, Ju[0], q * Jv[0]), fma(p, Ju[1], q * Jv[1]), fma(p, Ju[2], q * Jv[2])};   // row i of W_cp
    double y[3];
    kpba_fwd(f, w, y);
    const bool off = (held >> i) & 1;
#pragma unroll
    for (int j = 0; j < 3; ++j) Y[3 * r + j] = off ? 0.0 : y[j];
    a[NT + 6 + r] = off ? 0.0 : fma(y[0], zp[0], fma(y[1], zp[1], y[2] * zp[2]));
  }
}

// ================================================================ host side
// ---- what one linearisation hands to the host: YY (NP x NP, NP = 12 C rounded up to 16), acc (C x kKcAcc), cost, present scalars, max |g_p|
struct KcSystem {
  int C = 0, NP = 0;
  std::vector<double> YY, acc;
  double cost = 0.0, count = 0.0, gmax = 0.0;
  void shape(int C_) {
    C = C_; NP = (kKcRows * C + 15) / 16 * 16;
    YY.assign((size_t)NP * NP, 0.0);
    acc.assign((size_t)C * kKcAcc, 0.0);
  }
  double U(int c, int i, int j) const { return acc[(size_t)c * kKcAcc + (i >= j ? i * (i + 1) / 2 + j : j * (j + 1) / 2 + i)]; }
};

// the camera table of theta (12 per camera): k1, k2 from theta, p1, p2, k3 from dist5 (or zero)
inline void kpcam_table(int C, const double* theta, const double* dist5, TcCam* t) {
  for (int c = 0; c < C; ++c) {
    const double d[5] = {theta[12 * c + 4], theta[12 * c + 5], dist5 ? dist5[5 * c + 2] : 0.0, dist5 ? dist5[5 * c + 3] : 0.0, dist5 ? dist5[5 * c + 4] : 0.0};
    make_tc_cam(theta + 12 * c, d, t[c]);
  }
}

// ---- the Gaussian prior on the free intrinsic scalars: 0.5 sum pw (theta - theta_0)^2, pw (C, 6) = 1 / std^2, 0 = none (or pw NULL: no prior)
inline double kpcam_prior_cost(int C, const int* held, const double* pw, const double* theta, const double* theta0) {
  double s = 0.0;
  if (!pw) return s;
  for (int c = 0; c < C; ++c)
    for (int i = 0; i < 6; ++i)
      if (!((held[c] >> i) & 1) && pw[6 * c + i] > 0.0) {
        const double d = theta[12 * c + i] - theta0[12 * c + i];
        s += 0.5 * pw[6 * c + i] * d * d;
      }
  return s;
}

// the prior's weight on scalar k of the 12 C (0 for an extrinsic scalar or where there is no prior) and its share of the gradient there
inline double kpcam_prior_weight(const double* pw, int k) { return pw && k % kKcRows < 6 && pw[6 * (k / kKcRows) + k % kKcRows] > 0.0 ? pw[6 * (k / kKcRows) + k % kKcRows] : 0.0; }
inline double kpcam_prior_gradient(const double* pw, int k, const double* theta, const double* theta0) { return kpcam_prior_weight(pw, k) * (theta[k] - theta0[k]); }

// the closing rescale on the extrinsics columns of theta (kpba_rescale; a camera whose six extrinsics are all held keeps them)
inline double kpcam_rescale(int C, const int* held, double* theta, size_t P, double* pts, int gauge, int scale_cam, double baseline) {
  std::vector<double> ext((size_t)6 * C);
  std::vector<int> h6((size_t)C);
  for (int c = 0; c < C; ++c) {
    for (int k = 0; k < 6; ++k) ext[6 * c + k] = theta[12 * c + 6 + k];
    h6[c] = (held[c] >> 6) & 63;
  }
  const double s = kpba_rescale(C, h6.data(), ext.data(), P, pts, gauge, scale_cam, baseline);
  for (int c = 0; c < C; ++c)
    for (int k = 0; k < 6; ++k) theta[12 * c + 6 + k] = ext[6 * c + k];
  return s;
}
inline double kpcam_baseline(int C, const double* theta, int gauge, int scale_cam) {
  std::vector<double> ext((size_t)6 * C);
  for (int c = 0; c < C; ++c)
    for (int k = 0; k < 6; ++k) ext[6 * c + k] = theta[12 * c + 6 + k];
  return kpba_baseline(ext.data(), gauge, scale_cam);
}

struct KcResult : KbResult {
  double prior_cost = 0.0;
};

// ---- kpba_lm with 12 scalars per camera and the prior.  The rules of the loop (damping, acceptance, termination, history) are kpba_lm's; cost,
// trial cost, cost0 and the history include the prior's cost.  Where the prior enters: 1 / std^2 on the diagonal of U before the lam diag(.)
// damping; (theta - theta_0) / std^2 in the camera gradient, which counts in `optimality`; its cost added to the current and to the trial cost.
// The back end:  int reduce(const double* theta, double lam, KcSystem&)
//                int step(const double* theta_trial, const double* dtheta, double lam, double out[3])     (both 12 per camera)
//                void accept()
template <class BackEnd>
int kpcam_lm(BackEnd& be, int C, const int* held, double* theta, const double* pw, const KbOptions& opt, KcResult& res, double* hist, int hist_cap) {
  std::vector<int> idx;
  for (int c = 0; c < C; ++c)
    for (int i = 0; i < kKcRows; ++i)
      if (!((held[c] >> i) & 1)) idx.push_back(kKcRows * c + i);
  const int n = (int)idx.size(), N = kKcRows * C;
  KcSystem sys;
  sys.shape(C);
  std::vector<double> A((size_t)n * n), b((size_t)n), x((size_t)n), dth((size_t)N), trial((size_t)N), theta0(theta, theta + N);
  auto record = [&](double cost, double lam, bool accepted) {
    if (res.nhist < hist_cap) { hist[3 * res.nhist] = cost; hist[3 * res.nhist + 1] = lam; hist[3 * res.nhist + 2] = accepted ? 1.0 : 0.0; }
    ++res.nhist;
  };
  auto weight = [&](int k) { return kpcam_prior_weight(pw, k); };
  auto grad = [&](int k) { return kpcam_prior_gradient(pw, k, theta, theta0.data()) + sys.acc[(size_t)(k / kKcRows) * kKcAcc + kKcG + k % kKcRows]; };
  auto gradient = [&]() {
    double g = sys.gmax;
    for (int a = 0; a < n; ++a) g = fmax(g, fabs(grad(idx[a])));
    return g;
  };
  double lam = KB_LAMBDA0;
  if (int rc = be.reduce(theta, lam, sys)) return rc;
  double prior = kpcam_prior_cost(C, held, pw, theta, theta0.data());
  double cost = sys.cost + prior;
  res.cost0 = cost;
  res.nfev = res.njev = 1;
  record(cost, lam, true);
  res.optimality = gradient();
  int status = res.optimality <= opt.gtol ? 1 : -1;
  while (status == -1) {
    if (res.nfev >= opt.max_nfev) { status = 0; break; }
    for (int a = 0; a < n; ++a) {
      const int ca = idx[a] / kKcRows, ia = idx[a] % kKcRows;
      for (int k = 0; k < n; ++k) {
        const int ck = idx[k] / kKcRows, ik = idx[k] % kKcRows;
        double v = ca == ck ? sys.U(ca, ia, ik) : 0.0;
        if (a == k) {
          v += weight(idx[a]);
          v = fma(lam, v, v);
        }
        A[(size_t)a * n + k] = v - sys.YY[(size_t)idx[a] * sys.NP + idx[k]];
      }
      b[a] = sys.acc[(size_t)ca * kKcAcc + kKcYz + ia] - grad(idx[a]);
    }
    if (!kpba_dense_solve(n, A.data(), b.data(), x.data())) {   // not positive definite at this damping: more of it
      lam *= 10.0;
      if (!(lam < KB_LAMBDA_MAX)) { status = 3; break; }
      if (int rc = be.reduce(theta, lam, sys)) return rc;
      continue;
    }
    double step2 = 0.0, x2 = 0.0;
    for (int k = 0; k < N; ++k) { dth[k] = 0.0; trial[k] = theta[k]; }
    for (int a = 0; a < n; ++a) {
      dth[idx[a]] = x[a];
      trial[idx[a]] = theta[idx[a]] + x[a];
      step2 += x[a] * x[a];
      x2 += theta[idx[a]] * theta[idx[a]];
    }
    double out[3];
    if (int rc = be.step(trial.data(), dth.data(), lam, out)) return rc;
    ++res.nfev;
    const double trial_prior = kpcam_prior_cost(C, held, pw, trial.data(), theta0.data());
    const double trial_cost = out[0] + trial_prior;
    const double xn = sqrt(x2 + out[2]);
    const bool small = sqrt(step2 + out[1]) < opt.xtol * (opt.xtol + xn);
    if (trial_cost <= cost) {   // (NaN compares false)
      const double gain = cost - trial_cost;
      be.accept();
      for (int k = 0; k < N; ++k) theta[k] = trial[k];
      cost = trial_cost;
      prior = trial_prior;
      record(cost, lam, true);
      lam = fmax(0.1 * lam, KB_LAMBDA_MIN);
      if (int rc = be.reduce(theta, lam, sys)) return rc;
      ++res.njev;
      res.optimality = gradient();
      if (res.optimality <= opt.gtol) status = 1;
      else if (gain <= opt.ftol * cost) status = 2;
      else if (small) status = 3;
    } else {
      record(trial_cost, lam, false);
      lam *= 10.0;
      if (small || !(lam < KB_LAMBDA_MAX)) { status = 3; break; }
      if (int rc = be.reduce(theta, lam, sys)) return rc;
    }
  }
  res.cost = cost;
  res.prior_cost = prior;
  res.status = status;
  return 0;
}
}  // namespace mcba
