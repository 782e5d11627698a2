// mcba_cov_math.h -- the per-lane arithmetic of csrc/mcba_cov.hip: calibration uncertainty from the Schur system.
//   cameras:  Sigma_cc = sigma2 S_g^-1,  S_g = the undamped Schur complement with the held rows and columns replaced by the identity's,
//             Jacobi-scaled by its diagonal BEFORE it is factorised (S_g: cond ~1e12 as it stands, 1e6 .. 1e7 scaled), A = R^T R,
//             M = R^-T (= L^-1), A^-1 = M^T M, unscaled, held rows and columns 0;
//   frames:   Sigma_ff = sigma2 V_f^-1 + Y_f Sigma_cc Y_f^T,  Y_f = V_f^-1 W_f^T,  V_f^-1 from the frame factor L_f (diagonal slots 1 / L_ii).
// What a lane does is here; what the lanes do together (which thread owns which row, the matrix-core product Z = Y Sigma_cc) is the kernels'.
// The same text is compiled with g++ into tests/hostcheck/cov_hostcheck.cpp (tests/test_hostcheck_covariance.py).
#pragma once
#include "mcba_math.h"

namespace mcba {

// row i of the camera system (width cw per camera: 12, or 6 = extrinsics alone) is held fixed: one of the six extrinsics of the gauge camera
MCBA_HD bool cov_held(int i, int cw, int gauge) { return i / cw == gauge && i % cw >= cw - 6; }

// ---- frames
// V^-1 (packed upper triangle, tri6 order) from the frame factor Lp (row-major lower, diagonal slots 1 / L_ii): V^-1 = L^-T L^-1
MCBA_HD void cov_inv6(const double* Lp, double* Vi) {
  double id[6], Li[6][6];   // Li = L^-1, column by column: L m = e_j
#pragma unroll
  for (int k = 0; k < 6; ++k) id[k] = Lp[k * (k + 1) / 2 + k];
#pragma unroll
  for (int j = 0; j < 6; ++j) {
    double e[6], m[6];
#pragma unroll
    for (int k = 0; k < 6; ++k) e[k] = k == j ? 1.0 : 0.0;
    fwd6(Lp, id, e, m);
#pragma unroll
    for (int k = 0; k < 6; ++k) Li[k][j] = m[k];
  }
#pragma unroll
  for (int i = 0; i < 6; ++i) {
#pragma unroll
    for (int j = i; j < 6; ++j) {
      double s = 0.0;
#pragma unroll
      for (int k = j; k < 6; ++k) s += Li[k][i] * Li[k][j];   // (L^-1 is lower triangular: rows k >= max(i, j) alone)
      Vi[tri6(i, j)] = s;
    }
  }
}

// one column of Y_f = V_f^-1 W_f^T: the record's row w (6 entries) of one camera parameter -> y = V^-1 w
MCBA_HD void cov_y_row(const double* Vi, const double* w, double* y) {
#pragma unroll
  for (int k = 0; k < 6; ++k) {
    double s = 0.0;
#pragma unroll
    for (int l = 0; l < 6; ++l) s += Vi[k <= l ? tri6(k, l) : tri6(l, k)] * w[l];
    y[k] = s;
  }
}

// entry e = tri6(k, l) of a packed 6 x 6 upper triangle -> (k, l), k <= l
MCBA_HD void cov_tri6_pair(int e, int& k, int& l) {
  k = 0;
  while (e >= 6 - k) { e -= 6 - k; ++k; }
  l = k + e;
}

// block assembly, one entry: sigma2 (V^-1)_kl + (Z Y^T)_kl, NaN for a degenerate frame
MCBA_HD double cov_frame_entry(double vi, double zy, double sigma2, bool degenerate) { return degenerate ? __builtin_nan("") : sigma2 * vi + zy; }
// ... and the block: Sigma_ff (6 x 6 row-major, exactly symmetric) from the two packed upper triangles
MCBA_HD void cov_frame_block(const double* Vi, const double* zy, double sigma2, bool degenerate, double* out36) {
#pragma unroll
  for (int k = 0; k < 6; ++k) {
#pragma unroll
    for (int l = k; l < 6; ++l) {
      const double v = cov_frame_entry(Vi[tri6(k, l)], zy[tri6(k, l)], sigma2, degenerate);
      out36[6 * k + l] = v;
      out36[6 * l + k] = v;
    }
  }
}

// ---- cameras.  All matrices row-major with leading dimension ld; R holds the upper factor (A = R^T R: R[k][i], k <= i), M = R^-T.
// Jacobi scale of row i: 1 / sqrt(S_ii); false = the diagonal entry is not positive (the pivot that fails is i)
MCBA_HD bool cov_scale(double sii, bool held, double& isd) {
  isd = 1.0;
  if (held) return true;
  if (!(sii > 0.0)) return false;
  isd = 1.0 / sqrt(sii);
  return true;
}
// entry (k, i) of the scaled, gauge-fixed matrix
MCBA_HD double cov_scaled_entry(double ski, double isd_k, double isd_i, bool held_k, bool held_i, bool diag) {
  if (diag) return 1.0;
  if (held_k || held_i) return 0.0;
  return ski * isd_k * isd_i;
}
// the scaled Cholesky step of the lane that owns column i, at pivot j <= i: A_ji - sum_{k < j} R_ki R_kj (the caller takes the root on the
// diagonal -- not positive = pivot j fails -- and divides by it elsewhere)
MCBA_HD double cov_chol_step(const double* R, int ld, int i, int j) {
  double s = R[(size_t)j * ld + i];
  for (int k = 0; k < j; ++k) s -= R[(size_t)k * ld + i] * R[(size_t)k * ld + j];
  return s;
}
// column j of M = L^-1 (L = R^T), rows k0 .. n - 1 (k0 <= j; the rows above are zero and never read): forward substitution L m = e_j
MCBA_HD void cov_linv_column(const double* R, double* M, int ld, int n, int j, int k0) {
  for (int i = k0; i < n; ++i) {
    double s = i == j ? 1.0 : 0.0;
    for (int k = k0; k < i; ++k) s -= R[(size_t)k * ld + i] * M[(size_t)k * ld + j];
    M[(size_t)i * ld + j] = s / R[(size_t)i * ld + i];
  }
}
// entry (i, j) of Sigma_cc = sigma2 D^-1/2 (M^T M) D^-1/2: the same bits at (i, j) and (j, i)
MCBA_HD double cov_cam_entry(const double* M, const double* isd, int ld, int n, int i, int j, double sigma2) {
  double s = 0.0;
  for (int k = i > j ? i : j; k < n; ++k) s += M[(size_t)k * ld + i] * M[(size_t)k * ld + j];
  return sigma2 * ((isd[i] * isd[j]) * s);
}

}  // namespace mcba
