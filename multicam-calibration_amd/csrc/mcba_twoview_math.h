// mcba_twoview_math.h -- the per-lane arithmetic of csrc/mcba_twoview.hip: the relative pose of two cameras of known
// intrinsics from keypoint correspondences alone.  A hypothesis is the 8-point essential matrix of eight index-selected correspondences; it is
// scored over all correspondences with the truncated (MSAC) Sampson cost in pixels; the winner's four (R, t) are voted on by cheirality.
// Reused, not restated: undistort_px, triangulate_pair (null_vector4) of mcba_geom_math.h, jacobi_smallest9 and hartley of mcba_detect_math.h.
// New: a 3 x 3 one-sided Jacobi SVD (tv_svd3), tv_essential, tv_fundamental, tv_sampson2, tv_candidates, tv_depths.
// Conventions: x_b^T E x_a = 0 on normalised coordinates, E row-major; x_b = R x_a + t; E ~ [t]x R.
// The same text is compiled with g++ into tests/hostcheck/twoview_hostcheck.cpp (tests/test_hostcheck_twoview.py).
#pragma once
#include "mcba_geom_math.h"
#include "mcba_detect_math.h"

#if defined(__clang__)
#pragma clang fp contract(off)
#endif

namespace mcba {

constexpr int TV_OK = 1, TV_VOID = -1;   // status of a hypothesis

// A V = B with orthogonal columns (Hestenes): a[col][row] holds the columns of A on entry and of B = U Sigma on exit, v[col] the columns of V.
// Fixed number of sweeps (quadratic convergence: 4 - 5 reach FP64 for a 3 x 3), branch-free like null_vector4.
MCBA_HD void tv_svd3(double (&a)[3][3], double (&v)[3][3]) {
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) v[i][j] = i == j ? 1.0 : 0.0;
  for (int sweep = 0; sweep < 8; ++sweep) {
#pragma unroll
    for (int p = 0; p < 2; ++p)
#pragma unroll
      for (int q = p + 1; q < 3; ++q) {
        double alpha = 0.0, beta = 0.0, gamma = 0.0;
#pragma unroll
        for (int k = 0; k < 3; ++k) { alpha = fma(a[p][k], a[p][k], alpha); beta = fma(a[q][k], a[q][k], beta); gamma = fma(a[p][k], a[q][k], gamma); }
        const bool rot = gamma * gamma > 1e-32 * alpha * beta;   // already orthogonal to FP64: identity
        const double g = rot ? gamma : 1.0;
        const double zeta = (beta - alpha) / (2.0 * g);
        double t = 1.0 / (fabs(zeta) + sqrt(fma(zeta, zeta, 1.0)));
        t = zeta < 0.0 ? -t : t;
        t = rot ? t : 0.0;
        const double c = 1.0 / sqrt(fma(t, t, 1.0)), s = c * t;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
          const double ap = a[p][k], aq = a[q][k];
          a[p][k] = fma(c, ap, -(s * aq));
          a[q][k] = fma(s, ap, c * aq);
          const double vp = v[p][k], vq = v[q][k];
          v[p][k] = fma(c, vp, -(s * vq));
          v[q][k] = fma(s, vp, c * vq);
        }
      }
  }
}

MCBA_HD void tv_cross(const double* a, const double* b, double* c) {
  c[0] = fma(a[1], b[2], -(a[2] * b[1]));
  c[1] = fma(a[2], b[0], -(a[0] * b[2]));
  c[2] = fma(a[0], b[1], -(a[1] * b[0]));
}

// E = U diag(s1, s2, s3) V^T -> u1, u2 (unit), v1, v2: the singular vectors of the two largest singular values.  false: a non-finite entry
// or a vanishing second singular value.
MCBA_HD bool tv_top2(const double* E, double (&u)[2][3], double (&vv)[2][3]) {
  double a[3][3], v[3][3];
#pragma unroll
  for (int c = 0; c < 3; ++c)
#pragma unroll
    for (int r = 0; r < 3; ++r) a[c][r] = E[3 * r + c];
  tv_svd3(a, v);
  double n[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) n[c] = fma(a[c][0], a[c][0], fma(a[c][1], a[c][1], a[c][2] * a[c][2]));
  // the column of smallest norm is left out (lowest index on a tie); the other two keep their order
  int k = 0;
  k = n[1] < n[k] ? 1 : k;
  k = n[2] < n[k] ? 2 : k;
  const int i0 = k == 0 ? 1 : 0, i1 = k == 2 ? 1 : 2;
  const double s0 = sqrt(n[i0]), s1 = sqrt(n[i1]);
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    u[0][r] = a[i0][r] / s0; u[1][r] = a[i1][r] / s1;
    vv[0][r] = v[i0][r]; vv[1][r] = v[i1][r];
  }
  bool ok = s0 > 0.0 && s1 > 0.0;
#pragma unroll
  for (int r = 0; r < 3; ++r) ok = ok && fabs(u[0][r]) <= 1.5 && fabs(u[1][r]) <= 1.5 && fabs(vv[0][r]) <= 1.5 && fabs(vv[1][r]) <= 1.5;   // (NaN compares false)
  return ok;
}

// canonical sign of nine (or three) numbers: the entry of largest magnitude positive, lowest index on a tie
template <int N>
MCBA_HD void tv_canonical_sign(double* x) {
  int m = 0;
#pragma unroll
  for (int i = 1; i < N; ++i) m = fabs(x[i]) > fabs(x[m]) ? i : m;
  double xm = x[0];
#pragma unroll
  for (int i = 1; i < N; ++i) xm = i == m ? x[i] : xm;
  const double sg = xm < 0.0 ? -1.0 : 1.0;
#pragma unroll
  for (int i = 0; i < N; ++i) x[i] *= sg;
}

// The 8-point essential matrix of the correspondences xa[k] <-> xb[k] (8 x 2 each, normalised coordinates): Hartley normalisation of either
// set, the smallest eigenvector of the 9 x 9 normal matrix of the rows [xb xa, xb ya, xb, yb xa, yb ya, yb, xa, ya, 1], de-normalised,
// projected onto the essential manifold (singular values 1, 1, 0: |E|_F = sqrt 2), sign-canonical.  S: 81 doubles of work space (the caller
// places them).  Returns TV_OK, or TV_VOID with E all NaN when anything is not finite.
MCBA_HD int tv_essential(const double* xa, const double* xb, double* S, double* E) {
  double ax, ay, as, bx, by, bs;
  det::hartley(xa, 8, ax, ay, as);
  det::hartley(xb, 8, bx, by, bs);
  for (int i = 0; i < 81; ++i) S[i] = 0.0;
  for (int k = 0; k < 8; ++k) {
    const double x = as * (xa[2 * k] - ax), y = as * (xa[2 * k + 1] - ay);
    const double u = bs * (xb[2 * k] - bx), v = bs * (xb[2 * k + 1] - by);
    const double r[9] = {u * x, u * y, u, v * x, v * y, v, x, y, 1.0};
    for (int i = 0; i < 9; ++i)
      for (int j = i; j < 9; ++j) S[9 * i + j] = fma(r[i], r[j], S[9 * i + j]);
  }
  for (int i = 0; i < 9; ++i)
    for (int j = 0; j < i; ++j) S[9 * i + j] = S[9 * j + i];
  double e[9];
  det::jacobi_smallest9(S, e);
  // E = Tb^T En Ta, Ta = [[as, 0, -as ax], [0, as, -as ay], [0, 0, 1]], Tb likewise
  double M[9];
  for (int r = 0; r < 3; ++r) {
    M[3 * r] = e[3 * r] * as;
    M[3 * r + 1] = e[3 * r + 1] * as;
    M[3 * r + 2] = e[3 * r + 2] - e[3 * r] * as * ax - e[3 * r + 1] * as * ay;
  }
  double D[9];
  for (int c = 0; c < 3; ++c) {
    D[c] = bs * M[c];
    D[3 + c] = bs * M[3 + c];
    D[6 + c] = M[6 + c] - bs * bx * M[c] - bs * by * M[3 + c];
  }
  double u[2][3], v[2][3];
  bool ok = tv_top2(D, u, v);
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int c = 0; c < 3; ++c) E[3 * r + c] = fma(u[0][r], v[0][c], u[1][r] * v[1][c]);
  tv_canonical_sign<9>(E);
#pragma unroll
  for (int i = 0; i < 9; ++i) ok = ok && fabs(E[i]) <= 2.0;
  if (!ok) {
#pragma unroll
    for (int i = 0; i < 9; ++i) E[i] = __builtin_nan("");
  }
  return ok ? TV_OK : TV_VOID;
}

// F = K_b^-T E K_a^-1 for undistorted pixel coordinates; ka, kb = (fx, fy, cx, cy)
MCBA_HD void tv_fundamental(const double* E, const double* ka, const double* kb, double* F) {
  double M[9];
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    M[3 * r] = E[3 * r] / ka[0];
    M[3 * r + 1] = E[3 * r + 1] / ka[1];
    M[3 * r + 2] = E[3 * r + 2] - M[3 * r] * ka[2] - M[3 * r + 1] * ka[3];
  }
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    F[c] = M[c] / kb[0];
    F[3 + c] = M[3 + c] / kb[1];
    F[6 + c] = M[6 + c] - F[c] * kb[2] - F[3 + c] * kb[3];
  }
}

// squared Sampson distance in px^2 of the undistorted pixels (xa, ya) <-> (xb, yb): (x_b^T F x_a)^2 over the squared norms of the first two
// components of F x_a and F^T x_b.  A degenerate F gives NaN or inf, which no comparison takes for an inlier.
MCBA_HD double tv_sampson2(const double* F, double xa, double ya, double xb, double yb) {
  const double l0 = fma(F[0], xa, fma(F[1], ya, F[2])), l1 = fma(F[3], xa, fma(F[4], ya, F[5])), l2 = fma(F[6], xa, fma(F[7], ya, F[8]));
  const double m0 = fma(F[0], xb, fma(F[3], yb, F[6])), m1 = fma(F[1], xb, fma(F[4], yb, F[7]));
  const double num = fma(xb, l0, fma(yb, l1, l2));
  const double den = fma(l0, l0, fma(l1, l1, fma(m0, m0, m1 * m1)));
  return num * num * fast_rcp(den);
}
// the truncated cost term and the inlier test of one correspondence (a NaN compares false: not an inlier, the full threshold^2)
MCBA_HD bool tv_inlier(double e2, double t2) { return e2 <= t2; }
MCBA_HD double tv_cost_term(double e2, double t2) { return e2 <= t2 ? e2 : t2; }

// The four (R, t) of E, |t| = 1, det R = +1; Rt (4 x 12): R row-major, then t.  With t0 the unit left null vector of E in canonical sign:
//   0: ([t0]x R = +E, +t0)   1: (the same R, -t0)   2: ([t0]x R = -E, +t0)   3: (the same R, -t0).
// false (everything NaN) when E is not finite or has no two singular values.
MCBA_HD bool tv_candidates(const double* E, double* Rt) {
  double u[2][3], v[2][3], u3[3], v3[3];
  bool ok = tv_top2(E, u, v);
  tv_cross(u[0], u[1], u3);
  tv_cross(v[0], v[1], v3);
  // with U = [u1 u2 u3], V = [v1 v2 v3] (both proper): [u3]x (-u2 v1^T + u1 v2^T + u3 v3^T) = +E, [u3]x (u2 v1^T - u1 v2^T + u3 v3^T) = -E
  double t0[3] = {u3[0], u3[1], u3[2]};
  tv_canonical_sign<3>(t0);
  const double sg = (t0[0] == u3[0] && t0[1] == u3[1] && t0[2] == u3[2]) ? 1.0 : -1.0;
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const double w = fma(u[0][r], v[1][c], -(u[1][r] * v[0][c])), z = u3[r] * v3[c];
      const double Rp = z + sg * w, Rm = z - sg * w;   // [t0]x Rp = +E
      Rt[3 * r + c] = Rp; Rt[12 + 3 * r + c] = Rp;
      Rt[24 + 3 * r + c] = Rm; Rt[36 + 3 * r + c] = Rm;
    }
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    Rt[9 + r] = t0[r]; Rt[21 + r] = -t0[r]; Rt[33 + r] = t0[r]; Rt[45 + r] = -t0[r];
  }
#pragma unroll
  for (int i = 0; i < 48; ++i) ok = ok && fabs(Rt[i]) <= 2.0;
  if (!ok) {
#pragma unroll
    for (int i = 0; i < 48; ++i) Rt[i] = __builtin_nan("");
  }
  return ok;
}

// The two-view point of the normalised coordinates (xa, ya) <-> (xb, yb) under P_a = [I | 0], P_b = [R | t] (Rt: 12 doubles), in camera a's
// frame.  kept: triangulate_pair keeps it (finite); the return value: kept and in front of both cameras.
MCBA_HD bool tv_depths(const double* Rt, double xa, double ya, double xb, double yb, double X[3], bool& kept) {
  const double Pa[12] = {1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0};
  const double Pb[12] = {Rt[0], Rt[1], Rt[2], Rt[9], Rt[3], Rt[4], Rt[5], Rt[10], Rt[6], Rt[7], Rt[8], Rt[11]};
  kept = triangulate_pair(xa, ya, Pa, xb, yb, Pb, true, X[0], X[1], X[2]);
  const double zb = fma(Rt[6], X[0], fma(Rt[7], X[1], fma(Rt[8], X[2], Rt[11])));
  return kept && X[2] > 0.0 && zb > 0.0;
}

// one correspondence through k_tv_prepare: both detections undistorted (pixels) and normalised.  ka, kb = (fx, fy, cx, cy), da, db = (k1 k2 p1 p2 k3)
MCBA_HD void tv_prepare(double ua, double va, double ub, double vb, const double* ka, const double* da, const double* kb, const double* db, int und_iters, double out8[8]) {
  undistort_px(ua, va, ka[0], ka[1], ka[2], ka[3], da, und_iters, out8[0], out8[1]);
  undistort_px(ub, vb, kb[0], kb[1], kb[2], kb[3], db, und_iters, out8[2], out8[3]);
  out8[4] = (out8[0] - ka[2]) / ka[0]; out8[5] = (out8[1] - ka[3]) / ka[1];
  out8[6] = (out8[2] - kb[2]) / kb[0]; out8[7] = (out8[3] - kb[3]) / kb[1];
}

// lowest (cost, index), compared lexicographically
MCBA_HD bool tv_before(double cost_a, int h_a, double cost_b, int h_b) { return cost_a < cost_b || (cost_a == cost_b && h_a < h_b); }

}  // namespace mcba
