// mcba_resect_p3p_math.h -- the per-lane arithmetic of csrc/mcba_resect_p3p.hip: the minimal generator of the resection.
// A sample is three world points and their unit bearings (the normalised coordinates of k_rs_prepare, (x, y, 1) / |.|); Grunert's quartic in
// the depth ratio v = s_2 / s_0 (Haralick, Lee, Ottenberg, Noelle 1994) has up to four real roots, each gives the three depths, the rigid
// transform follows from the orthonormal frames of the two triangles (no SVD), and every candidate is settled by kP3Polish Gauss-Newton
// iterations on its own three points: 6 residuals, 6 unknowns, rs_gauss_newton_step<3> of mcba_resect_math.h.  A sample fills kP3Slots slots of
// the pose table in the order of its roots; the scorer, the winner and the mask of csrc/mcba_resect.hip take that table as it is.
// New: p3_real_roots4 (the real roots of a quartic by the interlacing of its derivatives' roots, every array index a constant), p3_quartic,
// p3_start, p3_roots, p3_candidate.  Conventions as in mcba_resect_math.h.
// The same text is compiled with g++ into tests/hostcheck/p3p_hostcheck.cpp (tests/test_hostcheck_p3p.py).
#pragma once
#include "mcba_resect_math.h"

#if defined(__clang__)
#pragma clang fp contract(off)
#endif

namespace mcba {

constexpr int kP3Sample = 3;     // points of a sample
constexpr int kP3Slots = 4;      // candidates of a sample: the real roots of the quartic
constexpr int kP3Polish = 5;     // Gauss-Newton iterations of a candidate (the share not settled by then)
constexpr int P3_BISECT = 64, P3_NEWTON = 4;   // halvings per bracket, Newton steps on the quartic itself (fp_real_roots10's budget)
// Three points count as collinear when the sine of the angle at the first one is at most this: |d1 x d2| <= P3_AREA_MIN |d1| |d2|.  The
// frames of such a triangle have no defined normal.  (AREA_MIN of tests/p3p_oracle.py.)
constexpr double P3_AREA_MIN = 1e-6;

template <int DEG>
MCBA_HD double p3_horner(const double* c, double t) {
  double v = c[DEG];
#pragma unroll
  for (int k = DEG - 1; k >= 0; --k) v = fma(v, t, c[k]);
  return v;
}

// One level of the interlacing: the roots of the degree-J polynomial c between the J - 1 separators sep (ascending, within -bound .. bound; a
// separator that stands for no root of the level below repeats its neighbour, so its interval is empty).  A sign change of the Horner values
// at the ends of an interval brackets one root: P3_BISECT halvings.  out[i], i = 0 .. J - 1: the root of interval i, or -- none there -- the
// interval's upper end, which keeps out ascending; the return value has bit i set where out[i] is a root.
template <int J>
MCBA_HD unsigned p3_level(const double* c, const double* sep, double bound, double* out) {
  unsigned found = 0;
  double lo = -bound, flo = p3_horner<J>(c, lo);
#pragma unroll
  for (int i = 0; i < J; ++i) {
    const double hi = i < J - 1 ? sep[i] : bound, fhi = p3_horner<J>(c, hi);
    const bool bracket = (flo < 0.0) != (fhi < 0.0);
    const bool neg = flo < 0.0;
    double l = lo, h = hi;
    for (int it = 0; it < P3_BISECT; ++it) {
      const double mid = 0.5 * (l + h);
      const bool same = (p3_horner<J>(c, mid) < 0.0) == neg;
      l = same ? mid : l;
      h = same ? h : mid;
    }
    out[i] = bracket ? 0.5 * (l + h) : hi;
    found |= bracket ? 1u << i : 0u;
    lo = hi;
    flo = fhi;
  }
  return found;
}

// The real roots of a quartic (5 coefficients, ascending), ascending, in roots[0 .. n - 1]; n is returned, 0 where the Cauchy bound
// 1 + max |a_k| / |a_4| is not finite (a vanishing leading coefficient, a NaN).  The roots of p''' separate those of p'', those of p'' the ones
// of p', those of p' the ones of p; P3_NEWTON Newton steps close the last level, each kept only where it lowers |p|.  Only signs of Horner
// values decide, every trip count is fixed, and every array index is a constant: the arrays are registers.
MCBA_HD int p3_real_roots4(const double* a, double* roots) {
  double mx = 0.0;
#pragma unroll
  for (int k = 0; k < 4; ++k) mx = fabs(a[k]) > mx ? fabs(a[k]) : mx;
  const double bound = 1.0 + mx / fabs(a[4]);
#pragma unroll
  for (int i = 0; i < 4; ++i) roots[i] = 0.0;
  if (!(bound <= 1e300)) return 0;
  const double d3[2] = {6.0 * a[3], 24.0 * a[4]}, d2[3] = {2.0 * a[2], 6.0 * a[3], 12.0 * a[4]}, d1[4] = {a[1], 2.0 * a[2], 3.0 * a[3], 4.0 * a[4]};
  double s1[1], s2[2], s3[3], s4[4];
  p3_level<1>(d3, s1, bound, s1);   // (no separators are read at level 1)
  p3_level<2>(d2, s1, bound, s2);
  p3_level<3>(d1, s2, bound, s3);
  const unsigned found = p3_level<4>(a, s3, bound, s4);
  int n = 0;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    double z = s4[i], fz = p3_horner<4>(a, z);
    for (int it = 0; it < P3_NEWTON; ++it) {
      const double zn = z - fz / p3_horner<3>(d1, z), fn = p3_horner<4>(a, zn);
      const bool take = fabs(fn) < fabs(fz);
      z = take ? zn : z;
      fz = take ? fn : fz;
    }
    const bool is = (found >> i & 1u) != 0;
#pragma unroll
    for (int s = 0; s < 4; ++s) roots[s] = is && n == s ? z : roots[s];
    n += is ? 1 : 0;
  }
  return n;
}

MCBA_HD double p3_dot(const double* a, const double* b) { return fma(a[0], b[0], fma(a[1], b[1], a[2] * b[2])); }

// |(A_1 - A_0) x (A_2 - A_0)| <= P3_AREA_MIN |A_1 - A_0| |A_2 - A_0| (or something is NaN); A: 3 x 3, a point per row
MCBA_HD bool p3_collinear(const double* A) {
  const double d1[3] = {A[3] - A[0], A[4] - A[1], A[5] - A[2]}, d2[3] = {A[6] - A[0], A[7] - A[1], A[8] - A[2]};
  double n[3];
  tv_cross(d1, d2, n);
  return !(p3_dot(n, n) > P3_AREA_MIN * P3_AREA_MIN * p3_dot(d1, d1) * p3_dot(d2, d2));
}

// Grunert's quartic A_0 + A_1 v + .. + A_4 v^4 of the world points X (3 x 3) and the unit bearings j (3 x 3): a = |X_1 X_2|, b = |X_0 X_2|,
// c = |X_0 X_1|, cos alpha = j_1 . j_2, cos beta = j_0 . j_2, cos gamma = j_0 . j_1.  aux: (a^2 - c^2) / b^2, the three cosines, b^2 -- what
// p3_start needs beside the root.
MCBA_HD void p3_quartic(const double* X, const double* j, double* A, double* aux) {
  const double e12[3] = {X[3] - X[6], X[4] - X[7], X[5] - X[8]}, e02[3] = {X[0] - X[6], X[1] - X[7], X[2] - X[8]}, e01[3] = {X[0] - X[3], X[1] - X[4], X[2] - X[5]};
  const double a2 = p3_dot(e12, e12), b2 = p3_dot(e02, e02), c2 = p3_dot(e01, e01);
  const double ca = p3_dot(j + 3, j + 6), cb = p3_dot(j, j + 6), cg = p3_dot(j, j + 3);
  const double p = (a2 - c2) / b2, q = (a2 + c2) / b2, ra = a2 / b2, rc = c2 / b2;
  A[4] = (p - 1.0) * (p - 1.0) - 4.0 * rc * ca * ca;
  A[3] = 4.0 * (p * (1.0 - p) * cb - (1.0 - q) * ca * cg + 2.0 * rc * ca * ca * cb);
  A[2] = 2.0 * (p * p - 1.0 + 2.0 * p * p * cb * cb + 2.0 * (1.0 - rc) * ca * ca - 4.0 * q * ca * cb * cg + 2.0 * (1.0 - ra) * cg * cg);
  A[1] = 4.0 * (-p * (1.0 + p) * cb + 2.0 * ra * cg * cg * cb - (1.0 - q) * ca * cg);
  A[0] = (1.0 + p) * (1.0 + p) - 4.0 * ra * cg * cg;
  aux[0] = p; aux[1] = ca; aux[2] = cb; aux[3] = cg; aux[4] = b2;
}

// the orthonormal frame of a triangle (3 x 3, a point per row), a basis vector per row of e: e_1 along 0 -> 1, e_3 the normal, e_2 = e_3 x e_1
MCBA_HD void p3_frame(const double* A, double* e) {
  const double d1[3] = {A[3] - A[0], A[4] - A[1], A[5] - A[2]}, d2[3] = {A[6] - A[0], A[7] - A[1], A[8] - A[2]};
  const double n1 = sqrt(p3_dot(d1, d1));
#pragma unroll
  for (int i = 0; i < 3; ++i) e[i] = d1[i] / n1;
  double n[3];
  tv_cross(e, d2, n);
  const double n3 = sqrt(p3_dot(n, n));
#pragma unroll
  for (int i = 0; i < 3; ++i) e[6 + i] = n[i] / n3;
  tv_cross(e + 6, e, e + 3);
}

// The pose of the root v: u = s_1 / s_0 from v, s_0 = b / sqrt(1 + v^2 - 2 v cos beta), the camera points Y_i = s_i j_i, R = F_Y F_X^T,
// t = Y_0 - R X_0.  false: a depth ratio is not positive (or NaN).  The pose may still be non-finite; p3_sample looks.
MCBA_HD bool p3_start(const double* X, const double* j, const double* aux, double v, double* pose) {
  const double p = aux[0], ca = aux[1], cb = aux[2], cg = aux[3], b2 = aux[4];
  const double u = ((p - 1.0) * v * v - 2.0 * p * cb * v + 1.0 + p) / (2.0 * (cg - v * ca));
  const double s0 = sqrt(b2 / (1.0 + v * v - 2.0 * v * cb));
  const double s[3] = {s0, u * s0, v * s0};
  double Y[9], ex[9], ey[9];
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int k = 0; k < 3; ++k) Y[3 * i + k] = s[i] * j[3 * i + k];
  p3_frame(X, ex);
  p3_frame(Y, ey);
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int c = 0; c < 3; ++c) pose[3 * r + c] = fma(ey[r], ex[c], fma(ey[3 + r], ex[3 + c], ey[6 + r] * ex[6 + c]));
#pragma unroll
  for (int r = 0; r < 3; ++r) pose[9 + r] = Y[r] - p3_dot(pose + 3 * r, X);
  return u > 0.0 && v > 0.0;
}

// What the candidates of a sample share: the bearings, p3_start's quantities, the real roots (nr of them, ascending), whether the world
// points or the bearings -- as points (x, y, 1) of the image plane -- are collinear
struct P3Roots {
  double j[9], aux[5], roots[kP3Slots];
  int nr;
  bool flat;
};

// X (3 x 3) world points, x (3 x 2) normalised coordinates
MCBA_HD void p3_roots(const double* X, const double* x, P3Roots& s) {
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    const double n = sqrt(fma(x[2 * i], x[2 * i], fma(x[2 * i + 1], x[2 * i + 1], 1.0)));
    s.j[3 * i] = x[2 * i] / n; s.j[3 * i + 1] = x[2 * i + 1] / n; s.j[3 * i + 2] = 1.0 / n;
  }
  const double b[9] = {x[0], x[1], 1.0, x[2], x[3], 1.0, x[4], x[5], 1.0};   // the image points: collinear <=> the camera centre is in the triangle's plane
  s.flat = p3_collinear(X) || p3_collinear(b);
  double A[5];
  p3_quartic(X, s.j, A, s.aux);
  s.nr = p3_real_roots4(A, s.roots);
}

// Slot k of a sample: the candidate of the k-th real root, ascending, settled by exactly kP3Polish Gauss-Newton iterations on the three
// points.  RS_VOID (pose all NaN) when there is no such root, when the world points or the bearings are collinear (p3_collinear), when a depth
// ratio is not positive, when anything is not finite or when a sample point ends with z <= 0 after the polish.  step6: the last polish step.
// No de-duplication: equal candidates cost the same, and the lower slot wins.
MCBA_HD int p3_candidate(const double* X, const double* x, const P3Roots& s, int k, double* pose, double* step6) {
  bool ok = p3_start(X, s.j, s.aux, s.roots[k], pose) && k < s.nr && !s.flat;
#pragma unroll
  for (int i = 0; i < 12; ++i) ok = ok && rs_finite(pose[i]);
#pragma unroll
  for (int i = 0; i < 6; ++i) step6[i] = 0.0;
  for (int it = 0; it < kP3Polish; ++it) rs_gauss_newton_step<kP3Sample>(X, x, pose, step6);
#pragma unroll
  for (int i = 0; i < 12; ++i) ok = ok && rs_finite(pose[i]);
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    double Xc[3];
    rs_camera_point(pose, X + 3 * i, Xc);
    ok = ok && Xc[2] > 0.0;
  }
  if (!ok) {
#pragma unroll
    for (int i = 0; i < 12; ++i) pose[i] = __builtin_nan("");
  }
  return ok ? RS_OK : RS_VOID;
}

}  // namespace mcba
