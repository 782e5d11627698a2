// mcba_fivepoint_math.h -- the per-lane arithmetic of csrc/mcba_fivepoint.hip: the essential matrices -- up to ten -- of
// five calibrated correspondences, the minimal hypothesis of the two-view RANSAC.  Nister's route: the 4-dimensional null space of the 5 x 9
// epipolar matrix, E = x X + y Y + z Z + W, the ten cubic constraints det E = 0 and 2 E E^T E - tr(E E^T) E = 0 as a 10 x 20 matrix, Gauss-Jordan
// on its cubic block, the degree-10 polynomial in z, its real roots, and per root a Gauss-Newton polish on the ten cubics themselves; then
// the same with x for the hidden variable, and the union of the two passes (fp_candidates says why).
// Every loop has a fixed trip count: two calls return the same bits.
// Reused, not restated: tv_top2, tv_canonical_sign of mcba_twoview_math.h (the candidates leave in tv_essential's convention).
// The same text is compiled with g++ into tests/hostcheck/fivepoint_hostcheck.cpp (tests/test_hostcheck_fivepoint.py).
#pragma once
#include "mcba_twoview_math.h"

#if defined(__clang__)
#pragma clang fp contract(off)
#endif

namespace mcba {

constexpr int FP_SAMPLE = 5, FP_SLOTS = 10;
// Floors below which a sample is void (DESIGN.md section 8f-17 has the derivation).  sigma_5 / sigma_1 of the 5 x 9 matrix: the smallest met
// over the 5760 samples of the test cases is 5.5e-5, where the candidates still agree with the oracle to their bound; the floor is 2.7
// decades below it and nine above where the null space stops being one (sigma_5 / sigma_1 ~ EPS).  Pivot of the elimination over the
// largest entry of the cubic block: the smallest met is 3.2e-7; the floor is 2.5 decades below it.
constexpr double FP_RANK_MIN = 1e-7, FP_PIVOT_MIN = 1e-9;
constexpr int FP_BISECT = 64, FP_NEWTON = 4, FP_POLISH = 6;
// A polished point is a solution when the residual of the ten cubics is below FP_RESIDUAL_MAX of the magnitude of their terms (a converged one
// sits at 1e-13 and below, a stalled one at 1e-2 and above); two are the same solution within FP_SAME (1 + its largest coordinate).
constexpr double FP_RESIDUAL_MAX = 1e-6, FP_SAME = 1e-6;

// the work space of one sample; the caller places it (the kernel: scratch -- the arrays are indexed at run time)
struct FpWork {
  double M[200];    // the 10 x 20 constraint matrix, reduced in place
  double M0[200];   // ... as it was: the polish evaluates the cubics themselves
  double basis[4][9];   // X, Y, Z, W
};

// ---------------------------------------------------------------- null space
// Householder QR of A^T (9 x 5; at[k] = column k = row k of A): the last four columns of Q span the null space of A; R has A's singular values.
// sigma_5 / sigma_1 by a one-sided Jacobi on R (fixed sweeps).  N: four orthonormal vectors of length 9.
MCBA_HD double fp_null_space(double (&at)[5][9], double (&N)[4][9]) {
  double R[5][5];   // R[c][r]: column c of R
#pragma unroll
  for (int c = 0; c < 5; ++c)
#pragma unroll
    for (int r = 0; r < 5; ++r) R[c][r] = 0.0;
  for (int k = 0; k < 5; ++k) {
    double n2 = 0.0;
    for (int r = k; r < 9; ++r) n2 = fma(at[k][r], at[k][r], n2);
    const double nrm = sqrt(n2), alpha = at[k][k] > 0.0 ? -nrm : nrm;
    at[k][k] -= alpha;                       // v = x - alpha e_1, kept in place of the column (rows k .. 8)
    const double vv = fma(at[k][k], at[k][k], n2 - (at[k][k] + alpha) * (at[k][k] + alpha));
    const double beta = vv > 0.0 ? 2.0 / vv : 0.0;
    for (int c = k + 1; c < 5; ++c) {
      double d = 0.0;
      for (int r = k; r < 9; ++r) d = fma(at[k][r], at[c][r], d);
      d *= beta;
      for (int r = k; r < 9; ++r) at[c][r] = fma(-d, at[k][r], at[c][r]);
    }
    R[k][k] = alpha;
    for (int c = k + 1; c < 5; ++c) R[c][k] = at[c][k];
  }
  for (int j = 0; j < 4; ++j) {
    double q[9];
    for (int r = 0; r < 9; ++r) q[r] = r == 5 + j ? 1.0 : 0.0;
    for (int k = 4; k >= 0; --k) {
      double vv = 0.0, d = 0.0;
      for (int r = k; r < 9; ++r) { vv = fma(at[k][r], at[k][r], vv); d = fma(at[k][r], q[r], d); }
      d *= vv > 0.0 ? 2.0 / vv : 0.0;
      for (int r = k; r < 9; ++r) q[r] = fma(-d, at[k][r], q[r]);
    }
    for (int r = 0; r < 9; ++r) N[j][r] = q[r];
  }
  for (int sweep = 0; sweep < 10; ++sweep)
    for (int p = 0; p < 4; ++p)
      for (int q = p + 1; q < 5; ++q) {
        double alpha = 0.0, beta = 0.0, gamma = 0.0;
        for (int k = 0; k < 5; ++k) { alpha = fma(R[p][k], R[p][k], alpha); beta = fma(R[q][k], R[q][k], beta); gamma = fma(R[p][k], R[q][k], gamma); }
        const bool rot = gamma * gamma > 1e-32 * alpha * beta;
        const double g = rot ? gamma : 1.0;
        const double zeta = (beta - alpha) / (2.0 * g);
        double t = 1.0 / (fabs(zeta) + sqrt(fma(zeta, zeta, 1.0)));
        t = zeta < 0.0 ? -t : t;
        t = rot ? t : 0.0;
        const double c = 1.0 / sqrt(fma(t, t, 1.0)), s = c * t;
        for (int k = 0; k < 5; ++k) {
          const double ap = R[p][k], aq = R[q][k];
          R[p][k] = fma(c, ap, -(s * aq));
          R[q][k] = fma(s, ap, c * aq);
        }
      }
  double lo = __builtin_inf(), hi = 0.0;
  for (int c = 0; c < 5; ++c) {
    double n2 = 0.0;
    for (int k = 0; k < 5; ++k) n2 = fma(R[c][k], R[c][k], n2);
    lo = n2 < lo ? n2 : lo;
    hi = n2 > hi ? n2 : hi;
  }
  return hi > 0.0 ? sqrt(lo / hi) : 0.0;   // (NaN: compares false against the floor's `>=`)
}

// The canonical basis of the subspace N spans: W, Z, Y, X = Gram-Schmidt (twice through) of the subspace's coordinates of the entries E33, E32,
// E31, E23.  Only the subspace matters to E; the roots depend on the basis, and "ascending z" is an order only once the basis is fixed.
MCBA_HD void fp_canonical_basis(const double (&N)[4][9], double (&basis)[4][9]) {
  double q[4][4];
  for (int j = 0; j < 4; ++j) {
    double c[4];
    for (int i = 0; i < 4; ++i) c[i] = N[i][8 - j];
    for (int pass = 0; pass < 2; ++pass)
      for (int k = 0; k < j; ++k) {
        double d = 0.0;
        for (int i = 0; i < 4; ++i) d = fma(q[k][i], c[i], d);
        for (int i = 0; i < 4; ++i) c[i] = fma(-d, q[k][i], c[i]);
      }
    double n2 = 0.0;
    for (int i = 0; i < 4; ++i) n2 = fma(c[i], c[i], n2);
    const double inv = 1.0 / sqrt(n2);
    for (int i = 0; i < 4; ++i) q[j][i] = c[i] * inv;
  }
  for (int j = 0; j < 4; ++j)
    for (int r = 0; r < 9; ++r) {
      double s = 0.0;
      for (int i = 0; i < 4; ++i) s = fma(q[j][i], N[i][r], s);
      basis[3 - j][r] = s;
    }
}

// ---------------------------------------------------------------- the ten cubics
// Polynomials in the homogeneous variables (x, y, z, 1) = 0 .. 3: a linear one is 4 numbers, a quadratic one 10 (pairs i <= j in the order of
// kQ2), a cubic one a row of the constraint matrix in Nister's column order
//   x^3 y^3 x^2y xy^2 x^2z x^2 y^2z y^2 xyz xy | xz^2 xz x | yz^2 yz y | z^3 z^2 z 1.
MCBA_HD void fp_mul11(const double* a, const double* b, double s, double* out10) {
  const int kQ2[4][4] = {{0, 1, 2, 3}, {1, 4, 5, 6}, {2, 5, 7, 8}, {3, 6, 8, 9}};
  for (int i = 0; i < 4; ++i)
    for (int j = 0; j < 4; ++j) out10[kQ2[i][j]] = fma(s * a[i], b[j], out10[kQ2[i][j]]);
}
MCBA_HD void fp_mul21(const double* a10, const double* b, double* row20) {
  const int kT3[10][4] = {{0, 2, 4, 5}, {2, 3, 8, 9}, {4, 8, 10, 11}, {5, 9, 11, 12}, {3, 1, 6, 7}, {8, 6, 13, 14}, {9, 7, 14, 15}, {10, 13, 16, 17}, {11, 14, 17, 18}, {12, 15, 18, 19}};
  for (int q = 0; q < 10; ++q)
    for (int v = 0; v < 4; ++v) row20[kT3[q][v]] = fma(a10[q], b[v], row20[kT3[q][v]]);
}

// M (10 x 20, row-major): row 0 = det E, row 1 + 3 i + j = (2 E E^T E - tr(E E^T) E)_ij
MCBA_HD void fp_constraints(const double (&basis)[4][9], double* M) {
  double lin[9][4];
  for (int e = 0; e < 9; ++e)
    for (int v = 0; v < 4; ++v) lin[e][v] = basis[v][e];
  for (int i = 0; i < 200; ++i) M[i] = 0.0;
  double G[3][3][10], tr[10];
  for (int i = 0; i < 3; ++i)
    for (int j = i; j < 3; ++j) {
      for (int m = 0; m < 10; ++m) G[i][j][m] = 0.0;
      for (int k = 0; k < 3; ++k) fp_mul11(lin[3 * i + k], lin[3 * j + k], 1.0, G[i][j]);
    }
  for (int m = 0; m < 10; ++m) tr[m] = G[0][0][m] + G[1][1][m] + G[2][2][m];
  for (int i = 0; i < 3; ++i)
    for (int j = i; j < 3; ++j)
      for (int m = 0; m < 10; ++m) {
        const double l = 2.0 * G[i][j][m] - (i == j ? tr[m] : 0.0);   // Lambda = 2 E E^T - tr I
        G[i][j][m] = l;
        G[j][i][m] = l;
      }
  double minor[10];
  const int ma[3] = {1, 2, 0}, mb[3] = {2, 0, 1};
  for (int c = 0; c < 3; ++c) {    // det E along the last row: minor c of the first two rows
    for (int m = 0; m < 10; ++m) minor[m] = 0.0;
    fp_mul11(lin[ma[c]], lin[3 + mb[c]], 1.0, minor);
    fp_mul11(lin[mb[c]], lin[3 + ma[c]], -1.0, minor);
    fp_mul21(minor, lin[6 + c], M);
  }
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j)
      for (int k = 0; k < 3; ++k) fp_mul21(G[i][k], lin[3 * k + j], M + 20 * (1 + 3 * i + j));
}

// Gauss-Jordan with partial pivoting on the cubic block (columns 0 .. 9) of M.  Returns the smallest |pivot| over the largest |entry| of the
// block as it came (0 when that is not a positive finite number).
MCBA_HD double fp_gauss_jordan(double* M) {
  double mx = 0.0;
  for (int r = 0; r < 10; ++r)
    for (int c = 0; c < 10; ++c) mx = fabs(M[20 * r + c]) > mx ? fabs(M[20 * r + c]) : mx;
  double worst = __builtin_inf();
  for (int k = 0; k < 10; ++k) {
    int p = k;
    for (int r = k + 1; r < 10; ++r) p = fabs(M[20 * r + k]) > fabs(M[20 * p + k]) ? r : p;
    for (int c = 0; c < 20; ++c) { const double t = M[20 * k + c]; M[20 * k + c] = M[20 * p + c]; M[20 * p + c] = t; }
    const double piv = M[20 * k + k];
    worst = fabs(piv) < worst ? fabs(piv) : worst;
    const double inv = 1.0 / piv;
    for (int c = 0; c < 20; ++c) M[20 * k + c] *= inv;
    for (int r = 0; r < 10; ++r) {
      if (r == k) continue;
      const double f = M[20 * r + k];
      for (int c = 0; c < 20; ++c) M[20 * r + c] = fma(-f, M[20 * k + c], M[20 * r + c]);
    }
  }
  return mx > 0.0 && mx <= 1.7976931348623157e308 && worst <= 1.7976931348623157e308 ? worst / mx : 0.0;
}

// ---------------------------------------------------------------- the polynomial in z
// out (na + nb - 1 coefficients, ascending) += s a b
MCBA_HD void fp_polymul(const double* a, int na, const double* b, int nb, double s, double* out) {
  for (int i = 0; i < na; ++i)
    for (int j = 0; j < nb; ++j) out[i + j] = fma(s * a[i], b[j], out[i + j]);
}
MCBA_HD double fp_horner(const double* c, int deg, double t) {
  double v = c[deg];
  for (int k = deg - 1; k >= 0; --k) v = fma(v, t, c[k]);
  return v;
}

// B (3 x 3 polynomials, ascending coefficients, 5 slots each; degrees 3, 3, 4) of the reduced M: rows (x^2z) - z (x^2), (y^2z) - z (y^2),
// (xyz) - z (xy), columns the coefficients of x, y and 1
MCBA_HD void fp_hidden_z(const double* M, double (&B)[3][3][5]) {
  for (int i = 0; i < 3; ++i) {
    const double* e = M + 20 * (4 + 2 * i) + 10;
    const double* f = M + 20 * (5 + 2 * i) + 10;
    for (int g = 0; g < 2; ++g) {   // x: columns 0 .. 2 (z^2, z, 1); y: 3 .. 5
      B[i][g][0] = e[3 * g + 2]; B[i][g][1] = e[3 * g + 1] - f[3 * g + 2]; B[i][g][2] = e[3 * g] - f[3 * g + 1]; B[i][g][3] = -f[3 * g]; B[i][g][4] = 0.0;
    }
    B[i][2][0] = e[9]; B[i][2][1] = e[8] - f[9]; B[i][2][2] = e[7] - f[8]; B[i][2][3] = e[6] - f[7]; B[i][2][4] = -f[6];
  }
}

// det B: 11 coefficients, ascending
MCBA_HD void fp_det_poly(const double (&B)[3][3][5], double* det) {
  double p1[8], p2[8], p3[7];
  for (int i = 0; i < 8; ++i) { p1[i] = 0.0; p2[i] = 0.0; }
  for (int i = 0; i < 7; ++i) p3[i] = 0.0;
  for (int i = 0; i < 11; ++i) det[i] = 0.0;
  fp_polymul(B[0][1], 4, B[1][2], 5, 1.0, p1); fp_polymul(B[0][2], 5, B[1][1], 4, -1.0, p1);
  fp_polymul(B[0][2], 5, B[1][0], 4, 1.0, p2); fp_polymul(B[0][0], 4, B[1][2], 5, -1.0, p2);
  fp_polymul(B[0][0], 4, B[1][1], 4, 1.0, p3); fp_polymul(B[0][1], 4, B[1][0], 4, -1.0, p3);
  fp_polymul(p1, 8, B[2][0], 4, 1.0, det); fp_polymul(p2, 8, B[2][1], 4, 1.0, det); fp_polymul(p3, 7, B[2][2], 5, 1.0, det);
}

// The real roots of a degree-10 polynomial (11 coefficients, ascending), ascending, by the interlacing of the derivatives' roots: the roots of
// p^(m) separate those of p^(m-1), so every level is a sign test and FP_BISECT halvings per interval between the level below's roots and the
// Cauchy bound; FP_NEWTON Newton steps close the last level (each kept only where it lowers |p|).  Only signs of Horner values decide, and every
// trip count is fixed.  Returns the number of roots, or -1 where the bound is not finite (a vanishing leading coefficient, a NaN).
MCBA_HD int fp_real_roots10(const double* a, double* roots) {
  double mx = 0.0;
  for (int k = 0; k < 10; ++k) mx = fabs(a[k]) > mx ? fabs(a[k]) : mx;
  const double bound = 1.0 + mx / fabs(a[10]);
  if (!(bound <= 1e300)) return -1;
  double sep[11], nxt[11], c[11];
  int ns = 0;
  for (int j = 1; j <= 10; ++j) {
    const int m = 10 - j;
    for (int k = 0; k <= j; ++k) {
      double f = 1.0;
      for (int i = 0; i < m; ++i) f *= (double)(k + m - i);
      c[k] = a[k + m] * f;
    }
    int nn = 0;
    double lo = -bound, flo = fp_horner(c, j, lo);
    for (int i = 0; i <= ns; ++i) {
      const double hi = i < ns ? sep[i] : bound, fhi = fp_horner(c, j, hi);
      if ((flo < 0.0) != (fhi < 0.0)) {
        double l = lo, h = hi;
        const bool neg = flo < 0.0;
        for (int it = 0; it < FP_BISECT; ++it) {
          const double mid = 0.5 * (l + h);
          const bool same = (fp_horner(c, j, mid) < 0.0) == neg;
          l = same ? mid : l;
          h = same ? h : mid;
        }
        nxt[nn++] = 0.5 * (l + h);
      }
      lo = hi;
      flo = fhi;
    }
    ns = nn;
    for (int i = 0; i < nn; ++i) sep[i] = nxt[i];
  }
  double d[10];
  for (int k = 0; k < 10; ++k) d[k] = a[k + 1] * (double)(k + 1);
  for (int i = 0; i < ns; ++i) {
    double z = sep[i], fz = fp_horner(a, 10, z);
    for (int it = 0; it < FP_NEWTON; ++it) {
      const double zn = z - fz / fp_horner(d, 9, z), fn = fp_horner(a, 10, zn);
      const bool take = fabs(fn) < fabs(fz);
      z = take ? zn : z;
      fz = take ? fn : fz;
    }
    roots[i] = z;
  }
  return ns;
}

// ---------------------------------------------------------------- per root
// (x, y) at a root z: the null vector of B(z) is the largest of the three cross products of its rows
MCBA_HD void fp_xy_of(const double (&B)[3][3][5], double z, double& x, double& y) {
  double b[3][3], best[3] = {0.0, 0.0, 0.0}, bn = -1.0;
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) b[i][j] = fp_horner(B[i][j], j == 2 ? 4 : 3, z);
  const int ra[3] = {0, 0, 1}, rb[3] = {1, 2, 2};
  for (int k = 0; k < 3; ++k) {
    double n[3];
    tv_cross(b[ra[k]], b[rb[k]], n);
    const double n2 = fma(n[0], n[0], fma(n[1], n[1], n[2] * n[2]));
    const bool take = n2 > bn;
    bn = take ? n2 : bn;
    for (int i = 0; i < 3; ++i) best[i] = take ? n[i] : best[i];
  }
  x = best[0] / best[2];
  y = best[1] / best[2];
}

// the ten cubics M0 (10 x 20) at v = (x, y, z): the residual's squared norm, J^T J (6: xx xy xz yy yz zz) and J^T r; scale2: the squared norm
// of the sums of the terms' magnitudes, what the residual is small against
MCBA_HD double fp_cubics_at(const double* M0, const double* v, double* JtJ, double* Jtr, double& scale2) {
  const int ex[3][20] = {{3, 0, 2, 1, 2, 2, 0, 0, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0}, {0, 3, 1, 2, 0, 0, 2, 2, 1, 1, 0, 0, 0, 1, 1, 1, 0, 0, 0, 0}, {0, 0, 0, 0, 1, 0, 1, 0, 1, 0, 2, 1, 0, 2, 1, 0, 3, 2, 1, 0}};
  double pw[3][4], dp[3][4];
  for (int a = 0; a < 3; ++a) {
    pw[a][0] = 1.0; pw[a][1] = v[a]; pw[a][2] = v[a] * v[a]; pw[a][3] = pw[a][2] * v[a];
    dp[a][0] = 0.0; dp[a][1] = 1.0; dp[a][2] = 2.0 * v[a]; dp[a][3] = 3.0 * pw[a][2];
  }
  double mono[20], dm[3][20];
  for (int k = 0; k < 20; ++k) {
    const double px = pw[0][ex[0][k]], py = pw[1][ex[1][k]], pz = pw[2][ex[2][k]];
    mono[k] = px * py * pz;
    dm[0][k] = dp[0][ex[0][k]] * py * pz; dm[1][k] = px * dp[1][ex[1][k]] * pz; dm[2][k] = px * py * dp[2][ex[2][k]];
  }
  for (int i = 0; i < 6; ++i) JtJ[i] = 0.0;
  for (int i = 0; i < 3; ++i) Jtr[i] = 0.0;
  double r2 = 0.0;
  scale2 = 0.0;
  for (int r = 0; r < 10; ++r) {
    double res = 0.0, mag = 0.0, j[3] = {0.0, 0.0, 0.0};
    for (int k = 0; k < 20; ++k) {
      const double m = M0[20 * r + k];
      res = fma(m, mono[k], res);
      mag += fabs(m * mono[k]);
      j[0] = fma(m, dm[0][k], j[0]); j[1] = fma(m, dm[1][k], j[1]); j[2] = fma(m, dm[2][k], j[2]);
    }
    r2 = fma(res, res, r2);
    scale2 = fma(mag, mag, scale2);
    JtJ[0] = fma(j[0], j[0], JtJ[0]); JtJ[1] = fma(j[0], j[1], JtJ[1]); JtJ[2] = fma(j[0], j[2], JtJ[2]);
    JtJ[3] = fma(j[1], j[1], JtJ[3]); JtJ[4] = fma(j[1], j[2], JtJ[4]); JtJ[5] = fma(j[2], j[2], JtJ[5]);
    Jtr[0] = fma(j[0], res, Jtr[0]); Jtr[1] = fma(j[1], res, Jtr[1]); Jtr[2] = fma(j[2], res, Jtr[2]);
  }
  return r2;
}

// FP_POLISH Gauss-Newton steps on the ten cubics from a root of the univariate polynomial; a step that does not lower the residual is not
// taken, and nothing moves after it.  Two solutions with nearly the same z are an ill-conditioned pair of roots of the polynomial in z and a
// well-conditioned pair of solutions of the system: this is what brings the candidates to the conditioning of the problem.  Returns the
// residual over its scale (fp_cubics_at), squared: a point where the steps stalled away from a solution shows there.
MCBA_HD double fp_polish(const double* M0, double* v) {
  double A[6], g[3], sc2, sc2n;
  double r2 = fp_cubics_at(M0, v, A, g, sc2);
  bool live = true;
  for (int it = 0; it < FP_POLISH; ++it) {
    // A^-1 g by the adjugate of the symmetric 3 x 3
    const double c00 = fma(A[3], A[5], -(A[4] * A[4])), c01 = fma(A[2], A[4], -(A[1] * A[5])), c02 = fma(A[1], A[4], -(A[2] * A[3]));
    const double c11 = fma(A[0], A[5], -(A[2] * A[2])), c12 = fma(A[1], A[2], -(A[0] * A[4])), c22 = fma(A[0], A[3], -(A[1] * A[1]));
    const double det = fma(A[0], c00, fma(A[1], c01, A[2] * c02));
    const double w[3] = {v[0] - fma(c00, g[0], fma(c01, g[1], c02 * g[2])) / det, v[1] - fma(c01, g[0], fma(c11, g[1], c12 * g[2])) / det,
                         v[2] - fma(c02, g[0], fma(c12, g[1], c22 * g[2])) / det};
    double A2[6], g2[3];
    const double r2n = fp_cubics_at(M0, w, A2, g2, sc2n);
    live = live && r2n < r2;   // (NaN: not taken)
    sc2 = live ? sc2n : sc2;
    for (int i = 0; i < 3; ++i) { v[i] = live ? w[i] : v[i]; g[i] = live ? g2[i] : g[i]; }
    for (int i = 0; i < 6; ++i) A[i] = live ? A2[i] : A[i];
    r2 = live ? r2n : r2;
  }
  return r2 / sc2;
}

// ---------------------------------------------------------------- the sample
// The candidates of the correspondences xa[k] <-> xb[k] (5 x 2 each, normalised coordinates): E10 (10 x 9) and status10 (10), the real
// solutions in ascending order of the polynomial's root in the leading slots -- projected onto singular values (1, 1, 0), |E|_F = sqrt 2,
// sign-canonical, TV_OK -- the others TV_VOID with E all NaN.  Returns the number of live slots; 0 for a void sample: something not finite,
// sigma_5 / sigma_1 < FP_RANK_MIN, a pivot below FP_PIVOT_MIN.  diag (2, or NULL): sigma_5 / sigma_1 and the pivot ratio.
MCBA_HD int fp_candidates(const double* xa, const double* xb, FpWork& w, double* E10, int* status10, double* diag) {
  for (int i = 0; i < 90; ++i) E10[i] = __builtin_nan("");
  for (int i = 0; i < FP_SLOTS; ++i) status10[i] = TV_VOID;
  double at[5][9], N[4][9];
  for (int k = 0; k < 5; ++k) {
    const double a[3] = {xa[2 * k], xa[2 * k + 1], 1.0}, b[3] = {xb[2 * k], xb[2 * k + 1], 1.0};
    for (int i = 0; i < 3; ++i)
      for (int j = 0; j < 3; ++j) at[k][3 * i + j] = b[i] * a[j];
  }
  const double ratio = fp_null_space(at, N);
  if (diag) { diag[0] = ratio; diag[1] = 0.0; }
  if (!(ratio >= FP_RANK_MIN)) return 0;
  fp_canonical_basis(N, w.basis);
  // Two passes, the hidden variable z, then x (the basis with X and Z exchanged): solutions whose z nearly coincide are a cluster of roots
  // of the polynomial in z, which the polish cannot always pull apart again, and are far apart in x.  The union, in ascending z.
  double sol[FP_SLOTS][3];
  int ns = 0;
  for (int pass = 0; pass < 2; ++pass) {
    double bp[4][9];
    for (int e = 0; e < 9; ++e) { bp[0][e] = w.basis[pass ? 2 : 0][e]; bp[1][e] = w.basis[1][e]; bp[2][e] = w.basis[pass ? 0 : 2][e]; bp[3][e] = w.basis[3][e]; }
    fp_constraints(bp, w.M);
    for (int i = 0; i < 200; ++i) w.M0[i] = w.M[i];
    const double piv = fp_gauss_jordan(w.M);
    if (pass == 0) {
      if (diag) diag[1] = piv;
      if (!(piv >= FP_PIVOT_MIN)) return 0;
    } else if (!(piv >= FP_PIVOT_MIN)) continue;
    double B[3][3][5], det[11], roots[10];
    fp_hidden_z(w.M, B);
    fp_det_poly(B, det);
    const int nr = fp_real_roots10(det, roots);
    for (int i = 0; i < nr; ++i) {
      double v[3];
      v[2] = roots[i];
      fp_xy_of(B, roots[i], v[0], v[1]);
      const double rel2 = fp_polish(w.M0, v);
      if (pass) { const double t = v[0]; v[0] = v[2]; v[2] = t; }
      if (!(rel2 <= FP_RESIDUAL_MAX * FP_RESIDUAL_MAX) || !(fabs(v[0]) + fabs(v[1]) + fabs(v[2]) <= 1e300)) continue;
      bool known = false;
      for (int k = 0; k < ns; ++k) {
        const double d = fmax(fabs(v[0] - sol[k][0]), fmax(fabs(v[1] - sol[k][1]), fabs(v[2] - sol[k][2])));
        known = known || d <= FP_SAME * (1.0 + fmax(fabs(sol[k][0]), fmax(fabs(sol[k][1]), fabs(sol[k][2]))));
      }
      if (known || ns == FP_SLOTS) continue;
      int at_ = ns;
      while (at_ > 0 && sol[at_ - 1][2] > v[2]) { for (int c = 0; c < 3; ++c) sol[at_][c] = sol[at_ - 1][c]; --at_; }
      for (int c = 0; c < 3; ++c) sol[at_][c] = v[c];
      ++ns;
    }
  }
  int n = 0;
  for (int i = 0; i < ns; ++i) {
    const double* v = sol[i];
    double D[9];
    for (int e = 0; e < 9; ++e) D[e] = fma(v[0], w.basis[0][e], fma(v[1], w.basis[1][e], fma(v[2], w.basis[2][e], w.basis[3][e])));
    double u[2][3], vv[2][3], E[9];
    bool ok = tv_top2(D, u, vv);
    for (int r = 0; r < 3; ++r)
      for (int c = 0; c < 3; ++c) E[3 * r + c] = fma(u[0][r], vv[0][c], u[1][r] * vv[1][c]);
    tv_canonical_sign<9>(E);
    for (int e = 0; e < 9; ++e) ok = ok && fabs(E[e]) <= 2.0;
    if (ok) {
      for (int e = 0; e < 9; ++e) E10[9 * n + e] = E[e];
      status10[n] = TV_OK;
      ++n;
    }
  }
  return n;
}

}  // namespace mcba
