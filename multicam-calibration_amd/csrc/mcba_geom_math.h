// mcba_geom_math.h -- the per-lane geometry that several kernels share, each piece written once: the packed Cholesky solve (k_pnp with N = 6,
// k_reproj_diag with N = 8), OpenCV's pixel undistortion (k_undistort, k_reproj_diag, both triangulation kernels), the two-view triangulation and
// the in-register nan-median of csrc/mcba_triangulate.hip, and the board-plane homography fit of k_reproj_diag (csrc/mcba_diag.hip).
// Nothing here needs a wavefront (DPP, ballots, LDS and the uniform loads stay in the .hip files), so the same text is compiled into the gfx950
// kernels and, with g++, into the host harness (tests/hostcheck/hostcheck.cpp, also under ASan + UBSan), where tests/test_hostcheck_math.py checks
// it against oracle/triangulate_oracle.py and oracle/diagnostics_oracle.py in the GPU-less tier.
#pragma once
#include "mcba_math.h"

namespace mcba {

// ---- packed symmetric N x N (upper triangle row-major): Cholesky solve in registers, in place on b
template <int N>
MCBA_HD constexpr int tri(int i, int j) { return i * N - (i * (i - 1)) / 2 + (j - i); }
template <int N>
MCBA_HD bool chol_solve(double* A, double* b) {
  bool ok = true;
  // A = L L^T, L stored over the upper triangle as L^T (row i = column i of L)
#pragma unroll
  for (int i = 0; i < N; ++i) {
#pragma unroll
    for (int j = i; j < N; ++j) {
      double s = A[tri<N>(i, j)];
#pragma unroll
      for (int k = 0; k < i; ++k) s = fma(-A[tri<N>(k, i)], A[tri<N>(k, j)], s);
      if (j == i) {
        ok = ok && s > 0.0;
        A[tri<N>(i, i)] = sqrt(s > 0.0 ? s : 1.0);
      } else {
        A[tri<N>(i, j)] = s / A[tri<N>(i, i)];
      }
    }
  }
#pragma unroll
  for (int i = 0; i < N; ++i) {
    double s = b[i];
#pragma unroll
    for (int k = 0; k < i; ++k) s = fma(-A[tri<N>(k, i)], b[k], s);
    b[i] = s / A[tri<N>(i, i)];
  }
#pragma unroll
  for (int i = N - 1; i >= 0; --i) {
    double s = b[i];
#pragma unroll
    for (int k = i + 1; k < N; ++k) s = fma(-A[tri<N>(i, k)], b[k], s);
    b[i] = s / A[tri<N>(i, i)];
  }
  return ok;
}

// ---- undistortion in pixels (cv2.undistortPoints(src, K, dist, None, K)); k = (k1 k2 p1 p2 k3)
// (undistort_norm in mcba_pnp_math.h is the other one, separate on purpose: fast_rcp, no guard, normalised output)
MCBA_HD void undistort_px(double u, double v, double fx, double fy, double cx, double cy, const double* k, int iters, double& uo, double& vo) {
  const double x0 = (u - cx) / fx, y0 = (v - cy) / fy;
  double x = x0, y = y0;
  bool stop = false;   // OpenCV's guard (cvUndistortPointsInternal): icdist < 0 -> the unrefined point, no further iterations
  for (int it = 0; it < iters; ++it) {
    const double r2 = fma(x, x, y * y);
    const double icdist = 1.0 / fma(fma(fma(k[4], r2, k[1]), r2, k[0]), r2, 1.0);
    stop = stop || icdist < 0.0;
    const double dx = fma(2.0 * k[2] * x, y, k[3] * fma(2.0 * x, x, r2));
    const double dy = fma(k[2], fma(2.0 * y, y, r2), 2.0 * k[3] * x * y);
    x = stop ? x0 : (x0 - dx) * icdist;
    y = stop ? y0 : (y0 - dy) * icdist;
  }
  uo = fma(x, fx, cx);
  vo = fma(y, fy, cy);
}

// ---- two-view triangulation
// right singular vector of the smallest singular value of the 4x4 matrix whose COLUMNS are a[0..3] (each a 4-vector)
MCBA_HD void null_vector4(double (&a)[4][4], double (&x)[4]) {
  double v[4][4];  // v[k] = column k of V
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) v[i][j] = i == j ? 1.0 : 0.0;
  for (int sweep = 0; sweep < 7; ++sweep) {  // quadratic convergence: 4-5 sweeps reach FP64 for a 4x4; fixed count, branch-free
#pragma unroll
    for (int p = 0; p < 3; ++p)
#pragma unroll
      for (int q = p + 1; q < 4; ++q) {
        double alpha = 0.0, beta = 0.0, gamma = 0.0;
#pragma unroll
        for (int k = 0; k < 4; ++k) { alpha = fma(a[p][k], a[p][k], alpha); beta = fma(a[q][k], a[q][k], beta); gamma = fma(a[p][k], a[q][k], gamma); }
        const bool rot = gamma * gamma > 1e-32 * alpha * beta;  // already orthogonal to FP64: identity
        const double g = rot ? gamma : 1.0;
        const double zeta = (beta - alpha) * fast_rcp(2.0 * g);
        const double az = fabs(zeta);
        double t = fast_rcp(az + sqrt(fma(zeta, zeta, 1.0)));
        t = zeta < 0.0 ? -t : t;
        t = rot ? t : 0.0;
        const double c = fast_rsqrt(fma(t, t, 1.0)), s = c * t;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const double ap = a[p][k], aq = a[q][k];
          a[p][k] = fma(c, ap, -(s * aq));
          a[q][k] = fma(s, ap, c * aq);
          const double vp = v[p][k], vq = v[q][k];
          v[p][k] = fma(c, vp, -(s * vq));
          v[q][k] = fma(s, vp, c * vq);
        }
      }
  }
  double best = 1e300;
#pragma unroll
  for (int k = 0; k < 4; ++k) x[k] = 0.0;
#pragma unroll
  for (int p = 0; p < 4; ++p) {
    double nrm = 0.0;
#pragma unroll
    for (int k = 0; k < 4; ++k) nrm = fma(a[p][k], a[p][k], nrm);
    const bool take = nrm < best;
    best = take ? nrm : best;
#pragma unroll
    for (int k = 0; k < 4; ++k) x[k] = take ? v[p][k] : x[k];
  }
}

// the point seen at (uxi, uyi) by the camera with the 3x4 projection Pi and at (uxj, uyj) by Pj (undistorted pixels; both = both detections
// present): 4x4 DLT system, its null vector, de-homogenised.  Returns keep; a pair that is not kept gives 1e300 in all three coordinates, so that
// it sorts to the end.  (A pair whose null vector has x[3] == 0 -- a point at infinity for that pair -- gives NaN or +-inf: such a pair does not
// count at all, in any coordinate; np.nanmedian drops the NaNs per coordinate, geometry.py:432)
MCBA_HD bool triangulate_pair(double uxi, double uyi, const double* Pi, double uxj, double uyj, const double* Pj, bool both, double& X, double& Y, double& Z) {
  double a[4][4];  // a[col][row]
#pragma unroll
  for (int col = 0; col < 4; ++col) {
    a[col][0] = fma(uxi, Pi[8 + col], -Pi[col]);
    a[col][1] = fma(uyi, Pi[8 + col], -Pi[4 + col]);
    a[col][2] = fma(uxj, Pj[8 + col], -Pj[col]);
    a[col][3] = fma(uyj, Pj[8 + col], -Pj[4 + col]);
  }
  if (!both) {  // keep the arithmetic finite; the result is discarded
#pragma unroll
    for (int col = 0; col < 4; ++col)
#pragma unroll
      for (int r = 0; r < 4; ++r) a[col][r] = col == r ? 1.0 : 0.0;
  }
  double x[4];
  null_vector4(a, x);
  const double iw = 1.0 / x[3];
  const double big = 1e300;
  const double vx = x[0] * iw, vy = x[1] * iw, vz = x[2] * iw;
  const bool keep = both && fabs(vx) < big && fabs(vy) < big && fabs(vz) < big;
  X = keep ? vx : big;
  Y = keep ? vy : big;
  Z = keep ? vz : big;
  return keep;
}

// nan-median of the n kept values among v[0..NP) (the others are 1e300): sort (odd-even transposition network, NP passes), pick the middle
// (or the mean of two); NaN when nothing was kept
template <int NP>
MCBA_HD double nan_median(double (&v)[NP], int n) {
#pragma unroll
  for (int pass = 0; pass < NP; ++pass)
#pragma unroll
    for (int k = pass & 1; k + 1 < NP; k += 2) {
      const double lo = fmin(v[k], v[k + 1]), hi = fmax(v[k], v[k + 1]);
      v[k] = lo; v[k + 1] = hi;
    }
  double m0 = 0.0, m1 = 0.0;
  const int i0 = (n - 1) >> 1, i1 = n >> 1;
#pragma unroll
  for (int k = 0; k < NP; ++k) { m0 = k == i0 ? v[k] : m0; m1 = k == i1 ? v[k] : m1; }
  return n > 0 ? 0.5 * (m0 + m1) : __builtin_nan("");
}

// ---- homography from image points to the board plane (the reprojection diagnostics' least-squares fit, h33 = 1)
// one point's two rows into the packed 8x8 normal equations: A += r0 r0^T + r1 r1^T, b += r0 t0 + r1 t1
MCBA_HD void normal8_add(const double (&r0)[8], const double (&r1)[8], double t0, double t1, double* A, double* b) {
#pragma unroll
  for (int i = 0; i < 8; ++i) {
#pragma unroll
    for (int j = i; j < 8; ++j) A[tri<8>(i, j)] = fma(r0[i], r0[j], fma(r1[i], r1[j], A[tri<8>(i, j)]));
    b[i] = fma(r0[i], t0, fma(r1[i], t1, b[i]));
  }
}

// sum over the points of |board - h(image)|^2; board_point(p, sx, sy, X, Y) hands out point p: image (sx, sy), board (X, Y), both normalised
template <class Fetch>
MCBA_HD double board_transfer_error(Fetch& board_point, int N, const double* hh) {
  double e = 0.0;
  for (int p = 0; p < N; ++p) {
    double sx, sy, X, Y;
    board_point(p, sx, sy, X, Y);
    const double iw = 1.0 / fma(hh[6], sx, fma(hh[7], sy, 1.0));
    const double ex = X - fma(hh[0], sx, fma(hh[1], sy, hh[2])) * iw, ey = Y - fma(hh[3], sx, fma(hh[4], sy, hh[5])) * iw;
    e = fma(ex, ex, fma(ey, ey, e));
  }
  return e;
}

// Normalised inhomogeneous DLT (h33 = 1; 8x8 normal equations) as the start, then Levenberg-Marquardt on the transfer error in the board plane
// -- the quantity OpenCV's findHomography refines -- with a FIXED number of rounds (every lane runs the same instruction stream; a rejected step
// only raises that lane's damping).  complete = false (a lane whose detection is incomplete; its points are all (0, 0)): unit diagonals keep the
// arithmetic finite, the result is discarded.  Out: h (8); returns the transfer error reached.
template <class Fetch>
MCBA_HD double board_homography_fit(Fetch& board_point, int N, bool complete, int lm_iters, double (&h)[8]) {
  {  // start: rows [s 1 0 0 0 -X s] h = X, [0 0 0 s 1 -Y s] h = Y  (s = (sx, sy))
    double A[36], b[8];
#pragma unroll
    for (int i = 0; i < 36; ++i) A[i] = 0.0;
#pragma unroll
    for (int i = 0; i < 8; ++i) b[i] = 0.0;
    for (int p = 0; p < N; ++p) {
      double sx, sy, X, Y;
      board_point(p, sx, sy, X, Y);
      const double r0[8] = {sx, sy, 1.0, 0.0, 0.0, 0.0, -X * sx, -X * sy};
      const double r1[8] = {0.0, 0.0, 0.0, sx, sy, 1.0, -Y * sx, -Y * sy};
      normal8_add(r0, r1, X, Y, A, b);
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) A[tri<8>(i, i)] = complete ? A[tri<8>(i, i)] : 1.0;
    const bool ok = chol_solve<8>(A, b);
#pragma unroll
    for (int i = 0; i < 8; ++i) h[i] = ok ? b[i] : ((i == 0 || i == 4) ? 1.0 : 0.0);  // degenerate detection: start from the identity
  }
  double e_cur = board_transfer_error(board_point, N, h), mu = 1e-4;
  for (int it = 0; it < lm_iters; ++it) {
    double A[36], g[8];
#pragma unroll
    for (int i = 0; i < 36; ++i) A[i] = 0.0;
#pragma unroll
    for (int i = 0; i < 8; ++i) g[i] = 0.0;
    for (int p = 0; p < N; ++p) {
      double sx, sy, X, Y;
      board_point(p, sx, sy, X, Y);
      const double iw = 1.0 / fma(h[6], sx, fma(h[7], sy, 1.0));
      const double px = fma(h[0], sx, fma(h[1], sy, h[2])) * iw, py = fma(h[3], sx, fma(h[4], sy, h[5])) * iw;
      const double r0[8] = {sx * iw, sy * iw, iw, 0.0, 0.0, 0.0, -px * sx * iw, -px * sy * iw};
      const double r1[8] = {0.0, 0.0, 0.0, sx * iw, sy * iw, iw, -py * sx * iw, -py * sy * iw};
      normal8_add(r0, r1, X - px, Y - py, A, g);
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) A[tri<8>(i, i)] = complete ? A[tri<8>(i, i)] * (1.0 + mu) : 1.0;   // Marquardt damping
    const bool ok = chol_solve<8>(A, g);
    double hn[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) hn[i] = h[i] + (ok ? g[i] : 0.0);
    const double e_new = board_transfer_error(board_point, N, hn);
    // (not worse beyond the round-off of the sum: near the optimum the decrease left is below it, and a strict test stalls each lane
    //  wherever its round-off says -- up to 1e-5 mm from the minimiser on the board plane; a tolerant one lets the Gauss-Newton steps finish)
    const bool accept = ok && e_new <= e_cur * (1.0 + 1e-12);   // (NaN compares false)
#pragma unroll
    for (int i = 0; i < 8; ++i) h[i] = accept ? hn[i] : h[i];
    e_cur = accept ? e_new : e_cur;
    mu = accept ? fmax(mu * 0.1, 1e-15) : fmin(mu * 10.0, 1e8);
  }
  return e_cur;
}

}  // namespace mcba
