// mcba_detect_math.h -- the per-pixel and per-corner arithmetic of csrc/mcba_detect.hip (chessboard detection; reference detection.py),
// written once for the GPU kernels and for the host harness (tests/hostcheck/detect_hostcheck.cpp compiles the same text with g++ and
// checks it against the numpy transcriptions of tests/cv_transcriptions.py in the GPU-less tier).
//
// Floating-point contraction is off in this header: the float32 patch of cornerSubPix and the bilinear warp of the anchor regions are
// evaluated operation by operation, as the IEEE float32 / float64 expressions they transcribe (so host, device and numpy round alike).
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#endif
#ifndef MCBA_HD
#if defined(__HIPCC__)
#define MCBA_HD __host__ __device__ __forceinline__
#else
#define MCBA_HD inline
#endif
#endif

#if defined(__clang__)
#pragma clang fp contract(off)
#endif

namespace mcba {
namespace det {

// OpenCV's fixed-point BGR -> grey (cvtColor COLOR_BGR2GRAY on 8-bit data): Y = (1868 B + 9617 G + 4899 R + 2^13) >> 14
MCBA_HD uint8_t grey_bgr(uint32_t b, uint32_t g, uint32_t r) { return (uint8_t)((1868u * b + 9617u * g + 4899u * r + 8192u) >> 14); }

// ---- cornerSubPix (OpenCV's published iteration)
// Gaussian weight of window sample (i, j), i, j in [0, 2h] x [0, 2w], as OpenCV 4 forms it: y = (i - h) / h and x = (j - w) / w in float32,
// vy = exp(-y y) and vx = exp(-x x) as float32, the mask their float32 product.  (The two exponentials are evaluated in float64 and rounded
// once to float32 -- the correctly rounded float exp; OpenCV's std::exp(float) may differ from it in the last bit.)
MCBA_HD float subpix_mask(int i, int j, int w, int h) {
  const float y = (float)(i - h) / (float)h;
  const float x = (float)(j - w) / (float)w;
  const float vy = (float)exp((double)(-y * y));
  const float vx = (float)exp((double)(-x * x));
  return vy * vx;
}

// getRectSubPix of an 8-bit image into float32: the (pw x ph) patch centred on (cx, cy); patch pixel (pi, pj) is the bilinear value at
// (cx - (pw - 1) / 2 + pj, cy - (ph - 1) / 2 + pi) with the four taps' coordinates clamped to the image (replicated borders).
MCBA_HD float rect_subpix(const uint8_t* img, int W, int H, float cx, float cy, int pw, int ph, int pi, int pj) {
  const float x0 = cx - (float)(pw - 1) * 0.5f;
  const float y0 = cy - (float)(ph - 1) * 0.5f;
  const float fx = floorf(x0), fy = floorf(y0);
  const float a = x0 - fx, b = y0 - fy;
  const float a11 = (1.f - a) * (1.f - b), a12 = a * (1.f - b), a21 = (1.f - a) * b, a22 = a * b;
  int ix = (int)fx + pj, iy = (int)fy + pi;
  const int xa = ix < 0 ? 0 : (ix >= W ? W - 1 : ix), xb = ix + 1 < 0 ? 0 : (ix + 1 >= W ? W - 1 : ix + 1);
  const int ya = iy < 0 ? 0 : (iy >= H ? H - 1 : iy), yb = iy + 1 < 0 ? 0 : (iy + 1 >= H ? H - 1 : iy + 1);
  const float p00 = img[(size_t)ya * W + xa], p01 = img[(size_t)ya * W + xb], p10 = img[(size_t)yb * W + xa], p11 = img[(size_t)yb * W + xb];
  return p00 * a11 + p01 * a12 + p10 * a21 + p11 * a22;
}

// the five sums of one iteration: a = sum gxx, b = sum gxy, c = sum gyy, bb1, bb2
struct SubpixSums { double a, b, c, bb1, bb2; };

// one window sample's contribution (i in [0, 2h], j in [0, 2w]); patch is (2h + 3) x (2w + 3), row-major
MCBA_HD void subpix_term(const float* patch, int w, int h, int i, int j, float m, SubpixSums& s) {
  const int pw = 2 * w + 3;
  const float* p = patch + (size_t)(i + 1) * pw + (j + 1);
  const double tgx = (double)(p[1] - p[-1]);
  const double tgy = (double)(p[pw] - p[-pw]);
  const double gxx = tgx * tgx * m, gxy = tgx * tgy * m, gyy = tgy * tgy * m;
  const double px = j - w, py = i - h;
  s.a += gxx;
  s.b += gxy;
  s.c += gyy;
  s.bb1 += gxx * px + gxy * py;
  s.bb2 += gxy * px + gyy * py;
}

// the update from the sums.  Returns false when det <= DBL_EPSILON^2 (the iteration stops, the corner unchanged); else the new corner
// and err = its squared step (float32 arithmetic, as the float Point2f difference is formed)
MCBA_HD bool subpix_update(const SubpixSums& s, float& x, float& y, double& err) {
  const double det = s.a * s.c - s.b * s.b;
  if (fabs(det) <= 2.220446049250313e-16 * 2.220446049250313e-16) return false;
  const double scale = 1.0 / det;
  const float nx = (float)((double)x + s.c * scale * s.bb1 - s.b * scale * s.bb2);
  const float ny = (float)((double)y - s.b * scale * s.bb1 + s.a * scale * s.bb2);
  const float dx = nx - x, dy = ny - y;
  err = (double)(dx * dx + dy * dy);
  x = nx;
  y = ny;
  return true;
}

MCBA_HD bool subpix_outside(float x, float y, int W, int H) { return x < 0.f || x >= (float)W || y < 0.f || y >= (float)H; }

constexpr int kSubpixMaxIter = 30;
constexpr double kSubpixEps2 = 0.001 * 0.001;

// ---- the anchor: 4-point perspective transform, bilinear warp with border value 0, Pearson correlation of two uint8 images
// M (3x3 row-major) with M (src[k], 1) ~ (dst[k], 1) for the four point pairs (8 x 8 system, Gaussian elimination with partial pivoting,
// M[8] = 1).  Returns false when the system is singular.
MCBA_HD bool persp4(const double* src, const double* dst, double* M) {
  double A[8][9];
  for (int k = 0; k < 4; ++k) {
    const double x = src[2 * k], y = src[2 * k + 1], u = dst[2 * k], v = dst[2 * k + 1];
    double* r0 = A[k];
    double* r1 = A[k + 4];
    r0[0] = x; r0[1] = y; r0[2] = 1; r0[3] = 0; r0[4] = 0; r0[5] = 0; r0[6] = -x * u; r0[7] = -y * u; r0[8] = u;
    r1[0] = 0; r1[1] = 0; r1[2] = 0; r1[3] = x; r1[4] = y; r1[5] = 1; r1[6] = -x * v; r1[7] = -y * v; r1[8] = v;
  }
  for (int c = 0; c < 8; ++c) {
    int p = c;
    for (int r = c + 1; r < 8; ++r)
      if (fabs(A[r][c]) > fabs(A[p][c])) p = r;
    if (fabs(A[p][c]) < 1e-300) return false;
    if (p != c)
      for (int k = 0; k < 9; ++k) { const double t = A[c][k]; A[c][k] = A[p][k]; A[p][k] = t; }
    for (int r = c + 1; r < 8; ++r) {
      const double f = A[r][c] / A[c][c];
      for (int k = c; k < 9; ++k) A[r][k] -= f * A[c][k];
    }
  }
  for (int c = 7; c >= 0; --c) {
    double v = A[c][8];
    for (int k = c + 1; k < 8; ++k) v -= A[c][k] * M[k];
    M[c] = v / A[c][c];
  }
  M[8] = 1.0;
  return true;
}

// bilinear value of the 8-bit image at (sx, sy) (integer coordinates = pixel centres); taps outside the image read 0
MCBA_HD double bilinear0(const uint8_t* img, int W, int H, double sx, double sy) {
  const double fx = floor(sx), fy = floor(sy);
  const double ax = sx - fx, ay = sy - fy;
  const long x0 = (long)fx, y0 = (long)fy;
  double p[4];
  for (int k = 0; k < 4; ++k) {
    const long x = x0 + (k & 1), y = y0 + (k >> 1);
    p[k] = (x >= 0 && x < W && y >= 0 && y < H) ? (double)img[(size_t)y * W + x] : 0.0;
  }
  return (1.0 - ay) * ((1.0 - ax) * p[0] + ax * p[1]) + ay * ((1.0 - ax) * p[2] + ax * p[3]);
}

// template pixel (x, y) warped through M (template -> image), rounded half to even and saturated to uint8
MCBA_HD uint8_t warp_pixel(const uint8_t* img, int W, int H, const double* M, int x, int y) {
  const double X = M[0] * x + M[1] * y + M[2], Y = M[3] * x + M[4] * y + M[5], Z = M[6] * x + M[7] * y + M[8];
  if (!(fabs(Z) > 0.0)) return 0;
  const double sx = X / Z, sy = Y / Z;
  if (!(fabs(sx) < 1e9 && fabs(sy) < 1e9)) return 0;
  const double v = rint(bilinear0(img, W, H, sx, sy));
  return (uint8_t)(v < 0.0 ? 0.0 : (v > 255.0 ? 255.0 : v));
}

constexpr int kTemplate = 40;
// the anchor template: 255, and 0 on the disc (x - 10)^2 + (y - 10)^2 <= 100 (317 pixels)
MCBA_HD uint8_t template_pixel(int x, int y) { return (x - 10) * (x - 10) + (y - 10) * (y - 10) <= 100 ? 0 : 255; }

// Pearson correlation from exact integer sums of n pairs (r, t): 0 when either has zero variance
MCBA_HD double pearson(double n, double sr, double st, double srr, double stt, double srt) {
  const double vr = n * srr - sr * sr, vt = n * stt - st * st;
  if (!(vr > 0.0) || !(vt > 0.0)) return 0.0;
  return (n * srt - sr * st) / sqrt(vr * vt);
}

// ---- extend_grid's homography: Hartley-normalised DLT of n correspondences xy -> uv, the right singular vector of the smallest singular
// value of A (2n x 9) as the eigenvector of A^T A (cyclic Jacobi).  H row-major, scaled so that H[8] = 1.
MCBA_HD void jacobi_smallest9(double* S, double* vec) {
  double V[81];
  for (int i = 0; i < 81; ++i) V[i] = (i % 10 == 0) ? 1.0 : 0.0;
  for (int sweep = 0; sweep < 30; ++sweep) {
    double off = 0.0;
    for (int p = 0; p < 9; ++p)
      for (int q = p + 1; q < 9; ++q) off += S[p * 9 + q] * S[p * 9 + q];
    double dn = 0.0;
    for (int p = 0; p < 9; ++p) dn += S[p * 9 + p] * S[p * 9 + p];
    if (off <= 1e-32 * dn) break;   // off-diagonal at rounding level of the largest eigenvalue
    for (int p = 0; p < 9; ++p)
      for (int q = p + 1; q < 9; ++q) {
        const double apq = S[p * 9 + q];
        if (apq == 0.0) continue;
        const double theta = (S[q * 9 + q] - S[p * 9 + p]) / (2.0 * apq);
        const double t = (theta >= 0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
        const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
        for (int k = 0; k < 9; ++k) {  // S <- S J (columns p, q)
          const double skp = S[k * 9 + p], skq = S[k * 9 + q];
          S[k * 9 + p] = c * skp - s * skq;
          S[k * 9 + q] = s * skp + c * skq;
        }
        for (int k = 0; k < 9; ++k) {  // S <- J^T S (rows p, q)
          const double spk = S[p * 9 + k], sqk = S[q * 9 + k];
          S[p * 9 + k] = c * spk - s * sqk;
          S[q * 9 + k] = s * spk + c * sqk;
        }
        for (int k = 0; k < 9; ++k) {
          const double vkp = V[k * 9 + p], vkq = V[k * 9 + q];
          V[k * 9 + p] = c * vkp - s * vkq;
          V[k * 9 + q] = s * vkp + c * vkq;
        }
      }
  }
  int m = 0;
  for (int i = 1; i < 9; ++i)
    if (S[i * 9 + i] < S[m * 9 + m]) m = i;
  for (int k = 0; k < 9; ++k) vec[k] = V[k * 9 + m];
}

// similarity that takes points to centroid 0 and mean distance sqrt(2): x' = s (x - m)
MCBA_HD void hartley(const double* p, int n, double& mx, double& my, double& s) {
  mx = 0; my = 0;
  for (int i = 0; i < n; ++i) { mx += p[2 * i]; my += p[2 * i + 1]; }
  mx /= n; my /= n;
  double d = 0;
  for (int i = 0; i < n; ++i) d += sqrt((p[2 * i] - mx) * (p[2 * i] - mx) + (p[2 * i + 1] - my) * (p[2 * i + 1] - my));
  d /= n;
  s = d > 0 ? 1.4142135623730951 / d : 1.0;
}

// the Hartley similarities of both point sets: x' = as (x - (ax, ay)), u' = bs (u - (bx, by))
struct DltNorm { double ax, ay, as, bx, by, bs; };

MCBA_HD DltNorm dlt_norm(const double* xy, const double* uv, int n) {
  DltNorm m;
  hartley(xy, n, m.ax, m.ay, m.as);
  hartley(uv, n, m.bx, m.by, m.bs);
  return m;
}

// entry e = 9 i + j of A^T A, A = the rows [x' y' 1 0 0 0 -u'x' -u'y' -u'], [0 0 0 x' y' 1 -v'x' -v'y' -v'] of the normalised points,
// summed over the points in index order (the kernel forms one entry per lane)
MCBA_HD double dlt_normal_entry(const double* xy, const double* uv, int n, const DltNorm& m, int e) {
  const int ei = e / 9, ej = e % 9;
  double acc = 0.0;
  for (int k = 0; k < n; ++k) {
    const double x = m.as * (xy[2 * k] - m.ax), y = m.as * (xy[2 * k + 1] - m.ay);
    const double u = m.bs * (uv[2 * k] - m.bx), v = m.bs * (uv[2 * k + 1] - m.by);
    const double r0[9] = {x, y, 1, 0, 0, 0, -u * x, -u * y, -u};
    const double r1[9] = {0, 0, 0, x, y, 1, -v * x, -v * y, -v};
    acc += r0[ei] * r0[ej] + r1[ei] * r1[ej];
  }
  return acc;
}

// the homography from the normal matrix S (destroyed): its smallest eigenvector, de-normalised, scaled so that H[8] = 1
MCBA_HD void dlt_finish(double* S, const DltNorm& m, double* H) {
  double h[9];
  jacobi_smallest9(S, h);
  // H = Tb^-1 Hn Ta, Ta = [[as, 0, -as ax], [0, as, -as ay], [0, 0, 1]], Tb^-1 = [[1/bs, 0, bx], [0, 1/bs, by], [0, 0, 1]]
  double HT[9];
  for (int r = 0; r < 3; ++r) {
    HT[r * 3 + 0] = h[r * 3 + 0] * m.as;
    HT[r * 3 + 1] = h[r * 3 + 1] * m.as;
    HT[r * 3 + 2] = h[r * 3 + 2] - h[r * 3 + 0] * m.as * m.ax - h[r * 3 + 1] * m.as * m.ay;
  }
  for (int c = 0; c < 3; ++c) {
    H[0 * 3 + c] = HT[0 * 3 + c] / m.bs + m.bx * HT[2 * 3 + c];
    H[1 * 3 + c] = HT[1 * 3 + c] / m.bs + m.by * HT[2 * 3 + c];
    H[2 * 3 + c] = HT[2 * 3 + c];
  }
  const double z = H[8];
  for (int i = 0; i < 9; ++i) H[i] /= z;
}

// the whole DLT on one thread (the host harness; k_det_anchor runs the same three pieces, dlt_normal_entry one entry per lane)
MCBA_HD void homography_dlt(const double* xy, const double* uv, int n, double* H) {
  const DltNorm m = dlt_norm(xy, uv, n);
  double S[81];
  for (int e = 0; e < 81; ++e) S[e] = dlt_normal_entry(xy, uv, n, m, e);
  dlt_finish(S, m, H);
}

MCBA_HD void apply_h(const double* H, double x, double y, double& u, double& v) {
  const double w = H[6] * x + H[7] * y + H[8];
  u = (H[0] * x + H[1] * y + H[2]) / w;
  v = (H[3] * x + H[4] * y + H[5]) / w;
}

// the four source quads of reorder_chessboard_corners (detection.py:466-471) on the grid extended by 3 rows and 1 column each side:
// ext[R][C] = H (C, R); quad k, corner q as (row, col) of ext, with R_ = rows + 6 - 1 and C_ = cols + 2 - 1 the last indices
MCBA_HD void quad_cell(int k, int q, int rows, int cols, int& R, int& C) {
  const int Rl = rows + 5, Cl = cols + 1;
  // region 0: ext[2,0], ext[0,0], ext[0,2], ext[2,2]
  // region 1: ext[0,-3], ext[0,-1], ext[2,-1], ext[2,-3]
  // region 2: ext[-3,-1], ext[-1,-1], ext[-1,-3], ext[-3,-3]
  // region 3: ext[-1,2], ext[-1,0], ext[-3,0], ext[-3,2]
  // (negative: counted from the end, as numpy indexes)
  int r, c;
  switch (k * 4 + q) {
    case 0: r = 2; c = 0; break;
    case 1: r = 0; c = 0; break;
    case 2: r = 0; c = 2; break;
    case 3: r = 2; c = 2; break;
    case 4: r = 0; c = -3; break;
    case 5: r = 0; c = -1; break;
    case 6: r = 2; c = -1; break;
    case 7: r = 2; c = -3; break;
    case 8: r = -3; c = -1; break;
    case 9: r = -1; c = -1; break;
    case 10: r = -1; c = -3; break;
    case 11: r = -3; c = -3; break;
    case 12: r = -1; c = 2; break;
    case 13: r = -1; c = 0; break;
    case 14: r = -3; c = 0; break;
    default: r = -3; c = 2; break;
  }
  R = r < 0 ? Rl + 1 + r : r;
  C = c < 0 ? Cl + 1 + c : c;
}

}  // namespace det
}  // namespace mcba
