// mcba_detect.hip -- chessboard detection (reference detection.py: detect_chessboard, reorder_chessboard_corners) on the device.
//
// Three stateless entry points (include/mcba.h, "chessboard detection"):
//   mcba_detect_chessboards  the whole pipeline for a batch of frames, chunked so that device memory stays within a fixed budget; per chunk one
//                            upload, the launches below back to back, one download:
//     k_det_prep     one lane per pixel: OpenCV's fixed-point BGR -> grey (frames of one channel are uploaded as the grey image itself)
//     k_det_resize   one lane per detection-scale pixel (scale_factor != 1): bilinear sample of the grey image at ((x + 1/2) / s - 1/2, ...)
//     k_det_saddle   16 x 16 output tiles (256 lanes) with a 4-pixel halo in LDS: separable Gaussian (sigma 1, 7 taps), Hessian by central
//                    differences, saddle response R = Ixy^2 - Ixx Iyy (zero within 5 px of the border); per-frame maximum by the tile's
//                    maximum and one integer atomic per tile
//     k_det_nms      one lane per pixel: R >= max(kRespFrac * max R, kRespFloor), strict 5 x 5 maximum (ties to the lower pixel index), a ring of 16
//                    samples at radius 3 around it that changes sides of its midpoint exactly 4 times (an X junction: L corners of the board's
//                    outline, dots and edges give 2 or 0), a parabolic sub-pixel offset; compacted by an atomic counter into at most
//                    MCBA_DETECT_MAX_CANDIDATES per frame (more: the frame is reported as overflowing, never truncated)
//     k_det_grid     one wavefront per frame, the candidates in LDS: seeds in descending R (ties: lower pixel index); the seed's nearest neighbour
//                    and nearest neighbour at 50..130 degrees to it span the lattice, which grows breadth-first on integer coordinates (prediction
//                    2 p(i) - p(i-1), else the parallelogram of a known neighbour row, else p + seed step; the nearest unused candidate within
//                    0.35 of the local step is taken).  Accepted: exactly board_rows x board_cols (either way round), completely filled, and the
//                    cells sampled at their centres alternate dark / light with a gap (a 2 x 2 board's one cell against its four edge
//                    neighbours).  Every choice over the candidate list compares
//                    (distance or R, pixel index), a total order, so the order the atomics appended the candidates in never shows.
//     k_det_subpix   one wavefront per corner: cornerSubPix on the full-resolution grey image (csrc/mcba_detect_math.h)
//     k_det_anchor   one workgroup per frame: extend_grid's homography (normalised DLT), the four 4-point transforms, 4 x 1600 warped samples,
//                    exact integer moments -> four correlations; the reference's flips, the sorted scores and the status
//   mcba_detect_subpix       k_det_subpix for given start corners of one image
//   mcba_detect_anchor       k_det_anchor's scores, regions and quads for given corners of one image (no reordering)
#include <stdint.h>

#include "mcba_detect_math.h"
#include "mcba_handle.h"

namespace mcba {

constexpr int kDetTile = 16;
constexpr int kDetHalo = 4;
constexpr int kDetRaw = kDetTile + 2 * kDetHalo;  // 24
constexpr int kDetSm = kDetTile + 2;              // 18
constexpr int kDetBorder = 5;                     // R is zero this close to the border
constexpr float kRespFrac = 0.05f;
constexpr float kRespFloor = 4.0f;
constexpr float kRingRadius = 3.0f;
constexpr float kRingContrast = 16.0f;
constexpr float kCellGap = 8.0f;
constexpr float kAcceptFrac = 0.35f;
constexpr int kGridSide = 64;   // lattice coordinates around the seed at (32, 32)
constexpr int kMaxFill = 1024;  // lattice cells filled before a seed is given up
constexpr int kDetSeeds = 6;
constexpr int kStatusOverflow = 3;

struct Cand { float x, y, r; int key; };

__device__ __forceinline__ uint8_t clamp_u8(float v) { v = rintf(v); return (uint8_t)(v < 0.f ? 0.f : (v > 255.f ? 255.f : v)); }

__device__ __forceinline__ float sample_clamped(const uint8_t* img, int W, int H, float x, float y) {
  const float fx = floorf(x), fy = floorf(y);
  const float ax = x - fx, ay = y - fy;
  const int x0 = (int)fx, y0 = (int)fy;
  const int xa = min(max(x0, 0), W - 1), xb = min(max(x0 + 1, 0), W - 1), ya = min(max(y0, 0), H - 1), yb = min(max(y0 + 1, 0), H - 1);
  const float p00 = img[(size_t)ya * W + xa], p01 = img[(size_t)ya * W + xb], p10 = img[(size_t)yb * W + xa], p11 = img[(size_t)yb * W + xb];
  return (1.f - ay) * ((1.f - ax) * p00 + ax * p01) + ay * ((1.f - ax) * p10 + ax * p11);
}

__global__ __launch_bounds__(256) void k_det_prep(const uint8_t* __restrict__ bgr, size_t n_pixels, uint8_t* __restrict__ grey) {
  for (size_t p = (size_t)blockIdx.x * 256 + threadIdx.x; p < n_pixels; p += (size_t)gridDim.x * 256)
    grey[p] = det::grey_bgr(bgr[3 * p], bgr[3 * p + 1], bgr[3 * p + 2]);
}

// grid: (ceil(Wd / 256), Hd, frames)
__global__ __launch_bounds__(256) void k_det_resize(const uint8_t* __restrict__ grey, int W, int H, uint8_t* __restrict__ det, int Wd, int Hd, float inv_s) {
  const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y, b = blockIdx.z;
  if (x >= Wd) return;
  const float sx = ((float)x + 0.5f) * inv_s - 0.5f, sy = ((float)y + 0.5f) * inv_s - 0.5f;
  det[((size_t)b * Hd + y) * Wd + x] = clamp_u8(sample_clamped(grey + (size_t)b * W * H, W, H, sx, sy));
}

// grid: (ceil(Wd / 16), ceil(Hd / 16), frames)
__global__ __launch_bounds__(256) void k_det_saddle(const uint8_t* __restrict__ det, int Wd, int Hd, float* __restrict__ resp, unsigned* __restrict__ rmax) {
  __shared__ float s_raw[kDetRaw][kDetRaw];
  __shared__ float s_h[kDetRaw][kDetSm];
  __shared__ float s_sm[kDetSm][kDetSm];
  __shared__ float s_wmax[4];
  const int tid = threadIdx.x, b = blockIdx.z;
  const int x0 = blockIdx.x * kDetTile, y0 = blockIdx.y * kDetTile;
  const uint8_t* img = det + (size_t)b * Wd * Hd;
  for (int i = tid; i < kDetRaw * kDetRaw; i += 256) {
    const int r = i / kDetRaw, c = i % kDetRaw;
    const int y = min(max(y0 - kDetHalo + r, 0), Hd - 1), x = min(max(x0 - kDetHalo + c, 0), Wd - 1);
    s_raw[r][c] = img[(size_t)y * Wd + x];
  }
  __syncthreads();
  const float g0 = 0.39905027f, g1 = 0.24203623f, g2 = 0.05400558f, g3 = 0.00443305f;  // exp(-k^2 / 2), normalised
  for (int i = tid; i < kDetRaw * kDetSm; i += 256) {
    const int r = i / kDetSm, c = i % kDetSm + 3;
    s_h[r][i % kDetSm] = g0 * s_raw[r][c] + g1 * (s_raw[r][c - 1] + s_raw[r][c + 1]) + g2 * (s_raw[r][c - 2] + s_raw[r][c + 2]) + g3 * (s_raw[r][c - 3] + s_raw[r][c + 3]);
  }
  __syncthreads();
  for (int i = tid; i < kDetSm * kDetSm; i += 256) {
    const int r = i / kDetSm + 3, c = i % kDetSm;
    s_sm[i / kDetSm][c] = g0 * s_h[r][c] + g1 * (s_h[r - 1][c] + s_h[r + 1][c]) + g2 * (s_h[r - 2][c] + s_h[r + 2][c]) + g3 * (s_h[r - 3][c] + s_h[r + 3][c]);
  }
  __syncthreads();
  const int ox = tid % kDetTile, oy = tid / kDetTile;
  const int x = x0 + ox, y = y0 + oy;
  const bool in = x < Wd && y < Hd;
  float R = 0.f;
  if (in && x >= kDetBorder && y >= kDetBorder && x < Wd - kDetBorder && y < Hd - kDetBorder) {
    const int r = oy + 1, c = ox + 1;
    const float ixx = s_sm[r][c + 1] - 2.f * s_sm[r][c] + s_sm[r][c - 1];
    const float iyy = s_sm[r + 1][c] - 2.f * s_sm[r][c] + s_sm[r - 1][c];
    const float ixy = 0.25f * (s_sm[r + 1][c + 1] - s_sm[r + 1][c - 1] - s_sm[r - 1][c + 1] + s_sm[r - 1][c - 1]);
    R = ixy * ixy - ixx * iyy;
  }
  if (in) resp[((size_t)b * Hd + y) * Wd + x] = R;
  // the frame's maximum: wavefront maxima, the tile's maximum in LDS, then one integer atomic per tile (positive floats order as their bit
  // patterns)
  float m = fmaxf(R, 0.f);
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) m = fmaxf(m, __shfl_xor(m, off, 64));
  if ((tid & 63) == 0) s_wmax[tid >> 6] = m;
  __syncthreads();
  if (tid == 0) {
    const float t = fmaxf(fmaxf(s_wmax[0], s_wmax[1]), fmaxf(s_wmax[2], s_wmax[3]));
    if (t > 0.f) atomicMax(rmax + b, __float_as_uint(t));
  }
}

// grid: (ceil(Wd / 16), ceil(Hd / 16), frames)
__global__ __launch_bounds__(256) void k_det_nms(const float* __restrict__ resp, const uint8_t* __restrict__ det, int Wd, int Hd, const unsigned* __restrict__ rmax,
                                                 unsigned* __restrict__ count, Cand* __restrict__ cand) {
  const int b = blockIdx.z;
  const int x = blockIdx.x * kDetTile + threadIdx.x % kDetTile, y = blockIdx.y * kDetTile + threadIdx.x / kDetTile;
  if (x < kDetBorder || y < kDetBorder || x >= Wd - kDetBorder || y >= Hd - kDetBorder) return;
  const float* rp = resp + (size_t)b * Wd * Hd;
  const float R = rp[(size_t)y * Wd + x];
  const float thr = fmaxf(kRespFrac * __uint_as_float(rmax[b]), kRespFloor);
  if (!(R >= thr)) return;
  for (int dy = -2; dy <= 2; ++dy)
    for (int dx = -2; dx <= 2; ++dx) {
      if (dx == 0 && dy == 0) continue;
      const float q = rp[(size_t)(y + dy) * Wd + (x + dx)];
      if (q > R || (q == R && (dy < 0 || (dy == 0 && dx < 0)))) return;
    }
  const uint8_t* img = det + (size_t)b * Wd * Hd;
  float v[16], lo = 1e30f, hi = -1e30f;
#pragma unroll
  for (int k = 0; k < 16; ++k) {
    float sn, cs;
    sincosf(0.39269908f * k, &sn, &cs);
    v[k] = sample_clamped(img, Wd, Hd, x + kRingRadius * cs, y + kRingRadius * sn);
    lo = fminf(lo, v[k]);
    hi = fmaxf(hi, v[k]);
  }
  if (hi - lo < kRingContrast) return;
  const float mid = 0.5f * (hi + lo);
  int changes = 0;
#pragma unroll
  for (int k = 0; k < 16; ++k) changes += (v[k] > mid) != (v[(k + 1) & 15] > mid);
  if (changes != 4) return;
  // parabolic offset of the peak (each axis), at most half a pixel
  const float rl = rp[(size_t)y * Wd + x - 1], rr = rp[(size_t)y * Wd + x + 1], ru = rp[(size_t)(y - 1) * Wd + x], rd = rp[(size_t)(y + 1) * Wd + x];
  const float cx = rl - 2.f * R + rr, cy = ru - 2.f * R + rd;
  const float ox = cx < 0.f ? fminf(fmaxf(0.5f * (rl - rr) / cx, -0.5f), 0.5f) : 0.f;
  const float oy = cy < 0.f ? fminf(fmaxf(0.5f * (ru - rd) / cy, -0.5f), 0.5f) : 0.f;
  const unsigned slot = atomicAdd(count + b, 1u);
  if (slot < MCBA_DETECT_MAX_CANDIDATES) cand[(size_t)b * MCBA_DETECT_MAX_CANDIDATES + slot] = Cand{x - ox, y - oy, R, y * Wd + x};
}

// (distance, key) lexicographic minimum over the wavefront; every lane ends with the same (d, key, idx)
__device__ __forceinline__ void wave_argmin(float& d, int& key, int& idx) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    const float od = __shfl_xor(d, off, 64);
    const int ok = __shfl_xor(key, off, 64), oi = __shfl_xor(idx, off, 64);
    if (od < d || (od == d && ok < key)) { d = od; key = ok; idx = oi; }
  }
}
__device__ __forceinline__ float wave_minf(float v) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v = fminf(v, __shfl_xor(v, off, 64));
  return v;
}
__device__ __forceinline__ float wave_maxf(float v) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v = fmaxf(v, __shfl_xor(v, off, 64));
  return v;
}

struct GridArgs {
  int Wd, Hd, W, H;
  float scale;  // detection scale s: full = (det + 1/2) / s - 1/2
  int rows, cols;  // board_shape[1], board_shape[0]
};

// one wavefront (64 lanes) per frame.  corners: frames x rows*cols float2 in the board layout (row r along board y, column c along board x,
// up to the flips the anchor decides); gstat: 0 no grid, 1 grid, kStatusOverflow
__global__ __launch_bounds__(64) void k_det_grid(const Cand* __restrict__ cand_all, const unsigned* __restrict__ count, const uint8_t* __restrict__ det, GridArgs g,
                                                 float2* __restrict__ corners, int* __restrict__ gstat) {
  __shared__ float s_x[MCBA_DETECT_MAX_CANDIDATES], s_y[MCBA_DETECT_MAX_CANDIDATES], s_r[MCBA_DETECT_MAX_CANDIDATES];
  __shared__ int s_key[MCBA_DETECT_MAX_CANDIDATES];
  __shared__ uint8_t s_used[MCBA_DETECT_MAX_CANDIDATES];
  __shared__ short s_grid[kGridSide * kGridSide];
  __shared__ short s_q[kMaxFill];
  const int lane = threadIdx.x, b = blockIdx.x;
  const unsigned nc = count[b];
  if (nc > MCBA_DETECT_MAX_CANDIDATES) {
    if (lane == 0) gstat[b] = kStatusOverflow;
    return;
  }
  const int n = (int)nc;
  const Cand* cand = cand_all + (size_t)b * MCBA_DETECT_MAX_CANDIDATES;
  for (int i = lane; i < n; i += 64) {
    const Cand c = cand[i];
    s_x[i] = c.x; s_y[i] = c.y; s_r[i] = c.r; s_key[i] = c.key;
    s_used[i] = 0;
  }
  __syncthreads();
  const uint8_t* img = det + (size_t)b * g.Wd * g.Hd;
  const int N = g.rows * g.cols;
  int tried[kDetSeeds];
  int found = 0;
  for (int si = 0; si < kDetSeeds && !found; ++si) {
    // seed: the largest R not tried yet (ties: lower pixel index) -- as an argmin of (-R, key)
    float bd = 3.0e38f;
    int bk = 0x7fffffff, bi = -1;
    for (int i = lane; i < n; i += 64) {
      bool t = false;
      for (int k = 0; k < si; ++k) t |= tried[k] == i;
      if (!t && (-s_r[i] < bd || (-s_r[i] == bd && s_key[i] < bk))) { bd = -s_r[i]; bk = s_key[i]; bi = i; }
    }
    wave_argmin(bd, bk, bi);
    if (bi < 0) break;
    tried[si] = bi;
    const int s = bi;
    const float sx = s_x[s], sy = s_y[s];
    // lattice steps: nearest neighbour a, nearest at 50..130 degrees to a: b
    bd = 3.0e38f; bk = 0x7fffffff; int n1 = -1;
    for (int i = lane; i < n; i += 64) {
      if (i == s) continue;
      const float dx = s_x[i] - sx, dy = s_y[i] - sy, d = dx * dx + dy * dy;
      if (d < bd || (d == bd && s_key[i] < bk)) { bd = d; bk = s_key[i]; n1 = i; }
    }
    wave_argmin(bd, bk, n1);
    if (n1 < 0) continue;
    const float ax = s_x[n1] - sx, ay = s_y[n1] - sy, la2 = ax * ax + ay * ay;
    bd = 3.0e38f; bk = 0x7fffffff; int n2 = -1;
    for (int i = lane; i < n; i += 64) {
      if (i == s || i == n1) continue;
      const float dx = s_x[i] - sx, dy = s_y[i] - sy, d = dx * dx + dy * dy;
      const float dot = dx * ax + dy * ay;
      if (dot * dot > 0.41317591f * d * la2) continue;  // |cos| > cos 50 deg
      if (d < bd || (d == bd && s_key[i] < bk)) { bd = d; bk = s_key[i]; n2 = i; }
    }
    wave_argmin(bd, bk, n2);
    if (n2 < 0) continue;
    const float bxs = s_x[n2] - sx, bys = s_y[n2] - sy;
    for (int i = lane; i < kGridSide * kGridSide; i += 64) s_grid[i] = -1;
    for (int i = lane; i < n; i += 64) s_used[i] = 0;
    __syncthreads();
    const int c0 = 32 * kGridSide + 32;
    if (lane == 0) {
      s_grid[c0] = (short)s; s_grid[c0 + 1] = (short)n1; s_grid[c0 + kGridSide] = (short)n2;
      s_used[s] = 1; s_used[n1] = 1; s_used[n2] = 1;
      s_q[0] = (short)c0; s_q[1] = (short)(c0 + 1); s_q[2] = (short)(c0 + kGridSide);
    }
    __syncthreads();
    int head = 0, tail = 3;
    bool bad = false;
    while (head < tail && !bad) {
      const int c = s_q[head++];
      const int ci = c / kGridSide, cj = c % kGridSide;
      for (int dir = 0; dir < 4 && !bad; ++dir) {
        const int di = dir == 2 ? 1 : (dir == 3 ? -1 : 0), dj = dir == 0 ? 1 : (dir == 1 ? -1 : 0);
        const int ni = ci + di, nj = cj + dj;
        if (ni < 0 || nj < 0 || ni >= kGridSide || nj >= kGridSide) { bad = true; break; }
        if (s_grid[ni * kGridSide + nj] >= 0) continue;
        const int pc = s_grid[c];
        const float px = s_x[pc], py = s_y[pc];
        float qx, qy, L;
        const int bi2 = ci - di, bj2 = cj - dj;
        const int back = (bi2 >= 0 && bj2 >= 0 && bi2 < kGridSide && bj2 < kGridSide) ? s_grid[bi2 * kGridSide + bj2] : -1;
        int e0 = -1, e1 = -1;
        if (back < 0) {  // parallelogram: a neighbour row / column that already holds the step
          for (int side = 0; side < 2 && e0 < 0; ++side) {
            const int ei = ci + (di == 0 ? (side ? -1 : 1) : 0), ej = cj + (dj == 0 ? (side ? -1 : 1) : 0);
            if (ei < 0 || ej < 0 || ei >= kGridSide || ej >= kGridSide || ei + di < 0 || ej + dj < 0 || ei + di >= kGridSide || ej + dj >= kGridSide) continue;
            const int a0 = s_grid[ei * kGridSide + ej], a1 = s_grid[(ei + di) * kGridSide + ej + dj];
            if (a0 >= 0 && a1 >= 0) { e0 = a0; e1 = a1; }
          }
        }
        if (back >= 0) {
          const float vx = px - s_x[back], vy = py - s_y[back];
          qx = px + vx; qy = py + vy; L = sqrtf(vx * vx + vy * vy);
        } else if (e0 >= 0) {
          const float vx = s_x[e1] - s_x[e0], vy = s_y[e1] - s_y[e0];
          qx = px + vx; qy = py + vy; L = sqrtf(vx * vx + vy * vy);
        } else {
          const float vx = dj != 0 ? dj * ax : di * bxs, vy = dj != 0 ? dj * ay : di * bys;
          qx = px + vx; qy = py + vy; L = sqrtf(vx * vx + vy * vy);
        }
        float d = 3.0e38f;
        int k = 0x7fffffff, idx = -1;
        for (int i = lane; i < n; i += 64) {
          if (s_used[i]) continue;
          const float dx = s_x[i] - qx, dy = s_y[i] - qy, dd = dx * dx + dy * dy;
          if (dd < d || (dd == d && s_key[i] < k)) { d = dd; k = s_key[i]; idx = i; }
        }
        wave_argmin(d, k, idx);
        const float tol = kAcceptFrac * L;
        if (idx >= 0 && d < tol * tol) {
          if (tail >= kMaxFill) { bad = true; break; }
          __syncthreads();
          if (lane == 0) {
            s_grid[ni * kGridSide + nj] = (short)idx;
            s_used[idx] = 1;
            s_q[tail] = (short)(ni * kGridSide + nj);
          }
          __syncthreads();
          ++tail;
        }
      }
    }
    if (bad || tail != N) continue;
    // bounding box of the filled cells
    int imin = kGridSide, imax = -1, jmin = kGridSide, jmax = -1;
    for (int t = 0; t < tail; ++t) {
      const int c = s_q[t], ci = c / kGridSide, cj = c % kGridSide;
      imin = min(imin, ci); imax = max(imax, ci); jmin = min(jmin, cj); jmax = max(jmax, cj);
    }
    const int ni = imax - imin + 1, nj = jmax - jmin + 1;
    bool rows_i;
    if (ni == g.rows && nj == g.cols) rows_i = true;
    else if (ni == g.cols && nj == g.rows) rows_i = false;
    else continue;
    if (ni * nj != tail) continue;
    // checkerboard test: cell centres alternate dark / light
    float lo0 = 1e30f, hi0 = -1e30f, lo1 = 1e30f, hi1 = -1e30f;
    for (int t = lane; t < (ni - 1) * (nj - 1); t += 64) {
      const int i = imin + t / (nj - 1), j = jmin + t % (nj - 1);
      const int q0 = s_grid[i * kGridSide + j], q1 = s_grid[i * kGridSide + j + 1], q2 = s_grid[(i + 1) * kGridSide + j], q3 = s_grid[(i + 1) * kGridSide + j + 1];
      const float mx = 0.25f * (s_x[q0] + s_x[q1] + s_x[q2] + s_x[q3]), my = 0.25f * (s_y[q0] + s_y[q1] + s_y[q2] + s_y[q3]);
      const float v = sample_clamped(img, g.Wd, g.Hd, mx, my);
      if (((i + j) & 1) == 0) { lo0 = fminf(lo0, v); hi0 = fmaxf(hi0, v); }
      else { lo1 = fminf(lo1, v); hi1 = fmaxf(hi1, v); }
    }
    if ((ni - 1) * (nj - 1) == 1 && lane < 4) {  // a 2 x 2 board has one cell: its four edge neighbours (outer squares) are the other colour
      const int q0 = s_grid[imin * kGridSide + jmin], q1 = s_grid[imin * kGridSide + jmin + 1], q2 = s_grid[(imin + 1) * kGridSide + jmin],
                q3 = s_grid[(imin + 1) * kGridSide + jmin + 1];
      const float cx = 0.25f * (s_x[q0] + s_x[q1] + s_x[q2] + s_x[q3]), cy = 0.25f * (s_y[q0] + s_y[q1] + s_y[q2] + s_y[q3]);
      const int ea = lane == 0 ? q0 : (lane == 1 ? q2 : (lane == 2 ? q0 : q1)), eb = lane == 0 ? q1 : (lane == 1 ? q3 : (lane == 2 ? q2 : q3));
      const float v = sample_clamped(img, g.Wd, g.Hd, s_x[ea] + s_x[eb] - cx, s_y[ea] + s_y[eb] - cy);  // 2 (edge midpoint) - centre
      if (((imin + jmin) & 1) == 0) { lo1 = fminf(lo1, v); hi1 = fmaxf(hi1, v); }
      else { lo0 = fminf(lo0, v); hi0 = fmaxf(hi0, v); }
    }
    lo0 = wave_minf(lo0); hi0 = wave_maxf(hi0); lo1 = wave_minf(lo1); hi1 = wave_maxf(hi1);
    if (!(lo0 - hi1 >= kCellGap || lo1 - hi0 >= kCellGap)) continue;
    if (g.rows == g.cols) {  // square board: the transposition that is right-handed in the image, cross(d_col, d_row) > 0
      const int q00 = s_grid[imin * kGridSide + jmin], q01 = s_grid[imin * kGridSide + jmin + 1], q10 = s_grid[(imin + 1) * kGridSide + jmin];
      const float ux = s_x[q01] - s_x[q00], uy = s_y[q01] - s_y[q00];  // along j
      const float vx = s_x[q10] - s_x[q00], vy = s_y[q10] - s_y[q00];  // along i
      rows_i = ux * vy - uy * vx > 0.f;  // rows along i, columns along j: d_col = u, d_row = v
    }
    const float inv = 1.f / g.scale;
    for (int k = lane; k < N; k += 64) {
      const int r = k / g.cols, c = k % g.cols;
      const int i = rows_i ? imin + r : imin + c, j = rows_i ? jmin + c : jmin + r;
      const int q = s_grid[i * kGridSide + j];
      corners[(size_t)b * N + k] = make_float2((s_x[q] + 0.5f) * inv - 0.5f, (s_y[q] + 0.5f) * inv - 0.5f);
    }
    found = 1;
  }
  if (lane == 0) gstat[b] = found;
}

// one wavefront per corner (blocks of 64).  start / out: frames x N float2; gstat (may be NULL): frames whose entry is not 1 are skipped
__global__ __launch_bounds__(64) void k_det_subpix(const uint8_t* __restrict__ grey, int W, int H, const float2* __restrict__ start, int N, const int* __restrict__ gstat,
                                                   int ww, int wh, float2* __restrict__ out) {
  __shared__ float s_patch[(2 * MCBA_DETECT_MAX_WINDOW + 3) * (2 * MCBA_DETECT_MAX_WINDOW + 3)];
  __shared__ float s_mask[(2 * MCBA_DETECT_MAX_WINDOW + 1) * (2 * MCBA_DETECT_MAX_WINDOW + 1)];
  const int g = blockIdx.x, lane = threadIdx.x;
  const int b = g / N;
  if (gstat && gstat[b] != 1) return;
  const uint8_t* img = grey + (size_t)b * W * H;
  const int win_w = 2 * ww + 1, win_h = 2 * wh + 1, pw = win_w + 2, ph = win_h + 2;
  for (int k = lane; k < win_w * win_h; k += 64) s_mask[k] = det::subpix_mask(k / win_w, k % win_w, ww, wh);
  const float2 c0 = start[g];
  float x = c0.x, y = c0.y;
  for (int iter = 0; iter < det::kSubpixMaxIter; ++iter) {
    __syncthreads();
    for (int k = lane; k < pw * ph; k += 64) s_patch[k] = det::rect_subpix(img, W, H, x, y, pw, ph, k / pw, k % pw);
    __syncthreads();
    det::SubpixSums s{0, 0, 0, 0, 0};
    for (int k = lane; k < win_w * win_h; k += 64) det::subpix_term(s_patch, ww, wh, k / win_w, k % win_w, s_mask[k], s);
    double v[5] = {s.a, s.b, s.c, s.bb1, s.bb2};
#pragma unroll
    for (int q = 0; q < 5; ++q) {
#pragma unroll
      for (int off = 32; off >= 1; off >>= 1) v[q] += __shfl_xor(v[q], off, 64);
      v[q] = __shfl(v[q], 0, 64);  // (lane 0's association order for every lane: the iteration stays wave-uniform)
    }
    const det::SubpixSums t{v[0], v[1], v[2], v[3], v[4]};
    double err = 0.0;
    if (!det::subpix_update(t, x, y, err)) break;
    if (det::subpix_outside(x, y, W, H)) break;
    if (!(err > det::kSubpixEps2)) break;
  }
  if (fabsf(x - c0.x) > (float)ww || fabsf(y - c0.y) > (float)wh) { x = c0.x; y = c0.y; }
  if (lane == 0) out[g] = make_float2(x, y);
}

struct AnchorArgs {
  int W, H;
  int rows, cols;       // the layout of corners: rows x cols, row-major
  int try_transpose;    // square boards in the pipeline: also score the transposed layout, keep the one whose best region scores higher
  double min_diff;
};

// one workgroup of 256 per frame.  corners: frames x N float2 (layout order).  scores: frames x 4 (the chosen layout's, unsorted when
// sorted_out == 0, else sorted descending); status: 1 accepted / 2 ambiguous; reordered: frames x N float2.  regions (frames x 4 x 1600) and
// quads (frames x 4 x 4 float2) may be NULL.
__global__ __launch_bounds__(256) void k_det_anchor(const uint8_t* __restrict__ grey, const float2* __restrict__ corners, const int* __restrict__ gstat, AnchorArgs a,
                                                    double* __restrict__ scores, int sorted_out, int8_t* __restrict__ status, float2* __restrict__ reordered,
                                                    uint8_t* __restrict__ regions, float2* __restrict__ quads) {
  __shared__ double s_H[9], s_S[81], s_M[4][9];
  __shared__ double s_xy[2 * MCBA_DETECT_MAX_CORNERS], s_uv[2 * MCBA_DETECT_MAX_CORNERS];
  __shared__ det::DltNorm s_nm;
  __shared__ double s_sc[2][4];
  __shared__ float s_quad[4][4][2];
  __shared__ unsigned long long s_mom[4][3];
  const int tid = threadIdx.x, b = blockIdx.x;
  if (gstat && gstat[b] != 1) return;
  const int N = a.rows * a.cols;
  const float2* cp = corners + (size_t)b * N;
  const uint8_t* img = grey + (size_t)a.W * a.H * b;
  const int nv = a.try_transpose ? 2 : 1;
  for (int v = 0; v < nv; ++v) {
    const int rows = v ? a.cols : a.rows, cols = v ? a.rows : a.cols;
    // layout v, grid (r, c) -> corner index: v == 0: r * a.cols + c; v == 1 (transposed): c * a.cols + r.  xy of (r, c) = (c + 1, r + 3):
    // extend_grid(.., 3, 1)'s coordinates.  The DLT is csrc/mcba_detect_math.h's: normalisation and de-normalisation on one lane, one entry
    // of the normal matrix per lane
    for (int k = tid; k < N; k += 256) {
      const int r = v ? k % a.cols : k / a.cols, c = v ? k / a.cols : k % a.cols;
      s_xy[2 * k] = c + 1; s_xy[2 * k + 1] = r + 3;
      s_uv[2 * k] = cp[k].x; s_uv[2 * k + 1] = cp[k].y;
    }
    __syncthreads();
    if (tid == 0) s_nm = det::dlt_norm(s_xy, s_uv, N);
    __syncthreads();
    if (tid < 81) s_S[tid] = det::dlt_normal_entry(s_xy, s_uv, N, s_nm, tid);
    __syncthreads();
    if (tid == 0) {
      double S[81];
      for (int i = 0; i < 81; ++i) S[i] = s_S[i];
      det::dlt_finish(S, s_nm, s_H);
    }
    __syncthreads();
    if (tid < 16) {  // the quads' corners on the extended grid, as float32 (the reference's np.float32)
      const int k = tid / 4, q = tid % 4;
      int R, C;
      det::quad_cell(k, q, rows, cols, R, C);
      double u, w;
      det::apply_h(s_H, C, R, u, w);
      s_quad[k][q][0] = (float)u;
      s_quad[k][q][1] = (float)w;
    }
    if (tid < 12) s_mom[tid / 3][tid % 3] = 0ull;
    __syncthreads();
    if (tid < 4) {  // template -> image: template corners (0, 40), (0, 0), (40, 0), (40, 40) onto the quad's
      const double tpl[8] = {0, 40, 0, 0, 40, 0, 40, 40};
      double src[8];
      for (int q = 0; q < 4; ++q) { src[2 * q] = s_quad[tid][q][0]; src[2 * q + 1] = s_quad[tid][q][1]; }
      double M[9];
      if (!det::persp4(tpl, src, M))
        for (int i = 0; i < 9; ++i) M[i] = 0.0;
      for (int i = 0; i < 9; ++i) s_M[tid][i] = M[i];
    }
    __syncthreads();
    unsigned long long m[4][3] = {};
    for (int p = tid; p < 4 * det::kTemplate * det::kTemplate; p += 256) {
      const int k = p / (det::kTemplate * det::kTemplate), pix = p % (det::kTemplate * det::kTemplate);
      const int x = pix % det::kTemplate, y = pix / det::kTemplate;
      const uint8_t r = det::warp_pixel(img, a.W, a.H, s_M[k], x, y);
      const unsigned t = det::template_pixel(x, y);
      m[k][0] += r; m[k][1] += (unsigned)r * r; m[k][2] += (unsigned)r * t;
      if (regions && v == 0) regions[((size_t)b * 4 + k) * det::kTemplate * det::kTemplate + pix] = r;
    }
    for (int k = 0; k < 4; ++k)
      for (int j = 0; j < 3; ++j) atomicAdd(&s_mom[k][j], m[k][j]);  // (integer: exact in any order)
    if (quads && v == 0 && tid < 16) quads[(size_t)b * 16 + tid] = make_float2(s_quad[tid / 4][tid % 4][0], s_quad[tid / 4][tid % 4][1]);
    __syncthreads();
    if (tid < 4) {
      const double n = det::kTemplate * det::kTemplate, st = 255.0 * (n - 317.0), stt = 255.0 * 255.0 * (n - 317.0);
      s_sc[v][tid] = det::pearson(n, (double)s_mom[tid][0], st, (double)s_mom[tid][1], stt, (double)s_mom[tid][2]);
    }
    __syncthreads();
  }
  if (tid == 0) {
    int v = 0;
    if (nv == 2) {
      const double m0 = fmax(fmax(s_sc[0][0], s_sc[0][1]), fmax(s_sc[0][2], s_sc[0][3]));
      const double m1 = fmax(fmax(s_sc[1][0], s_sc[1][1]), fmax(s_sc[1][2], s_sc[1][3]));
      v = m1 > m0 ? 1 : 0;
    }
    double sc[4];
    for (int k = 0; k < 4; ++k) sc[k] = s_sc[v][k];
    int best = 0;
    for (int k = 1; k < 4; ++k)
      if (sc[k] > sc[best]) best = k;  // np.argmax: the first maximum
    double so[4] = {sc[0], sc[1], sc[2], sc[3]};
    for (int i = 0; i < 4; ++i)
      for (int j = i + 1; j < 4; ++j)
        if (so[j] > so[i]) { const double t = so[i]; so[i] = so[j]; so[j] = t; }
    for (int k = 0; k < 4; ++k) scores[(size_t)b * 4 + k] = sorted_out ? so[k] : sc[k];
    status[b] = (int8_t)(so[0] - so[1] < a.min_diff ? 2 : 1);
    s_sc[0][0] = (double)v;
    s_sc[0][1] = (double)best;
  }
  __syncthreads();
  if (reordered) {
    const int v = (int)s_sc[0][0], best = (int)s_sc[0][1];
    const int rows = v ? a.cols : a.rows, cols = v ? a.rows : a.cols;
    const bool fr = best == 2 || best == 3, fc = best == 1 || best == 2;
    for (int k = tid; k < N; k += 256) {
      const int r = k / cols, c = k % cols;
      const int sr = fr ? rows - 1 - r : r, sc = fc ? cols - 1 - c : c;
      const int src = v ? sc * a.cols + sr : sr * a.cols + sc;
      reordered[(size_t)b * N + k] = cp[src];
    }
  }
}

}  // namespace mcba

using namespace mcba_internal;

namespace {

int check_image(int height, int width, int channels) {
  if (height < 8 || width < 8 || height > MCBA_DETECT_MAX_IMAGE_SIDE || width > MCBA_DETECT_MAX_IMAGE_SIDE)
    return fail(MCBA_ERR_ARG, "mcba_detect: image sides must lie in 8 .. MCBA_DETECT_MAX_IMAGE_SIDE");
  if (channels != 1 && channels != 3) return fail(MCBA_ERR_ARG, "mcba_detect: 1 (grey) or 3 (BGR) channels");
  return MCBA_OK;
}

int check_board(int cols, int rows) {
  if (cols < 2 || rows < 2 || cols > MCBA_DETECT_MAX_BOARD_SIDE || rows > MCBA_DETECT_MAX_BOARD_SIDE || cols * rows > MCBA_DETECT_MAX_CORNERS)
    return fail(MCBA_ERR_ARG, "mcba_detect: board sides 2 .. MCBA_DETECT_MAX_BOARD_SIDE, at most MCBA_DETECT_MAX_CORNERS corners");
  return MCBA_OK;
}

// frames (B, H, W, C) on the device -> grey (B, H, W); for C == 1 the upload went into grey directly
int launch_prep(const uint8_t* d_in, int B, int H, int W, int C, uint8_t* d_grey) {
  if (C == 1) return MCBA_OK;
  const size_t n = (size_t)B * H * W;
  const size_t blocks = std::min<size_t>((n + 255) / 256, 65536);
  mcba::k_det_prep<<<dim3((unsigned)blocks), dim3(256)>>>(d_in, n, d_grey);
  return check_launch();
}

}  // namespace

extern "C" {

int mcba_detect_chessboards(int n_images, int height, int width, int channels, const unsigned char* images, int board_cols, int board_rows, int win_w, int win_h,
                            double scale_factor, int reorder, double match_score_min_diff, size_t memory_budget, int device, float* uvs_out, double* scores_out,
                            signed char* status_out, double* kernel_ms) {
  if (n_images < 0 || !images || !uvs_out || !scores_out || !status_out) return fail(MCBA_ERR_ARG, "mcba_detect_chessboards: non-NULL arrays required");
  if (int rc = check_image(height, width, channels)) return rc;
  if (int rc = check_board(board_cols, board_rows)) return rc;
  if (win_w < 1 || win_h < 1 || win_w > MCBA_DETECT_MAX_WINDOW || win_h > MCBA_DETECT_MAX_WINDOW || width < 2 * win_w + 5 || height < 2 * win_h + 5)
    return fail(MCBA_ERR_ARG, "mcba_detect_chessboards: half-window 1 .. MCBA_DETECT_MAX_WINDOW and no larger than the image allows");
  if (!(scale_factor > 0.0) || !(scale_factor <= 1.0)) return fail(MCBA_ERR_ARG, "mcba_detect_chessboards: scale_factor in (0, 1]");
  const int Wd = scale_factor == 1.0 ? width : (int)rint(width * scale_factor), Hd = scale_factor == 1.0 ? height : (int)rint(height * scale_factor);
  if (Wd < 16 || Hd < 16) return fail(MCBA_ERR_ARG, "mcba_detect_chessboards: the detection-scale image is smaller than 16 x 16");
  if (int rc = stateless_device(device)) return rc;
  if (n_images == 0) return MCBA_OK;
  const int N = board_cols * board_rows;
  const bool resized = scale_factor != 1.0;
  const size_t px = (size_t)width * height, pxd = (size_t)Wd * Hd;
  const size_t per_frame = px * channels + (channels == 3 ? px : 0) + (resized ? pxd : 0) + 4 * pxd + MCBA_DETECT_MAX_CANDIDATES * sizeof(mcba::Cand) +
                           4 * N * sizeof(float2) + 64;
  const size_t budget = memory_budget ? memory_budget : ((size_t)256 << 20);
  // (at most 65 535 frames per chunk: the grid's z dimension of the per-pixel launches)
  int chunk = (int)std::min<size_t>(std::min<size_t>(std::max<size_t>(budget / per_frame, 1), (size_t)n_images), 65535);
  StatelessCall call;
  uint8_t *d_in = nullptr, *d_grey = nullptr, *d_det = nullptr;
  float* d_resp = nullptr;
  unsigned *d_rmax = nullptr, *d_cnt = nullptr;
  mcba::Cand* d_cand = nullptr;
  float2 *d_start = nullptr, *d_ref = nullptr, *d_out = nullptr;
  int* d_gstat = nullptr;
  double* d_scores = nullptr;
  int8_t* d_status = nullptr;
  if (int rc = call.scratch(&d_in, (size_t)chunk * px * channels)) return rc;   // staging: every chunk's put() below fills the B images that its kernels read
  d_grey = d_in;
  if (channels == 3)
    if (int rc = call.scratch(&d_grey, (size_t)chunk * px)) return rc;
  d_det = d_grey;
  if (resized)
    if (int rc = call.scratch(&d_det, (size_t)chunk * pxd)) return rc;
  if (int rc = call.scratch(&d_resp, (size_t)chunk * pxd)) return rc;
  if (int rc = call.scratch(&d_rmax, (size_t)chunk)) return rc;
  if (int rc = call.scratch(&d_cnt, (size_t)chunk)) return rc;
  if (int rc = call.scratch(&d_cand, (size_t)chunk * MCBA_DETECT_MAX_CANDIDATES)) return rc;
  if (int rc = call.scratch(&d_start, (size_t)chunk * N)) return rc;
  if (int rc = call.scratch(&d_ref, (size_t)chunk * N)) return rc;
  if (int rc = call.scratch(&d_out, (size_t)chunk * N)) return rc;
  if (int rc = call.scratch(&d_gstat, (size_t)chunk)) return rc;
  if (int rc = call.scratch(&d_scores, (size_t)chunk * 4)) return rc;
  if (int rc = call.scratch(&d_status, (size_t)chunk)) return rc;
  std::vector<int> gstat(chunk);
  std::vector<int8_t> st(chunk);
  std::vector<float2> uv((size_t)chunk * N);
  std::vector<double> sc((size_t)chunk * 4);
  HIPCHK(call.start());
  double total_ms = 0.0;
  const bool square = board_cols == board_rows;
  for (int f0 = 0; f0 < n_images; f0 += chunk) {
    const int B = std::min(chunk, n_images - f0);
    if (int rc = call.put(d_in, images + (size_t)f0 * px * channels, (size_t)B * px * channels)) return rc;
    HIPCHK(hipMemset(d_rmax, 0, (size_t)B * sizeof(unsigned)));
    HIPCHK(hipMemset(d_cnt, 0, (size_t)B * sizeof(unsigned)));
    HIPCHK(hipEventRecord(call.e0, nullptr));
    if (int rc = launch_prep(d_in, B, height, width, channels, d_grey)) return rc;
    if (resized) {
      mcba::k_det_resize<<<dim3((unsigned)((Wd + 255) / 256), (unsigned)Hd, (unsigned)B), dim3(256)>>>(d_grey, width, height, d_det, Wd, Hd, (float)(1.0 / scale_factor));
      if (int rc = check_launch()) return rc;
    }
    const dim3 tiles((unsigned)((Wd + mcba::kDetTile - 1) / mcba::kDetTile), (unsigned)((Hd + mcba::kDetTile - 1) / mcba::kDetTile), (unsigned)B);
    mcba::k_det_saddle<<<tiles, dim3(256)>>>(d_det, Wd, Hd, d_resp, d_rmax);
    if (int rc = check_launch()) return rc;
    mcba::k_det_nms<<<tiles, dim3(256)>>>(d_resp, d_det, Wd, Hd, d_rmax, d_cnt, d_cand);
    if (int rc = check_launch()) return rc;
    const mcba::GridArgs ga{Wd, Hd, width, height, (float)scale_factor, board_rows, board_cols};
    mcba::k_det_grid<<<dim3((unsigned)B), dim3(64)>>>(d_cand, d_cnt, d_det, ga, d_start, d_gstat);
    if (int rc = check_launch()) return rc;
    mcba::k_det_subpix<<<dim3((unsigned)(B * N)), dim3(64)>>>(d_grey, width, height, d_start, N, d_gstat, win_w, win_h, d_ref);
    if (int rc = check_launch()) return rc;
    if (reorder) {
      const mcba::AnchorArgs aa{width, height, board_rows, board_cols, square ? 1 : 0, match_score_min_diff};
      mcba::k_det_anchor<<<dim3((unsigned)B), dim3(256)>>>(d_grey, d_ref, d_gstat, aa, d_scores, 1, d_status, d_out, nullptr, nullptr);
      if (int rc = check_launch()) return rc;
    }
    HIPCHK(hipEventRecord(call.e1, nullptr));
    HIPCHK(hipEventSynchronize(call.e1));
    float ms = 0.f;
    HIPCHK(hipEventElapsedTime(&ms, call.e0, call.e1));
    total_ms += ms;
    if (int rc = call.download(gstat.data(), d_gstat, (size_t)B)) return rc;
    if (int rc = call.download(uv.data(), reorder ? d_out : d_ref, (size_t)B * N)) return rc;
    if (reorder) {
      if (int rc = call.download(st.data(), d_status, (size_t)B)) return rc;
      if (int rc = call.download(sc.data(), d_scores, (size_t)B * 4)) return rc;
    }
    for (int b = 0; b < B; ++b) {
      const size_t f = (size_t)f0 + b;
      const int g = gstat[b];
      const int s = g != 1 ? (g == mcba::kStatusOverflow ? mcba::kStatusOverflow : 0) : (reorder ? st[b] : 1);
      status_out[f] = (signed char)s;
      const bool grid = g == 1 && reorder;
      for (int k = 0; k < 4; ++k) scores_out[f * 4 + k] = grid ? sc[(size_t)b * 4 + k] : NAN;
      for (int k = 0; k < N; ++k) {
        uvs_out[(f * N + k) * 2] = s == 1 ? uv[(size_t)b * N + k].x : NAN;
        uvs_out[(f * N + k) * 2 + 1] = s == 1 ? uv[(size_t)b * N + k].y : NAN;
      }
    }
  }
  if (kernel_ms) *kernel_ms = total_ms;
  return MCBA_OK;
}

int mcba_detect_subpix(int height, int width, int channels, const unsigned char* image, int n_corners, const float* start, int win_w, int win_h, int device, float* out,
                       double* kernel_ms) {
  if (!image || n_corners < 0 || (n_corners && (!start || !out))) return fail(MCBA_ERR_ARG, "mcba_detect_subpix: non-NULL arrays required");
  if (int rc = check_image(height, width, channels)) return rc;
  if (win_w < 1 || win_h < 1 || win_w > MCBA_DETECT_MAX_WINDOW || win_h > MCBA_DETECT_MAX_WINDOW || width < 2 * win_w + 5 || height < 2 * win_h + 5)
    return fail(MCBA_ERR_ARG, "mcba_detect_subpix: half-window 1 .. MCBA_DETECT_MAX_WINDOW and no larger than the image allows");
  if (int rc = stateless_device(device)) return rc;
  if (n_corners == 0) return MCBA_OK;
  const size_t px = (size_t)width * height;
  StatelessCall call;
  uint8_t *d_in = nullptr, *d_grey = nullptr;
  float2 *d_start = nullptr, *d_out = nullptr;
  if (int rc = call.upload(&d_in, image, px * channels)) return rc;
  d_grey = d_in;
  if (channels == 3)
    if (int rc = call.scratch(&d_grey, px)) return rc;
  if (int rc = call.upload(&d_start, reinterpret_cast<const float2*>(start), (size_t)n_corners)) return rc;
  if (int rc = call.scratch(&d_out, (size_t)n_corners)) return rc;
  HIPCHK(call.start());
  if (int rc = launch_prep(d_in, 1, height, width, channels, d_grey)) return rc;
  mcba::k_det_subpix<<<dim3((unsigned)n_corners), dim3(64)>>>(d_grey, width, height, d_start, n_corners, nullptr, win_w, win_h, d_out);
  if (int rc = check_launch()) return rc;
  HIPCHK(call.stop(kernel_ms));
  return call.download(reinterpret_cast<float2*>(out), d_out, (size_t)n_corners);
}

int mcba_detect_anchor(int height, int width, int channels, const unsigned char* image, int board_cols, int board_rows, const float* uvs, int device, double* scores_out,
                       unsigned char* regions_out, float* quads_out, double* kernel_ms) {
  if (!image || !uvs || !scores_out) return fail(MCBA_ERR_ARG, "mcba_detect_anchor: non-NULL arrays required");
  if (int rc = check_image(height, width, channels)) return rc;
  if (int rc = check_board(board_cols, board_rows)) return rc;
  if (int rc = stateless_device(device)) return rc;
  const int N = board_cols * board_rows;
  const size_t px = (size_t)width * height;
  StatelessCall call;
  uint8_t *d_in = nullptr, *d_grey = nullptr, *d_reg = nullptr;
  float2 *d_uv = nullptr, *d_quad = nullptr;
  double* d_sc = nullptr;
  int8_t* d_st = nullptr;
  if (int rc = call.upload(&d_in, image, px * channels)) return rc;
  d_grey = d_in;
  if (channels == 3)
    if (int rc = call.scratch(&d_grey, px)) return rc;
  if (int rc = call.upload(&d_uv, reinterpret_cast<const float2*>(uvs), (size_t)N)) return rc;
  if (int rc = call.scratch(&d_sc, 4)) return rc;
  if (int rc = call.scratch(&d_st, 1)) return rc;
  if (int rc = call.scratch(&d_reg, 4 * 1600)) return rc;
  if (int rc = call.scratch(&d_quad, 16)) return rc;
  HIPCHK(call.start());
  if (int rc = launch_prep(d_in, 1, height, width, channels, d_grey)) return rc;
  const mcba::AnchorArgs aa{width, height, board_rows, board_cols, 0, 0.0};
  mcba::k_det_anchor<<<dim3(1), dim3(256)>>>(d_grey, d_uv, nullptr, aa, d_sc, 0, d_st, nullptr, d_reg, d_quad);
  if (int rc = check_launch()) return rc;
  HIPCHK(call.stop(kernel_ms));
  if (int rc = call.download(scores_out, d_sc, 4)) return rc;
  if (regions_out)
    if (int rc = call.download(regions_out, d_reg, 4 * 1600)) return rc;
  return quads_out ? call.download(reinterpret_cast<float2*>(quads_out), d_quad, 16) : MCBA_OK;
}

}  // extern "C"
