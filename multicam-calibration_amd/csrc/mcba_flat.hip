// mcba_flat.hip -- floor-plane alignment ("flatibration"; reference flatibration.py) on the device.
//
// Three stateless entry points (include/mcba.h, "floor-plane alignment"), each one upload, its kernels and one download:
//   mcba_flat_floor_points  per frame the keypoint of smallest (largest) z -- np.argmin / np.argmax semantics: first index on ties,
//                           the first NaN wins, an all-NaN frame gives index 0.  Each block stages a contiguous slab of whole frames
//                           through LDS with 16-B loads (consecutive lanes, consecutive bytes), then one lane scans one frame.
//   mcba_flat_ransac        every RANSAC hypothesis z = a x + b y + c against every point in ONE launch: the hypotheses sit in LDS,
//                           each lane keeps 4 points in registers and loops over the hypotheses; per hypothesis the exact inlier count
//                           and nine moments of the inliers (below) are reduced lane -> wavefront (xor butterfly) -> workgroup (LDS,
//                           waves in index order) -> per-block partials, then one block per hypothesis sums the partials in a fixed
//                           tree.  No floating-point atomics: the result depends on n alone, bit for bit.
//   mcba_flat_order_stats   transform the points (R p + t), keep x and y on the device, and find the requested order statistics of
//                           each by the radix select of mcba_diag.hip (launch_select: both coordinates, all ranks in the same 8 passes,
//                           enqueued back to back without a host wait).  Also the per-coordinate sums (fixed-order per-block partials)
//                           and NaN counts.
//
// Moments of the inliers of hypothesis h, in a per-call shift (sx, sy) for x, y and in the hypothesis' own residual r = z - (a x + b y + c)
// for z (inliers have |r| <= threshold, so nothing cancels): X = sum dx, Y = sum dy, R = sum r, XX, XY, YY, XR, YR, RR.
#include <stdint.h>

#include "mcba_device.h"
#include "mcba_handle.h"

namespace mcba {

constexpr int kFlatThreads = 256;
constexpr int kFloorLdsDoubles = 6144;  // 48 KiB of staged frames per block
constexpr int kScorePPT = 4;            // points per lane in the scoring kernel
constexpr int kScorePoints = kFlatThreads * kScorePPT;
constexpr int kMom = 9;                 // X Y R XX XY YY XR YR RR

__global__ __launch_bounds__(kFlatThreads) void k_floor_points(const double* __restrict__ kp, size_t n_frames, int K, int fpb, int down, double* __restrict__ out,
                                                               int* __restrict__ idx) {
  extern __shared__ double2 s_floor2[];
  double* s_kp = reinterpret_cast<double*>(s_floor2);
  const size_t f0 = (size_t)blockIdx.x * fpb;
  const int nf = (int)(n_frames - f0 < (size_t)fpb ? n_frames - f0 : (size_t)fpb);
  const int row = 3 * K;
  const size_t base = f0 * row;
  const int nd = nf * row;
  const double* src = kp + base;
  if ((base & 1) == 0) {  // 16-B aligned (the device buffer is): double2 loads, one trailing double
    const double2* s2 = reinterpret_cast<const double2*>(src);
    for (int i = threadIdx.x; i < (nd >> 1); i += kFlatThreads) s_floor2[i] = s2[i];
    if ((nd & 1) && threadIdx.x == 0) s_kp[nd - 1] = src[nd - 1];
  } else {
    for (int i = threadIdx.x; i < nd; i += kFlatThreads) s_kp[i] = src[i];
  }
  __syncthreads();
  for (int f = threadIdx.x; f < nf; f += kFlatThreads) {
    const double* fr = s_kp + (size_t)f * row;
    double best = fr[2];
    int bi = 0;
    // np.argmin / np.argmax: strict comparison keeps the first of equal values; a NaN is taken at once and ends the scan
    for (int k = 1; k < K && best == best; ++k) {
      const double v = fr[3 * k + 2];
      if (v != v || (down ? v > best : v < best)) { best = v; bi = k; }
    }
    const size_t g = f0 + f;
    idx[g] = bi;
    out[3 * g] = fr[3 * bi];
    out[3 * g + 1] = fr[3 * bi + 1];
    out[3 * g + 2] = fr[3 * bi + 2];
  }
}

// the inlier test of RANSAC: |z - (x a + y b + c)| <= threshold (sklearn: absolute_error loss, X @ coef_ + intercept_)
__device__ __forceinline__ double plane_residual(double x, double y, double z, double a, double b, double c) { return z - (fma(y, b, x * a) + c); }

// grid: ceil(n / kScorePoints) blocks.  part_m: blocks x H x kMom, part_n: blocks x H
__global__ __launch_bounds__(kFlatThreads) void k_ransac_score(const double* __restrict__ pts, size_t n, const double* __restrict__ planes, int H, double thr, double sx, double sy,
                                                               double* __restrict__ part_m, unsigned* __restrict__ part_n) {
  __shared__ double s_plane[MCBA_FLAT_MAX_HYPOTHESES * 3];
  __shared__ double s_m[kFlatThreads / 64][MCBA_FLAT_MAX_HYPOTHESES][kMom];
  __shared__ unsigned s_n[kFlatThreads / 64][MCBA_FLAT_MAX_HYPOTHESES];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  for (int i = tid; i < 3 * H; i += kFlatThreads) s_plane[i] = planes[i];
  double x[kScorePPT], y[kScorePPT], z[kScorePPT], dx[kScorePPT], dy[kScorePPT];
  bool ok[kScorePPT];
  const size_t p0 = (size_t)blockIdx.x * kScorePoints;
#pragma unroll
  for (int j = 0; j < kScorePPT; ++j) {
    const size_t p = p0 + (size_t)j * kFlatThreads + tid;
    ok[j] = p < n;
    x[j] = ok[j] ? pts[3 * p] : 0.0;
    y[j] = ok[j] ? pts[3 * p + 1] : 0.0;
    z[j] = ok[j] ? pts[3 * p + 2] : 0.0;
    dx[j] = x[j] - sx;
    dy[j] = y[j] - sy;
  }
  __syncthreads();
  for (int h = 0; h < H; ++h) {
    const double a = s_plane[3 * h], b = s_plane[3 * h + 1], c = s_plane[3 * h + 2];
    unsigned cnt = 0;
    double m[kMom];
#pragma unroll
    for (int k = 0; k < kMom; ++k) m[k] = 0.0;
#pragma unroll
    for (int j = 0; j < kScorePPT; ++j) {
      const double r = plane_residual(x[j], y[j], z[j], a, b, c);
      const bool in = ok[j] && fabs(r) <= thr;
      const double u = in ? dx[j] : 0.0, v = in ? dy[j] : 0.0, w = in ? r : 0.0;
      cnt += in ? 1u : 0u;
      m[0] += u; m[1] += v; m[2] += w;
      m[3] = fma(u, u, m[3]); m[4] = fma(u, v, m[4]); m[5] = fma(v, v, m[5]);
      m[6] = fma(u, w, m[6]); m[7] = fma(v, w, m[7]); m[8] = fma(w, w, m[8]);
    }
    cnt = wave_sum(cnt);
#pragma unroll
    for (int k = 0; k < kMom; ++k) m[k] = wave_sum(m[k]);
    if (lane == 0) {
      s_n[wave][h] = cnt;
#pragma unroll
      for (int k = 0; k < kMom; ++k) s_m[wave][h][k] = m[k];
    }
  }
  __syncthreads();
  double* pm = part_m + (size_t)blockIdx.x * H * kMom;
  for (int i = tid; i < H * kMom; i += kFlatThreads) {
    const int h = i / kMom, k = i - h * kMom;
    double v = s_m[0][h][k];
#pragma unroll
    for (int w = 1; w < kFlatThreads / 64; ++w) v += s_m[w][h][k];
    pm[i] = v;
  }
  for (int h = tid; h < H; h += kFlatThreads) {
    unsigned v = 0;
#pragma unroll
    for (int w = 0; w < kFlatThreads / 64; ++w) v += s_n[w][h];
    part_n[(size_t)blockIdx.x * H + h] = v;
  }
}

// one block per hypothesis: lane t sums the partials of blocks t, t + 256, ... in order, then a fixed LDS tree
__global__ __launch_bounds__(kFlatThreads) void k_ransac_finish(const double* __restrict__ part_m, const unsigned* __restrict__ part_n, int nblk, int H, double* __restrict__ mom,
                                                                unsigned long long* __restrict__ counts) {
  __shared__ double s_r[kMom][kFlatThreads];
  __shared__ unsigned long long s_c[kFlatThreads];
  const int h = blockIdx.x, tid = threadIdx.x;
  double m[kMom];
#pragma unroll
  for (int k = 0; k < kMom; ++k) m[k] = 0.0;
  unsigned long long c = 0;
  for (int bk = tid; bk < nblk; bk += kFlatThreads) {
    const double* src = part_m + ((size_t)bk * H + h) * kMom;
#pragma unroll
    for (int k = 0; k < kMom; ++k) m[k] += src[k];
    c += part_n[(size_t)bk * H + h];
  }
#pragma unroll
  for (int k = 0; k < kMom; ++k) s_r[k][tid] = m[k];
  s_c[tid] = c;
  __syncthreads();
  for (int s = kFlatThreads / 2; s >= 1; s >>= 1) {
    if (tid < s) {
#pragma unroll
      for (int k = 0; k < kMom; ++k) s_r[k][tid] += s_r[k][tid + s];
      s_c[tid] += s_c[tid + s];
    }
    __syncthreads();
  }
  if (tid < kMom) mom[(size_t)h * kMom + tid] = s_r[tid][0];
  if (tid == 0) counts[h] = s_c[0];
}

__global__ __launch_bounds__(kFlatThreads) void k_ransac_mask(const double* __restrict__ pts, size_t n, double a, double b, double c, double thr, unsigned char* __restrict__ mask) {
  const size_t p = (size_t)blockIdx.x * kFlatThreads + threadIdx.x;
  if (p >= n) return;
  mask[p] = fabs(plane_residual(pts[3 * p], pts[3 * p + 1], pts[3 * p + 2], a, b, c)) <= thr ? 1 : 0;
}

// rt12: R row-major (9) + t (3).  xy: 2 x n (x then y).  part_s: blocks x 2 (per-block sums, fixed order); nan2: NaN counts
__global__ __launch_bounds__(kFlatThreads) void k_flat_transform(const double* __restrict__ pts, size_t n, const double* __restrict__ rt12, double* __restrict__ xy,
                                                                 double* __restrict__ part_s, unsigned long long* __restrict__ nan2) {
  __shared__ double s_s[2][kFlatThreads / 64];
  __shared__ unsigned s_nan[2][kFlatThreads / 64];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const size_t p = (size_t)blockIdx.x * kFlatThreads + tid;
  double X = 0.0, Y = 0.0;
  unsigned nx = 0, ny = 0;
  if (p < n) {
    const double px = pts[3 * p], py = pts[3 * p + 1], pz = pts[3 * p + 2];
    X = rt12[0] * px + rt12[1] * py + rt12[2] * pz + rt12[9];
    Y = rt12[3] * px + rt12[4] * py + rt12[5] * pz + rt12[10];
    xy[p] = X;
    xy[n + p] = Y;
    nx = X != X ? 1u : 0u;
    ny = Y != Y ? 1u : 0u;
  }
  X = wave_sum(X);
  Y = wave_sum(Y);
  nx = wave_sum(nx);
  ny = wave_sum(ny);
  if (lane == 0) { s_s[0][wave] = X; s_s[1][wave] = Y; s_nan[0][wave] = nx; s_nan[1][wave] = ny; }
  __syncthreads();
  if (tid < 2) {
    double v = s_s[tid][0];
    unsigned c = s_nan[tid][0];
#pragma unroll
    for (int w = 1; w < kFlatThreads / 64; ++w) { v += s_s[tid][w]; c += s_nan[tid][w]; }
    part_s[2 * (size_t)blockIdx.x + tid] = v;
    if (c) atomicAdd(nan2 + tid, (unsigned long long)c);
  }
}

}  // namespace mcba

using namespace mcba_internal;

extern "C" {

int mcba_flat_floor_points(size_t n_frames, int n_keypoints, const double* keypoints, int z_points_down, int device, double* points_out, int* index_out, double* kernel_ms) {
  if (n_keypoints < 1 || n_keypoints > MCBA_FLAT_MAX_KEYPOINTS || !keypoints || !points_out)
    return fail(MCBA_ERR_ARG, "mcba_flat_floor_points: 1 .. MCBA_FLAT_MAX_KEYPOINTS keypoints per frame, non-NULL arrays required");
  if (int rc = stateless_device(device)) return rc;
  if (n_frames == 0) return MCBA_OK;
  const int K = n_keypoints;
  int fpb = mcba::kFloorLdsDoubles / (3 * K);
  fpb = fpb > mcba::kFlatThreads ? mcba::kFlatThreads : fpb;
  StatelessCall call;
  double *d_kp = nullptr, *d_out = nullptr;
  int* d_idx = nullptr;
  const size_t nin = n_frames * 3 * (size_t)K;
  if (int rc = call.upload(&d_kp, keypoints, nin)) return rc;
  if (int rc = call.scratch(&d_out, 3 * n_frames)) return rc;
  if (int rc = call.scratch(&d_idx, n_frames)) return rc;
  HIPCHK(call.start());
  const size_t nblk = (n_frames + fpb - 1) / fpb;
  mcba::k_floor_points<<<dim3((unsigned)nblk), dim3(mcba::kFlatThreads), (size_t)fpb * 3 * K * sizeof(double)>>>(d_kp, n_frames, K, fpb, z_points_down ? 1 : 0, d_out, d_idx);
  if (int rc = check_launch()) return rc;
  HIPCHK(call.stop(kernel_ms));
  if (int rc = call.download(points_out, d_out, 3 * n_frames)) return rc;
  return index_out ? call.download(index_out, d_idx, n_frames) : MCBA_OK;
}

int mcba_flat_ransac(size_t n_points, const double* points, int n_hypotheses, const double* planes, double threshold, const double* shift2, int device,
                     unsigned long long* counts_out, double* moments_out, unsigned char* mask_out, double* kernel_ms) {
  if (n_points < 1 || !points || n_hypotheses < 1 || n_hypotheses > MCBA_FLAT_MAX_HYPOTHESES || !planes || !shift2 || !counts_out || !moments_out)
    return fail(MCBA_ERR_ARG, "mcba_flat_ransac: points >= 1, 1 .. MCBA_FLAT_MAX_HYPOTHESES hypotheses, non-NULL arrays required");
  if (mask_out && n_hypotheses != 1) return fail(MCBA_ERR_ARG, "mcba_flat_ransac: the inlier mask needs exactly one hypothesis");
  if (int rc = stateless_device(device)) return rc;
  const int H = n_hypotheses;
  const size_t nblk = (n_points + mcba::kScorePoints - 1) / mcba::kScorePoints;
  StatelessCall call;
  double *d_pts = nullptr, *d_planes = nullptr, *d_pm = nullptr, *d_mom = nullptr;
  unsigned* d_pn = nullptr;
  unsigned long long* d_cnt = nullptr;
  unsigned char* d_mask = nullptr;
  if (int rc = call.upload(&d_pts, points, 3 * n_points)) return rc;
  if (int rc = call.upload(&d_planes, planes, 3 * (size_t)H)) return rc;
  if (int rc = call.scratch(&d_pm, nblk * H * mcba::kMom)) return rc;
  if (int rc = call.scratch(&d_pn, nblk * H)) return rc;
  if (int rc = call.scratch(&d_mom, (size_t)H * mcba::kMom)) return rc;
  if (int rc = call.scratch(&d_cnt, (size_t)H)) return rc;
  if (mask_out)
    if (int rc = call.scratch(&d_mask, n_points)) return rc;
  HIPCHK(call.start());
  mcba::k_ransac_score<<<dim3((unsigned)nblk), dim3(mcba::kFlatThreads)>>>(d_pts, n_points, d_planes, H, threshold, shift2[0], shift2[1], d_pm, d_pn);
  if (int rc = check_launch()) return rc;
  mcba::k_ransac_finish<<<dim3((unsigned)H), dim3(mcba::kFlatThreads)>>>(d_pm, d_pn, (int)nblk, H, d_mom, d_cnt);
  if (int rc = check_launch()) return rc;
  if (mask_out) {
    mcba::k_ransac_mask<<<dim3((unsigned)((n_points + mcba::kFlatThreads - 1) / mcba::kFlatThreads)), dim3(mcba::kFlatThreads)>>>(d_pts, n_points, planes[0], planes[1], planes[2],
                                                                                                                            threshold, d_mask);
    if (int rc = check_launch()) return rc;
  }
  HIPCHK(call.stop(kernel_ms));
  if (int rc = call.download(counts_out, d_cnt, (size_t)H)) return rc;
  if (int rc = call.download(moments_out, d_mom, (size_t)H * mcba::kMom)) return rc;
  return mask_out ? call.download(mask_out, d_mask, n_points) : MCBA_OK;
}

int mcba_flat_order_stats(size_t n_points, const double* points, const double* rt12, int n_ranks, const long long* ranks, int device, double* values_out, double* sums_out,
                          unsigned long long* nans_out, double* kernel_ms) {
  if (n_points < 1 || !points || !rt12 || n_ranks < 0 || n_ranks > mcba::kSelMaxRanks || (n_ranks && (!ranks || !values_out)) || !sums_out || !nans_out)
    return fail(MCBA_ERR_ARG, "mcba_flat_order_stats: points >= 1, 0 .. 8 ranks, non-NULL arrays required");
  for (int i = 0; i < n_ranks; ++i)
    if (ranks[i] < 0 || (unsigned long long)ranks[i] >= n_points) return fail(MCBA_ERR_ARG, "mcba_flat_order_stats: rank out of range");
  if (int rc = stateless_device(device)) return rc;
  const size_t n = n_points;
  const size_t nblk = (n + mcba::kFlatThreads - 1) / mcba::kFlatThreads;
  const std::vector<unsigned long long> rk(ranks, ranks + n_ranks);
  std::vector<mcba::SelState> st(2 * (size_t)n_ranks);   // group 0: x, group 1: y
  StatelessCall call;
  double *d_pts = nullptr, *d_rt = nullptr, *d_xy = nullptr, *d_ps = nullptr;
  unsigned long long* d_nan = nullptr;
  mcba::SelState* d_st = nullptr;
  if (int rc = call.upload(&d_pts, points, 3 * n)) return rc;
  if (int rc = call.upload(&d_rt, rt12, 12)) return rc;
  if (int rc = call.scratch(&d_xy, 2 * n)) return rc;
  if (int rc = call.scratch(&d_ps, 2 * nblk)) return rc;
  if (int rc = call.scratch(&d_nan, 2)) return rc;
  if (int rc = call.scratch(&d_st, st.size())) return rc;
  HIPCHK(hipMemset(d_nan, 0, 2 * sizeof(unsigned long long)));
  HIPCHK(call.start());
  mcba::k_flat_transform<<<dim3((unsigned)nblk), dim3(mcba::kFlatThreads)>>>(d_pts, n, d_rt, d_xy, d_ps, d_nan);
  if (int rc = check_launch()) return rc;
  if (n_ranks > 0) {
    // (the select skips NaNs, so a coordinate that holds one has fewer values than a rank may assume: the caller reports NaN for it)
    mcba::launch_select(nullptr, d_xy, nullptr, n, 2 /* groups: x, y */, 1 /* no frame mask */, d_st, 1 /* either sign */, rk.data(), n_ranks);
    if (int rc = check_launch()) return rc;
  }
  HIPCHK(call.stop(kernel_ms));
  std::vector<double> ps(2 * nblk);
  if (int rc = call.download(ps.data(), d_ps, 2 * nblk)) return rc;
  if (int rc = call.download(nans_out, d_nan, 2)) return rc;
  if (n_ranks > 0)
    if (int rc = call.download(st.data(), d_st, st.size())) return rc;
  for (size_t q = 0; q < st.size(); ++q) values_out[q] = mcba::sel_value(st[q]);
  for (int c = 0; c < 2; ++c) {  // the per-block sums, in block order
    double s = 0.0;
    for (size_t b = 0; b < nblk; ++b) s += ps[2 * b + c];
    sums_out[c] = s;
  }
  return MCBA_OK;
}

}  // extern "C"
