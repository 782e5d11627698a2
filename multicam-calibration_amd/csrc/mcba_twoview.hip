// mcba_twoview.hip -- two-view RANSAC (the reference has no counterpart): the relative pose of two cameras of known
// intrinsics from M keypoint correspondences and H host-drawn 8-point samples.  The per-lane arithmetic is in mcba_twoview_math.h, where the
// host harness checks the same text.
//   k_tv_prepare      lane = point: both detections undistorted; undistorted pixels and normalised coordinates in 8 planes (SoA)
//   k_tv_hypotheses   lane = hypothesis: tv_essential on the 8 sampled correspondences, tv_fundamental.  The two 9 x 9 work matrices of the
//                     eigenvector iteration (162 doubles) are in scratch: H is a few thousand at most, this is not the hot kernel
//   k_hyp_score       the hot one (mcba_hyp_score.h) with TvScore: F against the undistorted pixels of both views, the truncated Sampson cost
//   k_hyp_finish      the partials summed per hypothesis; defined here for this pipeline and the resection's (launch_hyp_finish)
//   k_tv_winner       one workgroup: the lowest (cost, index), hyp_argmin; its four (R, t)
//   k_tv_pose_count   lane = point: the winner's inlier mask; tv_depths under each candidate; in-front counts per workgroup
//   k_tv_pose_pick    one workgroup: the counts summed as in k_hyp_finish; highest (count, -index); rt12
//   k_tv_pose_points  lane = point: the two-view point under the chosen candidate, NaN for a non-inlier
// No atomics, floating-point or other: every sum has a fixed order, the results depend on (M, H) alone, bit for bit.
#include <hip/hip_runtime.h>
#include <math.h>
// No contraction beyond the fma() calls the text spells out: k_hyp_score<TvScore> and k_tv_pose_count must judge a correspondence alike to the last bit.
#pragma clang fp contract(off)
#include "mcba_hyp_score.h"
#include "../../include/mcba.h"

static_assert(mcba::kHypPoints == MCBA_TWOVIEW_POINTS_PER_BLOCK && mcba::kHypChunk == MCBA_TWOVIEW_CHUNK, "include/mcba.h names the launch shape of k_hyp_score");

namespace mcba {

__global__ __launch_bounds__(kHypThreads) void k_tv_prepare(const double* __restrict__ uv_a, const double* __restrict__ uv_b, size_t M, TvCams cams, int und_iters, double* __restrict__ prep) {
  const size_t p = (size_t)blockIdx.x * kHypThreads + threadIdx.x;
  if (p >= M) return;
  double o[8];
  tv_prepare(uv_a[2 * p], uv_a[2 * p + 1], uv_b[2 * p], uv_b[2 * p + 1], cams.ka, cams.da, cams.kb, cams.db, und_iters, o);
#pragma unroll
  for (int k = 0; k < 8; ++k) prep[(size_t)k * M + p] = o[k];
}

__global__ __launch_bounds__(64) void k_tv_hypotheses(const double* __restrict__ prep, size_t M, const int* __restrict__ samples, int H, const double* __restrict__ e_in, TvCams cams,
                                                      double* __restrict__ E, double* __restrict__ F, int* __restrict__ status) {
  const int h = blockIdx.x * 64 + threadIdx.x;
  if (h >= H) return;
  double e[9], f[9];
  int st;
  if (e_in) {
    bool ok = true;
#pragma unroll
    for (int i = 0; i < 9; ++i) { e[i] = e_in[9 * (size_t)h + i]; ok = ok && fabs(e[i]) <= 1.7976931348623157e308; }
    st = ok ? TV_OK : TV_VOID;
  } else {
    double xa[16], xb[16], S[81];
    for (int k = 0; k < 8; ++k) {
      const size_t s = (size_t)samples[8 * (size_t)h + k];   // (0 .. M - 1: checked on the host before the upload)
      xa[2 * k] = prep[4 * M + s]; xa[2 * k + 1] = prep[5 * M + s];
      xb[2 * k] = prep[6 * M + s]; xb[2 * k + 1] = prep[7 * M + s];
    }
    st = tv_essential(xa, xb, S, e);
  }
  tv_fundamental(e, cams.ka, cams.kb, f);
#pragma unroll
  for (int i = 0; i < 9; ++i) { E[9 * (size_t)h + i] = e[i]; F[9 * (size_t)h + i] = f[i]; }
  status[h] = st;
}

// k_hyp_score's two-view model: a hypothesis is F (9 doubles), a point the undistorted pixels of both views (planes 0 .. 3 of prep), one camera
struct TvScore {
  static constexpr int kDoubles = 9;
  static constexpr bool kCameras = false;
  struct Point { double xa, ya, xb, yb; bool ok; };
  const double* __restrict__ prep;
  size_t M;
  __device__ __forceinline__ Point load(int, size_t p) const {
    const bool ok = p < M;
    return {ok ? prep[p] : 0.0, ok ? prep[M + p] : 0.0, ok ? prep[2 * M + p] : 0.0, ok ? prep[3 * M + p] : 0.0, ok};
  }
  static __device__ __forceinline__ double error2(const double* f, const Point& q) { return tv_sampson2(f, q.xa, q.ya, q.xb, q.yb); }
};

// grid (H, C): lane t sums the partials of workgroups t, t + 256, ... in order, then a fixed LDS tree.  part_c, part_n: (C, nblk, H)
__global__ __launch_bounds__(kHypThreads) void k_hyp_finish(const double* __restrict__ part_c, const unsigned* __restrict__ part_n, size_t nblk, int H, const int* __restrict__ status,
                                                            double* __restrict__ cost, unsigned* __restrict__ count) {
  __shared__ double s_c[kHypThreads];
  __shared__ unsigned long long s_n[kHypThreads];
  const int h = blockIdx.x, c = blockIdx.y, tid = threadIdx.x;
  double cs = 0.0;
  unsigned long long n = 0;
  for (size_t bk = tid; bk < nblk; bk += kHypThreads) {
    cs += part_c[((size_t)c * nblk + bk) * H + h];
    n += part_n[((size_t)c * nblk + bk) * H + h];
  }
  s_c[tid] = cs;
  s_n[tid] = n;
  __syncthreads();
  for (int s = kHypThreads / 2; s >= 1; s >>= 1) {
    if (tid < s) { s_c[tid] += s_c[tid + s]; s_n[tid] += s_n[tid + s]; }
    __syncthreads();
  }
  if (tid == 0) {
    const bool ok = status[(size_t)c * H + h] == TV_OK;
    cost[(size_t)c * H + h] = ok ? s_c[0] : __builtin_inf();
    count[(size_t)c * H + h] = ok ? (unsigned)s_n[0] : 0u;
  }
}

// one workgroup: the winner (hyp_argmin) and its four (R, t)
__global__ __launch_bounds__(kHypThreads) void k_tv_winner(const double* __restrict__ cost, const unsigned* __restrict__ count, int H, const double* __restrict__ E, int* __restrict__ win_idx,
                                                           double* __restrict__ best4, double* __restrict__ cand) {
  double bc;
  const int w = hyp_argmin(cost, H, bc);
  if (threadIdx.x == 0) {
    win_idx[0] = w;
    best4[0] = (double)w; best4[1] = bc; best4[2] = (double)count[w];
    double Rt[48];
    tv_candidates(E + 9 * (size_t)w, Rt);
    for (int i = 0; i < 48; ++i) cand[i] = Rt[i];
  }
}

__device__ __forceinline__ bool tv_winner_inlier(const double* __restrict__ prep, size_t M, size_t p, const double* f, bool valid, double t2) {
  return valid && tv_inlier(tv_sampson2(f, prep[p], prep[M + p], prep[2 * M + p], prep[3 * M + p]), t2);
}

// part_f: blocks x 4
__global__ __launch_bounds__(kHypThreads) void k_tv_pose_count(const double* __restrict__ prep, size_t M, const double* __restrict__ F, const int* __restrict__ status, double t2,
                                                              const int* __restrict__ win_idx, const double* __restrict__ cand, unsigned char* __restrict__ inliers, unsigned* __restrict__ part_f) {
  __shared__ double s_f[9];
  __shared__ double s_rt[48];
  __shared__ unsigned s_n[kHypThreads / 64][4];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int w = win_idx[0];
  if (tid < 9) s_f[tid] = F[9 * (size_t)w + tid];
  if (tid >= 64 && tid < 64 + 48) s_rt[tid - 64] = cand[tid - 64];
  __syncthreads();
  const size_t p = (size_t)blockIdx.x * kHypThreads + tid;
  const bool here = p < M;
  const size_t q = here ? p : 0;
  double f[9];
#pragma unroll
  for (int i = 0; i < 9; ++i) f[i] = s_f[i];
  const bool in = tv_winner_inlier(prep, M, q, f, here && status[w] == TV_OK, t2);
  if (here) inliers[p] = in ? 1 : 0;
  const double xa = prep[4 * M + q], ya = prep[5 * M + q], xb = prep[6 * M + q], yb = prep[7 * M + q];
  for (int c = 0; c < 4; ++c) {
    double X[3];
    bool kept;
    const bool front = tv_depths(s_rt + 12 * c, xa, ya, xb, yb, X, kept);
    const unsigned n = wave_sum(in && front ? 1u : 0u);
    if (lane == 0) s_n[wave][c] = n;
  }
  __syncthreads();
  if (tid < 4) {
    unsigned n = s_n[0][tid];
#pragma unroll
    for (int k = 1; k < kHypThreads / 64; ++k) n += s_n[k][tid];
    part_f[4 * (size_t)blockIdx.x + tid] = n;
  }
}

// one workgroup: the four counts summed (strided lanes in order, a fixed tree); highest (count, -index)
__global__ __launch_bounds__(kHypThreads) void k_tv_pose_pick(const unsigned* __restrict__ part_f, size_t nblk, const double* __restrict__ cand, int* __restrict__ win_idx, double* __restrict__ best4,
                                                             double* __restrict__ rt12) {
  __shared__ unsigned long long s_n[4][kHypThreads];
  const int tid = threadIdx.x;
  unsigned long long n[4] = {0, 0, 0, 0};
  for (size_t bk = tid; bk < nblk; bk += kHypThreads) {
#pragma unroll
    for (int c = 0; c < 4; ++c) n[c] += part_f[4 * bk + c];
  }
#pragma unroll
  for (int c = 0; c < 4; ++c) s_n[c][tid] = n[c];
  __syncthreads();
  for (int s = kHypThreads / 2; s >= 1; s >>= 1) {
    if (tid < s) {
#pragma unroll
      for (int c = 0; c < 4; ++c) s_n[c][tid] += s_n[c][tid + s];
    }
    __syncthreads();
  }
  if (tid == 0) {
    int bc = 0;
    for (int c = 1; c < 4; ++c) bc = s_n[c][0] > s_n[bc][0] ? c : bc;
    win_idx[1] = bc;
    best4[3] = (double)s_n[bc][0];
    for (int i = 0; i < 12; ++i) rt12[i] = cand[12 * bc + i];
  }
}

__global__ __launch_bounds__(kHypThreads) void k_tv_pose_points(const double* __restrict__ prep, size_t M, const int* __restrict__ win_idx, const double* __restrict__ cand,
                                                               const unsigned char* __restrict__ inliers, double* __restrict__ points) {
  const size_t p = (size_t)blockIdx.x * kHypThreads + threadIdx.x;
  if (p >= M) return;
  const double* rt = cand + 12 * win_idx[1];
  double Rt[12];
#pragma unroll
  for (int i = 0; i < 12; ++i) Rt[i] = rt[i];
  double X[3];
  bool kept;
  tv_depths(Rt, prep[4 * M + p], prep[5 * M + p], prep[6 * M + p], prep[7 * M + p], X, kept);
  const bool give = inliers[p] && kept;
  const double nan = __builtin_nan("");
  points[3 * p] = give ? X[0] : nan; points[3 * p + 1] = give ? X[1] : nan; points[3 * p + 2] = give ? X[2] : nan;
}

// ---------------------------------------------------------------- launch wrappers
void launch_tv_prepare(hipStream_t st, const double* uv_a, const double* uv_b, size_t M, const TvCams& cams, int und_iters, double* prep) {
  k_tv_prepare<<<dim3((unsigned)hyp_point_blocks(M)), dim3(kHypThreads), 0, st>>>(uv_a, uv_b, M, cams, und_iters, prep);
}

void launch_tv_hypotheses(hipStream_t st, const double* prep, size_t M, const int* samples, int H, const double* e_in, const TvCams& cams, double* E, double* F, int* status) {
  k_tv_hypotheses<<<dim3((unsigned)((H + 63) / 64)), dim3(64), 0, st>>>(prep, M, samples, H, e_in, cams, E, F, status);
}

void launch_tv_score(hipStream_t st, const double* prep, size_t M, const double* F, int H, double threshold, double* part_c, unsigned* part_n) {
  launch_hyp_score(st, TvScore{prep, M}, M, 1, F, H, threshold, part_c, part_n);
}

void launch_hyp_finish(hipStream_t st, const double* part_c, const unsigned* part_n, size_t nblk, int C, int H, const int* status, double* cost, unsigned* count) {
  k_hyp_finish<<<dim3((unsigned)H, (unsigned)C), dim3(kHypThreads), 0, st>>>(part_c, part_n, nblk, H, status, cost, count);
}

void launch_tv_finish(hipStream_t st, const double* part_c, const unsigned* part_n, size_t nblk, int H, const double* E, const int* status, double* cost, unsigned* count, int* win_idx, double* best4,
                      double* cand) {
  launch_hyp_finish(st, part_c, part_n, nblk, 1, H, status, cost, count);
  k_tv_winner<<<dim3(1), dim3(kHypThreads), 0, st>>>(cost, count, H, E, win_idx, best4, cand);
}

void launch_tv_pose(hipStream_t st, const double* prep, size_t M, const double* F, const int* status, double threshold, const double* cand, unsigned* part_f, int* win_idx, double* best4, double* rt12,
                    unsigned char* inliers, double* points) {
  const size_t nblk = hyp_point_blocks(M);
  k_tv_pose_count<<<dim3((unsigned)nblk), dim3(kHypThreads), 0, st>>>(prep, M, F, status, threshold * threshold, win_idx, cand, inliers, part_f);
  k_tv_pose_pick<<<dim3(1), dim3(kHypThreads), 0, st>>>(part_f, nblk, cand, win_idx, best4, rt12);
  k_tv_pose_points<<<dim3((unsigned)nblk), dim3(kHypThreads), 0, st>>>(prep, M, win_idx, cand, inliers, points);
}

}  // namespace mcba
