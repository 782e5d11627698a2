// mcba_hyp_score.h -- the scoring core that the two RANSAC pipelines share (device only; SURVEY.md sections 8f-14, 8f-16): a table of hypotheses
// judged against every point, the truncated cost and the inlier count of each, the cheapest one.  mcba_twoview.hip and mcba_resect.hip
// instantiate the scorer with their model; the finish kernel is defined once, in mcba_twoview.hip (launch_hyp_finish of mcba_kernels.h).
//   k_hyp_score<Model>  the hot one, k_ransac_score's shape: a workgroup keeps kHypPoints points of one camera in registers (kHypPPT per lane) and
//                       loops over a chunk of kHypChunk hypotheses that sit in LDS; grid = (hyp_score_blocks, chunks, cameras); per hypothesis
//                       the inlier count and the truncated cost, lane -> wavefront (shuffles) -> workgroup (waves in index order) -> one
//                       partial per (camera, workgroup, hypothesis)
//   k_hyp_finish        workgroup = (hypothesis, camera): lane t sums the partials of workgroups t, t + 256, ... in order, then a fixed LDS tree
//   hyp_argmin          one workgroup: the lowest (cost, index) of a camera's row of costs, handed to every lane
// A model says what a hypothesis and a point are:
//   kDoubles            doubles per hypothesis (row-major in the table, (C, H, kDoubles))
//   kCameras            false: one camera, the grid has no z; true: the camera is blockIdx.z
//   Point load(c, p)    the values of point p of camera c and its ok flag; a point that is not ok (past the end, not usable) holds zeros and
//                       adds nothing.  It returns the values: an array filled through a pointer costs the two-view instance 25 VGPRs
//   error2(hyp, point)  the squared error that tv_cost_term and tv_inlier judge, inline: the kernels that re-judge the winner's points call the
//                       same function and agree to the last bit (no contraction in either translation unit)
// The launch shape (kHypThreads, kHypPPT, kHypPoints, kHypChunk, hyp_score_blocks, hyp_point_blocks) is declared in mcba_kernels.h, which the
// host bodies see too: they size the partials by it.  No atomics, floating-point or other: every sum has a fixed order.
#pragma once
#include "mcba_kernels.h"
#include "mcba_device.h"
#include "mcba_twoview_math.h"

namespace mcba {

// part_c, part_n: (C, gridDim.x, H)
template <class Model>
__global__ __launch_bounds__(kHypThreads) void k_hyp_score(Model m, const double* __restrict__ table, int H, double t2, double* __restrict__ part_c, unsigned* __restrict__ part_n) {
  constexpr int D = Model::kDoubles;
  __shared__ double s_hyp[kHypChunk * D];
  __shared__ double s_c[kHypThreads / 64][kHypChunk];
  __shared__ unsigned s_n[kHypThreads / 64][kHypChunk];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int c = Model::kCameras ? blockIdx.z : 0;
  const int h0 = blockIdx.y * kHypChunk, nh = H - h0 < kHypChunk ? H - h0 : kHypChunk;
  for (int i = tid; i < D * nh; i += kHypThreads) s_hyp[i] = table[D * ((size_t)c * H + h0) + i];
  typename Model::Point pt[kHypPPT];
  const size_t p0 = (size_t)blockIdx.x * kHypPoints;
#pragma unroll
  for (int j = 0; j < kHypPPT; ++j) pt[j] = m.load(c, p0 + (size_t)j * kHypThreads + tid);
  __syncthreads();
  for (int h = 0; h < nh; ++h) {
    double hyp[D];
#pragma unroll
    for (int i = 0; i < D; ++i) hyp[i] = s_hyp[D * h + i];
    double cs = 0.0;
    unsigned n = 0;
#pragma unroll
    for (int j = 0; j < kHypPPT; ++j) {
      const double e2 = Model::error2(hyp, pt[j]);
      cs += pt[j].ok ? tv_cost_term(e2, t2) : 0.0;
      n += pt[j].ok && tv_inlier(e2, t2) ? 1u : 0u;
    }
    cs = wave_sum(cs);
    n = wave_sum(n);
    if (lane == 0) { s_c[wave][h] = cs; s_n[wave][h] = n; }
  }
  __syncthreads();
  const size_t row = ((size_t)c * gridDim.x + blockIdx.x) * H + h0;
  for (int h = tid; h < nh; h += kHypThreads) {
    double cs = s_c[0][h];
    unsigned n = s_n[0][h];
#pragma unroll
    for (int w = 1; w < kHypThreads / 64; ++w) { cs += s_c[w][h]; n += s_n[w][h]; }
    part_c[row + h] = cs;
    part_n[row + h] = n;
  }
}

template <class Model>
void launch_hyp_score(hipStream_t st, const Model& m, size_t n_points, int C, const double* table, int H, double threshold, double* part_c, unsigned* part_n) {
  k_hyp_score<Model><<<dim3((unsigned)hyp_score_blocks(n_points), (unsigned)((H + kHypChunk - 1) / kHypChunk), (unsigned)C), dim3(kHypThreads), 0, st>>>(m, table, H, threshold * threshold, part_c,
                                                                                                                                                      part_n);
}

// The lowest (cost, index) of cost[0 .. H - 1], H >= 1 -- a total order, so the tree's shape does not matter -- to every lane of the one
// workgroup that calls it.  Hypothesis 0 beats the initial (inf, INT_MAX) even when it is void
__device__ __forceinline__ int hyp_argmin(const double* __restrict__ cost, int H, double& best_cost) {
  __shared__ double s_c[kHypThreads];
  __shared__ int s_h[kHypThreads];
  const int tid = threadIdx.x;
  double bc = __builtin_inf();
  int bh = 0x7fffffff;
  for (int h = tid; h < H; h += kHypThreads) {
    const double cs = cost[h];
    const bool take = tv_before(cs, h, bc, bh);
    bc = take ? cs : bc;
    bh = take ? h : bh;
  }
  s_c[tid] = bc;
  s_h[tid] = bh;
  __syncthreads();
  for (int s = kHypThreads / 2; s >= 1; s >>= 1) {
    if (tid < s && tv_before(s_c[tid + s], s_h[tid + s], s_c[tid], s_h[tid])) { s_c[tid] = s_c[tid + s]; s_h[tid] = s_h[tid + s]; }
    __syncthreads();
  }
  best_cost = s_c[0];
  return s_h[0];
}

}  // namespace mcba
