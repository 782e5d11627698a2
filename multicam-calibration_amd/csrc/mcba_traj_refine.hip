// mcba_traj_refine.hip -- trajectory refinement: keypoint tracks smoothed on the detections themselves, Gauss-Newton on
// the robust reprojection cost plus the second-difference prior.  Per-lane arithmetic: mcba_traj_refine_math.h (host-checked); the linear solve of
// every iteration is the smoother's elimination (mcba_smooth.hip) with level 0 in its right-hand-side mode.  No kernel here uses an atomic:
// every word has one writer, every sum a fixed order.  The camera table is staged in LDS as k_tri_refine stages it.
//   k_traj_count      workgroup = track: its usable and single frames, the non-finite coordinates of its start
//   k_traj_linearise  lane = (frame, track), tracks fastest: H_t and the gradient of the whole objective at x
//   k_traj_trial      workgroup = 256 frames of a running track: the objective at x + alpha d for alpha = 0, 1, 1/2, 1/4, 1/8 with the detections
//                     read once, the data and penalty parts at x, max |d|, max |x|; k_traj_final adds the workgroups' sums
//   k_traj_apply      lane = (frame, track): x <- x + alpha_k d
#include <hip/hip_runtime.h>

#include "mcba_device.h"
#include "mcba_kernels.h"
#include "mcba_traj_refine_math.h"

namespace mcba {

__global__ __launch_bounds__(256) void k_traj_count(TrData rd, int C, int K, int* __restrict__ n_usable, int* __restrict__ n_single, int* __restrict__ n_bad) {
  __shared__ double s_r[3][256];
  const int k = blockIdx.x;
  double r[3] = {0.0, 0.0, 0.0};
  for (size_t t = threadIdx.x; t < rd.T; t += 256) traj_count_frame(rd, C, K, k, t, r);   // (counts: exact in any order)
  const bool is_max[3] = {false, false, false};
  block_tree<3>(s_r, r, is_max);
  if (threadIdx.x == 0) { n_usable[k] = (int)s_r[0][0]; n_single[k] = (int)s_r[1][0]; n_bad[k] = (int)s_r[2][0]; }
}

// run[k] == 0: the track is not (or no longer) running and its lanes leave after the staging barrier
template <int LOSS>
__global__ __launch_bounds__(256) void k_traj_linearise(TrData rd, const KpCam* __restrict__ cams, int C, int K, const int* __restrict__ run) {
  __shared__ KpCam s_cam[kKpMaxCams];
  stage_cams(s_cam, cams, C);
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= rd.T * (size_t)K) return;
  const int k = (int)(i % K);
  if (!run[k]) return;
  traj_linearise_lane<LOSS>(s_cam, C, rd, K, k, i / K);
}

template <int LOSS>
__global__ __launch_bounds__(256) void k_traj_trial(TrData rd, const KpCam* __restrict__ cams, int C, int K, const int* __restrict__ list, int nblk, double* __restrict__ part) {
  __shared__ KpCam s_cam[kKpMaxCams];
  __shared__ double s_r[TR_SUMS][256];
  stage_cams(s_cam, cams, C);
  const int kk = blockIdx.x / nblk, b = blockIdx.x % nblk;
  const size_t t = (size_t)b * 256 + threadIdx.x;
  double r[TR_SUMS];
#pragma unroll
  for (int e = 0; e < TR_SUMS; ++e) r[e] = 0.0;
  if (t < rd.T) traj_trial_lane<LOSS>(s_cam, C, rd, K, list[kk], t, r);
  bool is_max[TR_SUMS];
#pragma unroll
  for (int e = 0; e < TR_SUMS; ++e) is_max[e] = e >= TR_DMAX;
  block_tree<TR_SUMS>(s_r, r, is_max);
  if (threadIdx.x < TR_SUMS) part[TR_SUMS * (size_t)blockIdx.x + threadIdx.x] = s_r[threadIdx.x][0];
}

// res[TR_SUMS kk ..] of the kk-th running track: the sums of its workgroups in a fixed order, the penalty part as a cost (0.5 / a^2 times the sum)
__global__ __launch_bounds__(256) void k_traj_final(const double* __restrict__ ia2, const int* __restrict__ list, int nblk, const double* __restrict__ part, double* __restrict__ res) {
  __shared__ double s_r[TR_SUMS][256];
  const int kk = blockIdx.x;
  double r[TR_SUMS];
#pragma unroll
  for (int e = 0; e < TR_SUMS; ++e) r[e] = 0.0;
  for (int b = threadIdx.x; b < nblk; b += 256) {
    const double* p = part + TR_SUMS * ((size_t)kk * nblk + b);
#pragma unroll
    for (int e = 0; e < TR_SUMS; ++e) r[e] = e >= TR_DMAX ? fmax(r[e], p[e]) : r[e] + p[e];
  }
  bool is_max[TR_SUMS];
#pragma unroll
  for (int e = 0; e < TR_SUMS; ++e) is_max[e] = e >= TR_DMAX;
  block_tree<TR_SUMS>(s_r, r, is_max);
  if (threadIdx.x < TR_SUMS) res[TR_SUMS * (size_t)kk + threadIdx.x] = threadIdx.x == TR_PEN ? 0.5 * ia2[list[kk]] * s_r[TR_PEN][0] : s_r[threadIdx.x][0];
}

__global__ __launch_bounds__(256) void k_traj_apply(TrData rd, int K, const double* __restrict__ alpha) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= rd.T * (size_t)K) return;
  traj_apply_lane(rd, i, alpha[i % K]);
}

// the three losses of the refinement (convex: the trial's backtracking assumes a descent direction of the Gauss-Newton model)
using TrajLossList = IntList<LOSS_LINEAR, LOSS_SOFT_L1, LOSS_HUBER>;

static bool traj_flat_grid(const TrData& rd, int K, unsigned& blocks) {
  const size_t b = (rd.T * (size_t)K + 255) / 256;
  blocks = (unsigned)b;
  return b >= 1 && b <= 0x7fffffffu;
}

int launch_traj_count(hipStream_t st, const TrData& rd, int C, int K, int* n_usable, int* n_single, int* n_bad) {
  if (C < 1 || C > kKpMaxCams || K < 1) return 1;
  k_traj_count<<<dim3((unsigned)K), dim3(256), 0, st>>>(rd, C, K, n_usable, n_single, n_bad);
  return 0;
}

int launch_traj_linearise(hipStream_t st, int loss, const TrData& rd, const KpCam* cams, int C, int K, const int* run) {
  unsigned blocks;
  if (C < 1 || C > kKpMaxCams || !traj_flat_grid(rd, K, blocks)) return 1;
  return with_int(TrajLossList{}, loss, [&](auto L) {
    k_traj_linearise<decltype(L)::value><<<dim3(blocks), dim3(256), 0, st>>>(rd, cams, C, K, run);
    return 0;
  });
}

// the sums of the nact running tracks of `list`: part (nact, blocks, TR_SUMS) scratch, res (nact, TR_SUMS)
int launch_traj_trial(hipStream_t st, int loss, const TrData& rd, const KpCam* cams, int C, int K, const int* list, int nact, double* part, double* res) {
  const int nblk = smooth_eval_blocks(rd.T);
  if (C < 1 || C > kKpMaxCams || nact < 1 || nact > K || (size_t)nblk * nact > 0x7fffffffu) return 1;
  if (with_int(TrajLossList{}, loss, [&](auto L) {
        k_traj_trial<decltype(L)::value><<<dim3((unsigned)(nblk * nact)), dim3(256), 0, st>>>(rd, cams, C, K, list, nblk, part);
        return 0;
      }))
    return 1;
  k_traj_final<<<dim3((unsigned)nact), dim3(256), 0, st>>>(rd.ia2, list, nblk, part, res);
  return 0;
}

int launch_traj_apply(hipStream_t st, const TrData& rd, int K, const double* alpha) {
  unsigned blocks;
  if (!traj_flat_grid(rd, K, blocks)) return 1;
  k_traj_apply<<<dim3(blocks), dim3(256), 0, st>>>(rd, K, alpha);
  return 0;
}

}  // namespace mcba
