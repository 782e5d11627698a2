// mcba_skeltraj.hip -- skeleton trajectories: keypoint tracks refined on the detections under the second-difference prior
// and joined inside every frame by bones of known length, Gauss-Newton whose linear system is solved by conjugate gradients preconditioned with
// the tracks' own block-pentadiagonal matrices (the smoother's elimination once per outer iteration, its re-solve once per CG iteration).
// Per-lane arithmetic: mcba_skeltraj_math.h (host-checked).  All FP64; no kernel here uses an atomic: every word has one writer, every sum a
// fixed order (a tree inside the workgroup, then one workgroup over the partials).  Every launch is flat: lane = (frame, keypoint), keypoints
// fastest; a lane whose track does not run adds nothing.  The kernels of a solve read its done word first and return at once when it is set.
//   k_skt_linearise   after k_traj_linearise: the bones' gradient into G, q = G, the directions and residuals of the bones
//   k_skt_start       p = z, d = 0, partials of r^T z            k_skt_operator   y = A p, partials of p^T y
//   k_skt_step        d += alpha p, q += alpha y                 k_skt_dot        partials of r^T z
//   k_skt_direction   p = z + beta p                             k_skt_scalars    one workgroup: a sum of partials, then alpha, beta, the done word
//   k_skt_trial       the whole objective at x + alpha d for alpha = 0, 1, 1/2, 1/4, 1/8, max |d|, max |x|; k_skt_trial_final adds the partials
#include <hip/hip_runtime.h>

#include "mcba_device.h"
#include "mcba_kernels.h"
#include "mcba_skeltraj_math.h"

namespace mcba {

// the lane's (frame, keypoint) index, or false: past the end or a track that does not run
__device__ __forceinline__ bool skt_lane(const SktData& sd, int K, size_t& idx, int& k) {
  idx = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= sd.rd.T * (size_t)K) return false;
  k = (int)(idx % K);
  return sd.run[k] != 0;
}
// the workgroup's sum of one double per lane into part[blockIdx.x]
__device__ __forceinline__ void skt_block_sum(double v, double* __restrict__ part) {
  __shared__ double s_r[1][256];
  const double r[1] = {v};
  const bool is_max[1] = {false};
  block_tree<1>(s_r, r, is_max);
  if (threadIdx.x == 0) part[blockIdx.x] = s_r[0][0];
}

__global__ __launch_bounds__(256) void k_skt_linearise(SktData sd, int K) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= sd.rd.T * (size_t)K) return;
  skt_linearise_lane(sd, K, (int)(i % K), i / K);
}

__global__ __launch_bounds__(256) void k_skt_start(SktData sd, int K, double* __restrict__ part) {
  size_t idx;
  int k;
  skt_block_sum(skt_lane(sd, K, idx, k) ? skt_start_lane(sd, idx) : 0.0, part);
}

__global__ __launch_bounds__(256) void k_skt_operator(SktData sd, int K, const int* __restrict__ w, double* __restrict__ part) {
  if (w[CG_DONE]) return;
  size_t idx;
  int k;
  skt_block_sum(skt_lane(sd, K, idx, k) ? skt_operator_lane(sd, K, k, idx / K) : 0.0, part);
}

__global__ __launch_bounds__(256) void k_skt_step(SktData sd, int K, const double* __restrict__ sc, const int* __restrict__ w) {
  if (w[CG_DONE]) return;
  size_t idx;
  int k;
  if (skt_lane(sd, K, idx, k)) skt_step_lane(sd, idx, sc[CG_ALPHA]);
}

__global__ __launch_bounds__(256) void k_skt_dot(SktData sd, int K, const int* __restrict__ w, double* __restrict__ part) {
  if (w[CG_DONE]) return;
  size_t idx;
  int k;
  skt_block_sum(skt_lane(sd, K, idx, k) ? skt_dot_lane(sd, idx) : 0.0, part);
}

__global__ __launch_bounds__(256) void k_skt_direction(SktData sd, int K, const double* __restrict__ sc, const int* __restrict__ w) {
  if (w[CG_DONE]) return;
  size_t idx;
  int k;
  if (skt_lane(sd, K, idx, k)) skt_direction_lane(sd, idx, sc[CG_BETA]);
}

__global__ __launch_bounds__(256) void k_skt_scalars(int where, unsigned nblk, const double* __restrict__ part, double tol2, int cg_max, double* __restrict__ sc, int* __restrict__ w) {
  if (where != CG_START && w[CG_DONE]) return;
  __shared__ double s_r[1][256];
  double r[1] = {0.0};
  for (unsigned b = threadIdx.x; b < nblk; b += 256) r[0] += part[b];
  const bool is_max[1] = {false};
  block_tree<1>(s_r, r, is_max);
  if (threadIdx.x == 0) skt_scalars(where, s_r[0][0], tol2, cg_max, sc, w);
}

template <int LOSS>
__global__ __launch_bounds__(256) void k_skt_trial(SktData sd, const KpCam* __restrict__ cams, int C, int K, double* __restrict__ part) {
  __shared__ KpCam s_cam[kKpMaxCams];
  __shared__ double s_r[SKT_SUMS][256];
  stage_cams(s_cam, cams, C);
  double r[SKT_SUMS];
#pragma unroll
  for (int e = 0; e < SKT_SUMS; ++e) r[e] = 0.0;
  size_t idx;
  int k;
  if (skt_lane(sd, K, idx, k)) skt_trial_lane<LOSS>(s_cam, C, sd, K, k, idx / K, r);
  bool is_max[SKT_SUMS];
#pragma unroll
  for (int e = 0; e < SKT_SUMS; ++e) is_max[e] = e == TR_DMAX || e == TR_XMAX;
  block_tree<SKT_SUMS>(s_r, r, is_max);
  if (threadIdx.x < SKT_SUMS) part[SKT_SUMS * (size_t)blockIdx.x + threadIdx.x] = s_r[threadIdx.x][0];
}

__global__ __launch_bounds__(256) void k_skt_trial_final(unsigned nblk, const double* __restrict__ part, double* __restrict__ res) {
  __shared__ double s_r[SKT_SUMS][256];
  double r[SKT_SUMS];
#pragma unroll
  for (int e = 0; e < SKT_SUMS; ++e) r[e] = 0.0;
  for (unsigned b = threadIdx.x; b < nblk; b += 256) {
    const double* p = part + SKT_SUMS * (size_t)b;
#pragma unroll
    for (int e = 0; e < SKT_SUMS; ++e) r[e] = e == TR_DMAX || e == TR_XMAX ? fmax(r[e], p[e]) : r[e] + p[e];
  }
  bool is_max[SKT_SUMS];
#pragma unroll
  for (int e = 0; e < SKT_SUMS; ++e) is_max[e] = e == TR_DMAX || e == TR_XMAX;
  block_tree<SKT_SUMS>(s_r, r, is_max);
  if (threadIdx.x < SKT_SUMS) res[threadIdx.x] = s_r[threadIdx.x][0];
}

using SktLossList = IntList<LOSS_LINEAR, LOSS_SOFT_L1, LOSS_HUBER>;

static bool skt_grid(const SktData& sd, int K, unsigned& blocks) {
  const size_t b = K >= 1 && K <= SK_MAX_K ? (sd.rd.T * (size_t)K + 255) / 256 : 0;
  blocks = (unsigned)b;
  return b >= 1 && b <= 0x7fffffffu;
}

int launch_skt_linearise(hipStream_t st, const SktData& sd, int K) {
  unsigned blocks;
  if (!skt_grid(sd, K, blocks)) return 1;
  k_skt_linearise<<<dim3(blocks), dim3(256), 0, st>>>(sd, K);
  return 0;
}

int launch_skt_cg_start(hipStream_t st, const SktData& sd, int K, double* part, double* sc, int* w) {
  unsigned blocks;
  if (!skt_grid(sd, K, blocks)) return 1;
  k_skt_start<<<dim3(blocks), dim3(256), 0, st>>>(sd, K, part);
  k_skt_scalars<<<dim3(1), dim3(256), 0, st>>>(CG_START, blocks, part, 0.0, 0, sc, w);
  return 0;
}

int launch_skt_cg_iteration(hipStream_t st, const SktData& sd, int K, const SmLevel* lv, int levels, const SmData& td, const int* list, int nact, double tol2, int cg_max, double* part,
                            double* sc, int* w) {
  unsigned blocks;
  if (!skt_grid(sd, K, blocks)) return 1;
  k_skt_operator<<<dim3(blocks), dim3(256), 0, st>>>(sd, K, w, part);
  k_skt_scalars<<<dim3(1), dim3(256), 0, st>>>(CG_AFTER_OPERATOR, blocks, part, tol2, cg_max, sc, w);
  k_skt_step<<<dim3(blocks), dim3(256), 0, st>>>(sd, K, sc, w);
  if (launch_smooth_resolve(st, lv, levels, td, K, list, nact, w + CG_DONE)) return 1;
  if (launch_smooth_backsub(st, lv, levels, td, K, list, nact, true)) return 1;
  k_skt_dot<<<dim3(blocks), dim3(256), 0, st>>>(sd, K, w, part);
  k_skt_scalars<<<dim3(1), dim3(256), 0, st>>>(CG_AFTER_DOT, blocks, part, tol2, cg_max, sc, w);
  k_skt_direction<<<dim3(blocks), dim3(256), 0, st>>>(sd, K, sc, w);
  return 0;
}

int launch_skt_trial(hipStream_t st, int loss, const SktData& sd, const KpCam* cams, int C, int K, double* part, double* res) {
  unsigned blocks;
  if (C < 1 || C > kKpMaxCams || !skt_grid(sd, K, blocks)) return 1;
  if (with_int(SktLossList{}, loss, [&](auto L) {
        k_skt_trial<decltype(L)::value><<<dim3(blocks), dim3(256), 0, st>>>(sd, cams, C, K, part);
        return 0;
      }))
    return 1;
  k_skt_trial_final<<<dim3(1), dim3(256), 0, st>>>(blocks, part, res);
  return 0;
}

}  // namespace mcba
