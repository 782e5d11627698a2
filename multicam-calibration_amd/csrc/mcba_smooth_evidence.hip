// mcba_smooth_evidence.hip -- the smoother's evidence: after launch_smooth_reduce and launch_smooth_backsub of
// mcba_smooth.hip, the three sums of a track's N(accel_std).  Per-lane arithmetic: mcba_smooth_evidence_math.h (host-checked).  No kernel here
// uses an atomic: every word has one writer, every sum a fixed order that depends on (T, segment) alone.
//   k_evidence_logdet  lane = (segment, track), tracks fastest, as k_smooth_reduce: the sum of log over the six stored diagonal planes of every block
//                      the lane factorised -- the plane reads of a wavefront are consecutive doubles
//   k_evidence_eval    workgroup = 256 frames of a track: sum w d^2 and the sum of squared second differences
//   k_evidence_final   workgroup = track: its eval partials, its lane partials of every level in level order, each by one fixed tree; its refused-pivot flag
#include <hip/hip_runtime.h>

#include "mcba_device.h"
#include "mcba_kernels.h"
#include "mcba_smooth_evidence_math.h"

namespace mcba {

// lane[(off + q) nact + kk]: the partial of segment q of the kk-th running track on this level
__global__ __launch_bounds__(64) void k_evidence_logdet(SmLevel lv, int K, const int* __restrict__ list, int nact, int nq, size_t off, double* __restrict__ lane) {
  const size_t gid = (size_t)blockIdx.x * 64 + threadIdx.x;
  if (gid >= (size_t)nq * nact) return;
  lane[off * nact + gid] = evidence_lane_logsum(lv, K, list[gid % nact], (int)(gid / nact));
}

__global__ __launch_bounds__(256) void k_evidence_eval(SmData td, int K, const int* __restrict__ list, int nblk, double* __restrict__ part) {
  __shared__ double s_r[2][256];
  const int kk = blockIdx.x / nblk, b = blockIdx.x % nblk;
  const size_t t = (size_t)b * 256 + threadIdx.x;
  double r[2] = {0.0, 0.0};
  if (t < td.T) evidence_eval_frame(td, K, list[kk], t, r);
  const bool is_max[2] = {false, false};
  block_tree<2>(s_r, r, is_max);
  if (threadIdx.x < 2) part[2 * (size_t)blockIdx.x + threadIdx.x] = s_r[threadIdx.x][0];
}

// res[EV_RES kk ..] = (sum w d^2, sum |second difference|^2, sum log of the stored pivots, bad[list[kk]] != 0) of the kk-th running track
__global__ __launch_bounds__(256) void k_evidence_final(int nact, int nblk, const double* __restrict__ part, size_t lanes, const double* __restrict__ lane, const int* __restrict__ list,
                                                        const int* __restrict__ bad, double* __restrict__ res) {
  __shared__ double s_r[3][256];
  const int kk = blockIdx.x;
  double r[3] = {0.0, 0.0, 0.0};
  for (int b = threadIdx.x; b < nblk; b += 256) {
    const double* p = part + 2 * ((size_t)kk * nblk + b);
    r[0] += p[0]; r[1] += p[1];
  }
  for (size_t j = threadIdx.x; j < lanes; j += 256) r[2] += lane[j * nact + kk];
  const bool is_max[3] = {false, false, false};
  block_tree<3>(s_r, r, is_max);
  if (threadIdx.x < 3) res[EV_RES * (size_t)kk + threadIdx.x] = s_r[threadIdx.x][0];
  if (threadIdx.x == 3) res[EV_RES * (size_t)kk + 3] = bad[list[kk]] ? 1.0 : 0.0;
}

// after launch_smooth_reduce and launch_smooth_backsub of the nact running tracks of list: res (nact, EV_RES).  td: x and d2 at the solution, w the
// weights the matrix was built with; bad: the flags of launch_smooth_reduce.  part: 2 smooth_eval_blocks(T) nact doubles, lane: evidence_lanes() nact doubles of scratch.
// marks: null, or an event recorded between the evaluation of the two cost sums and the log-determinant kernels
int launch_smooth_evidence(hipStream_t st, const SmLevel* lv, int levels, const SmData& td, int K, const int* list, int nact, const int* bad, double* part, double* lane, double* res, hipEvent_t mark) {
  if (levels < 1 || levels > SM_MAX_LEVELS || nact < 1 || nact > K) return 1;
  const int nblk = smooth_eval_blocks(td.T);
  if ((size_t)nblk * nact > 0x7fffffffu) return 1;
  k_evidence_eval<<<dim3((unsigned)(nblk * nact)), dim3(256), 0, st>>>(td, K, list, nblk, part);
  if (mark && hipEventRecord(mark, st) != hipSuccess) return 1;
  size_t off[SM_MAX_LEVELS];
  const size_t lanes = evidence_lanes(lv, levels, off);
  for (int l = 0; l < levels; ++l) {
    int nq;
    unsigned blocks;
    if (!smooth_grid(lv[l], nact, nq, blocks)) return 1;
    k_evidence_logdet<<<dim3(blocks), dim3(64), 0, st>>>(lv[l], K, list, nact, nq, off[l], lane);
  }
  k_evidence_final<<<dim3((unsigned)nact), dim3(256), 0, st>>>(nact, nblk, part, lanes, lane, list, bad, res);
  return 0;
}

}  // namespace mcba
