// mcba_smooth.hip -- trajectory smoothing: the fixed-interval smoother of keypoint tracks, one block-pentadiagonal
// SPD system per track and IRLS iteration, solved by a recursive partitioned (Schur) elimination.  Per-lane arithmetic: mcba_smooth_math.h
// (host-checked).  No kernel here uses an atomic: every word has one writer, every sum a fixed order.
//   k_smooth_prepare   lane = (frame, track): usable flag, Sigma^-1 (packed), the start weights
//   k_smooth_count     workgroup = track: its usable frames
//   k_smooth_reduce    lane = (segment, track), tracks fastest: forward elimination through the segment's interior, the Schur terms of its separators
//   k_smooth_resolve   lane = (segment, track): the forward pass alone for a new right-hand side, from the stored factors
//   k_smooth_backsub   lane = (segment, track): the interior's solution from its separators'; level 0 also writes d^2, the new weights, the step
//   k_smooth_eval      workgroup = 256 frames of a track: the sums of the objective, the largest step and coordinate; k_smooth_final adds them
#include <hip/hip_runtime.h>

#include "mcba_device.h"
#include "mcba_kernels.h"
#include "mcba_smooth_math.h"

namespace mcba {

__global__ __launch_bounds__(256) void k_smooth_prepare(size_t count, const double* __restrict__ pts, const double* __restrict__ cov6, const double* __restrict__ w_in, double* __restrict__ p,
                                                        double* __restrict__ winv, double* __restrict__ w) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= count) return;
  double p3[3], c6[6], po[3], wi[6], wo;
#pragma unroll
  for (int e = 0; e < 3; ++e) p3[e] = pts[3 * i + e];
#pragma unroll
  for (int e = 0; e < 6; ++e) c6[e] = cov6[6 * i + e];
  smooth_prepare_lane(p3, c6, w_in ? w_in[i] : 1.0, po, wi, wo);
#pragma unroll
  for (int e = 0; e < 3; ++e) p[3 * i + e] = po[e];
#pragma unroll
  for (int e = 0; e < 6; ++e) winv[6 * i + e] = wi[e];
  w[i] = wo;
}

__global__ __launch_bounds__(256) void k_smooth_count(size_t T, int K, const double* __restrict__ winv, int* __restrict__ n_usable) {
  __shared__ double s_r[1][256];
  const int k = blockIdx.x;
  double r[1] = {0.0};
  for (size_t t = threadIdx.x; t < T; t += 256) r[0] += winv[6 * (t * K + k)] != 0.0 ? 1.0 : 0.0;   // (counts: exact in any order)
  const bool is_max[1] = {false};
  block_tree<1>(s_r, r, is_max);
  if (threadIdx.x == 0) n_usable[k] = (int)s_r[0][0];
}

// lane -> (segment q, position kk in the list of running tracks), tracks fastest.  No launch bound beyond the workgroup size: the lane's
// state is about 150 doubles and wants the whole register file
template <bool LEVEL0, bool RHS = false>
__global__ __launch_bounds__(64) void k_smooth_reduce(SmLevel lv, SmLevel nx, SmData td, int K, const int* __restrict__ list, int nact, int nq, int* __restrict__ bad) {
  const size_t gid = (size_t)blockIdx.x * 64 + threadIdx.x;
  if (gid >= (size_t)nq * nact) return;
  smooth_reduce_lane<LEVEL0, RHS>(lv, nx, td, K, list[gid % nact], (int)(gid / nact), bad);
}

// the forward pass again for a new right-hand side, the factors of k_smooth_reduce in place (smooth_resolve_lane).  done: null, or a word in
// device memory: non-zero = the caller's iteration has ended and the launch returns at once
template <bool LEVEL0>
__global__ __launch_bounds__(64) void k_smooth_resolve(SmLevel lv, SmLevel nx, SmData td, int K, const int* __restrict__ list, int nact, int nq, const int* __restrict__ done) {
  if (done && *done) return;
  const size_t gid = (size_t)blockIdx.x * 64 + threadIdx.x;
  if (gid >= (size_t)nq * nact) return;
  smooth_resolve_lane<LEVEL0>(lv, nx, td, K, list[gid % nact], (int)(gid / nact));
}

template <bool LEVEL0, bool RHS = false>
__global__ __launch_bounds__(64) void k_smooth_backsub(SmLevel lv, SmLevel up, SmData td, int K, const int* __restrict__ list, int nact, int nq) {
  const size_t gid = (size_t)blockIdx.x * 64 + threadIdx.x;
  if (gid >= (size_t)nq * nact) return;
  smooth_backsub_lane<LEVEL0, RHS>(lv, up, td, K, list[gid % nact], (int)(gid / nact));
}

__global__ __launch_bounds__(256) void k_smooth_eval(SmData td, int K, const int* __restrict__ list, int nblk, double* __restrict__ part) {
  __shared__ double s_r[4][256];
  const int kk = blockIdx.x / nblk, b = blockIdx.x % nblk;
  const size_t t = (size_t)b * 256 + threadIdx.x;
  double r[4] = {0.0, 0.0, 0.0, 0.0};
  if (t < td.T) smooth_eval_frame(td, K, list[kk], t, r);
  const bool is_max[4] = {false, false, true, true};
  block_tree<4>(s_r, r, is_max);
  if (threadIdx.x < 4) part[4 * (size_t)blockIdx.x + threadIdx.x] = s_r[threadIdx.x][0];
}

// res[4 kk ..] = (objective, step, max |x|, 0) of the kk-th running track
__global__ __launch_bounds__(256) void k_smooth_final(SmData td, const int* __restrict__ list, int nblk, const double* __restrict__ part, double* __restrict__ res) {
  __shared__ double s_r[4][256];
  const int kk = blockIdx.x;
  double r[4] = {0.0, 0.0, 0.0, 0.0};
  for (int b = threadIdx.x; b < nblk; b += 256) {
    const double* p = part + 4 * ((size_t)kk * nblk + b);
    r[0] += p[0]; r[1] += p[1]; r[2] = fmax(r[2], p[2]); r[3] = fmax(r[3], p[3]);
  }
  const bool is_max[4] = {false, false, true, true};
  block_tree<4>(s_r, r, is_max);
  if (threadIdx.x == 0) {
    res[4 * kk] = smooth_objective(s_r[0][0], s_r[1][0], td.f2, td.ia2[list[kk]]);
    res[4 * kk + 1] = s_r[2][0];
    res[4 * kk + 2] = s_r[3][0];
    res[4 * kk + 3] = 0.0;
  }
}

void launch_smooth_prepare(hipStream_t st, size_t T, int K, const double* pts, const double* cov6, const double* w_in, double* p, double* winv, double* w, int* n_usable) {
  const size_t count = T * K;
  k_smooth_prepare<<<dim3((unsigned)((count + 255) / 256)), dim3(256), 0, st>>>(count, pts, cov6, w_in, p, winv, w);
  k_smooth_count<<<dim3((unsigned)K), dim3(256), 0, st>>>(T, K, winv, n_usable);
}

// the elimination of the nact running tracks of `list` (positions in the chunk of K tracks), every level up: the factors stay in lv[.].fac, lv[.].sep
// rhs: level 0 in the right-hand-side mode (SmData::rhs)
int launch_smooth_reduce(hipStream_t st, const SmLevel* lv, int levels, const SmData& td, int K, const int* list, int nact, int* bad, bool rhs) {
  if (levels < 1 || levels > SM_MAX_LEVELS || nact < 1 || nact > K) return 1;
  const SmLevel none{};
  for (int l = 0; l < levels; ++l) {
    int nq;
    unsigned blocks;
    if (!smooth_grid(lv[l], nact, nq, blocks)) return 1;
    const SmLevel& nx = l + 1 < levels ? lv[l + 1] : none;
    if (l == 0 && rhs) k_smooth_reduce<true, true><<<dim3(blocks), dim3(64), 0, st>>>(lv[0], nx, td, K, list, nact, nq, bad);
    else if (l == 0) k_smooth_reduce<true><<<dim3(blocks), dim3(64), 0, st>>>(lv[0], nx, td, K, list, nact, nq, bad);
    else k_smooth_reduce<false><<<dim3(blocks), dim3(64), 0, st>>>(lv[l], nx, td, K, list, nact, nq, bad);
  }
  return 0;
}

// after launch_smooth_reduce(rhs = true): the forward pass of every level again for the right-hand side td.rhs now holds; launch_smooth_backsub(rhs =
// true) follows it
int launch_smooth_resolve(hipStream_t st, const SmLevel* lv, int levels, const SmData& td, int K, const int* list, int nact, const int* done) {
  if (levels < 1 || levels > SM_MAX_LEVELS || nact < 1 || nact > K) return 1;
  const SmLevel none{};
  for (int l = 0; l < levels; ++l) {
    int nq;
    unsigned blocks;
    if (!smooth_grid(lv[l], nact, nq, blocks)) return 1;
    const SmLevel& nx = l + 1 < levels ? lv[l + 1] : none;
    if (l == 0) k_smooth_resolve<true><<<dim3(blocks), dim3(64), 0, st>>>(lv[0], nx, td, K, list, nact, nq, done);
    else k_smooth_resolve<false><<<dim3(blocks), dim3(64), 0, st>>>(lv[l], nx, td, K, list, nact, nq, done);
  }
  return 0;
}

// the back-substitution after launch_smooth_reduce, every level down; rhs as there (level 0 then writes the solution alone)
int launch_smooth_backsub(hipStream_t st, const SmLevel* lv, int levels, const SmData& td, int K, const int* list, int nact, bool rhs) {
  if (levels < 1 || levels > SM_MAX_LEVELS || nact < 1 || nact > K) return 1;
  const SmLevel none{};
  for (int l = levels - 1; l >= 0; --l) {
    int nq;
    unsigned blocks;
    if (!smooth_grid(lv[l], nact, nq, blocks)) return 1;
    const SmLevel& up = l + 1 < levels ? lv[l + 1] : none;
    if (l == 0 && rhs) k_smooth_backsub<true, true><<<dim3(blocks), dim3(64), 0, st>>>(lv[0], up, td, K, list, nact, nq);
    else if (l == 0) k_smooth_backsub<true><<<dim3(blocks), dim3(64), 0, st>>>(lv[0], up, td, K, list, nact, nq);
    else k_smooth_backsub<false><<<dim3(blocks), dim3(64), 0, st>>>(lv[l], up, td, K, list, nact, nq);
  }
  return 0;
}

// one linear solve of the nact running tracks of `list`, then their sums: res (nact, 4)
int launch_smooth_solve(hipStream_t st, const SmLevel* lv, int levels, const SmData& td, int K, const int* list, int nact, int* bad, double* part, double* res) {
  if (launch_smooth_reduce(st, lv, levels, td, K, list, nact, bad)) return 1;
  if (launch_smooth_backsub(st, lv, levels, td, K, list, nact)) return 1;
  const int nblk = smooth_eval_blocks(td.T);
  if ((size_t)nblk * nact > 0x7fffffffu) return 1;
  k_smooth_eval<<<dim3((unsigned)(nblk * nact)), dim3(256), 0, st>>>(td, K, list, nblk, part);
  k_smooth_final<<<dim3((unsigned)nact), dim3(256), 0, st>>>(td, list, nblk, part, res);
  return 0;
}

}  // namespace mcba
