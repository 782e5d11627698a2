// mcba_consensus.hip -- consensus triangulation (the reference has no counterpart): per point, every camera pair's two-view
// DLT point is scored against the raw detections of all cameras with the truncated reprojection cost, the cheapest names the inlier cameras,
// and the point is refitted on those alone.  The per-lane arithmetic is in mcba_consensus_math.h, where the host harness checks the same text.
//   k_consensus_lane<LOSS>   lane = point, search and refit in one launch: small rigs.  A run-time loop over the pairs, the two detections read
//                            again per pair (coalesced double2 loads from the (C, P) planes) and undistorted again; only the running best is kept.
//   k_consensus_wave         wavefront = point: the pairs k = lane, lane + 64, ... per lane, each lane its own running best, a wave arg-min over
//                            (cost, k), the winner's X and mask broadcast.  Its refit is a second launch on the same stream, lane = point again
//   k_consensus_refit<LOSS>  (one lane of a wavefront refitting while 63 wait would cost more than the 48 bytes per point in between).
//   k_consensus_lane_search  the lane form's search alone, followed by k_consensus_refit: development only (MCBA_CONSENSUS_FORM), the
//                            measurement behind the choice of the fused lane form.
// The camera table (KpCam, 21 doubles per camera) and the projection matrices derived from it (12 per camera) are staged in LDS once per
// workgroup.  No atomics, no cross-workgroup traffic.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdlib.h>
#include <string.h>
// No contraction of a * b + c beyond the fma() calls the text spells out: the backend's choice of what to contract depends on the code around an
// expression, and the forms below must score a hypothesis alike to the last bit to pick the same winner of an exact tie.
#pragma clang fp contract(off)
#include "mcba_kernels.h"
#include "mcba_consensus_math.h"

namespace mcba {

// s_cam: C entries; s_proj: C x 12 or nullptr.  Every thread of the workgroup calls this (two barriers).
__device__ __forceinline__ void stage_consensus(KpCam* s_cam, double* s_proj, const KpCam* __restrict__ cams, int C) {
  const double* src = reinterpret_cast<const double*>(cams);
  double* dst = reinterpret_cast<double*>(s_cam);
  for (int i = threadIdx.x; i < 21 * C; i += blockDim.x) dst[i] = src[i];
  __syncthreads();
  if (s_proj) {
    for (int c = threadIdx.x; c < C; c += blockDim.x) cons_projection(s_cam[c], s_proj + 12 * c);
    __syncthreads();
  }
}

__device__ __forceinline__ void store_info(double* __restrict__ info, size_t p, const double* inf8) {
  if (info) {
#pragma unroll
    for (int i = 0; i < 8; ++i) info[8 * p + i] = inf8[i];
  }
}

template <int LOSS>
__global__ __launch_bounds__(256) void k_consensus_lane(const double2* __restrict__ uvs, size_t npts, const KpCam* __restrict__ cams, int C, double threshold, int min_views, int und_iters,
                                                        double f_scale, int max_iterations, double* __restrict__ out, unsigned long long* __restrict__ mask, double* __restrict__ info) {
  __shared__ KpCam s_cam[kKpMaxCams];
  __shared__ double s_proj[12 * kKpMaxCams];
  stage_consensus(s_cam, s_proj, cams, C);
  const size_t p = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (p >= npts) return;
  const double2* det = uvs + p;
  auto observation = [&](int c, double& ou, double& ov) {
    const double2 o = det[(size_t)c * npts];
    ou = o.x; ov = o.y;
  };
  double X[3], inf8[8];
  unsigned long long m;
  consensus_point<LOSS>(s_cam, s_proj, C, observation, threshold, min_views, und_iters, f_scale, max_iterations, X, m, inf8);
  out[3 * p] = X[0]; out[3 * p + 1] = X[1]; out[3 * p + 2] = X[2];
  mask[p] = m;
  store_info(info, p, inf8);
}

// what a search leaves for k_consensus_refit: start (P, 3) the winner's X, mask (P), hyp (P, 2) = (cost, k as a double; kConsNone: no hypothesis)
__device__ __forceinline__ void store_best(const ConsBest& b, size_t p, double* __restrict__ start, unsigned long long* __restrict__ mask, double* __restrict__ hyp) {
  start[3 * p] = b.X[0]; start[3 * p + 1] = b.X[1]; start[3 * p + 2] = b.X[2];
  mask[p] = b.mask;
  hyp[2 * p] = b.cost; hyp[2 * p + 1] = (double)b.k;
}

__global__ __launch_bounds__(256) void k_consensus_lane_search(const double2* __restrict__ uvs, size_t npts, const KpCam* __restrict__ cams, int C, double threshold, int und_iters,
                                                               double* __restrict__ start, unsigned long long* __restrict__ mask, double* __restrict__ hyp) {
  __shared__ KpCam s_cam[kKpMaxCams];
  __shared__ double s_proj[12 * kKpMaxCams];
  stage_consensus(s_cam, s_proj, cams, C);
  const size_t p = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (p >= npts) return;
  const double2* det = uvs + p;
  auto observation = [&](int c, double& ou, double& ov) {
    const double2 o = det[(size_t)c * npts];
    ou = o.x; ov = o.y;
  };
  ConsBest best;
  cons_best_init(best);
  consensus_search(s_cam, s_proj, C, observation, threshold, und_iters, 0, 1, best);
  store_best(best, p, start, mask, hyp);
}

constexpr int kWavePoints = 4;   // points (wavefronts) of one workgroup of k_consensus_wave

__global__ __launch_bounds__(256) void k_consensus_wave(const double2* __restrict__ uvs, size_t npts, const KpCam* __restrict__ cams, int C, double threshold, int und_iters,
                                                        double* __restrict__ start, unsigned long long* __restrict__ mask, double* __restrict__ hyp) {
  __shared__ KpCam s_cam[kKpMaxCams];
  __shared__ double s_proj[12 * kKpMaxCams];
  __shared__ double2 s_det[kWavePoints][kKpMaxCams];   // the point's detections, read once per wavefront
  stage_consensus(s_cam, s_proj, cams, C);
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const size_t p = (size_t)blockIdx.x * kWavePoints + wave;
  if (p >= npts) return;  // whole wavefront; no workgroup barrier follows
  double2* det = s_det[wave];
  for (int c = lane; c < C; c += 64) det[c] = uvs[(size_t)c * npts + p];
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
  auto observation = [&](int c, double& ou, double& ov) {
    const double2 o = det[c];
    ou = o.x; ov = o.y;
  };
  ConsBest best;
  cons_best_init(best);
  consensus_search(s_cam, s_proj, C, observation, threshold, und_iters, lane, 64, best);
  // arg-min over the lanes of (cost, k); every lane ends with the same pair
  double bc = best.cost;
  int bk = best.k;
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    const double oc = __shfl_xor(bc, off, 64);
    const int ok = __shfl_xor(bk, off, 64);
    const bool take = cons_before(oc, ok, bc, bk);
    bc = take ? oc : bc;
    bk = take ? ok : bk;
  }
  const int owner = bk == kConsNone ? 0 : bk & 63;   // the lane that scored pair bk (no hypothesis: every lane holds the initial best)
  ConsBest win;
  win.cost = bc;
  win.k = bk;
#pragma unroll
  for (int i = 0; i < 3; ++i) win.X[i] = __shfl(best.X[i], owner, 64);
  const unsigned lo = __shfl((unsigned)(best.mask & 0xffffffffull), owner, 64), hi = __shfl((unsigned)(best.mask >> 32), owner, 64);
  win.mask = ((unsigned long long)hi << 32) | lo;
  if (lane == 0) store_best(win, p, start, mask, hyp);
}

// lane = point: the refit of a search's winner, in place on out (in: the winner's X)
template <int LOSS>
__global__ __launch_bounds__(256) void k_consensus_refit(const double2* __restrict__ uvs, size_t npts, const KpCam* __restrict__ cams, int C, int min_views, double f_scale, int max_iterations,
                                                         double* __restrict__ out, const unsigned long long* __restrict__ mask, const double* __restrict__ hyp, double* __restrict__ info) {
  __shared__ KpCam s_cam[kKpMaxCams];
  stage_consensus(s_cam, nullptr, cams, C);
  const size_t p = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (p >= npts) return;
  const double2* det = uvs + p;
  auto observation = [&](int c, double& ou, double& ov) {
    const double2 o = det[(size_t)c * npts];
    ou = o.x; ov = o.y;
  };
  ConsBest best;
  best.X[0] = out[3 * p]; best.X[1] = out[3 * p + 1]; best.X[2] = out[3 * p + 2];
  best.mask = mask[p];
  best.cost = hyp[2 * p];
  best.k = (int)hyp[2 * p + 1];
  double X[3], inf8[8];
  consensus_finish<LOSS>(s_cam, C, observation, best, min_views, f_scale, max_iterations, X, inf8);
  out[3 * p] = X[0]; out[3 * p + 1] = X[1]; out[3 * p + 2] = X[2];
  store_info(info, p, inf8);
}

// ---------------------------------------------------------------- launch wrapper
// form CONSENSUS_AUTO: the lane form up to 8 cameras, the wavefront form beyond (where the median-of-pairs kernels switch).  Development only:
// the environment variable MCBA_CONSENSUS_FORM = lane | wave | lane2 forces one form for every camera count (tests compare the forms with it;
// lane2 = k_consensus_lane_search + k_consensus_refit).
int launch_consensus(hipStream_t st, int form, int loss, const double* uvs, size_t npts, const KpCam* cams, int C, double threshold, int min_views, int und_iters, double f_scale,
                     int max_iterations, double* out, unsigned long long* mask, double* hyp, double* info) {
  if (C < 2 || C > kKpMaxCams || loss < LOSS_LINEAR || loss > LOSS_ARCTAN) return 1;
  if (form == CONSENSUS_AUTO) {
    form = C <= 8 ? CONSENSUS_LANE : CONSENSUS_WAVE;
    const char* env = getenv("MCBA_CONSENSUS_FORM");
    if (env && !strcmp(env, "lane")) form = CONSENSUS_LANE;
    else if (env && !strcmp(env, "wave")) form = CONSENSUS_WAVE;
    else if (env && !strcmp(env, "lane2")) form = CONSENSUS_LANE_SEARCH;
    else if (env && *env) return 1;
  }
  const dim3 g((unsigned)((npts + 255) / 256)), b(256);
  const double2* uv = reinterpret_cast<const double2*>(uvs);
  if (form == CONSENSUS_LANE) {
    return with_loss(loss, [&](auto L) {
      k_consensus_lane<decltype(L)::value><<<g, b, 0, st>>>(uv, npts, cams, C, threshold, min_views, und_iters, f_scale, max_iterations, out, mask, info);
      return 0;
    });
  }
  if (!hyp) return 1;
  if (form == CONSENSUS_WAVE) {
    const dim3 gw((unsigned)((npts + kWavePoints - 1) / kWavePoints));
    k_consensus_wave<<<gw, b, 0, st>>>(uv, npts, cams, C, threshold, und_iters, out, mask, hyp);
  } else if (form == CONSENSUS_LANE_SEARCH) {
    k_consensus_lane_search<<<g, b, 0, st>>>(uv, npts, cams, C, threshold, und_iters, out, mask, hyp);
  } else {
    return 1;
  }
  return with_loss(loss, [&](auto L) {
    k_consensus_refit<decltype(L)::value><<<g, b, 0, st>>>(uv, npts, cams, C, min_views, f_scale, max_iterations, out, mask, hyp, info);
    return 0;
  });
}

}  // namespace mcba
