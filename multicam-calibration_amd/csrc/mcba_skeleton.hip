// mcba_skeleton.hip -- skeleton-constrained keypoint refinement: the keypoints of a frame refined together, joined by
// bones of known length.  Everything computed is the text of mcba_skeleton_math.h (host-checked); this file owns the thread layout, the LDS and
// the barriers.  No kernel here uses an atomic: every word has one writer, every sum a fixed order, and a frame's result does not depend on
// which other frames share its workgroup.
//   k_skel_refine   thread = (frame, keypoint), keypoints fastest: 256 threads serve G = 256 / K frames, the 256 - G K last ones idle.  The camera
//                   table is staged in LDS as k_tri_refine stages it; the lanes of a frame exchange through SK_PLANES planes of doubles in LDS.
//                   The tree sweeps are level-synchronous, one barrier per level and direction.  The Levenberg-Marquardt loop is workgroup
//                   uniform: it is left on a workgroup-wide vote and finished frames idle, so no barrier sits in divergent control flow
//   k_skel_dist     thread = (bone, frame): the (E, T) plane of bone lengths for estimate_bone_lengths, NaN where an end is NaN
//   k_skel_absdev   thread = (bone, frame): |distance - the bone's median| in place
#include <hip/hip_runtime.h>

#include "mcba_device.h"
#include "mcba_kernels.h"
#include "mcba_skeleton_math.h"

namespace mcba {

// the context of skel_frame on the GPU: this thread's lane, its frame's slice of the planes, its frame's words
struct SkGpuCtx {
  SkLane ln;
  SkShared sh;
  SkFrameState* fs;
  size_t t;
  bool live;
  template <class F>
  __device__ __forceinline__ void each(F&& f) {
    if (live) f(ln, sh, *fs, t);
    __syncthreads();
  }
  template <class P>
  __device__ __forceinline__ bool any(P&& pred) {
    return __syncthreads_or(live && pred(*fs)) != 0;
  }
};

template <int LOSS>
__global__ __launch_bounds__(256) void k_skel_refine(SkArgs a, const SkPlan* __restrict__ plan, const KpCam* __restrict__ cams, int C) {
  __shared__ KpCam s_cam[kKpMaxCams];
  __shared__ SkPlan s_plan;
  __shared__ double s_v[SK_PLANES * 256];
  __shared__ int s_cls[256];
  __shared__ SkFrameState s_fs[256];
  {
    const int* src = reinterpret_cast<const int*>(plan);
    int* dst = reinterpret_cast<int*>(&s_plan);
    for (int i = threadIdx.x; i < (int)(sizeof(SkPlan) / sizeof(int)); i += 256) dst[i] = src[i];
  }
  stage_cams(s_cam, cams, C);   // (its barrier covers the plan as well)
  const int K = s_plan.K, G = skel_frames_per_group(K);
  const int g = threadIdx.x / K, k = threadIdx.x - g * K;
  SkGpuCtx cx;
  cx.t = (size_t)blockIdx.x * G + g;
  cx.live = g < G && cx.t < a.T;
  cx.ln.k = k;
  cx.sh = SkShared{s_v + g * K, s_cls + g * K, 256};
  cx.fs = s_fs + (g < G ? g : 0);
  skel_frame<LOSS>(cx, s_plan, s_cam, C, a);
}

__global__ __launch_bounds__(256) void k_skel_dist(const double* __restrict__ pts, const int* __restrict__ bones, size_t T, int K, int E, double* __restrict__ dist) {
  const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
  const int e = blockIdx.y;
  if (t >= T) return;
  const double* row = pts + 3 * t * (size_t)K;
  dist[(size_t)e * T + t] = skel_distance(row + 3 * bones[2 * e], row + 3 * bones[2 * e + 1]);
}

__global__ __launch_bounds__(256) void k_skel_absdev(double* __restrict__ dist, const SelState* __restrict__ sel, size_t T) {
  const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
  const int e = blockIdx.y;
  if (t >= T) return;
  const double med = sel_median(sel[2 * e], sel[2 * e + 1]);
  dist[(size_t)e * T + t] = fabs(dist[(size_t)e * T + t] - med);
}

int launch_skel_refine(hipStream_t st, int loss, const SkArgs& a, const SkPlan* plan_dev, int K, const KpCam* cams, int C) {
  if (C < 1 || C > kKpMaxCams || K < 1 || K > SK_MAX_K || a.T < 1) return 1;
  const size_t G = (size_t)skel_frames_per_group(K), blocks = (a.T + G - 1) / G;
  if (blocks > 0x7fffffffu) return 1;
  return with_loss(loss, [&](auto L) {
    k_skel_refine<decltype(L)::value><<<dim3((unsigned)blocks), dim3(256), 0, st>>>(a, plan_dev, cams, C);
    return 0;
  });
}

int launch_skel_dist(hipStream_t st, const double* pts, const int* bones, size_t T, int K, int E, double* dist) {
  const size_t bx = (T + 255) / 256;
  if (T < 1 || E < 1 || E > 65535 || bx > 0x7fffffffu) return 1;
  k_skel_dist<<<dim3((unsigned)bx, (unsigned)E), dim3(256), 0, st>>>(pts, bones, T, K, E, dist);
  return 0;
}

int launch_skel_absdev(hipStream_t st, double* dist, const SelState* sel, size_t T, int E) {
  const size_t bx = (T + 255) / 256;
  if (T < 1 || E < 1 || E > 65535 || bx > 0x7fffffffu) return 1;
  k_skel_absdev<<<dim3((unsigned)bx, (unsigned)E), dim3(256), 0, st>>>(dist, sel, T);
  return 0;
}

}  // namespace mcba
