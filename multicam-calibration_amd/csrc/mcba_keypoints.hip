// mcba_keypoints.hip -- what a lab does with a calibration, per tracked keypoint (reference geometry.py:128-152, :277-325):
//   k_project          3-D points into every camera of the table (`project_points`; the k1, k2 model of the reference or the five-coefficient
//                      forward model), or through one rigid transform (`apply_rigid_transform`)
//   k_keypoint_errors  the distance between each camera's detection and the projection of the point, in rows the radix select (mcba_diag.hip:
//                      launch_select) then takes the per-camera medians of
//   k_tri_refine       per point, Levenberg-Marquardt on the robust reprojection cost from the median-of-pairs estimate of k_triangulate
// Lane = point everywhere.  The camera table (21 doubles per camera, at most kKpMaxCams per launch) is staged in LDS once per workgroup and read
// from there with wave-uniform addresses (LDS broadcasts); points and detections are read coalesced from (C, P) planes.  No atomics, no
// cross-workgroup traffic.  The per-lane arithmetic is in mcba_keypoint_math.h, where the host harness checks the same text.
#include <hip/hip_runtime.h>
#include <math.h>
#include <algorithm>
#include "mcba_kernels.h"
#include "mcba_keypoint_math.h"

// (in both compilation passes: the weighted functor is taken for weighted, the plain one for unweighted)
static_assert(mcba::KpWeighted<mcba::KpDetections<true>>::value && !mcba::KpWeighted<mcba::KpDetections<false>>::value, "the observation functors select the weighted arithmetic");

namespace mcba {

// MODE 0: k1, k2 (project_only, the reference's project_points); 1: five coefficients; 2: the rigid transform of camera 0 alone, out (P, 3).
// MODE 0 / 1: out (C, P) double2 planes -- consecutive lanes store consecutive 16-byte elements.  24 + 16 C bytes per point.
template <int MODE>
__global__ __launch_bounds__(256) void k_project(const double* __restrict__ pts, size_t npts, const KpCam* __restrict__ cams, int C, double* __restrict__ out) {
  __shared__ KpCam s_cam[kKpMaxCams];
  stage_cams(s_cam, cams, C);
  for (size_t p = (size_t)blockIdx.x * 256 + threadIdx.x; p < npts; p += (size_t)gridDim.x * 256) {
    const double X[3] = {pts[3 * p], pts[3 * p + 1], pts[3 * p + 2]};
    if (MODE == 2) {
      double Xc[3];
      rigid_point(s_cam[0].pc, X, Xc);
      out[3 * p] = Xc[0]; out[3 * p + 1] = Xc[1]; out[3 * p + 2] = Xc[2];
    } else {
      double2* o = reinterpret_cast<double2*>(out) + p;
      for (int c = 0; c < C; ++c) {
        double2 r;
        if (MODE == 0) project_only(s_cam[c].K, s_cam[c].pc, X, r.x, r.y);
        else project5<false>(s_cam[c], X, r.x, r.y);
        o[(size_t)c * npts] = r;
      }
    }
  }
}

// err rows (C, Ppad): |detection - projection|, NaN where unseen and in the padding (the select skips NaNs).  24 + 16 C + 8 C bytes per point.
__global__ __launch_bounds__(256) void k_keypoint_errors(const double* __restrict__ pts, const double2* __restrict__ uvs, size_t npts, size_t npad, const KpCam* __restrict__ cams, int C,
                                                         double* __restrict__ err) {
  __shared__ KpCam s_cam[kKpMaxCams];
  stage_cams(s_cam, cams, C);
  const double nan = __builtin_nan("");
  for (size_t p = (size_t)blockIdx.x * 256 + threadIdx.x; p < npad; p += (size_t)gridDim.x * 256) {
    const bool in = p < npts;
    const double X[3] = {in ? pts[3 * p] : nan, in ? pts[3 * p + 1] : nan, in ? pts[3 * p + 2] : nan};
    for (int c = 0; c < C; ++c) {
      const double2 o = in ? uvs[(size_t)c * npts + p] : double2{nan, nan};
      err[(size_t)c * npad + p] = keypoint_error(s_cam[c], X, o.x, o.y);
    }
  }
}

// one lane = one point, any C <= kKpMaxCams: the loop over the cameras is a run-time loop over the LDS table, the detections are read again at
// every linearisation (coalesced double2 loads) instead of being kept in per-camera register arrays.  info (P, 4) or nullptr.
// WEIGHTED: sw, the (C, P) plane of sqrt(weight), is read beside each detection (one more coalesced 8-byte load); otherwise it is never touched.
template <int LOSS, bool WEIGHTED>
__global__ __launch_bounds__(256) void k_tri_refine(const double2* __restrict__ uvs, const double* __restrict__ start, size_t npts, const KpCam* __restrict__ cams, int C, double f_scale,
                                                    int max_iterations, double* __restrict__ out, double* __restrict__ info, const double* __restrict__ sw) {
  __shared__ KpCam s_cam[kKpMaxCams];
  stage_cams(s_cam, cams, C);
  const size_t p = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (p >= npts) return;
  const double X0[3] = {start[3 * p], start[3 * p + 1], start[3 * p + 2]};
  KpDetections<WEIGHTED> observation(uvs, sw, npts, p);
  double X[3], inf4[4];
  refine_point<LOSS>(s_cam, C, observation, X0, f_scale, max_iterations, X, inf4);
  out[3 * p] = X[0]; out[3 * p + 1] = X[1]; out[3 * p + 2] = X[2];
  if (info) {
#pragma unroll
    for (int i = 0; i < 4; ++i) info[4 * p + i] = inf4[i];
  }
}

// ---------------------------------------------------------------- launch wrappers (cams: device memory, C <= kKpMaxCams cameras of one group)
static unsigned stream_grid(size_t n) { return (unsigned)std::min<size_t>((n + 255) / 256, 4096); }

int launch_project(hipStream_t st, int mode, const double* pts, size_t npts, const KpCam* cams, int C, double* out) {
  if (C < 1 || C > kKpMaxCams || mode < 0 || mode > 2) return 1;
  const dim3 g(stream_grid(npts)), b(256);
  if (mode == 0) k_project<0><<<g, b, 0, st>>>(pts, npts, cams, C, out);
  else if (mode == 1) k_project<1><<<g, b, 0, st>>>(pts, npts, cams, C, out);
  else k_project<2><<<g, b, 0, st>>>(pts, npts, cams, 1, out);
  return 0;
}

int launch_keypoint_errors(hipStream_t st, const double* pts, const double* uvs, size_t npts, size_t npad, const KpCam* cams, int C, double* err) {
  if (C < 1 || C > kKpMaxCams || npad < npts) return 1;
  k_keypoint_errors<<<dim3(stream_grid(npad)), dim3(256), 0, st>>>(pts, reinterpret_cast<const double2*>(uvs), npts, npad, cams, C, err);
  return 0;
}

int launch_tri_refine(hipStream_t st, int loss, const double* uvs, const double* start, size_t npts, const KpCam* cams, int C, double f_scale, int max_iterations, double* out, double* info,
                      const double* sw) {
  if (C < 2 || C > kKpMaxCams) return 1;
  const dim3 g((unsigned)((npts + 255) / 256)), b(256);
  const double2* uv = reinterpret_cast<const double2*>(uvs);
  return with_weights(sw, [&](auto W) {
    return with_loss(loss, [&](auto L) {
      k_tri_refine<decltype(L)::value, decltype(W)::value><<<g, b, 0, st>>>(uv, start, npts, cams, C, f_scale, max_iterations, out, info, sw);
      return 0;
    });
  });
}

}  // namespace mcba
