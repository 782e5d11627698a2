// mcba_kpcam.hip -- free-point bundle adjustment of the cameras on keypoint detections with the intrinsics among the unknowns (SURVEY.md section
// 8f-15): the Schur reduction over the 3 x 3 point blocks into the 12 C x 12 C camera system, and the back-substitution with the trial cost under
// trial intrinsics and extrinsics.  Arithmetic: mcba_kpcam_math.h (host-checked).  mcba_kpba.hip with 12 rows per camera:
//   k_kpba_status   reused as it is (a point's status does not depend on which camera scalars are free)
//   k_kpcam_reduce  a workgroup walks chunks of 256 points.  Phase 1, lane = point: H_p, g_p, the factor L_p of the damped Jacobi-scaled block,
//                   z_p = L^-1 D g_p -> LDS.  Then per group of G points, in two passes, HALF 0 (the intrinsic rows 0 .. 5) and HALF 1 (the
//                   extrinsic rows 6 .. 11): item (camera, point), points fastest, writes its six rows of Y_cp = W_cp D L^-T into the
//                   (NP x 3 G) panel (zero rows: unseeing cameras, held scalars, padding) and sums its rows of U_c, g_c, Y_cp z_p over the
//                   group's points by a butterfly of fixed order.  The half is uniform over the workgroup, so a wavefront never runs both
//                   bodies, and an item carries 18 + 33 or 18 + 69 doubles, not 36 + 102.  Y Y^T on v_mfma_f64_16x16x4_f64, tiles on or below
//                   the diagonal only, each owned by one wavefront, accumulated in registers over all the workgroup's groups.  One partial
//                   system per workgroup.
//   k_kpba_finish   reused (its sizes are arguments): the partials in workgroup order -> the system
//   k_kpcam_step    lane = point: the blocks again at the current iterate with q = sum_c W_cp^T dtheta_c over 12 columns in the same pass,
//                   dX = -(H + lam diag H)^-1 (g + q), the trial point into the second buffer, its cost under the trial camera table
// No atomics: every sum has one order, the same in every call.
//
// Dynamic LDS of k_kpcam_reduce, in doubles:  256 * 13  +  102 C  +  NP * (3 G + 1),   NP = 12 C rounded up to 16
//   s_pt [256][13] (L 6 | d 3 | z 3 | usable)  |  s_acc [C][102]  |  s_Y [NP][RS], RS = 3 G + 1 (odd: the 16 rows a matrix-core operand reads
//   fall into 16 distinct bank pairs).  Static beside it: the camera table, the held words and the block tree's 3 x 256 doubles, counted as
//   12 KiB.  G is 64 if that fits the device's opt-in limit, else 32, else 16 (on 160 KiB: 64 up to 5 cameras, 32 up to 12).
// Partial system of a workgroup, NP NP + 102 C + 4 doubles: Y Y^T (only the tiles on or below the diagonal are written) | acc | cost, present
// scalars, max |g_p|, 0.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "mcba_device.h"
#include "mcba_kernels.h"
#include "mcba_kpcam_math.h"

namespace mcba {

typedef double kpcam_d4 __attribute__((ext_vector_type(4)));

constexpr int kKcChunk = 256;   // points of one phase 1 (kpba_groups counts chunks of this size)
constexpr int kKcPt = 13;       // per point in LDS: L (6) | d (3) | z (3) | usable (1)
constexpr size_t kKcStaticLds = 12 * 1024;

size_t kpcam_reduce_lds(int C, int G) {
  const int NP = (kKcRows * C + 15) / 16 * 16;
  return ((size_t)kKcChunk * kKcPt + (size_t)C * kKcAcc + (size_t)NP * (3 * G + 1)) * sizeof(double);
}
size_t kpcam_partial_size(int C) {
  const int NP = (kKcRows * C + 15) / 16 * 16;
  return (size_t)NP * NP + (size_t)C * kKcAcc + 4;
}
// points per group: 64 if its panel fits, else 32, else 16; force_g (16, 32 or 64: tests) overrides when it fits.  0: nothing fits
int kpcam_group(int C, int lds_limit, int force_g) {
  if ((force_g == 16 || force_g == 32 || force_g == 64) && kpcam_reduce_lds(C, force_g) + kKcStaticLds <= (size_t)lds_limit) return force_g;
  for (int G = 64; G >= 16; G >>= 1)
    if (kpcam_reduce_lds(C, G) + kKcStaticLds <= (size_t)lds_limit) return G;
  return 0;
}

// ---------------------------------------------------------------- k_kpcam_reduce
// one pass over the items of a group: the rows 6 HALF .. 6 HALF + 5 of every camera
template <int LOSS, bool WEIGHTED, int HALF>
__device__ __forceinline__ void kpcam_items(const double2* __restrict__ uvs, const double* __restrict__ pts, const double* __restrict__ sw, size_t npts, size_t p0, int sub, int G, int C, int RS,
                                            const TcCam* s_cam, const int* s_held, const double* s_pt, double* s_acc, double* s_Y, double fs2, double inv_fs2) {
  constexpr int NS = kpcam_half_size(HALF);
  for (int it = threadIdx.x; it < C * G; it += 256) {
    const int g = it % G, c = it / G, pl = sub * G + g;
    const double* sp = s_pt + pl * kKcPt;
    double Y[18], a[NS];
#pragma unroll
    for (int k = 0; k < 18; ++k) Y[k] = 0.0;
#pragma unroll
    for (int k = 0; k < NS; ++k) a[k] = 0.0;
    if (sp[12] != 0.0) {   // (a point past P is not usable)
      const size_t p = p0 + pl;
      const double2 o = uvs[(size_t)c * npts + p];
      const double sq = WEIGHTED ? sw[(size_t)c * npts + p] : 1.0;
      if (o.x == o.x && o.y == o.y && sq > 0.0) {
        const double X[3] = {pts[3 * p], pts[3 * p + 1], pts[3 * p + 2]};
        KbFactor f;
#pragma unroll
        for (int i = 0; i < 6; ++i) f.L[i] = sp[i];
#pragma unroll
        for (int i = 0; i < 3; ++i) f.d[i] = sp[6 + i];
        kpcam_item_w<LOSS, WEIGHTED, HALF>(s_cam[c], X, o.x, o.y, sq, fs2, inv_fs2, f, sp + 9, s_held[c], Y, a);
      }
    }
#pragma unroll
    for (int i = 0; i < 6; ++i) {
#pragma unroll
      for (int k = 0; k < 3; ++k) s_Y[(size_t)(kKcRows * c + 6 * HALF + i) * RS + 3 * g + k] = Y[3 * i + k];
    }
    // the camera's sums over the group's G points: C G is a multiple of G and G divides 64, so a group's lanes are all here or all absent
    for (int m = G >> 1; m > 0; m >>= 1) {
#pragma unroll
      for (int k = 0; k < NS; ++k) a[k] += __shfl_xor(a[k], m);
    }
    if (g == 0) {
#pragma unroll
      for (int k = 0; k < NS; ++k) s_acc[c * kKcAcc + kpcam_half_slot(HALF, k)] += a[k];   // (these slots of camera c are this lane's alone until the next barrier)
    }
  }
}

template <int LOSS, int TQ, bool WEIGHTED>
__global__ __launch_bounds__(256) void k_kpcam_reduce(const double2* __restrict__ uvs, const double* __restrict__ pts, const int* __restrict__ status, size_t npts, const TcCam* __restrict__ cams,
                                                      const int* __restrict__ held, int C, double f_scale, double lam, int G, double* __restrict__ part, const double* __restrict__ sw) {
  extern __shared__ __align__(16) double lds[];
  __shared__ TcCam s_cam[kKcMaxCams];
  __shared__ int s_held[kKcMaxCams];
  __shared__ double s_r[3][256];
  const int t = threadIdx.x, lane = t & 63;
  const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
  const int n12 = kKcRows * C, NP = (n12 + 15) / 16 * 16, NT = NP / 16, ntiles = NT * (NT + 1) / 2, RS = 3 * G + 1;
  double* s_pt = lds;                                   // [256][13]
  double* s_acc = s_pt + kKcChunk * kKcPt;              // [C][102]
  double* s_Y = s_acc + C * kKcAcc;                     // [NP][RS]
  const double fs2 = f_scale * f_scale, inv_fs2 = 1.0 / fs2;
  {
    const double* src = reinterpret_cast<const double*>(cams);
    double* dst = reinterpret_cast<double*>(s_cam);
    for (int i = t; i < 30 * C; i += 256) dst[i] = src[i];
    for (int i = t; i < C; i += 256) s_held[i] = held[i];
    for (int i = t; i < C * kKcAcc; i += 256) s_acc[i] = 0.0;
    for (int i = t; i < (NP - n12) * RS; i += 256) s_Y[(size_t)n12 * RS + i] = 0.0;   // the padding rows: zero once, no item writes them
  }
  kpcam_d4 tile[TQ];
#pragma unroll
  for (int q = 0; q < TQ; ++q) tile[q] = kpcam_d4{0.0, 0.0, 0.0, 0.0};
  double r[3] = {0.0, 0.0, 0.0};   // this lane's cost, present scalars, max |g_p|
  const size_t nchunks = (npts + kKcChunk - 1) / kKcChunk;
  for (size_t chunk = blockIdx.x; chunk < nchunks; chunk += gridDim.x) {
    const size_t p0 = chunk * kKcChunk;
    __syncthreads();   // the previous chunk's last group is done with s_pt (and, the first time, the staging above is visible)
    {
      const size_t p = p0 + t;
      double* sp = s_pt + t * kKcPt;
      KbFactor f;
#pragma unroll
      for (int i = 0; i < 6; ++i) f.L[i] = 0.0;
      f.d[0] = f.d[1] = f.d[2] = 0.0;
      double z[3] = {0.0, 0.0, 0.0};
      bool usable = false;
      if (p < npts && status[p] == KB_USED) {
        const double X[3] = {pts[3 * p], pts[3 * p + 1], pts[3 * p + 2]};
        KpDetections<WEIGHTED> observation(uvs, sw, npts, p);
        KbPoint pt;
        kpba_point<LOSS>(s_cam, C, observation, X, fs2, inv_fs2, nullptr, pt);
        r[0] += pt.cost;
        r[1] += 2.0 * pt.views;
        r[2] = fmax(r[2], fmax(fabs(pt.g[0]), fmax(fabs(pt.g[1]), fabs(pt.g[2]))));
        usable = kpba_factor(pt.H, lam, f);
        if (usable) kpba_fwd(f, pt.g, z);
      }
#pragma unroll
      for (int i = 0; i < 6; ++i) sp[i] = f.L[i];
#pragma unroll
      for (int i = 0; i < 3; ++i) { sp[6 + i] = f.d[i]; sp[9 + i] = z[i]; }
      sp[12] = usable ? 1.0 : 0.0;
    }
    __syncthreads();
    const int in_chunk = npts - p0 < (size_t)kKcChunk ? (int)(npts - p0) : kKcChunk;
    for (int sub = 0; sub * G < in_chunk; ++sub) {
      kpcam_items<LOSS, WEIGHTED, 0>(uvs, pts, sw, npts, p0, sub, G, C, RS, s_cam, s_held, s_pt, s_acc, s_Y, fs2, inv_fs2);
      kpcam_items<LOSS, WEIGHTED, 1>(uvs, pts, sw, npts, p0, sub, G, C, RS, s_cam, s_held, s_pt, s_acc, s_Y, fs2, inv_fs2);
      __syncthreads();
#pragma unroll
      for (int q = 0; q < TQ; ++q) {
        const int id = wave + 4 * q;   // wave-uniform
        if (id < ntiles) {
          int ti = 0;
          while ((ti + 1) * (ti + 2) / 2 <= id) ++ti;
          const int tj = id - ti * (ti + 1) / 2;
          const double* ya = s_Y + (size_t)(16 * ti + (lane & 15)) * RS + (lane >> 4);
          const double* yb = s_Y + (size_t)(16 * tj + (lane & 15)) * RS + (lane >> 4);
          kpcam_d4 acc = tile[q];
          for (int ks = 0; ks < 3 * G / 4; ++ks) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(ya[4 * ks], yb[4 * ks], acc, 0, 0, 0);
          tile[q] = acc;
        }
      }
      __syncthreads();   // the panel is free for the next group
    }
  }
  __syncthreads();
  double* out = part + (size_t)blockIdx.x * ((size_t)NP * NP + (size_t)C * kKcAcc + 4);
#pragma unroll
  for (int q = 0; q < TQ; ++q) {
    const int id = wave + 4 * q;
    if (id < ntiles) {
      int ti = 0;
      while ((ti + 1) * (ti + 2) / 2 <= id) ++ti;
      const int tj = id - ti * (ti + 1) / 2;
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) out[(size_t)(16 * ti + 4 * reg + (lane >> 4)) * NP + 16 * tj + (lane & 15)] = tile[q][reg];
    }
  }
  for (int i = t; i < C * kKcAcc; i += 256) out[(size_t)NP * NP + i] = s_acc[i];
  const bool is_max[3] = {false, false, true};
  block_tree<3>(s_r, r, is_max);
  if (t < 4) out[(size_t)NP * NP + (size_t)C * kKcAcc + t] = t < 3 ? s_r[t][0] : 0.0;
}

int launch_kpcam_reduce(hipStream_t st, int loss, const double* uvs, const double* pts, const int* status, size_t npts, const TcCam* cams, const int* held, int C, double f_scale, double lam, int G,
                        double* part, double* sys, const double* sw) {
  if (C < 2 || C > kKcMaxCams || (G != 16 && G != 32 && G != 64) || npts == 0 || npts > ((size_t)1 << 38)) return 1;
  const size_t lds = kpcam_reduce_lds(C, G);
  const int nwg = kpba_groups(npts), NP = (kKcRows * C + 15) / 16 * 16;
  const double2* uv = reinterpret_cast<const double2*>(uvs);
  const int NT = NP / 16, ntiles = NT * (NT + 1) / 2;   // tiles per wavefront: 3 up to 10 tiles (5 cameras), 12 up to 45
  const int rc = with_weights(sw, [&](auto W) {
    return with_loss(loss, [&](auto L) {
      return with_int<3, 12>(ntiles <= 12 ? 3 : 12, [&](auto TQ) {
        return launch_with_lds(k_kpcam_reduce<decltype(L)::value, decltype(TQ)::value, decltype(W)::value>, dim3((unsigned)nwg), lds, st, uv, pts, status, npts, cams, held, C, f_scale, lam, G, part, sw);
      });
    });
  });
  if (rc) return rc;
  launch_kpba_finish_sized(st, part, nwg, NP, C * kKcAcc, sys);
  return 0;
}

// ---------------------------------------------------------------- k_kpcam_step
// cams: the current table and, behind it, the trial table (2 C entries).  part4 per workgroup: trial cost, sum dX^2, 0, sum X^2.
template <int LOSS, bool WEIGHTED>
__global__ __launch_bounds__(256) void k_kpcam_step(const double2* __restrict__ uvs, const double* __restrict__ pts, double* __restrict__ trial, const int* __restrict__ status, size_t npts,
                                                    const TcCam* __restrict__ cams, const double* __restrict__ dtheta, int C, double f_scale, double lam, double* __restrict__ part4,
                                                    const double* __restrict__ sw) {
  __shared__ TcCam s_cam[2 * kKcMaxCams];
  __shared__ double s_dth[kKcRows * kKcMaxCams];
  __shared__ double s_r[3][256];
  const int t = threadIdx.x;
  {
    const double* src = reinterpret_cast<const double*>(cams);
    double* dst = reinterpret_cast<double*>(s_cam);
    for (int i = t; i < 60 * C; i += 256) dst[i] = src[i];
    for (int i = t; i < kKcRows * C; i += 256) s_dth[i] = dtheta[i];
    __syncthreads();
  }
  const double fs2 = f_scale * f_scale, inv_fs2 = 1.0 / fs2;
  double r[3] = {0.0, 0.0, 0.0};   // trial cost, sum dX^2, sum X^2
  const size_t nchunks = (npts + kKcChunk - 1) / kKcChunk;
  for (size_t chunk = blockIdx.x; chunk < nchunks; chunk += gridDim.x) {
    const size_t p = chunk * kKcChunk + t;
    if (p >= npts) continue;
    const double X[3] = {pts[3 * p], pts[3 * p + 1], pts[3 * p + 2]};
    double Xt[3] = {X[0], X[1], X[2]};
    if (status[p] == KB_USED) {
      KpDetections<WEIGHTED> observation(uvs, sw, npts, p);
      KbPoint pt;
      kpcam_point<LOSS>(s_cam, C, observation, X, fs2, inv_fs2, s_dth, pt);
      KbFactor f;
      double dX[3] = {0.0, 0.0, 0.0};
      if (kpba_factor(pt.H, lam, f)) kpba_point_step(f, pt.g, pt.q, dX);
#pragma unroll
      for (int j = 0; j < 3; ++j) {
        Xt[j] = X[j] + dX[j];
        r[1] = fma(dX[j], dX[j], r[1]);
        r[2] = fma(X[j], X[j], r[2]);
      }
      KbPoint tr;
      kpcam_point<LOSS>(s_cam + C, C, observation, Xt, fs2, inv_fs2, nullptr, tr);
      r[0] += tr.cost;
    }
#pragma unroll
    for (int j = 0; j < 3; ++j) trial[3 * p + j] = Xt[j];   // (a point that takes no part keeps its value in both buffers)
  }
  const bool is_max[3] = {false, false, false};   // sums alone
  block_tree<3>(s_r, r, is_max);
  if (t < 4) part4[4 * (size_t)blockIdx.x + t] = t == 0 ? s_r[0][0] : (t == 1 ? s_r[1][0] : (t == 3 ? s_r[2][0] : 0.0));
}

int launch_kpcam_step(hipStream_t st, int loss, const double* uvs, const double* pts, double* trial, const int* status, size_t npts, const TcCam* cams2, const double* dtheta, int C, double f_scale,
                      double lam, double* part4, double* out4, const double* sw) {
  if (C < 2 || C > kKcMaxCams || npts == 0 || npts > ((size_t)1 << 38)) return 1;
  const int nwg = kpba_groups(npts);
  const double2* uv = reinterpret_cast<const double2*>(uvs);
  if (with_weights(sw, [&](auto W) {
        return with_loss(loss, [&](auto L) {
          k_kpcam_step<decltype(L)::value, decltype(W)::value><<<dim3((unsigned)nwg), dim3(256), 0, st>>>(uv, pts, trial, status, npts, cams2, dtheta, C, f_scale, lam, part4, sw);
          return 0;
        });
      }))
    return 1;
  launch_kpba_finish_sized(st, part4, nwg, 0, 0, out4);
  return 0;
}

}  // namespace mcba
