// mcba_tricov.hip -- triangulation uncertainty: the covariance of every triangulated point, from the detection noise
// (sigma2 H^-1) and from the uncertainty of the cameras (G Sigma_cc G^T).  Per-lane arithmetic: mcba_tricov_math.h (host-checked).
//   k_tricov_point  lane = point: H^-1 (unscaled, packed), views, status; per-workgroup partials of (sum w f^2, present scalars, points of status 1,
//                   degenerate points), summed in a fixed order by k_tricov_final, which also fixes sigma2
//   k_tricov_scale  det6 = sigma2 H^-1 -- the whole call when no camera covariance is given
//   k_tricov_cal    G points per workgroup: their rows of G into LDS, Z = G Sigma_cc on v_mfma_f64_16x16x4_f64, the 3 x 3 diagonal blocks of Z G^T
#include <hip/hip_runtime.h>

#include <algorithm>

#include "mcba_device.h"
#include "mcba_kernels.h"
#include "mcba_quadform.h"
#include "mcba_tricov_math.h"

// (in both compilation passes: the weighted functor is taken for weighted, the plain one for unweighted)
static_assert(mcba::KpWeighted<mcba::KpDetections<true>>::value && !mcba::KpWeighted<mcba::KpDetections<false>>::value, "the observation functors select the weighted arithmetic");

namespace mcba {

// ---------------------------------------------------------------- k_tricov_point
// The camera table is staged in LDS as k_tri_refine stages it (the KpCam part of every entry).  No lane leaves before the workgroup's sums.
// WEIGHTED: sw, the (C, P) plane of sqrt(weight), is read beside each detection; views and the present scalars count the detections with sw > 0.
template <int LOSS, bool WEIGHTED>
__global__ __launch_bounds__(256) void k_tricov_point(const double2* __restrict__ uvs, const double* __restrict__ pts, size_t npts, const TcCam* __restrict__ cams, int C, double f_scale,
                                                      double* __restrict__ hinv, int* __restrict__ views, int* __restrict__ status, double* __restrict__ part,
                                                      const double* __restrict__ sw) {
  __shared__ KpCam s_cam[kKpMaxCams];
  __shared__ double s_r[4][256];
  stage_cams(s_cam, cams, C);
  const size_t p = (size_t)blockIdx.x * 256 + threadIdx.x;
  double r[4] = {0.0, 0.0, 0.0, 0.0};
  if (p < npts) {
    const double X[3] = {pts[3 * p], pts[3 * p + 1], pts[3 * p + 2]};
    KpDetections<WEIGHTED> observation(uvs, sw, npts, p);
    double Hi[6], wss;
    int nv;
    const int st = tricov_point<LOSS>(s_cam, C, observation, X, f_scale, Hi, nv, wss);
#pragma unroll
    for (int i = 0; i < 6; ++i) hinv[6 * p + i] = Hi[i];
    views[p] = nv;
    status[p] = st;
    if (st == TC_OK) { r[0] = wss; r[1] = 2.0 * nv; r[2] = 1.0; }
    if (st == TC_DEGENERATE) r[3] = 1.0;
  }
  const bool is_max[4] = {false, false, false, false};   // sums alone
  block_tree<4>(s_r, r, is_max);
  if (threadIdx.x < 4) part[4 * (size_t)blockIdx.x + threadIdx.x] = s_r[threadIdx.x][0];
}

// the partials in order: info[0] = sigma2, [1] = m, [2] = 3 P_u, [3] = points of status -1, [4] = degenerate points
__global__ __launch_bounds__(256) void k_tricov_final(const double* __restrict__ part, int nblocks, size_t npts, double sigma2_in, double* __restrict__ info) {
  __shared__ double s_r[4][256];
  double r[4] = {0.0, 0.0, 0.0, 0.0};
  for (int i = threadIdx.x; i < nblocks; i += 256) {
#pragma unroll
    for (int k = 0; k < 4; ++k) r[k] += part[4 * (size_t)i + k];
  }
  const bool is_max[4] = {false, false, false, false};   // sums alone
  block_tree<4>(s_r, r, is_max);
  if (threadIdx.x == 0) {
    const double wss = s_r[0][0], m = s_r[1][0], nfree = 3.0 * s_r[2][0], ndeg = s_r[3][0];
    info[0] = sigma2_in == sigma2_in ? sigma2_in : tricov_sigma2(wss, m, nfree);
    info[1] = m;
    info[2] = nfree;
    info[3] = (double)npts - s_r[2][0] - ndeg;
    info[4] = ndeg;
  }
}

int tricov_point_blocks(size_t npts) { return (int)((npts + 255) / 256); }

int launch_tricov_point(hipStream_t st, int loss, const double* uvs, const double* pts, size_t npts, const TcCam* cams, int C, double f_scale, double sigma2_in, double* hinv, int* views, int* status,
                        double* part, double* info, const double* sw) {
  if (C < 2 || C > kKpMaxCams || npts == 0 || npts > ((size_t)1 << 38)) return 1;
  const int nb = tricov_point_blocks(npts);
  const double2* uv = reinterpret_cast<const double2*>(uvs);
  if (with_weights(sw, [&](auto W) {
        return with_loss(loss, [&](auto L) {
          k_tricov_point<decltype(L)::value, decltype(W)::value><<<dim3((unsigned)nb), dim3(256), 0, st>>>(uv, pts, npts, cams, C, f_scale, hinv, views, status, part, sw);
          return 0;
        });
      }))
    return 1;
  k_tricov_final<<<dim3(1), dim3(256), 0, st>>>(part, nb, npts, sigma2_in, info);
  return 0;
}

// ---------------------------------------------------------------- k_tricov_scale
__global__ __launch_bounds__(256) void k_tricov_scale(const double* __restrict__ hinv, const int* __restrict__ status, const double* __restrict__ info, size_t count, double* __restrict__ det6) {
  const double sigma2 = info[0];
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < count; i += (size_t)gridDim.x * 256) det6[i] = tricov_det_entry(hinv[i], sigma2, status[i / 6] == TC_OK);
}

void launch_tricov_scale(hipStream_t st, const double* hinv, const int* status, const double* info, size_t npts, double* det6) {
  const size_t count = 6 * npts;
  k_tricov_scale<<<dim3((unsigned)std::min<size_t>((count + 255) / 256, 8192)), dim3(256), 0, st>>>(hinv, status, info, count, det6);
}

// ---------------------------------------------------------------- k_tricov_cal
// The plan of k_cov_frames (mcba_cov.hip) with 3 rows per item.  One workgroup = G consecutive points, 256 threads, R = 3 G rows of the stacked
// G matrices (row 3 g + k = row k of point g), RT = ceil(R / 16) row tiles, n = 12 C, KP = ceil(n / 32) 32.
//   1. the first 6 G threads: H^-1 of the group's points (zero unless the status is TC_OK: such a point's rows are zero)
//   2. item (camera c, point g), points fastest: G_c of the point -> s_Y[3 g + k][12 c + j]; zero for a camera that does not see the point;
//      columns n .. KP are zero
//   3. the diagonal blocks of G Sigma_cc G^T: diag_blocks (mcba_quadform.h), thread (g, k <= l) gets entry (k, l) of point g
//   4. cal6 and det6 = sigma2 H^-1 through LDS in runs of consecutive doubles; points >= P write nothing.
static size_t tricov_cal_lds(int n, int G) {
  const int KP = (n + 31) / 32 * 32, R = 3 * G;
  return ((size_t)R * (KP + 2) + stage_doubles(R) + (size_t)G * 6 * 3) * sizeof(double);
}

// WEIGHTED: item (camera, point) also reads element (c, p) of sw, the plane of sqrt(weight), and is zero unless it is > 0.  The operand costs
// four registers; the linear loss with three row tiles sits at 128 without it, the last count with four wavefronts per SIMD, so that one
// instantiation asks for them (the second launch bound) and gets 108 without scratch; every other one stays in the class of its unweighted twin.
template <int LOSS, int RT, bool WEIGHTED>
__global__ __launch_bounds__(256, (WEIGHTED && LOSS == LOSS_LINEAR && RT == 3) ? 4 : 1) void k_tricov_cal(const double2* __restrict__ uvs, const double* __restrict__ pts, size_t npts, const TcCam* __restrict__ cams, int C, double f_scale,
                                                    const double* __restrict__ hinv, const int* __restrict__ status, const double* __restrict__ Sig, int ld, const double* __restrict__ info,
                                                    double* __restrict__ det6, double* __restrict__ cal6, int G, int KP, const double* __restrict__ sw) {
  extern __shared__ __align__(16) double lds[];
  const int t = threadIdx.x;
  const int n = 12 * C, R = 3 * G, RS = KP + 2;
  double* s_Y = lds;                                   // [R][RS]
  double* s_P = s_Y + (size_t)R * RS;                  // the staging buffer of diag_blocks
  double* s_Hi = s_P + stage_doubles(R);               // [G][6]
  double* s_oc = s_Hi + G * 6;                         // [G][6] calibration term
  double* s_od = s_oc + G * 6;                         // [G][6] detection term
  const size_t p0 = (size_t)blockIdx.x * G;
  const int ng = npts - p0 < (size_t)G ? (int)(npts - p0) : G;
  const double fs2 = f_scale * f_scale, inv_fs2 = 1.0 / fs2;

  const bool own = t < G * 6;
  int og = 0, ok_ = 0, ol = 0;
  bool good = false;   // this thread's point is inside P and TC_OK
  if (own) {
    og = t / 6;
    tricov_tri3_pair(t % 6, ok_, ol);
    good = og < ng && status[p0 + og] == TC_OK;
    s_Hi[t] = good ? hinv[6 * p0 + t] : 0.0;
  }
  __syncthreads();
  for (int it = t; it < C * G; it += 256) {
    const int g = it % G, c = it / G;
    double gr[36];
#pragma unroll
    for (int k = 0; k < 36; ++k) gr[k] = 0.0;
    if (g < ng && status[p0 + g] == TC_OK) {
      const size_t p = p0 + g;
      const double2 o = uvs[(size_t)c * npts + p];
      const double s = WEIGHTED ? sw[(size_t)c * npts + p] : 1.0;
      if (o.x == o.x && o.y == o.y && s > 0.0) {
        const double X[3] = {pts[3 * p], pts[3 * p + 1], pts[3 * p + 2]};
        tricov_g_block_w<LOSS, WEIGHTED>(cams[c], X, o.x, o.y, s, s_Hi + 6 * g, fs2, inv_fs2, gr);
      }
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) {
#pragma unroll
      for (int j = 0; j < 12; ++j) s_Y[(size_t)(3 * g + k) * RS + 12 * c + j] = gr[12 * k + j];
    }
  }
  for (int it = t; it < R * (KP - n); it += 256) s_Y[(size_t)(it / (KP - n)) * RS + n + it % (KP - n)] = 0.0;
  // (the first barrier of diag_blocks orders these stores before the first read)

  const double zy = diag_blocks<RT, 3>(s_Y, s_P, Sig, ld, R, KP, own, og, ok_, ol);
  if (own) {
    s_oc[t] = tricov_cal_entry(zy, good);
    s_od[t] = tricov_det_entry(s_Hi[t], info[0], good);
  }
  __syncthreads();
  for (int i = t; i < ng * 6; i += 256) {
    cal6[6 * p0 + i] = s_oc[i];
    det6[6 * p0 + i] = s_od[i];
  }
}

// G points per workgroup: 16 (three row tiles) if its LDS fits, else 10 (two), else 5 (one: fits at 64 cameras); force_g (5, 10 or 16, tests)
// overrides when it fits
int tricov_group(int n, int lds_limit, int force_g) {
  if ((force_g == 5 || force_g == 10 || force_g == 16) && tricov_cal_lds(n, force_g) <= (size_t)lds_limit) return force_g;
  if (tricov_cal_lds(n, 16) <= (size_t)lds_limit) return 16;
  if (tricov_cal_lds(n, 10) <= (size_t)lds_limit) return 10;
  if (tricov_cal_lds(n, 5) <= (size_t)lds_limit) return 5;
  return 0;
}

int launch_tricov_cal(hipStream_t st, int loss, const double* uvs, const double* pts, size_t npts, const TcCam* cams, int C, double f_scale, const double* hinv, const int* status, const double* Sig,
                      int ld, const double* info, double* det6, double* cal6, int G, const double* sw) {
  const int n = 12 * C, KP = (n + 31) / 32 * 32;
  if (C < 2 || C > kKpMaxCams || (G != 5 && G != 10 && G != 16) || KP > ld || ld % 64 != 0 || npts == 0 || (npts + G - 1) / G > 0x7fffffffu) return 1;
  const size_t lds = tricov_cal_lds(n, G);
  const double2* uv = reinterpret_cast<const double2*>(uvs);
  const dim3 grid((unsigned)((npts + G - 1) / G));
  return with_weights(sw, [&](auto W) {
    return with_loss(loss, [&](auto L) {
      return with_int<1, 2, 3>(G == 16 ? 3 : (G == 10 ? 2 : 1), [&](auto RT) {
        return launch_with_lds(k_tricov_cal<decltype(L)::value, decltype(RT)::value, decltype(W)::value>, grid, lds, st, uv, pts, npts, cams, C, f_scale, hinv, status, Sig, ld, info, det6, cal6,
                               G, KP, sw);
      });
    });
  });
}

}  // namespace mcba
