// mcba_kpba_tiled.hip -- the tiled Schur reduction of the extrinsics refinement: the system of mcba_kpba.hip's k_kpba_reduce,
// in the same layout, for 2 to 64 cameras.  S = U + lam diag U - sum_p Y_p Y_p^T is entry-wise, so the cameras are cut into bands of kKtBand = 16
// (96 rows, six 16-row tiles) and the lower triangle of Y Y^T into band pairs (I >= J), each a workgroup's own.
//   k_kpba_factors        lane = point, once per evaluation: phase 1 of k_kpba_reduce -- H_p, g_p, the factor L_p of the damped Jacobi-scaled block,
//                         z_p = L^-1 D g_p, the usable flag -> fac (P, 13); cost, present scalars and max |g_p| -> the trailing scalars of partial x
//   k_kpba_reduce_tiled   workgroup (x, pair): x walks chunks of 256 points with the grid stride (the factors of a chunk: fac -> LDS).  Per group of
//                         G = 16 points: item (camera of band I or J, point) writes Y_cp into the (2 x 96) x (3 G) panel; the diagonal pair (I, I)
//                         also sums U_c, g_c, Y_cp z_p of its band's cameras by k_kpba_reduce's butterfly.  Then the tiles of the pair alone on
//                         v_mfma_f64_16x16x4_f64 -- 6 x 6 for I > J, the 21 on or below the diagonal for I = J --, each owned by one wavefront (at
//                         most 9 per wavefront), in registers over all the workgroup's chunks, written once into partial x.
// k_kpba_finish (mcba_kpba.hip) sums the partials in order, as for the resident reduction.  Operand addressing, the odd row stride and the ownership
// rule are k_kpba_reduce's.  No atomics: every sum has one order; every tile, camera sum and scalar of partial x has exactly one writer.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "mcba_device.h"
#include "mcba_kernels.h"
#include "mcba_kpba_math.h"

namespace mcba {

typedef double kpba_d4 __attribute__((ext_vector_type(4)));

constexpr int kKtChunk = 256;                          // points of one staging of factors (k_kpba_reduce's chunk)
constexpr int kKtPt = 13;                              // per point: L (6) | d (3) | z (3) | usable (1)
constexpr int kKtRows = 6 * kKtBand;                   // rows of a band: 96, six tiles
constexpr int kKtRS = 3 * kKtGroup + 1;                // row stride of the panel, odd: the 16 rows an operand reads fall into 16 distinct bank pairs
constexpr int kKtTQ = 9;                               // tiles per wavefront: 36 of an off-diagonal pair over 4 wavefronts
constexpr int kKtCapCams = 24, kKtCapGroups = 512;     // the resident path's largest allocation of partials: 512 at 24 cameras
static_assert(kKtBand * kKtGroup == 256 && kKtRows % 16 == 0 && (kKtRS & 1) && 4 * kKtTQ >= (kKtRows / 16) * (kKtRows / 16), "the band, the group and the tile budget fit each other");

// dynamic LDS of k_kpba_reduce_tiled: s_pt [256][13] | s_acc [16][33] | s_Y [2][96][49] doubles (103.6 KiB), beside 7.6 KiB static (s_cam, s_held)
size_t kpba_tiled_lds() { return ((size_t)kKtChunk * kKtPt + (size_t)kKtBand * kKbAcc + (size_t)2 * kKtRows * kKtRS) * sizeof(double); }
int kpba_tiled_pairs(int C) {
  const int nb = (C + kKtBand - 1) / kKtBand;
  return nb * (nb + 1) / 2;
}
// partial systems at most: the largest power of two with which all of them take no more than kKtCapGroups partials of kKtCapCams cameras do
int kpba_tiled_groups(int C, size_t npts) {
  const size_t room = (size_t)kKtCapGroups * kpba_partial_size(kKtCapCams) / kpba_partial_size(C);
  int cap = 1;
  while ((size_t)2 * cap <= std::min<size_t>(room, kKtCapGroups)) cap *= 2;
  return (int)std::min<size_t>((npts + kKtChunk - 1) / kKtChunk, (size_t)cap);
}

// ---------------------------------------------------------------- k_kpba_factors
template <int LOSS, bool WEIGHTED>
__global__ __launch_bounds__(256) void k_kpba_factors(const double2* __restrict__ uvs, const double* __restrict__ pts, const int* __restrict__ status, size_t npts, const TcCam* __restrict__ cams, int C,
                                                      double f_scale, double lam, double* __restrict__ fac, double* __restrict__ part, size_t PS, const double* __restrict__ sw) {
  __shared__ TcCam s_cam[kKtMaxCams];
  __shared__ double s_r[3][256];
  const int t = threadIdx.x;
  {
    const double* src = reinterpret_cast<const double*>(cams);
    double* dst = reinterpret_cast<double*>(s_cam);
    for (int i = t; i < 30 * C; i += 256) dst[i] = src[i];
    __syncthreads();
  }
  const double fs2 = f_scale * f_scale, inv_fs2 = 1.0 / fs2;
  double r[3] = {0.0, 0.0, 0.0};   // this lane's cost, present scalars, max |g_p|
  const size_t nchunks = (npts + kKtChunk - 1) / kKtChunk;
  for (size_t chunk = blockIdx.x; chunk < nchunks; chunk += gridDim.x) {
    const size_t p = chunk * kKtChunk + t;
    if (p >= npts) continue;
    KbFactor f;
#pragma unroll
    for (int i = 0; i < 6; ++i) f.L[i] = 0.0;
    f.d[0] = f.d[1] = f.d[2] = 0.0;
    double z[3] = {0.0, 0.0, 0.0};
    bool usable = false;
    if (status[p] == KB_USED) {
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
    double* sp = fac + p * kKtPt;
#pragma unroll
    for (int i = 0; i < 6; ++i) sp[i] = f.L[i];
#pragma unroll
    for (int i = 0; i < 3; ++i) { sp[6 + i] = f.d[i]; sp[9 + i] = z[i]; }
    sp[12] = usable ? 1.0 : 0.0;
  }
  const bool is_max[3] = {false, false, true};
  block_tree<3>(s_r, r, is_max);
  if (t < 4) part[(size_t)blockIdx.x * PS + PS - 4 + t] = t < 3 ? s_r[t][0] : 0.0;
}

// ---------------------------------------------------------------- k_kpba_reduce_tiled
// blockIdx.y = I (I + 1) / 2 + J.  Panel rows: slot 0 = band I (local row 6 k + i of its camera k), slot 1 = band J when I > J (then a full band).
// Rows of cameras past C are zeroed once and written by no item: with them the padding rows of the system are zero.
template <int LOSS, bool WEIGHTED>
__global__ __launch_bounds__(256) void k_kpba_reduce_tiled(const double2* __restrict__ uvs, const double* __restrict__ pts, size_t npts, const TcCam* __restrict__ cams, const int* __restrict__ held,
                                                           int C, double f_scale, const double* __restrict__ fac, double* __restrict__ part, const double* __restrict__ sw) {
  extern __shared__ __align__(16) double lds[];
  __shared__ TcCam s_cam[2 * kKtBand];
  __shared__ int s_held[2 * kKtBand];
  const int t = threadIdx.x, lane = t & 63;
  const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
  int I = 0;
  while ((I + 1) * (I + 2) / 2 <= (int)blockIdx.y) ++I;
  const int J = (int)blockIdx.y - I * (I + 1) / 2;
  const bool diag = I == J;
  const int NP = (6 * C + 15) / 16 * 16, NT = NP / 16;
  const int nI = min(kKtBand, C - kKtBand * I), ncam = diag ? nI : nI + kKtBand;   // (J < I: band J is a full one)
  const int ntI = min(kKtRows / 16, NT - (kKtRows / 16) * I);                      // row tiles of band I
  const int ntiles = diag ? ntI * (ntI + 1) / 2 : ntI * (kKtRows / 16);
  double* s_pt = lds;                                   // [256][13]
  double* s_acc = s_pt + kKtChunk * kKtPt;              // [16][33]: the cameras of band I (the diagonal pair alone)
  double* s_Y = s_acc + kKtBand * kKbAcc;               // [2][96][RS]
  const double fs2 = f_scale * f_scale, inv_fs2 = 1.0 / fs2;
  {
    double* dst = reinterpret_cast<double*>(s_cam);
    for (int i = t; i < 30 * ncam; i += 256) {
      const int k = i / 30, c = k < nI ? kKtBand * I + k : kKtBand * J + (k - nI);
      dst[i] = reinterpret_cast<const double*>(cams)[30 * c + i % 30];
    }
    for (int k = t; k < ncam; k += 256) s_held[k] = held[k < nI ? kKtBand * I + k : kKtBand * J + (k - nI)];
    for (int i = t; i < kKtBand * kKbAcc; i += 256) s_acc[i] = 0.0;
    for (int i = t; i < (kKtRows - 6 * nI) * kKtRS; i += 256) s_Y[(size_t)6 * nI * kKtRS + i] = 0.0;   // the rows of band I past its cameras
  }
  kpba_d4 tile[kKtTQ];
#pragma unroll
  for (int q = 0; q < kKtTQ; ++q) tile[q] = kpba_d4{0.0, 0.0, 0.0, 0.0};
  const size_t nchunks = (npts + kKtChunk - 1) / kKtChunk;
  for (size_t chunk = blockIdx.x; chunk < nchunks; chunk += gridDim.x) {
    const size_t p0 = chunk * kKtChunk;
    const int in_chunk = npts - p0 < (size_t)kKtChunk ? (int)(npts - p0) : kKtChunk;
    __syncthreads();   // the previous chunk's last group is done with s_pt (and, the first time, the staging above is visible)
    for (int i = t; i < kKtChunk * kKtPt; i += 256) s_pt[i] = i < in_chunk * kKtPt ? fac[p0 * kKtPt + i] : 0.0;   // (a point past P is not usable)
    __syncthreads();
    for (int sub = 0; sub * kKtGroup < in_chunk; ++sub) {
      for (int it = t; it < ncam * kKtGroup; it += 256) {
        const int g = it % kKtGroup, k = it / kKtGroup, pl = sub * kKtGroup + g;
        const int c = k < nI ? kKtBand * I + k : kKtBand * J + (k - nI);
        const int row0 = k < nI ? 6 * k : kKtRows + 6 * (k - nI);
        const double* sp = s_pt + pl * kKtPt;
        double Y[18], a[kKbAcc];
#pragma unroll
        for (int i = 0; i < 18; ++i) Y[i] = 0.0;
#pragma unroll
        for (int i = 0; i < kKbAcc; ++i) a[i] = 0.0;
        if (sp[12] != 0.0) {
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
            kpba_item_w<LOSS, WEIGHTED>(s_cam[k], X, o.x, o.y, sq, fs2, inv_fs2, f, sp + 9, s_held[k], Y, a);
          }
        }
#pragma unroll
        for (int i = 0; i < 6; ++i) {
#pragma unroll
          for (int j = 0; j < 3; ++j) s_Y[(size_t)(row0 + i) * kKtRS + 3 * g + j] = Y[3 * i + j];
        }
        if (diag) {   // (uniform over the workgroup) the camera's sums over the group's 16 points: a group's lanes are all here or all absent
          for (int m = kKtGroup >> 1; m > 0; m >>= 1) {
#pragma unroll
            for (int i = 0; i < kKbAcc; ++i) a[i] += __shfl_xor(a[i], m);
          }
          if (g == 0) {
#pragma unroll
            for (int i = 0; i < kKbAcc; ++i) s_acc[k * kKbAcc + i] += a[i];   // (camera k is this lane's alone until the next barrier)
          }
        }
      }
      __syncthreads();
#pragma unroll
      for (int q = 0; q < kKtTQ; ++q) {
        const int id = wave + 4 * q;   // wave-uniform
        if (id < ntiles) {
          int ti, tj;
          if (diag) {
            ti = 0;
            while ((ti + 1) * (ti + 2) / 2 <= id) ++ti;
            tj = id - ti * (ti + 1) / 2;
          } else {
            ti = id / (kKtRows / 16);
            tj = id % (kKtRows / 16);
          }
          const double* ya = s_Y + (size_t)(16 * ti + (lane & 15)) * kKtRS + (lane >> 4);
          const double* yb = s_Y + (size_t)((diag ? 0 : kKtRows) + 16 * tj + (lane & 15)) * kKtRS + (lane >> 4);
          kpba_d4 acc = tile[q];
#pragma unroll
          for (int ks = 0; ks < 3 * kKtGroup / 4; ++ks) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(ya[4 * ks], yb[4 * ks], acc, 0, 0, 0);
          tile[q] = acc;
        }
      }
      __syncthreads();   // the panel is free for the next group
    }
  }
  __syncthreads();
  double* out = part + (size_t)blockIdx.x * ((size_t)NP * NP + (size_t)C * kKbAcc + 4);
#pragma unroll
  for (int q = 0; q < kKtTQ; ++q) {
    const int id = wave + 4 * q;
    if (id < ntiles) {
      int ti, tj;
      if (diag) {
        ti = 0;
        while ((ti + 1) * (ti + 2) / 2 <= id) ++ti;
        tj = id - ti * (ti + 1) / 2;
      } else {
        ti = id / (kKtRows / 16);
        tj = id % (kKtRows / 16);
      }
      const size_t row = (size_t)kKtRows * I + 16 * ti + (lane >> 4), col = (size_t)kKtRows * J + 16 * tj + (lane & 15);   // (row < NP by ntI, col < NP as J <= I)
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) out[(row + 4 * reg) * NP + col] = tile[q][reg];
    }
  }
  if (diag)
    for (int i = t; i < nI * kKbAcc; i += 256) out[(size_t)NP * NP + (size_t)kKtBand * I * kKbAcc + i] = s_acc[i];
}

int launch_kpba_reduce_tiled(hipStream_t st, int loss, const double* uvs, const double* pts, const int* status, size_t npts, const TcCam* cams, const int* held, int C, double f_scale, double lam,
                             double* fac, double* part, double* sys, const double* sw) {
  if (C < 2 || C > kKtMaxCams || npts == 0 || npts > ((size_t)1 << 38)) return 1;
  const int nx = kpba_tiled_groups(C, npts), npairs = kpba_tiled_pairs(C);
  const size_t PS = kpba_partial_size(C);
  const double2* uv = reinterpret_cast<const double2*>(uvs);
  const int rc = with_weights(sw, [&](auto W) {
    return with_loss(loss, [&](auto L) {
      k_kpba_factors<decltype(L)::value, decltype(W)::value><<<dim3((unsigned)nx), dim3(256), 0, st>>>(uv, pts, status, npts, cams, C, f_scale, lam, fac, part, PS, sw);
      return launch_with_lds(k_kpba_reduce_tiled<decltype(L)::value, decltype(W)::value>, dim3((unsigned)nx, (unsigned)npairs), kpba_tiled_lds(), st, uv, pts, npts, cams, held, C, f_scale, fac, part, sw);
    });
  });
  if (rc) return rc;
  launch_kpba_finish(st, part, nx, C, sys);
  return 0;
}

}  // namespace mcba
