// mcba_cov.hip -- calibration uncertainty: the covariance of the cameras and of every frame pose from what one
// linearisation leaves on the device -- the records W_cf, V_cf (rec), the frame factors L_f (fbuf), the undamped Schur complement S0 (red).
// Per-lane arithmetic: mcba_cov_math.h (host-checked).
//   k_cov_wss     sum w f^2 and the number of present scalars from the residual vector (NaN = missing): two launches, fixed order
//   k_cov_check   per frame: is V_f = sum_c V_cf positive definite (0), is the frame without data (1), or neither (2)
//   k_cov_cam     S0 -> Sigma_cc, three launches (no waiting between workgroups): scale + factor (one workgroup), M = L^-1 (a thread per
//                 column), Sigma_cc = sigma2 D^-1/2 M^T M D^-1/2 (a thread per entry) into a zero-padded ld x ld buffer, ld = ceil(n / 64) 64
//   k_cov_frames  Sigma_ff = sigma2 V_f^-1 + Y_f Sigma_cc Y_f^T for G frames per workgroup, Z = Y Sigma_cc on v_mfma_f64_16x16x4_f64
#include <hip/hip_runtime.h>

#include <algorithm>

#include "mcba_cov_math.h"
#include "mcba_device.h"
#include "mcba_kernels.h"
#include "mcba_quadform.h"

namespace mcba {

// ---------------------------------------------------------------- k_cov_wss
constexpr int kCovWssBlocks = 1024;

template <int LOSS>
__global__ __launch_bounds__(256) void k_cov_wss(const double* __restrict__ res, size_t count, double fs2, double ifs2, double* __restrict__ part) {
  __shared__ double s_r[2][256];
  double r[2] = {0.0, 0.0};
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < count; i += (size_t)gridDim.x * 256) {
    const double v = res[i];
    if (v == v) {
      double rh, gw, w2;
      loss_weights<LOSS>(v, fs2, ifs2, rh, gw, w2);
      r[0] += gw * (v * v);
      r[1] += 1.0;
    }
  }
  const bool is_max[2] = {false, false};   // sums alone
  block_tree<2>(s_r, r, is_max);
  if (threadIdx.x == 0) { part[2 * blockIdx.x] = s_r[0][0]; part[2 * blockIdx.x + 1] = s_r[1][0]; }
}

// the partials in order: out[0] = sum w f^2, out[1] = present scalars
__global__ __launch_bounds__(256) void k_cov_wss_final(const double* __restrict__ part, int nblocks, double* __restrict__ out) {
  __shared__ double s_r[2][256];
  double r[2] = {0.0, 0.0};
  for (int i = threadIdx.x; i < nblocks; i += 256) { r[0] += part[2 * i]; r[1] += part[2 * i + 1]; }
  const bool is_max[2] = {false, false};   // sums alone
  block_tree<2>(s_r, r, is_max);
  if (threadIdx.x == 0) { out[0] = s_r[0][0]; out[1] = s_r[1][0]; }
}

int launch_cov_wss(hipStream_t st, int loss, double f_scale, const double* res, size_t count, double* part, double* out) {
  const int nb = (int)std::max<size_t>(1, std::min<size_t>(kCovWssBlocks, (count + 2047) / 2048));
  const double fs2 = f_scale * f_scale, ifs2 = 1.0 / fs2;
  if (with_loss(loss, [&](auto L) {
        hipLaunchKernelGGL(k_cov_wss<decltype(L)::value>, dim3(nb), dim3(256), 0, st, res, count, fs2, ifs2, part);
        return 0;
      }))
    return 1;
  hipLaunchKernelGGL(k_cov_wss_final, dim3(1), dim3(256), 0, st, part, nb, out);
  return 0;
}

// ---------------------------------------------------------------- k_cov_check
// lane = frame: V_f summed over the cameras in k_syrk's order (so the verdict is the one its factorisation came to), then the same chol6i.
// counts[0] += frames that are not positive definite, counts[1] += those of them that hold data (their records did reach S0)
__global__ __launch_bounds__(64) void k_cov_check(const double* __restrict__ rec, unsigned char* __restrict__ flag, int* __restrict__ counts, int C, int F, int Fpad) {
  const int f = blockIdx.x * 64 + threadIdx.x;
  if (f >= F) return;
  const int nfb = Fpad >> 6;
  double V[22];
#pragma unroll
  for (int k = 0; k < 22; ++k) V[k] = 0.0;
  const double2* r2 = reinterpret_cast<const double2*>(rec + (size_t)(f >> 6) * (MCBA_REC * 64)) + (size_t)36 * 64 + (f & 63);
  const size_t cstride = (size_t)nfb * (MCBA_REC * 64 / 2);
  for (int c = 0; c < C; ++c) {
#pragma unroll
    for (int k = 0; k < 11; ++k) {
      const double2 v = r2[(size_t)c * cstride + (size_t)k * 64];
      V[2 * k] += v.x;
      V[2 * k + 1] += v.y;   // (entry 21 is g_f[0]: summed, never looked at)
    }
  }
  bool data = false;
#pragma unroll
  for (int k = 0; k < 21; ++k) data = data || V[k] != 0.0;
  double Lp[21];
  const bool ok = chol6i(V, Lp);
  flag[f] = ok ? 0 : (data ? 2 : 1);
  if (!ok) {
    atomicAdd(counts, 1);
    if (data) atomicAdd(counts + 1, 1);
  }
}

void launch_cov_check(hipStream_t st, const double* rec, unsigned char* flag, int* counts, int C, int F, int Fpad) {
  hipLaunchKernelGGL(k_cov_check, dim3((F + 63) / 64), dim3(64), 0, st, rec, flag, counts, C, F, Fpad);
}

// ---------------------------------------------------------------- k_cov_cam
// One workgroup, thread i = column i of the upper factor R (A = R^T R).  Scale, fill, then column-Cholesky: at pivot j every thread i >= j
// takes its step (reads of R[k][i] are coalesced over i, R[k][j] is one address), thread j tests the pivot.  *pivot = the first that fails.
__global__ __launch_bounds__(1024) void k_cov_cam_factor(const double* __restrict__ S, int n, int cw, int gauge, double* R, int ld, double* isd, int* pivot) {
  __shared__ int s_fail;
  __shared__ double s_d;
  const int i = threadIdx.x;
  if (i == 0) s_fail = 0x7fffffff;
  __syncthreads();
  if (i < n) {
    double v;
    if (!cov_scale(S[(size_t)i * n + i], cov_held(i, cw, gauge), v)) atomicMin(&s_fail, i);
    isd[i] = v;
  }
  __syncthreads();
  if (s_fail != 0x7fffffff) {
    if (i == 0) *pivot = s_fail;
    return;
  }
  if (i < n) {
    const bool hi = cov_held(i, cw, gauge);
    const double di = isd[i];
    for (int k = 0; k <= i; ++k) R[(size_t)k * ld + i] = cov_scaled_entry(S[(size_t)k * n + i], isd[k], di, cov_held(k, cw, gauge), hi, k == i);
  }
  __syncthreads();
  for (int j = 0; j < n; ++j) {
    double s = 0.0;
    if (i >= j && i < n) s = cov_chol_step(R, ld, i, j);
    if (i == j) {
      if (!(s > 0.0)) s_fail = j;
      s_d = sqrt(s);
    }
    __syncthreads();
    if (s_fail != 0x7fffffff) {
      if (i == 0) *pivot = s_fail;
      return;
    }
    if (i >= j && i < n) R[(size_t)j * ld + i] = i == j ? s_d : s / s_d;
    __syncthreads();
  }
}

__global__ __launch_bounds__(64) void k_cov_cam_linv(const double* R, double* M, int ld, int n) {
  const int k0 = blockIdx.x * 64, j = k0 + threadIdx.x;
  if (j < n) cov_linv_column(R, M, ld, n, j, k0);
}

// every entry of the ld x ld buffer: the covariance inside n x n, zero in the held rows and columns and in the padding
__global__ __launch_bounds__(256) void k_cov_cam_gram(const double* __restrict__ M, const double* __restrict__ isd, double* __restrict__ Sig, int ld, int n, int cw, int gauge, double sigma2) {
  const int j = blockIdx.x * 64 + (threadIdx.x & 63), i = blockIdx.y * 4 + (threadIdx.x >> 6);
  if (i >= ld || j >= ld) return;
  double v = 0.0;
  if (i < n && j < n && !cov_held(i, cw, gauge) && !cov_held(j, cw, gauge)) v = cov_cam_entry(M, isd, ld, n, i, j, sigma2);
  Sig[(size_t)i * ld + j] = v;
}

void launch_cov_cam(hipStream_t st, const double* S0, int n, int cw, int gauge, double sigma2, double* R, double* M, double* isd, double* Sig, int ld, int* pivot) {
  hipLaunchKernelGGL(k_cov_cam_factor, dim3(1), dim3(1024), 0, st, S0, n, cw, gauge, R, ld, isd, pivot);
  hipLaunchKernelGGL(k_cov_cam_linv, dim3((n + 63) / 64), dim3(64), 0, st, R, M, ld, n);
  hipLaunchKernelGGL(k_cov_cam_gram, dim3(ld / 64, (ld + 3) / 4), dim3(256), 0, st, M, isd, Sig, ld, n, cw, gauge, sigma2);
}

// ---------------------------------------------------------------- k_cov_frames
// One workgroup = G consecutive frames (8: their 16-byte record entries are one 128-byte line per load; 4 when Y does not fit otherwise),
// 256 threads.  R = 6 G rows of the stacked Y (row 6 g + k = row k of Y of frame g), RT = ceil(R / 16) row tiles, KP = ceil(n / 32) 32.
//   1. the first G threads: V_f^-1 from fbuf's L_f (zero for a frame that is flagged or past the end: its Y is zero)
//   2. item (camera-system row r, frame g), frames fastest: the record's W row -> y = V^-1 w -> s_Y[6 g + k][r]; columns n .. KP are zero
//   3. the diagonal blocks of Y Sigma_cc Y^T: diag_blocks (mcba_quadform.h), thread (g, k <= l) gets entry (k, l) of frame g
//   4. Sigma_ff = sigma2 V^-1 + that, mirrored, through LDS to out[f][36] in runs of consecutive doubles; frames >= F write nothing.
static size_t cov_frames_lds(int n, int G) {
  const int KP = (n + 31) / 32 * 32, R = 6 * G;
  return ((size_t)R * (KP + 2) + stage_doubles(R) + (size_t)G * 21 + (size_t)G * 36) * sizeof(double);
}

template <int CW, int RT>
__global__ __launch_bounds__(256) void k_cov_frames(const double* __restrict__ rec, const double* __restrict__ fbuf, const unsigned char* __restrict__ flag, const double* __restrict__ Sig, int ld,
                                                   double sigma2, double* __restrict__ out, int C, int F, int Fpad, int G, int KP) {
  extern __shared__ __align__(16) double lds[];
  const int t = threadIdx.x;
  const int n = CW * C, nfb = Fpad >> 6, R = 6 * G, RS = KP + 2;
  double* s_Y = lds;                                   // [R][RS]
  double* s_P = s_Y + (size_t)R * RS;                  // the staging buffer of diag_blocks
  double* s_Vi = s_P + stage_doubles(R);               // [G][21]
  double* s_o = s_Vi + G * 21;                         // [G][36]
  const int f0 = blockIdx.x * G, ng = min(G, F - f0);

  if (t < G) {
    double Vi[21];
#pragma unroll
    for (int k = 0; k < 21; ++k) Vi[k] = 0.0;
    if (t < ng && flag[f0 + t] == 0) {
      double Lp[21];
      const double* fb = fbuf + (size_t)(f0 + t) * MCBA_FB;
#pragma unroll
      for (int k = 0; k < 21; ++k) Lp[k] = fb[k];
      cov_inv6(Lp, Vi);
    }
#pragma unroll
    for (int k = 0; k < 21; ++k) s_Vi[t * 21 + k] = Vi[k];
  }
  __syncthreads();
  for (int it = t; it < n * G; it += 256) {
    const int g = it % G, r = it / G;
    double y[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    if (g < ng) {
      const int c = r / CW, lr = r - CW * c + (12 - CW), f = f0 + g;
      const double2* w2 = reinterpret_cast<const double2*>(rec + ((size_t)c * nfb + (f >> 6)) * (MCBA_REC * 64)) + (size_t)(3 * lr) * 64 + (f & 63);
      double w[6];
#pragma unroll
      for (int k = 0; k < 3; ++k) { const double2 v = w2[k * 64]; w[2 * k] = v.x; w[2 * k + 1] = v.y; }
      cov_y_row(s_Vi + g * 21, w, y);
    }
#pragma unroll
    for (int k = 0; k < 6; ++k) s_Y[(size_t)(6 * g + k) * RS + r] = y[k];
  }
  for (int it = t; it < R * (KP - n); it += 256) s_Y[(size_t)(it / (KP - n)) * RS + n + it % (KP - n)] = 0.0;
  // (the first barrier of diag_blocks orders these stores before the first read)

  int og = 0, ok_ = 0, ol = 0;
  const bool own = t < G * 21;   // G <= 8: at most 168 (frame, k <= l) outputs, one per thread
  if (own) { og = t / 21; cov_tri6_pair(t % 21, ok_, ol); }
  const double zy = diag_blocks<RT, 6>(s_Y, s_P, Sig, ld, R, KP, own, og, ok_, ol);
  if (own) {
    const bool deg = og < ng && flag[f0 + og] != 0;
    const double v = cov_frame_entry(s_Vi[og * 21 + tri6(ok_, ol)], zy, sigma2, deg);
    s_o[og * 36 + 6 * ok_ + ol] = v;
    s_o[og * 36 + 6 * ol + ok_] = v;
  }
  __syncthreads();
  for (int i = t; i < ng * 36; i += 256) out[(size_t)f0 * 36 + i] = s_o[i];
}

// G frames per workgroup: 8 if its LDS fits, else 4 (beyond about 26 cameras); force_g (4 or 8, tests) overrides when it fits
int cov_frames_group(int n, int lds_limit, int force_g) {
  if ((force_g == 4 || force_g == 8) && cov_frames_lds(n, force_g) <= (size_t)lds_limit) return force_g;
  if (cov_frames_lds(n, 8) <= (size_t)lds_limit) return 8;
  if (cov_frames_lds(n, 4) <= (size_t)lds_limit) return 4;
  return 0;
}

int launch_cov_frames(hipStream_t st, const double* rec, const double* fbuf, const unsigned char* flag, const double* Sig, int ld, double sigma2, double* out, int C, int F, int Fpad, int cw, int G) {
  const int n = cw * C, KP = (n + 31) / 32 * 32;
  if ((G != 4 && G != 8) || KP > ld || ld % 64 != 0) return 1;
  const size_t lds = cov_frames_lds(n, G);
  return with_int<6, 12>(cw == 12 ? 12 : 6, [&](auto CW) {
    return with_int<2, 3>(G == 8 ? 3 : 2, [&](auto RT) {
      return launch_with_lds(k_cov_frames<decltype(CW)::value, decltype(RT)::value>, dim3((F + G - 1) / G), lds, st, rec, fbuf, flag, Sig, ld, sigma2, out, C, F, Fpad, G, KP);
    });
  });
}

}  // namespace mcba
