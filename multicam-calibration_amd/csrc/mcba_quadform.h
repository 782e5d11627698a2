// mcba_quadform.h -- the diagonal blocks of Y Sigma Y^T on the matrix cores: the panel loop shared by k_cov_frames (mcba_cov.hip, 6 rows per
// frame) and k_tricov_cal (mcba_tricov.hip, 3 rows per point).  A workgroup of 256 threads holds R = B G stacked rows of Y in LDS ([R][KP + 2],
// columns n .. KP zero, KP = ceil(n / 32) 32) and owns a staging buffer of stage_doubles(R) doubles behind it.
//   per panel of 64 columns of Sigma (wavefront w: columns 16 w .. 16 w + 15 of it), K in chunks of 32 rows staged through LDS (the next chunk's
//   loads fly during the matrix-core phase): Z tile += Y tile x Sigma chunk on v_mfma_f64_16x16x4_f64, RT = ceil(R / 16) row tiles.  Z goes to LDS
//   (over the staging buffer) and is contracted with Y: thread (g, k <= l) adds sum_j Z[B g + k][j] Y[B g + l][j] -- each item's own diagonal
//   block, nothing else.  The caller adds its own term to that sum and writes the blocks out through LDS.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>

namespace mcba {

constexpr int kQfKC = 32, kQfPS = 80, kQfZS = 66;   // rows of a staged chunk, its row stride, the row stride of Z

typedef double qf_d4 __attribute__((ext_vector_type(4)));

// doubles of the staging buffer: a [kQfKC][kQfPS] chunk of Sigma, later Z as [R][kQfZS]
__host__ __device__ constexpr size_t stage_doubles(int R) {
  return (size_t)kQfKC * kQfPS > (size_t)R * kQfZS ? (size_t)kQfKC * kQfPS : (size_t)R * kQfZS;
}

// Every thread of the workgroup calls this (barriers inside; the first one also orders the caller's stores to s_Y before the first read).
// Sig: the zero-padded ld x ld buffer, KP <= ld, ld a multiple of 64.  own: this thread holds entry (ok_ <= ol) of item og; the others get 0.
template <int RT, int B>
__device__ __forceinline__ double diag_blocks(const double* s_Y, double* s_P, const double* __restrict__ Sig, int ld, int R, int KP, bool own, int og, int ok_, int ol) {
  const int t = threadIdx.x, lane = t & 63;
  const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
  const int RS = KP + 2;
  double zy = 0.0;
  const int nkc = KP / kQfKC, npan = (KP + 63) / 64;
  int arow[RT];
#pragma unroll
  for (int ti = 0; ti < RT; ++ti) arow[ti] = min(16 * ti + (lane & 15), R - 1) * RS + (lane >> 4);   // (rows past R: a duplicate, its results are never stored)
  for (int J = 0; J < npan; ++J) {
    const bool active = 64 * J + 16 * wave < KP;   // wave-uniform: this wavefront's 16 columns hold anything
    qf_d4 acc[RT];
#pragma unroll
    for (int ti = 0; ti < RT; ++ti) acc[ti] = qf_d4{0.0, 0.0, 0.0, 0.0};
    double pv[8];
    auto fetch = [&](int kc) {   // rows 32 kc .. + 31, columns 64 J .. + 63 of the zero-padded ld x ld buffer: inside it (KP <= ld, ld a multiple of 64)
#pragma unroll
      for (int q = 0; q < 8; ++q) {
        const int idx = t + 256 * q;
        pv[q] = Sig[(size_t)(kQfKC * kc + (idx >> 6)) * ld + 64 * J + (idx & 63)];
      }
    };
    fetch(0);
    for (int kc = 0; kc < nkc; ++kc) {
      __syncthreads();   // the previous chunk's reads (or the previous panel's contraction) are done
#pragma unroll
      for (int q = 0; q < 8; ++q) { const int idx = t + 256 * q; s_P[(idx >> 6) * kQfPS + (idx & 63)] = pv[q]; }
      __syncthreads();
      if (kc + 1 < nkc) fetch(kc + 1);
      if (active) {
#pragma unroll
        for (int ks = 0; ks < kQfKC / 4; ++ks) {
          const double b = s_P[(4 * ks + (lane >> 4)) * kQfPS + 16 * wave + (lane & 15)];
#pragma unroll
          for (int ti = 0; ti < RT; ++ti) {
            const double a = s_Y[arow[ti] + kQfKC * kc + 4 * ks];
            acc[ti] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc[ti], 0, 0, 0);
          }
        }
      }
    }
    __syncthreads();   // every wavefront is done with the staging buffer: Z takes its place
    if (active) {
#pragma unroll
      for (int ti = 0; ti < RT; ++ti) {
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) {
          const int row = 16 * ti + 4 * reg + (lane >> 4);
          if (row < R) s_P[row * kQfZS + 16 * wave + (lane & 15)] = acc[ti][reg];
        }
      }
    }
    __syncthreads();
    if (own) {
      const int jn = min(64, KP - 64 * J);
      const double* zr = s_P + (B * og + ok_) * kQfZS;
      const double* yr = s_Y + (size_t)(B * og + ol) * RS + 64 * J;
      double s = 0.0;
      for (int j = 0; j < jn; ++j) s += zr[j] * yr[j];
      zy += s;
    }
  }
  return zy;
}

}  // namespace mcba
