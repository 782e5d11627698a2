// mcba_fivepoint.hip -- the five-point hypothesis generator of the two-view RANSAC (the reference has no counterpart):
// H host-drawn samples of five calibrated correspondences give up to ten essential matrices each.  The per-lane arithmetic is in
// mcba_fivepoint_math.h, where the host harness checks the same text.
//   k_tv5_hypotheses  lane = sample: fp_candidates on the five sampled correspondences, tv_fundamental per slot; a table of 10 H rows (E, F,
//                     status), the live candidates of a sample in its leading slots.  The work space of a sample (FpWork: two 10 x 20 matrices and
//                     the basis, 436 doubles, indexed at run time) is in scratch: H is 1024 at most, this is not the hot kernel
//   k_tv5_compact     one workgroup: the live slots packed, order-preserving, into the table k_hyp_score, k_hyp_finish, k_tv_winner and the pose
//                     kernels of mcba_twoview.hip see; lane t counts the live slots of its contiguous run, the runs' counts are prefix-summed in
//                     lane order, lane t writes its run.  map[i] = 10 sample + slot of packed row i.  No atomics: the order is the table's.
//                     Nothing live: row 0 is slot 0 (void, NaN), so that "hypothesis 0 wins with nothing" as in mcba_two_view_ransac
#include <hip/hip_runtime.h>
#include <math.h>
#pragma clang fp contract(off)
#include "mcba_kernels.h"
#include "mcba_fivepoint_math.h"
#include "../../include/mcba.h"

static_assert(mcba::FP_SAMPLE == MCBA_TWOVIEW5_SAMPLE && mcba::FP_SLOTS == MCBA_TWOVIEW5_SLOTS, "include/mcba.h names the shape of the candidate table");

namespace mcba {

__global__ __launch_bounds__(64) void k_tv5_hypotheses(const double* __restrict__ prep, size_t M, const int* __restrict__ samples, int H, TvCams cams, double* __restrict__ E10,
                                                       double* __restrict__ F10, int* __restrict__ status10) {
  const int h = blockIdx.x * 64 + threadIdx.x;
  if (h >= H) return;
  double xa[2 * FP_SAMPLE], xb[2 * FP_SAMPLE];
  for (int k = 0; k < FP_SAMPLE; ++k) {
    const size_t s = (size_t)samples[FP_SAMPLE * (size_t)h + k];   // (0 .. M - 1: checked on the host before the upload)
    xa[2 * k] = prep[4 * M + s]; xa[2 * k + 1] = prep[5 * M + s];
    xb[2 * k] = prep[6 * M + s]; xb[2 * k + 1] = prep[7 * M + s];
  }
  FpWork w;
  double e[9 * FP_SLOTS];
  int st[FP_SLOTS];
  fp_candidates(xa, xb, w, e, st, nullptr);
  for (int c = 0; c < FP_SLOTS; ++c) {
    double f[9];
    tv_fundamental(e + 9 * c, cams.ka, cams.kb, f);
    const size_t row = (size_t)FP_SLOTS * h + c;
    for (int i = 0; i < 9; ++i) { E10[9 * row + i] = e[9 * c + i]; F10[9 * row + i] = f[i]; }
    status10[row] = st[c];
  }
}

// S = 10 H slots.  Ep, Fp (n, 9), stp (n), map (n), n_packed[0] = n >= 1
__global__ __launch_bounds__(kHypThreads) void k_tv5_compact(const double* __restrict__ E10, const double* __restrict__ F10, const int* __restrict__ status10, int S, double* __restrict__ Ep,
                                                            double* __restrict__ Fp, int* __restrict__ stp, int* __restrict__ map, int* __restrict__ n_packed) {
  __shared__ int s_n[kHypThreads];
  const int tid = threadIdx.x;
  const int run = (S + kHypThreads - 1) / kHypThreads, s0 = tid * run, s1 = s0 + run < S ? s0 + run : S;
  int n = 0;
  for (int s = s0; s < s1; ++s) n += status10[s] == TV_OK ? 1 : 0;
  s_n[tid] = n;
  __syncthreads();
  if (tid == 0) {   // exclusive prefix in lane order (256 additions)
    int acc = 0;
    for (int t = 0; t < kHypThreads; ++t) { const int c = s_n[t]; s_n[t] = acc; acc += c; }
    n_packed[0] = acc > 0 ? acc : 1;
    if (acc == 0) {
      for (int i = 0; i < 9; ++i) { Ep[i] = E10[i]; Fp[i] = F10[i]; }
      stp[0] = TV_VOID;
      map[0] = 0;
    }
  }
  __syncthreads();
  int at = s_n[tid];
  for (int s = s0; s < s1; ++s)
    if (status10[s] == TV_OK) {
      for (int i = 0; i < 9; ++i) { Ep[9 * (size_t)at + i] = E10[9 * (size_t)s + i]; Fp[9 * (size_t)at + i] = F10[9 * (size_t)s + i]; }
      stp[at] = TV_OK;
      map[at] = s;
      ++at;
    }
}

void launch_tv5_hypotheses(hipStream_t st, const double* prep, size_t M, const int* samples, int H, const TvCams& cams, double* E10, double* F10, int* status10, double* Ep, double* Fp, int* stp,
                           int* map, int* n_packed) {
  k_tv5_hypotheses<<<dim3((unsigned)((H + 63) / 64)), dim3(64), 0, st>>>(prep, M, samples, H, cams, E10, F10, status10);
  k_tv5_compact<<<dim3(1), dim3(kHypThreads), 0, st>>>(E10, F10, status10, FP_SLOTS * H, Ep, Fp, stp, map, n_packed);
}

}  // namespace mcba
