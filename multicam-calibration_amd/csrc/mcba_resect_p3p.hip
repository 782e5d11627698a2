// mcba_resect_p3p.hip -- the minimal generator of the resection: H host-drawn 3-point samples per camera, up to four
// candidate poses each.  The per-lane arithmetic is in mcba_resect_p3p_math.h, where the host harness checks the same text.
//   k_rs3_hypotheses    lane = (camera, sample), 64 lanes per workgroup, the camera is blockIdx.y: p3_sample on the 3 sampled points --
//                       Grunert's quartic, its real roots, per root the pose from the two triangles' frames and five Gauss-Newton iterations
//                       -- and K [R | t]; slots 4 h .. 4 h + 3 of the (C, 4 H, 12) table, void slots included.  No work matrices: a lane's
//                       state is its 3 points, the quartic and one pose at a time
// The table is scored in place by k_hyp_score, k_hyp_finish, k_rs_winner and k_rs_mask (mcba_resect.hip) with 4 H for H: a void slot costs
// +inf there, so nothing is compacted and the cameras' different live counts need no bookkeeping.  No atomics.
#include <hip/hip_runtime.h>
#include <math.h>
// No contraction beyond the fma() calls the text spells out, as in mcba_resect.hip: the host build of the header rounds alike.
#pragma clang fp contract(off)
#include "mcba_kernels.h"
#include "mcba_device.h"
#include "mcba_resect_p3p_math.h"
#include "../../include/mcba.h"

static_assert(mcba::kP3Sample == MCBA_RESECT_P3P_SAMPLE && mcba::kP3Slots == MCBA_RESECT_P3P_SLOTS && mcba::kP3Polish == MCBA_RESECT_P3P_POLISH,
              "include/mcba.h names the sample size, the slots of a sample and the Gauss-Newton iterations of a candidate");
static_assert(MCBA_RESECT_P3P_SLOTS * MCBA_RESECT_P3P_MAX_SAMPLES <= MCBA_RESECT_MAX_HYPOTHESES, "the table of 4 H slots is within the scorer's bounds");

namespace mcba {

// samples: (C, H, 3); pose, KP: (C, 4 H, 12); status: (C, 4 H)
__global__ __launch_bounds__(64) void k_rs3_hypotheses(const double* __restrict__ points, const double* __restrict__ prep, size_t P, const int* __restrict__ samples, int H,
                                                       const double* __restrict__ cams, double* __restrict__ pose, double* __restrict__ KP, int* __restrict__ status) {
  const int h = blockIdx.x * 64 + threadIdx.x, c = blockIdx.y;
  if (h >= H) return;
  const size_t ch = (size_t)c * H + h;
  double X[9], x[6], k4[4];
#pragma unroll
  for (int k = 0; k < kP3Sample; ++k) {
    const size_t s = (size_t)samples[kP3Sample * ch + k];   // (0 .. P - 1 and usable: checked on the host before the upload)
    X[3 * k] = points[3 * s]; X[3 * k + 1] = points[3 * s + 1]; X[3 * k + 2] = points[3 * s + 2];
    x[2 * k] = prep[((size_t)c * 4 + 2) * P + s]; x[2 * k + 1] = prep[((size_t)c * 4 + 3) * P + s];
  }
  P3Roots r;
  p3_roots(X, x, r);
#pragma unroll
  for (int i = 0; i < 4; ++i) k4[i] = cams[9 * c + i];
#pragma unroll
  for (int k = 0; k < kP3Slots; ++k) {   // (unrolled: the root of a slot is a register, not an indexed array)
    const size_t row = kP3Slots * ch + k;
    double q[12], kp[12], step[6];
    const int st = p3_candidate(X, x, r, k, q, step);
    rs_pixel_matrix(q, k4, kp);
#pragma unroll
    for (int i = 0; i < 12; ++i) { pose[12 * row + i] = q[i]; KP[12 * row + i] = kp[i]; }
    status[row] = st;
  }
}

void launch_rs3_hypotheses(hipStream_t st, const double* points, const double* prep, size_t P, int C, const int* samples, int H, const double* cams, double* pose, double* KP, int* status) {
  k_rs3_hypotheses<<<dim3((unsigned)((H + 63) / 64), (unsigned)C), dim3(64), 0, st>>>(points, prep, P, samples, H, cams, pose, KP, status);
}

}  // namespace mcba
