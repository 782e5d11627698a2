// mcba_smooth_cov.hip -- trajectory uncertainty: the band of the inverse of the smoother's system, by selected inversion
// over the separator tree of its elimination.  Per-lane arithmetic: mcba_smooth_cov_math.h (host-checked).  No atomics: every word has one writer.
// The elimination is the smoother's own: launch_smooth_reduce of mcba_smooth.hip (the right-hand side rides along unused).
//   k_smooth_selinv  lane = (segment, track), laid out as k_smooth_backsub: the segment's diagonal and sub-diagonal blocks of the inverse from
//                    its separators'; level 0 writes the frames' covariances and, on request, the lag-one blocks
#include <hip/hip_runtime.h>

#include "mcba_device.h"
#include "mcba_kernels.h"
#include "mcba_smooth_cov_math.h"

namespace mcba {

// the lane's state is about 195 doubles: it wants the whole register file, as k_smooth_reduce, and still spills
template <bool LEVEL0>
__global__ __launch_bounds__(64) void k_smooth_selinv(SmLevel lv, SmLevel up, SmData td, double* __restrict__ z, const double* __restrict__ zup, double* __restrict__ cov6, double* __restrict__ lag9,
                                                      int K, const int* __restrict__ list, int nact, int nq) {
  const size_t gid = (size_t)blockIdx.x * 64 + threadIdx.x;
  if (gid >= (size_t)nq * nact) return;
  smooth_selinv_lane<LEVEL0>(lv, up, td, z, zup, cov6, lag9, K, list[gid % nact], (int)(gid / nact));
}

// the selected inversion, every level down.  z[l]: the SM_ZC planes of level l >= 1 (z[0] unused); cov6 (T, K, 6), lag9 (T - 1, K, 9) or null
int launch_smooth_selinv(hipStream_t st, const SmLevel* lv, int levels, const SmData& td, double* const* z, double* cov6, double* lag9, int K, const int* list, int nact) {
  if (levels < 1 || levels > SM_MAX_LEVELS || nact < 1 || nact > K) return 1;
  const SmLevel none{};
  for (int l = levels - 1; l >= 0; --l) {
    int nq;
    unsigned blocks;
    if (!smooth_grid(lv[l], nact, nq, blocks)) return 1;
    const SmLevel& up = l + 1 < levels ? lv[l + 1] : none;
    const double* zup = l + 1 < levels ? z[l + 1] : nullptr;
    if (l == 0) k_smooth_selinv<true><<<dim3(blocks), dim3(64), 0, st>>>(lv[0], up, td, nullptr, zup, cov6, lag9, K, list, nact, nq);
    else k_smooth_selinv<false><<<dim3(blocks), dim3(64), 0, st>>>(lv[l], up, td, z[l], zup, nullptr, nullptr, K, list, nact, nq);
  }
  return 0;
}

}  // namespace mcba
