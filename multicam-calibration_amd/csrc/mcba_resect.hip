// mcba_resect.hip -- camera resection (the reference resects only a planar board, through cv2.solvePnP): the pose of each
// of C cameras from P known 3-D points and that camera's own detections, H host-drawn 6-point samples per camera.  The per-lane arithmetic is
// in mcba_resect_math.h, where the host harness checks the same text.  Cameras are independent: the camera is a grid dimension everywhere.
//   k_rs_prepare        lane = (camera, point): the detection undistorted once; undistorted pixels and normalised coordinates in 4 planes per
//                       camera (SoA), a usable flag (point and detection finite)
//   k_rs_hypotheses     lane = (camera, hypothesis): rs_hypothesis on the 6 sampled points -- DLT, then ten Gauss-Newton iterations -- and
//                       K [R | t].  The two 12 x 12 work matrices (288 doubles) are in scratch: H is a few thousand at most, not the hot kernel
//   k_hyp_score         the hot one (mcba_hyp_score.h) with RsScore: K [R | t] against X, Y, Z and the undistorted u, v of the camera's usable
//                       points, the truncated reprojection cost; then k_hyp_finish of mcba_twoview.hip (launch_hyp_finish) with grid (H, C)
//   k_rs_winner         workgroup = camera: the lowest (cost, index), hyp_argmin; its pose
//   k_rs_mask           lane = (camera, point): the winner's inlier mask, with the scorer's own inline function
//   k_rs_normal         the polish: lane = (listed camera, point) over the masked points, rs_normal_item; kRsSys sums per workgroup in the
//                       scorer's order; COST_ONLY: the robust cost and the count alone (a trial pose)
//   k_rs_normal_finish  workgroup = listed camera: lane v sums value v of the partials in workgroup order
// No atomics, floating-point or other: every sum has a fixed order, the results depend on (P, H) alone, bit for bit.
#include <hip/hip_runtime.h>
#include <math.h>
// No contraction beyond the fma() calls the text spells out: k_hyp_score<RsScore> and k_rs_mask must judge a point alike to the last bit.
#pragma clang fp contract(off)
#include "mcba_hyp_score.h"
#include "mcba_resect_math.h"
#include "../../include/mcba.h"

static_assert(mcba::kHypPoints == MCBA_RESECT_POINTS_PER_BLOCK && mcba::kHypChunk == MCBA_RESECT_CHUNK, "include/mcba.h names the launch shape of k_hyp_score");
static_assert(mcba::RS_OK == mcba::TV_OK, "k_hyp_finish tells a live hypothesis of either pipeline by the one status");
static_assert(mcba::kRsSample == MCBA_RESECT_SAMPLE && mcba::kRsGnIterations == MCBA_RESECT_GN_ITERATIONS, "include/mcba.h names the sample size and the Gauss-Newton iterations of a hypothesis");
static_assert(mcba::kRsSys == MCBA_RESECT_SYSTEM, "include/mcba.h names the length of a camera's normal system");

namespace mcba {

// cams: (C, 9) = fx fy cx cy k1 k2 p1 p2 k3.  prep: per camera 4 planes of P doubles (undistorted u, v; normalised x, y); usable: (C, P)
__global__ __launch_bounds__(kHypThreads) void k_rs_prepare(const double* __restrict__ points, const double* __restrict__ uvs, size_t P, const double* __restrict__ cams, int und_iters,
                                                           double* __restrict__ prep, unsigned char* __restrict__ usable) {
  const size_t p = (size_t)blockIdx.x * kHypThreads + threadIdx.x;
  const int c = blockIdx.y;
  if (p >= P) return;
  const double u = uvs[2 * ((size_t)c * P + p)], v = uvs[2 * ((size_t)c * P + p) + 1];
  const bool ok = rs_usable(points[3 * p], points[3 * p + 1], points[3 * p + 2], u, v);
  double k9[9], o[4];
#pragma unroll
  for (int i = 0; i < 9; ++i) k9[i] = cams[9 * c + i];
  rs_prepare(u, v, k9, k9 + 4, und_iters, o);
#pragma unroll
  for (int k = 0; k < 4; ++k) prep[((size_t)c * 4 + k) * P + p] = ok ? o[k] : 0.0;
  usable[(size_t)c * P + p] = ok ? 1 : 0;
}

// pose, KP: (C, H, 12); status: (C, H).  pose_in (C, H, 12) or nullptr
__global__ __launch_bounds__(64) void k_rs_hypotheses(const double* __restrict__ points, const double* __restrict__ prep, size_t P, const int* __restrict__ samples, int H,
                                                      const double* __restrict__ pose_in, const double* __restrict__ cams, double* __restrict__ pose, double* __restrict__ KP,
                                                      int* __restrict__ status) {
  const int h = blockIdx.x * 64 + threadIdx.x, c = blockIdx.y;
  if (h >= H) return;
  const size_t ch = (size_t)c * H + h;
  double q[12], kp[12];
  int st;
  if (pose_in) {
    bool ok = true;
#pragma unroll
    for (int i = 0; i < 12; ++i) { q[i] = pose_in[12 * ch + i]; ok = ok && rs_finite(q[i]); }
    st = ok ? RS_OK : RS_VOID;
  } else {
    double X[18], x[12], S[144], V[144], step[6];
    for (int k = 0; k < kRsSample; ++k) {
      const size_t s = (size_t)samples[kRsSample * ch + k];   // (0 .. P - 1 and usable: checked on the host before the upload)
      X[3 * k] = points[3 * s]; X[3 * k + 1] = points[3 * s + 1]; X[3 * k + 2] = points[3 * s + 2];
      x[2 * k] = prep[((size_t)c * 4 + 2) * P + s]; x[2 * k + 1] = prep[((size_t)c * 4 + 3) * P + s];
    }
    st = rs_hypothesis(X, x, S, V, q, step);
  }
  double k4[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) k4[i] = cams[9 * c + i];
  rs_pixel_matrix(q, k4, kp);
#pragma unroll
  for (int i = 0; i < 12; ++i) { pose[12 * ch + i] = q[i]; KP[12 * ch + i] = kp[i]; }
  status[ch] = st;
}

// k_hyp_score's resection model: a hypothesis is K [R | t] (12 doubles), a point is X, Y, Z and the camera's undistorted u, v (planes 0, 1 of
// its prep); a point that is not usable for the camera is not ok
struct RsScore {
  static constexpr int kDoubles = 12;
  static constexpr bool kCameras = true;
  struct Point { double X, Y, Z, u, v; bool ok; };
  const double* __restrict__ points;
  const double* __restrict__ prep;
  const unsigned char* __restrict__ usable;
  size_t P;
  __device__ __forceinline__ Point load(int c, size_t p) const {
    const bool ok = p < P && usable[(size_t)c * P + (p < P ? p : 0)] != 0;
    const double* pu = prep + (size_t)c * 4 * P;
    return {ok ? points[3 * p] : 0.0, ok ? points[3 * p + 1] : 0.0, ok ? points[3 * p + 2] : 0.0, ok ? pu[p] : 0.0, ok ? pu[P + p] : 0.0, ok};
  }
  static __device__ __forceinline__ double error2(const double* kp, const Point& q) { return rs_error2(kp, q.X, q.Y, q.Z, q.u, q.v); }
};

// workgroup = camera: the winner (hyp_argmin) and its pose.  best4: (C, 4), slot 3 is the host's
__global__ __launch_bounds__(kHypThreads) void k_rs_winner(const double* __restrict__ cost, const unsigned* __restrict__ count, int H, const double* __restrict__ pose, int* __restrict__ win_idx,
                                                           double* __restrict__ best4, double* __restrict__ rt12) {
  const int tid = threadIdx.x, c = blockIdx.x;
  double bc;
  const int w = hyp_argmin(cost + (size_t)c * H, H, bc);
  if (tid == 0) {
    win_idx[c] = w;
    best4[4 * c] = (double)w; best4[4 * c + 1] = bc; best4[4 * c + 2] = (double)count[(size_t)c * H + w]; best4[4 * c + 3] = 0.0;
  }
  if (tid < 12) rt12[12 * c + tid] = pose[12 * ((size_t)c * H + w) + tid];
}

__global__ __launch_bounds__(kHypThreads) void k_rs_mask(const double* __restrict__ points, const double* __restrict__ prep, const unsigned char* __restrict__ usable, size_t P,
                                                        const double* __restrict__ KP, const int* __restrict__ status, int H, double t2, const int* __restrict__ win_idx,
                                                        unsigned char* __restrict__ inliers) {
  const size_t p = (size_t)blockIdx.x * kHypThreads + threadIdx.x;
  const int c = blockIdx.y;
  if (p >= P) return;
  const size_t cw = (size_t)c * H + win_idx[c];
  double kp[12];
#pragma unroll
  for (int i = 0; i < 12; ++i) kp[i] = KP[12 * cw + i];
  const bool ok = usable[(size_t)c * P + p] != 0 && status[cw] == RS_OK;
  const double* pu = prep + (size_t)c * 4 * P;
  const double e2 = rs_error2(kp, ok ? points[3 * p] : 0.0, ok ? points[3 * p + 1] : 0.0, ok ? points[3 * p + 2] : 0.0, ok ? pu[p] : 0.0, ok ? pu[P + p] : 0.0);
  inliers[(size_t)c * P + p] = ok && tv_inlier(e2, t2) ? 1 : 0;
}

// grid: (hyp_point_blocks(P), n).  ids (n): the camera of each listed problem (rows of uvs / mask); tcs (n): its camera at the pose to evaluate.
// part: (n, blocks, kRsSys), COST_ONLY: slots 27, 28 alone are written
template <int LOSS, bool COST_ONLY>
__global__ __launch_bounds__(kHypThreads) void k_rs_normal(const double* __restrict__ points, const double* __restrict__ uvs, const unsigned char* __restrict__ mask, size_t P,
                                                          const int* __restrict__ ids, const TcCam* __restrict__ tcs, double fs2, double inv_fs2, double* __restrict__ part) {
  constexpr int NV = COST_ONLY ? 2 : kRsSys, V0 = COST_ONLY ? 27 : 0;
  __shared__ double s_v[kHypThreads / 64][NV];
  __shared__ TcCam s_tc;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int k = blockIdx.y, c = ids[k];
  if (tid < 30) reinterpret_cast<double*>(&s_tc)[tid] = reinterpret_cast<const double*>(tcs + k)[tid];
  __syncthreads();
  const size_t p = (size_t)blockIdx.x * kHypThreads + tid;
  double acc[kRsSys];
#pragma unroll
  for (int i = 0; i < kRsSys; ++i) acc[i] = 0.0;
  bool use = p < P && mask[(size_t)c * P + (p < P ? p : 0)] != 0;
  double X[3] = {0.0, 0.0, 1.0}, ou = 0.0, ov = 0.0;
  if (use) {
    X[0] = points[3 * p]; X[1] = points[3 * p + 1]; X[2] = points[3 * p + 2];
    ou = uvs[2 * ((size_t)c * P + p)]; ov = uvs[2 * ((size_t)c * P + p) + 1];
    use = rs_usable(X[0], X[1], X[2], ou, ov);
  }
  if (use) {
    if (COST_ONLY) { acc[27] = rs_cost_item<LOSS>(s_tc, X, ou, ov, fs2, inv_fs2); acc[28] = 1.0; }
    else rs_normal_item<LOSS>(s_tc, X, ou, ov, fs2, inv_fs2, acc);
  }
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    const double s = wave_sum(acc[V0 + i]);
    if (lane == 0) s_v[wave][i] = s;
  }
  __syncthreads();
  if (tid < NV) {
    double s = s_v[0][tid];
#pragma unroll
    for (int w = 1; w < kHypThreads / 64; ++w) s += s_v[w][tid];
    part[((size_t)k * gridDim.x + blockIdx.x) * kRsSys + V0 + tid] = s;
  }
}

// workgroup (64 lanes) = listed camera: lane v sums value v over the workgroups in order.  sys: (n, kRsSys)
__global__ __launch_bounds__(64) void k_rs_normal_finish(const double* __restrict__ part, size_t nblk, int cost_only, double* __restrict__ sys) {
  const int k = blockIdx.x, v = threadIdx.x;
  if (v >= kRsSys) return;
  double s = 0.0;
  if (!cost_only || v >= 27)
    for (size_t bk = 0; bk < nblk; ++bk) s += part[((size_t)k * nblk + bk) * kRsSys + v];
  sys[(size_t)k * kRsSys + v] = s;
}

// ---------------------------------------------------------------- launch wrappers
void launch_rs_prepare(hipStream_t st, const double* points, const double* uvs, size_t P, int C, const double* cams, int und_iters, double* prep, unsigned char* usable) {
  k_rs_prepare<<<dim3((unsigned)hyp_point_blocks(P), (unsigned)C), dim3(kHypThreads), 0, st>>>(points, uvs, P, cams, und_iters, prep, usable);
}

void launch_rs_hypotheses(hipStream_t st, const double* points, const double* prep, size_t P, int C, const int* samples, int H, const double* pose_in, const double* cams, double* pose, double* KP,
                          int* status) {
  k_rs_hypotheses<<<dim3((unsigned)((H + 63) / 64), (unsigned)C), dim3(64), 0, st>>>(points, prep, P, samples, H, pose_in, cams, pose, KP, status);
}

void launch_rs_score(hipStream_t st, const double* points, const double* prep, const unsigned char* usable, size_t P, int C, const double* KP, int H, double threshold, double* part_c,
                     unsigned* part_n) {
  launch_hyp_score(st, RsScore{points, prep, usable, P}, P, C, KP, H, threshold, part_c, part_n);
}

void launch_rs_finish(hipStream_t st, const double* part_c, const unsigned* part_n, size_t nblk, int C, int H, const double* pose, const int* status, double* cost, unsigned* count, int* win_idx,
                      double* best4, double* rt12) {
  launch_hyp_finish(st, part_c, part_n, nblk, C, H, status, cost, count);
  k_rs_winner<<<dim3((unsigned)C), dim3(kHypThreads), 0, st>>>(cost, count, H, pose, win_idx, best4, rt12);
}

void launch_rs_mask(hipStream_t st, const double* points, const double* prep, const unsigned char* usable, size_t P, int C, const double* KP, const int* status, int H, double threshold,
                    const int* win_idx, unsigned char* inliers) {
  k_rs_mask<<<dim3((unsigned)hyp_point_blocks(P), (unsigned)C), dim3(kHypThreads), 0, st>>>(points, prep, usable, P, KP, status, H, threshold * threshold, win_idx, inliers);
}

template <int LOSS>
static void rs_normal_launch(hipStream_t st, bool cost_only, dim3 grid, const double* points, const double* uvs, const unsigned char* mask, size_t P, const int* ids, const TcCam* tcs, double fs2,
                             double* part) {
  if (cost_only) k_rs_normal<LOSS, true><<<grid, dim3(kHypThreads), 0, st>>>(points, uvs, mask, P, ids, tcs, fs2, 1.0 / fs2, part);
  else k_rs_normal<LOSS, false><<<grid, dim3(kHypThreads), 0, st>>>(points, uvs, mask, P, ids, tcs, fs2, 1.0 / fs2, part);
}

int launch_rs_normal(hipStream_t st, int loss, bool cost_only, const double* points, const double* uvs, const unsigned char* mask, size_t P, int n, const int* ids, const TcCam* tcs, double f_scale,
                     double* part, double* sys) {
  const size_t nblk = hyp_point_blocks(P);
  const dim3 grid((unsigned)nblk, (unsigned)n);
  const double fs2 = f_scale * f_scale;
  switch (loss) {
    case LOSS_LINEAR: rs_normal_launch<LOSS_LINEAR>(st, cost_only, grid, points, uvs, mask, P, ids, tcs, fs2, part); break;
    case LOSS_SOFT_L1: rs_normal_launch<LOSS_SOFT_L1>(st, cost_only, grid, points, uvs, mask, P, ids, tcs, fs2, part); break;
    case LOSS_HUBER: rs_normal_launch<LOSS_HUBER>(st, cost_only, grid, points, uvs, mask, P, ids, tcs, fs2, part); break;
    case LOSS_CAUCHY: rs_normal_launch<LOSS_CAUCHY>(st, cost_only, grid, points, uvs, mask, P, ids, tcs, fs2, part); break;
    case LOSS_ARCTAN: rs_normal_launch<LOSS_ARCTAN>(st, cost_only, grid, points, uvs, mask, P, ids, tcs, fs2, part); break;
    default: return 1;
  }
  k_rs_normal_finish<<<dim3((unsigned)n), dim3(64), 0, st>>>(part, nblk, cost_only ? 1 : 0, sys);
  return 0;
}

}  // namespace mcba
