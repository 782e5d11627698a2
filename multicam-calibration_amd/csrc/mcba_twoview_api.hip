// mcba_twoview_api.hip -- mcba_two_view_ransac of include/mcba.h: stateless, host arrays in and out, a device ordinal,
// no handle.  The correspondences and the samples go up once; the five stages of csrc/mcba_twoview.hip run on that copy, each between two events.
#include "mcba_handle.h"

using namespace mcba_internal;

extern "C" {

int mcba_two_view_ransac(size_t n_points, const double* uv_a, const double* uv_b, const double* cam12, const double* dist5, int n_hypotheses, const int* samples, const double* essential_in,
                         double threshold, int undistort_iterations, int device, double* rt12, double* best4, unsigned char* inliers, double* points, double* essential_out, double* cost_out,
                         unsigned* count_out, int* status_out, double* kernel_ms) {
  if (!uv_a || !uv_b || !cam12 || !dist5 || !rt12 || !best4 || !inliers || !points || (!samples && !essential_in) || undistort_iterations < 0)
    return fail(MCBA_ERR_ARG, "mcba_two_view_ransac: non-NULL arrays (samples or essential_in), undistort_iterations >= 0 required");
  if (n_points < 8) return fail(MCBA_ERR_ARG, "mcba_two_view_ransac: at least 8 common points required");
  if (n_hypotheses < 1 || n_hypotheses > MCBA_TWOVIEW_MAX_HYPOTHESES) return fail(MCBA_ERR_ARG, "mcba_two_view_ransac: 1 .. MCBA_TWOVIEW_MAX_HYPOTHESES (4096) hypotheses required");
  if (!(threshold > 0.0)) return fail(MCBA_ERR_ARG, "mcba_two_view_ransac: threshold (pixels) must be positive");
  const int H = n_hypotheses;
  const size_t M = n_points;
  if (samples && !essential_in)
    for (int h = 0; h < H; ++h) {
      const int* s = samples + 8 * (size_t)h;
      for (int k = 0; k < 8; ++k) {
        if (s[k] < 0 || (size_t)s[k] >= M) return fail(MCBA_ERR_ARG, "mcba_two_view_ransac: a sample index is outside 0 .. n_points - 1");
        for (int j = 0; j < k; ++j)
          if (s[j] == s[k]) return fail(MCBA_ERR_ARG, "mcba_two_view_ransac: an index is repeated within a sample");
      }
    }
  if (int rc = stateless_device(device)) return rc;
  mcba::TvCams cams;
  for (int i = 0; i < 4; ++i) { cams.ka[i] = cam12[i]; cams.kb[i] = cam12[12 + i]; }
  for (int i = 0; i < 5; ++i) { cams.da[i] = dist5[i]; cams.db[i] = dist5[5 + i]; }
  const size_t nblk = mcba::tv_score_blocks(M), nblk2 = mcba::tv_pose_blocks(M);
  StatelessCall call;
  double *d_ua = nullptr, *d_ub = nullptr, *d_ein = nullptr, *d_prep = nullptr, *d_E = nullptr, *d_F = nullptr, *d_pc = nullptr, *d_cost = nullptr, *d_best = nullptr, *d_cand = nullptr, *d_rt = nullptr,
         *d_pts = nullptr;
  int *d_smp = nullptr, *d_st = nullptr, *d_win = nullptr;
  unsigned *d_pn = nullptr, *d_cnt = nullptr, *d_pf = nullptr;
  unsigned char* d_inl = nullptr;
  if (int rc = call.upload(&d_ua, uv_a, 2 * M)) return rc;
  if (int rc = call.upload(&d_ub, uv_b, 2 * M)) return rc;
  if (essential_in) {
    if (int rc = call.upload(&d_ein, essential_in, 9 * (size_t)H)) return rc;
  } else if (int rc = call.upload(&d_smp, samples, 8 * (size_t)H)) return rc;
  if (int rc = call.scratch(&d_prep, 8 * M)) return rc;
  if (int rc = call.scratch(&d_E, 9 * (size_t)H)) return rc;
  if (int rc = call.scratch(&d_F, 9 * (size_t)H)) return rc;
  if (int rc = call.scratch(&d_st, (size_t)H)) return rc;
  if (int rc = call.scratch(&d_pc, nblk * H)) return rc;
  if (int rc = call.scratch(&d_pn, nblk * H)) return rc;
  if (int rc = call.scratch(&d_cost, (size_t)H)) return rc;
  if (int rc = call.scratch(&d_cnt, (size_t)H)) return rc;
  if (int rc = call.scratch(&d_win, (size_t)2)) return rc;
  if (int rc = call.scratch(&d_best, (size_t)4)) return rc;
  if (int rc = call.scratch(&d_cand, (size_t)48)) return rc;
  if (int rc = call.scratch(&d_pf, 4 * nblk2)) return rc;
  if (int rc = call.scratch(&d_rt, (size_t)12)) return rc;
  if (int rc = call.scratch(&d_inl, M)) return rc;
  if (int rc = call.scratch(&d_pts, 3 * M)) return rc;
  // the call's own events bracket the whole; four more separate the stages
  hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
  struct EventGuard {
    hipEvent_t* e;
    ~EventGuard() { for (int i = 0; i < 4; ++i) if (e[i]) (void)hipEventDestroy(e[i]); }
  } guard{ev};
  for (int i = 0; i < 4; ++i) HIPCHK(hipEventCreate(&ev[i]));
  HIPCHK(call.start());
  mcba::launch_tv_prepare(nullptr, d_ua, d_ub, M, cams, undistort_iterations, d_prep);
  if (int rc = check_launch()) return rc;
  HIPCHK(hipEventRecord(ev[0], nullptr));
  mcba::launch_tv_hypotheses(nullptr, d_prep, M, d_smp, H, d_ein, cams, d_E, d_F, d_st);
  if (int rc = check_launch()) return rc;
  HIPCHK(hipEventRecord(ev[1], nullptr));
  mcba::launch_tv_score(nullptr, d_prep, M, d_F, H, threshold, d_pc, d_pn);
  if (int rc = check_launch()) return rc;
  HIPCHK(hipEventRecord(ev[2], nullptr));
  mcba::launch_tv_finish(nullptr, d_pc, d_pn, nblk, H, d_E, d_st, d_cost, d_cnt, d_win, d_best, d_cand);
  if (int rc = check_launch()) return rc;
  HIPCHK(hipEventRecord(ev[3], nullptr));
  mcba::launch_tv_pose(nullptr, d_prep, M, d_F, d_st, threshold, d_cand, d_pf, d_win, d_best, d_rt, d_inl, d_pts);
  if (int rc = check_launch()) return rc;
  double total = 0.0;
  HIPCHK(call.stop(&total));
  if (kernel_ms) {
    const hipEvent_t seq[6] = {call.e0, ev[0], ev[1], ev[2], ev[3], call.e1};
    kernel_ms[0] = total;
    for (int i = 0; i < 5; ++i) {
      float ms = 0.f;
      HIPCHK(hipEventElapsedTime(&ms, seq[i], seq[i + 1]));
      kernel_ms[1 + i] = ms;
    }
  }
  if (int rc = call.download(rt12, d_rt, (size_t)12)) return rc;
  if (int rc = call.download(best4, d_best, (size_t)4)) return rc;
  if (int rc = call.download(inliers, d_inl, M)) return rc;
  if (int rc = call.download(points, d_pts, 3 * M)) return rc;
  if (essential_out)
    if (int rc = call.download(essential_out, d_E, 9 * (size_t)H)) return rc;
  if (cost_out)
    if (int rc = call.download(cost_out, d_cost, (size_t)H)) return rc;
  if (count_out)
    if (int rc = call.download(count_out, d_cnt, (size_t)H)) return rc;
  if (status_out)
    if (int rc = call.download(status_out, d_st, (size_t)H)) return rc;
  return MCBA_OK;
}

}  // extern "C"
