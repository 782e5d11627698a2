// mcba_twoview_api.hip -- mcba_two_view_ransac and mcba_two_view_ransac5 (section 8f-17) of include/mcba.h: stateless, host arrays in and out, a device ordinal,
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

// The five-point generator: the candidate table of 10 H slots and its packed form come from csrc/mcba_fivepoint.hip;
// the packed count comes back to the host (it sizes the grids), and from there on the launches are mcba_two_view_ransac's on the packed table.
int mcba_two_view_ransac5(size_t n_points, const double* uv_a, const double* uv_b, const double* cam12, const double* dist5, int n_samples, const int* samples, double threshold,
                          int undistort_iterations, int device, double* rt12, double* best4, unsigned char* inliers, double* points, double* essential_out, double* cost_out, unsigned* count_out,
                          int* status_out, double* kernel_ms) {
  if (!uv_a || !uv_b || !cam12 || !dist5 || !rt12 || !best4 || !inliers || !points || !samples || undistort_iterations < 0)
    return fail(MCBA_ERR_ARG, "mcba_two_view_ransac5: non-NULL arrays, undistort_iterations >= 0 required");
  if (n_points < 8) return fail(MCBA_ERR_ARG, "mcba_two_view_ransac5: at least 8 common points required");
  if (n_samples < 1 || n_samples > MCBA_TWOVIEW5_MAX_SAMPLES) return fail(MCBA_ERR_ARG, "mcba_two_view_ransac5: 1 .. MCBA_TWOVIEW5_MAX_SAMPLES (1024) samples required");
  if (!(threshold > 0.0)) return fail(MCBA_ERR_ARG, "mcba_two_view_ransac5: threshold (pixels) must be positive");
  const int H = n_samples;
  const size_t M = n_points, S = (size_t)MCBA_TWOVIEW5_SLOTS * H;
  for (int h = 0; h < H; ++h) {
    const int* s = samples + MCBA_TWOVIEW5_SAMPLE * (size_t)h;
    for (int k = 0; k < MCBA_TWOVIEW5_SAMPLE; ++k) {
      if (s[k] < 0 || (size_t)s[k] >= M) return fail(MCBA_ERR_ARG, "mcba_two_view_ransac5: a sample index is outside 0 .. n_points - 1");
      for (int j = 0; j < k; ++j)
        if (s[j] == s[k]) return fail(MCBA_ERR_ARG, "mcba_two_view_ransac5: an index is repeated within a sample");
    }
  }
  if (int rc = stateless_device(device)) return rc;
  mcba::TvCams cams;
  for (int i = 0; i < 4; ++i) { cams.ka[i] = cam12[i]; cams.kb[i] = cam12[12 + i]; }
  for (int i = 0; i < 5; ++i) { cams.da[i] = dist5[i]; cams.db[i] = dist5[5 + i]; }
  const size_t nblk = mcba::tv_score_blocks(M), nblk2 = mcba::tv_pose_blocks(M);
  StatelessCall call;
  double *d_ua = nullptr, *d_ub = nullptr, *d_prep = nullptr, *d_E10 = nullptr, *d_F10 = nullptr, *d_E = nullptr, *d_F = nullptr, *d_pc = nullptr, *d_cost = nullptr, *d_best = nullptr, *d_cand = nullptr,
         *d_rt = nullptr, *d_pts = nullptr;
  int *d_smp = nullptr, *d_st10 = nullptr, *d_st = nullptr, *d_map = nullptr, *d_n = nullptr, *d_win = nullptr;
  unsigned *d_pn = nullptr, *d_cnt = nullptr, *d_pf = nullptr;
  unsigned char* d_inl = nullptr;
  if (int rc = call.upload(&d_ua, uv_a, 2 * M)) return rc;
  if (int rc = call.upload(&d_ub, uv_b, 2 * M)) return rc;
  if (int rc = call.upload(&d_smp, samples, MCBA_TWOVIEW5_SAMPLE * (size_t)H)) return rc;
  if (int rc = call.scratch(&d_prep, 8 * M)) return rc;
  if (int rc = call.scratch(&d_E10, 9 * S)) return rc;
  if (int rc = call.scratch(&d_F10, 9 * S)) return rc;
  if (int rc = call.scratch(&d_st10, S)) return rc;
  if (int rc = call.scratch(&d_E, 9 * S)) return rc;
  if (int rc = call.scratch(&d_F, 9 * S)) return rc;
  if (int rc = call.scratch(&d_st, S)) return rc;
  if (int rc = call.scratch(&d_map, S)) return rc;
  if (int rc = call.scratch(&d_n, (size_t)1)) return rc;
  if (int rc = call.scratch(&d_cost, S)) return rc;
  if (int rc = call.scratch(&d_cnt, S)) return rc;
  if (int rc = call.scratch(&d_win, (size_t)2)) return rc;
  if (int rc = call.scratch(&d_best, (size_t)4)) return rc;
  if (int rc = call.scratch(&d_cand, (size_t)48)) return rc;
  if (int rc = call.scratch(&d_pf, 4 * nblk2)) return rc;
  if (int rc = call.scratch(&d_rt, (size_t)12)) return rc;
  if (int rc = call.scratch(&d_inl, M)) return rc;
  if (int rc = call.scratch(&d_pts, 3 * M)) return rc;
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
  mcba::launch_tv5_hypotheses(nullptr, d_prep, M, d_smp, H, cams, d_E10, d_F10, d_st10, d_E, d_F, d_st, d_map, d_n);
  if (int rc = check_launch()) return rc;
  int n = 0;   // the packed count sizes the launches below: one small copy, which also waits for the generator
  if (int rc = call.download(&n, d_n, (size_t)1)) return rc;
  if (n < 1 || (size_t)n > S) return fail(MCBA_ERR_HIP, "mcba_two_view_ransac5: the packed count is out of range");
  if (int rc = call.scratch(&d_pc, nblk * (size_t)n)) return rc;
  if (int rc = call.scratch(&d_pn, nblk * (size_t)n)) return rc;
  HIPCHK(hipEventRecord(ev[1], nullptr));
  mcba::launch_tv_score(nullptr, d_prep, M, d_F, n, threshold, d_pc, d_pn);
  if (int rc = check_launch()) return rc;
  HIPCHK(hipEventRecord(ev[2], nullptr));
  mcba::launch_tv_finish(nullptr, d_pc, d_pn, nblk, n, d_E, d_st, d_cost, d_cnt, d_win, d_best, d_cand);
  if (int rc = check_launch()) return rc;
  HIPCHK(hipEventRecord(ev[3], nullptr));
  mcba::launch_tv_pose(nullptr, d_prep, M, d_F, d_st, threshold, d_cand, d_pf, d_win, d_best, d_rt, d_inl, d_pts);
  if (int rc = check_launch()) return rc;
  double total = 0.0;
  HIPCHK(call.stop(&total));
  std::vector<int> map((size_t)n);
  std::vector<double> cost;
  std::vector<unsigned> count;
  double best[4];
  if (int rc = call.download(map.data(), d_map, (size_t)n)) return rc;
  if (int rc = call.download(best, d_best, (size_t)4)) return rc;
  if (!(best[0] >= 0.0 && best[0] < (double)n)) return fail(MCBA_ERR_HIP, "mcba_two_view_ransac5: the winner's index is out of range");
  if (cost_out) { cost.resize((size_t)n); if (int rc = call.download(cost.data(), d_cost, (size_t)n)) return rc; }
  if (count_out) { count.resize((size_t)n); if (int rc = call.download(count.data(), d_cnt, (size_t)n)) return rc; }
  for (int i = 0; i < n; ++i)
    if (map[(size_t)i] < 0 || (size_t)map[(size_t)i] >= S) return fail(MCBA_ERR_HIP, "mcba_two_view_ransac5: a packed row maps outside the table");
  if (kernel_ms) {
    const hipEvent_t seq[6] = {call.e0, ev[0], ev[1], ev[2], ev[3], call.e1};
    double ms6[6] = {total, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int i = 0; i < 5; ++i) {
      float ms = 0.f;
      HIPCHK(hipEventElapsedTime(&ms, seq[i], seq[i + 1]));
      ms6[1 + i] = ms;
    }
    for (int i = 0; i < 6; ++i) kernel_ms[i] = ms6[i];
  }
  if (int rc = call.download(rt12, d_rt, (size_t)12)) return rc;
  if (int rc = call.download(inliers, d_inl, M)) return rc;
  if (int rc = call.download(points, d_pts, 3 * M)) return rc;
  best4[0] = (double)map[(size_t)best[0]]; best4[1] = best[1]; best4[2] = best[2]; best4[3] = best[3];
  if (essential_out)
    if (int rc = call.download(essential_out, d_E10, 9 * S)) return rc;
  if (status_out)
    if (int rc = call.download(status_out, d_st10, S)) return rc;
  if (cost_out) {
    for (size_t s = 0; s < S; ++s) cost_out[s] = __builtin_inf();
    for (int i = 0; i < n; ++i) cost_out[map[(size_t)i]] = cost[(size_t)i];
  }
  if (count_out) {
    for (size_t s = 0; s < S; ++s) count_out[s] = 0u;
    for (int i = 0; i < n; ++i) count_out[map[(size_t)i]] = count[(size_t)i];
  }
  return MCBA_OK;
}

}  // extern "C"
