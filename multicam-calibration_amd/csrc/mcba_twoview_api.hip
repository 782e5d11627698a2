// mcba_twoview_api.hip -- mcba_two_view_ransac and mcba_two_view_ransac5 (section 8f-17) of include/mcba.h: stateless, host arrays in and out, a device ordinal,
// no handle.  The correspondences and the samples go up once; the five stages of csrc/mcba_twoview.hip run on that copy, each between two events.  The two entries are one body
// (two_view_ransac) that differs in the generator it launches: k_tv_hypotheses, or k_tv5_hypotheses of csrc/mcba_fivepoint.hip with ten table slots per sample, packed before the scorer.
#include "mcba_handle.h"
#include "mcba_ransac_host.h"

using namespace mcba_internal;

namespace {

constexpr mcba::Generator kEight{"mcba_two_view_ransac", 8, 1, MCBA_TWOVIEW_MAX_HYPOTHESES, ": 1 .. MCBA_TWOVIEW_MAX_HYPOTHESES (4096) hypotheses required"};
constexpr mcba::Generator kFive{"mcba_two_view_ransac5", MCBA_TWOVIEW5_SAMPLE, MCBA_TWOVIEW5_SLOTS, MCBA_TWOVIEW5_MAX_SAMPLES, ": 1 .. MCBA_TWOVIEW5_MAX_SAMPLES (1024) samples required"};

mcba::TvCams tv_cams_of(const double* cam12, const double* dist5) {
  mcba::TvCams cams;
  for (int i = 0; i < 4; ++i) { cams.ka[i] = cam12[i]; cams.kb[i] = cam12[12 + i]; }
  for (int i = 0; i < 5; ++i) { cams.da[i] = dist5[i]; cams.db[i] = dist5[5 + i]; }
  return cams;
}

// The body of mcba_two_view_ransac and mcba_two_view_ransac5: the checks, the upload, the stages between their events, the download.
// n_hypotheses counts samples; the table has S = n_hypotheses g.slots slots.  The five-point generator (g.slots > 1) packs the live slots of its
// table: the packed count comes back to the host (it sizes the grids), the launches from there on see the packed rows, and what is reported per
// hypothesis goes back to slot order through the map.
int two_view_ransac(const mcba::Generator& g, size_t n_points, const double* uv_a, const double* uv_b, const double* cam12, const double* dist5, int n_hypotheses, const int* samples,
                    const double* essential_in, double threshold, int undistort_iterations, int device, double* rt12, double* best4, unsigned char* inliers, double* points, double* essential_out,
                    double* cost_out, unsigned* count_out, int* status_out, double* kernel_ms) {
  auto bad = [&](int code, const char* what) { return fail(code, (std::string(g.who) + what).c_str()); };
  const bool packed = g.slots > 1;
  if (!uv_a || !uv_b || !cam12 || !dist5 || !rt12 || !best4 || !inliers || !points || (!samples && !essential_in) || undistort_iterations < 0)
    return bad(MCBA_ERR_ARG, packed ? ": non-NULL arrays, undistort_iterations >= 0 required" : ": non-NULL arrays (samples or essential_in), undistort_iterations >= 0 required");
  if (n_points < 8) return bad(MCBA_ERR_ARG, ": at least 8 common points required");
  if (n_hypotheses < 1 || n_hypotheses > g.max_h) return bad(MCBA_ERR_ARG, g.range);
  if (!(threshold > 0.0)) return bad(MCBA_ERR_ARG, ": threshold (pixels) must be positive");
  const int H = n_hypotheses;
  const size_t M = n_points, S = (size_t)g.slots * H;
  std::string msg;
  if (!essential_in && !mcba::samples_ok(g.who, samples, (size_t)H, g.size, M, nullptr, &msg)) return fail(MCBA_ERR_ARG, msg.c_str());
  if (int rc = stateless_device(device)) return rc;
  const mcba::TvCams cams = tv_cams_of(cam12, dist5);
  const size_t nblk = mcba::hyp_score_blocks(M), nblk2 = mcba::hyp_point_blocks(M);
  StatelessCall call;
  // E, F, st: the table the scorer sees; E10, F10, st10, map, n: the five-point generator's table in slot order, the packed rows' slots, their count
  double *d_ua = nullptr, *d_ub = nullptr, *d_ein = nullptr, *d_prep = nullptr, *d_E10 = nullptr, *d_F10 = nullptr, *d_E = nullptr, *d_F = nullptr, *d_pc = nullptr, *d_cost = nullptr, *d_best = nullptr,
         *d_cand = nullptr, *d_rt = nullptr, *d_pts = nullptr;
  int *d_smp = nullptr, *d_st10 = nullptr, *d_st = nullptr, *d_map = nullptr, *d_n = nullptr, *d_win = nullptr;
  unsigned *d_pn = nullptr, *d_cnt = nullptr, *d_pf = nullptr;
  unsigned char* d_inl = nullptr;
  if (int rc = call.upload(&d_ua, uv_a, 2 * M)) return rc;
  if (int rc = call.upload(&d_ub, uv_b, 2 * M)) return rc;
  if (essential_in) {
    if (int rc = call.upload(&d_ein, essential_in, 9 * S)) return rc;
  } else if (int rc = call.upload(&d_smp, samples, g.size * (size_t)H)) return rc;
  if (int rc = call.scratch(&d_prep, 8 * M)) return rc;
  if (packed) {
    if (int rc = call.scratch(&d_E10, 9 * S)) return rc;
    if (int rc = call.scratch(&d_F10, 9 * S)) return rc;
    if (int rc = call.scratch(&d_st10, S)) return rc;
    if (int rc = call.scratch(&d_map, S)) return rc;
    if (int rc = call.scratch(&d_n, (size_t)1)) return rc;
  }
  if (int rc = call.scratch(&d_E, 9 * S)) return rc;
  if (int rc = call.scratch(&d_F, 9 * S)) return rc;
  if (int rc = call.scratch(&d_st, S)) return rc;
  if (!packed) {
    if (int rc = call.scratch(&d_pc, nblk * S)) return rc;
    if (int rc = call.scratch(&d_pn, nblk * S)) return rc;
  }
  if (int rc = call.scratch(&d_cost, S)) return rc;
  if (int rc = call.scratch(&d_cnt, S)) return rc;
  if (int rc = call.scratch(&d_win, (size_t)2)) return rc;
  if (int rc = call.scratch(&d_best, (size_t)4)) return rc;
  if (int rc = call.scratch(&d_cand, (size_t)48)) return rc;
  if (int rc = call.scratch(&d_pf, 4 * nblk2)) return rc;
  if (int rc = call.scratch(&d_rt, (size_t)12)) return rc;
  if (int rc = call.scratch(&d_inl, M)) return rc;
  if (int rc = call.scratch(&d_pts, 3 * M)) return rc;
  StageEvents<4> stages;   // the call's own events bracket the whole; four more separate the stages
  HIPCHK(stages.create());
  HIPCHK(call.start());
  mcba::launch_tv_prepare(nullptr, d_ua, d_ub, M, cams, undistort_iterations, d_prep);
  if (int rc = check_launch()) return rc;
  HIPCHK(stages.mark());
  int n = H;   // the rows the scorer sees
  if (!packed) {
    mcba::launch_tv_hypotheses(nullptr, d_prep, M, d_smp, H, d_ein, cams, d_E, d_F, d_st);
    if (int rc = check_launch()) return rc;
  } else {
    mcba::launch_tv5_hypotheses(nullptr, d_prep, M, d_smp, H, cams, d_E10, d_F10, d_st10, d_E, d_F, d_st, d_map, d_n);
    if (int rc = check_launch()) return rc;
    // the packed count sizes the launches below: one small copy, which also waits for the generator
    if (int rc = call.download(&n, d_n, (size_t)1)) return rc;
    if (n < 1 || (size_t)n > S) return bad(MCBA_ERR_HIP, ": the packed count is out of range");
    if (int rc = call.scratch(&d_pc, nblk * (size_t)n)) return rc;
    if (int rc = call.scratch(&d_pn, nblk * (size_t)n)) return rc;
  }
  HIPCHK(stages.mark());
  mcba::launch_tv_score(nullptr, d_prep, M, d_F, n, threshold, d_pc, d_pn);
  if (int rc = check_launch()) return rc;
  HIPCHK(stages.mark());
  mcba::launch_tv_finish(nullptr, d_pc, d_pn, nblk, n, d_E, d_st, d_cost, d_cnt, d_win, d_best, d_cand);
  if (int rc = check_launch()) return rc;
  HIPCHK(stages.mark());
  mcba::launch_tv_pose(nullptr, d_prep, M, d_F, d_st, threshold, d_cand, d_pf, d_win, d_best, d_rt, d_inl, d_pts);
  if (int rc = check_launch()) return rc;
  double total = 0.0;
  HIPCHK(call.stop(&total));
  // packed rows: everything that is checked comes down before the first output is written
  std::vector<int> map;
  std::vector<double> cost;
  std::vector<unsigned> count;
  double best[4];
  if (int rc = call.download(best, d_best, (size_t)4)) return rc;
  if (packed) {
    map.resize((size_t)n);
    if (int rc = call.download(map.data(), d_map, (size_t)n)) return rc;
    if (!(best[0] >= 0.0 && best[0] < (double)n)) return bad(MCBA_ERR_HIP, ": the winner's index is out of range");
    if (cost_out) { cost.resize((size_t)n); if (int rc = call.download(cost.data(), d_cost, (size_t)n)) return rc; }
    if (count_out) { count.resize((size_t)n); if (int rc = call.download(count.data(), d_cnt, (size_t)n)) return rc; }
    for (int i = 0; i < n; ++i)
      if (map[(size_t)i] < 0 || (size_t)map[(size_t)i] >= S) return bad(MCBA_ERR_HIP, ": a packed row maps outside the table");
  }
  if (kernel_ms) HIPCHK(stages.fill(call, total, kernel_ms));
  if (int rc = call.download(rt12, d_rt, (size_t)12)) return rc;
  if (int rc = call.download(inliers, d_inl, M)) return rc;
  if (int rc = call.download(points, d_pts, 3 * M)) return rc;
  best4[0] = packed ? (double)map[(size_t)best[0]] : best[0]; best4[1] = best[1]; best4[2] = best[2]; best4[3] = best[3];
  if (essential_out)
    if (int rc = call.download(essential_out, packed ? d_E10 : d_E, 9 * S)) return rc;
  if (status_out)
    if (int rc = call.download(status_out, packed ? d_st10 : d_st, S)) return rc;
  if (!packed) {
    if (cost_out)
      if (int rc = call.download(cost_out, d_cost, S)) return rc;
    if (count_out)
      if (int rc = call.download(count_out, d_cnt, S)) return rc;
    return MCBA_OK;
  }
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

}  // namespace

extern "C" {

int mcba_two_view_ransac(size_t n_points, const double* uv_a, const double* uv_b, const double* cam12, const double* dist5, int n_hypotheses, const int* samples, const double* essential_in,
                         double threshold, int undistort_iterations, int device, double* rt12, double* best4, unsigned char* inliers, double* points, double* essential_out, double* cost_out,
                         unsigned* count_out, int* status_out, double* kernel_ms) {
  return two_view_ransac(kEight, n_points, uv_a, uv_b, cam12, dist5, n_hypotheses, samples, essential_in, threshold, undistort_iterations, device, rt12, best4, inliers, points, essential_out, cost_out,
                         count_out, status_out, kernel_ms);
}

int mcba_two_view_ransac5(size_t n_points, const double* uv_a, const double* uv_b, const double* cam12, const double* dist5, int n_samples, const int* samples, double threshold,
                          int undistort_iterations, int device, double* rt12, double* best4, unsigned char* inliers, double* points, double* essential_out, double* cost_out, unsigned* count_out,
                          int* status_out, double* kernel_ms) {
  return two_view_ransac(kFive, n_points, uv_a, uv_b, cam12, dist5, n_samples, samples, nullptr, threshold, undistort_iterations, device, rt12, best4, inliers, points, essential_out, cost_out, count_out,
                         status_out, kernel_ms);
}

}  // extern "C"
