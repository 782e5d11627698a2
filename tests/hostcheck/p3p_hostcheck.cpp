// Host build of csrc/mcba_resect_p3p_math.h -- the per-lane text of k_rs3_hypotheses (csrc/mcba_resect_p3p.hip) -- for g++: the loop over the
// samples of one camera that the GPU spreads over lanes.  The table it fills goes to the scorer of tests/hostcheck/resection_hostcheck.cpp
// (hc_resect_ransac with poses_in), which tests/test_hostcheck_p3p.py links beside this file.  With -DP3P_HOSTCHECK_MAIN it is a stand-alone
// program that reads a scene file (the sanitizer build: its own main, nothing preloaded).
#include <cstddef>
#include <cstdio>
#include <cstdint>
#include <vector>
#include "../../multicam-calibration_amd/csrc/mcba_resect_p3p_math.h"

using namespace mcba;

extern "C" {

void hc_rs_prepare(size_t P, const double* points, const double* uv, const double* cam12, const double* dist5, int und_iters, double* out4, unsigned char* usable);
int hc_resect_ransac(size_t P, const double* points, const double* uv, const double* cam12, const double* dist5, int H, const int* samples, const double* poses_in, double threshold, int und_iters,
                     double* rt12, double* best4, unsigned char* inliers, double* pose_out, double* cost_out, unsigned* count_out, int* status_out);

// One camera, H samples (H, 3) -> pose_out (4 H, 12), status_out (4 H), step_out (4 H, 6) or NULL.  Returns 0, or 1 for an argument out of
// range (nothing written): H outside 1 .. 1024, an index outside 0 .. P - 1, not usable or repeated within a sample.
int hc_p3p_candidates(size_t P, const double* points, const double* uv, const double* cam12, const double* dist5, int H, const int* samples, int und_iters, double* pose_out, int* status_out,
                      double* step_out) {
  if (P < 1 || H < 1 || H > 1024 || !samples) return 1;
  std::vector<double> prep(4 * P);
  std::vector<unsigned char> use(P);
  hc_rs_prepare(P, points, uv, cam12, dist5, und_iters, prep.data(), use.data());
  for (int h = 0; h < H; ++h)
    for (int k = 0; k < kP3Sample; ++k) {
      const int s = samples[kP3Sample * h + k];
      if (s < 0 || (size_t)s >= P || !use[s]) return 1;
      for (int i = 0; i < k; ++i)
        if (samples[kP3Sample * h + i] == s) return 1;
    }
  const double *nx = prep.data() + 2 * P, *ny = nx + P;
  for (int h = 0; h < H; ++h) {
    double X[9], x[6], step[6 * kP3Slots];
    for (int k = 0; k < kP3Sample; ++k) {
      const int s = samples[kP3Sample * h + k];
      for (int i = 0; i < 3; ++i) X[3 * k + i] = points[3 * (size_t)s + i];
      x[2 * k] = nx[s]; x[2 * k + 1] = ny[s];
    }
    P3Roots r;
    p3_roots(X, x, r);
    for (int k = 0; k < kP3Slots; ++k) status_out[kP3Slots * (size_t)h + k] = p3_candidate(X, x, r, k, pose_out + 12 * (kP3Slots * (size_t)h + k), step + 6 * k);
    if (step_out)
      for (int i = 0; i < 6 * kP3Slots; ++i) step_out[6 * kP3Slots * (size_t)h + i] = step[i];
  }
  return 0;
}

// the real roots of a quartic (5 coefficients, ascending): the count, roots[0 .. 3]
int hc_p3p_roots(const double* a, double* roots) { return p3_real_roots4(a, roots); }

}  // extern "C"

#ifdef P3P_HOSTCHECK_MAIN
// scene file: int64 P, int64 H, double threshold, int64 und_iters, then points (3 P), uv (2 P), cam12 (12), dist5 (5) doubles, samples (3 H) int32.
// Runs the generator, then the scorer on its table.
int main(int argc, char** argv) {
  if (argc < 2) return 2;
  FILE* fh = fopen(argv[1], "rb");
  if (!fh) return 2;
  int64_t P = 0, H = 0, it = 0;
  double thr = 0.0;
  bool ok = fread(&P, 8, 1, fh) == 1 && fread(&H, 8, 1, fh) == 1 && fread(&thr, 8, 1, fh) == 1 && fread(&it, 8, 1, fh) == 1 && P >= 6 && H >= 1 && P < (1 << 24) && H <= 1024;
  if (!ok) { fclose(fh); return 2; }
  std::vector<double> pts(3 * P), uv(2 * P), cam(12), dist(5);
  std::vector<int> smp(3 * H);
  ok = fread(pts.data(), 8, pts.size(), fh) == pts.size() && fread(uv.data(), 8, uv.size(), fh) == uv.size() && fread(cam.data(), 8, 12, fh) == 12 && fread(dist.data(), 8, 5, fh) == 5 &&
       fread(smp.data(), 4, smp.size(), fh) == smp.size();
  fclose(fh);
  if (!ok) return 2;
  const int64_t S = kP3Slots * H;
  std::vector<double> table(12 * S), rt(12), best(4), pose(12 * S), cost(S);
  std::vector<int> st(S), st2(S);
  std::vector<unsigned char> inl(P);
  std::vector<unsigned> cnt(S);
  if (hc_p3p_candidates((size_t)P, pts.data(), uv.data(), cam.data(), dist.data(), (int)H, smp.data(), (int)it, table.data(), st.data(), nullptr)) return 3;
  int live = 0;
  for (int64_t i = 0; i < S; ++i) live += st[i] == RS_OK;
  if (hc_resect_ransac((size_t)P, pts.data(), uv.data(), cam.data(), dist.data(), (int)S, nullptr, table.data(), thr, (int)it, rt.data(), best.data(), inl.data(), pose.data(), cost.data(), cnt.data(),
                       st2.data()))
    return 4;
  printf("live %d of %d slots; winner %d cost %.17g inliers %d usable %d\n", live, (int)S, (int)best[0], best[1], (int)best[2], (int)best[3]);
  return 0;
}
#endif
