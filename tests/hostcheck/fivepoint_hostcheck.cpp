// Host build of csrc/mcba_fivepoint_math.h -- the per-lane text of csrc/mcba_fivepoint.hip -- for g++: the loop over samples that the GPU
// spreads over lanes, the compaction of the live candidates in index order, and then the stages of tests/hostcheck/twoview_hostcheck.cpp on
// the packed table (included, not restated), with the arguments of mcba_two_view_ransac5 (include/mcba.h) less the device and the timing.
// tests/test_hostcheck_fivepoint.py compiles this into a shared object; with -DFP_HOSTCHECK_MAIN it is a stand-alone program that reads a
// scene file (the sanitizer build: its own main, nothing preloaded).
#include "twoview_hostcheck.cpp"
#include "../../multicam-calibration_amd/csrc/mcba_fivepoint_math.h"

extern "C" {

// the test hook: H samples of five correspondences handed in as they are (xa, xb: H x 5 x 2); diag (H x 2): sigma_5 / sigma_1, pivot ratio
void hc_fp_candidates(int H, const double* xa, const double* xb, double* E10, int* status10, int* n_live, double* diag) {
  std::vector<FpWork> w(1);
  for (int h = 0; h < H; ++h) n_live[h] = fp_candidates(xa + 10 * (size_t)h, xb + 10 * (size_t)h, w[0], E10 + 90 * (size_t)h, status10 + 10 * (size_t)h, diag ? diag + 2 * (size_t)h : nullptr);
}

// Returns 0, or 1 for an argument out of range (nothing written).  Tables in slot order (10 H rows); map (10 H ints): the slot of every packed
// candidate, n_packed of them (one void row where nothing is live).
int hc_two_view_ransac5(size_t M, const double* uv_a, const double* uv_b, const double* cam12, const double* dist5, int H, const int* samples, double threshold, int und_iters, double* rt12,
                        double* best4, unsigned char* inliers, double* points, double* essential_out, double* cost_out, unsigned* count_out, int* status_out, int* map_out, int* n_packed) {
  if (M < 8 || H < 1 || H > 1024 || !(threshold > 0.0)) return 1;
  for (int h = 0; h < H; ++h)
    for (int k = 0; k < 5; ++k) {
      const int s = samples[5 * (size_t)h + k];
      if (s < 0 || (size_t)s >= M) return 1;
      for (int j = 0; j < k; ++j)
        if (samples[5 * (size_t)h + j] == s) return 1;
    }
  std::vector<double> prep(8 * M);
  hc_tv_prepare(M, uv_a, uv_b, cam12, dist5, und_iters, prep.data());
  const double *nax = prep.data() + 4 * M, *nay = nax + M, *nbx = nay + M, *nby = nbx + M;
  const size_t S = 10 * (size_t)H;
  std::vector<double> E10(9 * S), xa(10 * (size_t)H), xb(10 * (size_t)H);
  std::vector<int> st10(S), nl((size_t)H), map;
  for (int h = 0; h < H; ++h)
    for (int k = 0; k < 5; ++k) {
      const int s = samples[5 * (size_t)h + k];
      xa[10 * (size_t)h + 2 * k] = nax[s]; xa[10 * (size_t)h + 2 * k + 1] = nay[s]; xb[10 * (size_t)h + 2 * k] = nbx[s]; xb[10 * (size_t)h + 2 * k + 1] = nby[s];
    }
  hc_fp_candidates(H, xa.data(), xb.data(), E10.data(), st10.data(), nl.data(), nullptr);
  for (size_t s = 0; s < S; ++s)
    if (st10[s] == TV_OK) map.push_back((int)s);
  if (map.empty()) map.push_back(0);   // nothing live: slot 0 "wins" with nothing
  const int n = (int)map.size();
  std::vector<double> Ep(9 * (size_t)n), cost((size_t)n), E_back(9 * (size_t)n);
  std::vector<unsigned> count((size_t)n);
  std::vector<int> stp((size_t)n);
  for (int i = 0; i < n; ++i)
    for (int e = 0; e < 9; ++e) Ep[9 * (size_t)i + e] = E10[9 * (size_t)map[i] + e];
  if (hc_two_view_ransac(M, uv_a, uv_b, cam12, dist5, n, nullptr, Ep.data(), threshold, und_iters, rt12, best4, inliers, points, E_back.data(), cost.data(), count.data(), stp.data())) return 1;
  best4[0] = (double)map[(size_t)best4[0]];
  for (size_t s = 0; s < S; ++s) {
    if (essential_out) for (int e = 0; e < 9; ++e) essential_out[9 * s + e] = E10[9 * s + e];
    if (cost_out) cost_out[s] = __builtin_inf();
    if (count_out) count_out[s] = 0u;
    if (status_out) status_out[s] = st10[s];
  }
  for (int i = 0; i < n; ++i) {
    if (cost_out) cost_out[map[i]] = cost[i];
    if (count_out) count_out[map[i]] = count[i];
    if (map_out) map_out[i] = map[i];
  }
  if (n_packed) *n_packed = n;
  return 0;
}

}  // extern "C"

#ifdef FP_HOSTCHECK_MAIN
// scene file: int64 M, int64 H, double threshold, int64 und_iters, then uv_a (2 M), uv_b (2 M), cam12 (24), dist5 (10) doubles, samples (5 H) int32
int main(int argc, char** argv) {
  if (argc < 2) return 2;
  FILE* fh = fopen(argv[1], "rb");
  if (!fh) return 2;
  int64_t M = 0, H = 0, it = 0;
  double thr = 0.0;
  bool ok = fread(&M, 8, 1, fh) == 1 && fread(&H, 8, 1, fh) == 1 && fread(&thr, 8, 1, fh) == 1 && fread(&it, 8, 1, fh) == 1 && M >= 8 && H >= 1 && M < (1 << 24) && H <= 1024;
  if (!ok) { fclose(fh); return 2; }
  std::vector<double> ua(2 * M), ub(2 * M), cam(24), dist(10);
  std::vector<int> smp(5 * H);
  ok = fread(ua.data(), 8, ua.size(), fh) == ua.size() && fread(ub.data(), 8, ub.size(), fh) == ub.size() && fread(cam.data(), 8, 24, fh) == 24 && fread(dist.data(), 8, 10, fh) == 10 &&
       fread(smp.data(), 4, smp.size(), fh) == smp.size();
  fclose(fh);
  if (!ok) return 2;
  std::vector<double> rt(12), best(4), pts(3 * M), E(90 * H), cost(10 * H);
  std::vector<unsigned char> inl(M);
  std::vector<unsigned> cnt(10 * H);
  std::vector<int> st(10 * H), map(10 * H);
  int n = 0;
  if (hc_two_view_ransac5((size_t)M, ua.data(), ub.data(), cam.data(), dist.data(), (int)H, smp.data(), thr, (int)it, rt.data(), best.data(), inl.data(), pts.data(), E.data(), cost.data(), cnt.data(),
                          st.data(), map.data(), &n))
    return 3;
  printf("winner %d cost %.17g inliers %d in front %d packed %d\n", (int)best[0], best[1], (int)best[2], (int)best[3], n);
  return 0;
}
#endif
