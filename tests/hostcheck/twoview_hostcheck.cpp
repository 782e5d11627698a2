// Host build of csrc/mcba_twoview_math.h -- the per-lane text of csrc/mcba_twoview.hip -- for g++: the loops over points, hypotheses and
// candidates that the GPU spreads over lanes, with the arguments of mcba_two_view_ransac (include/mcba.h) less the device and the timing.
// The sums run in index order here; the kernels' order is their own, and both are held to the bounds of tests/twoview_oracle.py.
// tests/test_hostcheck_twoview.py compiles this into a shared object; with -DTV_HOSTCHECK_MAIN it is a stand-alone program that reads a scene
// file (the sanitizer build: its own main, nothing preloaded).
#include <cstddef>
#include <cstdio>
#include <cstdint>
#include <vector>
#include "../../multicam-calibration_amd/csrc/mcba_twoview_math.h"
#include "../../multicam-calibration_amd/csrc/mcba_ransac_host.h"

using namespace mcba;

static void intrinsics_of(const double* cam12, const double* dist5, double ka[4], double da[5], double kb[4], double db[5]) {
  for (int i = 0; i < 4; ++i) { ka[i] = cam12[i]; kb[i] = cam12[12 + i]; }
  for (int i = 0; i < 5; ++i) { da[i] = dist5[i]; db[i] = dist5[5 + i]; }
}

extern "C" {

// The check that mcba_two_view_ransac and mcba_two_view_ransac5 make of their table of host-drawn samples before the upload (csrc/mcba_ransac_host.h), the same text.  usable: a byte
// per point, or NULL.  Returns 1 for a table that passes; 0 with the message in msg (cap bytes of room, NUL-terminated).
int hc_samples_ok(const char* who, const int* samples, size_t rows, int size, size_t limit, const unsigned char* usable, char* msg, size_t cap) {
  std::string m;
  const bool ok = samples_ok(who, samples, rows, size, limit, usable, &m);
  snprintf(msg, cap, "%s", m.c_str());
  return ok ? 1 : 0;
}

// out8: 8 planes of M doubles (undistorted pixels a.x a.y b.x b.y, normalised a.x a.y b.x b.y)
void hc_tv_prepare(size_t M, const double* uv_a, const double* uv_b, const double* cam12, const double* dist5, int und_iters, double* out8) {
  double ka[4], da[5], kb[4], db[5];
  intrinsics_of(cam12, dist5, ka, da, kb, db);
  for (size_t p = 0; p < M; ++p) {
    double o[8];
    tv_prepare(uv_a[2 * p], uv_a[2 * p + 1], uv_b[2 * p], uv_b[2 * p + 1], ka, da, kb, db, und_iters, o);
    for (int k = 0; k < 8; ++k) out8[k * M + p] = o[k];
  }
}

// Returns 0, or 1 for an argument out of range (nothing written).
int hc_two_view_ransac(size_t M, const double* uv_a, const double* uv_b, const double* cam12, const double* dist5, int H, const int* samples, const double* essential_in, double threshold,
                       int und_iters, double* rt12, double* best4, unsigned char* inliers, double* points, double* essential_out, double* cost_out, unsigned* count_out, int* status_out) {
  if (M < 8 || H < 1 || !(threshold > 0.0)) return 1;
  double ka[4], da[5], kb[4], db[5];
  intrinsics_of(cam12, dist5, ka, da, kb, db);
  std::vector<double> prep(8 * M);
  hc_tv_prepare(M, uv_a, uv_b, cam12, dist5, und_iters, prep.data());
  const double *pax = prep.data(), *pay = pax + M, *pbx = pay + M, *pby = pbx + M, *nax = pby + M, *nay = nax + M, *nbx = nay + M, *nby = nbx + M;
  std::vector<double> E(9 * (size_t)H), F(9 * (size_t)H), cost((size_t)H);
  std::vector<int> status((size_t)H);
  std::vector<unsigned> count((size_t)H);
  const double t2 = threshold * threshold;
  int win = 0;
  for (int h = 0; h < H; ++h) {
    double* e = E.data() + 9 * (size_t)h;
    if (essential_in) {
      bool ok = true;
      for (int i = 0; i < 9; ++i) { e[i] = essential_in[9 * (size_t)h + i]; ok = ok && fabs(e[i]) <= 1.7976931348623157e308; }
      status[h] = ok ? TV_OK : TV_VOID;
    } else {
      double xa[16], xb[16], S[81];
      for (int k = 0; k < 8; ++k) {
        const int s = samples[8 * (size_t)h + k];
        xa[2 * k] = nax[s]; xa[2 * k + 1] = nay[s]; xb[2 * k] = nbx[s]; xb[2 * k + 1] = nby[s];
      }
      status[h] = tv_essential(xa, xb, S, e);
    }
    double* f = F.data() + 9 * (size_t)h;
    tv_fundamental(e, ka, kb, f);
    double c = 0.0;
    unsigned n = 0;
    for (size_t p = 0; p < M; ++p) {
      const double e2 = tv_sampson2(f, pax[p], pay[p], pbx[p], pby[p]);
      c += tv_cost_term(e2, t2);
      n += tv_inlier(e2, t2) ? 1u : 0u;
    }
    cost[h] = status[h] == TV_OK ? c : __builtin_inf();
    count[h] = status[h] == TV_OK ? n : 0u;
    if (tv_before(cost[h], h, cost[win], win)) win = h;
  }
  double Rt[48];
  tv_candidates(E.data() + 9 * (size_t)win, Rt);
  const double* f = F.data() + 9 * (size_t)win;
  unsigned front[4] = {0, 0, 0, 0};
  for (size_t p = 0; p < M; ++p) {
    const bool in = status[win] == TV_OK && tv_inlier(tv_sampson2(f, pax[p], pay[p], pbx[p], pby[p]), t2);
    inliers[p] = in ? 1 : 0;
    for (int c = 0; c < 4; ++c) {
      double X[3];
      bool kept;
      const bool fr = tv_depths(Rt + 12 * c, nax[p], nay[p], nbx[p], nby[p], X, kept);
      front[c] += in && fr ? 1u : 0u;
    }
  }
  int bc = 0;
  for (int c = 1; c < 4; ++c) bc = front[c] > front[bc] ? c : bc;   // highest (count, -index)
  for (int i = 0; i < 12; ++i) rt12[i] = Rt[12 * bc + i];
  for (size_t p = 0; p < M; ++p) {
    double X[3];
    bool kept;
    tv_depths(Rt + 12 * bc, nax[p], nay[p], nbx[p], nby[p], X, kept);
    for (int i = 0; i < 3; ++i) points[3 * p + i] = inliers[p] && kept ? X[i] : __builtin_nan("");
  }
  best4[0] = (double)win; best4[1] = cost[win]; best4[2] = (double)count[win]; best4[3] = (double)front[bc];
  for (int h = 0; h < H; ++h) {
    if (essential_out) for (int i = 0; i < 9; ++i) essential_out[9 * (size_t)h + i] = E[9 * (size_t)h + i];
    if (cost_out) cost_out[h] = cost[h];
    if (count_out) count_out[h] = count[h];
    if (status_out) status_out[h] = status[h];
  }
  return 0;
}

}  // extern "C"

#ifdef TV_HOSTCHECK_MAIN
// scene file: int64 M, int64 H, double threshold, int64 und_iters, then uv_a (2 M), uv_b (2 M), cam12 (24), dist5 (10) doubles, samples (8 H) int32
int main(int argc, char** argv) {
  if (argc < 2) return 2;
  FILE* fh = fopen(argv[1], "rb");
  if (!fh) return 2;
  int64_t M = 0, H = 0, it = 0;
  double thr = 0.0;
  bool ok = fread(&M, 8, 1, fh) == 1 && fread(&H, 8, 1, fh) == 1 && fread(&thr, 8, 1, fh) == 1 && fread(&it, 8, 1, fh) == 1 && M >= 8 && H >= 1 && M < (1 << 24) && H < (1 << 16);
  if (!ok) { fclose(fh); return 2; }
  std::vector<double> ua(2 * M), ub(2 * M), cam(24), dist(10);
  std::vector<int> smp(8 * H);
  ok = fread(ua.data(), 8, ua.size(), fh) == ua.size() && fread(ub.data(), 8, ub.size(), fh) == ub.size() && fread(cam.data(), 8, 24, fh) == 24 && fread(dist.data(), 8, 10, fh) == 10 &&
       fread(smp.data(), 4, smp.size(), fh) == smp.size();
  fclose(fh);
  if (!ok) return 2;
  char msg[128];
  if (!hc_samples_ok("main", smp.data(), (size_t)H, 8, (size_t)M, nullptr, msg, sizeof msg)) return 6;
  std::vector<double> rt(12), best(4), pts(3 * M), E(9 * H), cost(H);
  std::vector<unsigned char> inl(M);
  std::vector<unsigned> cnt(H);
  std::vector<int> st(H);
  if (hc_two_view_ransac((size_t)M, ua.data(), ub.data(), cam.data(), dist.data(), (int)H, smp.data(), nullptr, thr, (int)it, rt.data(), best.data(), inl.data(), pts.data(), E.data(), cost.data(),
                         cnt.data(), st.data()))
    return 3;
  printf("winner %d cost %.17g inliers %d in front %d\n", (int)best[0], best[1], (int)best[2], (int)best[3]);
  return 0;
}
#endif
