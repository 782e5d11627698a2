// Host build of csrc/mcba_smooth_cov_math.h -- the per-lane text of k_smooth_selinv (csrc/mcba_smooth_cov.hip) behind k_smooth_reduce -- for g++:
// serial loops over the lanes in the kernels' order (prepare, every level up, every level down, tracks fastest), the level plan and the statuses
// of mcba_smooth_cov_api.hip.  tests/test_hostcheck_smoothing_cov.py compiles this as a shared library (plain -O2) and holds it to the GPU tier's
// bar; with -DSMOOTH_COV_HOSTCHECK_MAIN it is a stand-alone program that reads a scene file, which the same test builds with
// -fsanitize=address,undefined and runs as a child process.
#include <cmath>
#include <cstddef>
#include <cstdio>
#include <cstring>
#include <vector>
#include "../../multicam-calibration_amd/csrc/mcba_smooth_cov_math.h"

using namespace mcba;

extern "C" int hc_smooth_covariance(size_t T, int K, const double* points, const double* cov6, const double* accel_std, const double* weights, int segment, double* out_cov6, double* out_lag9,
                                    int* status, int* n_usable, double* info8) {
  if (T < 1 || K < 1 || (segment != 0 && (segment < SM_SEGMENT_MIN || segment > SM_SEGMENT_MAX))) return 1;
  if (segment == 0) segment = SM_SEGMENT_DEFAULT;
  const double nan = std::nan("");
  const size_t TK = T * K;
  SmLevel lv[SM_MAX_LEVELS];
  double* zc[SM_MAX_LEVELS];
  int levels = 0;
  std::vector<double> store(smooth_carve(T, segment, K, lv, SM_ZC, nullptr, nullptr), nan);   // NaN-filled: whatever reads a word nobody wrote shows
  if (store.empty()) return 1;
  smooth_carve(T, segment, K, lv, SM_ZC, store.data(), zc, &levels);
  std::vector<double> p(3 * TK), winv(6 * TK), w(TK), ia2(K), oc(6 * TK, nan), ol(out_lag9 ? 9 * (T - 1) * K : 0, nan);
  std::vector<int> bad(K, 0), list;
  for (int k = 0; k < K; ++k) { ia2[k] = 1.0 / (accel_std[k] * accel_std[k]); n_usable[k] = 0; }
  for (size_t i = 0; i < TK; ++i)
    if (smooth_prepare_lane(points + 3 * i, cov6 + 6 * i, weights ? weights[i] : 1.0, p.data() + 3 * i, winv.data() + 6 * i, w[i])) n_usable[i % K] += 1;
  for (int k = 0; k < K; ++k)
    if (n_usable[k] >= 2) list.push_back(k);
  SmData td{T, p.data(), winv.data(), w.data(), ia2.data(), nullptr, nullptr, nullptr, SM_LOSS_LINEAR, 1.0, 1.0};
  const SmLevel none{};
  const int nact = (int)list.size();
  if (nact > 0) {
    for (int l = 0; l < levels; ++l) {
      const int nq = smooth_lanes(lv[l]);
      const SmLevel& nx = l + 1 < levels ? lv[l + 1] : none;
      for (size_t gid = 0; gid < (size_t)nq * nact; ++gid) {
        if (l == 0) smooth_reduce_lane<true>(lv[0], nx, td, K, list[gid % nact], (int)(gid / nact), bad.data());
        else smooth_reduce_lane<false>(lv[l], nx, td, K, list[gid % nact], (int)(gid / nact), bad.data());
      }
    }
    for (int l = levels - 1; l >= 0; --l) {
      const int nq = smooth_lanes(lv[l]);
      const SmLevel& up = l + 1 < levels ? lv[l + 1] : none;
      const double* zup = l + 1 < levels ? zc[l + 1] : nullptr;
      for (size_t gid = 0; gid < (size_t)nq * nact; ++gid) {
        if (l == 0) smooth_selinv_lane<true>(lv[0], up, td, nullptr, zup, oc.data(), out_lag9 ? ol.data() : nullptr, K, list[gid % nact], (int)(gid / nact));
        else smooth_selinv_lane<false>(lv[l], up, td, zc[l], zup, nullptr, nullptr, K, list[gid % nact], (int)(gid / nact));
      }
    }
  }
  for (int k = 0; k < K; ++k) {
    const int st = n_usable[k] < 2 ? SM_TOO_FEW_FRAMES : bad[k] ? SM_PIVOT : SM_OK;
    status[k] = st;
    for (size_t t = 0; t < T; ++t) {
      const size_t i = t * K + k;
      for (int e = 0; e < 6; ++e) out_cov6[6 * i + e] = st == SM_OK ? oc[6 * i + e] : nan;
      if (out_lag9 && t + 1 < T)
        for (int e = 0; e < 9; ++e) out_lag9[9 * i + e] = st == SM_OK ? ol[9 * i + e] : nan;
    }
  }
  for (int i = 0; i < 8; ++i) info8[i] = 0.0;
  info8[0] = levels; info8[1] = segment; info8[2] = K; info8[3] = 1;
  return 0;
}

// the chunk rule and the carve of the C call: out4 = tracks per chunk, chunks, device bytes, levels; offs (3 per level) = where fac, sep and the
// SM_ZC planes of each level of a chunk of that many tracks start in its storage, in doubles (-1: none); total = the doubles of that storage
extern "C" int hc_smooth_chunks(size_t T, int K, int segment, double budget_mb, int lag, double* out4, long long* offs, long long* total) {
  if (segment == 0) segment = SM_SEGMENT_DEFAULT;
  int nchunks = 0, levels = 0;
  const int Kc = smooth_chunk_tracks(budget_mb * 1048576.0, smooth_cov_chunk_doubles(T, 1, segment, lag != 0), (size_t)K, nchunks);
  SmLevel lv[SM_MAX_LEVELS];
  double* zc[SM_MAX_LEVELS];
  std::vector<double> store(smooth_carve(T, segment, Kc, lv, SM_ZC, nullptr, nullptr));
  *total = (long long)smooth_carve(T, segment, Kc, lv, SM_ZC, store.data(), zc, &levels);
  for (int l = 0; l < levels; ++l) {
    offs[3 * l] = lv[l].fac - store.data();
    offs[3 * l + 1] = lv[l].sep ? lv[l].sep - store.data() : -1;
    offs[3 * l + 2] = zc[l] ? zc[l] - store.data() : -1;
  }
  out4[0] = Kc; out4[1] = nchunks; out4[2] = (double)smooth_cov_chunk_doubles(T, Kc, segment, lag != 0) * sizeof(double); out4[3] = levels;
  return 0;
}

#ifdef SMOOTH_COV_HOSTCHECK_MAIN
// scene file: int64 T, K, segment, has_weights, lag; points (T, K, 3), cov6 (T, K, 6), accel_std (K), [weights (T, K)].  Prints status, usable
// frames and the sums of the finite entries of both outputs per track.
int main(int argc, char** argv) {
  if (argc < 2) return 2;
  FILE* fh = fopen(argv[1], "rb");
  if (!fh) return 2;
  long long hd[5];
  if (fread(hd, sizeof(long long), 5, fh) != 5) return 2;
  const size_t T = (size_t)hd[0];
  const int K = (int)hd[1];
  std::vector<double> pts(3 * T * K), cov(6 * T * K), acc(K), win(hd[3] ? T * K : 0);
  if (fread(pts.data(), sizeof(double), pts.size(), fh) != pts.size() || fread(cov.data(), sizeof(double), cov.size(), fh) != cov.size() || fread(acc.data(), sizeof(double), acc.size(), fh) != acc.size())
    return 2;
  if (hd[3] && fread(win.data(), sizeof(double), win.size(), fh) != win.size()) return 2;
  fclose(fh);
  std::vector<double> oc(6 * T * K), ol(hd[4] ? 9 * (T - 1) * K : 0);
  std::vector<int> st(K), nu(K);
  double info[8];
  const int rc = hc_smooth_covariance(T, K, pts.data(), cov.data(), acc.data(), hd[3] ? win.data() : nullptr, (int)hd[2], oc.data(), hd[4] ? ol.data() : nullptr, st.data(), nu.data(), info);
  if (rc) return 1;
  for (int k = 0; k < K; ++k) {
    double s = 0.0, sl = 0.0;
    for (size_t t = 0; t < T; ++t) {
      for (int e = 0; e < 6; ++e) { const double v = oc[6 * (t * K + k) + e]; if (v == v) s += v; }
      if (hd[4] && t + 1 < T)
        for (int e = 0; e < 9; ++e) { const double v = ol[9 * (t * K + k) + e]; if (v == v) sl += v; }
    }
    printf("track %d status %d usable %d sum %.17g lag %.17g\n", k, st[k], nu[k], s, sl);
  }
  printf("levels %d\n", (int)info[0]);
  return 0;
}
#endif
