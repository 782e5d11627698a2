// Host build of csrc/mcba_smooth_math.h -- the per-lane text of csrc/mcba_smooth.hip (k_smooth_prepare, k_smooth_reduce, k_smooth_backsub,
// k_smooth_eval) -- for g++: serial loops over the lanes in the kernels' order (every level up, every level down, tracks fastest), the level plan
// and the stopping rule the C ABI uses, the IRLS loop of mcba_smooth_api.hip around them.  tests/test_hostcheck_smoothing.py compiles this as a
// shared library (plain -O2) and holds it to the GPU tier's bar; with -DSMOOTH_HOSTCHECK_MAIN it is a stand-alone program that reads a scene
// file, which the same test builds with -fsanitize=address,undefined and runs as a child process.
#include <cmath>
#include <cstddef>
#include <cstdio>
#include <cstring>
#include <vector>
#include "../../multicam-calibration_amd/csrc/mcba_smooth_math.h"

using namespace mcba;

extern "C" int hc_smooth_trajectories(size_t T, int K, const double* points, const double* cov6, const double* accel_std, const double* weights_in, int loss, double f_scale, int max_iterations,
                                      double xtol, int segment, double* out_points, double* out_weights, double* out_d2, int* status, int* n_usable, int* n_iterations, double* history,
                                      double* info8) {
  if (T < 1 || K < 1 || loss < 0 || loss > 2 || !(f_scale > 0.0) || max_iterations < 1 || (segment != 0 && (segment < SM_SEGMENT_MIN || segment > SM_SEGMENT_MAX))) return 1;
  if (segment == 0) segment = SM_SEGMENT_DEFAULT;
  const double nan = std::nan("");
  const size_t TK = T * K;
  SmLevel lv[SM_MAX_LEVELS];
  double* aux[SM_MAX_LEVELS];
  int levels = 0;
  std::vector<double> store(smooth_carve(T, segment, K, lv, 6, nullptr, nullptr), nan);   // NaN-filled: whatever reads a word nobody wrote shows
  if (store.empty()) return 1;
  smooth_carve(T, segment, K, lv, 6, store.data(), aux, &levels);
  for (int l = 1; l < levels; ++l) lv[l].x = aux[l];
  std::vector<double> p(3 * TK), winv(6 * TK), w(TK), x(3 * TK, 0.0), d2(TK, 0.0), dx(TK, nan), ia2(K);
  std::vector<int> bad(K, 0), list, stat(K, SM_OK);
  for (int k = 0; k < K; ++k) { ia2[k] = 1.0 / (accel_std[k] * accel_std[k]); n_usable[k] = 0; n_iterations[k] = 0; }
  for (size_t i = 0; i < TK; ++i)
    if (smooth_prepare_lane(points + 3 * i, cov6 + 6 * i, weights_in ? weights_in[i] : 1.0, p.data() + 3 * i, winv.data() + 6 * i, w[i])) n_usable[i % K] += 1;
  for (int k = 0; k < K; ++k) {
    if (n_usable[k] < 2) stat[k] = SM_TOO_FEW_FRAMES;
    else list.push_back(k);
  }
  for (size_t i = 0; i < (size_t)max_iterations * K * 2; ++i) history[i] = nan;
  SmData td{T, p.data(), winv.data(), w.data(), ia2.data(), x.data(), d2.data(), dx.data(), loss, f_scale * f_scale, 1.0 / (f_scale * f_scale)};
  const SmLevel none{};
  for (int it = 0; it < max_iterations && !list.empty(); ++it) {
    const int nact = (int)list.size();
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
      for (size_t gid = 0; gid < (size_t)nq * nact; ++gid) {
        if (l == 0) smooth_backsub_lane<true>(lv[0], up, td, K, list[gid % nact], (int)(gid / nact));
        else smooth_backsub_lane<false>(lv[l], up, td, K, list[gid % nact], (int)(gid / nact));
      }
    }
    std::vector<int> next;
    for (int kk = 0; kk < nact; ++kk) {
      const int k = list[kk];
      double acc[4] = {0.0, 0.0, 0.0, 0.0};
      for (size_t t = 0; t < T; ++t) smooth_eval_frame(td, K, k, t, acc);
      const double obj = smooth_objective(acc[0], acc[1], td.f2, ia2[k]), step = it == 0 ? HUGE_VAL : acc[2];
      n_iterations[k] = it + 1;
      history[((size_t)it * K + k) * 2] = obj;
      history[((size_t)it * K + k) * 2 + 1] = step;
      if (bad[k]) { stat[k] = SM_PIVOT; continue; }
      if (!smooth_stops(loss, it, max_iterations, step, acc[3], xtol)) next.push_back(k);
    }
    list.swap(next);
  }
  for (int k = 0; k < K; ++k) {
    const bool ok = stat[k] == SM_OK;
    status[k] = stat[k];
    for (size_t t = 0; t < T; ++t) {
      const size_t i = t * K + k;
      for (int e = 0; e < 3; ++e) out_points[3 * i + e] = ok ? x[3 * i + e] : nan;
      out_weights[i] = ok ? w[i] : 0.0;
      out_d2[i] = ok ? d2[i] : nan;
    }
  }
  for (int i = 0; i < 8; ++i) info8[i] = 0.0;
  info8[0] = levels; info8[1] = segment; info8[2] = K; info8[3] = 1;
  return 0;
}

// the chunk rule and the carve of the C call: out4 = tracks per chunk, chunks, device bytes, levels; offs (3 per level) = where fac, sep and the
// extra plane of each level of a chunk of that many tracks start in its storage, in doubles (-1: none); total = the doubles of that storage
extern "C" int hc_smooth_chunks(size_t T, int K, int segment, double budget_mb, double* out4, long long* offs, long long* total) {
  if (segment == 0) segment = SM_SEGMENT_DEFAULT;
  int nchunks = 0, levels = 0;
  const int Kc = smooth_chunk_tracks(budget_mb * 1048576.0, smooth_chunk_doubles(T, 1, segment), (size_t)K, nchunks);
  SmLevel lv[SM_MAX_LEVELS];
  double* aux[SM_MAX_LEVELS];
  std::vector<double> store(smooth_carve(T, segment, Kc, lv, 6, nullptr, nullptr));
  *total = (long long)smooth_carve(T, segment, Kc, lv, 6, store.data(), aux, &levels);
  for (int l = 0; l < levels; ++l) {
    offs[3 * l] = lv[l].fac - store.data();
    offs[3 * l + 1] = lv[l].sep ? lv[l].sep - store.data() : -1;
    offs[3 * l + 2] = aux[l] ? aux[l] - store.data() : -1;
  }
  out4[0] = Kc; out4[1] = nchunks; out4[2] = (double)smooth_chunk_doubles(T, Kc, segment) * sizeof(double); out4[3] = levels;
  return 0;
}

#ifdef SMOOTH_HOSTCHECK_MAIN
// scene file: int64 T, K, loss, max_iterations, segment, has_weights; double f_scale, xtol; points (T, K, 3), cov6 (T, K, 6), accel_std (K),
// [weights (T, K)].  Prints status, iterations and the sum of the finite coordinates per track.
int main(int argc, char** argv) {
  if (argc < 2) return 2;
  FILE* fh = fopen(argv[1], "rb");
  if (!fh) return 2;
  long long hd[6];
  double fd[2];
  if (fread(hd, sizeof(long long), 6, fh) != 6 || fread(fd, sizeof(double), 2, fh) != 2) return 2;
  const size_t T = (size_t)hd[0];
  const int K = (int)hd[1];
  std::vector<double> pts(3 * T * K), cov(6 * T * K), acc(K), win(hd[5] ? T * K : 0);
  if (fread(pts.data(), sizeof(double), pts.size(), fh) != pts.size() || fread(cov.data(), sizeof(double), cov.size(), fh) != cov.size() || fread(acc.data(), sizeof(double), acc.size(), fh) != acc.size())
    return 2;
  if (hd[5] && fread(win.data(), sizeof(double), win.size(), fh) != win.size()) return 2;
  fclose(fh);
  std::vector<double> x(3 * T * K), w(T * K), d2(T * K), hist((size_t)hd[3] * K * 2);
  std::vector<int> st(K), nu(K), ni(K);
  double info[8];
  const int rc = hc_smooth_trajectories(T, K, pts.data(), cov.data(), acc.data(), hd[5] ? win.data() : nullptr, (int)hd[2], fd[0], (int)hd[3], fd[1], (int)hd[4], x.data(), w.data(), d2.data(), st.data(),
                                        nu.data(), ni.data(), hist.data(), info);
  if (rc) return 1;
  for (int k = 0; k < K; ++k) {
    double s = 0.0;
    for (size_t t = 0; t < T; ++t)
      for (int e = 0; e < 3; ++e) { const double v = x[3 * (t * K + k) + e]; if (v == v) s += v; }
    printf("track %d status %d usable %d iterations %d sum %.17g\n", k, st[k], nu[k], ni[k], s);
  }
  printf("levels %d\n", (int)info[0]);
  return 0;
}
#endif
