// mcba_smooth_evidence_math.h -- the arithmetic of csrc/mcba_smooth_evidence.hip and the search rule of csrc/mcba_smooth_evidence_api.hip (SURVEY.md
// section 8f-24): the smoother's evidence as a function of a = accel_std.  Per track, with A(a) the matrix of mcba_smooth_math.h and x(a) its solve,
//   N(a) = sum_t w_t d_t^2(x) + a^-2 sum_t |x_{t-1} - 2 x_t + x_{t+1}|^2 + log det A(a) + 6 (T - 2) log a
// is -2 x the log restricted marginal likelihood up to a constant in a.  log det A is the sum over every factorised 6 x 6 pivot block of
// 2 sum_i log l_ii: the elimination keeps L of every block in lv.fac with its diagonal as reciprocals, so a lane sums log(stored) and the result is
// -2 x that sum.  Only the blocks smooth_reduce_lane factorised hold a factor -- the interior positions i < m of the segments that hold blocks, every
// block of the last level; separator slots, positions past n and an empty last segment are uninitialised memory and are never read.  The phantom
// frame of an odd T has the pivots 1 and adds log 1 = 0.
// Sums: one partial per lane (segment, track) of every level, then per track a fixed tree over its lanes in level order (evidence_tree256: the
// order of a 256-thread workgroup -- thread i adds the partials i, i + 256, .. and the halves are folded 128, 64, .. 1).  The data term and the
// penalty are summed the same way over 256-frame blocks.  The order depends on (T, segment) alone.
// The search rule of mcba_estimate_accel_std (evidence_search) is host code, written once here and mirrored in tests/evidence_oracle.py.
// The same text is compiled with g++ into tests/hostcheck/evidence_hostcheck.cpp (tests/test_hostcheck_evidence.py).
#pragma once
#include <math.h>

#include <vector>

#include "mcba_smooth_math.h"

namespace mcba {

constexpr int EV_RES = 4;                           // per running track: sum w d^2, sum |second difference|^2, sum log(stored pivot reciprocals), 1 = a pivot was refused
constexpr int EV_GRID_MIN = 3;
constexpr double EV_RTOL_MIN = 1e-6;                // rtol in [EV_RTOL_MIN, 1)
constexpr double EV_INVPHI = 0.6180339887498949;    // (sqrt 5 - 1) / 2
constexpr double EV_CURV_H = 0.2;                   // the curvature's step in log a

// ---- the lanes of one track over every level, in level order: level l owns the partials off[l] .. off[l] + smooth_lanes(lv[l]) - 1
inline size_t evidence_lanes(const SmLevel* lv, int levels, size_t* off = nullptr) {
  size_t n = 0;
  for (int l = 0; l < levels; ++l) {
    if (off) off[l] = n;
    n += (size_t)smooth_lanes(lv[l]);
  }
  return n;
}
// device doubles one chunk of K tracks of the evidence calls needs: the smoother's, a second weights plane, the lane partials, the sums
inline size_t evidence_chunk_doubles(size_t T, int K, int segment) {
  SmLevel lv[SM_MAX_LEVELS];
  const int L = smooth_plan(T, segment, K, lv);
  return smooth_chunk_doubles(T, K, segment) + T * (size_t)K + (evidence_lanes(lv, L) + EV_RES) * (size_t)K;
}

// ---- segment q of track k on level lv: the sum of log over the stored diagonal of every block the lane factorised (none: 0, nothing read)
MCBA_HD double evidence_lane_logsum(const SmLevel& lv, int K, int k, int q) {
  const int m = lv.m, n = lv.n;
  const long long j0 = (long long)q * (m + 1);
  const int len = n - j0 < m ? (int)(n - j0) : m;
  double s = 0.0;
  for (int i = 0; i < len; ++i) {
    const size_t nd = sm_node(lv, j0 + i, K, k);
#pragma unroll
    for (int d = 0; d < 6; ++d) s += log(lv.fac[(size_t)sm_tri(d, d) * lv.NS + nd]);
  }
  return s;
}

// ---- one (frame, track) at the solution: acc = (sum w d^2 with the weights the matrix was built with, sum |second difference|^2)
MCBA_HD void evidence_eval_frame(const SmData& td, int K, int k, size_t t, double* acc) {
  const size_t idx = t * K + k;
  if (td.winv[6 * idx] != 0.0) acc[0] = fma(td.w[idx], td.d2[idx], acc[0]);
  if (t >= 1 && t + 2 <= td.T) {
    const size_t a = idx - K, b = idx + K;
#pragma unroll
    for (int e = 0; e < 3; ++e) {
      const double s = td.x[3 * a + e] - 2.0 * td.x[3 * idx + e] + td.x[3 * b + e];
      acc[1] = fma(s, s, acc[1]);
    }
  }
}

// ---- the sum of n values p[i stride] in the order of a 256-thread workgroup (block_tree of mcba_device.h after a strided loop)
inline double evidence_tree256(const double* p, size_t n, size_t stride) {
  double s[256];
  for (int i = 0; i < 256; ++i) {
    double r = 0.0;
    for (size_t j = i; j < n; j += 256) r += p[j * stride];
    s[i] = r;
  }
  for (int h = 128; h > 0; h >>= 1)
    for (int i = 0; i < h; ++i) s[i] += s[i + h];
  return s[0];
}

// ---- a track's terms from its three sums: out = (N, data, penalty, log det); T the true frame count
MCBA_HD void evidence_terms(const double* sums, size_t T, double a, double ia2, double* out) {
  out[1] = sums[0];
  out[2] = ia2 * sums[1];
  out[3] = -2.0 * sums[2];
  out[0] = out[1] + out[2] + out[3] + 6.0 * ((double)T - 2.0) * log(a);
}

// ---- the search rule.  nt running tracks, track i in unit unit[i] of U units (a unit without tracks is left alone); a unit's objective is the sum
// of its tracks' N in track order, NaN counting as +infinity.  eval(a (nt), n (nt)) evaluates every track at its candidate and returns 0, or an
// error code that ends the search.  Every pass evaluates every track: a unit with nothing left to decide repeats its last candidate, so the
// passes number evidence_evaluations() whatever the data.
//   grid (G): evidence_grid's, given; n_grid (G, nt); per track: a_hat, log_std, n_best (its N at a_hat), edge (-1, 0, +1), all_nan (every candidate of its unit NaN)
inline void evidence_grid(double lo, double hi, int G, double* grid) {
  const double ul = log(lo), du = (log(hi) - ul) / (G - 1);
  for (int g = 0; g < G; ++g) grid[g] = g == 0 ? lo : g == G - 1 ? hi : exp(ul + g * du);
}
// the rounds of the golden section: the bracket starts two grid steps wide and every round takes the factor EV_INVPHI off it
inline int evidence_rounds(double lo, double hi, int G, double rtol) {
  double w = 2.0 * (log(hi) - log(lo)) / (G - 1);
  int r = 0;
  while (!(w < rtol) && r < 200) { w *= EV_INVPHI; ++r; }
  return r;
}
inline int evidence_evaluations(double lo, double hi, int G, double rtol) { return G + 2 + evidence_rounds(lo, hi, G, rtol) + 2; }

template <class Eval>
inline int evidence_search(int nt, const int* unit, int U, double lo, double hi, int G, double rtol, Eval&& eval, const double* grid, double* n_grid, double* a_hat, double* log_std, double* n_best,
                           int* edge, int* all_nan) {
  const double inf = HUGE_VAL, nan = __builtin_nan("");
  const double ul = log(lo), du = (log(hi) - ul) / (G - 1);
  std::vector<double> a_t(nt), n_t(nt), obj(U), cand(U, lo), og((size_t)G * U);
  auto pass = [&]() -> int {   // every unit at cand[]: n_t, obj
    for (int i = 0; i < nt; ++i) a_t[i] = cand[unit[i]];
    if (int rc = eval(a_t.data(), n_t.data())) return rc;
    for (int u = 0; u < U; ++u) obj[u] = 0.0;
    for (int i = 0; i < nt; ++i) obj[unit[i]] += n_t[i];
    for (int u = 0; u < U; ++u)
      if (!(obj[u] == obj[u])) obj[u] = inf;
    return 0;
  };
  // 1. the grid
  for (int g = 0; g < G; ++g) {
    for (int u = 0; u < U; ++u) cand[u] = grid[g];
    if (int rc = pass()) return rc;
    for (int i = 0; i < nt; ++i) n_grid[(size_t)g * nt + i] = n_t[i];
    for (int u = 0; u < U; ++u) og[(size_t)g * U + u] = obj[u];
  }
  // 2. the first argmin; state: 0 = refine, -1 / +1 = on an edge, 2 = every candidate NaN
  std::vector<int> gs(U, 0), state(U, 0);
  std::vector<double> ubest(U), fbest(U, inf), abest(U, nan);
  for (int u = 0; u < U; ++u) {
    for (int g = 0; g < G; ++g)
      if (og[(size_t)g * U + u] < fbest[u]) { fbest[u] = og[(size_t)g * U + u]; gs[u] = g; }
    state[u] = !(fbest[u] < inf) ? 2 : gs[u] == 0 ? -1 : gs[u] == G - 1 ? 1 : 0;
    ubest[u] = ul + gs[u] * du;
    if (state[u] != 2) abest[u] = grid[gs[u]];
    cand[u] = grid[gs[u]];
  }
  for (int i = 0; i < nt; ++i) n_best[i] = state[unit[i]] == 2 ? nan : n_grid[(size_t)gs[unit[i]] * nt + i];
  std::vector<char> better(U, 0);
  auto take = [&](const double* ucand) {   // the best point so far, first on a tie
    for (int u = 0; u < U; ++u) {
      better[u] = state[u] == 0 && obj[u] < fbest[u];
      if (better[u]) { fbest[u] = obj[u]; ubest[u] = ucand[u]; abest[u] = cand[u]; }
    }
    for (int i = 0; i < nt; ++i)
      if (better[unit[i]]) n_best[i] = n_t[i];
  };
  // 3. the golden section in u on [u_{g* - 1}, u_{g* + 1}]
  std::vector<double> a(U), b(U), c(U), d(U), fc(U, inf), fd(U, inf), ucand(U);
  for (int u = 0; u < U; ++u) {
    a[u] = ul + (gs[u] - 1) * du;
    b[u] = ul + (gs[u] + 1) * du;
    c[u] = b[u] - EV_INVPHI * (b[u] - a[u]);
    d[u] = a[u] + EV_INVPHI * (b[u] - a[u]);
    ucand[u] = ubest[u];
  }
  auto propose = [&](int u, double uu) {   // the next candidate of a unit that refines; the others keep theirs
    if (state[u] == 0) { ucand[u] = uu; cand[u] = exp(uu); }
  };
  for (int u = 0; u < U; ++u) propose(u, c[u]);
  if (int rc = pass()) return rc;
  for (int u = 0; u < U; ++u) fc[u] = obj[u];
  take(ucand.data());
  for (int u = 0; u < U; ++u) propose(u, d[u]);
  if (int rc = pass()) return rc;
  for (int u = 0; u < U; ++u) fd[u] = obj[u];
  take(ucand.data());
  const int rounds = evidence_rounds(lo, hi, G, rtol);
  std::vector<char> left(U, 0);   // the round's new point is c (the bracket lost its right end)
  for (int r = 0; r < rounds; ++r) {
    for (int u = 0; u < U; ++u) {
      left[u] = fc[u] < fd[u];
      if (left[u]) { b[u] = d[u]; d[u] = c[u]; fd[u] = fc[u]; c[u] = b[u] - EV_INVPHI * (b[u] - a[u]); }
      else { a[u] = c[u]; c[u] = d[u]; fc[u] = fd[u]; d[u] = a[u] + EV_INVPHI * (b[u] - a[u]); }
      propose(u, left[u] ? c[u] : d[u]);
    }
    if (int rc = pass()) return rc;
    for (int u = 0; u < U; ++u) (left[u] ? fc[u] : fd[u]) = obj[u];
    take(ucand.data());
  }
  // 4. the curvature at the best point: N at u + h, then at u - h
  std::vector<double> fp(U), fm(U);
  const std::vector<double> centre = ubest;
  for (int u = 0; u < U; ++u) propose(u, centre[u] + EV_CURV_H);
  if (int rc = pass()) return rc;
  fp = obj;
  for (int u = 0; u < U; ++u) propose(u, centre[u] - EV_CURV_H);
  if (int rc = pass()) return rc;
  fm = obj;
  for (int i = 0; i < nt; ++i) {
    const int u = unit[i];
    all_nan[i] = state[u] == 2;
    edge[i] = state[u] == -1 || state[u] == 1 ? state[u] : 0;
    a_hat[i] = state[u] == 2 ? nan : state[u] == -1 ? lo : state[u] == 1 ? hi : abest[u];
    double ls = nan;
    if (state[u] == 0) {
      const double kappa = (fp[u] - 2.0 * fbest[u] + fm[u]) / (EV_CURV_H * EV_CURV_H);
      if (kappa > 0.0 && sm_finite(kappa)) ls = sqrt(2.0 / kappa);
    }
    log_std[i] = ls;
  }
  return 0;
}

}  // namespace mcba
