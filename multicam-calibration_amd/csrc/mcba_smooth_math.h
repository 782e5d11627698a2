// mcba_smooth_math.h -- the per-lane arithmetic of csrc/mcba_smooth.hip: the fixed-interval smoother of keypoint tracks.
// Per track, frames t = 0 .. T-1, unknowns x_t in R^3:
//   minimise 0.5 f^2 sum_t rho(d_t^2 / f^2) + 0.5 / a^2 sum_{t=1}^{T-2} |x_{t-1} - 2 x_t + x_{t+1}|^2,   d_t^2 = (x_t - p_t)^T Sigma_t^-1 (x_t - p_t)
// by IRLS: each iteration solves A x = b, A = blockdiag(w_t Sigma_t^-1) + a^-2 (D2^T D2 (x) I3), b = blockdiag(w_t Sigma_t^-1) p.
// Frames are paired into super-frames (2 s, 2 s + 1): A is block-tridiagonal in 6 x 6 blocks D_s (symmetric) and E_s (the coupling of s to s - 1);
// an odd T gets a phantom frame (identity diagonal, no coupling, zero right-hand side).  Row s reads E_s x_{s-1} + D_s x_s + E_{s+1}^T x_{s+1} = r_s.
// One level of the elimination cuts a chain of n blocks into segments of m interior blocks separated by single separator blocks (block j is a
// separator when j mod (m + 1) == m).  smooth_reduce_lane eliminates the interior of one segment of one track:
//   D'_i = D_i - E_i D'_{i-1}^-1 E_i^T,  G_i = -E_i D'_{i-1}^-1 G_{i-1} (the fill column to the left separator),  g_i likewise,
// stores per interior block the factor L of D'_i (Jacobi-scaled Cholesky, diagonal kept as reciprocals), L^-1 G_i and L^-1 g_i (63 doubles), and hands
// the next level -- the chain of this level's separators -- what it adds to them: the right separator's own block less its Schur term (base),
// the Schur term on the left separator (cl, summed by the next level's loader: nobody adds into memory another lane writes) and the
// separator-to-separator coupling.  The last level is one segment without separators.  smooth_backsub_lane runs the levels top down:
//   x_i = L^-T (L^-1 g_i - L^-1 G_i x_L - L^-1 E_{i+1}^T x_{i+1}).
// Layout: element e of node (block j, track k) of a level lies at e NS + ((j mod (m + 1)) nq + j / (m + 1)) K + k: the lanes of a wavefront
// (consecutive segments and tracks) touch consecutive doubles at every step of their walks.
// The same text is compiled with g++ into tests/hostcheck/smoothing_hostcheck.cpp (tests/test_hostcheck_smoothing.py).
#pragma once
#include <stddef.h>

#include "mcba_tricov_math.h"

namespace mcba {

// status of a track
constexpr int SM_OK = 1, SM_TOO_FEW_FRAMES = -1, SM_PIVOT = -2;
constexpr int SM_SEGMENT_MIN = 2, SM_SEGMENT_MAX = 64, SM_SEGMENT_DEFAULT = 16, SM_MAX_LEVELS = 40;
// the smallest square of a pivot of a Jacobi-scaled 6 x 6 block that is still factorised
constexpr double SM_PIVOT2_MIN = 1e-12;
constexpr int SM_FAC = 63;   // per interior block: L (21, lower packed, reciprocal diagonal) | L^-1 G (36, row-major) | L^-1 g (6)
constexpr int SM_SEP = 90;   // per block of a level >= 1: base (D 21 | r 6) | cl (D 21 | r 6) | E (36, row-major)
constexpr int SM_LOSS_LINEAR = 0, SM_LOSS_SOFT_L1 = 1, SM_LOSS_HUBER = 2;

struct SmLevel {
  int n, m, nq;   // blocks of the chain, interior blocks per segment (n itself on the last level), segments that hold a block
  size_t NS;      // nodes per element plane: (m + 1) nq K
  double* fac;    // [SM_FAC][NS]
  double* sep;    // levels >= 1: [SM_SEP][NS]
  double* x;      // levels >= 1: [6][NS], the solution
};

// level 0 of one chunk of K tracks: the (T, K, .) planes
struct SmData {
  size_t T;
  const double* p;      // (T, K, 3): the points, zero where the frame is unusable
  const double* winv;   // (T, K, 6): Sigma^-1 packed 00 01 02 11 12 22, zero where the frame is unusable (entry 00 > 0 otherwise)
  double* w;            // (T, K): the IRLS weights, 0 on unusable frames
  const double* ia2;    // (K): 1 / accel_std^2
  double* x;            // (T, K, 3): the solution
  double* d2;           // (T, K): d_t^2 at the solution, NaN on unusable frames
  double* dx;           // (T, K): max |x_new - x_old| of the frame's three coordinates
  int loss;
  double f2, inv_f2;    // f_scale^2 and its reciprocal
  // the right-hand-side mode of level 0 (RHS: mcba_traj_refine_math.h): winv is then the packed diagonal block itself (weight 1, w unread), the
  // right-hand side is -rhs, and the solution goes to x and nowhere else
  const double* rhs;    // (T, K, 3): the gradient the solve steps against
};

MCBA_HD bool sm_finite(double v) { return v - v == 0.0; }

// the levels of T frames: returns their number (0 = more than SM_MAX_LEVELS, which no size_t reaches with segment >= 2 and 2^31 blocks)
inline int smooth_plan(size_t T, int segment, int K, SmLevel* lv) {
  int n = (int)((T + 1) / 2), L = 0;
  for (;;) {
    if (L == SM_MAX_LEVELS) return 0;
    SmLevel& a = lv[L++];
    a.n = n;
    a.m = n <= segment + 1 ? n : segment;
    a.nq = (n - 1) / (a.m + 1) + 1;
    a.NS = (size_t)(a.m + 1) * a.nq * K;
    a.fac = a.sep = a.x = nullptr;
    if (a.m == n) return L;
    n = n / (a.m + 1);
  }
}
// the lanes (segments) one track has on a level: the segments with a left separator, the last of which may be empty, and the first
MCBA_HD int smooth_lanes(const SmLevel& lv) { return lv.m == lv.n ? 1 : lv.n / (lv.m + 1) + 1; }
// the launch of a level for nact running tracks: nq = its lanes per track, blocks = workgroups of 64 lanes.  False: the grid would not fit
inline bool smooth_grid(const SmLevel& lv, int nact, int& nq, unsigned& blocks) {
  nq = smooth_lanes(lv);
  const size_t b = ((size_t)nq * nact + 63) / 64;
  blocks = (unsigned)b;
  return b <= 0x7fffffffu;
}
inline int smooth_eval_blocks(size_t T) { return (int)((T + 255) / 256); }   // workgroups of k_smooth_eval per track: part holds 4 doubles for each

// the plan and the level storage of a chunk of K tracks, in one walk: per level fac, from level 1 on sep, then `extra` doubles per node (the
// smoother's solution, 6; the SM_ZC planes of mcba_smooth_cov_math.h).  Returns the doubles it takes, 0 where smooth_plan returns no levels.
// base null: counts only.  Otherwise lv[l].fac and lv[l].sep are set and aux[l] is the level's extra plane (aux[0] = nullptr)
inline size_t smooth_carve(size_t T, int segment, int K, SmLevel* lv, int extra, double* base, double** aux, int* levels = nullptr) {
  const int L = smooth_plan(T, segment, K, lv);
  if (levels) *levels = L;
  size_t n = 0;
  for (int l = 0; l < L; ++l) {
    const size_t part[3] = {lv[l].NS * SM_FAC, l ? lv[l].NS * SM_SEP : 0, l ? lv[l].NS * extra : 0};
    if (base) {
      lv[l].fac = base + n;
      lv[l].sep = l ? base + n + part[0] : nullptr;
      aux[l] = l ? base + n + part[0] + part[1] : nullptr;
    }
    n += part[0] + part[1] + part[2];
  }
  return n;
}
// tracks per chunk of K tracks under a budget in bytes, one track taking per_track doubles: as many as fit, at least one; and the chunks
inline int smooth_chunk_tracks(double budget_bytes, size_t per_track, size_t K, int& nchunks) {
  const double fit = floor(budget_bytes / ((double)per_track * sizeof(double)));
  const int Kc = (int)((double)K < fit ? (double)K : fit > 1.0 ? fit : 1.0);
  nchunks = (int)((K + Kc - 1) / Kc);
  return Kc;
}
// device doubles (and ints, counted as doubles) one chunk of K tracks of the smoother needs.  (Approximate on purpose, and reported as
// device_bytes: the weights plane is counted whether given or not)
inline size_t smooth_chunk_doubles(size_t T, int K, int segment) {
  SmLevel lv[SM_MAX_LEVELS];
  return (size_t)T * K * 24 + (size_t)K * 8 + (size_t)4 * smooth_eval_blocks(T) * K + smooth_carve(T, segment, K, lv, 6, nullptr, nullptr);
}

MCBA_HD size_t sm_node(const SmLevel& lv, long long j, int K, int k) {
  const long long q = j / (lv.m + 1), i = j % (lv.m + 1);
  return ((size_t)i * lv.nq + (size_t)q) * K + k;
}
MCBA_HD constexpr int sm_tri(int i, int j) { return i * (i + 1) / 2 + j; }   // lower packed, i >= j

// ---- loss: rho(z) and rho'(z) of scipy's linear, soft_l1, huber
MCBA_HD double sm_rho(int loss, double z) {
  if (loss == SM_LOSS_SOFT_L1) return 2.0 * (sqrt(1.0 + z) - 1.0);
  if (loss == SM_LOSS_HUBER) return z <= 1.0 ? z : 2.0 * sqrt(z) - 1.0;
  return z;
}
MCBA_HD double sm_drho(int loss, double z) {
  if (loss == SM_LOSS_SOFT_L1) return 1.0 / sqrt(1.0 + z);
  if (loss == SM_LOSS_HUBER) return z <= 1.0 ? 1.0 : 1.0 / sqrt(z);
  return 1.0;
}

// ---- the entries of D2^T D2 (T frames): v(r) = the second difference centred at r exists
MCBA_HD double sm_v(long long r, size_t T) { return (r >= 1 && (size_t)r + 2 <= T) ? 1.0 : 0.0; }
MCBA_HD double sm_pen_diag(long long t, size_t T) { return sm_v(t + 1, T) + 4.0 * sm_v(t, T) + sm_v(t - 1, T); }
MCBA_HD double sm_pen_off1(long long t, size_t T) { return -2.0 * (sm_v(t, T) + sm_v(t + 1, T)); }   // entry (t, t + 1)
MCBA_HD double sm_pen_off2(long long t, size_t T) { return sm_v(t + 1, T); }                          // entry (t, t + 2)

// ---- prepare: one (frame, track).  usable = p and Sigma finite, Sigma positive definite by the rule of tricov_inv3, its inverse finite
MCBA_HD bool smooth_prepare_lane(const double* p3, const double* c6, double w_in, double* p_out, double* winv, double& w) {
  bool ok = sm_finite(p3[0]) && sm_finite(p3[1]) && sm_finite(p3[2]);
#pragma unroll
  for (int i = 0; i < 6; ++i) ok = ok && sm_finite(c6[i]);
  double Hi[6];
  ok = ok && tricov_inv3(c6, Hi);
#pragma unroll
  for (int i = 0; i < 6; ++i) ok = ok && sm_finite(Hi[i]);
#pragma unroll
  for (int i = 0; i < 6; ++i) winv[i] = ok ? Hi[i] : 0.0;
#pragma unroll
  for (int i = 0; i < 3; ++i) p_out[i] = ok ? p3[i] : 0.0;
  w = ok ? w_in : 0.0;
  return ok;
}

// ---- a 6 x 6 symmetric positive definite block: L of the Jacobi-scaled Cholesky factorisation, unscaled again, its diagonal as reciprocals.
// bad is set when a diagonal entry is not positive or the square of a scaled pivot is below SM_PIVOT2_MIN (the pivot is then taken as 1)
MCBA_HD void sm_chol6(const double* A, double* L, bool& bad) {
  double s[6], is[6];
#pragma unroll
  for (int i = 0; i < 6; ++i) {
    const double a = A[sm_tri(i, i)];
    const bool pos = a > 0.0 && sm_finite(a);
    if (!pos) bad = true;
    s[i] = pos ? sqrt(a) : 1.0;
    is[i] = 1.0 / s[i];
  }
  double rd[6];   // reciprocal scaled pivots
#pragma unroll
  for (int j = 0; j < 6; ++j) {
    double d = A[sm_tri(j, j)] * is[j] * is[j];
#pragma unroll
    for (int k = 0; k < j; ++k) d = fma(-L[sm_tri(j, k)], L[sm_tri(j, k)], d);
    if (!(d >= SM_PIVOT2_MIN)) { bad = true; d = 1.0; }
    const double l = sqrt(d);
    rd[j] = 1.0 / l;
#pragma unroll
    for (int i = j + 1; i < 6; ++i) {
      double v = A[sm_tri(i, j)] * is[i] * is[j];
#pragma unroll
      for (int k = 0; k < j; ++k) v = fma(-L[sm_tri(i, k)], L[sm_tri(j, k)], v);
      L[sm_tri(i, j)] = v * rd[j];
    }
  }
#pragma unroll
  for (int i = 0; i < 6; ++i) {
#pragma unroll
    for (int j = 0; j < i; ++j) L[sm_tri(i, j)] *= s[i];
    L[sm_tri(i, i)] = rd[i] * is[i];
  }
}
// L y = b in place; b has stride `st`
MCBA_HD void sm_fwd6(const double* L, double* b, int st = 1) {
#pragma unroll
  for (int i = 0; i < 6; ++i) {
    double v = b[i * st];
#pragma unroll
    for (int k = 0; k < i; ++k) v = fma(-L[sm_tri(i, k)], b[k * st], v);
    b[i * st] = v * L[sm_tri(i, i)];
  }
}
// L^T x = y in place
MCBA_HD void sm_bwd6(const double* L, double* b) {
#pragma unroll
  for (int i = 5; i >= 0; --i) {
    double v = b[i];
#pragma unroll
    for (int k = i + 1; k < 6; ++k) v = fma(-L[sm_tri(k, i)], b[k], v);
    b[i] = v * L[sm_tri(i, i)];
  }
}

// ---- the coupling E of level-0 block j to block j - 1 (rows: frames 2 j, 2 j + 1; columns: frames 2 j - 2, 2 j - 1), its three scalars
MCBA_HD void sm_e0_scalars(const SmData& td, int k, long long j, double& e00, double& e01, double& e11) {
  const long long t0 = 2 * j;
  const double s = j > 0 ? td.ia2[k] : 0.0;
  e00 = s * sm_pen_off2(t0 - 2, td.T);
  e01 = s * sm_pen_off1(t0 - 1, td.T);
  e11 = s * sm_pen_off2(t0 - 1, td.T);
}

// ---- block j of a level: D (21), r (6), E (36: the coupling to block j - 1, zero for j = 0)
template <bool LEVEL0, bool RHS = false>
MCBA_HD void smooth_load(const SmLevel& lv, const SmData& td, int K, int k, long long j, double* D, double* r, double* E) {
  if (LEVEL0) {
    const double ia2 = td.ia2[k];
#pragma unroll
    for (int e = 0; e < 21; ++e) D[e] = 0.0;
#pragma unroll
    for (int e = 0; e < 36; ++e) E[e] = 0.0;
#pragma unroll
    for (int f = 0; f < 2; ++f) {
      const long long t = 2 * j + f;
      if ((size_t)t < td.T) {
        const size_t idx = (size_t)t * K + k;
        double wi[6], p[3];
        if (RHS) {
#pragma unroll
          for (int e = 0; e < 6; ++e) wi[e] = td.winv[6 * idx + e];
        } else {
          const double w = td.w[idx];
#pragma unroll
          for (int e = 0; e < 6; ++e) wi[e] = w * td.winv[6 * idx + e];
#pragma unroll
          for (int e = 0; e < 3; ++e) p[e] = td.p[3 * idx + e];
        }
        const double pd = ia2 * sm_pen_diag(t, td.T);
#pragma unroll
        for (int a = 0; a < 3; ++a) {
#pragma unroll
          for (int b = 0; b <= a; ++b) D[sm_tri(3 * f + a, 3 * f + b)] = sym3(wi, a, b) + (a == b ? pd : 0.0);
          r[3 * f + a] = RHS ? -td.rhs[3 * idx + a] : fma(sym3(wi, a, 0), p[0], fma(sym3(wi, a, 1), p[1], sym3(wi, a, 2) * p[2]));
        }
      } else {   // the phantom frame of an odd T
#pragma unroll
        for (int a = 0; a < 3; ++a) { D[sm_tri(3 * f + a, 3 * f + a)] = 1.0; r[3 * f + a] = 0.0; }
      }
    }
    const double o = ia2 * sm_pen_off1(2 * j, td.T);
#pragma unroll
    for (int a = 0; a < 3; ++a) D[sm_tri(3 + a, a)] = o;
    double e00, e01, e11;
    sm_e0_scalars(td, k, j, e00, e01, e11);
#pragma unroll
    for (int a = 0; a < 3; ++a) { E[a * 6 + a] = e00; E[a * 6 + 3 + a] = e01; E[(3 + a) * 6 + 3 + a] = e11; }
  } else {
    const size_t nd = sm_node(lv, j, K, k);
#pragma unroll
    for (int e = 0; e < 21; ++e) D[e] = lv.sep[(size_t)e * lv.NS + nd] + lv.sep[(size_t)(27 + e) * lv.NS + nd];
#pragma unroll
    for (int e = 0; e < 6; ++e) r[e] = lv.sep[(size_t)(21 + e) * lv.NS + nd] + lv.sep[(size_t)(48 + e) * lv.NS + nd];
#pragma unroll
    for (int e = 0; e < 36; ++e) E[e] = lv.sep[(size_t)(54 + e) * lv.NS + nd];
  }
}

// ---- reduce: segment q of track k on level lv; nx = the next level (untouched on the last one).  bad[k] = 1 on a refused pivot
template <bool LEVEL0, bool RHS = false>
MCBA_HD void smooth_reduce_lane(const SmLevel& lv, const SmLevel& nx, const SmData& td, int K, int k, int q, int* bad) {
  const int m = lv.m, n = lv.n;
  const long long j0 = (long long)q * (m + 1);
  const bool hasL = q > 0;
  const int len = n - j0 < m ? (int)(n - j0) : m;
  double CL[27];
#pragma unroll
  for (int e = 0; e < 27; ++e) CL[e] = 0.0;
  if (len > 0) {
    double D[21], g[6], G[36], E[36];
    smooth_load<LEVEL0, RHS>(lv, td, K, k, j0, D, g, E);
#pragma unroll
    for (int e = 0; e < 36; ++e) G[e] = hasL ? E[e] : 0.0;
    bool isbad = false;
    for (int i = 0; i < len; ++i) {
      double L[21];
      sm_chol6(D, L, isbad);
#pragma unroll
      for (int c = 0; c < 6; ++c) sm_fwd6(L, G + c, 6);
      sm_fwd6(L, g);
      const size_t nd = sm_node(lv, j0 + i, K, k);
#pragma unroll
      for (int e = 0; e < 21; ++e) lv.fac[(size_t)e * lv.NS + nd] = L[e];
#pragma unroll
      for (int e = 0; e < 36; ++e) lv.fac[(size_t)(21 + e) * lv.NS + nd] = G[e];
#pragma unroll
      for (int e = 0; e < 6; ++e) lv.fac[(size_t)(57 + e) * lv.NS + nd] = g[e];
      if (hasL) {
#pragma unroll
        for (int a = 0; a < 6; ++a) {
#pragma unroll
          for (int b = 0; b <= a; ++b) {
            double v = CL[sm_tri(a, b)];
#pragma unroll
            for (int r = 0; r < 6; ++r) v = fma(-G[r * 6 + a], G[r * 6 + b], v);
            CL[sm_tri(a, b)] = v;
          }
          double v = CL[21 + a];
#pragma unroll
          for (int r = 0; r < 6; ++r) v = fma(-G[r * 6 + a], g[r], v);
          CL[21 + a] = v;
        }
      }
      const long long jn = j0 + i + 1;
      if (jn < n) {
        double rn[6];
        smooth_load<LEVEL0, RHS>(lv, td, K, k, jn, D, rn, E);
        double Et[36];   // L^-1 E^T
#pragma unroll
        for (int r = 0; r < 6; ++r) {
#pragma unroll
          for (int c = 0; c < 6; ++c) Et[r * 6 + c] = E[c * 6 + r];
        }
#pragma unroll
        for (int c = 0; c < 6; ++c) sm_fwd6(L, Et + c, 6);
#pragma unroll
        for (int a = 0; a < 6; ++a) {
#pragma unroll
          for (int b = 0; b <= a; ++b) {
            double v = D[sm_tri(a, b)];
#pragma unroll
            for (int r = 0; r < 6; ++r) v = fma(-Et[r * 6 + a], Et[r * 6 + b], v);
            D[sm_tri(a, b)] = v;
          }
          double v = rn[a];
#pragma unroll
          for (int r = 0; r < 6; ++r) v = fma(-Et[r * 6 + a], g[r], v);
          rn[a] = v;
        }
#pragma unroll
        for (int c = 0; c < 6; ++c) {   // G <- -Et^T G, a column at a time
          double col[6];
#pragma unroll
          for (int a = 0; a < 6; ++a) {
            double v = 0.0;
#pragma unroll
            for (int r = 0; r < 6; ++r) v = fma(-Et[r * 6 + a], G[r * 6 + c], v);
            col[a] = v;
          }
#pragma unroll
          for (int a = 0; a < 6; ++a) G[a * 6 + c] = col[a];
        }
#pragma unroll
        for (int e = 0; e < 6; ++e) g[e] = rn[e];
        if (i + 1 == len) {   // block jn is the right separator: block q of the next level
          const size_t ns = sm_node(nx, q, K, k);
#pragma unroll
          for (int e = 0; e < 21; ++e) nx.sep[(size_t)e * nx.NS + ns] = D[e];
#pragma unroll
          for (int e = 0; e < 6; ++e) nx.sep[(size_t)(21 + e) * nx.NS + ns] = g[e];
#pragma unroll
          for (int e = 0; e < 36; ++e) nx.sep[(size_t)(54 + e) * nx.NS + ns] = G[e];
        }
      }
    }
    if (isbad) bad[k] = 1;
  }
  if (hasL) {   // (an empty last segment hands its separator zeros)
    const size_t ns = sm_node(nx, q - 1, K, k);
#pragma unroll
    for (int e = 0; e < 27; ++e) nx.sep[(size_t)(27 + e) * nx.NS + ns] = CL[e];
  }
}

// ---- the right-hand side alone of block j of a level: level 0 in its right-hand-side mode (-rhs, zero on the phantom frame), a level >= 1 as
// smooth_load sums it
template <bool LEVEL0>
MCBA_HD void smooth_load_rhs(const SmLevel& lv, const SmData& td, int K, int k, long long j, double* r) {
  if (LEVEL0) {
#pragma unroll
    for (int f = 0; f < 2; ++f) {
      const long long t = 2 * j + f;
      const bool in = (size_t)t < td.T;
      const size_t idx = in ? (size_t)t * K + k : 0;
#pragma unroll
      for (int a = 0; a < 3; ++a) r[3 * f + a] = in ? -td.rhs[3 * idx + a] : 0.0;
    }
  } else {
    const size_t nd = sm_node(lv, j, K, k);
#pragma unroll
    for (int e = 0; e < 6; ++e) r[e] = lv.sep[(size_t)(21 + e) * lv.NS + nd] + lv.sep[(size_t)(48 + e) * lv.NS + nd];
  }
}

// ---- re-solve: the forward pass of smooth_reduce_lane for a new right-hand side of a matrix it has already eliminated (level 0: in its
// right-hand-side mode).  From the stored L and L^-1 G and the coupling E formed again (level 0: its three scalars; above: the level's own
// record) it rewrites L^-1 g per interior block and the right-hand-side halves of the separator records (base 21 .. 26, cl 48 .. 53), and
// nothing else: smooth_backsub_lane follows it unchanged.  The step to the next block is r_{i+1} - E_{i+1} (L^-T L^-1 g_i): one back
// substitution with L in place of the six forward ones that make L^-1 E^T, so the result agrees with a fresh elimination to rounding, not in bits
template <bool LEVEL0>
MCBA_HD void smooth_resolve_lane(const SmLevel& lv, const SmLevel& nx, const SmData& td, int K, int k, int q) {
  const int m = lv.m, n = lv.n;
  const long long j0 = (long long)q * (m + 1);
  const bool hasL = q > 0;
  const int len = n - j0 < m ? (int)(n - j0) : m;
  double CLr[6];
#pragma unroll
  for (int e = 0; e < 6; ++e) CLr[e] = 0.0;
  if (len > 0) {
    double g[6];
    smooth_load_rhs<LEVEL0>(lv, td, K, k, j0, g);
    for (int i = 0; i < len; ++i) {
      const size_t nd = sm_node(lv, j0 + i, K, k);
      double L[21];
#pragma unroll
      for (int e = 0; e < 21; ++e) L[e] = lv.fac[(size_t)e * lv.NS + nd];
      sm_fwd6(L, g);
#pragma unroll
      for (int e = 0; e < 6; ++e) lv.fac[(size_t)(57 + e) * lv.NS + nd] = g[e];
      if (hasL) {
#pragma unroll
        for (int a = 0; a < 6; ++a) {
          double v = CLr[a];
#pragma unroll
          for (int r = 0; r < 6; ++r) v = fma(-lv.fac[(size_t)(21 + r * 6 + a) * lv.NS + nd], g[r], v);
          CLr[a] = v;
        }
      }
      const long long jn = j0 + i + 1;
      if (jn < n) {
        double rn[6], w[6];
#pragma unroll
        for (int e = 0; e < 6; ++e) w[e] = g[e];
        sm_bwd6(L, w);
        smooth_load_rhs<LEVEL0>(lv, td, K, k, jn, rn);
        if (LEVEL0) {
          double e00, e01, e11;
          sm_e0_scalars(td, k, jn, e00, e01, e11);
#pragma unroll
          for (int a = 0; a < 3; ++a) {
            rn[a] -= fma(e00, w[a], e01 * w[3 + a]);
            rn[3 + a] = fma(-e11, w[3 + a], rn[3 + a]);
          }
        } else {
          const size_t ne = sm_node(lv, jn, K, k);
#pragma unroll
          for (int r = 0; r < 6; ++r) {
            double v = rn[r];
#pragma unroll
            for (int c = 0; c < 6; ++c) v = fma(-lv.sep[(size_t)(54 + r * 6 + c) * lv.NS + ne], w[c], v);
            rn[r] = v;
          }
        }
#pragma unroll
        for (int e = 0; e < 6; ++e) g[e] = rn[e];
        if (i + 1 == len) {   // block jn is the right separator: block q of the next level
          const size_t ns = sm_node(nx, q, K, k);
#pragma unroll
          for (int e = 0; e < 6; ++e) nx.sep[(size_t)(21 + e) * nx.NS + ns] = g[e];
        }
      }
    }
  }
  if (hasL) {   // (an empty last segment hands its separator zeros)
    const size_t ns = sm_node(nx, q - 1, K, k);
#pragma unroll
    for (int e = 0; e < 6; ++e) nx.sep[(size_t)(48 + e) * nx.NS + ns] = CLr[e];
  }
}

// ---- the solution of block j: levels >= 1 keep it in lv.x; level 0 writes the frames' x, dx, d2 and the new weights
template <bool LEVEL0, bool RHS = false>
MCBA_HD void smooth_store_x(const SmLevel& lv, const SmData& td, int K, int k, long long j, const double* x) {
  if (LEVEL0 && RHS) {
#pragma unroll
    for (int f = 0; f < 2; ++f) {
      const long long t = 2 * j + f;
      if ((size_t)t >= td.T) continue;
      const size_t idx = (size_t)t * K + k;
#pragma unroll
      for (int e = 0; e < 3; ++e) td.x[3 * idx + e] = x[3 * f + e];
    }
  } else if (LEVEL0) {
#pragma unroll
    for (int f = 0; f < 2; ++f) {
      const long long t = 2 * j + f;
      if ((size_t)t >= td.T) continue;
      const size_t idx = (size_t)t * K + k;
      double dx = 0.0, d[3];
#pragma unroll
      for (int e = 0; e < 3; ++e) {
        dx = fmax(dx, fabs(x[3 * f + e] - td.x[3 * idx + e]));
        td.x[3 * idx + e] = x[3 * f + e];
        d[e] = x[3 * f + e] - td.p[3 * idx + e];
      }
      td.dx[idx] = dx;
      double wi[6];
#pragma unroll
      for (int e = 0; e < 6; ++e) wi[e] = td.winv[6 * idx + e];
      const bool usable = wi[0] != 0.0;
      double q2 = 0.0;
#pragma unroll
      for (int a = 0; a < 3; ++a) q2 = fma(d[a], fma(sym3(wi, a, 0), d[0], fma(sym3(wi, a, 1), d[1], sym3(wi, a, 2) * d[2])), q2);
      td.d2[idx] = usable ? q2 : __builtin_nan("");
      td.w[idx] = usable ? sm_drho(td.loss, q2 * td.inv_f2) : 0.0;
    }
  } else {
    const size_t nd = sm_node(lv, j, K, k);
#pragma unroll
    for (int e = 0; e < 6; ++e) lv.x[(size_t)e * lv.NS + nd] = x[e];
  }
}

// ---- back-substitution: segment q of track k on level lv; up = the level above (the solution of this level's separators)
template <bool LEVEL0, bool RHS = false>
MCBA_HD void smooth_backsub_lane(const SmLevel& lv, const SmLevel& up, const SmData& td, int K, int k, int q) {
  const int m = lv.m, n = lv.n;
  const long long j0 = (long long)q * (m + 1);
  const bool hasL = q > 0, hasR = j0 + m < n;
  const int len = n - j0 < m ? (int)(n - j0) : m;
  if (len <= 0) return;
  double xL[6], xn[6];
#pragma unroll
  for (int e = 0; e < 6; ++e) xL[e] = xn[e] = 0.0;
  if (hasL) {
    const size_t nd = sm_node(up, q - 1, K, k);
#pragma unroll
    for (int e = 0; e < 6; ++e) xL[e] = up.x[(size_t)e * up.NS + nd];
  }
  if (hasR) {
    const size_t nd = sm_node(up, q, K, k);
#pragma unroll
    for (int e = 0; e < 6; ++e) xn[e] = up.x[(size_t)e * up.NS + nd];
    smooth_store_x<LEVEL0, RHS>(lv, td, K, k, j0 + m, xn);
  }
  for (int i = len - 1; i >= 0; --i) {
    const long long j = j0 + i;
    const size_t nd = sm_node(lv, j, K, k);
    double L[21], v[6];
#pragma unroll
    for (int e = 0; e < 21; ++e) L[e] = lv.fac[(size_t)e * lv.NS + nd];
#pragma unroll
    for (int e = 0; e < 6; ++e) v[e] = lv.fac[(size_t)(57 + e) * lv.NS + nd];
    if (hasL) {
#pragma unroll
      for (int r = 0; r < 6; ++r) {
#pragma unroll
        for (int c = 0; c < 6; ++c) v[r] = fma(-lv.fac[(size_t)(21 + r * 6 + c) * lv.NS + nd], xL[c], v[r]);
      }
    }
    if (j + 1 < n) {   // u = L^-1 E_{j+1}^T x_{j+1}
      double u[6];
      if (LEVEL0) {
        double e00, e01, e11;
        sm_e0_scalars(td, k, j + 1, e00, e01, e11);
#pragma unroll
        for (int a = 0; a < 3; ++a) { u[a] = e00 * xn[a]; u[3 + a] = fma(e01, xn[a], e11 * xn[3 + a]); }
      } else {
        const size_t ne = sm_node(lv, j + 1, K, k);
#pragma unroll
        for (int c = 0; c < 6; ++c) {
          double s = 0.0;
#pragma unroll
          for (int r = 0; r < 6; ++r) s = fma(lv.sep[(size_t)(54 + r * 6 + c) * lv.NS + ne], xn[r], s);
          u[c] = s;
        }
      }
      sm_fwd6(L, u);
#pragma unroll
      for (int e = 0; e < 6; ++e) v[e] -= u[e];
    }
    sm_bwd6(L, v);
    smooth_store_x<LEVEL0, RHS>(lv, td, K, k, j, v);
#pragma unroll
    for (int e = 0; e < 6; ++e) xn[e] = v[e];
  }
}

// ---- evaluation of one (frame, track) at the solution: acc = (sum rho, sum |second difference|^2, max dx, max |x|)
MCBA_HD void smooth_eval_frame(const SmData& td, int K, int k, size_t t, double* acc) {
  const size_t idx = t * K + k;
  if (td.winv[6 * idx] != 0.0) acc[0] += sm_rho(td.loss, td.d2[idx] * td.inv_f2);
  double x[3];
#pragma unroll
  for (int e = 0; e < 3; ++e) x[e] = td.x[3 * idx + e];
  if (t >= 1 && t + 2 <= td.T) {
    const size_t a = idx - K, b = idx + K;
#pragma unroll
    for (int e = 0; e < 3; ++e) {
      const double s = td.x[3 * a + e] - 2.0 * x[e] + td.x[3 * b + e];
      acc[1] = fma(s, s, acc[1]);
    }
  }
  acc[2] = fmax(acc[2], td.dx[idx]);
  acc[3] = fmax(acc[3], fmax(fabs(x[0]), fmax(fabs(x[1]), fabs(x[2]))));
}
// the objective of a track from its sums
MCBA_HD double smooth_objective(double sum_rho, double sum_pen, double f2, double ia2) { return 0.5 * f2 * sum_rho + 0.5 * ia2 * sum_pen; }

// ---- the loop's decision for one track after solve number `it` (0-based): true = the track stops.  The first solve has no step (infinite);
// the linear loss is one solve
MCBA_HD bool smooth_stops(int loss, int it, int max_iterations, double step, double xmax, double xtol) {
  if (loss == SM_LOSS_LINEAR || it + 1 >= max_iterations) return true;
  return it >= 1 && step < xtol * xmax;
}

}  // namespace mcba
