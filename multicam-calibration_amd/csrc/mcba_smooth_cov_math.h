// mcba_smooth_cov_math.h -- the per-lane arithmetic of csrc/mcba_smooth_cov.hip: the covariance of every smoothed point,
// the band of Z = A^-1 of the system of mcba_smooth_math.h, by selected inversion over the separator tree its elimination leaves behind.
// smooth_reduce_lane keeps per interior block i of a segment (left separator l, right neighbour n = block i + 1 or the right separator) the factor
// L of D'_i and L^-1 G_i; with P = L^-T (L^-1 G_i) and Q = L^-T L^-1 E_n^T the eliminated unknown reads x_i = D'_i^-1 g'_i - P x_l - Q x_n, so
//   Z_il = -P Z_ll - Q Z_nl,   Z_in = -P Z_nl^T - Q Z_nn,   Z_ii = L^-T L^-1 - Z_il P^T - Z_in Q^T (symmetrised).
// smooth_selinv_lane walks one segment of one track from its right separator leftwards, carrying Z_nn and Z_nl (Z_ll is fixed and read at every
// step), then n <- i.  The start values are the diagonal and sub-diagonal blocks of the level above, where this level's separators q - 1 and q are neighbours; the P terms
// drop out where there is no left separator, the Q terms where no block follows; the top level is one segment, Z_last = D'^-1.
// A level >= 1 keeps per block j SM_ZC doubles, laid out as SmLevel's planes: Zd = Z_jj (21, lower packed) | Zs = Z_{j,j-1} (36, row-major; block
// 0 of a chain has none).  Every record has one writer: the lane that walks over the block, or that has it as its right separator.
// Level 0 writes what the caller gets: per frame the 3 x 3 diagonal block packed 00 01 02 11 12 22 into cov6 (T, K, 6) and, on request,
// Z_{t,t+1} row-major into lag9 (T - 1, K, 9), rows of frame t.  The phantom frame of an odd T is never written.
// Registers: P is made in place over the loaded L^-1 G, Q one column at a time (column c of Q comes from row c of E_n: contiguous, and three
// scalars on level 0) and a second time for Z_ii; every index into a lane's array is a compile-time constant.
// The same text is compiled with g++ into tests/hostcheck/smoothing_cov_hostcheck.cpp (tests/test_hostcheck_smoothing_cov.py).
#pragma once
#include "mcba_smooth_math.h"

namespace mcba {

constexpr int SM_ZC = 57;   // per block of a level >= 1: Zd (21) | Zs (36)

// device doubles (and ints, counted as doubles) one chunk of K tracks of the covariance call needs.  (Approximate on purpose, and reported as
// device_bytes: the weights plane is counted whether given or not, the lag plane as T rows, not T - 1)
inline size_t smooth_cov_chunk_doubles(size_t T, int K, int segment, bool lag) {
  SmLevel lv[SM_MAX_LEVELS];
  return (size_t)T * K * (20 + 6 + (lag ? 9 : 0)) + (size_t)K * 4 + smooth_carve(T, segment, K, lv, SM_ZC, nullptr, nullptr);
}

MCBA_HD constexpr int sm_sym(int a, int b) { return a >= b ? sm_tri(a, b) : sm_tri(b, a); }

// L^T x = y in place; b has stride `st`
MCBA_HD void sm_bwd6s(const double* L, double* b, int st) {
#pragma unroll
  for (int i = 5; i >= 0; --i) {
    double v = b[i * st];
#pragma unroll
    for (int k = i + 1; k < 6; ++k) v = fma(-L[sm_tri(k, i)], b[k * st], v);
    b[i * st] = v * L[sm_tri(i, i)];
  }
}

// column c of Q = D'_i^-1 E_n^T, n = block j + 1 of the level: row c of E_n through both triangular solves
template <bool LEVEL0, int C>
MCBA_HD void sm_q_column(const SmLevel& lv, const double* L, double e00, double e01, double e11, size_t ne, double* q) {
  if (LEVEL0) {
#pragma unroll
    for (int r = 0; r < 6; ++r) q[r] = 0.0;
    q[C] = C < 3 ? e00 : e11;
    if (C < 3) q[C < 3 ? 3 + C : C] = e01;
  } else {
#pragma unroll
    for (int r = 0; r < 6; ++r) q[r] = lv.sep[(size_t)(54 + C * 6 + r) * lv.NS + ne];
  }
  sm_fwd6(L, q);
  sm_bwd6(L, q);
}

// Z_il -= q (x) row c of Z_nl (with a left separator), Z_in -= q (x) row c of Z_nn
template <int C>
MCBA_HD void sm_q_apply(const double* q, bool hasL, const double* Znl, const double* Znn, double* Zil, double* Zin) {
#pragma unroll
  for (int a = 0; a < 6; ++a) {
#pragma unroll
    for (int b = 0; b < 6; ++b) {
      if (hasL) Zil[a * 6 + b] = fma(-q[a], Znl[C * 6 + b], Zil[a * 6 + b]);
      Zin[a * 6 + b] = fma(-q[a], Znn[sm_sym(C, b)], Zin[a * 6 + b]);
    }
  }
}

// S -= sym(column c of Z_in (x) q): the term -Z_in Q^T of Z_ii, symmetrised
template <int C>
MCBA_HD void sm_q_close(const double* q, const double* Zin, double* S) {
#pragma unroll
  for (int a = 0; a < 6; ++a) {
#pragma unroll
    for (int b = 0; b <= a; ++b) S[sm_tri(a, b)] -= 0.5 * fma(Zin[a * 6 + C], q[b], Zin[b * 6 + C] * q[a]);
  }
}

// ---- what block j of a level keeps of its diagonal block S (lower packed): levels >= 1 the record Zd; level 0 the frames' 3 x 3 blocks and the
// lag block inside the super-frame
template <bool LEVEL0>
MCBA_HD void smooth_store_zd(const SmLevel& lv, const SmData& td, double* z, double* cov6, double* lag9, int K, int k, long long j, const double* S) {
  if (LEVEL0) {
#pragma unroll
    for (int f = 0; f < 2; ++f) {
      const long long t = 2 * j + f;
      if ((size_t)t >= td.T) continue;
      double* o = cov6 + 6 * ((size_t)t * K + k);
      o[0] = S[sm_tri(3 * f, 3 * f)]; o[1] = S[sm_tri(3 * f + 1, 3 * f)]; o[2] = S[sm_tri(3 * f + 2, 3 * f)];
      o[3] = S[sm_tri(3 * f + 1, 3 * f + 1)]; o[4] = S[sm_tri(3 * f + 2, 3 * f + 1)]; o[5] = S[sm_tri(3 * f + 2, 3 * f + 2)];
    }
    if (lag9 && (size_t)(2 * j + 1) < td.T) {
      double* o = lag9 + 9 * ((size_t)(2 * j) * K + k);
#pragma unroll
      for (int a = 0; a < 3; ++a) {
#pragma unroll
        for (int b = 0; b < 3; ++b) o[a * 3 + b] = S[sm_tri(3 + b, a)];
      }
    }
  } else {
    const size_t nd = sm_node(lv, j, K, k);
#pragma unroll
    for (int e = 0; e < 21; ++e) z[(size_t)e * lv.NS + nd] = S[e];
  }
}

// ---- the block Z_{hi,lo} of two neighbours lo = hi - 1 of a level, given as M = Z_{hi,lo} (TRANSPOSED false) or M = Z_{lo,hi} (true): levels >= 1
// the record Zs of block hi; level 0 the lag block of the last frame of lo and the first of hi
template <bool LEVEL0, bool TRANSPOSED>
MCBA_HD void smooth_store_zs(const SmLevel& lv, double* z, double* lag9, int K, int k, long long hi, const double* M) {
  if (LEVEL0) {
    if (!lag9) return;
    double* o = lag9 + 9 * ((size_t)(2 * hi - 1) * K + k);   // Z_{t,t+1}, t = 2 hi - 1: rows 3 .. 5 of Z_{lo,hi}
#pragma unroll
    for (int a = 0; a < 3; ++a) {
#pragma unroll
      for (int b = 0; b < 3; ++b) o[a * 3 + b] = TRANSPOSED ? M[(3 + a) * 6 + b] : M[b * 6 + 3 + a];
    }
  } else {
    const size_t nd = sm_node(lv, hi, K, k);
#pragma unroll
    for (int r = 0; r < 6; ++r) {
#pragma unroll
      for (int c = 0; c < 6; ++c) z[(size_t)(21 + r * 6 + c) * lv.NS + nd] = TRANSPOSED ? M[c * 6 + r] : M[r * 6 + c];
    }
  }
}

// ---- selected inversion: segment q of track k on level lv.  z: this level's records (levels >= 1), zup / up: the level above (the blocks of this
// level's separators; unused on the top level), cov6 / lag9: level 0's outputs (lag9 may be null)
template <bool LEVEL0>
MCBA_HD void smooth_selinv_lane(const SmLevel& lv, const SmLevel& up, const SmData& td, double* z, const double* zup, double* cov6, double* lag9, int K, int k, int q) {
  const int m = lv.m, n = lv.n;
  const long long j0 = (long long)q * (m + 1);
  const bool hasL = q > 0, hasR = j0 + m < n;
  const int len = n - j0 < m ? (int)(n - j0) : m;
  if (len <= 0) return;
  double Znn[21], Znl[36];
#pragma unroll
  for (int e = 0; e < 21; ++e) Znn[e] = 0.0;
#pragma unroll
  for (int e = 0; e < 36; ++e) Znl[e] = 0.0;
  const size_t ndl = hasL ? sm_node(up, q - 1, K, k) : 0;
  if (hasR) {
    const size_t nd = sm_node(up, q, K, k);
#pragma unroll
    for (int e = 0; e < 21; ++e) Znn[e] = zup[(size_t)e * up.NS + nd];
    if (hasL) {
#pragma unroll
      for (int e = 0; e < 36; ++e) Znl[e] = zup[(size_t)(21 + e) * up.NS + nd];
    }
    smooth_store_zd<LEVEL0>(lv, td, z, cov6, lag9, K, k, j0 + m, Znn);
  }
  for (int i = len - 1; i >= 0; --i) {
    const long long j = j0 + i;
    const size_t nd = sm_node(lv, j, K, k);
    const bool hasN = j + 1 < n;
    double L[21], P[36], Zil[36], Zin[36], S[21];
#pragma unroll
    for (int e = 0; e < 21; ++e) L[e] = lv.fac[(size_t)e * lv.NS + nd];
#pragma unroll
    for (int e = 0; e < 36; ++e) Zil[e] = Zin[e] = P[e] = 0.0;
    if (hasL) {
#pragma unroll
      for (int e = 0; e < 36; ++e) P[e] = lv.fac[(size_t)(21 + e) * lv.NS + nd];
#pragma unroll
      for (int c = 0; c < 6; ++c) sm_bwd6s(L, P + c, 6);
      double Zll[21];   // (read again at every step: it would be 21 more live doubles through the whole walk)
#pragma unroll
      for (int e = 0; e < 21; ++e) Zll[e] = zup[(size_t)e * up.NS + ndl];
#pragma unroll
      for (int a = 0; a < 6; ++a) {
#pragma unroll
        for (int b = 0; b < 6; ++b) {
          double v = 0.0, u = 0.0;
#pragma unroll
          for (int c = 0; c < 6; ++c) {
            v = fma(-P[a * 6 + c], Zll[sm_sym(c, b)], v);
            u = fma(-P[a * 6 + c], Znl[b * 6 + c], u);
          }
          Zil[a * 6 + b] = v;
          Zin[a * 6 + b] = hasN ? u : 0.0;
        }
      }
    }
    double e00 = 0.0, e01 = 0.0, e11 = 0.0;
    size_t ne = 0;
    if (hasN) {
      if (LEVEL0) sm_e0_scalars(td, k, j + 1, e00, e01, e11);
      else ne = sm_node(lv, j + 1, K, k);
      double qc[6];
      sm_q_column<LEVEL0, 0>(lv, L, e00, e01, e11, ne, qc); sm_q_apply<0>(qc, hasL, Znl, Znn, Zil, Zin);
      sm_q_column<LEVEL0, 1>(lv, L, e00, e01, e11, ne, qc); sm_q_apply<1>(qc, hasL, Znl, Znn, Zil, Zin);
      sm_q_column<LEVEL0, 2>(lv, L, e00, e01, e11, ne, qc); sm_q_apply<2>(qc, hasL, Znl, Znn, Zil, Zin);
      sm_q_column<LEVEL0, 3>(lv, L, e00, e01, e11, ne, qc); sm_q_apply<3>(qc, hasL, Znl, Znn, Zil, Zin);
      sm_q_column<LEVEL0, 4>(lv, L, e00, e01, e11, ne, qc); sm_q_apply<4>(qc, hasL, Znl, Znn, Zil, Zin);
      sm_q_column<LEVEL0, 5>(lv, L, e00, e01, e11, ne, qc); sm_q_apply<5>(qc, hasL, Znl, Znn, Zil, Zin);
      smooth_store_zs<LEVEL0, true>(lv, z, lag9, K, k, j + 1, Zin);
    }
    if (i == 0 && hasL) smooth_store_zs<LEVEL0, false>(lv, z, lag9, K, k, j, Zil);
    // Z_ii: D'^-1 a column at a time, then the two products
#pragma unroll
    for (int c = 0; c < 6; ++c) {
      double u[6];
#pragma unroll
      for (int r = 0; r < 6; ++r) u[r] = r == c ? 1.0 : 0.0;
      sm_fwd6(L, u);
      sm_bwd6(L, u);
#pragma unroll
      for (int a = c; a < 6; ++a) S[sm_tri(a, c)] = u[a];
    }
    if (hasL) {
#pragma unroll
      for (int a = 0; a < 6; ++a) {
#pragma unroll
        for (int b = 0; b <= a; ++b) {
          double v = 0.0;
#pragma unroll
          for (int c = 0; c < 6; ++c) v += fma(Zil[a * 6 + c], P[b * 6 + c], Zil[b * 6 + c] * P[a * 6 + c]);
          S[sm_tri(a, b)] -= 0.5 * v;
        }
      }
    }
    if (hasN) {
      double qc[6];
      sm_q_column<LEVEL0, 0>(lv, L, e00, e01, e11, ne, qc); sm_q_close<0>(qc, Zin, S);
      sm_q_column<LEVEL0, 1>(lv, L, e00, e01, e11, ne, qc); sm_q_close<1>(qc, Zin, S);
      sm_q_column<LEVEL0, 2>(lv, L, e00, e01, e11, ne, qc); sm_q_close<2>(qc, Zin, S);
      sm_q_column<LEVEL0, 3>(lv, L, e00, e01, e11, ne, qc); sm_q_close<3>(qc, Zin, S);
      sm_q_column<LEVEL0, 4>(lv, L, e00, e01, e11, ne, qc); sm_q_close<4>(qc, Zin, S);
      sm_q_column<LEVEL0, 5>(lv, L, e00, e01, e11, ne, qc); sm_q_close<5>(qc, Zin, S);
    }
    smooth_store_zd<LEVEL0>(lv, td, z, cov6, lag9, K, k, j, S);
#pragma unroll
    for (int e = 0; e < 21; ++e) Znn[e] = S[e];
#pragma unroll
    for (int e = 0; e < 36; ++e) Znl[e] = Zil[e];
  }
}

}  // namespace mcba
