// mcba_sparse.hip -- the kernels of the sparse-Schur handle (mcba_create_sparse): rigs of any number of cameras.
//
// The dense handle forms S = U - sum_f Y_f Y_f^T over all 12C + 1 rows per frame (k_syrk) and factorises the reduced system in one
// workgroup (k_solve_cam): both are sized for <= 40 cameras.  A wide rig is sparse -- a board pose is seen by a handful of its cameras --
// so here the reduction runs over the CO-VISIBLE camera pairs only, and the reduced system is factorised by a stream-ordered sequence
// of multi-workgroup launches.  Every per-(camera, frame) kernel (k_gram, k_cost, k_backsub, k_sum_trial, ...) is shared with the dense
// handle unchanged; the reduce buffer has the dense layout (S0 | rhs | diag U | g_c | scalars), so the frame-sharded all-reduce applies.
//
//   k_sp_seen      (upload)  which (camera, frame) pairs have a detection: the host builds the visibility index from it
//   k_sp_factor    per frame: V_f = sum over its cameras of V_cf, Marquardt / x_scale damping, L L^T = V_f + lambda D_f, z = L^-1 g_f
//                  -> fbuf (the MCBA_FB layout k_backsub reads); per workgroup {max |g_f|, #failed factorisations} -> fpart
//   k_sp_y         per seen (camera, frame) and row: Y_cf = W_cf L_f^-T  (cw x 6 per entry, entry order = the visibility index's)
//   k_sp_pairs     per chunk of <= 64 frames of a co-visible pair (i <= j): sum Y_i Y_j^T, and for i == j also sum Y_i z
//   k_sp_assemble  per (camera block i, camera block j) of S0: the pair's chunk sums in chunk order, U_c on the diagonal blocks,
//                  rhs_c = sum Y_c z - g_c; zero blocks where two cameras share no frame
//   (diag U, g_c and the scalars: k_reduce_system's tail, launched with no tile pairs)
//   k_sp_solve_pre / k_sp_load / {k_sp_potrf, k_sp_trsm, k_sp_update} x blocks / k_sp_finish: right-looking blocked Cholesky, block
//                  64, of the system augmented with the right-hand side as row n (L y = rhs falls out as row n of the factor), the
//                  trailing update on v_mfma_f64_16x16x4_f64; the LM bookkeeping of k_solve_cam (termination, gtol, failed factorisation
//                  -> more damping and a rebuild-only tick) in the first and last launch.
// Every sum has a fixed order; there are no floating-point atomics.
#include <hip/hip_runtime.h>
#include <stdlib.h>
#include <algorithm>
#include "mcba_kernels.h"
#include "mcba_device.h"
#include "mcba_lm.h"
#include "mcba_math.h"

namespace mcba {

// ---------------------------------------------------------------- visibility: seen[c * F + f] = any finite scalar in (c, f)
__global__ __launch_bounds__(256) void k_sp_seen(const double* __restrict__ obs_raw, unsigned char* __restrict__ seen, int C, int F, int N) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= (size_t)C * F) return;
  const double* p = obs_raw + i * 2 * N;
  bool any = false;
  for (int k = 0; k < 2 * N; ++k) any = any || (p[k] == p[k]);
  seen[i] = any ? 1 : 0;
}
void launch_sp_seen(hipStream_t st, const double* obs_raw, unsigned char* seen, int C, int F, int N) {
  const size_t cnt = (size_t)C * F;
  k_sp_seen<<<dim3((unsigned)((cnt + 255) / 256)), dim3(256), 0, st>>>(obs_raw, seen, C, F, N);
}

// ---------------------------------------------------------------- frame factors (lane = frame): k_syrk's stage 1 over the frame's own cameras
// V_f is summed over the seen cameras in ascending order -- the dense kernel adds the same terms in the same order (plus exact zeros).
template <bool XS>
__global__ __launch_bounds__(64) void k_sp_factor(Sel sl, const double* __restrict__ rec0, const double* __restrict__ rec1, double* __restrict__ fbuf, double* __restrict__ fpart,
                                                  const int* __restrict__ frame_off, const int* __restrict__ ent_cam, const double* __restrict__ dscale, int C, int F, int Fpad) {
  if (!sel_active(sl, false)) return;
  const int f = blockIdx.x * 64 + threadIdx.x, nfb = Fpad >> 6;
  const double lambda = sel_lambda(sl);
  const double* __restrict__ rec = sel_index(sl) ? rec1 : rec0;
  double gmax = 0.0, nfail = 0.0;
  if (f < F) {
    double V[28];
#pragma unroll
    for (int k = 0; k < 28; ++k) V[k] = 0.0;
    for (int e = frame_off[f]; e < frame_off[f + 1]; ++e) {
      const int c = ent_cam[e];
      const double2* r2 = reinterpret_cast<const double2*>(rec + ((size_t)c * nfb + (f >> 6)) * (MCBA_REC * 64)) + (size_t)36 * 64 + (f & 63);
#pragma unroll
      for (int k = 0; k < 14; ++k) { const double2 v = r2[(size_t)k * 64]; V[2 * k] += v.x; V[2 * k + 1] += v.y; }
    }
    double* gf = V + 21;
    double D[6], dsv[6];
#pragma unroll
    for (int k = 0; k < 6; ++k) {
      const double d = V[tri6(k, k)];
      const double ds = XS ? dscale[(size_t)12 * C + 6 * (size_t)f + k] : 0.0;
      D[k] = ds > 0.0 ? ds : (d > 0.0 ? d : 1.0);
      dsv[k] = ds;
      V[tri6(k, k)] = d + lambda * D[k];
    }
    double gfm[6];
    unsigned fm = 0;
#pragma unroll
    for (int k = 0; k < 6; ++k) { gfm[k] = gf[k]; if (XS && dsv[k] < 0.0) fm |= 1u << k; }
    if (XS && fm) {   // frozen coordinates (mcba_set_frozen): identity row / column, zero gradient -- as k_syrk
#pragma unroll
      for (int k = 0; k < 6; ++k) {
        if ((fm >> k) & 1u) {
#pragma unroll
          for (int j = 0; j < 6; ++j) V[j <= k ? tri6(j, k) : tri6(k, j)] = j == k ? 1.0 : 0.0;
          gfm[k] = 0.0;
        }
      }
    }
    double Lp[21], id[6], z[6];
    const bool ok = chol6i(V, Lp);
#pragma unroll
    for (int k = 0; k < 6; ++k) id[k] = Lp[k * (k + 1) / 2 + k];
    fwd6(Lp, id, gfm, z);
#pragma unroll
    for (int k = 0; k < 6; ++k) gmax = fmax(gmax, fabs(gfm[k]));
    nfail = ok ? 0.0 : 1.0;
    double o[40];
#pragma unroll
    for (int k = 0; k < 21; ++k) o[k] = Lp[k];
#pragma unroll
    for (int k = 0; k < 6; ++k) { o[21 + k] = z[k]; o[27 + k] = gf[k]; o[33 + k] = D[k]; }
    o[39] = XS ? (double)fm : 0.0;
    double* fbp = fbuf + (size_t)f * MCBA_FB;
#pragma unroll
    for (int k = 0; k < 40; k += 2) *reinterpret_cast<double2*>(fbp + k) = make_double2(o[k], o[k + 1]);
  }
  const double wm = wave_max(gmax), wn = wave_sum(nfail);
  if (threadIdx.x == 0) { fpart[2 * blockIdx.x] = wm; fpart[2 * blockIdx.x + 1] = wn; }
}

// ---------------------------------------------------------------- Y_cf = W_cf L_f^-T: thread = (entry, row)
__global__ __launch_bounds__(256) void k_sp_y(Sel sl, const double* __restrict__ rec0, const double* __restrict__ rec1, const double* __restrict__ fbuf, const int* __restrict__ ent_cam,
                                              const int* __restrict__ ent_frame, int nent, double* __restrict__ Y, int Fpad, int cw) {
  if (!sel_active(sl, false)) return;
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= (size_t)nent * cw) return;
  const int e = (int)(i / cw), r = (int)(i - (size_t)e * cw);
  const int c = ent_cam[e], f = ent_frame[e], nfb = Fpad >> 6, lr = r + 12 - cw;
  const double* __restrict__ rec = sel_index(sl) ? rec1 : rec0;
  const double2* w2 = reinterpret_cast<const double2*>(rec + ((size_t)c * nfb + (f >> 6)) * (MCBA_REC * 64)) + (size_t)(3 * lr) * 64 + (f & 63);
  double w[6];
#pragma unroll
  for (int k = 0; k < 3; ++k) { const double2 v = w2[(size_t)k * 64]; w[2 * k] = v.x; w[2 * k + 1] = v.y; }
  const double* fb = fbuf + (size_t)f * MCBA_FB;
  double Lp[21], id[6], y[6];
#pragma unroll
  for (int k = 0; k < 21; ++k) Lp[k] = fb[k];
#pragma unroll
  for (int k = 0; k < 6; ++k) id[k] = Lp[k * (k + 1) / 2 + k];
  const unsigned fm = (unsigned)fb[39];   // frozen coordinates: their column of W counts as zero
#pragma unroll
  for (int k = 0; k < 6; ++k) w[k] = ((fm >> k) & 1u) ? 0.0 : w[k];
  fwd6(Lp, id, w, y);
  double* o = Y + ((size_t)e * 12 + r) * 6;
#pragma unroll
  for (int k = 0; k < 6; ++k) o[k] = y[k];
}

void launch_sp_factor(hipStream_t st, Sel s, const double* rec0, const double* rec1, double* fbuf, double* fpart, const int* frame_off, const int* ent_cam, const int* ent_frame, int nent,
                      double* Y, const double* dscale, int C, int F, int Fpad, int cw) {
  if (dscale) k_sp_factor<true><<<dim3(Fpad / 64), dim3(64), 0, st>>>(s, rec0, rec1, fbuf, fpart, frame_off, ent_cam, dscale, C, F, Fpad);
  else k_sp_factor<false><<<dim3(Fpad / 64), dim3(64), 0, st>>>(s, rec0, rec1, fbuf, fpart, frame_off, ent_cam, dscale, C, F, Fpad);
  if (nent > 0) {
    const size_t items = (size_t)nent * cw;
    k_sp_y<<<dim3((unsigned)((items + 255) / 256)), dim3(256), 0, st>>>(s, rec0, rec1, fbuf, ent_cam, ent_frame, nent, Y, Fpad, cw);
  }
}

// ---------------------------------------------------------------- pair chunks: thread t < cw^2 = element (a, b) of sum Y_i Y_j^T, t in [cw^2, cw^2 + cw): row a of sum Y_i z (i == j)
// items: per pair-frame (entry of camera i, entry of camera j, frame), in pair order and ascending frame order inside a pair.
constexpr int kSpStage = 16;
__global__ __launch_bounds__(256) void k_sp_pairs(Sel sl, const double* __restrict__ Y, const double* __restrict__ fbuf, const int* __restrict__ items, const int* __restrict__ chunks,
                                                  double* __restrict__ part, int cw) {
  if (!sel_active(sl, false)) return;
  __shared__ double s_yi[kSpStage][72], s_yj[kSpStage][72], s_z[kSpStage][6];
  const int ch = blockIdx.x, t = threadIdx.x;
  const int first = chunks[3 * ch], count = chunks[3 * ch + 1], diag = chunks[3 * ch + 2];
  const int a = t < cw * cw ? t / cw : t - cw * cw, b = t < cw * cw ? t - cw * (t / cw) : 0;
  const bool elem = t < cw * cw, rhs = diag && t >= cw * cw && t < cw * cw + cw;
  const int per = cw * 6;
  double acc = 0.0;
  for (int base = 0; base < count; base += kSpStage) {
    const int ns = min(kSpStage, count - base);
    for (int k = t; k < ns * (2 * per + 6); k += 256) {
      const int m = k / (2 * per + 6), q = k - m * (2 * per + 6);
      const int* it = items + 3 * (size_t)(first + base + m);
      if (q < per) s_yi[m][q] = Y[(size_t)it[0] * 72 + q];
      else if (q < 2 * per) s_yj[m][q - per] = Y[(size_t)it[1] * 72 + (q - per)];
      else s_z[m][q - 2 * per] = fbuf[(size_t)it[2] * MCBA_FB + 21 + (q - 2 * per)];
    }
    __syncthreads();
    if (elem) {
      for (int m = 0; m < ns; ++m) {
#pragma unroll
        for (int k = 0; k < 6; ++k) acc = fma(s_yi[m][6 * a + k], s_yj[m][6 * b + k], acc);
      }
    } else if (rhs) {
      for (int m = 0; m < ns; ++m) {
#pragma unroll
        for (int k = 0; k < 6; ++k) acc = fma(s_yi[m][6 * a + k], s_z[m][k], acc);
      }
    }
    __syncthreads();
  }
  if (elem || rhs) part[(size_t)ch * 160 + t] = acc;
}

// ---------------------------------------------------------------- S0 and rhs, one workgroup per (camera block bi, camera block bj)
// pair_map[i * C + j] (i <= j): pair id or -1; pair_chunks[p] .. pair_chunks[p + 1]: the pair's chunks, in frame order.
__global__ __launch_bounds__(256) void k_sp_assemble(Sel sl, const double* __restrict__ gp0, const double* __restrict__ gp1, const double* __restrict__ part, const int* __restrict__ pair_map,
                                                     const int* __restrict__ pair_chunks, double* __restrict__ red, int C, int nfb, int cw) {
  if (!sel_active(sl, false)) return;
  const int bi = blockIdx.x, bj = blockIdx.y, t = threadIdx.x, n = cw * C, coff = 12 - cw;
  const bool diag = bi == bj;
  if (t >= cw * cw + (diag ? cw : 0)) return;
  const int lo = min(bi, bj), hi = max(bi, bj);
  const int p = pair_map[(size_t)lo * C + hi];
  const double* __restrict__ gpart = sel_index(sl) ? gp1 : gp0;
  const size_t camstride = (size_t)MCBA_GP * nfb;
  double v = 0.0;
  int a, b, slot;
  if (t < cw * cw) {
    a = t / cw; b = t - cw * a;
    slot = bi <= bj ? a * cw + b : b * cw + a;   // the pair's block is (lo, hi): (hi, lo) is its transpose
  } else {
    a = t - cw * cw; b = 0;
    slot = t;
  }
  if (p >= 0) {
    for (int q = pair_chunks[p]; q < pair_chunks[p + 1]; ++q) v += part[(size_t)q * 160 + slot];
  }
  if (t < cw * cw) {
    double u = 0.0;
    if (diag) {
      const int la = a + coff, lb = b + coff;
      const double* up = gpart + (size_t)bi * camstride + (size_t)tri12(min(la, lb), max(la, lb)) * nfb;
      for (int k = 0; k < nfb; ++k) u += up[k];
    }
    red[(size_t)(bi * cw + a) * n + bj * cw + b] = u - v;   // S0 = blockdiag(U) - sum Y Y^T
  } else {
    const double* gp = gpart + (size_t)bi * camstride + (size_t)(78 + a + coff) * nfb;
    double g = 0.0;
    for (int k = 0; k < nfb; ++k) g += gp[k];
    red[(size_t)n * n + bi * cw + a] = v - g;   // rhs = sum Y z - g_c
  }
}

void launch_sp_pairs(hipStream_t st, Sel s, const double* Y, const double* fbuf, const int* items, const int* chunks, int nchunks, double* part, const double* gp0, const double* gp1,
                     const int* pair_map, const int* pair_chunks, double* red, int C, int nfb, int cw) {
  if (nchunks > 0) k_sp_pairs<<<dim3(nchunks), dim3(256), 0, st>>>(s, Y, fbuf, items, chunks, part, cw);
  k_sp_assemble<<<dim3(C, C), dim3(256), 0, st>>>(s, gp0, gp1, part, pair_map, pair_chunks, red, C, nfb, cw);
}

// ================================================================ the reduced solve
// ctl[0]: 0 factorise and solve, 1 nothing to do (terminated: the state is posted), 2 no solve possible (a frame block failed);
// ctl[1]: 1 = a pivot of the factorisation was not positive / not finite.  Every launch after k_sp_solve_pre reads them first.
constexpr int kSpNB = 64;

// LM state -> device state and the host-mapped ring slot; the sequence number goes last (as post_state in mcba_solve.hip)
__device__ __forceinline__ void sp_post_state(const SolveArgs& a, const double* st, bool write_back) {
  const int tid = threadIdx.x;
  if (tid < MCBA_LMS - 1) {
    const double v = st[tid];
    if (write_back) a.lms[tid] = v;
    if (a.host_state) a.host_state[tid] = v;
  }
  if (!a.host_state) return;
  __threadfence_system();
  __syncthreads();
  if (tid == 0) *reinterpret_cast<volatile double*>(a.host_state + MCBA_LMS - 1) = a.seq;
}

__device__ __forceinline__ double sp_block_reduce(double v, bool take_max, double* s_red) {  // 256 threads
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) { const double o = __shfl_xor(v, off, 64); v = take_max ? fmax(v, o) : v + o; }
  __syncthreads();
  if (lane == 0) s_red[wave] = v;
  __syncthreads();
  double r = s_red[0];
  for (int w = 1; w < 4; ++w) r = take_max ? fmax(r, s_red[w]) : r + s_red[w];
  return r;
}

// first-order optimality, termination verdicts, the damping of this solve (k_solve_cam's prologue).  One workgroup of 256.
__global__ __launch_bounds__(256) void k_sp_solve_pre(SolveArgs a, int* __restrict__ ctl, double* __restrict__ damp) {
  __shared__ double lst[MCBA_LMS];
  __shared__ double s_red[8];
  __shared__ int s_mode;
  const int n = a.n, tid = threadIdx.x;
  const double* __restrict__ diagU = a.red + (size_t)n * n + n;
  const double* __restrict__ gc = diagU + n;
  const double* __restrict__ scal = gc + n;
  if (tid < MCBA_LMS) lst[tid] = a.lms_in[tid];
  double gm = 0.0;
  for (int i = tid; i < n; i += 256) {
    if (!(a.fixed && a.fixed[i])) gm = fmax(gm, fabs(gc[i]));
  }
  if (tid < 12) gm = fmax(gm, scal[4 + tid]);
  const double g_inf = sp_block_reduce(gm, true, s_red);
  if (lst[MCBA_LM_DONE] != 0.0) {
    if (tid == 0) { ctl[0] = 1; ctl[1] = 0; }
    sp_post_state(a, lst, false);
    return;
  }
  if (tid == 0) {
    int mode = 0;
    lst[MCBA_LM_TICK] += 1.0;
    lst[MCBA_LM_GINF] = g_inf;
    const double pending = lst[MCBA_LM_PENDING];
    if (pending != 0.0) { lst[MCBA_LM_DONE] = pending; mode = 1; }
    else if (g_inf < a.gtol) { lst[MCBA_LM_DONE] = 1.0; mode = 1; }
    else if (scal[2] != 0.0) mode = 2;
    s_mode = mode;
    ctl[0] = mode;
    ctl[1] = 0;
  }
  __syncthreads();
  const int mode = s_mode;
  if (mode == 1) {
    sp_post_state(a, lst, true);
    return;
  }
  const double lambda = lst[1];
  for (int i = tid; i < a.npad; i += 256) {
    double d = 1.0;
    if (i < n) {
      const double dsc = a.dscale ? a.dscale[a.cw == 12 ? i : 12 * (i / 6) + 6 + i % 6] : 0.0;
      const double du = dsc > 0.0 ? dsc : diagU[i];
      d = du > 0.0 ? du : 1.0;
    }
    damp[i] = lambda * d;
  }
  if (tid < MCBA_LMS - 1) a.lms[tid] = lst[tid];   // (k_sp_finish continues from here; the ring slot is posted there)
}

// the augmented damped matrix, lower triangle: rows < n S0 + lambda D_c, row n the right-hand side (1 on the diagonal), rows > n identity;
// parameters held fixed get an identity row and column and a zero right-hand side.  Thread = element; A is npad x npad, row-major.
__global__ __launch_bounds__(256) void k_sp_load(const double* __restrict__ red, const unsigned char* __restrict__ fixed, const double* __restrict__ damp, const int* __restrict__ ctl,
                                                 double* __restrict__ A, int n, int npad) {
  if (ctl[0] != 0) return;
  const int j = blockIdx.x * 256 + threadIdx.x;
  for (int i = blockIdx.y; i < npad; i += gridDim.y) {   // (rows strided: the grid's y extent is bounded)
  if (j > i || j >= npad) continue;
  double v;
  if (i < n) {
    v = red[(size_t)i * n + j];
    if (i == j) v += damp[i];
    if (fixed && (fixed[i] || fixed[j])) v = i == j ? 1.0 : 0.0;
  } else if (i == n) {
    v = j < n ? ((fixed && fixed[j]) ? 0.0 : red[(size_t)n * n + j]) : 1.0;
  } else {
    v = i == j ? 1.0 : 0.0;
  }
  A[(size_t)i * npad + j] = v;
  }
}

// diagonal block k: Cholesky in LDS by one wavefront (lane = row), left-looking by columns.  Row n (the right-hand side) gets the pivot 1.
__global__ __launch_bounds__(64) void k_sp_potrf(double* __restrict__ A, int* __restrict__ ctl, int n, int npad, int k) {
  if (ctl[0] != 0 || ctl[1] != 0) return;
  __shared__ double L[kSpNB][kSpNB + 1];
  const int lane = threadIdx.x, r0 = kSpNB * k;
  for (int c = 0; c < kSpNB; ++c) L[lane][c] = c <= lane ? A[(size_t)(r0 + lane) * npad + r0 + c] : 0.0;
  __syncthreads();
  bool bad = false;
  for (int j = 0; j < kSpNB; ++j) {
    double s = L[lane][j];
    for (int m = 0; m < j; ++m) s = fma(-L[lane][m], L[j][m], s);
    __syncthreads();
    if (lane == j) {
      double piv;
      if (r0 + j == n) piv = 1.0;
      else if (s > 0.0 && s < INFINITY) piv = sqrt(s);
      else { piv = 1.0; bad = true; }
      L[j][j] = piv;
    }
    __syncthreads();
    if (lane > j) L[lane][j] = s / L[j][j];
    __syncthreads();
  }
  for (int c = 0; c <= lane; ++c) A[(size_t)(r0 + lane) * npad + r0 + c] = L[lane][c];
  if (__any(bad) && lane == 0) ctl[1] = 1;
}

// panel below the diagonal block: L_ik = A_ik L_kk^-T, thread = row.  L_kk packed (lower triangle, read as broadcasts), the rows
// column-major in LDS (lane t reads X[m][t]: consecutive banks)
__global__ __launch_bounds__(64) void k_sp_trsm(double* __restrict__ A, const int* __restrict__ ctl, int npad, int k) {
  if (ctl[0] != 0 || ctl[1] != 0) return;
  __shared__ double L[kSpNB * (kSpNB + 1) / 2];
  __shared__ double X[kSpNB][64];
  const int t = threadIdx.x, r0 = kSpNB * k;
  for (int c = 0; c <= t; ++c) L[t * (t + 1) / 2 + c] = A[(size_t)(r0 + t) * npad + r0 + c];
  const int row = r0 + kSpNB + blockIdx.x * 64 + t;
  const bool on = row < npad;
  double* ap = A + (size_t)(on ? row : r0) * npad + r0;
  for (int c = 0; c < kSpNB; ++c) X[c][t] = on ? ap[c] : 0.0;
  __syncthreads();
  for (int j = 0; j < kSpNB; ++j) {
    const double* lj = L + j * (j + 1) / 2;
    double s = X[j][t];
    for (int m = 0; m < j; ++m) s = fma(-X[m][t], lj[m], s);
    X[j][t] = s / lj[j];
  }
  if (on) for (int c = 0; c < kSpNB; ++c) ap[c] = X[c][t];
}

// trailing update A_IJ -= L_Ik L_Jk^T for k < J <= I: one 64 x 64 tile per workgroup, wavefront w a 32 x 32 quadrant (2 x 2 MFMA tiles),
// the K = 64 panel columns in two LDS stages of 32
typedef double sp_d4 __attribute__((ext_vector_type(4)));
__global__ __launch_bounds__(256) void k_sp_update(double* __restrict__ A, const int* __restrict__ ctl, int npad, int k, int nblk) {
  if (ctl[0] != 0 || ctl[1] != 0) return;
  __shared__ double Li[kSpNB][33], Lj[kSpNB][33];
  // tile id -> (I, J), J <= I, both in (k, nblk)
  int q = blockIdx.x, I = k + 1;
  while (q > I - (k + 1)) { q -= I - k; ++I; }
  const int J = k + 1 + q;
  const int t = threadIdx.x, wave = t >> 6, lane = t & 63;
  const int qr = (wave >> 1) * 32, qc = (wave & 1) * 32;
  sp_d4 acc[2][2];
#pragma unroll
  for (int x = 0; x < 2; ++x)
#pragma unroll
    for (int y = 0; y < 2; ++y) acc[x][y] = sp_d4{0.0, 0.0, 0.0, 0.0};
  for (int kh = 0; kh < kSpNB; kh += 32) {
    for (int e = t; e < kSpNB * 32; e += 256) {
      const int r = e >> 5, c = e & 31;
      Li[r][c] = A[(size_t)(kSpNB * I + r) * npad + kSpNB * k + kh + c];
      Lj[r][c] = A[(size_t)(kSpNB * J + r) * npad + kSpNB * k + kh + c];
    }
    __syncthreads();
#pragma unroll
    for (int ks = 0; ks < 8; ++ks) {
      const int kk = 4 * ks + (lane >> 4);
      double av[2], bv[2];
#pragma unroll
      for (int x = 0; x < 2; ++x) av[x] = Li[qr + 16 * x + (lane & 15)][kk];
#pragma unroll
      for (int y = 0; y < 2; ++y) bv[y] = Lj[qc + 16 * y + (lane & 15)][kk];
#pragma unroll
      for (int x = 0; x < 2; ++x)
#pragma unroll
        for (int y = 0; y < 2; ++y) acc[x][y] = __builtin_amdgcn_mfma_f64_16x16x4f64(av[x], bv[y], acc[x][y], 0, 0, 0);
    }
    __syncthreads();
  }
  // D layout of v_mfma_f64_16x16x4_f64: col = lane & 15, row = (lane >> 4) + 4 reg
#pragma unroll
  for (int x = 0; x < 2; ++x)
#pragma unroll
    for (int y = 0; y < 2; ++y)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = kSpNB * I + qr + 16 * x + (lane >> 4) + 4 * r, col = kSpNB * J + qc + 16 * y + (lane & 15);
        A[(size_t)row * npad + col] -= acc[x][y][r];
      }
}

// backward sweep L^T d = y (y = row n of the factor), the camera step, the step scalars and the failure handling of k_solve_cam; posts the
// state.  One workgroup of 256; y (npad doubles) lives in device memory -- no LDS bound on the number of cameras -- and is touched by this
// workgroup alone (every element by one thread per phase, barriers between the phases); the diagonal block goes through LDS.
__global__ __launch_bounds__(256) void k_sp_finish(SolveArgs a, const int* __restrict__ ctl, const double* __restrict__ A, const double* __restrict__ damp, double* __restrict__ y) {
  __shared__ double Lk[kSpNB * (kSpNB + 1)];
  __shared__ double lst[MCBA_LMS];
  __shared__ double s_red[8];
  const int n = a.n, npad = a.npad, nblk = npad / kSpNB, tid = threadIdx.x;
  const int mode = ctl[0];
  if (mode == 1) return;   // k_sp_solve_pre posted the state already
  const bool fact_ok = ctl[1] == 0;
  if (tid < MCBA_LMS) lst[tid] = a.lms[tid];
  const double* __restrict__ gc = a.red + (size_t)n * n + 2 * n;
  const bool solve = mode == 0 && fact_ok;
  if (solve) {
    for (int j = tid; j < npad; j += 256) y[j] = j < n ? A[(size_t)n * npad + j] : 0.0;
    __syncthreads();
    for (int kb = nblk - 1; kb >= 0; --kb) {
      const int r0 = kSpNB * kb;
      for (int e = tid; e < kSpNB * kSpNB; e += 256) {
        const int r = e / kSpNB, c = e - r * kSpNB;
        Lk[r * (kSpNB + 1) + c] = c <= r ? A[(size_t)(r0 + r) * npad + r0 + c] : 0.0;
      }
      __syncthreads();
      if (tid < 64) {   // L_kk^T d_k = y_k, column-oriented: lane m keeps y_(r0 + m)
        double ym = y[r0 + tid];
        for (int j = kSpNB - 1; j >= 0; --j) {
          const double dj = __shfl(ym, j, 64) / Lk[j * (kSpNB + 1) + j];
          if (tid == j) ym = dj;
          else if (tid < j) ym = fma(-Lk[j * (kSpNB + 1) + tid], dj, ym);
        }
        y[r0 + tid] = r0 + tid < n ? ym : 0.0;   // (row n and the padding: no unknowns)
      }
      __syncthreads();
      for (int j = tid; j < r0; j += 256) {
        double s0 = y[j], s1 = 0.0;
        for (int t = 0; t < kSpNB; t += 2) {
          s0 = fma(-A[(size_t)(r0 + t) * npad + j], y[r0 + t], s0);
          s1 = fma(-A[(size_t)(r0 + t + 1) * npad + j], y[r0 + t + 1], s1);
        }
        y[j] = s0 + s1;
      }
      __syncthreads();
    }
  }
  __syncthreads();
  const double lambda = lst[1];
  const int sel = static_cast<int>(lst[3]) & 1;
  const double* xc = sel ? a.x1 : a.x0;
  double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
  if (solve) {
    for (int i = tid; i < n; i += 256) {
      const double d = y[i], xv = xc[a.cw == 12 ? i : 12 * (i / 6) + 6 + i % 6];
      a.dc[i] = d;
      s3 += (fabs(d) < 1e300) ? 0.0 : 1.0;
      s0 += d * (damp[i] * d - gc[i]);
      s1 += d * d;
      s2 += xv * xv;
    }
  }
  s0 = sp_block_reduce(s0, false, s_red);
  s1 = sp_block_reduce(s1, false, s_red);
  s2 = sp_block_reduce(s2, false, s_red);
  s3 = sp_block_reduce(s3, false, s_red);
  if (tid == 0) {
    const bool failed = !solve || s3 != 0.0 || !(fabs(s0) < 1e300);
    lst[MCBA_LM_SOLVE_INFO] = mode == 2 ? 2.0 : failed ? 1.0 : 0.0;
    if (failed) {   // more damping; the next tick rebuilds the reduced system without a trial step
      const double lam = fmin(lambda * lst[2], a.lam_max);
      lst[1] = lam;
      lst[2] *= 2.0;
      lst[MCBA_LM_SKIP] = 1.0;
      if (lam >= a.lam_max) lst[MCBA_LM_DONE] = 3.0;
    } else {
      lst[MCBA_LM_SKIP] = 0.0;
      lst[MCBA_LM_PRED_CAM] = s0;
      lst[MCBA_LM_DCN2] = s1;
      lst[MCBA_LM_XCN2] = s2;
    }
  }
  __syncthreads();
  sp_post_state(a, lst, true);
}

int sp_npad(int n) { return (n + 1 + kSpNB - 1) / kSpNB * kSpNB; }

// the launches of one reduced solve; bracket(ctx, stage, begin) around each stage for profiling: 0 pre + load, 1 potrf, 2 trsm, 3 update, 4 finish
void launch_sp_solve(hipStream_t st, const SolveArgs& a, int* ctl, double* damp, double* A, double* y, void (*bracket)(void*, int, int), void* ctx) {
  const int npad = a.npad, nblk = npad / kSpNB;
  bracket(ctx, 0, 1);
  k_sp_solve_pre<<<dim3(1), dim3(256), 0, st>>>(a, ctl, damp);
  k_sp_load<<<dim3((npad + 255) / 256, std::min(npad, 65535)), dim3(256), 0, st>>>(a.red, a.fixed, damp, ctl, A, a.n, npad);
  bracket(ctx, 0, 0);
  for (int k = 0; k < nblk; ++k) {
    bracket(ctx, 1, 1);
    k_sp_potrf<<<dim3(1), dim3(64), 0, st>>>(A, ctl, a.n, npad, k);
    bracket(ctx, 1, 0);
    if (k + 1 < nblk) {
      const int rows = npad - kSpNB * (k + 1), T = nblk - k - 1;
      bracket(ctx, 2, 1);
      k_sp_trsm<<<dim3((rows + 63) / 64), dim3(64), 0, st>>>(A, ctl, npad, k);
      bracket(ctx, 2, 0);
      bracket(ctx, 3, 1);
      k_sp_update<<<dim3(T * (T + 1) / 2), dim3(256), 0, st>>>(A, ctl, npad, k, nblk);
      bracket(ctx, 3, 0);
    }
  }
  bracket(ctx, 4, 1);
  k_sp_finish<<<dim3(1), dim3(256), 0, st>>>(a, ctl, A, damp, y);
  bracket(ctx, 4, 0);
}

}  // namespace mcba
