// mcba_skeltraj_math.h -- the per-lane arithmetic of csrc/mcba_skeltraj.hip: skeleton trajectories, the tracks of
// mcba_traj_refine_math.h joined inside every frame by the bones of mcba_skeleton_math.h.  One problem per call, unknowns x_{t,k} of the running
// tracks:
//   minimise  the data term and the second-difference prior of section 8f-21  +  0.5 sum_t sum_{active bones (k, p)} ((|x_tk - x_tp| - L) / s)^2
// by Gauss-Newton in step form (traj_decide on the call's objective).  The system of an iteration is A d = -G, A = M + B: M the tracks'
// block-pentadiagonal matrices (the smoother's elimination, level 0 in its right-hand-side mode), B the bones' Gauss-Newton terms
// (+ u u^T / s^2 on both diagonal blocks, - u u^T / s^2 off them).  It is solved by conjugate gradients preconditioned with M:
//   linearise  traj_linearise_lane, then the bone gradient into G, the directions u and the bone residuals              skt_linearise_lane
//   z0         M z0 = -G: one elimination and back-substitution; p = z0, d = 0, q = G (q = -r, the model's gradient)    skt_start_lane
//   per CG iteration   y = A p and p^T y (skt_operator_lane); alpha = rz / p^T y; d += alpha p, q += alpha y (skt_step_lane);
//                      M z = -q from the stored factors (smooth_resolve_lane, smooth_backsub_lane); rz' = -q^T z (skt_dot_lane);
//                      beta = rz' / rz; p = z + beta p (skt_direction_lane)
//   trial      the whole objective at x + alpha d, alpha = 0, 1, 1/2, 1/4, 1/8 (traj_trial_lane plus the bone term, counted by the child) skt_trial_lane
// The scalars of the recurrence live in device memory (skt_scalars); a bone is owned by its child keypoint: planes (T, K, .) hold the record of
// bone (k, parent k) at k.  The forest here is the active one: SkPlan of the bones whose two tracks run.
// The same text is compiled with g++ into tests/hostcheck/skeltraj_hostcheck.cpp (tests/test_hostcheck_skeltraj.py).
#pragma once
#include "mcba_skeleton_math.h"
#include "mcba_traj_refine_math.h"

namespace mcba {

// the sums of the call: TR_SUMS as there (the penalty already a cost) and the bone cost at x
constexpr int SKT_BONE = TR_SUMS, SKT_SUMS = TR_SUMS + 1;
// the scalars of the recurrence (doubles) and its words (ints)
constexpr int CG_RZ = 0, CG_RZ0 = 1, CG_ALPHA = 2, CG_BETA = 3, CG_PAP = 4, CG_DOUBLES = 8;
constexpr int CG_DONE = 0, CG_ITERATIONS = 1, CG_INTS = 2;
constexpr int CG_START = 0, CG_AFTER_OPERATOR = 1, CG_AFTER_DOT = 2;   // the three places skt_scalars is called from
constexpr int SKT_HOST_READS_EVERY = 8;                                // CG iterations between two reads of the done word

// the planes of the call beyond TrData's: all (T, K, 3) but bres (T, K)
struct SktData {
  TrData rd;
  double* q;      // the gradient of the quadratic model at d: G + A d, minus the residual of the recurrence
  double* p;      // the search direction
  double* y;      // A p
  double* z;      // M^-1 (-q)
  double* dir;    // u of bone (k, parent k), from the parent's end to the child's; NaN where k has no active bone
  double* bres;   // (|x_k - x_p| - L) / s of that bone, NaN likewise
  const SkPlan* plan;   // the active forest
  const int* run;       // (K): the track runs
};

// device doubles (and ints, counted as doubles) the call needs: the detection and weight planes (3 C per frame and track), x, d, H, G (15), q, p,
// y, z, dir (15), bres (1), the per-track words, the plan, the partial sums of a flat launch, the scalars, the levels
inline size_t skeltraj_chunk_doubles(size_t T, int K, int C, int segment) {
  SmLevel lv[SM_MAX_LEVELS];
  const size_t blocks = (T * (size_t)K + 255) / 256;
  return (size_t)T * K * (3 * (size_t)C + 31) + (size_t)K * 8 + sizeof(SkPlan) / sizeof(double) + (size_t)SKT_SUMS * (blocks + 1) + CG_DOUBLES + CG_INTS +
         smooth_carve(T, segment, K, lv, 6, nullptr, nullptr);
}

// the bone between a child's point xk and its parent's xp: direction u (parent to child) and residual r.  A zero length gives 1 / 0: a
// non-finite direction and, through it, a NaN objective
MCBA_HD void skt_bone(const double* xk, const double* xp, double L, double is, double* u, double& r) {
  const double e[3] = {xk[0] - xp[0], xk[1] - xp[1], xk[2] - xp[2]};
  const double len = sqrt(sk_dot3(e, e)), il = 1.0 / len;
  u[0] = e[0] * il; u[1] = e[1] * il; u[2] = e[2] * il;
  r = (len - L) * is;
}

// ---- bone linearisation: one (frame, keypoint) after traj_linearise_lane: the gradient of its own bone and of its children's bones (index
// order) added to G, q = G, the record of its own bone.  A keypoint that does not run, or has no active bone, gets a NaN record
MCBA_HD void skt_linearise_lane(const SktData& sd, int K, int k, size_t t) {
  const size_t idx = t * K + k;
  const SkPlan& pl = *sd.plan;
  const double nan = __builtin_nan("");
  const int par = sd.run[k] ? pl.parent[k] : -1;
  if (par < 0) {
#pragma unroll
    for (int e = 0; e < 3; ++e) sd.dir[3 * idx + e] = nan;
    sd.bres[idx] = nan;
  }
  if (!sd.run[k]) return;
  const double X[3] = {sd.rd.x[3 * idx], sd.rd.x[3 * idx + 1], sd.rd.x[3 * idx + 2]};
  double G[3] = {sd.rd.G[3 * idx], sd.rd.G[3 * idx + 1], sd.rd.G[3 * idx + 2]};
  if (par >= 0) {
    const size_t ip = t * K + par;
    const double P[3] = {sd.rd.x[3 * ip], sd.rd.x[3 * ip + 1], sd.rd.x[3 * ip + 2]};
    double u[3], r;
    skt_bone(X, P, pl.length[k], pl.inv_std[k], u, r);
    const double gr = r * pl.inv_std[k];
#pragma unroll
    for (int e = 0; e < 3; ++e) { G[e] = fma(gr, u[e], G[e]); sd.dir[3 * idx + e] = u[e]; }
    sd.bres[idx] = r;
  }
  for (int ci = pl.child_start[k]; ci < pl.child_start[k + 1]; ++ci) {
    const int c = pl.child[ci];
    const size_t ic = t * K + c;
    const double Cx[3] = {sd.rd.x[3 * ic], sd.rd.x[3 * ic + 1], sd.rd.x[3 * ic + 2]};
    double u[3], r;
    skt_bone(Cx, X, pl.length[c], pl.inv_std[c], u, r);
    const double gr = r * pl.inv_std[c];
#pragma unroll
    for (int e = 0; e < 3; ++e) G[e] = fma(-gr, u[e], G[e]);
  }
#pragma unroll
  for (int e = 0; e < 3; ++e) sd.rd.G[3 * idx + e] = sd.q[3 * idx + e] = G[e];
}

// ---- operator: one (frame, keypoint) of a running track: y = A p there -- H p, a^-2 times the stencil of D2^T D2 over t (as traj_linearise_lane
// applies it to x), the bones' terms, own bone first, then the children in index order; returns p^T y of the lane
MCBA_HD double skt_operator_lane(const SktData& sd, int K, int k, size_t t) {
  const size_t idx = t * K + k;
  const long long tt = (long long)t;
  const SkPlan& pl = *sd.plan;
  const size_t T = sd.rd.T;
  const double* p = sd.p;
  const double P[3] = {p[3 * idx], p[3 * idx + 1], p[3 * idx + 2]};
  double H[6];
#pragma unroll
  for (int e = 0; e < 6; ++e) H[e] = sd.rd.H[6 * idx + e];
  const double ia2 = sd.rd.ia2[k];
  const double c0 = sm_pen_diag(tt, T), cp1 = sm_pen_off1(tt, T), cm1 = sm_pen_off1(tt - 1, T), cp2 = sm_pen_off2(tt, T), cm2 = sm_pen_off2(tt - 2, T);
  double y[3];
#pragma unroll
  for (int e = 0; e < 3; ++e) {
    double s = c0 * P[e];
    if (cp1 != 0.0) s = fma(cp1, p[3 * (idx + K) + e], s);
    if (cm1 != 0.0) s = fma(cm1, p[3 * (idx - K) + e], s);
    if (cp2 != 0.0) s = fma(cp2, p[3 * (idx + 2 * (size_t)K) + e], s);
    if (cm2 != 0.0) s = fma(cm2, p[3 * (idx - 2 * (size_t)K) + e], s);
    y[e] = fma(ia2, s, fma(sym3(H, e, 0), P[0], fma(sym3(H, e, 1), P[1], sym3(H, e, 2) * P[2])));
  }
  const int par = pl.parent[k];
  if (par >= 0) {
    const size_t ip = t * K + par;
    const double u[3] = {sd.dir[3 * idx], sd.dir[3 * idx + 1], sd.dir[3 * idx + 2]};
    const double dp[3] = {P[0] - p[3 * ip], P[1] - p[3 * ip + 1], P[2] - p[3 * ip + 2]};
    const double c = pl.inv_var[k] * sk_dot3(u, dp);
#pragma unroll
    for (int e = 0; e < 3; ++e) y[e] = fma(c, u[e], y[e]);
  }
  for (int ci = pl.child_start[k]; ci < pl.child_start[k + 1]; ++ci) {
    const int ch = pl.child[ci];
    const size_t ic = t * K + ch;
    const double u[3] = {sd.dir[3 * ic], sd.dir[3 * ic + 1], sd.dir[3 * ic + 2]};
    const double dp[3] = {P[0] - p[3 * ic], P[1] - p[3 * ic + 1], P[2] - p[3 * ic + 2]};
    const double c = pl.inv_var[ch] * sk_dot3(u, dp);
#pragma unroll
    for (int e = 0; e < 3; ++e) y[e] = fma(c, u[e], y[e]);
  }
#pragma unroll
  for (int e = 0; e < 3; ++e) sd.y[3 * idx + e] = y[e];
  return sk_dot3(P, y);
}

// ---- the vector updates of the recurrence, one (frame, keypoint) of a running track each
// after the first solve: p = z, d = 0; returns the lane's share of r^T z = -q^T z
MCBA_HD double skt_start_lane(const SktData& sd, size_t idx) {
  double s = 0.0;
#pragma unroll
  for (int e = 0; e < 3; ++e) {
    const double z = sd.z[3 * idx + e];
    sd.p[3 * idx + e] = z;
    sd.rd.d[3 * idx + e] = 0.0;
    s = fma(-sd.q[3 * idx + e], z, s);
  }
  return s;
}
MCBA_HD void skt_step_lane(const SktData& sd, size_t idx, double alpha) {
#pragma unroll
  for (int e = 0; e < 3; ++e) {
    sd.rd.d[3 * idx + e] = fma(alpha, sd.p[3 * idx + e], sd.rd.d[3 * idx + e]);
    sd.q[3 * idx + e] = fma(alpha, sd.y[3 * idx + e], sd.q[3 * idx + e]);
  }
}
MCBA_HD double skt_dot_lane(const SktData& sd, size_t idx) {
  double s = 0.0;
#pragma unroll
  for (int e = 0; e < 3; ++e) s = fma(-sd.q[3 * idx + e], sd.z[3 * idx + e], s);
  return s;
}
MCBA_HD void skt_direction_lane(const SktData& sd, size_t idx, double beta) {
#pragma unroll
  for (int e = 0; e < 3; ++e) sd.p[3 * idx + e] = fma(beta, sd.p[3 * idx + e], sd.z[3 * idx + e]);
}

// ---- the scalars of the recurrence from a finished sum (one thread): sc (CG_DOUBLES), w (CG_INTS).  The solve ends (w[CG_DONE]) when
// r^T z <= tol2 r0^T z0 (a NaN ends it too), after cg_max iterations, on a start with nothing to do and on a p^T A p that is not positive
MCBA_HD void skt_scalars(int where, double sum, double tol2, int cg_max, double* sc, int* w) {
  if (where == CG_START) {
    sc[CG_RZ] = sc[CG_RZ0] = sum;
    sc[CG_ALPHA] = sc[CG_BETA] = sc[CG_PAP] = 0.0;
    w[CG_ITERATIONS] = 0;
    w[CG_DONE] = sum > 0.0 ? 0 : 1;
  } else if (where == CG_AFTER_OPERATOR) {
    sc[CG_PAP] = sum;
    const bool ok = sum > 0.0;
    sc[CG_ALPHA] = ok ? sc[CG_RZ] / sum : 0.0;
    if (!ok) w[CG_DONE] = 1;
  } else {
    sc[CG_BETA] = sum / sc[CG_RZ];
    sc[CG_RZ] = sum;
    w[CG_ITERATIONS] += 1;
    if (!(sum > tol2 * sc[CG_RZ0]) || w[CG_ITERATIONS] >= cg_max) w[CG_DONE] = 1;
  }
}

// ---- trial: one (frame, keypoint) of a running track: traj_trial_lane's sums with the penalty as a cost, and the lane's own bone at every alpha
template <int LOSS>
MCBA_HD void skt_trial_lane(const KpCam* cams, int C, const SktData& sd, int K, int k, size_t t, double* acc) {
  double tr[TR_SUMS];
#pragma unroll
  for (int e = 0; e < TR_SUMS; ++e) tr[e] = 0.0;
  traj_trial_lane<LOSS>(cams, C, sd.rd, K, k, t, tr);
#pragma unroll
  for (int a = 0; a <= TR_TRIALS; ++a) acc[a] += tr[a];
  acc[TR_DATA] += tr[TR_DATA];
  acc[TR_PEN] += 0.5 * sd.rd.ia2[k] * tr[TR_PEN];
  acc[TR_DMAX] = fmax(acc[TR_DMAX], tr[TR_DMAX]);
  acc[TR_XMAX] = fmax(acc[TR_XMAX], tr[TR_XMAX]);
  const SkPlan& pl = *sd.plan;
  const int par = pl.parent[k];
  if (par < 0) return;
  const size_t idx = t * K + k, ip = t * K + par;
  double x[2][3], d[2][3];
#pragma unroll
  for (int e = 0; e < 3; ++e) {
    x[0][e] = sd.rd.x[3 * idx + e]; d[0][e] = sd.rd.d[3 * idx + e];
    x[1][e] = sd.rd.x[3 * ip + e]; d[1][e] = sd.rd.d[3 * ip + e];
  }
#pragma unroll
  for (int a = 0; a <= TR_TRIALS; ++a) {
    const double al = traj_alpha(a);
    const double xk[3] = {fma(al, d[0][0], x[0][0]), fma(al, d[0][1], x[0][1]), fma(al, d[0][2], x[0][2])};
    const double xp[3] = {fma(al, d[1][0], x[1][0]), fma(al, d[1][1], x[1][1]), fma(al, d[1][2], x[1][2])};
    double u[3], r;
    skt_bone(xk, xp, pl.length[k], pl.inv_std[k], u, r);
    const double c = fma(0.5 * r, r, u[0] - u[0]);   // (a bone of zero length has a finite residual and no direction: NaN, a rejected trial)
    acc[a] += c;
    if (a == 0) acc[SKT_BONE] += c;
  }
}

// the call converged: it stopped on nothing accepted or on a small step, not on the iteration limit alone
MCBA_HD bool skt_converged(const double* res, double xtol, double alpha) { return alpha == 0.0 || alpha * res[TR_DMAX] < xtol * res[TR_XMAX]; }

}  // namespace mcba
