// mcba_skeleton_math.h -- everything csrc/mcba_skeleton.hip computes: the keypoints of a frame refined together, joined
// by bones of known length.  Frames are independent; the skeleton is a forest over the K <= 64 keypoints, keypoint k with parent p(k), bone
// length L_k and bone_std s_k.  Per frame, over the positions x_k of its active keypoints:
//   minimise 0.5 sum_k sum_{c sees k} f^2 [rho(ru^2 / f^2) + rho(rv^2 / f^2)] + 0.5 sum_{active bones} ((|x_k - x_p(k)| - L_k) / s_k)^2,
//   (ru, rv) = sw (detection - project5_c(x_k)),  sw = sqrt(w) / pixel_std_c
// by Levenberg-Marquardt with Marquardt's damping, the iteration of refine_point (mcba_keypoint_math.h) with the frame's whole objective in the
// place of the point's.  The Gauss-Newton matrix of a bone with direction u = (x_k - x_p) / |x_k - x_p| is + u u^T / s^2 on both diagonal blocks
// and - u u^T / s^2 off the diagonal (the second-order term is left out: it is indefinite for a compressed bone), so the frame's matrix is block
// structured on the forest with rank-one off-diagonal blocks and a leaf-to-root elimination has no fill:
//   fold child k into its parent    A_p -= (u^T A_k^-1 u / s^4) u u^T,   b_p += (u^T A_k^-1 b_k / s^2) u          (two scalars per bone)
//   back-substitution, root to leaf d_k = A_k^-1 (b_k + u (u^T d_p) / s^2)
//   selected inversion, root to leaf Z_kk = A_k^-1 + (u^T Z_pp u / s^4) (A_k^-1 u) (A_k^-1 u)^T,  roots: Z_kk = A_k^-1
// One lane = one (frame, keypoint).  skel_frame is the whole procedure of a frame, written once as phases over the frame's lanes with a barrier
// behind each: the kernel runs it with one thread per lane (the phase's body, then the workgroup's barrier; the loop's exit is a workgroup-wide
// vote), tests/hostcheck/skeleton_hostcheck.cpp with a serial loop over the lanes per phase -- the same text, the same order of every sum.
// Lanes exchange through a few planes of doubles (LDS on the GPU): the point, the step, the bone's direction and its scalars.  No atomics:
// every word has one writer, a parent adds its children in index order, one lane sums the frame's cost in keypoint order.
#pragma once
#include "mcba_keypoint_math.h"

namespace mcba {

constexpr int SK_MAX_K = 64;
// status of a keypoint in a frame | of a frame
constexpr int SK_USABLE = 2, SK_SINGLE = 1, SK_OUT = -1, SK_NO_ANCHOR = -2;
constexpr int SK_CONVERGED = 1, SK_ITERATION_LIMIT = 0, SK_NOTHING = -1;
constexpr double SK_LAM_START = 1e-4, SK_LAM_FLOOR = 1e-12, SK_LAM_STOP = 1e12;

// ---- the forest plan: from parent (K) in the caller's numbering (-1 = root) the depth of every keypoint, the processing order (by depth, then
// by index: parents before children), and the child lists in index order
struct SkPlan {
  int K, levels;                                   // levels: the deepest depth + 1
  int parent[SK_MAX_K], level[SK_MAX_K], order[SK_MAX_K], child_start[SK_MAX_K + 1], child[SK_MAX_K];
  double length[SK_MAX_K], inv_std[SK_MAX_K], inv_var[SK_MAX_K];   // of the bone (k, parent[k]): L, 1 / s, 1 / s^2; 0 for a root
};

// 0, or: 1 K out of range, 2 a parent index out of range or a self-bone, 3 a cycle, 4 a bone length or bone_std not positive and finite
inline int skel_plan(int K, const int* parent, const double* bone_length, const double* bone_std, SkPlan& pl) {
  if (K < 1 || K > SK_MAX_K) return 1;
  pl.K = K;
  pl.levels = 1;
  for (int k = 0; k < K; ++k)
    if (parent[k] < -1 || parent[k] >= K || parent[k] == k) return 2;
  for (int k = 0; k < K; ++k) {
    int depth = 0;
    for (int j = k; parent[j] >= 0; j = parent[j])
      if (++depth >= K) return 3;   // (a walk of K steps has met a keypoint twice)
    pl.parent[k] = parent[k];
    pl.level[k] = depth;
    if (depth + 1 > pl.levels) pl.levels = depth + 1;
    const bool root = parent[k] < 0;
    const double L = root ? 0.0 : bone_length[k], s = root ? 0.0 : bone_std[k];
    if (!root && !(L > 0.0 && L <= 1.7976931348623157e308 && s > 0.0 && s <= 1.7976931348623157e308 && 1.0 / (s * s) <= 1.7976931348623157e308)) return 4;
    pl.length[k] = L;
    pl.inv_std[k] = root ? 0.0 : 1.0 / s;
    pl.inv_var[k] = root ? 0.0 : (1.0 / s) * (1.0 / s);
  }
  int n = 0;
  for (int l = 0; l < pl.levels; ++l)
    for (int k = 0; k < K; ++k)
      if (pl.level[k] == l) pl.order[n++] = k;
  n = 0;
  for (int p = 0; p < K; ++p) {
    pl.child_start[p] = n;
    for (int k = 0; k < K; ++k)
      if (parent[k] == p) pl.child[n++] = k;
  }
  pl.child_start[K] = n;
  for (int k = n; k < SK_MAX_K; ++k) pl.child[k] = 0;
  for (int k = K; k < SK_MAX_K; ++k) {
    pl.parent[k] = -1; pl.level[k] = 0; pl.order[k] = 0; pl.child_start[k + 1] = n;
    pl.length[k] = pl.inv_std[k] = pl.inv_var[k] = 0.0;
  }
  return 0;
}

// frames one workgroup of 256 threads serves
MCBA_HD int skel_frames_per_group(int K) { return 256 / K; }

// ---- the planes through which the lanes of a frame exchange: plane e of keypoint k lies at p[e * stride + k]
constexpr int SK_X = 0, SK_D = 3, SK_U = 6, SK_GR = 9, SK_Q1 = 10, SK_Q2 = 11, SK_C = 12, SK_DM = 13, SK_XM = 14, SK_PLANES = 15;
constexpr int SK_Z = 0;   // the covariance sweep: Z_kk (6) over the planes of the point and the step, which it no longer needs
struct SkShared {
  double* p;
  int* cls;   // (K): the keypoints' statuses
  int stride;
  MCBA_HD double& at(int plane, int k) const { return p[plane * stride + k]; }
};

// the words of one frame
struct SkFrameState {
  double lam, cost, cost0, data0, bone0, trial;
  int it, status, done, accept;
};

// the registers of one lane
struct SkLane {
  int k, parent, level, cls, bone, run;   // bone: its bone to the parent is active in this frame; run: the frame was running when the iteration began
  double len, is, w;                       // L, 1 / s, 1 / s^2
  double x[3], H[6], g[3], c, u[3], r;     // the point, the data term's linearisation and cost there, the bone's direction and residual (|.| - L) / s
  double xt[3], Ht[6], gt[3], ct, ut[3], rt;   // the same at the trial point
  double A[6], G[3];                       // the diagonal block (bones included, undamped) and the gradient of the whole objective
  double Lf[6], v[3], z[3], d[3];          // the block's Cholesky factor after the folds, L^-1 u, L^-1 b, the step
};

// the detections of one (frame, keypoint): element c of a plane lies `stride` = T K further
struct SkObs {
  const double* det;
  const double* sw;
  size_t stride;
  MCBA_HD void operator()(int c, double& ou, double& ov, double& s) const {
    const size_t i = (size_t)c * stride;
    ou = det[2 * i]; ov = det[2 * i + 1];
    s = sw[i];
  }
};

// what a launch reads and writes (device or host memory); outputs of the other mode are null
struct SkArgs {
  size_t T;
  const double* det;     // (C, T K, 2)
  const double* sw;      // (C, T K)
  const double* start;   // (T, K, 3)
  double fs2, inv_fs2, lam0, xtol;
  int max_iterations, system, cov;
  double* points;        // (T, K, 3)
  int* kstatus;          // (T, K)
  int* fstatus;          // (T)
  int* nit;              // (T)
  double* cost;          // (T)
  double* cost0;         // (T)
  double* bone_res;      // (T, K): of the bone (k, parent k)
  double* info6;         // (T, K, 6): system, or cov
  double* dir;           // (T, K, 3): system, or cov
  double* cov6;          // (T, K, 6): cov
  double* grad;          // (T, K, 3): system
  double* step;          // (T, K, 3): system
  double* data_cost;     // (T): system
  double* bone_cost;     // (T): system
  double* trial_cost;    // (T): system
};

MCBA_HD bool sk_finite(double v) { return v - v == 0.0; }
MCBA_HD double sk_max3(const double* a) { return fmax(fabs(a[0]), fmax(fabs(a[1]), fabs(a[2]))); }
MCBA_HD double sk_dot3(const double* a, const double* b) { return fma(a[0], b[0], fma(a[1], b[1], a[2] * b[2])); }

// the Cholesky factor of a 3 x 3 block, every pivot checked: false (and a NaN factor) for a pivot that is not positive -- a refused pivot makes
// every number behind it NaN, the trial's objective with them, and a NaN objective is a rejected step
MCBA_HD bool skel_chol3(const double* A, double* L) {
  const double nan = __builtin_nan("");
  const double d0 = A[0];
  bool ok = d0 > 0.0;
  L[0] = sqrt(d0);
  L[1] = A[1] / L[0];
  L[2] = A[2] / L[0];
  const double d1 = A[3] - L[1] * L[1];
  ok = ok && d1 > 0.0;
  L[3] = sqrt(d1);
  L[4] = (A[4] - L[2] * L[1]) / L[3];
  const double d2 = A[5] - L[2] * L[2] - L[4] * L[4];
  ok = ok && d2 > 0.0;
  L[5] = sqrt(d2);
  if (!ok)
    for (int i = 0; i < 6; ++i) L[i] = nan;
  return ok;
}

// ---- the activity sweeps of one frame, by one lane.  cls in: SK_USABLE, SK_SINGLE or SK_OUT per keypoint; out: a keypoint of a connected
// piece (of what is left when the SK_OUT keypoints and their bones are taken away) without a usable keypoint becomes SK_NO_ANCHOR.  With parents
// ordered before children the per-piece flag "holds a usable keypoint" is two sweeps of ORs over the parent array, one up and one down.
// Returns the number of keypoints fitted
MCBA_HD int skel_activity(const SkPlan& pl, int* cls) {
  unsigned long long in = 0, has = 0;
  for (int k = 0; k < pl.K; ++k) {
    if (cls[k] > 0) in |= 1ull << k;
    if (cls[k] == SK_USABLE) has |= 1ull << k;
  }
  for (int i = pl.K - 1; i >= 0; --i) {
    const int k = pl.order[i], p = pl.parent[k];
    if (p >= 0 && (in >> k & 1) && (in >> p & 1) && (has >> k & 1)) has |= 1ull << p;
  }
  for (int i = 0; i < pl.K; ++i) {
    const int k = pl.order[i], p = pl.parent[k];
    if (p >= 0 && (in >> k & 1) && (in >> p & 1) && (has >> p & 1)) has |= 1ull << k;
  }
  int n = 0;
  for (int k = 0; k < pl.K; ++k)
    if (in >> k & 1) {
      if (has >> k & 1) ++n;
      else cls[k] = SK_NO_ANCHOR;
    }
  return n;
}

// ---- the bone of a lane at the points the frame has published in plane `px`: its direction u and residual r = (|x_k - x_p| - L) / s
MCBA_HD void skel_bone(const SkLane& ln, const SkShared& sh, int px, const double* x, double* u, double& r) {
  const double e[3] = {x[0] - sh.at(px, ln.parent), x[1] - sh.at(px + 1, ln.parent), x[2] - sh.at(px + 2, ln.parent)};
  const double len = sqrt(sk_dot3(e, e)), il = 1.0 / len;
  u[0] = e[0] * il; u[1] = e[1] * il; u[2] = e[2] * il;
  r = (len - ln.len) * ln.is;
}

// ---- the accept and stop rule of a frame after a trial (refine_point's): the trial is accepted when the frame's objective is not larger (NaN
// compares false); the damping falls tenfold on acceptance (floor 1e-12) and rises tenfold on rejection.  The frame stops, converged, when the
// step max |d| < xtol max |x| -- accepted or not: then no point nearby is better -- or when the damping has reached 1e12; otherwise at max_iterations
MCBA_HD void skel_decide(SkFrameState& fs, double trial, double dmax, double xmax, double xtol, int max_iterations) {
  ++fs.it;
  fs.trial = trial;
  const bool small_step = dmax < xtol * xmax;
  fs.accept = trial <= fs.cost ? 1 : 0;
  if (fs.accept) {
    fs.cost = trial;
    fs.lam = fmax(0.1 * fs.lam, SK_LAM_FLOOR);
    if (small_step) { fs.done = 1; fs.status = SK_CONVERGED; }
  } else {
    fs.lam *= 10.0;
    if (small_step || !(fs.lam < SK_LAM_STOP)) { fs.done = 1; fs.status = SK_CONVERGED; }
  }
  if (!fs.done && fs.it >= max_iterations) fs.done = 1;   // (status: SK_ITERATION_LIMIT from the start)
}

// ---- phases shared by the loop and the covariance sweep
// publish the bone's direction and gradient scalar r / s
MCBA_HD void skel_publish_bone(const SkLane& ln, const SkShared& sh) {
  sh.at(SK_U, ln.k) = ln.u[0]; sh.at(SK_U + 1, ln.k) = ln.u[1]; sh.at(SK_U + 2, ln.k) = ln.u[2];
  sh.at(SK_GR, ln.k) = ln.r * ln.is;
}

// the diagonal block and the gradient of the whole objective: the data term's, the lane's own bone, its children's bones in index order
MCBA_HD void skel_assemble(SkLane& ln, const SkShared& sh, const SkPlan& pl) {
#pragma unroll
  for (int e = 0; e < 6; ++e) ln.A[e] = ln.H[e];
#pragma unroll
  for (int e = 0; e < 3; ++e) ln.G[e] = ln.g[e];
  if (ln.bone) {
    const double gr = ln.r * ln.is;
    int q = 0;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      const double a = ln.w * ln.u[i];
#pragma unroll
      for (int j = i; j < 3; ++j, ++q) ln.A[q] = fma(a, ln.u[j], ln.A[q]);
      ln.G[i] = fma(gr, ln.u[i], ln.G[i]);
    }
  }
  for (int ci = pl.child_start[ln.k]; ci < pl.child_start[ln.k + 1]; ++ci) {
    const int c = pl.child[ci];
    if (sh.cls[c] <= 0) continue;
    const double uc[3] = {sh.at(SK_U, c), sh.at(SK_U + 1, c), sh.at(SK_U + 2, c)}, wc = pl.inv_var[c], gr = sh.at(SK_GR, c);
    int q = 0;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      const double a = wc * uc[i];
#pragma unroll
      for (int j = i; j < 3; ++j, ++q) ln.A[q] = fma(a, uc[j], ln.A[q]);
      ln.G[i] = fma(-gr, uc[i], ln.G[i]);
    }
  }
}

// the upward sweep of one level: the damped block less its children's folds, its factor, L^-1 u and L^-1 b, the two scalars of its own fold
MCBA_HD void skel_eliminate(SkLane& ln, const SkShared& sh, const SkPlan& pl, double lam) {
  double A[6] = {fma(lam, ln.A[0], ln.A[0]), ln.A[1], ln.A[2], fma(lam, ln.A[3], ln.A[3]), ln.A[4], fma(lam, ln.A[5], ln.A[5])};
  double b[3] = {-ln.G[0], -ln.G[1], -ln.G[2]};
  for (int ci = pl.child_start[ln.k]; ci < pl.child_start[ln.k + 1]; ++ci) {
    const int c = pl.child[ci];
    if (sh.cls[c] <= 0) continue;
    const double uc[3] = {sh.at(SK_U, c), sh.at(SK_U + 1, c), sh.at(SK_U + 2, c)}, q1 = sh.at(SK_Q1, c), q2 = sh.at(SK_Q2, c);
    int q = 0;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      const double a = q1 * uc[i];
#pragma unroll
      for (int j = i; j < 3; ++j, ++q) A[q] = fma(-a, uc[j], A[q]);
      b[i] = fma(q2, uc[i], b[i]);
    }
  }
  skel_chol3(A, ln.Lf);
  fwd3(ln.Lf, b, ln.z);
  if (ln.bone) {
    fwd3(ln.Lf, ln.u, ln.v);
    sh.at(SK_Q1, ln.k) = ln.w * ln.w * sk_dot3(ln.v, ln.v);
    sh.at(SK_Q2, ln.k) = ln.w * sk_dot3(ln.v, ln.z);
  }
}

// the downward sweep of one level: d_k = A_k^-1 (b_k + u (u^T d_p) / s^2)
MCBA_HD void skel_substitute(SkLane& ln, const SkShared& sh) {
  double rhs[3] = {ln.z[0], ln.z[1], ln.z[2]};
  if (ln.bone) {
    const double dp[3] = {sh.at(SK_D, ln.parent), sh.at(SK_D + 1, ln.parent), sh.at(SK_D + 2, ln.parent)};
    const double s = ln.w * sk_dot3(ln.u, dp);
#pragma unroll
    for (int e = 0; e < 3; ++e) rhs[e] = fma(s, ln.v[e], rhs[e]);
  }
  bwd3(ln.Lf, rhs, ln.d);
  sh.at(SK_D, ln.k) = ln.d[0]; sh.at(SK_D + 1, ln.k) = ln.d[1]; sh.at(SK_D + 2, ln.k) = ln.d[2];
}

// the selected inversion of one level: Z_kk, published for the children
MCBA_HD void skel_selinv(SkLane& ln, const SkShared& sh, double* Z) {
  double col[3][3];
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    const double e[3] = {i == 0 ? 1.0 : 0.0, i == 1 ? 1.0 : 0.0, i == 2 ? 1.0 : 0.0};
    double y[3];
    fwd3(ln.Lf, e, y);
    bwd3(ln.Lf, y, col[i]);
  }
  Z[0] = col[0][0]; Z[1] = 0.5 * (col[0][1] + col[1][0]); Z[2] = 0.5 * (col[0][2] + col[2][0]);
  Z[3] = col[1][1]; Z[4] = 0.5 * (col[1][2] + col[2][1]); Z[5] = col[2][2];
  if (ln.bone) {
    double Zp[6], ai[3];
#pragma unroll
    for (int e = 0; e < 6; ++e) Zp[e] = sh.at(SK_Z + e, ln.parent);
    bwd3(ln.Lf, ln.v, ai);   // A_k^-1 u
    const double Zu[3] = {fma(Zp[0], ln.u[0], fma(Zp[1], ln.u[1], Zp[2] * ln.u[2])), fma(Zp[1], ln.u[0], fma(Zp[3], ln.u[1], Zp[4] * ln.u[2])),
                          fma(Zp[2], ln.u[0], fma(Zp[4], ln.u[1], Zp[5] * ln.u[2]))};
    const double s = ln.w * ln.w * sk_dot3(ln.u, Zu);
    int q = 0;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      const double a = s * ai[i];
#pragma unroll
      for (int j = i; j < 3; ++j, ++q) Z[q] = fma(a, ai[j], Z[q]);
    }
  }
#pragma unroll
  for (int e = 0; e < 6; ++e) sh.at(SK_Z + e, ln.k) = Z[e];
}

// ---- the procedure of a frame.  cx.each(f) runs f(lane, shared planes, frame words, frame) for every lane of every frame the context holds and
// puts a barrier behind the phase; cx.any(pred) is pred(frame words) OR-ed over those frames, a barrier as well.  Control flow around the
// phases depends on the plan, the arguments and cx.any alone: it is uniform over a workgroup
template <int LOSS, class Ctx>
MCBA_HD void skel_frame(Ctx& cx, const SkPlan& pl, const KpCam* cams, int C, const SkArgs& a) {
  const int K = pl.K;
  const double nan = __builtin_nan("");
  auto obs_of = [&](const SkLane& ln, size_t t) {
    const size_t idx = t * K + ln.k;
    return SkObs{a.det + 2 * idx, a.sw + idx, a.T * (size_t)K};
  };
  // the start, the views
  cx.each([&](SkLane& ln, const SkShared& sh, SkFrameState&, size_t t) {
    const int k = ln.k;
    ln.parent = pl.parent[k]; ln.level = pl.level[k];
    ln.len = pl.length[k]; ln.is = pl.inv_std[k]; ln.w = pl.inv_var[k];
    const size_t idx = t * K + k;
#pragma unroll
    for (int e = 0; e < 3; ++e) ln.x[e] = a.start[3 * idx + e];
    SkObs obs = obs_of(ln, t);
    int views = 0;
    for (int c = 0; c < C; ++c) {
      double ou, ov, sw;
      if (kp_observe(obs, c, ou, ov, sw, 0)) ++views;
    }
    const bool fin = sk_finite(ln.x[0]) && sk_finite(ln.x[1]) && sk_finite(ln.x[2]);
    sh.cls[k] = !fin || views == 0 ? SK_OUT : views >= 2 ? SK_USABLE : SK_SINGLE;
  });
  cx.each([&](SkLane& ln, const SkShared& sh, SkFrameState& fs, size_t) {
    if (ln.k != 0) return;
    const int n = skel_activity(pl, sh.cls);
    fs.lam = a.lam0; fs.cost = fs.cost0 = fs.data0 = fs.bone0 = fs.trial = nan;
    fs.it = 0; fs.accept = 0;
    fs.done = n == 0;
    fs.status = n == 0 ? SK_NOTHING : SK_ITERATION_LIMIT;
  });
  // the linearisation at the start
  cx.each([&](SkLane& ln, const SkShared& sh, SkFrameState&, size_t t) {
    ln.cls = sh.cls[ln.k];
    ln.bone = ln.cls > 0 && ln.parent >= 0 && sh.cls[ln.parent] > 0;
    ln.u[0] = ln.u[1] = ln.u[2] = ln.r = 0.0;
    ln.c = 0.0;
    if (ln.cls <= 0) return;
    SkObs obs = obs_of(ln, t);
    keypoint_linearise<LOSS>(cams, C, obs, ln.x, a.fs2, a.inv_fs2, ln.H, ln.g, ln.c);
    sh.at(SK_X, ln.k) = ln.x[0]; sh.at(SK_X + 1, ln.k) = ln.x[1]; sh.at(SK_X + 2, ln.k) = ln.x[2];
  });
  cx.each([&](SkLane& ln, const SkShared& sh, SkFrameState&, size_t) {
    if (ln.cls <= 0) return;
    double cb = 0.0;
    if (ln.bone) {
      skel_bone(ln, sh, SK_X, ln.x, ln.u, ln.r);
      cb = 0.5 * ln.r * ln.r;
    }
    sh.at(SK_DM, ln.k) = ln.c;
    sh.at(SK_XM, ln.k) = cb;
    ln.c += cb;
    sh.at(SK_C, ln.k) = ln.c;
  });
  cx.each([&](SkLane& ln, const SkShared& sh, SkFrameState& fs, size_t) {
    if (ln.k != 0 || fs.done) return;
    double cost = 0.0, data = 0.0, bone = 0.0;
    for (int k = 0; k < K; ++k)
      if (sh.cls[k] > 0) { cost += sh.at(SK_C, k); data += sh.at(SK_DM, k); bone += sh.at(SK_XM, k); }
    fs.cost = fs.cost0 = cost; fs.data0 = data; fs.bone0 = bone;
  });

  // the loop
  while (cx.any([](const SkFrameState& fs) { return !fs.done; })) {
    cx.each([&](SkLane& ln, const SkShared& sh, SkFrameState& fs, size_t) {
      ln.run = !fs.done && ln.cls > 0;
      if (ln.run) skel_publish_bone(ln, sh);
    });
    cx.each([&](SkLane& ln, const SkShared& sh, SkFrameState&, size_t) {
      if (ln.run) skel_assemble(ln, sh, pl);
    });
    for (int lev = pl.levels - 1; lev >= 0; --lev)
      cx.each([&](SkLane& ln, const SkShared& sh, SkFrameState& fs, size_t) {
        if (ln.run && ln.level == lev) skel_eliminate(ln, sh, pl, fs.lam);
      });
    for (int lev = 0; lev < pl.levels; ++lev)
      cx.each([&](SkLane& ln, const SkShared& sh, SkFrameState&, size_t) {
        if (ln.run && ln.level == lev) skel_substitute(ln, sh);
      });
    // the trial point
    cx.each([&](SkLane& ln, const SkShared& sh, SkFrameState&, size_t) {
      if (!ln.run) return;
#pragma unroll
      for (int e = 0; e < 3; ++e) { ln.xt[e] = ln.x[e] + ln.d[e]; sh.at(SK_X + e, ln.k) = ln.xt[e]; }
    });
    cx.each([&](SkLane& ln, const SkShared& sh, SkFrameState&, size_t t) {
      if (!ln.run) return;
      SkObs obs = obs_of(ln, t);
      keypoint_linearise<LOSS>(cams, C, obs, ln.xt, a.fs2, a.inv_fs2, ln.Ht, ln.gt, ln.ct);
      ln.ut[0] = ln.ut[1] = ln.ut[2] = ln.rt = 0.0;
      if (ln.bone) {
        skel_bone(ln, sh, SK_X, ln.xt, ln.ut, ln.rt);
        ln.ct += 0.5 * ln.rt * ln.rt;
      }
      sh.at(SK_C, ln.k) = ln.ct;
      sh.at(SK_DM, ln.k) = sk_max3(ln.d);
      sh.at(SK_XM, ln.k) = sk_max3(ln.x);
    });
    cx.each([&](SkLane& ln, const SkShared& sh, SkFrameState& fs, size_t) {
      if (ln.k != 0 || fs.done) return;
      double trial = 0.0, dmax = 0.0, xmax = 0.0;
      for (int k = 0; k < K; ++k)
        if (sh.cls[k] > 0) { trial += sh.at(SK_C, k); dmax = fmax(dmax, sh.at(SK_DM, k)); xmax = fmax(xmax, sh.at(SK_XM, k)); }
      skel_decide(fs, trial, dmax, xmax, a.xtol, a.max_iterations);
    });
    if (a.system) break;
    cx.each([&](SkLane& ln, const SkShared&, SkFrameState& fs, size_t) {
      if (!ln.run || !fs.accept) return;
#pragma unroll
      for (int e = 0; e < 6; ++e) ln.H[e] = ln.Ht[e];
#pragma unroll
      for (int e = 0; e < 3; ++e) { ln.x[e] = ln.xt[e]; ln.g[e] = ln.gt[e]; ln.u[e] = ln.ut[e]; }
      ln.c = ln.ct; ln.r = ln.rt;
    });
  }

  if (a.system) {
    // one evaluation laid open, before anything is accepted
    cx.each([&](SkLane& ln, const SkShared&, SkFrameState& fs, size_t t) {
      const size_t idx = t * K + ln.k;
      const bool on = ln.cls > 0;
      a.kstatus[idx] = ln.cls;
#pragma unroll
      for (int e = 0; e < 6; ++e) a.info6[6 * idx + e] = on ? ln.A[e] : nan;
#pragma unroll
      for (int e = 0; e < 3; ++e) {
        a.grad[3 * idx + e] = on ? ln.G[e] : nan;
        a.step[3 * idx + e] = on ? ln.d[e] : nan;
        a.dir[3 * idx + e] = ln.bone ? ln.u[e] : nan;
      }
      if (ln.k == 0) {
        a.fstatus[t] = fs.status == SK_NOTHING ? SK_NOTHING : SK_CONVERGED;
        a.data_cost[t] = fs.data0; a.bone_cost[t] = fs.bone0; a.trial_cost[t] = fs.trial;
      }
    });
    return;
  }

  // the result
  cx.each([&](SkLane& ln, const SkShared&, SkFrameState& fs, size_t t) {
    const size_t idx = t * K + ln.k;
    const bool on = ln.cls > 0;
    a.kstatus[idx] = ln.cls;
#pragma unroll
    for (int e = 0; e < 3; ++e) a.points[3 * idx + e] = on ? ln.x[e] : nan;
    a.bone_res[idx] = ln.bone ? ln.r : nan;
    if (ln.k == 0) { a.fstatus[t] = fs.status; a.nit[t] = fs.it; a.cost[t] = fs.cost; a.cost0[t] = fs.cost0; }
  });
  if (!a.cov) return;
  // the marginal covariance at the result: one more elimination without damping, then the selected inversion root to leaf
  cx.each([&](SkLane& ln, const SkShared& sh, SkFrameState&, size_t) {
    ln.run = ln.cls > 0;
    if (ln.run) skel_publish_bone(ln, sh);
  });
  cx.each([&](SkLane& ln, const SkShared& sh, SkFrameState&, size_t t) {
    const size_t idx = t * K + ln.k;
    if (ln.run) skel_assemble(ln, sh, pl);
#pragma unroll
    for (int e = 0; e < 6; ++e) a.info6[6 * idx + e] = ln.run ? ln.A[e] : nan;
#pragma unroll
    for (int e = 0; e < 3; ++e) a.dir[3 * idx + e] = ln.bone ? ln.u[e] : nan;
  });
  for (int lev = pl.levels - 1; lev >= 0; --lev)
    cx.each([&](SkLane& ln, const SkShared& sh, SkFrameState&, size_t) {
      if (ln.run && ln.level == lev) skel_eliminate(ln, sh, pl, 0.0);
    });
  for (int lev = 0; lev < pl.levels; ++lev)
    cx.each([&](SkLane& ln, const SkShared& sh, SkFrameState&, size_t t) {
      if (ln.level != lev) return;
      const size_t idx = t * K + ln.k;
      double Z[6] = {nan, nan, nan, nan, nan, nan};
      if (ln.run) skel_selinv(ln, sh, Z);
#pragma unroll
      for (int e = 0; e < 6; ++e) a.cov6[6 * idx + e] = Z[e];
    });
}

// ---- estimate_bone_lengths: the distance of one (bone, frame), NaN where an end has a NaN.  Plain products and sums in the written order, no
// fused multiply-add: the float64 value numpy's sqrt(dx * dx + dy * dy + dz * dz) has
MCBA_HD double skel_distance(const double* a, const double* b) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const double dx = a[0] - b[0], dy = a[1] - b[1], dz = a[2] - b[2];
  const double xx = dx * dx, yy = dy * dy, zz = dz * dz;
  const double s = xx + yy;
  return sqrt(s + zz);
}

}  // namespace mcba
