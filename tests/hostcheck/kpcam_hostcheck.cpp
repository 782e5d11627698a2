// Host build of csrc/mcba_kpcam_math.h -- the arithmetic of csrc/mcba_kpcam.hip (k_kpcam_reduce, k_kpcam_step) and the Levenberg-Marquardt loop of
// csrc/mcba_kpcam_api.hip -- for g++: the kernels' sums as plain loops (points ascending; per point the cameras ascending, per camera the two
// halves of an item), the product Y Y^T as plain loops, the loop itself the very text the C ABI runs (kpcam_lm, prior included).
// tests/test_hostcheck_kpcam.py compiles this as a shared library (plain -O2) and holds it to the GPU tier's bounds; with -DKPCAM_MAIN it is a
// stand-alone program (two small cases) that the same test builds with -fsanitize=address,undefined and runs as a child process.
#include <cmath>
#include <cstddef>
#include <cstdio>
#include <vector>
#include "../../multicam-calibration_amd/csrc/mcba_kpcam_math.h"

using namespace mcba;

template <int LOSS>
struct HostBackEnd12 {
  int C;
  size_t P;
  const double* uvs;     // (C, P, 2)
  const double* dist5;   // p1, p2, k3 (k1, k2 come with the 12 scalars)
  const int* held;
  double f_scale;
  std::vector<double> X[2];
  std::vector<int> status;
  std::vector<TcCam> tab, tab_trial;
  int cur = 0;

  void statuses(const double* theta) {
    tab.resize((size_t)C);
    kpcam_table(C, theta, dist5, tab.data());
    status.resize(P);
    for (size_t p = 0; p < P; ++p) {
      auto obs = [&](int c, double& ou, double& ov) { ou = uvs[2 * ((size_t)c * P + p)]; ov = uvs[2 * ((size_t)c * P + p) + 1]; };
      KbPoint pt;
      kpba_point<LOSS_LINEAR>(tab.data(), C, obs, X[cur].data() + 3 * p, 1.0, 1.0, nullptr, pt);
      status[p] = kpba_status(pt.views, X[cur].data() + 3 * p, pt.H);
    }
  }
  int reduce(const double* theta, double lam, KcSystem& sys) {
    tab.resize((size_t)C);
    kpcam_table(C, theta, dist5, tab.data());
    sys.shape(C);
    sys.cost = sys.count = sys.gmax = 0.0;
    const double fs2 = f_scale * f_scale, inv_fs2 = 1.0 / fs2;
    const int n12 = kKcRows * C;
    std::vector<double> Y((size_t)n12 * 3);
    for (size_t p = 0; p < P; ++p) {
      if (status[p] != KB_USED) continue;
      const double* Xp = X[cur].data() + 3 * p;
      auto obs = [&](int c, double& ou, double& ov) { ou = uvs[2 * ((size_t)c * P + p)]; ov = uvs[2 * ((size_t)c * P + p) + 1]; };
      KbPoint pt;
      kpba_point<LOSS>(tab.data(), C, obs, Xp, fs2, inv_fs2, nullptr, pt);
      sys.cost += pt.cost;
      sys.count += 2.0 * pt.views;
      sys.gmax = fmax(sys.gmax, fmax(fabs(pt.g[0]), fmax(fabs(pt.g[1]), fabs(pt.g[2]))));
      KbFactor f;
      if (!kpba_factor(pt.H, lam, f)) continue;
      double zp[3];
      kpba_fwd(f, pt.g, zp);
      for (double& v : Y) v = 0.0;
      for (int c = 0; c < C; ++c) {
        double ou, ov;
        obs(c, ou, ov);
        if (!(ou == ou && ov == ov)) continue;
        double a0[kpcam_half_size(0)], a1[kpcam_half_size(1)];
        kpcam_item_w<LOSS, false, 0>(tab[c], Xp, ou, ov, 1.0, fs2, inv_fs2, f, zp, held[c], Y.data() + 36 * c, a0);
        kpcam_item_w<LOSS, false, 1>(tab[c], Xp, ou, ov, 1.0, fs2, inv_fs2, f, zp, held[c], Y.data() + 36 * c + 18, a1);
        for (int k = 0; k < kpcam_half_size(0); ++k) sys.acc[(size_t)c * kKcAcc + kpcam_half_slot(0, k)] += a0[k];
        for (int k = 0; k < kpcam_half_size(1); ++k) sys.acc[(size_t)c * kKcAcc + kpcam_half_slot(1, k)] += a1[k];
      }
      for (int i = 0; i < n12; ++i)
        for (int j = 0; j < n12; ++j) sys.YY[(size_t)i * sys.NP + j] += Y[3 * i] * Y[3 * j] + Y[3 * i + 1] * Y[3 * j + 1] + Y[3 * i + 2] * Y[3 * j + 2];
    }
    return 0;
  }
  int step(const double* theta_trial, const double* dtheta, double lam, double out[3]) {
    tab_trial.resize((size_t)C);
    kpcam_table(C, theta_trial, dist5, tab_trial.data());
    const double fs2 = f_scale * f_scale, inv_fs2 = 1.0 / fs2;
    out[0] = out[1] = out[2] = 0.0;
    X[1 - cur] = X[cur];
    for (size_t p = 0; p < P; ++p) {
      if (status[p] != KB_USED) continue;
      const double* Xp = X[cur].data() + 3 * p;
      auto obs = [&](int c, double& ou, double& ov) { ou = uvs[2 * ((size_t)c * P + p)]; ov = uvs[2 * ((size_t)c * P + p) + 1]; };
      KbPoint pt, tr;
      kpcam_point<LOSS>(tab.data(), C, obs, Xp, fs2, inv_fs2, dtheta, pt);
      KbFactor f;
      double dX[3] = {0.0, 0.0, 0.0};
      if (kpba_factor(pt.H, lam, f)) kpba_point_step(f, pt.g, pt.q, dX);
      double* Xt = X[1 - cur].data() + 3 * p;
      for (int j = 0; j < 3; ++j) { Xt[j] = Xp[j] + dX[j]; out[1] += dX[j] * dX[j]; out[2] += Xp[j] * Xp[j]; }
      kpcam_point<LOSS>(tab_trial.data(), C, obs, Xt, fs2, inv_fs2, nullptr, tr);
      out[0] += tr.cost;
    }
    return 0;
  }
  void accept() { cur = 1 - cur; }
};

template <int LOSS>
static int run(int C, size_t P, const double* uvs, const double* cam12, const double* dist5, const double* pts0, int* held, const double* pw, int gauge, int scale_cam, double f_scale,
               const KbOptions& opt, double* cams, double* pts, int* status, double* res9, double* hist, int hist_cap) {
  HostBackEnd12<LOSS> be{C, P, uvs, dist5, held, f_scale};
  be.X[0].assign(pts0, pts0 + 3 * P);
  for (int k = 0; k < 12 * C; ++k) cams[k] = cam12[k];
  be.statuses(cams);
  for (int c = 0; c < C; ++c) {   // a camera that no used point sees is held whole
    bool seen = false;
    for (size_t p = 0; p < P && !seen; ++p) seen = be.status[p] == KB_USED && uvs[2 * ((size_t)c * P + p)] == uvs[2 * ((size_t)c * P + p)] && uvs[2 * ((size_t)c * P + p) + 1] == uvs[2 * ((size_t)c * P + p) + 1];
    if (!seen) held[c] = kKcHeldAll;
  }
  if ((held[scale_cam] & 0xFC0) == 0xFC0) return 2;   // no used point in the scale camera: nothing fixes the scale
  held[gauge] |= 0xFC0;
  const double baseline = kpcam_baseline(C, cams, gauge, scale_cam);
  KcResult r;
  if (int rc = kpcam_lm(be, C, held, cams, pw, opt, r, hist, hist_cap)) return rc;
  for (size_t p = 0; p < P; ++p) {
    status[p] = be.status[p];
    for (int j = 0; j < 3; ++j) pts[3 * p + j] = status[p] == KB_USED ? be.X[be.cur][3 * p + j] : std::nan("");
  }
  const double s = kpcam_rescale(C, held, cams, P, pts, gauge, scale_cam, baseline);
  res9[0] = r.cost; res9[1] = r.cost0; res9[2] = r.optimality; res9[3] = r.nfev; res9[4] = r.njev; res9[5] = r.status; res9[6] = s; res9[7] = r.nhist; res9[8] = r.prior_cost;
  return 0;
}

template <int LOSS>
static void system_at(int C, size_t P, const double* uvs, const double* cam12, const double* dist5, const double* pts, const int* held, double f_scale, double lam, double* YY, double* acc,
                      double* scal3, int* status) {
  HostBackEnd12<LOSS> be{C, P, uvs, dist5, held, f_scale};
  be.X[0].assign(pts, pts + 3 * P);
  be.statuses(cam12);
  KcSystem sys;
  be.reduce(cam12, lam, sys);
  for (size_t i = 0; i < sys.YY.size(); ++i) YY[i] = sys.YY[i];
  for (size_t i = 0; i < sys.acc.size(); ++i) acc[i] = sys.acc[i];
  scal3[0] = sys.cost; scal3[1] = sys.count; scal3[2] = sys.gmax;
  for (size_t p = 0; p < P; ++p) status[p] = be.status[p];
}

template <int LOSS>
static void step_at(int C, size_t P, const double* uvs, const double* cam12, const double* dist5, const double* pts, double f_scale, double lam, const double* cam_trial, const double* dtheta,
                    double* trial, double* out3) {
  HostBackEnd12<LOSS> be{C, P, uvs, dist5, nullptr, f_scale};
  be.X[0].assign(pts, pts + 3 * P);
  be.statuses(cam12);
  be.step(cam_trial, dtheta, lam, out3);
  for (size_t i = 0; i < 3 * P; ++i) trial[i] = be.X[1][i];
}

#define KPCAM_LOSSES(CALL)                          \
  switch (loss) {                                    \
    case LOSS_LINEAR: CALL(LOSS_LINEAR);             \
    case LOSS_SOFT_L1: CALL(LOSS_SOFT_L1);           \
    case LOSS_HUBER: CALL(LOSS_HUBER);               \
    case LOSS_CAUCHY: CALL(LOSS_CAUCHY);             \
    case LOSS_ARCTAN: CALL(LOSS_ARCTAN);             \
    default: return 1;                               \
  }

extern "C" {

// uvs (C, P, 2), cam12 (C, 12) the start (k1, k2 in columns 4, 5; dist5 supplies p1, p2, k3), pts0 (P, 3); held (C) in/out, 12 bits; pw (C, 6) = 1 / std^2 or NULL.
// Out: cams (C, 12), pts (P, 3), status (P), res9 = cost cost0 optimality nfev njev status scale evaluations prior_cost, hist (hist_cap, 3).
int hc_kpcam(int C, size_t P, const double* uvs, const double* cam12, const double* dist5, const double* pts0, int* held, const double* pw, int gauge, int scale_cam, int loss, double f_scale,
             double ftol, double xtol, double gtol, int max_nfev, double* cams, double* pts, int* status, double* res9, double* hist, int hist_cap) {
  const KbOptions opt{ftol, xtol, gtol, max_nfev};
#define CALL(L) return run<L>(C, P, uvs, cam12, dist5, pts0, held, pw, gauge, scale_cam, f_scale, opt, cams, pts, status, res9, hist, hist_cap)
  KPCAM_LOSSES(CALL)
#undef CALL
}

// the system at (cam12, pts) and damping lam: YY (NP, NP), acc (C, 102), scal3 = cost, present scalars, max |g_p|, status (P).  1: unknown loss
int hc_kpcam_system(int C, size_t P, const double* uvs, const double* cam12, const double* dist5, const double* pts, const int* held, int loss, double f_scale, double lam, double* YY, double* acc,
                    double* scal3, int* status) {
#define CALL(L) system_at<L>(C, P, uvs, cam12, dist5, pts, held, f_scale, lam, YY, acc, scal3, status); return 0
  KPCAM_LOSSES(CALL)
#undef CALL
}

// HostBackEnd12::step once at (cam12, pts): trial (P, 3), out3 = trial cost under cam_trial, sum dX^2, sum X^2
int hc_kpcam_step(int C, size_t P, const double* uvs, const double* cam12, const double* dist5, const double* pts, int loss, double f_scale, double lam, const double* cam_trial, const double* dtheta,
                  double* trial, double* out3) {
#define CALL(L) step_at<L>(C, P, uvs, cam12, dist5, pts, f_scale, lam, cam_trial, dtheta, trial, out3); return 0
  KPCAM_LOSSES(CALL)
#undef CALL
}

// the prior's cost at theta (C, 12) about theta0 (C, 12)
double hc_kpcam_prior_cost(int C, const int* held, const double* pw, const double* theta, const double* theta0) { return kpcam_prior_cost(C, held, pw, theta, theta0); }

// what kpcam_lm adds to the gradient of scalar k (of the 12 C)
double hc_kpcam_prior_gradient(const double* pw, int k, const double* theta, const double* theta0) { return kpcam_prior_gradient(pw, k, theta, theta0); }

}  // extern "C"

#ifdef KPCAM_MAIN
static int run_case(int C, int P, int loss, bool with_unseen, bool with_prior) {
  std::vector<double> cam12(12 * C), dist5(5 * C), pts(3 * P), uvs((size_t)2 * C * P);
  for (int c = 0; c < C; ++c) {
    const double q[12] = {900.0 + 10 * c, 905.0, 640.0, 512.0, -0.1, 0.02, 0.02 * c, 0.05 * c, -0.01 * c, -150.0 * c, 10.0 * c, 5.0 * c};
    for (int k = 0; k < 12; ++k) cam12[12 * c + k] = q[k];
    const double d[5] = {-0.1, 0.02, 1e-3, -5e-4, 0.01};
    for (int k = 0; k < 5; ++k) dist5[5 * c + k] = d[k];
  }
  std::vector<TcCam> tab(C);
  kpcam_table(C, cam12.data(), dist5.data(), tab.data());
  for (int p = 0; p < P; ++p) {
    pts[3 * p] = 37.0 * (p % 5) - 80.0 + 3.0 * p; pts[3 * p + 1] = 60.0 - 29.0 * (p % 4); pts[3 * p + 2] = 900.0 + 45.0 * (p % 3) - 11.0 * p;
    for (int c = 0; c < C; ++c) {
      double u, v;
      project5<false>(tab[c].kc, pts.data() + 3 * p, u, v);
      double* o = uvs.data() + 2 * ((size_t)c * P + p);
      o[0] = u + 0.3 * ((p + c) % 3 - 1); o[1] = v - 0.2 * ((p + 2 * c) % 3 - 1);
      if (with_unseen && ((p == P - 1 && c >= 1) || c == C - 1)) o[0] = o[1] = std::nan("");   // the last point: one view; the last camera sees nothing
    }
  }
  for (int c = 1; c < C; ++c) { cam12[12 * c + 6] += 2e-3; cam12[12 * c + 10] += 1.0; cam12[12 * c] *= 1.005; }   // the start: off the optimum
  std::vector<int> held(C, 0x03C), status(P);   // focal free; principal point and distortion held
  held[1] |= 1 << 9;
  std::vector<double> pw(6 * C, 0.0);
  for (int c = 0; c < C; ++c) pw[6 * c] = pw[6 * c + 1] = 1.0 / (4.5 * 4.5);
  std::vector<double> cams(12 * C), out(3 * P), res(9), hist(3 * 40);
  if (hc_kpcam(C, P, uvs.data(), cam12.data(), dist5.data(), pts.data(), held.data(), with_prior ? pw.data() : nullptr, 0, 1, loss, 1.5, 1e-12, 1e-12, 1e-10, 40, cams.data(), out.data(), status.data(),
               res.data(), hist.data(), 40) != 0)
    return 1;
  int bad = 0;
  if (!(res[0] <= res[1])) { printf("the cost rose: %g -> %g\n", res[1], res[0]); ++bad; }
  if (with_unseen && (status[P - 1] != KB_TOO_FEW_VIEWS || held[C - 1] != kKcHeldAll)) { printf("status %d held %d\n", status[P - 1], held[C - 1]); ++bad; }
  if ((held[0] & 0xFC0) != 0xFC0) ++bad;
  for (int p = 0; p < P; ++p)
    if (std::isfinite(out[3 * p]) != (status[p] == KB_USED)) ++bad;
  printf("C %d P %d loss %d prior %d: cost %.6g -> %.6g (prior %.3g), %g evaluations, status %g, scale %.12g, fx %.6f -> %.6f\n", C, P, loss, (int)with_prior, res[1], res[0], res[8], res[3], res[5], res[6],
         cam12[12], cams[12]);
  return bad;
}

int main() {
  const int bad = run_case(3, 14, LOSS_LINEAR, false, true) + run_case(4, 16, LOSS_SOFT_L1, true, false);
  printf(bad ? "FAILED\n" : "kpcam hostcheck ok\n");
  return bad ? 1 : 0;
}
#endif
