// Host build of the weighted paths of csrc/mcba_keypoint_math.h, csrc/mcba_tricov_math.h and csrc/mcba_kpba_math.h for
// g++: what the weighted instantiations of k_tri_refine, k_tricov_point, k_tricov_cal, k_kpba_status, k_kpba_reduce and k_kpba_step do per lane or
// item, as plain loops in the kernels' order, through an observation functor of four arguments that hands out sqrt(w) as the kernels' does.  The
// weights come in as the C ABI takes them, (C, P) values w >= 0, and are turned into the plane of sqrt(w) (0 for a zero or NaN weight) as the C
// ABI turns them.  tests/test_hostcheck_weights.py compiles this as a shared library (plain -O2) and holds it to tests/weights_oracle.py; with
// -DWEIGHTS_MAIN it is a stand-alone program that the same test builds with -fsanitize=address,undefined and runs as a child process.
#include <cmath>
#include <cstddef>
#include <cstdio>
#include <vector>
#include "../../multicam-calibration_amd/csrc/mcba_kpba_math.h"

using namespace mcba;

#define BY_LOSS(loss, CALL)                         \
  switch (loss) {                                   \
    case LOSS_LINEAR: { constexpr int L = LOSS_LINEAR; CALL; } break;   \
    case LOSS_SOFT_L1: { constexpr int L = LOSS_SOFT_L1; CALL; } break; \
    case LOSS_HUBER: { constexpr int L = LOSS_HUBER; CALL; } break;     \
    case LOSS_CAUCHY: { constexpr int L = LOSS_CAUCHY; CALL; } break;   \
    case LOSS_ARCTAN: { constexpr int L = LOSS_ARCTAN; CALL; } break;   \
    default: return 1;                              \
  }

static std::vector<double> sqrt_plane(const double* w, size_t count) {
  std::vector<double> sq(count);
  for (size_t i = 0; i < count; ++i) sq[i] = w[i] > 0.0 ? sqrt(w[i]) : 0.0;
  return sq;
}

// one point's detections and sqrt(w): the four-argument observation functor
struct Detections {
  const double* uvs;
  const double* sw;
  size_t P, p;
  void operator()(int c, double& ou, double& ov, double& s) const {
    const double* o = uvs + 2 * ((size_t)c * P + p);
    ou = o[0]; ov = o[1];
    s = sw[(size_t)c * P + p];
  }
};

// ---------------------------------------------------------------- k_tri_refine
template <int LOSS>
static void refine_all(int C, size_t P, const double* uvs, const double* sw, const KpCam* t, const double* start, double f_scale, int max_iterations, double* out, double* info) {
  for (size_t p = 0; p < P; ++p) {
    Detections obs{uvs, sw, P, p};
    refine_point<LOSS>(t, C, obs, start + 3 * p, f_scale, max_iterations, out + 3 * p, info + 4 * p);
  }
}

// ---------------------------------------------------------------- k_tricov_point, k_tricov_cal
template <int LOSS>
static void tricov_all(int C, size_t P, const double* pts, const double* uvs, const double* sw, const TcCam* tab, const double* cam_cov, double f_scale, double sigma2_in, double* det6,
                       double* cal6, int* views, int* status, double* info8) {
  const int n = 12 * C;
  const double fs2 = f_scale * f_scale, inv_fs2 = 1.0 / fs2;
  std::vector<KpCam> cams((size_t)C);
  for (int c = 0; c < C; ++c) cams[c] = tab[c].kc;
  std::vector<double> hinv(6 * P);
  double wss = 0.0, m = 0.0, nok = 0.0, ndeg = 0.0;
  for (size_t p = 0; p < P; ++p) {
    Detections obs{uvs, sw, P, p};
    double w;
    status[p] = tricov_point<LOSS>(cams.data(), C, obs, pts + 3 * p, f_scale, hinv.data() + 6 * p, views[p], w);
    if (status[p] == TC_OK) { wss += w; m += 2.0 * views[p]; nok += 1.0; }
    if (status[p] == TC_DEGENERATE) ndeg += 1.0;
  }
  const double sigma2 = sigma2_in == sigma2_in ? sigma2_in : tricov_sigma2(wss, m, 3.0 * nok);
  info8[0] = sigma2; info8[1] = m; info8[2] = 3.0 * nok; info8[3] = (double)P - nok - ndeg; info8[4] = ndeg;
  info8[5] = info8[6] = info8[7] = 0.0;
  std::vector<double> G((size_t)3 * n), Z((size_t)3 * n);
  for (size_t p = 0; p < P; ++p) {
    const bool ok = status[p] == TC_OK;
    for (int e = 0; e < 6; ++e) det6[6 * p + e] = tricov_det_entry(hinv[6 * p + e], sigma2, ok);
    if (!cam_cov) continue;
    for (double& v : G) v = 0.0;
    if (ok) {
      for (int c = 0; c < C; ++c) {
        const double* o = uvs + 2 * ((size_t)c * P + p);
        const double s = sw[(size_t)c * P + p];
        if (!(o[0] == o[0] && o[1] == o[1] && s > 0.0)) continue;
        double g[36];
        tricov_g_block<LOSS>(tab[c], pts + 3 * p, o[0], o[1], s, hinv.data() + 6 * p, fs2, inv_fs2, g);
        for (int k = 0; k < 3; ++k)
          for (int j = 0; j < 12; ++j) G[(size_t)k * n + 12 * c + j] = g[12 * k + j];
      }
    }
    for (int k = 0; k < 3; ++k)
      for (int j = 0; j < n; ++j) {
        double s = 0.0;
        for (int i = 0; i < n; ++i) s += G[(size_t)k * n + i] * cam_cov[(size_t)i * n + j];
        Z[(size_t)k * n + j] = s;
      }
    for (int e = 0; e < 6; ++e) {
      int k, l;
      tricov_tri3_pair(e, k, l);
      double s = 0.0;
      for (int j = 0; j < n; ++j) s += Z[(size_t)k * n + j] * G[(size_t)l * n + j];
      cal6[6 * p + e] = tricov_cal_entry(s, ok);
    }
  }
}

// ---------------------------------------------------------------- k_kpba_status, k_kpba_reduce, k_kpba_step and the loop
template <int LOSS>
struct HostBackEnd {
  int C;
  size_t P;
  const double* uvs;     // (C, P, 2)
  const double* sw;      // (C, P)
  const double* cam12;   // (C, 12): intrinsics; the extrinsics come per call
  const double* dist5;
  const int* held;
  double f_scale;
  std::vector<double> X[2];
  std::vector<int> status;
  std::vector<TcCam> tab, tab_trial;
  int cur = 0;

  void table(const double* ext, std::vector<TcCam>& t) const {
    t.resize((size_t)C);
    for (int c = 0; c < C; ++c) {
      double q[12];
      for (int k = 0; k < 6; ++k) { q[k] = cam12[12 * c + k]; q[6 + k] = ext[6 * c + k]; }
      make_tc_cam(q, dist5 ? dist5 + 5 * c : nullptr, t[c]);
    }
  }
  void statuses(const double* ext) {
    table(ext, tab);
    status.resize(P);
    for (size_t p = 0; p < P; ++p) {
      Detections obs{uvs, sw, P, p};
      KbPoint pt;
      kpba_point<LOSS_LINEAR>(tab.data(), C, obs, X[cur].data() + 3 * p, 1.0, 1.0, nullptr, pt);
      status[p] = kpba_status(pt.views, X[cur].data() + 3 * p, pt.H);
    }
  }
  int reduce(const double* ext, double lam, KbSystem& sys) {
    table(ext, tab);
    sys.shape(C);
    sys.cost = sys.count = sys.gmax = 0.0;
    const double fs2 = f_scale * f_scale, inv_fs2 = 1.0 / fs2;
    const int n6 = 6 * C;
    std::vector<double> Y((size_t)n6 * 3);
    for (size_t p = 0; p < P; ++p) {
      if (status[p] != KB_USED) continue;
      const double* Xp = X[cur].data() + 3 * p;
      Detections obs{uvs, sw, P, p};
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
        double ou, ov, s;
        obs(c, ou, ov, s);
        if (!(ou == ou && ov == ov && s > 0.0)) continue;
        double acc[kKbAcc];
        kpba_item<LOSS>(tab[c], Xp, ou, ov, s, fs2, inv_fs2, f, zp, held[c], Y.data() + 18 * c, acc);
        for (int k = 0; k < kKbAcc; ++k) sys.acc[(size_t)c * kKbAcc + k] += acc[k];
      }
      for (int i = 0; i < n6; ++i)
        for (int j = 0; j < n6; ++j) sys.YY[(size_t)i * sys.NP + j] += Y[3 * i] * Y[3 * j] + Y[3 * i + 1] * Y[3 * j + 1] + Y[3 * i + 2] * Y[3 * j + 2];
    }
    return 0;
  }
  int step(const double* ext_trial, const double* dtheta, double lam, double out[3]) {
    table(ext_trial, tab_trial);
    const double fs2 = f_scale * f_scale, inv_fs2 = 1.0 / fs2;
    out[0] = out[1] = out[2] = 0.0;
    X[1 - cur] = X[cur];
    for (size_t p = 0; p < P; ++p) {
      if (status[p] != KB_USED) continue;
      const double* Xp = X[cur].data() + 3 * p;
      Detections obs{uvs, sw, P, p};
      KbPoint pt, tr;
      kpba_point<LOSS>(tab.data(), C, obs, Xp, fs2, inv_fs2, dtheta, pt);
      KbFactor f;
      double dX[3] = {0.0, 0.0, 0.0};
      if (kpba_factor(pt.H, lam, f)) kpba_point_step(f, pt.g, pt.q, dX);
      double* Xt = X[1 - cur].data() + 3 * p;
      for (int j = 0; j < 3; ++j) { Xt[j] = Xp[j] + dX[j]; out[1] += dX[j] * dX[j]; out[2] += Xp[j] * Xp[j]; }
      kpba_point<LOSS>(tab_trial.data(), C, obs, Xt, fs2, inv_fs2, nullptr, tr);
      out[0] += tr.cost;
    }
    return 0;
  }
  void accept() { cur = 1 - cur; }
  void start(const double* pts, std::vector<double>& ext) {
    X[0].assign(pts, pts + 3 * P);
    ext.resize((size_t)6 * C);
    for (int c = 0; c < C; ++c)
      for (int k = 0; k < 6; ++k) ext[6 * c + k] = cam12[12 * c + 6 + k];
    statuses(ext.data());
  }
};

template <int LOSS>
static int run(int C, size_t P, const double* uvs, const double* sw, const double* cam12, const double* dist5, const double* pts0, int* held, int gauge, int scale_cam, double f_scale,
               const KbOptions& opt, double* ext_out, double* pts, int* status, double* res8, double* hist, int hist_cap) {
  HostBackEnd<LOSS> be{C, P, uvs, sw, cam12, dist5, held, f_scale};
  std::vector<double> ext;
  be.start(pts0, ext);
  for (int c = 0; c < C; ++c) {   // a camera that no used point sees with a positive weight is held whole
    bool seen = false;
    for (size_t p = 0; p < P && !seen; ++p) {
      const double* o = uvs + 2 * ((size_t)c * P + p);
      seen = be.status[p] == KB_USED && o[0] == o[0] && o[1] == o[1] && sw[(size_t)c * P + p] > 0.0;
    }
    if (!seen) held[c] = 63;
  }
  if (held[scale_cam] == 63) return 2;
  held[gauge] = 63;
  const double baseline = kpba_baseline(ext.data(), gauge, scale_cam);
  KbResult r;
  if (int rc = kpba_lm(be, C, held, ext.data(), opt, r, hist, hist_cap)) return rc;
  for (size_t p = 0; p < P; ++p) {
    status[p] = be.status[p];
    for (int j = 0; j < 3; ++j) pts[3 * p + j] = status[p] == KB_USED ? be.X[be.cur][3 * p + j] : std::nan("");
  }
  const double s = kpba_rescale(C, held, ext.data(), P, pts, gauge, scale_cam, baseline);
  for (int k = 0; k < 6 * C; ++k) ext_out[k] = ext[k];
  res8[0] = r.cost; res8[1] = r.cost0; res8[2] = r.optimality; res8[3] = r.nfev; res8[4] = r.njev; res8[5] = r.status; res8[6] = s; res8[7] = r.nhist;
  return 0;
}

template <int LOSS>
static void system_at(int C, size_t P, const double* uvs, const double* sw, const double* cam12, const double* dist5, const double* pts, const int* held, double f_scale, double lam,
                      const double* ext_trial, const double* dtheta, double* YY, double* acc, double* scal3, int* status, double* trial, double* out3) {
  HostBackEnd<LOSS> be{C, P, uvs, sw, cam12, dist5, held, f_scale};
  std::vector<double> ext;
  be.start(pts, ext);
  KbSystem sys;
  be.reduce(ext.data(), lam, sys);
  for (size_t i = 0; i < sys.YY.size(); ++i) YY[i] = sys.YY[i];
  for (size_t i = 0; i < sys.acc.size(); ++i) acc[i] = sys.acc[i];
  scal3[0] = sys.cost; scal3[1] = sys.count; scal3[2] = sys.gmax;
  for (size_t p = 0; p < P; ++p) status[p] = be.status[p];
  if (ext_trial) {
    be.step(ext_trial, dtheta, lam, out3);
    for (size_t i = 0; i < 3 * P; ++i) trial[i] = be.X[1][i];
  }
}

extern "C" {

// k_tri_refine: uvs (C, P, 2), w (C, P), start / out (P, 3), info (P, 4).  1: a loss out of range
int hc_w_refine(int C, size_t P, const double* uvs, const double* w, const double* cam12, const double* dist5, const double* start, int loss, double f_scale, int max_iterations, double* out,
                double* info) {
  std::vector<KpCam> t((size_t)C);
  for (int c = 0; c < C; ++c) make_kp_cam(cam12 + 12 * c, dist5 ? dist5 + 5 * c : nullptr, t[c]);
  const std::vector<double> sw = sqrt_plane(w, (size_t)C * P);
  BY_LOSS(loss, refine_all<L>(C, P, uvs, sw.data(), t.data(), start, f_scale, max_iterations, out, info));
  return 0;
}

// k_tricov_point + k_tricov_cal: cam_cov (12 C, 12 C) or NULL (cal6 then untouched); det6 / cal6 (P, 6), views / status (P), info8
int hc_w_tricov(int C, size_t P, const double* pts, const double* uvs, const double* w, const double* cam12, const double* dist5, const double* cam_cov, int loss, double f_scale,
                double sigma2_in, double* det6, double* cal6, int* views, int* status, double* info8) {
  std::vector<TcCam> tab((size_t)C);
  for (int c = 0; c < C; ++c) make_tc_cam(cam12 + 12 * c, dist5 ? dist5 + 5 * c : nullptr, tab[c]);
  const std::vector<double> sw = sqrt_plane(w, (size_t)C * P);
  BY_LOSS(loss, tricov_all<L>(C, P, pts, uvs, sw.data(), tab.data(), cam_cov, f_scale, sigma2_in, det6, cal6, views, status, info8));
  return 0;
}

// one evaluation: YY (NP, NP), acc (C, 33), scal3 = cost, present scalars, max |g_p|, status (P); with ext_trial and dtheta also trial (P, 3) and
// out3 = trial cost, sum dX^2, sum X^2
int hc_w_system(int C, size_t P, const double* uvs, const double* w, const double* cam12, const double* dist5, const double* pts, const int* held, int loss, double f_scale, double lam,
                const double* ext_trial, const double* dtheta, double* YY, double* acc, double* scal3, int* status, double* trial, double* out3) {
  const std::vector<double> sw = sqrt_plane(w, (size_t)C * P);
  BY_LOSS(loss, system_at<L>(C, P, uvs, sw.data(), cam12, dist5, pts, held, f_scale, lam, ext_trial, dtheta, YY, acc, scal3, status, trial, out3));
  return 0;
}

// the loop: held (C) in/out; ext (C, 6), pts (P, 3), status (P), res8 = cost cost0 optimality nfev njev status scale evaluations, hist (hist_cap, 3)
int hc_w_kpba(int C, size_t P, const double* uvs, const double* w, const double* cam12, const double* dist5, const double* pts0, int* held, int gauge, int scale_cam, int loss, double f_scale,
              double ftol, double xtol, double gtol, int max_nfev, double* ext, double* pts, int* status, double* res8, double* hist, int hist_cap) {
  const KbOptions opt{ftol, xtol, gtol, max_nfev};
  const std::vector<double> sw = sqrt_plane(w, (size_t)C * P);
  BY_LOSS(loss, return run<L>(C, P, uvs, sw.data(), cam12, dist5, pts0, held, gauge, scale_cam, f_scale, opt, ext, pts, status, res8, hist, hist_cap));
  return 0;
}

}  // extern "C"

#ifdef WEIGHTS_MAIN
// 4 cameras x 11 points, weights on four levels with zeros and a NaN, a camera that sees nothing, a point with one view of positive weight:
// every entry point once, and the identities that need no oracle (a zero weight = a NaN detection, bit for bit)
int main() {
  const int C = 4, P = 11;
  std::vector<double> cam12(12 * C), dist5(5 * C), pts(3 * P), uvs((size_t)2 * C * P), w((size_t)C * P);
  for (int c = 0; c < C; ++c) {
    const double q[12] = {900.0 + 10 * c, 905.0, 640.0, 512.0, -0.1, 0.02, 0.02 * c, 0.05 * c, -0.01 * c, -150.0 * c, 10.0 * c, 5.0 * c};
    for (int k = 0; k < 12; ++k) cam12[12 * c + k] = q[k];
    const double d[5] = {-0.1, 0.02, 1e-3, -5e-4, 0.01};
    for (int k = 0; k < 5; ++k) dist5[5 * c + k] = d[k];
  }
  std::vector<TcCam> tab(C);
  for (int c = 0; c < C; ++c) make_tc_cam(cam12.data() + 12 * c, dist5.data() + 5 * c, tab[c]);
  const double levels[4] = {0.25, 1.0, 4.0, 0.0};
  for (int p = 0; p < P; ++p) {
    pts[3 * p] = 37.0 * (p % 5) - 80.0 + 3.0 * p; pts[3 * p + 1] = 60.0 - 29.0 * (p % 4); pts[3 * p + 2] = 900.0 + 45.0 * (p % 3) - 11.0 * p;
    for (int c = 0; c < C; ++c) {
      double u, v;
      project5<false>(tab[c].kc, pts.data() + 3 * p, u, v);
      double* o = uvs.data() + 2 * ((size_t)c * P + p);
      o[0] = u + 0.3 * ((p + c) % 3 - 1); o[1] = v - 0.2 * ((p + 2 * c) % 3 - 1);
      w[(size_t)c * P + p] = levels[(3 * p + c) % 7 == 0 ? 3 : (p + 2 * c) % 3];
      if (c == C - 1) o[0] = o[1] = std::nan("");                    // the last camera sees nothing
      if (p == P - 1 && c >= 1) w[(size_t)c * P + p] = c == 1 ? std::nan("") : 0.0;   // the last point: one view of positive weight
    }
  }
  for (int c = 1; c < C; ++c) { cam12[12 * c + 6] += 2e-3; cam12[12 * c + 10] += 1.0; }
  int bad = 0;
  // the same problem with the zero and NaN weights written as NaN detections and weight 1 there
  std::vector<double> uvs2 = uvs, w2 = w;
  for (size_t i = 0; i < (size_t)C * P; ++i)
    if (!(w[i] > 0.0)) { uvs2[2 * i] = uvs2[2 * i + 1] = std::nan(""); w2[i] = 1.0; }
  std::vector<double> out(3 * P), out2(3 * P), info(4 * P), info2(4 * P);
  bad += hc_w_refine(C, P, uvs.data(), w.data(), cam12.data(), dist5.data(), pts.data(), LOSS_SOFT_L1, 1.5, 50, out.data(), info.data());
  bad += hc_w_refine(C, P, uvs2.data(), w2.data(), cam12.data(), dist5.data(), pts.data(), LOSS_SOFT_L1, 1.5, 50, out2.data(), info2.data());
  for (int i = 0; i < 3 * P; ++i)
    if (!(out[i] == out2[i] || (out[i] != out[i] && out2[i] != out2[i]))) { printf("refine: zero weight != NaN detection at %d\n", i); ++bad; }
  if (info[4 * (P - 1) + 3] != KP_TOO_FEW_VIEWS) { printf("refine: the one-view point has status %g\n", info[4 * (P - 1) + 3]); ++bad; }
  const int n = 12 * C;
  std::vector<double> cov((size_t)n * n), det(6 * P), cal(6 * P), det2(6 * P), cal2(6 * P), info8(8), info8b(8);
  for (int i = 0; i < n; ++i)
    for (int j = 0; j < n; ++j) cov[(size_t)i * n + j] = (i == j ? 1e-4 : 2e-6) * (1.0 + 0.01 * ((i + j) % 5));
  std::vector<int> views(P), status(P), views2(P), status2(P);
  bad += hc_w_tricov(C, P, out.data(), uvs.data(), w.data(), cam12.data(), dist5.data(), cov.data(), LOSS_CAUCHY, 2.0, std::nan(""), det.data(), cal.data(), views.data(), status.data(), info8.data());
  bad += hc_w_tricov(C, P, out.data(), uvs2.data(), w2.data(), cam12.data(), dist5.data(), cov.data(), LOSS_CAUCHY, 2.0, std::nan(""), det2.data(), cal2.data(), views2.data(), status2.data(),
                     info8b.data());
  for (int p = 0; p < P; ++p) {
    if (views[p] != views2[p] || status[p] != status2[p]) { printf("tricov: point %d views %d / %d status %d / %d\n", p, views[p], views2[p], status[p], status2[p]); ++bad; }
    for (int e = 0; e < 6; ++e)
      if (std::isfinite(det[6 * p + e]) != (status[p] == TC_OK) || std::isfinite(cal[6 * p + e]) != (status[p] == TC_OK)) ++bad;
  }
  if (status[P - 1] != TC_TOO_FEW_VIEWS) { printf("tricov: the one-view point has status %d\n", status[P - 1]); ++bad; }
  std::vector<int> held(C, 0), kst(P);
  held[0] = 63; held[1] |= 1 << 3;
  std::vector<double> ext(6 * C), kpts(3 * P), res(8), hist(3 * 40);
  const int rc = hc_w_kpba(C, P, uvs.data(), w.data(), cam12.data(), dist5.data(), pts.data(), held.data(), 0, 1, LOSS_SOFT_L1, 1.5, 1e-12, 1e-12, 1e-10, 40, ext.data(), kpts.data(), kst.data(),
                           res.data(), hist.data(), 40);
  if (rc != 0) { printf("kpba: returned %d\n", rc); ++bad; }
  if (!(res[0] <= res[1])) { printf("kpba: the cost rose: %g -> %g\n", res[1], res[0]); ++bad; }
  if (kst[P - 1] != KB_TOO_FEW_VIEWS || held[C - 1] != 63) { printf("kpba: status %d held %d\n", kst[P - 1], held[C - 1]); ++bad; }
  const int NP = (6 * C + 15) / 16 * 16;
  std::vector<double> YY((size_t)NP * NP), acc((size_t)C * kKbAcc), scal(3), trial(3 * P), out3(3), dth(6 * C, 1e-4), ext_trial(6 * C);
  for (int c = 0; c < C; ++c)
    for (int k = 0; k < 6; ++k) ext_trial[6 * c + k] = cam12[12 * c + 6 + k] + dth[6 * c + k];
  bad += hc_w_system(C, P, uvs.data(), w.data(), cam12.data(), dist5.data(), pts.data(), held.data(), LOSS_HUBER, 1.0, 1e-4, ext_trial.data(), dth.data(), YY.data(), acc.data(), scal.data(),
                     kst.data(), trial.data(), out3.data());
  printf("refine cost %.6g; tricov sigma2 %.6g m %g; kpba cost %.6g -> %.6g in %g evaluations; system cost %.6g count %g trial cost %.6g\n", info[0], info8[0], info8[1], res[1], res[0], res[3], scal[0],
         scal[1], out3[0]);
  printf(bad ? "FAILED\n" : "weights hostcheck ok\n");
  return bad ? 1 : 0;
}
#endif
