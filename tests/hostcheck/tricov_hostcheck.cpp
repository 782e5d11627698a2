// Host build of csrc/mcba_tricov_math.h -- the per-lane text of csrc/mcba_tricov.hip (k_tricov_point, k_tricov_cal) -- for g++: the loops over the
// points that the GPU runs one lane (or one workgroup item) each, the camera table built by the same make_tc_cam the C ABI uses, the product
// Z = G Sigma_cc as plain loops.  tests/test_hostcheck_tricov.py compiles this as a shared library (plain -O2) and holds it to the GPU tier's
// bound; with -DTRICOV_MAIN it is a stand-alone program (two small cases) that the same test builds with -fsanitize=address,undefined and runs
// as a child process.
#include <cmath>
#include <cstddef>
#include <cstdio>
#include <vector>
#include "../../multicam-calibration_amd/csrc/mcba_tricov_math.h"

using namespace mcba;

template <int LOSS>
static void tricov_all(int C, size_t P, const double* pts, const double* uvs, const TcCam* tab, const double* cam_cov, double f_scale, double sigma2_in, double* det6, double* cal6,
                       double* G_out, int* views, int* status, double* info8) {
  const int n = 12 * C;
  const double fs2 = f_scale * f_scale, inv_fs2 = 1.0 / fs2;
  std::vector<KpCam> cams((size_t)C);
  for (int c = 0; c < C; ++c) cams[c] = tab[c].kc;
  std::vector<double> hinv(6 * P);
  double wss = 0.0, m = 0.0, nok = 0.0, ndeg = 0.0;
  for (size_t p = 0; p < P; ++p) {
    auto observation = [&](int c, double& ou, double& ov) {
      const double* o = uvs + 2 * ((size_t)c * P + p);
      ou = o[0]; ov = o[1];
    };
    double w;
    status[p] = tricov_point<LOSS>(cams.data(), C, observation, pts + 3 * p, f_scale, hinv.data() + 6 * p, views[p], w);
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
    if (!cam_cov && !G_out) continue;
    for (double& v : G) v = 0.0;
    if (ok) {
      for (int c = 0; c < C; ++c) {
        const double* o = uvs + 2 * ((size_t)c * P + p);
        if (!(o[0] == o[0] && o[1] == o[1])) continue;
        double g[36];
        tricov_g_block<LOSS>(tab[c], pts + 3 * p, o[0], o[1], hinv.data() + 6 * p, fs2, inv_fs2, g);
        for (int k = 0; k < 3; ++k)
          for (int j = 0; j < 12; ++j) G[(size_t)k * n + 12 * c + j] = g[12 * k + j];
      }
    }
    if (G_out)
      for (size_t i = 0; i < (size_t)3 * n; ++i) G_out[(size_t)3 * n * p + i] = ok ? G[i] : std::nan("");
    if (!cam_cov) continue;
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

extern "C" {

// uvs (C, P, 2), pts (P, 3), cam_cov (12 C, 12 C) or NULL; det6 / cal6 (P, 6), G_out (P, 3, 12 C) or NULL, views / status (P), info8.
// Returns 0, or 1 for a loss out of range.
int hc_tricov(int C, size_t P, const double* pts, const double* uvs, const double* cam12, const double* dist5, const double* cam_cov, int loss, double f_scale, double sigma2_in, double* det6,
              double* cal6, double* G_out, int* views, int* status, double* info8) {
  std::vector<TcCam> tab((size_t)C);
  for (int c = 0; c < C; ++c) make_tc_cam(cam12 + 12 * c, dist5 ? dist5 + 5 * c : nullptr, tab[c]);
  switch (loss) {
    case LOSS_LINEAR: tricov_all<LOSS_LINEAR>(C, P, pts, uvs, tab.data(), cam_cov, f_scale, sigma2_in, det6, cal6, G_out, views, status, info8); break;
    case LOSS_SOFT_L1: tricov_all<LOSS_SOFT_L1>(C, P, pts, uvs, tab.data(), cam_cov, f_scale, sigma2_in, det6, cal6, G_out, views, status, info8); break;
    case LOSS_HUBER: tricov_all<LOSS_HUBER>(C, P, pts, uvs, tab.data(), cam_cov, f_scale, sigma2_in, det6, cal6, G_out, views, status, info8); break;
    case LOSS_CAUCHY: tricov_all<LOSS_CAUCHY>(C, P, pts, uvs, tab.data(), cam_cov, f_scale, sigma2_in, det6, cal6, G_out, views, status, info8); break;
    case LOSS_ARCTAN: tricov_all<LOSS_ARCTAN>(C, P, pts, uvs, tab.data(), cam_cov, f_scale, sigma2_in, det6, cal6, G_out, views, status, info8); break;
    default: return 1;
  }
  return 0;
}

// one camera at one point: uv (2), A (2, 3), B (2, 12)
void hc_tricov_rows(const double* cam12, const double* dist5, const double* X, double* uv, double* A, double* B) {
  TcCam tc;
  make_tc_cam(cam12, dist5, tc);
  tricov_cam_rows(tc, X, uv[0], uv[1], A, A + 3, B, B + 12);
}

}  // extern "C"

#ifdef TRICOV_MAIN
// two cameras a baseline apart looking down +z (the second with a small rotation), a third one further along
static void rig(int C, double* cam12, double* dist5) {
  for (int c = 0; c < C; ++c) {
    const double q[12] = {900.0 + 10 * c, 905.0, 640.0, 512.0, -0.1, 0.02, 0.0, c == 0 ? 0.0 : 0.05 * c, 0.0, -150.0 * c, 10.0 * c, 0.0};
    for (int k = 0; k < 12; ++k) cam12[12 * c + k] = q[k];
    const double d[5] = {-0.1, 0.02, 1e-3, -5e-4, 0.01};
    for (int k = 0; k < 5; ++k) dist5[5 * c + k] = d[k];
  }
}

static int run_case(int C, int P, bool with_cov, bool with_degenerate) {
  std::vector<double> cam12(12 * C), dist5(5 * C), pts(3 * P), uvs((size_t)2 * C * P), cov;
  rig(C, cam12.data(), dist5.data());
  if (with_degenerate)
    for (int k = 0; k < 12; ++k) cam12[12 + k] = cam12[k];   // camera 1 = camera 0: a point they alone see has a singular H
  std::vector<TcCam> tab(C);
  for (int c = 0; c < C; ++c) make_tc_cam(cam12.data() + 12 * c, dist5.data() + 5 * c, tab[c]);
  for (int p = 0; p < P; ++p) {
    pts[3 * p] = 40.0 * p - 60.0; pts[3 * p + 1] = 25.0 - 13.0 * p; pts[3 * p + 2] = 900.0 + 35.0 * p;
    for (int c = 0; c < C; ++c) {
      double u, v;
      project5<false>(tab[c].kc, pts.data() + 3 * p, u, v);
      double* o = uvs.data() + 2 * ((size_t)c * P + p);
      o[0] = u + 0.3 * ((p + c) % 3 - 1); o[1] = v - 0.2 * ((p + 2 * c) % 3 - 1);
      if ((with_degenerate && p == 0 && c >= 2) || (P > 2 && p == P - 1 && c >= 1)) o[0] = o[1] = std::nan("");   // point 0: cameras 0, 1 alone; the last: one view
    }
  }
  const int n = 12 * C;
  if (with_cov) {
    cov.assign((size_t)n * n, 0.0);
    for (int i = 0; i < n; ++i)
      for (int j = 0; j < n; ++j) cov[(size_t)i * n + j] = (i == j ? 1e-4 : 2e-6) * (1.0 + 0.01 * ((i + j) % 5));
  }
  std::vector<double> det(6 * P), cal(6 * P), G((size_t)3 * n * P), info(8);
  std::vector<int> views(P), status(P);
  if (hc_tricov(C, P, pts.data(), uvs.data(), cam12.data(), dist5.data(), with_cov ? cov.data() : nullptr, LOSS_SOFT_L1, 2.0, std::nan(""), det.data(), with_cov ? cal.data() : nullptr, G.data(),
                views.data(), status.data(), info.data()) != 0) return 1;
  int bad = 0;
  for (int p = 0; p < P; ++p) {
    const int want = (P > 2 && p == P - 1) ? TC_TOO_FEW_VIEWS : (with_degenerate && p == 0 ? TC_DEGENERATE : TC_OK);
    if (status[p] != want) { printf("point %d: status %d, expected %d\n", p, status[p], want); ++bad; }
    for (int e = 0; e < 6; ++e) {
      const bool fin = std::isfinite(det[6 * p + e]) && (!with_cov || std::isfinite(cal[6 * p + e]));
      if (fin != (want == TC_OK)) { printf("point %d entry %d: finite %d\n", p, e, (int)fin); ++bad; }
    }
  }
  printf("C %d P %d: sigma2 %.6g m %g free %g unusable %g degenerate %g\n", C, P, info[0], info[1], info[2], info[3], info[4]);
  return bad;
}

int main() {
  const int bad = run_case(2, 1, false, false) + run_case(3, 5, true, true);
  printf(bad ? "FAILED\n" : "tricov hostcheck ok\n");
  return bad ? 1 : 0;
}
#endif
