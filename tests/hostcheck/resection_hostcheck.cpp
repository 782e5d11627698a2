// Host build of csrc/mcba_resect_math.h -- the per-lane text of csrc/mcba_resect.hip and the loop rs_lm -- for g++: the loops over points and
// hypotheses that the GPU spreads over lanes, for one camera, with the arguments of mcba_resect_ransac / mcba_resect_refine (include/mcba.h) less
// the device and the timing.  The sums run in index order here; the kernels' order is their own, and both are held to the bounds of
// tests/resection_oracle.py.  tests/test_hostcheck_resection.py compiles this into a shared object; with -DRS_HOSTCHECK_MAIN it is a stand-alone
// program that reads a scene file (the sanitizer build: its own main, nothing preloaded).
#include <cstddef>
#include <cstdio>
#include <cstdint>
#include <vector>
#include "../../multicam-calibration_amd/csrc/mcba_resect_math.h"
#include "../../multicam-calibration_amd/csrc/mcba_ransac_host.h"

using namespace mcba;

extern "C" {

// The check that mcba_resect_ransac and mcba_resect_ransac_p3p make of a camera's table of host-drawn samples before the upload
// (csrc/mcba_ransac_host.h), the same text.  usable: a byte per point, or NULL.  Returns 1 for a table that passes; 0 with the message in msg
// (cap bytes of room, NUL-terminated).
int hc_samples_ok(const char* who, const int* samples, size_t rows, int size, size_t limit, const unsigned char* usable, char* msg, size_t cap) {
  std::string m;
  const bool ok = samples_ok(who, samples, rows, size, limit, usable, &m);
  snprintf(msg, cap, "%s", m.c_str());
  return ok ? 1 : 0;
}

// out4: 4 planes of P doubles (undistorted u, v; normalised x, y), usable: P bytes
void hc_rs_prepare(size_t P, const double* points, const double* uv, const double* cam12, const double* dist5, int und_iters, double* out4, unsigned char* usable) {
  const double k9[9] = {cam12[0], cam12[1], cam12[2], cam12[3], dist5[0], dist5[1], dist5[2], dist5[3], dist5[4]};
  for (size_t p = 0; p < P; ++p) {
    const bool ok = rs_usable(points[3 * p], points[3 * p + 1], points[3 * p + 2], uv[2 * p], uv[2 * p + 1]);
    double o[4];
    rs_prepare(uv[2 * p], uv[2 * p + 1], k9, k9 + 4, und_iters, o);
    for (int k = 0; k < 4; ++k) out4[k * P + p] = ok ? o[k] : 0.0;
    usable[p] = ok ? 1 : 0;
  }
}

// One camera.  Returns 0, or 1 for an argument out of range (nothing written).
int hc_resect_ransac(size_t P, const double* points, const double* uv, const double* cam12, const double* dist5, int H, const int* samples, const double* poses_in, double threshold, int und_iters,
                     double* rt12, double* best4, unsigned char* inliers, double* pose_out, double* cost_out, unsigned* count_out, int* status_out) {
  if (P < 1 || H < 1 || !(threshold > 0.0) || (!samples && !poses_in)) return 1;
  std::vector<double> prep(4 * P);
  std::vector<unsigned char> use(P);
  hc_rs_prepare(P, points, uv, cam12, dist5, und_iters, prep.data(), use.data());
  size_t n_use = 0;
  for (size_t p = 0; p < P; ++p) n_use += use[p];
  if (!poses_in)
    for (int i = 0; i < kRsSample * H; ++i)
      if (samples[i] < 0 || (size_t)samples[i] >= P || !use[samples[i]]) return 1;
  const double *pu = prep.data(), *pv = pu + P, *nx = pv + P, *ny = nx + P;
  std::vector<double> pose(12 * (size_t)H), KP(12 * (size_t)H), cost((size_t)H);
  std::vector<int> status((size_t)H);
  std::vector<unsigned> count((size_t)H);
  const double t2 = threshold * threshold;
  int win = 0;
  for (int h = 0; h < H; ++h) {
    double* q = pose.data() + 12 * (size_t)h;
    if (poses_in) {
      bool ok = true;
      for (int i = 0; i < 12; ++i) { q[i] = poses_in[12 * (size_t)h + i]; ok = ok && rs_finite(q[i]); }
      status[h] = ok ? RS_OK : RS_VOID;
    } else {
      double X[18], x[12], S[144], V[144], step[6];
      for (int k = 0; k < kRsSample; ++k) {
        const int s = samples[kRsSample * (size_t)h + k];
        for (int j = 0; j < 3; ++j) X[3 * k + j] = points[3 * (size_t)s + j];
        x[2 * k] = nx[s]; x[2 * k + 1] = ny[s];
      }
      status[h] = rs_hypothesis(X, x, S, V, q, step);
    }
    double* kp = KP.data() + 12 * (size_t)h;
    rs_pixel_matrix(q, cam12, kp);
    double c = 0.0;
    unsigned n = 0;
    for (size_t p = 0; p < P; ++p) {
      if (!use[p]) continue;
      const double e2 = rs_error2(kp, points[3 * p], points[3 * p + 1], points[3 * p + 2], pu[p], pv[p]);
      c += tv_cost_term(e2, t2);
      n += tv_inlier(e2, t2) ? 1u : 0u;
    }
    cost[h] = status[h] == RS_OK ? c : __builtin_inf();
    count[h] = status[h] == RS_OK ? n : 0u;
    if (tv_before(cost[h], h, cost[win], win)) win = h;
  }
  const double* kp = KP.data() + 12 * (size_t)win;
  for (size_t p = 0; p < P; ++p)
    inliers[p] = use[p] && status[win] == RS_OK && tv_inlier(rs_error2(kp, points[3 * p], points[3 * p + 1], points[3 * p + 2], pu[p], pv[p]), t2) ? 1 : 0;
  for (int i = 0; i < 12; ++i) rt12[i] = pose[12 * (size_t)win + i];
  best4[0] = (double)win; best4[1] = cost[win]; best4[2] = (double)count[win]; best4[3] = (double)n_use;
  for (int h = 0; h < H; ++h) {
    if (pose_out) for (int i = 0; i < 12; ++i) pose_out[12 * (size_t)h + i] = pose[12 * (size_t)h + i];
    if (cost_out) cost_out[h] = cost[h];
    if (count_out) count_out[h] = count[h];
    if (status_out) status_out[h] = status[h];
  }
  return 0;
}

}  // extern "C"

namespace {

// rs_lm's back end in plain loops: one camera per problem, the points in index order
struct HostBackEnd {
  int loss;
  size_t P;
  const double *points, *uvs, *cam12, *dist5;
  const unsigned char* mask;
  double f_scale;
  int evaluations = 0;

  template <int LOSS>
  void one(bool cost_only, int c, const double* pose6, double* sys) const {
    double cam[12];
    for (int i = 0; i < 6; ++i) { cam[i] = cam12[12 * c + i]; cam[6 + i] = pose6[i]; }
    TcCam tc;
    make_tc_cam(cam, dist5 + 5 * c, tc);
    const double fs2 = f_scale * f_scale, inv = 1.0 / fs2;
    for (int i = 0; i < kRsSys; ++i) sys[i] = 0.0;
    for (size_t p = 0; p < P; ++p) {
      const double* X = points + 3 * p;
      const double ou = uvs[2 * ((size_t)c * P + p)], ov = uvs[2 * ((size_t)c * P + p) + 1];
      if (!mask[(size_t)c * P + p] || !rs_usable(X[0], X[1], X[2], ou, ov)) continue;
      if (cost_only) { sys[27] += rs_cost_item<LOSS>(tc, X, ou, ov, fs2, inv); sys[28] += 1.0; continue; }
      double acc[kRsSys];
      rs_normal_item<LOSS>(tc, X, ou, ov, fs2, inv, acc);
      for (int i = 0; i < kRsSys; ++i) sys[i] += acc[i];
    }
  }
  void evaluate(bool cost_only, int n, const int* ids, const double* poses6, double* sys) {
    ++evaluations;
    for (int k = 0; k < n; ++k) {
      double* s = sys + (size_t)kRsSys * k;
      switch (loss) {
        case LOSS_LINEAR: one<LOSS_LINEAR>(cost_only, ids[k], poses6 + 6 * k, s); break;
        case LOSS_SOFT_L1: one<LOSS_SOFT_L1>(cost_only, ids[k], poses6 + 6 * k, s); break;
        case LOSS_HUBER: one<LOSS_HUBER>(cost_only, ids[k], poses6 + 6 * k, s); break;
        case LOSS_CAUCHY: one<LOSS_CAUCHY>(cost_only, ids[k], poses6 + 6 * k, s); break;
        default: one<LOSS_ARCTAN>(cost_only, ids[k], poses6 + 6 * k, s); break;
      }
    }
  }
  int normal(int n, const int* ids, const double* poses6, double* out) { evaluate(false, n, ids, poses6, out); return 0; }
  int trial(int n, const int* ids, const double* poses6, double* cost) {
    std::vector<double> sys((size_t)kRsSys * n);
    evaluate(true, n, ids, poses6, sys.data());
    for (int k = 0; k < n; ++k) cost[k] = sys[(size_t)kRsSys * k + 27];
    return 0;
  }
};

}  // namespace

extern "C" {

// mcba_resect_refine's arguments less the device.  Returns 0, or 1 for an argument out of range.  evaluations (1 int or NULL): calls of the back end.
int hc_resect_refine(int C, size_t P, const double* points, const double* uvs, const unsigned char* mask, const double* cam12, const double* dist5, const int* active, int loss, double f_scale,
                     double ftol, double xtol, double gtol, int max_nfev, double* extrinsics_out, double* result, double* system_out, int* evaluations) {
  if (C < 1 || P < 1 || loss < LOSS_LINEAR || loss > LOSS_ARCTAN || !(f_scale > 0.0) || max_nfev < 1) return 1;
  std::vector<RsCamera> cams((size_t)C);
  for (int c = 0; c < C; ++c) {
    for (int i = 0; i < 6; ++i) cams[c].pose[i] = cam12[12 * c + 6 + i];
    for (int i = 0; i < kRsSys; ++i) cams[c].sys[i] = __builtin_nan("");
    cams[c].status = (!active || active[c]) ? -1 : -2;
  }
  HostBackEnd be{loss, P, points, uvs, cam12, dist5, mask, f_scale};
  const KbOptions opt{ftol, xtol, gtol, max_nfev};
  if (rs_lm(be, C, cams.data(), opt)) return 2;
  const double nan = __builtin_nan("");
  for (int c = 0; c < C; ++c) {
    const RsCamera& cm = cams[c];
    const bool on = cm.status != -2;
    for (int i = 0; i < 6; ++i) extrinsics_out[6 * c + i] = cm.pose[i];
    double* r = result + 8 * c;
    r[0] = on ? cm.cost0 : nan; r[1] = on ? cm.cost : nan; r[2] = on ? cm.optimality : nan; r[3] = on ? cm.nfev : nan; r[4] = on ? cm.njev : nan;
    r[5] = on ? cm.status : nan; r[6] = on ? cm.sys[28] : nan; r[7] = on ? cm.lam : nan;
    if (system_out)
      for (int i = 0; i < kRsSys; ++i) system_out[kRsSys * c + i] = cm.sys[i];
  }
  if (evaluations) *evaluations = be.evaluations;
  return 0;
}

}  // extern "C"

#ifdef RS_HOSTCHECK_MAIN
// scene file: int64 P, int64 H, double threshold, int64 und_iters, then points (3 P), uv (2 P), cam12 (12), dist5 (5) doubles, samples (6 H) int32.
// Runs the RANSAC, then the polish (soft_l1) from the winner on its inliers.
int main(int argc, char** argv) {
  if (argc < 2) return 2;
  FILE* fh = fopen(argv[1], "rb");
  if (!fh) return 2;
  int64_t P = 0, H = 0, it = 0;
  double thr = 0.0;
  bool ok = fread(&P, 8, 1, fh) == 1 && fread(&H, 8, 1, fh) == 1 && fread(&thr, 8, 1, fh) == 1 && fread(&it, 8, 1, fh) == 1 && P >= 6 && H >= 1 && P < (1 << 24) && H < (1 << 16);
  if (!ok) { fclose(fh); return 2; }
  std::vector<double> pts(3 * P), uv(2 * P), cam(12), dist(5);
  std::vector<int> smp(6 * H);
  ok = fread(pts.data(), 8, pts.size(), fh) == pts.size() && fread(uv.data(), 8, uv.size(), fh) == uv.size() && fread(cam.data(), 8, 12, fh) == 12 && fread(dist.data(), 8, 5, fh) == 5 &&
       fread(smp.data(), 4, smp.size(), fh) == smp.size();
  fclose(fh);
  if (!ok) return 2;
  char msg[128];
  if (!hc_samples_ok("main", smp.data(), (size_t)H, 6, (size_t)P, nullptr, msg, sizeof msg)) return 6;
  std::vector<double> rt(12), best(4), pose(12 * H), cost(H);
  std::vector<unsigned char> inl(P);
  std::vector<unsigned> cnt(H);
  std::vector<int> st(H);
  if (hc_resect_ransac((size_t)P, pts.data(), uv.data(), cam.data(), dist.data(), (int)H, smp.data(), nullptr, thr, (int)it, rt.data(), best.data(), inl.data(), pose.data(), cost.data(), cnt.data(),
                       st.data()))
    return 3;
  printf("winner %d cost %.17g inliers %d usable %d\n", (int)best[0], best[1], (int)best[2], (int)best[3]);
  // rotation vector of the winner (angles below pi), then the polish
  const double c = fmin(1.0, fmax(-1.0, (rt[0] + rt[4] + rt[8] - 1.0) / 2.0)), th = acos(c);
  const double w[3] = {rt[7] - rt[5], rt[2] - rt[6], rt[3] - rt[1]};
  const double f = th < 1e-12 ? 0.5 : th / (2.0 * sin(th));
  for (int i = 0; i < 3; ++i) { cam[6 + i] = f * w[i]; cam[9 + i] = rt[9 + i]; }
  std::vector<double> ext(6), res(8), sys(kRsSys);
  int ev = 0;
  if (hc_resect_refine(1, (size_t)P, pts.data(), uv.data(), inl.data(), cam.data(), dist.data(), nullptr, LOSS_SOFT_L1, 1.0, 1e-8, 1e-8, 1e-8, 50, ext.data(), res.data(), sys.data(), &ev)) return 4;
  printf("polish cost %.17g -> %.17g nfev %d status %d evaluations %d\n", res[0], res[1], (int)res[3], (int)res[5], ev);
  return res[1] <= res[0] ? 0 : 5;
}
#endif
