// Host build of csrc/mcba_keypoint_math.h -- the per-lane text of csrc/mcba_keypoints.hip (k_project, k_keypoint_errors, k_tri_refine) -- for g++:
// the loops over the points that the GPU runs one lane each, with the camera table built by the same make_kp_cam the C ABI uses.
// tests/test_hostcheck_keypoints.py compiles this (also under AddressSanitizer + UBSan) and applies the GPU tier's gates to it.
#include <cstddef>
#include <vector>
#include "../../multicam-calibration_amd/csrc/mcba_keypoint_math.h"

using namespace mcba;

static std::vector<KpCam> table(int C, const double* cam12, const double* dist5) {
  std::vector<KpCam> t((size_t)C);
  for (int c = 0; c < C; ++c) make_kp_cam(cam12 + 12 * c, dist5 ? dist5 + 5 * c : nullptr, t[c]);
  return t;
}

template <int LOSS>
static void refine_all(int C, size_t P, const double* uvs, const KpCam* t, const double* start, double f_scale, int max_iterations, double* out, double* info) {
  for (size_t p = 0; p < P; ++p) {
    auto observation = [&](int c, double& ou, double& ov) {
      const double* o = uvs + 2 * ((size_t)c * P + p);
      ou = o[0]; ov = o[1];
    };
    refine_point<LOSS>(t, C, observation, start + 3 * p, f_scale, max_iterations, out + 3 * p, info + 4 * p);
  }
}

extern "C" {

// mode 0: project_only (k1, k2 of cam12 or of dist5), 1: the five-coefficient model.  out (C, P, 2)
void hc_kp_project(int C, size_t P, const double* pts, const double* cam12, const double* dist5, int mode, double* out) {
  const std::vector<KpCam> t = table(C, cam12, dist5);
  for (int c = 0; c < C; ++c)
    for (size_t p = 0; p < P; ++p) {
      double* o = out + 2 * ((size_t)c * P + p);
      if (mode == 0) project_only(t[c].K, t[c].pc, pts + 3 * p, o[0], o[1]);
      else project5<false>(t[c], pts + 3 * p, o[0], o[1]);
    }
}

void hc_kp_rigid(size_t P, const double* pts, const double* T12, double* out) {
  PairConst pc;
  for (int i = 0; i < 9; ++i) pc.Rcf[i] = T12[i];
  for (int i = 0; i < 3; ++i) pc.tcf[i] = T12[9 + i];
  for (size_t p = 0; p < P; ++p) rigid_point(pc, pts + 3 * p, out + 3 * p);
}

// uvs (C, P, 2); err (C, P)
void hc_kp_errors(int C, size_t P, const double* pts, const double* uvs, const double* cam12, const double* dist5, double* err) {
  const std::vector<KpCam> t = table(C, cam12, dist5);
  for (int c = 0; c < C; ++c)
    for (size_t p = 0; p < P; ++p) {
      const double* o = uvs + 2 * ((size_t)c * P + p);
      err[(size_t)c * P + p] = keypoint_error(t[c], pts + 3 * p, o[0], o[1]);
    }
}

// start / out (P, 3), info (P, 4); loss 0 .. 4.  Returns 0, or 1 for a loss out of range.
int hc_kp_refine(int C, size_t P, const double* uvs, const double* cam12, const double* dist5, const double* start, int loss, double f_scale, int max_iterations, double* out, double* info) {
  const std::vector<KpCam> t = table(C, cam12, dist5);
  switch (loss) {
    case LOSS_LINEAR: refine_all<LOSS_LINEAR>(C, P, uvs, t.data(), start, f_scale, max_iterations, out, info); break;
    case LOSS_SOFT_L1: refine_all<LOSS_SOFT_L1>(C, P, uvs, t.data(), start, f_scale, max_iterations, out, info); break;
    case LOSS_HUBER: refine_all<LOSS_HUBER>(C, P, uvs, t.data(), start, f_scale, max_iterations, out, info); break;
    case LOSS_CAUCHY: refine_all<LOSS_CAUCHY>(C, P, uvs, t.data(), start, f_scale, max_iterations, out, info); break;
    case LOSS_ARCTAN: refine_all<LOSS_ARCTAN>(C, P, uvs, t.data(), start, f_scale, max_iterations, out, info); break;
    default: return 1;
  }
  return 0;
}

}  // extern "C"
