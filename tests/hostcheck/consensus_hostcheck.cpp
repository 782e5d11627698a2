// Host build of csrc/mcba_consensus_math.h -- the per-lane text of csrc/mcba_consensus.hip -- for g++: the loop over the points that the GPU runs
// one lane (or one wavefront) each, with the camera table built by the same make_kp_cam the C ABI uses.  stride 1 is the lane form's whole-point
// routine; stride > 1 runs the wavefront form's schedule on the host: `stride` running bests, one per residue of the pair index, then the
// lexicographic (cost, k) minimum over them.  tests/test_hostcheck_consensus.py compiles this (also under AddressSanitizer + UBSan).
#include <cstddef>
#include <vector>
#include "../../multicam-calibration_amd/csrc/mcba_consensus_math.h"

using namespace mcba;

template <int LOSS>
static void consensus_all(int C, size_t P, const double* uvs, const KpCam* t, const double* proj, double threshold, int min_views, int und_iters, double f_scale, int max_iterations, int stride,
                          double* out, unsigned long long* mask, double* info) {
  for (size_t p = 0; p < P; ++p) {
    auto observation = [&](int c, double& ou, double& ov) {
      const double* o = uvs + 2 * ((size_t)c * P + p);
      ou = o[0]; ov = o[1];
    };
    if (stride <= 1) {
      consensus_point<LOSS>(t, proj, C, observation, threshold, min_views, und_iters, f_scale, max_iterations, out + 3 * p, mask[p], info + 8 * p);
      continue;
    }
    ConsBest win;
    cons_best_init(win);
    for (int lane = 0; lane < stride; ++lane) {
      ConsBest b;
      cons_best_init(b);
      consensus_search(t, proj, C, observation, threshold, und_iters, lane, stride, b);
      if (cons_before(b.cost, b.k, win.cost, win.k)) win = b;
    }
    consensus_finish<LOSS>(t, C, observation, win, min_views, f_scale, max_iterations, out + 3 * p, info + 8 * p);
    mask[p] = win.mask;
  }
}

extern "C" {

// uvs (C, P, 2); out (P, 3), mask (P), info (P, 8); loss 0 .. 4.  Returns 0, or 1 for an argument out of range.
int hc_consensus(int C, size_t P, const double* uvs, const double* cam12, const double* dist5, double threshold, int min_views, int und_iters, int loss, double f_scale, int max_iterations, int stride,
                 double* out, unsigned long long* mask, double* info) {
  if (C < 2 || C > kKpMaxCams || !(threshold > 0.0) || min_views < 2) return 1;
  std::vector<KpCam> t((size_t)C);
  std::vector<double> proj((size_t)12 * C);
  for (int c = 0; c < C; ++c) {
    make_kp_cam(cam12 + 12 * c, dist5 ? dist5 + 5 * c : nullptr, t[c]);
    cons_projection(t[c], proj.data() + 12 * c);
  }
  switch (loss) {
    case LOSS_LINEAR: consensus_all<LOSS_LINEAR>(C, P, uvs, t.data(), proj.data(), threshold, min_views, und_iters, f_scale, max_iterations, stride, out, mask, info); break;
    case LOSS_SOFT_L1: consensus_all<LOSS_SOFT_L1>(C, P, uvs, t.data(), proj.data(), threshold, min_views, und_iters, f_scale, max_iterations, stride, out, mask, info); break;
    case LOSS_HUBER: consensus_all<LOSS_HUBER>(C, P, uvs, t.data(), proj.data(), threshold, min_views, und_iters, f_scale, max_iterations, stride, out, mask, info); break;
    case LOSS_CAUCHY: consensus_all<LOSS_CAUCHY>(C, P, uvs, t.data(), proj.data(), threshold, min_views, und_iters, f_scale, max_iterations, stride, out, mask, info); break;
    case LOSS_ARCTAN: consensus_all<LOSS_ARCTAN>(C, P, uvs, t.data(), proj.data(), threshold, min_views, und_iters, f_scale, max_iterations, stride, out, mask, info); break;
    default: return 1;
  }
  return 0;
}

// the hypothesis of pair (pairs[2 p], pairs[2 p + 1]) for every point p: out (P, 3), kept (P) 0 / 1 (void: out untouched)
void hc_consensus_hypothesis(int C, size_t P, const double* uvs, const double* cam12, const double* dist5, int und_iters, const int* pairs, double* out, int* kept) {
  std::vector<KpCam> t((size_t)C);
  std::vector<double> proj((size_t)12 * C);
  for (int c = 0; c < C; ++c) {
    make_kp_cam(cam12 + 12 * c, dist5 ? dist5 + 5 * c : nullptr, t[c]);
    cons_projection(t[c], proj.data() + 12 * c);
  }
  for (size_t p = 0; p < P; ++p) {
    auto observation = [&](int c, double& ou, double& ov) {
      const double* o = uvs + 2 * ((size_t)c * P + p);
      ou = o[0]; ov = o[1];
    };
    const int i = pairs[2 * p], j = pairs[2 * p + 1];
    kept[p] = i >= 0 && j > i && j < C && consensus_hypothesis(t.data(), proj.data(), i, j, observation, und_iters, out + 3 * p) ? 1 : 0;
  }
}

}  // extern "C"
