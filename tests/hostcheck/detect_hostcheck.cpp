// Host-side harness for csrc/mcba_detect_math.h -- TEST INFRASTRUCTURE ONLY.
// Compiles the detection kernels' arithmetic with g++ so that tests/test_detection_cpu.py can check it against the numpy transcriptions of
// tests/cv_transcriptions.py without a GPU.  Never loaded by the product.
#include "../../multicam-calibration_amd/csrc/mcba_detect_math.h"
#include <vector>

using namespace mcba::det;

extern "C" {

void hc_grey(long n, const uint8_t* bgr, uint8_t* out) {
  for (long i = 0; i < n; ++i) out[i] = grey_bgr(bgr[3 * i], bgr[3 * i + 1], bgr[3 * i + 2]);
}

void hc_rect_subpix(const uint8_t* img, int W, int H, float cx, float cy, int pw, int ph, float* out) {
  for (int i = 0; i < ph; ++i)
    for (int j = 0; j < pw; ++j) out[i * pw + j] = rect_subpix(img, W, H, cx, cy, pw, ph, i, j);
}

void hc_subpix_mask(int w, int h, float* out) {
  for (int i = 0; i < 2 * h + 1; ++i)
    for (int j = 0; j < 2 * w + 1; ++j) out[i * (2 * w + 1) + j] = subpix_mask(i, j, w, h);
}

// one iteration from (x, y); returns 0 when the determinant test stops it.  xy: in / out
int hc_subpix_iteration(const uint8_t* img, int W, int H, int w, int h, float* xy) {
  const int pw = 2 * w + 3, ph = 2 * h + 3;
  std::vector<float> patch(pw * ph);
  hc_rect_subpix(img, W, H, xy[0], xy[1], pw, ph, patch.data());
  SubpixSums s{0, 0, 0, 0, 0};
  for (int i = 0; i < 2 * h + 1; ++i)
    for (int j = 0; j < 2 * w + 1; ++j) subpix_term(patch.data(), w, h, i, j, subpix_mask(i, j, w, h), s);
  double err = 0;
  return subpix_update(s, xy[0], xy[1], err) ? 1 : 0;
}

void hc_corner_subpix(const uint8_t* img, int W, int H, int n, const float* start, int w, int h, float* out) {
  for (int k = 0; k < n; ++k) {
    float xy[2] = {start[2 * k], start[2 * k + 1]};
    const int pw = 2 * w + 3, ph = 2 * h + 3;
    std::vector<float> patch(pw * ph);
    for (int iter = 0; iter < kSubpixMaxIter; ++iter) {
      hc_rect_subpix(img, W, H, xy[0], xy[1], pw, ph, patch.data());
      SubpixSums s{0, 0, 0, 0, 0};
      for (int i = 0; i < 2 * h + 1; ++i)
        for (int j = 0; j < 2 * w + 1; ++j) subpix_term(patch.data(), w, h, i, j, subpix_mask(i, j, w, h), s);
      double err = 0;
      if (!subpix_update(s, xy[0], xy[1], err)) break;
      if (subpix_outside(xy[0], xy[1], W, H)) break;
      if (!(err > kSubpixEps2)) break;
    }
    if (fabsf(xy[0] - start[2 * k]) > (float)w || fabsf(xy[1] - start[2 * k + 1]) > (float)h) { xy[0] = start[2 * k]; xy[1] = start[2 * k + 1]; }
    out[2 * k] = xy[0];
    out[2 * k + 1] = xy[1];
  }
}

int hc_persp4(const double* src, const double* dst, double* M) { return persp4(src, dst, M) ? 1 : 0; }

void hc_warp(const uint8_t* img, int W, int H, const double* M, uint8_t* out) {
  for (int y = 0; y < kTemplate; ++y)
    for (int x = 0; x < kTemplate; ++x) out[y * kTemplate + x] = warp_pixel(img, W, H, M, x, y);
}

void hc_template(uint8_t* out) {
  for (int y = 0; y < kTemplate; ++y)
    for (int x = 0; x < kTemplate; ++x) out[y * kTemplate + x] = template_pixel(x, y);
}

double hc_pearson(int n, const uint8_t* r, const uint8_t* t) {
  double sr = 0, st = 0, srr = 0, stt = 0, srt = 0;
  for (int i = 0; i < n; ++i) { sr += r[i]; st += t[i]; srr += (double)r[i] * r[i]; stt += (double)t[i] * t[i]; srt += (double)r[i] * t[i]; }
  return pearson(n, sr, st, srr, stt, srt);
}

void hc_homography(const double* xy, const double* uv, int n, double* H) { homography_dlt(xy, uv, n, H); }

}  // extern "C"
