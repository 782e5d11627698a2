// mcba_ransac_host.h -- what the host bodies of the RANSAC entry points share before anything reaches the device (mcba_twoview_api.hip,
// mcba_resect_api.hip): the descriptor of a hypothesis generator and the check of a table of host-drawn samples.  Plain C++, no HIP types: the
// host harnesses (tests/hostcheck) compile the same text with g++.
#pragma once
#include <cstddef>
#include <string>

namespace mcba {

// What tells the generators of an estimator apart: indices per sample, rows of the hypothesis table per sample, the bound on the number of
// samples and the message (after the entry's name) for a count outside it.
struct Generator {
  const char* who;
  int size, slots, max_h;
  const char* range;
};

// rows samples of `size` indices each: every index within 0 .. limit - 1, usable (usable[index] != 0; nullptr: every point is) and not repeated
// within its sample.  True, or false with *msg = who + the first fault met, row by row, index by index, in this order.
inline bool samples_ok(const char* who, const int* samples, size_t rows, int size, size_t limit, const unsigned char* usable, std::string* msg) {
  for (size_t r = 0; r < rows; ++r) {
    const int* s = samples + (size_t)size * r;
    for (int k = 0; k < size; ++k) {
      const char* what = nullptr;
      if (s[k] < 0 || (size_t)s[k] >= limit) what = ": a sample index is outside 0 .. n_points - 1";
      else if (usable && !usable[s[k]]) what = ": a sampled point is not usable for its camera";
      else
        for (int j = 0; j < k && !what; ++j)
          if (s[j] == s[k]) what = ": an index is repeated within a sample";
      if (what) { *msg = std::string(who) + what; return false; }
    }
  }
  return true;
}

}  // namespace mcba
