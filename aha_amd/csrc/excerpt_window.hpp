// excerpt_window.hpp -- the window of an excerpts call (AHA_GREP_CONTEXT; DESIGN.md 4.16 "Excerpts"): a covered stretch
// [s, e) of the document [a, b) widened by the context, clipped to the document and snapped outwards to UTF-8 character
// boundaries.  Host and device: the kernels of scan_excerpt.hip and a stand-alone CPU program (tests/cpp/
// spec_excerpt_window.cpp) share this one definition.  The rule is bytewise and reads the caller's own bytes, at most three
// on each side and none outside [a, b); on anything but valid UTF-8 it is still defined.  64-bit positions throughout.
#pragma once
#include <cstdint>

#ifndef AHA_HD
#if defined(__HIPCC__)
#define AHA_HD __host__ __device__
#else
#define AHA_HD
#endif
#endif

namespace aha {

constexpr uint32_t kExcerptMaxContext = 0x7FFFFFFFu;  // the largest before / after of a call
constexpr int kExcerptSnap = 3;                       // continuation bytes an edge steps over at most

AHA_HD inline bool excerpt_cont(uint8_t c) { return (c & 0xC0u) == 0x80u; }

// at most three times: x > a and corpus[x] is a continuation byte -> x - 1.  a <= x; x < b wherever x > a
AHA_HD inline uint64_t excerpt_snap_left(const uint8_t *corpus, uint64_t a, uint64_t x) {
  for (int k = 0; k < kExcerptSnap; k++) {
    if (x > a && excerpt_cont(corpus[x]))
      x--;
    else
      break;
  }
  return x;
}

// at most three times: x < b and corpus[x] is a continuation byte -> x + 1.  x <= b
AHA_HD inline uint64_t excerpt_snap_right(const uint8_t *corpus, uint64_t b, uint64_t x) {
  for (int k = 0; k < kExcerptSnap; k++) {
    if (x < b && excerpt_cont(corpus[x]))
      x++;
    else
      break;
  }
  return x;
}

// the window's first byte: for a stretch that starts at s, a <= s < b
AHA_HD inline uint64_t excerpt_w0(const uint8_t *corpus, uint64_t a, uint64_t s, uint32_t before) {
  return excerpt_snap_left(corpus, a, s - a > before ? s - before : a);
}

// the byte behind the window's last: for a stretch that ends at e (exclusive), a < e <= b
AHA_HD inline uint64_t excerpt_w1(const uint8_t *corpus, uint64_t b, uint64_t e, uint32_t after) {
  return excerpt_snap_right(corpus, b, b - e > after ? e + after : b);
}

}  // namespace aha
