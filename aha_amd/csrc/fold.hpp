// fold.hpp -- the ASCII case fold of AHA_OPT_FOLD_ASCII (include/aha_hip.h), host and device.  The ONLY place the rule is
// written down: fold(b) = b + 32 for 0x41 <= b <= 0x5A ('A' .. 'Z'), b otherwise.  Bytes >= 0x80, '@', '[', '`' and '{' stay,
// lengths and UTF-8 lead bytes never change.  Compile folds a copy of the keys with it (capi.cpp), the prefix-filter engine
// folds its text loads (scan_filter.hip), every other engine reads a copy folded on the way (scan_fold.hip).
#pragma once
#include <cstddef>
#include <cstdint>

#ifndef AHA_HD
#if defined(__HIPCC__)
#define AHA_HD __host__ __device__
#else
#define AHA_HD
#endif
#endif

namespace aha {

AHA_HD inline uint8_t fold8(uint8_t b) { return (uint8_t)(b - 0x41u) < 26u ? (uint8_t)(b + 32u) : b; }

// Four bytes at once, no carry from one byte into the next: with t = the low seven bits of every byte, bit 7 of t + 0x3f is
// set for t >= 0x41 and bit 7 of t + 0x25 for t >= 0x5b, so m has bit 7 of exactly the bytes in 'A' .. 'Z' (~w: not those
// with their own bit 7 set); m >> 2 is their 0x20.
AHA_HD inline uint32_t fold32(uint32_t w) {
  const uint32_t t = w & 0x7f7f7f7fu;
  const uint32_t m = (t + 0x3f3f3f3fu) & ~(t + 0x25252525u) & ~w & 0x80808080u;
  return w | (m >> 2);
}

// 16 bytes as four words (any type with .x .y .z .w or operator[] would do: the kernels' own vector types differ)
AHA_HD inline void fold128(uint32_t &a, uint32_t &b, uint32_t &c, uint32_t &d) {
  a = fold32(a);
  b = fold32(b);
  c = fold32(c);
  d = fold32(d);
}

inline void fold_bytes(uint8_t *p, size_t n) {
  for (size_t i = 0; i < n; i++) p[i] = fold8(p[i]);
}

}  // namespace aha
