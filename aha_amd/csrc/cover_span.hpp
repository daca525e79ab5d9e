// cover_span.hpp -- one span into a bit mask (cover calls: scan_cover.hip, and k_count's cover mode in kernels.hip).
// Bit j of the mask is word j >> 5, bit j & 31.  Vector atomics and plain C++ only.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace aha {

// f(word, bits) for every mask word that the bits [s, e) touch: the first and the last with a partial mask, whole words between
template <class F>
__device__ __forceinline__ void cover_span_words(uint64_t s, uint64_t e, F f) {
  if (s >= e) return;
  const uint64_t w0 = s >> 5, w1 = (e - 1) >> 5;
  const uint32_t m0 = ~0u << (uint32_t)(s & 31), m1 = ~0u >> (31u - (uint32_t)((e - 1) & 31));
  if (w0 == w1) {
    f(w0, m0 & m1);
    return;
  }
  f(w0, m0);
  for (uint64_t w = w0 + 1; w < w1; w++) f(w, ~0u);
  f(w1, m1);
}

// (bits are only ever set between the clear and the end of a call: a word that already shows them needs no atomic, and a stale
// read costs one that changes nothing)
__device__ __forceinline__ void cover_or_word(uint32_t *word, uint32_t bits) {
  if ((*word & bits) != bits) atomicOr(word, bits);
}

// mask bits [s, e) |= 1 in global memory
__device__ __forceinline__ void cover_or_global(uint32_t *mask, uint64_t s, uint64_t e) {
  cover_span_words(s, e, [&](uint64_t w, uint32_t bits) { cover_or_word(mask + w, bits); });
}

}  // namespace aha
