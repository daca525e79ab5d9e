// class_overflow.hpp -- the one place where a class-counts call (aha_ac_class_counts_batch*, engine.cpp device_class_counts) can
// overflow its uint32 entries, as a host function of its own: it cannot be reached at test sizes, so it is kept small enough to
// be read and is tested on made-up hit offsets (tests/cpp/spec_class_overflow.cpp).  Host code only; no HIP.
#pragma once
#include <cstdint>

namespace aha {

// hit_off[0 .. n_docs]: the documents' hit offsets as the count call gives them (ascending).  A class count of a document is at
// most that document's hit count (a key names a class at most once), so a batch with fewer than 2^32 hits in all cannot
// overflow and no document is looked at; otherwise the first document with 2^32 hits or more is the answer (*doc, where asked
// for).  false: every count of the call fits 32 bits.
inline bool class_counts_overflow(const uint64_t *hit_off, uint64_t n_docs, uint64_t *doc = nullptr) {
  constexpr uint64_t kLimit = 1ull << 32;
  if (!n_docs || hit_off[n_docs] - hit_off[0] < kLimit) return false;
  for (uint64_t d = 0; d < n_docs; d++)
    if (hit_off[d + 1] - hit_off[d] >= kLimit) {
      if (doc) *doc = d;
      return true;
    }
  return false;
}

}  // namespace aha
