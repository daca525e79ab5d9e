// doc_ranges.hpp -- the one place where the rule is written by which a call that works on a hit list per range (doc counts,
// select and replace, class counts: engine.cpp) cuts a batch into ranges of whole documents whose hits fit a bound of scratch.
// The bound that matters (about 2 GiB of hits) cannot be reached at test sizes, so the rule is a host function of its own, small
// enough to be read, and is tested on made-up hit offsets (tests/cpp/spec_doc_ranges.cpp).  Host code only; no HIP.
#pragma once
#include <cstdint>
#include <vector>

namespace aha {

struct DocRange {
  uint64_t d0, d1;  // the documents [d0, d1)
  bool solo;        // one document whose cost alone is beyond the bound: the caller never matches it
};

// hit_off[0 .. n_docs]: the documents' hit offsets as the count call gives them (ascending); cost(h): the bytes a document with
// h hits holds in scratch while its range is worked on, cost(0) == 0.
//   - No hit at all: no range.
//   - All documents together cost at most `bound`: the one range [0, n_docs), the caller's batch as it is.
//   - Otherwise a range opens at the next document with hits.  It is solo, and that document alone, where the document's cost
//     exceeds the bound; else it takes the documents behind it while the sum stays at most the bound -- hitless ones cost nothing
//     and come along.  The documents in no range have no hits.
// The ranges come out ascending and disjoint.  false: no memory for `out`.
template <class Cost>
bool doc_ranges(const uint64_t *hit_off, uint64_t n_docs, uint64_t bound, Cost cost, std::vector<DocRange> &out) {
  out.clear();
  if (!n_docs || hit_off[n_docs] == hit_off[0]) return true;
  try {
    uint64_t all = 0;
    for (uint64_t d = 0; d < n_docs && all <= bound; d++) {
      const uint64_t c = cost(hit_off[d + 1] - hit_off[d]);
      all = c > bound ? c : all + c;  // (both at most the bound before the sum: no wrap)
    }
    if (all <= bound) {
      out.push_back(DocRange{0, n_docs, false});
      return true;
    }
    for (uint64_t d0 = 0; d0 < n_docs;) {
      if (hit_off[d0 + 1] == hit_off[d0]) {
        d0++;
        continue;
      }
      uint64_t d1 = d0 + 1, bytes = cost(hit_off[d0 + 1] - hit_off[d0]);
      const bool solo = bytes > bound;
      while (!solo && d1 < n_docs) {
        const uint64_t c = cost(hit_off[d1 + 1] - hit_off[d1]);
        if (c > bound || bytes + c > bound) break;
        bytes += c;
        d1++;
      }
      out.push_back(DocRange{d0, d1, solo});
      d0 = d1;
    }
  } catch (...) {
    return false;
  }
  return true;
}

// The tiling of a token call (engine.cpp device_select_to with AHA_SELECT_TOKENS), whose ranges take every document, hits or
// none, and whose work per range grows with the text as well: bounds[0] = 0 < bounds[1] < .. < bounds.back() = n_docs (range r
// is [bounds[r], bounds[r + 1]); n_docs == 0: bounds = {0}, no range).  A range takes documents while its hits cost at most
// `bound` bytes (12 each) AND its text costs at most `bound` bytes (8 each: the L table of the select passes, the largest
// scratch a text byte holds); a document beyond either is a range of its own.
// doc_off[0 .. n_docs]: the documents' offsets into the text.  All documents within both bounds: the one range [0, n_docs).
// false: no memory for `bounds`.
inline bool doc_tiles(const uint64_t *hit_off, const uint64_t *doc_off, uint64_t n_docs, uint64_t bound, std::vector<uint64_t> &bounds) {
  try {
    bounds.assign(1, 0);
    for (uint64_t d0 = 0; d0 < n_docs;) {
      // (differences of ascending offsets: no wrap.)  Documents without a byte cost nothing and come along, so every range
      // holds text unless the whole batch has none; the first document with text is taken whatever it costs
      uint64_t d1 = d0;
      bool any = false;
      for (; d1 < n_docs; d1++) {
        if (doc_off[d1 + 1] == doc_off[d1]) continue;
        if (any && (hit_off[d1 + 1] - hit_off[d0] > bound / 12 || doc_off[d1 + 1] - doc_off[d0] > bound / 8)) break;
        any = true;
      }
      bounds.push_back(d1);
      d0 = d1;
    }
  } catch (...) {
    return false;
  }
  return true;
}

}  // namespace aha
