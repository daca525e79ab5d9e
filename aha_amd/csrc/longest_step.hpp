// longest_step.hpp -- one byte of match_longest_ (src/aha/ac.cr:118-143) for the feed's kernels (scan_feedlongest.hip): the
// step of kernels.hip (k_longest_docs / k_longest_chunks), restated over three small types so that it can take the two bytes in
// front of the current one as values and compiles as plain host code too (tests/cpp/spec_feed_longest.cpp):
//   P     the probe of the image: P::go(A, B, b, key), P::fail(A, B), P::child_or_root(A, B, b)  (devcommon.hpp Probe<COMPACT>)
//   AUT   the image: root, s1_lo, s2_lo, s2_hi, term_bits, stale_bits                            (image.hpp DevAut)
//   PREV  the two bytes in front of the current one, y() = text[p - 1], x() = text[p - 2]: the shadow fail links of the states
//         without a header are functions of them (automaton.hpp, Placement::headerless) and nothing else looks back.
//         LongestPrevRegs carries them as values -- a feed's piece starts with the bytes of ANOTHER sequence's piece in front of
//         it, or with no text at all; LongestPrevPtr reads them through the text pointer as the batch kernels do
// kernels.hip keeps its own copy of the step (and of Pending, kNoKey, kValueNode: the same definitions).  Both batch kernels were
// built on this header once: the instructions of their write passes came out the same and those of their count passes in another
// register allocation, and the batch mode-2 call measured 0.4 % slower than the parent's over two alternating series
// (profiles/feed_longest_bench.json, "gate"; DESIGN.md 4.10 "Feed match_longest"), so the batch kernels stay as they were.  A
// change to one copy of the step belongs in the other; tests/test_gpu_longest.py and tests/test_gpu_feed_longest.py hold both to
// the oracle.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define AHA_LS_FN __device__ __forceinline__
#else
#define AHA_LS_FN inline
#endif

namespace aha {

constexpr uint32_t kNoKey = 0xFFFFFFFFu;  // a pending end that yields nothing
constexpr uint32_t kValueNode = 0xFFFFFFFEu;
struct Pending {
  int64_t p = -1;      // absolute position of the pending end (-1: none)
  uint32_t key = 0;
  uint32_t endc = 0;   // chars mode: lead bytes of the document up to and including p
};

struct LongestPrevPtr {
  const uint8_t *tp;  // the current (not yet consumed) byte
  AHA_LS_FN uint32_t y() const { return tp[-1]; }
  AHA_LS_FN uint32_t x() const { return tp[-2]; }
};

struct LongestPrevRegs {
  uint32_t y_ = 0, x_ = 0;
  AHA_LS_FN uint32_t y() const { return y_; }
  AHA_LS_FN uint32_t x() const { return x_; }
  AHA_LS_FN void push(uint32_t b) {
    x_ = y_;
    y_ = b;
  }
};

// fails[nid] (ac.cr:189) of a non-root state B: devcommon.hpp fail_of with the two bytes in front taken from `prev`
template <class P, class AUT, class PREV>
AHA_LS_FN uint32_t longest_fail_of(const AUT &A, uint32_t B, const PREV &prev) {
  if (B >= A.s2_hi) return P::fail(A, B);  // header (every state when the ranges are all 0)
  if (B < A.s1_lo) return A.root;          // depth 1
  const uint32_t y = prev.y();
  if (B >= A.s2_lo) {  // depth >= 3: the deepest state of depth <= 2 spelled by the last two bytes
    const uint32_t x = prev.x();
    const uint32_t s1 = P::child_or_root(A, A.root, x);
    if (s1 != A.root) {
      const uint32_t s2 = P::child_or_root(A, s1, y);
      if (s2 != A.root) return s2;
    }
  }
  return P::child_or_root(A, A.root, y);  // depth-1 state of the last byte, or root
}

// One byte b at position p.  Returns true when a pending end was yielded (into *out).
template <class P, class AUT, class PREV>
AHA_LS_FN bool longest_step(const AUT &A, uint32_t &B, uint32_t b, const PREV &prev, int64_t p, uint32_t lc, bool intersectable,
                            Pending &pend, Pending *out) {
  bool yielded = false;
  if (B == kValueNode) {  // no goto from it, no fail link: the pending (empty) end is yielded, the byte is gone
    *out = pend;
    pend.p = -1;
    B = A.root;
    return true;
  }
  for (;;) {
    uint32_t key = 0;
    if (b == 0 && A.term_bits && ((A.term_bits[B >> 5] >> (B & 31)) & 1u)) {
      B = kValueNode;
      pend.p = p;
      pend.key = kNoKey;
      pend.endc = lc;
      break;
    }
    const int r = b ? P::go(A, B, b, key) : 0;  // a NUL byte has no other goto (keys hold none)
    if (r) {
      if (r == 2) {
        pend.p = p;
        pend.key = key;
        pend.endc = lc;
      } else if (A.stale_bits && ((A.stale_bits[B >> 5] >> (B & 31)) & 1u)) {
        pend.p = p;
        pend.key = kNoKey;
        pend.endc = lc;
      }
      break;
    }
    if (pend.p >= 0) {
      *out = pend;
      yielded = true;
      pend.p = -1;
      if (!intersectable) B = A.root;
    }
    if (B == A.root) break;
    B = longest_fail_of<P>(A, B, prev);
  }
  return yielded;
}

}  // namespace aha
