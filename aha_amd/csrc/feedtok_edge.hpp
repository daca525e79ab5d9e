// feedtok_edge.hpp -- what a feed token call (aha_feed_select_batch* with AHA_FEED_SELECT_TOKENS; DESIGN.md 4.10 "Feed tokens")
// decides at the two ends of a piece's tokens.  Host and device: the edge pass of scan_feedtokens.hip and a stand-alone CPU
// program (tests/cpp/spec_feedtok_edge.cpp) share this one definition.  All positions are bytes of the sequence.
//   t0 <= c0 <= c1 <= n1   the token cursor and the select cursor the call finds, the select cursor it leaves, the new length
//   n_starts, last_start   the token starts in [c0, c1) by the rule of token_rule.hpp -- c0 itself standing for a document's
//                          start where t0 == c0 -- and the last of them (read only where n_starts > 0)
// [t0, c0) is the front part of a gap token that is still open (the carried token); with the starts it gives the token list
// Tok1 of T[t0 .. c1).  c1 is a certain boundary iff the call is FINAL, gaps are runs, the last settled hit ends there, or the
// byte at c1 is known and is no continuation byte.  Where it is not certain, the last token of Tok1 -- a gap token that ends
// at c1 -- stays open: it is not reported and the token cursor stops at its start.
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

struct FeedTokEdge {
  uint64_t t1;       // the token cursor the call leaves
  uint64_t count;    // tokens the call reports for the piece
  uint32_t carried;  // Tok1 begins with the carried token [t0, ..)
  uint32_t open;     // the last token of Tok1 is not reported
  uint32_t too_long; // the call would leave more than `bound` bytes behind the token cursor
};

// hit_end_at_c1: the last hit the call settles ends at c1.  cont_at_c1: byte c1 is a continuation byte (read only where c1 < n1)
AHA_HD inline FeedTokEdge feedtok_edge(uint64_t t0, uint64_t c0, uint64_t c1, uint64_t n1, uint64_t n_starts, uint64_t last_start,
                                       bool hit_end_at_c1, bool cont_at_c1, bool final, bool gap_runs, uint64_t bound) {
  FeedTokEdge e;
  e.carried = t0 < c0 ? 1u : 0u;
  e.open = 0;
  const uint64_t n_tok = n_starts + e.carried;
  const bool certain = final || gap_runs || hit_end_at_c1 || (c1 < n1 && !cont_at_c1);
  if (n_tok == 0) {  // (t0 == c0 == c1: nothing to report)
    e.t1 = t0;
    e.count = 0;
  } else if (certain) {
    e.t1 = c1;
    e.count = n_tok;
  } else {
    e.open = 1;
    e.t1 = n_starts ? last_start : t0;
    e.count = n_tok - 1;
  }
  e.too_long = !final && n1 - e.t1 > bound ? 1u : 0u;
  return e;
}

}  // namespace aha
