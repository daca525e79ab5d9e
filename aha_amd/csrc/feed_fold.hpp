// feed_fold.hpp -- one byte of the fold a feed on a handle folded beyond ASCII sees (AHA_FEED_FOLD; DESIGN.md 4.13 "Feeds on
// handles folded beyond ASCII"), host and device: the sequence's context and the piece behind it taken as ONE run of bytes that
// ends with the piece.  Both kernels of scan_feedfold.hip are this function -- kff_heads for the first two bytes of a piece,
// kff_windows for every byte of a head window -- and tests/cpp/spec_feed_fold.cpp holds it against fold2_bytes / fold3_bytes_with
// of ctx || P.
#pragma once
#include <cstdint>

#include "fold.hpp"

namespace aha {

// Byte k of ctx || P, k relative to the piece's first byte (k < 0: the context's byte -k from its end); 0 -- neither a lead nor
// a continuation byte -- where there is none: in front of the context and behind the piece's end.  Every index is tested first,
// so an empty context, an empty piece and a piece of one or two bytes need no case of their own.
AHA_HD inline uint32_t feedfold_at(const uint8_t *ctx, uint32_t lc, const uint8_t *p, uint64_t L, int64_t k) {
  if (k < 0) return -k <= (int64_t)lc ? ctx[(int64_t)lc + k] : 0u;
  return (uint64_t)k < L ? p[k] : 0u;
}

// Byte k of fold(ctx || P), the handle's fold `mode`: 2 fold2 (T.pair alone is read), 3 fold3, 4 foldk (T holds FK's tables).
// A character cut between the context and the piece is folded whole, one still open at the piece's end passes through.
AHA_HD inline uint8_t feedfold_byte(const Fold3Tables &T, int mode, const uint8_t *ctx, uint32_t lc, const uint8_t *p, uint64_t L,
                                    int64_t k) {
  const uint32_t prev = feedfold_at(ctx, lc, p, L, k - 1), cur = feedfold_at(ctx, lc, p, L, k), next = feedfold_at(ctx, lc, p, L, k + 1);
  if (mode == 2) return fold2_byte(T.pair, prev, cur, next);
  return fold3_byte(T, feedfold_at(ctx, lc, p, L, k - 2), prev, cur, next, feedfold_at(ctx, lc, p, L, k + 2));
}

}  // namespace aha
