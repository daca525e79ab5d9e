// scan_feedtokens.hip -- the feed token path (aha_feed_select_batch* with AHA_FEED_SELECT_TOKENS; DESIGN.md 4.10 "Feed tokens"):
// dictionary segmentation of sequences that arrive in pieces.
//
// A token call is a feed select call (scan_feedselect.hip) up to its rank: feed_select_settle leaves L, the select mask, the
// piece-start mask, eoff, n0 and cend over the call's NE extended positions.  Beside the select cursor c the feed keeps a token
// cursor t <= c per sequence: everything in front of t has been reported as tokens, and [t, c) is the front part of a gap token
// that is still open -- in character mode a character whose next lead byte has not been seen.  A call finds (c0, t0), leaves
// (c1, t1) and reports the tokens of T[t0 .. c1) as one document under the hits it settles, without the last where nothing yet
// says that it ends at c1 (feedtok_edge.hpp).  Over the extended positions, piece by piece:
//   kft_bounds   per piece c0 and c1 as extended positions, t0, and whether c0 stands for a document's start (t0 == c0)
//   ktk_spans    (scan_tokens.hip, shared) S: the bytes inside a selected hit
//   kft_starts   T: where a token starts inside [c0, c1) of every piece, by the rule of token_rule.hpp, a lane per mask word.  The
//                continuation bits of an extended position come from the sequence's context bank (the W' positions in front of
//                the piece, read singly) or from the caller's piece: the 32 bytes of a word by the three 16-byte loads, aligned
//                to the ADDRESS, that hold them.  A load that would reach outside [text, text + n_bytes) is replaced by single
//                reads of the wanted bytes.  With AHA_FEED_SELECT_GAP_RUNS no text is read.
//   (rank)       select_launch_rank / select_launch_rank_docs over T: the starts in front of every block and every piece
//   kft_edge     per piece: is c1 a certain boundary, does the carried token close, t1, the token count, the open-length check
//   kft_offsets  one block: the pieces' offsets into the tokens, the total behind them (one read-back with the verdict)
//   kft_emit     over the ranked T, the lanes strided over the ranks (for_ranked_slots, as ktk_emit): a start writes its own start
//                and value and the end of the token in front; a piece's last reported token ends at c1; the carried token starts
//                at t0 - n0, written by a lane per piece.  Every field is written exactly once: no atomics.
//   kft_commit   behind kfd_commit and kfs_commit, after success only: the token state and piece_hold = n1 - t1
// Nothing here is per token but the output.  Vector loads, stores and atomics and plain C++ only.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "feed.hpp"
#include "feedtok_edge.hpp"
#include "post_common.hpp"
#include "token_rule.hpp"

namespace aha {
namespace {

using post::grid_for;

constexpr int kFtThreads = 256;
constexpr int kFtScanThreads = 1024;

__device__ __forceinline__ const uint8_t *ft_ctx_row(const FeedArgs &F, uint32_t id) {
  return F.ctx + ((uint64_t)F.seqs[id].bank * F.n_seqs + id) * F.W;
}

__global__ void __launch_bounds__(kFtThreads) kft_bounds(FeedArgs F, FeedSelArgs S, FeedTokArgs K) {
  for (uint64_t d = blockIdx.x * (uint64_t)kFtThreads + threadIdx.x; d < F.D; d += (uint64_t)gridDim.x * kFtThreads) {
    const uint32_t id = F.ids[d];
    const uint64_t n0 = S.n0[d], wb = min((uint64_t)F.W, n0), E = S.eoff[d + 1] - S.eoff[d], n1 = n0 - wb + E;
    // (c0 lies in [n0 - wb, n0] and t0 <= c0 on a sequence fed through token calls alone, and no other gets here; the clamps
    // keep every index inside the extended positions whatever the state holds)
    const uint64_t c0 = max(min((uint64_t)S.sseq[id].cursor, n0), n0 - wb);
    const uint64_t t0 = n0 ? min((uint64_t)K.tseq[id].t, c0) : 0;
    const uint64_t c1 = min(feedsel_cursor(c0, n0, wb, S.cend[d], n1, F.W, S.final), n1);
    FeedTokPiece pc;
    pc.t0 = t0;
    pc.t1 = t0;
    pc.c0 = (uint32_t)(c0 - (n0 - wb));
    pc.c1 = (uint32_t)(c1 - (n0 - wb));
    pc.flags = t0 < c0 ? kFeedTokCarried : 0u;
    pc.count = 0;
    K.piece[d] = pc;
  }
}

// the continuation bits of corpus bytes [pos, pos + len), len <= 32, as bits [0, len): the three aligned 16-byte pieces that
// hold them, each by one load where it lies inside [text, text + n_bytes), else its wanted bytes singly
__device__ __forceinline__ uint32_t ft_cont_span(const uint8_t *text, uint64_t n_bytes, uint64_t pos, uint32_t len) {
  const uint32_t k = (uint32_t)(reinterpret_cast<uintptr_t>(text + pos) & 15);
  const int64_t q0 = (int64_t)pos - (int64_t)k;  // the corpus position of the first aligned piece (below 0: in front of the text)
  uint64_t bits = 0;
#pragma unroll
  for (uint32_t c = 0; c < 3; c++) {
    const int64_t q = q0 + 16 * (int64_t)c;
    if (q >= (int64_t)(pos + len)) break;
    uint32_t b16 = 0;
    if (q >= 0 && (uint64_t)q + 16 <= n_bytes) {
      const uint4 v = *reinterpret_cast<const uint4 *>(text + q);
      b16 = token_cont4(v.x) | token_cont4(v.y) << 4 | token_cont4(v.z) << 8 | token_cont4(v.w) << 12;
    } else {
      for (uint32_t j = 0; j < 16; j++) {
        const int64_t a = q + (int64_t)j;
        if (a >= (int64_t)pos && a < (int64_t)(pos + len) && (text[a] & 0xC0u) == 0x80u) b16 |= 1u << j;
      }
    }
    bits |= (uint64_t)b16 << (16 * c);
  }
  const uint32_t r = (uint32_t)(bits >> k);
  return len >= 32 ? r : r & ~(~0u << len);
}

// the bits of [a, b) inside the word that starts at p0 (p0 <= a <= b <= p0 + 32)
__device__ __forceinline__ uint32_t ft_span_bits(uint64_t p0, uint64_t a, uint64_t b) {
  if (a >= b) return 0u;
  const uint32_t n = (uint32_t)(b - a), m = n >= 32 ? ~0u : ~(~0u << n);
  return m << (uint32_t)(a - p0);
}

__global__ void __launch_bounds__(kFtThreads) kft_starts(FeedArgs F, FeedSelArgs S, FeedTokArgs K) {
  const uint64_t n_words = (S.NE + 31) / 32;
  for (uint64_t w = blockIdx.x * (uint64_t)kFtThreads + threadIdx.x; w < n_words; w += (uint64_t)gridDim.x * kFtThreads) {
    const uint64_t p0 = w * 32, p1 = min(p0 + 32, S.NE);
    uint32_t valid = 0, doc = 0, cont = 0;
    uint64_t d = owner_of(S.eoff, F.D, p0);
    for (uint64_t p = p0; p < p1 && d < F.D; d++) {
      const uint64_t e0 = S.eoff[d], e1 = S.eoff[d + 1];
      if (e1 <= p) continue;  // (a piece without extended positions)
      const FeedTokPiece pc = K.piece[d];
      const uint64_t a = max(p, e0 + pc.c0), b = min(p1, e0 + pc.c1);  // the part of [c0, c1) in this word
      if (a < b) {
        valid |= ft_span_bits(p0, a, b);
        if (a == e0 + pc.c0 && !(pc.flags & kFeedTokCarried)) doc |= 1u << (uint32_t)(a - p0);
        if (!K.gap_runs) {
          const uint64_t wb = min((uint64_t)F.W, S.n0[d]), body = e0 + wb;  // the piece's own first byte
          if (a < body) {
            const uint8_t *row = ft_ctx_row(F, F.ids[d]);
            for (uint64_t x = a; x < min(b, body); x++)
              if ((row[x - e0] & 0xC0u) == 0x80u) cont |= 1u << (uint32_t)(x - p0);
          }
          if (b > body) {
            const uint64_t x = max(a, body);
            cont |= ft_cont_span(F.text, F.n_bytes, F.off[d] + (x - body), (uint32_t)(b - x)) << (uint32_t)(x - p0);
          }
        }
      }
      p = min(p1, e1);
    }
    const uint32_t sel = S.select[w], in = K.inside[w], first = S.start[w];
    uint32_t t = token_starts(sel, in, doc, w ? K.inside[w - 1] >> 31 : 0u, cont, K.gap_runs != 0, valid);
    // a piece's first extended position has no predecessor: the position in front belongs to another piece
    t &= ~first | sel | (~in & (doc | (K.gap_runs ? 0u : ~cont)));
    K.starts[w] = t;
  }
}

__global__ void __launch_bounds__(kFtThreads) kft_edge(FeedArgs F, FeedSelArgs S, FeedTokArgs K) {
  for (uint64_t d = blockIdx.x * (uint64_t)kFtThreads + threadIdx.x; d < F.D; d += (uint64_t)gridDim.x * kFtThreads) {
    const uint32_t id = F.ids[d];
    FeedTokPiece pc = K.piece[d];
    const uint64_t e0 = S.eoff[d], E = S.eoff[d + 1] - e0, n0 = S.n0[d], wb = min((uint64_t)F.W, n0), base = n0 - wb;
    const uint64_t n_starts = K.raw[d + 1] - K.raw[d];
    uint64_t last = 0;
    if (n_starts) {  // the last start in [c0, c1): word by word from the back
      const uint64_t lo = e0 + pc.c0, hi = e0 + pc.c1;
      for (uint64_t w = (hi - 1) >> 5;; w--) {
        const uint64_t p0 = w * 32;
        const uint32_t bits = K.starts[w] & ft_span_bits(p0, max(lo, p0), min(hi, p0 + 32));
        if (bits) {
          last = p0 + (31u - (uint32_t)__clz(bits));
          break;
        }
        if (p0 <= lo) break;  // (never: n_starts of them lie in the range)
      }
    }
    const bool hit_end = S.cend[d] && S.cend[d] == pc.c1;
    bool cont = false;
    if (!S.final && !K.gap_runs && !hit_end && pc.c1 < E) {
      const uint8_t b = pc.c1 < wb ? ft_ctx_row(F, id)[pc.c1] : F.text[F.off[d] + (pc.c1 - wb)];
      cont = (b & 0xC0u) == 0x80u;
    }
    const FeedTokEdge e = feedtok_edge(pc.t0, base + pc.c0, base + pc.c1, base + E, n_starts, base + (last - e0), hit_end, cont,
                                       S.final != 0, K.gap_runs != 0, K.bound);
    pc.t1 = e.t1;
    pc.flags = (e.carried ? kFeedTokCarried : 0u) | (e.open ? kFeedTokOpen : 0u);
    pc.count = (uint32_t)e.count;
    K.piece[d] = pc;
    if (e.too_long) atomicOr(K.verdict, 1u);
  }
}

// one block: pto[0 .. D] = the exclusive scan of the pieces' token counts
__global__ void __launch_bounds__(kFtScanThreads) kft_offsets(FeedArgs F, FeedTokArgs K) {
  __shared__ uint64_t s[kFtScanThreads];
  const uint64_t total = block_run_scan<kFtScanThreads>(
      F.D, [&](uint64_t d) { return (uint64_t)K.piece[d].count; }, [&](uint64_t d, uint64_t run) { K.pto[d] = run; }, s);
  if (threadIdx.x == kFtScanThreads - 1) {
    K.pto[F.D] = total;
    *K.total = total;
  }
}

__global__ void __launch_bounds__(kFtThreads) kft_emit(FeedArgs F, FeedSelArgs S, FeedTokArgs K) {
  __shared__ uint32_t s_words[(kFtThreads / 64) * 2 * kRankBlockWords];
  for_ranked_slots<kFtThreads>(K.starts, (S.NE + 31) / 32, rank_blocks(S.NE), K.blk, s_words, [&](uint64_t w, uint32_t i, uint64_t at) {
    const uint64_t p = w * 32 + i;
    const uint64_t d = owner_of(S.eoff, F.D, p);
    const FeedTokPiece pc = K.piece[d];
    const uint64_t e0 = S.eoff[d], wb = min((uint64_t)F.W, S.n0[d]);
    const uint64_t k = at - K.raw[d], n_starts = K.raw[d + 1] - K.raw[d];  // the k-th start of its piece
    const uint32_t carried = pc.flags & kFeedTokCarried ? 1u : 0u;
    const uint64_t slot = K.pto[d] + carried + k;
    const int32_t rel = (int32_t)((int64_t)(p - e0) - (int64_t)wb);
    const bool is_last = k + 1 == n_starts;
    if (!(is_last && (pc.flags & kFeedTokOpen))) {
      K.out[slot * 3] = rel;
      K.out[slot * 3 + 2] = bit_at(S.select, p) ? (int32_t)(uint32_t)S.L[p] : -1;
      if (is_last) K.out[slot * 3 + 1] = (int32_t)((int64_t)pc.c1 - (int64_t)wb);
    }
    if (k || carried) K.out[(slot - 1) * 3 + 1] = rel;  // the token in front ends here
  });
  // the carried tokens: a lane per piece
  for (uint64_t d = blockIdx.x * (uint64_t)kFtThreads + threadIdx.x; d < F.D; d += (uint64_t)gridDim.x * kFtThreads) {
    const FeedTokPiece pc = K.piece[d];
    if (!(pc.flags & kFeedTokCarried)) continue;
    const uint64_t n_starts = K.raw[d + 1] - K.raw[d];
    if (!n_starts && (pc.flags & kFeedTokOpen)) continue;  // it stays open
    const uint64_t slot = K.pto[d], wb = min((uint64_t)F.W, S.n0[d]);
    K.out[slot * 3] = (int32_t)((int64_t)pc.t0 - (int64_t)S.n0[d]);
    K.out[slot * 3 + 2] = -1;
    if (!n_starts) K.out[slot * 3 + 1] = (int32_t)((int64_t)pc.c1 - (int64_t)wb);
  }
}

// behind kfs_commit, which leaves the select state and, under FINAL, a sequence of length 0
__global__ void __launch_bounds__(kFtThreads) kft_commit(FeedArgs F, FeedSelArgs S, FeedTokArgs K) {
  for (uint64_t d = blockIdx.x * (uint64_t)kFtThreads + threadIdx.x; d < F.D; d += (uint64_t)gridDim.x * kFtThreads) {
    const uint64_t n0 = S.n0[d], wb = min((uint64_t)F.W, n0), n1 = n0 - wb + (S.eoff[d + 1] - S.eoff[d]);
    FeedTokSeq ns;
    ns.seen = S.final ? 0 : n1;
    ns.t = S.final ? 0 : K.piece[d].t1;
    K.tseq[F.ids[d]] = ns;
    if (K.hold) K.hold[d] = S.final ? 0u : (uint32_t)(n1 - ns.t);
  }
}

}  // namespace

void feedtok_launch_bounds(const FeedArgs &F, const FeedSelArgs &S, const FeedTokArgs &K, uint32_t max_blocks, void *stream) {
  hipLaunchKernelGGL(kft_bounds, dim3(grid_for(F.D, kFtThreads, max_blocks)), dim3(kFtThreads), 0, (hipStream_t)stream, F, S, K);
}

void feedtok_launch_starts(const FeedArgs &F, const FeedSelArgs &S, const FeedTokArgs &K, uint32_t max_blocks, void *stream) {
  hipLaunchKernelGGL(kft_starts, dim3(grid_for((S.NE + 31) / 32, kFtThreads, max_blocks)), dim3(kFtThreads), 0, (hipStream_t)stream, F, S,
                     K);
}

void feedtok_launch_edge(const FeedArgs &F, const FeedSelArgs &S, const FeedTokArgs &K, uint32_t max_blocks, void *stream) {
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(kft_edge, dim3(grid_for(F.D, kFtThreads, max_blocks)), dim3(kFtThreads), 0, s, F, S, K);
  hipLaunchKernelGGL(kft_offsets, dim3(1), dim3(kFtScanThreads), 0, s, F, K);
}

void feedtok_launch_emit(const FeedArgs &F, const FeedSelArgs &S, const FeedTokArgs &K, uint32_t max_blocks, void *stream) {
  const uint64_t units = std::max<uint64_t>(rank_blocks(S.NE) * 64, F.D);
  hipLaunchKernelGGL(kft_emit, dim3(grid_for(units, kFtThreads, max_blocks)), dim3(kFtThreads), 0, (hipStream_t)stream, F, S, K);
}

void feedtok_launch_commit(const FeedArgs &F, const FeedSelArgs &S, const FeedTokArgs &K, uint32_t max_blocks, void *stream) {
  hipLaunchKernelGGL(kft_commit, dim3(grid_for(F.D, kFtThreads, max_blocks)), dim3(kFtThreads), 0, (hipStream_t)stream, F, S, K);
}
}  // namespace aha
