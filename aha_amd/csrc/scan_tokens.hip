// scan_tokens.hip -- the token path (aha_ac_select_batch* with AHA_SELECT_TOKENS; DESIGN.md 4.14 "Tokens"): every document as
// a gap-free sequence of tokens, the selected hits and between them single characters (or, with AHA_SELECT_GAP_RUNS, whole gaps).
// The passes work on the positions of a range's text, p in [0, nb), after scan_select.hip has left L, the document-start mask
// and the select mask of the range:
//   ktk_spans    S: every set bit p of the select mask ORs [p, p + len(L[p])) (cover_span.hpp) -- the bytes inside a selected
//                hit, not the cover mask, which is the union of all hits.  A lane per mask word.
//   ktk_starts   T: where a token starts, word by word by the rule of token_rule.hpp.  A lane owns one mask word and its 32
//                text bytes as two aligned 16-byte loads.  The text may start anywhere: the loads are aligned to the ADDRESS,
//                so the words they give are `head` bits behind the mask's words -- a mask word is the funnel of two
//                neighbouring lanes' words (token_rule.hpp, as kgr_ends of scan_grep.hip).  The head bytes and the bytes
//                behind the last whole piece are read one by one: nothing outside [text, text + nb) is touched.
//   (rank)       select_launch_rank / select_launch_rank_docs over T: the tokens in front of every block and every document.
//   ktk_emit     over the ranked T, the lanes strided over the ranks (for_ranked_slots: T is dense, up to a token per byte, and
//                a lane per mask word would scatter every store of the wave over 64 places): a set bit p of rank r in
//                document d writes out[r].start and out[r].value -- the low word of
//                L[p] where p is a selected hit's start, else -1 -- and, where p > 0, out[r - 1].end: the token in front ends
//                where this one starts, at its document's end where p starts a document.  The range's last token ends with the
//                range.  Every field is written exactly once: no atomics.
// The feed form (tokens of sequences in pieces) is scan_feedtokens.hip, which shares ktk_spans.
// Out of scope: character offsets, groups, tokens of match_longest, id remapping (include/aha_hip.h).
// Vector loads, stores and atomics and plain C++ only.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "cover_span.hpp"
#include "image.hpp"
#include "post_common.hpp"
#include "token_rule.hpp"

namespace aha {
namespace {

using post::grid_for;

__global__ __launch_bounds__(256) void ktk_spans(const unsigned long long *L, uint64_t nb, const uint32_t *select, uint64_t n_words,
                                                 uint32_t *S) {
  for (uint64_t w = (uint64_t)blockIdx.x * 256 + threadIdx.x; w < n_words; w += (uint64_t)gridDim.x * 256) {
    uint32_t bits = select[w];
    while (bits) {
      const uint64_t p = w * 32 + ((uint32_t)__ffs(bits) - 1u);
      bits &= bits - 1u;
      cover_or_global(S, p, min(p + (uint64_t)(L[p] >> 32), nb));
    }
  }
}

// T[0, n_words): the token starts, whole words, the bits from nb on 0.  head < 16: the bytes in front of the first 16-byte
// aligned address (all of the text where it is shorter)
__global__ __launch_bounds__(256) void ktk_starts(const uint8_t *corpus, uint64_t nb, uint32_t head, const uint32_t *select,
                                                  const uint32_t *S, const uint32_t *doc_start, bool gap_runs, uint64_t n_words,
                                                  uint32_t *T) {
  const int lane = threadIdx.x & 63;
  const uint8_t *text = corpus + head;
  const uint64_t na = nb - head;
  const uint64_t wave = ((uint64_t)blockIdx.x * 256 + threadIdx.x) >> 6, n_waves = (uint64_t)gridDim.x * 4;
  for (uint64_t w0 = wave * 64; w0 < n_words; w0 += n_waves * 64) {  // (the same trips in every lane of a wave)
    const uint64_t w = w0 + lane;
    uint32_t cur = 0, prev = 0;
    if (!gap_runs) {  // (uniform: the text is not read where no character is cut out)
      cur = w < n_words ? token_cont32(text, w, na) : 0u;
      prev = __shfl_up(cur, 1, 64);
      if (lane == 0) prev = w0 ? token_cont32(text, w0 - 1, na) : token_cont_head(corpus, head);
    }
    if (w < n_words)
      T[w] = token_starts(select[w], S[w], doc_start[w], w ? S[w - 1] >> 31 : 0u, token_funnel(prev, cur, head), gap_runs,
                          token_valid(w, nb));
  }
}

// the tokens in position order; total = blk[n_blk] of them, at least one (nb > 0: position 0 starts a document)
__global__ __launch_bounds__(256) void ktk_emit(const uint32_t *T, uint64_t n_words, uint64_t n_blk, const unsigned long long *blk,
                                                const uint32_t *select, const uint32_t *doc_start, const unsigned long long *L,
                                                const uint64_t *rel, uint64_t nd, uint64_t nb, int32_t *out) {
  __shared__ uint32_t s_words[4 * 2 * kRankBlockWords];
  for_ranked_slots(T, n_words, n_blk, blk, s_words, [&](uint64_t w, uint32_t i, uint64_t at) {
    const uint64_t p = w * 32 + i;
    const uint64_t d = owner_of(rel, nd, p);  // (rel[0] = 0)
    out[at * 3] = (int32_t)(p - rel[d]);
    out[at * 3 + 2] = bit_at(select, p) ? (int32_t)(uint32_t)L[p] : -1;
    if (p) {  // (position 0 is a token start, so at >= 1 here) the token in front ends here, in the document of p - 1
      const uint64_t dp = bit_at(doc_start, p) ? owner_of(rel, nd, p - 1) : d;
      out[(at - 1) * 3 + 1] = (int32_t)(p - rel[dp]);
    }
  });
  if (blockIdx.x == 0 && threadIdx.x == 0) out[(blk[n_blk] - 1) * 3 + 1] = (int32_t)(nb - rel[owner_of(rel, nd, nb - 1)]);
}

}  // namespace

void tokens_launch_spans(const uint64_t *L, uint64_t nb, const uint32_t *select, uint32_t *S, uint32_t max_blocks, void *stream) {
  const uint64_t n_words = (nb + 31) / 32;
  hipLaunchKernelGGL(ktk_spans, dim3(grid_for(n_words, 256, max_blocks)), dim3(256), 0, (hipStream_t)stream,
                     reinterpret_cast<const unsigned long long *>(L), nb, select, n_words, S);
}

void tokens_launch_starts(const uint8_t *text, uint64_t nb, const uint32_t *select, const uint32_t *S, const uint32_t *doc_start,
                          bool gap_runs, uint32_t *T, uint32_t max_blocks, void *stream) {
  const uint64_t n_words = (nb + 31) / 32;
  const uint32_t head = (uint32_t)std::min<uint64_t>(nb, (16 - reinterpret_cast<uintptr_t>(text) % 16) % 16);
  hipLaunchKernelGGL(ktk_starts, dim3(grid_for(n_words, 256, max_blocks)), dim3(256), 0, (hipStream_t)stream, text, nb, head, select, S,
                     doc_start, gap_runs, n_words, T);
}

void tokens_launch_emit(const uint32_t *T, uint64_t nb, const uint64_t *blk, const uint32_t *select, const uint32_t *doc_start,
                        const uint64_t *L, const uint64_t *rel, uint64_t nd, void *out, uint32_t max_blocks, void *stream) {
  const uint64_t n_words = (nb + 31) / 32, n_blk = rank_blocks(nb);
  hipLaunchKernelGGL(ktk_emit, dim3(grid_for(n_blk * 64, 256, max_blocks)), dim3(256), 0, (hipStream_t)stream, T, n_words, n_blk,
                     reinterpret_cast<const unsigned long long *>(blk), select, doc_start,
                     reinterpret_cast<const unsigned long long *>(L), rel, nd, nb, (int32_t *)out);
}

}  // namespace aha
