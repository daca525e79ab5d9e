// scan_greprule.hip -- rule grep (aha_ac_grep_batch* with AHA_GREP_RULE; DESIGN.md 4.16 "Rule grep"): which documents stay is a rule
// over their class counts (the D x C table of aha_ac_class_counts_batch*), grep's tail (scan_grep.hip) takes it from there.
//   kgq_keep    a lane per document, a wave per 64 documents, a workgroup per 256.  A lane per row would read at a stride of 4 C
//               bytes: up to 32 classes several rows share a cache line and every term asks for it again, beyond that every
//               load instruction touches 64 lines for 64 words.  So the wave stages the columns its terms name through LDS, a
//               chunk of kRuleChunkClasses columns at a time (all C of them where C is at most that: 64 x C contiguous words):
//               lane k loads word k of the wave's 64 x W block, whole lines are used, and the LDS rows are W | 1 words apart,
//               so the 32 lanes of a half-wave write and read 32 different banks.  A chunk no term names is never read.
//               The rule is a kernel argument (1 KiB): the terms sorted by chunk, their groups renumbered 0 .. 63; a lane
//               keeps one bit per group, "a term of it failed", and passes when some group of the rule has none: OR over
//               groups, AND inside one.  keep: whole words by wave ballot, no atomics, no memset.
//   kgq_edges   a lane per mask word: dropped = ~keep inside D; S = dropped and the predecessor is not (a run starts), T = dropped
//               and the successor is not (a run ends); document 0 and document D - 1 are edges; the bits from D on are 0.
// Vector loads and stores and plain C++ only.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "image.hpp"
#include "post_common.hpp"

namespace aha {
namespace {

using post::grid_for;

struct RuleArg {
  aha_rule_term t[kRuleMaxTerms];  // sorted by class_id / kRuleChunkClasses; group: the dense index of the caller's group
};
static_assert(sizeof(RuleArg) == 1024, "the rule travels as a kernel argument of 1 KiB");

constexpr uint32_t kGqRowStride = kRuleChunkClasses | 1u;  // the widest staged row
constexpr uint32_t kGqWaveWords = 64 * kGqRowStride;       // LDS words of one wave: 64 rows

// one term over a document of `len` bytes with `cnt` hits of the term's class
__device__ __forceinline__ bool gq_term(const aha_rule_term &t, uint32_t cnt, uint64_t len) {
  const uint64_t lhs = t.den_bytes ? (uint64_t)cnt * t.den_bytes : cnt;
  const uint64_t rhs = t.den_bytes ? (uint64_t)t.num * len : t.num;
  return t.op == AHA_RULE_LT ? lhs < rhs : lhs >= rhs;
}

// groups: bit g = the rule has a group g
__global__ __launch_bounds__(256) void kgq_keep(const uint32_t *rows, uint32_t C, const uint64_t *doc_off, uint64_t n_docs, RuleArg R,
                                                uint32_t n_terms, unsigned long long groups, uint32_t invert, uint32_t *keep) {
  __shared__ uint32_t lds[4 * kGqWaveWords];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  uint32_t *mine = lds + wv * kGqWaveWords;
  const uint64_t n_words = (n_docs + 31) / 32;
  for (uint64_t b0 = (uint64_t)blockIdx.x * 256; b0 < n_docs; b0 += (uint64_t)gridDim.x * 256) {  // (the same trips in every wave)
    const uint64_t d0 = b0 + (uint64_t)wv * 64, d = d0 + lane;
    const uint32_t nd = d0 < n_docs ? (uint32_t)std::min<uint64_t>(64, n_docs - d0) : 0u;
    const uint64_t len = d < n_docs ? doc_off[d + 1] - doc_off[d] : 0;
    unsigned long long failed = 0;
    uint32_t i = 0;
    while (i < n_terms) {  // (uniform: the terms come from the kernel's arguments) one chunk of columns per trip
      const uint32_t c0 = R.t[i].class_id / kRuleChunkClasses * kRuleChunkClasses;
      const uint32_t W = std::min(kRuleChunkClasses, C - c0), Wp = W | 1u;
      const bool pow2 = (W & (W - 1)) == 0;
      const uint32_t sh = (uint32_t)__ffs(W) - 1u;
      const uint32_t *src = rows + d0 * C + c0;  // (nothing is read where nd == 0; else rows [d0, d0 + nd), columns [c0, c0 + W))
      for (uint32_t k = lane; k < nd * W; k += 64) {
        const uint32_t r = pow2 ? k >> sh : k / W, c = k - r * W;
        mine[r * Wp + c] = src[(uint64_t)r * C + c];
      }
      __syncthreads();
      for (; i < n_terms && R.t[i].class_id / kRuleChunkClasses * kRuleChunkClasses == c0; i++) {
        const uint32_t cnt = mine[lane * Wp + (R.t[i].class_id - c0)];  // (a lane beyond nd reads a stale word: not used)
        if (!gq_term(R.t[i], cnt, len)) failed |= 1ull << R.t[i].group;
      }
      __syncthreads();  // (the next chunk overwrites the rows)
    }
    const bool k = d < n_docs && ((~failed & groups) != 0) != (invert != 0);
    const unsigned long long bk = __ballot(k);
    const uint64_t w = d0 / 32 + lane;
    if (lane < 2 && w < n_words) keep[w] = (uint32_t)(bk >> (32 * lane));
  }
}

__global__ __launch_bounds__(256) void kgq_edges(const uint32_t *keep, uint64_t n_docs, uint32_t *S, uint32_t *T) {
  const uint64_t n_words = (n_docs + 31) / 32;
  const uint32_t tail = (uint32_t)(n_docs & 31);
  for (uint64_t w = (uint64_t)blockIdx.x * 256 + threadIdx.x; w < n_words; w += (uint64_t)gridDim.x * 256) {
    const uint32_t valid = (w + 1 == n_words && tail) ? (1u << tail) - 1u : 0xFFFFFFFFu;
    const uint32_t dropped = ~keep[w] & valid;
    const uint32_t before = w ? ~keep[w - 1] >> 31 : 0u;                   // the last document of the word in front is dropped
    const uint32_t behind = w + 1 < n_words ? ~keep[w + 1] & 1u : 0u;      // the first document of the next word is (it exists)
    S[w] = dropped & ~(dropped << 1 | before);
    T[w] = dropped & ~(dropped >> 1 | behind << 31);
  }
}

}  // namespace

void greprule_launch_keep(const uint32_t *rows, uint32_t n_classes, const uint64_t *doc_off, uint64_t n_docs,
                          const aha_rule_term *terms, uint32_t n_terms, bool invert, uint32_t *keep, uint32_t max_blocks, void *stream) {
  if (!n_docs) return;
  n_terms = std::min(n_terms, kRuleMaxTerms);
  RuleArg R{};
  unsigned long long groups = 0;
  uint32_t n_groups = 0;
  uint16_t seen[kRuleMaxTerms];
  for (uint32_t i = 0; i < n_terms; i++) {  // the caller's group ids, arbitrary, as 0 .. 63 in the order they appear
    uint32_t g = 0;
    while (g < n_groups && seen[g] != terms[i].group) g++;
    if (g == n_groups) seen[n_groups++] = terms[i].group;
    R.t[i] = terms[i];
    R.t[i].group = (uint16_t)g;
    groups |= 1ull << g;
  }
  std::stable_sort(R.t, R.t + n_terms, [](const aha_rule_term &a, const aha_rule_term &b) {
    return a.class_id / kRuleChunkClasses < b.class_id / kRuleChunkClasses;
  });
  hipLaunchKernelGGL(kgq_keep, dim3(grid_for(n_docs, 256, max_blocks)), dim3(256), 0, (hipStream_t)stream, rows, n_classes, doc_off, n_docs,
                     R, n_terms, groups, invert ? 1u : 0u, keep);
}

void greprule_launch_edges(const uint32_t *keep, uint64_t n_docs, uint32_t *S, uint32_t *T, uint32_t max_blocks, void *stream) {
  if (!n_docs) return;
  hipLaunchKernelGGL(kgq_edges, dim3(grid_for((n_docs + 31) / 32, 256, max_blocks)), dim3(256), 0, (hipStream_t)stream, keep, n_docs, S, T);
}

}  // namespace aha
