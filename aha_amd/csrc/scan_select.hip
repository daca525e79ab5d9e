// scan_select.hip -- the select path (aha_ac_select_batch*): per document the leftmost-longest, non-overlapping hits of the
// match's hit list.  The hit list of a range of whole documents lies in scratch (engine.cpp device_select); the
// passes here work on positions of the range's text, p in [0, nb):
//   ksl_longest     L[p] = max over the hits that start at p of (len << 32 | value): keys are distinct, so the longest hit of a
//                   start is unique and its value comes with it.  One 64-bit atomicMax per hit; the hit's document -- its
//                   offsets are relative to it -- by a binary search of the hit's index in the range's hit offsets.
//   ksl_marks       cover mask: the union of [p, p + len(L[p])), which is the union of all hits (every hit lies inside the
//                   longest one of its start); document-start mask: one bit per document that starts below nb.
//   ksl_walk        a run start is a p with L[p] != 0 that is a document start or whose predecessor is uncovered.  The greedy
//                   rule never jumps over an uncovered byte or a document start (a jump is a hit, which covers what it jumps
//                   over and lies inside one document) and lands on the first start behind one, so every run is walked alone, by
//                   one lane: p += len where L[p] != 0 (the start is taken: a bit of the select mask), p += 1 otherwise, until
//                   an uncovered byte, a document start or nb.
//   ksl_rank_*      the rank of the select mask: set bits per block of 64 words, their exclusive scan (the range's total
//                   behind it), and per document base + rank(its first byte) -- the documents' offsets into the selection.
//   ksl_emit        every set bit in position order as {s - doc_base, s - doc_base + len, value}, once the total fits.
// Vector atomics and plain C++ only.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "cover_span.hpp"
#include "image.hpp"
#include "post_common.hpp"

namespace aha {
namespace {

using post::grid_for;

constexpr int kSlScanThreads = 1024;

// hits[0, n_hits): the range's hits, document by document; hit_off[d] - hit_off[0]: the first hit of document d
__global__ __launch_bounds__(256) void ksl_longest(const int32_t *hits, uint64_t n_hits, const uint64_t *hit_off, const uint64_t *rel,
                                                   uint64_t nd, uint64_t nb, unsigned long long *L) {
  const uint64_t h0 = hit_off[0];
  for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < n_hits; i += (uint64_t)gridDim.x * 256) {
    const int32_t start = hits[i * 3], end = hits[i * 3 + 1];
    const uint32_t value = (uint32_t)hits[i * 3 + 2];
    if (start < 0 || end <= start) continue;
    const uint64_t d = owner_of(hit_off, nd, i, h0);  // (hit_off[0] - h0 = 0 <= i)
    const uint64_t p = rel[d] + (uint64_t)start;
    if (p + (uint64_t)(end - start) > min(rel[d + 1], nb)) continue;  // (never: a hit lies inside its document)
    atomicMax(L + p, (unsigned long long)(uint32_t)(end - start) << 32 | value);
  }
}

__global__ __launch_bounds__(256) void ksl_marks(const unsigned long long *L, uint64_t nb, const uint64_t *rel, uint64_t nd,
                                                 uint32_t *cover, uint32_t *doc_start) {
  const uint64_t tid = (uint64_t)blockIdx.x * 256 + threadIdx.x, nt = (uint64_t)gridDim.x * 256;
  for (uint64_t p = tid; p < nb; p += nt) {
    const unsigned long long v = L[p];
    if (v) cover_or_global(cover, p, min(p + (uint64_t)(v >> 32), nb));
  }
  for (uint64_t d = tid; d < nd; d += nt) {
    const uint64_t p = rel[d];
    if (p < nb) cover_or_word(doc_start + (p >> 5), 1u << (uint32_t)(p & 31));
  }
}

__global__ __launch_bounds__(256) void ksl_walk(const unsigned long long *L, uint64_t nb, const uint32_t *cover, const uint32_t *doc_start,
                                                uint32_t *select) {
  for (uint64_t p0 = (uint64_t)blockIdx.x * 256 + threadIdx.x; p0 < nb; p0 += (uint64_t)gridDim.x * 256) {
    if (!L[p0]) continue;
    if (p0 && !bit_at(doc_start, p0) && bit_at(cover, p0 - 1)) continue;  // inside a run: its walker comes by
    uint64_t p = p0;
    for (;;) {
      atomicOr(select + (p >> 5), 1u << (uint32_t)(p & 31));
      p += (uint64_t)(L[p] >> 32);
      // the next start of the run: covered bytes without a hit of their own are stepped over
      while (p < nb && !bit_at(doc_start, p) && bit_at(cover, p) && !L[p]) p++;
      if (p >= nb || bit_at(doc_start, p) || !bit_at(cover, p)) break;
    }
  }
}

// blk[b] = set bits of words [64 b, 64 b + 64): a wave per block
__global__ __launch_bounds__(256) void ksl_rank_blocks(const uint32_t *select, uint64_t n_words, uint64_t n_blk, unsigned long long *blk) {
  const int lane = threadIdx.x & 63;
  const uint64_t wave = ((uint64_t)blockIdx.x * 256 + threadIdx.x) >> 6, n_waves = (uint64_t)gridDim.x * 4;
  for (uint64_t b = wave; b < n_blk; b += n_waves) {
    const uint64_t w = b * kRankBlockWords + lane;
    const uint32_t c = wave_sum(w < n_words ? (uint32_t)__popc(select[w]) : 0u);
    if (lane == 0) blk[b] = c;
  }
}

// blk[0, n_blk] in place: the counts -> the set bits before every block, blk[n_blk] = the total.  One workgroup.
__global__ __launch_bounds__(kSlScanThreads) void ksl_rank_scan(unsigned long long *blk, uint64_t n_blk) {
  __shared__ unsigned long long s_sum[kSlScanThreads];
  const unsigned long long total = block_run_scan<kSlScanThreads>(
      n_blk, [&](uint64_t b) { return blk[b]; }, [&](uint64_t b, unsigned long long run) { blk[b] = run; }, s_sum);
  if (threadIdx.x == kSlScanThreads - 1) blk[n_blk] = total;
}

// out[d] = base + the set bits below position rel[d], for the range's documents d in [0, nd): a wave per document
__global__ __launch_bounds__(256) void ksl_rank_docs(const uint32_t *select, const unsigned long long *blk, const uint64_t *rel,
                                                     uint64_t nd, uint64_t base, unsigned long long *out) {
  const int lane = threadIdx.x & 63;
  const uint64_t wave = ((uint64_t)blockIdx.x * 256 + threadIdx.x) >> 6, n_waves = (uint64_t)gridDim.x * 4;
  for (uint64_t d = wave; d < nd; d += n_waves) {
    const uint64_t x = rel[d], b = x / (kRankBlockWords * 32), w = b * kRankBlockWords + lane, wx = x >> 5;
    uint32_t c = 0;
    if (w < wx)
      c = (uint32_t)__popc(select[w]);
    else if (w == wx && (x & 31))
      c = (uint32_t)__popc(select[w] & ~(~0u << (uint32_t)(x & 31)));
    c = wave_sum(c);
    if (lane == 0) out[d] = base + blk[b] + c;
  }
}

// the selection in position order
__global__ __launch_bounds__(256) void ksl_emit(const uint32_t *select, uint64_t n_words, uint64_t n_blk, const unsigned long long *blk,
                                                const unsigned long long *L, const uint64_t *rel, uint64_t nd, int32_t *out) {
  for_ranked_bits(select, n_words, n_blk, blk, [&](uint64_t w, uint32_t i, uint64_t at) {
    const uint64_t p = w * 32 + i;
    const unsigned long long v = L[p];
    const uint64_t s = p - rel[owner_of(rel, nd, p)];  // (rel[0] = 0)
    out[at * 3] = (int32_t)s;
    out[at * 3 + 1] = (int32_t)(s + (uint64_t)(v >> 32));
    out[at * 3 + 2] = (int32_t)(uint32_t)v;
  });
}

}  // namespace

uint64_t select_rank_blocks(uint64_t n_bytes) { return rank_blocks(n_bytes); }

void select_launch_longest(const void *hits, uint64_t n_hits, const uint64_t *hit_off, const uint64_t *rel, uint64_t nd, uint64_t nb,
                           uint64_t *L, uint32_t max_blocks, void *stream) {
  hipLaunchKernelGGL(ksl_longest, dim3(grid_for(n_hits, 256, max_blocks)), dim3(256), 0, (hipStream_t)stream, (const int32_t *)hits, n_hits,
                     hit_off, rel, nd, nb, reinterpret_cast<unsigned long long *>(L));
}

void select_launch_marks(const uint64_t *L, uint64_t nb, const uint64_t *rel, uint64_t nd, uint32_t *cover, uint32_t *doc_start,
                         uint32_t max_blocks, void *stream) {
  hipLaunchKernelGGL(ksl_marks, dim3(grid_for(std::max(nb, nd), 256, max_blocks)), dim3(256), 0, (hipStream_t)stream,
                     reinterpret_cast<const unsigned long long *>(L), nb, rel, nd, cover, doc_start);
}

void select_launch_walk(const uint64_t *L, uint64_t nb, const uint32_t *cover, const uint32_t *doc_start, uint32_t *select,
                        uint32_t max_blocks, void *stream) {
  hipLaunchKernelGGL(ksl_walk, dim3(grid_for(nb, 256, max_blocks)), dim3(256), 0, (hipStream_t)stream,
                     reinterpret_cast<const unsigned long long *>(L), nb, cover, doc_start, select);
}

void select_launch_rank(const uint32_t *select, uint64_t nb, uint64_t *blk, uint32_t max_blocks, void *stream) {
  const uint64_t n_words = (nb + 31) / 32, n_blk = rank_blocks(nb);
  unsigned long long *b = reinterpret_cast<unsigned long long *>(blk);
  hipLaunchKernelGGL(ksl_rank_blocks, dim3(grid_for(n_blk * 64, 256, max_blocks)), dim3(256), 0, (hipStream_t)stream, select, n_words, n_blk, b);
  hipLaunchKernelGGL(ksl_rank_scan, dim3(1), dim3(kSlScanThreads), 0, (hipStream_t)stream, b, n_blk);
}

void select_launch_rank_docs(const uint32_t *select, const uint64_t *blk, const uint64_t *rel, uint64_t nd, uint64_t base,
                             uint64_t *out, uint32_t max_blocks, void *stream) {
  hipLaunchKernelGGL(ksl_rank_docs, dim3(grid_for(nd * 64, 256, max_blocks)), dim3(256), 0, (hipStream_t)stream, select,
                     reinterpret_cast<const unsigned long long *>(blk), rel, nd, base, reinterpret_cast<unsigned long long *>(out));
}

void select_launch_emit(const uint32_t *select, uint64_t nb, const uint64_t *blk, const uint64_t *L, const uint64_t *rel, uint64_t nd,
                        void *out, uint32_t max_blocks, void *stream) {
  const uint64_t n_words = (nb + 31) / 32, n_blk = rank_blocks(nb);
  hipLaunchKernelGGL(ksl_emit, dim3(grid_for(n_blk * 64, 256, max_blocks)), dim3(256), 0, (hipStream_t)stream, select, n_words, n_blk,
                     reinterpret_cast<const unsigned long long *>(blk), reinterpret_cast<const unsigned long long *>(L), rel, nd,
                     (int32_t *)out);
}

}  // namespace aha
