// scan_excerpt.hip -- the excerpts path (aha_ac_grep_batch* with AHA_GREP_CONTEXT; DESIGN.md 4.16 "Excerpts"): from the
// byte-level cover mask M of a batch (the count call's cover mode, scan_cover.hip) and its document boundaries to the gaps
// between the excerpts, as "deleted hits" for replace's scan and copy.  No pass looks at a hit: a covered run of a document,
// widened by the context, clipped and snapped (excerpt_window.hpp), gives the union of its hits' windows, because the snaps are
// monotone.  The ranked masks here are walked by post_common.hpp's for_ranked_bits.
//   kex_edges      two masks over bytes from M alone, a lane per mask word, the neighbouring words funnelled across the wave:
//                  S: bit p is covered and p - 1 is not (or p = 0); T: bit p is covered and p + 1 is not (or p + 1 = N).
//                  Whole words are written; the bits of M from N on are not trusted.
//   kex_doc_edges  a lane per inner document boundary q: where q - 1 and q are both covered a run ends and one starts there,
//                  bit q - 1 of T and bit q of S (an OR of a bit that only ever goes up: no order can show).
//   kex_windows    over the ranked S and T: the j-th bits delimit run j.  S's bit gives the run's document (owner_of over
//                  doc_offsets) and w0[j], T's bit gives w1[j]: at most three text bytes each.
//   kex_merge      a lane per run, two masks over runs by wave ballot: first[j] = j is the first run, or of another document
//                  than j - 1, or w0[j] > w1[j - 1]; last[j] = the same test seen from j + 1.  The r-th bits of the two
//                  delimit excerpt r = [w0[first_r], w1[last_r]).
//   kex_gaps       over the ranked first and last masks: the R + 1 stretches outside the excerpts, A[0] = 0, end[r] = p_r,
//                  A[r + 1] = q_r, end[R] = N.
//   kex_delta      delta[j] = -(end[j] - A[j]), the stretch's synthesized selection row and the one-entry table (the empty
//                  replacement): what scan_replace.hip's scan and copy take, as kgr_delta does for grep.
//   kex_emit       once the call is known to fit: starts[r] = A[r] + shift[r] - shift[r + 1] (= p_r), out_offsets[r] = A[r] +
//                  shift[r] for r in [0, R], the last being the total.
// Every kernel strides over its work; positions and ranks are 64-bit.  Scratch beyond the count call's: N / 8 bytes for M,
// 2 N / 8 for S and T, 16 bytes per 2048 text bytes of block ranks, and per run 24 bytes of windows, 2 bits of masks, their
// block ranks and (per excerpt, at most one per run) 28 bytes of gap rows and the scan's block sums.
// Vector loads, stores and atomics and plain C++ only.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "excerpt_window.hpp"
#include "image.hpp"
#include "post_common.hpp"

namespace aha {
namespace {

using post::grid_for;

__global__ __launch_bounds__(256) void kex_edges(const uint32_t *M, uint64_t n_words, uint64_t n_bytes, uint32_t *S, uint32_t *T) {
  const int lane = threadIdx.x & 63;
  const uint32_t tail = (uint32_t)(n_bytes & 31);
  const uint64_t wave = ((uint64_t)blockIdx.x * 256 + threadIdx.x) >> 6, n_waves = (uint64_t)gridDim.x * 4;
  for (uint64_t w0 = wave * 64; w0 < n_words; w0 += n_waves * 64) {  // (the same trips in every lane of a wave)
    const uint64_t w = w0 + lane;
    uint32_t cur = w < n_words ? M[w] : 0u;
    if (tail && w + 1 == n_words) cur &= (1u << tail) - 1u;
    uint32_t prev = __shfl_up(cur, 1, 64), next = __shfl_down(cur, 1, 64);
    if (lane == 0) prev = w0 ? M[w0 - 1] : 0u;                   // (a word in front of the last: all its bits are text)
    if (lane == 63) next = w0 + 64 < n_words ? M[w0 + 64] : 0u;  // (its bit 0 is text: the word exists)
    if (w < n_words) {
      S[w] = cur & ~(cur << 1 | prev >> 31);
      T[w] = cur & ~(cur >> 1 | next << 31);
    }
  }
}

__global__ __launch_bounds__(256) void kex_doc_edges(const uint32_t *M, const uint64_t *doc_off, uint64_t n_docs, uint64_t n_bytes,
                                                     uint32_t *S, uint32_t *T) {
  for (uint64_t d = (uint64_t)blockIdx.x * 256 + threadIdx.x + 1; d < n_docs; d += (uint64_t)gridDim.x * 256) {
    const uint64_t q = doc_off[d];
    if (q && q < n_bytes && bit_at(M, q - 1) && bit_at(M, q)) {  // (never beyond: the offsets are checked)
      atomicOr(S + (q >> 5), 1u << (uint32_t)(q & 31));
      atomicOr(T + ((q - 1) >> 5), 1u << (uint32_t)((q - 1) & 31));
    }
  }
}

// blk_s / blk_t: the set bits of S / T before every block (select_launch_rank).  doc[j], w0[j], w1[j] of run j
__global__ __launch_bounds__(256) void kex_windows(const uint32_t *S, const uint32_t *T, uint64_t n_words, uint64_t n_blk,
                                                   const unsigned long long *blk_s, const unsigned long long *blk_t,
                                                   const uint8_t *corpus, const uint64_t *doc_off, uint64_t n_docs, uint32_t before,
                                                   uint32_t after, uint64_t *doc, uint64_t *w0, uint64_t *w1) {
  for_ranked_bits(S, n_words, n_blk, blk_s, [&](uint64_t w, uint32_t i, uint64_t at) {
    const uint64_t p = w * 32 + i, d = owner_of(doc_off, n_docs, p);
    doc[at] = d;
    w0[at] = excerpt_w0(corpus, doc_off[d], p, before);
  });
  for_ranked_bits(T, n_words, n_blk, blk_t, [&](uint64_t w, uint32_t i, uint64_t at) {
    const uint64_t p = w * 32 + i, d = owner_of(doc_off, n_docs, p);
    w1[at] = excerpt_w1(corpus, doc_off[d + 1], p + 1, after);
  });
}

// first / last: ceil(n_runs / 32) words each, whole words are written
__global__ __launch_bounds__(256) void kex_merge(const uint64_t *doc, const uint64_t *w0, const uint64_t *w1, uint64_t n_runs,
                                                 uint32_t *first, uint32_t *last) {
  const int lane = threadIdx.x & 63;
  const uint64_t n_words = (n_runs + 31) / 32;
  const uint64_t wave = ((uint64_t)blockIdx.x * 256 + threadIdx.x) >> 6, n_waves = (uint64_t)gridDim.x * 4;
  for (uint64_t j0 = wave * 64; j0 < n_runs; j0 += n_waves * 64) {  // (the same trips in every lane of a wave)
    const uint64_t j = j0 + lane;
    bool f = false, l = false;
    if (j < n_runs) {
      const uint64_t d = doc[j];
      f = j == 0 || doc[j - 1] != d || w0[j] > w1[j - 1];
      l = j + 1 == n_runs || doc[j + 1] != d || w0[j + 1] > w1[j];
    }
    const unsigned long long bf = __ballot(f), bl = __ballot(l);
    const uint64_t w = j0 / 32 + lane;
    if (lane < 2 && w < n_words) {
      first[w] = (uint32_t)(bf >> (32 * lane));
      last[w] = (uint32_t)(bl >> (32 * lane));
    }
  }
}

// A[0 .. R], end[0 .. R] (in shift): the stretches outside the excerpts
__global__ __launch_bounds__(256) void kex_gaps(const uint32_t *first, const uint32_t *last, uint64_t n_words, uint64_t n_blk,
                                                const unsigned long long *blk_f, const unsigned long long *blk_l, const uint64_t *w0,
                                                const uint64_t *w1, uint64_t n_bytes, uint64_t n_exc, uint64_t *A, long long *end) {
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    A[0] = 0;
    end[n_exc] = (long long)n_bytes;
  }
  for_ranked_bits(first, n_words, n_blk, blk_f, [&](uint64_t w, uint32_t i, uint64_t at) { end[at] = (long long)w0[w * 32 + i]; });
  for_ranked_bits(last, n_words, n_blk, blk_l, [&](uint64_t w, uint32_t i, uint64_t at) { A[at + 1] = w1[w * 32 + i]; });
}

// shift[j]: end[j] -> delta[j]; sel[j] = a hit of key 0; ent[0] = the empty replacement
__global__ __launch_bounds__(256) void kex_delta(const uint64_t *A, long long *shift, uint64_t n, int32_t *sel, RepEntry *ent) {
  const uint64_t tid = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (tid == 0) {
    ent[0].off = 0;
    ent[0].len = 0;
    ent[0].keep = 0;
  }
  for (uint64_t j = tid; j < n; j += (uint64_t)gridDim.x * 256) {
    shift[j] = (long long)A[j] - shift[j];
    sel[j * 3] = 0;
    sel[j * 3 + 1] = 0;
    sel[j * 3 + 2] = 0;
  }
}

// shift[0 .. R + 1]: the scanned deltas.  starts[0, R) and out_off[0 .. R], either may be null
__global__ __launch_bounds__(256) void kex_emit(const uint64_t *A, const long long *shift, uint64_t n_exc, unsigned long long *starts,
                                                unsigned long long *out_off) {
  for (uint64_t r = (uint64_t)blockIdx.x * 256 + threadIdx.x; r <= n_exc; r += (uint64_t)gridDim.x * 256) {
    const long long o = (long long)A[r] + shift[r];
    if (out_off) out_off[r] = (unsigned long long)o;
    if (starts && r < n_exc) starts[r] = (unsigned long long)(o - shift[r + 1]);
  }
}

}  // namespace

void excerpt_launch_edges(const uint32_t *M, uint64_t n_bytes, const uint64_t *doc_off, uint64_t n_docs, uint32_t *S, uint32_t *T,
                          uint32_t max_blocks, void *stream) {
  if (!n_bytes) return;
  const uint64_t n_words = (n_bytes + 31) / 32;
  hipLaunchKernelGGL(kex_edges, dim3(grid_for(n_words, 256, max_blocks)), dim3(256), 0, (hipStream_t)stream, M, n_words, n_bytes, S, T);
  if (n_docs > 1)
    hipLaunchKernelGGL(kex_doc_edges, dim3(grid_for(n_docs - 1, 256, max_blocks)), dim3(256), 0, (hipStream_t)stream, M, doc_off, n_docs,
                       n_bytes, S, T);
}

void excerpt_launch_windows(const uint32_t *S, const uint32_t *T, uint64_t n_bytes, const uint64_t *blk_s, const uint64_t *blk_t,
                            const uint8_t *corpus, const uint64_t *doc_off, uint64_t n_docs, uint32_t before, uint32_t after,
                            uint64_t n_runs, uint64_t *doc, uint64_t *w0, uint64_t *w1, uint32_t *first, uint32_t *last,
                            uint32_t max_blocks, void *stream) {
  if (!n_runs) return;
  const uint64_t n_words = (n_bytes + 31) / 32, n_blk = rank_blocks(n_bytes);
  hipLaunchKernelGGL(kex_windows, dim3(grid_for(n_blk * 64, 256, max_blocks)), dim3(256), 0, (hipStream_t)stream, S, T, n_words, n_blk,
                     reinterpret_cast<const unsigned long long *>(blk_s), reinterpret_cast<const unsigned long long *>(blk_t), corpus,
                     doc_off, n_docs, before, after, doc, w0, w1);
  hipLaunchKernelGGL(kex_merge, dim3(grid_for(n_runs, 256, max_blocks)), dim3(256), 0, (hipStream_t)stream, doc, w0, w1, n_runs, first,
                     last);
}

void excerpt_launch_gaps(const uint32_t *first, const uint32_t *last, uint64_t n_runs, const uint64_t *blk_f, const uint64_t *blk_l,
                         const uint64_t *w0, const uint64_t *w1, uint64_t n_bytes, uint64_t n_exc, uint64_t *A, int64_t *shift,
                         void *sel, RepEntry *ent, uint32_t max_blocks, void *stream) {
  const uint64_t n_words = (n_runs + 31) / 32, n_blk = rank_blocks(n_runs);
  hipLaunchKernelGGL(kex_gaps, dim3(grid_for(std::max<uint64_t>(n_blk, 1) * 64, 256, max_blocks)), dim3(256), 0, (hipStream_t)stream,
                     first, last, n_words, n_blk, reinterpret_cast<const unsigned long long *>(blk_f),
                     reinterpret_cast<const unsigned long long *>(blk_l), w0, w1, n_bytes, n_exc, A, reinterpret_cast<long long *>(shift));
  hipLaunchKernelGGL(kex_delta, dim3(grid_for(n_exc + 1, 256, max_blocks)), dim3(256), 0, (hipStream_t)stream, A,
                     reinterpret_cast<long long *>(shift), n_exc + 1, (int32_t *)sel, ent);
}

void excerpt_launch_emit(const uint64_t *A, const int64_t *shift, uint64_t n_exc, uint64_t *starts, uint64_t *out_off, uint32_t max_blocks,
                         void *stream) {
  hipLaunchKernelGGL(kex_emit, dim3(grid_for(n_exc + 1, 256, max_blocks)), dim3(256), 0, (hipStream_t)stream, A,
                     reinterpret_cast<const long long *>(shift), n_exc, reinterpret_cast<unsigned long long *>(starts),
                     reinterpret_cast<unsigned long long *>(out_off));
}

}  // namespace aha
