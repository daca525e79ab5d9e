// scan_grep.hip -- the records and grep paths (aha_ac_records_batch*, aha_ac_grep_batch*).
// Records: one pass over the text finds where records end; the rank of that mask (select_launch_rank) numbers them.  The
// ranked masks here are walked by post_common.hpp's for_ranked_bits.
//   kgr_ends         the record-end mask, one bit per text byte: bit p = (corpus[p] == delim).  A lane owns one mask word, 32
//                    text bytes, as two aligned 16-byte loads.  The corpus may start anywhere: the loads are aligned to the
//                    ADDRESS, so the words they give are `head` bits behind the mask's words (head = the bytes in front of
//                    the first aligned address, below 16) -- a mask word is the funnel of two neighbouring lanes' words.  The
//                    head bytes and the bytes behind the last whole piece are read one by one: nothing outside
//                    [corpus, corpus + N) is touched.
//   kgr_doc_ends     a lane per document: a document's end is a record's end, bit doc_offsets[d] - 1 (a boundary behind a
//                    delimiter sets a set bit: counted once; an empty document sets its predecessor's bit again).
//   kgr_emit_ends    every set bit p in position order: rec_offsets[rank + 1] = p + 1.
// Grep: hits per document (the count call) -> which documents stay -> the dropped runs as "deleted hits" for replace's copy.
//   kgr_flag         a lane per document, three masks over documents by wave ballot: keep; S = dropped and the predecessor
//                    is kept or there is none (a run of dropped documents starts); T = dropped and the successor is kept or
//                    there is none (a run ends).  The j-th bit of S and the j-th bit of T delimit run j.
//   kgr_runs         over the ranked S and T masks: A[j] = doc_offsets[a_j], end[j] = doc_offsets[b_j + 1] -- no lane walks
//                    along a run.
//   kgr_delta        delta[j] = -(end[j] - A[j]), the run's synthesized selection row and the one-entry table (the empty
//                    replacement): what scan_replace.hip's scan and copy take.
//   kgr_emit_docs    every kept document d in order, r = its rank among the kept: kept_docs[r] = d, doc_out_offsets[r] =
//                    doc_offsets[d] + shift[runs that start in front of d]; the last entry is the total.
// Vector loads, stores and atomics and plain C++ only.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "image.hpp"
#include "post_common.hpp"

namespace aha {
namespace {

using post::grid_for;

// bit k = (byte k of w == the byte b4 repeats), k in [0, 4)
__device__ __forceinline__ uint32_t gr_eq4(uint32_t w, uint32_t b4) {
  const uint32_t x = w ^ b4;
  const uint32_t z = ~(((x & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | x) & 0x80808080u;  // 0x80 where the byte of x is 0, exactly
  return (((z >> 7) * 0x00204081u) >> 21) & 0xFu;
}

// the 16 bits of the aligned piece at text position a (a + head is the position in the corpus; the address is 16-byte
// aligned): a whole piece by one load, the bytes of the last, partial one singly, nothing behind the text
__device__ __forceinline__ uint32_t gr_piece(const uint8_t *text, uint64_t a, uint64_t na, uint32_t delim, uint32_t b4) {
  if (a + 16 <= na) {
    const uint4 v = *reinterpret_cast<const uint4 *>(text + a);
    return gr_eq4(v.x, b4) | gr_eq4(v.y, b4) << 4 | gr_eq4(v.z, b4) << 8 | gr_eq4(v.w, b4) << 12;
  }
  uint32_t bits = 0;
  for (uint32_t k = 0; k < 16; k++)
    if (a + k < na && text[a + k] == delim) bits |= 1u << k;
  return bits;
}

// the aligned word j: text positions [32 j, 32 j + 32) behind the head
__device__ __forceinline__ uint32_t gr_word(const uint8_t *text, uint64_t j, uint64_t na, uint32_t delim, uint32_t b4) {
  return gr_piece(text, j * 32, na, delim, b4) | gr_piece(text, j * 32 + 16, na, delim, b4) << 16;
}

// mask[0, n_words): bit p = (corpus[p] == delim), the bits from n_bytes on are 0.  head < 16: the bytes in front of the
// first 16-byte aligned address (all of the text where it is shorter)
__global__ __launch_bounds__(256) void kgr_ends(const uint8_t *corpus, uint64_t n_bytes, uint32_t head, uint32_t delim,
                                                uint64_t n_words, uint32_t *mask) {
  const int lane = threadIdx.x & 63;
  const uint32_t b4 = delim * 0x01010101u;
  const uint8_t *text = corpus + head;
  const uint64_t na = n_bytes - head;
  const uint64_t wave = ((uint64_t)blockIdx.x * 256 + threadIdx.x) >> 6, n_waves = (uint64_t)gridDim.x * 4;
  for (uint64_t w0 = wave * 64; w0 < n_words; w0 += n_waves * 64) {  // (the same trips in every lane of a wave)
    const uint64_t w = w0 + lane;
    const uint32_t cur = w < n_words ? gr_word(text, w, na, delim, b4) : 0u;
    uint32_t prev = __shfl_up(cur, 1, 64);
    if (lane == 0) {
      prev = 0;
      if (w0) {
        prev = gr_word(text, w0 - 1, na, delim, b4);
      } else {  // the head bytes, as the top bits of the word in front of the first
        for (uint32_t k = 0; k < head; k++)
          if (corpus[k] == delim) prev |= 1u << (32 - head + k);
      }
    }
    // the mask word = the last `head` bits of prev, then the first 32 - head bits of cur
    if (w < n_words) mask[w] = (uint32_t)(((unsigned long long)cur << 32 | prev) >> (32 - head));
  }
}

__global__ __launch_bounds__(256) void kgr_doc_ends(const uint64_t *doc_off, uint64_t n_docs, uint64_t n_bytes, uint32_t *mask) {
  for (uint64_t d = (uint64_t)blockIdx.x * 256 + threadIdx.x + 1; d <= n_docs; d += (uint64_t)gridDim.x * 256) {
    const uint64_t q = doc_off[d];
    if (q && q <= n_bytes) atomicOr(mask + ((q - 1) >> 5), 1u << (uint32_t)((q - 1) & 31));  // (never beyond: the offsets are checked)
  }
}

__global__ __launch_bounds__(256) void kgr_emit_ends(const uint32_t *mask, uint64_t n_words, uint64_t n_blk, const unsigned long long *blk,
                                                     unsigned long long *rec_off) {
  if (blockIdx.x == 0 && threadIdx.x == 0) rec_off[0] = 0;
  for_ranked_bits(mask, n_words, n_blk, blk, [&](uint64_t w, uint32_t i, uint64_t at) { rec_off[at + 1] = w * 32 + i + 1; });
}

// dho[0 .. D]: the documents' hit offsets.  keep / S / T: ceil(D / 32) words each, whole words are written
__global__ __launch_bounds__(256) void kgr_flag(const uint64_t *dho, uint64_t n_docs, uint32_t invert, uint32_t *keep, uint32_t *S,
                                                uint32_t *T) {
  const int lane = threadIdx.x & 63;
  const uint64_t n_words = (n_docs + 31) / 32;
  const uint64_t wave = ((uint64_t)blockIdx.x * 256 + threadIdx.x) >> 6, n_waves = (uint64_t)gridDim.x * 4;
  for (uint64_t d0 = wave * 64; d0 < n_docs; d0 += n_waves * 64) {  // (the same trips in every lane of a wave)
    const uint64_t d = d0 + lane;
    bool k = false, s = false, t = false;
    if (d < n_docs) {
      const uint64_t h0 = dho[d], h1 = dho[d + 1];
      k = (h1 > h0) != (invert != 0);
      if (!k) {
        s = d == 0 || (dho[d] > dho[d - 1]) != (invert != 0);
        t = d + 1 == n_docs || (dho[d + 2] > h1) != (invert != 0);
      }
    }
    const unsigned long long bk = __ballot(k), bs = __ballot(s), bt = __ballot(t);
    const uint64_t w = d0 / 32 + lane;
    if (lane < 2 && w < n_words) {
      keep[w] = (uint32_t)(bk >> (32 * lane));
      S[w] = (uint32_t)(bs >> (32 * lane));
      T[w] = (uint32_t)(bt >> (32 * lane));
    }
  }
}

// blk_s / blk_t: the set bits of S / T before every block (select_launch_rank).  start[j] = where run j's first document
// starts, end[j] = where its last one ends
__global__ __launch_bounds__(256) void kgr_runs(const uint32_t *S, const uint32_t *T, uint64_t n_words, uint64_t n_blk,
                                                const unsigned long long *blk_s, const unsigned long long *blk_t, const uint64_t *doc_off,
                                                uint64_t *start, long long *end) {
  for_ranked_bits(S, n_words, n_blk, blk_s, [&](uint64_t w, uint32_t i, uint64_t at) { start[at] = doc_off[w * 32 + i]; });
  for_ranked_bits(T, n_words, n_blk, blk_t, [&](uint64_t w, uint32_t i, uint64_t at) { end[at] = (long long)doc_off[w * 32 + i + 1]; });
}

// shift[j]: end[j] -> delta[j]; sel[j] = a hit of key 0; ent[0] = the empty replacement
__global__ __launch_bounds__(256) void kgr_delta(const uint64_t *start, long long *shift, uint64_t n, int32_t *sel, RepEntry *ent) {
  const uint64_t tid = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (tid == 0) {
    ent[0].off = 0;
    ent[0].len = 0;
    ent[0].keep = 0;
  }
  for (uint64_t j = tid; j < n; j += (uint64_t)gridDim.x * 256) {
    shift[j] = (long long)start[j] - shift[j];
    sel[j * 3] = 0;
    sel[j * 3 + 1] = 0;
    sel[j * 3 + 2] = 0;
  }
}

__global__ __launch_bounds__(256) void kgr_emit_docs(const uint32_t *keep, const uint32_t *S, uint64_t n_words, uint64_t n_blk,
                                                     const unsigned long long *blk_k, const unsigned long long *blk_s,
                                                     const uint64_t *doc_off, uint64_t n_docs, const long long *shift, uint64_t n_runs,
                                                     unsigned long long *kept_docs, unsigned long long *doc_out) {
  const int lane = threadIdx.x & 63;
  const uint64_t wave = ((uint64_t)blockIdx.x * 256 + threadIdx.x) >> 6, n_waves = (uint64_t)gridDim.x * 4;
  if (wave == 0 && lane == 0 && doc_out) doc_out[blk_k[n_blk]] = (unsigned long long)((long long)doc_off[n_docs] + shift[n_runs]);
  for (uint64_t b = wave; b < n_blk; b += n_waves) {
    const uint64_t w = b * kRankBlockWords + lane;
    uint32_t bits = w < n_words ? keep[w] : 0u;
    const uint32_t sbits = w < n_words ? S[w] : 0u;
    uint64_t at = blk_k[b] + wave_excl_scan((uint32_t)__popc(bits));
    const uint64_t runs = blk_s[b] + wave_excl_scan((uint32_t)__popc(sbits));  // the runs that start in front of this word
    while (bits) {
      const uint32_t i = (uint32_t)__ffs(bits) - 1u;
      bits &= bits - 1u;
      const uint64_t d = w * 32 + i;
      const uint64_t j = runs + (uint32_t)__popc(sbits & ((1u << i) - 1u));
      if (kept_docs) kept_docs[at] = d;
      if (doc_out) doc_out[at] = (unsigned long long)((long long)doc_off[d] + shift[j]);
      at++;
    }
  }
}

}  // namespace

void grep_launch_ends(const uint8_t *corpus, uint64_t n_bytes, uint8_t delim, const uint64_t *doc_off, uint64_t n_docs, uint32_t *mask,
                      uint32_t max_blocks, void *stream) {
  if (!n_bytes) return;
  const uint64_t n_words = (n_bytes + 31) / 32;
  const uint32_t head = (uint32_t)std::min<uint64_t>((16 - (reinterpret_cast<uintptr_t>(corpus) & 15)) & 15, n_bytes);
  hipLaunchKernelGGL(kgr_ends, dim3(grid_for(n_words, 256, max_blocks)), dim3(256), 0, (hipStream_t)stream, corpus, n_bytes, head,
                     (uint32_t)delim, n_words, mask);
  if (n_docs)
    hipLaunchKernelGGL(kgr_doc_ends, dim3(grid_for(n_docs, 256, max_blocks)), dim3(256), 0, (hipStream_t)stream, doc_off, n_docs, n_bytes,
                       mask);
}

void grep_launch_emit_ends(const uint32_t *mask, uint64_t n_bytes, const uint64_t *blk, uint64_t *rec_off, uint32_t max_blocks,
                           void *stream) {
  const uint64_t n_words = (n_bytes + 31) / 32, n_blk = rank_blocks(n_bytes);
  hipLaunchKernelGGL(kgr_emit_ends, dim3(grid_for(n_blk * 64, 256, max_blocks)), dim3(256), 0, (hipStream_t)stream, mask, n_words, n_blk,
                     reinterpret_cast<const unsigned long long *>(blk), reinterpret_cast<unsigned long long *>(rec_off));
}

void grep_launch_flag(const uint64_t *dho, uint64_t n_docs, bool invert, uint32_t *keep, uint32_t *S, uint32_t *T, uint32_t max_blocks,
                      void *stream) {
  if (!n_docs) return;
  hipLaunchKernelGGL(kgr_flag, dim3(grid_for(n_docs, 256, max_blocks)), dim3(256), 0, (hipStream_t)stream, dho, n_docs, invert ? 1u : 0u,
                     keep, S, T);
}

void grep_launch_runs(const uint32_t *S, const uint32_t *T, uint64_t n_docs, const uint64_t *blk_s, const uint64_t *blk_t,
                      const uint64_t *doc_off, uint64_t n_runs, uint64_t *start, int64_t *shift, void *sel, RepEntry *ent,
                      uint32_t max_blocks, void *stream) {
  const uint64_t n_words = (n_docs + 31) / 32, n_blk = rank_blocks(n_docs);
  if (n_runs)
    hipLaunchKernelGGL(kgr_runs, dim3(grid_for(n_blk * 64, 256, max_blocks)), dim3(256), 0, (hipStream_t)stream, S, T, n_words, n_blk,
                       reinterpret_cast<const unsigned long long *>(blk_s), reinterpret_cast<const unsigned long long *>(blk_t), doc_off,
                       start, reinterpret_cast<long long *>(shift));
  hipLaunchKernelGGL(kgr_delta, dim3(grid_for(n_runs, 256, max_blocks)), dim3(256), 0, (hipStream_t)stream, start,
                     reinterpret_cast<long long *>(shift), n_runs, (int32_t *)sel, ent);
}

void grep_launch_emit_docs(const uint32_t *keep, const uint32_t *S, uint64_t n_docs, const uint64_t *blk_k, const uint64_t *blk_s,
                           const uint64_t *doc_off, const int64_t *shift, uint64_t n_runs, uint64_t *kept_docs, uint64_t *doc_out,
                           uint32_t max_blocks, void *stream) {
  const uint64_t n_words = (n_docs + 31) / 32, n_blk = rank_blocks(n_docs);
  hipLaunchKernelGGL(kgr_emit_docs, dim3(grid_for(std::max<uint64_t>(n_blk, 1) * 64, 256, max_blocks)), dim3(256), 0, (hipStream_t)stream,
                     keep, S, n_words, n_blk, reinterpret_cast<const unsigned long long *>(blk_k),
                     reinterpret_cast<const unsigned long long *>(blk_s), doc_off, n_docs, reinterpret_cast<const long long *>(shift),
                     n_runs, reinterpret_cast<unsigned long long *>(kept_docs), reinterpret_cast<unsigned long long *>(doc_out));
}

}  // namespace aha
