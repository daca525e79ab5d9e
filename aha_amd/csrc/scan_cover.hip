// scan_cover.hip -- the cover path (aha_ac_cover_batch*): which bytes lie inside a hit, and a redacted copy, without the hit list.
//
// All hits of one END position end at the same byte and the first one -- the END state's own key -- is the longest (the others
// hang on its output chain: proper suffixes, src/aha/ac.cr:265-278).  So the union of the hits' spans is the union of ONE span
// per event, [end - len(head key), end): no chain is walked, nothing is held per hit.  A cover call keeps the count call's
// pipeline (traversal, full-size event regions, per-chunk hit counts, total) and puts these passes where the key counts stand:
//   kv_chunk_docs   per chunk the first document that starts at or behind its first byte (the records hold the end offset IN
//                   THE DOCUMENT; the document of an event is the last one that starts in the event's chunk with a rank --
//                   doc_ev_rank / doc_hit_rank, noted by the traversal at the boundary -- at or below the event's, else the
//                   document that holds the chunk's first byte)
//   kv_clear        the mask, unless the pass was aborted (a call that fails writes none of the caller's buffers)
//   kv_spans        one span per event, from the records kc_visits reads (scan_count.hip).  A workgroup takes groups of
//                   consecutive chunks and keeps the bits of the group's text range in LDS (32 KiB: 256 KiB of text): the part of
//                   a span inside the tile is ORed there, what lies outside -- a span reaches back up to Lmax - 1 bytes -- goes to
//                   the global mask with atomicOr; the tile's non-zero words go out with atomicOr too (a neighbour may have
//                   written into them).
//   kv_redact       corpus + mask -> redacted, 16 bytes per lane;  kv_doc_covered / kv_total: popcounts of the mask.
// The two-pass engine's form (a separator filter, keys beyond 4096 bytes) is k_count's cover mode (kernels.hip).
#include <hip/hip_runtime.h>

#include <algorithm>

#include "automaton.hpp"
#include "cover_span.hpp"
#include "devcommon.hpp"
#include "image.hpp"
#include "post_common.hpp"
#include "unit.hpp"

namespace aha {
namespace {

using post::grid_for;

constexpr int kCvThreads = 256;
constexpr uint32_t kCvTileWords = 8192;                // 32 KiB of LDS
constexpr uint64_t kCvTileBytes = kCvTileWords * 32ull;  // the text its bits stand for
enum { kSrcRegions = 0, kSrcUnit = 1 };

__global__ __launch_bounds__(256) void kv_chunk_docs(V2Args M, uint64_t *cdoc) {
  const uint64_t c = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (c > M.n_chunks) return;
  cdoc[c] = first_boundary(M.doc_off, M.n_docs, min(c * M.S, M.n_bytes));
}

// words[0, n) = 0 unless the pass was aborted; 16 bytes per lane where the words are aligned for it
__global__ __launch_bounds__(256) void kv_clear(uint32_t *words, uint64_t n, const unsigned long long *abortf) {
  if (abortf && *abortf) return;
  const uint64_t head = min<uint64_t>(n, ((16u - (uint32_t)(reinterpret_cast<uintptr_t>(words) & 15u)) & 15u) / 4u);
  const uint64_t n4 = (n - head) / 4;
  const uint64_t tid = (uint64_t)blockIdx.x * 256 + threadIdx.x, nt = (uint64_t)gridDim.x * 256;
  uint4 *body = reinterpret_cast<uint4 *>(words + head);
  for (uint64_t i = tid; i < n4; i += nt) body[i] = make_uint4(0, 0, 0, 0);
  if (tid < head) words[tid] = 0u;
  const uint64_t tail0 = head + n4 * 4;
  if (tid < n - tail0) words[tail0 + tid] = 0u;
}

// the largest d in [lo, hi) with rank[d] <= r, or lo - 1: rank[] does not fall over the documents that start in one chunk
__device__ __forceinline__ uint64_t cv_doc(const uint32_t *rank, uint64_t lo, uint64_t hi, uint32_t r) {
  while (lo < hi) {
    const uint64_t mid = (lo + hi) >> 1;
    if (rank[mid] <= r)
      lo = mid + 1;
    else
      hi = mid;
  }
  return lo - 1;
}

// G: chunks of a group (kSrcUnit: a multiple of 64, the traversal's waves).  bit0: the batch's first byte in the mask (a
// document range of a larger batch)
template <int SRC>
__global__ __launch_bounds__(kCvThreads) void kv_spans(DevAut A, V2Args M, const uint2 *uend, const uint64_t *cdoc, uint32_t *mask,
                                                       uint64_t bit0, uint32_t G) {
  __shared__ uint32_t s_tile[kCvTileWords];
  if (M.cursor[1]) return;  // (an aborted pass: nothing is written)
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  constexpr uint32_t kWaves = kCvThreads / 64;
  const uint32_t stride = M.ev_stride;
  const uint64_t S = M.S, N = M.n_bytes, D = M.n_docs;
  const uint64_t n_groups = (M.n_chunks + G - 1) / G;
  for (uint64_t g = blockIdx.x; g < n_groups; g += gridDim.x) {
    const uint64_t c0 = g * G, c1 = min<uint64_t>(c0 + G, M.n_chunks);
    const uint64_t tw0 = (bit0 + c0 * S) >> 5;  // the tile's first word of the mask
    const uint32_t tw = (uint32_t)min<uint64_t>(((bit0 + min(c1 * S, N) + 31) >> 5) - tw0, kCvTileWords);
    for (uint32_t i = threadIdx.x; i < tw; i += kCvThreads) s_tile[i] = 0u;
    __syncthreads();
    // one span: bits [s, e) of the batch
    auto span = [&](uint64_t e, uint32_t len) {
      e = min(e, N);  // (what the records and the validated offsets guarantee anyway: no word beyond the mask is touched)
      const uint64_t s = e - min<uint64_t>(e, len);
      cover_span_words(bit0 + s, bit0 + e, [&](uint64_t w, uint32_t bits) {
        const uint64_t r = w - tw0;
        if (r < tw)
          cover_or_word(&s_tile[r], bits);
        else
          cover_or_word(mask + w, bits);
      });
    };
    if (SRC == kSrcRegions) {
      for (uint64_t c = c0 + wv; c < c1; c += kWaves) {  // a wave per chunk
        const uint32_t n = min(M.ev_cnt[c], stride);
        if (!n) continue;
        const uint2 *reg = M.evd + c * stride;
        const uint64_t lo = cdoc[c], hi = cdoc[c + 1];
        const uint64_t base0 = lo ? M.doc_off[lo - 1] : 0ull;  // the document that holds the chunk's first byte
        for (uint32_t i = lane; i < n; i += 64) {
          const uint2 rec = reg[i];
          if ((rec.x >> 24) == 0u) continue;  // (a record that stands for no hit -- the pair engine's voided events)
          const uint32_t id = rec.x & 0xFFFFFFu;
          const uint32_t len = A.chain ? A.chain[id].x : A.key_ln[id].x;  // the head key of the chain
          uint64_t base = base0;
          if (hi > lo) {
            const uint64_t d = cv_doc(M.doc_ev_rank, lo, hi, i);
            if (d > D) continue;  // (no document: never, chunk 0 starts with document 0)
            base = M.doc_off[d];
          }
          span(base + rec.y, len);
        }
      }
    } else {
      const uint32_t bb = M.unit_bb, bmask = (1u << bb) - 1u;
      for (uint64_t q = c0 / 64; q * 64 < c1; q++) {  // the traversal's groups of 64 chunks, all waves on each
        const uint64_t c = q * 64 + lane;
        const uint32_t total = wave_sum(c < M.n_chunks ? min(M.ev_cnt[c], stride) : 0u);  // (every wave sums the group's events for itself)
        const uint32_t *src = M.evg + q * 64 * stride * 3;
        for (uint32_t i = threadIdx.x; i < total; i += kCvThreads) {
          const uint32_t x = src[(size_t)i * 3], y = src[(size_t)i * 3 + 1], z = src[(size_t)i * 3 + 2];
          if (u_rec_n(x, z, bb) == 0u) continue;
          const uint2 ue = uend[x & bmask];
          const uint32_t len = (ue.x >> 24) | (ue.y >> 24) << 8;
          const uint64_t ce = q * 64 + ((x >> bb) & 63u);  // the event's chunk
          if (ce >= M.n_chunks) continue;
          const uint64_t lo = cdoc[ce], hi = cdoc[ce + 1];
          const uint64_t d = hi > lo ? cv_doc(M.doc_hit_rank, lo, hi, u_rec_before(z)) : lo - 1;
          if (d > D) continue;
          span(M.doc_off[d] + y, len);
        }
      }
    }
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < tw; i += kCvThreads) {
      const uint32_t v = s_tile[i];
      if (v) atomicOr(mask + tw0 + i, v);
    }
    __syncthreads();
  }
}

// bits -> a byte mask: bit k of the low four bits to byte k
__device__ __forceinline__ uint32_t cv_spread4(uint32_t bits4) { return ((bits4 * 0x00204081u) & 0x01010101u) * 0xFFu; }

// dst[j] = fill where bit j of the mask is set, src[j] elsewhere; dst == src: in place.  A lane takes 16 bytes -- one load and
// one store of 16 bytes where both pointers are aligned for it, byte by byte otherwise and in the tail.
__global__ __launch_bounds__(256) void kv_redact(const uint8_t *src, uint8_t *dst, const uint32_t *mask, uint64_t n, uint32_t fill) {
  const bool wide = ((reinterpret_cast<uintptr_t>(src) | reinterpret_cast<uintptr_t>(dst)) & 15u) == 0;
  const uint64_t n16 = (n + 15) / 16;
  const uint32_t f4 = fill * 0x01010101u;
  for (uint64_t j = (uint64_t)blockIdx.x * 256 + threadIdx.x; j < n16; j += (uint64_t)gridDim.x * 256) {
    const uint32_t bits = (mask[j >> 1] >> ((j & 1) * 16)) & 0xFFFFu;
    const uint64_t p = j * 16;
    if (wide && p + 16 <= n) {
      if (!bits && src == dst) continue;
      uint4 v = *reinterpret_cast<const uint4 *>(src + p);
      const uint32_t m0 = cv_spread4(bits & 15u), m1 = cv_spread4((bits >> 4) & 15u), m2 = cv_spread4((bits >> 8) & 15u),
                     m3 = cv_spread4(bits >> 12);
      v.x = (v.x & ~m0) | (f4 & m0);
      v.y = (v.y & ~m1) | (f4 & m1);
      v.z = (v.z & ~m2) | (f4 & m2);
      v.w = (v.w & ~m3) | (f4 & m3);
      *reinterpret_cast<uint4 *>(dst + p) = v;
    } else {
      const uint32_t m = (uint32_t)min<uint64_t>(16, n - p);
      for (uint32_t k = 0; k < m; k++) {
        const bool set = (bits >> k) & 1u;
        if (set)
          dst[p + k] = (uint8_t)fill;
        else if (src != dst)
          dst[p + k] = src[p + k];
      }
    }
  }
}

// set bits of mask bits [a, b), by the lanes of one wave
__device__ __forceinline__ uint64_t cv_popcount_range(const uint32_t *mask, uint64_t a, uint64_t b, int lane) {
  uint64_t cnt = 0;
  if (a < b) {
    const uint64_t w0 = a >> 5, w1 = (b - 1) >> 5;
    for (uint64_t w = w0 + lane; w <= w1; w += 64) {
      uint32_t v = mask[w];
      if (w == w0) v &= ~0u << (uint32_t)(a & 31);
      if (w == w1) v &= ~0u >> (31u - (uint32_t)((b - 1) & 31));
      cnt += (uint32_t)__popc(v);
    }
  }
  return wave_sum(cnt);
}

// doc_covered[d] = set bits of the document's range (documents are not word-aligned): a wave per document
__global__ __launch_bounds__(256) void kv_doc_covered(const uint32_t *mask, const uint64_t *doc_off, uint64_t n_docs,
                                                      unsigned long long *doc_covered) {
  const int lane = threadIdx.x & 63;
  const uint64_t wave = ((uint64_t)blockIdx.x * 256 + threadIdx.x) >> 6, n_waves = (uint64_t)gridDim.x * 4;
  for (uint64_t d = wave; d < n_docs; d += n_waves) {
    const uint64_t cnt = cv_popcount_range(mask, doc_off[d], doc_off[d + 1], lane);
    if (lane == 0) doc_covered[d] = cnt;
  }
}

// *total += set bits of words[0, n) (the bits behind the batch are clear)
__global__ __launch_bounds__(256) void kv_total(const uint32_t *words, uint64_t n, unsigned long long *total) {
  uint64_t cnt = 0;
  for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (uint64_t)gridDim.x * 256) cnt += (uint32_t)__popc(words[i]);
  cnt = wave_sum(cnt);
  if ((threadIdx.x & 63) == 0 && cnt) atomicAdd(total, (unsigned long long)cnt);
}

}  // namespace

void cover_launch_clear(uint32_t *words, uint64_t n_words, const unsigned long long *abortf, uint32_t max_blocks, void *stream) {
  hipLaunchKernelGGL(kv_clear, dim3(grid_for((n_words + 3) / 4 + 8, 256, max_blocks)), dim3(256), 0, (hipStream_t)stream, words, n_words,
                     abortf);
}

void cover_launch_spans(const DevAut &A, const V2Args &M, const uint2 *uend, uint64_t *cdoc, uint32_t *mask, uint64_t bit0,
                        uint32_t max_blocks, void *stream) {
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(kv_chunk_docs, dim3((uint32_t)((M.n_chunks + 1 + 255) / 256)), dim3(256), 0, s, M, cdoc);
  // chunks of a group: what a tile holds the bits of, at most 256 (a wave per chunk, in turns)
  uint64_t G = std::max<uint64_t>(1, std::min<uint64_t>(kCvTileBytes / M.S, 256));
  if (uend) G = std::max<uint64_t>(64, G / 64 * 64);
  const uint64_t n_groups = (M.n_chunks + G - 1) / G;
  const dim3 grid(grid_for(n_groups, 1, max_blocks));
  if (uend)
    hipLaunchKernelGGL(kv_spans<kSrcUnit>, grid, dim3(kCvThreads), 0, s, A, M, uend, cdoc, mask, bit0, (uint32_t)G);
  else
    hipLaunchKernelGGL(kv_spans<kSrcRegions>, grid, dim3(kCvThreads), 0, s, A, M, uend, cdoc, mask, bit0, (uint32_t)G);
}

void cover_launch_redact(const uint8_t *src, uint8_t *dst, const uint32_t *mask, uint64_t n_bytes, uint8_t fill, uint32_t max_blocks,
                         void *stream) {
  hipLaunchKernelGGL(kv_redact, dim3(grid_for((n_bytes + 15) / 16, 256, max_blocks)), dim3(256), 0, (hipStream_t)stream, src, dst, mask,
                     n_bytes, (uint32_t)fill);
}

void cover_launch_doc_covered(const uint32_t *mask, const uint64_t *doc_off, uint64_t n_docs, uint64_t *doc_covered,
                              uint32_t max_blocks, void *stream) {
  hipLaunchKernelGGL(kv_doc_covered, dim3(grid_for(n_docs * 64, 256, max_blocks)), dim3(256), 0, (hipStream_t)stream, mask, doc_off, n_docs,
                     reinterpret_cast<unsigned long long *>(doc_covered));
}

void cover_launch_total(const uint32_t *mask, uint64_t n_words, uint64_t *total, uint32_t max_blocks, void *stream) {
  hipLaunchKernelGGL(kv_total, dim3(grid_for(n_words, 256, max_blocks)), dim3(256), 0, (hipStream_t)stream, mask, n_words,
                     reinterpret_cast<unsigned long long *>(total));
}

}  // namespace aha
