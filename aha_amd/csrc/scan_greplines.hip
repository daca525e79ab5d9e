// scan_greplines.hip -- context lines (aha_ac_grep_batch* with AHA_GREP_LINES; DESIGN.md 4.16 "Context lines"): the match mask m
// of grep (one bit per record, kgr_flag) dilated by `before` and `after` records inside groups of records, into the keep mask
// that rule grep's edges (kgq_edges) and grep's tail take as they are.  The excerpts passes (scan_excerpt.hip) in record space:
// a run of matching records of one group, widened by the context and clipped to its group, is the union of its records'
// windows; no pass walks along a run or a window.  The ranked masks are walked by post_common.hpp's for_ranked_bits.
//   kgl_edges        two masks over records from m alone, a lane per mask word, the neighbouring words funnelled across the
//                    wave: Sm: record r matches and r - 1 does not (or r = 0); Tm: r matches and r + 1 does not (or r + 1 = D).
//                    Whole words are written; the bits from D on are 0.
//   kgl_group_edges  a lane per inner group boundary q (0 < q < D): where q - 1 and q both match a run ends and one starts
//                    there, bit q - 1 of Tm and bit q of Sm (an OR of a bit that only ever goes up: no order can show; the
//                    boundaries of empty groups name the same q and set the same bits).
//   kgl_windows      over the ranked Sm and Tm: the j-th bits delimit run j = records [s, t].  Its group g is the last with
//                    group_offsets[g] <= s (owner_of: empty groups are stepped over), w0[j] = max(lo, s - before),
//                    w1[j] = min(hi, t + 1 + after), in 64 bits.  Without groups the one group is [0, D).
//   kgl_toggle       a lane per run: first = j is the first run, or of another group than j - 1, or w0[j] > w1[j - 1]; last =
//                    the same test seen from j + 1.  A first run XORs bit w0[j] of the toggle mask (D + 1 bits, cleared in
//                    front), a last run bit w1[j].  The chunks of one group neither overlap nor touch, so a bit is toggled
//                    twice only where a chunk ends on its group's end and the next group's chunk starts there: the two cancel,
//                    and both sides are kept -- which is what is wanted.
//   kgl_fill         a wave per rank block of the ranked toggle mask, a lane per word: the parity of the toggles in front of the
//                    word (the block's rank plus the wave's scan of the popcounts) flips the word's inclusive prefix XOR (a
//                    ladder of five shifts); record r is kept when an odd number of toggles lies at or in front of it.  Whole
//                    words of keep are written, the bits from D on 0.
//   kgl_emit_match   once the call is known to fit, over the ranked keep mask: is_match[i] = bit kept_docs[i] of m.
// Every kernel strides over its work; positions and ranks are 64-bit; every lane does O(1) work whatever the contexts are.
// Vector loads, stores and atomics and plain C++ only; no LDS.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "image.hpp"
#include "post_common.hpp"

namespace aha {
namespace {

using post::grid_for;

__global__ __launch_bounds__(256) void kgl_edges(const uint32_t *m, uint64_t n_words, uint64_t n_docs, uint32_t *Sm, uint32_t *Tm) {
  const int lane = threadIdx.x & 63;
  const uint32_t tail = (uint32_t)(n_docs & 31);
  const uint64_t wave = ((uint64_t)blockIdx.x * 256 + threadIdx.x) >> 6, n_waves = (uint64_t)gridDim.x * 4;
  for (uint64_t w0 = wave * 64; w0 < n_words; w0 += n_waves * 64) {  // (the same trips in every lane of a wave)
    const uint64_t w = w0 + lane;
    uint32_t cur = w < n_words ? m[w] : 0u;
    if (tail && w + 1 == n_words) cur &= (1u << tail) - 1u;
    uint32_t prev = __shfl_up(cur, 1, 64), next = __shfl_down(cur, 1, 64);
    if (lane == 0) prev = w0 ? m[w0 - 1] : 0u;                   // (a word in front of the last: all its bits are records)
    if (lane == 63) next = w0 + 64 < n_words ? m[w0 + 64] : 0u;  // (its bit 0 is a record: the word exists)
    if (w < n_words) {
      Sm[w] = cur & ~(cur << 1 | prev >> 31);
      Tm[w] = cur & ~(cur >> 1 | next << 31);
    }
  }
}

// goff[0 .. n_groups]: checked (first 0, ascending, last n_docs) before this runs
__global__ __launch_bounds__(256) void kgl_group_edges(const uint32_t *m, const uint64_t *goff, uint64_t n_groups, uint64_t n_docs,
                                                       uint32_t *Sm, uint32_t *Tm) {
  for (uint64_t g = (uint64_t)blockIdx.x * 256 + threadIdx.x + 1; g < n_groups; g += (uint64_t)gridDim.x * 256) {
    const uint64_t q = goff[g];
    if (q && q < n_docs && bit_at(m, q - 1) && bit_at(m, q)) {
      atomicOr(Sm + (q >> 5), 1u << (uint32_t)(q & 31));
      atomicOr(Tm + ((q - 1) >> 5), 1u << (uint32_t)((q - 1) & 31));
    }
  }
}

// blk_s / blk_t: the set bits of Sm / Tm before every block (select_launch_rank).  grp[j], w0[j], w1[j] of run j.  goff null:
// one group, [0, n_docs)
__global__ __launch_bounds__(256) void kgl_windows(const uint32_t *Sm, const uint32_t *Tm, uint64_t n_words, uint64_t n_blk,
                                                   const unsigned long long *blk_s, const unsigned long long *blk_t,
                                                   const uint64_t *goff, uint64_t n_groups, uint64_t n_docs, uint32_t before,
                                                   uint32_t after, uint64_t *grp, uint64_t *w0, uint64_t *w1) {
  for_ranked_bits(Sm, n_words, n_blk, blk_s, [&](uint64_t w, uint32_t i, uint64_t at) {
    const uint64_t s = w * 32 + i, g = goff ? owner_of(goff, n_groups, s) : 0;
    const uint64_t lo = goff ? goff[g] : 0;
    grp[at] = g;
    w0[at] = std::max<uint64_t>(lo, s - std::min<uint64_t>(s, before));
  });
  for_ranked_bits(Tm, n_words, n_blk, blk_t, [&](uint64_t w, uint32_t i, uint64_t at) {
    const uint64_t t = w * 32 + i;
    const uint64_t hi = goff ? goff[owner_of(goff, n_groups, t) + 1] : n_docs;
    w1[at] = std::min<uint64_t>(hi, t + 1 + after);
  });
}

// tog: ceil((n_docs + 1) / 32) words, clear; every chunk's two ends are toggled
__global__ __launch_bounds__(256) void kgl_toggle(const uint64_t *grp, const uint64_t *w0, const uint64_t *w1, uint64_t n_runs,
                                                  uint32_t *tog) {
  for (uint64_t j = (uint64_t)blockIdx.x * 256 + threadIdx.x; j < n_runs; j += (uint64_t)gridDim.x * 256) {
    const uint64_t g = grp[j], a = w0[j], b = w1[j];
    const bool first = j == 0 || grp[j - 1] != g || a > w1[j - 1];
    const bool last = j + 1 == n_runs || grp[j + 1] != g || w0[j + 1] > b;
    if (first) atomicXor(tog + (a >> 5), 1u << (uint32_t)(a & 31));
    if (last) atomicXor(tog + (b >> 5), 1u << (uint32_t)(b & 31));
  }
}

// blk_x: the set bits of tog before every block (select_launch_rank over n_docs + 1 bits), t_words its words, n_blk its blocks
__global__ __launch_bounds__(256) void kgl_fill(const uint32_t *tog, uint64_t t_words, uint64_t n_blk, const unsigned long long *blk_x,
                                                uint64_t n_docs, uint32_t *keep) {
  const int lane = threadIdx.x & 63;
  const uint64_t n_words = (n_docs + 31) / 32;
  const uint32_t tail = (uint32_t)(n_docs & 31);
  const uint64_t wave = ((uint64_t)blockIdx.x * 256 + threadIdx.x) >> 6, n_waves = (uint64_t)gridDim.x * 4;
  for (uint64_t b = wave; b < n_blk; b += n_waves) {  // (the same trips in every lane of a wave)
    const uint64_t w = b * kRankBlockWords + lane;
    uint32_t x = w < t_words ? tog[w] : 0u;
    const uint64_t front = blk_x[b] + wave_excl_scan((uint32_t)__popc(x));  // the toggles in front of this word
    x ^= x << 1;
    x ^= x << 2;
    x ^= x << 4;
    x ^= x << 8;
    x ^= x << 16;
    if (front & 1) x = ~x;
    if (w < n_words) {
      if (tail && w + 1 == n_words) x &= (1u << tail) - 1u;
      keep[w] = x;
    }
  }
}

// blk_k: the set bits of keep before every block.  is_match[0, n_kept)
__global__ __launch_bounds__(256) void kgl_emit_match(const uint32_t *keep, uint64_t n_words, uint64_t n_blk,
                                                      const unsigned long long *blk_k, const uint32_t *m, uint8_t *is_match) {
  for_ranked_bits(keep, n_words, n_blk, blk_k,
                  [&](uint64_t w, uint32_t i, uint64_t at) { is_match[at] = (uint8_t)((m[w] >> i) & 1u); });
}

}  // namespace

void greplines_launch_edges(const uint32_t *m, uint64_t n_docs, const uint64_t *goff, uint64_t n_groups, uint32_t *Sm, uint32_t *Tm,
                            uint32_t max_blocks, void *stream) {
  if (!n_docs) return;
  const uint64_t n_words = (n_docs + 31) / 32;
  hipLaunchKernelGGL(kgl_edges, dim3(grid_for(n_words, 256, max_blocks)), dim3(256), 0, (hipStream_t)stream, m, n_words, n_docs, Sm, Tm);
  if (goff && n_groups > 1)
    hipLaunchKernelGGL(kgl_group_edges, dim3(grid_for(n_groups - 1, 256, max_blocks)), dim3(256), 0, (hipStream_t)stream, m, goff,
                       n_groups, n_docs, Sm, Tm);
}

void greplines_launch_windows(const uint32_t *Sm, const uint32_t *Tm, uint64_t n_docs, const uint64_t *blk_s, const uint64_t *blk_t,
                              const uint64_t *goff, uint64_t n_groups, uint32_t before, uint32_t after, uint64_t n_runs, uint64_t *grp,
                              uint64_t *w0, uint64_t *w1, uint32_t *tog, uint32_t max_blocks, void *stream) {
  if (!n_runs) return;
  const uint64_t n_words = (n_docs + 31) / 32, n_blk = rank_blocks(n_docs);
  hipLaunchKernelGGL(kgl_windows, dim3(grid_for(n_blk * 64, 256, max_blocks)), dim3(256), 0, (hipStream_t)stream, Sm, Tm, n_words, n_blk,
                     reinterpret_cast<const unsigned long long *>(blk_s), reinterpret_cast<const unsigned long long *>(blk_t), goff,
                     n_groups, n_docs, before, after, grp, w0, w1);
  hipLaunchKernelGGL(kgl_toggle, dim3(grid_for(n_runs, 256, max_blocks)), dim3(256), 0, (hipStream_t)stream, grp, w0, w1, n_runs, tog);
}

void greplines_launch_fill(const uint32_t *tog, const uint64_t *blk_x, uint64_t n_docs, uint32_t *keep, uint32_t max_blocks,
                           void *stream) {
  if (!n_docs) return;
  const uint64_t t_words = (n_docs + 1 + 31) / 32, n_blk = rank_blocks(n_docs + 1);
  hipLaunchKernelGGL(kgl_fill, dim3(grid_for(n_blk * 64, 256, max_blocks)), dim3(256), 0, (hipStream_t)stream, tog, t_words, n_blk,
                     reinterpret_cast<const unsigned long long *>(blk_x), n_docs, keep);
}

void greplines_launch_emit_match(const uint32_t *keep, const uint64_t *blk_k, uint64_t n_docs, const uint32_t *m, uint8_t *is_match,
                                 uint32_t max_blocks, void *stream) {
  if (!n_docs) return;
  const uint64_t n_words = (n_docs + 31) / 32, n_blk = rank_blocks(n_docs);
  hipLaunchKernelGGL(kgl_emit_match, dim3(grid_for(n_blk * 64, 256, max_blocks)), dim3(256), 0, (hipStream_t)stream, keep, n_words, n_blk,
                     reinterpret_cast<const unsigned long long *>(blk_k), m, is_match);
}

}  // namespace aha
