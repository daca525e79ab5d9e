// scan_feedsep.hip -- the separator filter of a feed (aha_feed_open_params with sep_size > 0; feed.cpp).
//
// The reference's filter (src/aha/ac.cr:321-340) is a predicate on each hit of the unfiltered list: with pass(c) = c >= sep_size
// || sep[c], a hit {start, end} of a sequence T survives when (end == |T| || pass(T[end])) && (start == 0 || pass(T[start - 1])).
// The byte behind a hit that ends with a piece is not there yet, so such a feed reports a hit one byte late: a call that takes a
// sequence from n0 to n1 bytes reports the survivors with end in [n0, n1).  Its context is W = Lmax + 1 bytes wide, so a hit
// that ended with the piece before is a hit of the context alone and its left neighbour lies in the context too; kfd_merge
// (scan_feed.hip, kEdge) puts those in front of every piece's true hits.  The kernels here take that list, relative to the piece
// (end in [0, |P|], start down to -Lmax):
//   kfp_flag          one bit per true hit: end < |P|, the byte at `end` passes, and the byte at start - 1 -- in the piece, or in
//                     the sequence's context bank for a negative index -- passes or the hit starts the sequence.  A lane per
//                     hit, a ballot per wave, one 64-bit store per 64 hits: no atomics, no clear in front
//   (select_launch_rank, scan_select.hip: the kept hits before every rank block of 2048, the total behind them -- the host's capacity check)
//   kfp_compact       the kept hits into the caller's buffer in the order of the list: a lane per true hit, a wave per mask word
//   (select_launch_rank_docs: piece_hit_offsets = the rank at every piece's first true hit)
//   kfp_count         a count call: the kept hits' values into the feed's K-word vector, summed per workgroup in the LDS table
//                     of count_table.hpp first; kfp_count_finish then writes the caller's key_counts (or adds into them)
// A finish call (aha_feed_finish_batch*) names sequences that end here: their contexts are matched as documents (the window
// batch of a call of empty pieces), kfp_flag_finish keeps the hits that end on the context's last byte and pass on the left,
// kfp_compact<true> rebases them to the sequence's end (end = 0, start = -len), kfp_restart gives the lengths as bases and
// sets the sequences back to length 0.  Every store is a vector store; every grid is bounded and its kernel strides.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "count_table.hpp"
#include "feed.hpp"
#include "fold.hpp"
#include "post_common.hpp"

namespace aha {
namespace {

using post::grid_for;

constexpr int kFpThreads = 256;

__device__ __forceinline__ bool fp_pass(const FeedSepArgs &P, uint8_t c) {
  const uint32_t b = P.fold ? fold8(c) : c;
  return !((P.blocked[b >> 5] >> (b & 31u)) & 1u);
}

__global__ void __launch_bounds__(kFpThreads) kfp_flag(FeedArgs F, FeedSepArgs P) {
  const int lane = threadIdx.x & 63;
  const uint64_t n = P.n_true;
  for (uint64_t i0 = blockIdx.x * (uint64_t)kFpThreads + (threadIdx.x & ~63u); i0 < n; i0 += (uint64_t)gridDim.x * kFpThreads) {
    const uint64_t i = i0 + lane;
    const uint64_t d0 = owner_of(P.tho, F.D, i0);  // (the wave's hits lie in few pieces: one search serves the lanes of the first)
    bool keep = false;
    if (i < n) {
      const uint64_t d = i < P.tho[d0 + 1] ? d0 : owner_of(P.tho, F.D, i);
      const uint64_t a = F.off[d], L = F.off[d + 1] - a;
      const int64_t st = P.hits[3 * i], en = P.hits[3 * i + 1];
      if (en >= 0 && (uint64_t)en < L && fp_pass(P, F.text[a + (uint64_t)en])) {
        const uint32_t id = F.ids[d];
        const FeedSeq sq = F.seqs[id];
        const int64_t lc = (int64_t)min((uint64_t)F.W, sq.bytes);
        const int64_t left = st - 1;
        if (left >= 0) {
          keep = (uint64_t)left < L && fp_pass(P, F.text[a + (uint64_t)left]);
        } else if ((int64_t)sq.bytes + st == 0) {
          keep = true;  // the hit starts the sequence
        } else if (lc + left >= 0) {
          keep = fp_pass(P, F.ctx[((uint64_t)sq.bank * F.n_seqs + id) * F.W + (uint64_t)(lc + left)]);
        }
      }
    }
    const unsigned long long m = __ballot(keep);
    if (lane == 0) P.keep[i0 >> 6] = m;
  }
}

// the hits of the X block of a window batch of empty pieces: X_d = the context of sequence ids[d]
__global__ void __launch_bounds__(kFpThreads) kfp_flag_finish(FeedArgs F, FeedSepArgs P) {
  const int lane = threadIdx.x & 63;
  const uint64_t n = P.n_true;
  for (uint64_t i0 = blockIdx.x * (uint64_t)kFpThreads + (threadIdx.x & ~63u); i0 < n; i0 += (uint64_t)gridDim.x * kFpThreads) {
    const uint64_t i = i0 + lane;
    const uint64_t d0 = owner_of(P.tho, F.D, i0);  // (the wave's hits lie in few pieces: one search serves the lanes of the first)
    bool keep = false;
    if (i < n) {
      const uint64_t d = i < P.tho[d0 + 1] ? d0 : owner_of(P.tho, F.D, i);
      const uint64_t w0 = F.woff[d];
      const int64_t lc = (int64_t)(F.woff[d + 1] - w0);
      const int64_t st = P.hits[3 * i], en = P.hits[3 * i + 1];
      if (en == lc && st >= 0 && st < en) {
        if (st > 0)
          keep = fp_pass(P, F.win[w0 + (uint64_t)(st - 1)]);
        else
          keep = F.seqs[F.ids[d]].bytes == (uint64_t)lc;  // the context is the whole sequence: the hit starts it
      }
    }
    const unsigned long long m = __ballot(keep);
    if (lane == 0) P.keep[i0 >> 6] = m;
  }
}

// kFinish: the kept hits all end on their context's last byte, the sequence's end: relative to it.  A lane per true hit, a wave
// per 64-bit word of the mask: the kept hits in front of the word are the rank block's count and the set bits of the block's
// words before it (a block is 32 such words), so the loads and the stores of a wave are contiguous.
template <bool kFinish>
__global__ void __launch_bounds__(kFpThreads) kfp_compact(FeedSepArgs P) {
  const int lane = threadIdx.x & 63;
  const uint64_t n = P.n_true;
  for (uint64_t i0 = blockIdx.x * (uint64_t)kFpThreads + (threadIdx.x & ~63u); i0 < n; i0 += (uint64_t)gridDim.x * kFpThreads) {
    const uint64_t w = i0 >> 6;
    const unsigned long long m = P.keep[w];
    if (!m) continue;  // (wave-uniform)
    const uint64_t b = w / (kRankBlockWords / 2), w0 = b * (kRankBlockWords / 2);
    const uint32_t c = wave_sum((lane < (int)(kRankBlockWords / 2) && w0 + (uint64_t)lane < w) ? (uint32_t)__popcll(P.keep[w0 + lane]) : 0u);
    if ((m >> lane) & 1ull) {
      const uint64_t i = i0 + lane;
      const uint64_t at = P.blk[b] + c + (uint64_t)__popcll(m & ((1ull << lane) - 1ull));
      const int32_t st = P.hits[3 * i], en = P.hits[3 * i + 1], v = P.hits[3 * i + 2];
      P.out[3 * at] = kFinish ? st - en : st;
      P.out[3 * at + 1] = kFinish ? 0 : en;
      P.out[3 * at + 2] = v;
    }
  }
}

__global__ void __launch_bounds__(kFpThreads) kfp_count(FeedArgs F, FeedSepArgs P) {
  __shared__ uint32_t s_id[kCtSlots];
  __shared__ unsigned long long s_cnt[kCtSlots];
  const CtTable t{s_id, s_cnt};
  ct_clear(t);
  __syncthreads();
  const uint64_t n = P.n_true;
  const uint32_t K = F.K;
  unsigned long long *kc = F.kc;
  auto spill = [kc](uint32_t id, unsigned long long v) { atomicAdd(&kc[id], v); };
  for (uint64_t i0 = blockIdx.x * (uint64_t)kFpThreads; i0 < n; i0 += (uint64_t)gridDim.x * kFpThreads) {
    const uint64_t i = i0 + threadIdx.x;
    uint32_t id = 0;
    bool live = i < n && ((P.keep[i >> 6] >> (i & 63)) & 1ull);
    if (live) {
      id = (uint32_t)P.hits[3 * i + 2];
      live = id < K;
    }
    ct_event<false>(t, live, id, false, spill);
  }
  __syncthreads();
  for (uint32_t i = threadIdx.x; i < kCtSlots; i += kFpThreads) {
    const uint32_t id = s_id[i];
    if (id != kCtEmpty && s_cnt[i]) atomicAdd(&kc[id], s_cnt[i]);
  }
}

__global__ void __launch_bounds__(kFpThreads) kfp_count_finish(FeedArgs F) {
  for (uint64_t k = blockIdx.x * (uint64_t)kFpThreads + threadIdx.x; k < F.K; k += (uint64_t)gridDim.x * kFpThreads) {
    const uint64_t v = F.kc[k];
    F.key_counts[k] = F.accumulate ? F.key_counts[k] + v : v;
  }
}

// (a sequence of length 0 has an empty context: only the counters are cleared, as aha_feed_reset does)
__global__ void __launch_bounds__(kFpThreads) kfp_restart(FeedArgs F, FeedSepArgs P) {
  for (uint64_t d = blockIdx.x * (uint64_t)kFpThreads + threadIdx.x; d < F.D; d += (uint64_t)gridDim.x * kFpThreads) {
    const uint32_t id = F.ids[d];
    if (P.bases) P.bases[d] = F.seqs[id].bytes;
    F.seqs[id].bytes = 0;
    F.seqs[id].chars = 0;
  }
}

}  // namespace

void feedsep_launch_flag(const FeedArgs &F, const FeedSepArgs &P, uint32_t max_blocks, void *stream) {
  hipLaunchKernelGGL(kfp_flag, dim3(grid_for(P.n_true, kFpThreads, max_blocks)), dim3(kFpThreads), 0, (hipStream_t)stream, F, P);
}

void feedsep_launch_flag_finish(const FeedArgs &F, const FeedSepArgs &P, uint32_t max_blocks, void *stream) {
  hipLaunchKernelGGL(kfp_flag_finish, dim3(grid_for(P.n_true, kFpThreads, max_blocks)), dim3(kFpThreads), 0, (hipStream_t)stream, F, P);
}

void feedsep_launch_compact(const FeedSepArgs &P, bool finish, uint32_t max_blocks, void *stream) {
  const dim3 grid(grid_for(P.n_true, kFpThreads, max_blocks));
  if (finish)
    hipLaunchKernelGGL(kfp_compact<true>, grid, dim3(kFpThreads), 0, (hipStream_t)stream, P);
  else
    hipLaunchKernelGGL(kfp_compact<false>, grid, dim3(kFpThreads), 0, (hipStream_t)stream, P);
}

void feedsep_launch_count(const FeedArgs &F, const FeedSepArgs &P, uint32_t max_blocks, void *stream) {
  // (a table of 48 KiB per workgroup: at least 16 Ki hits each)
  const uint32_t grid = grid_for(P.n_true, 16384, std::min<uint32_t>(max_blocks, 1024u));
  hipLaunchKernelGGL(kfp_count, dim3(grid), dim3(kFpThreads), 0, (hipStream_t)stream, F, P);
}

void feedsep_launch_count_finish(const FeedArgs &F, uint32_t max_blocks, void *stream) {
  hipLaunchKernelGGL(kfp_count_finish, dim3(grid_for(F.K, kFpThreads, std::min<uint32_t>(max_blocks, 1024u))), dim3(kFpThreads), 0, (hipStream_t)stream, F);
}

void feedsep_launch_restart(const FeedArgs &F, const FeedSepArgs &P, void *stream) {
  hipLaunchKernelGGL(kfp_restart, dim3(grid_for(F.D, kFpThreads, 1024u)), dim3(kFpThreads), 0, (hipStream_t)stream, F, P);
}

}  // namespace aha
