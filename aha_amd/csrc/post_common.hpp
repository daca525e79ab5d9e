// post_common.hpp -- the idioms the post passes share: the scans and sums over a wave, the scan of one workgroup over a short
// table, the owner search in an offset table, the walk over a ranked bit mask, and the launch grid.  One definition of each;
// a new family of passes uses these and brings no copy of its own ("Shared helpers of the post passes").
// devcommon.hpp includes this header for the wave section, so the engines and the post passes scan a wave with the same code.
// Vector loads, stores and atomics and plain C++ only.  Library-internal.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

namespace aha {

// --------------------------------------------------------------------- wave
// Every lane of the wave must reach these calls together: a cross-lane read from an inactive lane is undefined.
template <typename T>
__device__ __forceinline__ T wave_incl_scan(T v) {
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    T o = __shfl_up(v, d, 64);
    if (lane >= d) v += o;
  }
  return v;
}

// 32-bit scans over the wave with DPP moves instead of six trips through the LDS crossbar (__shfl_up is ds_bpermute):
// row_shr 1, 2, 4, 8 scan each row of 16 lanes; row_bcast15 adds the last lane of rows 0 / 2 to rows 1 / 3, row_bcast31 the
// last lane of row 1 to rows 2 and 3.  A lane without a source (or in a row the mask leaves out) receives `old`, the
// operation's identity.
#define AHA_DPP_SCAN(V, ID, OP)                                                                   \
  V = OP(V, (uint32_t)__builtin_amdgcn_update_dpp((int)(ID), (int)(V), 0x111, 0xf, 0xf, false)); \
  V = OP(V, (uint32_t)__builtin_amdgcn_update_dpp((int)(ID), (int)(V), 0x112, 0xf, 0xf, false)); \
  V = OP(V, (uint32_t)__builtin_amdgcn_update_dpp((int)(ID), (int)(V), 0x114, 0xf, 0xf, false)); \
  V = OP(V, (uint32_t)__builtin_amdgcn_update_dpp((int)(ID), (int)(V), 0x118, 0xf, 0xf, false)); \
  V = OP(V, (uint32_t)__builtin_amdgcn_update_dpp((int)(ID), (int)(V), 0x142, 0xa, 0xf, false)); \
  V = OP(V, (uint32_t)__builtin_amdgcn_update_dpp((int)(ID), (int)(V), 0x143, 0xc, 0xf, false));
__device__ __forceinline__ uint32_t dpp_op_add(uint32_t a, uint32_t b) { return a + b; }
__device__ __forceinline__ uint32_t dpp_op_max(uint32_t a, uint32_t b) { return a > b ? a : b; }
__device__ __forceinline__ uint32_t wave_incl_scan(uint32_t v) {
  AHA_DPP_SCAN(v, 0u, dpp_op_add)
  return v;
}
__device__ __forceinline__ uint32_t wave_incl_scan_max(uint32_t v) {
  AHA_DPP_SCAN(v, 0u, dpp_op_max)
  return v;
}
// lane i <- lane i - 1 (lane 0 <- first), lane 63's value for everyone
__device__ __forceinline__ uint32_t wave_shr1(uint32_t v, uint32_t first) {
  return (uint32_t)__builtin_amdgcn_update_dpp((int)first, (int)v, 0x138, 0xf, 0xf, false);
}
__device__ __forceinline__ uint32_t wave_last(uint32_t v) { return (uint32_t)__builtin_amdgcn_readlane((int)v, 63); }

// the values of the lanes in front of this one (the DPP scan for uint32_t, the generic one for 64-bit and signed values)
template <typename T>
__device__ __forceinline__ T wave_excl_scan(T v) {
  return wave_incl_scan(v) - v;
}
// the sum (the maximum) over the wave, in every lane: a butterfly, or for uint32_t the DPP scan's last lane
template <typename T>
__device__ __forceinline__ T wave_sum(T v) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
  return v;
}
__device__ __forceinline__ uint32_t wave_sum(uint32_t v) { return wave_last(wave_incl_scan(v)); }
__device__ __forceinline__ uint32_t wave_max(uint32_t v) { return wave_last(wave_incl_scan_max(v)); }

// -------------------------------------------------------------------- owner
// the largest d in [0, n) with off[d] - sub <= x.  off ascends and off[0] - sub <= x (0 comes back where n < 2); equal
// entries -- documents without a hit, pieces that stage nothing -- are stepped over: the last of them owns x
__device__ __forceinline__ uint64_t owner_of(const uint64_t *off, uint64_t n, uint64_t x, uint64_t sub = 0) {
  uint64_t lo = 1, hi = n;
  while (lo < hi) {
    const uint64_t mid = (lo + hi) >> 1;
    if (off[mid] - sub <= x)
      lo = mid + 1;
    else
      hi = mid;
  }
  return lo - 1;
}

// ----------------------------------------------------------- workgroup scan
// The exclusive scan of items [0, n) by one workgroup of THREADS lanes (lds: THREADS words of LDS): lane t owns the run
// [min(n, t per), min(n, t per + per)), per = ceil(n / THREADS); the runs' sums are scanned in LDS (Hillis-Steele).  item(i)
// is the value of item i, put(i, run) stores the sum of the items in front of i; the total comes back in every lane.  item
// is called twice per index, by the same lane, the second time in front of put(i, ..): it is a function of i alone, what it
// writes on the side it writes twice, and put may overwrite what item(i) reads.
template <int THREADS, typename T, class Item, class Put>
__device__ __forceinline__ T block_run_scan(uint64_t n, Item item, Put put, T *lds) {
  const uint64_t per = (n + THREADS - 1) / THREADS;
  const uint64_t i0 = min(n, (uint64_t)threadIdx.x * per), i1 = min(n, i0 + per);
  T mine = 0;
  for (uint64_t i = i0; i < i1; i++) mine += item(i);
  lds[threadIdx.x] = mine;
  __syncthreads();
  for (int k = 1; k < THREADS; k <<= 1) {
    const T v = (int)threadIdx.x >= k ? lds[threadIdx.x - k] : T(0);
    __syncthreads();
    lds[threadIdx.x] += v;
    __syncthreads();
  }
  T run = lds[threadIdx.x] - mine;
  for (uint64_t i = i0; i < i1; i++) {
    const T c = item(i);
    put(i, run);
    run += c;
  }
  return lds[THREADS - 1];
}

// ------------------------------------------------------------- ranked masks
// A bit mask in 32-bit words is ranked in blocks of kRankBlockWords words -- a wave, a word per lane: blk[b] = the set bits in
// front of block b, blk[rank_blocks(n_bits)] = the total (select_launch_rank).
constexpr uint32_t kRankBlockWords = 64;
constexpr uint64_t rank_blocks(uint64_t n_bits) { return ((n_bits + 31) / 32 + kRankBlockWords - 1) / kRankBlockWords; }

__device__ __forceinline__ bool bit_at(const uint32_t *mask, uint64_t p) { return (mask[p >> 5] >> (uint32_t)(p & 31)) & 1u; }

// f(w, i, rank) for every set bit of words[0, n_words), i the bit's index in word w and rank the set bits in front of it: a
// wave per rank block, the waves of the grid (workgroups of THREADS lanes) stride over the n_blk blocks
template <int THREADS = 256, class F>
__device__ __forceinline__ void for_ranked_bits(const uint32_t *words, uint64_t n_words, uint64_t n_blk, const unsigned long long *blk,
                                                F f) {
  const int lane = threadIdx.x & 63;
  const uint64_t wave = ((uint64_t)blockIdx.x * THREADS + threadIdx.x) >> 6, n_waves = (uint64_t)gridDim.x * (THREADS / 64);
  for (uint64_t b = wave; b < n_blk; b += n_waves) {
    const uint64_t w = b * kRankBlockWords + lane;
    uint32_t bits = w < n_words ? words[w] : 0u;
    uint64_t at = blk[b] + wave_excl_scan((uint32_t)__popc(bits));
    while (bits) {
      const uint32_t i = (uint32_t)__ffs(bits) - 1u;
      bits &= bits - 1u;
      f(w, i, at++);
    }
  }
}

// The same walk with the lanes strided over the RANKS of a block instead of owning a word each: in every trip the wave's lanes
// hold 64 consecutive ranks, so what f stores at out[rank] is stored side by side -- for passes that write a row per set bit of
// a dense mask, where a lane that walks its own word's bits scatters the wave's stores over 64 places.  The block's words and
// their exclusive counts go through LDS (lds: 128 words per wave of the workgroup); the word of rank j is the last whose
// count is at most j, the bit its (j - count)-th set one.  Only the waves of a workgroup that reach a block touch their part
// of lds: wave-level ordering, no workgroup barrier.
template <int THREADS = 256, class F>
__device__ __forceinline__ void for_ranked_slots(const uint32_t *words, uint64_t n_words, uint64_t n_blk, const unsigned long long *blk,
                                                 uint32_t *lds, F f) {
  const int lane = threadIdx.x & 63;
  uint32_t *w_bits = lds + (threadIdx.x >> 6) * (2 * kRankBlockWords), *w_pre = w_bits + kRankBlockWords;
  const uint64_t wave = ((uint64_t)blockIdx.x * THREADS + threadIdx.x) >> 6, n_waves = (uint64_t)gridDim.x * (THREADS / 64);
  for (uint64_t b = wave; b < n_blk; b += n_waves) {
    const uint64_t w = b * kRankBlockWords + lane;
    const uint32_t bits = w < n_words ? words[w] : 0u;
    const uint32_t incl = wave_incl_scan((uint32_t)__popc(bits));
    const uint32_t n = wave_last(incl);
    w_bits[lane] = bits;
    w_pre[lane] = incl - (uint32_t)__popc(bits);
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    const uint64_t base = blk[b];
    for (uint32_t j = (uint32_t)lane; j < n; j += 64) {
      uint32_t l = 0;
#pragma unroll
      for (uint32_t step = kRankBlockWords / 2; step; step >>= 1)
        if (w_pre[l + step] <= j) l += step;
      const uint32_t word = w_bits[l];
      uint32_t k = j - w_pre[l], i = 0;
#pragma unroll
      for (uint32_t step = 16; step; step >>= 1) {  // the k-th set bit of word: the half that holds it, five times
        const uint32_t c = (uint32_t)__popc((word >> i) & ((1u << step) - 1u));
        if (k >= c) {
          k -= c;
          i += step;
        }
      }
      f(b * kRankBlockWords + l, i, base + j);
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();  // (the next block's words overwrite these)
  }
}

// --------------------------------------------------------------------- host
// the workgroups of a launch whose kernel strides: ceil(units / per_block), at least 1, at most cap.  (In a namespace of its
// own: scan_v2.hip, which sees this header through devcommon.hpp, has a grid_for of its own with other parameter types; the
// post passes say `using post::grid_for`.)
namespace post {
inline uint32_t grid_for(uint64_t units, uint64_t per_block, uint32_t cap) {
  return (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>((units + per_block - 1) / per_block, cap));
}
}  // namespace post

}  // namespace aha
