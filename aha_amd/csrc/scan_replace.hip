// scan_replace.hip -- the replace path (aha_ac_replace_batch*): the substituted copy of a batch from its selection (DESIGN.md
// 4.15).  The selection of the whole batch lies in scratch (engine.cpp device_replace): sel[0, n), document by document, with
// the documents' offsets dso[0 .. D] into it.  Hit j starts at corpus byte A[j]; replacing it changes the length of everything
// behind it by delta[j]; shift[j] = the sum of the deltas in front of j.  In the output, hit j's replacement starts at
// O[j] = A[j] + shift[j], is r[j] bytes long (0 for a kept key: its bytes are gap text) and the text behind it -- the gap up to
// O[j + 1] -- comes from corpus position q - shift[j + 1].
//   krp_delta        A[j] and delta[j], one lane per selected hit; the hit's document by a binary search of j in dso.
//   krp_scan_*       delta -> shift, exclusive, signed 64-bit: block sums, one workgroup over the sums, the add.
//   krp_doc_offsets  where every document's result starts: doc_offsets[d] + shift[dso[d]]; the last entry is the total.
//   krp_copy         driven by the output: a wave owns 1024 consecutive output bytes, a lane 16 of them.  The segment of an
//                    output position q is the LAST j with O[j] <= q (deletions make ties: the earlier ones give no byte).  A
//                    tile inside one gap is a copy at a fixed distance: two aligned 16-byte loads, a byte alignment, one
//                    aligned 16-byte store per lane.  Any other tile: every lane walks the segments of its 16 bytes.
// Vector loads and stores and plain C++ only.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "image.hpp"
#include "post_common.hpp"

namespace aha {
namespace {

using post::grid_for;

constexpr int kRpScanThreads = 256;  // lanes of the one workgroup over the block sums
constexpr int kRpItems = kRpScanBlock / 256;  // items per lane of a block
constexpr uint64_t kRpTile = 1024;  // output bytes of one wave's tile: 16 per lane

__global__ __launch_bounds__(256) void krp_delta(const int32_t *sel, uint64_t n, const uint64_t *dso, const uint64_t *doc_off,
                                                 uint64_t n_docs, const RepEntry *ent, uint32_t n_keys, uint64_t *start,
                                                 long long *shift) {
  for (uint64_t j = (uint64_t)blockIdx.x * 256 + threadIdx.x; j < n; j += (uint64_t)gridDim.x * 256) {
    const int32_t s = sel[j * 3], e = sel[j * 3 + 1];
    const uint32_t v = (uint32_t)sel[j * 3 + 2];
    start[j] = doc_off[owner_of(dso, n_docs, j)] + (uint64_t)s;  // (dso[0] = 0; documents without a selection are stepped over)
    const bool keep = v >= n_keys || ent[v].keep;  // (never beyond the keys: a hit's value is a key)
    shift[j] = keep ? 0ll : (long long)ent[v].len - (long long)(e - s);
  }
}

// sums[b] = the sum of the items of block b
__global__ __launch_bounds__(256) void krp_scan_sums(const long long *x, uint64_t n, uint64_t n_blk, long long *sums) {
  __shared__ long long s_part[4];
  for (uint64_t b = blockIdx.x; b < n_blk; b += gridDim.x) {
    const uint64_t i0 = b * kRpScanBlock + (uint64_t)threadIdx.x * kRpItems;
    long long c = 0;
#pragma unroll
    for (int k = 0; k < kRpItems; k++)
      if (i0 + k < n) c += x[i0 + k];
    c = wave_sum(c);
    if ((threadIdx.x & 63) == 0) s_part[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) sums[b] = s_part[0] + s_part[1] + s_part[2] + s_part[3];
    __syncthreads();
  }
}

// sums[0, n_blk] in place: the blocks' sums -> the sum before every block, sums[n_blk] = the total.  One workgroup.
__global__ __launch_bounds__(kRpScanThreads) void krp_scan_top(long long *sums, uint64_t n_blk) {
  __shared__ long long s_sum[kRpScanThreads];
  const long long total = block_run_scan<kRpScanThreads>(
      n_blk, [&](uint64_t b) { return sums[b]; }, [&](uint64_t b, long long run) { sums[b] = run; }, s_sum);
  if (threadIdx.x == kRpScanThreads - 1) sums[n_blk] = total;
}

// x[0, n) in place: the items -> the sum of the items in front of each; x[n] = the total
__global__ __launch_bounds__(256) void krp_scan_add(long long *x, uint64_t n, uint64_t n_blk, const long long *sums) {
  __shared__ long long s_wave[4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (uint64_t b = blockIdx.x; b < n_blk; b += gridDim.x) {
    const uint64_t i0 = b * kRpScanBlock + (uint64_t)threadIdx.x * kRpItems;
    long long v[kRpItems], c = 0;
#pragma unroll
    for (int k = 0; k < kRpItems; k++) {
      v[k] = i0 + k < n ? x[i0 + k] : 0ll;
      c += v[k];
    }
    const long long incl = wave_incl_scan(c);  // the items of the lanes up to this one
    if (lane == 63) s_wave[wave] = incl;
    __syncthreads();
    long long run = sums[b] + incl - c;
    for (int w = 0; w < wave; w++) run += s_wave[w];
#pragma unroll
    for (int k = 0; k < kRpItems; k++) {
      if (i0 + k < n) x[i0 + k] = run;
      run += v[k];
    }
    __syncthreads();
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) x[n] = sums[n_blk];
}

__global__ __launch_bounds__(256) void krp_doc_offsets(const uint64_t *doc_off, const uint64_t *dso, const long long *shift,
                                                       uint64_t n_docs, uint64_t *doc_out) {
  for (uint64_t d = (uint64_t)blockIdx.x * 256 + threadIdx.x; d <= n_docs; d += (uint64_t)gridDim.x * 256)
    doc_out[d] = (uint64_t)((long long)doc_off[d] + shift[dso[d]]);
}

struct RpArgs {
  const uint8_t *text;
  const int32_t *sel;
  const uint64_t *start;
  const long long *shift;
  uint64_t n;
  const RepEntry *ent;
  uint32_t n_keys;
  const uint8_t *blob;
  uint8_t *out;
  uint64_t total;
};

// what one segment contributes: r bytes of the blob from O on, then corpus text at the distance sh_next up to next_o
struct RpSeg {
  uint64_t o, r, boff, next_o;
  long long sh_next;
};

__device__ __forceinline__ uint64_t rp_o(const RpArgs &a, uint64_t j) { return (uint64_t)((long long)a.start[j] + a.shift[j]); }

// the last j in [0, n) with O[j] <= q, -1 where there is none (q lies in front of the first selected hit)
__device__ __forceinline__ long long rp_find(const RpArgs &a, uint64_t q) {
  uint64_t lo = 0, hi = a.n;
  while (lo < hi) {
    const uint64_t mid = (lo + hi) >> 1;
    if (rp_o(a, mid) <= q)
      lo = mid + 1;
    else
      hi = mid;
  }
  return (long long)lo - 1;
}

__device__ __forceinline__ RpSeg rp_seg(const RpArgs &a, long long j) {
  RpSeg s;
  s.o = 0;
  s.r = 0;
  s.boff = 0;
  if (j >= 0) {
    const uint32_t v = (uint32_t)a.sel[j * 3 + 2];
    s.o = rp_o(a, (uint64_t)j);
    if (v < a.n_keys && !a.ent[v].keep) {  // (a kept hit is gap text)
      s.r = a.ent[v].len;
      s.boff = a.ent[v].off;
    }
  }
  const uint64_t nx = (uint64_t)(j + 1);
  s.sh_next = a.shift[nx];
  s.next_o = nx < a.n ? rp_o(a, nx) : ~0ull;
  return s;
}

// output bytes [q, q + cnt), cnt <= 16, segment by segment; one 16-byte store where the lane has all 16 at an aligned address
__device__ __forceinline__ void rp_lane(const RpArgs &a, uint64_t q, uint32_t cnt) {
  long long j = rp_find(a, q);
  RpSeg s = rp_seg(a, j);
  uint32_t w[4] = {0u, 0u, 0u, 0u};
#pragma unroll
  for (uint32_t b = 0; b < 16; b++) {
    if (b < cnt) {
      const uint64_t p = q + b;
      while (s.next_o <= p) s = rp_seg(a, ++j);  // (ties: up to the last segment that starts at or before p)
      const uint32_t c = p - s.o < s.r ? a.blob[s.boff + (p - s.o)] : a.text[(uint64_t)((long long)p - s.sh_next)];
      w[b >> 2] |= c << (8 * (b & 3));
    }
  }
  uint8_t *dst = a.out + q;
  if (cnt == 16 && (reinterpret_cast<uintptr_t>(dst) & 15) == 0) {
    *reinterpret_cast<uint4 *>(dst) = make_uint4(w[0], w[1], w[2], w[3]);
  } else {
#pragma unroll
    for (uint32_t b = 0; b < 16; b++)
      if (b < cnt) dst[b] = (uint8_t)(w[b >> 2] >> (8 * (b & 3)));
  }
}

// head: the bytes in front of the first 16-byte aligned address of out (a byte per lane of the first wave); then tiles
__global__ __launch_bounds__(256) void krp_copy(RpArgs a, uint64_t head, uint64_t n_tiles) {
  const uint32_t lane = threadIdx.x & 63;
  const uint64_t wave = (uint64_t)blockIdx.x * 4 + (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const uint64_t n_waves = (uint64_t)gridDim.x * 4;
  if (wave == 0 && lane < head) rp_lane(a, lane, 1);
  for (uint64_t t = wave; t < n_tiles; t += n_waves) {
    const uint64_t q0 = head + t * kRpTile;
    bool fast = false;
    long long sh = 0;
    if (q0 + kRpTile <= a.total) {
      const RpSeg s = rp_seg(a, rp_find(a, q0));
      fast = q0 >= s.o + s.r && s.next_o >= q0 + kRpTile;  // the whole tile lies in one gap
      sh = s.sh_next;
    }
    const uint64_t q = q0 + (uint64_t)lane * 16;
    if (fast) {
      // 16 bytes from an address of any alignment: the aligned piece that holds the first byte and, where the bytes go on
      // into it, the next one -- both hold a byte of the corpus
      const uintptr_t src = reinterpret_cast<uintptr_t>(a.text) + (uintptr_t)((long long)q - sh);
      const uint32_t k = (uint32_t)(src & 15);
      const uint4 lo = *reinterpret_cast<const uint4 *>(src - k);
      uint4 hi = make_uint4(0u, 0u, 0u, 0u);
      if (k) hi = *reinterpret_cast<const uint4 *>(src - k + 16);
      uint32_t v0, v1, v2, v3, v4;
      switch (k >> 2) {  // (k is the same in every lane of the tile)
        case 0: v0 = lo.x, v1 = lo.y, v2 = lo.z, v3 = lo.w, v4 = hi.x; break;
        case 1: v0 = lo.y, v1 = lo.z, v2 = lo.w, v3 = hi.x, v4 = hi.y; break;
        case 2: v0 = lo.z, v1 = lo.w, v2 = hi.x, v3 = hi.y, v4 = hi.z; break;
        default: v0 = lo.w, v1 = hi.x, v2 = hi.y, v3 = hi.z, v4 = hi.w; break;
      }
      const uint32_t b = k & 3;
      uint4 r;
      r.x = __builtin_amdgcn_alignbyte(v1, v0, b);
      r.y = __builtin_amdgcn_alignbyte(v2, v1, b);
      r.z = __builtin_amdgcn_alignbyte(v3, v2, b);
      r.w = __builtin_amdgcn_alignbyte(v4, v3, b);
      *reinterpret_cast<uint4 *>(a.out + q) = r;
    } else if (q < a.total) {
      rp_lane(a, q, (uint32_t)min((uint64_t)16, a.total - q));
    }
  }
}

}  // namespace

void replace_launch_delta(const void *sel, uint64_t n, const uint64_t *dso, const uint64_t *doc_off, uint64_t n_docs,
                          const RepEntry *ent, uint32_t n_keys, uint64_t *start, int64_t *shift, uint32_t max_blocks, void *stream) {
  if (!n) return;
  hipLaunchKernelGGL(krp_delta, dim3(grid_for(n, 256, max_blocks)), dim3(256), 0, (hipStream_t)stream, (const int32_t *)sel, n, dso,
                     doc_off, n_docs, ent, n_keys, start, reinterpret_cast<long long *>(shift));
}

void replace_launch_scan(int64_t *shift, uint64_t n, int64_t *sums, uint32_t max_blocks, void *stream) {
  const uint64_t n_blk = replace_scan_blocks(n);
  const uint32_t grid = grid_for(n_blk, 1, max_blocks);
  long long *x = reinterpret_cast<long long *>(shift), *sm = reinterpret_cast<long long *>(sums);
  if (n_blk) hipLaunchKernelGGL(krp_scan_sums, dim3(grid), dim3(256), 0, (hipStream_t)stream, x, n, n_blk, sm);
  hipLaunchKernelGGL(krp_scan_top, dim3(1), dim3(kRpScanThreads), 0, (hipStream_t)stream, sm, n_blk);
  hipLaunchKernelGGL(krp_scan_add, dim3(grid), dim3(256), 0, (hipStream_t)stream, x, n, n_blk, sm);
}

void replace_launch_doc_offsets(const uint64_t *doc_off, const uint64_t *dso, const int64_t *shift, uint64_t n_docs,
                                uint64_t *doc_out, uint32_t max_blocks, void *stream) {
  hipLaunchKernelGGL(krp_doc_offsets, dim3(grid_for(n_docs + 1, 256, max_blocks)), dim3(256), 0, (hipStream_t)stream, doc_off, dso,
                     reinterpret_cast<const long long *>(shift), n_docs, doc_out);
}

void replace_launch_copy(const uint8_t *text, const void *sel, const uint64_t *start, const int64_t *shift, uint64_t n,
                         const RepEntry *ent, uint32_t n_keys, const uint8_t *blob, uint8_t *out, uint64_t total,
                         uint32_t max_blocks, void *stream) {
  if (!total) return;
  const uint64_t head = std::min<uint64_t>((16 - (reinterpret_cast<uintptr_t>(out) & 15)) & 15, total);
  const uint64_t n_tiles = (total - head + kRpTile - 1) / kRpTile;
  const RpArgs a{text, (const int32_t *)sel, start, reinterpret_cast<const long long *>(shift), n, ent, n_keys, blob, out, total};
  const uint32_t grid = grid_for(n_tiles, 4, max_blocks);
  hipLaunchKernelGGL(krp_copy, dim3(grid), dim3(256), 0, (hipStream_t)stream, a, head, n_tiles);
}

}  // namespace aha
