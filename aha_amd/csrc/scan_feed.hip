// scan_feed.hip -- the feed path (aha_feed_match_batch*): sequences that arrive in pieces across calls.
//
// The state after a byte is the longest suffix of the text that is a trie path, so it -- and what is emitted there -- depends
// only on the last Lmax bytes.  With W = max(Lmax - 1, 0) and ctx = the last min(W, consumed) bytes of the sequence, the hits
// of a piece P whose end lies in P are:
//   boundary hits  the hits of X = ctx || P[0 .. min(W, |P|)) matched alone, without its first y (y = the hits of ctx alone),
//                  shifted by |ctx| (or leads(ctx) on a char feed);
//   main hits      the hits of P matched alone, without its first z (z = the hits of P[0 .. min(W, |P|)) alone).
// Both selections are by count: each document's hits are in end order, so what is dropped is a prefix.  The matches themselves
// are plain device_match calls (engine.cpp); the kernels here only check, cut the windows, merge and commit:
//   kfd_check    the piece offsets and sequence ids, before anything is indexed with them (a verdict word the host reads)
//   kfd_scan     one block: the window lengths into their offsets, or the hits per piece into piece_hit_offsets
//   kfd_windows  the window batch [X_0..X_{D-1} | ctx_0.. | P'_0..] and leads(ctx)
//   kfd_leads    leads(P) per piece (char feeds), a reduction over the pieces
//   kfd_merge    the kept hits into the caller's buffer, rebased; one thread per 4 output hits (3 x 16-byte stores)
//   kfd_commit   after success only: bases, the counters, the new contexts (written to the other bank)
// A count call (aha_feed_count_batch*) sums the same selection per key instead: per piece, as multisets of key ids,
//   hits(piece) = hits(X) - hits(ctx) + hits(P) - hits(P')        (P' = P[0 .. min(W, |P|)))
// The main pass counts the pieces (device_count) into the feed's vector kc; then
//   kfd_count_windows  kc += +1 per hit of the X block, -1 per hit of the ctx and P' blocks (uint64, wrapping), summed per
//                      workgroup in the LDS table of count_table.hpp first
//   kfd_scan           the hits per piece into piece_hit_offsets, as for a match
//   kfd_count_finish   the caller's key_counts = kc (or += kc): the first write the caller sees, after everything succeeded
// A cover call (aha_feed_cover_batch*) wants the bytes inside the piece's hits, not the hits.  The main pass covers the pieces
// alone (device_count with a mask); every event of it that ends beyond P[0 .. W') is exact (W' = min(W, |P|)), the others set
// bits only inside [0, W').  A hit that touches P[0 .. W') starts before W', so it ends at or before W' + W <= 2 W: the head
// window is widened to X2 = ctx || P[0 .. min(2 W, |P|)), whose hits with end > |ctx| are exact hits of the sequence and hold
// every hit that touches P[0 .. W') or reaches back into the context.  So
//   mask(P) = (cover(P alone) with bits [0, W') cleared) OR the spans of { h in hits(X2): end > |ctx| }, clipped to the piece
//   back(P) = max(0, |ctx| - the least start among them)
// and, with P' widened to P[0 .. min(2 W, |P|)) as well, the hits per piece are x - y + m - z as for a count.
//   kfd_cover_clear    bits [0, W') of every piece: pieces are not word-aligned and two may share a mask word
//   kfd_cover_windows  the clipped spans with atomicOr; back with a wave reduction and one atomicMax per piece and wave
// A feed with a separator filter (scan_feedsep.hip) keeps W = Lmax + 1 bytes of context -- both facts hold for any W >= Lmax - 1
// -- and its calls also want the hits that ended with the piece before, which are hits of ctx alone:
//   kfd_edge           per piece the hits of ctx alone that end on its last byte: a suffix of X's first y hits, by position
//   kfd_scan<2>        the true hits per piece with them; kfd_merge<true> puts them in front of the piece's boundary hits
// (instantiations of their own: a plain feed launches what it always launched)
#include <hip/hip_runtime.h>

#include "count_table.hpp"
#include "cover_span.hpp"
#include "feed.hpp"
#include "post_common.hpp"

namespace aha {
namespace {

using post::grid_for;

constexpr int kFdThreads = 256;
constexpr int kFdScanThreads = 1024;
constexpr uint64_t kFdSpan = 64 * 1024;  // kfd_leads: bytes per workgroup trip
constexpr uint64_t kFdCountSpan = 16 * 1024;  // kfd_count_windows: window hits per workgroup trip (at least)

__device__ __forceinline__ uint32_t is_lead(uint8_t b) { return (b & 0xC0u) != 0x80u ? 1u : 0u; }

__global__ void kfd_check(FeedArgs F) {
  uint32_t bad = 0;
  for (uint64_t d = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; d <= F.D; d += (uint64_t)gridDim.x * blockDim.x) {
    if (d == 0 && F.off[0] != 0) bad |= 1u;
    if (d == F.D) {
      if (F.off[F.D] != F.n_bytes) bad |= 1u;
      continue;
    }
    const uint64_t a = F.off[d], b = F.off[d + 1];
    if (b < a)
      bad |= 1u;
    else if (b - a >= F.max_piece)
      bad |= 2u;
    const uint32_t id = F.ids[d];
    if (id >= F.n_seqs)
      bad |= 1u;
    else if (atomicExch(&F.seqs[id].stamp, F.stamp) == F.stamp)  // named twice in this call
      bad |= 1u;
    else if (F.sel && F.sel[id].seen != F.seqs[id].bytes)  // a select call: bytes of the sequence went past its select state
      bad |= 4u;
    else if (F.tok && F.seqs[id].bytes && F.tok[id].seen != F.seqs[id].bytes)  // a token call: ... past its token state
      bad |= 16u;
    else if (F.grep && F.grep[id].seen != F.seqs[id].bytes)  // a grep call: bytes of the sequence went past its grep state
      bad |= 8u;
  }
  if (bad) atomicOr(F.verdict, bad);
}

// per-piece quantities of the two scans
__device__ __forceinline__ uint64_t win_len(const FeedArgs &F, uint64_t i) {
  const uint64_t part = i / F.D, d = i - part * F.D;
  const uint64_t lc = min((uint64_t)F.W, F.seqs[F.ids[d]].bytes);
  const uint64_t lp = min((uint64_t)F.Wp, F.off[d + 1] - F.off[d]);
  return part == 0 ? lc + lp : (part == 1 ? lc : lp);
}
__device__ __forceinline__ uint64_t kept_hits(const FeedArgs &F, uint64_t d) {
  const uint64_t D = F.D;
  const uint64_t x = F.wdho[d + 1] - F.wdho[d], y = F.wdho[D + d + 1] - F.wdho[D + d];
  const uint64_t z = F.wdho[2 * D + d + 1] - F.wdho[2 * D + d], m = F.mdho[d + 1] - F.mdho[d];
  return (x - y) + (m - z);
}
// ... of a call on a feed with a separator filter: the hits that end on the context's last byte too
__device__ __forceinline__ uint64_t true_hits(const FeedArgs &F, uint64_t d) { return kept_hits(F, d) + F.edge[d]; }
template <int kMode>
__device__ __forceinline__ uint64_t scan_item(const FeedArgs &F, uint64_t i) {
  return kMode == 0 ? win_len(F, i) : (kMode == 1 ? kept_hits(F, i) : true_hits(F, i));
}

// one block of kFdScanThreads: exclusive scan of n per-piece values into out[0..n], out[n] = the total
template <int kMode>
__global__ void __launch_bounds__(kFdScanThreads) kfd_scan(FeedArgs F) {
  __shared__ uint64_t s[kFdScanThreads];
  if (*F.verdict) return;
  const uint64_t n = kMode == 0 ? 3 * F.D : F.D;
  uint64_t *out = kMode == 0 ? F.woff : F.pho;  // (kMode 2: the true hits per piece of a call on a feed with a separator filter)
  const uint64_t total =
      block_run_scan<kFdScanThreads>(n, [&](uint64_t i) { return scan_item<kMode>(F, i); }, [&](uint64_t i, uint64_t run) { out[i] = run; }, s);
  if (threadIdx.x == kFdScanThreads - 1) {
    out[n] = total;
    if (kMode == 0) *F.win_total = total;
  }
}

__global__ void __launch_bounds__(kFdThreads) kfd_windows(FeedArgs F) {
  __shared__ uint32_t s_leads;
  const uint64_t D = F.D;
  for (uint64_t d = blockIdx.x; d < D; d += gridDim.x) {
    const uint32_t id = F.ids[d];
    const FeedSeq sq = F.seqs[id];
    const uint32_t lc = (uint32_t)min((uint64_t)F.W, sq.bytes);
    const uint32_t lp = (uint32_t)min((uint64_t)F.Wp, F.off[d + 1] - F.off[d]);
    const uint8_t *c = F.ctx + ((uint64_t)sq.bank * F.n_seqs + id) * F.W;
    const uint8_t *p = F.text + F.off[d];
    uint8_t *x = F.win + F.woff[d], *cw = F.win + F.woff[D + d], *pw = F.win + F.woff[2 * D + d];
    if (threadIdx.x == 0) s_leads = 0;
    __syncthreads();
    uint32_t leads = 0;
    for (uint32_t i = threadIdx.x; i < lc; i += kFdThreads) {
      const uint8_t b = c[i];
      x[i] = b;
      cw[i] = b;
      leads += is_lead(b);
    }
    for (uint32_t i = threadIdx.x; i < lp; i += kFdThreads) {
      const uint8_t b = p[i];
      x[lc + i] = b;
      pw[i] = b;
    }
    if (F.chars) {
      if (leads) atomicAdd(&s_leads, leads);
      __syncthreads();
      if (threadIdx.x == 0) F.lead_ctx[d] = s_leads;
    }
    __syncthreads();
  }
}

// leads(P_d) += the lead bytes of the piece within each 64 KiB span (lead_p cleared by the host)
__global__ void __launch_bounds__(kFdThreads) kfd_leads(FeedArgs F) {
  __shared__ uint32_t s_cnt;
  for (uint64_t a0 = blockIdx.x * kFdSpan; a0 < F.n_bytes; a0 += (uint64_t)gridDim.x * kFdSpan) {
    const uint64_t b = min(F.n_bytes, a0 + kFdSpan);
    uint64_t lo = 0, hi = F.D - 1;  // the last piece that starts at or before a0
    while (lo < hi) {
      const uint64_t mid = (lo + hi + 1) / 2;
      if (F.off[mid] <= a0)
        lo = mid;
      else
        hi = mid - 1;
    }
    uint64_t d = lo, a = a0;
    while (a < b) {
      while (F.off[d + 1] <= a) d++;  // (empty pieces)
      const uint64_t e = min(b, F.off[d + 1]);
      if (threadIdx.x == 0) s_cnt = 0;
      __syncthreads();
      uint32_t n = 0;
      for (uint64_t i = a + threadIdx.x; i < e; i += kFdThreads) n += is_lead(F.text[i]);
      if (n) atomicAdd(&s_cnt, n);
      __syncthreads();
      if (threadIdx.x == 0 && s_cnt) atomicAdd(&F.lead_p[d], (unsigned long long)s_cnt);
      __syncthreads();
      a = e;
    }
  }
}

// edge[d] = the hits of ctx_d alone that end on its last byte, where the piece has a byte to test them against (a feed with a
// separator filter: they are reported now).  X_d's first y hits are those of ctx_d alone, in end order: the ones with
// end = |ctx_d| are a suffix of them, found by position (such a feed is in bytes).
__global__ void __launch_bounds__(kFdThreads) kfd_edge(FeedArgs F) {
  const uint64_t D = F.D;
  for (uint64_t d = blockIdx.x * (uint64_t)kFdThreads + threadIdx.x; d < D; d += (uint64_t)gridDim.x * kFdThreads) {
    const int64_t lc = (int64_t)(F.woff[D + d + 1] - F.woff[D + d]);
    const uint64_t y = F.wdho[D + d + 1] - F.wdho[D + d];
    uint64_t e = 0;
    if (lc > 0 && F.off[d + 1] > F.off[d]) {
      const int32_t *h = F.whits + 3 * F.wdho[d];
      uint64_t lo = 0, hi = y;  // the first of the y hits with end >= lc
      while (lo < hi) {
        const uint64_t mid = (lo + hi) >> 1;
        if ((int64_t)h[3 * mid + 1] < lc)
          lo = mid + 1;
        else
          hi = mid;
      }
      e = y - lo;
    }
    F.edge[d] = e;
  }
}

// kEdge: a call on a feed with a separator filter -- the last edge[d] hits of ctx_d alone stand in front of the boundary hits
template <bool kEdge>
__global__ void __launch_bounds__(kFdThreads) kfd_merge(FeedArgs F) {
  const uint64_t D = F.D;
  const uint64_t i0 = (blockIdx.x * (uint64_t)kFdThreads + threadIdx.x) * 4;
  if (i0 >= F.total) return;
  uint64_t lo = 0, hi = D - 1;  // the last piece whose first output hit is at or before i0
  while (lo < hi) {
    const uint64_t mid = (lo + hi + 1) / 2;
    if (F.pho[mid] <= i0)
      lo = mid;
    else
      hi = mid - 1;
  }
  uint64_t d = lo;
  int32_t h[12];
  const int n = (int)min((uint64_t)4, F.total - i0);
  for (int k = 0; k < n; k++) {
    const uint64_t i = i0 + k;
    while (F.pho[d + 1] <= i) d++;
    const uint64_t j = i - F.pho[d];
    const uint64_t y = F.wdho[D + d + 1] - F.wdho[D + d];
    const uint64_t e = kEdge ? F.edge[d] : 0ull;
    const uint64_t xy = (F.wdho[d + 1] - F.wdho[d]) - y + e;
    const int32_t *src;
    int32_t sh = 0;
    if (j < xy) {  // a boundary hit: X's offsets less the context
      src = F.whits + 3 * (F.wdho[d] + y - e + j);
      sh = F.chars ? (int32_t)F.lead_ctx[d] : (int32_t)(F.woff[D + d + 1] - F.woff[D + d]);
    } else {  // a main hit: already relative to the piece
      const uint64_t z = F.wdho[2 * D + d + 1] - F.wdho[2 * D + d];
      src = F.mhits + 3 * (F.mdho[d] + z + (j - xy));
    }
    h[3 * k] = src[0] - sh;
    h[3 * k + 1] = src[1] - sh;
    h[3 * k + 2] = src[2];
  }
  int32_t *o = F.out + 3 * i0;
  if (n == 4 && (reinterpret_cast<uintptr_t>(o) & 15u) == 0) {
    uint4 *o4 = reinterpret_cast<uint4 *>(o);
    o4[0] = make_uint4(h[0], h[1], h[2], h[3]);
    o4[1] = make_uint4(h[4], h[5], h[6], h[7]);
    o4[2] = make_uint4(h[8], h[9], h[10], h[11]);
  } else {
    for (int k = 0; k < 3 * n; k++) o[k] = h[k];
  }
}

__global__ void __launch_bounds__(kFdThreads) kfd_commit(FeedArgs F) {
  __shared__ FeedSeq s_sq;
  for (uint64_t d = blockIdx.x; d < F.D; d += gridDim.x) {
    const uint32_t id = F.ids[d];
    if (threadIdx.x == 0) s_sq = F.seqs[id];
    __syncthreads();
    const FeedSeq sq = s_sq;
    const uint64_t L = F.off[d + 1] - F.off[d];
    const uint64_t lc = min((uint64_t)F.W, sq.bytes), ln = min((uint64_t)F.W, sq.bytes + L);
    const uint64_t skip = lc + L - ln;  // the new context: the last ln bytes of old context || P
    const uint8_t *old = F.ctx + ((uint64_t)sq.bank * F.n_seqs + id) * F.W;
    uint8_t *nw = F.ctx + ((uint64_t)(1u - sq.bank) * F.n_seqs + id) * F.W;
    const uint8_t *p = F.text + F.off[d];
    for (uint64_t i = threadIdx.x; i < ln; i += kFdThreads) {
      const uint64_t src = skip + i;
      nw[i] = src < lc ? old[src] : p[src - lc];
    }
    if (threadIdx.x == 0) {
      if (F.bases) F.bases[d] = F.chars ? sq.chars : sq.bytes;
      FeedSeq ns = sq;
      ns.bytes = sq.bytes + L;
      if (F.chars) ns.chars = sq.chars + F.lead_p[d];
      ns.bank = 1u - sq.bank;
      F.seqs[id] = ns;
    }
    __syncthreads();
  }
}

// kc[value] += 1 for a hit of the X block, -= 1 for one of the ctx or P' blocks.  The terms are not each non-negative per
// key, but their sum with the main pass's count is (it is the piece's count), so the wrapping uint64 sums are exact.
__global__ void __launch_bounds__(kFdThreads) kfd_count_windows(FeedArgs F) {
  __shared__ uint32_t s_id[kCtSlots];
  __shared__ unsigned long long s_cnt[kCtSlots];
  const CtTable t{s_id, s_cnt};
  ct_clear(t);
  __syncthreads();
  const uint64_t n = F.n_whits, plus = F.wdho[F.D];
  unsigned long long *kc = F.kc;
  auto spill = [kc](uint32_t id, unsigned long long v) { atomicAdd(&kc[id], v); };
  for (uint64_t i0 = blockIdx.x * (uint64_t)kFdThreads; i0 < n; i0 += (uint64_t)gridDim.x * kFdThreads) {
    const uint64_t i = i0 + threadIdx.x;
    const bool live = i < n;
    const uint32_t id = live ? (uint32_t)F.whits[3 * i + 2] : 0u;
    ct_event<true>(t, live, id, i >= plus, spill);
  }
  __syncthreads();
  for (uint32_t i = threadIdx.x; i < kCtSlots; i += kFdThreads) {
    const uint32_t id = s_id[i];
    if (id != kCtEmpty && s_cnt[i]) atomicAdd(&kc[id], s_cnt[i]);
  }
}

__global__ void __launch_bounds__(kFdThreads) kfd_count_finish(FeedArgs F) {
  for (uint64_t k = blockIdx.x * (uint64_t)kFdThreads + threadIdx.x; k < F.K; k += (uint64_t)gridDim.x * kFdThreads) {
    const uint64_t v = F.kc[k];
    F.key_counts[k] = F.accumulate ? F.key_counts[k] + v : v;
  }
}

// mask bits [off[d], off[d] + min(W, |P_d|)) = 0, a wave per piece.  The first and the last word lose only the piece's own bits
// (a neighbour's bits may stand in them); the words between are the piece's alone.
__global__ void __launch_bounds__(kFdThreads) kfd_cover_clear(FeedArgs F) {
  const int lane = threadIdx.x & 63;
  const uint64_t wave = ((uint64_t)blockIdx.x * kFdThreads + threadIdx.x) >> 6, n_waves = (uint64_t)gridDim.x * (kFdThreads / 64);
  for (uint64_t d = wave; d < F.D; d += n_waves) {
    const uint64_t a = F.off[d], b = a + min((uint64_t)F.W, F.off[d + 1] - a);
    if (a >= b) continue;
    const uint64_t w0 = a >> 5, w1 = (b - 1) >> 5;
    const uint32_t m0 = ~0u << (uint32_t)(a & 31), m1 = ~0u >> (31u - (uint32_t)((b - 1) & 31));
    for (uint64_t w = w0 + lane; w <= w1; w += 64) {
      uint32_t bits = ~0u;
      if (w == w0) bits &= m0;
      if (w == w1) bits &= m1;
      if (bits == ~0u)
        F.mask[w] = 0u;
      else
        atomicAnd(F.mask + w, ~bits);
    }
  }
}

// the hits of the X2 block that end in the piece: their spans, clipped to the piece, into the mask; back[d] = the most bytes
// one of them reaches into the context.  A lane takes a hit per trip; the hits of a wave belong to few pieces (they are in
// document order), so back costs one reduction and one atomicMax per piece and wave.
__global__ void __launch_bounds__(kFdThreads) kfd_cover_windows(FeedArgs F) {
  const uint64_t D = F.D, n = F.wdho[D];
  const int lane = threadIdx.x & 63;
  for (uint64_t i0 = blockIdx.x * (uint64_t)kFdThreads + (threadIdx.x & ~63u); i0 < n; i0 += (uint64_t)gridDim.x * kFdThreads) {
    const uint64_t i = i0 + lane;
    uint64_t d = 0;
    uint32_t bk = 0;
    if (i < n) {
      uint64_t lo = 0, hi = D - 1;  // the window whose hits hold i: the last one whose first hit is at or before i
      while (lo < hi) {
        const uint64_t mid = (lo + hi + 1) / 2;
        if (F.wdho[mid] <= i)
          lo = mid;
        else
          hi = mid - 1;
      }
      d = lo;
      const int64_t lc = (int64_t)(F.woff[D + d + 1] - F.woff[D + d]);
      const int64_t st = F.whits[3 * i], en = F.whits[3 * i + 1];
      if (en > lc) {
        const uint64_t a = F.off[d], L = F.off[d + 1] - a;
        const uint64_t s = st > lc ? (uint64_t)(st - lc) : 0ull, e = min((uint64_t)(en - lc), L);
        cover_or_global(F.mask, a + s, a + e);
        if (st < lc) bk = (uint32_t)(lc - st);
      }
    }
    if (!F.back) continue;
    unsigned long long todo = __ballot(bk != 0);
    while (todo) {
      const int lead = __ffsll(todo) - 1;
      const uint64_t dl = (uint64_t)__shfl((uint32_t)d, lead, 64) | (uint64_t)__shfl((uint32_t)(d >> 32), lead, 64) << 32;
      const bool mine = bk != 0 && d == dl;
      const uint32_t v = wave_max(mine ? bk : 0u);
      if (lane == lead) atomicMax(&F.back[dl], v);
      todo &= ~__ballot(mine);
    }
  }
}

}  // namespace

void feed_launch_check(const FeedArgs &F, void *stream) {
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(kfd_check, dim3(grid_for(F.D + 1, kFdThreads, 1024)), dim3(kFdThreads), 0, s, F);
  hipLaunchKernelGGL(kfd_scan<0>, dim3(1), dim3(kFdScanThreads), 0, s, F);
}

void feed_launch_check_only(const FeedArgs &F, void *stream) {
  hipLaunchKernelGGL(kfd_check, dim3(grid_for(F.D + 1, kFdThreads, 1024)), dim3(kFdThreads), 0, (hipStream_t)stream, F);
}

void feed_launch_windows(const FeedArgs &F, void *stream) {
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(kfd_windows, dim3(grid_for(F.D, 1, 4096)), dim3(kFdThreads), 0, s, F);
  feed_launch_leads(F, stream);
}

void feed_launch_leads(const FeedArgs &F, void *stream) {
  if (F.chars && F.n_bytes)
    hipLaunchKernelGGL(kfd_leads, dim3(grid_for(F.n_bytes, kFdSpan, 4096)), dim3(kFdThreads), 0, (hipStream_t)stream, F);
}

void feed_launch_merge(const FeedArgs &F, void *stream) {
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(kfd_scan<1>, dim3(1), dim3(kFdScanThreads), 0, s, F);
  if (F.total) {
    const uint64_t groups = (F.total + 3) / 4;
    hipLaunchKernelGGL(kfd_merge<false>, dim3((uint32_t)((groups + kFdThreads - 1) / kFdThreads)), dim3(kFdThreads), 0, s, F);
  }
}

void feed_launch_edge(const FeedArgs &F, void *stream) {
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(kfd_edge, dim3(grid_for(F.D, kFdThreads, 1024)), dim3(kFdThreads), 0, s, F);
  hipLaunchKernelGGL(kfd_scan<2>, dim3(1), dim3(kFdScanThreads), 0, s, F);
}

void feed_launch_merge_edge(const FeedArgs &F, void *stream) {
  if (!F.total) return;
  const uint64_t groups = (F.total + 3) / 4;
  hipLaunchKernelGGL(kfd_merge<true>, dim3((uint32_t)((groups + kFdThreads - 1) / kFdThreads)), dim3(kFdThreads), 0,
                     (hipStream_t)stream, F);
}

void feed_launch_count(const FeedArgs &F, void *stream) {
  hipStream_t s = (hipStream_t)stream;
  if (F.kc && F.n_whits)
    hipLaunchKernelGGL(kfd_count_windows, dim3(grid_for(F.n_whits, kFdCountSpan, 1024)), dim3(kFdThreads), 0, s, F);
  hipLaunchKernelGGL(kfd_scan<1>, dim3(1), dim3(kFdScanThreads), 0, s, F);
  if (F.key_counts && F.K)
    hipLaunchKernelGGL(kfd_count_finish, dim3(grid_for(F.K, kFdThreads, 1024)), dim3(kFdThreads), 0, s, F);
}

void feed_launch_cover(const FeedArgs &F, void *stream) {
  hipStream_t s = (hipStream_t)stream;
  if (F.W && F.n_bytes) hipLaunchKernelGGL(kfd_cover_clear, dim3(grid_for(F.D * 64, kFdThreads, 4096)), dim3(kFdThreads), 0, s, F);
  if (F.n_whits)
    hipLaunchKernelGGL(kfd_cover_windows, dim3(grid_for(F.n_whits, 4 * kFdThreads, 1024)), dim3(kFdThreads), 0, s, F);
  hipLaunchKernelGGL(kfd_scan<1>, dim3(1), dim3(kFdScanThreads), 0, s, F);
}

void feed_launch_commit(const FeedArgs &F, void *stream) {
  hipLaunchKernelGGL(kfd_commit, dim3(grid_for(F.D, 1, 4096)), dim3(kFdThreads), 0, (hipStream_t)stream, F);
}
}  // namespace aha
