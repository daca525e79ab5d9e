// scan_feedgrep.hip -- the feed grep path (aha_feed_grep_batch*; DESIGN.md 4.10 "Feed grep"): the lines of sequences that arrive
// in pieces, kept when they have a hit.
//
// The pieces of a call are split into fragments as a records call splits documents (scan_grep.hip).  A fragment that begins a
// record is matched from the root as that record is: its own count is exact.  Only a piece's first fragment can continue a
// record that earlier pieces left open, and "the hits of a record" are those of the record AS ITS OWN DOCUMENT -- neither the
// hits of the sequence that lie in it nor the fragment's own.  The feed's two facts (scan_feed.hip) hold for any sequence, so
// they are applied to the record as the sequence: with W = max(Lmax - 1, 0), c = min(W, open_len), e0 = the first fragment's
// length, g = min(W, e0) and ctx = the sequence's context (whose last c bytes are the record's last c bytes),
//   X = ctx[-c:] || P[0 .. g),  Y = ctx[-c:],  Z = P[0 .. g)
//   has(first fragment's record) = open_hit  ||  hits(X) - hits(Y) > 0  ||  hits(fragment) - hits(Z) > 0
// each of X, Y, Z and the fragment matched as its own document (device_count; what is dropped is a prefix, so counts do).
//   kfg_layout    one block: c and g per piece, the window batch's offsets [X_0.. | Y_0.. | Z_0..] (empty windows where no
//                 record is open or the piece is empty), the batch's size
//   kfg_windows   a workgroup per piece: the windows' bytes from the sequence's context bank and the piece
//   kfg_has       a lane per fragment: closed (its last byte is the delimiter, or FINAL), has (its own count), keep
//   kfg_first     a lane per piece: has and keep of the first fragment of a piece with an open record, by the formula above
//   kfg_flag      a lane per fragment: scan_grep.hip kgr_flag's three ballot masks (keep, S, T) from the flags; an open tail
//                 counts as dropped
//   kfg_commit    a lane per piece, behind kfd_commit, after success only: piece_head, piece_hold, piece_rec_bases and the new
//                 state; under FINAL the sequence starts again from length 0
// Vector loads and stores and plain C++ only; every grid is bounded and strides.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "feed.hpp"
#include "post_common.hpp"

namespace aha {
namespace {

using post::grid_for;

constexpr int kFgThreads = 256;
constexpr int kFgScanThreads = 1024;
constexpr uint8_t kFgKeep = 1, kFgHas = 2, kFgClosed = 4;

// the length of window i of the batch: i / D = 0: X_d, 1: Y_d, 2: Z_d
__device__ __forceinline__ uint64_t fg_win_len(const FeedArgs &F, const FeedGrepArgs &G, uint64_t i) {
  const uint64_t part = i / F.D, d = i - part * F.D;
  const uint32_t id = F.ids[d];
  const uint64_t open = G.gseq[id].open_len, L = F.off[d + 1] - F.off[d];
  if (!open || !L) return 0;
  const uint64_t c = min(min((uint64_t)F.W, open), F.seqs[id].bytes);  // (open <= bytes: the record is a suffix of the sequence)
  const uint64_t j = G.pro[d], g = min((uint64_t)F.W, G.frag[j + 1] - G.frag[j]);
  return part == 0 ? c + g : (part == 1 ? c : g);
}

// one block: the exclusive scan of the 3 D window lengths into F.woff[0 .. 3 D], the total into *F.win_total too
__global__ void __launch_bounds__(kFgScanThreads) kfg_layout(FeedArgs F, FeedGrepArgs G) {
  __shared__ uint64_t s[kFgScanThreads];
  const uint64_t n = 3 * F.D;
  const uint64_t total =
      block_run_scan<kFgScanThreads>(n, [&](uint64_t i) { return fg_win_len(F, G, i); }, [&](uint64_t i, uint64_t run) { F.woff[i] = run; }, s);
  if (threadIdx.x == kFgScanThreads - 1) {
    F.woff[n] = total;
    *F.win_total = total;
  }
}

__global__ void __launch_bounds__(kFgThreads) kfg_windows(FeedArgs F, FeedGrepArgs G) {
  const uint64_t D = F.D;
  for (uint64_t d = blockIdx.x; d < D; d += gridDim.x) {
    const uint32_t c = (uint32_t)(F.woff[D + d + 1] - F.woff[D + d]), g = (uint32_t)(F.woff[2 * D + d + 1] - F.woff[2 * D + d]);
    if (!c && !g) continue;  // (the same in every lane)
    const uint32_t id = F.ids[d];
    const FeedSeq sq = F.seqs[id];
    const uint32_t lc = (uint32_t)min((uint64_t)F.W, sq.bytes);  // the context's bytes; c <= lc
    const uint8_t *ctx = F.ctx + ((uint64_t)sq.bank * F.n_seqs + id) * F.W + (lc - c);
    const uint8_t *p = F.text + F.off[d];
    uint8_t *x = F.win + F.woff[d], *y = F.win + F.woff[D + d], *z = F.win + F.woff[2 * D + d];
    for (uint32_t i = threadIdx.x; i < c; i += kFgThreads) {
      const uint8_t b = ctx[i];
      x[i] = b;
      y[i] = b;
    }
    for (uint32_t i = threadIdx.x; i < g; i += kFgThreads) {
      const uint8_t b = p[i];
      x[c + i] = b;
      z[i] = b;
    }
  }
}

__global__ void __launch_bounds__(kFgThreads) kfg_has(FeedArgs F, FeedGrepArgs G) {
  for (uint64_t j = blockIdx.x * (uint64_t)kFgThreads + threadIdx.x; j < G.R; j += (uint64_t)gridDim.x * kFgThreads) {
    const bool closed = G.final || F.text[G.frag[j + 1] - 1] == (uint8_t)G.delim;  // (a fragment is never empty)
    const bool has = G.fdho[j + 1] > G.fdho[j];
    G.flag[j] = (uint8_t)((closed && has != (G.invert != 0) ? kFgKeep : 0) | (has ? kFgHas : 0) | (closed ? kFgClosed : 0));
  }
}

__global__ void __launch_bounds__(kFgThreads) kfg_first(FeedArgs F, FeedGrepArgs G) {
  const uint64_t D = F.D;
  for (uint64_t d = blockIdx.x * (uint64_t)kFgThreads + threadIdx.x; d < D; d += (uint64_t)gridDim.x * kFgThreads) {
    const FeedGrepSeq q = G.gseq[F.ids[d]];
    if (!q.open_len || F.off[d + 1] == F.off[d]) continue;
    const uint64_t j = G.pro[d];
    const uint64_t x = F.wdho[d + 1] - F.wdho[d], y = F.wdho[D + d + 1] - F.wdho[D + d];
    const uint64_t z = F.wdho[2 * D + d + 1] - F.wdho[2 * D + d], m = G.fdho[j + 1] - G.fdho[j];
    const bool has = q.open_hit || x > y || m > z;
    const bool closed = (G.flag[j] & kFgClosed) != 0;
    G.flag[j] = (uint8_t)((closed && has != (G.invert != 0) ? kFgKeep : 0) | (has ? kFgHas : 0) | (closed ? kFgClosed : 0));
  }
}

// keep / S / T: ceil(R / 32) words each, whole words are written (scan_grep.hip kgr_flag, from the flags)
__global__ void __launch_bounds__(kFgThreads) kfg_flag(FeedGrepArgs G) {
  const int lane = threadIdx.x & 63;
  const uint64_t R = G.R, n_words = (R + 31) / 32;
  const uint64_t wave = ((uint64_t)blockIdx.x * kFgThreads + threadIdx.x) >> 6, n_waves = (uint64_t)gridDim.x * (kFgThreads / 64);
  for (uint64_t j0 = wave * 64; j0 < R; j0 += n_waves * 64) {  // (the same trips in every lane of a wave)
    const uint64_t j = j0 + lane;
    bool k = false, s = false, t = false;
    if (j < R) {
      k = (G.flag[j] & kFgKeep) != 0;
      if (!k) {
        s = j == 0 || (G.flag[j - 1] & kFgKeep) != 0;
        t = j + 1 == R || (G.flag[j + 1] & kFgKeep) != 0;
      }
    }
    const unsigned long long bk = __ballot(k), bs = __ballot(s), bt = __ballot(t);
    const uint64_t w = j0 / 32 + lane;
    if (lane < 2 && w < n_words) {
      G.keep[w] = (uint32_t)(bk >> (32 * lane));
      G.S[w] = (uint32_t)(bs >> (32 * lane));
      G.T[w] = (uint32_t)(bt >> (32 * lane));
    }
  }
}

// behind kfd_commit: F.seqs[id].bytes is n1 already, the grep state is still the one the call found
__global__ void __launch_bounds__(kFgThreads) kfg_commit(FeedArgs F, FeedGrepArgs G) {
  for (uint64_t d = blockIdx.x * (uint64_t)kFgThreads + threadIdx.x; d < F.D; d += (uint64_t)gridDim.x * kFgThreads) {
    const uint32_t id = F.ids[d];
    const FeedGrepSeq q = G.gseq[id];
    const uint64_t L = F.off[d + 1] - F.off[d], j0 = G.pro[d], j1 = G.pro[d + 1], n_frag = j1 - j0;
    const bool tail_open = n_frag && !(G.flag[j1 - 1] & kFgClosed);
    const uint64_t closed = n_frag - (tail_open ? 1 : 0);
    uint64_t head = 0;
    if (L) {
      if (q.open_len && (G.flag[j0] & kFgClosed) && (G.flag[j0] & kFgKeep)) head = q.open_len;
    } else if (G.final && q.open_len) {  // the open record closes without a fragment
      if ((q.open_hit != 0) != (G.invert != 0)) head = q.open_len;
    }
    const uint64_t hold = tail_open ? G.frag[j1] - G.frag[j1 - 1] : 0;
    FeedGrepSeq ns{};
    if (!G.final) {
      ns.seen = F.seqs[id].bytes;
      if (closed) {
        ns.open_len = hold;
        ns.open_hit = tail_open ? (G.flag[j1 - 1] & kFgHas) != 0 : 0u;
        ns.recs = q.recs + closed;
      } else {
        ns.open_len = q.open_len + L;
        ns.open_hit = n_frag ? (G.flag[j0] & kFgHas) != 0 : q.open_hit;
        ns.recs = q.recs;
      }
    } else {  // as after aha_feed_reset: a sequence of length 0 has an empty context
      F.seqs[id].bytes = 0;
      F.seqs[id].chars = 0;
    }
    G.gseq[id] = ns;
    if (G.head) G.head[d] = head;
    if (G.hold) G.hold[d] = (uint32_t)hold;
    if (G.rec_bases) G.rec_bases[d] = q.recs;
  }
}

}  // namespace

void feedgrep_launch_layout(const FeedArgs &F, const FeedGrepArgs &G, void *stream) {
  hipLaunchKernelGGL(kfg_layout, dim3(1), dim3(kFgScanThreads), 0, (hipStream_t)stream, F, G);
}

void feedgrep_launch_windows(const FeedArgs &F, const FeedGrepArgs &G, void *stream) {
  hipLaunchKernelGGL(kfg_windows, dim3(grid_for(F.D, 1, 4096)), dim3(kFgThreads), 0, (hipStream_t)stream, F, G);
}

void feedgrep_launch_flag(const FeedArgs &F, const FeedGrepArgs &G, uint32_t max_blocks, void *stream) {
  hipStream_t s = (hipStream_t)stream;
  if (!G.R) return;
  hipLaunchKernelGGL(kfg_has, dim3(grid_for(G.R, kFgThreads, max_blocks)), dim3(kFgThreads), 0, s, F, G);
  if (F.D) hipLaunchKernelGGL(kfg_first, dim3(grid_for(F.D, kFgThreads, max_blocks)), dim3(kFgThreads), 0, s, F, G);
  hipLaunchKernelGGL(kfg_flag, dim3(grid_for(G.R, kFgThreads, max_blocks)), dim3(kFgThreads), 0, s, G);
}

void feedgrep_launch_commit(const FeedArgs &F, const FeedGrepArgs &G, uint32_t max_blocks, void *stream) {
  if (!F.D) return;
  hipLaunchKernelGGL(kfg_commit, dim3(grid_for(F.D, kFgThreads, max_blocks)), dim3(kFgThreads), 0, (hipStream_t)stream, F, G);
}
}  // namespace aha
