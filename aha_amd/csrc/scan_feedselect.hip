// scan_feedselect.hip -- the feed select path (aha_feed_select_batch*): the leftmost-longest, non-overlapping hits of sequences
// that arrive in pieces (DESIGN.md 4.10 "Feed select").
//
// A hit that starts at s ends at or before s + Lmax, so with W = max(Lmax - 1, 0) and F(n) = max(0, n - W) every hit with a
// start below F(n) is known once the sequence is n bytes long, and so is the greedy choice at every such start.  A call on a
// piece P that takes its sequence from n0 to n1 bytes therefore works on the extended positions [F(n0), n1) -- the last
// W' = min(W, n0) bytes in front of the piece, then the piece -- and reports the selected hits with a start in [F(n0), F(n1))
// (the frontier; n1 under FINAL).  What it needs from the past is not text but the open hits: per sequence the feed keeps
//   tail[W]   the longest known hit (len << 32 | value, the form of scan_select.hip) that starts at each of the last min(W, n)
//             bytes: a hit that ends inside the context cannot be re-derived from the context, so it is carried;
//   cursor c  everything in front of it is final: inside a reported hit or in no selected hit ever.  The greedy walk of the
//             next call starts there; tail entries and hits with a start below c are ignored.
// The true hits of the pieces (end inside the piece, start down to -W') come from the feed's own passes (feed.cpp: window
// batch, main pass, kfd_merge into scratch).  Over all pieces' extended positions, piece by piece (eoff):
//   kfs_layout    eoff = the scan of W'_d + |P_d|; n0 per piece.  One block.
//   kfs_tail      L[x] = the sequence's tail entry, for the W'_d positions in front of the piece at or behind the cursor
//   kfs_longest   L[x] = max(L[x], len << 32 | value) per hit of the call at or behind the cursor: one 64-bit atomicMax
//   ksl_marks     (scan_select.hip, shared) the cover mask and one bit per piece's first extended position
//   kfs_walk      one walker per run, as ksl_walk: runs are independent for the reason given there -- a jump is a hit, which
//                 covers what it jumps over and lies inside one piece's extended positions.  The one difference: a walker takes
//                 a start only below its piece's frontier.  A run that crosses the frontier is walked up to it; its rest stays
//                 open.  The end of the last hit taken per piece (cend) by atomicMax: ends ascend along the greedy walk.
//   ksl_rank_*    (shared) the rank of the select mask: the total, and the pieces' offsets into the selection
//   kfs_emit      every set bit in position order as {x - W', x - W' + len, value}, once the total fits
//   kfs_commit    behind kfd_commit, after success only: tail = L over the last min(W, n1) positions (entries of the old tail
//                 stay where |P| < W), cursor = max(cursor, end of the last hit taken, F(n1)), piece_hold = n1 - cursor; under
//                 FINAL the sequence starts again from length 0.
// Nothing here is proportional to W x hits.  Vector atomics and plain C++ only.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "feed.hpp"
#include "post_common.hpp"

namespace aha {
namespace {

using post::grid_for;

constexpr int kFsThreads = 256;
constexpr int kFsScanThreads = 1024;
__device__ __forceinline__ uint64_t fs_back(const FeedArgs &F, const FeedSelArgs &S, uint64_t d) { return min((uint64_t)F.W, S.n0[d]); }

// one block: n0[d], eoff[0 .. D] = the exclusive scan of min(W, n0[d]) + |P_d|
__global__ void __launch_bounds__(kFsScanThreads) kfs_layout(FeedArgs F, FeedSelArgs S) {
  __shared__ uint64_t s[kFsScanThreads];
  const uint64_t total = block_run_scan<kFsScanThreads>(
      F.D,
      [&](uint64_t d) {
        const uint64_t n0 = F.seqs[F.ids[d]].bytes;
        S.n0[d] = n0;
        return min((uint64_t)F.W, n0) + (F.off[d + 1] - F.off[d]);
      },
      [&](uint64_t d, uint64_t run) { S.eoff[d] = run; }, s);
  if (threadIdx.x == kFsScanThreads - 1) S.eoff[F.D] = total;
}

// a thread per piece and tail entry
__global__ void __launch_bounds__(kFsThreads) kfs_tail(FeedArgs F, FeedSelArgs S) {
  const uint64_t W = F.W, n = F.D * W;
  for (uint64_t i = blockIdx.x * (uint64_t)kFsThreads + threadIdx.x; i < n; i += (uint64_t)gridDim.x * kFsThreads) {
    const uint64_t d = i / W, j = i - d * W;
    const uint64_t wb = fs_back(F, S, d);
    if (j < W - wb) continue;  // in front of the sequence's first byte
    const uint32_t id = F.ids[d];
    const uint64_t x = j - (W - wb);
    if (S.n0[d] - wb + x < S.sseq[id].cursor) continue;  // a settled hit covers it
    const unsigned long long v = S.tail[(uint64_t)id * W + j];
    if (v) S.L[S.eoff[d] + x] = v;
  }
}

__global__ void __launch_bounds__(kFsThreads) kfs_longest(FeedArgs F, FeedSelArgs S) {
  for (uint64_t i = blockIdx.x * (uint64_t)kFsThreads + threadIdx.x; i < S.n_hits; i += (uint64_t)gridDim.x * kFsThreads) {
    const int64_t st = S.hits[3 * i], en = S.hits[3 * i + 1];
    const uint32_t value = (uint32_t)S.hits[3 * i + 2];
    if (en <= st) continue;
    const uint64_t d = owner_of(S.pho, F.D, i);
    const int64_t wb = (int64_t)fs_back(F, S, d), x = st + wb;
    const uint64_t e0 = S.eoff[d], E = S.eoff[d + 1] - e0;
    if (x < 0 || (uint64_t)(x + (en - st)) > E) continue;  // (never: a hit lies inside its piece's extended positions)
    if (S.n0[d] - (uint64_t)wb + (uint64_t)x < S.sseq[F.ids[d]].cursor) continue;
    atomicMax(S.L + e0 + (uint64_t)x, (unsigned long long)(uint32_t)(en - st) << 32 | value);
  }
}

__global__ void __launch_bounds__(kFsThreads) kfs_walk(FeedArgs F, FeedSelArgs S) {
  const uint64_t nb = S.NE;
  for (uint64_t p0 = blockIdx.x * (uint64_t)kFsThreads + threadIdx.x; p0 < nb; p0 += (uint64_t)gridDim.x * kFsThreads) {
    if (!S.L[p0]) continue;
    if (p0 && !bit_at(S.start, p0) && bit_at(S.cover, p0 - 1)) continue;  // inside a run: its walker comes by
    const uint64_t d = owner_of(S.eoff, F.D, p0);
    const uint64_t e0 = S.eoff[d], e1 = S.eoff[d + 1], E = e1 - e0;
    const uint64_t front = e0 + (S.final ? E : (E > F.W ? E - F.W : 0));
    uint64_t p = p0, last = 0;
    while (p < front) {
      atomicOr(S.select + (p >> 5), 1u << (uint32_t)(p & 31));
      p += (uint64_t)(S.L[p] >> 32);
      last = p;
      // the next start of the run: covered bytes without a hit of their own are stepped over
      while (p < e1 && bit_at(S.cover, p) && !S.L[p]) p++;
      if (p >= e1 || !bit_at(S.cover, p)) break;
    }
    if (last) atomicMax(S.cend + d, (unsigned long long)(last - e0));
  }
}

// the selection in position order (ksl_emit, with the piece's own origin)
__global__ void __launch_bounds__(kFsThreads) kfs_emit(FeedArgs F, FeedSelArgs S) {
  for_ranked_bits<kFsThreads>(S.select, (S.NE + 31) / 32, rank_blocks(S.NE), S.blk, [&](uint64_t w, uint32_t i, uint64_t at) {
    const uint64_t p = w * 32 + i;
    const unsigned long long v = S.L[p];
    const uint64_t d = owner_of(S.eoff, F.D, p);
    const int64_t st = (int64_t)(p - S.eoff[d]) - (int64_t)fs_back(F, S, d);
    S.out[at * 3] = (int32_t)st;
    S.out[at * 3 + 1] = (int32_t)(st + (int64_t)(v >> 32));
    S.out[at * 3 + 2] = (int32_t)(uint32_t)v;
  });
}

// a workgroup per piece, behind kfd_commit (F.seqs[id].bytes is the new length there; n0 is the old one)
__global__ void __launch_bounds__(kFsThreads) kfs_commit(FeedArgs F, FeedSelArgs S) {
  const uint64_t W = F.W;
  for (uint64_t d = blockIdx.x; d < F.D; d += gridDim.x) {
    const uint32_t id = F.ids[d];
    const uint64_t n0 = S.n0[d], wb = fs_back(F, S, d), e0 = S.eoff[d], E = S.eoff[d + 1] - e0, n1 = n0 - wb + E;
    if (!S.final) {
      // entry j = byte n1 - W + j of the sequence = extended position E - W + j
      for (uint64_t j = threadIdx.x; j < W; j += kFsThreads) S.tail[(uint64_t)id * W + j] = E + j >= W ? S.L[e0 + (E + j - W)] : 0ull;
    }
    if (threadIdx.x == 0) {
      const uint64_t c = feedsel_cursor(S.sseq[id].cursor, n0, wb, S.cend[d], n1, W, S.final);
      FeedSelSeq ns;
      ns.seen = S.final ? 0 : n1;
      ns.cursor = S.final ? 0 : c;
      S.sseq[id] = ns;
      if (S.final) {  // as after aha_feed_reset: a sequence of length 0 has an empty context
        F.seqs[id].bytes = 0;
        F.seqs[id].chars = 0;
        if (S.tseq) S.tseq[id] = FeedTokSeq{0ull, 0ull};  // ... and no token is open (scan_feedtokens.hip)
      }
      if (S.hold) S.hold[d] = S.final ? 0u : (uint32_t)(n1 - c);
    }
  }
}

}  // namespace

void feedsel_launch_layout(const FeedArgs &F, const FeedSelArgs &S, void *stream) {
  hipLaunchKernelGGL(kfs_layout, dim3(1), dim3(kFsScanThreads), 0, (hipStream_t)stream, F, S);
}

void feedsel_launch_longest(const FeedArgs &F, const FeedSelArgs &S, uint32_t max_blocks, void *stream) {
  hipStream_t s = (hipStream_t)stream;
  if (F.D * F.W) hipLaunchKernelGGL(kfs_tail, dim3(grid_for(F.D * F.W, kFsThreads, max_blocks)), dim3(kFsThreads), 0, s, F, S);
  if (S.n_hits) hipLaunchKernelGGL(kfs_longest, dim3(grid_for(S.n_hits, kFsThreads, max_blocks)), dim3(kFsThreads), 0, s, F, S);
}

void feedsel_launch_walk(const FeedArgs &F, const FeedSelArgs &S, uint32_t max_blocks, void *stream) {
  hipLaunchKernelGGL(kfs_walk, dim3(grid_for(S.NE, kFsThreads, max_blocks)), dim3(kFsThreads), 0, (hipStream_t)stream, F, S);
}

void feedsel_launch_emit(const FeedArgs &F, const FeedSelArgs &S, uint32_t max_blocks, void *stream) {
  hipLaunchKernelGGL(kfs_emit, dim3(grid_for(rank_blocks(S.NE) * 64, kFsThreads, max_blocks)), dim3(kFsThreads), 0, (hipStream_t)stream, F, S);
}

void feedsel_launch_commit(const FeedArgs &F, const FeedSelArgs &S, void *stream) {
  hipLaunchKernelGGL(kfs_commit, dim3(grid_for(F.D, 1, 4096)), dim3(kFsThreads), 0, (hipStream_t)stream, F, S);
}
}  // namespace aha
