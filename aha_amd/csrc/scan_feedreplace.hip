// scan_feedreplace.hip -- the feed replace path (aha_feed_replace_batch*): the substituted stream of sequences that arrive in
// pieces, built on the device (DESIGN.md 4.10 "Feed replace").
//
// A replace call is a select call for the feed's state (feed.cpp feed_replace; scan_feedselect.hip).  A piece P takes its
// sequence T from n0 to n1 bytes; the call finds the cursor at c0 and leaves it at c1 (feedsel_cursor, feed.hpp), and every hit
// it settles lies inside [c0, c1).  The piece's result is T[c0 .. c1) with those hits replaced, so the call stages that text:
//   kfr_layout   per piece hold0 = n0 - c0, the staged length c1 - c0 = hold0 + |P| - hold1 with hold1 = n1 - c1; ext_off = the
//                exclusive scan of the lengths, bias = ext_off + hold0.  One block (block_run_scan, post_common.hpp).
//   kfr_stage    ext[ext_off[d] ..) = the last hold0 bytes of the sequence's context -- old[lc - hold0 .. lc) of its current
//                bank, lc = min(W, n0): the caller's bytes on a folded handle too (kfd_commit fills the banks from the caller's
//                text) --, then the piece's bytes up to c1.  Driven by the staged positions, as krp_copy by the output: a wave
//                owns 1024 staged bytes, a lane 16.  A tile wholly inside one piece's own bytes is a copy at a fixed distance:
//                two aligned 16-byte loads, a byte alignment, one aligned 16-byte store per lane.  Any other tile: every lane
//                walks its 16 bytes, piece by piece.
// The staged batch (ext, ext_off) with the settled selection (rows relative to the piece: staged position = bias[d] + start, the
// start possibly negative) is an ordinary replace problem: krp_delta with bias as its document offsets, the scan,
// krp_doc_offsets with ext_off, krp_copy (scan_replace.hip), unchanged.  Both kernels run in front of the commits: they read the
// sequences' old lengths, cursors and banks.  Vector loads and stores and plain C++ only.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "feed.hpp"
#include "post_common.hpp"

namespace aha {
namespace {

using post::grid_for;

constexpr int kFrScanThreads = 1024;
constexpr uint64_t kFrTile = 1024;  // staged bytes of one wave's tile: 16 per lane

// what piece d stages: -> hold0 (its return value is the staged length c1 - c0)
__device__ __forceinline__ uint64_t fr_piece(const FeedArgs &F, const FeedSelArgs &S, uint64_t d, uint32_t *hold0) {
  const uint32_t id = F.ids[d];
  const uint64_t n0 = F.seqs[id].bytes, L = F.off[d + 1] - F.off[d], n1 = n0 + L;
  const uint64_t wb = min((uint64_t)F.W, n0);
  const uint64_t c0 = S.sseq[id].cursor;
  // (c0 lies in [n0 - wb, n0] on a sequence fed through select and replace calls alone, and no other gets here; the clamp
  // keeps every index inside the context row whatever the state holds)
  const uint64_t h0 = min(n0 - min(c0, n0), wb);
  const uint64_t c1 = feedsel_cursor(n0 - h0, n0, wb, S.cend[d], n1, F.W, S.final);
  *hold0 = (uint32_t)h0;
  return h0 + L - (n1 - min(c1, n1));
}

// one block: hold0[d], ext_off[0 .. D] = the exclusive scan of the staged lengths, bias
__global__ void __launch_bounds__(kFrScanThreads) kfr_layout(FeedArgs F, FeedSelArgs S, FeedRepArgs R) {
  __shared__ uint64_t s[kFrScanThreads];
  const uint64_t total = block_run_scan<kFrScanThreads>(
      F.D,
      [&](uint64_t d) {
        uint32_t h0;
        const uint64_t len = fr_piece(F, S, d, &h0);
        R.hold0[d] = h0;
        return len;
      },
      [&](uint64_t d, uint64_t run) {
        R.ext_off[d] = run;
        R.bias[d] = run + R.hold0[d];  // (this lane's own store)
      },
      s);
  if (threadIdx.x == kFrScanThreads - 1) R.ext_off[F.D] = R.bias[F.D] = total;
}

// where piece d's staged bytes come from: the first hold0 of them from the context row, the rest from the piece
struct FrSrc {
  uint64_t e0, e1;      // its staged positions
  uint64_t h0;          // hold0
  const uint8_t *held;  // staged byte i < h0 = held[i]
  const uint8_t *body;  // staged byte i >= h0 = body[i - h0]
};

__device__ __forceinline__ FrSrc fr_src(const FeedArgs &F, const FeedRepArgs &R, uint64_t d) {
  FrSrc s;
  s.e0 = R.ext_off[d];
  s.e1 = R.ext_off[d + 1];
  s.h0 = R.hold0[d];
  const uint32_t id = F.ids[d];
  const FeedSeq sq = F.seqs[id];
  const uint64_t lc = min((uint64_t)F.W, sq.bytes);
  s.held = F.ctx + ((uint64_t)sq.bank * F.n_seqs + id) * F.W + (lc - s.h0);  // (h0 <= lc: kfr_layout)
  s.body = F.text + F.off[d];
  return s;
}

// staged bytes [q, q + cnt), cnt <= 16, piece by piece; one 16-byte store where the lane has all 16 (ext + q is aligned)
__device__ __forceinline__ void fr_lane(const FeedArgs &F, const FeedRepArgs &R, uint64_t q, uint32_t cnt) {
  uint64_t d = owner_of(R.ext_off, F.D, q);  // (ext_off[0] = 0; pieces that stage nothing are stepped over)
  FrSrc s = fr_src(F, R, d);
  uint32_t w[4] = {0u, 0u, 0u, 0u};
#pragma unroll
  for (uint32_t b = 0; b < 16; b++) {
    if (b < cnt) {
      const uint64_t p = q + b;
      while (p >= s.e1) s = fr_src(F, R, ++d);  // (p < ext_off[D]: d stays below D)
      const uint64_t i = p - s.e0;
      const uint32_t c = i < s.h0 ? s.held[i] : s.body[i - s.h0];
      w[b >> 2] |= c << (8 * (b & 3));
    }
  }
  uint8_t *dst = R.ext + q;
  if (cnt == 16) {
    *reinterpret_cast<uint4 *>(dst) = make_uint4(w[0], w[1], w[2], w[3]);
  } else {
#pragma unroll
    for (uint32_t b = 0; b < 16; b++)
      if (b < cnt) dst[b] = (uint8_t)(w[b >> 2] >> (8 * (b & 3)));
  }
}

__global__ __launch_bounds__(256) void kfr_stage(FeedArgs F, FeedRepArgs R) {
  const uint32_t lane = threadIdx.x & 63;
  const uint64_t wave = (uint64_t)blockIdx.x * 4 + (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const uint64_t n_waves = (uint64_t)gridDim.x * 4;
  const uint64_t total = R.ext_off[F.D], n_tiles = (total + kFrTile - 1) / kFrTile;
  for (uint64_t t = wave; t < n_tiles; t += n_waves) {
    const uint64_t q0 = t * kFrTile;
    bool fast = false;
    const uint8_t *from = nullptr;
    if (q0 + kFrTile <= total) {
      const uint64_t d = owner_of(R.ext_off, F.D, q0);
      const uint64_t b0 = R.bias[d];  // the piece's own bytes start here
      fast = q0 >= b0 && q0 + kFrTile <= R.ext_off[d + 1];
      from = F.text + F.off[d] + (q0 - b0);
    }
    const uint64_t q = q0 + (uint64_t)lane * 16;
    if (fast) {
      // 16 bytes from an address of any alignment: the aligned piece that holds the first byte and, where the bytes go on
      // into it, the next one -- both hold a byte of the caller's text
      const uintptr_t src = reinterpret_cast<uintptr_t>(from) + (uintptr_t)lane * 16;
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
      *reinterpret_cast<uint4 *>(R.ext + q) = r;
    } else if (q < total) {
      fr_lane(F, R, q, (uint32_t)min((uint64_t)16, total - q));
    }
  }
}

}  // namespace

void feedrep_launch_layout(const FeedArgs &F, const FeedSelArgs &S, const FeedRepArgs &R, void *stream) {
  hipLaunchKernelGGL(kfr_layout, dim3(1), dim3(kFrScanThreads), 0, (hipStream_t)stream, F, S, R);
}

void feedrep_launch_stage(const FeedArgs &F, const FeedRepArgs &R, uint64_t max_bytes, uint32_t max_blocks, void *stream) {
  if (!max_bytes || !F.D) return;
  const uint64_t n_tiles = (max_bytes + kFrTile - 1) / kFrTile;
  const uint32_t grid = grid_for(n_tiles, 4, max_blocks);
  hipLaunchKernelGGL(kfr_stage, dim3(grid), dim3(256), 0, (hipStream_t)stream, F, R);
}
}  // namespace aha
