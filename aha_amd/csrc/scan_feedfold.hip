// scan_feedfold.hip -- what a feed on a handle folded beyond ASCII adds to the feed path (AHA_FEED_FOLD on a handle compiled with
// AHA_OPT_FOLD_SIMPLE, _BMP or _KANA; DESIGN.md 4.13 "Feeds on handles folded beyond ASCII"), for gfx950.  A translation unit of its
// own with its own copies of the tables: the code objects of scan_fold.hip, scan_foldk.hip and scan_feed.hip stay what they were.
//
// Such a call answers as if the sequence ended with this piece: its hits are those of fold(S[0 .. n1)) matched as one document
// with n0 < end <= n1.  The feed keeps ORIGINAL bytes in its context (W = Lmax + 1 of them) and folds per call:
//   the staged copies   P~: every piece folded on its own into the feed's scratch (scan_fold.hip, scan_foldk.hip with the piece
//                       offsets as document offsets) -- right everywhere but in the first two bytes of a piece whose character
//                       began in the context
//   kff_heads           those bytes: bytes 0 .. min(2, |P|) - 1 of every piece from ctx || P (feedfold_byte), a lane per piece,
//                       behind the copies' fix-up on the same stream
//   kff_windows         kfd_windows' window batch, folded: X~ = fold(ctx || P)[0 .. |ctx| + |P'|) -- the fold looks two bytes
//                       past the cut into the piece -- and the ctx and P' blocks as COPIES of its two parts, so "the first y hits
//                       of X are those of ctx alone" and "the first z hits of P are those of P' alone" stay true by count, and
//                       P'~ = P~[0 .. |P'|) byte for byte.  The first two bytes of X~ may differ from the sequence's fold (their
//                       character began in front of the context); a hit that touches them ends inside the context, where the
//                       ctx block has the same hit: that is what the two extra bytes of context are for.
// Both matches then read text that is already folded (device_match / device_count, `as_is`); kfd_commit, kfd_leads and a cover
// call's redaction keep reading the caller's bytes.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "feed.hpp"
#include "feed_fold.hpp"

namespace aha {
namespace {

constexpr int kFfThreads = 256;
constexpr uint32_t kFfWindowBlocks = 4096;  // kff_windows: workgroups at the most; beyond that a workgroup strides the pieces
constexpr uint32_t kFfHeadBlocks = 16;      // kff_heads: workgroups at the most (4096 lanes); beyond that a lane strides the pieces

__device__ const uint16_t d_ff_pair[AHA_FOLD2_ENTRIES] = {AHA_FOLD2_TABLE};  // (this code object's copies of the tables)
__device__ const uint8_t d_ff_index3[AHA_FOLD3_INDEX_ENTRIES] = {AHA_FOLD3_INDEX};
__device__ const uint16_t d_ff_live3[AHA_FOLD3_LIVE_ENTRIES] = {AHA_FOLD3_LIVE};
__device__ const uint8_t d_ff_indexk[AHA_FOLDK_INDEX_ENTRIES] = {AHA_FOLDK_INDEX};
__device__ const uint16_t d_ff_livek[AHA_FOLDK_LIVE_ENTRIES] = {AHA_FOLDK_LIVE};

template <int kMode>
__device__ __forceinline__ Fold3Tables ff_tables() {
  return Fold3Tables{d_ff_pair, kMode == 4 ? d_ff_indexk : d_ff_index3, kMode == 4 ? d_ff_livek : d_ff_live3};
}

// A lane per piece: a few bytes each, straight from the tables in memory.  dst = F.ftext, where the staged copy and its fix-up
// have run; the caller's text and the context are only read.
template <int kMode>
__global__ void __launch_bounds__(kFfThreads) kff_heads(FeedArgs F) {
  const Fold3Tables T = ff_tables<kMode>();
  const uint64_t stride = (uint64_t)gridDim.x * kFfThreads;
  for (uint64_t d = (uint64_t)blockIdx.x * kFfThreads + threadIdx.x; d < F.D; d += stride) {
    const uint64_t a = F.off[d], L = F.off[d + 1] - a;
    if (!L) continue;
    const uint32_t id = F.ids[d];
    const FeedSeq sq = F.seqs[id];
    const uint32_t lc = (uint32_t)min((uint64_t)F.W, sq.bytes);
    const uint8_t *c = F.ctx + ((uint64_t)sq.bank * F.n_seqs + id) * F.W;
    const uint8_t *p = F.text + a;
    F.ftext[a] = feedfold_byte(T, kMode, c, lc, p, L, 0);
    if (L > 1) F.ftext[a + 1] = feedfold_byte(T, kMode, c, lc, p, L, 1);
  }
}

// kfd_windows (scan_feed.hip) with every byte through feedfold_byte over the tables in LDS -- 3840 bytes for the simple fold,
// 3840 + 992 + 3712 for the BMP fold, 3840 + 992 + 4224 for the kana fold -- staged once per workgroup.  A workgroup per piece;
// a lane writes byte i of X~ and the same byte into the ctx block (i < |ctx|) or the P' block.
template <int kMode>
__global__ void __launch_bounds__(kFfThreads) kff_windows(FeedArgs F) {
  constexpr uint32_t kIndex = kMode == 2 ? 1 : kMode == 3 ? AHA_FOLD3_INDEX_ENTRIES : AHA_FOLDK_INDEX_ENTRIES;
  constexpr uint32_t kLive = kMode == 2 ? 1 : kMode == 3 ? AHA_FOLD3_LIVE_ENTRIES : AHA_FOLDK_LIVE_ENTRIES;
  __shared__ uint16_t tab[AHA_FOLD2_ENTRIES];
  __shared__ uint16_t live[kLive];
  __shared__ uint8_t index[kIndex];
  __shared__ uint32_t s_leads;
  const Fold3Tables G = ff_tables<kMode>();
  for (uint32_t t = threadIdx.x; t < AHA_FOLD2_ENTRIES; t += kFfThreads) tab[t] = G.pair[t];
  if (kMode != 2) {
    for (uint32_t t = threadIdx.x; t < kLive; t += kFfThreads) live[t] = G.live[t];
    for (uint32_t t = threadIdx.x; t < kIndex; t += kFfThreads) index[t] = G.index[t];
  }
  __syncthreads();
  const Fold3Tables T = {tab, index, live};
  const uint64_t D = F.D;
  for (uint64_t d = blockIdx.x; d < D; d += gridDim.x) {
    const uint32_t id = F.ids[d];
    const FeedSeq sq = F.seqs[id];
    const uint64_t L = F.off[d + 1] - F.off[d];
    const uint32_t lc = (uint32_t)min((uint64_t)F.W, sq.bytes);
    const uint32_t lp = (uint32_t)min((uint64_t)F.Wp, L);
    const uint8_t *c = F.ctx + ((uint64_t)sq.bank * F.n_seqs + id) * F.W;
    const uint8_t *p = F.text + F.off[d];
    uint8_t *x = F.win + F.woff[d], *cw = F.win + F.woff[D + d], *pw = F.win + F.woff[2 * D + d];
    if (threadIdx.x == 0) s_leads = 0;
    __syncthreads();
    uint32_t leads = 0;
    for (uint32_t i = threadIdx.x; i < lc + lp; i += kFfThreads) {
      const uint8_t b = feedfold_byte(T, kMode, c, lc, p, L, (int64_t)i - (int64_t)lc);
      x[i] = b;
      if (i < lc) {
        cw[i] = b;
        leads += (b & 0xC0u) != 0x80u ? 1u : 0u;  // (the fold keeps a lead byte a lead byte)
      } else {
        pw[i - lc] = b;
      }
    }
    if (F.chars) {
      if (leads) atomicAdd(&s_leads, leads);
      __syncthreads();
      if (threadIdx.x == 0) F.lead_ctx[d] = s_leads;
    }
    __syncthreads();
  }
}

uint32_t ff_grid(uint64_t units, uint64_t per_block, uint32_t cap) {
  return (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>((units + per_block - 1) / per_block, cap));
}

}  // namespace

void feedfold_launch_heads(const FeedArgs &F, int mode, void *stream) {
  if (!F.D || !F.n_bytes) return;
  const dim3 grid(ff_grid(F.D, kFfThreads, kFfHeadBlocks)), block(kFfThreads);
  hipStream_t s = (hipStream_t)stream;
  if (mode == 4)
    hipLaunchKernelGGL(kff_heads<4>, grid, block, 0, s, F);
  else if (mode == 3)
    hipLaunchKernelGGL(kff_heads<3>, grid, block, 0, s, F);
  else
    hipLaunchKernelGGL(kff_heads<2>, grid, block, 0, s, F);
}

void feedfold_launch_windows(const FeedArgs &F, int mode, void *stream) {
  if (!F.D) return;
  const dim3 grid(ff_grid(F.D, 1, kFfWindowBlocks)), block(kFfThreads);
  hipStream_t s = (hipStream_t)stream;
  if (mode == 4)
    hipLaunchKernelGGL(kff_windows<4>, grid, block, 0, s, F);
  else if (mode == 3)
    hipLaunchKernelGGL(kff_windows<3>, grid, block, 0, s, F);
  else
    hipLaunchKernelGGL(kff_windows<2>, grid, block, 0, s, F);
}

}  // namespace aha
