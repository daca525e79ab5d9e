// scan_feedlongest.hip -- match_longest on a feed (aha_feed_open_params with longest = 1 | 2; feed.cpp, DESIGN.md 4.10 "Feed
// match_longest").
//
// match_longest_ (src/aha/ac.cr:118-143) reports a hit late -- at the first byte behind it that finds no goto -- and, with
// intersectable = false, resets its state at every yield, so the state at a cut is a function of the whole sequence and cannot
// be rebuilt from a context window.  A longest feed therefore carries the loop's state per sequence (FeedLongSeq, feed.hpp: the
// automaton state, the pending end as a distance back from the sequence's end, its key, the last two bytes for the shadow fail
// links) and a call walks its pieces as the documents of a two-pass batch (count -> block scan -> write, the scratch of the
// batch match_longest) that start from the carried state and do NOT flush at their end: what is pending there is state.
//   kfl_pieces<C, W>   a thread per piece, the piece in order: exact for both modes, the only form for intersectable = false
//   kfl_chunks<C, W>   intersectable = true: a thread per chunk with k_longest_chunks' warm-up (kernels.hip).  A thread owns the
//                      yields whose pending end lies in its chunk; the chunk with a piece's first byte also owns the carried
//                      pending end.  A warm-up that would reach in front of its piece begins at the piece's first byte from the
//                      carried state, which is exact like a document start; a thread that crosses a cut inside its chunk loads
//                      the next piece's carried state there.  No walk goes on past a piece's end.
//   pass 1 (W = false) also leaves the state at every non-empty piece's end in scratch (kfl_pieces: its thread; kfl_chunks: the
//                      thread whose chunk holds the piece's last byte -- its state is exact from its chunk's first byte on)
//   kfl_commit         once the total is known to fit: bases, the sequences' lengths, the scratch states into the feed
//   kfl_finish<W>      a finish call: the pending hit of every named sequence, counted and scanned by one workgroup, then written
//                      relative to the sequence's end, with the bases; the sequences start again at length 0
// Positions inside the walks are the call's text offsets plus kFlBias, so a carried pending end in front of the batch's first
// byte is still a non-negative Pending::p.  The two bytes in front of the current one are values in registers, seeded from the
// carried state: at a piece's first bytes the text in front of it is another sequence's, or not the caller's memory at all.
// Every store is a vector store from C++.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "automaton.hpp"
#include "devcommon.hpp"
#include "feed.hpp"
#include "image.hpp"
#include "longest_step.hpp"

namespace aha {
namespace {

constexpr int64_t kFlBias = 1ll << 32;  // (a piece is shorter than 2^31 bytes, a pending end less than 2^32 bytes back)

__device__ __forceinline__ void fl_load(const DevAut &A, const FeedLongSeq *at, uint64_t piece_start, uint32_t &B, Pending &pend,
                                        LongestPrevRegs &prev) {
  const uint4 q = *reinterpret_cast<const uint4 *>(at);  // {state, back, key, prev}
  B = q.x ? q.x - 1u : A.root;
  pend.p = q.y ? kFlBias + (int64_t)piece_start - (int64_t)q.y : -1;
  pend.key = q.z;
  pend.endc = 0;
  prev.y_ = q.w & 0xFFu;
  prev.x_ = (q.w >> 8) & 0xFFu;
}

__device__ __forceinline__ void fl_store(const DevAut &A, FeedLongSeq *at, uint64_t piece_end, uint32_t B, const Pending &pend,
                                         const LongestPrevRegs &prev) {
  uint4 q;
  q.x = B == A.root ? 0u : B + 1u;
  q.y = pend.p >= 0 ? (uint32_t)(kFlBias + (int64_t)piece_end - pend.p) : 0u;
  q.z = pend.p >= 0 ? pend.key : 0u;
  q.w = prev.y_ | prev.x_ << 8;
  *reinterpret_cast<uint4 *>(at) = q;
}

// Hit(idx - len + 1, idx + 1) ac.cr:255-257, relative to the piece's first byte: a hit may lie wholly in front of it
__device__ __forceinline__ void fl_emit(const DevAut &A, const MatchArgs &M, const Pending &h, uint64_t piece_start, uint64_t &idx) {
  if (idx < M.cap) {
    aha_hit o;
    o.end = (int32_t)(h.p - kFlBias - (int64_t)piece_start) + 1;
    o.start = o.end - (int32_t)A.key_ln[h.key].x;
    o.value = (int32_t)h.key;
    M.out[idx] = o;
  }
  idx++;
}

template <bool COMPACT, bool WRITE>
__global__ __launch_bounds__(kBlock) void kfl_pieces(DevAut A, MatchArgs M, const uint32_t *ids, FeedLongArgs L, int intersectable) {
  __shared__ uint64_t sm[kBlock / 64];
  const uint64_t d = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
  const bool live = d < M.n_docs;
  uint64_t idx = 0;
  if (WRITE) idx = M.blk_hits[blockIdx.x] + block_excl_scan<uint64_t>(live ? M.counts[d] : 0u, sm, nullptr);
  uint32_t hits = 0;
  if (live) {
    const uint64_t a = M.doc_off[d], e = M.doc_off[d + 1];
    if (WRITE && M.doc_hit_off) M.doc_hit_off[d] = idx;
    uint32_t B;
    Pending pend, out;
    LongestPrevRegs prev;
    fl_load(A, L.lseq + ids[d], a, B, pend, prev);
    for (uint64_t p = a; p < e; p++) {
      const uint32_t b = M.text[p];
      if (longest_step<Probe<COMPACT>>(A, B, b, prev, kFlBias + (int64_t)p, 0u, intersectable != 0, pend, &out) && out.key != kNoKey) {
        if (WRITE) fl_emit(A, M, out, a, idx);
        hits++;
      }
      prev.push(b);
    }
    if (!WRITE) {
      M.counts[d] = hits;
      if (e > a) fl_store(A, L.end + d, e, B, pend, prev);  // (an empty piece passes its sequence's state through: kfl_commit)
    }
  }
  if (!WRITE) {
    uint64_t tot;
    block_excl_scan<uint64_t>(hits, sm, &tot);
    if (threadIdx.x == 0) M.blk_hits[blockIdx.x] = tot;
  } else if (d == M.n_docs && M.doc_hit_off) {
    M.doc_hit_off[d] = M.totals[0];
  }
}

template <bool COMPACT, bool WRITE>
__global__ __launch_bounds__(kBlock) void kfl_chunks(DevAut A, MatchArgs M, const uint32_t *ids, FeedLongArgs L) {
  __shared__ uint64_t sm[kBlock / 64];
  const uint64_t c = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
  const bool live = c < M.n_chunks;
  uint64_t idx = 0;
  if (WRITE) idx = M.blk_hits[blockIdx.x] + block_excl_scan<uint64_t>(live ? M.counts[c] : 0u, sm, nullptr);
  uint32_t hits = 0;
  if (live) {
    const uint64_t N = M.n_bytes, D = M.n_docs;
    const uint64_t a = c * M.chunk, e = min(a + M.chunk, N);
    uint64_t dn = first_boundary(M.doc_off, D, a);  // first piece that starts at or after a
    uint64_t nb = M.doc_off[dn];
    uint64_t doc_start = a;
    uint64_t p = a;
    uint32_t B = A.root;
    Pending pend, out;
    LongestPrevRegs prev;  // (from the root nothing looks back before the walk itself has pushed the bytes it needs)
    if (nb != a) {         // a lies inside piece dn - 1
      doc_start = M.doc_off[dn - 1];
      const uint64_t W = 2ull * A.max_len;
      p = a - min<uint64_t>(a - doc_start, W);
      if (M.has_nul) {
        // k_longest_chunks' reach-back rule (kernels.hip): the warm-up must reach 2 * Lmax NUL-free bytes in front of the
        // earliest NUL it crosses, or two NULs in a row, or the piece's first byte -- whose carried state, kValueNode included,
        // is an exact anchor like a document start.  Past kNulBack bytes the chunk gives up (totals[1] = 2: piece by piece).
        constexpr uint64_t kNulBack = 4096;
        uint64_t hi = a;  // [p, hi) has not been searched yet
        for (;;) {
          uint64_t z = ~0ull;
          for (uint64_t q = p; q < hi; q++)
            if (M.text[q] == 0) {
              z = q;
              break;
            }
          if (z == ~0ull || p == doc_start) break;
          if (z > doc_start && M.text[z - 1] == 0) {  // two in a row: the root behind them
            p = z + 1;
            break;
          }
          if (a - z > kNulBack) {
            M.totals[1] = 2ull;
            break;
          }
          hi = z;
          p = z - min<uint64_t>(z - doc_start, W);
        }
      }
      if (p == doc_start) fl_load(A, L.lseq + ids[dn - 1], doc_start, B, pend, prev);
    }
    // a pending end in front of the piece's first byte is the carried one: it belongs to the chunk with that byte
    auto mine = [&](const Pending &h) {
      const int64_t q = h.p - kFlBias;
      if (q < (int64_t)doc_start) return doc_start >= a && doc_start < e;
      return (uint64_t)q >= a && (uint64_t)q < e;
    };
    for (;;) {
      if (p == nb) {  // the end of piece dn - 1: what is pending stays state; the next piece starts from its own carried state
        if (!WRITE && nb > a && nb <= e) fl_store(A, L.end + (dn - 1), nb, B, pend, prev);  // (its last byte is this chunk's)
        pend.p = -1;
        if (p >= e) break;
        do {
          if (WRITE && M.doc_hit_off && p >= a) M.doc_hit_off[dn] = idx;
          dn++;
          nb = dn <= D ? M.doc_off[dn] : ~0ull;
        } while (nb == p);
        if (p >= N) break;
        doc_start = p;
        fl_load(A, L.lseq + ids[dn - 1], p, B, pend, prev);
      }
      if (p >= e && (pend.p < 0 || !mine(pend))) break;  // nothing of this chunk is pending any more
      const uint32_t b = M.text[p];
      if (longest_step<Probe<COMPACT>>(A, B, b, prev, kFlBias + (int64_t)p, 0u, true, pend, &out) && mine(out) && out.key != kNoKey) {
        if (WRITE) fl_emit(A, M, out, doc_start, idx);
        hits++;
      }
      prev.push(b);
      p++;
    }
    if (!WRITE) M.counts[c] = hits;
    if (WRITE && e == N && M.doc_hit_off) {  // pieces that start at N (empty tail pieces) and the final total
      const uint64_t tot = M.totals[0];
      for (uint64_t q = first_boundary(M.doc_off, D, N); q <= D; q++) M.doc_hit_off[q] = tot;
    }
  }
  if (!WRITE) {
    uint64_t tot;
    block_excl_scan<uint64_t>(hits, sm, &tot);
    if (threadIdx.x == 0) M.blk_hits[blockIdx.x] = tot;
  }
}

__global__ void __launch_bounds__(kBlock) kfl_commit(FeedArgs F, FeedLongArgs L) {
  for (uint64_t d = blockIdx.x * (uint64_t)kBlock + threadIdx.x; d < F.D; d += (uint64_t)gridDim.x * kBlock) {
    const uint32_t id = F.ids[d];
    const uint64_t n0 = F.seqs[id].bytes, len = F.off[d + 1] - F.off[d];
    if (F.bases) F.bases[d] = n0;
    if (len) {
      F.seqs[id].bytes = n0 + len;
      *reinterpret_cast<uint4 *>(L.lseq + id) = *reinterpret_cast<const uint4 *>(L.end + d);
    }
  }
}

__device__ __forceinline__ bool fl_has_hit(const FeedLongSeq &q) { return q.back != 0 && q.key != kNoKey; }

// kWrite = false: one workgroup; F.pho[d] = the named sequences in front of d with a pending hit, F.pho[D] their total
template <bool kWrite>
__global__ void __launch_bounds__(kBlock) kfl_finish(FeedArgs F, FeedLongArgs L, const uint2 *key_ln) {
  if (!kWrite) {
    __shared__ uint64_t sm[kBlock / 64];
    uint64_t carry = 0;
    for (uint64_t d0 = 0; d0 < F.D; d0 += kBlock) {
      const uint64_t d = d0 + threadIdx.x;
      const uint64_t v = d < F.D && fl_has_hit(L.lseq[F.ids[d]]) ? 1u : 0u;
      uint64_t tot;
      const uint64_t ex = block_excl_scan<uint64_t>(v, sm, &tot);
      if (d < F.D) F.pho[d] = carry + ex;
      carry += tot;
    }
    if (threadIdx.x == 0) F.pho[F.D] = carry;
  } else {
    for (uint64_t d = blockIdx.x * (uint64_t)kBlock + threadIdx.x; d < F.D; d += (uint64_t)gridDim.x * kBlock) {
      const uint32_t id = F.ids[d];
      const FeedLongSeq q = L.lseq[id];
      if (fl_has_hit(q)) {  // its last byte lies q.back bytes in front of the sequence's end
        const int32_t end = 1 - (int32_t)q.back;
        int32_t *o = F.out + 3 * F.pho[d];
        o[0] = end - (int32_t)key_ln[q.key].x;
        o[1] = end;
        o[2] = (int32_t)q.key;
      }
      if (F.bases) F.bases[d] = F.seqs[id].bytes;
      if (L.sho) L.sho[d] = F.pho[d];
      *reinterpret_cast<uint4 *>(L.lseq + id) = make_uint4(0u, 0u, 0u, 0u);
      F.seqs[id].bytes = 0;
      F.seqs[id].chars = 0;
    }
    if (L.sho && blockIdx.x == 0 && threadIdx.x == 0) L.sho[F.D] = F.pho[F.D];
  }
}

uint32_t fl_grid(uint64_t items) { return (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>((items + kBlock - 1) / kBlock, 4096)); }

}  // namespace

void feedlong_launch_walk(const DevAut &A, const MatchArgs &M, const FeedArgs &F, const FeedLongArgs &L, bool chunks, bool intersectable,
                          bool write, void *stream) {
  hipStream_t s = (hipStream_t)stream;
  if (!chunks) {  // one thread per piece (+1 for the closing offset)
    const uint32_t g = (uint32_t)((M.n_docs + 1 + kBlock - 1) / kBlock);
    const int isect = intersectable ? 1 : 0;
#define AHA_FLP(C, W) hipLaunchKernelGGL((kfl_pieces<C, W>), dim3(g), dim3(kBlock), 0, s, A, M, F.ids, L, isect)
    if (A.compact) { if (write) AHA_FLP(true, true); else AHA_FLP(true, false); }
    else           { if (write) AHA_FLP(false, true); else AHA_FLP(false, false); }
#undef AHA_FLP
  } else {
    const uint32_t g = (uint32_t)((M.n_chunks + kBlock - 1) / kBlock);
#define AHA_FLC(C, W) hipLaunchKernelGGL((kfl_chunks<C, W>), dim3(g), dim3(kBlock), 0, s, A, M, F.ids, L)
    if (A.compact) { if (write) AHA_FLC(true, true); else AHA_FLC(true, false); }
    else           { if (write) AHA_FLC(false, true); else AHA_FLC(false, false); }
#undef AHA_FLC
  }
}

void feedlong_launch_commit(const FeedArgs &F, const FeedLongArgs &L, void *stream) {
  hipLaunchKernelGGL(kfl_commit, dim3(fl_grid(F.D)), dim3(kBlock), 0, (hipStream_t)stream, F, L);
}

void feedlong_launch_finish(const FeedArgs &F, const FeedLongArgs &L, const void *key_ln, bool write, void *stream) {
  if (write)
    hipLaunchKernelGGL(kfl_finish<true>, dim3(fl_grid(F.D)), dim3(kBlock), 0, (hipStream_t)stream, F, L, (const uint2 *)key_ln);
  else
    hipLaunchKernelGGL(kfl_finish<false>, dim3(1), dim3(kBlock), 0, (hipStream_t)stream, F, L, (const uint2 *)key_ln);
}

}  // namespace aha
