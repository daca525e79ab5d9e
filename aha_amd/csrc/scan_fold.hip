// scan_fold.hip -- the staged copy of a folded handle (AHA_OPT_FOLD_ASCII, fold.hpp) for gfx950: every engine but the
// prefix filter (scan_filter.hip folds its own loads) reads its text from scratch, folded on the way there.  One streaming
// pass, dst[j] = fold(src[j]): src is any byte address (a slice of a larger buffer), dst is 16-byte aligned, so the pass is
// at once the "aligned copy of an unaligned corpus" the engines need anyway (engine.cpp).  The caller's text is only read.
// A handle compiled with AHA_OPT_FOLD_SIMPLE gets the same pass with the two-byte characters folded through the table
// (k_fold2_copy: the buffer as ONE run of bytes) and a second, tiny one that takes back what the first did across a document
// boundary (k_fold2_fix): together fold2 of every document on its own (fold.hpp).  AHA_OPT_FOLD_BMP: the same two steps with
// the three-byte characters folded too (k_fold3_copy, k_fold3_fix): fold3 of every document on its own.  The pieces of a lane's
// work that the kernel of AHA_OPT_FOLD_KANA shares (scan_foldk.hip) are in fold_piece.hpp.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>

#include "fold.hpp"
#include "fold_piece.hpp"
#include "image.hpp"

namespace aha {

namespace {

// 16 bytes per lane per step, four steps in flight; a lane's pieces lie a whole grid apart, so a wave's loads and stores are
// 1 KiB of consecutive bytes.  The last n % 16 bytes go byte by byte (block 0).
__global__ __launch_bounds__(256) void k_fold_copy(const uint8_t *__restrict__ src, uint8_t *__restrict__ dst, uint64_t n) {
  const uint64_t pieces = n / 16, stride = (uint64_t)gridDim.x * 256;
  kc_v4u *out = reinterpret_cast<kc_v4u *>(dst);
  uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  for (; i + 3 * stride < pieces; i += 4 * stride) {
    const kc_v4u a = kc_load16(src + i * 16), b = kc_load16(src + (i + stride) * 16);
    const kc_v4u c = kc_load16(src + (i + 2 * stride) * 16), d = kc_load16(src + (i + 3 * stride) * 16);
    out[i] = kc_fold16(a);
    out[i + stride] = kc_fold16(b);
    out[i + 2 * stride] = kc_fold16(c);
    out[i + 3 * stride] = kc_fold16(d);
  }
  for (; i < pieces; i += stride) out[i] = kc_fold16(kc_load16(src + i * 16));
  const uint64_t tail = pieces * 16 + threadIdx.x;
  if (blockIdx.x == 0 && threadIdx.x < 16 && tail < n) dst[tail] = fold8(src[tail]);
}

// ---- the simple fold (AHA_OPT_FOLD_SIMPLE) --------------------------------------------------------------------------------
__device__ const uint16_t d_fold2_table[AHA_FOLD2_ENTRIES] = {AHA_FOLD2_TABLE};

// fold2 of piece i (bytes [16 i, 16 i + 16) of src, loaded as v) within the n bytes of src.  A piece of ASCII takes fold32 and
// nothing else.  Otherwise byte by byte from the byte and its two neighbours; the one before byte 0 and the one after byte 15
// belong to another lane (the next piece, another wave's 1 KiB, a piece a grid stride away) and are loaded from src only
// where they decide something -- byte 0 a continuation byte, byte 15 a lead byte -- and only inside [0, n).  The lane that
// holds a pair's lead writes the folded lead, the lane that holds its continuation byte the folded continuation, both from
// the same table entry: every lane writes its own 16 bytes and no others.
__device__ __forceinline__ kc_v4u kc_fold2_piece(const uint16_t *tab, const uint8_t *__restrict__ src, uint64_t i, uint64_t n, kc_v4u v) {
  if (!((v[0] | v[1] | v[2] | v[3]) & 0x80808080u)) return kc_fold16(v);
  const uint64_t j0 = i * 16;
  uint32_t prev = 0, next = 0;
  if (fold2_cont(kc_byte(v, 0)) && j0 > 0) prev = src[j0 - 1];
  if (fold2_lead(kc_byte(v, 15)) && j0 + 16 < n) next = src[j0 + 16];
  kc_v4u o = {0, 0, 0, 0};
#pragma unroll
  for (int k = 0; k < 16; k++) {
    const uint32_t p = k ? kc_byte(v, k - 1) : prev, nx = k < 15 ? kc_byte(v, k + 1) : next;
    o[k >> 2] |= (uint32_t)fold2_byte(tab, p, kc_byte(v, k), nx) << ((k & 3) * 8);
  }
  return o;
}

// k_fold_copy's loop (16 bytes per lane per step, consecutive lanes on consecutive pieces, the n % 16 tail byte by byte in
// block 0) with the table -- 3840 bytes -- staged in LDS once per workgroup.
__global__ __launch_bounds__(256) void k_fold2_copy(const uint8_t *__restrict__ src, uint8_t *__restrict__ dst, uint64_t n) {
  __shared__ uint16_t tab[AHA_FOLD2_ENTRIES];
  for (uint32_t t = threadIdx.x; t < AHA_FOLD2_ENTRIES; t += 256) tab[t] = d_fold2_table[t];
  __syncthreads();
  const uint64_t pieces = n / 16, stride = (uint64_t)gridDim.x * 256;
  kc_v4u *out = reinterpret_cast<kc_v4u *>(dst);
  uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  for (; i + 3 * stride < pieces; i += 4 * stride) {
    const kc_v4u a = kc_load16(src + i * 16), b = kc_load16(src + (i + stride) * 16);
    const kc_v4u c = kc_load16(src + (i + 2 * stride) * 16), d = kc_load16(src + (i + 3 * stride) * 16);
    out[i] = kc_fold2_piece(tab, src, i, n, a);
    out[i + stride] = kc_fold2_piece(tab, src, i + stride, n, b);
    out[i + 2 * stride] = kc_fold2_piece(tab, src, i + 2 * stride, n, c);
    out[i + 3 * stride] = kc_fold2_piece(tab, src, i + 3 * stride, n, d);
  }
  for (; i < pieces; i += stride) out[i] = kc_fold2_piece(tab, src, i, n, kc_load16(src + i * 16));
  const uint64_t tail = pieces * 16 + threadIdx.x;
  if (blockIdx.x == 0 && threadIdx.x < 16 && tail < n)
    dst[tail] = fold2_byte(tab, tail > 0 ? src[tail - 1] : 0u, src[tail], tail + 1 < n ? src[tail + 1] : 0u);
}

// A lane per interior document boundary b = off[d] - off[0], 1 <= d < D.  Where the bytes on its two sides are a lead and a
// continuation byte, k_fold2_copy paired them; a lone lead byte and a lone continuation byte have no fold of their own, so the
// original bytes are what fold2 of either document has there.  (b is taken as it comes: offsets nobody has validated yet
// only ever pass 0 < b < n, and a batch with such offsets is refused before its hits are looked at.)
__global__ __launch_bounds__(256) void k_fold2_fix(const uint8_t *__restrict__ src, uint8_t *__restrict__ dst, uint64_t n,
                                                   const uint64_t *__restrict__ off, uint64_t D) {
  const uint64_t stride = (uint64_t)gridDim.x * 256;
  for (uint64_t d = 1 + (uint64_t)blockIdx.x * 256 + threadIdx.x; d < D; d += stride) {
    const uint64_t b = off[d] - off[0];
    if (b == 0 || b >= n) continue;
    const uint8_t lead = src[b - 1], cont = src[b];
    if (fold2_lead(lead) && fold2_cont(cont)) {
      dst[b - 1] = lead;
      dst[b] = cont;
    }
  }
}

// ---- the fold of the three-byte characters (AHA_OPT_FOLD_BMP) -------------------------------------------------------------
__device__ const uint8_t d_fold3_index[AHA_FOLD3_INDEX_ENTRIES] = {AHA_FOLD3_INDEX};
__device__ const uint16_t d_fold3_live[AHA_FOLD3_LIVE_ENTRIES] = {AHA_FOLD3_LIVE};

// k_fold2_copy's loop with both tables -- 3840 + 992 + 3712 bytes -- staged in LDS once per workgroup.
template <bool kLive>
__global__ __launch_bounds__(256) void k_fold3_copy(const uint8_t *__restrict__ src, uint8_t *__restrict__ dst, uint64_t n) {
  __shared__ uint16_t tab[AHA_FOLD2_ENTRIES];
  __shared__ uint16_t live[AHA_FOLD3_LIVE_ENTRIES];
  __shared__ uint8_t index[AHA_FOLD3_INDEX_ENTRIES];
  for (uint32_t t = threadIdx.x; t < AHA_FOLD2_ENTRIES; t += 256) tab[t] = d_fold2_table[t];
  for (uint32_t t = threadIdx.x; t < AHA_FOLD3_LIVE_ENTRIES; t += 256) live[t] = d_fold3_live[t];
  for (uint32_t t = threadIdx.x; t < AHA_FOLD3_INDEX_ENTRIES; t += 256) index[t] = d_fold3_index[t];
  __syncthreads();
  const Fold3Tables T = {tab, index, live};
  const uint64_t pieces = n / 16, stride = (uint64_t)gridDim.x * 256;
  kc_v4u *out = reinterpret_cast<kc_v4u *>(dst);
  uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  for (; i + 3 * stride < pieces; i += 4 * stride) {
    const kc_v4u a = kc_load16(src + i * 16), b = kc_load16(src + (i + stride) * 16);
    const kc_v4u c = kc_load16(src + (i + 2 * stride) * 16), d = kc_load16(src + (i + 3 * stride) * 16);
    const uint32_t ha = kc_fold3_halo(src, i, n, a), hb = kc_fold3_halo(src, i + stride, n, b);
    const uint32_t hc = kc_fold3_halo(src, i + 2 * stride, n, c), hd = kc_fold3_halo(src, i + 3 * stride, n, d);
    out[i] = kc_fold3_apply<kLive>(T, a, ha);
    out[i + stride] = kc_fold3_apply<kLive>(T, b, hb);
    out[i + 2 * stride] = kc_fold3_apply<kLive>(T, c, hc);
    out[i + 3 * stride] = kc_fold3_apply<kLive>(T, d, hd);
  }
  for (; i < pieces; i += stride) {
    const kc_v4u a = kc_load16(src + i * 16);
    out[i] = kc_fold3_apply<kLive>(T, a, kc_fold3_halo(src, i, n, a));
  }
  const uint64_t tail = pieces * 16 + threadIdx.x;
  if (blockIdx.x == 0 && threadIdx.x < 16 && tail < n)
    dst[tail] = fold3_byte(T, tail > 1 ? src[tail - 2] : 0u, tail > 0 ? src[tail - 1] : 0u, src[tail], tail + 1 < n ? src[tail + 1] : 0u,
                           tail + 2 < n ? src[tail + 2] : 0u);
}

// A lane per interior document boundary b, as in k_fold2_fix.  k_fold3_copy folded across b where a pair lies at (b - 1, b) or a
// triple is cut 1|2 (b - 1, b, b + 1) or 2|1 (b - 2, b - 1, b); the fragments -- a lead byte alone or with one continuation
// byte, continuation bytes without their lead -- have no fold of their own, so the original bytes are what fold3 of either
// document has there.  A triple cut twice (a one-byte or empty document inside it) is put back by two lanes, both with the
// same source bytes.  (b is taken as it comes, see k_fold2_fix; every index is checked against [0, n) here.)
__global__ __launch_bounds__(256) void k_fold3_fix(const uint8_t *__restrict__ src, uint8_t *__restrict__ dst, uint64_t n,
                                                   const uint64_t *__restrict__ off, uint64_t D) {
  const uint64_t stride = (uint64_t)gridDim.x * 256;
  for (uint64_t d = 1 + (uint64_t)blockIdx.x * 256 + threadIdx.x; d < D; d += stride) {
    const uint64_t b = off[d] - off[0];
    if (b == 0 || b >= n) continue;
    const uint8_t before = src[b - 1], at = src[b];
    if (!fold2_cont(at)) continue;
    if (fold2_lead(before)) {
      dst[b - 1] = before;
      dst[b] = at;
    } else if (fold3_lead(before)) {
      if (b + 1 < n && fold2_cont(src[b + 1])) {
        dst[b - 1] = before;
        dst[b] = at;
        dst[b + 1] = src[b + 1];
      }
    } else if (fold2_cont(before) && b >= 2 && fold3_lead(src[b - 2])) {
      dst[b - 2] = src[b - 2];
      dst[b - 1] = before;
      dst[b] = at;
    }
  }
}

}  // namespace

// (the grid of both staged copies: a workgroup per 1024 pieces, max_blocks at the most -- beyond that lanes stride)
uint32_t fold_grid(uint64_t n_bytes, uint32_t max_blocks) {
  const uint64_t want = (n_bytes / 16 + 4 * 256 - 1) / (4 * 256);
  return (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(want, std::max<uint32_t>(max_blocks, 1u)));
}

void fold2_launch_copy(const uint8_t *src, uint8_t *dst, uint64_t n_bytes, const uint64_t *doc_offsets, uint64_t n_docs,
                       uint32_t max_blocks, void *stream) {
  if (!n_bytes) return;
  hipLaunchKernelGGL(k_fold2_copy, dim3(fold_grid(n_bytes, max_blocks)), dim3(256), 0, (hipStream_t)stream, src, dst, n_bytes);
  if (!doc_offsets || n_docs < 2) return;
  const uint64_t want = (n_docs - 1 + 255) / 256;
  const uint32_t grid = (uint32_t)std::min<uint64_t>(want, std::max<uint32_t>(max_blocks, 1u));
  hipLaunchKernelGGL(k_fold2_fix, dim3(grid), dim3(256), 0, (hipStream_t)stream, src, dst, n_bytes, doc_offsets, n_docs);
}

// AHA_FOLD3_LIVE_TEST=1 launches the instantiation with the live-lead test; it measured slower on every text, Chinese
// included, so the default is the one without (read at every launch, so that one process can time both
// kernels call by call)
static bool fold3_live_test() {
  const char *e = getenv("AHA_FOLD3_LIVE_TEST");
  return e && e[0] == '1' && !e[1];
}

void fold3_launch_copy(const uint8_t *src, uint8_t *dst, uint64_t n_bytes, const uint64_t *doc_offsets, uint64_t n_docs,
                       uint32_t max_blocks, void *stream) {
  if (!n_bytes) return;
  if (fold3_live_test())
    hipLaunchKernelGGL(k_fold3_copy<true>, dim3(fold_grid(n_bytes, max_blocks)), dim3(256), 0, (hipStream_t)stream, src, dst, n_bytes);
  else
    hipLaunchKernelGGL(k_fold3_copy<false>, dim3(fold_grid(n_bytes, max_blocks)), dim3(256), 0, (hipStream_t)stream, src, dst, n_bytes);
  if (!doc_offsets || n_docs < 2) return;
  const uint64_t want = (n_docs - 1 + 255) / 256;
  const uint32_t grid = (uint32_t)std::min<uint64_t>(want, std::max<uint32_t>(max_blocks, 1u));
  hipLaunchKernelGGL(k_fold3_fix, dim3(grid), dim3(256), 0, (hipStream_t)stream, src, dst, n_bytes, doc_offsets, n_docs);
}

// (k_fold3_fix on its own, for the staged copy of AHA_OPT_FOLD_KANA in scan_foldk.hip: putting back original bytes does not depend
// on the table)
void fold3_launch_fix(const uint8_t *src, uint8_t *dst, uint64_t n_bytes, const uint64_t *doc_offsets, uint64_t n_docs,
                      uint32_t max_blocks, void *stream) {
  if (!n_bytes || !doc_offsets || n_docs < 2) return;
  const uint64_t want = (n_docs - 1 + 255) / 256;
  const uint32_t grid = (uint32_t)std::min<uint64_t>(want, std::max<uint32_t>(max_blocks, 1u));
  hipLaunchKernelGGL(k_fold3_fix, dim3(grid), dim3(256), 0, (hipStream_t)stream, src, dst, n_bytes, doc_offsets, n_docs);
}

void fold_launch_copy(const uint8_t *src, uint8_t *dst, uint64_t n_bytes, uint32_t max_blocks, void *stream) {
  if (!n_bytes) return;
  hipLaunchKernelGGL(k_fold_copy, dim3(fold_grid(n_bytes, max_blocks)), dim3(256), 0, (hipStream_t)stream, src, dst, n_bytes);
}

}  // namespace aha
