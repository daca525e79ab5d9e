// scan_foldk.hip -- the staged copy of a handle compiled with AHA_OPT_FOLD_KANA (fold.hpp: foldk, FK's tables) for gfx950: a
// kernel of its own, k_foldk_copy, beside scan_fold.hip's -- whose code object stays, instruction for instruction and address
// for address, what it was: modes 1 to 3 launch exactly the kernels they launched.  dst = foldk of every document of src on its
// own: k_foldk_copy folds the buffer as ONE run of bytes, k_fold3_fix (scan_fold.hip) takes back what that did across a
// document boundary.  The halo of a lane's piece comes from memory (kc_fold3_halo, fold_piece.hpp) or from the neighbouring
// lanes' pieces.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <cstring>

#include "fold.hpp"
#include "fold_piece.hpp"
#include "image.hpp"

namespace aha {

namespace {

// ---- the kana fold (AHA_OPT_FOLD_KANA) --------------------------------------------------------------------------------------
__device__ const uint16_t d_foldk_pair[AHA_FOLD2_ENTRIES] = {AHA_FOLD2_TABLE};  // (this code object's copy of the pair table)
__device__ const uint8_t d_foldk_index[AHA_FOLDK_INDEX_ENTRIES] = {AHA_FOLDK_INDEX};
__device__ const uint16_t d_foldk_live[AHA_FOLDK_LIVE_ENTRIES] = {AHA_FOLDK_LIVE};

// kc_fold3_halo's two halves, each under its conditions: the two bytes in front of piece i (in the low half), the two behind it
// (in the high half), loaded from src only where they decide something and only inside [0, n)
__device__ __forceinline__ uint32_t kc_halo_front(const uint8_t *__restrict__ src, uint64_t i, const kc_v4u &v) {
  if (fold2_cont(kc_byte(v, 0)) && i > 0) return (uint32_t)src[i * 16 - 2] | ((uint32_t)src[i * 16 - 1] << 8);
  return 0;
}
__device__ __forceinline__ uint32_t kc_halo_back(const uint8_t *__restrict__ src, uint64_t i, uint64_t n, const kc_v4u &v) {
  const uint64_t j0 = i * 16;
  const uint32_t b14 = kc_byte(v, 14), b15 = kc_byte(v, 15);
  uint32_t h = 0;
  if ((fold2_lead(b15) || fold3_lead(b15) || (fold3_lead(b14) && fold2_cont(b15))) && j0 + 16 < n) h |= (uint32_t)src[j0 + 16] << 16;
  if (fold3_lead(b15) && j0 + 17 < n) h |= (uint32_t)src[j0 + 17] << 24;
  return h;
}
// The halo of piece i taken from the neighbouring lanes' pieces: consecutive lanes hold consecutive pieces, so the two bytes in
// front are bytes 14, 15 of the lane below and the two behind are bytes 0, 1 of the lane above -- two cross-lane moves and no
// load.  EVERY lane of the wave must arrive here together (a cross-lane read from an inactive lane is undefined): the
// callers' loops are wave-uniform, and a lane without a piece (own == false, v == 0) takes part in the moves and in nothing
// else.  Only a wave's two edges load from src, under kc_fold3_halo's conditions: lane 0 the bytes in front; lane 63, and the
// lane whose neighbour above has no piece (the bytes behind are the tail's, or there are none), the bytes behind.  The bytes
// a neighbour hands over are the true ones where kc_fold3_halo leaves 0 because they decide nothing: fold3_byte gives the same.
__device__ __forceinline__ uint32_t kc_foldk_halo_lane(const uint8_t *__restrict__ src, uint64_t i, uint64_t n, uint64_t pieces,
                                                       const kc_v4u &v, bool own) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t below = __shfl_up(v[3], 1, 64), above = __shfl_down(v[0], 1, 64);
  uint32_t h = (below >> 16) | (above << 16);
  if (!((v[0] | v[1] | v[2] | v[3]) & 0x80808080u)) return 0;  // (a piece of ASCII, and a lane without a piece)
  if (lane == 0) h = (h & 0xFFFF0000u) | (own ? kc_halo_front(src, i, v) : 0u);
  if (lane == 63 || i + 1 >= pieces) h = (h & 0x0000FFFFu) | (own ? kc_halo_back(src, i, n, v) : 0u);
  return h;
}

// k_fold3_copy's loop over the pair table and FK's two levels -- 3840 + 992 + 4224 bytes -- staged in LDS once per workgroup.
// kLane == false: kc_fold3_halo as it is (the halo from memory), k_fold3_copy's loops as they are.  kLane == true: the halo from
// the neighbouring lanes (kc_foldk_halo_lane); for that a wave takes a step with all its 64 lanes or not at all -- the
// unrolled loop runs while the wave's LAST lane has its fourth piece, the remainder loop while its FIRST lane has a piece, and
// there a lane past the end loads nothing and stores nothing but stays through the exchange.  (stride is a multiple of 256, so
// i - lane is the piece of the wave's lane 0 at every step.)
template <bool kLane>
__global__ __launch_bounds__(256) void k_foldk_copy(const uint8_t *__restrict__ src, uint8_t *__restrict__ dst, uint64_t n) {
  __shared__ uint16_t tab[AHA_FOLD2_ENTRIES];
  __shared__ uint16_t live[AHA_FOLDK_LIVE_ENTRIES];
  __shared__ uint8_t index[AHA_FOLDK_INDEX_ENTRIES];
  for (uint32_t t = threadIdx.x; t < AHA_FOLD2_ENTRIES; t += 256) tab[t] = d_foldk_pair[t];
  for (uint32_t t = threadIdx.x; t < AHA_FOLDK_LIVE_ENTRIES; t += 256) live[t] = d_foldk_live[t];
  for (uint32_t t = threadIdx.x; t < AHA_FOLDK_INDEX_ENTRIES; t += 256) index[t] = d_foldk_index[t];
  __syncthreads();
  const Fold3Tables T = {tab, index, live};
  const uint64_t pieces = n / 16, stride = (uint64_t)gridDim.x * 256;
  const uint64_t lane = threadIdx.x & 63u;
  kc_v4u *out = reinterpret_cast<kc_v4u *>(dst);
  uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  for (; (kLane ? i - lane + 63 : i) + 3 * stride < pieces; i += 4 * stride) {
    const kc_v4u a = kc_load16(src + i * 16), b = kc_load16(src + (i + stride) * 16);
    const kc_v4u c = kc_load16(src + (i + 2 * stride) * 16), d = kc_load16(src + (i + 3 * stride) * 16);
    uint32_t ha, hb, hc, hd;
    if (kLane) {
      ha = kc_foldk_halo_lane(src, i, n, pieces, a, true), hb = kc_foldk_halo_lane(src, i + stride, n, pieces, b, true);
      hc = kc_foldk_halo_lane(src, i + 2 * stride, n, pieces, c, true), hd = kc_foldk_halo_lane(src, i + 3 * stride, n, pieces, d, true);
    } else {
      ha = kc_fold3_halo(src, i, n, a), hb = kc_fold3_halo(src, i + stride, n, b);
      hc = kc_fold3_halo(src, i + 2 * stride, n, c), hd = kc_fold3_halo(src, i + 3 * stride, n, d);
    }
    out[i] = kc_fold3_apply<false>(T, a, ha);
    out[i + stride] = kc_fold3_apply<false>(T, b, hb);
    out[i + 2 * stride] = kc_fold3_apply<false>(T, c, hc);
    out[i + 3 * stride] = kc_fold3_apply<false>(T, d, hd);
  }
  for (; (kLane ? i - lane : i) < pieces; i += stride) {
    const bool own = i < pieces;  // (always so without kLane)
    kc_v4u a = {0, 0, 0, 0};
    if (own) a = kc_load16(src + i * 16);
    const uint32_t ha = kLane ? kc_foldk_halo_lane(src, i, n, pieces, a, own) : kc_fold3_halo(src, i, n, a);
    if (own) out[i] = kc_fold3_apply<false>(T, a, ha);
  }
  const uint64_t tail = pieces * 16 + threadIdx.x;
  if (blockIdx.x == 0 && threadIdx.x < 16 && tail < n)
    dst[tail] = fold3_byte(T, tail > 1 ? src[tail - 2] : 0u, tail > 0 ? src[tail - 1] : 0u, src[tail], tail + 1 < n ? src[tail + 1] : 0u,
                           tail + 2 < n ? src[tail + 2] : 0u);
}

}  // namespace

// AHA_FOLDK_HALO=mem|lane chooses k_foldk_copy's instantiation: the halo from memory or from the neighbouring lanes (DESIGN.md
// 4.13 has the measurement behind the default; read at every launch, so that one process can time both call by call).
// Anything else is the default.
static const bool kFoldkLaneDefault = true;
static bool foldk_lane_halo() {
  const char *e = getenv("AHA_FOLDK_HALO");
  if (e && !strcmp(e, "lane")) return true;
  if (e && !strcmp(e, "mem")) return false;
  return kFoldkLaneDefault;
}

void foldk_launch_copy(const uint8_t *src, uint8_t *dst, uint64_t n_bytes, const uint64_t *doc_offsets, uint64_t n_docs,
                       uint32_t max_blocks, void *stream) {
  if (!n_bytes) return;
  if (foldk_lane_halo())
    hipLaunchKernelGGL(k_foldk_copy<true>, dim3(fold_grid(n_bytes, max_blocks)), dim3(256), 0, (hipStream_t)stream, src, dst, n_bytes);
  else
    hipLaunchKernelGGL(k_foldk_copy<false>, dim3(fold_grid(n_bytes, max_blocks)), dim3(256), 0, (hipStream_t)stream, src, dst, n_bytes);
  // (putting back original bytes does not depend on the table: k_fold3_fix as it is, scan_fold.hip)
  fold3_launch_fix(src, dst, n_bytes, doc_offsets, n_docs, max_blocks, stream);
}

}  // namespace aha
