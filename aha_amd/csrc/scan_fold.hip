// scan_fold.hip -- the staged copy of a folded handle (AHA_OPT_FOLD_ASCII, fold.hpp) for gfx950: every engine but the
// prefix filter (scan_filter.hip folds its own loads) reads its text from scratch, folded on the way there.  One streaming
// pass, dst[j] = fold(src[j]): src is any byte address (a slice of a larger buffer), dst is 16-byte aligned, so the pass is
// at once the "aligned copy of an unaligned corpus" the engines need anyway (engine.cpp).  The caller's text is only read.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "fold.hpp"
#include "image.hpp"

namespace aha {

namespace {

typedef uint32_t kc_v4u __attribute__((ext_vector_type(4)));

__device__ __forceinline__ kc_v4u kc_load16(const uint8_t *__restrict__ p) {
  kc_v4u v;
  __builtin_memcpy(&v, p, 16);  // (gfx950 global loads take unaligned addresses)
  return v;
}
__device__ __forceinline__ kc_v4u kc_fold16(kc_v4u v) { return kc_v4u{fold32(v[0]), fold32(v[1]), fold32(v[2]), fold32(v[3])}; }

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

}  // namespace

void fold_launch_copy(const uint8_t *src, uint8_t *dst, uint64_t n_bytes, uint32_t max_blocks, void *stream) {
  if (!n_bytes) return;
  const uint64_t want = (n_bytes / 16 + 4 * 256 - 1) / (4 * 256);
  const uint32_t grid = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(want, std::max<uint32_t>(max_blocks, 1u)));
  hipLaunchKernelGGL(k_fold_copy, dim3(grid), dim3(256), 0, (hipStream_t)stream, src, dst, n_bytes);
}

}  // namespace aha
