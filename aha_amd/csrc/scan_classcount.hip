// scan_classcount.hip -- the class-counts path (aha_ac_class_counts_batch*): per document one row of C numbers, the hits of the
// document's keys added up by key class.  The hit list of a range of whole documents lies in scratch, document
// by document (engine.cpp device_class_counts); the caller's table out[D][C] is clear when the first kernel runs.
//   kcc_add        a workgroup takes slices of kCcSlice consecutive hits, grid-stride.  The slice's first and last document come
//                  from owner_of (post_common.hpp: the largest d with hit_off[d] - hit_off[0] <= i; it steps over documents
//                  without hits).  Where (documents of the slice) x C fits kCcTable words, the slice is summed in LDS -- slot
//                  (d - d_lo) * C + c -- and every non-zero slot is flushed with one global add; a document's hits may straddle
//                  slices, so a row can be flushed by several workgroups.  Otherwise (many tiny documents, a wide C) every
//                  (hit, class) pair is one global add: the adds are spread over many rows there.  In both forms a wave first
//                  takes the equal pairs of its first live lane out by ballot (one add for all lanes that hold it), as kc_visits
//                  does for hot keys: a document of one repeated key would queue a whole slice on one word.
//   kcc_fold_keys  a document whose hit list is beyond the bound of the hit buffer is never matched: its per-key counts (a count
//                  call over it alone) are added into its row, a lane per key with a non-zero count.
// Integer adds only: the result does not depend on their order.  Vector atomics and plain C++ only.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "image.hpp"
#include "post_common.hpp"

namespace aha {
namespace {

using post::grid_for;

constexpr int kCcThreads = 256;
static_assert(kCcSlice % kCcThreads == 0, "a slice is a whole number of rounds of the workgroup");

// one (document, class) pair per live lane, as its slot: add(slot, n) is called once for the slot of the wave's first live lane,
// with the number of lanes that hold it, and once with 1 for every other live lane.  All 64 lanes reach this call.
template <class Add>
__device__ __forceinline__ void cc_pair(bool live, uint64_t slot, Add add) {
  const unsigned long long m = __ballot(live);
  if (!m) return;
  const int lane = threadIdx.x & 63, leader = __ffsll((long long)m) - 1;
  const uint32_t lo = (uint32_t)__shfl((int)(uint32_t)slot, leader, 64), hi = (uint32_t)__shfl((int)(uint32_t)(slot >> 32), leader, 64);
  const uint64_t first = (uint64_t)hi << 32 | lo;
  const bool same = live && slot == first;
  const uint32_t n = (uint32_t)__popcll(__ballot(same));
  if (lane == leader)
    add(first, n);
  else if (live && !same)
    add(slot, 1u);
}

// hits[0, n_hits): the range's hits, document by document; hit_off[d] - hit_off[0]: the first hit of document d of its nd;
// out: the row of the range's first document
__global__ __launch_bounds__(kCcThreads) void kcc_add(const int32_t *hits, uint64_t n_hits, const uint64_t *hit_off, uint64_t nd,
                                                      const uint64_t *cls_off, const uint32_t *cls_ids, uint32_t n_keys, uint32_t C,
                                                      uint32_t *out) {
  __shared__ uint32_t s_tab[kCcTable];
  const uint64_t h0 = hit_off[0];
  const uint64_t n_slices = (n_hits + kCcSlice - 1) / kCcSlice;
  for (uint64_t slice = blockIdx.x; slice < n_slices; slice += gridDim.x) {
    const uint64_t i0 = slice * kCcSlice, i1 = min(i0 + (uint64_t)kCcSlice, n_hits);
    const uint64_t d_lo = owner_of(hit_off, nd, i0, h0), d_hi = owner_of(hit_off, nd, i1 - 1, h0);
    const uint64_t span = d_hi - d_lo + 1;
    const bool lds = span * C <= kCcTable;  // (span <= nd < 2^32 and C <= 2^16: no overflow)
    const uint32_t n_slots = lds ? (uint32_t)(span * C) : 0u;
    uint32_t *rows = out + d_lo * C;
    if (lds) {
      __syncthreads();  // (the flush of the slice before has read the table)
      for (uint32_t k = threadIdx.x; k < n_slots; k += kCcThreads) s_tab[k] = 0u;
      __syncthreads();
    }
    for (uint64_t b = i0; b < i1; b += kCcThreads) {
      const uint64_t i = b + threadIdx.x;
      const uint32_t value = i < i1 ? (uint32_t)hits[i * 3 + 2] : n_keys;
      uint64_t row = 0, j0 = 0;
      uint32_t n = 0;
      if (value < n_keys) {
        row = owner_of(hit_off + d_lo, span, i, h0);  // (hit_off[d_lo] - h0 <= i0 <= i)
        j0 = cls_off[value];
        n = (uint32_t)(cls_off[value + 1] - j0);
      }
      for (uint32_t j = 0; __any(j < n); j++) {
        const bool on = j < n;
        const uint32_t c = on ? cls_ids[j0 + j] : 0u;
        const uint64_t slot = row * C + c;
        if (lds)
          cc_pair(on, slot, [&](uint64_t s, uint32_t v) { atomicAdd(&s_tab[s], v); });
        else
          cc_pair(on, slot, [&](uint64_t s, uint32_t v) { atomicAdd(rows + s, v); });
      }
    }
    if (lds) {
      __syncthreads();
      for (uint32_t k = threadIdx.x; k < n_slots; k += kCcThreads) {
        const uint32_t v = s_tab[k];
        if (v) atomicAdd(rows + k, v);
      }
    }
  }
}

// key_counts[0, n_keys): one document's hits per key; row: that document's row
__global__ __launch_bounds__(kCcThreads) void kcc_fold_keys(const unsigned long long *key_counts, uint32_t n_keys, const uint64_t *cls_off,
                                                            const uint32_t *cls_ids, uint32_t *row) {
  for (uint64_t k = (uint64_t)blockIdx.x * kCcThreads + threadIdx.x; k < n_keys; k += (uint64_t)gridDim.x * kCcThreads) {
    const uint32_t v = (uint32_t)key_counts[k];  // (below 2^32: class_overflow.hpp)
    if (!v) continue;
    for (uint64_t j = cls_off[k]; j < cls_off[k + 1]; j++) atomicAdd(row + cls_ids[j], v);
  }
}

}  // namespace

void classcount_launch_add(const void *hits, uint64_t n_hits, const uint64_t *hit_off, uint64_t nd, const uint64_t *cls_off,
                           const uint32_t *cls_ids, uint32_t n_keys, uint32_t n_classes, uint32_t *out, uint32_t max_blocks,
                           void *stream) {
  if (!n_hits) return;
  hipLaunchKernelGGL(kcc_add, dim3(grid_for(n_hits, kCcSlice, max_blocks)), dim3(kCcThreads), 0, (hipStream_t)stream, (const int32_t *)hits, n_hits, hit_off, nd, cls_off,
                     cls_ids, n_keys, n_classes, out);
}

void classcount_launch_fold_keys(const uint64_t *key_counts, uint32_t n_keys, const uint64_t *cls_off, const uint32_t *cls_ids,
                                 uint32_t *row, uint32_t max_blocks, void *stream) {
  if (!n_keys) return;
  hipLaunchKernelGGL(kcc_fold_keys, dim3(grid_for(n_keys, kCcThreads, max_blocks)), dim3(kCcThreads), 0, (hipStream_t)stream,
                     reinterpret_cast<const unsigned long long *>(key_counts), n_keys, cls_off, cls_ids, row);
}

}  // namespace aha
