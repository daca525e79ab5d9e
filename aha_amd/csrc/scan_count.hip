// scan_count.hip -- the count path (aha_ac_count_batch*): hits per key without the hit list.
//
// At every position where the traversal reaches a real END state with head key h the reference yields one hit for each key
// on h's output chain (src/aha/ac.cr:265-278; key_ln[].next, already truncated as the reference truncates it).  So a count
// call keeps the traversal and the per-chunk hit counts of its pipeline (the per-document offsets and the total come from
// them as in a match) and replaces the expansion by two steps:
//   kc_visits  one add per EVENT (END position) into visits[h], read from the records the expansion would have read: the
//              chunks' regions after k2d_count / ku_regroup / kf_walk / kp_pairs (x = key or chain offset | count << 24), or the
//              character-level traversal's wave-ordered records (the END state's base; uend[base] holds the key).
//   kc_chain   key_counts[j] += visits[h] for every j on chain(h): O(sum of the chain lengths of the keys seen), not of the text.
// Events pile up on few keys (cfg 5: a few short keys take most of them), so neither step adds into global memory per event:
// a workgroup sums into an LDS table of {id, 64-bit count} (count_table.hpp, shared with scan_feed.hip: open addressing, a
// few probes; what does not find a place adds to global memory at once) and flushes it with one global add per distinct id
// at its end.  In kc_visits a wave first takes
// its most frequent id out by ballot (one LDS add for all lanes that hold it), so the table's atomics do not queue on it.
#include <hip/hip_runtime.h>

#include "automaton.hpp"
#include "count_table.hpp"
#include "devcommon.hpp"
#include "image.hpp"
#include "post_common.hpp"
#include "unit.hpp"

namespace aha {
namespace {

constexpr int kCtThreads = 256;
// Record sources of kc_visits.  REGIONS: the chunks' event regions after the count pass (id = key id or chain offset).
// UNIT: the character-level traversal's wave-ordered records (id = base of the END state).
enum { kSrcRegions = 0, kSrcUnit = 1 };

template <int SRC>
__device__ __forceinline__ uint32_t ct_key(const DevAut &A, const uint2 *uend, uint32_t id) {
  if (SRC == kSrcUnit) return uend[id].x & 0xFFFFFFu;
  return A.chain ? A.chain[id].y : id;
}

// one event per live lane (count_table.hpp); what finds no slot goes to visits[] at once
template <int SRC>
__device__ __forceinline__ void ct_visit(const CtTable &t, const DevAut &A, const uint2 *uend, unsigned long long *visits,
                                         bool live, uint32_t id) {
  ct_event<false>(t, live, id, false,
                  [&](uint32_t i, unsigned long long v) { atomicAdd(&visits[ct_key<SRC>(A, uend, i)], v); });
}

template <int SRC>
__device__ __forceinline__ void ct_flush(const CtTable &t, const DevAut &A, const uint2 *uend, unsigned long long *dst) {
  for (uint32_t i = threadIdx.x; i < kCtSlots; i += kCtThreads) {
    const uint32_t id = t.id[i];
    if (id != kCtEmpty) atomicAdd(&dst[ct_key<SRC>(A, uend, id)], t.cnt[i]);
  }
}

template <int SRC>
__global__ __launch_bounds__(kCtThreads) void kc_visits(DevAut A, V2Args M, const uint2 *uend, unsigned long long *visits) {
  __shared__ uint32_t s_id[kCtSlots];
  __shared__ unsigned long long s_cnt[kCtSlots];
  __shared__ uint32_t s_total;
  if (M.cursor[1]) return;  // (an aborted pass: nothing is counted)
  const CtTable t{s_id, s_cnt};
  ct_clear(t);
  const uint32_t stride = M.ev_stride;
  if (SRC == kSrcRegions) {
    __syncthreads();
    for (uint64_t c = blockIdx.x; c < M.n_chunks; c += gridDim.x) {
      const uint32_t n = min(M.ev_cnt[c], stride);
      const uint2 *reg = M.evd + c * stride;
      for (uint32_t i0 = 0; i0 < n; i0 += kCtThreads) {
        const uint32_t i = i0 + threadIdx.x;
        const uint32_t x = i < n ? reg[i].x : 0u;
        // (count 0: a record that stands for no hit -- the pair engine's voided events)
        ct_visit<SRC>(t, A, uend, visits, (x >> 24) != 0u, x & 0xFFFFFFu);
      }
    }
  } else {
    const uint32_t bb = M.unit_bb, bmask = (1u << bb) - 1u;
    const uint64_t n_groups = (M.n_chunks + 63) / 64;
    for (uint64_t g = blockIdx.x; g < n_groups; g += gridDim.x) {
      __syncthreads();  // (the table is clear; s_total of the group before is read)
      if (threadIdx.x < 64) {
        const uint64_t c = g * 64 + threadIdx.x;
        const uint32_t tot = wave_sum(c < M.n_chunks ? min(M.ev_cnt[c], stride) : 0u);
        if (threadIdx.x == 0) s_total = tot;
      }
      __syncthreads();
      const uint32_t total = s_total;
      const uint32_t *src = M.evg + g * 64 * stride * 3;
      for (uint32_t i0 = 0; i0 < total; i0 += kCtThreads) {
        const uint32_t i = i0 + threadIdx.x;
        uint32_t x = 0u, z = 0u;
        if (i < total) {
          x = src[(size_t)i * 3];
          z = src[(size_t)i * 3 + 2];
        }
        ct_visit<SRC>(t, A, uend, visits, i < total && u_rec_n(x, z, bb) != 0u, x & bmask);
      }
    }
  }
  __syncthreads();
  ct_flush<SRC>(t, A, uend, visits);
}

// key_counts[j] += visits[h] for every key j on chain(h) = h, key_ln[h].y, ... (until -1: the chains are truncated as the
// reference truncates them, src/aha/ac.cr:265-278)
__global__ __launch_bounds__(kCtThreads) void kc_chain(const uint2 *key_ln, uint32_t n_keys, const unsigned long long *visits,
                                                      unsigned long long *out, const unsigned long long *abortf) {
  __shared__ uint32_t s_id[kCtSlots];
  __shared__ unsigned long long s_cnt[kCtSlots];
  if (abortf && *abortf) return;
  const CtTable t{s_id, s_cnt};
  ct_clear(t);
  __syncthreads();
  for (uint32_t h = blockIdx.x * kCtThreads + threadIdx.x; h < n_keys; h += gridDim.x * kCtThreads) {
    const unsigned long long v = visits[h];
    if (!v) continue;
    int32_t k = (int32_t)h;
    do {
      if (!ct_add(t, (uint32_t)k, v)) atomicAdd(&out[k], v);
      k = (int32_t)key_ln[k].y;
    } while (k >= 0);
  }
  __syncthreads();
  for (uint32_t i = threadIdx.x; i < kCtSlots; i += kCtThreads) {
    const uint32_t id = s_id[i];
    if (id != kCtEmpty) atomicAdd(&out[id], s_cnt[i]);
  }
}

}  // namespace

// visits[] += the events of the pass: region records (post = the DevAut the region pipeline's post passes use) or, uend
// non-null, the character-level traversal's wave-ordered records
void count_launch_visits(const DevAut &A, const V2Args &M, const uint2 *uend, unsigned long long *visits, uint32_t max_blocks,
                         void *stream) {
  const uint64_t units = uend ? (M.n_chunks + 63) / 64 : M.n_chunks;
  const dim3 grid(post::grid_for(units, 1, max_blocks));
  if (uend)
    hipLaunchKernelGGL(kc_visits<kSrcUnit>, grid, dim3(kCtThreads), 0, (hipStream_t)stream, A, M, uend, visits);
  else
    hipLaunchKernelGGL(kc_visits<kSrcRegions>, grid, dim3(kCtThreads), 0, (hipStream_t)stream, A, M, uend, visits);
}

void count_launch_chain(const uint2 *key_ln, uint32_t n_keys, const unsigned long long *visits, unsigned long long *out,
                        const unsigned long long *abortf, void *stream) {
  const dim3 grid(post::grid_for(n_keys, kCtThreads, 1024));
  hipLaunchKernelGGL(kc_chain, grid, dim3(kCtThreads), 0, (hipStream_t)stream, key_ln, n_keys, visits, out, abortf);
}

}  // namespace aha
