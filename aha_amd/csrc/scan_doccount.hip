// scan_doccount.hip -- the document counts (aha_ac_doc_counts_batch*): for every document one {key, count} pair per distinct
// value among its hits, ascending by key id, without the hit list going back to the caller.
//
// The hits of a range of whole documents lie in the call's scratch as the match wrote them (12-byte triples, in document
// order; only `value` is read here).  The host knows every document's hit count and gives each document to one of three
// forms (engine.cpp device_doc_counts):
//   kdc_sort     h <= sort_max (4096): a workgroup loads the document's ids into LDS, sorts them (bitonic: ids only, no
//                payload, so stability is of no concern), run-length encodes.
//   kdc_range    sort_max < h < dense_min: a workgroup walks the key space in ranges of range_keys (8192) ids; per range an
//                LDS row of counts, one LDS add per hit that falls into it, then an ordered compaction of the row.  The hits
//                are read K / range_keys times (from L2: they are below K / 8 * 12 bytes), nothing is sorted.
//   kdc_add + kdc_compact   h >= dense_min: a row of K uint32 in scratch per document in flight.  kdc_add takes slices of
//                64 Ki hits, sums them in the {id, count} LDS table of count_table.hpp (hits pile up on few keys) and adds
//                every distinct id of the slice to the row once; kdc_compact scans the row in order, writes the non-zero
//                entries and clears them.  O(K) per document, hence the floor on h.
// Every form leaves a document's pairs in a temp place of its own and their number in n_pairs[doc]: the sort and the dense
// form over the document's own hits (at most h pairs of 8 bytes where h triples of 12 were -- all of them read before the
// first pair is written), the range form, which reads its hits again and again, in a buffer beside them.  The host scans
// the numbers; kdc_gather then copies the pairs that lie below the caller's capacity to their final place.
// LDS per workgroup: 32 KiB (sort: ids + run starts), 32 KiB (range), 48 KiB (add: the table) -- three to five per CU.
#include <hip/hip_runtime.h>

#include "count_table.hpp"
#include "image.hpp"
#include "post_common.hpp"

namespace aha {
namespace {

constexpr int kDcThreads = 256;
constexpr uint32_t kDcPad = 0xFFFFFFFFu;  // above every key id: the sort's padding

// exclusive prefix of v over the workgroup's 256 threads and the total; s_w: 4 words of LDS
__device__ __forceinline__ uint32_t dc_block_scan(uint32_t v, uint32_t *s_w, uint32_t *total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint32_t inc = wave_incl_scan(v);
  __syncthreads();  // (s_w of the round before is read)
  if (lane == 63) s_w[wave] = inc;
  __syncthreads();
  uint32_t base = 0, tot = 0;
#pragma unroll
  for (int w = 0; w < kDcThreads / 64; w++) {
    const uint32_t t = s_w[w];
    if (w < wave) base += t;
    tot += t;
  }
  *total = tot;
  return base + inc - v;
}

__global__ __launch_bounds__(kDcThreads) void kdc_sort(const DcItem *items, const uint32_t *hits, uint32_t *n_pairs) {
  __shared__ uint32_t s_id[kDcSortMax];
  __shared__ uint32_t s_pos[kDcSortMax + 1];
  __shared__ uint32_t s_w[kDcThreads / 64];
  const DcItem it = items[blockIdx.x];
  const uint32_t n = it.n;
  uint32_t P = 1;
  while (P < n) P <<= 1;
  const uint32_t *src = hits + it.begin * 3 + 2;
  for (uint32_t i = threadIdx.x; i < P; i += kDcThreads) s_id[i] = i < n ? src[(size_t)i * 3] : kDcPad;
  __syncthreads();
  for (uint32_t k = 2; k <= P; k <<= 1) {
    for (uint32_t j = k >> 1; j > 0; j >>= 1) {
      for (uint32_t i = threadIdx.x; i < P; i += kDcThreads) {
        const uint32_t p = i ^ j;
        if (p > i) {
          const uint32_t a = s_id[i], b = s_id[p];
          if (((i & k) == 0) ? a > b : a < b) {
            s_id[i] = b;
            s_id[p] = a;
          }
        }
      }
      __syncthreads();
    }
  }
  // run starts, in order
  uint32_t runs = 0;
  for (uint32_t i0 = 0; i0 < n; i0 += kDcThreads) {
    const uint32_t i = i0 + threadIdx.x;
    const bool head = i < n && (i == 0 || s_id[i] != s_id[i - 1]);
    uint32_t tot;
    const uint32_t at = dc_block_scan(head ? 1u : 0u, s_w, &tot);
    if (head) s_pos[runs + at] = i;
    runs += tot;
  }
  if (threadIdx.x == 0) {
    s_pos[runs] = n;
    n_pairs[it.doc] = runs;
  }
  __syncthreads();
  for (uint32_t r = threadIdx.x; r < runs; r += kDcThreads) {
    const uint32_t p = s_pos[r];
    it.out[2 * (size_t)r] = s_id[p];
    it.out[2 * (size_t)r + 1] = s_pos[r + 1] - p;
  }
}

__global__ __launch_bounds__(kDcThreads) void kdc_range(const DcItem *items, const uint32_t *hits, uint32_t n_keys,
                                                        uint32_t range_keys, uint32_t *n_pairs) {
  __shared__ uint32_t s_cnt[kDcRangeKeys];
  __shared__ uint32_t s_w[kDcThreads / 64];
  const DcItem it = items[blockIdx.x];
  const uint32_t n = it.n;
  const uint32_t *src = hits + it.begin * 3 + 2;
  uint32_t written = 0;
  for (uint32_t r0 = 0; r0 < n_keys; r0 += range_keys) {
    const uint32_t rn = min(range_keys, n_keys - r0);
    for (uint32_t i = threadIdx.x; i < rn; i += kDcThreads) s_cnt[i] = 0u;
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < n; i += kDcThreads) {
      const uint32_t v = src[(size_t)i * 3] - r0;  // (below r0: wraps above rn)
      if (v < rn) atomicAdd(&s_cnt[v], 1u);
    }
    __syncthreads();
    for (uint32_t i0 = 0; i0 < rn; i0 += kDcThreads) {
      const uint32_t i = i0 + threadIdx.x;
      const uint32_t c = i < rn ? s_cnt[i] : 0u;
      uint32_t tot;
      const uint32_t at = dc_block_scan(c ? 1u : 0u, s_w, &tot);
      if (c) {
        it.out[2 * (size_t)(written + at)] = r0 + i;
        it.out[2 * (size_t)(written + at) + 1] = c;
      }
      written += tot;
    }
    __syncthreads();  // (the row is read: the next range clears it)
  }
  if (threadIdx.x == 0) n_pairs[it.doc] = written;
}

// slices of the dense documents' hits: it.doc = the document's row
__global__ __launch_bounds__(kDcThreads) void kdc_add(const DcItem *items, uint32_t n_items, const uint32_t *hits, uint32_t *rows,
                                                      uint32_t n_keys) {
  __shared__ uint32_t s_id[kCtSlots];
  __shared__ unsigned long long s_cnt[kCtSlots];
  const CtTable t{s_id, s_cnt};
  for (uint32_t x = blockIdx.x; x < n_items; x += gridDim.x) {
    const DcItem it = items[x];
    uint32_t *row = rows + (size_t)it.doc * n_keys;
    const uint32_t *src = hits + it.begin * 3 + 2;
    ct_clear(t);
    __syncthreads();
    for (uint32_t i0 = 0; i0 < it.n; i0 += kDcThreads) {
      const uint32_t i = i0 + threadIdx.x;
      const bool live = i < it.n;
      const uint32_t v = live ? src[(size_t)i * 3] : 0u;
      ct_event<false>(t, live, v, false, [&](uint32_t id, unsigned long long c) { atomicAdd(&row[id], (uint32_t)c); });
    }
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < kCtSlots; i += kDcThreads) {
      const uint32_t id = s_id[i];
      if (id != kCtEmpty) atomicAdd(&row[id], (uint32_t)s_cnt[i]);
    }
    __syncthreads();  // (the table is flushed: the next slice clears it)
  }
}

// a workgroup per row: the non-zero entries in order; a uint32 row (kdc_add's) is cleared on the way, a uint64 row (the key
// counts of a count call over one document) is left as it is.  it.doc = the document, it.out = where its pairs go
template <class T, bool CLEAR>
__global__ __launch_bounds__(kDcThreads) void kdc_compact(const DcItem *items, T *rows, uint32_t n_keys, uint32_t *n_pairs) {
  __shared__ uint32_t s_w[kDcThreads / 64];
  constexpr uint32_t kPer = 16;
  const DcItem it = items[blockIdx.x];
  T *row = rows + (size_t)blockIdx.x * n_keys;
  uint32_t written = 0;
  for (uint32_t t0 = 0; t0 < n_keys; t0 += kDcThreads * kPer) {
    const uint32_t k0 = t0 + threadIdx.x * kPer;
    T c[kPer];
    uint32_t nz = 0;
#pragma unroll
    for (uint32_t j = 0; j < kPer; j++) {
      c[j] = k0 + j < n_keys ? row[k0 + j] : T(0);
      nz += c[j] != T(0);
    }
    uint32_t tot;
    uint32_t at = written + dc_block_scan(nz, s_w, &tot);
#pragma unroll
    for (uint32_t j = 0; j < kPer; j++) {
      if (c[j] != T(0)) {
        it.out[2 * (size_t)at] = k0 + j;
        it.out[2 * (size_t)at + 1] = (uint32_t)c[j];
        at++;
        if (CLEAR) row[k0 + j] = T(0);
      }
    }
    written += tot;
  }
  if (threadIdx.x == 0) n_pairs[it.doc] = written;
}

// pair i of the range (i < n): its document by bisection of the range's pair offsets, then from the document's temp place
__global__ __launch_bounds__(kDcThreads) void kdc_gather(const uint64_t *pair_off, const uint32_t *const *src, uint64_t n_docs,
                                                         uint64_t n, uint32_t *out) {
  for (uint64_t i = (uint64_t)blockIdx.x * kDcThreads + threadIdx.x; i < n; i += (uint64_t)gridDim.x * kDcThreads) {
    uint64_t lo = 0, hi = n_docs;  // the last d with pair_off[d] <= i
    while (hi - lo > 1) {
      const uint64_t mid = (lo + hi) >> 1;
      if (pair_off[mid] <= i) lo = mid; else hi = mid;
    }
    const uint32_t *p = src[lo] + 2 * (i - pair_off[lo]);
    out[2 * i] = p[0];
    out[2 * i + 1] = p[1];
  }
}

}  // namespace

void doccount_launch_sort(const DcItem *items, uint32_t n_items, const void *hits, uint32_t *n_pairs, void *stream) {
  if (n_items) hipLaunchKernelGGL(kdc_sort, dim3(n_items), dim3(kDcThreads), 0, (hipStream_t)stream, items, (const uint32_t *)hits, n_pairs);
}

void doccount_launch_range(const DcItem *items, uint32_t n_items, const void *hits, uint32_t n_keys, uint32_t range_keys,
                           uint32_t *n_pairs, void *stream) {
  if (n_items)
    hipLaunchKernelGGL(kdc_range, dim3(n_items), dim3(kDcThreads), 0, (hipStream_t)stream, items, (const uint32_t *)hits, n_keys,
                       range_keys, n_pairs);
}

void doccount_launch_add(const DcItem *slices, uint32_t n_slices, const void *hits, uint32_t *rows, uint32_t n_keys,
                         uint32_t max_blocks, void *stream) {
  if (n_slices)
    hipLaunchKernelGGL(kdc_add, dim3(std::max(1u, std::min(n_slices, max_blocks))), dim3(kDcThreads), 0, (hipStream_t)stream, slices,
                       n_slices, (const uint32_t *)hits, rows, n_keys);
}

void doccount_launch_compact(const DcItem *docs, uint32_t n_rows, uint32_t *rows, uint32_t n_keys, uint32_t *n_pairs, void *stream) {
  if (n_rows)
    hipLaunchKernelGGL((kdc_compact<uint32_t, true>), dim3(n_rows), dim3(kDcThreads), 0, (hipStream_t)stream, docs, rows, n_keys,
                       n_pairs);
}

void doccount_launch_compact64(const DcItem *doc, unsigned long long *row, uint32_t n_keys, uint32_t *n_pairs, void *stream) {
  hipLaunchKernelGGL((kdc_compact<unsigned long long, false>), dim3(1), dim3(kDcThreads), 0, (hipStream_t)stream, doc, row, n_keys,
                     n_pairs);
}

void doccount_launch_gather(const uint64_t *pair_off, const uint32_t *const *src, uint64_t n_docs, uint64_t n, void *out,
                            void *stream) {
  if (!n) return;
  const uint64_t blocks = std::min<uint64_t>((n + kDcThreads - 1) / kDcThreads, 8192);
  hipLaunchKernelGGL(kdc_gather, dim3((uint32_t)blocks), dim3(kDcThreads), 0, (hipStream_t)stream, pair_off, src, n_docs, n,
                     (uint32_t *)out);
}

}  // namespace aha
