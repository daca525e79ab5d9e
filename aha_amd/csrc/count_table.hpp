// count_table.hpp -- the per-workgroup LDS table of {id, 64-bit count} the count kernels sum into before they add to global
// memory (scan_count.hip: kc_visits, kc_chain; scan_feed.hip: kfd_count_windows).  Library-internal, device code only.
//
// Open addressing with a few probes; what does not find a place is added to global memory at once by the caller.  Counts
// are uint64 and wrap: a signed sum (kfd_count_windows adds -1 as 2^64 - 1) is exact modulo 2^64.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace aha {

constexpr int kCtLog2 = 12;
constexpr uint32_t kCtSlots = 1u << kCtLog2;  // 48 KiB of LDS: 4 B id + 8 B count per slot
constexpr uint32_t kCtEmpty = 0xFFFFFFFFu;
constexpr int kCtProbes = 8;

struct CtTable {
  uint32_t *id;
  unsigned long long *cnt;
};

__device__ __forceinline__ void ct_clear(const CtTable &t) {
  for (uint32_t i = threadIdx.x; i < kCtSlots; i += blockDim.x) {
    t.id[i] = kCtEmpty;
    t.cnt[i] = 0ull;
  }
}

// adds v to id's slot; false: no slot within kCtProbes (the caller adds to global memory)
__device__ __forceinline__ bool ct_add(const CtTable &t, uint32_t id, unsigned long long v) {
  const uint32_t h = (id * 0x9E3779B1u) >> (32 - kCtLog2);
  for (int p = 0; p < kCtProbes; p++) {
    const uint32_t s = (h + (uint32_t)p) & (kCtSlots - 1u);
    uint32_t k = t.id[s];
    if (k == kCtEmpty) k = atomicCAS(&t.id[s], kCtEmpty, id);
    if (k == kCtEmpty || k == id) {
      atomicAdd(&t.cnt[s], v);
      return true;
    }
  }
  return false;
}

// one event per live lane, +1 each (SIGNED: -1 where neg): the wave's first id is taken out by ballot for all lanes that
// hold it (one LDS add for all of them, so the table's atomics do not queue on the wave's most frequent id), then every
// other lane adds its own.  spill(id, v) adds to global memory what finds no slot.  All 64 lanes reach this call: the
// ballots need them.
template <bool SIGNED, class Spill>
__device__ __forceinline__ void ct_event(const CtTable &t, bool live, uint32_t id, bool neg, Spill spill) {
  const int lane = threadIdx.x & 63;
  const unsigned long long m = __ballot(live);
  if (!m) return;
  const int leader = __ffsll((long long)m) - 1;
  const uint32_t lid = (uint32_t)__shfl((int)id, leader, 64);
  const bool same = live && id == lid;
  unsigned long long v = (unsigned long long)__popcll(__ballot(same));
  if (SIGNED) v -= 2ull * (unsigned long long)__popcll(__ballot(same && neg));
  if (lane == leader && v && !ct_add(t, lid, v)) spill(lid, v);
  const unsigned long long mine = SIGNED && neg ? ~0ull : 1ull;
  if (live && !same && !ct_add(t, id, mine)) spill(id, mine);
}

}  // namespace aha
