// fold_piece.hpp -- what a lane of the staged copies does with one 16-byte piece (scan_fold.hip: k_fold_copy, k_fold2_copy,
// k_fold3_copy; scan_foldk.hip: k_foldk_copy): the piece as four words, its bytes, the halo of a three-byte fold loaded from
// memory (kc_fold3_halo) and the fold of the piece over a set of tables (kc_fold3_apply).  Device code only, every function
// inlined into the kernel that calls it.
#pragma once
#include <hip/hip_runtime.h>

#include "fold.hpp"

namespace aha {

namespace {

typedef uint32_t kc_v4u __attribute__((ext_vector_type(4)));

__device__ __forceinline__ kc_v4u kc_load16(const uint8_t *__restrict__ p) {
  kc_v4u v;
  __builtin_memcpy(&v, p, 16);  // (gfx950 global loads take unaligned addresses)
  return v;
}
__device__ __forceinline__ kc_v4u kc_fold16(kc_v4u v) { return kc_v4u{fold32(v[0]), fold32(v[1]), fold32(v[2]), fold32(v[3])}; }

__device__ __forceinline__ uint32_t kc_byte(const kc_v4u &v, int k) { return (v[k >> 2] >> ((k & 3) * 8)) & 0xFFu; }

// bit 7 of every byte of w that is >= 0x80 and whose low seven bits t lie in lo .. hi (fold32's sums: no carry between bytes)
__device__ __forceinline__ uint32_t kc_in(uint32_t t, uint32_t lo, uint32_t hi) {
  return (t + (0x80u - lo) * 0x01010101u) & ~(t + (0x7Fu - hi) * 0x01010101u);
}
// ... that is a lead byte whose character may move: 0xC2 .. 0xDF (the two-byte table), 0xE1, 0xE2, 0xEA, 0xEF (the only lead
// bytes of the code points F3 moves: fold3_table.hpp)
__device__ __forceinline__ uint32_t kc_live32(uint32_t w) {
  const uint32_t t = w & 0x7f7f7f7fu;
  return (kc_in(t, 0x42, 0x5F) | kc_in(t, 0x61, 0x62) | kc_in(t, 0x6A, 0x6A) | kc_in(t, 0x6F, 0x6F)) & w & 0x80808080u;
}

// fold3 of piece i (fold.hpp) in two steps, so that the neighbour loads of the four pieces a lane has in flight are in flight
// together.  kc_fold3_halo: up to two bytes before the piece and two after it decide what its own bytes become; they belong to
// other lanes (the next piece, another wave's 1 KiB, a piece a grid stride away) and are loaded from src only where they
// decide something and only inside [0, n): the two before when byte 0 is a continuation byte (the second or third byte of a
// character that began there; j0 > 0 is j0 >= 16, so j0 - 2 is inside), the one after when byte 15 is a lead byte or bytes 14,
// 15 open a triple, the second one after when byte 15 is the lead of a triple.  -> prev2 | prev << 8 | next << 16 | next2 << 24,
// 0 (neither a lead nor a continuation byte) where nothing was loaded; a piece of ASCII loads nothing.
__device__ __forceinline__ uint32_t kc_fold3_halo(const uint8_t *__restrict__ src, uint64_t i, uint64_t n, const kc_v4u &v) {
  if (!((v[0] | v[1] | v[2] | v[3]) & 0x80808080u)) return 0;
  const uint64_t j0 = i * 16;
  uint32_t h = 0;
  if (fold2_cont(kc_byte(v, 0)) && j0 > 0) h = (uint32_t)src[j0 - 2] | ((uint32_t)src[j0 - 1] << 8);
  const uint32_t b14 = kc_byte(v, 14), b15 = kc_byte(v, 15);
  if ((fold2_lead(b15) || fold3_lead(b15) || (fold3_lead(b14) && fold2_cont(b15))) && j0 + 16 < n) h |= (uint32_t)src[j0 + 16] << 16;
  if (fold3_lead(b15) && j0 + 17 < n) h |= (uint32_t)src[j0 + 17] << 24;
  return h;
}
// kc_fold3_apply: a piece of ASCII takes fold32 and nothing else.  kLive (opt-in, see fold3_live_test): so does a piece in
// which no character can move -- no live lead byte in it, none in the two bytes before it where its first character began
// there: Chinese text, whose lead bytes are 0xE3 .. 0xE9, then never reaches the tables.  Otherwise byte by byte from the
// byte and its neighbours (fold3_byte); the lanes that own the bytes of one triple each compute their byte from the same
// table entry.  Every lane writes its own 16 bytes and no others.
template <bool kLive>
__device__ __forceinline__ kc_v4u kc_fold3_apply(const Fold3Tables &T, const kc_v4u &v, uint32_t halo) {
  if (!((v[0] | v[1] | v[2] | v[3]) & 0x80808080u)) return kc_fold16(v);
  if (kLive && !(kc_live32(v[0]) | kc_live32(v[1]) | kc_live32(v[2]) | kc_live32(v[3]) | kc_live32(halo & 0xFFFFu))) return kc_fold16(v);
  uint32_t c[20];  // (bytes -2 .. 17 of the piece)
  c[0] = halo & 0xFFu;
  c[1] = (halo >> 8) & 0xFFu;
  c[18] = (halo >> 16) & 0xFFu;
  c[19] = halo >> 24;
#pragma unroll
  for (int k = 0; k < 16; k++) c[k + 2] = kc_byte(v, k);
  kc_v4u o = {0, 0, 0, 0};
#pragma unroll
  for (int k = 0; k < 16; k++) o[k >> 2] |= (uint32_t)fold3_byte(T, c[k], c[k + 1], c[k + 2], c[k + 3], c[k + 4]) << ((k & 3) * 8);
  return o;
}

}  // namespace

}  // namespace aha
