// fold.hpp -- the case folds of AHA_OPT_FOLD_ASCII, AHA_OPT_FOLD_SIMPLE and AHA_OPT_FOLD_BMP and the kana fold of
// AHA_OPT_FOLD_KANA (include/aha_hip.h), host and device.  The ONLY place the rules are written down.
// ASCII: fold(b) = b + 32 for 0x41 <= b <= 0x5A ('A' .. 'Z'), b otherwise.  Bytes >= 0x80, '@', '[', '`' and '{' stay,
// lengths and UTF-8 lead bytes never change.  Compile folds a copy of the keys with it (capi.cpp), the prefix-filter engine
// folds its text loads (scan_filter.hip), every other engine reads a copy folded on the way (scan_fold.hip).
// SIMPLE: fold2 of one buffer, byte for byte as long as its input.  At every j with buf[j] in 0xC2 .. 0xDF, j + 1 < n and
// buf[j + 1] in 0x80 .. 0xBF the pair is the UTF-8 of a code point cp in U+0080 .. U+07FF and becomes the UTF-8 of F(cp)
// (fold_table.hpp: two bytes again, a lead byte stays a lead byte); such pairs cannot overlap; every other byte gets the ASCII
// fold.  A rule on bytes, not on well-formed text: a stray continuation byte, a lead byte at the end, 0xC0, 0xC1 and the
// bytes of three- and four-byte sequences stay.  Keys are folded one by one, a batch document by document (fold2_bytes here,
// scan_fold.hip there): a lead byte never pairs with a byte of the next key or document.
// BMP: fold3 of one buffer, as long as its input again.  At every j with buf[j] in 0xE0 .. 0xEF, j + 2 < n and buf[j + 1],
// buf[j + 2] both in 0x80 .. 0xBF the triple becomes the UTF-8 of F3(cp) (fold3_table.hpp: three bytes again), where an overlong
// form (cp < 0x800) and a surrogate are their own F3; else the pair rule of fold2; else the ASCII fold.  A lead byte is never a
// continuation byte, so triples and pairs cannot overlap and every output byte is a function of the byte and its two
// neighbours on each side (fold3_byte).  A truncated triple, four-byte sequences and 0xF5 .. 0xFF stay.  33 code points whose
// only case partner is written in another number of bytes (the Kelvin, ohm and Angstrom signs, U+1E9E, U+1C80 .. U+1C87,
// U+2C62 and others: include/aha_hip.h has the list) stay.
// KANA (AHA_OPT_FOLD_KANA): foldk is fold3 with FK for F3 (foldk_table.hpp): FK(cp) = K(cp) where K moves cp -- hiragana U+3041 ..
// U+3096, U+309D, U+309E and the half-width katakana U+FF66 .. U+FF9D, each to its katakana letter --, else F3(cp).  The byte
// logic is fold3's; only the tables differ (Fold3Tables); the device pass is scan_foldk.hip.
#pragma once
#include <cstddef>
#include <cstdint>

#include "fold3_table.hpp"
#include "fold_table.hpp"
#include "foldk_table.hpp"

#ifndef AHA_HD
#if defined(__HIPCC__)
#define AHA_HD __host__ __device__
#else
#define AHA_HD
#endif
#endif

namespace aha {

AHA_HD inline uint8_t fold8(uint8_t b) { return (uint8_t)(b - 0x41u) < 26u ? (uint8_t)(b + 32u) : b; }

// Four bytes at once, no carry from one byte into the next: with t = the low seven bits of every byte, bit 7 of t + 0x3f is
// set for t >= 0x41 and bit 7 of t + 0x25 for t >= 0x5b, so m has bit 7 of exactly the bytes in 'A' .. 'Z' (~w: not those
// with their own bit 7 set); m >> 2 is their 0x20.
AHA_HD inline uint32_t fold32(uint32_t w) {
  const uint32_t t = w & 0x7f7f7f7fu;
  const uint32_t m = (t + 0x3f3f3f3fu) & ~(t + 0x25252525u) & ~w & 0x80808080u;
  return w | (m >> 2);
}

// 16 bytes as four words (any type with .x .y .z .w or operator[] would do: the kernels' own vector types differ)
AHA_HD inline void fold128(uint32_t &a, uint32_t &b, uint32_t &c, uint32_t &d) {
  a = fold32(a);
  b = fold32(b);
  c = fold32(c);
  d = fold32(d);
}

inline void fold_bytes(uint8_t *p, size_t n) {
  for (size_t i = 0; i < n; i++) p[i] = fold8(p[i]);
}

// ---- the simple fold: the pieces both sides share (the table itself comes as an argument: the device reads its copy in LDS)
AHA_HD inline bool fold2_lead(uint32_t b) { return b - 0xC2u < 30u; }           // 0xC2 .. 0xDF
AHA_HD inline bool fold2_cont(uint32_t b) { return (b & 0xC0u) == 0x80u; }      // 0x80 .. 0xBF
// F(cp) of the pair (lead, cont); both hold, so 0x80 <= cp <= 0x7FF
AHA_HD inline uint32_t fold2_pair(const uint16_t *table, uint32_t lead, uint32_t cont) {
  return table[(((lead & 0x1Fu) << 6) | (cont & 0x3Fu)) - 0x80u];
}
// One byte of fold2 from the byte and its two neighbours (0 -- neither a lead nor a continuation byte -- where there is none):
// the lead byte and the continuation byte of a pair come from the same table entry, whoever asks for them.
AHA_HD inline uint8_t fold2_byte(const uint16_t *table, uint32_t prev, uint32_t cur, uint32_t next) {
  if (fold2_lead(cur) && fold2_cont(next)) return (uint8_t)(0xC0u | (fold2_pair(table, cur, next) >> 6));
  if (fold2_cont(cur) && fold2_lead(prev)) return (uint8_t)(0x80u | (fold2_pair(table, prev, cur) & 0x3Fu));
  return fold8((uint8_t)cur);
}

// fold2 of one buffer in place (one key, one document): the host's statement of the rule
inline void fold2_bytes(uint8_t *p, size_t n) {
  for (size_t i = 0; i < n; i++) {
    if (fold2_lead(p[i]) && i + 1 < n && fold2_cont(p[i + 1])) {
      const uint32_t f = fold2_pair(kFold2Table, p[i], p[i + 1]);
      p[i] = (uint8_t)(0xC0u | (f >> 6));
      p[i + 1] = (uint8_t)(0x80u | (f & 0x3Fu));
      i++;
    } else {
      p[i] = fold8(p[i]);
    }
  }
}

// ---- the fold of the three-byte characters (AHA_OPT_FOLD_BMP): the two-byte table, and F3 in two levels (fold3_table.hpp)
struct Fold3Tables {
  const uint16_t *pair;   // kFold2Table or its copy in LDS
  const uint8_t *index;   // kFold3Index -- or kFoldKIndex: the same form, FK for F3
  const uint16_t *live;   // kFold3Live / kFoldKLive
};
AHA_HD inline bool fold3_lead(uint32_t b) { return (b & 0xF0u) == 0xE0u; }      // 0xE0 .. 0xEF
// F3(cp) of the triple (lead, c1, c2), all three hold; an overlong form (cp < 0x800) is its own fold, and so is a surrogate
// (its block is not live): encoded again they are the bytes they were
// (both look-ups are made whatever they find, at an entry that exists, and chosen afterwards: on the device the lanes of a
// wave then stay together)
AHA_HD inline uint32_t fold3_triple(const Fold3Tables &T, uint32_t lead, uint32_t c1, uint32_t c2) {
  const uint32_t cp = ((lead & 0xFu) << 12) | ((c1 & 0x3Fu) << 6) | (c2 & 0x3Fu);
  const uint32_t block = cp >> 6;
  const uint32_t k = block < 0x20u ? 0u : T.index[block < 0x20u ? 0u : block - 0x20u];
  const uint32_t f = T.live[(k ? k - 1u : 0u) * 64u + (cp & 63u)];
  return k ? f : cp;
}
// One byte of fold3 from the byte and its two neighbours on each side (0 where there is none): the three bytes of a triple
// come from the same table entry, whoever asks for them.
// Which byte of which triple or pair `cur` is comes first, as flags; then one look-up for the triple, or one for the pair.
AHA_HD inline uint8_t fold3_byte(const Fold3Tables &T, uint32_t prev2, uint32_t prev, uint32_t cur, uint32_t next, uint32_t next2) {
  const bool cc = fold2_cont(cur), nc = fold2_cont(next);
  const bool first = fold3_lead(cur) & nc & fold2_cont(next2);
  const bool second = cc & fold3_lead(prev) & nc;
  const bool third = cc & fold2_cont(prev) & fold3_lead(prev2);
  if (first | second | third) {
    const uint32_t f = fold3_triple(T, first ? cur : second ? prev : prev2, first ? next : second ? cur : prev, first ? next2 : second ? next : cur);
    return (uint8_t)(first ? 0xE0u | (f >> 12) : second ? 0x80u | ((f >> 6) & 0x3Fu) : 0x80u | (f & 0x3Fu));
  }
  const bool opens = fold2_lead(cur) & nc, closes = cc & fold2_lead(prev);
  if (opens | closes) {
    const uint32_t f = fold2_pair(T.pair, opens ? cur : prev, opens ? next : cur);
    return (uint8_t)(opens ? 0xC0u | (f >> 6) : 0x80u | (f & 0x3Fu));
  }
  return fold8((uint8_t)cur);
}

// fold3 of one buffer in place (one key, one document) with the tables T: the host's statement of the rule
inline void fold3_bytes_with(const Fold3Tables &T, uint8_t *p, size_t n) {
  for (size_t i = 0; i < n; i++) {
    if (fold3_lead(p[i]) && i + 2 < n && fold2_cont(p[i + 1]) && fold2_cont(p[i + 2])) {
      const uint32_t f = fold3_triple(T, p[i], p[i + 1], p[i + 2]);
      p[i] = (uint8_t)(0xE0u | (f >> 12));
      p[i + 1] = (uint8_t)(0x80u | ((f >> 6) & 0x3Fu));
      p[i + 2] = (uint8_t)(0x80u | (f & 0x3Fu));
      i += 2;
    } else if (fold2_lead(p[i]) && i + 1 < n && fold2_cont(p[i + 1])) {
      const uint32_t f = fold2_pair(T.pair, p[i], p[i + 1]);
      p[i] = (uint8_t)(0xC0u | (f >> 6));
      p[i + 1] = (uint8_t)(0x80u | (f & 0x3Fu));
      i++;
    } else {
      p[i] = fold8(p[i]);
    }
  }
}
inline void fold3_bytes(uint8_t *p, size_t n) { fold3_bytes_with(Fold3Tables{kFold2Table, kFold3Index, kFold3Live}, p, n); }
// foldk of one buffer in place (AHA_OPT_FOLD_KANA): the same rule over FK's tables
inline void foldk_bytes(uint8_t *p, size_t n) { fold3_bytes_with(Fold3Tables{kFold2Table, kFoldKIndex, kFoldKLive}, p, n); }
// ... and one byte of it from the byte and its neighbours
inline uint8_t foldk_byte(uint32_t prev2, uint32_t prev, uint32_t cur, uint32_t next, uint32_t next2) {
  return fold3_byte(Fold3Tables{kFold2Table, kFoldKIndex, kFoldKLive}, prev2, prev, cur, next, next2);
}

}  // namespace aha
