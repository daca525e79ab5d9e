// spec_foldk.cpp -- the host statement of the fold of AHA_OPT_FOLD_KANA (aha_amd/csrc/fold.hpp: foldk_bytes, foldk_byte) against
// the committed tables (foldk_table.hpp beside fold3_table.hpp and fold_table.hpp) and against the rule said position by
// position: foldk is fold3 with FK for F3, FK(cp) = K(cp) where K moves cp, else F3(cp).  K is written out here from the rule
// (hiragana + 0x60, the two iteration marks, the half-width katakana by their NFKC images), not read from the table.  A
// stand-alone program (its own main; no GPU, no library): built with -fsanitize=address,undefined by
// tests/test_fold_kana_host.py, every buffer on the heap at its exact length.
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../aha_amd/csrc/fold.hpp"

static int failures = 0;
#define CHECK(cond)                                              \
  do {                                                           \
    if (!(cond)) {                                               \
      if (failures++ < 20) fprintf(stderr, "line %d: %s\n", __LINE__, #cond); \
    }                                                            \
  } while (0)

typedef std::vector<uint8_t> Buf;

static bool lead2(uint8_t b) { return b >= 0xC2 && b <= 0xDF; }
static bool lead3(uint8_t b) { return b >= 0xE0 && b <= 0xEF; }
static bool cont(uint8_t b) { return b >= 0x80 && b <= 0xBF; }

// NFKC of U+FF66 .. U+FF9D (Unicode 13.0.0), one code point each
static const uint16_t kHalfwidth[56] = {
    0x30F2, 0x30A1, 0x30A3, 0x30A5, 0x30A7, 0x30A9, 0x30E3, 0x30E5, 0x30E7, 0x30C3, 0x30FC, 0x30A2, 0x30A4, 0x30A6,
    0x30A8, 0x30AA, 0x30AB, 0x30AD, 0x30AF, 0x30B1, 0x30B3, 0x30B5, 0x30B7, 0x30B9, 0x30BB, 0x30BD, 0x30BF, 0x30C1,
    0x30C4, 0x30C6, 0x30C8, 0x30CA, 0x30CB, 0x30CC, 0x30CD, 0x30CE, 0x30CF, 0x30D2, 0x30D5, 0x30D8, 0x30DB, 0x30DE,
    0x30DF, 0x30E0, 0x30E1, 0x30E2, 0x30E4, 0x30E6, 0x30E8, 0x30E9, 0x30EA, 0x30EB, 0x30EC, 0x30ED, 0x30EF, 0x30F3,
};

// K of a code point, 0 where K does not move it
static uint32_t K(uint32_t cp) {
  if (cp >= 0x3041 && cp <= 0x3096) return cp + 0x60;
  if (cp == 0x309D || cp == 0x309E) return cp + 0x60;
  if (cp >= 0xFF66 && cp <= 0xFF9D) return kHalfwidth[cp - 0xFF66];
  return 0;
}
static uint32_t F3(uint32_t cp) {
  if (cp < 0x800 || cp > 0xFFFF) return cp;
  const uint32_t k = aha::kFold3Index[(cp >> 6) - 0x20];
  return k ? aha::kFold3Live[(k - 1) * 64 + (cp & 63)] : cp;
}
// FK from the rule ...
static uint32_t FK(uint32_t cp) { return K(cp) ? K(cp) : F3(cp); }
// ... and from the two levels of the committed table
static uint32_t FKtable(uint32_t cp) {
  if (cp < 0x800 || cp > 0xFFFF) return cp;
  const uint32_t k = aha::kFoldKIndex[(cp >> 6) - 0x20];
  return k ? aha::kFoldKLive[(k - 1) * 64 + (cp & 63)] : cp;
}

// the rule position by position: which triple or pair position j lies in, if any
static Buf expect(const Buf &in) {
  const size_t n = in.size();
  Buf out(n);
  auto opens3 = [&](size_t j) { return j + 2 < n && lead3(in[j]) && cont(in[j + 1]) && cont(in[j + 2]); };
  auto opens2 = [&](size_t j) { return j + 1 < n && lead2(in[j]) && cont(in[j + 1]); };
  for (size_t j = 0; j < n; j++) {
    size_t at = n;  // where the triple that holds j begins
    for (size_t back = 0; back < 3 && back <= j; back++)
      if (opens3(j - back)) at = j - back;
    if (at != n) {
      const uint32_t f = FK(((in[at] & 0xFu) << 12) | ((in[at + 1] & 0x3Fu) << 6) | (in[at + 2] & 0x3Fu));
      const uint8_t enc[3] = {(uint8_t)(0xE0u | (f >> 12)), (uint8_t)(0x80u | ((f >> 6) & 0x3Fu)), (uint8_t)(0x80u | (f & 0x3Fu))};
      out[j] = enc[j - at];
    } else if (opens2(j)) {
      const uint32_t cp = ((in[j] & 0x1Fu) << 6) | (in[j + 1] & 0x3Fu);
      out[j] = (uint8_t)(0xC0u | (aha::kFold2Table[cp - 0x80] >> 6));
    } else if (j > 0 && opens2(j - 1)) {
      const uint32_t cp = ((in[j - 1] & 0x1Fu) << 6) | (in[j] & 0x3Fu);
      out[j] = (uint8_t)(0x80u | (aha::kFold2Table[cp - 0x80] & 0x3Fu));
    } else {
      out[j] = aha::fold8(in[j]);
    }
  }
  return out;
}

// foldk_bytes of a heap copy of exactly in.size() bytes
static Buf folded(const Buf &in) {
  uint8_t *p = new uint8_t[in.size()];
  if (!in.empty()) memcpy(p, in.data(), in.size());
  aha::foldk_bytes(p, in.size());
  Buf out(p, p + in.size());
  delete[] p;
  return out;
}
static Buf folded3(Buf in) {
  aha::fold3_bytes(in.data(), in.size());
  return in;
}

// the same buffer byte by byte through foldk_byte, the neighbours read from a heap copy of the exact length
static Buf bytewise(const Buf &in) {
  const size_t n = in.size();
  uint8_t *p = new uint8_t[n];
  if (n) memcpy(p, in.data(), n);
  Buf out(n);
  for (size_t j = 0; j < n; j++)
    out[j] = aha::foldk_byte(j > 1 ? p[j - 2] : 0u, j > 0 ? p[j - 1] : 0u, p[j], j + 1 < n ? p[j + 1] : 0u, j + 2 < n ? p[j + 2] : 0u);
  delete[] p;
  return out;
}

static Buf utf8(uint32_t cp) { return Buf{(uint8_t)(0xE0u | (cp >> 12)), (uint8_t)(0x80u | ((cp >> 6) & 0x3Fu)), (uint8_t)(0x80u | (cp & 0x3Fu))}; }

int main() {
  // the table: the two levels, FK = K over F3 at every code point of the BMP, idempotent, K and F3 never meet
  int live_blocks = 0, moved = 0, kmoved = 0;
  for (uint32_t b = 0; b < AHA_FOLDK_INDEX_ENTRIES; b++) {
    CHECK(aha::kFoldKIndex[b] <= AHA_FOLDK_LIVE_ENTRIES / 64);
    live_blocks += aha::kFoldKIndex[b] != 0;
    if (aha::kFold3Index[b]) CHECK(aha::kFoldKIndex[b] != 0);  // F3's live blocks are live here too
  }
  CHECK(AHA_FOLDK_INDEX_ENTRIES == 992 && live_blocks == 33 && AHA_FOLDK_LIVE_ENTRIES == 33 * 64);
  for (uint32_t b : {0x3040u, 0x3080u, 0xFF40u, 0xFF80u}) CHECK(aha::kFoldKIndex[(b >> 6) - 0x20] != 0 && aha::kFold3Index[(b >> 6) - 0x20] == 0);
  for (uint32_t cp = 0; cp <= 0xFFFF; cp++) {
    const uint32_t f = FKtable(cp);
    CHECK(f == FK(cp));
    CHECK(FKtable(f) == f);
    if (cp < 0x800 || (cp >= 0xD800 && cp <= 0xDFFF)) CHECK(f == cp);
    if (cp >= 0x800) CHECK(f >= 0x800 && f <= 0xFFFF && !(f >= 0xD800 && f <= 0xDFFF && f != cp));
    moved += f != cp;
    if (K(cp)) {
      kmoved++;
      CHECK(F3(cp) == cp && F3(K(cp)) == K(cp) && !K(K(cp)));  // K and F3 never meet; no image is a source
      CHECK(K(cp) >= 0x30A1 && K(cp) <= 0x30FE);                // every image is a katakana letter or mark
    }
  }
  CHECK(kmoved == 144 && moved == 679 + 144);

  // every code point of the BMP as UTF-8, alone and between neighbours: foldk_bytes and foldk_byte against the rule
  for (uint32_t cp = 0; cp <= 0xFFFF; cp++) {
    Buf in;
    if (cp < 0x80)
      in = Buf{(uint8_t)cp};
    else if (cp < 0x800)
      in = Buf{(uint8_t)(0xC0u | (cp >> 6)), (uint8_t)(0x80u | (cp & 0x3Fu))};
    else
      in = utf8(cp);
    const Buf out = folded(in);
    CHECK(out == expect(in) && bytewise(in) == out && folded(out) == out && out.size() == in.size());
    if (cp >= 0x800) {
      const bool plain = !(cp >= 0xD800 && cp <= 0xDFFF);
      CHECK(out == (plain ? utf8(FK(cp)) : in));
      CHECK(lead3(out[0]) && cont(out[1]) && cont(out[2]));
      if (!K(cp)) CHECK(out == folded3(in));  // where K moves nothing foldk is fold3
    }
    if (FK(cp) != cp || (cp & 0x3F) == 0) {
      Buf w{'A'};
      w.insert(w.end(), in.begin(), in.end());
      w.push_back('Z');
      const Buf fw = folded(w);
      CHECK(fw.front() == 'a' && fw.back() == 'z' && Buf(fw.begin() + 1, fw.end() - 1) == out && bytewise(w) == fw);
      if (in.size() == 3) {
        CHECK(folded(Buf{in[0], in[1]}) == (Buf{in[0], in[1]}));  // truncated: no fold
        CHECK(folded(Buf{in[1], in[2]}) == (Buf{in[1], in[2]}));  // without its lead
        CHECK(folded(Buf{in[0], in[1], 'x'}) == (Buf{in[0], in[1], 'x'}));
      }
    }
  }
  // overlong triples (cp < 0x800 written in three bytes) pass through
  for (uint32_t b = 0x80; b <= 0x9F; b++)
    for (uint32_t c = 0x80; c <= 0xBF; c++) {
      const Buf in{0xE0, (uint8_t)b, (uint8_t)c};
      CHECK(folded(in) == in && bytewise(in) == in);
    }

  // every buffer of up to 4 bytes over the corner alphabet (kana leads and continuation bytes among them), of 5 bytes over its
  // first nine
  const uint8_t alphabet[] = {'Q', 0xE3, 0x81, 0x82, 0xEF, 0xBD, 0xB1, 0xBE, 0xF0, 'a', 0xC3, 0xE0, 0xED, 0xC1, 0x9D, 0xA0};
  for (size_t n = 0; n <= 5; n++) {
    const size_t A = n < 5 ? sizeof(alphabet) : 9;
    size_t total = 1;
    for (size_t i = 0; i < n; i++) total *= A;
    for (size_t c = 0; c < total; c++) {
      Buf in(n);
      size_t x = c;
      for (size_t i = 0; i < n; i++, x /= A) in[i] = alphabet[x % A];
      const Buf out = folded(in);
      CHECK(out == expect(in));
      CHECK(bytewise(in) == out);
      CHECK(folded(out) == out);  // idempotent
    }
  }

  // corners by name
  CHECK(folded(Buf{}) == Buf{});
  CHECK(folded(Buf{0xE3, 0x81, 0x82}) == (Buf{0xE3, 0x82, 0xA2}));  // U+3042 hiragana a -> U+30A2: another second byte
  CHECK(folded(Buf{0xE3, 0x81, 0x81}) == (Buf{0xE3, 0x82, 0xA1}));  // U+3041 -> U+30A1
  CHECK(folded(Buf{0xE3, 0x82, 0x96}) == (Buf{0xE3, 0x83, 0xB6}));  // U+3096 -> U+30F6
  CHECK(folded(Buf{0xE3, 0x82, 0x9D}) == (Buf{0xE3, 0x83, 0xBD}));  // U+309D -> U+30FD
  CHECK(folded(Buf{0xE3, 0x82, 0x9F}) == (Buf{0xE3, 0x82, 0x9F}));  // U+309F stays
  CHECK(folded(Buf{0xE3, 0x82, 0x99}) == (Buf{0xE3, 0x82, 0x99}));  // the combining voiced mark stays
  CHECK(folded(Buf{0xE3, 0x82, 0xA2}) == (Buf{0xE3, 0x82, 0xA2}));  // katakana a is the representative
  CHECK(folded(Buf{0xEF, 0xBD, 0xB1}) == (Buf{0xE3, 0x82, 0xA2}));  // U+FF71 half-width a -> U+30A2: another lead byte
  CHECK(folded(Buf{0xEF, 0xBD, 0xB0}) == (Buf{0xE3, 0x83, 0xBC}));  // U+FF70 -> U+30FC
  CHECK(folded(Buf{0xEF, 0xBD, 0xA6}) == (Buf{0xE3, 0x83, 0xB2}));  // U+FF66 -> U+30F2
  CHECK(folded(Buf{0xEF, 0xBE, 0x9D}) == (Buf{0xE3, 0x83, 0xB3}));  // U+FF9D -> U+30F3
  CHECK(folded(Buf{0xEF, 0xBD, 0xA5}) == (Buf{0xEF, 0xBD, 0xA5}));  // U+FF65 stays
  CHECK(folded(Buf{0xEF, 0xBE, 0x9E}) == (Buf{0xEF, 0xBE, 0x9E}) && folded(Buf{0xEF, 0xBE, 0x9F}) == (Buf{0xEF, 0xBE, 0x9F}));
  // half-width ka + voiced mark: katakana ka and the unchanged mark, six bytes
  CHECK(folded(Buf{0xEF, 0xBD, 0xB6, 0xEF, 0xBE, 0x9E}) == (Buf{0xE3, 0x82, 0xAB, 0xEF, 0xBE, 0x9E}));
  CHECK(folded(Buf{0xEF, 0xBC, 0xA1}) == (Buf{0xEF, 0xBD, 0x81}));  // F3 still folds: U+FF21 -> U+FF41
  CHECK(folded(Buf{0xE4, 0xBD, 0xA0, 'X'}) == (Buf{0xE4, 0xBD, 0xA0, 'x'}));
  CHECK(folded(Buf{0xD0, 0xA0, 0xE3, 0x81, 0x82, 'B'}) == (Buf{0xD1, 0x80, 0xE3, 0x82, 0xA2, 'b'}));  // pair, triple, ASCII
  CHECK(folded(Buf{0xF0, 0x9F, 0x98, 0x80}) == (Buf{0xF0, 0x9F, 0x98, 0x80}));
  CHECK(folded(Buf{'A', 0xE3, 0x81}) == (Buf{'a', 0xE3, 0x81}));  // truncated at the end
  if (failures) {
    fprintf(stderr, "spec_foldk: %d failures\n", failures);
    return 1;
  }
  printf("spec_foldk: ok\n");
  return 0;
}
