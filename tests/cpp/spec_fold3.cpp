// spec_fold3.cpp -- the host statement of the fold of AHA_OPT_FOLD_BMP (aha_amd/csrc/fold.hpp: fold3_bytes, fold3_byte) against
// the committed tables (fold_table.hpp, fold3_table.hpp) and against the rule said position by position: j opens a triple when
// buf[j] is 0xE0 .. 0xEF, j + 2 < n and buf[j + 1], buf[j + 2] are 0x80 .. 0xBF; else a pair when buf[j] is 0xC2 .. 0xDF, j + 1 < n
// and buf[j + 1] is 0x80 .. 0xBF; a byte in neither gets fold8.  A stand-alone program (its own main; no GPU, no library):
// built with -fsanitize=address,undefined by tests/test_fold_bmp_host.py, every buffer on the heap at its exact length.
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

// F3 of a code point, from the two levels of the committed table; everything outside U+0800 .. U+FFFF is itself
static uint32_t F3(uint32_t cp) {
  if (cp < 0x800 || cp > 0xFFFF) return cp;
  const uint32_t k = aha::kFold3Index[(cp >> 6) - 0x20];
  return k ? aha::kFold3Live[(k - 1) * 64 + (cp & 63)] : cp;
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
      const uint32_t f = F3(((in[at] & 0xFu) << 12) | ((in[at + 1] & 0x3Fu) << 6) | (in[at + 2] & 0x3Fu));
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

// fold3_bytes of a heap copy of exactly in.size() bytes
static Buf folded(const Buf &in) {
  uint8_t *p = new uint8_t[in.size()];
  if (!in.empty()) memcpy(p, in.data(), in.size());
  aha::fold3_bytes(p, in.size());
  Buf out(p, p + in.size());
  delete[] p;
  return out;
}

// the same buffer byte by byte through fold3_byte, the neighbours read from a heap copy of the exact length
static Buf bytewise(const Buf &in) {
  const aha::Fold3Tables T = {aha::kFold2Table, aha::kFold3Index, aha::kFold3Live};
  const size_t n = in.size();
  uint8_t *p = new uint8_t[n];
  if (n) memcpy(p, in.data(), n);
  Buf out(n);
  for (size_t j = 0; j < n; j++)
    out[j] = aha::fold3_byte(T, j > 1 ? p[j - 2] : 0u, j > 0 ? p[j - 1] : 0u, p[j], j + 1 < n ? p[j + 1] : 0u, j + 2 < n ? p[j + 2] : 0u);
  delete[] p;
  return out;
}

static Buf utf8(uint32_t cp) { return Buf{(uint8_t)(0xE0u | (cp >> 12)), (uint8_t)(0x80u | ((cp >> 6) & 0x3Fu)), (uint8_t)(0x80u | (cp & 0x3Fu))}; }

int main() {
  // the table: in the block, idempotent, the counts of the header
  int moved = 0, lead_changes = 0, second_changes = 0, live_blocks = 0;
  for (uint32_t b = 0; b < AHA_FOLD3_INDEX_ENTRIES; b++) {
    CHECK(aha::kFold3Index[b] <= AHA_FOLD3_LIVE_ENTRIES / 64);
    live_blocks += aha::kFold3Index[b] != 0;
  }
  CHECK(live_blocks == 29 && AHA_FOLD3_LIVE_ENTRIES == 29 * 64);
  for (uint32_t cp = 0x800; cp <= 0xFFFF; cp++) {
    const uint32_t f = F3(cp);
    CHECK(f >= 0x800 && f <= 0xFFFF && !(f >= 0xD800 && f <= 0xDFFF && f != cp));
    CHECK(F3(f) == f);
    if (cp >= 0xD800 && cp <= 0xDFFF) CHECK(f == cp);
    moved += f != cp;
    lead_changes += (f >> 12) != (cp >> 12);
    second_changes += (f >> 6) != (cp >> 6);
    if (f != cp) {
      const uint32_t l = 0xE0u | (cp >> 12);
      CHECK(l == 0xE1 || l == 0xE2 || l == 0xEA || l == 0xEF);  // (what the device pass's live-lead test relies on)
    }
  }
  CHECK(moved == 679 && lead_changes == 124 && second_changes == 255);

  // every triple (lead, c1, c2) with the three classes of neighbours: against the table, lengths and lead bytes kept
  for (uint32_t a = 0xE0; a <= 0xEF; a++)
    for (uint32_t b = 0x80; b <= 0xBF; b++)
      for (uint32_t c = 0x80; c <= 0xBF; c++) {
        const Buf in{(uint8_t)a, (uint8_t)b, (uint8_t)c};
        const uint32_t cp = ((a & 0xFu) << 12) | ((b & 0x3Fu) << 6) | (c & 0x3Fu);
        const Buf out = folded(in);
        const bool plain = cp >= 0x800 && !(cp >= 0xD800 && cp <= 0xDFFF);
        CHECK(out == (plain ? utf8(F3(cp)) : in));  // overlong forms and surrogates byte for byte
        CHECK(lead3(out[0]) && cont(out[1]) && cont(out[2]));
        CHECK(bytewise(in) == out);
        if (F3(cp) != cp || cp < 0x840) {
          const Buf w = folded(Buf{'A', (uint8_t)a, (uint8_t)b, (uint8_t)c, 'Z'});
          CHECK(w[0] == 'a' && w[1] == out[0] && w[2] == out[1] && w[3] == out[2] && w[4] == 'z');
          CHECK(folded(Buf{(uint8_t)a, (uint8_t)b}) == (Buf{(uint8_t)a, (uint8_t)b}));  // truncated: no fold
          CHECK(folded(Buf{(uint8_t)b, (uint8_t)c}) == (Buf{(uint8_t)b, (uint8_t)c}));  // without its lead
        }
      }
  // every three-byte buffer whose first byte is no triple lead is what its parts are under the pair rule / fold8
  for (uint32_t a = 0; a < 256; a++)
    for (uint32_t b = 0; b < 256; b += 7)
      for (uint32_t c = 0; c < 256; c += 11) {
        const Buf in{(uint8_t)a, (uint8_t)b, (uint8_t)c};
        CHECK(folded(in) == expect(in));
        CHECK(bytewise(in) == expect(in));
      }

  // every buffer of up to 4 bytes over the corner alphabet, of 5 bytes over its first nine
  const uint8_t alphabet[] = {'Q', 0xD0, 0xA0, 0x80, 0xBC, 0xE1, 0xEF, 0xE4, 0xF0, 'a', 0xC3, 0xE0, 0xED, 0xC1};
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
  CHECK(folded(Buf{0xE1}) == Buf{0xE1} && folded(Buf{'A', 0xE1, 0xBA}) == (Buf{'a', 0xE1, 0xBA}));  // truncated at the end
  CHECK(folded(Buf{0xBC, 0xA1}) == (Buf{0xBC, 0xA1}));                                              // continuation bytes alone
  CHECK(folded(Buf{0xEF, 0xBC, 0xA1}) == (Buf{0xEF, 0xBD, 0x81}));                                  // U+FF21 -> U+FF41
  CHECK(folded(Buf{0xEF, 0xEF, 0xBC, 0xA1}) == (Buf{0xEF, 0xEF, 0xBD, 0x81}));                      // a lead in front of a triple
  CHECK(folded(Buf{0xE1, 0x82, 0xA0}) == (Buf{0xE2, 0xB4, 0x80}));                                  // U+10A0 -> U+2D00: another lead
  CHECK(folded(Buf{0xE1, 0x8E, 0xA0}) == (Buf{0xEA, 0xAD, 0xB0}));                                  // U+13A0 -> U+AB70
  CHECK(folded(Buf{0xE1, 0xBB, 0x86}) == (Buf{0xE1, 0xBB, 0x87}));                                  // U+1EC6 -> U+1EC7 (Vietnamese)
  CHECK(folded(Buf{0xE1, 0xBC, 0x88}) == (Buf{0xE1, 0xBC, 0x80}));                                  // U+1F08 -> U+1F00 (polytonic Greek)
  CHECK(folded(Buf{0xE2, 0x84, 0xAA}) == (Buf{0xE2, 0x84, 0xAA}));                                  // the Kelvin sign stays
  CHECK(folded(Buf{0xE1, 0xBA, 0x9E}) == (Buf{0xE1, 0xBA, 0x9E}));                                  // U+1E9E stays
  CHECK(folded(Buf{0xE4, 0xBD, 0xA0, 'X'}) == (Buf{0xE4, 0xBD, 0xA0, 'x'}));                        // a Chinese character
  CHECK(folded(Buf{0xE0, 0x80, 0x80}) == (Buf{0xE0, 0x80, 0x80}) && folded(Buf{0xED, 0xA0, 0x80}) == (Buf{0xED, 0xA0, 0x80}));
  CHECK(folded(Buf{0xF0, 0x9F, 0x98, 0x80}) == (Buf{0xF0, 0x9F, 0x98, 0x80}));                      // a four-byte character
  CHECK(folded(Buf{0xD0, 0xA0, 0xEF, 0xBC, 0xA1, 'B'}) == (Buf{0xD1, 0x80, 0xEF, 0xBD, 0x81, 'b'}));  // pair, triple, ASCII

  // where no triple is, fold3 is fold2
  {
    Buf in;
    for (int i = 0; i < 256; i++) {
      in.push_back((uint8_t)i);
      in.push_back((uint8_t)(i < 0xE0 || i > 0xEF ? 0xA0 : '|'));
      in.push_back('|');
    }
    Buf want = in;
    aha::fold2_bytes(want.data(), want.size());
    CHECK(folded(in) == want);
  }
  if (failures) {
    fprintf(stderr, "spec_fold3: %d failures\n", failures);
    return 1;
  }
  printf("spec_fold3: ok\n");
  return 0;
}
