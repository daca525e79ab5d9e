// spec_fold2.cpp -- the host statement of the simple fold (aha_amd/csrc/fold.hpp: fold2_bytes) against the committed table
// (fold_table.hpp) and against the rule said position by position: j opens a pair when buf[j] is 0xC2 .. 0xDF, j + 1 < n and
// buf[j + 1] is 0x80 .. 0xBF; a byte in no pair gets fold8.  A stand-alone program (its own main; no GPU, no library): built
// with -fsanitize=address,undefined by tests/test_fold_simple_host.py, every buffer on the heap at its exact length.
#include <cstdio>
#include <cstring>
#include <string>
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

static bool lead(uint8_t b) { return b >= 0xC2 && b <= 0xDF; }
static bool cont(uint8_t b) { return b >= 0x80 && b <= 0xBF; }

// the rule position by position, from the table
static Buf expect(const Buf &in) {
  Buf out(in.size());
  for (size_t j = 0; j < in.size(); j++) {
    const bool opens = lead(in[j]) && j + 1 < in.size() && cont(in[j + 1]);
    const bool closes = j > 0 && lead(in[j - 1]) && cont(in[j]);
    if (opens) {
      const uint32_t cp = ((in[j] & 0x1Fu) << 6) | (in[j + 1] & 0x3Fu);
      out[j] = (uint8_t)(0xC0u | (aha::kFold2Table[cp - 0x80] >> 6));
    } else if (closes) {
      const uint32_t cp = ((in[j - 1] & 0x1Fu) << 6) | (in[j] & 0x3Fu);
      out[j] = (uint8_t)(0x80u | (aha::kFold2Table[cp - 0x80] & 0x3Fu));
    } else {
      out[j] = aha::fold8(in[j]);
    }
  }
  return out;
}

// fold2_bytes of a heap copy of exactly in.size() bytes
static Buf folded(const Buf &in) {
  uint8_t *p = new uint8_t[in.size()];
  if (!in.empty()) memcpy(p, in.data(), in.size());
  aha::fold2_bytes(p, in.size());
  Buf out(p, p + in.size());
  delete[] p;
  return out;
}

static Buf bytes(const char *s) { return Buf((const uint8_t *)s, (const uint8_t *)s + strlen(s)); }

int main() {
  // the table: in the block, idempotent
  int moved = 0, lead_changes = 0;
  for (uint32_t cp = 0x80; cp < 0x800; cp++) {
    const uint32_t f = aha::kFold2Table[cp - 0x80];
    CHECK(f >= 0x80 && f < 0x800);
    CHECK(aha::kFold2Table[f - 0x80] == f);
    moved += f != cp;
    lead_changes += (f >> 6) != (cp >> 6);
  }
  CHECK(moved == 450 && lead_changes == 108);

  // every two-byte buffer: the (lead, cont) pairs against the table, everything else against fold8
  for (uint32_t a = 0; a < 256; a++)
    for (uint32_t b = 0; b < 256; b++) {
      const Buf in{(uint8_t)a, (uint8_t)b};
      const Buf out = folded(in);
      if (lead((uint8_t)a) && cont((uint8_t)b)) {
        const uint32_t cp = ((a & 0x1Fu) << 6) | (b & 0x3Fu), f = aha::kFold2Table[cp - 0x80];
        CHECK(out[0] == (0xC0u | (f >> 6)) && out[1] == (0x80u | (f & 0x3Fu)));
        CHECK(lead(out[0]) && cont(out[1]));  // a lead byte stays a lead byte
        // ... the same between two ASCII letters, and behind a lead byte that has its own continuation byte
        const Buf w = folded(Buf{'A', (uint8_t)a, (uint8_t)b, 'Z'});
        CHECK(w[0] == 'a' && w[1] == out[0] && w[2] == out[1] && w[3] == 'z');
      } else {
        CHECK(out[0] == aha::fold8((uint8_t)a) && out[1] == aha::fold8((uint8_t)b));
      }
      CHECK(out == expect(in));
    }

  // every buffer of up to 5 bytes over the corner alphabet
  const uint8_t alphabet[] = {'a', 'Q', 0xD0, 0xD1, 0xCE, 0xC3, 0xA0, 0x80, 0xBF, 0xE4, 0xC1};
  const size_t A = sizeof(alphabet);
  for (size_t n = 0; n <= 5; n++) {
    size_t total = 1;
    for (size_t i = 0; i < n; i++) total *= A;
    for (size_t c = 0; c < total; c++) {
      Buf in(n);
      size_t x = c;
      for (size_t i = 0; i < n; i++, x /= A) in[i] = alphabet[x % A];
      const Buf out = folded(in);
      CHECK(out == expect(in));
      CHECK(folded(out) == out);  // idempotent
    }
  }

  // corners by name
  CHECK(folded(Buf{}) == Buf{});
  CHECK(folded(Buf{0xD0}) == Buf{0xD0});                                  // a lead byte at the end
  CHECK(folded(Buf{'A', 0xD0}) == (Buf{'a', 0xD0}));
  CHECK(folded(Buf{0xA0}) == Buf{0xA0});                                  // a lone continuation byte
  CHECK(folded(Buf{0xA0, 0xA0, 0xA0}) == (Buf{0xA0, 0xA0, 0xA0}));
  CHECK(folded(Buf{0xC0, 0x80}) == (Buf{0xC0, 0x80}) && folded(Buf{0xC1, 0x81}) == (Buf{0xC1, 0x81}));
  CHECK(folded(Buf{0xE4, 0xB8, 0xAD, 'X'}) == (Buf{0xE4, 0xB8, 0xAD, 'x'}));  // a three-byte character
  CHECK(folded(Buf{0xF0, 0x9F, 0x98, 0x80}) == (Buf{0xF0, 0x9F, 0x98, 0x80}));  // a four-byte character
  CHECK(folded(Buf{0xD0, 0xA0}) == (Buf{0xD1, 0x80}));                    // U+0420 -> U+0440: another lead byte
  CHECK(folded(Buf{0xCE, 0xA0}) == (Buf{0xCF, 0x80}));                    // U+03A0 -> U+03C0
  CHECK(folded(Buf{0xD0, 0xD0, 0xA0}) == (Buf{0xD0, 0xD1, 0x80}));        // a lead byte in front of a pair
  CHECK(folded(bytes("\xD0\x9F\xD0\xA0\xD0\x98\xD0\x92\xD0\x95\xD0\xA2")) == bytes("\xD0\xBF\xD1\x80\xD0\xB8\xD0\xB2\xD0\xB5\xD1\x82"));
  CHECK(folded(bytes("\xC3\x89" "COLE")) == bytes("\xC3\xA9" "cole"));
  CHECK(folded(bytes("\xC3\x9F")) == bytes("\xC3\x9F") && folded(bytes("\xC4\xB0\xC4\xB1\xC5\xBF")) == bytes("\xC4\xB0\xC4\xB1\xC5\xBF"));
  CHECK(folded(bytes("\xC2\xB5")) == bytes("\xCE\xBC") && folded(bytes("\xCF\x82")) == bytes("\xCF\x83"));  // micro sign, final sigma

  // bytes outside pairs agree with the ASCII fold of a whole buffer
  {
    Buf in;
    for (int i = 0; i < 256; i++) {
      in.push_back((uint8_t)i);
      in.push_back('|');
    }
    Buf want = in;
    aha::fold_bytes(want.data(), want.size());
    CHECK(folded(in) == want);
  }
  if (failures) {
    fprintf(stderr, "spec_fold2: %d failures\n", failures);
    return 1;
  }
  printf("spec_fold2: ok\n");
  return 0;
}
