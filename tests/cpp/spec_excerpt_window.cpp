// excerpt_window.hpp against the definition of include/aha_hip.h (AHA_GREP_CONTEXT) written out as a plain loop in signed
// arithmetic: every byte string over {2-byte lead, 3-byte lead, 4-byte lead, continuation, ASCII} up to length 7 as one document,
// every hit inside it and every before / after from 0 to 8; up to length 5 every sub-range of the string as the document too,
// so the bytes next to the document are of every class.  The text sits in a heap buffer of exactly its length: built with
// -fsanitize=address,undefined by tests/test_excerpt_host.py, one byte read outside the buffer is reported.  Stand-alone, no GPU.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../aha_amd/csrc/excerpt_window.hpp"

static const uint8_t kAlphabet[5] = {0xC3, 0xE6, 0xF0, 0x80, 'A'};
static long long checked = 0, fails = 0;

static long long ref_w0(const uint8_t *t, long long a, long long s, long long before) {
  long long x = s - before;
  if (x < a) x = a;
  for (int k = 0; k < 3; k++)
    if (x > a && (t[x] & 0xC0) == 0x80) x -= 1;
  return x;
}

static long long ref_w1(const uint8_t *t, long long b, long long e, long long after) {
  long long x = e + after;
  if (x > b) x = b;
  for (int k = 0; k < 3; k++)
    if (x < b && (t[x] & 0xC0) == 0x80) x += 1;
  return x;
}

static void fail(const char *what, const uint8_t *t, int L, long long a, long long b, long long p, long long c, long long got,
                 long long want) {
  if (fails++ < 10) {
    std::printf("FAIL %s: text", what);
    for (int i = 0; i < L; i++) std::printf(" %02x", t[i]);
    std::printf(" doc [%lld, %lld) at %lld context %lld: %lld, want %lld\n", a, b, p, c, got, want);
  }
}

// the document [a, b) of the text t[0, L): every stretch [s, e) inside it, every context
static void check_doc(const uint8_t *t, int L, long long a, long long b) {
  for (long long s = a; s < b; s++)
    for (uint32_t before = 0; before <= 8; before++) {
      const long long got = (long long)aha::excerpt_w0(t, (uint64_t)a, (uint64_t)s, before), want = ref_w0(t, a, s, before);
      checked++;
      if (got != want || got < a || got > s) fail("w0", t, L, a, b, s, before, got, want);
    }
  for (long long e = a + 1; e <= b; e++)
    for (uint32_t after = 0; after <= 8; after++) {
      const long long got = (long long)aha::excerpt_w1(t, (uint64_t)b, (uint64_t)e, after), want = ref_w1(t, b, e, after);
      checked++;
      if (got != want || got > b || got < e) fail("w1", t, L, a, b, e, after, got, want);
    }
}

int main() {
  for (int L = 1; L <= 7; L++) {
    long long n = 1;
    for (int i = 0; i < L; i++) n *= 5;
    for (long long code = 0; code < n; code++) {
      std::vector<uint8_t> text((size_t)L);  // (exactly L bytes on the heap)
      long long c = code;
      for (int i = 0; i < L; i++, c /= 5) text[(size_t)i] = kAlphabet[c % 5];
      const uint8_t *t = text.data();
      check_doc(t, L, 0, L);
      if (L <= 5)
        for (long long a = 0; a < L; a++)
          for (long long b = a + 1; b <= L; b++)
            if (a != 0 || b != L) check_doc(t, L, a, b);
    }
  }
  {  // the largest context clips to the document's ends, where no byte is looked at
    std::vector<uint8_t> text(5, 0x80);
    checked += 2;
    if (aha::excerpt_w0(text.data(), 0, 4, aha::kExcerptMaxContext) != 0) fails++;
    if (aha::excerpt_w1(text.data(), 5, 1, aha::kExcerptMaxContext) != 5) fails++;
  }
  std::printf("%lld windows checked, %lld failure(s)\n", checked, fails);
  return fails ? 1 : 0;
}
