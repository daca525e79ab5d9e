// token_rule.hpp against the bytewise rule of include/aha_hip.h (AHA_SELECT_TOKENS), the way ktk_starts of scan_tokens.hip
// drives it: word by word, the continuation bits from 16-byte loads aligned to the address.  Random texts over {ASCII, 2-, 3-,
// 4-byte lead, continuation, 0xFF} of every length around one and two word borders, cut into documents anywhere and covered by
// random non-overlapping selected hits, at EVERY alignment of the text (head = 0 .. 15 bytes in front of the first aligned
// address, so a word border of the masks falls on every offset of a loaded piece), in both gap modes; then the named cases: a
// three-byte character whose lead is the last byte of a word, a hit that ends on a word border followed by a gap or by another
// hit, a stray run of continuation bytes.  The text sits at the end of a heap buffer of exactly its length: built with
// -fsanitize=address,undefined by tests/test_tokens_host.py, one byte read behind it is reported.  Stand-alone, no GPU.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../aha_amd/csrc/token_rule.hpp"

static long long checked = 0, fails = 0;
static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd(uint32_t n) {
  rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull;
  return (uint32_t)(rng_state >> 33) % n;
}

struct Case {
  std::vector<uint8_t> text;
  std::vector<uint8_t> doc_start, select, inside;  // one flag per position
};

// the rule, position by position
static std::vector<uint8_t> by_bytes(const Case &c, bool gap_runs) {
  const size_t n = c.text.size();
  std::vector<uint8_t> t(n, 0);
  for (size_t p = 0; p < n; p++) {
    const bool b = !c.inside[p] && (c.doc_start[p] || (p > 0 && c.inside[p - 1]) || (!gap_runs && (c.text[p] & 0xC0) != 0x80));
    t[p] = c.select[p] || b;
  }
  return t;
}

static std::vector<uint32_t> words_of(const std::vector<uint8_t> &flags) {
  std::vector<uint32_t> w((flags.size() + 31) / 32, 0u);
  for (size_t p = 0; p < flags.size(); p++)
    if (flags[p]) w[p >> 5] |= 1u << (p & 31);
  return w;
}

// the rule, word by word, over the text placed `head` bytes in front of a 16-byte aligned address
static void check(const Case &c, uint32_t head_want) {
  const uint64_t nb = c.text.size(), n_words = (nb + 31) / 32;
  const size_t lead_in = (16 - head_want) % 16;  // buf is aligned; corpus = buf + lead_in ends with the buffer
  void *mem = nullptr;
  if (posix_memalign(&mem, 16, lead_in + nb + (lead_in + nb == 0)) != 0) std::abort();
  uint8_t *buf = static_cast<uint8_t *>(mem);
  std::memset(buf, 0x41, lead_in);
  uint8_t *corpus = buf + lead_in;
  if (nb) std::memcpy(corpus, c.text.data(), nb);
  const uint32_t head = (uint32_t)(nb < (16 - reinterpret_cast<uintptr_t>(corpus) % 16) % 16 ? nb : (16 - reinterpret_cast<uintptr_t>(corpus) % 16) % 16);
  const uint8_t *text = corpus + head;
  const uint64_t na = nb - head;
  const std::vector<uint32_t> sel = words_of(c.select), ins = words_of(c.inside), ds = words_of(c.doc_start);
  for (int gap = 0; gap < 2; gap++) {
    const std::vector<uint32_t> want = words_of(by_bytes(c, gap != 0));
    for (uint64_t w = 0; w < n_words; w++) {
      const uint32_t cur = aha::token_cont32(text, w, na);
      const uint32_t prev = w ? aha::token_cont32(text, w - 1, na) : aha::token_cont_head(corpus, head);
      const uint32_t got = aha::token_starts(sel[w], ins[w], ds[w], w ? ins[w - 1] >> 31 : 0u, aha::token_funnel(prev, cur, head), gap != 0,
                                             aha::token_valid(w, nb));
      checked++;
      if (got != want[w] && fails++ < 10)
        std::printf("FAIL head %u length %llu gap_runs %d word %llu: %08x, want %08x\n", head, (unsigned long long)nb, gap,
                    (unsigned long long)w, got, want[w]);
    }
  }
  std::free(mem);
}

static Case blank(size_t n, uint8_t fill) {
  Case c;
  c.text.assign(n, fill);
  c.doc_start.assign(n, 0);
  c.select.assign(n, 0);
  c.inside.assign(n, 0);
  if (n) c.doc_start[0] = 1;
  return c;
}

static void add_hit(Case &c, size_t s, size_t e) {
  c.select[s] = 1;
  for (size_t p = s; p < e; p++) c.inside[p] = 1;
}

static Case random_case(size_t n) {
  static const uint8_t kAlphabet[6] = {'A', 0xC3, 0xE6, 0xF0, 0x80, 0xFF};
  Case c = blank(n, 0);
  for (size_t p = 0; p < n; p++) c.text[p] = kAlphabet[rnd(6)];
  for (size_t p = 1; p < n; p++) c.doc_start[p] = rnd(12) == 0;
  // selected hits: non-overlapping, each inside one document
  for (size_t p = 0; p < n;) {
    if (rnd(3)) {
      p += 1 + rnd(4);
      continue;
    }
    size_t e = p + 1 + rnd(rnd(4) ? 5 : 40);
    if (e > n) e = n;
    for (size_t q = p + 1; q < e; q++)
      if (c.doc_start[q]) {
        e = q;
        break;
      }
    add_hit(c, p, e);
    p = e;
  }
  return c;
}

int main() {
  static const size_t kLengths[] = {0, 1, 2, 3, 15, 16, 17, 30, 31, 32, 33, 34, 35, 47, 48, 49, 63, 64, 65, 66, 95, 96, 97, 130};
  for (uint32_t head = 0; head < 16; head++) {
    for (size_t n : kLengths)
      for (int trial = 0; trial < 40; trial++) check(random_case(n), head);
    for (size_t border : {(size_t)32, (size_t)64}) {
      Case c = blank(border + 8, 'x');  // a three-byte character: its lead is the word's last byte -- no token starts behind it
      c.text[border - 1] = 0xE6;
      c.text[border] = 0x88;
      c.text[border + 1] = 0x91;
      check(c, head);
      c = blank(border + 8, 'x');  // a hit that ends on the border, a gap behind it: "p - 1 is inside" crosses the word
      c.text[border] = 0x80;
      add_hit(c, border - 3, border);
      check(c, head);
      add_hit(c, border, border + 2);  // ... and another hit at once
      check(c, head);
      c = blank(border + 40, 0x80);  // a stray run of continuation bytes over the border: one token
      c.text[3] = 'a';
      check(c, head);
      c = blank(border + 8, 'x');  // a document that starts on the border with a continuation byte
      c.text[border] = 0x80;
      c.doc_start[border] = 1;
      check(c, head);
    }
  }
  std::printf("%lld words checked, %lld failure(s)\n", checked, fails);
  return fails ? 1 : 0;
}
