// doc_tiles of aha_amd/csrc/doc_ranges.hpp -- the ranges of a token call -- on made-up hit and text offsets: the ranges tile
// every document, each holds text unless the batch has none, and a range of more than one document with text is within both
// bounds (hits: 12 bytes each; text: 8 bytes of scratch each).  Stand-alone, no GPU; built with -fsanitize=address,undefined
// by tests/test_tokens_host.py.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../aha_amd/csrc/doc_ranges.hpp"

static long long checked = 0, fails = 0;
static uint64_t rng_state = 12345;
static uint32_t rnd(uint32_t n) {
  rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull;
  return (uint32_t)(rng_state >> 33) % n;
}

static void check(const std::vector<uint64_t> &hit, const std::vector<uint64_t> &off, uint64_t bound) {
  const uint64_t D = off.size() - 1;
  std::vector<uint64_t> b;
  bool ok = aha::doc_tiles(hit.data(), off.data(), D, bound, b) && !b.empty() && b[0] == 0 && b.back() == D;
  for (size_t r = 0; ok && r + 1 < b.size(); r++) {
    const uint64_t d0 = b[r], d1 = b[r + 1];
    ok = d1 > d0;
    uint64_t with_text = 0;
    for (uint64_t d = d0; d < d1; d++) with_text += off[d + 1] > off[d];
    if (off[D] > 0) ok = ok && with_text > 0;  // every range holds text
    if (with_text > 1) ok = ok && (hit[d1] - hit[d0]) * 12 <= bound && (off[d1] - off[d0]) * 8 <= bound;
    // greedy: the next document with text would not have fitted
    if (ok && d1 < D) {
      uint64_t n = d1;
      while (n < D && off[n + 1] == off[n]) n++;
      ok = n < D && ((hit[n + 1] - hit[d0]) * 12 > bound || (off[n + 1] - off[d0]) * 8 > bound);
    }
  }
  if (off[D] > 0 && (hit[D] - hit[0]) * 12 <= bound && off[D] * 8 <= bound) ok = ok && b.size() == 2;  // one range
  checked++;
  if (!ok && fails++ < 10) std::printf("FAIL D %llu bound %llu\n", (unsigned long long)D, (unsigned long long)bound);
}

int main() {
  for (int trial = 0; trial < 20000; trial++) {
    const uint64_t D = rnd(12);
    std::vector<uint64_t> hit(1, 0), off(1, 0);
    for (uint64_t d = 0; d < D; d++) {
      const uint64_t len = rnd(3) ? rnd(40) : 0;
      off.push_back(off.back() + len);
      hit.push_back(hit.back() + (len && rnd(2) ? rnd(2 * (uint32_t)len + 1) : 0));
    }
    check(hit, off, 12 + rnd(600));
  }
  std::vector<uint64_t> b;
  const uint64_t z[1] = {0};
  if (!aha::doc_tiles(z, z, 0, 100, b) || b.size() != 1) fails++;  // D = 0: no range
  std::printf("%lld tilings checked, %lld failure(s)\n", checked, fails);
  return fails ? 1 : 0;
}
