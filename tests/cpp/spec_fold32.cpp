// fold32 / fold128 / fold8 of aha_amd/csrc/fold.hpp (the word forms the kernels use) against the bytewise rule: every byte
// value in every lane, the other three lanes filled with each of 14 bytes around the rule's edges (0x40/0x41, 0x5A/0x5B, their
// + 0x20 and + 0x80 twins, 0x00, 0x7F, 0xFF) -- a sample, which is enough for a form whose sums never leave their byte.  Built
// and run by tests/test_fold_host.py.
#include <cstdint>
#include <cstdio>

#include "../../aha_amd/csrc/fold.hpp"

static uint8_t rule(uint8_t b) { return (b >= 0x41 && b <= 0x5A) ? (uint8_t)(b + 32) : b; }

int main() {
  int fails = 0;
  for (int b = 0; b < 256; b++)
    if (aha::fold8((uint8_t)b) != rule((uint8_t)b)) fails++;
  const uint8_t others[] = {0x00, 0x40, 0x41, 0x5A, 0x5B, 0x60, 0x61, 0x7A, 0x7B, 0x7F, 0x80, 0xC1, 0xDA, 0xFF};
  for (int lane = 0; lane < 4; lane++)
    for (int b = 0; b < 256; b++)
      for (uint8_t o : others) {
        uint32_t w = 0, want = 0;
        for (int j = 0; j < 4; j++) {
          const uint8_t x = j == lane ? (uint8_t)b : o;
          w |= (uint32_t)x << (8 * j);
          want |= (uint32_t)rule(x) << (8 * j);
        }
        if (aha::fold32(w) != want) {
          if (fails < 8) std::printf("FAIL fold32(%08x) = %08x, want %08x\n", w, aha::fold32(w), want);
          fails++;
        }
        uint32_t q[4] = {w, ~w, w ^ 0x20202020u, w};
        uint32_t wq[4];
        for (int k = 0; k < 4; k++) {
          wq[k] = 0;
          for (int j = 0; j < 4; j++) wq[k] |= (uint32_t)rule((uint8_t)(q[k] >> (8 * j))) << (8 * j);
        }
        aha::fold128(q[0], q[1], q[2], q[3]);
        for (int k = 0; k < 4; k++)
          if (q[k] != wq[k]) fails++;
      }
  std::printf("%d failures\n", fails);
  return fails ? 1 : 0;
}
