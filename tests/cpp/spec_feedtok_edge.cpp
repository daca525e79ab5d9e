// feedtok_edge.hpp against the contract of include/aha_hip.h ("Feed tokens"), stated on token lists: for every
// t0 <= c0 <= c1 <= n1 <= 12, every set of token starts in [c0, c1) (all of them where the range has at most 7 positions, else
// 96 random ones; c0 is a start where t0 == c0 < c1, as a document's first position is), the class of the byte at c1
// (continuation or not), the last hit ending at c1 or not, FINAL and GAP_RUNS, and three bounds of the open length: build
// Tok1 as a list of (start, end), decide whether c1 is a certain boundary, drop the last token where it is not, and compare
// what is reported, t1 and the open-length verdict with the header's answer.  Built with -fsanitize=address,undefined by
// tests/test_feed_tokens_host.py.  Stand-alone, no GPU.
#include <cstdint>
#include <cstdio>
#include <utility>
#include <vector>

#include "../../aha_amd/csrc/feedtok_edge.hpp"

static long long checked = 0, fails = 0;
static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd() {
  rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull;
  return (uint32_t)(rng_state >> 33);
}

static void check(uint64_t t0, uint64_t c0, uint64_t c1, uint64_t n1, uint32_t mask, bool hit_end, bool cont, bool final, bool gap_runs,
                  uint64_t bound) {
  // Tok1, token by token
  std::vector<uint64_t> starts;
  if (t0 < c0) starts.push_back(t0);
  uint64_t n_starts = 0, last = 0;
  for (uint64_t p = c0; p < c1; p++)
    if ((mask >> (p - c0)) & 1u) {
      starts.push_back(p);
      n_starts++;
      last = p;
    }
  std::vector<std::pair<uint64_t, uint64_t>> tok;
  for (size_t i = 0; i < starts.size(); i++) tok.push_back({starts[i], i + 1 < starts.size() ? starts[i + 1] : c1});
  const bool certain = final || gap_runs || hit_end || (c1 < n1 && !cont);
  uint64_t t1 = t0;
  bool open = false;
  if (!tok.empty()) {
    if (certain) {
      t1 = c1;
    } else {
      t1 = tok.back().first;
      tok.pop_back();
      open = true;
    }
  }
  const bool too_long = !final && n1 - t1 > bound;
  // the reported tokens tile [t0, t1)
  uint64_t at = t0;
  bool tiles = true;
  for (auto &t : tok) {
    tiles = tiles && t.first == at && t.second > t.first;
    at = t.second;
  }
  tiles = tiles && at == t1;

  const aha::FeedTokEdge e = aha::feedtok_edge(t0, c0, c1, n1, n_starts, last, hit_end, cont, final, gap_runs, bound);
  checked++;
  if (!tiles || e.t1 != t1 || e.count != tok.size() || (e.open != 0) != open || (e.carried != 0) != (t0 < c0) ||
      (e.too_long != 0) != too_long) {
    if (fails++ < 10)
      printf("FAIL t0=%llu c0=%llu c1=%llu n1=%llu mask=%x hit_end=%d cont=%d final=%d gap_runs=%d bound=%llu: t1 %llu / %llu, count %llu / "
             "%zu, open %u / %d, too_long %u / %d, tiles %d\n",
             (unsigned long long)t0, (unsigned long long)c0, (unsigned long long)c1, (unsigned long long)n1, mask, hit_end, cont, final,
             gap_runs, (unsigned long long)bound, (unsigned long long)e.t1, (unsigned long long)t1, (unsigned long long)e.count, tok.size(),
             e.open, open, e.too_long, too_long, tiles);
  }
}

int main() {
  const uint64_t bounds[3] = {1, 4, 0x3FFFFFFFull};
  for (uint64_t n1 = 0; n1 <= 12; n1++)
    for (uint64_t c1 = 0; c1 <= n1; c1++)
      for (uint64_t c0 = 0; c0 <= c1; c0++)
        for (uint64_t t0 = 0; t0 <= c0; t0++) {
          const uint32_t len = (uint32_t)(c1 - c0);
          const uint32_t n_masks = len <= 7 ? 1u << len : 96u;
          for (uint32_t k = 0; k < n_masks; k++) {
            uint32_t mask = len <= 7 ? k : rnd() & ((1u << len) - 1u);
            if (t0 == c0 && len) mask |= 1u;  // c0 stands for a document's start
            for (int flags = 0; flags < 16; flags++) {
              const bool hit_end = flags & 1, cont = flags & 2, final = flags & 4, gap_runs = flags & 8;
              if (hit_end && !mask) continue;  // (a hit the call settles starts in [c0, c1))
              for (uint64_t bound : bounds) check(t0, c0, c1, n1, mask, hit_end, cont, final, gap_runs, bound);
            }
          }
        }
  printf("spec_feedtok_edge: %lld cases, %lld failure(s)\n", checked, fails);
  return fails ? 1 : 0;
}
