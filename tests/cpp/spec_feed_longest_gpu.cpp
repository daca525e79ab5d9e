// A longest feed through include/aha/ac.hpp (aha::Feed::match_longest(ac, n, intersectable), finish_batch / finish): at every
// two-piece cut the calls and the finish give AC::match_longest of the whole, a hit is reported at the byte that yields it, and
// count and select calls are refused.  Run on the GPU by tests/test_gpu_feed_longest.py.
#include <cstdio>
#include <string>
#include <vector>

#include "aha/ac.hpp"

static int fails = 0;
static void check(const std::string &name, bool ok) {
  if (!ok) {
    std::printf("FAIL %s\n", name.c_str());
    fails++;
  }
}
static bool same(const std::vector<aha::Hit> &a, const std::vector<aha::Hit> &b) {
  if (a.size() != b.size()) return false;
  for (size_t i = 0; i < a.size(); i++)
    if (a[i].start != b[i].start || a[i].end != b[i].end || a[i].value != b[i].value) return false;
  return true;
}

int main() {
  auto m = aha::AC::compile({"he", "hers", "she", "sherlock", "lock", "ock", "s"});
  const std::string text = std::string("sherlocks hershey ushers sherl") + '\0' + "ock he" + '\0' + "rs";
  for (int isect = 0; isect < 2; isect++) {
    std::vector<aha::Hit> want;
    m.match_longest(text, isect != 0, [&](const aha::Hit &h) { want.push_back(h); });
    check("the whole has hits", want.size() > 4);
    for (size_t cut = 0; cut <= text.size(); cut++) {
      auto f = aha::Feed::match_longest(m, 3, isect != 0);
      auto got = f.match(1, text.substr(0, cut));
      const auto more = f.match(1, text.substr(cut));
      got.insert(got.end(), more.begin(), more.end());
      const auto last = f.finish(1);
      got.insert(got.end(), last.begin(), last.end());
      check("mode " + std::to_string(isect + 1) + " cut at " + std::to_string(cut),
            same(got, want) && last.size() <= 1 && f.position(1).first == 0);
    }
  }
  {
    auto f = aha::Feed::match_longest(m, 2);
    std::vector<uint64_t> bases, pho;
    auto h = f.match_batch("a she", {0, 5}, {0}, &pho, &bases);
    check("a pending end waits", h.empty() && pho[1] == 0);
    h = f.match_batch("rl", {0, 2}, {0}, &pho, &bases);
    check("... through direct gotos", h.empty() && bases[0] == 5);
    h = f.match_batch("x", {0, 1}, {0}, &pho, &bases);
    check("... and is yielded at the first byte without a goto, wholly in earlier pieces",
          h.size() == 1 && h[0].start == -5 && h[0].end == -2 && h[0].value == 2 && bases[0] == 7);
    f.match(0, " hers");
    std::vector<uint64_t> sho;
    h = f.finish_batch({0}, &sho, &bases);
    check("finish: the pending hit, relative to the sequence's end",
          h.size() == 1 && h[0].start == -4 && h[0].end == 0 && h[0].value == 1 && bases[0] == 13 && sho[1] == 1 && f.position(0).first == 0);
    f.match(1, "she");
    bool refused = false;
    try {
      f.count(1, "he");
    } catch (const aha::Error &e) {
      refused = e.code == AHA_E_INVALID;
    }
    check("count is refused, the feed unchanged", refused && f.position(1).first == 3);
    refused = false;
    try {
      f.select(1, "he");
    } catch (const aha::Error &e) {
      refused = e.code == AHA_E_INVALID;
    }
    check("select is refused, the feed unchanged", refused && f.position(1).first == 3);
    f.reset(1);
    check("reset drops the pending end", f.finish(1).empty());
  }
  if (fails) {
    std::printf("spec_feed_longest_gpu: %d FAILED\n", fails);
    return 1;
  }
  std::printf("spec_feed_longest_gpu: ok\n");
  return 0;
}
