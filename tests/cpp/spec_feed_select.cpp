// Feed select through include/aha/ac.hpp (aha::Feed::select_batch / select): the header's own example at every cut, the
// "longer key completes later" case, FINAL, and the stream law against AC::select of the whole.  Run on the GPU by
// tests/test_gpu_feed_select_cpp.py.
#include <cstdio>
#include <string>
#include <vector>

#include "aha/ac.hpp"

static int fails = 0;
static void check(const std::string &name, bool ok) {
  std::printf("%s %s\n", ok ? "ok  " : "FAIL", name.c_str());
  if (!ok) fails++;
}
static bool same(const std::vector<aha::Hit> &a, const std::vector<aha::Hit> &b) {
  if (a.size() != b.size()) return false;
  for (size_t i = 0; i < a.size(); i++)
    if (a[i].start != b[i].start || a[i].end != b[i].end || a[i].value != b[i].value) return false;
  return true;
}

int main() {
  {  // keys ab, bcd, cd, d over "abcd": (0,2,ab), (2,4,cd) at every cut
    auto m = aha::AC::compile({"ab", "bcd", "cd", "d"});
    const std::string text = "abcd";
    const auto want = m.select(text);
    check("the whole: two hits", want.size() == 2 && want[0].end == 2 && want[1].start == 2 && want[1].value == 2);
    for (size_t cut = 0; cut <= text.size(); cut++) {
      aha::Feed f(m, 3);
      auto got = f.select(2, text.substr(0, cut));
      const auto more = f.select(2, text.substr(cut), true);
      got.insert(got.end(), more.begin(), more.end());
      check("abcd cut at " + std::to_string(cut), same(got, want) && f.position(2).first == 0);
    }
  }
  {  // keys ab, abcde: "ab" reports nothing, "cde" then reports (0, 5) with a negative start
    auto m = aha::AC::compile({"ab", "abcde"});
    aha::Feed f(m, 2);
    aha::Feed::Select info;
    auto h = f.select_batch("ab", {0, 2}, {1}, false, &info);
    check("nothing early", h.empty() && info.piece_hold == std::vector<uint32_t>({2}) && info.bases == std::vector<uint64_t>({0}) &&
                               info.n_hits == 1);
    h = f.select_batch("cde", {0, 3}, {1}, false, &info);
    check("the longer key afterwards", h.size() == 1 && h[0].start == -2 && h[0].end == 3 && h[0].value == 1 &&
                                           info.piece_hold[0] == 0 && info.bases[0] == 2 && info.piece_sel_offsets[1] == 1);
    h = f.select(1, "ab");
    check("open again", h.empty() && f.position(1).first == 7);
    h = f.select_batch("", {0, 0}, {1}, true, &info);
    check("FINAL with an empty piece", h.size() == 1 && h[0].start == -2 && h[0].end == 0 && h[0].value == 0 && info.piece_hold[0] == 0 &&
                                           f.position(1).first == 0);
    bool refused = false;
    f.match(0, "ab");
    try {
      f.select(0, "cde");
    } catch (const aha::Error &) {
      refused = true;
    }
    check("select behind a match call is refused", refused && f.position(0).first == 2);
    f.reset(0);
    check("... until reset", f.select(0, "abcde", true).size() == 1);
  }
  {  // the stream law on a longer text, pieces of every small size
    auto m = aha::AC::compile({"he", "she", "his", "hers", "ushers", "said his", "s"});
    const std::string text = "ushers she said his hers hehehe ushers ssh";
    const auto want = m.select(text);
    for (size_t step : {1, 2, 3, 5, 7, 64}) {
      aha::Feed f(m, 1);
      std::vector<aha::Hit> got;
      for (size_t a = 0; a < text.size(); a += step) {
        const auto h = f.select(0, text.substr(a, step), a + step >= text.size());
        got.insert(got.end(), h.begin(), h.end());
      }
      check("stream law over pieces of " + std::to_string(step) + " bytes", same(got, want));
    }
  }
  std::printf("%d failures\n", fails);
  return fails ? 1 : 0;
}
