// A feed with a separator filter through include/aha/ac.hpp (aha::Feed(ac, n, BitArray), finish_batch / finish): whole-word
// hits at every cut against AC::match(seq, sep) of the whole, the hit reported one byte late, finish, count, and the refusal of
// cover and select.  Run on the GPU by tests/test_gpu_feed_sep_cpp.py.
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
  aha::BitArray sep(256);
  for (char c : std::string(" .,:;!?")) sep.set((unsigned char)c);
  auto m = aha::AC::compile({"error", "err", "or", "terrors", "s"});
  const std::string text = "error: terrors or err. s errors,or";
  std::vector<aha::Hit> want;
  m.match(text, sep, [&](const aha::Hit &h) { want.push_back(h); });
  check("the whole: some hits are filtered", !want.empty() && want.size() < 12);
  for (size_t cut = 0; cut <= text.size(); cut++) {
    aha::Feed f(m, 3, sep);
    auto got = f.match(1, text.substr(0, cut));
    const auto more = f.match(1, text.substr(cut));
    got.insert(got.end(), more.begin(), more.end());
    const auto last = f.finish(1);
    got.insert(got.end(), last.begin(), last.end());
    check("cut at " + std::to_string(cut), same(got, want) && f.position(1).first == 0);
  }
  {
    aha::Feed f(m, 2, sep);
    std::vector<uint64_t> bases, pho;
    auto h = f.match_batch("an error", {0, 8}, {0}, &pho, &bases);
    check("a hit that ends with the piece waits", h.empty() && pho[1] == 0);
    h = f.match_batch(": x", {0, 3}, {0}, &pho, &bases);
    check("... and is reported one byte late", h.size() == 1 && h[0].start == -5 && h[0].end == 0 && h[0].value == 0 && bases[0] == 8);
    f.match(0, " err");
    std::vector<uint64_t> sho;
    h = f.finish_batch({0}, &sho, &bases);
    check("finish: relative to the sequence's end", h.size() == 1 && h[0].start == -3 && h[0].end == 0 && h[0].value == 1 &&
                                                       bases[0] == 15 && sho[1] == 1 && f.position(0).first == 0);
    const auto kc = f.count(1, "err or s ");
    check("count is the match call's histogram", kc == std::vector<uint64_t>({0, 1, 1, 0, 1}));
    bool refused = false;
    try {
      f.select(1, "err");
    } catch (const aha::Error &e) {
      refused = e.code == AHA_E_INVALID;
    }
    check("select is refused, the feed unchanged", refused && f.position(1).first == 9);
    refused = false;
    try {
      f.finish_batch({1, 1});
    } catch (const aha::Error &e) {
      refused = e.code == AHA_E_INVALID;
    }
    check("a sequence named twice", refused && f.position(1).first == 9);
    aha::Feed plain(m, 1);
    refused = false;
    try {
      plain.finish(0);
    } catch (const aha::Error &e) {
      refused = e.code == AHA_E_INVALID;
    }
    check("finish on a plain feed is refused", refused);
  }
  std::printf("%d failures\n", fails);
  return fails ? 1 : 0;
}
