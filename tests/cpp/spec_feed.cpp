// Feeds through include/aha/ac.hpp (aha::Feed): a sequence fed in pieces gives the hits of the whole sequence, the bases and
// positions follow, reset starts over.  Built by tests/test_feed_host.py (compiles) and run on the GPU by
// tests/test_gpu_feed_cpp.py.
#include <cstdio>
#include <string>
#include <vector>

#include "aha/ac.hpp"

static int fails = 0;
static void check(const char *name, bool ok) {
  std::printf("%s %s\n", ok ? "ok  " : "FAIL", name);
  if (!ok) fails++;
}

static bool same(const std::vector<aha::Hit> &a, const std::vector<aha::Hit> &b) {
  if (a.size() != b.size()) return false;
  for (size_t i = 0; i < a.size(); i++)
    if (a[i].start != b[i].start || a[i].end != b[i].end || a[i].value != b[i].value) return false;
  return true;
}

int main() {
  auto m = aha::AC::compile({"he", "she", "his", "hers", "e", "我", "我是", "是中", "ushers"});
  const std::string text = std::string("ushers she said his hers ") + "我是中国人" + std::string(1, '\0') + "hehehe ushers";
  std::vector<aha::Hit> want;
  m.match(text, [&](const aha::Hit &h) { want.push_back(h); });

  for (size_t step : {1, 2, 3, 5, 7, 64}) {
    aha::Feed f(m, 2);
    std::vector<aha::Hit> got;
    for (size_t a = 0; a < text.size(); a += step)
      for (const auto &h : f.match(1, std::string_view(text).substr(a, step))) got.push_back(h);
    check(("pieces of " + std::to_string(step) + " bytes").c_str(), same(got, want));
    check("position", f.position(1).first == text.size() && f.position(0).first == 0);
  }

  // two sequences in one call, then the second half of each; bases and per-piece offsets
  aha::Feed f(m, 2);
  const size_t h = 13;
  std::vector<uint64_t> pho, bases;
  const std::string first = text.substr(0, h) + text.substr(0, 2 * h);
  auto a = f.match_batch(first, {0, h, 3 * h}, {1, 0}, &pho, &bases);
  check("first call bases", bases == std::vector<uint64_t>({0, 0}));
  const std::string second = text.substr(2 * h) + text.substr(h);
  auto b = f.match_batch(second, {0, text.size() - 2 * h, second.size()}, {0, 1}, nullptr, &bases);
  check("second call bases", bases == std::vector<uint64_t>({2 * h, h}));
  check("first call offsets", pho.size() == 3 && pho[2] == a.size());
  f.reset(1);
  check("reset", f.position(1).first == 0 && f.position(0).first == text.size());
  check("after reset", same(f.match(1, text), want));
  std::printf("%d failures\n", fails);
  return fails ? 1 : 0;
}
