// Feed counts through include/aha/ac.hpp (aha::Feed::count_batch): a sequence fed in pieces gives, summed, the hits per key of
// the whole sequence; running totals, offsets and bases follow; a count and a match may share a feed.  Built by
// tests/test_feed_count_host.py (compiles) and run on the GPU by tests/test_gpu_feed_count_cpp.py.
#include <cstdio>
#include <string>
#include <vector>

#include "aha/ac.hpp"

static int fails = 0;
static void check(const char *name, bool ok) {
  std::printf("%s %s\n", ok ? "ok  " : "FAIL", name);
  if (!ok) fails++;
}

int main() {
  auto m = aha::AC::compile({"he", "she", "his", "hers", "e", "我", "我是", "是中", "ushers"});
  const uint32_t K = m.n_keys();
  const std::string text = std::string("ushers she said his hers ") + "我是中国人" + std::string(1, '\0') + "hehehe ushers";
  std::vector<uint64_t> want;
  const uint64_t n_want = m.count_batch(text, {0, text.size()}, &want);

  for (size_t step : {1, 2, 3, 5, 7, 64}) {
    aha::Feed f(m, 2);
    std::vector<uint64_t> total(K, 0);
    uint64_t n = 0;
    for (size_t a = 0; a < text.size(); a += step) {
      const std::string piece = text.substr(a, step);
      n += f.count_batch(piece, {0, piece.size()}, {1}, &total, nullptr, nullptr, true);
    }
    check(("running totals over pieces of " + std::to_string(step) + " bytes").c_str(), total == want && n == n_want);
    check("position", f.position(1).first == text.size() && f.position(0).first == 0);
  }

  // two sequences in one call, then the rest of each; offsets, bases, and a match in between
  aha::Feed f(m, 2);
  const size_t h = 13;
  std::vector<uint64_t> kc, pho, bases;
  const std::string first = text.substr(0, h) + text.substr(0, 2 * h);
  const uint64_t n1 = f.count_batch(first, {0, h, 3 * h}, {1, 0}, &kc, &pho, &bases);
  check("first call bases", bases == std::vector<uint64_t>({0, 0}));
  check("first call offsets", pho.size() == 3 && pho[2] == n1);
  const auto mid = f.match(0, text.substr(2 * h, h));
  std::vector<uint64_t> kc2;
  const std::string second = text.substr(3 * h) + text.substr(h);
  f.count_batch(second, {0, text.size() - 3 * h, second.size()}, {0, 1}, &kc2, nullptr, &bases);
  check("second call bases", bases == std::vector<uint64_t>({3 * h, h}));
  std::vector<uint64_t> sum(K, 0);
  for (uint32_t k = 0; k < K; k++) sum[k] = kc[k] + kc2[k];
  for (const auto &x : mid) sum[x.value]++;
  for (uint32_t k = 0; k < K; k++) want[k] *= 2;
  check("both sequences whole", sum == want);
  check("count(seq, piece)", f.count(1, "") == std::vector<uint64_t>(K, 0) && f.position(1).first == text.size());
  std::printf("%d failures\n", fails);
  return fails ? 1 : 0;
}
