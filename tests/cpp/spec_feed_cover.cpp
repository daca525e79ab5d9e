// Feed cover through include/aha/ac.hpp (aha::Feed::cover_batch / redact_batch / redact): a sequence fed in pieces of any
// size gives, by the stream law, AC::redact_batch of the whole; the mask, piece_back, piece_covered, offsets and bases
// follow; cover, count and match calls share a feed.  Built by tests/test_feed_cover_host.py (compiles) and run on the GPU by
// tests/test_gpu_feed_cover_cpp.py.
#include <cstdio>
#include <string>
#include <vector>

#include "aha/ac.hpp"

static int fails = 0;
static void check(const std::string &name, bool ok) {
  std::printf("%s %s\n", ok ? "ok  " : "FAIL", name.c_str());
  if (!ok) fails++;
}

int main() {
  auto m = aha::AC::compile({"he", "she", "his", "hers", "我", "我是", "是中", "ushers", "said his"});
  const std::string text = std::string("ushers she said his hers ") + "我是中国人" + std::string(1, '\0') + "hehehe ushers";
  const std::string want = m.redact_batch(text, {0, text.size()}, '#');
  uint64_t n_want = 0;
  const auto want_mask = m.cover_batch(text, {0, text.size()}, nullptr, &n_want);
  uint64_t want_covered = 0;
  for (char c : want) want_covered += c == '#';

  for (size_t step : {1, 2, 3, 5, 7, 64}) {
    aha::Feed f(m, 2);
    std::string out;
    uint64_t hits = 0, covered = 0;
    bool bounds = true;
    for (size_t a = 0; a < text.size(); a += step) {
      const std::string piece = text.substr(a, step);
      aha::Feed::Cover c;
      const std::string red = f.redact_batch(piece, {0, piece.size()}, {1}, '#', &c);
      const uint32_t back = c.piece_back[0];
      bounds = bounds && back <= out.size() && back <= 7 && c.bases[0] == a && c.piece_covered[0] == c.n_covered;
      for (uint32_t k = 0; k < back; k++) {  // (the stream law: bytes handed out before that lie inside a hit ending here)
        covered += out[out.size() - 1 - k] != '#';
        out[out.size() - 1 - k] = '#';
      }
      out += red;
      hits += c.n_hits;
      covered += c.n_covered;
    }
    check("stream law over pieces of " + std::to_string(step) + " bytes", out == want && bounds);
    check("hits and covered bytes", hits == n_want && covered == want_covered);
    check("position", f.position(1).first == text.size() && f.position(0).first == 0);
  }

  // the mask of two sequences in one call, a count and a match in between
  aha::Feed f(m, 2);
  const size_t h = 13;
  aha::Feed::Cover c1, c2;
  const std::string first = text.substr(0, h) + text.substr(0, 2 * h);
  const auto m1 = f.cover_batch(first, {0, h, 3 * h}, {1, 0}, &c1);
  check("first call", m1.size() == (3 * h + 31) / 32 && c1.bases == std::vector<uint64_t>({0, 0}) && c1.piece_hit_offsets[2] == c1.n_hits &&
                          c1.piece_back == std::vector<uint32_t>({0, 0}));
  const auto mid = f.match(0, text.substr(2 * h, h));
  const auto kc = f.count(1, text.substr(h, h));
  const std::string second = text.substr(3 * h) + text.substr(2 * h);
  const auto m2 = f.cover_batch(second, {0, text.size() - 3 * h, second.size()}, {0, 1}, &c2);
  check("second call bases", c2.bases == std::vector<uint64_t>({3 * h, 2 * h}));
  auto bit = [](const std::vector<uint32_t> &w, size_t j) { return (w[j >> 5] >> (j & 31)) & 1u; };
  bool same = true;
  for (size_t j = 0; j < text.size() - 3 * h; j++) same = same && bit(m2, j) == bit(want_mask, 3 * h + j);
  for (size_t j = 0; j < text.size() - 2 * h; j++) same = same && bit(m2, text.size() - 3 * h + j) == bit(want_mask, 2 * h + j);
  check("second call mask", same);
  uint64_t kc_sum = 0;
  for (auto v : kc) kc_sum += v;
  check("all hits of sequence 1", c1.piece_hit_offsets[1] + kc_sum + (c2.piece_hit_offsets[2] - c2.piece_hit_offsets[1]) == n_want);
  uint32_t back = 9;
  check("redact(seq, piece)", f.redact(1, " she", '#', &back) == " ###" && back == 0);
  std::printf("%d failures\n", fails);
  return fails ? 1 : 0;
}
