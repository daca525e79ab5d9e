// Cover calls through include/aha/ac.hpp (AC::cover_batch, AC::redact_batch, AC::redact) against the match call of the same
// batch: built by tests/test_cover_host.py (compiles) and run on the GPU by tests/test_gpu_cover_cpp.py.
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
  auto m = aha::AC::compile({"he", "she", "his", "hers", "e", "我", "我是", "是中"});
  const std::string corpus = std::string("ushers she said his hers") + "我是中国人" + "" + "hehehe";
  const std::vector<uint64_t> offs = {0, 24, 24 + 15, 24 + 15, 24 + 15 + 6};
  // what the match call says: the union of the hits' spans
  std::vector<uint64_t> mdho;
  const auto hits = m.match_batch(corpus, offs, &mdho);
  std::vector<bool> want(corpus.size(), false);
  std::vector<uint64_t> want_cov(offs.size() - 1, 0);
  for (size_t d = 0; d + 1 < offs.size(); d++)
    for (uint64_t i = mdho[d]; i < mdho[d + 1]; i++)
      for (int32_t j = hits[i].start; j < hits[i].end; j++) want[offs[d] + j] = true;
  std::string want_red = corpus;
  for (size_t d = 0; d + 1 < offs.size(); d++)
    for (uint64_t j = offs[d]; j < offs[d + 1]; j++)
      if (want[j]) {
        want_cov[d]++;
        want_red[j] = '*';
      }

  std::vector<uint64_t> cov;
  uint64_t n_hits = 0;
  const auto mask = m.cover_batch(corpus, offs, &cov, &n_hits);
  bool same = mask.size() == (corpus.size() + 31) / 32;
  for (size_t j = 0; same && j < mask.size() * 32; j++)
    same = (((mask[j >> 5] >> (j & 31)) & 1u) != 0) == (j < corpus.size() && want[j]);
  check("cover_batch: mask", same);
  check("cover_batch: doc_covered", cov == want_cov);
  check("cover_batch: hits", n_hits == hits.size());
  std::vector<uint64_t> cov2;
  check("redact_batch: bytes", m.redact_batch(corpus, offs, '*', &cov2) == want_red);
  check("redact_batch: doc_covered", cov2 == want_cov);
  check("redact: one sequence", m.redact("ushers", '#') == "u#####");
  check("cover_batch: deterministic", m.cover_batch(corpus, offs) == mask);
  std::printf("%d failures\n", fails);
  return fails ? 1 : 0;
}
