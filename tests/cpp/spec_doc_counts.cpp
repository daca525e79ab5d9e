// Document counts through include/aha/ac.hpp (AC::doc_counts_batch) against the match call of the same batch: built by
// tests/test_doc_counts_host.py (compiles) and run on the GPU by tests/test_gpu_doc_counts_cpp.py.
#include <cstdio>
#include <map>
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
  // what the match call says: per document, hits per key in ascending key order
  std::vector<uint64_t> mdho;
  const auto hits = m.match_batch(corpus, offs, &mdho);
  std::vector<aha_key_count> want;
  std::vector<uint64_t> want_off = {0};
  for (size_t d = 0; d + 1 < offs.size(); d++) {
    std::map<int32_t, uint32_t> row;
    for (uint64_t i = mdho[d]; i < mdho[d + 1]; i++) row[hits[i].value]++;
    for (const auto &kv : row) want.push_back(aha_key_count{kv.first, kv.second});
    want_off.push_back(want.size());
  }

  std::vector<uint64_t> dpo;
  uint64_t n_hits = 0;
  const auto pairs = m.doc_counts_batch(corpus, offs, &dpo, &n_hits);
  bool same = pairs.size() == want.size();
  for (size_t i = 0; same && i < want.size(); i++) same = pairs[i].key == want[i].key && pairs[i].count == want[i].count;
  check("doc_counts_batch: pairs", same);
  check("doc_counts_batch: offsets", dpo == want_off);
  check("doc_counts_batch: hits", n_hits == hits.size());
  const auto again = m.doc_counts_batch(corpus, offs);
  bool twice = again.size() == pairs.size();
  for (size_t i = 0; twice && i < pairs.size(); i++) twice = again[i].key == pairs[i].key && again[i].count == pairs[i].count;
  check("doc_counts_batch: deterministic", twice);
  std::printf("%d failures\n", fails);
  return fails ? 1 : 0;
}
