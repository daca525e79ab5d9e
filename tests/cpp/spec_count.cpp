// Count calls through include/aha/ac.hpp (AC::count_batch, AC::count_resident) against the match call of the same batch:
// built by tests/test_count_host.py (compiles) and run on the GPU by tests/test_gpu_count_cpp.py.
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
  // what the match call says: hits per key and per document
  std::vector<uint64_t> mdho;
  const auto hits = m.match_batch(corpus, offs, &mdho);
  std::vector<uint64_t> want(m.n_keys(), 0);
  for (const auto &h : hits) want[(size_t)h.value]++;

  std::vector<uint64_t> kc, dho;
  const uint64_t n = m.count_batch(corpus, offs, &kc, &dho);
  check("count_batch: total", n == hits.size());
  check("count_batch: per key", kc == want);
  check("count_batch: per document", dho == mdho);
  const uint64_t n2 = m.count_batch(corpus, offs, nullptr, &dho);
  check("count_batch without key counts", n2 == hits.size() && dho == mdho);
  m.count_batch(corpus, offs, &kc, nullptr, true);  // running totals: twice the batch
  bool twice = true;
  for (size_t k = 0; k < want.size(); k++) twice &= kc[k] == 2 * want[k];
  check("count_batch accumulate", twice);

  aha::Corpus c(corpus, offs);
  void *d_kc = nullptr;
  if (aha_buffer_alloc(0, want.size() * 8, &d_kc) != AHA_OK) return 2;
  std::vector<uint64_t> zero(want.size(), 0), got(want.size());
  aha_buffer_upload(0, d_kc, zero.data(), zero.size() * 8);
  const uint64_t n3 = m.count_resident(c, static_cast<uint64_t *>(d_kc), true, &dho);
  m.count_resident(c, static_cast<uint64_t *>(d_kc), true);
  aha_buffer_download(0, got.data(), d_kc, got.size() * 8);
  aha_buffer_free(0, d_kc);
  bool res = n3 == hits.size() && dho == mdho;
  for (size_t k = 0; k < want.size(); k++) res &= got[k] == 2 * want[k];
  check("count_resident accumulate", res);
  std::printf("%d failures\n", fails);
  return fails ? 1 : 0;
}
