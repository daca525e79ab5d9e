// The fold_ascii option of include/aha/ac.hpp (AC::compile, AC::from_bytes, Group::compile) against a plain handle compiled
// from the lower-cased keys over the lower-cased text: built by tests/test_fold_host.py (compiles) and run on the GPU by
// tests/test_gpu_fold_cpp.py.
#include <cstdio>
#include <string>
#include <vector>

#include "aha/ac.hpp"

static int fails = 0;
static void check(const char *name, bool ok) {
  std::printf("%s %s\n", ok ? "ok  " : "FAIL", name);
  if (!ok) fails++;
}
static std::string lower(std::string s) {
  for (char &c : s)
    if (c >= 'A' && c <= 'Z') c = (char)(c + 32);
  return s;
}
static bool same(const std::vector<aha::Hit> &a, const std::vector<aha::Hit> &b) {
  if (a.size() != b.size()) return false;
  for (size_t i = 0; i < a.size(); i++)
    if (a[i].start != b[i].start || a[i].end != b[i].end || a[i].value != b[i].value) return false;
  return true;
}

int main() {
  const std::vector<std::string> keys = {"He", "SHE", "his", "hERs", "e", "我", "我是Q", "是中"};
  std::vector<std::string> low;
  for (auto &k : keys) low.push_back(lower(k));
  auto f = aha::AC::compile(keys, -1, true);
  auto p = aha::AC::compile(low);
  const std::string corpus = std::string("uSHerS She saiD HIS hErs") + "我是q中国人" + "" + "HEhEHe";
  const std::vector<uint64_t> offs = {0, 24, 24 + 16, 24 + 16, 24 + 16 + 6};
  check("fold_ascii(): the flag", f.fold_ascii() && !p.fold_ascii());
  check("match: one sequence", same(f.match("uSHerS"), p.match("ushers")) && f.match("uSHerS").size() == 4);
  check("match: a plain handle is case-sensitive", p.match("uSHerS").size() < 4);
  std::vector<uint64_t> da, db;
  check("match_batch: hits", same(f.match_batch(corpus, offs, &da), p.match_batch(lower(corpus), offs, &db)));
  check("match_batch: offsets", da == db);
  check("match_batch: char offsets", same(f.match_batch(corpus, offs, nullptr, true), p.match_batch(lower(corpus), offs, nullptr, true)));
  // redaction keeps the caller's bytes outside the hits
  const std::string red = f.redact_batch(corpus, offs, '*'), redp = p.redact_batch(lower(corpus), offs, '*');
  bool ok = red.size() == corpus.size();
  for (size_t j = 0; ok && j < red.size(); j++) ok = redp[j] == '*' ? red[j] == '*' : red[j] == corpus[j];
  check("redact_batch: the original bytes outside the mask", ok);
  check("key(id): as spelled", f[1] == "SHE" && f[6] == "我是Q");
  check("id(key): folds its argument", f["she"] == 1 && f["She"] == 1 && f["我是q"] == 6);
  auto again = aha::AC::from_bytes(f.to_bytes(), -1, true);
  check("from_bytes(fold_ascii)", again.fold_ascii() && again[1] == "SHE" && same(again.match("uSHerS"), p.match("ushers")));
  auto plain_again = aha::AC::from_bytes(f.to_bytes());
  check("from_bytes without the option: case-sensitive", !plain_again.fold_ascii() && plain_again.match("ushers").size() == 1);
  auto g = aha::Group::compile(keys, {0, 0, 0}, true);
  check("Group::compile(fold_ascii)", same(g.match_batch(corpus, offs), p.match_batch(lower(corpus), offs)));
  std::printf("%d failures\n", fails);
  return fails ? 1 : 0;
}
