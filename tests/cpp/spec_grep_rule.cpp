// Rule grep through include/aha/ac.hpp (AC::grep_rule_batch): the worked example of include/aha_hip.h -- keys he, she, hers with
// classes {0}, {0, 1}, {} over the documents "ushers" and "he" -- plain and inverted, with the rows: built by
// tests/test_grep_rule_host.py (compiles) and run on the GPU by tests/test_gpu_grep_rule_cpp.py.
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
  using aha::AC;
  auto m = AC::compile({"he", "she", "hers"});
  auto t = m.classes({{0}, {0, 1}, {}}, 2);
  const std::string text = "ushershe";
  using Offs = std::vector<uint64_t>;
  const Offs offs{0, 6, 8};
  {  // {c0 >= 2} keeps document 0
    Offs kept, doo;
    std::vector<uint32_t> rows;
    uint64_t n_hits = 0;
    const std::string out = m.grep_rule_batch(text, offs, t, {AC::term(0, AHA_RULE_GE, 2)}, false, &kept, &doo, &rows, &n_hits);
    check("count rule: kept_docs", kept == Offs{0});
    check("count rule: doc_out_offsets", doo == Offs{0, 6});
    check("count rule: bytes", out == "ushers");
    check("count rule: rows", rows == std::vector<uint32_t>{2, 1, 1, 0});
    check("count rule: rows are class counts", rows == m.class_counts_batch(text, offs, t));
    check("count rule: all hits", n_hits == 4);
    check("count rule: deterministic", m.grep_rule_batch(text, offs, t, {AC::term(0, AHA_RULE_GE, 2)}) == out);
    const std::string inv = m.grep_rule_batch(text, offs, t, {AC::term(0, AHA_RULE_GE, 2)}, true, &kept, &doo);
    check("count rule inverted", kept == Offs{1} && doo == Offs{0, 2} && inv == "he");
  }
  {  // {c0 >= 1 AND c1 < 1} keeps document 1
    Offs kept;
    const std::string out = m.grep_rule_batch(text, offs, t, {AC::term(0, AHA_RULE_GE, 1), AC::term(1, AHA_RULE_LT, 1)}, false, &kept);
    check("two terms: kept_docs", kept == Offs{1});
    check("two terms: bytes", out == "he");
  }
  {  // {c0 >= 1 per 3 bytes} keeps both; as two groups {c0 >= 2} OR {c1 < 1} too
    Offs kept;
    check("density rule", m.grep_rule_batch(text, offs, t, {AC::term(0, AHA_RULE_GE, 1, 3)}, false, &kept) == text && kept == Offs{0, 1});
    check("two groups", m.grep_rule_batch(text, offs, t, {AC::term(1, AHA_RULE_LT, 1, 0, 9), AC::term(0, AHA_RULE_GE, 2, 0, 4)}) == text);
    check("nothing kept", m.grep_rule_batch(text, offs, t, {AC::term(1, AHA_RULE_GE, 2)}).empty());
  }
  {  // refused before any device work
    bool threw = false;
    try {
      m.grep_rule_batch(text, offs, t, {AC::term(2, AHA_RULE_GE, 1)});
    } catch (const aha::Error &) {
      threw = true;
    }
    check("a class the table does not have", threw);
    check("plain grep as it was", m.grep_batch(text, offs) == text);
  }
  if (fails) std::printf("%d FAILED\n", fails);
  return fails ? 1 : 0;
}
