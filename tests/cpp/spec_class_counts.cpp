// Class counts through include/aha/ac.hpp (AC::classes, AC::class_counts_batch, AC::class_counts): the worked example of the
// header's comment: built by tests/test_class_counts_host.py (compiles) and run on the GPU by tests/test_gpu_class_counts_cpp.py.
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
  auto m = aha::AC::compile({"he", "she", "hers"});
  using Row = std::vector<uint32_t>;
  auto t = m.classes({{0}, {0, 1}, {}}, 2);  // he: class 0; she: classes 0 and 1; hers: none
  uint64_t n_hits = 0;
  const Row out = m.class_counts_batch("ushershe", {0, 6, 8}, t, &n_hits);
  check("class counts: the table", out == Row{2, 1, 1, 0});
  check("class counts: all hits", n_hits == 4);
  check("class counts: deterministic", m.class_counts_batch("ushershe", {0, 6, 8}, t) == out);
  check("class counts: one sequence", m.class_counts("ushers", t) == Row{2, 1});
  check("class counts: empty documents", m.class_counts_batch("he", {0, 0, 2, 2}, t) == Row{0, 0, 1, 0, 0, 0});
  check("class counts: no document", m.class_counts_batch("", {0}, t).empty());
  auto none = m.classes({{}, {}, {}}, 3);
  check("class counts: no key has a class", m.class_counts("ushers", none) == Row{0, 0, 0});
  {  // a table outlives its handle and is refused by another
    auto other = aha::AC::compile({"he", "she", "hers"});
    bool refused = false;
    try {
      other.class_counts("ushers", t);
    } catch (const aha::Error &e) {
      refused = e.code == AHA_E_INVALID;
    }
    check("class counts: a table of another handle", refused);
    bool bad = false;
    try {
      m.classes({{0}, {1, 1}, {}}, 2);
    } catch (const aha::Error &e) {
      bad = e.code == AHA_E_INVALID;
    }
    check("classes: a class twice for a key", bad);
  }
  if (fails) std::printf("%d FAILED\n", fails);
  return fails ? 1 : 0;
}
