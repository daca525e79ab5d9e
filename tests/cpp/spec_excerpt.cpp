// Excerpts through include/aha/ac.hpp (AC::excerpts_batch): the examples of include/aha_hip.h under AHA_GREP_CONTEXT: built by
// tests/test_excerpt_host.py (compiles) and run on the GPU by tests/test_gpu_excerpt_cpp.py.
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
  using Offs = std::vector<uint64_t>;
  {  // example 1: key ab over "xxabxxxxabx" and "ab"
    auto m = AC::compile({"ab"});
    const std::string text = "xxabxxxxabxab";
    const Offs offs{0, 11, 13};
    const auto e = m.excerpts_batch(text, offs, 1, 2);
    check("1a: starts", e.starts == Offs{1, 7, 11});
    check("1a: offsets", e.out_offsets == Offs{0, 5, 9, 11});
    check("1a: bytes", e.out == "xabxxxabxab" && e[0] == "xabxx" && e[1] == "xabx" && e[2] == "ab");
    check("1a: all hits", e.n_hits == 3);
    check("1a: deterministic", m.excerpts_batch(text, offs, 1, 2).out == e.out);
    const auto f = m.excerpts_batch(text, offs, 1, 3);
    check("1b: merged inside one document", f.starts == Offs{1, 11} && f.out_offsets == Offs{0, 10, 12});
    check("1b: bytes", f.out == "xabxxxxabxab");
    // example 3: no context = the covered runs; example 4: the largest context = the documents grep keeps
    const auto z = m.excerpts_batch(text, offs, 0, 0);
    check("3: covered runs", z.starts == Offs{2, 8, 11} && z.out == "ababab");
    const auto all = m.excerpts_batch(text, offs, 0x7FFFFFFFu, 0x7FFFFFFFu);
    Offs kept, doo;
    const std::string g = m.grep_batch(text, offs, false, &kept, &doo);
    check("4: grep's documents", all.out == g && all.starts == Offs{0, 11} && all.out_offsets == doo);
    const auto none = m.excerpts_batch("xxxx", {0, 4}, 2, 2);
    check("no hit: no excerpt", none.size() == 0 && none.out.empty() && none.out_offsets == Offs{0} && none.n_hits == 0);
  }
  {  // example 2: the context ends inside characters and is snapped outwards
    auto m = AC::compile({"\xE6\x98\xAF"});
    const std::string text = "\xE6\x88\x91\xE6\x98\xAF\xE4\xB8\xAD";
    const auto e = m.excerpts_batch(text, {0, 9}, 1, 1);
    check("2: the whole document", e.starts == Offs{0} && e.out == text && e.n_hits == 1);
  }
  {  // refused before any device work
    auto m = AC::compile({"ab"});
    bool threw = false;
    try {
      m.excerpts_batch("ab", {0, 2}, 0x80000000u, 0);
    } catch (const aha::Error &) {
      threw = true;
    }
    check("a context above 0x7FFFFFFF is refused", threw);
  }
  std::printf("%d failure(s)\n", fails);
  return fails ? 1 : 0;
}
