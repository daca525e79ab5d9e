// Context lines through include/aha/ac.hpp (AC::grep_lines_batch): the example of include/aha_hip.h under AHA_GREP_LINES: built by
// tests/test_grep_lines_host.py (compiles) and run on the GPU by tests/test_gpu_grep_lines_cpp.py.
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
  using Flags = std::vector<uint8_t>;
  auto m = AC::compile({"ab"});
  const std::string text = "x\nab\ny\nz\nab\nw\n";
  const Offs offs{0, 2, 5, 7, 9, 12, 14};
  {  // before = 1, after = 0, no groups
    AC::LinesOptions o;
    o.before = 1;
    const auto l = m.grep_lines_batch(text, offs, o);
    check("a: kept", l.kept_docs == Offs{0, 1, 3, 4});
    check("a: is_match", l.is_match == Flags{0, 1, 0, 1});
    check("a: offsets", l.doc_out_offsets == Offs{0, 2, 5, 7, 10});
    check("a: bytes", l.out == "x\nab\nz\nab\n" && l[0] == "x\n" && l[3] == "ab\n");
    check("a: all hits", l.n_hits == 2);
    check("a: deterministic", m.grep_lines_batch(text, offs, o).out == l.out);
  }
  {  // the same with two groups: line 3 is not context of line 4
    AC::LinesOptions o;
    o.before = 1;
    o.groups = {0, 4, 6};
    const auto l = m.grep_lines_batch(text, offs, o);
    check("b: kept", l.kept_docs == Offs{0, 1, 4} && l.is_match == Flags{0, 1, 1} && l.out == "x\nab\nab\n");
  }
  {  // invert, no context
    AC::LinesOptions o;
    o.invert = true;
    const auto l = m.grep_lines_batch(text, offs, o);
    check("c: kept", l.kept_docs == Offs{0, 2, 3, 5} && l.is_match == Flags{1, 1, 1, 1} && l.out == "x\ny\nz\nw\n");
  }
  {  // no context = plain grep; the largest context without groups = everything
    AC::LinesOptions o;
    Offs kept, doo;
    const std::string g = m.grep_batch(text, offs, false, &kept, &doo);
    const auto l = m.grep_lines_batch(text, offs, o);
    check("d: plain grep", l.out == g && l.kept_docs == kept && l.doc_out_offsets == doo && l.is_match == Flags{1, 1});
    o.before = o.after = 0x7FFFFFFFu;
    check("d: every record", m.grep_lines_batch(text, offs, o).out == text);
    check("d: no match, nothing", AC::compile({"qq"}).grep_lines_batch(text, offs, o).size() == 0);
  }
  {  // refused before any device work
    bool threw = false;
    try {
      AC::LinesOptions o;
      o.before = 0x80000000u;
      m.grep_lines_batch(text, offs, o);
    } catch (const aha::Error &) {
      threw = true;
    }
    check("a context above 0x7FFFFFFF is refused", threw);
  }
  std::printf("%d failure(s)\n", fails);
  return fails ? 1 : 0;
}
