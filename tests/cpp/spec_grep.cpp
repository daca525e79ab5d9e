// Records and grep calls through include/aha/ac.hpp (AC::records_batch, AC::grep_batch, AC::grep): the worked example of
// include/aha_hip.h and its inverted form: built by tests/test_grep_host.py (compiles) and run on the GPU by
// tests/test_gpu_grep_cpp.py.
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
  auto m = aha::AC::compile({"ab", "b\n"});
  const std::string text = "xab\nq\n\nb";
  using Offs = std::vector<uint64_t>;
  {  // records: "xab\n", "q\n", "\n", "b"
    Offs dro;
    const Offs rec = m.records_batch(text, {0, text.size()}, '\n', &dro);
    check("records: offsets", rec == Offs{0, 4, 6, 7, 8});
    check("records: doc_rec_offsets", dro == Offs{0, 4});
    check("records: one sequence", m.records(text) == rec);
    Offs dro2;
    const Offs rec2 = m.records_batch(text, {0, 0, 4, 5, 8, 8}, '\n', &dro2);  // boundaries on, behind and before delimiters
    check("records: document ends are record ends", rec2 == Offs{0, 4, 5, 6, 7, 8} && dro2 == Offs{0, 0, 1, 2, 5, 5});
    check("records: no delimiter", m.records("abc") == Offs{0, 3} && m.records("") == Offs{0});
  }
  {  // grep over the records: "b\n" anchors at a record's end, so it hits in "xab\n" and not in the last record
    const Offs rec = m.records(text);
    Offs kept, doo;
    uint64_t n_hits = 0;
    const std::string out = m.grep_batch(text, rec, false, &kept, &doo, &n_hits);
    check("grep: kept_docs", kept == Offs{0});
    check("grep: doc_out_offsets", doo == Offs{0, 4});
    check("grep: bytes", out == "xab\n");
    check("grep: all hits", n_hits == 2);
    check("grep: deterministic", m.grep_batch(text, rec) == out);
    const std::string inv = m.grep_batch(text, rec, true, &kept, &doo);
    check("grep inverted: kept_docs", kept == Offs{1, 2, 3});
    check("grep inverted: doc_out_offsets", doo == Offs{0, 2, 3, 4});
    check("grep inverted: bytes", inv == "q\n\nb");
  }
  {  // the composition
    using Lines = std::vector<std::string>;
    check("grep: lines", m.grep(text) == Lines{"xab\n"});
    check("grep: lines inverted", m.grep(text, '\n', true) == Lines{"q\n", "\n", "b"});
    check("grep: nothing kept", m.grep("q\nq\n").empty() && m.grep("", '\n', true).empty());
    check("grep: another delimiter", m.grep("ab;q;b\n;", ';') == Lines{"ab;", "b\n;"});
  }
  if (fails) std::printf("%d FAILED\n", fails);
  return fails ? 1 : 0;
}
