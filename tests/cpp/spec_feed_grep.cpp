// Feed grep through include/aha/ac.hpp (aha::Feed::grep_batch / grep): the three traps of the header, the per-piece outputs of
// a worked example, FINAL with an empty piece, mixing and the stream law against AC::grep of the whole at every cut and over
// pieces of every small size.  Run on the GPU by tests/test_gpu_feed_grep_cpp.py.
#include <cstdio>
#include <string>
#include <vector>

#include "aha/ac.hpp"

static int fails = 0;
static void check(const std::string &name, bool ok) {
  std::printf("%s %s\n", ok ? "ok  " : "FAIL", name.c_str());
  if (!ok) fails++;
}
using Lines = std::vector<std::string>;
static Lines stream(aha::AC &m, const std::string &text, const std::vector<size_t> &cuts, bool invert = false) {
  aha::Feed f(m, 2);
  Lines got;
  size_t a = 0;
  for (size_t i = 0; i <= cuts.size(); i++) {
    const size_t b = i < cuts.size() ? cuts[i] : text.size();
    const Lines l = f.grep(1, text.substr(a, b - a), '\n', invert, i == cuts.size());
    got.insert(got.end(), l.begin(), l.end());
    a = b;
  }
  return got;
}

int main() {
  {  // keys abc, b; pieces "a" | "b\n": the record "ab\n" has no hit, the fragment "b\n" from the root has one
    auto m = aha::AC::compile({"abc", "b"});
    check("trap 1: the whole", m.grep("ab\n").empty());
    check("trap 1: a | b\\n", stream(m, "ab\n", {1}).empty());
    check("trap 1: inverted", stream(m, "ab\n", {1}, true) == Lines({"ab\n"}));
  }
  {  // keys x\nabc, b; the record "ab\n" has a hit, the sequence "x\nab\n" matched as one text has none
    auto m = aha::AC::compile({"x\nabc", "b"});
    check("trap 2: the whole", m.grep("x\nab\n") == Lines({"ab\n"}) && m.match("x\nab\n").empty());
    for (size_t cut = 0; cut <= 5; cut++)
      check("trap 2: cut at " + std::to_string(cut), stream(m, "x\nab\n", {cut}) == Lines({"ab\n"}));
  }
  {  // a key \nb never hits in a record; a key b\n only at a record's end
    auto m = aha::AC::compile({"\nb"});
    check("trap 3: \\nb", stream(m, "a\nb\nb", {2}).empty() && stream(m, "a\nb\nb", {1, 3}).empty());
    auto e = aha::AC::compile({"b\n"});
    check("trap 3: b\\n", stream(e, "ab\nb", {2}) == Lines({"ab\n"}) && stream(e, "ab\nb", {3}) == Lines({"ab\n"}));
  }
  {  // the per-piece outputs
    auto m = aha::AC::compile({"abc", "cab"});
    aha::Feed f(m, 3);
    aha::Feed::Grep g;
    std::string out = f.grep_batch("xa", {0, 2}, {2}, '\n', false, false, &g);
    check("an open piece", out.empty() && g.piece_hold == std::vector<uint32_t>({2}) && g.piece_head[0] == 0 && g.n_recs == 1 &&
                               g.kept_recs.empty() && g.bases[0] == 0);
    out = f.grep_batch("bcyy", {0, 4}, {2}, '\n', false, false, &g);
    check("the hit in the straddle, still open", out.empty() && g.piece_hold[0] == 4 && g.piece_head[0] == 0 && g.bases[0] == 2);
    out = f.grep_batch("z\nq\ncab\nw", {0, 9}, {2}, '\n', false, false, &g);
    check("it closes and is kept", out == "z\ncab\n" && g.piece_head[0] == 6 && g.piece_hold[0] == 1 && g.n_recs == 4 &&
                                       g.kept_recs == std::vector<uint64_t>({0, 2}) &&
                                       g.rec_out_offsets == std::vector<uint64_t>({0, 2, 6}) &&
                                       g.piece_kept_offsets == std::vector<uint64_t>({0, 2}) && g.piece_rec_bases[0] == 0 &&
                                       g.bases[0] == 6);
    out = f.grep_batch("", {0, 0}, {2}, '\n', true, true, &g);
    check("FINAL with an empty piece, inverted", out.empty() && g.piece_head[0] == 1 && g.piece_hold[0] == 0 && g.n_recs == 0 &&
                                                     g.piece_rec_bases[0] == 3 && f.position(2).first == 0);
    bool refused = false;
    f.match(0, "ab");
    try {
      f.grep(0, "c\n");
    } catch (const aha::Error &) {
      refused = true;
    }
    check("grep behind a match call is refused", refused && f.position(0).first == 2);
    f.reset(0);
    check("... until reset", f.grep(0, "abc\n") == Lines({"abc\n"}));
    refused = false;
    try {
      f.grep(1, "abc;", ';');
    } catch (const aha::Error &) {
      refused = true;
    }
    check("another delimiter is refused", refused && f.position(1).first == 0);
  }
  {  // the stream law on a longer text, pieces of every small size
    auto m = aha::AC::compile({"he", "she", "his", "hers", "ushers", "said his", "s\n"});
    const std::string text = "ushers\nno\n\nshe said his\nhers hehehe\nnothing\nushers ss\nh";
    for (bool invert : {false, true}) {
      const Lines want = m.grep(text, '\n', invert);
      for (size_t step : {1, 2, 3, 5, 7, 64}) {
        aha::Feed f(m, 1);
        Lines got;
        for (size_t a = 0; a < text.size(); a += step) {
          const Lines l = f.grep(0, text.substr(a, step), '\n', invert, a + step >= text.size());
          got.insert(got.end(), l.begin(), l.end());
        }
        check("stream law over pieces of " + std::to_string(step) + " bytes" + (invert ? ", inverted" : ""), got == want);
      }
    }
  }
  std::printf("%d failures\n", fails);
  return fails ? 1 : 0;
}
