// Feed replace through include/aha/ac.hpp (aha::Feed::replace_batch / replace): the header's own example, the "longer key
// completes later" case, FINAL, and the stream law against AC::replace_batch of the whole.  Run on the GPU by
// tests/test_gpu_feed_replace_cpp.py.
#include <cstdio>
#include <string>
#include <vector>

#include "aha/ac.hpp"

static int fails = 0;
static void check(const std::string &name, bool ok) {
  std::printf("%s %s\n", ok ? "ok  " : "FAIL", name.c_str());
  if (!ok) fails++;
}

int main() {
  {  // the header's example: keys ab -> "<AB>", abcde -> "" (W = 4)
    auto m = aha::AC::compile({"ab", "abcde"});
    const auto table = m.replacements({"<AB>", ""});
    aha::Feed f(m, 2);
    aha::Feed::Replace info;
    auto out = f.replace_batch("xab", {0, 3}, {1}, table, false, &info);
    check("nothing lies in front of F(3) = 0", out.empty() && info.piece_hold == std::vector<uint32_t>({3}) &&
                                                   info.bases == std::vector<uint64_t>({0}) && info.n_selected == 0 && info.n_hits == 1);
    out = f.replace_batch("cd", {0, 2}, {1}, table, false, &info);
    check("x is final", out == "x" && info.piece_hold[0] == 4 && info.bases[0] == 3 && info.piece_out_offsets[1] == 1);
    out = f.replace_batch("eab", {0, 3}, {1}, table, false, &info);
    check("the longer key completes later and is deleted", out.empty() && info.piece_hold[0] == 2 && info.n_selected == 1 &&
                                                               f.position(1).first == 8);
    out = f.replace_batch("", {0, 0}, {1}, table, true, &info);
    check("FINAL with an empty piece", out == "<AB>" && info.piece_hold[0] == 0 && f.position(1).first == 0);
    check("the sequence starts again", f.replace(1, "abcdeab", table, true) == "<AB>" && f.position(1).first == 0);
    // two pieces in one call, in this order in out
    out = f.replace_batch("ababxcde", {0, 3, 8}, {1, 0}, table, true, &info);
    check("two sequences in one call", out == "<AB>abxcde" && info.piece_out_offsets == std::vector<uint64_t>({0, 5, 10}));
    bool refused = false;
    f.match(0, "ab");
    try {
      f.replace(0, "cde", table);
    } catch (const aha::Error &) {
      refused = true;
    }
    check("replace behind a match call is refused", refused && f.position(0).first == 2);
    f.reset(0);
    check("... until reset", f.replace(0, "abcde", table, true).empty());
    // select and replace calls mixed
    check("a select call first", f.select(0, "xabc").empty());
    check("then replace from where the cursor stands", f.replace(0, "deab", table) == "x" && f.replace(0, "", table, true) == "<AB>");
  }
  {  // a kept key, and a table of another handle
    auto m = aha::AC::compile({"ab", "bcd", "cd", "d"});
    const auto table = m.replacements({"1", "22", "", "four"}, {false, false, false, true});
    const std::string text = "abcdabcddx";
    const auto want = m.replace_batch(text, {0, text.size()}, table);
    check("the whole", want == "11dx");
    for (size_t cut = 0; cut <= text.size(); cut++) {
      aha::Feed f(m, 3);
      auto got = f.replace(2, text.substr(0, cut), table);
      got += f.replace(2, text.substr(cut), table, true);
      check("abcdabcddx cut at " + std::to_string(cut), got == want && f.position(2).first == 0);
    }
    auto other = aha::AC::compile({"ab", "bcd", "cd", "d"});
    aha::Feed g(other, 1);
    bool refused = false;
    try {
      g.replace(0, "abcd", table, true);
    } catch (const aha::Error &) {
      refused = true;
    }
    check("a table of another handle is refused", refused && g.position(0).first == 0);
  }
  {  // the stream law on a longer text, pieces of every small size
    auto m = aha::AC::compile({"he", "she", "his", "hers", "ushers", "said his", "s"});
    const auto table = m.replacements({"HE", "", "<his>", "hers and more", "U", "", "s"}, {false, false, false, false, false, false, true});
    const std::string text = "ushers she said his hers hehehe ushers ssh";
    const auto want = m.replace_batch(text, {0, text.size()}, table);
    check("the whole differs from the text", want != text && !want.empty());
    for (size_t step : {1, 2, 3, 5, 7, 64}) {
      aha::Feed f(m, 1);
      std::string got;
      for (size_t a = 0; a < text.size(); a += step) got += f.replace(0, text.substr(a, step), table, a + step >= text.size());
      check("stream law over pieces of " + std::to_string(step) + " bytes", got == want);
    }
  }
  std::printf("%d failures\n", fails);
  return fails ? 1 : 0;
}
