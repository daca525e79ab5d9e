// Feed tokens through include/aha/ac.hpp (aha::Feed::tokens_batch / tokens): the header's four examples, call by call, and the
// stream law against AC::tokens of the whole, in both gap modes.  Run on the GPU by tests/test_gpu_feed_tokens_cpp.py.
#include <cstdio>
#include <string>
#include <vector>

#include "aha/ac.hpp"

static int fails = 0;
static void check(const std::string &name, bool ok) {
  std::printf("%s %s\n", ok ? "ok  " : "FAIL", name.c_str());
  if (!ok) fails++;
}
using Toks = std::vector<aha::Hit>;
static bool same(const Toks &a, const Toks &b) {
  if (a.size() != b.size()) return false;
  for (size_t i = 0; i < a.size(); i++)
    if (a[i].start != b[i].start || a[i].end != b[i].end || a[i].value != b[i].value) return false;
  return true;
}
static aha::Hit tok(int32_t s, int32_t e, int32_t v) {
  aha::Hit h;
  h.start = s;
  h.end = e;
  h.value = v;
  return h;
}
// one call on sequence 1: the tokens with absolute offsets and the hold
static bool step(aha::Feed &f, const std::string &piece, bool final, bool gap_runs, const Toks &want, uint32_t hold) {
  aha::Feed::Select info;
  auto got = f.tokens_batch(piece, {0, piece.size()}, {1}, final, gap_runs, &info);
  for (auto &t : got) {
    t.start += (int32_t)info.bases[0];
    t.end += (int32_t)info.bases[0];
  }
  return same(got, want) && info.piece_hold[0] == hold && info.piece_sel_offsets[1] == want.size();
}
static Toks joined(const Toks &t) {
  Toks out;
  for (const auto &x : t) {
    if (!out.empty() && x.value == -1 && out.back().value == -1 && out.back().end == x.start)
      out.back().end = x.end;
    else
      out.push_back(x);
  }
  return out;
}

int main() {
  {  // keys ab, abcde: W = 4
    auto m = aha::AC::compile({"ab", "abcde"});
    aha::Feed f(m, 2);
    check("1: xab", step(f, "xab", false, false, {}, 3));
    check("1: cd", step(f, "cd", false, false, {tok(0, 1, -1)}, 4));
    check("1: eab", step(f, "eab", false, false, {tok(1, 6, 1)}, 2));
    check("1: FINAL", step(f, "", true, false, {tok(6, 8, 0)}, 0) && f.position(1).first == 0);
    bool refused = false;
    f.select(0, "ab");
    try {
      f.tokens(0, "cde");
    } catch (const aha::Error &) {
      refused = true;
    }
    check("tokens behind a select call are refused", refused && f.position(0).first == 2);
    f.reset(0);
    check("... until reset", f.tokens(0, "abcde", true).size() == 1);
  }
  {  // a key of one character between two others, cut 4 | 4 | 1
    auto m = aha::AC::compile({"\xE6\x98\xAF"});
    const std::string t = "\xE6\x88\x91\xE6\x98\xAF\xE4\xB8\xAD";
    aha::Feed f(m, 2);
    check("2: first", step(f, t.substr(0, 4), false, false, {}, 4));
    check("2: second", step(f, t.substr(4, 4), false, false, {tok(0, 3, -1), tok(3, 6, 0)}, 2));
    check("2: third", step(f, t.substr(8), false, false, {}, 3));
    check("2: FINAL", step(f, "", true, false, {tok(6, 9, -1)}, 0));
  }
  {  // W = 0 and a character whose bytes arrive one by one
    auto m = aha::AC::compile({"a"});
    aha::Feed f(m, 2);
    check("3: first", step(f, "xa\xC3", false, false, {tok(0, 1, -1), tok(1, 2, 0)}, 1));
    check("3: second", step(f, "\xA9", false, false, {}, 2));
    check("3: third", step(f, "y", false, false, {tok(2, 4, -1)}, 1));
    check("3: FINAL", step(f, "", true, false, {tok(4, 5, -1)}, 0));
  }
  {  // gaps as runs come in parts
    auto m = aha::AC::compile({"ab"});
    aha::Feed f(m, 2);
    check("4: first", step(f, "zzzzzz", false, true, {tok(0, 5, -1)}, 1));
    check("4: second", step(f, "zzab", false, true, {tok(5, 8, -1), tok(8, 10, 0)}, 0));
    check("4: FINAL", step(f, "zz", true, true, {tok(10, 12, -1)}, 0));
  }
  {  // the stream laws on a longer text, pieces of every small size
    auto m = aha::AC::compile({"he", "she", "his", "hers", "ushers", "said his", "\xE4\xB8\xAD\xE5\x9B\xBD"});
    const std::string text = "ushers she said \xE6\x88\x91\xE6\x98\xAF\xE4\xB8\xAD\xE5\x9B\xBD\xE4\xBA\xBA his hers \xC3\xA9\x80\x80 hehe";
    for (bool gap_runs : {false, true}) {
      const auto want = m.tokens(text, gap_runs);
      for (size_t step_len : {1, 2, 3, 5, 7, 64}) {
        aha::Feed f(m, 1);
        Toks got;
        for (size_t a = 0; a < text.size(); a += step_len) {
          const auto h = f.tokens(0, text.substr(a, step_len), a + step_len >= text.size(), gap_runs);
          got.insert(got.end(), h.begin(), h.end());
        }
        check(std::string(gap_runs ? "gap runs" : "characters") + ": stream law over pieces of " + std::to_string(step_len) + " bytes",
              same(gap_runs ? joined(got) : got, want));
      }
    }
  }
  std::printf("%d failures\n", fails);
  return fails ? 1 : 0;
}
