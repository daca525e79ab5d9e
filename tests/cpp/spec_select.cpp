// Select calls through include/aha/ac.hpp (AC::select_batch, AC::select) against the greedy rule over the match call of the same
// batch: built by tests/test_select_host.py (compiles) and run on the GPU by tests/test_gpu_select_cpp.py.
#include <cstdio>
#include <string>
#include <vector>

#include "aha/ac.hpp"

static int fails = 0;
static void check(const char *name, bool ok) {
  std::printf("%s %s\n", ok ? "ok  " : "FAIL", name);
  if (!ok) fails++;
}

static bool same(const std::vector<aha::Hit> &a, const std::vector<aha::Hit> &b) {
  if (a.size() != b.size()) return false;
  for (size_t i = 0; i < a.size(); i++)
    if (a[i].start != b[i].start || a[i].end != b[i].end || a[i].value != b[i].value) return false;
  return true;
}

// the rule, straight: smallest start at or behind p, of those the largest end
static std::vector<aha::Hit> greedy(const std::vector<aha::Hit> &hits, const std::vector<uint64_t> &dho, std::vector<uint64_t> *dso) {
  std::vector<aha::Hit> out;
  dso->assign(1, 0);
  for (size_t d = 0; d + 1 < dho.size(); d++) {
    int32_t p = 0;
    for (;;) {
      const aha::Hit *best = nullptr;
      for (uint64_t i = dho[d]; i < dho[d + 1]; i++) {
        const aha::Hit &h = hits[i];
        if (h.start < p) continue;
        if (!best || h.start < best->start || (h.start == best->start && h.end > best->end)) best = &h;
      }
      if (!best) break;
      out.push_back(*best);
      p = best->end;
    }
    dso->push_back(out.size());
  }
  return out;
}

int main() {
  {  // the reference's KAT keys and a few more, over a ragged batch
    auto m = aha::AC::compile({"he", "she", "his", "hers", "e", "我", "我是", "是中"});
    const std::string corpus = std::string("ushers she said his hers") + "我是中国人" + "" + "hehehe";
    const std::vector<uint64_t> offs = {0, 24, 24 + 15, 24 + 15, 24 + 15 + 6};
    std::vector<uint64_t> mdho, want_dso, dso;
    const auto hits = m.match_batch(corpus, offs, &mdho);
    const auto want = greedy(hits, mdho, &want_dso);
    uint64_t n_hits = 0;
    const auto sel = m.select_batch(corpus, offs, &dso, &n_hits);
    check("select_batch: hits", same(sel, want) && !sel.empty());
    check("select_batch: doc_sel_offsets", dso == want_dso);
    check("select_batch: all hits", n_hits == hits.size());
    check("select_batch: deterministic", same(m.select_batch(corpus, offs), sel));
    const auto one = m.select("ushers");
    std::vector<uint64_t> d1, w1;
    const auto h1 = m.match_batch("ushers", {0, 6}, &d1);
    check("select: one sequence", same(one, greedy(h1, d1, &w1)));
  }
  {  // a selected hit that is not the first at its end: at end 4 the own key is bcd, cd hangs on its chain
    auto m = aha::AC::compile({"ab", "bcd", "cd", "d"});
    const auto sel = m.select("abcd");
    check("chain case", sel.size() == 2 && sel[0].start == 0 && sel[0].end == 2 && sel[0].value == 0 && sel[1].start == 2 &&
                            sel[1].end == 4 && sel[1].value == 2);
    check("empty sequence", m.select("").empty());
  }
  std::printf("%d failures\n", fails);
  return fails ? 1 : 0;
}
