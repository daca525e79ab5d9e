// Replace calls through include/aha/ac.hpp (AC::Replacements, AC::replace_batch) against slices joined over AC::select_batch of
// the same batch: built by tests/test_replace_host.py (compiles) and run on the GPU by tests/test_gpu_replace_cpp.py.
#include <cstdio>
#include <string>
#include <vector>

#include "aha/ac.hpp"

static int fails = 0;
static void check(const char *name, bool ok) {
  std::printf("%s %s\n", ok ? "ok  " : "FAIL", name);
  if (!ok) fails++;
}

// the contract, straight: per document the slices between the selected hits joined with the replacements
static std::string joined(const std::string &corpus, const std::vector<uint64_t> &offs, const std::vector<aha::Hit> &sel,
                          const std::vector<uint64_t> &dso, const std::vector<std::string> &repl, const std::vector<bool> &keep,
                          std::vector<uint64_t> *doo) {
  std::string out;
  doo->assign(1, 0);
  for (size_t d = 0; d + 1 < offs.size(); d++) {
    const std::string doc = corpus.substr(offs[d], offs[d + 1] - offs[d]);
    size_t at = 0;
    for (uint64_t i = dso[d]; i < dso[d + 1]; i++) {
      const aha::Hit &h = sel[i];
      out += doc.substr(at, h.start - at);
      out += keep[h.value] ? doc.substr(h.start, h.end - h.start) : repl[h.value];
      at = h.end;
    }
    out += doc.substr(at);
    doo->push_back(out.size());
  }
  return out;
}

int main() {
  {  // the reference's KAT keys and a few more, over a ragged batch: shorter, equal, longer, empty, with NUL, kept
    auto m = aha::AC::compile({"he", "she", "his", "hers", "e", "我", "我是", "是中"});
    const std::vector<std::string> repl = {"HE", "", "their own", std::string("h\0s", 3), "-", "I", "", "x"};
    const std::vector<bool> keep = {false, false, false, false, true, false, true, false};
    const std::string corpus = std::string("ushers she said his hers") + "我是中国人" + "" + "hehehe";
    const std::vector<uint64_t> offs = {0, 24, 24 + 15, 24 + 15, 24 + 15 + 6};
    std::vector<uint64_t> dso, want_doo, doo;
    uint64_t sel_hits = 0;
    const auto sel = m.select_batch(corpus, offs, &dso, &sel_hits);
    const std::string want = joined(corpus, offs, sel, dso, repl, keep, &want_doo);
    auto table = m.replacements(repl, keep);
    uint64_t n_sel = 0, n_hits = 0;
    const std::string got = m.replace_batch(corpus, offs, table, &doo, &n_sel, &n_hits);
    check("replace_batch: bytes", got == want && got != corpus);
    check("replace_batch: doc_out_offsets", doo == want_doo);
    check("replace_batch: counts", n_sel == sel.size() && n_hits == sel_hits);
    check("replace_batch: deterministic", m.replace_batch(corpus, offs, table) == got);
    aha::AC::Replacements moved = std::move(table);
    check("Replacements: moved", moved.handle() != nullptr && table.handle() == nullptr &&
                                     m.replace_batch(corpus, offs, moved) == got);
    auto other = aha::AC::compile({"he", "she", "his", "hers", "e", "我", "我是", "是中"});
    bool refused = false;
    try {
      other.replace_batch(corpus, offs, moved);
    } catch (const aha::Error &) {
      refused = true;
    }
    check("a table of another handle is refused", refused);
  }
  {  // a selected hit that is not the first at its end: at end 4 the own key is bcd, cd hangs on its chain
    auto m = aha::AC::compile({"ab", "bcd", "cd", "d"});
    auto t = m.replacements({"<AB>", "?", "", "!"});
    check("chain case", m.replace_batch("abcd", {0, 4}, t) == "<AB>");
    check("empty sequence", m.replace_batch("", {0, 0}, t).empty());
    std::vector<uint64_t> doo;
    check("everything deleted", m.replace_batch("cdcd", {0, 2, 4}, t, &doo).empty() && doo == std::vector<uint64_t>({0, 0, 0}));
  }
  std::printf("%d failures\n", fails);
  return fails ? 1 : 0;
}
