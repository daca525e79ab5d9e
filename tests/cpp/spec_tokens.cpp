// Token calls through include/aha/ac.hpp (AC::tokens_batch, AC::tokens, AC::tokens_batch_device) against forward maximum
// matching written out over AC::select_batch of the same batch: built by tests/test_tokens_host.py (compiles) and run on the
// GPU by tests/test_gpu_tokens_cpp.py.
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

// the selection of every document filled up: between two selected hits one token per character, or one per gap
static std::vector<aha::Hit> fill(const std::string &corpus, const std::vector<uint64_t> &offs, const std::vector<aha::Hit> &sel,
                                  const std::vector<uint64_t> &dso, bool gap_runs, std::vector<uint64_t> *dto) {
  std::vector<aha::Hit> out;
  dto->assign(1, 0);
  for (size_t d = 0; d + 1 < offs.size(); d++) {
    const int32_t n = (int32_t)(offs[d + 1] - offs[d]);
    const unsigned char *doc = reinterpret_cast<const unsigned char *>(corpus.data()) + offs[d];
    uint64_t i = dso[d];
    for (int32_t p = 0; p < n;) {
      if (i < dso[d + 1] && sel[i].start == p) {
        out.push_back(sel[i]);
        p = sel[i++].end;
        continue;
      }
      const int32_t stop = i < dso[d + 1] ? sel[i].start : n;
      int32_t q = p + 1;
      while (q < stop && (gap_runs || (doc[q] & 0xC0) == 0x80)) q++;
      out.push_back(aha::Hit{p, q, -1});
      p = q;
    }
    dto->push_back(out.size());
  }
  return out;
}

int main() {
  auto m = aha::AC::compile({"我是", "中国", "he", "she", "hers"});
  std::string corpus;
  std::vector<uint64_t> offs = {0};
  for (const char *doc : {"我是中国人", "", "ushers, 中国 and 我是!", "\x80\x80plain"}) {  // (the last is cut inside a character)
    corpus += doc;
    offs.push_back(corpus.size());
  }
  std::vector<uint64_t> dso, dto, want_dto;
  const auto sel = m.select_batch(corpus, offs, &dso);
  for (int gap = 0; gap < 2; gap++) {
    const auto want = fill(corpus, offs, sel, dso, gap != 0, &want_dto);
    uint64_t n_hits = 0;
    const auto toks = m.tokens_batch(corpus, offs, gap != 0, &dto, &n_hits);
    check(gap ? "tokens_batch, gap runs: tokens" : "tokens_batch: tokens", same(toks, want) && toks.size() > sel.size());
    check(gap ? "tokens_batch, gap runs: doc_tok_offsets" : "tokens_batch: doc_tok_offsets", dto == want_dto);
    check("tokens_batch: deterministic", same(m.tokens_batch(corpus, offs, gap != 0), toks));
    // the device form on a corpus in HBM: a sizing call, then the tokens
    aha::Corpus c(corpus, offs);
    const aha_corpus *h = c.handle();
    const int dev = aha_corpus_device(h);
    uint64_t need = 0;
    bool sized = false;
    try {
      m.tokens_batch_device(aha_corpus_bytes(h), aha_corpus_doc_offsets(h), offs.size() - 1, corpus.size(), nullptr, 0, nullptr, gap != 0,
                            &need);
    } catch (const aha::Error &e) {
      sized = e.code == AHA_E_CAPACITY;
    }
    check("tokens_batch_device: sizing call", sized && need == want.size());
    void *d_out = nullptr, *d_dto = nullptr;
    bool ok = aha_buffer_alloc(dev, need * sizeof(aha::Hit), &d_out) == AHA_OK &&
              aha_buffer_alloc(dev, offs.size() * sizeof(uint64_t), &d_dto) == AHA_OK;
    std::vector<aha::Hit> got(need);
    std::vector<uint64_t> got_dto(offs.size());
    if (ok) {
      const uint64_t n = m.tokens_batch_device(aha_corpus_bytes(h), aha_corpus_doc_offsets(h), offs.size() - 1, corpus.size(),
                                               static_cast<aha::Hit *>(d_out), need, static_cast<uint64_t *>(d_dto), gap != 0);
      ok = n == need && aha_buffer_download(dev, got.data(), d_out, need * sizeof(aha::Hit)) == AHA_OK &&
           aha_buffer_download(dev, got_dto.data(), d_dto, offs.size() * sizeof(uint64_t)) == AHA_OK;
    }
    aha_buffer_free(dev, d_out);
    aha_buffer_free(dev, d_dto);
    check("tokens_batch_device: tokens and offsets", ok && same(got, want) && got_dto == want_dto);
  }
  {
    const auto t = m.tokens("我是中国人");
    check("tokens: the README example", t.size() == 3 && t[0].value == 0 && t[1].value == 1 && t[2].value == -1 && t[2].start == 12 &&
                                            t[2].end == 15);
    check("tokens: empty sequence", m.tokens("").empty());
    check("tokens: no hit at all", m.tokens("xyz").size() == 3 && m.tokens("xyz", true).size() == 1);
  }
  std::printf("%d failures\n", fails);
  return fails ? 1 : 0;
}
