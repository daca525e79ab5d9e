// aha/ac.hpp -- C++ host-side mirror of the reference's Crystal API for the
// accelerated path, on top of the C ABI (include/aha_hip.h):
//
//   Aha::AC.compile(keys)                    src/aha/ac.cr:62-69
//   AC#match(seq : Bytes) { |hit| }          src/aha/ac.cr:280-286
//   AC#match(seq : String) { |hit| }         src/aha/matcher.cr:34-39  (char offsets)
//   AC#match(seq, sep : BitArray) { |hit| }  src/aha/ac.cr:321-340, matcher.cr:41-46
//   AC#[](id) / AC#[](key)                   src/aha/ac.cr:41-43
//   Aha::Hit#start/#end/#value               src/aha/matcher.cr:2-11
//
// Errors are thrown as aha::Error carrying the reference's message text.
// Header-only; link with -laha_hip.  No CPU fallback: matching needs a GPU.
#pragma once

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <map>
#include <stdexcept>
#include <string>
#include <string_view>
#include <utility>
#include <vector>

#include "../aha_hip.h"

namespace aha {

using Hit = aha_hit;  // {start, end, value : Int32}

struct Error : std::runtime_error {
  int32_t code;
  uint32_t key_index;
  Error(int32_t c, const std::string &msg, uint32_t k = 0) : std::runtime_error(msg), code(c), key_index(k) {}
};

// BitArray as used by match(seq, sep)
class BitArray {
 public:
  explicit BitArray(int size) : size_(size), bits_((size_t)(size > 0 ? (size + 7) / 8 : 1), 0) {}
  int size() const { return size_; }
  void set(int i, bool v = true) {
    if (i < 0 || i >= size_) throw std::out_of_range("BitArray index");
    if (v)
      bits_[(size_t)i >> 3] |= (uint8_t)(1u << (i & 7));
    else
      bits_[(size_t)i >> 3] &= (uint8_t)~(1u << (i & 7));
  }
  const std::vector<uint8_t> &bytes() const { return bits_; }

 private:
  int size_;
  std::vector<uint8_t> bits_;
};

// A batch resident in HBM (aha_corpus_upload): uploaded once, matched as often as wanted -- by AC::match_corpus.
class Corpus {
 public:
  Corpus(std::string_view bytes, const std::vector<uint64_t> &doc_offsets, int device = 0) {
    if (doc_offsets.empty()) throw Error(AHA_E_INVALID, "doc_offsets holds D + 1 entries");
    int32_t rc = aha_corpus_upload(device, reinterpret_cast<const uint8_t *>(bytes.data()), doc_offsets.data(),
                                   doc_offsets.size() - 1, &c_);
    if (rc != AHA_OK) {
      const char *m = aha_last_error(nullptr);
      throw Error(rc, (m && *m) ? m : aha_strerror(rc));
    }
  }
  Corpus(const Corpus &) = delete;
  Corpus &operator=(const Corpus &) = delete;
  ~Corpus() { aha_corpus_free(c_); }
  const aha_corpus *handle() const { return c_; }

 private:
  aha_corpus *c_ = nullptr;
};

class AC {
 public:
  AC(const AC &) = delete;
  AC &operator=(const AC &) = delete;
  AC(AC &&o) noexcept : h_(o.h_) { o.h_ = nullptr; }
  ~AC() { aha_ac_free(h_); }

  // Aha::AC.compile(keys).  fold_ascii: an ASCII case-insensitive handle (AHA_OPT_FOLD_ASCII, aha_hip.h): every call gives what a
  // plain handle compiled from the lower-cased keys gives over the lower-cased text; key(id) keeps the spelling given here.
  // fold_simple: that plus the simple case fold of the two-byte UTF-8 characters (AHA_OPT_FOLD_SIMPLE: Latin-1, Latin
  // Extended-A/B, Greek, Cyrillic, Armenian), every document folded on its own; such a handle has no feeds and no groups yet.
  // fold_bmp: that plus the three-byte characters (AHA_OPT_FOLD_BMP: full-width Latin, Vietnamese, polytonic Greek, Georgian,
  // Cherokee, Glagolitic, Coptic ..), with the same limits.  fold_kana: that plus hiragana and half-width katakana matched as
  // katakana (AHA_OPT_FOLD_KANA: length-preserving, so a half-width letter and its voiced mark stay two characters)
  static AC compile(const std::vector<std::string> &keys, int device = -1, bool fold_ascii = false, bool fold_simple = false,
                    bool fold_bmp = false, bool fold_kana = false) {
    std::vector<uint8_t> blob;
    std::vector<uint64_t> offs(keys.size() + 1, 0);
    for (size_t i = 0; i < keys.size(); i++) {
      blob.insert(blob.end(), keys[i].begin(), keys[i].end());
      offs[i + 1] = blob.size();
    }
    aha_options o{};
    o.struct_size = sizeof(o);
    o.device = device;
    o.flags = (fold_ascii ? AHA_OPT_FOLD_ASCII : 0u) | (fold_simple ? AHA_OPT_FOLD_SIMPLE : 0u) | (fold_bmp ? AHA_OPT_FOLD_BMP : 0u) |
              (fold_kana ? AHA_OPT_FOLD_KANA : 0u);
    aha_ac *h = nullptr;
    uint32_t bad = 0;
    int32_t rc = aha_ac_compile(blob.data(), offs.data(), (uint32_t)keys.size(), &o, &h, &bad);
    if (rc == AHA_E_DUP_KEY) throw Error(rc, "key:" + keys[bad] + " appear twice.", bad);  // ac.cr:66
    if (rc != AHA_OK) throw Error(rc, aha_strerror(rc), bad);
    return AC(h);
  }

  // AC#match(seq : Bytes) -- byte offsets; hits in the reference's order
  template <class F>
  void match(std::string_view seq, F &&block) const {
    run(seq, nullptr, false, std::forward<F>(block));
  }
  // AC#match(seq : String) -- char offsets (valid UTF-8)
  template <class F>
  void match_string(std::string_view seq, F &&block) const {
    run(seq, nullptr, true, std::forward<F>(block));
  }
  // AC#match(seq, sep)
  template <class F>
  void match(std::string_view seq, const BitArray &sep, F &&block, bool chars = false) const {
    run(seq, &sep, chars, std::forward<F>(block));
  }
  std::vector<Hit> match(std::string_view seq, bool chars = false) const {
    std::vector<Hit> v;
    run(seq, nullptr, chars, [&](const Hit &h) { v.push_back(h); });
    return v;
  }
  // AC#match_longest(seq, intersectable = false) -- src/aha/ac.cr:297-319 (String form: chars = true)
  template <class F>
  void match_longest(std::string_view seq, bool intersectable, F &&block, bool chars = false) const {
    run(seq, nullptr, chars, std::forward<F>(block), intersectable ? 2 : 1);
  }
  // D documents in one call (new: the reference is one sequence per call): hits of all documents in document order,
  // doc_hit_offsets[d] .. doc_hit_offsets[d + 1] are document d's
  std::vector<Hit> match_batch(std::string_view corpus, const std::vector<uint64_t> &doc_offsets,
                               std::vector<uint64_t> *doc_hit_offsets = nullptr, bool chars = false) const {
    if (doc_offsets.empty()) throw Error(AHA_E_INVALID, "doc_offsets holds D + 1 entries");
    aha_match_params p{};
    p.struct_size = sizeof(p);
    p.char_offsets = chars ? 1 : 0;
    const uint64_t D = doc_offsets.size() - 1;
    std::vector<uint64_t> dho(D + 1);
    std::vector<Hit> out(corpus.size() / 8 + 64);
    uint64_t n = 0;
    for (;;) {
      int32_t rc = aha_ac_match_batch(h_, reinterpret_cast<const uint8_t *>(corpus.data()), doc_offsets.data(), D, &p,
                                      out.data(), out.size(), dho.data(), &n);
      if (rc == AHA_E_CAPACITY) {
        out.resize(n);
        continue;
      }
      if (rc != AHA_OK) {
        const char *m = aha_last_error(h_);
        throw Error(rc, (m && *m) ? m : aha_strerror(rc));
      }
      break;
    }
    out.resize(n);
    if (doc_hit_offsets) *doc_hit_offsets = std::move(dho);
    return out;
  }

  // The same on a batch that already lives in HBM: the device entry point on the library's own buffers (no copy of
  // the corpus per call; the hits are downloaded at the end).
  std::vector<Hit> match_corpus(const Corpus &c, std::vector<uint64_t> *doc_hit_offsets = nullptr,
                                bool chars = false) const {
    const aha_corpus *h = c.handle();
    const int dev = aha_corpus_device(h);
    const uint64_t D = aha_corpus_n_docs(h);
    aha_match_params p{};
    p.struct_size = sizeof(p);
    p.char_offsets = chars ? 1 : 0;
    void *d_dho = nullptr, *d_out = nullptr;
    uint64_t cap = aha_corpus_n_bytes(h) / 8 + 64, n = 0;
    auto fail = [&](int32_t rc, const char *m) {
      aha_buffer_free(dev, d_dho);
      aha_buffer_free(dev, d_out);
      throw Error(rc, (m && *m) ? m : aha_strerror(rc));
    };
    int32_t rc = aha_buffer_alloc(dev, (D + 1) * sizeof(uint64_t), &d_dho);
    if (rc != AHA_OK) fail(rc, aha_last_error(nullptr));
    for (;;) {
      if ((rc = aha_buffer_alloc(dev, cap * sizeof(Hit), &d_out)) != AHA_OK) fail(rc, aha_last_error(nullptr));
      rc = aha_ac_match_batch_device(h_, aha_corpus_bytes(h), aha_corpus_doc_offsets(h), D, aha_corpus_n_bytes(h), &p,
                                     static_cast<Hit *>(d_out), cap, static_cast<uint64_t *>(d_dho), &n, nullptr);
      if (rc != AHA_E_CAPACITY) break;
      aha_buffer_free(dev, d_out);
      d_out = nullptr;
      cap = n;
    }
    if (rc != AHA_OK) fail(rc, aha_last_error(h_));
    std::vector<Hit> out(n);
    std::vector<uint64_t> dho(D + 1);
    if ((rc = aha_buffer_download(dev, out.data(), d_out, n * sizeof(Hit))) != AHA_OK ||
        (rc = aha_buffer_download(dev, dho.data(), d_dho, (D + 1) * sizeof(uint64_t))) != AHA_OK)
      fail(rc, aha_last_error(nullptr));
    aha_buffer_free(dev, d_dho);
    aha_buffer_free(dev, d_out);
    if (doc_hit_offsets) *doc_hit_offsets = std::move(dho);
    return out;
  }

  // K: the number of keys (the length of a key-count vector)
  uint32_t n_keys() const {
    aha_ac_info_t i{};
    i.struct_size = sizeof(i);
    const int32_t rc = aha_ac_info(h_, &i);
    if (rc != AHA_OK) throw Error(rc, aha_strerror(rc));
    return i.n_keys;
  }

  // Hits per key of match_batch without the hit list (aha_ac_count_batch): key_counts[k] = hits with value k.  accumulate:
  // add into *key_counts (which then must hold K entries) instead of overwriting it -- running totals over many batches.
  uint64_t count_batch(std::string_view corpus, const std::vector<uint64_t> &doc_offsets, std::vector<uint64_t> *key_counts,
                       std::vector<uint64_t> *doc_hit_offsets = nullptr, bool accumulate = false) const {
    if (doc_offsets.empty()) throw Error(AHA_E_INVALID, "doc_offsets holds D + 1 entries");
    aha_match_params p{};
    p.struct_size = sizeof(p);
    const uint64_t D = doc_offsets.size() - 1;
    std::vector<uint64_t> dho(D + 1);
    if (key_counts && !accumulate) key_counts->assign(n_keys(), 0);
    if (key_counts && key_counts->size() != n_keys()) throw Error(AHA_E_INVALID, "key_counts holds K entries");
    uint64_t n = 0;
    const int32_t rc = aha_ac_count_batch(h_, reinterpret_cast<const uint8_t *>(corpus.data()), doc_offsets.data(), D, &p,
                                          accumulate ? AHA_COUNT_ACCUMULATE : 0u, key_counts ? key_counts->data() : nullptr,
                                          dho.data(), &n);
    if (rc != AHA_OK) {
      const char *m = aha_last_error(h_);
      throw Error(rc, (m && *m) ? m : aha_strerror(rc));
    }
    if (doc_hit_offsets) *doc_hit_offsets = std::move(dho);
    return n;
  }

  // (the call behind cover_batch / redact_batch: returns *n_covered)
  uint64_t cover_call(std::string_view corpus, const std::vector<uint64_t> &doc_offsets, std::vector<uint32_t> *mask,
                      std::string *redacted, uint8_t fill, std::vector<uint64_t> *doc_covered, uint64_t *n_hits) const {
    if (doc_offsets.empty()) throw Error(AHA_E_INVALID, "doc_offsets holds D + 1 entries");
    aha_match_params p{};
    p.struct_size = sizeof(p);
    const uint64_t D = doc_offsets.size() - 1, N = doc_offsets.back();
    if (mask) mask->assign((N + 31) / 32, 0u);
    if (redacted) redacted->assign(N, '\0');
    if (doc_covered) doc_covered->assign(D, 0);
    uint64_t nc = 0, nh = 0;
    const int32_t rc = aha_ac_cover_batch(h_, reinterpret_cast<const uint8_t *>(corpus.data()), doc_offsets.data(), D, &p, 0,
                                          mask && !mask->empty() ? mask->data() : nullptr,
                                          redacted && N ? reinterpret_cast<uint8_t *>(&(*redacted)[0]) : nullptr, fill,
                                          doc_covered && D ? doc_covered->data() : nullptr, &nc, &nh);
    if (rc != AHA_OK) {
      const char *m = aha_last_error(h_);
      throw Error(rc, (m && *m) ? m : aha_strerror(rc));
    }
    if (n_hits) *n_hits = nh;
    return nc;
  }

  // The document x key table of match_batch without the hit list (aha_ac_doc_counts_batch): document d's {key, count} pairs,
  // ascending by key, are [(*doc_pair_offsets)[d], (*doc_pair_offsets)[d + 1]) of what is returned.  A sizing call first.
  std::vector<aha_key_count> doc_counts_batch(std::string_view corpus, const std::vector<uint64_t> &doc_offsets,
                                              std::vector<uint64_t> *doc_pair_offsets = nullptr, uint64_t *n_hits = nullptr) const {
    if (doc_offsets.empty()) throw Error(AHA_E_INVALID, "doc_offsets holds D + 1 entries");
    aha_match_params p{};
    p.struct_size = sizeof(p);
    const uint64_t D = doc_offsets.size() - 1;
    const uint8_t *text = reinterpret_cast<const uint8_t *>(corpus.data());
    std::vector<uint64_t> dpo(D + 1);
    std::vector<aha_key_count> pairs;
    uint64_t n = 0, nh = 0;
    int32_t rc = aha_ac_doc_counts_batch(h_, text, doc_offsets.data(), D, &p, nullptr, 0, dpo.data(), &n, &nh);
    if (rc == AHA_E_CAPACITY) {
      pairs.resize(n);
      rc = aha_ac_doc_counts_batch(h_, text, doc_offsets.data(), D, &p, pairs.data(), pairs.size(), dpo.data(), &n, &nh);
    }
    if (rc != AHA_OK) {
      const char *m = aha_last_error(h_);
      throw Error(rc, (m && *m) ? m : aha_strerror(rc));
    }
    if (doc_pair_offsets) *doc_pair_offsets = std::move(dpo);
    if (n_hits) *n_hits = nh;
    return pairs;
  }

  // Per document the leftmost-longest, non-overlapping hits of match_batch (aha_ac_select_batch; byte offsets): document d's
  // selection, ascending by start, is [(*doc_sel_offsets)[d], (*doc_sel_offsets)[d + 1]) of what is returned.  A sizing call first.
  std::vector<Hit> select_batch(std::string_view corpus, const std::vector<uint64_t> &doc_offsets,
                                std::vector<uint64_t> *doc_sel_offsets = nullptr, uint64_t *n_hits = nullptr) const {
    return select_flags(corpus, doc_offsets, 0, doc_sel_offsets, n_hits);
  }
  std::vector<Hit> select(std::string_view seq) const { return select_batch(seq, {0, seq.size()}); }

  // Every document as a gap-free sequence of tokens (aha_ac_select_batch with AHA_SELECT_TOKENS; byte offsets): the hits of
  // select_batch with their key index as value and, between them, one token per character (gap_runs: one per gap) with value
  // -1.  Document d's tokens are [(*doc_tok_offsets)[d], (*doc_tok_offsets)[d + 1]) of what is returned.  A sizing call first.
  std::vector<Hit> tokens_batch(std::string_view corpus, const std::vector<uint64_t> &doc_offsets, bool gap_runs = false,
                                std::vector<uint64_t> *doc_tok_offsets = nullptr, uint64_t *n_hits = nullptr) const {
    return select_flags(corpus, doc_offsets, AHA_SELECT_TOKENS | (gap_runs ? AHA_SELECT_GAP_RUNS : 0u), doc_tok_offsets, n_hits);
  }
  std::vector<Hit> tokens(std::string_view seq, bool gap_runs = false) const { return tokens_batch(seq, {0, seq.size()}, gap_runs); }

  // The device-resident form (aha_ac_select_batch_device with AHA_SELECT_TOKENS): d_ pointers are memory of the handle's
  // device, d_out holds cap tokens (null with cap 0: a sizing call), d_doc_tok_offsets D + 1 entries or null.  Returns the
  // number of tokens; throws Error(AHA_E_CAPACITY) where cap is too small (*n_required = the tokens needed; nothing written).
  uint64_t tokens_batch_device(const uint8_t *d_corpus, const uint64_t *d_doc_offsets, uint64_t n_docs, uint64_t n_bytes, Hit *d_out,
                               uint64_t cap, uint64_t *d_doc_tok_offsets = nullptr, bool gap_runs = false,
                               uint64_t *n_required = nullptr, uint64_t *n_hits = nullptr, void *stream = nullptr) const {
    aha_match_params p{};
    p.struct_size = sizeof(p);
    uint64_t n = 0, nh = 0;
    const int32_t rc = aha_ac_select_batch_device(h_, d_corpus, d_doc_offsets, n_docs, n_bytes, &p,
                                                  AHA_SELECT_TOKENS | (gap_runs ? AHA_SELECT_GAP_RUNS : 0u), d_out, cap,
                                                  d_doc_tok_offsets, &n, &nh, stream);
    if (n_required) *n_required = n;
    if (rc != AHA_OK) {
      const char *m = aha_last_error(h_);
      throw Error(rc, (m && *m) ? m : aha_strerror(rc));
    }
    if (n_hits) *n_hits = nh;
    return n;
  }

 private:
  std::vector<Hit> select_flags(std::string_view corpus, const std::vector<uint64_t> &doc_offsets, uint32_t flags,
                                std::vector<uint64_t> *doc_sel_offsets, uint64_t *n_hits) const {
    if (doc_offsets.empty()) throw Error(AHA_E_INVALID, "doc_offsets holds D + 1 entries");
    aha_match_params p{};
    p.struct_size = sizeof(p);
    const uint64_t D = doc_offsets.size() - 1;
    const uint8_t *text = reinterpret_cast<const uint8_t *>(corpus.data());
    std::vector<uint64_t> dso(D + 1);
    std::vector<Hit> sel;
    uint64_t n = 0, nh = 0;
    int32_t rc = aha_ac_select_batch(h_, text, doc_offsets.data(), D, &p, flags, nullptr, 0, dso.data(), &n, &nh);
    if (rc == AHA_E_CAPACITY) {
      sel.resize(n);
      rc = aha_ac_select_batch(h_, text, doc_offsets.data(), D, &p, flags, sel.data(), sel.size(), dso.data(), &n, &nh);
    }
    if (rc != AHA_OK) {
      const char *m = aha_last_error(h_);
      throw Error(rc, (m && *m) ? m : aha_strerror(rc));
    }
    if (doc_sel_offsets) *doc_sel_offsets = std::move(dso);
    if (n_hits) *n_hits = nh;
    return sel;
  }

 public:

  // A replacement table of this handle (aha_repl_create): per key its replacement, or keep -- validated and uploaded once,
  // immutable, freed with the object (before or after the handle).
  class Replacements {
   public:
    Replacements() = default;
    ~Replacements() { aha_repl_free(t_); }
    Replacements(Replacements &&o) noexcept : t_(o.t_) { o.t_ = nullptr; }
    Replacements &operator=(Replacements &&o) noexcept {
      if (this != &o) {
        aha_repl_free(t_);
        t_ = o.t_;
        o.t_ = nullptr;
      }
      return *this;
    }
    Replacements(const Replacements &) = delete;
    Replacements &operator=(const Replacements &) = delete;
    const aha_repl *handle() const { return t_; }

   private:
    friend class AC;
    explicit Replacements(aha_repl *t) : t_(t) {}
    aha_repl *t_ = nullptr;
  };
  // repl: one entry per key (an empty string deletes the key's hits); keep[k] = true: key k's hits stay as they are
  Replacements replacements(const std::vector<std::string> &repl, const std::vector<bool> &keep = {}) const {
    const uint32_t K = n_keys();
    if (repl.size() != K || (!keep.empty() && keep.size() != K)) throw Error(AHA_E_INVALID, "one replacement per key");
    std::string blob;
    std::vector<uint64_t> offs(K + 1, 0);
    std::vector<uint32_t> bits((K + 31) / 32 + 1, 0);
    for (uint32_t k = 0; k < K; k++) {
      const bool kept = !keep.empty() && keep[k];
      if (kept)
        bits[k >> 5] |= 1u << (k & 31);
      else
        blob += repl[k];
      offs[k + 1] = blob.size();
    }
    aha_repl *t = nullptr;
    int32_t rc = aha_repl_create(h_, reinterpret_cast<const uint8_t *>(blob.data()), offs.data(), bits.data(), &t);
    if (rc != AHA_OK) {
      const char *m = aha_last_error(h_);
      throw Error(rc, (m && *m) ? m : aha_strerror(rc));
    }
    return Replacements(t);
  }
  // The batch with every selected hit (select_batch) replaced as the table says, built on the device (aha_ac_replace_batch):
  // document d's result is [(*doc_out_offsets)[d], (*doc_out_offsets)[d + 1]) of what is returned.  A sizing call first.
  std::string replace_batch(std::string_view corpus, const std::vector<uint64_t> &doc_offsets, const Replacements &table,
                            std::vector<uint64_t> *doc_out_offsets = nullptr, uint64_t *n_selected = nullptr,
                            uint64_t *n_hits = nullptr) const {
    if (doc_offsets.empty()) throw Error(AHA_E_INVALID, "doc_offsets holds D + 1 entries");
    aha_match_params p{};
    p.struct_size = sizeof(p);
    const uint64_t D = doc_offsets.size() - 1;
    const uint8_t *text = reinterpret_cast<const uint8_t *>(corpus.data());
    std::vector<uint64_t> doo(D + 1);
    std::string out;
    uint64_t n = 0, ns = 0, nh = 0;
    int32_t rc = aha_ac_replace_batch(h_, table.handle(), text, doc_offsets.data(), D, &p, 0, nullptr, 0, doo.data(), &n, &ns, &nh);
    if (rc == AHA_E_CAPACITY) {
      out.resize(n);
      rc = aha_ac_replace_batch(h_, table.handle(), text, doc_offsets.data(), D, &p, 0, reinterpret_cast<uint8_t *>(&out[0]),
                                out.size(), doo.data(), &n, &ns, &nh);
    }
    if (rc != AHA_OK) {
      const char *m = aha_last_error(h_);
      throw Error(rc, (m && *m) ? m : aha_strerror(rc));
    }
    if (doc_out_offsets) *doc_out_offsets = std::move(doo);
    if (n_selected) *n_selected = ns;
    if (n_hits) *n_hits = nh;
    return out;
  }

  // The batch split into records at `delim` and at the documents' ends, on the device (aha_ac_records_batch): what is returned
  // holds R + 1 offsets, 0 first; a record ends behind a delimiter or at a document's end and is never empty; it is a
  // doc_offsets for every batch call.  doc_rec_offsets (optional): D + 1 offsets into the records.  A sizing call first.
  std::vector<uint64_t> records_batch(std::string_view corpus, const std::vector<uint64_t> &doc_offsets, char delim = '\n',
                                      std::vector<uint64_t> *doc_rec_offsets = nullptr) const {
    if (doc_offsets.empty()) throw Error(AHA_E_INVALID, "doc_offsets holds D + 1 entries");
    const uint64_t D = doc_offsets.size() - 1;
    const uint8_t *text = reinterpret_cast<const uint8_t *>(corpus.data());
    const uint8_t dl = static_cast<uint8_t>(delim);
    std::vector<uint64_t> dro(D + 1);
    uint64_t n = 0;
    int32_t rc = aha_ac_records_batch(h_, text, doc_offsets.data(), D, dl, 0, nullptr, 0, nullptr, &n);
    std::vector<uint64_t> rec(n + 1, 0);
    if (rc == AHA_E_CAPACITY || rc == AHA_OK) rc = aha_ac_records_batch(h_, text, doc_offsets.data(), D, dl, 0, rec.data(), n, dro.data(), &n);
    if (rc != AHA_OK) {
      const char *m = aha_last_error(h_);
      throw Error(rc, (m && *m) ? m : aha_strerror(rc));
    }
    if (doc_rec_offsets) *doc_rec_offsets = std::move(dro);
    return rec;
  }
  std::vector<uint64_t> records(std::string_view seq, char delim = '\n') const { return records_batch(seq, {0, seq.size()}, delim); }
  // The documents with at least one hit of match_batch -- invert: those without one -- compacted on the device
  // (aha_ac_grep_batch): their bytes one behind the other; kept_docs (optional): their indices, ascending; doc_out_offsets
  // (optional): n_kept + 1 offsets into what is returned.  A sizing call first.
  std::string grep_batch(std::string_view corpus, const std::vector<uint64_t> &doc_offsets, bool invert = false,
                         std::vector<uint64_t> *kept_docs = nullptr, std::vector<uint64_t> *doc_out_offsets = nullptr,
                         uint64_t *n_hits = nullptr) const {
    if (doc_offsets.empty()) throw Error(AHA_E_INVALID, "doc_offsets holds D + 1 entries");
    aha_match_params p{};
    p.struct_size = sizeof(p);
    const uint64_t D = doc_offsets.size() - 1;
    const uint8_t *text = reinterpret_cast<const uint8_t *>(corpus.data());
    const uint32_t flags = invert ? AHA_GREP_INVERT : 0u;
    uint64_t nk = 0, nb = 0, nh = 0;
    int32_t rc = aha_ac_grep_batch(h_, text, doc_offsets.data(), D, &p, flags, nullptr, nullptr, 0, nullptr, 0, &nk, &nb, &nh);
    std::vector<uint64_t> kept(nk + 1), doo(nk + 1);
    std::string out(nb, '\0');
    if (rc == AHA_OK)
      rc = aha_ac_grep_batch(h_, text, doc_offsets.data(), D, &p, flags, kept.data(), doo.data(), nk,
                             nb ? reinterpret_cast<uint8_t *>(&out[0]) : nullptr, nb, &nk, &nb, &nh);
    if (rc != AHA_OK) {
      const char *m = aha_last_error(h_);
      throw Error(rc, (m && *m) ? m : aha_strerror(rc));
    }
    kept.resize(nk);
    if (kept_docs) *kept_docs = std::move(kept);
    if (doc_out_offsets) *doc_out_offsets = std::move(doo);
    if (n_hits) *n_hits = nh;
    return out;
  }
  // The records of seq (split at delim, each with its delimiter) that have a hit; invert: those that have none.
  std::vector<std::string> grep(std::string_view seq, char delim = '\n', bool invert = false) const {
    const std::vector<uint64_t> rec = records(seq, delim);
    std::vector<uint64_t> doo;
    const std::string out = grep_batch(seq, rec, invert, nullptr, &doo);
    std::vector<std::string> lines;
    for (size_t i = 0; i + 1 < doo.size(); i++) lines.push_back(out.substr(doo[i], doo[i + 1] - doo[i]));
    return lines;
  }

  // A class table of this handle (aha_classes_create): per key its classes -- none, one or several of n_classes --, validated
  // and uploaded once, immutable, freed with the object (before or after the handle).
  class Classes {
   public:
    Classes() = default;
    ~Classes() { aha_classes_free(t_); }
    Classes(Classes &&o) noexcept : t_(o.t_), n_(o.n_) { o.t_ = nullptr; }
    Classes &operator=(Classes &&o) noexcept {
      if (this != &o) {
        aha_classes_free(t_);
        t_ = o.t_;
        n_ = o.n_;
        o.t_ = nullptr;
      }
      return *this;
    }
    Classes(const Classes &) = delete;
    Classes &operator=(const Classes &) = delete;
    const aha_classes *handle() const { return t_; }
    uint32_t n_classes() const { return n_; }

   private:
    friend class AC;
    Classes(aha_classes *t, uint32_t n) : t_(t), n_(n) {}
    aha_classes *t_ = nullptr;
    uint32_t n_ = 0;
  };
  // per_key: one entry per key, the key's class ids in ascending order (empty: the key counts nowhere)
  Classes classes(const std::vector<std::vector<uint32_t>> &per_key, uint32_t n_classes) const {
    const uint32_t K = n_keys();
    if (per_key.size() != K) throw Error(AHA_E_INVALID, "one class list per key");
    std::vector<uint32_t> ids;
    std::vector<uint64_t> offs(K + 1, 0);
    for (uint32_t k = 0; k < K; k++) {
      ids.insert(ids.end(), per_key[k].begin(), per_key[k].end());
      offs[k + 1] = ids.size();
    }
    aha_classes *t = nullptr;
    int32_t rc = aha_classes_create(h_, ids.data(), offs.data(), n_classes, &t);
    if (rc != AHA_OK) {
      const char *m = aha_last_error(h_);
      throw Error(rc, (m && *m) ? m : aha_strerror(rc));
    }
    return Classes(t, n_classes);
  }
  // The hits of match_batch counted per document and key class, on the device (aha_ac_class_counts_batch): D x C entries,
  // row-major; entry d * C + c = the hits of document d whose key is in class c (a key in several classes counts in each).
  // No hit list, no pairs, no capacity: the size is known before the call.  (A batch that already lives in HBM goes through the
  // C ABI's aha_ac_class_counts_batch_device, which writes the table in place on the caller's stream.)
  //   auto m = aha::AC::compile({"he", "she", "hers"});
  //   auto t = m.classes({{0}, {0, 1}, {}}, 2);                        // he: class 0; she: classes 0 and 1; hers: none
  //   m.class_counts_batch("ushershe", {0, 6, 8}, t)                   // "ushers": she, he, hers; "he": he
  //     == std::vector<uint32_t>{2, 1, 1, 0};
  std::vector<uint32_t> class_counts_batch(std::string_view corpus, const std::vector<uint64_t> &doc_offsets, const Classes &table,
                                           uint64_t *n_hits = nullptr) const {
    if (doc_offsets.empty()) throw Error(AHA_E_INVALID, "doc_offsets holds D + 1 entries");
    aha_match_params p{};
    p.struct_size = sizeof(p);
    const uint64_t D = doc_offsets.size() - 1;
    std::vector<uint32_t> out(D * table.n_classes());
    uint64_t nh = 0;
    int32_t rc = aha_ac_class_counts_batch(h_, table.handle(), reinterpret_cast<const uint8_t *>(corpus.data()), doc_offsets.data(), D,
                                           &p, 0, out.data(), &nh);
    if (rc != AHA_OK) {
      const char *m = aha_last_error(h_);
      throw Error(rc, (m && *m) ? m : aha_strerror(rc));
    }
    if (n_hits) *n_hits = nh;
    return out;
  }
  std::vector<uint32_t> class_counts(std::string_view seq, const Classes &table) const {
    return class_counts_batch(seq, {0, seq.size()}, table);
  }

  // Rule grep (aha_ac_grep_batch with AHA_GREP_RULE): the documents whose class counts pass a rule -- invert: those that do not
  // -- compacted on the device as grep_batch compacts them.  A rule is 1 to 64 terms (aha_rule_term): count[class_id] OP num, or
  // with den_bytes > 0 "num hits per den_bytes bytes of the document"; OP is AHA_RULE_GE or AHA_RULE_LT; a document passes when
  // some group has all its terms true.  rows (optional): the D x C table as class_counts_batch returns it.
  //   auto m = aha::AC::compile({"he", "she", "hers"});
  //   auto t = m.classes({{0}, {0, 1}, {}}, 2);
  //   m.grep_rule_batch("ushershe", {0, 6, 8}, t, {AC::term(0, AHA_RULE_GE, 2)})                                == "ushers"
  //   m.grep_rule_batch("ushershe", {0, 6, 8}, t, {AC::term(0, AHA_RULE_GE, 1), AC::term(1, AHA_RULE_LT, 1)})   == "he"
  //   m.grep_rule_batch("ushershe", {0, 6, 8}, t, {AC::term(0, AHA_RULE_GE, 1, 3)})                             == "ushershe"
  static aha_rule_term term(uint32_t class_id, uint32_t op, uint32_t num, uint32_t den_bytes = 0, uint16_t group = 0) {
    aha_rule_term t{};
    t.class_id = class_id;
    t.op = (uint16_t)op;
    t.group = group;
    t.num = num;
    t.den_bytes = den_bytes;
    return t;
  }
  std::string grep_rule_batch(std::string_view corpus, const std::vector<uint64_t> &doc_offsets, const Classes &table,
                              const std::vector<aha_rule_term> &terms, bool invert = false, std::vector<uint64_t> *kept_docs = nullptr,
                              std::vector<uint64_t> *doc_out_offsets = nullptr, std::vector<uint32_t> *rows = nullptr,
                              uint64_t *n_hits = nullptr) const {
    if (doc_offsets.empty()) throw Error(AHA_E_INVALID, "doc_offsets holds D + 1 entries");
    aha_grep_params gp{};
    gp.match.struct_size = sizeof(gp);
    gp.classes = table.handle();
    gp.terms = terms.data();
    gp.n_terms = (uint32_t)terms.size();
    const uint64_t D = doc_offsets.size() - 1;
    const uint8_t *text = reinterpret_cast<const uint8_t *>(corpus.data());
    const uint32_t flags = AHA_GREP_RULE | (invert ? AHA_GREP_INVERT : 0u);
    uint64_t nk = 0, nb = 0, nh = 0;
    int32_t rc = aha_ac_grep_batch(h_, text, doc_offsets.data(), D, &gp.match, flags, nullptr, nullptr, 0, nullptr, 0, &nk, &nb, &nh);
    std::vector<uint64_t> kept(nk + 1), doo(nk + 1);
    std::vector<uint32_t> table_rows(rows ? D * table.n_classes() : 0);
    std::string out(nb, '\0');
    if (rc == AHA_OK) {
      gp.rows = table_rows.empty() ? nullptr : table_rows.data();
      rc = aha_ac_grep_batch(h_, text, doc_offsets.data(), D, &gp.match, flags, kept.data(), doo.data(), nk,
                             nb ? reinterpret_cast<uint8_t *>(&out[0]) : nullptr, nb, &nk, &nb, &nh);
    }
    if (rc != AHA_OK) {
      const char *m = aha_last_error(h_);
      throw Error(rc, (m && *m) ? m : aha_strerror(rc));
    }
    kept.resize(nk);
    if (kept_docs) *kept_docs = std::move(kept);
    if (doc_out_offsets) *doc_out_offsets = std::move(doo);
    if (rows) *rows = std::move(table_rows);
    if (n_hits) *n_hits = nh;
    return out;
  }

  // Excerpts (aha_ac_grep_batch with AHA_GREP_CONTEXT): the hits of match_batch in their context -- `before` bytes in front of
  // every hit and `after` behind it, clipped to the document, snapped outwards to UTF-8 character boundaries, neighbouring
  // contexts of one document merged -- cut out on the device.  Excerpt r starts at corpus byte starts[r]; its bytes are
  // out.substr(out_offsets[r], out_offsets[r + 1] - out_offsets[r]).
  //   auto m = aha::AC::compile({"ab"});
  //   auto e = m.excerpts_batch("xxabxxxxabxab", {0, 11, 13}, 1, 2);   // starts {1, 7, 11}, out "xabxxxabxab", n_hits 3
  //   m.excerpts_batch("xxabxxxxabxab", {0, 11, 13}, 1, 3).starts      == {1, 11}
  struct Excerpts {
    std::vector<uint64_t> starts;       // R
    std::vector<uint64_t> out_offsets;  // R + 1
    std::string out;
    uint64_t n_hits = 0;
    std::string_view operator[](size_t r) const {
      return std::string_view(out).substr(out_offsets[r], out_offsets[r + 1] - out_offsets[r]);
    }
    size_t size() const { return starts.size(); }
  };
  static aha_excerpt_params excerpt_params(uint32_t before, uint32_t after) {
    aha_excerpt_params ep{};
    ep.match.struct_size = sizeof(ep);
    ep.before = before;
    ep.after = after;
    return ep;
  }
  Excerpts excerpts_batch(std::string_view corpus, const std::vector<uint64_t> &doc_offsets, uint32_t before, uint32_t after) const {
    if (doc_offsets.empty()) throw Error(AHA_E_INVALID, "doc_offsets holds D + 1 entries");
    const aha_excerpt_params ep = excerpt_params(before, after);
    const uint64_t D = doc_offsets.size() - 1;
    const uint8_t *text = reinterpret_cast<const uint8_t *>(corpus.data());
    uint64_t nk = 0, nb = 0, nh = 0;
    int32_t rc = aha_ac_grep_batch(h_, text, doc_offsets.data(), D, &ep.match, AHA_GREP_CONTEXT, nullptr, nullptr, 0, nullptr, 0, &nk,
                                   &nb, &nh);
    Excerpts e;
    e.starts.resize(nk + 1);
    e.out_offsets.resize(nk + 1);
    e.out.assign(nb, '\0');
    if (rc == AHA_OK)
      rc = aha_ac_grep_batch(h_, text, doc_offsets.data(), D, &ep.match, AHA_GREP_CONTEXT, e.starts.data(), e.out_offsets.data(), nk,
                             nb ? reinterpret_cast<uint8_t *>(&e.out[0]) : nullptr, nb, &nk, &nb, &nh);
    if (rc != AHA_OK) {
      const char *m = aha_last_error(h_);
      throw Error(rc, (m && *m) ? m : aha_strerror(rc));
    }
    e.starts.resize(nk);
    e.n_hits = nh;
    return e;
  }
  // The device-resident form over HBM pointers of the handle's device (d_starts [cap], d_out_offsets [cap + 1], d_out
  // [cap_bytes]; any may be null): R, the bytes and the hits come back; AHA_E_CAPACITY throws with nothing written (*n_required
  // and *bytes_required, where given, hold the two required numbers either way).
  uint64_t excerpts_batch_device(const uint8_t *d_corpus, const uint64_t *d_doc_offsets, uint64_t n_docs, uint64_t n_bytes,
                                 uint32_t before, uint32_t after, uint64_t *d_starts, uint64_t *d_out_offsets, uint64_t cap,
                                 uint8_t *d_out, uint64_t cap_bytes, uint64_t *n_out_bytes = nullptr, uint64_t *n_hits = nullptr,
                                 void *stream = nullptr, uint64_t *n_required = nullptr) const {
    const aha_excerpt_params ep = excerpt_params(before, after);
    uint64_t nk = 0, nb = 0, nh = 0;
    const int32_t rc = aha_ac_grep_batch_device(h_, d_corpus, d_doc_offsets, n_docs, n_bytes, &ep.match, AHA_GREP_CONTEXT, d_starts,
                                                d_out_offsets, cap, d_out, cap_bytes, &nk, &nb, &nh, stream);
    if (n_required) *n_required = nk;
    if (n_out_bytes) *n_out_bytes = nb;
    if (n_hits) *n_hits = nh;
    if (rc != AHA_OK) {
      const char *m = aha_last_error(h_);
      throw Error(rc, (m && *m) ? m : aha_strerror(rc));
    }
    return nk;
  }

  // Context lines (aha_ac_grep_batch with AHA_GREP_LINES): grep -B, -A and -C over the documents (records) of a batch.  A
  // document is kept when it has a hit (invert: when it has none) or lies at most `before` documents in front of / `after`
  // behind such a document of its group; groups (G + 1 offsets into the documents, such as the doc_rec_offsets of records();
  // empty: one group) bound the context, so it never crosses a file.
  //   auto m = aha::AC::compile({"ab"});
  //   aha::AC::LinesOptions o;
  //   o.before = 1;
  //   auto l = m.grep_lines_batch("x\nab\ny\nz\nab\nw\n", {0, 2, 5, 7, 9, 12, 14}, o);
  //   // l.kept_docs {0, 1, 3, 4}, l.is_match {0, 1, 0, 1}, l.out "x\nab\nz\nab\n"
  struct LinesOptions {
    uint32_t before = 0, after = 0;
    bool invert = false;
    std::vector<uint64_t> groups;  // empty: the whole batch is one group
  };
  struct Lines {
    std::vector<uint64_t> kept_docs;        // n_kept, ascending
    std::vector<uint64_t> doc_out_offsets;  // n_kept + 1
    std::vector<uint8_t> is_match;          // n_kept: 1 where the kept document matched, 0 where it is context
    std::string out;
    uint64_t n_hits = 0;
    std::string_view operator[](size_t i) const {
      return std::string_view(out).substr(doc_out_offsets[i], doc_out_offsets[i + 1] - doc_out_offsets[i]);
    }
    size_t size() const { return kept_docs.size(); }
  };
  static aha_grep_lines_params grep_lines_params(uint32_t before, uint32_t after, const uint64_t *group_offsets, uint64_t n_groups,
                                                 uint8_t *is_match) {
    aha_grep_lines_params lp{};
    lp.match.struct_size = sizeof(lp);
    lp.before = before;
    lp.after = after;
    lp.group_offsets = n_groups ? group_offsets : nullptr;
    lp.n_groups = n_groups;
    lp.is_match = is_match;
    return lp;
  }
  Lines grep_lines_batch(std::string_view corpus, const std::vector<uint64_t> &doc_offsets, const LinesOptions &opt) const {
    if (doc_offsets.empty()) throw Error(AHA_E_INVALID, "doc_offsets holds D + 1 entries");
    const uint64_t D = doc_offsets.size() - 1, G = opt.groups.empty() ? 0 : opt.groups.size() - 1;
    aha_grep_lines_params lp = grep_lines_params(opt.before, opt.after, opt.groups.data(), G, nullptr);
    const uint32_t flags = AHA_GREP_LINES | (opt.invert ? AHA_GREP_INVERT : 0u);
    const uint8_t *text = reinterpret_cast<const uint8_t *>(corpus.data());
    uint64_t nk = 0, nb = 0, nh = 0;
    int32_t rc = aha_ac_grep_batch(h_, text, doc_offsets.data(), D, &lp.match, flags, nullptr, nullptr, 0, nullptr, 0, &nk, &nb, &nh);
    Lines l;
    l.kept_docs.resize(nk + 1);
    l.doc_out_offsets.resize(nk + 1);
    l.is_match.resize(nk + 1);
    l.out.assign(nb, '\0');
    if (rc == AHA_OK) {
      lp.is_match = nk ? l.is_match.data() : nullptr;
      rc = aha_ac_grep_batch(h_, text, doc_offsets.data(), D, &lp.match, flags, l.kept_docs.data(), l.doc_out_offsets.data(), nk,
                             nb ? reinterpret_cast<uint8_t *>(&l.out[0]) : nullptr, nb, &nk, &nb, &nh);
    }
    if (rc != AHA_OK) {
      const char *m = aha_last_error(h_);
      throw Error(rc, (m && *m) ? m : aha_strerror(rc));
    }
    l.kept_docs.resize(nk);
    l.is_match.resize(nk);
    l.n_hits = nh;
    return l;
  }
  // The device-resident form over HBM pointers of the handle's device (d_kept_docs [cap_docs], d_doc_out_offsets [cap_docs + 1],
  // d_is_match [cap_docs], d_out [cap_bytes]; any may be null; d_group_offsets [n_groups + 1] or null): n_kept, the bytes and the
  // hits come back; AHA_E_CAPACITY throws with nothing written (*n_required and *n_out_bytes, where given, hold the two required
  // numbers either way).  opt.groups is not looked at.
  uint64_t grep_lines_batch_device(const uint8_t *d_corpus, const uint64_t *d_doc_offsets, uint64_t n_docs, uint64_t n_bytes,
                                   const LinesOptions &opt, const uint64_t *d_group_offsets, uint64_t n_groups, uint64_t *d_kept_docs,
                                   uint64_t *d_doc_out_offsets, uint8_t *d_is_match, uint64_t cap_docs, uint8_t *d_out,
                                   uint64_t cap_bytes, uint64_t *n_out_bytes = nullptr, uint64_t *n_hits = nullptr,
                                   void *stream = nullptr, uint64_t *n_required = nullptr) const {
    const aha_grep_lines_params lp = grep_lines_params(opt.before, opt.after, d_group_offsets, n_groups, d_is_match);
    const uint32_t flags = AHA_GREP_LINES | (opt.invert ? AHA_GREP_INVERT : 0u);
    uint64_t nk = 0, nb = 0, nh = 0;
    const int32_t rc = aha_ac_grep_batch_device(h_, d_corpus, d_doc_offsets, n_docs, n_bytes, &lp.match, flags, d_kept_docs,
                                                d_doc_out_offsets, cap_docs, d_out, cap_bytes, &nk, &nb, &nh, stream);
    if (n_required) *n_required = nk;
    if (n_out_bytes) *n_out_bytes = nb;
    if (n_hits) *n_hits = nh;
    if (rc != AHA_OK) {
      const char *m = aha_last_error(h_);
      throw Error(rc, (m && *m) ? m : aha_strerror(rc));
    }
    return nk;
  }

  // Which bytes of the batch lie inside a hit of match_batch, without the hit list (aha_ac_cover_batch): bit j of the batch is
  // word j >> 5, bit j & 31 of what is returned; doc_covered (optional): covered bytes per document.
  std::vector<uint32_t> cover_batch(std::string_view corpus, const std::vector<uint64_t> &doc_offsets,
                                    std::vector<uint64_t> *doc_covered = nullptr, uint64_t *n_hits = nullptr) const {
    std::vector<uint32_t> mask;
    cover_call(corpus, doc_offsets, &mask, nullptr, 0, doc_covered, n_hits);
    return mask;
  }
  // The batch with every byte inside a hit replaced by `fill`.
  std::string redact_batch(std::string_view corpus, const std::vector<uint64_t> &doc_offsets, char fill = '*',
                           std::vector<uint64_t> *doc_covered = nullptr) const {
    std::string red;
    cover_call(corpus, doc_offsets, nullptr, &red, static_cast<uint8_t>(fill), doc_covered, nullptr);
    return red;
  }
  std::string redact(std::string_view seq, char fill = '*') const { return redact_batch(seq, {0, seq.size()}, fill); }

  // The same on a batch resident in HBM (aha_ac_count_batch_device): d_key_counts is device memory of K uint64 (or null) and
  // keeps running totals there with accumulate; returns the hit count.
  uint64_t count_resident(const Corpus &c, uint64_t *d_key_counts, bool accumulate = false,
                          std::vector<uint64_t> *doc_hit_offsets = nullptr) const {
    const aha_corpus *h = c.handle();
    const int dev = aha_corpus_device(h);
    const uint64_t D = aha_corpus_n_docs(h);
    aha_match_params p{};
    p.struct_size = sizeof(p);
    void *d_dho = nullptr;
    int32_t rc = AHA_OK;
    if (doc_hit_offsets && (rc = aha_buffer_alloc(dev, (D + 1) * sizeof(uint64_t), &d_dho)) != AHA_OK)
      throw Error(rc, aha_last_error(nullptr));
    uint64_t n = 0;
    rc = aha_ac_count_batch_device(h_, aha_corpus_bytes(h), aha_corpus_doc_offsets(h), D, aha_corpus_n_bytes(h), &p,
                                   accumulate ? AHA_COUNT_ACCUMULATE : 0u, d_key_counts, static_cast<uint64_t *>(d_dho), &n,
                                   nullptr);
    if (rc == AHA_OK && doc_hit_offsets) {
      doc_hit_offsets->resize(D + 1);
      rc = aha_buffer_download(dev, doc_hit_offsets->data(), d_dho, (D + 1) * sizeof(uint64_t));
    }
    if (d_dho) aha_buffer_free(dev, d_dho);
    if (rc != AHA_OK) {
      const char *m = aha_last_error(h_);
      throw Error(rc, (m && *m) ? m : aha_strerror(rc));
    }
    return n;
  }

  // AC#[](sid : Int) : String ;  AC#[](key) : Int (IndexError when absent)
  std::string operator[](int32_t id) const {
    int32_t n = aha_ac_key(h_, id, nullptr, 0);
    if (n < 0) throw Error(n, "Index out of bounds");
    std::string s((size_t)n, '\0');
    aha_ac_key(h_, id, reinterpret_cast<uint8_t *>(&s[0]), n);
    return s;
  }
  int32_t operator[](std::string_view key) const {
    int32_t r = aha_ac_id(h_, reinterpret_cast<const uint8_t *>(key.data()), (int32_t)key.size());
    if (r < 0) throw Error(r, "Index out of bounds");
    return r;
  }
  // AC#save / AC.load (src/aha/ac.cr:45-60): the library's own container, see aha_hip.h
  std::vector<uint8_t> to_bytes() const {
    int64_t n = aha_ac_save(h_, nullptr, 0);
    if (n < 0) throw Error((int32_t)n, aha_strerror((int32_t)n));
    std::vector<uint8_t> v((size_t)n);
    aha_ac_save(h_, v.data(), (uint64_t)n);
    return v;
  }
  // (the container stores the keys as spelled and no options: say fold_ascii / fold_simple / fold_bmp / fold_kana again)
  static AC from_bytes(const std::vector<uint8_t> &data, int device = -1, bool fold_ascii = false, bool fold_simple = false,
                       bool fold_bmp = false, bool fold_kana = false) {
    aha_options o{};
    o.struct_size = sizeof(o);
    o.device = device;
    o.flags = (fold_ascii ? AHA_OPT_FOLD_ASCII : 0u) | (fold_simple ? AHA_OPT_FOLD_SIMPLE : 0u) | (fold_bmp ? AHA_OPT_FOLD_BMP : 0u) |
              (fold_kana ? AHA_OPT_FOLD_KANA : 0u);
    aha_ac *h = nullptr;
    int32_t rc = aha_ac_load(data.data(), data.size(), &o, &h);
    if (rc != AHA_OK) throw Error(rc, aha_strerror(rc));
    return AC(h);
  }
  bool fold_ascii() const { return (aha_ac_flags(h_) & AHA_OPT_FOLD_ASCII) != 0; }
  bool fold_simple() const { return (aha_ac_flags(h_) & AHA_OPT_FOLD_SIMPLE) != 0; }
  bool fold_bmp() const { return (aha_ac_flags(h_) & AHA_OPT_FOLD_BMP) != 0; }
  bool fold_kana() const { return (aha_ac_flags(h_) & AHA_OPT_FOLD_KANA) != 0; }
  aha_ac *handle() const { return h_; }

 private:
  explicit AC(aha_ac *h) : h_(h) {}
  template <class F>
  void run(std::string_view seq, const BitArray *sep, bool chars, F &&block, int longest = 0) const {
    aha_match_params p{};
    p.struct_size = sizeof(p);
    p.char_offsets = chars ? 1 : 0;
    p.longest = longest;
    if (sep) {
      p.sep_size = sep->size();
      std::memcpy(p.sep_bits, sep->bytes().data(), sep->bytes().size() < 32 ? sep->bytes().size() : 32);
    }
    std::vector<Hit> out(seq.size() / 4 + 64);
    uint64_t n = 0;
    for (;;) {
      int32_t rc = aha_ac_match_bytes(h_, reinterpret_cast<const uint8_t *>(seq.data()), seq.size(), &p,
                                      out.data(), out.size(), &n);
      if (rc == AHA_E_CAPACITY) {
        out.resize(n);
        continue;
      }
      if (rc != AHA_OK) {
        const char *m = aha_last_error(h_);
        throw Error(rc, (m && *m) ? m : aha_strerror(rc));
      }
      break;
    }
    for (uint64_t i = 0; i < n; i++) block(out[i]);
  }
  aha_ac *h_;
};

// Aha::ACBig = ACX(Int64) (src/aha/ac.cr:9): wider node ids, the same Hit with an Int32 value (ac.cr:273)
using ACBig = AC;

// Sequences that arrive in pieces across calls (aha_feed_*): a call matches a batch of pieces, piece d the next part of
// sequence seq_ids[d], and gives exactly the hits one match over the whole sequence so far reports with an end inside the
// piece.  Offsets are relative to the piece (start may be negative); bases[d] is the sequence's length before it.  Free the
// feed before its AC.
class Feed {
 public:
  // fold: on an AC compiled with a fold beyond ASCII (simple, BMP, kana) a FOLDED feed (kFeedFold = AHA_FEED_FOLD) -- every call
  // answers as if the sequence ended with its piece: a character cut between two calls is folded whole, one still open at a call's
  // end is matched unfolded; match, count and cover calls (select, replace and grep calls throw).  Without it such an AC has no
  // feeds; on any other AC it changes nothing
  static constexpr uint32_t kFeedFold = AHA_FEED_FOLD;
  Feed(const AC &ac, uint32_t n_seqs, bool chars = false, bool fold = false) : ac_(ac.handle()) {
    const int32_t rc = aha_feed_open(ac_, n_seqs, (chars ? AHA_FEED_CHARS : 0u) | (fold ? kFeedFold : 0u), &f_);
    if (rc != AHA_OK) {
      const char *m = aha_last_error(ac_);
      throw Error(rc, (m && *m) ? m : aha_strerror(rc));
    }
  }
  // a feed whose match and count calls apply the separator filter of match(seq, sep) to the whole sequence
  // (aha_feed_open_params): a call reports the surviving hits that end before the piece's last byte -- one that ended with the
  // piece before has end == 0 --, finish_batch / finish those that end with the sequence; cover and select calls throw
  Feed(const AC &ac, uint32_t n_seqs, const BitArray &sep) : ac_(ac.handle()) {
    aha_match_params p{};
    p.struct_size = sizeof(p);
    p.sep_size = sep.size();
    std::memcpy(p.sep_bits, sep.bytes().data(), sep.bytes().size() < 32 ? sep.bytes().size() : 32);
    const int32_t rc = aha_feed_open_params(ac_, n_seqs, 0u, &p, &f_);
    if (rc != AHA_OK) {
      const char *m = aha_last_error(ac_);
      throw Error(rc, (m && *m) ? m : aha_strerror(rc));
    }
  }
  // a longest feed (aha_feed_open_params with longest = 1 | 2), the mirror of AC#match_longest(seq, intersectable) for a sequence
  // in pieces: a call that takes a sequence from n0 to n1 bytes gives the hits of match_longest(whole sequence) that are yielded
  // at a byte in [n0, n1) -- a hit may lie wholly in earlier pieces --, finish_batch / finish the one hit still pending, and the
  // sequence starts again.  Byte offsets; count, cover, select, replace and grep calls throw
  static Feed match_longest(const AC &ac, uint32_t n_seqs, bool intersectable = false) {
    aha_match_params p{};
    p.struct_size = sizeof(p);
    p.longest = intersectable ? 2 : 1;
    return Feed(ac, n_seqs, p);
  }
  Feed(const Feed &) = delete;
  Feed &operator=(const Feed &) = delete;
  Feed(Feed &&o) noexcept : ac_(o.ac_), f_(o.f_), grep_held_(std::move(o.grep_held_)) { o.f_ = nullptr; }
  ~Feed() { aha_feed_free(f_); }

  // host buffers: the hits of the call; piece_hit_offsets (D+1) and bases (D) when asked for
  std::vector<Hit> match_batch(std::string_view corpus, const std::vector<uint64_t> &piece_offsets,
                               const std::vector<uint32_t> &seq_ids, std::vector<uint64_t> *piece_hit_offsets = nullptr,
                               std::vector<uint64_t> *bases = nullptr) {
    const uint64_t D = piece_offsets.empty() ? 0 : piece_offsets.size() - 1;
    if (seq_ids.size() != D) throw Error(AHA_E_INVALID, "one sequence id per piece");
    if (piece_hit_offsets) piece_hit_offsets->assign(D + 1, 0);
    if (bases) bases->assign(D, 0);
    std::vector<Hit> out(corpus.size() / 8 + 64);
    uint64_t n = 0;
    for (;;) {
      const int32_t rc = aha_feed_match_batch(f_, reinterpret_cast<const uint8_t *>(corpus.data()), piece_offsets.data(),
                                              seq_ids.data(), D, out.data(), out.size(),
                                              piece_hit_offsets ? piece_hit_offsets->data() : nullptr,
                                              bases ? bases->data() : nullptr, &n);
      if (rc == AHA_E_CAPACITY) {  // (the feed is unchanged: the same call again)
        out.resize(n);
        continue;
      }
      check(rc);
      break;
    }
    out.resize(n);
    return out;
  }
  // the next piece of one sequence: its hits with absolute offsets (they must fit Int32)
  std::vector<Hit> match(uint32_t seq, std::string_view piece) {
    std::vector<uint64_t> bases;
    auto hits = match_batch(piece, {0, piece.size()}, {seq}, nullptr, &bases);
    for (auto &h : hits) {
      h.start += (int32_t)bases[0];
      h.end += (int32_t)bases[0];
    }
    return hits;
  }
  // a feed with a separator filter: the named sequences end here (aha_feed_finish_batch).  The surviving hits that end with
  // them, relative to each sequence's end (end == 0, start == -len); seq_hit_offsets (n + 1) and bases (n: the sequences'
  // lengths) when asked for.  The sequences start again at length 0.  A longest feed: the one hit of each sequence that is
  // still pending (end <= 0).
  std::vector<Hit> finish_batch(const std::vector<uint32_t> &seq_ids, std::vector<uint64_t> *seq_hit_offsets = nullptr,
                                std::vector<uint64_t> *bases = nullptr) {
    const uint64_t D = seq_ids.size();
    if (seq_hit_offsets) seq_hit_offsets->assign(D + 1, 0);
    if (bases) bases->assign(D, 0);
    std::vector<Hit> out(4 * D + 16);
    uint64_t n = 0;
    for (;;) {
      const int32_t rc = aha_feed_finish_batch(f_, seq_ids.data(), D, out.data(), out.size(),
                                               seq_hit_offsets ? seq_hit_offsets->data() : nullptr,
                                               bases ? bases->data() : nullptr, &n);
      if (rc == AHA_E_CAPACITY) {  // (the sequences have not restarted: the same call again)
        out.resize(n);
        continue;
      }
      check(rc);
      break;
    }
    out.resize(n);
    return out;
  }
  // one sequence ends here: the surviving hits that end with it, with absolute offsets (they must fit Int32)
  std::vector<Hit> finish(uint32_t seq) {
    std::vector<uint64_t> bases;
    auto hits = finish_batch({seq}, nullptr, &bases);
    for (auto &h : hits) {
      h.start += (int32_t)bases[0];
      h.end += (int32_t)bases[0];
    }
    return hits;
  }
  // hits per key of match_batch on the same pieces without the hit list (aha_feed_count_batch); the sequences move on as a
  // match call would move them.  accumulate: add into *key_counts (which then must hold K entries) instead of overwriting
  // it; a call that throws leaves it as it was.  Returns the hit count.
  uint64_t count_batch(std::string_view corpus, const std::vector<uint64_t> &piece_offsets, const std::vector<uint32_t> &seq_ids,
                       std::vector<uint64_t> *key_counts, std::vector<uint64_t> *piece_hit_offsets = nullptr,
                       std::vector<uint64_t> *bases = nullptr, bool accumulate = false) {
    const uint64_t D = piece_offsets.empty() ? 0 : piece_offsets.size() - 1;
    if (piece_offsets.empty()) throw Error(AHA_E_INVALID, "piece_offsets holds D + 1 entries");
    if (seq_ids.size() != D) throw Error(AHA_E_INVALID, "one sequence id per piece");
    std::vector<uint64_t> kc, pho(D + 1), b(D);
    if (key_counts) {
      aha_ac_info_t i{};
      i.struct_size = sizeof(i);
      check(aha_ac_info(ac_, &i));
      if (accumulate && key_counts->size() != i.n_keys) throw Error(AHA_E_INVALID, "key_counts holds K entries");
      kc = accumulate ? *key_counts : std::vector<uint64_t>(i.n_keys, 0);
    }
    uint64_t n = 0;
    check(aha_feed_count_batch(f_, reinterpret_cast<const uint8_t *>(corpus.data()), piece_offsets.data(), seq_ids.data(), D,
                               accumulate ? AHA_COUNT_ACCUMULATE : 0u, key_counts ? kc.data() : nullptr, pho.data(), b.data(),
                               &n));
    if (key_counts) *key_counts = std::move(kc);
    if (piece_hit_offsets) *piece_hit_offsets = std::move(pho);
    if (bases) *bases = std::move(b);
    return n;
  }
  // the next piece of one sequence: its hits per key (K entries)
  std::vector<uint64_t> count(uint32_t seq, std::string_view piece) {
    std::vector<uint64_t> kc;
    count_batch(piece, {0, piece.size()}, {seq}, &kc);
    return kc;
  }
  // What a cover call of pieces gives beside the mask or the redacted bytes (aha_feed_cover_batch).
  struct Cover {
    std::vector<uint32_t> piece_back;         // bytes in front of piece d inside a hit that ends in it (earlier pieces' bytes)
    std::vector<uint64_t> piece_covered;      // covered bytes inside piece d
    std::vector<uint64_t> piece_hit_offsets;  // D + 1, as match_batch gives them
    std::vector<uint64_t> bases;              // D
    uint64_t n_covered = 0, n_hits = 0;
  };
  // (the call behind cover_batch / redact_batch)
  Cover cover_call(std::string_view corpus, const std::vector<uint64_t> &piece_offsets, const std::vector<uint32_t> &seq_ids,
                   std::vector<uint32_t> *mask, std::string *redacted, uint8_t fill) {
    if (piece_offsets.empty()) throw Error(AHA_E_INVALID, "piece_offsets holds D + 1 entries");
    const uint64_t D = piece_offsets.size() - 1, n = piece_offsets.back();
    if (seq_ids.size() != D) throw Error(AHA_E_INVALID, "one sequence id per piece");
    if (corpus.size() < n) throw Error(AHA_E_INVALID, "the corpus is shorter than the last offset");
    Cover c;
    c.piece_back.assign(D, 0);
    c.piece_covered.assign(D, 0);
    c.piece_hit_offsets.assign(D + 1, 0);
    c.bases.assign(D, 0);
    std::vector<uint32_t> m(mask ? (n + 31) / 32 : 0);
    std::string red(redacted ? n : 0, '\0');
    check(aha_feed_cover_batch(f_, reinterpret_cast<const uint8_t *>(corpus.data()), piece_offsets.data(), seq_ids.data(), D, 0,
                               mask && !m.empty() ? m.data() : nullptr,
                               redacted && n ? reinterpret_cast<uint8_t *>(&red[0]) : nullptr, fill,
                               D ? c.piece_back.data() : nullptr, D ? c.piece_covered.data() : nullptr,
                               c.piece_hit_offsets.data(), D ? c.bases.data() : nullptr, &c.n_covered, &c.n_hits));
    if (mask) *mask = std::move(m);
    if (redacted) *redacted = std::move(red);
    return c;
  }
  // Which bytes of the pieces lie inside a hit of their sequences, without the hit list: bit j of the batch is word j >> 5,
  // bit j & 31 of what is returned.  The sequences move on as a match call would move them.
  std::vector<uint32_t> cover_batch(std::string_view corpus, const std::vector<uint64_t> &piece_offsets,
                                    const std::vector<uint32_t> &seq_ids, Cover *info = nullptr) {
    std::vector<uint32_t> mask;
    Cover c = cover_call(corpus, piece_offsets, seq_ids, &mask, nullptr, 0);
    if (info) *info = std::move(c);
    return mask;
  }
  // The pieces with every byte inside a hit replaced by fill.  The last info->piece_back[d] bytes of the sequence in front of
  // piece d lie inside a hit as well: written one behind the other with those bytes overwritten, the pieces of a sequence give
  // AC::redact of the whole.
  std::string redact_batch(std::string_view corpus, const std::vector<uint64_t> &piece_offsets,
                           const std::vector<uint32_t> &seq_ids, char fill = '*', Cover *info = nullptr) {
    std::string red;
    Cover c = cover_call(corpus, piece_offsets, seq_ids, nullptr, &red, static_cast<uint8_t>(fill));
    if (info) *info = std::move(c);
    return red;
  }
  // the next piece of one sequence redacted; *back: how many bytes handed out before are covered too
  std::string redact(uint32_t seq, std::string_view piece, char fill = '*', uint32_t *back = nullptr) {
    Cover c;
    std::string red = redact_batch(piece, {0, piece.size()}, {seq}, fill, &c);
    if (back) *back = c.piece_back[0];
    return red;
  }
  // What a select call of pieces gives beside the hits (aha_feed_select_batch).
  struct Select {
    std::vector<uint64_t> piece_sel_offsets;  // D + 1: where each piece's hits lie
    std::vector<uint64_t> bases;              // D: the sequence's length before the piece
    std::vector<uint32_t> piece_hold;         // D: bytes at the end of the sequence whose fate is still open
    uint64_t n_hits = 0;                      // what match_batch of the same pieces would count
  };
  // The selected hits (leftmost-longest, non-overlapping, as AC::select of the whole sequence) that this call settles: for a
  // piece that takes its sequence from n0 to n1 bytes those with a start in [F(n0), F(n1)), F(n) = max(0, n - (Lmax - 1));
  // with final = true up to n1, and the named sequences start again from length 0.  Offsets are relative to the piece (start
  // may be negative, end may be <= 0).  Byte feeds only, and only for sequences fed through select calls since their reset.
  std::vector<Hit> select_batch(std::string_view corpus, const std::vector<uint64_t> &piece_offsets,
                                const std::vector<uint32_t> &seq_ids, bool final = false, Select *info = nullptr) {
    return select_flags(corpus, piece_offsets, seq_ids, final ? AHA_FEED_SELECT_FINAL : 0u, info);
  }
  // aha_feed_select_batch with `flags`: the selection, or with AHA_FEED_SELECT_TOKENS the tokens
  std::vector<Hit> select_flags(std::string_view corpus, const std::vector<uint64_t> &piece_offsets,
                                const std::vector<uint32_t> &seq_ids, uint32_t flags, Select *info) {
    if (piece_offsets.empty()) throw Error(AHA_E_INVALID, "piece_offsets holds D + 1 entries");
    const uint64_t D = piece_offsets.size() - 1;
    if (seq_ids.size() != D) throw Error(AHA_E_INVALID, "one sequence id per piece");
    if (corpus.size() < piece_offsets.back()) throw Error(AHA_E_INVALID, "the corpus is shorter than the last offset");
    Select c;
    c.piece_sel_offsets.assign(D + 1, 0);
    c.bases.assign(D, 0);
    c.piece_hold.assign(D, 0);
    std::vector<Hit> out(64);
    uint64_t n = 0;
    for (;;) {
      const int32_t rc = aha_feed_select_batch(f_, reinterpret_cast<const uint8_t *>(corpus.data()), piece_offsets.data(),
                                               seq_ids.data(), D, flags, out.data(), out.size(), c.piece_sel_offsets.data(),
                                               D ? c.bases.data() : nullptr, D ? c.piece_hold.data() : nullptr, &n, &c.n_hits);
      if (rc == AHA_E_CAPACITY) {  // (the feed is unchanged: the same call again)
        out.resize(n);
        continue;
      }
      check(rc);
      break;
    }
    out.resize(n);
    if (info) *info = std::move(c);
    return out;
  }
  // the next piece of one sequence: the selected hits it settles, with absolute offsets (they must fit Int32)
  std::vector<Hit> select(uint32_t seq, std::string_view piece, bool final = false) {
    Select c;
    auto hits = select_batch(piece, {0, piece.size()}, {seq}, final, &c);
    for (auto &h : hits) {
      h.start += (int32_t)c.bases[0];
      h.end += (int32_t)c.bases[0];
    }
    return hits;
  }
  // The tokens that this call settles (aha_feed_select_batch with AHA_FEED_SELECT_TOKENS): dictionary segmentation, as
  // AC::tokens_batch of the whole sequence, of sequences in pieces.  Per sequence the feed keeps a token cursor behind which
  // everything has been reported; the call reports the tokens from there up to the select cursor it leaves, without the last
  // where nothing yet says that it ends there.  value = the key or -1; gap_runs: gaps are not cut into characters and come in
  // parts; final: everything is reported and the named sequences start again from length 0.  info->piece_sel_offsets are the
  // pieces' offsets into the tokens, info->piece_hold the bytes behind the token cursor (it may exceed Lmax - 1).  Byte feeds
  // only, and only for sequences fed through token calls since their reset or final call.
  std::vector<Hit> tokens_batch(std::string_view corpus, const std::vector<uint64_t> &piece_offsets,
                                const std::vector<uint32_t> &seq_ids, bool final = false, bool gap_runs = false,
                                Select *info = nullptr) {
    return select_flags(corpus, piece_offsets, seq_ids,
                        (final ? AHA_FEED_SELECT_FINAL : 0u) | AHA_FEED_SELECT_TOKENS | (gap_runs ? AHA_FEED_SELECT_GAP_RUNS : 0u), info);
  }
  // the next piece of one sequence: the tokens it settles, with absolute offsets (they must fit Int32)
  std::vector<Hit> tokens(uint32_t seq, std::string_view piece, bool final = false, bool gap_runs = false) {
    Select c;
    auto toks = tokens_batch(piece, {0, piece.size()}, {seq}, final, gap_runs, &c);
    for (auto &t : toks) {
      t.start += (int32_t)c.bases[0];
      t.end += (int32_t)c.bases[0];
    }
    return toks;
  }
  // What a replace call of pieces gives beside the bytes (aha_feed_replace_batch).
  struct Replace {
    std::vector<uint64_t> piece_out_offsets;  // D + 1: where each piece's result lies
    std::vector<uint64_t> bases;              // D: the sequence's length before the piece
    std::vector<uint32_t> piece_hold;         // D: bytes at the end of the sequence that no result holds yet
    uint64_t n_selected = 0, n_hits = 0;      // as select_batch of the same pieces
  };
  // The substituted stream, built on the device: for a piece that moves its sequence's select cursor from c0 to c1 the bytes
  // T[c0 .. c1) with every hit the call settles (select_batch of the same pieces) replaced as the table says -- a table of the
  // feed's handle (AC::replacements).  With final = true everything settles and the named sequences start again from length
  // 0.  The results of one sequence's pieces, concatenated, are AC::replace_batch of the whole.  A sizing call first (it
  // changes nothing).  Byte feeds only, and only for sequences fed through select or replace calls since their reset.
  std::string replace_batch(std::string_view corpus, const std::vector<uint64_t> &piece_offsets,
                            const std::vector<uint32_t> &seq_ids, const AC::Replacements &table, bool final = false,
                            Replace *info = nullptr) {
    if (piece_offsets.empty()) throw Error(AHA_E_INVALID, "piece_offsets holds D + 1 entries");
    const uint64_t D = piece_offsets.size() - 1;
    if (seq_ids.size() != D) throw Error(AHA_E_INVALID, "one sequence id per piece");
    if (corpus.size() < piece_offsets.back()) throw Error(AHA_E_INVALID, "the corpus is shorter than the last offset");
    const uint32_t flags = final ? AHA_FEED_REPLACE_FINAL : 0u;
    const uint8_t *text = reinterpret_cast<const uint8_t *>(corpus.data());
    Replace c;
    c.piece_out_offsets.assign(D + 1, 0);
    c.bases.assign(D, 0);
    c.piece_hold.assign(D, 0);
    std::string out;
    uint64_t n = 0;
    int32_t rc = aha_feed_replace_batch(f_, table.handle(), text, piece_offsets.data(), seq_ids.data(), D, flags, nullptr, 0,
                                        c.piece_out_offsets.data(), D ? c.bases.data() : nullptr,
                                        D ? c.piece_hold.data() : nullptr, &n, &c.n_selected, &c.n_hits);
    if (rc == AHA_E_CAPACITY) {  // (the feed is unchanged: the same call again, with room)
      out.resize(n);
      rc = aha_feed_replace_batch(f_, table.handle(), text, piece_offsets.data(), seq_ids.data(), D, flags,
                                  reinterpret_cast<uint8_t *>(&out[0]), out.size(), c.piece_out_offsets.data(),
                                  D ? c.bases.data() : nullptr, D ? c.piece_hold.data() : nullptr, &n, &c.n_selected, &c.n_hits);
    }
    check(rc);
    out.resize(n);
    if (info) *info = std::move(c);
    return out;
  }
  // the next piece of one sequence: the substituted bytes that can no longer change; final: the rest
  std::string replace(uint32_t seq, std::string_view piece, const AC::Replacements &table, bool final = false) {
    return replace_batch(piece, {0, piece.size()}, {seq}, table, final);
  }
  // What a grep call of pieces gives beside the kept bytes (aha_feed_grep_batch).
  struct Grep {
    std::vector<uint64_t> kept_recs;           // n_kept: the kept closed fragments, numbered as records of the pieces
    std::vector<uint64_t> rec_out_offsets;     // n_kept + 1: where each lies in the result
    std::vector<uint64_t> piece_rec_offsets;   // D + 1: where each piece's fragments lie
    std::vector<uint64_t> piece_kept_offsets;  // D + 1: kept fragments per piece, scanned
    std::vector<uint32_t> piece_hold;          // D: bytes at the end of the piece that belong to the record left open
    std::vector<uint64_t> piece_head;          // D: held bytes to emit in front of the piece's first kept fragment
    std::vector<uint64_t> bases;               // D: the sequence's length before the piece
    std::vector<uint64_t> piece_rec_bases;     // D: the sequence's records closed before the call
    uint64_t n_recs = 0, n_hits = 0;
  };
  // The lines of sequences in pieces, kept when they have a hit: the pieces are split at `delim` as AC::records splits
  // documents; a fragment closes when it ends with the delimiter (or with final = true) and is kept when (its record, matched
  // as its own document, has a hit) != invert -- a piece's first fragment may continue a record earlier pieces left open.
  // -> the kept fragments' bytes of this call's pieces, one behind the other.  The caller keeps the bytes of the open record
  // (piece_hold) and emits them in front of the piece's first kept fragment when piece_head says so.  With final = true the
  // named sequences start again from length 0.  Byte feeds only, one delimiter per feed, and only for sequences fed through
  // grep calls since their reset.  A call with no room first (it changes nothing).
  std::string grep_batch(std::string_view corpus, const std::vector<uint64_t> &piece_offsets, const std::vector<uint32_t> &seq_ids,
                         char delim = '\n', bool invert = false, bool final = false, Grep *info = nullptr) {
    if (piece_offsets.empty()) throw Error(AHA_E_INVALID, "piece_offsets holds D + 1 entries");
    const uint64_t D = piece_offsets.size() - 1;
    if (seq_ids.size() != D) throw Error(AHA_E_INVALID, "one sequence id per piece");
    if (corpus.size() < piece_offsets.back()) throw Error(AHA_E_INVALID, "the corpus is shorter than the last offset");
    const uint32_t flags = (invert ? AHA_GREP_INVERT : 0u) | (final ? AHA_FEED_GREP_FINAL : 0u);
    const uint8_t *text = reinterpret_cast<const uint8_t *>(corpus.data());
    Grep c;
    c.piece_rec_offsets.assign(D + 1, 0);
    c.piece_kept_offsets.assign(D + 1, 0);
    c.piece_hold.assign(D, 0);
    c.piece_head.assign(D, 0);
    c.bases.assign(D, 0);
    c.piece_rec_bases.assign(D, 0);
    c.kept_recs.assign(1, 0);
    c.rec_out_offsets.assign(1, 0);
    std::string out(1, '\0');
    uint64_t nk = 0, nb = 0;
    auto call = [&](uint64_t cap_recs, uint64_t cap_bytes) {
      return aha_feed_grep_batch(f_, text, piece_offsets.data(), seq_ids.data(), D, (uint8_t)delim, flags, c.kept_recs.data(),
                                 c.rec_out_offsets.data(), cap_recs, reinterpret_cast<uint8_t *>(&out[0]), cap_bytes,
                                 c.piece_rec_offsets.data(), c.piece_kept_offsets.data(), D ? c.piece_hold.data() : nullptr,
                                 D ? c.piece_head.data() : nullptr, D ? c.bases.data() : nullptr,
                                 D ? c.piece_rec_bases.data() : nullptr, &c.n_recs, &nk, &nb, &c.n_hits);
    };
    int32_t rc = call(0, 0);
    if (rc == AHA_E_CAPACITY) {  // (the feed is unchanged: the same call again, with room)
      c.kept_recs.assign(std::max<uint64_t>(nk, 1), 0);
      c.rec_out_offsets.assign(nk + 1, 0);
      out.assign(std::max<uint64_t>(nb, 1), '\0');
      rc = call(nk, nb);
    }
    check(rc);
    c.kept_recs.resize(nk);
    c.rec_out_offsets.resize(nk + 1);
    out.resize(nb);
    if (info) *info = std::move(c);
    return out;
  }
  // the next piece of one sequence: the kept lines that close with it, the held bytes of the open line in front of the first
  // where it is kept; the open line's bytes stay in this object.  final: the open line closes.  One delimiter and one invert
  // per sequence; the lines of a sequence's pieces, in order, are AC::grep of the whole.
  std::vector<std::string> grep(uint32_t seq, std::string_view piece, char delim = '\n', bool invert = false, bool final = false) {
    Grep c;
    const std::string raw = grep_batch(piece, {0, piece.size()}, {seq}, delim, invert, final, &c);
    std::vector<std::string> lines;
    for (size_t i = 0; i + 1 < c.rec_out_offsets.size(); i++)
      lines.emplace_back(raw.substr(c.rec_out_offsets[i], c.rec_out_offsets[i + 1] - c.rec_out_offsets[i]));
    std::string &held = grep_held_[seq];
    if (c.piece_head[0]) {
      const std::string open = held.substr(held.size() - c.piece_head[0]);
      if (lines.empty())
        lines.push_back(open);  // (an empty piece under final: the line closes without a fragment)
      else
        lines[0] = open + lines[0];
    }
    if (final)
      held.clear();
    else if (c.piece_hold[0] == piece.size())
      held.append(piece);
    else
      held.assign(piece.substr(piece.size() - c.piece_hold[0]));
    return lines;
  }
  void reset(uint32_t seq = UINT32_MAX) {
    check(aha_feed_reset(f_, seq));
    if (seq == UINT32_MAX)
      grep_held_.clear();
    else
      grep_held_.erase(seq);
  }
  // {bytes, chars} fed to the sequence so far
  std::pair<uint64_t, uint64_t> position(uint32_t seq) const {
    uint64_t b = 0, c = 0;
    check(aha_feed_position(f_, seq, &b, &c));
    return {b, c};
  }
  aha_feed *handle() const { return f_; }

 private:
  Feed(const AC &ac, uint32_t n_seqs, const aha_match_params &p) : ac_(ac.handle()) {
    const int32_t rc = aha_feed_open_params(ac_, n_seqs, 0u, &p, &f_);
    if (rc != AHA_OK) {
      const char *m = aha_last_error(ac_);
      throw Error(rc, (m && *m) ? m : aha_strerror(rc));
    }
  }
  void check(int32_t rc) const {
    if (rc == AHA_OK) return;
    const char *m = aha_last_error(ac_);
    throw Error(rc, (m && *m) ? m : aha_strerror(rc));
  }
  aha_ac *ac_;
  aha_feed *f_ = nullptr;
  std::map<uint32_t, std::string> grep_held_;  // grep(): the bytes of every sequence's open line
};

// Several GPUs of one node behind one object (aha_group_*): contiguous byte-balanced document ranges, one per device entry,
// all-gatherv of the hit buffers.  match_batch: host buffers in and out; upload + match_resident: the batch stays on the
// devices, the hits too (shard_hits reads one device's copy of the whole ordered stream).
class Group {
 public:
  Group(const Group &) = delete;
  Group &operator=(const Group &) = delete;
  ~Group() { aha_group_free(g_); }

  static Group compile(const std::vector<std::string> &keys, const std::vector<int32_t> &devices, bool fold_ascii = false) {
    if (aha_abi_version() != AHA_ABI_VERSION) throw Error(AHA_E_INVALID, "libaha_hip.so is not the ABI this header declares");
    std::vector<uint8_t> blob;
    std::vector<uint64_t> offs(keys.size() + 1, 0);
    for (size_t i = 0; i < keys.size(); i++) {
      blob.insert(blob.end(), keys[i].begin(), keys[i].end());
      offs[i + 1] = blob.size();
    }
    aha_group *g = nullptr;
    uint32_t bad = 0;
    int32_t rc = aha_group_compile(blob.data(), offs.data(), (uint32_t)keys.size(), devices.data(), (int32_t)devices.size(),
                                   fold_ascii ? AHA_OPT_FOLD_ASCII : 0u, &g, &bad);
    if (rc == AHA_E_DUP_KEY) throw Error(rc, "key:" + keys[bad] + " appear twice.", bad);
    if (rc != AHA_OK) throw Error(rc, aha_strerror(rc), bad);
    return Group(g);
  }
  Group(Group &&o) noexcept : g_(o.g_) { o.g_ = nullptr; }

  std::vector<Hit> match_batch(std::string_view corpus, const std::vector<uint64_t> &doc_offsets,
                               std::vector<uint64_t> *doc_hit_offsets = nullptr, bool chars = false) const {
    if (doc_offsets.empty()) throw Error(AHA_E_INVALID, "doc_offsets holds D + 1 entries");
    aha_match_params p{};
    p.struct_size = sizeof(p);
    p.char_offsets = chars ? 1 : 0;
    std::vector<uint64_t> dho(doc_offsets.size(), 0);
    std::vector<Hit> out(corpus.size() / 8 + 64);
    uint64_t n = 0;
    for (;;) {
      int32_t rc = aha_group_match_batch(g_, reinterpret_cast<const uint8_t *>(corpus.data()), doc_offsets.data(),
                                         doc_offsets.size() - 1, &p, out.data(), out.size(), dho.data(), &n);
      if (rc == AHA_E_CAPACITY) {
        out.resize(n);
        continue;
      }
      if (rc != AHA_OK) throw Error(rc, aha_group_last_error(g_));
      break;
    }
    out.resize(n);
    if (doc_hit_offsets) *doc_hit_offsets = dho;
    return out;
  }

  // the batch resident on the devices (aha_group_corpus_upload); must not outlive its group
  class Resident {
   public:
    Resident(const Resident &) = delete;
    Resident &operator=(const Resident &) = delete;
    Resident(Resident &&o) noexcept : c_(o.c_), n_docs_(o.n_docs_) { o.c_ = nullptr; }
    ~Resident() { aha_group_corpus_free(c_); }
    uint64_t n_docs() const { return n_docs_; }
    const aha_group_corpus *handle() const { return c_; }

   private:
    friend class Group;
    Resident(aha_group_corpus *c, uint64_t n) : c_(c), n_docs_(n) {}
    aha_group_corpus *c_;
    uint64_t n_docs_;
  };
  Resident upload(std::string_view corpus, const std::vector<uint64_t> &doc_offsets) const {
    if (doc_offsets.empty()) throw Error(AHA_E_INVALID, "doc_offsets holds D + 1 entries");
    aha_group_corpus *c = nullptr;
    int32_t rc = aha_group_corpus_upload(g_, reinterpret_cast<const uint8_t *>(corpus.data()), doc_offsets.data(),
                                         doc_offsets.size() - 1, &c);
    if (rc != AHA_OK) throw Error(rc, aha_group_last_error(g_));
    return Resident(c, doc_offsets.size() - 1);
  }
  // every device matches its resident range, then the all-gatherv: the hit count (the hits stay on the devices)
  uint64_t match_resident(const Resident &c, std::vector<uint64_t> *doc_hit_offsets = nullptr, bool chars = false) const {
    aha_match_params p{};
    p.struct_size = sizeof(p);
    p.char_offsets = chars ? 1 : 0;
    std::vector<uint64_t> dho(c.n_docs() + 1, 0);
    uint64_t n = 0;
    int32_t rc = aha_group_match_batch_device(g_, c.handle(), &p, dho.data(), &n);
    if (rc != AHA_OK) throw Error(rc, aha_group_last_error(g_));
    if (doc_hit_offsets) *doc_hit_offsets = dho;
    return n;
  }
  std::vector<Hit> shard_hits(int32_t shard) const {
    uint64_t n = 0;
    aha_group_download_shard(g_, shard, nullptr, 0, &n);
    std::vector<Hit> out(n + 1);
    int32_t rc = aha_group_download_shard(g_, shard, out.data(), out.size(), &n);
    if (rc != AHA_OK) throw Error(rc, aha_group_last_error(g_));
    out.resize(n);
    return out;
  }
  aha_group *handle() const { return g_; }

 private:
  explicit Group(aha_group *g) : g_(g) {}
  aha_group *g_;
};

}  // namespace aha
