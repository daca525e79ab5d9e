// engine.cpp -- which kernels answer a call: the engines' setup on a device handle, the pipeline of one pass (match_v2:
// regions / full regions / slabs; byte-level, character-level, skip-ahead or prefix-filter traversal), and the sequence of
// passes of a device-resident batch (device_match: the prefix filter's back-off, the repeat with larger regions, the hand-over
// to the two-pass engine).  The C ABI around it is capi.cpp; what they share is handle.hpp.
#include "handle.hpp"
#include "class_overflow.hpp"
#include "doc_ranges.hpp"

#include <chrono>
#include <optional>

namespace ahai {

// ---- single-traversal engine: sizing, scratch, orchestration ----------------
constexpr size_t kLdsPerCU = 160 * 1024;
constexpr uint64_t kV2MaxRegionBytes = 48ull << 30;

// The skip-ahead traversal (scan_skip.hip) can take a handle's plain byte-offset matches when the unit image has 22-bit
// bases and no key is a single unit.  It is OPT-IN (AHA_ENGINE=skip -- the unit image for every eligible key set like "unit" --
// or AHA_SKIP=1 beside the library's own choice): measured on cfg 3 its second kernel is bound by the scattered 16-byte text
// requests of its free-running lanes -- 3.75 ms per GiB against 2.24 for ku_traverse (profiles/r06_skip_engine.txt, DESIGN.md
// section 4.7) --, so no key set gets it by default.
bool skip_eligible(const aha_ac *ac) {
  const UnitImage &u = ac->unit;
  if (!u.ok || u.base_bits != 22 || u.unit_key || u.mark_bloom.empty()) return false;
  const char *eng = getenv("AHA_ENGINE");
  if (eng && strcmp(eng, "skip") != 0) return false;
  // (its walk has the header trip only: images whose states mostly own a header take ku_traverse<.., HB> -- v2_setup's rule)
  const char *hb = getenv("AHA_UNIT_HEADER_BESIDE");
  if (hb ? atoi(hb) != 0 : (!eng && (uint64_t)u.n_nfr * 5 >= u.n_states)) return false;  // (AHA_ENGINE=skip: the header trip)
  const char *sk = getenv("AHA_SKIP");
  if (sk) return atoi(sk) != 0;
  return eng != nullptr;
}

// Host-only plan: how much of the image the traversal kernel keeps in LDS.
// The pair engine (scan_pair.hip) takes a handle's plain byte-offset matches when the unit image has 22-bit bases, no key is a
// single unit, the two-unit paths have a perfect hash table and no trie path holds more than three END states of three
// units or more (the slots its first pass leaves for a deep walk's events).  AHA_ENGINE=pair builds the unit image for every
// eligible key set like "unit" does; AHA_PAIR=0 / 1 overrides the library's own choice.
bool pair_eligible(const aha_ac *ac) {
  const UnitImage &u = ac->unit;
  if (!u.ok || u.base_bits != 22 || u.unit_key || u.pair_tab.empty() || u.mark_bloom.empty() || u.deep_ends_max > kPairMaxDeepEnds ||
      ac->aut.max_key_len > 255)
    return false;
  for (uint32_t k = 0; k < ac->aut.n_keys; k++)
    if (ac->aut.key_cnt[k] >= 255u) return false;  // (an event's hits ride in one byte of the pair table's payload)
  const char *eng = getenv("AHA_ENGINE");
  if (eng && strcmp(eng, "pair") != 0) return false;
  const char *pr = getenv("AHA_PAIR");
  if (pr) return atoi(pr) != 0;
  return eng != nullptr;
}

void plan_engine(aha_ac *ac, const Placement &pl) {
  (void)pl;
  const size_t in_bytes = (size_t)(kV2Threads / 64) * 64 * (kV2Piece + 4);  // padded LDS input rows
  const size_t slot = ac->compact ? 4 : 8;
  // AHA_V2_BPC=2: two workgroups per CU (half the LDS each, twice the waves)
  const char *bpc = getenv("AHA_V2_BPC");
  ac->v2_bpc = (bpc && strcmp(bpc, "2") == 0) ? 2 : 1;
  const size_t budget = kLdsPerCU / ac->v2_bpc - in_bytes;
  // AHA_LDS_SLOTS=n caps the prefix (tests: forces the partial-prefix kernel on small automata)
  const char *cap_s = getenv("AHA_LDS_SLOTS");
  const size_t cap_slots = cap_s ? (size_t)std::max(256, atoi(cap_s)) & ~(size_t)255 : SIZE_MAX;
  if ((size_t)ac->n_slots * slot <= budget && ac->n_slots <= cap_slots) {  // the whole automaton lives in LDS
    ac->v2_lds_slots = ac->n_slots;
    return;
  }
  ac->v2_lds_slots = (uint32_t)std::min<size_t>(std::min<size_t>(budget / slot, cap_slots), ac->n_slots) & ~3u;
}

// Document counts: the bounds and thresholds of device_doc_counts, read once per handle (tests lower them to reach every form
// and the document ranges with small batches; DESIGN.md sections 4.11 and 7).
static void doccount_setup(aha_ac *ac) {
  auto env = [](const char *name, uint64_t dflt, uint64_t lo, uint64_t hi) {
    const char *v = getenv(name);
    if (!v || atoll(v) <= 0) return dflt;
    return std::min(std::max<uint64_t>((uint64_t)atoll(v), lo), hi);
  };
  const uint64_t K = ac->aut.n_keys;
  ac->dc_hit_bytes = env("AHA_DOCCOUNT_HIT_BYTES", kV2MaxRegionBytes, 12, kV2MaxRegionBytes);
  ac->dc_row_bytes = env("AHA_DOCCOUNT_ROW_BYTES", 1ull << 30, 4, 1ull << 34);
  ac->dc_sort_max = (uint32_t)env("AHA_DOCCOUNT_SORT_MAX", kDcSortMax, 1, kDcSortMax);
  ac->dc_range_keys = (uint32_t)env("AHA_DOCCOUNT_RANGE_KEYS", kDcRangeKeys, 1, kDcRangeKeys);
  // the dense form costs O(K) per document: from K / 8 hits on
  ac->dc_dense_min = (uint32_t)env("AHA_DOCCOUNT_DENSE_MIN", std::max<uint64_t>(ac->dc_sort_max + 1ull, K / 8), 1, 0x7FFFFFFFull);
  // select calls: the bound of a range's hit buffer, by default the document counts' (device_select)
  ac->sel_hit_bytes = env("AHA_SELECT_HIT_BYTES", ac->dc_hit_bytes, 12, kV2MaxRegionBytes);
  // replace calls: the cap of the scan's and the copy's grids (tests: 1, so that workgroups loop over tiles)
  ac->rep_blocks = (uint32_t)env("AHA_REPLACE_BLOCKS", 0, 1, 1u << 20);
  // records and grep calls: the cap of their grids, the reused rank, scan and copy launches included
  ac->grep_blocks = (uint32_t)env("AHA_GREP_BLOCKS", 0, 1, 1u << 20);
  // class-counts calls: the bound of a range's hit buffer, by default the document counts', and the cap of their kernels' grids
  // (tests: a few hits, so that a batch takes several ranges or a document goes through its key counts; 1 block)
  ac->cls_hit_bytes = env("AHA_CLASS_HIT_BYTES", ac->dc_hit_bytes, 12, kV2MaxRegionBytes);
  ac->cls_blocks = (uint32_t)env("AHA_CLASS_BLOCKS", 0, 1, 1u << 20);
  // rule grep: the bound of the class-count table a call keeps in scratch where the caller gives no rows (tests: a few bytes,
  // so that the refusal is reached).  1 GiB: 4 M documents of 64 classes, well under the device's memory
  ac->rule_table_bytes = env("AHA_RULE_TABLE_BYTES", 1ull << 30, 4, 1ull << 36);
  // the passes after the traversal: the cap of their grids (tests: 1 and 3, so that every lane strides)
  ac->post_blocks = (uint32_t)env("AHA_POST_BLOCKS", 0, 1, 1u << 20);
  // feed token calls: how long a token may stay open, so that int32 offsets hold it (tests: a few bytes)
  ac->feed_token_open = (uint32_t)env("AHA_FEED_TOKEN_OPEN", 0x3FFFFFFFull, 1, 0x3FFFFFFFull);
}

uint32_t post_grid(const aha_ac *ac) { return ac->post_blocks ? ac->post_blocks : 8u * std::max<uint32_t>(ac->v2_grid, 64u); }

void v2_setup(aha_ac *ac) {
  doccount_setup(ac);
  const char *eng = getenv("AHA_ENGINE");
  if (eng && strcmp(eng, "v1") == 0) return;
  int cus = 0;
  if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, ac->device) != hipSuccess || cus <= 0)
    return;
  if (v2_prepare(ac->compact, v2_lds_bytes(ac->v2_lds_slots, ac->compact)) != 0) return;
  // AHA_RESERVE_CUS=n: leave n CUs without a persistent traversal workgroup so that
  // collective (RCCL) kernels of an overlapped exchange can run beside it
  const char *rs = getenv("AHA_RESERVE_CUS");
  int reserve = rs ? atoi(rs) : 0;
  if (reserve < 0 || reserve >= cus) reserve = 0;
  ac->v2_grid = (uint32_t)(cus - reserve) * ac->v2_bpc;
  ac->v2_ok = true;
  if (ac->pf_d && filter_prepare() == 0 && upload(ac, ac->pf_bloom, &ac->fdev.bloom) == AHA_OK) {
    ac->fdev.d = ac->pf_d;
    ac->fdev.log2 = ac->pf_log2;
    ac->pf_cus = (uint32_t)(cus - reserve);
    ac->pf_ok = true;
  }
  // character-level engine: one step per UTF-8-shaped unit (unit.hpp).  One workgroup per CU: its LDS holds the root's
  // transitions of the whole alphabet.
  if (ac->unit.ok && ac->v2_bpc == 1 && unit_lds_bytes(ac->unit.n_syms) <= kLdsPerCU) {
    const Automaton &a = ac->aut;
    std::vector<uint32_t> info(ac->unit.end_key.size(), 0xFFFFFFFFu);
    for (size_t i = 0; i < info.size(); i++) {
      const int32_t k = ac->unit.end_key[i];
      if (k >= 0) info[i] = ac->key_info.empty() ? ((uint32_t)k | (std::min<uint32_t>(a.key_cnt[k], 255u) << 24)) : ac->key_info[k];
    }
    // the fused expansion's table: one gather gives an event's first hit and where the rest of its chain is
    uint32_t max_cnt = 0;
    for (uint32_t k = 0; k < a.n_keys; k++) max_cnt = std::max(max_cnt, a.key_cnt[k]);
    const char *upost = getenv("AHA_UNIT_POST");  // "regroup": the general post passes (tests)
    const bool fused = !ac->key_info.empty() && max_cnt <= kUFusedMaxChain && a.max_key_len < 65536 &&
                       !(upost && strcmp(upost, "regroup") == 0);
    std::vector<uint2> uend, uendc;
    if (fused) {
      uend.assign(ac->unit.end_key.size(), uint2{0, 0});
      uendc = uend;
      for (size_t i = 0; i < uend.size(); i++) {
        const int32_t k = ac->unit.end_key[i];
        if (k < 0) continue;
        const uint32_t co = ac->key_info[k] & 0xFFFFFFu, len = a.key_len[k], kc = a.key_kc[k] + 1u;
        uend[i] = uint2{(uint32_t)k | (len & 0xFFu) << 24, co | (len >> 8) << 24};
        uendc[i] = uint2{(uint32_t)k | (kc & 0xFFu) << 24, co | (kc >> 8) << 24};
      }
    }
    const uint64_t *us = nullptr;
    if (fused && upload(ac, uend, &ac->d_unit_end) == AHA_OK && upload(ac, uendc, &ac->d_unit_end_chars) == AHA_OK)
      ac->unit_fused = true;
    if (unit_prepare(ac->unit.n_syms) == 0 && upload(ac, ac->unit.slots, &us) == AHA_OK &&
        upload(ac, ac->unit.root, &ac->udev.root) == AHA_OK && upload(ac, ac->unit.tables, &ac->udev.tables) == AHA_OK &&
        upload(ac, info, &ac->d_unit_end_info) == AHA_OK) {
      ac->udev.slots = reinterpret_cast<const uint2 *>(us);
      ac->udev.n_slots = ac->unit.n_slots;
      ac->udev.big_lo = ac->unit.n_shared;
      ac->udev.n_low = ac->unit.n_low;
      ac->udev.g0 = ac->unit.g0;
      ac->udev.base_bits = ac->unit.base_bits;
      ac->udev.n_syms = ac->unit.n_syms;
      ac->udev.max_len = a.max_key_len;
      // text falls out of deep matches where many states own a fail header: then the header comes beside the probe (a second
      // load in every trip) instead of in a trip of its own -- -8.5 % on cfg 5, +3.5 % on cfg 3 (profiles/r04_two_walks.txt)
      const char *hb = getenv("AHA_UNIT_HEADER_BESIDE");  // 0 / 1: tests
      const char *eng2 = getenv("AHA_ENGINE");
      ac->udev.hdr_beside = hb ? (uint32_t)(atoi(hb) != 0)
                               : (uint32_t)(!(eng2 && strcmp(eng2, "skip") == 0) && (uint64_t)ac->unit.n_nfr * 5 >= ac->unit.n_states);
      ac->unit_ok = true;
      // the skip-ahead traversal over the same image: its filter over the two-unit paths (unit.hpp, MARKS)
      if (skip_eligible(ac) && !ac->udev.hdr_beside && skip_prepare(ac->unit.n_syms, ac->unit.mark_log2) == 0 &&
          upload(ac, ac->unit.mark_bloom, &ac->sdev.bloom) == AHA_OK) {
        ac->sdev.log2 = ac->unit.mark_log2;
        ac->sdev.k1 = ac->unit.pair_k1;
        ac->skip_ok = true;
      }
      // the pair engine: the same filter, the pair table with the events' payloads (what end_info holds for the state), its
      // displacement bytes
      if (pair_eligible(ac) && pair_prepare(ac->unit.n_syms, ac->unit.mark_log2, ac->unit.pair_groups) == 0) {
        std::vector<uint32_t> tab = ac->unit.pair_tab;
        for (size_t i = 0; i < tab.size(); i += 4) {
          const int32_t k = (int32_t)tab[i + 2];
          tab[i + 2] = (tab[i] == 0u || k < 0) ? 0u : (ac->key_info.empty() ? ((uint32_t)k | (std::min<uint32_t>(a.key_cnt[k], 255u) << 24)) : ac->key_info[k]);
        }
        const uint32_t *dt = nullptr;
        if (upload(ac, ac->unit.mark_bloom, &ac->pdev.bloom) == AHA_OK && upload(ac, tab, &dt) == AHA_OK &&
            upload(ac, ac->unit.pair_disp, &ac->pdev.disp) == AHA_OK) {
          ac->pdev.tab = reinterpret_cast<const uint4 *>(dt);
          ac->pdev.bloom_log2 = ac->unit.mark_log2;
          ac->pdev.k1 = ac->unit.pair_k1;
          ac->pdev.log2 = ac->unit.pair_log2;
          ac->pdev.groups = ac->unit.pair_groups;
          ac->pair_ok = true;
        }
      }
    }
  }
}

// a grow-only slot that answers for itself: the allocator's error as the call's
static int32_t reserve_or_text(Buf &b, size_t bytes) {
  const hipError_t e = reserve(b, bytes, kGrowEighth);
  if (e == hipSuccess) return AHA_OK;
  tls_err = std::string("hipMalloc(&b.p, want): ") + hipGetErrorString(e);
  return AHA_E_HIP;
}
// a slot of v2buf (handle.hpp V2Slot)
static int32_t v2_reserve(Scratch *sc, V2Slot slot, size_t bytes) {
  // a new counter block (see Scratch::cursor_dirty): cleared in full by the next call, whatever its address
  if (slot == kCursor && sc->v2buf[slot].bytes < bytes) sc->reset_cursor();
  return reserve_or_text(sc->v2buf[slot], bytes);
}

// Pipeline of one call, a function of the call alone (the handle keeps no history):
//   kRegions      per-chunk event regions sized from the caller's capacity (a hit is an event or hangs on one, so the
//                 batch has at most `cap` events the caller can take: twice the average per chunk, plus slack)
//   kFullRegions  regions of one event per input byte (cannot overflow); taken at once when cap says the caller
//                 expects more than one hit per 4 bytes, else after a region overflowed
//   kSlabs        slab + sort pipeline: separator filter, fewer than 16 hits per chunk expected (its cost follows the
//                 events, not the chunks), or regions beyond the temp bound
enum V2Mode { kRegions = 0, kFullRegions = 1, kSlabs = 2 };
// Field widths of the 4-byte exchange stream for this automaton (include/aha_hip.h): the key id needs vb bits, a key's
// length lb bits (in bytes; its length in characters is not longer); when at least 6 bits are left for the step of `end`
// the word carries the length, else only id and a 12-bit step (ids below 2^20) and the receiver looks the length up.
StreamFmt stream_fmt(const aha_ac *ac) {
  auto bits = [](uint32_t x) {
    uint32_t b = 0;
    while (x) {
      b++;
      x >>= 1;
    }
    return b;
  };
  const uint32_t vb = std::max(1u, bits(ac->aut.n_keys ? ac->aut.n_keys - 1 : 0)), lb = std::max(1u, bits(ac->aut.max_key_len));
  // (a step field below 10 bits makes every gap of 1 KiB an exception -- 4 more bytes on the link --, which costs a
  // sparse hit stream more than the key-length lookup on arrival saves: then the word carries id and a 12-bit step only)
  if (vb + lb + 10 <= 32) return StreamFmt{std::min(12u, 32 - vb - lb), lb};
  return StreamFmt{12, 0};
}

// device-resident offsets that are not what the call says (k_check_docs): out of order, or a document of 2 GiB
static int32_t bad_offsets(bool order) {
  tls_err = order ? "doc offsets: need doc_offsets[0] = 0, ascending, doc_offsets[n_docs] = n_bytes" : aha_strerror(AHA_E_TOO_LONG);
  return order ? AHA_E_INVALID : AHA_E_TOO_LONG;
}
// the pinned words a call's verdict and totals come back in, and their device address
int32_t ensure_h_v2(aha_ac *ac, Scratch *sc) {
  if (sc->h_v2) return AHA_OK;
  HIPCHK(ac, hipHostMalloc((void **)&sc->h_v2, 5 * sizeof(unsigned long long), hipHostMallocDefault));
  if (hipHostGetDevicePointer((void **)&sc->h_v2_dev, sc->h_v2, 0) != hipSuccess) {
    (void)hipGetLastError();
    sc->h_v2_dev = nullptr;  // (then the words come back by a copy)
  }
  return AHA_OK;
}

// scratch of a cover call (Scratch::covbuf), grow-only; null: no memory
static void *cover_reserve(Scratch *sc, CoverSlot slot, size_t bytes) { return reserve_ptr(sc->covbuf[slot], bytes, kGrowEighth); }

// The kernels read a text in aligned 16-byte pieces, and a folded handle (AHA_OPT_FOLD_ASCII) matches the folded text: *text
// becomes its copy in `dst` (n_bytes + 64 bytes of scratch), a plain device-to-device copy (~0.7 ms per GiB: about a fifth of
// a match) or, with `fold` (the handle's fold mode: 1 ASCII, 2 simple, 3 BMP, 4 kana), the one streaming pass that does both jobs
// (scan_fold.hip).  The simple, the BMP and the kana fold are those of every document on its own: doc_off (device) are the n_docs + 1 offsets of
// exactly these n_bytes, a batch or a range of whole documents.  The caller's text is only read.
static int32_t stage_text(aha_ac *ac, const uint8_t **text, uint64_t n_bytes, void *dst, int fold, const uint64_t *doc_off,
                          uint64_t n_docs, hipStream_t s) {
  if (fold) {
    const uint32_t max_blocks = post_grid(ac);
    if (fold == 4)
      foldk_launch_copy(*text, (uint8_t *)dst, n_bytes, doc_off, n_docs, max_blocks, s);
    else if (fold == 3)
      fold3_launch_copy(*text, (uint8_t *)dst, n_bytes, doc_off, n_docs, max_blocks, s);
    else if (fold == 2)
      fold2_launch_copy(*text, (uint8_t *)dst, n_bytes, doc_off, n_docs, max_blocks, s);
    else
      fold_launch_copy(*text, (uint8_t *)dst, n_bytes, max_blocks, s);
    HIPCHK(ac, hipGetLastError());
  } else {
    HIPCHK(ac, hipMemcpyAsync(dst, *text, n_bytes, hipMemcpyDeviceToDevice, s));
  }
  *text = (const uint8_t *)dst;
  return AHA_OK;
}
// ... of a whole batch, in v2buf[kText]
static int32_t stage_batch(aha_ac *ac, Scratch *sc, const uint8_t **text, uint64_t n_bytes, int fold, const uint64_t *doc_off,
                           uint64_t n_docs, hipStream_t s) {
  if (int32_t rc = v2_reserve(sc, kText, n_bytes + 64)) return rc;
  return stage_text(ac, text, n_bytes, sc->v2buf[kText].p, fold, doc_off, n_docs, s);
}
// M.fold (the fold mode): M.text is still the caller's.  Only the prefix-filter engine takes it like that, and only the ASCII
// fold (it folds in its own loads; with the simple, the BMP and the kana fold -- M.fold >= 2 -- it reads the staged copy like everyone else: match_v2); every
// other path -- the byte-level and character-level engines, the opt-in ones, the two-pass engine, match_longest, a pass
// behind a hand-back of the filter -- calls this first: the copy is made at that moment, once per call.
static int32_t stage_folded(aha_ac *ac, Scratch *sc, MatchArgs &M, hipStream_t s) {
  if (!M.fold) return AHA_OK;
  const int32_t rc = stage_batch(ac, sc, &M.text, M.n_bytes, M.fold, M.doc_off, M.n_docs, s);
  if (rc == AHA_OK) M.fold = 0;
  return rc;
}
// The text of a device-resident batch as the engines take it (device_match, device_count): an unaligned view (a slice of a
// larger buffer) is copied once into scratch, folded on the way on a folded handle; an aligned text stays the caller's, and on
// a folded handle M.fold says so: the prefix-filter engine reads it where it lies, the others stage it (stage_folded).
// (M.doc_off and M.n_docs are the batch's by now: the simple fold goes document by document)
// as_is: the text is already as the engines take it -- a folded feed's pieces and windows (feed.cpp), folded by the feed with
// its sequences' contexts in view: M.fold stays 0 and only an unaligned view is copied.  Folding folded text again would change
// no byte (F, F3 and FK are idempotent and fragments pass through): the switch saves a staged pass, it corrects nothing.
static int32_t take_text(aha_ac *ac, Scratch *sc, const uint8_t *d_corpus, uint64_t n_bytes, MatchArgs &M, hipStream_t s,
                         bool as_is = false) {
  M.text = d_corpus;
  const int fold = as_is ? 0 : ac->fold_mode();
  if (reinterpret_cast<uintptr_t>(d_corpus) % 16 != 0) return stage_batch(ac, sc, &M.text, n_bytes, fold, M.doc_off, M.n_docs, s);
  M.fold = fold;
  return AHA_OK;
}
// The two-pass engine's chunk: `chunk0`, doubled until the warm-up (a multiple of Lmax - 1 bytes) is a small fraction of it --
// 8 * Lmax for its own passes, 16 * Lmax for match_longest's.
static void two_pass_chunks(const aha_ac *ac, MatchArgs &M, uint32_t chunk0, uint64_t lmax_mul) {
  M.chunk = chunk0;
  while (M.chunk < lmax_mul * ac->aut.max_key_len && M.chunk < (1u << 20)) M.chunk *= 2;
  M.n_chunks = (M.n_bytes + M.chunk - 1) / M.chunk;
}
// the two-pass engine's totals (handle.hpp TwoPassSlot) and the pinned words they come back in: what match_longest's NUL look
// needs before the rest is bound
static int32_t two_pass_totals(aha_ac *ac, Scratch *sc) {
  if (int32_t rc = reserve_or_text(sc->tpbuf[kTpTotals], 2 * sizeof(uint64_t))) return rc;
  if (!sc->h_totals) HIPCHK(ac, hipHostMalloc((void **)&sc->h_totals, 2 * sizeof(uint64_t), hipHostMallocDefault));
  return AHA_OK;
}
static uint64_t *d_totals(Scratch *sc) { return (uint64_t *)sc->tpbuf[kTpTotals].p; }
// ... and its scratch for `units` counters (chunks or documents) and M.n_docs documents, reserved and bound to M
static int32_t bind_two_pass(aha_ac *ac, Scratch *sc, MatchArgs &M, uint64_t units, uint64_t *n_blocks) {
  *n_blocks = (units + kBlock - 1) / kBlock;
  const size_t sizes[kTpCount] = {units * 4, units * 4, *n_blocks * 8, *n_blocks * 8, (M.n_docs + 1) * 8, 0};  // (kTpTotals: below)
  for (int i = 0; i < kTpTotals; i++)
    if (int32_t rc = reserve_or_text(sc->tpbuf[i], sizes[i])) return rc;
  if (int32_t rc = two_pass_totals(ac, sc)) return rc;
  auto at = [sc](TwoPassSlot slot) { return sc->tpbuf[slot].p; };
  M.counts = (uint32_t *)at(kTpCounts);
  M.leads = (uint32_t *)at(kTpLeads);
  M.blk_hits = (uint64_t *)at(kTpBlkHits);
  M.blk_leads = (uint64_t *)at(kTpBlkLeads);
  M.docg = (uint64_t *)at(kTpDocG);
  M.totals = d_totals(sc);
  return AHA_OK;
}
// One pass's aha_timing from the events of its scratch set, published: ms_total ev[0] .. ev[4], ms_count ev[0] .. ev[count_end],
// ms_write ev[3] .. ev[4], ms_scan and ms_aux between the pairs given (first < 0: not measured); `t` carries the rest.
static void publish_event_timing(aha_ac *ac, Scratch *sc, aha_timing t, int count_end, int scan0, int scan1, int aux0, int aux1) {
  t.struct_size = sizeof(t);
  (void)hipEventElapsedTime(&t.ms_total, sc->ev[0], sc->ev[4]);
  (void)hipEventElapsedTime(&t.ms_count, sc->ev[0], sc->ev[count_end]);
  if (scan0 >= 0) (void)hipEventElapsedTime(&t.ms_scan, sc->ev[scan0], sc->ev[scan1]);
  if (aux0 >= 0) (void)hipEventElapsedTime(&t.ms_aux, sc->ev[aux0], sc->ev[aux1]);
  (void)hipEventElapsedTime(&t.ms_write, sc->ev[3], sc->ev[4]);
  publish_timing(ac, t);
}

// ---- one pass of the single-traversal engines: plan_v2 decides, launch_v2 reserves, binds and launches, verdict_v2 reads back
// What a pass will do, decided before anything is allocated or launched.
struct V2Plan {
  V2Mode mode;         // the pipeline (the mode asked for, after the rules below)
  bool direct;         // ... one of the region pipelines
  bool dense;          // more than one hit per 4 input bytes expected
  bool filt, want_pair, pair, unit, skip;  // the engine: prefix filter, pair (wanted / taken), character-level, ... behind the skip marks; none: byte-level
  uint64_t S;          // chunk bytes
  uint64_t n_chunks;
  uint64_t stride;     // events per chunk region
  uint64_t rec_bytes;  // bytes per event of the regions: 8 (byte-level engine), 12 (character-level, fused expansion), 12 + 8 (general passes)
  uint64_t ev_cap;     // slab pipeline: events the temp holds
  uint64_t cand_cap;   // deep candidates the pair engine has room for
  size_t sizes[kV2Count];  // bytes per slot of v2buf (0: not used by this pass)
};

// The planner: a function of the handle's facts, the call's arguments and the lab / test overrides of the environment.
// Returns 0 and the plan; 1 when the two-pass engine must take the batch; 4 when a count call's full-size regions are beyond the
// bound (the caller counts in document ranges).  A plan with want_pair && !direct is not to be run: the pair engine's chunk gave
// regions beyond the temp bound, and the caller plans again without that engine.
static int32_t plan_v2(const aha_ac *ac, const MatchArgs &M1, V2Mode mode, V2Plan &P) {
  const uint64_t N = M1.n_bytes;
  const uint32_t Lmax = ac->aut.max_key_len;
  // a count call (device_count): full-size regions -- sized from the text, there is no capacity -- and the count passes instead
  // of the expansion; where they are beyond the bound or cannot be allocated the pass returns 4 before it launches anything,
  // and the caller counts the batch in document ranges (count_ranges)
  const bool counting = M1.count_only != 0;
  uint64_t s_min = std::max<uint64_t>(64, ((8ull * Lmax + 63) / 64) * 64);
  if (s_min > kV2MaxS) return 1;
  const char *de = getenv("AHA_DIRECT");
  uint64_t lanes = (uint64_t)ac->v2_grid * kV2Threads;
  uint64_t S = ((N + lanes - 1) / lanes + 63) / 64 * 64;
  S = std::min<uint64_t>(std::max<uint64_t>(S, s_min), kV2MaxS);
  // the prefix-filter engine: no separator filter, the event regions; a wave takes a chunk of 4, 8, 16 or 32 KiB -- the larger,
  // the fuller its batches of 64 candidates and the fewer chunks the post passes see (cfg 2 at 64 MiB: 0.136 ms with 4 KiB,
  // 0.117 with 16 KiB) -- while every wave of the device still has one, and while the image, if it fits LDS at all, still
  // fits beside the longer candidate lists.
  // (a call with char offsets: kf_filter finds out on its way whether the batch is plain ASCII -- then a character count is a
  // byte count --, otherwise kf_walk counts the continuation bytes of its chunk; the table it keeps for that counts against LDS)
  const bool filt = ac->pf_ok && !ac->unit_ok && !M1.sep && !M1.no_filter && mode != kSlabs && !(de && strcmp(de, "0") == 0);
  if (filt) {
    S = 4096;
    while (S < kV2MaxS && N / (2 * S) >= (uint64_t)ac->pf_cus * 16 &&
           (filter_image_in_lds(ac->n_slots, (uint32_t)(2 * S), M1.chars != 0) || !filter_image_in_lds(ac->n_slots, 4096, M1.chars != 0)))
      S *= 2;
    if (const char *fc = getenv("AHA_FILTER_CHUNK")) {  // the tests' way to the larger chunks without a batch of 128+ MiB
      const long v = atol(fc);
      if (v == 4096 || v == 8192 || v == 16384 || v == 32768) S = (uint64_t)v;
    }
  }
  // the pair engine (scan_pair.hip): byte offsets, no separator filter, the event regions with its tile as the chunk
  const bool want_pair = ac->pair_ok && !M1.chars && !M1.sep && !M1.no_pair && mode != kSlabs && N >= 64 && !(de && strcmp(de, "0") == 0) &&
                         ac->pair_off.load(std::memory_order_relaxed) < 3;
  if (want_pair) S = pair_tile_bytes();
  const uint64_t n_chunks = (N + S - 1) / S;
  if (n_chunks > 0xFFFFFFFFull) return 1;
  // plain mode (byte offsets or char offsets, no separator filter): per-chunk event regions, no sort
  const bool dense = M1.cap / 4 > N / 16;        // more than one hit per 4 input bytes expected
  const bool sparse = M1.cap < 16ull * n_chunks;  // fewer than 16 hits per chunk expected
  if (de && strcmp(de, "0") == 0) mode = kSlabs;
  // (the character-level engine leaves its events wave by wave and expands them group by group: its cost follows the
  // events too, so a handle that has it keeps the regions for sparse batches)
  if (M1.sep || (mode == kRegions && sparse && !ac->unit_ok && !filt)) mode = kSlabs;
  if (mode == kRegions && dense) mode = kFullRegions;
  if (counting) mode = kFullRegions;
  uint64_t stride = S;
  // twice the average the caller allows for, plus a slack of 1/64 of the chunk (64 events at 4 KiB): 16 bytes per hit of
  // capacity + 1/8 byte per input byte
  if (mode == kRegions) stride = std::min<uint64_t>(S, 2 * (M1.cap / n_chunks) + std::max<uint64_t>(16, S / 64));
  const uint64_t rec_bytes = want_pair ? 8 : (ac->unit_ok ? (ac->unit_fused ? 12 : 20) : 8);
  if (counting) {
    // (AHA_COUNT_REGION_BYTES: a lower bound for the tests, which reach the document ranges with small batches)
    const char *rb = getenv("AHA_COUNT_REGION_BYTES");
    const uint64_t bound = rb && atoll(rb) > 0 ? std::min<uint64_t>((uint64_t)atoll(rb), kV2MaxRegionBytes) : kV2MaxRegionBytes;
    if (n_chunks * stride * rec_bytes > bound) return 4;
  }
  if (mode != kSlabs && n_chunks * stride * rec_bytes > kV2MaxRegionBytes) mode = kSlabs;
  const bool direct = mode != kSlabs;
  const uint64_t waves = (uint64_t)ac->v2_grid * (kV2Threads / 64);
  const uint64_t ev_cap = direct ? 0 : ((M1.cap + waves * kV2Slab + kV2Slab) / kV2Slab) * kV2Slab;
  const bool chars = M1.chars != 0, pair = want_pair && direct;
  // byte offsets through the event regions: the character-level traversal where the key set has a unit image
  const bool unit = ac->unit_ok && direct && !pair;
  // ... started only at the marks of a first, stateless pass where the handle has the filter for it (byte offsets)
  // (not a batch below one piece of the marking pass: its lanes ask for 16-byte windows wherever they stand)
  const bool skip = unit && ac->skip_ok && !chars && N >= 64;
  // deep candidates the pair engine has room for (cfg 3: one per ~120 bytes), in segments of its waves: 256 each at least
  const uint64_t cand_cap = pair ? std::max<uint64_t>(N / 48 + 4096, waves * 256) : 0;
  P = V2Plan{mode, direct, dense, filt, want_pair, pair, unit, skip, S, n_chunks, stride, rec_bytes, ev_cap, cand_cap, {}};
  if (want_pair && !direct) return 0;  // (regions beyond the temp bound: the chunk was the pair engine's)
  const uint64_t n_slabs = ev_cap / kV2Slab + 2;
  const uint64_t n_blk = std::max<uint64_t>((n_chunks + 255) / 256, (ev_cap + 255) / 256) + 2;
  const uint64_t n_reg = direct ? n_chunks * stride : 0;
  const uint64_t n_docs1 = M1.n_docs + 1;
  size_t *z = P.sizes;
  z[kEv] = z[kSortedEv] = ev_cap * 16;
  z[kSortedCnt] = ev_cap * 4;
  z[kSlabUsed] = direct ? 0 : n_slabs * 4;
  z[kEvCnt] = n_chunks * 4;
  z[kDocEvRank] = n_docs1 * 4;
  z[kEvBase] = n_chunks * 8;
  z[kBlkA] = z[kBlkB] = n_blk * 8;
  z[kCursor] = kCursorBytes;
  z[kEvAux] = z[kSortedAux] = chars ? ev_cap * 4 : 0;
  z[kLeadCnt] = z[kChunkDoc0] = (chars || pair) ? n_chunks * 4 : 0;
  z[kDocLeadRank] = chars ? n_docs1 * 4 : 0;
  z[kLeadBase] = chars ? n_chunks * 8 : 0;
  z[kEvRegions] = (unit && ac->unit_fused) ? 0 : n_reg * 8;
  z[kText] = 0;  // (the callers' and stage_folded's)
  z[kChunkHits] = direct ? n_chunks * 4 : 0;
  z[kHitBase] = direct ? n_chunks * 8 : 0;
  z[kDocHitRank] = unit ? n_docs1 * 4 : 0;
  z[kEvGroups] = unit ? n_reg * 12 : 0;
  z[kEngineA] = filt ? ((N + 63) / 64 + 2) * 8 : (skip ? skip_bitmap_bytes(N) : (pair ? n_chunks * 4 : 0));
  z[kEngineB] = filt ? n_chunks * filter_chunk_rec_bytes() : (pair ? pair_cand_bytes(cand_cap) : 0);
  z[kEngineC] = pair ? pair_walk_bytes(cand_cap) : 0;
  z[kKeyVisits] = 0;  // (device_count's)
  return 0;
}

// Bind and launch: the plan's scratch reserved and bound to the kernels' arguments, the counter block's phase, the traversal
// and the post passes on the stream.  AHA_OK: everything is launched, M is what the kernels got; kNoRegions: no room for the
// event regions (someone else holds the HBM), nothing was launched -- the slab pipeline needs far less temp.
constexpr int32_t kNoRegions = 5;
static int32_t launch_v2(aha_ac *ac, Scratch *sc, MatchArgs &M1, const V2Plan &P, V2Args &M, bool prof, hipStream_t s) {
  const uint64_t N = M1.n_bytes;
  const bool counting = M1.count_only != 0, direct = P.direct, filt = P.filt, pair = P.pair, unit = P.unit, skip = P.skip;
  M = V2Args{};
  M.doc_off = M1.doc_off;
  M.n_docs = M1.n_docs;
  M.n_bytes = N;
  M.S = (uint32_t)P.S;
  M.n_chunks = P.n_chunks;
  M.lds_slots = ac->v2_lds_slots;
  M.chars = M1.chars;
  M.sep = M1.sep;
  memcpy(M.sep_block, M1.sep_block, sizeof(M.sep_block));
  M.out = M1.out;
  M.cap = M1.cap;
  M.doc_hit_off = M1.doc_hit_off;
  M.unit_bb = ac->unit.base_bits;
  M.direct = direct ? 1 : 0;
  M.dense_hits = P.dense ? 1 : 0;
  M.ev_stride = (uint32_t)P.stride;
  M.ev_cap = P.ev_cap;
  int32_t rc;
  for (int i = 0; i < kV2Count; i++) {
    if (!P.sizes[i]) continue;
    if ((rc = v2_reserve(sc, (V2Slot)i, P.sizes[i]))) return ((i == kEvRegions || i == kEvGroups) && P.mode != kSlabs) ? kNoRegions : rc;
  }
  if (M1.fold && (!filt || M1.fold >= 2) && (rc = stage_folded(ac, sc, M1, s))) return rc;
  const bool fold_loads = filt && M1.fold;  // (the filter engine on the caller's own text: the ASCII fold only)
  auto at = [sc](V2Slot slot) { return sc->v2buf[slot].p; };
  M.text = M1.text;
  M.ev = (uint4 *)at(kEv);
  M.sorted_ev = (uint4 *)at(kSortedEv);
  M.sorted_cnt = (uint32_t *)at(kSortedCnt);
  M.slab_used = (uint32_t *)at(kSlabUsed);
  M.ev_cnt = (uint32_t *)at(kEvCnt);
  M.doc_ev_rank = (uint32_t *)at(kDocEvRank);
  M.ev_base = (uint64_t *)at(kEvBase);
  M.blk_a = (uint64_t *)at(kBlkA);
  M.blk_b = (uint64_t *)at(kBlkB);
  if (sc->cursor_buf != at(kCursor)) {  // (a new buffer: nothing is known about its words)
    sc->cursor_buf = at(kCursor);
    sc->cursor_dirty = true;
  }
  M.ev_aux = (uint32_t *)at(kEvAux);
  M.sorted_aux = (uint32_t *)at(kSortedAux);
  M.lead_cnt = (uint32_t *)at(kLeadCnt);
  M.chunk_doc0 = (uint32_t *)at(kChunkDoc0);
  M.doc_lead_rank = (uint32_t *)at(kDocLeadRank);
  M.lead_base = (uint64_t *)at(kLeadBase);
  M.evd = (uint2 *)at(kEvRegions);
  M.evg = (uint32_t *)at(kEvGroups);
  M.doc_hit_rank = (uint32_t *)at(kDocHitRank);
  M.chunk_hits = (uint32_t *)at(kChunkHits);
  M.hit_base = (uint64_t *)at(kHitBase);
  if ((rc = ensure_h_v2(ac, sc))) return rc;
  // the region pipelines' last kernel -- the per-document offsets -- leaves the host's five words itself
  M.publish = (direct && M.doc_hit_off && sc->h_v2_dev) ? sc->h_v2_dev : nullptr;
  // the call's counter block; the kernel that publishes also clears the other block for the next call
  static const bool always_clear = getenv("AHA_CURSOR_MEMSET") != nullptr;  // (lab: the memset in front of every call, as before round 6)
  if (sc->cursor_dirty || always_clear) {
    HIPCHK(ac, hipMemsetAsync(at(kCursor), 0, kCursorBytes, s));
    sc->cursor_phase = 0;
  }
  M.cursor = (unsigned long long *)at(kCursor) + 16 * sc->cursor_phase;
  M.totals = (uint64_t *)M.cursor + 2;
  M.clear_next = M.publish ? (unsigned long long *)at(kCursor) + 16 * (sc->cursor_phase ^ 1u) : nullptr;
  sc->cursor_dirty = true;  // (until this call has run to its end)

  // device-resident offsets nobody has looked at yet: validated here, in front of the traversal; a bad verdict lands in
  // cursor[1], where the traversal and every post pass look first (no read-back before the launch: -30 us per call)
  if (M1.check_docs) launch_check_docs(M.doc_off, M.n_docs, N, nullptr, M.cursor + 1, s);
  if (M1.kc_visits) HIPCHK(ac, hipMemsetAsync(M1.kc_visits, 0, (size_t)ac->aut.n_keys * 8, s));  // (this pass's events only)
  if (prof) HIPCHK(ac, hipEventRecord(sc->ev[0], s));
  const uint64_t n_tiles = (M.n_chunks + kV2Threads - 1) / kV2Threads;
  DevAut post = ac->dev;
  if (pair) {
    post.end_info = ac->d_unit_end_info;  // its deep events carry bases of the unit image
    post.compact = 1;
    pair_launch(ac->pdev, ac->udev, post, M, at(kEngineA), at(kEngineB), at(kEngineC), P.cand_cap, ac->v2_grid,
                prof ? (void *)sc->ev[2] : nullptr, s);  // (profiling only: ms_count = the pair pass, ms_scan = the deep walks)
  } else if (unit) {
    post.end_info = ac->d_unit_end_info;  // events carry bases of the unit image
    post.compact = 1;
    if (skip) {
      skip_launch_mark(ac->sdev, M, at(kEngineA), ac->v2_grid, s);
      if (prof) HIPCHK(ac, hipEventRecord(sc->ev[2], s));  // (profiling only: ms_count = the marks, ms_scan = the walk)
      skip_launch_traverse(ac->udev, M, at(kEngineA), (uint32_t)std::min<uint64_t>(ac->v2_grid, n_tiles), s);
    } else {
      unit_launch_traverse(ac->udev, M, (uint32_t)std::min<uint64_t>(ac->v2_grid, n_tiles), s);
    }
  } else if (filt) {
    // filter (one bit per byte position), then the candidates' goto walks, a wave per chunk
    unsigned long long *non_ascii = M1.chars ? M.cursor + 6 : nullptr;
    (fold_loads ? filter_launch_filter_fold : filter_launch_filter)(ac->fdev, M, at(kEngineA), at(kEngineB), non_ascii, ac->pf_cus, s);
    if (prof) HIPCHK(ac, hipEventRecord(sc->ev[2], s));  // (profiling only: ms_count = the filter, ms_scan = the walks)
    (fold_loads ? filter_launch_walk_fold : filter_launch_walk)(ac->dev, M, at(kEngineA), at(kEngineB), non_ascii, ac->pf_cus, s);
  } else {
    v2_launch_traverse(ac->dev, M, (uint32_t)std::min<uint64_t>(ac->v2_grid, n_tiles), s);
  }
  if (prof) HIPCHK(ac, hipEventRecord(sc->ev[1], s));
  if (counting) {
    // the count path: the hits per chunk and their scan as in a match (total, documents' offsets), the events per head key
    // instead of the expansion, then the chains (scan_count.hip)
    const unsigned long long *abortf = (const unsigned long long *)(M.cursor + 1);
    // workgroups of the visit count: four per CU.  The kernel is bound by its LDS table's atomics, not by the flushes' global
    // adds: 64 / 256 / 1024 workgroups took 4.29 / 1.09 / 0.71 ms on cfg 3 at 1 GiB (AHA_COUNT_BLOCKS: lab)
    static const long count_blocks_env = getenv("AHA_COUNT_BLOCKS") ? atol(getenv("AHA_COUNT_BLOCKS")) : 0;
    const uint32_t count_blocks = count_blocks_env > 0 ? (uint32_t)count_blocks_env : 4u * ac->v2_grid;
    // a cover call: the mask cleared (unless the pass was aborted), then one span per event from the same records
    uint64_t *cdoc = nullptr;
    if (M1.cover_mask) {
      if (!(cdoc = (uint64_t *)cover_reserve(sc, kCovChunkDoc, (M.n_chunks + 1) * 8))) {
        tls_err = "hipMalloc failed for the scratch of a cover call";
        return AHA_E_HIP;
      }
      if (M1.cover_clear) cover_launch_clear(M1.cover_mask, (N + 31) / 32, abortf, ac->post_blocks ? ac->post_blocks : 8u * ac->v2_grid, s);
    }
    if (unit && ac->unit_fused) {
      v2_launch_hit_scan(M, s);
      if (prof) HIPCHK(ac, hipEventRecord(sc->ev[3], s));
      if (M1.kc_visits) count_launch_visits(post, M, ac->d_unit_end, M1.kc_visits, count_blocks, s);
      if (cdoc) cover_launch_spans(post, M, ac->d_unit_end, cdoc, M1.cover_mask, M1.cover_bit0, count_blocks, s);
    } else {
      if (unit) unit_launch_regroup(post, M, s);
      v2_launch_count_post(post, M, s, unit || filt || pair);
      if (prof) HIPCHK(ac, hipEventRecord(sc->ev[3], s));
      if (M1.kc_visits) count_launch_visits(post, M, nullptr, M1.kc_visits, count_blocks, s);
      if (cdoc) cover_launch_spans(post, M, nullptr, cdoc, M1.cover_mask, M1.cover_bit0, count_blocks, s);
    }
    if (M1.kc_visits) count_launch_chain(ac->dev.key_ln, ac->aut.n_keys, M1.kc_visits, M1.kc_out, abortf, s);
    if (unit && ac->unit_fused)
      unit_launch_doc_offsets(M, s);
    else
      v2_launch_doc_offsets(post, M, s);
  } else if (direct) {
    // (no event between the traversal and the post passes of this pipeline: a record costs ~5 us of stream time, and ev[1]
    // stands for ev[2] in the timing below)
    if (unit && ac->unit_fused) {  // the traversal counted the hits: bases, then the expansion straight from the wave-ordered events
      v2_launch_hit_scan(M, s);
      if (M.chars) v2_launch_lead_scan(M, s);  // characters before every chunk (the traversal counted them per chunk)
      if (prof) HIPCHK(ac, hipEventRecord(sc->ev[3], s));
      unit_launch_expand(M.chars ? ac->d_unit_end_chars : ac->d_unit_end, post, M, 2u * ac->v2_grid, s);
    } else {
      if (unit) unit_launch_regroup(post, M, s);  // the wave-ordered events back into the chunks' regions, counted
      v2_launch_direct_post(post, M, s, prof ? (void *)sc->ev[3] : nullptr, unit || filt || pair);  // (kf_walk and kp_pairs count like ku_regroup)
    }
  } else {
    v2_launch_chunk_scan(M, s);
    if (prof) HIPCHK(ac, hipEventRecord(sc->ev[2], s));
    v2_launch_sort(ac->dev, M, M.ev_cap, s);
    if (prof) HIPCHK(ac, hipEventRecord(sc->ev[3], s));
    v2_launch_expand(ac->dev, M, M.ev_cap, s);
  }
  if (prof) HIPCHK(ac, hipEventRecord(sc->ev[4], s));
  HIPCHK(ac, hipGetLastError());
  return AHA_OK;
}

// The verdict: the call's five words read back, cursor[1] mapped to what match_v2 returns, the pair engine's give-ups counted,
// the timing published.
static int32_t verdict_v2(aha_ac *ac, Scratch *sc, MatchArgs &M1, const V2Plan &P, const V2Args &M, bool prof, hipStream_t s,
                          uint64_t *n_hits) {
  const bool counting = M1.count_only != 0, direct = P.direct, filt = P.filt, pair = P.pair, unit = P.unit, skip = P.skip;
  [[maybe_unused]] const uint64_t N = M1.n_bytes;  // (the lab blocks below)
  if (M.publish) {
    // (done by k2d_doc_offsets / ku_doc_offsets)
  } else if (sc->h_v2_dev) {
    launch_publish_words((const unsigned long long *)M.cursor, sc->h_v2_dev, 5, s);
  } else {
    HIPCHK(ac, hipMemcpyAsync(sc->h_v2, M.cursor, 5 * 8, hipMemcpyDeviceToHost, s));
  }
  HIPCHK(ac, hipStreamSynchronize(s));
  if (M.clear_next) {  // every kernel of the call has run: the other block is clear
    sc->cursor_dirty = false;
    sc->cursor_phase ^= 1u;
  }
#ifdef AHA_EXPAND_CLK
  {  // (lab: the dense expansion's phases, clock cycles summed over the sampled chunks' waves)
    unsigned long long w[16];
    (void)hipMemcpy(w, M.cursor, sizeof(w), hipMemcpyDeviceToHost);
    if (w[15])
      fprintf(stderr, "k2d_expand_dense, %llu sampled chunks, %.1f windows each; cycles per window: A %.0f  B2 %.0f  wait %.0f  fill %.0f  wall-clock ticks of 10 ns per chunk %.0f; clocks per chunk %.0f\n",
              w[15], (double)w[13] / w[15], (double)w[8] / w[13], (double)w[9] / w[13], (double)w[10] / w[13], (double)w[11] / w[13], (double)w[12] / w[15],
              (double)w[14] / w[15]);
    if (w[7]) fprintf(stderr, "  blocks sampled %llu: %.1f chunks each, %.0f clocks from the kernel's first instruction to its stores' acknowledgement\n", w[7], (double)w[6] / w[7], (double)w[5] / w[7]);
  }
#endif
#ifdef AHA_SK_STATS
  if (skip) {
    unsigned long long w[16];
    (void)hipMemcpy(w, M.cursor, sizeof(w), hipMemcpyDeviceToHost);
    fprintf(stderr, "ks_traverse: %llu lane-trips (%.4f per byte), %llu jumps, %llu fresh, %llu wave-trips (%.1f %% of the lane slots used)\n", w[8],
            (double)w[8] / (double)N, w[9], w[11], w[10], 100.0 * (double)w[8] / (64.0 * (double)w[10]));
  }
#endif
  if (sc->h_v2[1] >= 16) return bad_offsets(sc->h_v2[1] & 1);  // (k_check_docs: nothing was indexed with them)
  if (sc->h_v2[1] == 3 && pair) {  // the pair engine gave the batch up (documents of a few bytes, a piece dense with events): engine 4 takes it
    if (!counting && !M1.neutral) ac->pair_off.fetch_add(1, std::memory_order_relaxed);  // (three times: the handle stops trying; a count call
                                                                           // leaves the handle's history as it found it)
    M1.no_pair = 1;
  }
  if (sc->h_v2[1] == 3) return 3;  // the prefix-filter engine gave up (candidates too dense, nested keys): the caller repeats without it
                                   // (check_docs stays set: the repeat validates the offsets again -- 5 us -- rather than trust
                                   // that no plain store of a hand-back overwrote a bad verdict)
  M1.check_docs = 0;  // (looked at: a repeated pass or the two-pass engine need not look again)
  if (sc->h_v2[1] == 2) return 2;  // a chunk's event region overflowed: the caller repeats with full-size regions
  if (sc->h_v2[1]) return 1;  // event temp exhausted (cap too small): exact count via the two-pass engine
  *n_hits = sc->h_v2[2];
  if (prof) {  // (the events were recorded)
    aha_timing t{};
    t.engine = pair ? 7 : (skip ? 6 : (unit ? 4 : (filt ? 5 : 2)));
    t.chunk_bytes = M.S;
    t.n_kernels = 9;
    t.n_chunks = M.n_chunks;
    t.n_hits = *n_hits;
    // an engine with a pass in front of its traversal (filter, marks, pairs): ms_count is that pass, ms_scan the traversal
    const bool front = filt || skip || pair;
    if (direct)
      publish_event_timing(ac, sc, t, front ? 2 : 1, front ? 2 : -1, 1, 1, 3);
    else
      publish_event_timing(ac, sc, t, front ? 2 : 1, 1, 2, 2, 3);
  }
  return AHA_OK;
}

// One pass over a batch through the engine and pipeline the planner picks for `mode`.  Returns AHA_OK, an error, +1 when the
// caller must fall back to the two-pass engine, +2 when a region overflowed, +3 when the prefix-filter or the pair engine
// handed the batch back, +4 when a count call's regions do not fit (count_ranges).
static int32_t match_v2(aha_ac *ac, Scratch *sc, MatchArgs &M1, hipStream_t s, uint64_t *n_hits, V2Mode mode) {
  for (;;) {
    V2Plan P;
    int32_t rc = plan_v2(ac, M1, mode, P);
    if (rc) return rc;
    if (P.want_pair && !P.direct) {  // the same pipeline, planned again without the pair engine and its chunk
      M1.no_pair = 1;
      mode = P.mode;
      continue;
    }
    V2Args M;
    const bool prof = ac->profiling.load() && sc->ev_ready;  // (read once per pass: the verdict times what the launch recorded)
    rc = launch_v2(ac, sc, M1, P, M, prof, s);
    if (rc == kNoRegions) {  // planned again as the slab pipeline; a count call has none: document ranges
      if (M1.count_only) return 4;
      mode = kSlabs;
      continue;
    }
    if (rc) return rc;
    return verdict_v2(ac, sc, M1, P, M, prof, s, n_hits);
  }
}

// the events of a scratch set are created by the first profiled call that leases it
int32_t ready_events(aha_ac *ac, Scratch *sc) {
  if (!ac->profiling.load() || sc->ev_ready) return AHA_OK;
  // (timing only -- nothing synchronizes with them, the call ends in hipStreamSynchronize --: created without the system-scope
  // fence of a default event, i.e. without a cache write-back and invalidation between the kernels they stand between.  A
  // 64 MiB call of cfg 2: 86 us against 89.5 with the fences (AHA_EVENT_FENCE=1) -- and 65 without any events: the five
  // records themselves cost ~4 us each, profiles/r06_cfg2_fixed_costs.txt)
  static const unsigned ev_flags = getenv("AHA_EVENT_FENCE") ? hipEventDefault : hipEventDisableSystemFence;
  for (auto &e : sc->ev) HIPCHK(ac, hipEventCreateWithFlags(&e, ev_flags));
  sc->ev_ready = true;
  return AHA_OK;
}

// the offsets live in HBM: one small kernel and an 4-byte read-back before anything indexes with them (open_call, where no
// single-traversal pass validates them on the device; device_records)
static int32_t check_docs_now(aha_ac *ac, Scratch *sc, const uint64_t *d_doc_offsets, uint64_t n_docs, uint64_t n_bytes,
                              hipStream_t s) {
  int32_t rc2;
  if ((rc2 = v2_reserve(sc, kCursor, kCursorBytes))) return rc2;
  if ((rc2 = ensure_h_v2(ac, sc))) return rc2;
  uint32_t *flag = (uint32_t *)sc->v2buf[kCursor].p + 64;  // (the third block: odd words)
  HIPCHK(ac, hipMemsetAsync(flag, 0, 4, s));
  launch_check_docs(d_doc_offsets, n_docs, n_bytes, flag, nullptr, s);
  HIPCHK(ac, hipMemcpyAsync(sc->h_v2, flag, 4, hipMemcpyDeviceToHost, s));
  HIPCHK(ac, hipStreamSynchronize(s));
  const uint32_t bad = (uint32_t)sc->h_v2[0];
  return (bad & 3u) ? bad_offsets(bad & 1u) : AHA_OK;
}

// What device_match and device_count open with.  The checks of the arguments they share (args_ok: the family's own, given its
// place among them), the device, the parameters into M, the events; `decide(M, longest)` is the family's say once the parameters
// are known -- below 0 its refusal, 1 where a single-traversal pass will validate unchecked offsets on the device in front of
// its traversal (match_v2), 0 where the verdict is read back here (check_docs_now) --; d_zero[0 .. zero_bytes) is cleared once
// the offsets stand (a count call's key counts); an empty batch is answered (`done`), any other gets its text (take_text).
struct Opening {
  std::optional<DeviceGuard> g;
  MatchArgs M{};
  int longest = 0;
  bool done = false;  // an empty batch: the documents' hit offsets are cleared, the stream has run, the call returns AHA_OK
};
template <class Decide>
static int32_t open_call(aha_ac *ac, Scratch *sc, const Batch &B, bool args_ok, uint64_t *d_doc_hit_off, uint64_t *n_hits, CallOpt opt,
                         Decide decide, void *d_zero, size_t zero_bytes, Opening &O) {
  if (!ac || !n_hits || !B.doc_off) return AHA_E_INVALID;
  if (ac->device < 0) return no_device();
  if (!args_ok) return AHA_E_INVALID;
  O.g.emplace(ac->device);
  hipStream_t s = B.stream;
  MatchArgs &M = O.M;
  int32_t rc = fill_params(ac, B.params, M, &O.longest);
  if (rc) return rc;
  const int32_t defer = decide(M, O.longest);
  if (defer < 0) return defer;
  if ((rc = ready_events(ac, sc))) return rc;
  if (has(opt, CallOpt::kQuiet)) M.no_filter = M.no_pair = 1;  // (neither engine that keeps a history of hand-backs)
  M.neutral = has(opt, CallOpt::kNeutral) ? 1 : 0;
  *n_hits = 0;
  if (!B.checked && !defer && (rc = check_docs_now(ac, sc, B.doc_off, B.n_docs, B.n_bytes, s))) return rc;
  M.check_docs = (!B.checked && defer) ? 1 : 0;
  if (d_zero) HIPCHK(ac, hipMemsetAsync(d_zero, 0, zero_bytes, s));
  if (B.n_bytes == 0) {
    if (d_doc_hit_off) HIPCHK(ac, hipMemsetAsync(d_doc_hit_off, 0, (B.n_docs + 1) * sizeof(uint64_t), s));
    HIPCHK(ac, hipStreamSynchronize(s));
    O.done = true;
    return AHA_OK;
  }
  if (!B.text) return AHA_E_INVALID;
  M.doc_off = B.doc_off;
  M.n_docs = B.n_docs;
  M.n_bytes = B.n_bytes;
  return take_text(ac, sc, B.text, B.n_bytes, M, s, has(opt, CallOpt::kAsIs));
}

// the verdict of a match once the hits are counted
static int32_t fits(uint64_t n_hits, uint64_t cap) {
  if (n_hits <= cap) return AHA_OK;
  tls_err = "output buffer too small";
  return AHA_E_CAPACITY;
}

// match_longest: count -> scan -> write, like the two-pass engine (kernels.hip)
static int32_t match_longest_pass(aha_ac *ac, Scratch *sc, MatchArgs &M, int longest, hipStream_t s, uint64_t *n_hits) {
  int32_t rc;
  if ((rc = stage_folded(ac, sc, M, s))) return rc;
  int mode = longest == 1 ? 1 : (M.chars ? 3 : 2);
  if ((rc = two_pass_totals(ac, sc))) return rc;
  if (mode == 2) {
    // the chunked form is exact only for text without NUL bytes (kernels.hip, k_has_nul): look first
    HIPCHK(ac, hipMemsetAsync(d_totals(sc), 0, 2 * sizeof(uint64_t), s));
    launch_has_nul(M.text, M.n_bytes, d_totals(sc) + 1, s);
    HIPCHK(ac, hipMemcpyAsync(sc->h_totals, d_totals(sc), 2 * sizeof(uint64_t), hipMemcpyDeviceToHost, s));
    HIPCHK(ac, hipStreamSynchronize(s));
    M.has_nul = sc->h_totals[1] ? 1 : 0;  // the chunks' warm-ups then reach back past the NULs they cross (kernels.hip)
  }
  two_pass_chunks(ac, M, 1024, 16);  // the warm-up is 2 * Lmax
  uint64_t n_blocks;
  if ((rc = bind_two_pass(ac, sc, M, mode == 2 ? M.n_chunks : M.n_docs + 1, &n_blocks))) return rc;
  const int chars = M.chars;
  if ((rc = ensure_stale(ac))) return rc;
  launch_longest(ac->dev_longest, M, mode, false, s);
  if (mode == 2 && M.has_nul) {  // a chunk whose warm-up would not end (a NUL every few bytes) gave up: document by document
    HIPCHK(ac, hipMemcpyAsync(sc->h_totals, d_totals(sc), 2 * sizeof(uint64_t), hipMemcpyDeviceToHost, s));
    HIPCHK(ac, hipStreamSynchronize(s));
    if (sc->h_totals[1] == 2) {
      mode = 3;
      if ((rc = bind_two_pass(ac, sc, M, M.n_docs + 1, &n_blocks))) return rc;
      launch_longest(ac->dev_longest, M, mode, false, s);
    }
  }
  M.chars = 0;  // the block scan has no lead counts to scan here
  launch_scan_blocks(M, n_blocks, s);
  M.chars = chars;
  launch_longest(ac->dev_longest, M, mode, true, s);
  HIPCHK(ac, hipGetLastError());
  HIPCHK(ac, hipMemcpyAsync(sc->h_totals, d_totals(sc), 2 * sizeof(uint64_t), hipMemcpyDeviceToHost, s));
  HIPCHK(ac, hipStreamSynchronize(s));
  *n_hits = sc->h_totals[0];
  return fits(*n_hits, M.cap);
}

// The single-traversal ladder: the prefix filter's back-off, the pass, once more behind a hand-back, full-size regions behind
// an overflow, slabs.  AHA_OK, an error, or 1: the two-pass engine takes the batch (*repeats: the passes thrown away so far).
static int32_t single_traversal_ladder(aha_ac *ac, Scratch *sc, MatchArgs &M, CallOpt opt, hipStream_t s, uint64_t *n_hits,
                                       uint32_t *repeats) {
  const bool quiet = has(opt, CallOpt::kQuiet), neutral = has(opt, CallOpt::kNeutral);
  // a handle whose batches keep coming back from the prefix-filter engine (text dense with key starts) skips it for 2, 4,
  // .. 64 calls before it tries again: a batch that is handed back has paid for the filter and part of the walks
  const int pm = M.chars ? 1 : 0;  // (calls with char offsets keep their own count)
  if (ac->pf_ok && neutral) {  // (as the next match call would, without counting down)
    if (ac->pf_skip[pm].load(std::memory_order_relaxed)) M.no_filter = 1;
  } else if (ac->pf_ok && !quiet) {  // (calls on one handle may run side by side: the count goes down by compare-exchange, never below 0)
    uint32_t v = ac->pf_skip[pm].load(std::memory_order_relaxed);
    while (v && !ac->pf_skip[pm].compare_exchange_weak(v, v - 1, std::memory_order_relaxed)) {
    }
    if (v) M.no_filter = 1;
  }
  const bool tried = ac->pf_ok && !M.no_filter;
  int32_t rc = match_v2(ac, sc, M, s, n_hits, kRegions);
  if (rc == 3) {  // the prefix-filter engine handed the batch back: once more on the byte-level engine
    (*repeats)++;
    M.no_filter = 1;
    if (!neutral) {
      const uint32_t streak = std::min(ac->pf_streak[pm].fetch_add(1, std::memory_order_relaxed) + 1, 6u);
      ac->pf_skip[pm].store(1u << streak, std::memory_order_relaxed);
    }
    rc = match_v2(ac, sc, M, s, n_hits, kRegions);
  } else if (tried && rc == AHA_OK && !neutral) {
    ac->pf_streak[pm].store(0, std::memory_order_relaxed);
  }
  if (rc == 2) {  // denser than cap said: regions of one event per byte
    (*repeats)++;
    rc = match_v2(ac, sc, M, s, n_hits, kFullRegions);
  }
  if (rc == 3) {
    M.no_filter = 1;
    rc = match_v2(ac, sc, M, s, n_hits, kFullRegions);
  }
  if (rc == 2) rc = match_v2(ac, sc, M, s, n_hits, kSlabs);  // (not reached: full-size regions cannot overflow)
  if (rc == AHA_OK && *repeats) note_repeats(ac, *repeats);
  if (rc < 0) return rc;
  if (rc == AHA_OK) return fits(*n_hits, M.cap);
  *n_hits = 0;  // rc == 1: the two-pass engine
  (*repeats)++;
  if (M.check_docs && (rc = check_docs_now(ac, sc, M.doc_off, M.n_docs, M.n_bytes, s))) return rc;  // (no single-traversal pass has looked at the offsets)
  return 1;
}

// The two-pass engine: count -> scan -> write over chunks with a warm-up (kernels.hip); every batch fits it.
static int32_t two_pass_pass(aha_ac *ac, Scratch *sc, MatchArgs &M, uint32_t repeats, hipStream_t s, uint64_t *n_hits) {
  int32_t rc;
  if ((rc = stage_folded(ac, sc, M, s))) return rc;
  two_pass_chunks(ac, M, ac->chunk, 8);  // warm-up is Lmax-1 bytes per chunk
  uint64_t n_blocks;
  if ((rc = bind_two_pass(ac, sc, M, M.n_chunks, &n_blocks))) return rc;

  const bool prof = ac->profiling.load() && sc->ev_ready;
  if (prof) HIPCHK(ac, hipEventRecord(sc->ev[0], s));
  launch_count(ac->dev, M, s);
  if (prof) HIPCHK(ac, hipEventRecord(sc->ev[1], s));
  launch_scan_blocks(M, n_blocks, s);
  if (prof) HIPCHK(ac, hipEventRecord(sc->ev[2], s));
  if (M.chars) launch_docg(M, s);
  if (prof) HIPCHK(ac, hipEventRecord(sc->ev[3], s));
  launch_write(ac->dev, M, s);
  if (prof) HIPCHK(ac, hipEventRecord(sc->ev[4], s));
  HIPCHK(ac, hipGetLastError());
  HIPCHK(ac, hipMemcpyAsync(sc->h_totals, d_totals(sc), 2 * sizeof(uint64_t), hipMemcpyDeviceToHost, s));
  HIPCHK(ac, hipStreamSynchronize(s));
  *n_hits = sc->h_totals[0];
  if (prof) {
    aha_timing t{};
    t.n_kernels = M.chars ? 4 : 3;
    t.n_chunks = M.n_chunks;
    t.n_hits = *n_hits;
    t.engine = 1;
    t.chunk_bytes = M.chunk;
    t.repeats = repeats;
    publish_event_timing(ac, sc, t, 1, 1, 2, 2, 3);
  }
  return fits(*n_hits, M.cap);
}

// One device-resident batch matched: the opening, then the engine that takes it.  The single-traversal pipelines validate
// unchecked offsets on the device in front of their traversal; every other path -- an empty batch, match_longest, the two-pass
// engine -- reads the verdict back first.
int32_t device_match(aha_ac *ac, Scratch *sc, const Batch &B, const HitOut &out, uint64_t *n_hits, CallOpt opt) {
  Opening O;
  auto decide = [&](const MatchArgs &, int longest) { return (int32_t)(ac->v2_ok && !longest && B.n_bytes != 0); };
  int32_t rc = open_call(ac, sc, B, !(out.cap && !out.d_out), out.d_doc_hit_off, n_hits, opt, decide, nullptr, 0, O);
  if (rc || O.done) return rc;
  MatchArgs &M = O.M;
  M.out = out.d_out;
  M.cap = out.cap;
  M.doc_hit_off = out.d_doc_hit_off;
  if (O.longest) return match_longest_pass(ac, sc, M, O.longest, B.stream, n_hits);
  uint32_t repeats = 0;  // passes thrown away (aha_timing.repeats)
  if (ac->v2_ok && (rc = single_traversal_ladder(ac, sc, M, opt, B.stream, n_hits, &repeats)) != 1) return rc;
  return two_pass_pass(ac, sc, M, repeats, B.stream, n_hits);
}

// ---- count calls (aha_ac_count_batch*) ------------------------------------------------------------------------------
// The two-pass engine's counting form over one batch: ONE traversal (k_count with per-key adds; it notes every document's
// hits before its start within its chunk, k_count_doc_offsets adds the chunks' bases), the scan, the chain pass.
static int32_t count_two_pass(aha_ac *ac, Scratch *sc, MatchArgs M, hipStream_t s, uint64_t *n_hits, uint32_t repeats) {
  if (int32_t rcf = stage_folded(ac, sc, M, s)) return rcf;
  two_pass_chunks(ac, M, ac->chunk, 8);  // warm-up is Lmax-1 bytes per chunk
  uint64_t n_blocks;
  if (int32_t rc = bind_two_pass(ac, sc, M, M.n_chunks, &n_blocks)) return rc;
  const bool prof = ac->profiling.load() && sc->ev_ready;
  if (M.kc_visits) HIPCHK(ac, hipMemsetAsync(M.kc_visits, 0, (size_t)ac->aut.n_keys * 8, s));
  // (a cover call: the offsets have been looked at by now -- device_count -- so the mask may be touched)
  if (M.cover_mask && M.cover_clear) HIPCHK(ac, hipMemsetAsync(M.cover_mask, 0, (size_t)((M.n_bytes + 31) / 32) * 4, s));
  if (prof) HIPCHK(ac, hipEventRecord(sc->ev[0], s));
  launch_count(ac->dev, M, s);
  if (prof) HIPCHK(ac, hipEventRecord(sc->ev[1], s));
  launch_scan_blocks(M, n_blocks, s);
  if (prof) HIPCHK(ac, hipEventRecord(sc->ev[3], s));
  if (M.kc_visits) count_launch_chain(ac->dev.key_ln, ac->aut.n_keys, M.kc_visits, M.kc_out, nullptr, s);
  if (M.doc_hit_off) launch_count_doc_offsets(M, s);
  if (prof) HIPCHK(ac, hipEventRecord(sc->ev[4], s));
  HIPCHK(ac, hipGetLastError());
  HIPCHK(ac, hipMemcpyAsync(sc->h_totals, d_totals(sc), 2 * sizeof(uint64_t), hipMemcpyDeviceToHost, s));
  HIPCHK(ac, hipStreamSynchronize(s));
  *n_hits = sc->h_totals[0];
  if (prof) {
    aha_timing t{};
    t.n_kernels = 3 + (M.kc_visits ? 1 : 0) + (M.doc_hit_off ? 1 : 0);
    t.n_chunks = M.n_chunks;
    t.n_hits = *n_hits;
    t.engine = 1;
    t.chunk_bytes = M.chunk;
    t.repeats = repeats;
    publish_event_timing(ac, sc, t, 1, 1, 3, -1, -1);
  }
  return AHA_OK;
}

// One batch through the single-traversal engines' count pipeline: AHA_OK, < 0, 1 (the two-pass engine takes it: as a match
// of the batch would) or 4 (the full-size regions do not fit: count_ranges).  The handle's back-off state is read, not written.
static int32_t count_single(aha_ac *ac, Scratch *sc, MatchArgs &M, hipStream_t s, uint64_t *n_hits) {
  uint32_t repeats = 0;
  if (ac->pf_ok && ac->pf_skip[0].load(std::memory_order_relaxed)) M.no_filter = 1;  // (as the next match call would)
  int32_t rc = match_v2(ac, sc, M, s, n_hits, kFullRegions);
  for (int i = 0; i < 2 && rc == 3; i++) {  // handed back by the prefix-filter or the pair engine: once more without it
    repeats++;
    M.no_filter = 1;
    rc = match_v2(ac, sc, M, s, n_hits, kFullRegions);
  }
  if (rc == 3) rc = 1;
  if (rc == AHA_OK && repeats) note_repeats(ac, repeats);
  return rc;
}

static void *count_reserve(Scratch *sc, CountSlot slot, size_t bytes) { return reserve_ptr(sc->cntbuf[slot], bytes, kGrowQuarter); }

// The documents [d0, d1) of B cut out as a checked batch of their own: the text from the range's first byte, the offsets
// relative to it in rel_slot.  `off` is the host's copy of B.doc_off; `rel` is the host's side of the upload and stays the
// host's until B.stream has run.  The kernels read aligned 16-byte pieces: where text_slot is given and the range's first byte
// is not aligned, the range is copied there, folded on the way by mode `fold` (stage_text) -- R.text then differs from
// B.text + off[d0].  No memory for a slot: nomem_text, AHA_E_HIP.
static int32_t slice(aha_ac *ac, const Batch &B, const uint64_t *off, uint64_t d0, uint64_t d1, std::vector<uint64_t> &rel, Buf &rel_slot,
                     Buf *text_slot, Grow grow, int fold, const char *nomem_text, Batch &R) {
  auto nomem = [&] {
    tls_err = nomem_text;
    return AHA_E_HIP;
  };
  const uint64_t nd = d1 - d0, nb = off[d1] - off[d0];
  try {
    rel.resize(nd + 1);
  } catch (...) {
    return AHA_E_NOMEM;
  }
  for (uint64_t d = 0; d <= nd; d++) rel[d] = off[d0 + d] - off[d0];
  uint64_t *d_rel = (uint64_t *)reserve_ptr(rel_slot, (nd + 1) * 8, grow);
  if (!d_rel) return nomem();
  HIPCHK(ac, hipMemcpyAsync(d_rel, rel.data(), (nd + 1) * 8, hipMemcpyHostToDevice, B.stream));
  R = checked_batch(B.text + off[d0], d_rel, nd, nb, B.params, B.stream);
  if (text_slot && nb && reinterpret_cast<uintptr_t>(R.text) % 16 != 0) {
    void *t = reserve_ptr(*text_slot, nb + 64, grow);
    if (!t) return nomem();
    if (int32_t rc = stage_text(ac, &R.text, nb, t, fold, d_rel, nd, B.stream)) return rc;
  }
  return AHA_OK;
}

// A batch whose full-size regions are beyond the bound or cannot be allocated (HBM held elsewhere): counted in ranges of whole
// documents, one after another, each through the same pipeline -- the key counts add up in the caller's vector as they do
// for running totals, the documents' offsets are rebased on the host.  A range that still does not fit is halved; a single
// document that does not (its regions: up to 20 bytes per byte of a document below 2 GiB) is the only batch that goes to the
// two-pass engine's counting form here.
static int32_t count_ranges(aha_ac *ac, Scratch *sc, const MatchArgs &M0, hipStream_t s, uint64_t *n_hits) {
  const uint64_t D = M0.n_docs;
  const Batch B0 = checked_batch(M0.text, M0.doc_off, D, M0.n_bytes, nullptr, s);  // (the text as take_text left it)
  const char *nomem_text = "hipMalloc failed for a document range of a count call";
  std::vector<uint64_t> off, hd, tmp, rel;
  try {
    off.resize(D + 1);
    if (M0.doc_hit_off) hd.resize(D + 1);
  } catch (...) {
    return AHA_E_NOMEM;
  }
  HIPCHK(ac, hipMemcpyAsync(off.data(), M0.doc_off, (D + 1) * 8, hipMemcpyDeviceToHost, s));
  HIPCHK(ac, hipStreamSynchronize(s));
  uint64_t limit = std::max<uint64_t>(M0.n_bytes / 2, 1), base = 0;
  uint32_t ranges = 0;
  int32_t rc;
  // a cover call: the ranges share one mask (they run one after another on the stream, so a word two of them touch is safe);
  // it is cleared once, here -- the offsets have been validated
  if (M0.cover_mask) HIPCHK(ac, hipMemsetAsync(M0.cover_mask, 0, (size_t)((M0.n_bytes + 31) / 32) * 4, s));
  for (uint64_t d0 = 0; d0 < D;) {
    uint64_t d1 = d0 + 1;
    while (d1 < D && off[d1 + 1] - off[d0] <= limit) d1++;
    const uint64_t nd = d1 - d0, nb = off[d1] - off[d0];
    try {
      tmp.resize(nd + 1);
    } catch (...) {
      return AHA_E_NOMEM;
    }
    uint64_t *d_dho = M0.doc_hit_off ? (uint64_t *)count_reserve(sc, kCntDho, (nd + 1) * 8) : nullptr;
    if (M0.doc_hit_off && !d_dho) {
      tls_err = nomem_text;
      return AHA_E_HIP;
    }
    // the range as a batch of its own.  (A folded handle whose text is still the caller's: an unaligned range is folded on the
    // way, an aligned one stays the caller's -- the prefix-filter engine folds in its loads, the others stage it)
    Batch R;
    if ((rc = slice(ac, B0, off.data(), d0, d1, rel, sc->cntbuf[kCntRel], &sc->cntbuf[kCntText], kGrowQuarter, M0.fold, nomem_text, R)))
      return rc;
    MatchArgs Mr = M0;
    Mr.text = R.text;
    Mr.doc_off = R.doc_off;
    Mr.n_docs = nd;
    Mr.n_bytes = nb;
    Mr.doc_hit_off = d_dho;
    Mr.check_docs = 0;
    Mr.cover_bit0 = M0.cover_bit0 + off[d0];
    Mr.cover_clear = 0;
    if (R.text != M0.text + off[d0]) Mr.fold = 0;  // (staged, and folded on the way)
    uint64_t nh = 0;
    rc = AHA_OK;
    if (nb == 0) {
      if (d_dho) HIPCHK(ac, hipMemsetAsync(d_dho, 0, (nd + 1) * 8, s));
    } else {
      MatchArgs M = Mr;  // (a pass changes its arguments: the two-pass engine gets the range's own)
      rc = count_single(ac, sc, M, s, &nh);
      if (rc == 4 && nd > 1) {  // nothing was launched: the same documents in smaller ranges
        limit = std::max<uint64_t>(limit / 2, 1);
        continue;
      }
      if (rc == 4 || rc == 1) rc = count_two_pass(ac, sc, Mr, s, &nh, 1);
    }
    if (rc != AHA_OK) return rc;
    if (d_dho) {
      HIPCHK(ac, hipMemcpyAsync(tmp.data(), d_dho, (nd + 1) * 8, hipMemcpyDeviceToHost, s));
      HIPCHK(ac, hipStreamSynchronize(s));
      for (uint64_t d = 0; d <= nd; d++) hd[d0 + d] = base + tmp[d];
    }
    base += nh;
    d0 = d1;
    ranges++;
  }
  if (M0.doc_hit_off) {
    HIPCHK(ac, hipMemcpyAsync(M0.doc_hit_off, hd.data(), (D + 1) * 8, hipMemcpyHostToDevice, s));
    HIPCHK(ac, hipStreamSynchronize(s));
  }
  *n_hits = base;
  note_repeats(ac, ranges - 1);  // (aha_timing.repeats: the passes of the call beside its last one, the earlier ranges)
  return AHA_OK;
}

// The pieces of a call on a longest feed as the documents of a two-pass match_longest batch (scan_feedlongest.hip): the steps of
// device_match's match_longest branch with the feed's walks in place of the batch kernels.  Mode 2 (intersectable) takes a thread
// per chunk where the pieces are at least a chunk long on average -- below that most chunks hold a cut, a thread per piece has as
// many threads and none of them walks a warm-up (DESIGN.md 4.10 "Feed match_longest") -- and a thread per piece otherwise, as
// mode 1 always does and as a call whose chunks gave up on a NUL every few bytes does.
int32_t device_feed_longest_count(aha_ac *ac, Scratch *sc, const FeedArgs &F, FeedLongArgs &L, int longest, FeedLongPlan &P,
                                  uint64_t *n_hits, void *stream) {
  DeviceGuard g(ac->device);
  hipStream_t s = (hipStream_t)stream;
  MatchArgs &M = P.M;
  M = MatchArgs{};
  int32_t rc;
  *n_hits = 0;
  M.doc_off = F.off;
  M.n_docs = F.D;
  M.n_bytes = F.n_bytes;
  if ((rc = take_text(ac, sc, F.text, F.n_bytes, M, s))) return rc;
  if ((rc = stage_folded(ac, sc, M, s))) return rc;
  if ((rc = two_pass_totals(ac, sc))) return rc;
  L.end = (FeedLongSeq *)reserve_ptr(sc->flngbuf[kFlEnd], std::max<uint64_t>(F.D, 1) * sizeof(FeedLongSeq), kGrowEighth);
  if (!L.end) {
    tls_err = "hipMalloc failed for the scratch of a call on a longest feed";
    return AHA_E_HIP;
  }
  P.intersectable = longest == 2;
  two_pass_chunks(ac, M, 1024, 16);  // the warm-up is 2 * Lmax
  P.chunks = P.intersectable && F.n_bytes / F.D >= M.chunk;
  if (const char *walk = getenv("AHA_FEED_LONGEST_WALK")) {  // (tools/feed_longest_bench.py: both walks at every piece length)
    if (P.intersectable && !strcmp(walk, "chunks")) P.chunks = true;
    if (!strcmp(walk, "pieces")) P.chunks = false;
  }
  if (P.chunks) {
    // the chunked form is exact only for text without NUL bytes (kernels.hip, k_has_nul): look first
    HIPCHK(ac, hipMemsetAsync(d_totals(sc), 0, 2 * sizeof(uint64_t), s));
    launch_has_nul(M.text, F.n_bytes, d_totals(sc) + 1, s);
    HIPCHK(ac, hipMemcpyAsync(sc->h_totals, d_totals(sc), 2 * sizeof(uint64_t), hipMemcpyDeviceToHost, s));
    HIPCHK(ac, hipStreamSynchronize(s));
    M.has_nul = sc->h_totals[1] ? 1 : 0;
  }
  uint64_t n_blocks;
  if ((rc = bind_two_pass(ac, sc, M, P.chunks ? M.n_chunks : F.D + 1, &n_blocks))) return rc;
  if ((rc = ensure_stale(ac))) return rc;
  feedlong_launch_walk(ac->dev_longest, M, F, L, P.chunks, P.intersectable, false, s);
  if (P.chunks && M.has_nul) {  // a chunk whose warm-up would not end (a NUL every few bytes) gave up: piece by piece
    HIPCHK(ac, hipMemcpyAsync(sc->h_totals, d_totals(sc), 2 * sizeof(uint64_t), hipMemcpyDeviceToHost, s));
    HIPCHK(ac, hipStreamSynchronize(s));
    if (sc->h_totals[1] == 2) {
      P.chunks = false;
      if ((rc = bind_two_pass(ac, sc, M, F.D + 1, &n_blocks))) return rc;
      feedlong_launch_walk(ac->dev_longest, M, F, L, false, true, false, s);
    }
  }
  launch_scan_blocks(M, n_blocks, s);
  HIPCHK(ac, hipGetLastError());
  HIPCHK(ac, hipMemcpyAsync(sc->h_totals, d_totals(sc), 2 * sizeof(uint64_t), hipMemcpyDeviceToHost, s));
  HIPCHK(ac, hipStreamSynchronize(s));
  *n_hits = sc->h_totals[0];
  return AHA_OK;
}

int32_t device_feed_longest_write(aha_ac *ac, const FeedArgs &F, const FeedLongArgs &L, FeedLongPlan &P, aha_hit *d_out, uint64_t cap,
                                  uint64_t *d_pho, void *stream) {
  DeviceGuard g(ac->device);
  P.M.out = d_out;
  P.M.cap = cap;
  P.M.doc_hit_off = d_pho;
  feedlong_launch_walk(ac->dev_longest, P.M, F, L, P.chunks, P.intersectable, true, stream);
  HIPCHK(ac, hipGetLastError());
  return AHA_OK;
}

// One device-resident batch counted (aha_ac_count_batch_device): the match's engine and pipeline with the count passes in
// place of the expansion (match_v2, `counting`); document ranges where its full-size regions do not fit (count_ranges); the
// two-pass engine's counting form where a match of the batch takes that engine, and for a separator filter (a test per hit).
// Byte offsets throughout: char offsets change no count.  The handle's history (the prefix filter's back-off, the pair
// engine's give-ups) is read, never written: the next match call behaves as if this call had not happened.
int32_t device_count(aha_ac *ac, Scratch *sc, const Batch &B, uint32_t flags, uint64_t *d_key_counts, uint64_t *d_doc_hit_offsets,
                     uint64_t *n_hits, CallOpt opt, uint32_t *cover_mask) {
  Opening O;
  bool single = false;
  auto decide = [&](const MatchArgs &M, int longest) {
    if (longest) {  // (the entry points refuse it with their own texts before any device work: capi.cpp no_longest_form)
      tls_err = "count calls have no match_longest form";
      return (int32_t)AHA_E_INVALID;
    }
    single = ac->v2_ok && !M.sep && B.n_bytes != 0;
    return (int32_t)single;
  };
  // the caller's counts: cleared unless it keeps running totals (then only added to, by the passes that run to their end)
  const bool clear = d_key_counts && !(flags & AHA_COUNT_ACCUMULATE);
  int32_t rc = open_call(ac, sc, B, !(flags & ~AHA_COUNT_ACCUMULATE), d_doc_hit_offsets, n_hits, opt, decide, clear ? d_key_counts : nullptr,
                         ac ? (size_t)ac->aut.n_keys * 8 : 0, O);
  if (rc || O.done) return rc;
  hipStream_t s = B.stream;
  MatchArgs &M = O.M;
  const uint32_t K = ac->aut.n_keys;
  auto check_now = [&]() { return check_docs_now(ac, sc, B.doc_off, B.n_docs, B.n_bytes, s); };
  M.chars = 0;
  M.out = nullptr;
  M.cap = 0;
  M.doc_hit_off = d_doc_hit_offsets;
  M.count_only = 1;
  M.cover_mask = cover_mask;  // (a cover call, device_cover: every pass that runs to its end leaves its events' spans there)
  M.cover_clear = cover_mask ? 1 : 0;
  M.kc_out = reinterpret_cast<unsigned long long *>(d_key_counts);
  if (d_key_counts) {
    if (M.sep) {
      M.kc_hits = M.kc_out;  // (a test per hit: straight into the caller's counts)
    } else {
      if ((rc = v2_reserve(sc, kKeyVisits, (size_t)std::max<uint32_t>(K, 1) * 8))) return rc;
      M.kc_visits = (unsigned long long *)sc->v2buf[kKeyVisits].p;
    }
  }
  if (single) {
    const MatchArgs M0 = M;
    rc = count_single(ac, sc, M, s, n_hits);
    if (rc <= AHA_OK) return rc;
    *n_hits = 0;
    if (M.check_docs && (rc = check_now())) return rc;  // (no single-traversal pass has looked at the offsets)
    M.check_docs = 0;
    if (rc == 4) {
      MatchArgs Mr = M0;
      Mr.check_docs = 0;
      return count_ranges(ac, sc, Mr, s, n_hits);
    }
  }
  return count_two_pass(ac, sc, M, s, n_hits, single ? 1 : 0);
}


// ---- cover calls (aha_ac_cover_batch*) ---------------------------------------------------------------------------------
// One device-resident batch covered.  device_count without key counts and with a mask: the engine a match would take, document
// ranges, the two-pass engine's form for a separator filter -- each pass leaves one span per event in the mask (scan_cover.hip;
// k_count's cover mode).  Then, over the finished mask and only where asked for: the redacted copy, the documents' covered
// bytes; the total always.  Scratch beyond the count call's: N / 8 bytes where the caller gives no mask, 8 bytes per chunk,
// nothing per hit.
int32_t device_cover(aha_ac *ac, Scratch *sc, const Batch &B, uint32_t flags, uint32_t *d_mask, uint8_t *d_redacted, uint8_t fill,
                     uint64_t *d_doc_covered, uint64_t *n_covered, uint64_t *n_hits_out) {
  if (!ac || !n_covered || !B.doc_off || flags) return AHA_E_INVALID;
  if (ac->device < 0) return no_device();
  DeviceGuard g(ac->device);
  hipStream_t s = B.stream;
  const uint64_t n_docs = B.n_docs, n_bytes = B.n_bytes;
  *n_covered = 0;
  if (n_hits_out) *n_hits_out = 0;
  const uint64_t n_words = (n_bytes + 31) / 32;
  auto nomem = [&]() {
    tls_err = "hipMalloc failed for the scratch of a cover call";
    return AHA_E_HIP;
  };
  uint32_t *mask = d_mask;
  if (!mask && n_words && !(mask = (uint32_t *)cover_reserve(sc, kCovMask, n_words * 4))) return nomem();
  uint64_t *d_total = (uint64_t *)cover_reserve(sc, kCovTotal, 8);
  if (!d_total) return nomem();
  int32_t rc;
  uint64_t n_hits = 0;
  if ((rc = device_count(ac, sc, B, 0, nullptr, nullptr, &n_hits, CallOpt::kNone, mask))) return rc;
  const bool prof = ac->profiling.load();
  const auto t0 = std::chrono::steady_clock::now();
  const uint32_t blocks = post_grid(ac);
  uint64_t total = 0;
  if (n_bytes) {
    HIPCHK(ac, hipMemsetAsync(d_total, 0, 8, s));
    cover_launch_total(mask, n_words, d_total, blocks, s);
    if (d_redacted) cover_launch_redact(B.text, d_redacted, mask, n_bytes, fill, blocks, s);
    if (d_doc_covered && n_docs) cover_launch_doc_covered(mask, B.doc_off, n_docs, d_doc_covered, blocks, s);
    HIPCHK(ac, hipGetLastError());
    HIPCHK(ac, hipMemcpyAsync(&total, d_total, 8, hipMemcpyDeviceToHost, s));
  } else if (d_doc_covered && n_docs) {
    HIPCHK(ac, hipMemsetAsync(d_doc_covered, 0, n_docs * 8, s));
  }
  HIPCHK(ac, hipStreamSynchronize(s));
  *n_covered = total;
  if (n_hits_out) *n_hits_out = n_hits;
  if (prof) {  // ms_write: the passes after the traversal -- the spans (the pass's own figure) and the passes over the mask
    const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    std::lock_guard<std::mutex> lk(ac->last_mu);
    ac->last.ms_write += (float)ms;
    ac->last.n_hits = n_hits;
  }
  return AHA_OK;
}

// ---- calls that work on a hit list per range of documents: doc counts, select and replace, class counts -----------------
// Each counts first (device_count with the documents' hit offsets), cuts the batch into ranges of whole documents whose hits fit
// the family's bound (doc_ranges.hpp: the rule) and matches range after range into the family's scratch.

// The profiling book of such a call: the timing of the pass that traversed, the time of the matches, the ranges.
struct RangeBook {
  aha_ac *ac;
  bool after_match;  // t_trav is taken again after the first match (select, class counts); else the caller says when (doc counts)
  std::chrono::steady_clock::time_point t0{};
  double ms_match = 0.0;
  bool first = true;
  aha_timing t_trav{};  // the timing of a pass that traversed (profiling)
  void take() {
    if (!ac->profiling.load()) return;
    std::lock_guard<std::mutex> lk(ac->last_mu);
    t_trav = ac->last;
  }
  void begin() {
    t0 = std::chrono::steady_clock::now();
    take();
  }
  void matched(std::chrono::steady_clock::time_point t_m0) {
    ms_match += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_m0).count();
  }
  void first_done() {
    if (first) take();
    first = false;
  }
  // the engine that traversed, the call's hits; ms_write = the call from its first range on, less its matches; repeats = the
  // ranges before the last.  `to` == null: published; else handed over (SelectSink::timing: the caller publishes)
  void finish(uint64_t n_hits, size_t n_ranges, aha_timing *to) {
    if (!ac->profiling.load()) return;
    const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    t_trav.struct_size = sizeof(t_trav);
    t_trav.n_hits = n_hits;
    t_trav.ms_write = (float)std::max(0.0, ms - ms_match);
    t_trav.repeats = n_ranges ? (uint32_t)(n_ranges - 1) : 0;
    if (to)
      *to = t_trav;
    else
      publish_timing(ac, t_trav);
  }
};

// What the ranges of one call share: the caller's batch, the family's slots and their growth, its name in the messages.
struct RangeCall {
  aha_ac *ac;
  Scratch *sc;
  Batch B;
  Buf &rel_slot, &text_slot, &hits_slot;
  Grow grow;
  const char *family, *nomem_text;
  RangeBook book;
  std::vector<uint64_t> off, rel;  // the documents' offsets on the host (taken when the first range needs them); a range's own

  int32_t nomem() const {
    tls_err = nomem_text;
    return AHA_E_HIP;
  }

  // the documents' offsets on the host, fetched once
  int32_t host_offsets() {
    if (!off.empty()) return AHA_OK;
    try {
      off.resize(B.n_docs + 1);
    } catch (...) {
      return AHA_E_NOMEM;
    }
    HIPCHK(ac, hipMemcpyAsync(off.data(), B.doc_off, (B.n_docs + 1) * 8, hipMemcpyDeviceToHost, B.stream));
    HIPCHK(ac, hipStreamSynchronize(B.stream));
    return AHA_OK;
  }

  // The documents [d0, d1) as a checked batch: the caller's arrays where that is the whole batch, else their slice.
  // (the kernels read aligned 16-byte pieces; a folded handle's match and count make their own folded -- and aligned -- copy,
  // so only an unfolded handle's unaligned range is staged here)
  int32_t batch(uint64_t d0, uint64_t d1, Batch &R) {
    R = B;
    R.checked = true;  // (the count call in front has looked at the offsets)
    if (d0 == 0 && d1 == B.n_docs) return AHA_OK;
    if (int32_t rc = host_offsets()) return rc;
    if (int32_t rc = slice(ac, B, off.data(), d0, d1, rel, rel_slot, ac->fold() ? nullptr : &text_slot, grow, 0, nomem_text, R)) return rc;
    HIPCHK(ac, hipStreamSynchronize(B.stream));  // (rel is the host's until the copy has run)
    return AHA_OK;
  }

  // The range's rh hits (the count's figure) into hits_slot: every engine, the handle's back-off state read and never written.
  int32_t match(const Batch &R, uint64_t rh, aha_hit **d_hits) {
    if (!(*d_hits = (aha_hit *)reserve_ptr(hits_slot, rh * sizeof(aha_hit), grow))) return nomem();
    const auto t_m0 = std::chrono::steady_clock::now();
    uint64_t got = 0;
    if (int32_t rc = device_match(ac, sc, R, HitOut{*d_hits, rh, nullptr}, &got, CallOpt::kNeutral)) return rc;
    if (got != rh) {
      tls_err = std::string(family) + ": the match and the count of a range disagree";
      return AHA_E_HIP;
    }
    book.matched(t_m0);
    if (book.after_match) book.first_done();
    return AHA_OK;
  }
};

// ---- document counts (aha_ac_doc_counts_batch*) ----------------------------------------------------------------------
static void *dc_reserve(Scratch *sc, DocCountSlot slot, size_t bytes) {
  if (slot == kDcRows && sc->dcbuf[slot].bytes < bytes) sc->dc_rows_clear = false;  // (new rows: nothing is known about their words)
  return reserve_ptr(sc->dcbuf[slot], bytes, kGrowOrExact);
}

// One device-resident batch as {key, count} pairs per document (aha_ac_doc_counts_batch_device).
//   1. device_count without key counts: the hits per document and their total, no capacity (and the offsets' validation).
//   2. The ranges of doc_ranges.hpp (one, as a rule), each matched into the call's scratch (RangeCall, above).
//   3. Per document one of the three forms of scan_doccount.hip, chosen from its hit count; the pairs per document come back,
//      the host adds them up (the offsets, the capacity check), kdc_gather writes the pairs below the capacity.
// A single document whose hits are beyond the bound is never matched: a count call over it alone gives its key counts -- the
// dense form's row --, which are compacted like one.
int32_t device_doc_counts(aha_ac *ac, Scratch *sc, const Batch &B0, aha_key_count *d_out, uint64_t cap, uint64_t *d_doc_pair_offsets,
                          uint64_t *n_pairs, uint64_t *n_hits_out) {
  if (!ac || !n_pairs || !B0.doc_off) return AHA_E_INVALID;
  if (ac->device < 0) return no_device();
  if (cap && !d_out) return AHA_E_INVALID;
  DeviceGuard g(ac->device);
  hipStream_t s = B0.stream;
  const uint64_t D = B0.n_docs, K = ac->aut.n_keys;
  *n_pairs = 0;
  if (n_hits_out) *n_hits_out = 0;
  // byte offsets throughout: char offsets change no count
  aha_match_params pb;
  memset(&pb, 0, sizeof(pb));
  if (B0.params) memcpy(&pb, B0.params, std::min<size_t>(B0.params->struct_size, sizeof(pb)));
  pb.char_offsets = 0;
  Batch B = B0;
  B.params = B0.params ? &pb : nullptr;
  RangeCall call{ac, sc, B, sc->dcbuf[kDcRel], sc->dcbuf[kDcText], sc->dcbuf[kDcHits],
                 kGrowOrExact, "document counts", "hipMalloc failed for the scratch of a document-count call", RangeBook{ac, false}};
  auto nomem = [&]() { return call.nomem(); };
  int32_t rc;
  uint64_t *d_dho = (uint64_t *)dc_reserve(sc, kDcHitOff, (D + 1) * 8);
  if (!d_dho) return nomem();
  uint64_t n_hits = 0;
  if ((rc = device_count(ac, sc, B, 0, nullptr, d_dho, &n_hits))) return rc;
  if (n_hits_out) *n_hits_out = n_hits;
  std::vector<uint64_t> hd, dpo, po;
  std::vector<uint32_t> np;
  std::vector<DcItem> items;
  std::vector<const uint32_t *> srcs;
  std::vector<DocRange> ranges;
  try {
    hd.resize(D + 1);
    dpo.assign(D + 1, 0);
  } catch (...) {
    return AHA_E_NOMEM;
  }
  HIPCHK(ac, hipMemcpyAsync(hd.data(), d_dho, (D + 1) * 8, hipMemcpyDeviceToHost, s));
  HIPCHK(ac, hipStreamSynchronize(s));
  call.book.begin();
  const uint32_t sort_max = ac->dc_sort_max, dense_min = ac->dc_dense_min;
  // what a document holds in scratch while its range is worked on: its hits, and in the range form its pairs beside them
  auto form = [&](uint64_t h) { return h <= sort_max ? 0 : (h < dense_min ? 1 : 2); };
  auto doc_bytes = [&](uint64_t h) { return h * sizeof(aha_hit) + (form(h) == 1 ? std::min<uint64_t>(h, K) * 8 : 0); };
  // (where the batch is cut, a range starts at a document with hits, not at the hitless ones before it: fewer bytes are matched,
  // the same pairs come out; the pair offsets of the documents in no range are the host's to write)
  if (!doc_ranges(hd.data(), D, ac->dc_hit_bytes, doc_bytes, ranges)) return AHA_E_NOMEM;
  uint64_t total = 0, done = 0;  // (done: the documents whose pair offsets stand)
  for (const DocRange &g : ranges) {
    const uint64_t d0 = g.d0, d1 = g.d1, nd = d1 - d0, rh = hd[d1] - hd[d0];
    for (uint64_t d = done; d < d0; d++) dpo[d + 1] = total;
    Batch R;
    if ((rc = call.batch(d0, d1, R))) return rc;
    uint32_t *d_np = (uint32_t *)dc_reserve(sc, kDcPairsPerDoc, nd * 4);
    if (!d_np) return nomem();
    HIPCHK(ac, hipMemsetAsync(d_np, 0, nd * 4, s));
    try {
      srcs.assign(nd, nullptr);
      np.resize(nd);
      items.clear();
    } catch (...) {
      return AHA_E_NOMEM;
    }
    if (g.solo) {
      const auto t_m0 = std::chrono::steady_clock::now();
      unsigned long long *row = (unsigned long long *)dc_reserve(sc, kDcSoloRow, std::max<uint64_t>(K, 1) * 8);
      uint32_t *tmp = (uint32_t *)dc_reserve(sc, kDcRangePairs, std::max<uint64_t>(K, 1) * 8);
      DcItem *d_items = (DcItem *)dc_reserve(sc, kDcItems, sizeof(DcItem));
      if (!row || !tmp || !d_items) return nomem();
      uint64_t got = 0;
      if ((rc = device_count(ac, sc, R, 0, (uint64_t *)row, nullptr, &got))) return rc;
      call.book.matched(t_m0);
      items.assign(1, DcItem{0, tmp, 0, 0});
      HIPCHK(ac, hipMemcpyAsync(d_items, items.data(), sizeof(DcItem), hipMemcpyHostToDevice, s));
      doccount_launch_compact64(d_items, row, (uint32_t)K, d_np, s);
      srcs[0] = tmp;
    } else {
      aha_hit *d_hits = nullptr;
      if ((rc = call.match(R, rh, &d_hits))) return rc;
      // the work items: [sort | range | dense documents (a row each, in groups) | slices of the dense documents' hits]
      uint32_t n_form[3] = {0, 0, 0};
      uint64_t range_pairs = 0, n_slices = 0;
      for (uint64_t d = 0; d < nd; d++) {
        const uint64_t h = hd[d0 + d + 1] - hd[d0 + d];
        if (!h) continue;
        const int f = form(h);
        n_form[f]++;
        if (f == 1) range_pairs += std::min<uint64_t>(h, K);
        if (f == 2) n_slices += (h + kDcSliceHits - 1) / kDcSliceHits;
      }
      const uint64_t rows_max = std::max<uint64_t>(1, ac->dc_row_bytes / (std::max<uint64_t>(K, 1) * 4));
      const uint64_t n_rows = std::min<uint64_t>(n_form[2], rows_max);
      uint32_t *d_rtmp = range_pairs ? (uint32_t *)dc_reserve(sc, kDcRangePairs, range_pairs * 8) : nullptr;
      uint32_t *d_rows = n_rows ? (uint32_t *)dc_reserve(sc, kDcRows, n_rows * K * 4) : nullptr;
      if ((range_pairs && !d_rtmp) || (n_rows && !d_rows)) return nomem();
      if (n_rows && !sc->dc_rows_clear) HIPCHK(ac, hipMemsetAsync(d_rows, 0, sc->dcbuf[kDcRows].bytes, s));
      const size_t o_range = n_form[0], o_dense = o_range + n_form[1], o_slice = o_dense + n_form[2];
      try {
        items.resize(o_slice + n_slices);
      } catch (...) {
        return AHA_E_NOMEM;
      }
      size_t at[3] = {0, o_range, o_dense}, at_slice = o_slice;
      uint64_t rt = 0;
      uint32_t *hw = reinterpret_cast<uint32_t *>(d_hits);
      for (uint64_t d = 0; d < nd; d++) {
        const uint64_t b = hd[d0 + d] - hd[d0], h = hd[d0 + d + 1] - hd[d0 + d];
        if (!h) continue;
        const int f = form(h);
        uint32_t *out = hw + b * 3;  // over the document's own hits
        if (f == 1) {
          out = d_rtmp + 2 * rt;
          rt += std::min<uint64_t>(h, K);
        }
        srcs[d] = out;
        if (f == 2) {
          const uint32_t row = (uint32_t)((at[2] - o_dense) % rows_max);
          for (uint64_t x = 0; x < h; x += kDcSliceHits)
            items[at_slice++] = DcItem{b + x, nullptr, (uint32_t)std::min<uint64_t>(kDcSliceHits, h - x), row};
        }
        items[at[f]++] = DcItem{b, out, (uint32_t)h, (uint32_t)d};
      }
      DcItem *d_items = (DcItem *)dc_reserve(sc, kDcItems, std::max<size_t>(items.size(), 1) * sizeof(DcItem));
      if (!d_items) return nomem();
      HIPCHK(ac, hipMemcpyAsync(d_items, items.data(), items.size() * sizeof(DcItem), hipMemcpyHostToDevice, s));
      doccount_launch_sort(d_items, n_form[0], d_hits, d_np, s);
      doccount_launch_range(d_items + o_range, n_form[1], d_hits, (uint32_t)K, ac->dc_range_keys, d_np, s);
      if (n_form[2]) sc->dc_rows_clear = false;  // (until the last compaction has run)
      size_t sl = o_slice;
      for (uint64_t g0 = 0; g0 < n_form[2]; g0 += rows_max) {  // the dense documents, as many at a time as there are rows
        const uint32_t gn = (uint32_t)std::min<uint64_t>(rows_max, n_form[2] - g0);
        size_t sl1 = sl;
        for (uint32_t r = 0; r < gn; r++) sl1 += (items[o_dense + g0 + r].n + kDcSliceHits - 1) / kDcSliceHits;
        doccount_launch_add(d_items + sl, (uint32_t)(sl1 - sl), d_hits, d_rows, (uint32_t)K, 3u * ac->v2_grid + 3u, s);
        doccount_launch_compact(d_items + o_dense + g0, gn, d_rows, (uint32_t)K, d_np, s);
        sl = sl1;
      }
    }
    HIPCHK(ac, hipGetLastError());
    HIPCHK(ac, hipMemcpyAsync(np.data(), d_np, nd * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(ac, hipStreamSynchronize(s));
    sc->dc_rows_clear = true;
    // the range's pair offsets; the pairs below the capacity to their place
    try {
      po.resize(nd + 1);
    } catch (...) {
      return AHA_E_NOMEM;
    }
    po[0] = 0;
    for (uint64_t d = 0; d < nd; d++) {
      po[d + 1] = po[d] + np[d];
      dpo[d0 + d + 1] = total + po[d + 1];
    }
    const uint64_t room = cap > total ? cap - total : 0, n_write = std::min<uint64_t>(room, po[nd]);
    if (n_write) {
      uint64_t *d_po = (uint64_t *)dc_reserve(sc, kDcGather, (nd + 1) * 8 + nd * sizeof(uint32_t *));
      if (!d_po) return nomem();
      const uint32_t **d_src = reinterpret_cast<const uint32_t **>(d_po + nd + 1);
      HIPCHK(ac, hipMemcpyAsync(d_po, po.data(), (nd + 1) * 8, hipMemcpyHostToDevice, s));
      HIPCHK(ac, hipMemcpyAsync(d_src, srcs.data(), nd * sizeof(uint32_t *), hipMemcpyHostToDevice, s));
      doccount_launch_gather(d_po, d_src, nd, n_write, d_out + total, s);
      HIPCHK(ac, hipGetLastError());
      HIPCHK(ac, hipStreamSynchronize(s));
    }
    total += po[nd];
    call.book.first_done();  // (after the first range, matched or solo)
    done = d1;
  }
  for (uint64_t d = done; d < D; d++) dpo[d + 1] = total;
  if (d_doc_pair_offsets) {
    HIPCHK(ac, hipMemcpyAsync(d_doc_pair_offsets, dpo.data(), (D + 1) * 8, hipMemcpyHostToDevice, s));
    HIPCHK(ac, hipStreamSynchronize(s));
  }
  *n_pairs = total;
  call.book.finish(n_hits, ranges.size(), nullptr);
  if (total > cap) {
    tls_err = "output buffer too small";
    return AHA_E_CAPACITY;
  }
  return AHA_OK;
}

// ---- select calls (aha_ac_select_batch*) -----------------------------------------------------------------------------
static void *sel_reserve(Scratch *sc, SelectSlot slot, size_t bytes) { return reserve_ptr(sc->selbuf[slot], bytes, kGrowEighth); }

// One device-resident batch selected (aha_ac_select_batch_device): per document the leftmost-longest, non-overlapping hits.
//   1. device_count without key counts: the hits per document and their total, no capacity (and the offsets' validation).
//   2. The ranges of doc_ranges.hpp (one, as a rule), tiled so that every document is in one, each matched into the call's
//      scratch (RangeCall, above).
//   3. The passes of scan_select.hip over the range: L, the masks, the walk, the rank -- the range's total comes back.
//   4. Once the call's total is known to fit: the selection to its place, then the documents' offsets.
// A failing call writes none of the caller's buffers, so nothing is emitted before the total of ALL ranges is known: with one
// range its L and select mask are still in scratch then; with more, the ranges are worked through a second time (steps 2 and 3
// again, then the emit) -- the price of the rare case, instead of a second buffer of the selection's size.
int32_t device_select(aha_ac *ac, Scratch *sc, const Batch &B, const HitOut &out, uint64_t *n_selected, uint64_t *n_hits_out,
                      uint32_t flags) {
  return device_select_to(ac, sc, B, out, n_selected, n_hits_out, nullptr, flags);
}

// device_select with a say in where the selection goes (handle.hpp SelectSink).  sink == null: the public entries, as above.
// With a sink every range's selection is emitted behind the ranges' before it as soon as the range has been worked -- one count
// and one match per range whatever the number of ranges -- and d_out, cap and d_doc_sel_offsets are not used.
// With AHA_SELECT_TOKENS in flags (no sink): the tokens of every document instead (scan_tokens.hip; DESIGN.md 4.14 "Tokens").
// Step 3 goes on behind the walk: S, the bytes inside a selected hit; T, the token starts, from S, the masks and the caller's
// own bytes of the range; the rank is T's, and step 4 emits the tokens.  The ranges tile ALL documents, hits or none
// (doc_ranges.hpp doc_tiles), bounded by their text as well as by their hits; a range without a hit is not matched.
int32_t device_select_to(aha_ac *ac, Scratch *sc, const Batch &B, const HitOut &out, uint64_t *n_selected, uint64_t *n_hits_out,
                         const SelectSink *sink, uint32_t flags) {
  if (!ac || !n_selected || !B.doc_off) return AHA_E_INVALID;
  aha_hit *d_out = out.d_out;  // (a sink gives its own, range by range)
  uint64_t cap = out.cap;
  uint64_t *const d_doc_sel_offsets = out.d_doc_hit_off;
  const bool tokens = (flags & AHA_SELECT_TOKENS) != 0, gap_runs = (flags & AHA_SELECT_GAP_RUNS) != 0;
  if (tokens && sink) return AHA_E_INVALID;
  if (ac->device < 0) return no_device();
  if (cap && !d_out) return AHA_E_INVALID;
  DeviceGuard g(ac->device);
  hipStream_t s = B.stream;
  const uint64_t D = B.n_docs, n_bytes = B.n_bytes;
  *n_selected = 0;
  if (n_hits_out) *n_hits_out = 0;
  RangeCall call{ac, sc, B, sc->selbuf[kSelRel], sc->selbuf[kSelText],
                 sc->selbuf[kSelHits], kGrowEighth, "select", "hipMalloc failed for the scratch of a select call", RangeBook{ac, true}};
  auto nomem = [&]() { return call.nomem(); };
  int32_t rc;
  uint64_t *d_dho = (uint64_t *)sel_reserve(sc, kSelHitOff, (D + 1) * 8);
  uint64_t *d_dso = (uint64_t *)sel_reserve(sc, kSelDocOff, (D + 1) * 8);
  if (!d_dho || !d_dso) return nomem();
  uint64_t n_hits = 0;
  if ((rc = device_count(ac, sc, B, 0, nullptr, d_dho, &n_hits))) return rc;
  std::vector<uint64_t> hd, bounds;
  std::vector<DocRange> ranges;
  try {
    hd.resize(D + 1);
    bounds.push_back(0);
  } catch (...) {
    return AHA_E_NOMEM;
  }
  HIPCHK(ac, hipMemcpyAsync(hd.data(), d_dho, (D + 1) * 8, hipMemcpyDeviceToHost, s));
  HIPCHK(ac, hipStreamSynchronize(s));
  call.book.begin();
  // the ranges, tiled: each from the end of the one before it (the first from 0), the last to D -- the walk takes every document,
  // hitless ones cost nothing, and a document beyond the bound is matched like any other (no solo form)
  if (tokens) {  // ... every document, hits or none, the text bounded too; no byte at all: no range, no token
    if (n_bytes) {
      if ((rc = call.host_offsets())) return rc;
      if (!doc_tiles(hd.data(), call.off.data(), D, ac->sel_hit_bytes, bounds)) return AHA_E_NOMEM;
    }
  } else {
    if (!doc_ranges(hd.data(), D, ac->sel_hit_bytes, [](uint64_t h) { return h * sizeof(aha_hit); }, ranges)) return AHA_E_NOMEM;
    try {
      for (const DocRange &g : ranges) bounds.push_back(g.d1);
    } catch (...) {
      return AHA_E_NOMEM;
    }
    if (!ranges.empty()) bounds.back() = D;
  }
  const size_t n_ranges = bounds.size() - 1;  // 0: no hit at all (a token call: no byte at all)
  const uint32_t blocks = post_grid(ac);
  uint64_t total = 0;
  // what a worked range leaves in scratch for the emit
  struct Range {
    const uint64_t *d_rel;
    uint64_t nd, nb;
    uint64_t *L, *blk;
    uint32_t *select;  // the ranked mask: the select mask, a token call's T
    uint32_t *doc_start, *hit_start;  // a token call: the document-start mask; the select mask
  } R{};
  // steps 2 and 3 for the documents [d0, d1); *sel = the range's selected hits
  auto work = [&](uint64_t d0, uint64_t d1, uint64_t *sel) -> int32_t {
    const uint64_t rh = hd[d1] - hd[d0];
    Batch Rb;
    if ((rc = call.batch(d0, d1, Rb))) return rc;
    const uint64_t *d_rel = Rb.doc_off;
    const uint64_t nd = Rb.n_docs, nb = Rb.n_bytes, n_words = (nb + 31) / 32, n_blk = select_rank_blocks(nb);
    uint64_t *L = (uint64_t *)sel_reserve(sc, kSelLongest, nb * 8);
    uint32_t *masks = (uint32_t *)sel_reserve(sc, kSelMasks, 3 * n_words * 4);
    uint64_t *blk = (uint64_t *)sel_reserve(sc, kSelBlocks, (n_blk + 1) * 8);
    if (!L || !masks || !blk) return nomem();
    uint32_t *S = nullptr, *T = nullptr;
    if (tokens) {
      S = (uint32_t *)sel_reserve(sc, kSelSpans, n_words * 4);
      T = (uint32_t *)sel_reserve(sc, kSelTokens, n_words * 4);
      if (!S || !T) return nomem();
    }
    aha_hit *d_hits = nullptr;
    if (rh || !tokens) {  // (a token call works ranges without a hit: nothing to match)
      if ((rc = call.match(Rb, rh, &d_hits))) return rc;
    }
    uint32_t *cover = masks, *doc_start = masks + n_words, *select = masks + 2 * n_words;
    HIPCHK(ac, hipMemsetAsync(L, 0, nb * 8, s));
    HIPCHK(ac, hipMemsetAsync(masks, 0, 3 * n_words * 4, s));
    if (rh || !tokens) select_launch_longest(d_hits, rh, d_dho + d0, d_rel, nd, nb, L, blocks, s);
    select_launch_marks(L, nb, d_rel, nd, cover, doc_start, blocks, s);
    select_launch_walk(L, nb, cover, doc_start, select, blocks, s);
    if (tokens) {
      HIPCHK(ac, hipMemsetAsync(S, 0, n_words * 4, s));
      tokens_launch_spans(L, nb, select, S, blocks, s);
      tokens_launch_starts(Rb.text, nb, select, S, doc_start, gap_runs, T, blocks, s);
    }
    select_launch_rank(tokens ? T : select, nb, blk, blocks, s);
    HIPCHK(ac, hipGetLastError());
    HIPCHK(ac, hipMemcpyAsync(sel, blk + n_blk, 8, hipMemcpyDeviceToHost, s));
    HIPCHK(ac, hipStreamSynchronize(s));
    R = Range{d_rel, nd, nb, L, blk, tokens ? T : select, doc_start, select};
    return AHA_OK;
  };
  auto emit = [&](uint64_t base) -> int32_t {
    if (tokens)
      tokens_launch_emit(R.select, R.nb, R.blk, R.hit_start, R.doc_start, R.L, R.d_rel, R.nd, d_out + base, blocks, s);
    else
      select_launch_emit(R.select, R.nb, R.blk, R.L, R.d_rel, R.nd, d_out + base, blocks, s);
    HIPCHK(ac, hipGetLastError());
    return AHA_OK;
  };
  // the count pass: every range's total, the documents' offsets into scratch
  for (size_t r = 0; r < n_ranges; r++) {
    uint64_t sel = 0;
    if ((rc = work(bounds[r], bounds[r + 1], &sel))) return rc;
    select_launch_rank_docs(R.select, R.blk, R.d_rel, R.nd, total, d_dso + bounds[r], blocks, s);
    HIPCHK(ac, hipGetLastError());
    if (sink && sel) {  // the range's selection to its place in the sink's buffer at once
      if ((rc = sink->place(total, total + sel, &d_out))) return rc;
      if ((rc = emit(total))) return rc;
    }
    if (n_ranges > 1) HIPCHK(ac, hipStreamSynchronize(s));  // (the next range takes the scratch)
    total += sel;
  }
  if (sink) {  // the documents' offsets stay in scratch, all D + 1 of them
    if (!n_ranges) {
      HIPCHK(ac, hipMemsetAsync(d_dso, 0, (D + 1) * 8, s));
    } else {
      HIPCHK(ac, hipMemcpyAsync(d_dso + D, &total, 8, hipMemcpyHostToDevice, s));
    }
    HIPCHK(ac, hipStreamSynchronize(s));
    cap = total;
  } else if (total <= cap) {
    if (n_ranges == 1 && total) {
      if ((rc = emit(0))) return rc;
    } else if (n_ranges > 1) {  // the emit pass
      uint64_t base = 0;
      for (size_t r = 0; r < n_ranges; r++) {
        uint64_t sel = 0;
        if ((rc = work(bounds[r], bounds[r + 1], &sel))) return rc;
        if (sel && (rc = emit(base))) return rc;
        HIPCHK(ac, hipStreamSynchronize(s));
        base += sel;
      }
      if (base != total) {
        tls_err = "select: the two passes over the ranges disagree";
        return AHA_E_HIP;
      }
    }
    if (d_doc_sel_offsets) {
      if (!n_ranges) {
        HIPCHK(ac, hipMemsetAsync(d_doc_sel_offsets, 0, (D + 1) * 8, s));
      } else {
        HIPCHK(ac, hipMemcpyAsync(d_doc_sel_offsets, d_dso, D * 8, hipMemcpyDeviceToDevice, s));
        HIPCHK(ac, hipMemcpyAsync(d_doc_sel_offsets + D, &total, 8, hipMemcpyHostToDevice, s));
      }
    }
    HIPCHK(ac, hipStreamSynchronize(s));
  }
  *n_selected = total;
  if (n_hits_out) *n_hits_out = n_hits;
  call.book.finish(n_hits, n_ranges, sink ? sink->timing : nullptr);
  if (total > cap) {
    tls_err = "output buffer too small";
    return AHA_E_CAPACITY;
  }
  return AHA_OK;
}

// ---- replace calls (aha_ac_replace_batch*) ---------------------------------------------------------------------------
static void *rep_reserve(Scratch *sc, ReplaceSlot slot, size_t bytes) { return reserve_ptr(sc->repbuf[slot], bytes, kGrowEighth); }

// One device-resident batch substituted (aha_ac_replace_batch_device).
//   1. device_select_to with a sink: the selection of ALL ranges into repbuf[kRepSel], the documents' offsets into it in
//      selbuf[kSelDocOff] -- select's cost, one count and one match per range.
//   2. Per selected hit its first byte in the corpus and its change of length; the exclusive scan of the changes; the
//      documents' offsets into the result (scan_replace.hip).  The last of them is the total: it comes back to the host.
//   3. Once the total is known to fit: the copy, then the documents' offsets to the caller.
// A failing call writes none of the caller's buffers.
int32_t device_replace(aha_ac *ac, Scratch *sc, const aha_repl *table, const Batch &B, uint8_t *d_out, uint64_t cap_bytes,
                       uint64_t *d_doc_out_offsets, uint64_t *n_out_bytes, uint64_t *n_selected, uint64_t *n_hits_out) {
  if (!ac || !table || !n_out_bytes || !B.doc_off) return AHA_E_INVALID;
  if (ac->device < 0 || !table->d_ent) return no_device();
  if (cap_bytes && !d_out) return AHA_E_INVALID;
  DeviceGuard g(ac->device);
  hipStream_t s = B.stream;
  const uint64_t D = B.n_docs;
  *n_out_bytes = 0;
  auto nomem = [&]() {
    tls_err = "hipMalloc failed for the scratch of a replace call";
    return AHA_E_HIP;
  };
  int32_t rc = AHA_OK;
  aha_timing t_sel;  // what the select inside measured: the engine, the hits, the ranges (profiling)
  memset(&t_sel, 0, sizeof(t_sel));
  SelectSink sink;
  sink.timing = &t_sel;
  sink.place = [&](uint64_t kept, uint64_t upto, aha_hit **at) -> int32_t {
    Buf &cur = sc->repbuf[kRepSel];
    if (cur.bytes < upto * sizeof(aha_hit)) {
      if (!kept) {
        if (!rep_reserve(sc, kRepSel, upto * sizeof(aha_hit))) return nomem();
      } else {  // a further range: the larger buffer, what is there already into it, then the two change places
        Buf &spare = sc->repbuf[kRepSelSpare];
        if (!rep_reserve(sc, kRepSelSpare, upto * sizeof(aha_hit))) return nomem();
        hipError_t e = hipMemcpyAsync(spare.p, cur.p, kept * sizeof(aha_hit), hipMemcpyDeviceToDevice, s);
        if (e == hipSuccess) e = hipStreamSynchronize(s);
        if (e != hipSuccess) {
          (void)hipGetLastError();
          tls_err = std::string("replace: moving the selection into a larger buffer: ") + hipGetErrorString(e);
          return AHA_E_HIP;
        }
        std::swap(cur, spare);
      }
    }
    *at = (aha_hit *)cur.p;
    return AHA_OK;
  };
  uint64_t n = 0, n_hits = 0;
  if ((rc = device_select_to(ac, sc, B, HitOut{nullptr, 0, nullptr}, &n, &n_hits, &sink))) return rc;
  const auto t_sel1 = std::chrono::steady_clock::now();
  const uint64_t *d_dso = (const uint64_t *)sc->selbuf[kSelDocOff].p;
  const aha_hit *d_sel = (const aha_hit *)sc->repbuf[kRepSel].p;
  const uint64_t n_blk = replace_scan_blocks(n);
  uint64_t *A = (uint64_t *)rep_reserve(sc, kRepStart, std::max<uint64_t>(n, 1) * 8);
  int64_t *shift = (int64_t *)rep_reserve(sc, kRepShift, (n + 1) * 8);
  int64_t *sums = (int64_t *)rep_reserve(sc, kRepSums, (n_blk + 1) * 8);
  uint64_t *d_doo = (uint64_t *)rep_reserve(sc, kRepDocOut, (D + 1) * 8);
  if (!A || !shift || !sums || !d_doo) return nomem();
  const uint32_t blocks = ac->rep_blocks ? ac->rep_blocks : post_grid(ac);
  replace_launch_delta(d_sel, n, d_dso, B.doc_off, D, table->d_ent, table->n_keys, A, shift, blocks, s);
  replace_launch_scan(shift, n, sums, blocks, s);
  replace_launch_doc_offsets(B.doc_off, d_dso, shift, D, d_doo, blocks, s);
  HIPCHK(ac, hipGetLastError());
  uint64_t total = 0;
  HIPCHK(ac, hipMemcpyAsync(&total, d_doo + D, 8, hipMemcpyDeviceToHost, s));
  HIPCHK(ac, hipStreamSynchronize(s));
  if (total <= cap_bytes) {
    replace_launch_copy(B.text, d_sel, A, shift, n, table->d_ent, table->n_keys, (const uint8_t *)table->d_blob, d_out, total,
                        blocks, s);
    HIPCHK(ac, hipGetLastError());
    if (d_doc_out_offsets) HIPCHK(ac, hipMemcpyAsync(d_doc_out_offsets, d_doo, (D + 1) * 8, hipMemcpyDeviceToDevice, s));
    HIPCHK(ac, hipStreamSynchronize(s));
  }
  *n_out_bytes = total;
  if (n_selected) *n_selected = n;
  if (n_hits_out) *n_hits_out = n_hits;
  if (t_sel.struct_size) {  // (the select inside profiled) as select reports; ms_write = everything after the match
    t_sel.ms_write += (float)std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_sel1).count();
    publish_timing(ac, t_sel);
  }
  if (total > cap_bytes) {
    tls_err = "output buffer too small";
    return AHA_E_CAPACITY;
  }
  return AHA_OK;
}

// ---- records and grep calls (aha_ac_records_batch*, aha_ac_grep_batch*) ------------------------------------------------
static void *grp_reserve(Scratch *sc, GrepSlot slot, size_t bytes) { return reserve_ptr(sc->grpbuf[slot], bytes, kGrowEighth); }
uint32_t grep_grid(const aha_ac *ac) { return ac->grep_blocks ? ac->grep_blocks : post_grid(ac); }

// The first half of a records call: the record-end mask and its rank into grpbuf, the total read back.
int32_t device_records_settle(aha_ac *ac, Scratch *sc, const Batch &B, uint8_t delim, uint64_t *n_records) {
  hipStream_t s = B.stream;
  const uint64_t n_bytes = B.n_bytes;
  *n_records = 0;
  if (!n_bytes) return AHA_OK;
  const uint32_t blocks = grep_grid(ac);
  const uint64_t n_words = (n_bytes + 31) / 32, n_blk = select_rank_blocks(n_bytes);
  uint32_t *mask = (uint32_t *)grp_reserve(sc, kGrpEnds, n_words * 4);
  uint64_t *blk = (uint64_t *)grp_reserve(sc, kGrpEndBlocks, (n_blk + 1) * 8);
  if (!mask || !blk) {
    tls_err = "hipMalloc failed for the scratch of a records call";
    return AHA_E_HIP;
  }
  uint64_t total = 0;
  grep_launch_ends(B.text, n_bytes, delim, B.doc_off, B.n_docs, mask, blocks, s);
  select_launch_rank(mask, n_bytes, blk, blocks, s);
  HIPCHK(ac, hipGetLastError());
  HIPCHK(ac, hipMemcpyAsync(&total, blk + n_blk, 8, hipMemcpyDeviceToHost, s));
  HIPCHK(ac, hipStreamSynchronize(s));
  *n_records = total;
  return AHA_OK;
}

// The second half, once the total is known to fit: every set bit as a record's end, the documents' offsets into the records.
int32_t device_records_emit(aha_ac *ac, Scratch *sc, const Batch &B, uint64_t *d_rec_offsets, uint64_t *d_doc_rec_offsets) {
  hipStream_t s = B.stream;
  const uint64_t n_docs = B.n_docs, n_bytes = B.n_bytes;
  if (n_bytes) {
    const uint32_t blocks = grep_grid(ac);
    const uint32_t *mask = (const uint32_t *)sc->grpbuf[kGrpEnds].p;
    const uint64_t *blk = (const uint64_t *)sc->grpbuf[kGrpEndBlocks].p;
    if (d_rec_offsets) grep_launch_emit_ends(mask, n_bytes, blk, d_rec_offsets, blocks, s);
    if (d_doc_rec_offsets) select_launch_rank_docs(mask, blk, B.doc_off, n_docs + 1, 0, d_doc_rec_offsets, blocks, s);
    HIPCHK(ac, hipGetLastError());
  } else {
    if (d_rec_offsets) HIPCHK(ac, hipMemsetAsync(d_rec_offsets, 0, 8, s));
    if (d_doc_rec_offsets) HIPCHK(ac, hipMemsetAsync(d_doc_rec_offsets, 0, (n_docs + 1) * 8, s));
  }
  HIPCHK(ac, hipStreamSynchronize(s));
  return AHA_OK;
}

// One device-resident batch split into records (aha_ac_records_batch_device).  The handle's keys play no part: its device,
// scratch and stream do.
//   1. The record-end mask in one pass over the text, the documents' ends OR-ed in behind it (scan_grep.hip).
//   2. Its rank by select's ranker; the total comes back to the host, where the capacity verdict is given.
//   3. Once it fits: every set bit as a record's end, and the documents' offsets into the records -- the rank of their first
//      byte (select's per-position rank).
// A failing call writes none of the caller's buffers.  Scratch: N / 8 bytes of mask, 8 bytes per 2048 text bytes.
int32_t device_records(aha_ac *ac, Scratch *sc, const Batch &B, uint8_t delim, uint64_t *d_rec_offsets, uint64_t cap_records,
                       uint64_t *d_doc_rec_offsets, uint64_t *n_records) {
  if (!ac || !n_records || !B.doc_off) return AHA_E_INVALID;
  if (cap_records && !d_rec_offsets) return AHA_E_INVALID;
  if (ac->device < 0) return no_device();
  DeviceGuard g(ac->device);
  *n_records = 0;
  int32_t rc;
  if (!B.checked && (rc = check_docs_now(ac, sc, B.doc_off, B.n_docs, B.n_bytes, B.stream))) return rc;
  if (B.n_bytes && !B.text) return AHA_E_INVALID;
  uint64_t total = 0;
  if ((rc = device_records_settle(ac, sc, B, delim, &total))) return rc;
  *n_records = total;
  if (total > cap_records) {
    tls_err = "output buffer too small";
    return AHA_E_CAPACITY;
  }
  return device_records_emit(ac, sc, B, d_rec_offsets, d_doc_rec_offsets);
}

// The keep, S and T masks over documents, their three block ranks and the one-entry table in grpbuf: what fills the masks
// (kgr_flag from the hit offsets, or a rule over the class counts) is the caller's business, the tail below takes them.
struct GrepMasks {
  uint32_t *keep, *S, *T;
  uint64_t *blk_k, *blk_s, *blk_t;
  RepEntry *ent;
};
static bool grep_masks(Scratch *sc, uint64_t D, GrepMasks &M) {
  const uint64_t n_words = (D + 31) / 32, n_blk = select_rank_blocks(D);
  uint32_t *masks = (uint32_t *)grp_reserve(sc, kGrpDocMasks, std::max<uint64_t>(n_words, 1) * 3 * 4);
  uint64_t *blks = (uint64_t *)grp_reserve(sc, kGrpDocBlocks, (n_blk + 1) * 3 * 8);
  M.ent = (RepEntry *)grp_reserve(sc, kGrpTable, sizeof(RepEntry));
  if (!masks || !blks || !M.ent) return false;
  M.keep = masks, M.S = masks + n_words, M.T = masks + 2 * n_words;
  M.blk_k = blks, M.blk_s = blks + (n_blk + 1), M.blk_t = blks + 2 * (n_blk + 1);
  return true;
}

// Grep's tail, from the three masks on (steps 2 to 4 of device_grep below): their ranks, the runs, the scan, the verdict, then
// -- once both numbers fit -- the kept documents and the copy.  *kept and *total are the required numbers either way; *fits
// says whether anything was written to the caller.  more_per_doc: the caller has a per-document buffer of its own that cap_docs
// bounds (context lines' is_match), so the verdict looks at cap_docs without kept_docs or doc_out_offsets too.
static int32_t grep_tail(aha_ac *ac, Scratch *sc, const Batch &B, const GrepMasks &M, uint64_t *d_kept_docs, uint64_t *d_doc_out_offsets,
                         uint64_t cap_docs, uint8_t *d_out, uint64_t cap_bytes, uint64_t *kept_out, uint64_t *total_out, bool *fits_out,
                         bool more_per_doc = false) {
  hipStream_t s = B.stream;
  const uint8_t *d_corpus = B.text;
  const uint64_t *d_doc_offsets = B.doc_off;
  const uint64_t D = B.n_docs, n_bytes = B.n_bytes;
  auto nomem = [&]() {
    tls_err = "hipMalloc failed for the scratch of a grep call";
    return AHA_E_HIP;
  };
  const uint32_t blocks = grep_grid(ac);
  const uint64_t n_blk = select_rank_blocks(D);
  select_launch_rank(M.keep, D, M.blk_k, blocks, s);
  select_launch_rank(M.S, D, M.blk_s, blocks, s);
  select_launch_rank(M.T, D, M.blk_t, blocks, s);
  HIPCHK(ac, hipGetLastError());
  uint64_t kept = 0, n_runs = 0;
  HIPCHK(ac, hipMemcpyAsync(&kept, M.blk_k + n_blk, 8, hipMemcpyDeviceToHost, s));
  HIPCHK(ac, hipMemcpyAsync(&n_runs, M.blk_s + n_blk, 8, hipMemcpyDeviceToHost, s));
  HIPCHK(ac, hipStreamSynchronize(s));
  const uint64_t n_sum = replace_scan_blocks(n_runs);
  aha_hit *sel = (aha_hit *)grp_reserve(sc, kGrpSel, std::max<uint64_t>(n_runs, 1) * sizeof(aha_hit));
  uint64_t *A = (uint64_t *)grp_reserve(sc, kGrpStart, std::max<uint64_t>(n_runs, 1) * 8);
  int64_t *shift = (int64_t *)grp_reserve(sc, kGrpShift, (n_runs + 1) * 8);
  int64_t *sums = (int64_t *)grp_reserve(sc, kGrpSums, (n_sum + 1) * 8);
  if (!sel || !A || !shift || !sums) return nomem();
  grep_launch_runs(M.S, M.T, D, M.blk_s, M.blk_t, d_doc_offsets, n_runs, A, shift, sel, M.ent, blocks, s);
  replace_launch_scan(shift, n_runs, sums, blocks, s);
  HIPCHK(ac, hipGetLastError());
  int64_t change = 0;
  HIPCHK(ac, hipMemcpyAsync(&change, shift + n_runs, 8, hipMemcpyDeviceToHost, s));
  HIPCHK(ac, hipStreamSynchronize(s));
  const uint64_t total = (uint64_t)((int64_t)n_bytes + change);
  const bool per_doc = d_kept_docs || d_doc_out_offsets;
  const bool fits = !((per_doc || more_per_doc) && kept > cap_docs) && !(d_out && total > cap_bytes);
  if (fits) {
    if (per_doc)
      grep_launch_emit_docs(M.keep, M.S, D, M.blk_k, M.blk_s, d_doc_offsets, shift, n_runs, d_kept_docs, d_doc_out_offsets, blocks, s);
    if (d_out)
      replace_launch_copy(d_corpus, sel, A, shift, n_runs, M.ent, 1, (const uint8_t *)M.ent, d_out, total, blocks, s);
    HIPCHK(ac, hipGetLastError());
    HIPCHK(ac, hipStreamSynchronize(s));
  }
  *kept_out = kept;
  *total_out = total;
  *fits_out = fits;
  return AHA_OK;
}

// One device-resident batch filtered (aha_ac_grep_batch_device).
//   1. device_count without key counts: the documents' hit offsets into scratch, the total, the offsets validated.
//   2. The keep, S and T masks over documents (scan_grep.hip kgr_flag) and their ranks by select's ranker: the kept documents
//      and the dropped runs come back to the host as two counts.
//   3. Per dropped run its first byte and its change of length (minus its bytes); replace's scan gives shift; the total comes
//      back to the host, where the verdict is given.  Nothing has been written to the caller so far.
//   4. The kept documents' indices and offsets, and replace's copy fed with the runs as deleted hits.
// A failing call writes none of the caller's buffers.  Steps 2 (from the ranks on) to 4 are grep_tail, which rule grep shares.
int32_t device_grep(aha_ac *ac, Scratch *sc, const Batch &B, uint32_t flags, uint64_t *d_kept_docs, uint64_t *d_doc_out_offsets,
                    uint64_t cap_docs, uint8_t *d_out, uint64_t cap_bytes, uint64_t *n_kept, uint64_t *n_out_bytes, uint64_t *n_hits_out) {
  if (!ac || !n_kept || !B.doc_off || (flags & ~AHA_GREP_INVERT)) return AHA_E_INVALID;
  if ((cap_docs && !d_kept_docs && !d_doc_out_offsets) || (cap_bytes && !d_out)) return AHA_E_INVALID;
  if (ac->device < 0) return no_device();
  DeviceGuard g(ac->device);
  hipStream_t s = B.stream;
  const uint64_t D = B.n_docs;
  *n_kept = 0;
  if (n_out_bytes) *n_out_bytes = 0;
  if (n_hits_out) *n_hits_out = 0;
  auto nomem = [&]() {
    tls_err = "hipMalloc failed for the scratch of a grep call";
    return AHA_E_HIP;
  };
  uint64_t *d_dho = (uint64_t *)grp_reserve(sc, kGrpHitOff, (D + 1) * 8);
  if (!d_dho) return nomem();
  int32_t rc;
  uint64_t n_hits = 0;
  if ((rc = device_count(ac, sc, B, 0, nullptr, d_dho, &n_hits))) return rc;
  const bool prof = ac->profiling.load();
  const auto t0 = std::chrono::steady_clock::now();
  GrepMasks M;
  if (!grep_masks(sc, D, M)) return nomem();
  grep_launch_flag(d_dho, D, (flags & AHA_GREP_INVERT) != 0, M.keep, M.S, M.T, grep_grid(ac), s);
  uint64_t kept = 0, total = 0;
  bool fits = false;
  if ((rc = grep_tail(ac, sc, B, M, d_kept_docs, d_doc_out_offsets, cap_docs, d_out, cap_bytes, &kept, &total, &fits))) return rc;
  *n_kept = kept;
  if (n_out_bytes) *n_out_bytes = total;
  if (n_hits_out) *n_hits_out = n_hits;
  if (prof) {  // ms_write: everything after the count
    const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    std::lock_guard<std::mutex> lk(ac->last_mu);
    ac->last.ms_write += (float)ms;
    ac->last.n_hits = n_hits;
  }
  if (!fits) {
    tls_err = "output buffer too small";
    return AHA_E_CAPACITY;
  }
  return AHA_OK;
}

// The excerpts of one device-resident batch (aha_ac_grep_batch_device with AHA_GREP_CONTEXT; scan_excerpt.hip).
//   1. device_count with a cover mask in scratch and without hit offsets: M, the total, the offsets validated.
//   2. S and T over bytes -- where a covered run of one document starts and ends -- and their ranks by select's ranker: the run
//      count comes back to the host.
//   3. Per run its document and its window, clipped and snapped; the first and last masks over runs and their ranks: the
//      excerpt count R comes back to the host.
//   4. The R + 1 stretches outside the excerpts as deleted hits; replace's scan gives shift; the total comes back to the host,
//      where the verdict is given.  Nothing has been written to the caller so far.
//   5. The excerpts' starts and offsets, and replace's copy.
// A failing call writes none of the caller's buffers.  Scratch beyond the count call's: 3 N / 8 bytes of masks, 16 bytes per
// 2048 text bytes of block ranks, 24 bytes + 2 bits (and their block ranks) per run, 28 bytes per excerpt and the scan's sums.
int32_t device_excerpts(aha_ac *ac, Scratch *sc, const Batch &B0, const aha_excerpt_params *ep, uint64_t *d_starts,
                        uint64_t *d_out_offsets, uint64_t cap_docs, uint8_t *d_out, uint64_t cap_bytes, uint64_t *n_kept,
                        uint64_t *n_out_bytes, uint64_t *n_hits_out) {
  if (!ac || !n_kept || !B0.doc_off || !ep) return AHA_E_INVALID;
  if ((cap_docs && !d_starts && !d_out_offsets) || (cap_bytes && !d_out)) return AHA_E_INVALID;
  if (ac->device < 0) return no_device();
  DeviceGuard g(ac->device);
  Batch B = B0;
  B.params = &ep->match;
  hipStream_t s = B.stream;
  const uint8_t *d_corpus = B.text;
  const uint64_t *d_doc_offsets = B.doc_off;
  const uint64_t D = B.n_docs, n_bytes = B.n_bytes;
  *n_kept = 0;
  if (n_out_bytes) *n_out_bytes = 0;
  if (n_hits_out) *n_hits_out = 0;
  auto nomem = [&]() {
    tls_err = "hipMalloc failed for the scratch of an excerpts call";
    return AHA_E_HIP;
  };
  const uint32_t blocks = grep_grid(ac);
  const uint64_t n_words = (n_bytes + 31) / 32, n_blk = select_rank_blocks(n_bytes);
  uint32_t *masks = (uint32_t *)grp_reserve(sc, kGrpExMasks, std::max<uint64_t>(n_words, 1) * 3 * 4);
  uint64_t *blks = (uint64_t *)grp_reserve(sc, kGrpExBlocks, (n_blk + 1) * 2 * 8);
  if (!masks || !blks) return nomem();
  uint32_t *Mk = masks, *S = masks + n_words, *T = masks + 2 * n_words;
  uint64_t *blk_s = blks, *blk_t = blks + (n_blk + 1);
  int32_t rc;
  uint64_t n_hits = 0;
  if ((rc = device_count(ac, sc, B, 0, nullptr, nullptr, &n_hits, CallOpt::kNone, n_bytes ? Mk : nullptr))) return rc;
  const bool prof = ac->profiling.load();
  const auto t0 = std::chrono::steady_clock::now();
  uint64_t n_runs = 0, n_exc = 0, total = 0;
  if (n_bytes && n_hits) {
    excerpt_launch_edges(Mk, n_bytes, d_doc_offsets, D, S, T, blocks, s);
    select_launch_rank(S, n_bytes, blk_s, blocks, s);
    select_launch_rank(T, n_bytes, blk_t, blocks, s);
    HIPCHK(ac, hipGetLastError());
    HIPCHK(ac, hipMemcpyAsync(&n_runs, blk_s + n_blk, 8, hipMemcpyDeviceToHost, s));
    HIPCHK(ac, hipStreamSynchronize(s));
  }
  uint64_t *A = nullptr;
  int64_t *shift = nullptr;
  aha_hit *sel = nullptr;
  RepEntry *ent = nullptr;
  if (n_runs) {
    const uint64_t r_words = (n_runs + 31) / 32, r_blk = select_rank_blocks(n_runs);
    uint64_t *runs = (uint64_t *)grp_reserve(sc, kGrpExRuns, n_runs * 3 * 8);
    uint32_t *rmasks = (uint32_t *)grp_reserve(sc, kGrpExRunMasks, r_words * 2 * 4);
    uint64_t *rblks = (uint64_t *)grp_reserve(sc, kGrpExRunBlocks, (r_blk + 1) * 2 * 8);
    if (!runs || !rmasks || !rblks) return nomem();
    uint64_t *doc = runs, *w0 = runs + n_runs, *w1 = runs + 2 * n_runs;
    uint32_t *first = rmasks, *last = rmasks + r_words;
    uint64_t *blk_f = rblks, *blk_l = rblks + (r_blk + 1);
    excerpt_launch_windows(S, T, n_bytes, blk_s, blk_t, d_corpus, d_doc_offsets, D, ep->before, ep->after, n_runs, doc, w0, w1, first,
                           last, blocks, s);
    select_launch_rank(first, n_runs, blk_f, blocks, s);
    select_launch_rank(last, n_runs, blk_l, blocks, s);
    HIPCHK(ac, hipGetLastError());
    HIPCHK(ac, hipMemcpyAsync(&n_exc, blk_f + r_blk, 8, hipMemcpyDeviceToHost, s));
    HIPCHK(ac, hipStreamSynchronize(s));
    const uint64_t n_gaps = n_exc + 1, n_sum = replace_scan_blocks(n_gaps);
    sel = (aha_hit *)grp_reserve(sc, kGrpSel, n_gaps * sizeof(aha_hit));
    A = (uint64_t *)grp_reserve(sc, kGrpStart, n_gaps * 8);
    shift = (int64_t *)grp_reserve(sc, kGrpShift, (n_gaps + 1) * 8);
    int64_t *sums = (int64_t *)grp_reserve(sc, kGrpSums, (n_sum + 1) * 8);
    ent = (RepEntry *)grp_reserve(sc, kGrpTable, sizeof(RepEntry));
    if (!sel || !A || !shift || !sums || !ent) return nomem();
    excerpt_launch_gaps(first, last, n_runs, blk_f, blk_l, w0, w1, n_bytes, n_exc, A, shift, sel, ent, blocks, s);
    replace_launch_scan(shift, n_gaps, sums, blocks, s);
    HIPCHK(ac, hipGetLastError());
    int64_t change = 0;
    HIPCHK(ac, hipMemcpyAsync(&change, shift + n_gaps, 8, hipMemcpyDeviceToHost, s));
    HIPCHK(ac, hipStreamSynchronize(s));
    total = (uint64_t)((int64_t)n_bytes + change);
  }
  const bool per_exc = d_starts || d_out_offsets;
  const bool fits = !(per_exc && n_exc > cap_docs) && !(d_out && total > cap_bytes);
  if (fits) {
    if (n_exc) {
      if (per_exc) excerpt_launch_emit(A, shift, n_exc, d_starts, d_out_offsets, blocks, s);
      if (d_out) replace_launch_copy(d_corpus, sel, A, shift, n_exc + 1, ent, 1, (const uint8_t *)ent, d_out, total, blocks, s);
      HIPCHK(ac, hipGetLastError());
    } else if (d_out_offsets) {
      HIPCHK(ac, hipMemsetAsync(d_out_offsets, 0, 8, s));  // (entry R is the total)
    }
    HIPCHK(ac, hipStreamSynchronize(s));
  }
  *n_kept = n_exc;
  if (n_out_bytes) *n_out_bytes = total;
  if (n_hits_out) *n_hits_out = n_hits;
  if (prof) {  // ms_write: everything after the count
    const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    std::lock_guard<std::mutex> lk(ac->last_mu);
    ac->last.ms_write += (float)ms;
    ac->last.n_hits = n_hits;
  }
  if (!fits) {
    tls_err = "output buffer too small";
    return AHA_E_CAPACITY;
  }
  return AHA_OK;
}

// ---- class counts (aha_ac_class_counts_batch*) -----------------------------------------------------------------------
uint32_t class_grid(const aha_ac *ac) { return ac->cls_blocks ? ac->cls_blocks : post_grid(ac); }
static void *cls_reserve(Scratch *sc, ClassSlot slot, size_t bytes) { return reserve_ptr(sc->clsbuf[slot], bytes, kGrowEighth); }

// One device-resident batch as hits per (document, key class) (aha_ac_class_counts_batch_device): d_out[D][C], every entry written.
//   1. device_count without key counts: the hits per document and their total (and the offsets' validation).  A call with 2^32
//      hits or more is checked for a document that could overflow a uint32 (class_overflow.hpp) before d_out is touched.
//   2. d_out is cleared on the call's stream.
//   3. The ranges of doc_ranges.hpp (one, as a rule), each matched into the call's scratch (RangeCall, above), then kcc_add over
//      the hit list (scan_classcount.hip).  A single document beyond the bound is never matched: a count call over it alone
//      gives its key counts, which kcc_fold_keys adds into its row through the table.
int32_t device_class_counts(aha_ac *ac, Scratch *sc, const aha_classes *table, const Batch &B, uint32_t *d_out, uint64_t *n_hits_out) {
  if (!ac || !table || !B.doc_off) return AHA_E_INVALID;
  if (ac->device < 0 || !table->d_off) return no_device();
  if (B.n_docs && !d_out) return AHA_E_INVALID;
  DeviceGuard g(ac->device);
  hipStream_t s = B.stream;
  const uint64_t D = B.n_docs, C = table->n_classes;
  const uint32_t K = ac->aut.n_keys;
  if (n_hits_out) *n_hits_out = 0;
  RangeCall call{ac, sc, B, sc->clsbuf[kClsRel], sc->clsbuf[kClsText],
                 sc->clsbuf[kClsHits], kGrowEighth, "class counts", "hipMalloc failed for the scratch of a class-counts call",
                 RangeBook{ac, true}};
  auto nomem = [&]() { return call.nomem(); };
  int32_t rc;
  uint64_t *d_dho = (uint64_t *)cls_reserve(sc, kClsHitOff, (D + 1) * 8);
  if (!d_dho) return nomem();
  uint64_t n_hits = 0;
  if ((rc = device_count(ac, sc, B, 0, nullptr, d_dho, &n_hits))) return rc;
  call.book.begin();
  // the ranges: the whole batch where all hits are known to fit the bound (the hit offsets stay on the device then)
  std::vector<DocRange> ranges;
  std::vector<uint64_t> hd;
  const uint64_t bound = ac->cls_hit_bytes;
  try {
    if (n_hits && n_hits <= bound / sizeof(aha_hit) && n_hits < (1ull << 32)) {  // (2^32 hits: the documents are looked at)
      ranges.push_back(DocRange{0, D, false});
    } else if (n_hits) {
      hd.resize(D + 1);
      call.off.resize(D + 1);
      HIPCHK(ac, hipMemcpyAsync(hd.data(), d_dho, (D + 1) * 8, hipMemcpyDeviceToHost, s));
      HIPCHK(ac, hipMemcpyAsync(call.off.data(), B.doc_off, (D + 1) * 8, hipMemcpyDeviceToHost, s));
      HIPCHK(ac, hipStreamSynchronize(s));
      uint64_t bad = 0;
      if (class_counts_overflow(hd.data(), D, &bad)) {
        tls_err = "class counts: document " + std::to_string(bad) + " has 2^32 hits or more";
        return AHA_E_TOO_LONG;
      }
      if (!doc_ranges(hd.data(), D, bound, [](uint64_t h) { return h * sizeof(aha_hit); }, ranges)) return AHA_E_NOMEM;
    }
  } catch (...) {
    return AHA_E_NOMEM;
  }
  if (D) HIPCHK(ac, hipMemsetAsync(d_out, 0, D * C * 4, s));
  const uint32_t blocks = class_grid(ac);
  for (size_t r = 0; r < ranges.size(); r++) {
    const uint64_t d0 = ranges[r].d0, d1 = ranges[r].d1, rh = hd.empty() ? n_hits : hd[d1] - hd[d0];
    Batch R;
    if ((rc = call.batch(d0, d1, R))) return rc;
    const uint64_t nd = R.n_docs;
    if (ranges[r].solo) {
      const auto t_m0 = std::chrono::steady_clock::now();
      uint64_t got = 0;
      uint64_t *row = (uint64_t *)cls_reserve(sc, kClsSoloRow, std::max<uint64_t>(K, 1) * 8);
      if (!row) return nomem();
      if ((rc = device_count(ac, sc, R, 0, row, nullptr, &got))) return rc;
      call.book.matched(t_m0);
      if (got != rh) {
        tls_err = "class counts: the two counts of a document disagree";
        return AHA_E_HIP;
      }
      classcount_launch_fold_keys(row, K, table->d_off, table->d_ids, d_out + d0 * C, blocks, s);
    } else {
      aha_hit *d_hits = nullptr;
      if ((rc = call.match(R, rh, &d_hits))) return rc;
      classcount_launch_add(d_hits, rh, d_dho + d0, nd, table->d_off, table->d_ids, K, (uint32_t)C, d_out + d0 * C, blocks, s);
    }
    HIPCHK(ac, hipGetLastError());
    if (r + 1 < ranges.size()) HIPCHK(ac, hipStreamSynchronize(s));  // (the next range takes the scratch)
  }
  HIPCHK(ac, hipStreamSynchronize(s));
  if (n_hits_out) *n_hits_out = n_hits;
  call.book.finish(n_hits, ranges.size(), nullptr);
  return AHA_OK;
}

// ---- rule grep (aha_ac_grep_batch* with AHA_GREP_RULE) ------------------------------------------------------------------
// One device-resident batch filtered by a rule over its class counts (DESIGN.md 4.16 "Rule grep").  gp was checked by capi.cpp.
//   1. device_class_counts as it is: the D x C table into d_rows where the caller gave it and the call cannot fail any more
//      (RuleRows::kEarly: the capacities cover every outcome, or d_rows is the host entry's staging buffer), else into
//      grpbuf[kGrpRows], which AHA_RULE_TABLE_BYTES bounds.
//   2. kgq_keep: the keep mask from the rule; kgq_edges: S and T from keep (scan_greprule.hip).
//   3. grep_tail.  Once it is known to fit, a table in scratch is copied into d_rows.
// A failing call writes none of the caller's buffers, d_rows included.
int32_t device_grep_rule(aha_ac *ac, Scratch *sc, const Batch &B0, const aha_grep_params *gp, uint32_t *d_rows, RuleRows rows,
                         uint32_t flags, uint64_t *d_kept_docs, uint64_t *d_doc_out_offsets, uint64_t cap_docs, uint8_t *d_out,
                         uint64_t cap_bytes, uint64_t *n_kept, uint64_t *n_out_bytes, uint64_t *n_hits_out) {
  if (!ac || !gp || !gp->classes || !gp->terms || !n_kept || !B0.doc_off) return AHA_E_INVALID;
  if (gp->n_terms == 0 || gp->n_terms > kRuleMaxTerms || (flags & ~(AHA_GREP_INVERT | AHA_GREP_RULE))) return AHA_E_INVALID;
  if ((cap_docs && !d_kept_docs && !d_doc_out_offsets) || (cap_bytes && !d_out)) return AHA_E_INVALID;
  if (ac->device < 0) return no_device();
  DeviceGuard g(ac->device);
  Batch B = B0;
  B.params = &gp->match;
  hipStream_t s = B.stream;
  const aha_classes *table = gp->classes;
  const uint64_t D = B.n_docs, C = table->n_classes;
  *n_kept = 0;
  if (n_out_bytes) *n_out_bytes = 0;
  if (n_hits_out) *n_hits_out = 0;
  auto nomem = [&]() {
    tls_err = "hipMalloc failed for the scratch of a grep call";
    return AHA_E_HIP;
  };
  const bool direct = d_rows && rows == RuleRows::kEarly;
  uint32_t *tab = d_rows;
  if (!direct) {
    if (D * C * 4 > ac->rule_table_bytes) {
      tls_err = "rule grep: the class-count table of " + std::to_string(D) + " x " + std::to_string(C) +
                " entries exceeds AHA_RULE_TABLE_BYTES (" + std::to_string(ac->rule_table_bytes) +
                "): pass rows with capacities for every document and byte, or smaller batches";
      return AHA_E_TOO_LARGE;
    }
    tab = (uint32_t *)grp_reserve(sc, kGrpRows, std::max<uint64_t>(D * C * 4, 4));
    if (!tab) return nomem();
  }
  int32_t rc;
  uint64_t n_hits = 0;
  if ((rc = device_class_counts(ac, sc, table, B, tab, &n_hits))) return rc;
  const bool prof = ac->profiling.load();
  const auto t0 = std::chrono::steady_clock::now();
  GrepMasks M;
  if (!grep_masks(sc, D, M)) return nomem();
  const uint32_t blocks = grep_grid(ac);
  greprule_launch_keep(tab, (uint32_t)C, B.doc_off, D, gp->terms, gp->n_terms, (flags & AHA_GREP_INVERT) != 0, M.keep, blocks, s);
  greprule_launch_edges(M.keep, D, M.S, M.T, blocks, s);
  uint64_t kept = 0, total = 0;
  bool fits = false;
  if ((rc = grep_tail(ac, sc, B, M, d_kept_docs, d_doc_out_offsets, cap_docs, d_out, cap_bytes, &kept, &total, &fits))) return rc;
  if (fits && d_rows && !direct && D) {
    HIPCHK(ac, hipMemcpyAsync(d_rows, tab, D * C * 4, hipMemcpyDeviceToDevice, s));
    HIPCHK(ac, hipStreamSynchronize(s));
  }
  *n_kept = kept;
  if (n_out_bytes) *n_out_bytes = total;
  if (n_hits_out) *n_hits_out = n_hits;
  if (prof) {  // engine, n_hits, repeats: the class-count call's; ms_write: everything after its match
    const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    std::lock_guard<std::mutex> lk(ac->last_mu);
    ac->last.ms_write += (float)ms;
    ac->last.n_hits = n_hits;
  }
  if (!fits) {
    tls_err = "output buffer too small";
    return AHA_E_CAPACITY;
  }
  return AHA_OK;
}

// ---- context lines (aha_ac_grep_batch* with AHA_GREP_LINES) --------------------------------------------------------------
// Group offsets live in HBM: k_check_docs over (group_offsets, G, D) and a 4-byte read-back before anything indexes with them.
// Only its order verdict counts: the 2 GiB limit per span is for documents in bytes, a group may hold any number of records.
static int32_t check_groups_now(aha_ac *ac, Scratch *sc, const uint64_t *d_groups, uint64_t n_groups, uint64_t n_docs, hipStream_t s) {
  int32_t rc2;
  if ((rc2 = v2_reserve(sc, kCursor, kCursorBytes))) return rc2;
  if ((rc2 = ensure_h_v2(ac, sc))) return rc2;
  uint32_t *flag = (uint32_t *)sc->v2buf[kCursor].p + 64;  // (check_docs_now's word)
  HIPCHK(ac, hipMemsetAsync(flag, 0, 4, s));
  launch_check_docs(d_groups, n_groups, n_docs, flag, nullptr, s);
  HIPCHK(ac, hipMemcpyAsync(sc->h_v2, flag, 4, hipMemcpyDeviceToHost, s));
  HIPCHK(ac, hipStreamSynchronize(s));
  if ((uint32_t)sc->h_v2[0] & 1u) {
    tls_err = "group offsets: need group_offsets[0] = 0, ascending, group_offsets[n_groups] = n_docs";
    return AHA_E_INVALID;
  }
  return AHA_OK;
}

// One device-resident batch filtered with context (DESIGN.md 4.16 "Context lines").  lp was checked by capi.cpp.
//   1. device_count without key counts: the records' hit offsets into scratch, the total, the offsets validated; the group
//      offsets validated (check_groups_now).
//   2. kgr_flag as it is, its keep mask into a slot of its own: m.  (Its S and T land in grep's slots and are overwritten in 5.)
//   3. Sm and Tm over records -- where a run of matching records of one group starts and ends (kgl_edges, kgl_group_edges) --
//      and their ranks: the run count comes back to the host.
//   4. Per run its group and its window, then the toggles of the merged windows' ends (kgl_windows, kgl_toggle); the toggle
//      mask's rank; kgl_fill writes grep's keep mask.  Without a run the keep mask is cleared instead.
//   5. kgq_edges and grep_tail as rule grep calls them.  Once the call is known to fit, kgl_emit_match over the ranked keep mask.
// A failing call writes none of the caller's buffers.  Scratch beyond grep's: 4 bits per record of masks, 24 bytes per 2048
// records of block ranks, 24 bytes per matching run.
int32_t device_grep_lines(aha_ac *ac, Scratch *sc, const Batch &B0, const aha_grep_lines_params *lp, const uint64_t *d_groups,
                          uint8_t *d_is_match, uint32_t flags, uint64_t *d_kept_docs, uint64_t *d_doc_out_offsets, uint64_t cap_docs,
                          uint8_t *d_out, uint64_t cap_bytes, uint64_t *n_kept, uint64_t *n_out_bytes, uint64_t *n_hits_out) {
  if (!ac || !lp || !n_kept || !B0.doc_off || (flags & ~(AHA_GREP_INVERT | AHA_GREP_LINES))) return AHA_E_INVALID;
  if ((cap_docs && !d_kept_docs && !d_doc_out_offsets && !d_is_match) || (cap_bytes && !d_out)) return AHA_E_INVALID;
  if ((d_is_match && !cap_docs) || (!d_groups != !lp->n_groups)) return AHA_E_INVALID;
  if (ac->device < 0) return no_device();
  DeviceGuard g(ac->device);
  Batch B = B0;
  B.params = &lp->match;
  hipStream_t s = B.stream;
  const uint64_t D = B.n_docs, G = lp->n_groups;
  *n_kept = 0;
  if (n_out_bytes) *n_out_bytes = 0;
  if (n_hits_out) *n_hits_out = 0;
  auto nomem = [&]() {
    tls_err = "hipMalloc failed for the scratch of a grep call";
    return AHA_E_HIP;
  };
  uint64_t *d_dho = (uint64_t *)grp_reserve(sc, kGrpHitOff, (D + 1) * 8);
  if (!d_dho) return nomem();
  int32_t rc;
  uint64_t n_hits = 0;
  if ((rc = device_count(ac, sc, B, 0, nullptr, d_dho, &n_hits))) return rc;
  if (d_groups && (rc = check_groups_now(ac, sc, d_groups, G, D, s))) return rc;
  const bool prof = ac->profiling.load();
  const auto t0 = std::chrono::steady_clock::now();
  GrepMasks M;
  if (!grep_masks(sc, D, M)) return nomem();
  const uint32_t blocks = grep_grid(ac);
  const uint64_t n_words = (D + 31) / 32, n_blk = select_rank_blocks(D);
  const uint64_t t_words = (D + 1 + 31) / 32, t_blk = select_rank_blocks(D + 1);
  uint32_t *lmasks = (uint32_t *)grp_reserve(sc, kGrpLnMasks, (3 * n_words + t_words) * 4);
  uint64_t *lblks = (uint64_t *)grp_reserve(sc, kGrpLnBlocks, (2 * (n_blk + 1) + (t_blk + 1)) * 8);
  if (!lmasks || !lblks) return nomem();
  uint32_t *m = lmasks, *Sm = lmasks + n_words, *Tm = lmasks + 2 * n_words, *tog = lmasks + 3 * n_words;
  uint64_t *blk_sm = lblks, *blk_tm = lblks + (n_blk + 1), *blk_x = lblks + 2 * (n_blk + 1);
  uint64_t n_runs = 0;
  if (D) {
    grep_launch_flag(d_dho, D, (flags & AHA_GREP_INVERT) != 0, m, M.S, M.T, blocks, s);
    greplines_launch_edges(m, D, d_groups, G, Sm, Tm, blocks, s);
    select_launch_rank(Sm, D, blk_sm, blocks, s);
    select_launch_rank(Tm, D, blk_tm, blocks, s);
    HIPCHK(ac, hipGetLastError());
    HIPCHK(ac, hipMemcpyAsync(&n_runs, blk_sm + n_blk, 8, hipMemcpyDeviceToHost, s));
    HIPCHK(ac, hipStreamSynchronize(s));
    if (n_runs) {
      uint64_t *runs = (uint64_t *)grp_reserve(sc, kGrpLnRuns, n_runs * 3 * 8);
      if (!runs) return nomem();
      HIPCHK(ac, hipMemsetAsync(tog, 0, t_words * 4, s));
      greplines_launch_windows(Sm, Tm, D, blk_sm, blk_tm, d_groups, G, lp->before, lp->after, n_runs, runs, runs + n_runs,
                               runs + 2 * n_runs, tog, blocks, s);
      select_launch_rank(tog, D + 1, blk_x, blocks, s);
      greplines_launch_fill(tog, blk_x, D, M.keep, blocks, s);
    } else {
      HIPCHK(ac, hipMemsetAsync(M.keep, 0, n_words * 4, s));
    }
    greprule_launch_edges(M.keep, D, M.S, M.T, blocks, s);
    HIPCHK(ac, hipGetLastError());
  }
  uint64_t kept = 0, total = 0;
  bool fits = false;
  if ((rc = grep_tail(ac, sc, B, M, d_kept_docs, d_doc_out_offsets, cap_docs, d_out, cap_bytes, &kept, &total, &fits, d_is_match != nullptr)))
    return rc;
  if (fits && d_is_match && kept) {
    greplines_launch_emit_match(M.keep, M.blk_k, D, m, d_is_match, blocks, s);
    HIPCHK(ac, hipGetLastError());
    HIPCHK(ac, hipStreamSynchronize(s));
  }
  *n_kept = kept;
  if (n_out_bytes) *n_out_bytes = total;
  if (n_hits_out) *n_hits_out = n_hits;
  if (prof) {  // ms_write: everything after the count
    const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    std::lock_guard<std::mutex> lk(ac->last_mu);
    ac->last.ms_write += (float)ms;
    ac->last.n_hits = n_hits;
  }
  if (!fits) {
    tls_err = "output buffer too small";
    return AHA_E_CAPACITY;
  }
  return AHA_OK;
}

}  // namespace ahai
