// image.hpp -- structures shared by the host C ABI (capi.cpp) and the HIP
// kernels (kernels.hip).  Plain data, passed to kernels by value.
#pragma once
#include <cstdint>

#include "../../include/aha_hip.h"

namespace aha {

// Automaton image resident in HBM (see automaton.hpp for the slot formats).
struct DevAut {
  const void *slots;         // uint2[n_slots] (wide) or uint32[n_slots] (compact)
  const int32_t *end_key;    // compact only: key id at header slots of end states
  const uint32_t *end_info;  // compact only: end_key (or, with flattened chains, its chain offset) | min(key_cnt, 255) << 24
  const uint2 *key_ln;       // [K] {len, next}: ac.cr key_lens / output.next chain
  const uint32_t *key_cnt;   // [K] hits emitted when the key's state is reached
  const uint32_t *key_kc;    // [K] lead bytes in key[1..len)
  // the output chains once more, flattened (null when their total length is unreasonable): key k's chain is
  // chain[chain_off[k] .. + key_cnt[k]) = {len, key} of the key itself and of every key after it on the chain, so the
  // expansion reads consecutive entries instead of chasing key_ln.next (cfg 5: 947 M dependent gathers otherwise)
  // With the flattened chains an event record carries `chain offset | min(chain length, 255) << 24` instead of the key
  // id (k2d_count takes it from end_info / key_info with the one gather it makes anyway); chains need 24-bit offsets.
  const uint32_t *key_info;   // [K] chain_off[k] | min(key_cnt[k], 255) << 24 (wide format: gathered by the count pass)
  const uint2 *chain;         // {len, key}
  const uint2 *chain_chars;   // {lead bytes in key[1..len) + 1 = the key's length in characters, key}, same index (char
                              // offsets: one gather per hit like the byte offsets, not a second one for the length)
  uint32_t root;
  uint32_t n_slots;
  uint32_t max_len;
  uint32_t compact;
  // shadow fail: a state with base in [s2_lo, s2_hi) has depth >= 3 and a fail target of depth <= 2, i.e. its fail
  // target is the depth<=2 state of the last two input bytes, which k2_traverse keeps in registers (0,0 = off)
  uint32_t s1_lo;            // [s1_lo, s2_lo): depth-2 states; their fail target is the depth-1 state of the last byte
  uint32_t s2_lo;
  uint32_t s2_hi;
  // match_longest only: bit B set <=> the state with base B carries one of Cedar's stale END flags (cedar_replay.cpp);
  // null when there is none
  const uint32_t *stale_bits;
  const uint32_t *term_bits;   // match_longest: one bit per slot, set at the base of a state that ends a key AND has children
                               // (its Cedar node keeps the value in a label-0 child, which a NUL byte reaches; kernels.hip)
};

struct MatchArgs {
  const uint8_t *text;
  const uint64_t *doc_off;   // [D+1]
  uint64_t n_docs;
  uint64_t n_bytes;
  uint64_t n_chunks;
  uint32_t chunk;            // bytes per chunk (multiple of 16)
  int32_t chars;             // 1: String overload, char offsets (matcher.cr:34-39)
  int32_t sep;               // 1: match(seq, sep) (ac.cr:321-340)
  uint32_t sep_block[8];     // bit c set <=> (c < sep.size && !sep[c])
  int32_t has_nul;           // match_longest, chunked form: the batch holds NUL bytes (the warm-ups look for them)
  int32_t no_filter;         // host side: this call has been handed back by the prefix-filter engine (scan_filter.hip)
  int32_t no_pair;           // ... by the pair engine (scan_pair.hip)
  int32_t check_docs;        // host side: the device-resident doc offsets have not been validated yet -- the single-traversal
                             // pipelines do it on the device, in front of the traversal, without a round trip to the host
  // scratch
  uint32_t *counts;          // [n_chunks] hits per chunk
  uint32_t *leads;           // [n_chunks] UTF-8 lead bytes per chunk (chars mode)
  uint64_t *blk_hits;        // [n_blocks] per-block sums, then exclusive bases
  uint64_t *blk_leads;       // [n_blocks]
  uint64_t *docg;            // [D+1] absolute lead-byte count at each doc start
  uint64_t *totals;          // [2] total hits, total leads
  // outputs
  aha_hit *out;
  uint64_t cap;
  uint64_t *doc_hit_off;     // [D+1] or null
  // count calls (aha_ac_count_batch*): no hit is written; the pipelines add per key instead (scan_count.hip)
  int32_t count_only;                // host side: the call counts (its pipeline, its repeats: engine.cpp device_count)
  unsigned long long *kc_visits;     // [K] events per head key (the two-pass engine's k_count<.., true> without a separator filter)
  unsigned long long *kc_hits;       // [K] hits per key (k_count<.., true> with a separator filter: per hit, both neighbour tests)
  unsigned long long *kc_out;        // [K] the caller's key counts (the chain pass adds into them)
  int32_t neutral;                   // host side: a match inside a document-count call -- the handle's back-off state is read, not written
  // cover calls (aha_ac_cover_batch*): a count call without key counts whose events leave one span each in a bit mask
  // (scan_cover.hip; the two-pass engine: k_count's cover mode)
  uint32_t *cover_mask;              // bit cover_bit0 + j = byte j of this batch; null: not a cover call
  uint64_t cover_bit0;               // the batch's first byte in the mask (a document range of a larger batch)
  int32_t cover_clear;               // host side: the pass clears the mask itself, once it knows the offsets are good
  // host side, a handle compiled with AHA_OPT_FOLD_ASCII: `text` is still the caller's (16-byte aligned) and not folded yet.  The
  // prefix-filter engine reads it as it is and folds in its loads; every other path takes the folded copy first (engine.cpp
  // stage_folded), which clears this.  The value is the handle's fold mode (handle.hpp): 1 ASCII, 2 simple, 3 BMP, 4 kana -- from 2 on the
  // prefix-filter engine takes the folded copy too (its loads fold ASCII only)
  int32_t fold;
};

constexpr int kBlock = 256;  // threads per block in the traversal kernels

// ---- single-traversal engine (scan_v2.hip) ---------------------------------
constexpr int kV2Threads = 1024;      // one persistent workgroup per CU
constexpr int kV2Piece = 32;          // input bytes staged per lane per round (multiple of 16)
constexpr uint32_t kV2Slab = 512;     // event records a wave reserves per atomic
constexpr uint32_t kV2MaxS = 32768;   // super-chunk bytes per lane (rel/seq fit 15/16 bits)

// One record per position whose state ends a key (fetch is expanded later):
//   x = chunk id, y = seq << 16 | last_byte_of_doc << 15 | rel (pos - chunk start),
//   z = end offset inside the document (bytes), w = key id (wide) / state base (compact)
struct V2Args {
  const uint8_t *text;
  const uint64_t *doc_off;
  uint64_t n_docs;
  uint64_t n_bytes;
  uint64_t n_chunks;
  uint32_t S;                // super-chunk bytes per lane, multiple of 64
  uint32_t lds_slots;        // automaton slots cached in LDS (prefix of the image)
  int32_t chars;
  int32_t sep;
  uint32_t sep_block[8];
  // traversal outputs
  uint4 *ev;                 // [ev_cap] event records in arrival order
  uint32_t *ev_aux;          // [ev_cap] chars mode: lead count << 1 | exact
  uint64_t ev_cap;
  unsigned long long *cursor;  // [0] next free record, [1] overflow flag
  uint32_t *slab_used;       // [ev_cap / kV2Slab + 1] valid records per slab
  uint32_t *ev_cnt;          // [n_chunks] events per chunk
  uint32_t *lead_cnt;        // [n_chunks] chars: lead bytes per chunk
  uint32_t *chunk_doc0;      // [n_chunks] chars: document containing the chunk start
  uint32_t *doc_ev_rank;     // [D+1] events of the chunk before the document start
  uint32_t *doc_lead_rank;   // [D+1] chars: lead bytes of the chunk before the document start
  // post passes
  uint64_t *ev_base;         // [n_chunks] exclusive scan of ev_cnt
  uint64_t *lead_base;       // [n_chunks] exclusive scan of lead_cnt
  uint64_t *blk_a;           // block sums / bases scratch
  uint64_t *blk_b;
  uint4 *sorted_ev;          // [ev_cap] {key, end_b, chunk, y} in final order
  uint32_t *sorted_aux;      // [ev_cap]
  uint32_t *sorted_cnt;      // [ev_cap] hits per event
  uint64_t *totals;          // [0] hits [1] leads [2] events
  // direct event regions (plain mode): chunk c stores its events in order at evd[c * ev_stride + seq], so the
  // post passes need no sort: count (wave per chunk) -> scan -> expand (wave per chunk)
  int32_t direct;
  int32_t dense_hits;        // THIS call's capacity allows for more than one hit per 4 input bytes (capi.cpp match_v2)
  uint32_t ev_stride;        // events a chunk may store (S / 4); more -> overflow flag, slab pipeline instead
  uint2 *evd;                // [n_chunks * ev_stride] {state base (compact) or key id, end offset in the document}
  uint32_t *evg;             // [n_chunks * ev_stride * 3] character-level traversal: the events of 64 chunks (a wave) together,
                             // in the order of the wave's trips: {END state base | lane | min(hits, 255) (unit.hpp u_rec_x / u_rec_z), end offset
                             // in the document, hits of the chunk before the event}
  uint32_t *doc_hit_rank;    // [D+1] character-level traversal: hits of the chunk before the document start (exact when no
                             // event stands for more than 15 hits: the record carries the count in bits 28..31 then)
  uint32_t unit_bb;          // character-level traversal: base width of the image (event records: base | lane << bb | hits << bb + 6)
  uint32_t *chunk_hits;      // [n_chunks]
  uint64_t *hit_base;        // [n_chunks] exclusive scan of chunk_hits
  aha_hit *out;
  uint64_t cap;
  uint64_t *doc_hit_off;
  // region pipelines: where the call's last kernel -- the per-document offsets -- leaves the five words the host reads
  // (cursor[0..1], totals[0..2]: k_publish_words as a launch of its own costs ~5 us of a 64 MiB call); null: nobody publishes
  unsigned long long *publish;
  // the 16 counter words of the NEXT call on this scratch, cleared by the same kernel (engine.cpp: Scratch::cursor_phase); null: nobody clears
  unsigned long long *clear_next;
  // the region pipeline's expansion launch: its blocks from doc_from on compute the documents' hit offsets (0: a launch of their own)
  uint32_t doc_from, doc_lanes16;
};

// ---- character-level engine (scan_unit.hip, unit.hpp) ---------------------------
struct UnitDev {
  const uint2 *slots;      // [n_slots] {lo, hi} entries
  const uint32_t *root;    // [n_syms] the root's transitions by symbol
  const uint32_t *tables;  // [kUTabWords] decode tables
  uint32_t n_slots;
  uint32_t big_lo;         // bases from here on are big states: a private block each (unit.hpp, BIG STATES)
  uint32_t n_low;          // symbols below it index a big state's block directly, the others a group record
  uint32_t g0;             // group record of symbol s: base + g0 + (s >> 5)
  uint32_t base_bits;      // 22 or 23 (unit.hpp, BASE WIDTH)
  uint32_t n_syms;
  uint32_t max_len;        // longest key, bytes
  uint32_t hdr_beside;     // 1: the traversal requests a state's header beside its probe (scan_unit.hip ku_traverse<.., HB>)
};
size_t unit_lds_bytes(uint32_t n_syms);
int unit_prepare(uint32_t n_syms);  // raises the dynamic-LDS limit; hipError_t as int
void unit_launch_traverse(const UnitDev &U, const V2Args &M, uint32_t grid, void *stream);
void unit_launch_regroup(const DevAut &A, const V2Args &M, void *stream);  // evg -> evd + chunk_hits (replaces k2d_count)
// evg + hit_base -> out, doc_hit_off: the whole expansion in one pass over the wave-ordered events.  uend[base] of an END
// state = {key | (key length & 255) << 24, offset of its flattened output chain | (key length >> 8) << 24}
void unit_launch_expand(const uint2 *uend, const DevAut &A, const V2Args &M, uint32_t workgroups, void *stream);
void v2_launch_hit_scan(const V2Args &M, void *stream);   // chunk_hits -> hit_base, totals[0]
void v2_launch_lead_scan(const V2Args &M, void *stream);  // lead_cnt -> lead_base, totals[1] (char offsets)

// ---- skip-ahead traversal over the unit image (scan_skip.hip; unit.hpp, MARKS)
struct SkipDev {
  const uint32_t *bloom;  // [1 << log2] blocked Bloom filter over the two-unit paths, keyed by raw bytes
  uint32_t log2;
  uint32_t k1;            // the second unit's multiplier of the pair hash (UnitImage::pair_k1)
};
int skip_prepare(uint32_t n_syms, uint32_t log2_words);  // raises the dynamic-LDS limits; hipError_t as int
size_t skip_bitmap_bytes(uint64_t n_bytes);             // scratch of a call: one bit per byte position, padded
// ks_mark: text -> bitmap (bit p: a two-unit path may start at p).  ks_traverse: ku_traverse's walk and outputs (evg, ev_cnt,
// chunk_hits, doc_*_rank), started only at marked positions.
void skip_launch_mark(const SkipDev &K, const V2Args &M, void *bitmap, uint32_t grid, void *stream);
void skip_launch_traverse(const UnitDev &U, const V2Args &M, const void *bitmap, uint32_t grid, void *stream);

// ---- pair engine (scan_pair.hip; unit.hpp, PAIR TABLE)
struct PairDev {
  const uint32_t *bloom;   // the marks' filter
  const uint4 *tab;        // [1 << log2] {raw0 | hits << 24, raw1, event payload (0: none), child filter}
  const uint8_t *disp;     // [groups]
  uint32_t bloom_log2, k1, log2, groups;
};

int pair_prepare(uint32_t n_syms, uint32_t bloom_log2, uint32_t groups);  // raises the dynamic-LDS limits; hipError_t as int
uint32_t pair_tile_bytes();                 // a tile of kp_pairs = a chunk of the event regions (V2Args.S)
size_t pair_cand_bytes(uint64_t cap);       // scratch: the deep candidates' list and what kp_walk finds for each
size_t pair_walk_bytes(uint64_t cap);
// tile_dn: n_chunks words; V2Args.lead_cnt / chunk_doc0 (free with byte offsets): a tile's first candidate and their number;
// cursor[7]: the list's length.  mid_event (nullable): recorded behind kp_pairs.
void pair_launch(const PairDev &P, const UnitDev &U, const DevAut &A, const V2Args &M, void *tile_dn, void *cand, void *wres,
                 uint64_t cand_cap, uint32_t grid, void *mid_event, void *stream);

// ---- prefix-filter engine (scan_filter.hip): byte-level, for batches where few positions can start a key
constexpr uint32_t kFilterMul = 0x9E3779B1u;  // an entry of the filter: scan_filter.hip kf_filter, capi.cpp filter_entry
constexpr uint32_t kFilterLog2 = 14;  // 2^14 words = 64 KiB: blocked Bloom filter over the keys' first D bytes
struct FilterDev {
  const uint32_t *bloom;
  uint32_t d;     // bytes of a key the filter looks at: min(4, shortest key)
  uint32_t log2;  // the filter has 2^log2 words (10 .. kFilterLog2)
};
// kf_walk keeps the image in LDS, beside its 16 waves' candidate lists, when both fit (chunks of 32 KiB: 57 KiB of image, 4 KiB: 115)
bool filter_image_in_lds(uint32_t n_slots, uint32_t chunk_bytes, bool chars = false);
int filter_prepare();  // once per process, before the first launch (LDS beyond 64 KiB is opt-in)
// filter_launch_filter: bitmap (one bit per byte position of M.text) and -- on the same launch -- the chunk records of chunks
// of M.S bytes (4, 8, 16 or 32 KiB; chunk_rec: n_chunks * filter_chunk_rec_bytes() of scratch).  non_ascii (nullable): set
// to 1 when the batch holds a byte >= 0x80; kf_walk then hands the call back (cursor[1] = 3).
// filter_launch_walk: bitmap + records -> evd / ev_cnt / doc_ev_rank.
size_t filter_chunk_rec_bytes();
void filter_launch_filter(const FilterDev &F, const V2Args &M, void *bitmap, void *chunk_rec, unsigned long long *non_ascii,
                          uint32_t cus, void *stream);
void filter_launch_walk(const DevAut &A, const V2Args &M, const void *bitmap, const void *chunk_rec, const unsigned long long *non_ascii,
                        uint32_t cus, void *stream);

// the same two launches for a folded handle (AHA_OPT_FOLD_ASCII): every text load folds (fold.hpp), M.text is the caller's
void filter_launch_filter_fold(const FilterDev &F, const V2Args &M, void *bitmap, void *chunk_rec, unsigned long long *non_ascii,
                               uint32_t cus, void *stream);
void filter_launch_walk_fold(const DevAut &A, const V2Args &M, const void *bitmap, const void *chunk_rec,
                             const unsigned long long *non_ascii, uint32_t cus, void *stream);
// scan_fold.hip: dst[j] = fold(src[j]) for j < n_bytes; src any byte address, dst 16-byte aligned; src is only read
void fold_launch_copy(const uint8_t *src, uint8_t *dst, uint64_t n_bytes, uint32_t max_blocks, void *stream);
// ... with AHA_OPT_FOLD_SIMPLE: dst = fold2 (fold.hpp) of every document of src on its own.  doc_offsets (device, n_docs + 1
// entries; the first is subtracted from the others) are those of exactly these n_bytes: a batch or a range of whole documents
void fold2_launch_copy(const uint8_t *src, uint8_t *dst, uint64_t n_bytes, const uint64_t *doc_offsets, uint64_t n_docs,
                       uint32_t max_blocks, void *stream);
// ... with AHA_OPT_FOLD_BMP: dst = fold3 of every document of src on its own, the same arguments
void fold3_launch_copy(const uint8_t *src, uint8_t *dst, uint64_t n_bytes, const uint64_t *doc_offsets, uint64_t n_docs,
                       uint32_t max_blocks, void *stream);
// (the second step of it alone, and the grid of the staged copies: a workgroup per 1024 pieces, max_blocks at the most)
void fold3_launch_fix(const uint8_t *src, uint8_t *dst, uint64_t n_bytes, const uint64_t *doc_offsets, uint64_t n_docs,
                      uint32_t max_blocks, void *stream);
uint32_t fold_grid(uint64_t n_bytes, uint32_t max_blocks);
// ... with AHA_OPT_FOLD_KANA: dst = foldk of every document of src on its own, the same arguments (a kernel of its own,
// scan_foldk.hip)
void foldk_launch_copy(const uint8_t *src, uint8_t *dst, uint64_t n_bytes, const uint64_t *doc_offsets, uint64_t n_docs,
                       uint32_t max_blocks, void *stream);

size_t v2_lds_bytes(uint32_t lds_slots, bool compact);
int v2_prepare(bool compact, size_t lds_bytes);  // raises the dynamic-LDS limit; hipError_t as int
void v2_launch_traverse(const DevAut &A, const V2Args &M, uint32_t grid, void *stream);
// scans ev_cnt (and lead_cnt) into ev_base / lead_base; totals[2] = events, totals[1] = leads
void v2_launch_chunk_scan(const V2Args &M, void *stream);
void v2_launch_sort(const DevAut &A, const V2Args &M, uint64_t n_records, void *stream);
void v2_launch_expand(const DevAut &A, const V2Args &M, uint64_t n_events, void *stream);
// direct pipeline (plain mode): per-chunk hit counts, their scan, expansion and document offsets
void v2_launch_direct_post(const DevAut &A, const V2Args &M, void *stream, void *ev_mid, bool counted = false);
// the count path of the same pipeline: per-chunk hit counts (unless counted) and their scan; then the documents' offsets
void v2_launch_count_post(const DevAut &A, const V2Args &M, void *stream, bool counted);
void v2_launch_doc_offsets(const DevAut &A, const V2Args &M, void *stream);
void unit_launch_doc_offsets(const V2Args &M, void *stream);  // the fused path's document offsets (ku_doc_offsets)
// count path (scan_count.hip): events per head key from the region records (uend null) or the character-level traversal's
// wave-ordered records (uend = its END table); then key_counts[j] += visits[h] for every j on chain(h)
void count_launch_visits(const DevAut &A, const V2Args &M, const uint2 *uend, unsigned long long *visits, uint32_t max_blocks,
                         void *stream);
void count_launch_chain(const uint2 *key_ln, uint32_t n_keys, const unsigned long long *visits, unsigned long long *out,
                        const unsigned long long *abortf, void *stream);

// cover path (scan_cover.hip): the mask's words cleared unless *abortf; one span per event of the pass into mask (records as
// for count_launch_visits; cdoc: n_chunks + 1 words of scratch, the chunks' first documents); the passes over the finished mask
void cover_launch_clear(uint32_t *words, uint64_t n_words, const unsigned long long *abortf, uint32_t max_blocks, void *stream);
void cover_launch_spans(const DevAut &A, const V2Args &M, const uint2 *uend, uint64_t *cdoc, uint32_t *mask, uint64_t bit0,
                        uint32_t max_blocks, void *stream);
void cover_launch_redact(const uint8_t *src, uint8_t *dst, const uint32_t *mask, uint64_t n_bytes, uint8_t fill, uint32_t max_blocks,
                         void *stream);
void cover_launch_doc_covered(const uint32_t *mask, const uint64_t *doc_off, uint64_t n_docs, uint64_t *doc_covered,
                              uint32_t max_blocks, void *stream);
void cover_launch_total(const uint32_t *mask, uint64_t n_words, uint64_t *total, uint32_t max_blocks, void *stream);

// document counts (scan_doccount.hip; engine.cpp device_doc_counts).  One unit of work of its kernels: `n` hits from hit
// `begin` of the range's hit buffer; `doc` = the document within the range (kdc_add: the row of the slice's document); `out`
// = where the document's pairs go for the time being.
struct DcItem {
  uint64_t begin;
  uint32_t *out;
  uint32_t n;
  uint32_t doc;
};
constexpr uint32_t kDcSortMax = 4096;      // ids kdc_sort holds in LDS
constexpr uint32_t kDcRangeKeys = 8192;    // counts kdc_range holds in LDS
constexpr uint32_t kDcSliceHits = 1u << 16;  // hits of one slice of kdc_add
void doccount_launch_sort(const DcItem *items, uint32_t n_items, const void *hits, uint32_t *n_pairs, void *stream);
void doccount_launch_range(const DcItem *items, uint32_t n_items, const void *hits, uint32_t n_keys, uint32_t range_keys,
                           uint32_t *n_pairs, void *stream);
void doccount_launch_add(const DcItem *slices, uint32_t n_slices, const void *hits, uint32_t *rows, uint32_t n_keys,
                         uint32_t max_blocks, void *stream);
void doccount_launch_compact(const DcItem *docs, uint32_t n_rows, uint32_t *rows, uint32_t n_keys, uint32_t *n_pairs, void *stream);
void doccount_launch_compact64(const DcItem *doc, unsigned long long *row, uint32_t n_keys, uint32_t *n_pairs, void *stream);
void doccount_launch_gather(const uint64_t *pair_off, const uint32_t *const *src, uint64_t n_docs, uint64_t n, void *out,
                            void *stream);

// select path (scan_select.hip; engine.cpp device_select), over one range of whole documents: nd documents at rel[0 .. nd] of nb
// bytes of text, their n_hits hits in `hits` (hit_off[d] - hit_off[0]: the first hit of document d).  L: nb words of 8 bytes,
// clear; cover / doc_start / select: nb bits each, clear; blk: select_rank_blocks(nb) + 1 words of 8 bytes -- after
// select_launch_rank the selected hits before every block of the select mask, the range's total in the last word.
uint64_t select_rank_blocks(uint64_t n_bytes);
void select_launch_longest(const void *hits, uint64_t n_hits, const uint64_t *hit_off, const uint64_t *rel, uint64_t nd, uint64_t nb,
                           uint64_t *L, uint32_t max_blocks, void *stream);
void select_launch_marks(const uint64_t *L, uint64_t nb, const uint64_t *rel, uint64_t nd, uint32_t *cover, uint32_t *doc_start,
                         uint32_t max_blocks, void *stream);
void select_launch_walk(const uint64_t *L, uint64_t nb, const uint32_t *cover, const uint32_t *doc_start, uint32_t *select,
                        uint32_t max_blocks, void *stream);
void select_launch_rank(const uint32_t *select, uint64_t nb, uint64_t *blk, uint32_t max_blocks, void *stream);
void select_launch_rank_docs(const uint32_t *select, const uint64_t *blk, const uint64_t *rel, uint64_t nd, uint64_t base,
                             uint64_t *out, uint32_t max_blocks, void *stream);
void select_launch_emit(const uint32_t *select, uint64_t nb, const uint64_t *blk, const uint64_t *L, const uint64_t *rel, uint64_t nd,
                        void *out, uint32_t max_blocks, void *stream);

// token path (scan_tokens.hip; engine.cpp device_select_to with AHA_SELECT_TOKENS), over one range after select_launch_walk;
// nb > 0.  S / T: ceil(nb / 32) whole words each; S clear.
// S: the bytes inside a selected hit
void tokens_launch_spans(const uint64_t *L, uint64_t nb, const uint32_t *select, uint32_t *S, uint32_t max_blocks, void *stream);
// T: where a token starts (token_rule.hpp); text: the caller's bytes of the range, any alignment, not read with gap_runs
void tokens_launch_starts(const uint8_t *text, uint64_t nb, const uint32_t *select, const uint32_t *S, const uint32_t *doc_start,
                          bool gap_runs, uint32_t *T, uint32_t max_blocks, void *stream);
// out[0, total): the tokens of the ranked T (blk: select_launch_rank over T) as {start, end, value or -1}, relative to their documents
void tokens_launch_emit(const uint32_t *T, uint64_t nb, const uint64_t *blk, const uint32_t *select, const uint32_t *doc_start,
                        const uint64_t *L, const uint64_t *rel, uint64_t nd, void *out, uint32_t max_blocks, void *stream);

// replace path (scan_replace.hip; engine.cpp device_replace), over the whole batch: its selection sel[0, n) (document by
// document, dso[0 .. n_docs] the documents' offsets into it, dso[n_docs] = n) and the replacement table on the device.
struct RepEntry {   // one key of a replacement table
  uint64_t off;     // its replacement's first byte in the blob
  uint32_t len;     // ... and its length
  uint32_t keep;    // != 0: hits of this key stay as they are
};
constexpr uint32_t kRpScanBlock = 256;  // items of one block of the scan: an item per lane
inline uint64_t replace_scan_blocks(uint64_t n) { return (n + kRpScanBlock - 1) / kRpScanBlock; }
// start[j] = the hit's first byte in the corpus, shift[j] = its change of length (delta)
void replace_launch_delta(const void *sel, uint64_t n, const uint64_t *dso, const uint64_t *doc_off, uint64_t n_docs,
                          const RepEntry *ent, uint32_t n_keys, uint64_t *start, int64_t *shift, uint32_t max_blocks, void *stream);
// shift[0, n) in place: the deltas -> their exclusive sums, shift[n] = their total; sums: replace_scan_blocks(n) + 1 words
void replace_launch_scan(int64_t *shift, uint64_t n, int64_t *sums, uint32_t max_blocks, void *stream);
// doc_out[d] = doc_off[d] + shift[dso[d]] for d in [0, n_docs]
void replace_launch_doc_offsets(const uint64_t *doc_off, const uint64_t *dso, const int64_t *shift, uint64_t n_docs,
                                uint64_t *doc_out, uint32_t max_blocks, void *stream);
// out[0, total): the substituted copy
void replace_launch_copy(const uint8_t *text, const void *sel, const uint64_t *start, const int64_t *shift, uint64_t n,
                         const RepEntry *ent, uint32_t n_keys, const uint8_t *blob, uint8_t *out, uint64_t total,
                         uint32_t max_blocks, void *stream);

// records and grep paths (scan_grep.hip; engine.cpp device_records, device_grep).  Masks are ranked by select_launch_rank.
// mask[0, ceil(n_bytes / 32)): bit p = (corpus[p] == delim) or p + 1 is a document's end; the corpus may have any alignment
void grep_launch_ends(const uint8_t *corpus, uint64_t n_bytes, uint8_t delim, const uint64_t *doc_off, uint64_t n_docs, uint32_t *mask,
                      uint32_t max_blocks, void *stream);
// rec_off[0] = 0, rec_off[r + 1] = p + 1 for the r-th set bit p of the ranked mask
void grep_launch_emit_ends(const uint32_t *mask, uint64_t n_bytes, const uint64_t *blk, uint64_t *rec_off, uint32_t max_blocks,
                           void *stream);
// keep / S / T: ceil(n_docs / 32) words each, from the documents' hit offsets dho[0 .. n_docs]
void grep_launch_flag(const uint64_t *dho, uint64_t n_docs, bool invert, uint32_t *keep, uint32_t *S, uint32_t *T, uint32_t max_blocks,
                      void *stream);
// the dropped runs as replace's copy takes them: start[j], shift[j] = delta[j] (n_runs + 1 words: the scan's), sel[j] (12 bytes
// each), ent[0] = the empty replacement
void grep_launch_runs(const uint32_t *S, const uint32_t *T, uint64_t n_docs, const uint64_t *blk_s, const uint64_t *blk_t,
                      const uint64_t *doc_off, uint64_t n_runs, uint64_t *start, int64_t *shift, void *sel, RepEntry *ent,
                      uint32_t max_blocks, void *stream);
// kept_docs[r], doc_out[r] for the kept documents in order (either may be null), doc_out[n_kept] = the total
void grep_launch_emit_docs(const uint32_t *keep, const uint32_t *S, uint64_t n_docs, const uint64_t *blk_k, const uint64_t *blk_s,
                           const uint64_t *doc_off, const int64_t *shift, uint64_t n_runs, uint64_t *kept_docs, uint64_t *doc_out,
                           uint32_t max_blocks, void *stream);

// excerpts path (scan_excerpt.hip; engine.cpp device_excerpts), from the cover mask M of the batch (one bit per text byte).
// Masks are ranked by select_launch_rank; the gaps go to replace_launch_scan and replace_launch_copy as grep's dropped runs do.
// S / T: ceil(n_bytes / 32) whole words each: a covered run of one document starts / ends at the bit
void excerpt_launch_edges(const uint32_t *M, uint64_t n_bytes, const uint64_t *doc_off, uint64_t n_docs, uint32_t *S, uint32_t *T,
                          uint32_t max_blocks, void *stream);
// run j, delimited by the j-th bits of S and T: its document, its window [w0[j], w1[j]) (excerpt_window.hpp; corpus: the
// caller's bytes, any alignment), and the masks over runs first / last, ceil(n_runs / 32) whole words each
void excerpt_launch_windows(const uint32_t *S, const uint32_t *T, uint64_t n_bytes, const uint64_t *blk_s, const uint64_t *blk_t,
                            const uint8_t *corpus, const uint64_t *doc_off, uint64_t n_docs, uint32_t before, uint32_t after,
                            uint64_t n_runs, uint64_t *doc, uint64_t *w0, uint64_t *w1, uint32_t *first, uint32_t *last,
                            uint32_t max_blocks, void *stream);
// the n_exc + 1 stretches outside the excerpts as replace's copy takes them: start[j], shift[j] = delta[j] (n_exc + 2 words:
// the scan's), sel[j] (12 bytes each), ent[0] = the empty replacement
void excerpt_launch_gaps(const uint32_t *first, const uint32_t *last, uint64_t n_runs, const uint64_t *blk_f, const uint64_t *blk_l,
                         const uint64_t *w0, const uint64_t *w1, uint64_t n_bytes, uint64_t n_exc, uint64_t *start, int64_t *shift,
                         void *sel, RepEntry *ent, uint32_t max_blocks, void *stream);
// starts[r] for r in [0, n_exc), out_off[r] for r in [0, n_exc] from the scanned shift (either may be null)
void excerpt_launch_emit(const uint64_t *start, const int64_t *shift, uint64_t n_exc, uint64_t *starts, uint64_t *out_off,
                         uint32_t max_blocks, void *stream);

// rule grep (scan_greprule.hip; engine.cpp device_grep_rule).  rows: the class counts, n_classes words per document.
// terms: HOST memory, at most kRuleMaxTerms, in any order and with any group ids (they travel as a kernel argument).
// keep[0, ceil(n_docs / 32)): bit d = (the rule passes for document d) != invert, whole words, the bits from n_docs on 0
constexpr uint32_t kRuleMaxTerms = 64;
constexpr uint32_t kRuleChunkClasses = 32;  // columns of the table a wave stages through LDS at a time, for its 64 rows
void greprule_launch_keep(const uint32_t *rows, uint32_t n_classes, const uint64_t *doc_off, uint64_t n_docs,
                          const aha_rule_term *terms, uint32_t n_terms, bool invert, uint32_t *keep, uint32_t max_blocks, void *stream);
// S / T from keep alone, ceil(n_docs / 32) whole words each: a run of dropped documents starts / ends at the bit
void greprule_launch_edges(const uint32_t *keep, uint64_t n_docs, uint32_t *S, uint32_t *T, uint32_t max_blocks, void *stream);

// context lines (scan_greplines.hip; engine.cpp device_grep_lines), from the match mask m of the batch (one bit per record, the
// bits from n_docs on 0).  goff: the checked group offsets, n_groups + 1 entries, or null (one group).  Masks are ranked by
// select_launch_rank.
// Sm / Tm: ceil(n_docs / 32) whole words each: a run of matching records of one group starts / ends at the bit
void greplines_launch_edges(const uint32_t *m, uint64_t n_docs, const uint64_t *goff, uint64_t n_groups, uint32_t *Sm, uint32_t *Tm,
                            uint32_t max_blocks, void *stream);
// run j, delimited by the j-th bits of Sm and Tm: its group and its window [w0[j], w1[j]) in records; then the two ends of every
// chunk (the merged windows of one group) XOR-ed into tog, ceil((n_docs + 1) / 32) words that the caller cleared
void greplines_launch_windows(const uint32_t *Sm, const uint32_t *Tm, uint64_t n_docs, const uint64_t *blk_s, const uint64_t *blk_t,
                              const uint64_t *goff, uint64_t n_groups, uint32_t before, uint32_t after, uint64_t n_runs, uint64_t *grp,
                              uint64_t *w0, uint64_t *w1, uint32_t *tog, uint32_t max_blocks, void *stream);
// keep[0, ceil(n_docs / 32)): bit r = an odd number of toggles lies at or in front of r (blk_x: tog ranked over n_docs + 1 bits)
void greplines_launch_fill(const uint32_t *tog, const uint64_t *blk_x, uint64_t n_docs, uint32_t *keep, uint32_t max_blocks,
                           void *stream);
// is_match[i] = bit d of m for the i-th set bit d of the ranked keep mask
void greplines_launch_emit_match(const uint32_t *keep, const uint64_t *blk_k, uint64_t n_docs, const uint32_t *m, uint8_t *is_match,
                                 uint32_t max_blocks, void *stream);

// class-counts path (scan_classcount.hip; engine.cpp device_class_counts), over one range of whole documents: its n_hits hits in
// `hits` (hit_off[d] - hit_off[0]: the first hit of document d of its nd), key k's classes cls_ids[cls_off[k] .. cls_off[k+1]),
// out: the row of the range's first document (n_classes words per document, cleared before the call's first range).
// Starting values, not tuned ones:
constexpr uint32_t kCcSlice = 2048;  // consecutive hits one workgroup takes at a time
constexpr uint32_t kCcTable = 8192;  // words of its LDS table (32 KiB): (documents of a slice) x n_classes beyond it adds to HBM directly
void classcount_launch_add(const void *hits, uint64_t n_hits, const uint64_t *hit_off, uint64_t nd, const uint64_t *cls_off,
                           const uint32_t *cls_ids, uint32_t n_keys, uint32_t n_classes, uint32_t *out, uint32_t max_blocks,
                           void *stream);
// one document's hits per key (a count call over it alone) added into its row
void classcount_launch_fold_keys(const uint64_t *key_counts, uint32_t n_keys, const uint64_t *cls_off, const uint32_t *cls_ids,
                                 uint32_t *row, uint32_t max_blocks, void *stream);

// exchange format of the multi-GPU all-gatherv (kernels.hip): {end, value} pairs <-> Hit triples
void launch_hits_pack(const int32_t *hits, uint64_t n, int32_t *pairs, void *stream);
void launch_hits_unpack(const DevAut &A, const int32_t *pairs, uint64_t n, int chars, int32_t *hits, void *stream);
// 4-byte exchange stream (kernels.hip): stream_words holds n + ceil(n/1024) + exceptions words (capacity 2n + ceil(n/1024))
// field widths of the 4-byte exchange stream's words (kernels.hip): value << (step_bits + len_bits) | len << step_bits | step
struct StreamFmt {
  uint32_t step_bits;  // 6..12; 2^step_bits - 1 = exception
  uint32_t len_bits;   // 0: the key's length is not carried (looked up on arrival)
};
void launch_hits_pack4(const int32_t *hits, uint64_t n, uint32_t *stream_words, unsigned long long *n_words, StreamFmt F,
                       void *stream);
void launch_hits_unpack4(const DevAut &A, const uint32_t *stream_words, uint64_t n, int chars, int32_t *hits, StreamFmt F,
                         void *stream);
// several streams in one launch: stream k starts at word word_off[k] of `land`, holds n_hits[k] hits, goes to hits[out_off[k]..]
constexpr uint32_t kMaxSegs = 64;
void launch_hits_unpack4_segs(const DevAut &A, const uint32_t *land, const uint64_t *word_off, const uint64_t *n_hits,
                              const uint64_t *out_off, uint32_t n_segs, int chars, int32_t *hits, StreamFmt F, void *stream);

// flag[0] |= 1: not the offsets of n_docs documents over n_bytes; |= 2: a document of 2^31 bytes or more
void launch_publish_words(const unsigned long long *src, unsigned long long *host_dst, int n, void *stream);
void launch_check_docs(const uint64_t *doc_off, uint64_t n_docs, uint64_t n_bytes, uint32_t *flag, unsigned long long *abort_word,
                       void *stream);

// launchers (kernels.hip)
void launch_count(const DevAut &A, const MatchArgs &M, void *stream);
void launch_scan_blocks(const MatchArgs &M, uint64_t n_blocks, void *stream);
void launch_count_doc_offsets(const MatchArgs &M, void *stream);  // count calls: k_count's per-document notes + chunk bases
void launch_docg(const MatchArgs &M, void *stream);
void launch_write(const DevAut &A, const MatchArgs &M, void *stream);
// match_longest (ac.cr:118-143): mode 1 = intersectable false (a thread per document), 2 = true (a thread per chunk,
// byte offsets), 3 = true with a thread per document (char offsets)
void launch_has_nul(const uint8_t *text, uint64_t n, uint64_t *flag, void *stream);  // *flag = 1 when the text holds a NUL byte
void launch_longest(const DevAut &A, const MatchArgs &M, int mode, bool write, void *stream);

}  // namespace aha
