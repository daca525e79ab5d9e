// handle.hpp -- what capi.cpp (the C ABI: compile, export, buffers, the host entry points) and engine.cpp (which kernels answer a
// call: engine choice, pipelines, retries, the prefix filter's back-off) share: the handle, a call's scratch set and the helpers
// both sides use.  Library-internal; nothing here is exported (exports.map).
#pragma once
#include <hip/hip_runtime_api.h>
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <atomic>
#include <functional>
#include <condition_variable>
#include <memory>
#include <mutex>
#include <new>
#include <thread>
#include <string>
#include <type_traits>
#include <vector>
#include "automaton.hpp"
#include "cedar_replay.hpp"
#include "image.hpp"
#include "feed.hpp"
#include "unit.hpp"
#include "internal.hpp"

namespace ahai {
using namespace aha;
struct Buf {
  void *p = nullptr;
  size_t bytes = 0;
};
// ---- the grow-only device buffers of a scratch set, by family; every slot has a name (a wrong index is silent corruption)
// v2buf: one pass of the single-traversal engines (engine.cpp plan_v2 sizes them, launch_v2 binds them)
enum V2Slot {
  kEv,           // slab pipeline: the events as the traversal leaves them
  kSortedEv,     // slab pipeline: the events in chunk order
  kSortedCnt,    // slab pipeline: hits per sorted event
  kSlabUsed,     // slab pipeline: events per slab
  kEvCnt,        // events per chunk
  kDocEvRank,    // per document: its first event's rank
  kEvBase,       // events before every chunk
  kBlkA,         // block sums of the scans
  kBlkB,         // ... and their second array
  kCursor,       // TWO blocks of 16 counter words and a third of odd words (Scratch::cursor_*); a new buffer resets the cursor
  kEvAux,        // char offsets, slab pipeline: the events' lead counts
  kSortedAux,    // ... in chunk order
  kLeadCnt,      // char offsets: continuation bytes per chunk; the pair engine: its tiles' counts
  kChunkDoc0,    // char offsets / pair engine: every chunk's first document
  kDocLeadRank,  // char offsets: per document, the lead count before it
  kLeadBase,     // char offsets: lead counts before every chunk
  kEvRegions,    // region pipelines: the chunks' event regions, 8 bytes per event
  kText,         // the aligned and / or folded copy of a caller's text (stage_text)
  kChunkHits,    // region pipelines: hits per chunk
  kHitBase,      // region pipelines: hits before every chunk
  kDocHitRank,   // character-level engine: per document, its first hit's rank
  kEvGroups,     // character-level engine: the wave-ordered events, 12 bytes each
  kEngineA,      // the filter's candidate bitmap / the skip engine's marks / the pair engine's tile records
  kEngineB,      // the filter's chunk records / the pair engine's candidates
  kEngineC,      // the pair engine's deep walks
  kKeyVisits,    // count calls: events per head key (device_count)
  kV2Count
};
// hostbuf: device staging of the host-buffer entry points (capi.cpp)
enum HostSlot {
  kHostCorpus,   // the text (a cover call redacts it in place)
  kHostDocs,     // the document offsets, relative to their range
  kHostOffsets,  // what comes back per document: hit offsets, pair offsets, covered bytes
  kHostOut,      // what comes back per call: hits, key counts, pairs, the mask
  kHostCount
};
// cntbuf: count calls in document ranges (engine.cpp count_ranges)
enum CountSlot {
  kCntRel,   // the range's document offsets, relative to its first byte
  kCntText,  // the aligned copy of an unaligned range
  kCntDho,   // the range's hit offsets
  kCntCount
};
// dcbuf: document counts (engine.cpp device_doc_counts)
enum DocCountSlot {
  kDcHitOff,      // the documents' hit offsets (the count call in front)
  kDcHits,        // a range's hits
  kDcRel,         // the range's document offsets, relative to its first byte
  kDcText,        // the aligned copy of an unaligned range
  kDcItems,       // the work items
  kDcPairsPerDoc, // pairs per document
  kDcRows,        // the dense form's rows; a new buffer is not known to be clear (Scratch::dc_rows_clear)
  kDcRangePairs,  // the range form's pairs
  kDcGather,      // pair offsets + sources of the gather
  kDcSoloRow,     // one document's key counts (a document beyond the hit buffer's bound)
  kDcCount
};
// covbuf: cover calls (engine.cpp device_cover)
enum CoverSlot {
  kCovMask,       // the mask where the caller gives none
  kCovChunkDoc,   // the chunks' first documents
  kCovTotal,      // the total
  kCovCount
};
// selbuf: select calls (engine.cpp device_select)
enum SelectSlot {
  kSelHitOff,   // the documents' hit offsets (the count call in front)
  kSelHits,     // a range's hits
  kSelRel,      // the range's document offsets, relative to its first byte
  kSelText,     // the aligned copy of an unaligned range
  kSelLongest,  // L: per text byte of the range the longest hit that starts there, len << 32 | value
  kSelMasks,    // the cover, document-start and select masks, one bit per text byte each
  kSelBlocks,   // the selected hits before every 64 words of the select mask, the range's total behind them
  kSelDocOff,   // the documents' offsets into the selection, until the call is known to succeed
  kSelSpans,    // token calls: S, the bytes inside a selected hit, one bit per text byte
  kSelTokens,   // token calls: T, the token starts, one bit per text byte
  kSelCount
};
// repbuf: replace calls (engine.cpp device_replace)
enum ReplaceSlot {
  kRepSel,       // the selection of the whole batch, 12 bytes per selected hit
  kRepSelSpare,  // ... while it grows over document ranges: the larger buffer, then the two change places
  kRepStart,     // A: per selected hit its first byte in the corpus
  kRepShift,     // per selected hit the change of length in front of it, the total change behind the last
  kRepSums,      // the scan's block sums
  kRepDocOut,    // the documents' offsets into the result, until the call is known to succeed
  kRepCount
};
// fselbuf: feed select calls (feed.cpp feed_select; scan_feedselect.hip)
enum FeedSelectSlot {
  kFsHits,     // the call's true hits, piece by piece (kfd_merge into scratch)
  kFsHitOff,   // where each piece's lie
  kFsExtOff,   // the pieces' extended positions: offsets
  kFsBases,    // the sequences' lengths before the pieces
  kFsLongest,  // L: per extended position the longest hit that starts there, len << 32 | value
  kFsMasks,    // the cover, piece-start and select masks, one bit per extended position each
  kFsBlocks,   // the selected hits before every 64 words of the select mask, the total behind them
  kFsEnds,     // per piece the end of its last selected hit
  kFsSelOff,   // the pieces' offsets into the selection, until the call is known to succeed
  kFsCount
};
// ftokbuf: feed token calls (feed.cpp feed_tokens; scan_feedtokens.hip), beside a feed select call's fselbuf
enum FeedTokenSlot {
  kFtMasks,    // S, the bytes inside a selected hit, and T, the token starts, one bit per extended position each
  kFtBlocks,   // the token starts before every 64 words of T, the total behind them
  kFtPieces,   // per piece the cursors it finds and leaves, its flags and its token count (FeedTokPiece)
  kFtRawOff,   // the token starts in front of every piece's extended positions
  kFtTokOff,   // the pieces' offsets into the tokens, until the call is known to succeed
  kFtTotal,    // the call's token total and its verdict (one read-back)
  kFtCount
};
// frepbuf: feed replace calls (feed.cpp feed_replace; scan_feedreplace.hip, scan_replace.hip)
enum FeedReplaceSlot {
  kFrRows,    // the settled selection, piece by piece, relative to the piece (kfs_emit into scratch), 12 bytes each
  kFrExt,     // ext: the staged text T[c0 .. c1) of every piece
  kFrExtOff,  // where each piece's staged text lies
  kFrBias,    // ... and where its own first byte lies in it: ext_off + hold0
  kFrHold0,   // per piece the bytes between the cursor and the piece
  kFrStart,   // A: per settled hit its first byte in ext
  kFrShift,   // per settled hit the change of length in front of it, the total change behind the last
  kFrSums,    // the scan's block sums
  kFrOutOff,  // the pieces' offsets into the result, until the call is known to succeed
  kFrCount
};
// fsepbuf: calls on a feed with a separator filter (feed.cpp feed_sep_true, feed_finish_sep; scan_feedsep.hip)
enum FeedSepSlot {
  kFpEdge,     // per piece the hits that end on its context's last byte
  kFpTrueOff,  // where each piece's true hits lie
  kFpTrue,     // the call's true hits, piece by piece (kfd_merge into scratch), 12 bytes each
  kFpKeep,     // one bit per true hit: it survives the filter and is reported by this call
  kFpBlocks,   // the kept hits before every 2048 true hits, the total behind them
  kFpZeroOff,  // a finish call: the offsets of its empty pieces
  kFpCount
};
// grpbuf: records and grep calls (engine.cpp device_records, device_grep; scan_grep.hip)
enum GrepSlot {
  kGrpEnds,       // records: the record-end mask, one bit per text byte
  kGrpEndBlocks,  // records: the set bits before every 64 words of it, the total behind them
  kGrpHitOff,     // grep: the documents' hit offsets (the count call in front)
  kGrpDocMasks,   // grep: the keep, S and T masks, one bit per document each
  kGrpDocBlocks,  // grep: their three block ranks, each with its total behind it
  kGrpSel,        // grep: one synthesized selection row per dropped run, 12 bytes each
  kGrpStart,      // grep: A, per dropped run its first byte in the corpus
  kGrpShift,      // grep: per dropped run the change of length in front of it, the total change behind the last
  kGrpSums,       // grep: the scan's block sums
  kGrpTable,      // grep: the one-entry replacement table (the empty replacement)
  kGrpRows,       // rule grep: the D x C class counts where the caller gives no rows (bounded by AHA_RULE_TABLE_BYTES)
  kGrpExMasks,    // excerpts: the cover mask M, then S and T, one bit per text byte each
  kGrpExBlocks,   // excerpts: the block ranks of S and T, each with its total behind it
  kGrpExRuns,     // excerpts: per covered run its document, w0 and w1, 24 bytes
  kGrpExRunMasks, // excerpts: the first and last masks, one bit per run each
  kGrpExRunBlocks,// excerpts: their two block ranks, each with its total behind it (the gap rows: kGrpSel .. kGrpTable)
  kGrpLnMasks,    // context lines: the match mask m, Sm and Tm, one bit per record each, and the toggle mask of D + 1 bits
  kGrpLnBlocks,   // context lines: the block ranks of Sm, Tm and the toggle mask, each with its total behind it
  kGrpLnRuns,     // context lines: per matching run its group, w0 and w1, 24 bytes
  kGrpCount
};
// fgrpbuf: feed grep calls (feed.cpp feed_grep; scan_feedgrep.hip).  The fragments come from device_records, whose mask
// (grpbuf) is dead once they are emitted; nothing here shares a buffer with grpbuf or with another slot of this family
enum FeedGrepSlot {
  kFgFragOff,     // the fragments' offsets into the pieces' bytes
  kFgPieceFrag,   // the pieces' offsets into the fragments (piece_rec_offsets)
  kFgWinOff,      // the window batch [X | Y | Z]: its document offsets
  kFgWin,         // ... its bytes
  kFgWinHitOff,   // ... its per-document hit offsets
  kFgFragHitOff,  // the fragments' hit offsets, each matched from the root
  kFgFlags,       // per fragment: keep, has, closed
  kFgMasks,       // the keep, S and T masks, one bit per fragment each
  kFgBlocks,      // their three block ranks, each with its total behind it
  kFgSel,         // one synthesized selection row per dropped run, 12 bytes each
  kFgStart,       // A, per dropped run its first byte in the pieces' bytes
  kFgShift,       // per dropped run the change of length in front of it, the total change behind the last
  kFgSums,        // the scan's block sums
  kFgTable,       // the one-entry replacement table (the empty replacement)
  kFgCount
};
// flngbuf: calls on a longest feed (engine.cpp device_feed_longest_count; scan_feedlongest.hip)
enum FeedLongSlot {
  kFlEnd,  // the state at every piece's end, 16 bytes each (pass 1 writes it, kfl_commit moves it into the feed)
  kFlCount
};
// clsbuf: class-counts calls (engine.cpp device_class_counts; scan_classcount.hip)
enum ClassSlot {
  kClsHitOff,   // the documents' hit offsets (the count call in front)
  kClsHits,     // the hits of the range in flight, 12 bytes each
  kClsRel,      // the range's document offsets, relative to its first byte
  kClsText,     // the aligned copy of an unaligned range
  kClsSoloRow,  // one document's key counts (a document beyond the hit buffer's bound)
  kClsCount
};
// tpbuf: the two-pass engine and match_longest (engine.cpp bind_two_pass; kernels.hip, scan_feedlongest.hip)
enum TwoPassSlot {
  kTpCounts,    // hits per counter: a chunk, or a document of match_longest's per-document modes
  kTpLeads,     // char offsets: continuation bytes per chunk
  kTpBlkHits,   // block sums of the scan over the hits
  kTpBlkLeads,  // ... and over the leads
  kTpDocG,      // char offsets: per document, the lead count before it
  kTpTotals,    // 2 double words: the call's hits; match_longest's NUL look and its chunks' give-up
  kTpCount
};
// Device scratch of ONE match call (grow-only, reused by later calls that lease the same set).
struct Scratch {
  std::mutex mu;  // held by the call that leased the set
  uint64_t *h_totals = nullptr;  // pinned: tpbuf[kTpTotals] read back
  hipEvent_t ev[6] = {};
  bool ev_ready = false;
  Buf v2buf[kV2Count];
  Buf hostbuf[kHostCount];
  Buf cntbuf[kCntCount];
  Buf dcbuf[kDcCount];
  Buf covbuf[kCovCount];
  Buf selbuf[kSelCount];
  Buf repbuf[kRepCount];
  Buf fselbuf[kFsCount];
  Buf ftokbuf[kFtCount];
  Buf frepbuf[kFrCount];
  Buf fsepbuf[kFpCount];
  Buf grpbuf[kGrpCount];
  Buf fgrpbuf[kFgCount];
  Buf clsbuf[kClsCount];
  Buf flngbuf[kFlCount];
  Buf tpbuf[kTpCount];
  // every family above, for free_scratch and scratch_bytes (S: Scratch or const Scratch): a new family is one more line here
  template <class S, class Fn>
  static void each_buf(S &sc, Fn fn) {
    for (auto &b : sc.v2buf) fn(b);
    for (auto &b : sc.hostbuf) fn(b);
    for (auto &b : sc.cntbuf) fn(b);
    for (auto &b : sc.dcbuf) fn(b);
    for (auto &b : sc.covbuf) fn(b);
    for (auto &b : sc.selbuf) fn(b);
    for (auto &b : sc.repbuf) fn(b);
    for (auto &b : sc.fselbuf) fn(b);
    for (auto &b : sc.ftokbuf) fn(b);
    for (auto &b : sc.frepbuf) fn(b);
    for (auto &b : sc.fsepbuf) fn(b);
    for (auto &b : sc.grpbuf) fn(b);
    for (auto &b : sc.fgrpbuf) fn(b);
    for (auto &b : sc.clsbuf) fn(b);
    for (auto &b : sc.flngbuf) fn(b);
    for (auto &b : sc.tpbuf) fn(b);
  }
  bool dc_rows_clear = false;  // every word of dcbuf[kDcRows] is zero (kdc_compact clears what kdc_add wrote; a call that failed may not have)
  hipStream_t hs[3] = {};  // host-buffer entry: private non-blocking streams for upload, match, download
  unsigned long long *h_v2 = nullptr;  // pinned: cursor[2] + totals[3]
  unsigned long long *h_v2_dev = nullptr;  // the same words as the device addresses them
  // v2buf[kCursor] holds TWO blocks of 16 counter words (and a third of odd words): a call counts in one of them, and its last kernel
  // clears the other for the call behind it -- no memset in front of a call (5 us of a 64 MiB call).  Dirty: the blocks are
  // not known to be clear (new buffer, a call that did not run to its end): the next call clears both itself.
  const void *cursor_buf = nullptr;
  bool cursor_dirty = true;
  uint32_t cursor_phase = 0;
  void reset_cursor() {
    cursor_buf = nullptr;
    cursor_dirty = true;
    cursor_phase = 0;
  }
};
constexpr size_t kCursorBytes = 3 * 16 * 8;
constexpr size_t kMaxScratch = 8;
// last error text of the calling thread (aha_last_error): calls on one handle may run concurrently
extern thread_local std::string tls_err;
}  // namespace ahai

using namespace aha;  // (the library's own translation units only)
struct aha_ac {
  Automaton aut;
  // AHA_OPT_* the handle was compiled with (aha_ac_flags).  With AHA_OPT_FOLD_ASCII `aut` -- its blob included -- is that of the
  // FOLDED keys (fold.hpp): everything derived from it (images, filter, stale ends, find_key) is what a plain handle compiled
  // from fold(keys) has; key_spelling holds the keys as the caller wrote them (same offsets) for aha_ac_key and aha_ac_save
  uint32_t opt_flags = 0;
  static uint64_t next_serial() {
    static std::atomic<uint64_t> n{0};
    return ++n;
  }
  const uint64_t serial = next_serial();  // one per handle ever made in this process (a replacement table names its handle by it)
  std::vector<uint8_t> key_spelling;
  bool fold() const { return (opt_flags & (AHA_OPT_FOLD_ASCII | AHA_OPT_FOLD_SIMPLE | AHA_OPT_FOLD_BMP | AHA_OPT_FOLD_KANA)) != 0; }  // any fold
  // which one: 0 none, 1 ASCII (fold8), 2 simple (fold2: AHA_OPT_FOLD_SIMPLE implies the ASCII fold), 3 BMP (fold3:
  // AHA_OPT_FOLD_BMP implies both), 4 kana (foldk: AHA_OPT_FOLD_KANA implies all three).  >= 2: every engine reads a staged
  // copy, >= 3: three-byte characters take part; == 4: FK's tables and the kernel of their own
  int fold_mode() const {
    return (opt_flags & AHA_OPT_FOLD_KANA) ? 4 : (opt_flags & AHA_OPT_FOLD_BMP) ? 3 : (opt_flags & AHA_OPT_FOLD_SIMPLE) ? 2 : (opt_flags & AHA_OPT_FOLD_ASCII) ? 1 : 0;
  }
  Image img;  // host copy of the device image (export / debugging)
  uint32_t n_slots = 0;
  uint32_t slot_bytes = 0;
  bool compact = false;
  uint64_t image_bytes = 0;
  int device = -1;
  DevAut dev{};
  std::vector<void *> dev_allocs;
  // dev_allocs / image_bytes once the handle is in use (upload_late): a call that holds its scratch set takes it, so it is
  // never pool_mu -- aha_ac_release_scratch holds pool_mu while it waits for the sets
  std::mutex alloc_mu;
  // per-call scratch sets: a match call leases one for its duration (Lease below); concurrent calls on one handle
  // get different sets, up to kMaxScratch of them, then wait
  std::mutex pool_mu;
  std::vector<std::unique_ptr<ahai::Scratch>> pool;
  // profiling
  std::atomic<bool> profiling{false};
  std::mutex last_mu;
  aha_timing last{};
  uint32_t chunk = 256;
  // single-traversal engine (scan_v2.hip)
  bool v2_ok = false;
  uint32_t v2_lds_slots = 0;
  uint32_t v2_grid = 0;
  uint32_t v2_bpc = 1;
  // prefix-filter engine (scan_filter.hip): blocked Bloom filter over the keys' first pf_d bytes; usable when the keys are at
  // least 3 bytes long, none longer than 64, the image compact and the filter at most a quarter full
  std::vector<uint32_t> pf_bloom;
  uint32_t pf_d = 0;
  uint32_t pf_cus = 0;
  uint32_t pf_log2 = 0;
  std::atomic<uint32_t> pf_skip[2] = {}, pf_streak[2] = {};  // calls to go without the filter; give-ups in a row ([1]: char offsets)
  bool pf_ok = false;
  FilterDev fdev{};
  uint32_t s1_lo = 0, s2_lo = 0, s2_hi = 0;   // states with base in [s2_lo, s2_hi): depth >= 3 and a fail target of depth <= 2
  // character-level image (unit.hpp, scan_unit.hip): built for key sets of UTF-8-shaped units with mostly multi-byte
  // characters; plain byte-offset matches through the event regions then take one step per character
  UnitImage unit;
  bool unit_ok = false;  // uploaded and usable on the device
  UnitDev udev{};
  const uint32_t *d_unit_end_info = nullptr;
  const uint2 *d_unit_end_chars = nullptr;  // ... with the key's length in characters (char offsets)
  const uint2 *d_unit_end = nullptr;  // fused expansion (scan_unit.hip ku_expand_groups): key, key length, chain offset per END base
  bool unit_fused = false;            // ... usable: flattened chains of at most 15 keys, key lengths below 2^16
  // skip-ahead traversal over the unit image (unit.hpp MARKS, scan_skip.hip): the filter over the two-unit paths on the device
  bool skip_ok = false;
  SkipDev sdev{};
  // pair engine (unit.hpp PAIR TABLE, scan_pair.hip): the two-unit paths as a perfect hash table on the device
  bool pair_ok = false;
  PairDev pdev{};
  std::atomic<uint32_t> pair_off{0};  // batches it gave up (three: the handle stops trying)
  // document counts: read from the environment when the handle is compiled (engine.cpp doccount_setup)
  uint64_t dc_hit_bytes = 0, dc_row_bytes = 0;  // bounds of a range's hit buffer and of the dense rows in flight
  uint32_t dc_sort_max = 0, dc_dense_min = 0, dc_range_keys = 0;
  uint64_t sel_hit_bytes = 0;  // select calls: the bound of a range's hit buffer (AHA_SELECT_HIT_BYTES)
  uint32_t rep_blocks = 0;  // replace calls: the cap of the scan's and the copy's grids (AHA_REPLACE_BLOCKS; 0: the default)
  uint32_t grep_blocks = 0;  // records and grep calls: the cap of their grids (AHA_GREP_BLOCKS; 0: the default)
  uint32_t post_blocks = 0;  // the passes after the traversal: the cap of their grids (AHA_POST_BLOCKS; 0: the default)
  // feed token calls: the bytes a non-final call may leave behind a sequence's token cursor (AHA_FEED_TOKEN_OPEN; tests lower it)
  uint32_t feed_token_open = 0x3FFFFFFFu;
  uint64_t rule_table_bytes = 0;  // rule grep: the bound of the class-count table in scratch (AHA_RULE_TABLE_BYTES)
  uint64_t cls_hit_bytes = 0;  // class-counts calls: the bound of a range's hit buffer (AHA_CLASS_HIT_BYTES)
  uint32_t cls_blocks = 0;  // ... and the cap of their kernels' grids (AHA_CLASS_BLOCKS; 0: the default)
  uint32_t seg2 = 0;  // slots below it: the root's and the depth-1 states' rows
  // match_longest only (cedar_replay.cpp): the states that carry one of Cedar's stale END flags, derived on the first
  // match_longest call (it replays every insert: as long again as the rest of compile); dev_longest = dev + the bitmap
  std::vector<uint2> chain_host;     // the flattened output chains {key length, key}
  std::vector<uint32_t> key_info;    // [K] flattened-chain offset | min(chain length, 255) << 24 (empty: no flat chains)
  std::vector<uint32_t> state_base;  // [n_states] base of every state in the image
  std::once_flag stale_once;
  std::vector<uint32_t> stale_states;
  int32_t stale_rc = AHA_OK;
  DevAut dev_longest{};
};

// A replacement table (aha_repl_create): immutable once made, so concurrent calls share it.  It belongs to the handle it was
// made for by that handle's id, not by a pointer into it: either may be freed first.
struct aha_repl {
  uint64_t owner = 0;             // aha_ac::serial of its handle
  int device = -1;                // -1: host copy only (a host-only handle)
  uint32_t n_keys = 0;
  std::vector<uint8_t> blob;
  std::vector<aha::RepEntry> ent;  // [K]
  void *d_blob = nullptr;
  aha::RepEntry *d_ent = nullptr;
};

// A class table (aha_classes_create): key k's classes are ids[off[k] .. off[k+1]), strictly ascending and below n_classes.
// Immutable once made and tied to its handle by that handle's id, as a replacement table is.
struct aha_classes {
  uint64_t owner = 0;  // aha_ac::serial of its handle
  int device = -1;     // -1: host copy only (a host-only handle)
  uint32_t n_keys = 0, n_classes = 0;
  std::vector<uint64_t> off;  // [K + 1]
  std::vector<uint32_t> ids;  // [off[K]]
  uint64_t *d_off = nullptr;
  uint32_t *d_ids = nullptr;
};

namespace ahai {
#define HIPCHK(ac, call)                                                              \
  do {                                                                                \
    hipError_t e_ = (call);                                                           \
    if (e_ != hipSuccess) {                                                           \
      tls_err = std::string(#call) + ": " + hipGetErrorString(e_);                  \
      return AHA_E_HIP;                                                               \
    }                                                                                 \
  } while (0)

// Leases one scratch set for the duration of a call: a free one if there is any, a new one while the handle has fewer
// than kMaxScratch, else it waits for the first.
class Lease {
 public:
  explicit Lease(aha_ac *ac) {
    {
      std::lock_guard<std::mutex> lk(ac->pool_mu);
      for (auto &u : ac->pool)
        if (u->mu.try_lock()) {
          sc_ = u.get();
          break;
        }
      if (!sc_ && ac->pool.size() < kMaxScratch) {
        ac->pool.emplace_back(new Scratch());
        sc_ = ac->pool.back().get();
        sc_->mu.lock();
      }
      if (!sc_) wait_ = ac->pool[0].get();
    }
    if (!sc_) {
      wait_->mu.lock();
      sc_ = wait_;
    }
  }
  ~Lease() { sc_->mu.unlock(); }
  Lease(const Lease &) = delete;
  Lease &operator=(const Lease &) = delete;
  Scratch *get() const { return sc_; }

 private:
  Scratch *sc_ = nullptr;
  Scratch *wait_ = nullptr;
};

// a match entry point on a handle without a device (or where there is none): the error and its text
inline int32_t no_device() {
  tls_err = aha_strerror(AHA_E_NO_DEVICE);
  return AHA_E_NO_DEVICE;
}
void free_scratch(Scratch *sc, bool all);
uint64_t scratch_bytes(const Scratch *sc);
// THE allocator of the grow-only buffers: b holds at least `bytes` afterwards, or nothing (the HIP error is returned, the
// runtime's sticky one cleared).  What a new buffer gets beyond `bytes` is its family's rule:
enum Grow {
  kGrowEighth,   // bytes + bytes / 8 + 256 (v2buf, covbuf, selbuf, repbuf, fselbuf, ftokbuf, frepbuf, fsepbuf, grpbuf, fgrpbuf, clsbuf, flngbuf, tpbuf)
  kGrowQuarter,  // bytes + bytes / 4 + 4096 (cntbuf, hostbuf)
  kGrowOrExact   // an eighth, else exactly `bytes`; `bytes` is what it records (dcbuf: what is known to be there)
};
hipError_t reserve(Buf &b, size_t bytes, Grow grow);
inline void *reserve_ptr(Buf &b, size_t bytes, Grow grow) { return reserve(b, bytes, grow) == hipSuccess ? b.p : nullptr; }  // null: no memory
// adds the passes that were thrown away to the timing the last pass published (profiling on)
void note_repeats(aha_ac *ac, uint32_t repeats);
void publish_timing(aha_ac *ac, const aha_timing &t);

template <typename T>
int32_t upload(aha_ac *ac, const std::vector<T> &v, const T **out) {
  void *d = nullptr;
  size_t bytes = std::max<size_t>(v.size() * sizeof(T), 16);
  HIPCHK(ac, hipMalloc(&d, bytes));
  ac->dev_allocs.push_back(d);
  if (!v.empty()) HIPCHK(ac, hipMemcpy(d, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice));
  ac->image_bytes += v.size() * sizeof(T);
  *out = reinterpret_cast<const T *>(d);
  return AHA_OK;
}

// upload() for tables that appear after compile (the first match_longest call), possibly while other threads match on the
// handle: the copy goes over a private non-blocking stream (no call of the library touches the NULL stream), the handle's
// allocation list is touched under alloc_mu.
template <class T>
int32_t upload_late(aha_ac *ac, const std::vector<T> &v, const T **out) {
  void *d = nullptr;
  const size_t bytes = std::max<size_t>(v.size() * sizeof(T), 16);
  HIPCHK(ac, hipMalloc(&d, bytes));
  {
    std::lock_guard<std::mutex> lk(ac->alloc_mu);
    ac->dev_allocs.push_back(d);
    ac->image_bytes += v.size() * sizeof(T);
  }
  if (!v.empty()) {
    hipStream_t st = nullptr;
    HIPCHK(ac, hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
    hipError_t e = hipMemcpyAsync(d, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    (void)hipStreamDestroy(st);
    HIPCHK(ac, e);
  }
  *out = reinterpret_cast<const T *>(d);
  return AHA_OK;
}

int32_t upload_image(aha_ac *ac, const Image &img);
int32_t fill_params(aha_ac *ac, const aha_match_params *p, MatchArgs &M, int *longest);

struct DeviceGuard {
  int prev = -1;
  bool active = false;
  explicit DeviceGuard(int dev) {
    if (hipGetDevice(&prev) == hipSuccess && prev != dev) {
      active = hipSetDevice(dev) == hipSuccess;
    }
  }
  ~DeviceGuard() {
    if (active) (void)hipSetDevice(prev);
  }
};

int32_t ensure_stale(aha_ac *ac);  // match_longest: the states with one of Cedar's stale END flags, derived on first use (capi.cpp)

// ---- engine.cpp
bool skip_eligible(const aha_ac *ac);
bool pair_eligible(const aha_ac *ac);
void plan_engine(aha_ac *ac, const Placement &pl);  // host-only plan: how much of the image the byte-level traversal keeps in LDS
void v2_setup(aha_ac *ac);                          // once per device handle: kernels' LDS limits, grids, the engines' device tables
StreamFmt stream_fmt(const aha_ac *ac);             // field widths of the 4-byte exchange stream for this automaton
int32_t ready_events(aha_ac *ac, Scratch *sc);      // the events of a scratch set are created by the first profiled call that leases it
// the hits as the 4-byte exchange stream as well (aha_ac_match_batch_device_stream); null: not asked for
struct PackOut {
  uint32_t *d_words;
  uint64_t cap_words;
  uint64_t *d_n_words;
};
// A device-resident batch: what every device_* call below works on.
struct Batch {
  const uint8_t *text;             // the documents' bytes, one behind the other (null only where n_bytes == 0)
  const uint64_t *doc_off;         // the n_docs + 1 offsets into text, device memory: [0] = 0, ascending, [n_docs] = n_bytes
  uint64_t n_docs, n_bytes;
  const aha_match_params *params;  // null: the defaults (records calls: not looked at)
  hipStream_t stream;              // everything the call does is ordered on it (the ABI's void *, cast once there)
  bool checked;                    // whoever made the batch has validated doc_off; false: the call validates it on the device
};
// ... made by name, so that no call site spells `checked` as a bare true or false
inline Batch checked_batch(const uint8_t *text, const uint64_t *doc_off, uint64_t n_docs, uint64_t n_bytes, const aha_match_params *params,
                           hipStream_t stream) {
  return Batch{text, doc_off, n_docs, n_bytes, params, stream, true};
}
inline Batch unchecked_batch(const uint8_t *text, const uint64_t *doc_off, uint64_t n_docs, uint64_t n_bytes,
                             const aha_match_params *params, hipStream_t stream) {
  return Batch{text, doc_off, n_docs, n_bytes, params, stream, false};
}
// How device_match and device_count treat the handle's back-off state and the text.  Combined with |; nothing converts to it.
enum class CallOpt : uint32_t {
  kNone = 0,
  // every engine, but the back-off state is only read (the match inside a document-count call)
  kNeutral = 1,
  // neither the prefix-filter nor the pair engine, so the handle's back-off state is neither read nor written (a feed's window
  // batch, feed.cpp: an internal batch must not change which engine the caller's next call takes)
  kQuiet = 2,
  // the text is already as the engines take it -- folded by a folded feed (feed.cpp, scan_feedfold.hip) -- so a folded handle's
  // staged pass is left out; only an unaligned view is still copied.  No other caller passes it.
  kAsIs = 4
};
constexpr CallOpt operator|(CallOpt a, CallOpt b) { return (CallOpt)((uint32_t)a | (uint32_t)b); }
constexpr bool has(CallOpt o, CallOpt f) { return ((uint32_t)o & (uint32_t)f) != 0; }
constexpr CallOpt as_is_if(int fold) { return fold ? CallOpt::kAsIs : CallOpt::kNone; }  // (a feed's fold mode)
static_assert(!std::is_constructible<CallOpt, bool>::value && !std::is_convertible<bool, CallOpt>::value &&
                  !std::is_convertible<int, CallOpt>::value,
              "a bool in an option's place must not compile");
// where a match leaves its hits: d_out[0 .. cap), and per document its first hit's index where doc_hit_off is given
struct HitOut {
  aha_hit *d_out;
  uint64_t cap;
  uint64_t *d_doc_hit_off;
};
// one device-resident batch through whichever engine takes it (retries, hand-backs, the two-pass engine as the last resort)
int32_t device_match(aha_ac *ac, Scratch *sc, const Batch &B, const HitOut &out, uint64_t *n_hits, CallOpt opt = CallOpt::kNone);
// one device-resident batch counted (aha_ac_count_batch_device): the match's engine, the count passes instead of the expansion.
// Of the options only kAsIs applies: a count call never writes the back-off state.
int32_t device_count(aha_ac *ac, Scratch *sc, const Batch &B, uint32_t flags, uint64_t *d_key_counts, uint64_t *d_doc_hit_offsets,
                     uint64_t *n_hits, CallOpt opt = CallOpt::kNone, uint32_t *cover_mask = nullptr);
// one device-resident batch as {key, count} pairs per document (aha_ac_doc_counts_batch_device): a count call for the hits per
// document, the match into scratch, the per-document reduction (scan_doccount.hip)
int32_t device_doc_counts(aha_ac *ac, Scratch *sc, const Batch &B, aha_key_count *d_out, uint64_t cap, uint64_t *d_doc_pair_offsets,
                          uint64_t *n_pairs, uint64_t *n_hits);
// one device-resident batch covered (aha_ac_cover_batch_device): the count call's pipeline without key counts, one span per
// event into the mask (scan_cover.hip), then the redacted copy and the documents' covered bytes where asked for
int32_t device_cover(aha_ac *ac, Scratch *sc, const Batch &B, uint32_t flags, uint32_t *d_mask, uint8_t *d_redacted, uint8_t fill,
                     uint64_t *d_doc_covered, uint64_t *n_covered, uint64_t *n_hits);
// one device-resident batch selected (aha_ac_select_batch_device): a count call for the hits per document, the match into
// scratch, the leftmost-longest non-overlapping hits of every document from it (scan_select.hip)
int32_t device_select(aha_ac *ac, Scratch *sc, const Batch &B, const HitOut &out, uint64_t *n_selected, uint64_t *n_hits,
                      uint32_t flags = 0);
// What device_select_to does with the selection.  Without a sink (device_select, the public entries): the caller's buffer where
// the total fits, the documents' offsets to the caller's array.  With one (device_replace): `place(kept, upto, &at)` is asked,
// range by range, for a buffer that holds `upto` hits and still has the first `kept` ones (it returns the call's error, with
// tls_err set, where it has none); every range is emitted as soon as it has been worked, so no range is matched twice; the
// documents' offsets stay in selbuf[kSelDocOff], D + 1 of them.  The call's timing (profiling) is handed to `timing` and not
// published: the caller publishes once, with its own share added.
// flags: AHA_SELECT_TOKENS (| AHA_SELECT_GAP_RUNS) -- the tokens of every document instead of the selection (scan_tokens.hip);
// the ranges then tile all documents whether they have hits or not, and a range is bounded by its text (8 bytes of L each)
// as well as by its hits.
// Only without a sink.
struct SelectSink {
  std::function<int32_t(uint64_t kept, uint64_t upto, aha_hit **at)> place;
  aha_timing *timing = nullptr;
};
int32_t device_select_to(aha_ac *ac, Scratch *sc, const Batch &B, const HitOut &out, uint64_t *n_selected, uint64_t *n_hits,
                         const SelectSink *sink, uint32_t flags = 0);
// one device-resident batch substituted (aha_ac_replace_batch_device): device_select_to with the selection into scratch, then the
// scan over the changes of length and the output-driven copy (scan_replace.hip)
int32_t device_replace(aha_ac *ac, Scratch *sc, const aha_repl *table, const Batch &B, uint8_t *d_out, uint64_t cap_bytes,
                       uint64_t *d_doc_out_offsets, uint64_t *n_out_bytes, uint64_t *n_selected, uint64_t *n_hits);
// one device-resident batch split into records (aha_ac_records_batch_device): the record-end mask in one pass over the text,
// its rank, the offsets once the count is known to fit (scan_grep.hip)
int32_t device_records(aha_ac *ac, Scratch *sc, const Batch &B, uint8_t delim, uint64_t *d_rec_offsets, uint64_t cap_records,
                       uint64_t *d_doc_rec_offsets, uint64_t *n_records);
// its two halves, split at the total (a feed grep call sizes the fragments' offsets from it): the mask and its rank into
// grpbuf, *n_records read back; then, with grpbuf untouched in between, the offsets (either may be null).  No argument checks,
// and B.checked is not looked at.
int32_t device_records_settle(aha_ac *ac, Scratch *sc, const Batch &B, uint8_t delim, uint64_t *n_records);
int32_t device_records_emit(aha_ac *ac, Scratch *sc, const Batch &B, uint64_t *d_rec_offsets, uint64_t *d_doc_rec_offsets);
// the cap of the grids of the passes after the traversal: fold copies, cover, select, the feeds' (AHA_POST_BLOCKS); the fallback
// of the families' own caps
uint32_t post_grid(const aha_ac *ac);
uint32_t grep_grid(const aha_ac *ac);  // the cap of the records and grep grids (AHA_GREP_BLOCKS)
// one device-resident batch filtered (aha_ac_grep_batch_device): device_count for the hits per document, the kept documents and
// the dropped runs from them (scan_grep.hip), replace's scan and copy over the runs (scan_replace.hip)
int32_t device_grep(aha_ac *ac, Scratch *sc, const Batch &B, uint32_t flags, uint64_t *d_kept_docs, uint64_t *d_doc_out_offsets,
                    uint64_t cap_docs, uint8_t *d_out, uint64_t cap_bytes, uint64_t *n_kept, uint64_t *n_out_bytes, uint64_t *n_hits);
// the same filtered by a rule over the class counts (AHA_GREP_RULE; gp checked by capi.cpp grep_rule_args; the match parameters
// are gp->match, B.params is not looked at): device_class_counts into d_rows or scratch, the keep mask from the rule and S and T
// from keep (scan_greprule.hip), then grep's tail.
enum class RuleRows {
  kLate,  // d_rows is the caller's and the call may still fail on capacity: the table goes to scratch, then to d_rows
  kEarly  // d_rows may be written before the verdict (it is not the caller's buffer, or the call cannot fail on capacity)
};
int32_t device_grep_rule(aha_ac *ac, Scratch *sc, const Batch &B, const aha_grep_params *gp, uint32_t *d_rows, RuleRows rows,
                         uint32_t flags, uint64_t *d_kept_docs, uint64_t *d_doc_out_offsets, uint64_t cap_docs, uint8_t *d_out,
                         uint64_t cap_bytes, uint64_t *n_kept, uint64_t *n_out_bytes, uint64_t *n_hits);
// the excerpts of one device-resident batch (AHA_GREP_CONTEXT; ep checked by capi.cpp grep_context_args; the match parameters
// are ep->match, B.params is not looked at): device_count with a cover mask in scratch, the covered runs, their windows and the
// merge (scan_excerpt.hip), replace's scan and copy over the gaps between the excerpts.  d_starts takes grep's d_kept_docs,
// d_out_offsets its d_doc_out_offsets
int32_t device_excerpts(aha_ac *ac, Scratch *sc, const Batch &B, const aha_excerpt_params *ep, uint64_t *d_starts,
                        uint64_t *d_out_offsets, uint64_t cap_docs, uint8_t *d_out, uint64_t cap_bytes, uint64_t *n_kept,
                        uint64_t *n_out_bytes, uint64_t *n_hits);
// grep with context lines (AHA_GREP_LINES; lp checked by capi.cpp grep_lines_args; the match parameters are lp->match, B.params
// is not looked at): grep's match mask dilated by lp->before and lp->after records inside the groups (scan_greplines.hip), rule
// grep's edges, then grep's tail.  d_groups (lp->n_groups + 1 entries or null) and d_is_match (cap_docs bytes or null) are
// device memory whatever lp->group_offsets and lp->is_match point to
int32_t device_grep_lines(aha_ac *ac, Scratch *sc, const Batch &B, const aha_grep_lines_params *lp, const uint64_t *d_groups,
                          uint8_t *d_is_match, uint32_t flags, uint64_t *d_kept_docs, uint64_t *d_doc_out_offsets, uint64_t cap_docs,
                          uint8_t *d_out, uint64_t cap_bytes, uint64_t *n_kept, uint64_t *n_out_bytes, uint64_t *n_hits);
// one device-resident batch as a dense table of hits per (document, key class) (aha_ac_class_counts_batch_device):
// device_count for the hits per document, the match of every range of whole documents into scratch, one add per (hit, class)
// into d_out[n_docs][table->n_classes] (scan_classcount.hip)
int32_t device_class_counts(aha_ac *ac, Scratch *sc, const aha_classes *table, const Batch &B, uint32_t *d_out, uint64_t *n_hits);
// the pieces of a call on a longest feed (feed.cpp feed_long_prepare; scan_feedlongest.hip), walked as the documents of a
// two-pass match_longest batch that start from the feed's carried states.  _count: the text as the kernels take it (folded on a
// folded handle), the NUL look and the chunks in mode 2, pass 1 and the block scan; *n_hits = the call's hits (one read-back),
// P = what pass 2 needs.  _write: pass 2 into d_out (cap >= *n_hits) and d_pho [D + 1]; nothing is synchronised.  F.n_bytes > 0.
struct FeedLongPlan {
  MatchArgs M;
  bool chunks = false, intersectable = false;
};
int32_t device_feed_longest_count(aha_ac *ac, Scratch *sc, const FeedArgs &F, FeedLongArgs &L, int longest, FeedLongPlan &P,
                                  uint64_t *n_hits, void *stream);
int32_t device_feed_longest_write(aha_ac *ac, const FeedArgs &F, const FeedLongArgs &L, FeedLongPlan &P, aha_hit *d_out, uint64_t cap,
                                  uint64_t *d_pho, void *stream);
uint32_t class_grid(const aha_ac *ac);  // the cap of the class-counts grids (AHA_CLASS_BLOCKS)
}  // namespace ahai
