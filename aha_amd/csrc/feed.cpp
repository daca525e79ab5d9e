// feed.cpp -- feeds (aha_feed_*, include/aha_hip.h): sequences that arrive in pieces across calls.
//
// A call on D pieces (scan_feed.hip has the two facts it rests on):
//   kfd_check + kfd_scan   validate offsets and ids; the window lengths into their offsets (one read-back: verdict, size)
//   kfd_windows            the window batch [X_d | ctx_d | P'_d] (+ kfd_leads: leads(P_d) on char feeds)
//   device_match, quiet    the window batch (3D documents)                     -> x_d, y_d, z_d
//   device_match           the caller's pieces as they are, from the root       -> m_d (the engine a plain match takes)
//   the host               total = (nX - nY) + (nM - nZ) from block totals: above cap -> AHA_E_CAPACITY, nothing committed
//   kfd_scan + kfd_merge   piece_hit_offsets, the kept hits into the caller's buffer
//   kfd_commit             bases, counters, the new contexts
// A count call (aha_feed_count_batch*) shares the first three steps (feed_windows), then
//   device_count           the caller's pieces, from the root, into the feed's K-word vector   -> m_d (a plain count's engine)
//   kfd_count_windows      + the window hits: +1 for the X block, -1 for the ctx and P' blocks
//   kfd_scan + kfd_count_finish + kfd_commit   piece_hit_offsets, then the caller's key counts, then the feed's state
// A cover call (aha_feed_cover_batch*) widens the head windows to 2 W bytes of the piece (X2, P'2; scan_feed.hip), then
//   device_match, quiet    the window batch, byte offsets on char feeds too: its hit list is at most 3 W bytes of text per piece
//   device_count + mask    the caller's pieces, from the root: their hits per piece and one span per event into a mask in the
//                          feed's scratch (a plain cover's engine; nothing is held per hit of this pass)
//   kfd_cover_clear + kfd_cover_windows + kfd_scan   the mask corrected at the cuts, piece_back, piece_hit_offsets
//   kfd_commit             the new contexts -- from the caller's text, so before an in-place redaction
//   kv_total, kv_doc_covered, the mask's copy, kv_redact (scan_cover.hip)   each only where asked for; the redaction last
// A select call (aha_feed_select_batch*) takes the first five steps of a match call with the hits into scratch, then
//   scan_feedselect.hip    the pieces' extended positions, L from the sequences' tails and the hits, the masks, the walk up to the
//                          frontier, the rank (one read-back: the total) -- above cap -> AHA_E_CAPACITY, nothing committed
//   kfs_emit, kfd_commit + kfs_commit   the selection, the offsets; then the feed's state and, behind it, the select state
// A token call (aha_feed_select_batch* with AHA_FEED_SELECT_TOKENS) is a select call up to the rank (feed_select_settle), then
//   scan_feedtokens.hip    per piece the cursors it finds and leaves; the inside mask (ktk_spans) and the token starts over the
//                          extended positions, their rank; per piece the edge decision (feedtok_edge.hpp), the token counts
//                          scanned (one read-back: the total and the verdict) -- a token open beyond the bound -> AHA_E_TOO_LONG,
//                          above cap -> AHA_E_CAPACITY, nothing committed
//   kft_emit, kfd_commit + kfs_commit + kft_commit   the tokens, the offsets; then the feed's state, the select state, the token state
// A replace call (aha_feed_replace_batch*) is a select call up to the rank (feed_select_settle), then
//   kfs_emit               the settled selection into scratch instead of a caller buffer
//   scan_feedreplace.hip   per piece the open bytes in front of it and the cursor it will leave; the staged text T[c0 .. c1) of
//                          every piece, the open bytes from the sequence's context bank
//   scan_replace.hip       its passes over the staged batch, unchanged (one read-back: the byte total) -- above cap_bytes ->
//                          AHA_E_CAPACITY, nothing committed
//   krp_copy, kfd_commit + kfs_commit   the result, the offsets; then the feed's state as a select call leaves it
// A feed with a separator filter (aha_feed_open_params; scan_feedsep.hip, DESIGN.md 4.10 "Feed separator filter") keeps
// W = Lmax + 1 bytes of context, so a hit that ended with the piece before and its left neighbour lie in the context.  Its match
// and count calls take the first five steps of a match call unfiltered with the hits into scratch, then
//   kfd_edge + kfd_scan + kfd_merge   the call's true hits piece by piece, the ones that end on the context's last byte included
//   kfp_flag, the rank                one bit per true hit (end < |P|, both neighbours pass), the kept hits before every 2048 (one
//                                     read-back: the total) -- above cap -> AHA_E_CAPACITY, nothing committed
//   kfp_compact | kfp_count           the kept hits, or their values per key; the offsets from the same ranks; kfd_commit
// and aha_feed_finish_batch* matches the named sequences' contexts as the window batch of a call of empty pieces, keeps the hits
// that end on the last byte and pass on the left, and sets those sequences back to length 0 (kfp_restart).
// A grep call (aha_feed_grep_batch*; DESIGN.md 4.10 "Feed grep") lays out windows of its own, per record and not per sequence:
//   kfd_check              offsets, ids, duplicates, and that the named sequences went through grep calls alone (one read-back)
//   device_records         the pieces split into fragments, in two halves: the total sizes the fragments' offsets (one read-back)
//   kfg_layout, kfg_windows   the window batch [X_d | Y_d | Z_d] of the pieces whose first fragment continues an open record
//                          (one read-back: its size)
//   device_count x 2       the window batch, then the fragments as documents from the root (a plain grep's engine and count path)
//   kfg_has, kfg_first, kfg_flag   keep, S and T over the fragments; an open tail counts as dropped
//   scan_grep.hip, scan_replace.hip   grep's steps over these masks, unchanged (two read-backs: the kept fragments and the runs,
//                          then the byte total) -- above either capacity -> AHA_E_CAPACITY, nothing committed
//   kgr_emit_docs, krp_copy, kfd_commit + kfg_commit   the kept fragments, their bytes, the offsets; then the feed's state and,
//                          behind it, the grep state
// A longest feed (aha_feed_open_params with longest = 1 | 2; scan_feedlongest.hip, DESIGN.md 4.10 "Feed match_longest") keeps no
// context: it carries match_longest_'s whole state per sequence (FeedLongSeq, 16 bytes).  Its match calls are
//   kfd_check              offsets, ids, duplicates (one read-back)
//   device_feed_longest_count   the text as the kernels take it (folded on a folded handle), the NUL look and the chunks in
//                          mode 2, pass 1 from the carried states -- it leaves the states at the pieces' ends in scratch -- and the
//                          block scan (one read-back: the total) -- above cap -> AHA_E_CAPACITY, nothing committed
//   device_feed_longest_write, kfl_commit   pass 2: the hits and piece_hit_offsets; then bases, lengths and the carried states
// and aha_feed_finish_batch* reports the named sequences' pending hits (kfl_finish: counted, then written) and restarts them.
// A folded feed (AHA_FEED_FOLD on a handle folded beyond ASCII; scan_feedfold.hip, DESIGN.md 4.13 "Feeds on handles folded beyond
// ASCII") keeps W = Lmax + 1 ORIGINAL bytes of context and answers every call as if the sequence ended with its piece.  Its
// match, count and cover calls are the plain feed's with the first three steps folded (feed_windows):
//   the staged copy + kff_heads   the pieces folded once into the feed's scratch, every piece on its own, then the first two bytes
//                          of each from ctx || P
//   kff_windows            the window batch cut from fold(ctx || P), in kfd_windows' place
//   device_match / device_count, as_is   both matches read text that is folded already; everything behind them is unchanged
// Calls on one feed are serialised by its mutex; its scratch is its own.  The two matches lease one of the handle's scratch
// sets like any call, so different feeds and plain calls on the same handle run side by side.
// Every public batch entry has one shape: its family's argument checks (feed_*_args: the refusals both entries share), one call
// scope (FeedCall: the mutex, the device, the lease), for a host entry the staging of the pieces (stage_pieces: the host checks,
// then the scope, then the upload), the family function on device-resident pieces (feed_match .. feed_grep), and for a host entry
// the read-backs (fetch).  What a family adds to the arguments of a call (feed_args) it sets itself.
#include "feed.hpp"

#include <initializer_list>
#include <optional>

#include "handle.hpp"

using namespace ahai;

namespace {
// the feed's grow-only scratch; every slot has a name.  kH*: the host entries' staging of what the caller gives and takes
enum FeedSlot {
  kMisc,        // the verdict, the window batch's size, a cover call's total
  kWin,         // the window batch's bytes
  kWoff,        // ... its document offsets
  kWdho,        // ... its per-document hit offsets
  kWhits,       // ... its hits
  kMdho,        // the main pass's per-document hit offsets
  kMhits,       // ... its hits
  kPho,         // piece hit offsets, where the caller takes none
  kLeadCtx,     // leads(ctx) (char feeds)
  kLeadP,       // leads(P) (char feeds)
  kHCorpus,     // the pieces
  kHOff,        // piece_offsets
  kHIds,        // seq_ids
  kHOut,        // the result: hits, or a replace or grep call's bytes
  kHPho,        // piece_hit_offsets and what stands in its place: sel, out and seq_hit offsets
  kHBases,      // piece_bases
  kKc,          // a count call's per-key sums
  kHKc,         // key_counts
  kMask,        // a cover call's mask
  kHBack,       // piece_back
  kHCov,        // piece_covered
  kHHold,       // piece_hold
  kHKept,       // kept_recs
  kHRecOut,     // rec_out_offsets
  kHPieceRec,   // piece_rec_offsets
  kHPieceKept,  // piece_kept_offsets
  kHHead,       // piece_head
  kHRecBases,   // piece_rec_bases
  kFold,        // a folded feed: the pieces as the engines take them (FeedArgs::ftext)
  kFeedSlots
};
}  // namespace

struct aha_feed {
  aha_ac *ac = nullptr;
  uint32_t n_seqs = 0;
  uint32_t W = 0;  // bytes of context per sequence: max(Lmax - 1, 0), or Lmax + 1 with a separator filter or on a folded feed
  bool chars = false;
  bool sep = false;         // opened with a separator filter: W = Lmax + 1, match and count calls report a hit one byte late
  uint32_t blocked[8] = {};  // bit c: byte c does not pass (c < sep_size && !sep[c])
  int longest = 0;          // opened with longest = 1 | 2: match_longest, intersectable = false | true; no context is kept
  int fold = 0;             // opened with AHA_FEED_FOLD on a handle folded beyond ASCII: its fold mode (2, 3, 4), W = Lmax + 1, and
                            // every call answers as if the sequence ended with its piece (scan_feedfold.hip); else 0
  FeedLongSeq *d_long = nullptr;  // ... its carried states, allocated at open (16 bytes per sequence)
  std::mutex mu;
  FeedSeq *d_seqs = nullptr;
  uint8_t *d_ctx = nullptr;
  // select and replace calls: allocated by the feed's first one (8 W + 16 bytes per sequence)
  FeedSelSeq *d_sel = nullptr;
  unsigned long long *d_tail = nullptr;
  // token calls: allocated by the feed's first one (16 bytes per sequence)
  FeedTokSeq *d_tok = nullptr;
  // grep calls: allocated by the feed's first one (32 bytes per sequence); the delimiter its first successful one fixed
  FeedGrepSeq *d_grep = nullptr;
  int grep_delim = -1;
  uint32_t stamp = 0;
  Buf buf[kFeedSlots];        // grow-only scratch (FeedSlot)
  uint64_t *h_pin = nullptr;  // pinned: read-backs
  hipStream_t hs = nullptr;   // the host entry's stream (and position / reset)
};

namespace {
void *reserve(aha_feed *f, int i, size_t bytes) {
  Buf &b = f->buf[i];
  bytes = std::max<size_t>(bytes, 16);
  if (b.bytes >= bytes) return b.p;
  const size_t grown = std::max(bytes, b.bytes + b.bytes / 4);
  if (b.p) (void)hipFree(b.p);
  b = Buf();
  if (hipMalloc(&b.p, grown) != hipSuccess) {
    (void)hipGetLastError();
    b.p = nullptr;
    return nullptr;
  }
  b.bytes = grown;
  return b.p;
}

int32_t no_memory(const char *what) {
  tls_err = std::string("hipMalloc failed for the feed's ") + what;
  return AHA_E_HIP;
}

// the first half of every call: checks, the window batch and its match.  hits: the window batch's hit list is needed (a match,
// or a count with key counts); otherwise only its per-document offsets (a count without: device_count of the windows).
// wide: a cover call -- the head windows take 2 W bytes of the piece, and the window hits are in bytes on a char feed too.
// -> *n_w, and the hits of the three blocks nx (X), ny (ctx), nz (P').
int32_t feed_windows(aha_feed *f, Scratch *sc, FeedArgs &F, hipStream_t s, bool hits, uint64_t *n_w, uint64_t *nx,
                     uint64_t *ny, uint64_t *nz, bool wide = false) {
  aha_ac *ac = f->ac;
  const uint64_t D = F.D;
  if (++f->stamp == 0) f->stamp = 1;  // (a stamp comes back after 2^32 calls; a sequence must be named in neither)
  F.stamp = f->stamp;
  F.seqs = f->d_seqs;
  F.ctx = f->d_ctx;
  F.n_seqs = f->n_seqs;
  F.W = f->W;
  F.Wp = wide ? 2 * f->W : f->W;
  F.chars = f->chars ? 1 : 0;
  F.max_piece = (1ull << 31) - std::max<uint64_t>(ac->aut.max_key_len, 1);
  uint64_t *misc = (uint64_t *)reserve(f, kMisc, 24);  // (the third word: a cover call's total)
  F.woff = (uint64_t *)reserve(f, kWoff, (3 * D + 1) * 8);
  F.lead_ctx = (uint64_t *)reserve(f, kLeadCtx, D * 8);
  F.lead_p = (unsigned long long *)reserve(f, kLeadP, D * 8);
  uint64_t *wdho = (uint64_t *)reserve(f, kWdho, (3 * D + 1) * 8);
  uint64_t *mdho = (uint64_t *)reserve(f, kMdho, (D + 1) * 8);
  if (!misc || !F.woff || !F.lead_ctx || !F.lead_p || !wdho || !mdho) return no_memory("offsets");
  F.verdict = (uint32_t *)misc;
  F.win_total = misc + 1;
  F.wdho = wdho;
  F.mdho = mdho;
  HIPCHK(ac, hipMemsetAsync(F.verdict, 0, 4, s));
  feed_launch_check(F, s);
  HIPCHK(ac, hipGetLastError());
  HIPCHK(ac, hipMemcpyAsync(f->h_pin, misc, 16, hipMemcpyDeviceToHost, s));
  HIPCHK(ac, hipStreamSynchronize(s));
  const uint32_t bad = (uint32_t)f->h_pin[0];
  if (bad & 1u) {
    tls_err = "feed: need piece_offsets[0] = 0, ascending, piece_offsets[n_pieces] = n_bytes, seq_ids below n_seqs and each once";
    return AHA_E_INVALID;
  }
  if (bad & 4u) {
    tls_err = "feed select: bytes of a named sequence went through a match, count or cover call; select works again after its reset";
    return AHA_E_INVALID;
  }
  if (bad & 16u) {
    tls_err = "feed select with tokens: bytes of a named sequence went through a call that reports no tokens; tokens work again after "
              "its reset or its FINAL call";
    return AHA_E_INVALID;
  }
  if (bad & 2u) {
    tls_err = "feed: a piece must be shorter than 2^31 bytes minus the longest key";
    return AHA_E_TOO_LONG;
  }
  const uint64_t n_win = f->h_pin[1];
  F.win = (uint8_t *)reserve(f, kWin, n_win + 64);
  if (!F.win) return no_memory("windows");
  if (F.chars && D) HIPCHK(ac, hipMemsetAsync(F.lead_p, 0, D * 8, s));
  if (f->fold) {
    // a folded feed: the pieces folded once into the feed's scratch -- every piece on its own (consecutive pieces belong to
    // different sequences, so the copies' fix-up at the boundaries is always wanted), then the first two bytes of each with the
    // sequence's context in view -- and the windows cut from the fold of ctx || P; both matches read them as they are
    F.ftext = (uint8_t *)reserve(f, kFold, F.n_bytes + 64);
    if (!F.ftext) return no_memory("folded pieces");
    const uint32_t max_blocks = post_grid(ac);
    if (f->fold == 4)
      foldk_launch_copy(F.text, F.ftext, F.n_bytes, F.off, D, max_blocks, s);
    else if (f->fold == 3)
      fold3_launch_copy(F.text, F.ftext, F.n_bytes, F.off, D, max_blocks, s);
    else
      fold2_launch_copy(F.text, F.ftext, F.n_bytes, F.off, D, max_blocks, s);
    feedfold_launch_heads(F, f->fold, s);
    feedfold_launch_windows(F, f->fold, s);
    feed_launch_leads(F, s);
  } else {
    feed_launch_windows(F, s);
  }
  HIPCHK(ac, hipGetLastError());

  aha_match_params p{};
  p.struct_size = sizeof(p);
  p.char_offsets = wide ? 0 : F.chars;
  const Batch win = checked_batch(F.win, F.woff, 3 * D, n_win, &p, s);  // (offsets the feed's own kernels wrote)
  *n_w = 0;
  if (hits) {
    // the window batch: at most 4 W bytes per piece (6 W: a cover call); its hit scratch grows to what it needed once
    for (int attempt = 0;; attempt++) {
      const uint64_t cap_w = f->buf[kWhits].bytes / sizeof(aha_hit);
      const HitOut hits_w{cap_w ? (aha_hit *)f->buf[kWhits].p : nullptr, cap_w, wdho};
      int32_t rc = device_match(ac, sc, win, hits_w, n_w, CallOpt::kQuiet | as_is_if(f->fold));
      if (rc == AHA_E_CAPACITY && attempt == 0) {
        if (!reserve(f, kWhits, std::max<uint64_t>(*n_w, 1024) * sizeof(aha_hit))) return no_memory("window hits");
        continue;
      }
      if (rc) return rc;
      break;
    }
  } else {
    // (a count call never writes the handle's back-off state, so it needs no quiet form)
    int32_t rc = device_count(ac, sc, win, 0, nullptr, wdho, n_w, as_is_if(f->fold));
    if (rc) return rc;
  }
  F.whits = (const int32_t *)f->buf[kWhits].p;
  *nx = *ny = *nz = 0;
  if (D) {
    HIPCHK(ac, hipMemcpyAsync(f->h_pin, wdho + D, 8, hipMemcpyDeviceToHost, s));
    HIPCHK(ac, hipMemcpyAsync(f->h_pin + 1, wdho + 2 * D, 8, hipMemcpyDeviceToHost, s));
    HIPCHK(ac, hipStreamSynchronize(s));
    *nx = f->h_pin[0];
    *ny = f->h_pin[1] - *nx;
    *nz = *n_w - f->h_pin[1];
  }
  return AHA_OK;
}

// the text of a call's main pass: the caller's pieces, or on a folded feed their folded copy (feed_windows made it), which the
// engines then take as it is -- one staged pass per call, not two
const uint8_t *main_text(const aha_feed *f, const FeedArgs &F) { return f->fold ? F.ftext : F.text; }
// ... as a batch: the pieces are its documents, their offsets were checked when they were staged
static Batch main_batch(const aha_feed *f, const FeedArgs &F, const aha_match_params *p, hipStream_t s) {
  return checked_batch(main_text(f, F), F.off, F.D, F.n_bytes, p, s);
}

// the part of a match call before anything is written for the caller: the windows, then the main pass.  *total = the call's
// hits; AHA_E_CAPACITY when they are more than cap.
int32_t feed_prepare(aha_feed *f, Scratch *sc, FeedArgs &F, uint64_t cap, hipStream_t s, uint64_t *total) {
  aha_ac *ac = f->ac;
  uint64_t n_w = 0, nx = 0, ny = 0, nz = 0;
  int32_t rc = feed_windows(f, sc, F, s, true, &n_w, &nx, &ny, &nz);
  if (rc) return rc;
  aha_match_params p{};
  p.struct_size = sizeof(p);
  p.char_offsets = F.chars;
  // the main pass: what the caller's buffer can take plus the hits it drops
  const uint64_t cap_m = cap + nz;
  aha_hit *mh = cap_m ? (aha_hit *)reserve(f, kMhits, cap_m * sizeof(aha_hit)) : nullptr;
  if (cap_m && !mh) return no_memory("hits");
  uint64_t n_m = 0;
  rc = device_match(ac, sc, main_batch(f, F, &p, s), HitOut{mh, cap_m, (uint64_t *)F.mdho}, &n_m, as_is_if(f->fold));
  if (rc && rc != AHA_E_CAPACITY) return rc;
  F.mhits = (const int32_t *)mh;
  *total = (nx - ny) + (n_m - nz);
  F.total = *total;
  if (rc == AHA_E_CAPACITY || *total > cap) {
    tls_err = "output buffer too small";
    return AHA_E_CAPACITY;
  }
  return AHA_OK;
}

// a whole count call on device-resident pieces: the windows, the main pass into the feed's vector, the window hits added,
// then -- nothing the caller owns is written before -- the caller's key counts and offsets and the feed's state
int32_t feed_sep_count(aha_feed *f, Scratch *sc, FeedArgs &F, hipStream_t s, uint64_t *total);
int32_t feed_count(aha_feed *f, Scratch *sc, FeedArgs &F, hipStream_t s, uint64_t *total) {
  if (f->sep) return feed_sep_count(f, sc, F, s, total);
  aha_ac *ac = f->ac;
  const bool per_key = F.key_counts != nullptr;
  uint64_t n_w = 0, nx = 0, ny = 0, nz = 0;
  int32_t rc = feed_windows(f, sc, F, s, per_key, &n_w, &nx, &ny, &nz);
  if (rc) return rc;
  F.n_whits = per_key ? n_w : 0;
  F.K = ac->aut.n_keys;
  F.kc = per_key ? (unsigned long long *)reserve(f, kKc, (size_t)std::max<uint32_t>(F.K, 1) * 8) : nullptr;
  if (per_key && !F.kc) return no_memory("key counts");
  if (!F.pho && !(F.pho = (uint64_t *)reserve(f, kPho, (F.D + 1) * 8))) return no_memory("piece hit offsets");
  // the main pass: the engine and count path a plain count of the pieces takes (its timing is the call's)
  aha_match_params p{};
  p.struct_size = sizeof(p);
  uint64_t n_m = 0;
  rc = device_count(ac, sc, main_batch(f, F, &p, s), 0, (uint64_t *)F.kc, (uint64_t *)F.mdho, &n_m, as_is_if(f->fold));
  if (rc) return rc;
  *total = (nx - ny) + (n_m - nz);
  F.total = *total;
  feed_launch_count(F, s);
  feed_launch_commit(F, s);
  HIPCHK(ac, hipGetLastError());
  HIPCHK(ac, hipStreamSynchronize(s));
  return AHA_OK;
}

// a whole cover call on device-resident pieces.  Everything up to the main pass writes feed scratch only; what the caller owns
// -- piece_back, piece_hit_offsets, bases, piece_covered, the mask, and last the redacted bytes (d_redacted may be the corpus:
// the new contexts are taken from it first) -- is written once nothing can be refused any more.
int32_t feed_cover(aha_feed *f, Scratch *sc, FeedArgs &F, hipStream_t s, uint32_t *d_mask, uint8_t *d_redacted, uint8_t fill,
                   uint64_t *d_piece_covered, uint64_t *total, uint64_t *n_covered) {
  aha_ac *ac = f->ac;
  uint64_t n_w = 0, nx = 0, ny = 0, nz = 0;
  int32_t rc = feed_windows(f, sc, F, s, true, &n_w, &nx, &ny, &nz, true);
  if (rc) return rc;
  F.n_whits = nx;
  const uint64_t n_words = (F.n_bytes + 31) / 32;
  F.mask = (uint32_t *)reserve(f, kMask, n_words * 4 + 16);
  if (!F.mask) return no_memory("mask");
  if (!F.pho && !(F.pho = (uint64_t *)reserve(f, kPho, (F.D + 1) * 8))) return no_memory("piece hit offsets");
  // the main pass: the engine and cover path a plain cover of the pieces takes; it clears the mask's words itself
  aha_match_params p{};
  p.struct_size = sizeof(p);
  uint64_t n_m = 0;
  rc = device_count(ac, sc, main_batch(f, F, &p, s), 0, nullptr, (uint64_t *)F.mdho, &n_m, as_is_if(f->fold), F.mask);
  if (rc) return rc;
  *total = (nx - ny) + (n_m - nz);
  F.total = *total;
  if (F.back && F.D) HIPCHK(ac, hipMemsetAsync(F.back, 0, F.D * 4, s));
  feed_launch_cover(F, s);
  feed_launch_commit(F, s);
  HIPCHK(ac, hipGetLastError());
  uint64_t *d_total = (uint64_t *)f->buf[kMisc].p + 2;
  f->h_pin[0] = 0;
  if (F.n_bytes) {
    const uint32_t blocks = post_grid(ac);
    HIPCHK(ac, hipMemsetAsync(d_total, 0, 8, s));
    cover_launch_total(F.mask, n_words, d_total, blocks, s);
    if (d_piece_covered && F.D) cover_launch_doc_covered(F.mask, F.off, F.D, d_piece_covered, blocks, s);
    if (d_mask) HIPCHK(ac, hipMemcpyAsync(d_mask, F.mask, n_words * 4, hipMemcpyDeviceToDevice, s));
    if (d_redacted) cover_launch_redact(F.text, d_redacted, F.mask, F.n_bytes, fill, blocks, s);
    HIPCHK(ac, hipGetLastError());
    HIPCHK(ac, hipMemcpyAsync(f->h_pin, d_total, 8, hipMemcpyDeviceToHost, s));
  } else if (d_piece_covered && F.D) {
    HIPCHK(ac, hipMemsetAsync(d_piece_covered, 0, F.D * 8, s));
  }
  HIPCHK(ac, hipStreamSynchronize(s));
  *n_covered = f->h_pin[0];
  return AHA_OK;
}

int32_t no_scratch() {
  tls_err = "hipMalloc failed for the scratch of a feed select call";
  return AHA_E_HIP;
}

uint32_t select_blocks(const aha_ac *ac) { return post_grid(ac); }

// the part of a select call that writes scratch only, shared with a replace call: the windows and the main pass with the true
// hits into scratch, the extended positions, L, the masks, the walk and the rank.  -> S (everything but hold and out),
// *n_selected = the selection's total (one read-back), *n_hits = the call's true hits.  Nothing of the feed's state changes.
int32_t feed_select_settle(aha_feed *f, Scratch *sc, FeedArgs &F, uint32_t flags, FeedSelArgs &S, hipStream_t s, uint64_t *n_selected,
                           uint64_t *n_hits) {
  aha_ac *ac = f->ac;
  const uint64_t D = F.D, W = f->W;
  if (!f->d_sel) {  // the feed's first select call: no sequence has select state yet
    const size_t sel_bytes = (size_t)f->n_seqs * sizeof(FeedSelSeq), tail_bytes = std::max<size_t>((size_t)f->n_seqs * W * 8, 16);
    void *a = nullptr, *b = nullptr;
    if (hipMalloc(&a, sel_bytes) != hipSuccess || hipMalloc(&b, tail_bytes) != hipSuccess) {
      (void)hipGetLastError();
      if (a) (void)hipFree(a);
      return no_memory("select state");
    }
    hipError_t e = hipMemsetAsync(a, 0, sel_bytes, s);
    if (e == hipSuccess) e = hipMemsetAsync(b, 0, tail_bytes, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) {
      (void)hipFree(a);
      (void)hipFree(b);
      HIPCHK(ac, e);
    }
    f->d_sel = (FeedSelSeq *)a;
    f->d_tail = (unsigned long long *)b;
  }
  F.sel = f->d_sel;
  uint64_t n_w = 0, nx = 0, ny = 0, nz = 0;
  int32_t rc = feed_windows(f, sc, F, s, true, &n_w, &nx, &ny, &nz);
  if (rc) return rc;
  auto fs_reserve = [sc](FeedSelectSlot slot, size_t bytes) { return reserve_ptr(sc->fselbuf[slot], bytes, kGrowEighth); };
  S = FeedSelArgs{};
  S.sseq = f->d_sel;
  S.tail = f->d_tail;
  S.tseq = f->d_tok;
  S.final = (flags & AHA_FEED_SELECT_FINAL) ? 1u : 0u;
  S.eoff = (uint64_t *)fs_reserve(kFsExtOff, (D + 1) * 8);
  S.n0 = (uint64_t *)fs_reserve(kFsBases, std::max<uint64_t>(D, 1) * 8);
  S.cend = (unsigned long long *)fs_reserve(kFsEnds, std::max<uint64_t>(D, 1) * 8);
  S.pso = (uint64_t *)fs_reserve(kFsSelOff, (D + 1) * 8);
  uint64_t *pho = (uint64_t *)fs_reserve(kFsHitOff, (D + 1) * 8);
  if (!S.eoff || !S.n0 || !S.cend || !S.pso || !pho) return no_scratch();
  // the pieces' extended positions (the ids are checked by now); their sum comes back with the main pass
  feedsel_launch_layout(F, S, s);
  HIPCHK(ac, hipGetLastError());
  HIPCHK(ac, hipMemcpyAsync(f->h_pin + 2, S.eoff + D, 8, hipMemcpyDeviceToHost, s));
  // the main pass, with the exact count where the hit buffer of the calls before is too small
  aha_match_params p{};
  p.struct_size = sizeof(p);
  uint64_t n_m = 0;
  if (!f->buf[kMhits].bytes && !reserve(f, kMhits, 1024 * sizeof(aha_hit))) return no_memory("hits");
  for (int attempt = 0;; attempt++) {
    const uint64_t cap_m = f->buf[kMhits].bytes / sizeof(aha_hit);
    const HitOut hits_m{cap_m ? (aha_hit *)f->buf[kMhits].p : nullptr, cap_m, (uint64_t *)F.mdho};
    rc = device_match(ac, sc, checked_batch(F.text, F.off, D, F.n_bytes, &p, s), hits_m, &n_m, CallOpt::kNeutral);
    if (rc == AHA_E_CAPACITY && attempt == 0) {
      if (!reserve(f, kMhits, std::max<uint64_t>(n_m, 1024) * sizeof(aha_hit))) return no_memory("hits");
      continue;
    }
    if (rc) return rc;
    break;
  }
  HIPCHK(ac, hipStreamSynchronize(s));
  F.mhits = (const int32_t *)f->buf[kMhits].p;
  const uint64_t n_true = (nx - ny) + (n_m - nz), NE = f->h_pin[2];
  F.total = n_true;
  int32_t *hits = (int32_t *)fs_reserve(kFsHits, std::max<uint64_t>(n_true, 1) * sizeof(aha_hit));
  if (!hits) return no_scratch();
  int32_t *caller_out = F.out;
  uint64_t *caller_pho = F.pho;
  F.out = hits;
  F.pho = pho;
  feed_launch_merge(F, s);
  F.out = caller_out;
  F.pho = caller_pho;
  HIPCHK(ac, hipGetLastError());
  S.hits = hits;
  S.pho = pho;
  S.n_hits = n_true;
  S.NE = NE;
  uint64_t total = 0;
  const uint32_t blocks = select_blocks(ac);
  if (NE) {
    const uint64_t n_words = (NE + 31) / 32, n_blk = select_rank_blocks(NE);
    S.L = (unsigned long long *)fs_reserve(kFsLongest, NE * 8);
    uint32_t *masks = (uint32_t *)fs_reserve(kFsMasks, 3 * n_words * 4);
    S.blk = (unsigned long long *)fs_reserve(kFsBlocks, (n_blk + 1) * 8);
    if (!S.L || !masks || !S.blk) return no_scratch();
    S.cover = masks;
    S.start = masks + n_words;
    S.select = masks + 2 * n_words;
    HIPCHK(ac, hipMemsetAsync(S.L, 0, NE * 8, s));
    HIPCHK(ac, hipMemsetAsync(masks, 0, 3 * n_words * 4, s));
    HIPCHK(ac, hipMemsetAsync(S.cend, 0, D * 8, s));
    feedsel_launch_longest(F, S, blocks, s);
    select_launch_marks((const uint64_t *)S.L, NE, S.eoff, D, S.cover, S.start, blocks, s);
    feedsel_launch_walk(F, S, blocks, s);
    select_launch_rank(S.select, NE, (uint64_t *)S.blk, blocks, s);
    // (eoff[D] = NE: the last entry is the total)
    select_launch_rank_docs(S.select, (const uint64_t *)S.blk, S.eoff, D + 1, 0, S.pso, blocks, s);
    HIPCHK(ac, hipGetLastError());
    HIPCHK(ac, hipMemcpyAsync(f->h_pin, S.blk + n_blk, 8, hipMemcpyDeviceToHost, s));
    HIPCHK(ac, hipStreamSynchronize(s));
    total = f->h_pin[0];
  } else {
    HIPCHK(ac, hipMemsetAsync(S.pso, 0, (D + 1) * 8, s));
    if (D) HIPCHK(ac, hipMemsetAsync(S.cend, 0, D * 8, s));
  }
  *n_selected = total;
  if (n_hits) *n_hits = n_true;
  return AHA_OK;
}

// a whole select call on device-resident pieces.  Everything up to the total's read-back writes scratch only; the caller's
// hits, offsets, bases and hold and the feed's state are written once the total is known to fit.
int32_t feed_select(aha_feed *f, Scratch *sc, FeedArgs &F, uint32_t flags, aha_hit *d_out, uint64_t cap, uint64_t *d_pso,
                    uint32_t *d_hold, hipStream_t s, uint64_t *n_selected, uint64_t *n_hits) {
  aha_ac *ac = f->ac;
  const uint64_t D = F.D;
  FeedSelArgs S{};
  int32_t rc = feed_select_settle(f, sc, F, flags, S, s, n_selected, n_hits);
  if (rc) return rc;
  S.hold = d_hold;
  S.out = reinterpret_cast<int32_t *>(d_out);
  const uint64_t total = *n_selected;
  if (total > cap) {
    tls_err = "output buffer too small";
    return AHA_E_CAPACITY;
  }
  if (total) feedsel_launch_emit(F, S, select_blocks(ac), s);
  if (d_pso) HIPCHK(ac, hipMemcpyAsync(d_pso, S.pso, (D + 1) * 8, hipMemcpyDeviceToDevice, s));
  feed_launch_commit(F, s);
  feedsel_launch_commit(F, S, s);
  HIPCHK(ac, hipGetLastError());
  HIPCHK(ac, hipStreamSynchronize(s));
  return AHA_OK;
}

// a whole token call on device-resident pieces (AHA_FEED_SELECT_TOKENS; scan_feedtokens.hip): a select call's settle, the piece
// bounds, the inside and start masks over the extended positions, their rank, the edge decisions and the pieces' offsets, one
// read-back of the token total and the verdict.  Everything up to it writes scratch only; then the tokens, the offsets, the two
// commits of a select call and the token state.
int32_t feed_tokens(aha_feed *f, Scratch *sc, FeedArgs &F, uint32_t flags, aha_hit *d_out, uint64_t cap, uint64_t *d_pto,
                    uint32_t *d_hold, hipStream_t s, uint64_t *n_tokens, uint64_t *n_hits) {
  aha_ac *ac = f->ac;
  const uint64_t D = F.D;
  if (!f->d_tok) {  // the feed's first token call: no sequence has token state yet
    const size_t bytes = (size_t)f->n_seqs * sizeof(FeedTokSeq);
    void *a = nullptr;
    if (hipMalloc(&a, bytes) != hipSuccess) {
      (void)hipGetLastError();
      return no_memory("token state");
    }
    hipError_t e = hipMemsetAsync(a, 0, bytes, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) {
      (void)hipFree(a);
      HIPCHK(ac, e);
    }
    f->d_tok = (FeedTokSeq *)a;
  }
  F.tok = f->d_tok;
  FeedSelArgs S{};
  uint64_t n_sel = 0;
  int32_t rc = feed_select_settle(f, sc, F, flags & AHA_FEED_SELECT_FINAL, S, s, &n_sel, n_hits);
  if (rc) return rc;
  auto ft_reserve = [sc](FeedTokenSlot slot, size_t bytes) { return reserve_ptr(sc->ftokbuf[slot], bytes, kGrowEighth); };
  const uint64_t NE = S.NE, n_words = (NE + 31) / 32, n_blk = select_rank_blocks(NE);
  FeedTokArgs K{};
  K.tseq = f->d_tok;
  K.gap_runs = (flags & AHA_FEED_SELECT_GAP_RUNS) ? 1u : 0u;
  K.bound = ac->feed_token_open;
  K.piece = (FeedTokPiece *)ft_reserve(kFtPieces, std::max<uint64_t>(D, 1) * sizeof(FeedTokPiece));
  K.raw = (uint64_t *)ft_reserve(kFtRawOff, (D + 1) * 8);
  K.pto = (uint64_t *)ft_reserve(kFtTokOff, (D + 1) * 8);
  uint64_t *tot = (uint64_t *)ft_reserve(kFtTotal, 16);
  if (!K.piece || !K.raw || !K.pto || !tot) return no_scratch();
  K.total = tot;
  K.verdict = (uint32_t *)(tot + 1);
  HIPCHK(ac, hipMemsetAsync(tot, 0, 16, s));
  const uint32_t blocks = select_blocks(ac);
  feedtok_launch_bounds(F, S, K, blocks, s);
  if (NE) {
    uint32_t *masks = (uint32_t *)ft_reserve(kFtMasks, 2 * n_words * 4);
    K.blk = (unsigned long long *)ft_reserve(kFtBlocks, (n_blk + 1) * 8);
    if (!masks || !K.blk) return no_scratch();
    K.inside = masks;
    K.starts = masks + n_words;
    HIPCHK(ac, hipMemsetAsync(K.inside, 0, n_words * 4, s));
    tokens_launch_spans((const uint64_t *)S.L, NE, S.select, K.inside, blocks, s);
    feedtok_launch_starts(F, S, K, blocks, s);
    select_launch_rank(K.starts, NE, (uint64_t *)K.blk, blocks, s);
    select_launch_rank_docs(K.starts, (const uint64_t *)K.blk, S.eoff, D + 1, 0, K.raw, blocks, s);
  } else {
    HIPCHK(ac, hipMemsetAsync(K.raw, 0, (D + 1) * 8, s));
  }
  feedtok_launch_edge(F, S, K, blocks, s);
  HIPCHK(ac, hipGetLastError());
  HIPCHK(ac, hipMemcpyAsync(f->h_pin, tot, 16, hipMemcpyDeviceToHost, s));
  HIPCHK(ac, hipStreamSynchronize(s));
  const uint64_t total = f->h_pin[0];
  if ((uint32_t)f->h_pin[1] & 1u) {
    tls_err = "feed select with tokens: a token would stay open for more than 2^30 - 1 bytes (a run of continuation bytes); a FINAL "
              "call or AHA_FEED_SELECT_GAP_RUNS closes it";
    return AHA_E_TOO_LONG;
  }
  *n_tokens = total;
  if (total > cap) {
    tls_err = "output buffer too small";
    return AHA_E_CAPACITY;
  }
  K.out = reinterpret_cast<int32_t *>(d_out);
  K.hold = d_hold;
  if (total) feedtok_launch_emit(F, S, K, blocks, s);
  if (d_pto) HIPCHK(ac, hipMemcpyAsync(d_pto, K.pto, (D + 1) * 8, hipMemcpyDeviceToDevice, s));
  feed_launch_commit(F, s);
  feedsel_launch_commit(F, S, s);  // (S.hold is null: a token call's hold is the token cursor's)
  feedtok_launch_commit(F, S, K, blocks, s);
  HIPCHK(ac, hipGetLastError());
  HIPCHK(ac, hipStreamSynchronize(s));
  return AHA_OK;
}

// a whole replace call on device-resident pieces: a select call's settle with the selection into scratch (kfs_emit), the staged
// text T[c0 .. c1) of every piece (scan_feedreplace.hip), replace's passes over the staged batch (scan_replace.hip), one
// read-back of the byte total.  Everything up to it writes scratch only; then the copy, the offsets and both commits.
// out_slot >= 0: the result goes into that buffer of the feed, sized once the total is known (the host entry); else into d_out.
int32_t feed_replace(aha_feed *f, Scratch *sc, const aha_repl *table, FeedArgs &F, uint32_t flags, uint8_t *d_out, int out_slot,
                     uint64_t cap_bytes, uint64_t *d_poo, uint32_t *d_hold, hipStream_t s, uint64_t *n_out_bytes,
                     uint64_t *n_selected, uint64_t *n_hits) {
  aha_ac *ac = f->ac;
  const uint64_t D = F.D;
  FeedSelArgs S{};
  uint64_t n = 0, n_true = 0;
  int32_t rc = feed_select_settle(f, sc, F, flags, S, s, &n, &n_true);
  if (rc) return rc;
  auto fr_reserve = [sc](FeedReplaceSlot slot, size_t bytes) { return reserve_ptr(sc->frepbuf[slot], bytes, kGrowEighth); };
  const uint64_t max_ext = F.n_bytes + D * f->W, n_blk = replace_scan_blocks(n);
  int32_t *rows = (int32_t *)fr_reserve(kFrRows, std::max<uint64_t>(n, 1) * sizeof(aha_hit));
  FeedRepArgs R{};
  R.ext = (uint8_t *)fr_reserve(kFrExt, max_ext + 16);
  R.ext_off = (uint64_t *)fr_reserve(kFrExtOff, (D + 1) * 8);
  R.bias = (uint64_t *)fr_reserve(kFrBias, (D + 1) * 8);
  R.hold0 = (uint32_t *)fr_reserve(kFrHold0, std::max<uint64_t>(D, 1) * 4);
  uint64_t *A = (uint64_t *)fr_reserve(kFrStart, std::max<uint64_t>(n, 1) * 8);
  int64_t *shift = (int64_t *)fr_reserve(kFrShift, (n + 1) * 8);
  int64_t *sums = (int64_t *)fr_reserve(kFrSums, (n_blk + 1) * 8);
  uint64_t *poo = (uint64_t *)fr_reserve(kFrOutOff, (D + 1) * 8);
  if (!rows || !R.ext || !R.ext_off || !R.bias || !R.hold0 || !A || !shift || !sums || !poo) {
    tls_err = "hipMalloc failed for the scratch of a feed replace call";
    return AHA_E_HIP;
  }
  S.out = rows;
  if (n) feedsel_launch_emit(F, S, select_blocks(ac), s);
  const uint32_t blocks = ac->rep_blocks ? ac->rep_blocks : select_blocks(ac);
  feedrep_launch_layout(F, S, R, s);
  feedrep_launch_stage(F, R, max_ext, blocks, s);
  // the staged batch is a replace problem: the rows are relative to the piece, so bias stands for the document offsets
  replace_launch_delta(rows, n, S.pso, R.bias, D, table->d_ent, table->n_keys, A, shift, blocks, s);
  replace_launch_scan(shift, n, sums, blocks, s);
  replace_launch_doc_offsets(R.ext_off, S.pso, shift, D, poo, blocks, s);
  HIPCHK(ac, hipGetLastError());
  HIPCHK(ac, hipMemcpyAsync(f->h_pin, poo + D, 8, hipMemcpyDeviceToHost, s));
  HIPCHK(ac, hipStreamSynchronize(s));
  const uint64_t total = f->h_pin[0];
  *n_out_bytes = total;
  if (n_selected) *n_selected = n;
  if (n_hits) *n_hits = n_true;
  if (total > cap_bytes) {
    tls_err = "output buffer too small";
    return AHA_E_CAPACITY;
  }
  if (out_slot >= 0 && !(d_out = (uint8_t *)reserve(f, out_slot, total))) return no_memory("result");
  replace_launch_copy(R.ext, rows, A, shift, n, table->d_ent, table->n_keys, (const uint8_t *)table->d_blob, d_out, total, blocks, s);
  if (d_poo) HIPCHK(ac, hipMemcpyAsync(d_poo, poo, (D + 1) * 8, hipMemcpyDeviceToDevice, s));
  S.hold = d_hold;
  feed_launch_commit(F, s);
  feedsel_launch_commit(F, S, s);
  HIPCHK(ac, hipGetLastError());
  HIPCHK(ac, hipStreamSynchronize(s));
  return AHA_OK;
}

// the caller's buffers of a grep call, on the device.  The host entry gives slots of the feed's staging buffers for the three
// whose size only the call knows (>= 0: wanted; they are reserved once the totals are known)
struct GrepOut {
  uint64_t *kept = nullptr, *rec_out = nullptr;
  uint8_t *out = nullptr;
  int kept_slot = -1, rec_out_slot = -1, out_slot = -1;
  uint64_t cap_recs = 0, cap_bytes = 0;
  uint64_t *piece_rec = nullptr, *piece_kept = nullptr, *head = nullptr, *rec_bases = nullptr;
  uint32_t *hold = nullptr;
};

// a whole grep call on device-resident pieces.  Everything up to the second total's read-back writes scratch only; the caller's
// buffers and the feed's state are written once both totals are known to fit.
int32_t feed_grep(aha_feed *f, Scratch *sc, FeedArgs &F, uint8_t delim, uint32_t flags, GrepOut &O, hipStream_t s, uint64_t *n_recs,
                  uint64_t *n_kept, uint64_t *n_out_bytes, uint64_t *n_hits) {
  aha_ac *ac = f->ac;
  const uint64_t D = F.D;
  if (f->grep_delim >= 0 && f->grep_delim != (int)delim) {
    tls_err = "feed grep: the delimiter is fixed by the feed's first grep call";
    return AHA_E_INVALID;
  }
  if (!f->d_grep) {  // the feed's first grep call: no sequence has grep state yet
    const size_t bytes = (size_t)f->n_seqs * sizeof(FeedGrepSeq);
    void *a = nullptr;
    if (hipMalloc(&a, bytes) != hipSuccess) {
      (void)hipGetLastError();
      return no_memory("grep state");
    }
    hipError_t e = hipMemsetAsync(a, 0, bytes, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) {
      (void)hipFree(a);
      HIPCHK(ac, e);
    }
    f->d_grep = (FeedGrepSeq *)a;
  }
  if (++f->stamp == 0) f->stamp = 1;
  F.stamp = f->stamp;
  F.seqs = f->d_seqs;
  F.ctx = f->d_ctx;
  F.n_seqs = f->n_seqs;
  F.W = F.Wp = f->W;
  F.chars = 0;
  F.max_piece = (1ull << 31) - std::max<uint64_t>(ac->aut.max_key_len, 1);
  F.grep = f->d_grep;
  uint64_t *misc = (uint64_t *)reserve(f, kMisc, 24);
  if (!misc) return no_memory("offsets");
  F.verdict = (uint32_t *)misc;
  F.win_total = misc + 1;
  HIPCHK(ac, hipMemsetAsync(F.verdict, 0, 4, s));
  feed_launch_check_only(F, s);
  HIPCHK(ac, hipGetLastError());
  HIPCHK(ac, hipMemcpyAsync(f->h_pin, misc, 8, hipMemcpyDeviceToHost, s));
  HIPCHK(ac, hipStreamSynchronize(s));
  const uint32_t bad = (uint32_t)f->h_pin[0];
  if (bad & 1u) {
    tls_err = "feed: need piece_offsets[0] = 0, ascending, piece_offsets[n_pieces] = n_bytes, seq_ids below n_seqs and each once";
    return AHA_E_INVALID;
  }
  if (bad & 8u) {
    tls_err = "feed grep: bytes of a named sequence went through another kind of call; grep works again after its reset";
    return AHA_E_INVALID;
  }
  if (bad & 2u) {
    tls_err = "feed: a piece must be shorter than 2^31 bytes minus the longest key";
    return AHA_E_TOO_LONG;
  }
  auto fg_reserve = [sc](FeedGrepSlot slot, size_t bytes) { return reserve_ptr(sc->fgrpbuf[slot], bytes, kGrowEighth); };
  auto nomem = [&]() {
    tls_err = "hipMalloc failed for the scratch of a feed grep call";
    return AHA_E_HIP;
  };
  // the fragments: a records call over the pieces, its offsets sized from its total
  int32_t rc;
  uint64_t R = 0;
  const Batch pieces = checked_batch(F.text, F.off, D, F.n_bytes, nullptr, s);
  if ((rc = device_records_settle(ac, sc, pieces, delim, &R))) return rc;
  uint64_t *frag = (uint64_t *)fg_reserve(kFgFragOff, (R + 1) * 8);
  uint64_t *pro = (uint64_t *)fg_reserve(kFgPieceFrag, (D + 1) * 8);
  if (!frag || !pro) return nomem();
  if ((rc = device_records_emit(ac, sc, pieces, frag, pro))) return rc;
  F.woff = (uint64_t *)fg_reserve(kFgWinOff, (3 * D + 1) * 8);
  uint64_t *wdho = (uint64_t *)fg_reserve(kFgWinHitOff, (3 * D + 1) * 8);
  uint64_t *fdho = (uint64_t *)fg_reserve(kFgFragHitOff, (R + 1) * 8);
  const uint32_t blocks = grep_grid(ac);
  const uint64_t n_words = (R + 31) / 32, n_blk = select_rank_blocks(R);
  uint8_t *flag = (uint8_t *)fg_reserve(kFgFlags, std::max<uint64_t>(R, 1));
  uint32_t *masks = (uint32_t *)fg_reserve(kFgMasks, std::max<uint64_t>(n_words, 1) * 3 * 4);
  uint64_t *blks = (uint64_t *)fg_reserve(kFgBlocks, (n_blk + 1) * 3 * 8);
  RepEntry *ent = (RepEntry *)fg_reserve(kFgTable, sizeof(RepEntry));
  if (!F.woff || !wdho || !fdho || !flag || !masks || !blks || !ent) return nomem();
  F.wdho = wdho;
  FeedGrepArgs G{};
  G.gseq = f->d_grep;
  G.delim = delim;
  G.invert = (flags & AHA_GREP_INVERT) ? 1u : 0u;
  G.final = (flags & AHA_FEED_GREP_FINAL) ? 1u : 0u;
  G.R = R;
  G.frag = frag;
  G.pro = pro;
  G.fdho = fdho;
  G.flag = flag;
  G.keep = masks;
  G.S = masks + n_words;
  G.T = masks + 2 * n_words;
  // the windows of the pieces whose first fragment continues an open record
  feedgrep_launch_layout(F, G, s);
  HIPCHK(ac, hipGetLastError());
  HIPCHK(ac, hipMemcpyAsync(f->h_pin, F.win_total, 8, hipMemcpyDeviceToHost, s));
  HIPCHK(ac, hipStreamSynchronize(s));
  const uint64_t n_win = f->h_pin[0];
  F.win = (uint8_t *)fg_reserve(kFgWin, n_win + 64);
  if (!F.win) return nomem();
  if (n_win) {
    feedgrep_launch_windows(F, G, s);
    HIPCHK(ac, hipGetLastError());
  }
  // both counts without key counts: a count call never writes the handle's back-off state.  The fragments' pass last: it is
  // the engine and count path a plain grep of them takes, and its timing is the call's
  aha_match_params p{};
  p.struct_size = sizeof(p);
  uint64_t n_w = 0, n_m = 0;
  if ((rc = device_count(ac, sc, checked_batch(F.win, F.woff, 3 * D, n_win, &p, s), 0, nullptr, wdho, &n_w))) return rc;
  if ((rc = device_count(ac, sc, checked_batch(F.text, frag, R, F.n_bytes, &p, s), 0, nullptr, fdho, &n_m))) return rc;
  // grep's steps over the fragments (engine.cpp device_grep)
  uint64_t *blk_k = blks, *blk_s = blks + (n_blk + 1), *blk_t = blks + 2 * (n_blk + 1);
  feedgrep_launch_flag(F, G, blocks, s);
  select_launch_rank(G.keep, R, blk_k, blocks, s);
  select_launch_rank(G.S, R, blk_s, blocks, s);
  select_launch_rank(G.T, R, blk_t, blocks, s);
  HIPCHK(ac, hipGetLastError());
  HIPCHK(ac, hipMemcpyAsync(f->h_pin, blk_k + n_blk, 8, hipMemcpyDeviceToHost, s));
  HIPCHK(ac, hipMemcpyAsync(f->h_pin + 1, blk_s + n_blk, 8, hipMemcpyDeviceToHost, s));
  HIPCHK(ac, hipStreamSynchronize(s));
  const uint64_t kept = f->h_pin[0], n_runs = f->h_pin[1];
  const uint64_t n_sum = replace_scan_blocks(n_runs);
  aha_hit *sel = (aha_hit *)fg_reserve(kFgSel, std::max<uint64_t>(n_runs, 1) * sizeof(aha_hit));
  uint64_t *A = (uint64_t *)fg_reserve(kFgStart, std::max<uint64_t>(n_runs, 1) * 8);
  int64_t *shift = (int64_t *)fg_reserve(kFgShift, (n_runs + 1) * 8);
  int64_t *sums = (int64_t *)fg_reserve(kFgSums, (n_sum + 1) * 8);
  if (!sel || !A || !shift || !sums) return nomem();
  grep_launch_runs(G.S, G.T, R, blk_s, blk_t, frag, n_runs, A, shift, sel, ent, blocks, s);
  replace_launch_scan(shift, n_runs, sums, blocks, s);
  HIPCHK(ac, hipGetLastError());
  HIPCHK(ac, hipMemcpyAsync(f->h_pin, shift + n_runs, 8, hipMemcpyDeviceToHost, s));
  HIPCHK(ac, hipStreamSynchronize(s));
  const uint64_t total = (uint64_t)((int64_t)F.n_bytes + (int64_t)f->h_pin[0]);
  if (n_recs) *n_recs = R;
  *n_kept = kept;
  if (n_out_bytes) *n_out_bytes = total;
  if (n_hits) *n_hits = n_m;
  const bool per_rec = O.kept || O.rec_out || O.kept_slot >= 0 || O.rec_out_slot >= 0, want_out = O.out || O.out_slot >= 0;
  if ((per_rec && kept > O.cap_recs) || (want_out && total > O.cap_bytes)) {
    tls_err = "output buffer too small";
    return AHA_E_CAPACITY;
  }
  // the part that writes: the caller's buffers, then the feed's own state and, behind it, the grep state
  if (O.kept_slot >= 0 && !(O.kept = (uint64_t *)reserve(f, O.kept_slot, kept * 8))) return no_memory("result");
  if (O.rec_out_slot >= 0 && !(O.rec_out = (uint64_t *)reserve(f, O.rec_out_slot, (kept + 1) * 8))) return no_memory("result");
  if (O.out_slot >= 0 && !(O.out = (uint8_t *)reserve(f, O.out_slot, total))) return no_memory("result");
  if (per_rec) grep_launch_emit_docs(G.keep, G.S, R, blk_k, blk_s, frag, shift, n_runs, O.kept, O.rec_out, blocks, s);
  if (want_out) replace_launch_copy(F.text, sel, A, shift, n_runs, ent, 1, (const uint8_t *)ent, O.out, total, blocks, s);
  if (O.piece_kept) {
    if (R)
      select_launch_rank_docs(G.keep, blk_k, pro, D + 1, 0, O.piece_kept, blocks, s);
    else
      HIPCHK(ac, hipMemsetAsync(O.piece_kept, 0, (D + 1) * 8, s));
  }
  if (O.piece_rec) HIPCHK(ac, hipMemcpyAsync(O.piece_rec, pro, (D + 1) * 8, hipMemcpyDeviceToDevice, s));
  G.hold = O.hold;
  G.head = O.head;
  G.rec_bases = O.rec_bases;
  feed_launch_commit(F, s);
  feedgrep_launch_commit(F, G, blocks, s);
  HIPCHK(ac, hipGetLastError());
  HIPCHK(ac, hipStreamSynchronize(s));
  f->grep_delim = delim;
  return AHA_OK;
}

// the part that writes: the caller's hits and offsets, then the feed's own state
int32_t feed_emit(aha_feed *f, FeedArgs &F, hipStream_t s) {
  if (!F.pho) {
    F.pho = (uint64_t *)reserve(f, kPho, (F.D + 1) * 8);
    if (!F.pho) return no_memory("piece hit offsets");
  }
  feed_launch_merge(F, s);
  feed_launch_commit(F, s);
  HIPCHK(f->ac, hipGetLastError());
  HIPCHK(f->ac, hipStreamSynchronize(s));
  return AHA_OK;
}

int32_t no_sep_scratch() {
  tls_err = "hipMalloc failed for the scratch of a call on a feed with a separator filter";
  return AHA_E_HIP;
}

int32_t sep_refused(const char *what) {
  tls_err = std::string("feed ") + what + ": the feed has a separator filter, which feed " + what +
            " calls do not take yet (a follow-up); feed match and count calls do";
  return AHA_E_INVALID;
}

uint32_t sep_blocks(const aha_ac *ac) { return post_grid(ac); }

// the keep mask of P.n_true hits and its rank; *n_kept = the total (one read-back)
int32_t feed_sep_rank(aha_feed *f, Scratch *sc, const FeedArgs &F, FeedSepArgs &P, bool finish, hipStream_t s, uint64_t *n_kept) {
  aha_ac *ac = f->ac;
  *n_kept = 0;
  if (!P.n_true) return AHA_OK;
  const uint64_t n_blk = select_rank_blocks(P.n_true);
  P.keep = (unsigned long long *)reserve_ptr(sc->fsepbuf[kFpKeep], ((P.n_true + 63) / 64) * 8, kGrowEighth);
  P.blk = (unsigned long long *)reserve_ptr(sc->fsepbuf[kFpBlocks], (n_blk + 1) * 8, kGrowEighth);
  if (!P.keep || !P.blk) return no_sep_scratch();
  if (finish)
    feedsep_launch_flag_finish(F, P, sep_blocks(ac), s);
  else
    feedsep_launch_flag(F, P, sep_blocks(ac), s);
  select_launch_rank(reinterpret_cast<const uint32_t *>(P.keep), P.n_true, reinterpret_cast<uint64_t *>(P.blk), sep_blocks(ac), s);
  HIPCHK(ac, hipGetLastError());
  HIPCHK(ac, hipMemcpyAsync(f->h_pin, P.blk + n_blk, 8, hipMemcpyDeviceToHost, s));
  HIPCHK(ac, hipStreamSynchronize(s));
  *n_kept = f->h_pin[0];
  return AHA_OK;
}

// the filtered offsets: the rank at every piece's first true hit (off: D + 1 entries, off[D] = P.n_true)
int32_t feed_sep_offsets(aha_feed *f, const FeedSepArgs &P, const uint64_t *off, uint64_t D, uint64_t *d_out, hipStream_t s) {
  if (!d_out) return AHA_OK;
  if (P.n_true)
    select_launch_rank_docs(reinterpret_cast<const uint32_t *>(P.keep), reinterpret_cast<const uint64_t *>(P.blk), off, D + 1, 0, d_out,
                            sep_blocks(f->ac), s);
  else
    HIPCHK(f->ac, hipMemsetAsync(d_out, 0, (D + 1) * 8, s));
  return AHA_OK;
}

// the part of a match or count call on a feed with a separator filter that writes scratch only: the windows and the main pass
// unfiltered, the call's true hits piece by piece (the hits that ended with the pieces before included), the keep mask and its
// rank.  *n_kept = the hits the call reports, also F.total.
int32_t feed_sep_true(aha_feed *f, Scratch *sc, FeedArgs &F, hipStream_t s, FeedSepArgs &P, uint64_t *n_kept) {
  aha_ac *ac = f->ac;
  const uint64_t D = F.D;
  uint64_t n_w = 0, nx = 0, ny = 0, nz = 0;
  int32_t rc = feed_windows(f, sc, F, s, true, &n_w, &nx, &ny, &nz);
  if (rc) return rc;
  // the main pass, with the exact count where the hit buffer of the calls before is too small (the caller's cap says nothing
  // about the unfiltered hits); like a count call it writes none of the handle's back-off state
  aha_match_params p{};
  p.struct_size = sizeof(p);
  uint64_t n_m = 0;
  if (!f->buf[kMhits].bytes && !reserve(f, kMhits, 1024 * sizeof(aha_hit))) return no_memory("hits");
  for (int attempt = 0;; attempt++) {
    const uint64_t cap_m = f->buf[kMhits].bytes / sizeof(aha_hit);
    const HitOut hits_m{cap_m ? (aha_hit *)f->buf[kMhits].p : nullptr, cap_m, (uint64_t *)F.mdho};
    rc = device_match(ac, sc, checked_batch(F.text, F.off, D, F.n_bytes, &p, s), hits_m, &n_m, CallOpt::kNeutral);
    if (rc == AHA_E_CAPACITY && attempt == 0) {
      if (!reserve(f, kMhits, std::max<uint64_t>(n_m, 1024) * sizeof(aha_hit))) return no_memory("hits");
      continue;
    }
    if (rc) return rc;
    break;
  }
  F.mhits = (const int32_t *)f->buf[kMhits].p;
  F.edge = (uint64_t *)reserve_ptr(sc->fsepbuf[kFpEdge], std::max<uint64_t>(D, 1) * 8, kGrowEighth);
  uint64_t *tho = (uint64_t *)reserve_ptr(sc->fsepbuf[kFpTrueOff], (D + 1) * 8, kGrowEighth);
  if (!F.edge || !tho) return no_sep_scratch();
  int32_t *caller_out = F.out;
  uint64_t *caller_pho = F.pho;
  F.pho = tho;
  feed_launch_edge(F, s);
  HIPCHK(ac, hipGetLastError());
  HIPCHK(ac, hipMemcpyAsync(f->h_pin, tho + D, 8, hipMemcpyDeviceToHost, s));
  HIPCHK(ac, hipStreamSynchronize(s));
  const uint64_t n_true = f->h_pin[0];
  int32_t *hits = (int32_t *)reserve_ptr(sc->fsepbuf[kFpTrue], std::max<uint64_t>(n_true, 1) * sizeof(aha_hit), kGrowEighth);
  if (!hits) return no_sep_scratch();
  F.out = hits;
  F.total = n_true;
  feed_launch_merge_edge(F, s);
  F.out = caller_out;
  F.pho = caller_pho;
  HIPCHK(ac, hipGetLastError());
  memcpy(P.blocked, f->blocked, sizeof(P.blocked));
  P.fold = ac->fold() ? 1u : 0u;
  P.hits = hits;
  P.tho = tho;
  P.n_true = n_true;
  if ((rc = feed_sep_rank(f, sc, F, P, false, s, n_kept))) return rc;
  F.total = *n_kept;
  return AHA_OK;
}

int32_t feed_sep_prepare(aha_feed *f, Scratch *sc, FeedArgs &F, uint64_t cap, hipStream_t s, FeedSepArgs &P, uint64_t *total) {
  int32_t rc = feed_sep_true(f, sc, F, s, P, total);
  if (rc) return rc;
  if (*total > cap) {
    tls_err = "output buffer too small";
    return AHA_E_CAPACITY;
  }
  return AHA_OK;
}

// the part that writes: the kept hits and their offsets, then the feed's own state
int32_t feed_sep_emit(aha_feed *f, FeedArgs &F, FeedSepArgs &P, hipStream_t s) {
  P.out = F.out;
  if (F.total) feedsep_launch_compact(P, false, sep_blocks(f->ac), s);
  int32_t rc = feed_sep_offsets(f, P, P.tho, F.D, F.pho, s);
  if (rc) return rc;
  feed_launch_commit(F, s);
  HIPCHK(f->ac, hipGetLastError());
  HIPCHK(f->ac, hipStreamSynchronize(s));
  return AHA_OK;
}

// a whole count call on a feed with a separator filter: the true hit list is built in scratch as for a match call (12 bytes per
// unfiltered hit: what this count form costs beyond the plain one), the kept hits' values summed per key
int32_t feed_sep_count(aha_feed *f, Scratch *sc, FeedArgs &F, hipStream_t s, uint64_t *total) {
  aha_ac *ac = f->ac;
  FeedSepArgs P{};
  int32_t rc = feed_sep_true(f, sc, F, s, P, total);
  if (rc) return rc;
  F.K = ac->aut.n_keys;
  if (F.key_counts && F.K) {
    F.kc = (unsigned long long *)reserve(f, kKc, (size_t)F.K * 8);
    if (!F.kc) return no_memory("key counts");
    HIPCHK(ac, hipMemsetAsync(F.kc, 0, (size_t)F.K * 8, s));
    if (*total) feedsep_launch_count(F, P, sep_blocks(ac), s);
    feedsep_launch_count_finish(F, sep_blocks(ac), s);
  }
  if ((rc = feed_sep_offsets(f, P, P.tho, F.D, F.pho, s))) return rc;
  feed_launch_commit(F, s);
  HIPCHK(ac, hipGetLastError());
  HIPCHK(ac, hipStreamSynchronize(s));
  return AHA_OK;
}

// a whole finish call on device-resident ids: the named sequences' contexts matched as the window batch of a call of empty
// pieces (which checks the ids on the device: kfd_check), the hits of its X block that end on the context's last byte and pass on
// the left.  Everything up to the total's read-back writes scratch only.
int32_t feed_finish_sep(aha_feed *f, Scratch *sc, const uint32_t *d_ids, uint64_t D, aha_hit *d_out, uint64_t cap, uint64_t *d_sho,
                        uint64_t *d_bases, hipStream_t s, uint64_t *total) {
  aha_ac *ac = f->ac;
  uint64_t *zero = (uint64_t *)reserve_ptr(sc->fsepbuf[kFpZeroOff], (D + 1) * 8, kGrowEighth);
  if (!zero) return no_sep_scratch();
  HIPCHK(ac, hipMemsetAsync(zero, 0, (D + 1) * 8, s));
  FeedArgs F{};
  F.off = zero;
  F.ids = d_ids;
  F.D = D;
  uint64_t n_w = 0, nx = 0, ny = 0, nz = 0;
  int32_t rc = feed_windows(f, sc, F, s, true, &n_w, &nx, &ny, &nz);
  if (rc) return rc;
  FeedSepArgs P{};
  memcpy(P.blocked, f->blocked, sizeof(P.blocked));
  P.fold = ac->fold() ? 1u : 0u;
  P.hits = F.whits;
  P.tho = F.wdho;  // (its first D + 1 entries: the X block)
  P.n_true = nx;
  P.out = reinterpret_cast<int32_t *>(d_out);
  P.bases = d_bases;
  if ((rc = feed_sep_rank(f, sc, F, P, true, s, total))) return rc;
  if (*total > cap) {
    tls_err = "output buffer too small";
    return AHA_E_CAPACITY;
  }
  if (*total) feedsep_launch_compact(P, true, sep_blocks(ac), s);
  if ((rc = feed_sep_offsets(f, P, F.wdho, D, d_sho, s))) return rc;
  feedsep_launch_restart(F, P, s);
  HIPCHK(ac, hipGetLastError());
  HIPCHK(ac, hipStreamSynchronize(s));
  return AHA_OK;
}

int32_t longest_refused(const char *what) {
  tls_err = std::string("feed ") + what + ": the feed was opened for match_longest, which feed " + what +
            " calls do not take yet (a follow-up); feed match and finish calls do";
  return AHA_E_INVALID;
}

// kfd_check alone and its verdict: the first step of a call on a longest feed (F.off, F.ids, F.D, F.n_bytes are the call's)
int32_t feed_long_check(aha_feed *f, FeedArgs &F, hipStream_t s) {
  aha_ac *ac = f->ac;
  if (++f->stamp == 0) f->stamp = 1;
  F.stamp = f->stamp;
  F.seqs = f->d_seqs;
  F.n_seqs = f->n_seqs;
  F.max_piece = (1ull << 31) - std::max<uint64_t>(ac->aut.max_key_len, 1);
  uint64_t *misc = (uint64_t *)reserve(f, kMisc, 24);
  if (!misc) return no_memory("offsets");
  F.verdict = (uint32_t *)misc;
  HIPCHK(ac, hipMemsetAsync(F.verdict, 0, 4, s));
  feed_launch_check_only(F, s);
  HIPCHK(ac, hipGetLastError());
  HIPCHK(ac, hipMemcpyAsync(f->h_pin, misc, 8, hipMemcpyDeviceToHost, s));
  HIPCHK(ac, hipStreamSynchronize(s));
  const uint32_t bad = (uint32_t)f->h_pin[0];
  if (bad & 1u) {
    tls_err = "feed: need piece_offsets[0] = 0, ascending, piece_offsets[n_pieces] = n_bytes, seq_ids below n_seqs and each once";
    return AHA_E_INVALID;
  }
  if (bad & 2u) {
    tls_err = "feed: a piece must be shorter than 2^31 bytes minus the longest key";
    return AHA_E_TOO_LONG;
  }
  return AHA_OK;
}

// the part of a match call on a longest feed that writes scratch only: the check and pass 1.  *total = the call's hits;
// AHA_E_CAPACITY when they are more than cap.
int32_t feed_long_prepare(aha_feed *f, Scratch *sc, FeedArgs &F, uint64_t cap, hipStream_t s, FeedLongArgs &L, FeedLongPlan &P,
                          uint64_t *total) {
  int32_t rc = feed_long_check(f, F, s);
  if (rc) return rc;
  L = FeedLongArgs{};
  L.lseq = f->d_long;
  *total = 0;
  if (F.n_bytes && (rc = device_feed_longest_count(f->ac, sc, F, L, f->longest, P, total, s))) return rc;
  F.total = *total;
  if (*total > cap) {
    tls_err = "output buffer too small";
    return AHA_E_CAPACITY;
  }
  return AHA_OK;
}

// the part that writes: the caller's hits and offsets, then the feed's own state
int32_t feed_long_emit(aha_feed *f, FeedArgs &F, const FeedLongArgs &L, FeedLongPlan &P, uint64_t cap, hipStream_t s) {
  aha_ac *ac = f->ac;
  if (!F.pho && !(F.pho = (uint64_t *)reserve(f, kPho, (F.D + 1) * 8))) return no_memory("piece hit offsets");
  if (F.n_bytes) {
    int32_t rc = device_feed_longest_write(ac, F, L, P, reinterpret_cast<aha_hit *>(F.out), cap, F.pho, s);
    if (rc) return rc;
  } else {
    HIPCHK(ac, hipMemsetAsync(F.pho, 0, (F.D + 1) * 8, s));
  }
  feedlong_launch_commit(F, L, s);
  HIPCHK(ac, hipGetLastError());
  HIPCHK(ac, hipStreamSynchronize(s));
  return AHA_OK;
}

// a whole finish call on a longest feed, device-resident ids: the ids checked as the ids of a call of empty pieces, the named
// sequences' pending hits counted (one read-back), then -- once they fit -- written, with the bases, and the sequences restarted
int32_t feed_finish_long(aha_feed *f, Scratch *sc, const uint32_t *d_ids, uint64_t D, aha_hit *d_out, uint64_t cap, uint64_t *d_sho,
                         uint64_t *d_bases, hipStream_t s, uint64_t *total) {
  aha_ac *ac = f->ac;
  uint64_t *zero = (uint64_t *)reserve_ptr(sc->fsepbuf[kFpZeroOff], (D + 1) * 8, kGrowEighth);
  if (!zero) return no_memory("offsets");
  HIPCHK(ac, hipMemsetAsync(zero, 0, (D + 1) * 8, s));
  FeedArgs F{};
  F.off = zero;
  F.ids = d_ids;
  F.D = D;
  int32_t rc = feed_long_check(f, F, s);
  if (rc) return rc;
  if (!(F.pho = (uint64_t *)reserve(f, kPho, (D + 1) * 8))) return no_memory("piece hit offsets");
  FeedLongArgs L{};
  L.lseq = f->d_long;
  L.sho = d_sho;
  F.out = reinterpret_cast<int32_t *>(d_out);
  F.bases = d_bases;
  feedlong_launch_finish(F, L, ac->dev.key_ln, false, s);
  HIPCHK(ac, hipGetLastError());
  HIPCHK(ac, hipMemcpyAsync(f->h_pin, F.pho + D, 8, hipMemcpyDeviceToHost, s));
  HIPCHK(ac, hipStreamSynchronize(s));
  *total = f->h_pin[0];
  if (*total > cap) {
    tls_err = "output buffer too small";
    return AHA_E_CAPACITY;
  }
  feedlong_launch_finish(F, L, ac->dev.key_ln, true, s);
  HIPCHK(ac, hipGetLastError());
  HIPCHK(ac, hipStreamSynchronize(s));
  return AHA_OK;
}

// a whole match call on device-resident pieces, whatever the feed was opened for: the part that writes scratch only (*total =
// the call's hits; above cap -> AHA_E_CAPACITY, nothing committed), then the part that writes.  out_slot >= 0: the hits go into
// that buffer of the feed, sized once the total is known (the host entry); else into d_out.
int32_t feed_match(aha_feed *f, Scratch *sc, FeedArgs &F, aha_hit *d_out, int out_slot, uint64_t cap, hipStream_t s, uint64_t *total) {
  FeedSepArgs P{};
  FeedLongArgs L{};
  FeedLongPlan plan;
  int32_t rc = f->longest ? feed_long_prepare(f, sc, F, cap, s, L, plan, total)
               : f->sep   ? feed_sep_prepare(f, sc, F, cap, s, P, total)
                          : feed_prepare(f, sc, F, cap, s, total);
  if (rc) return rc;
  if (out_slot >= 0 && !(d_out = (aha_hit *)reserve(f, out_slot, *total * sizeof(aha_hit)))) return no_memory("hits");
  F.out = reinterpret_cast<int32_t *>(d_out);
  if (f->longest) return feed_long_emit(f, F, L, plan, out_slot >= 0 ? *total : cap, s);
  return f->sep ? feed_sep_emit(f, F, P, s) : feed_emit(f, F, s);
}

// a whole finish call on device-resident ids
int32_t feed_finish(aha_feed *f, Scratch *sc, const uint32_t *d_ids, uint64_t D, aha_hit *d_out, uint64_t cap, uint64_t *d_sho,
                    uint64_t *d_bases, hipStream_t s, uint64_t *total) {
  return f->longest ? feed_finish_long(f, sc, d_ids, D, d_out, cap, d_sho, d_bases, s, total)
                    : feed_finish_sep(f, sc, d_ids, D, d_out, cap, d_sho, d_bases, s, total);
}

// ---- what the public entries share ------------------------------------------------------------------------------------
bool bad_feed(const aha_feed *f) { return !f || !f->ac || f->ac->device < 0; }

// one call's scope: the feed's mutex, its device, one of the handle's scratch sets -- taken in this order
struct FeedCall {
  std::lock_guard<std::mutex> lk;
  DeviceGuard g;
  Lease lease;
  explicit FeedCall(aha_feed *f) : lk(f->mu), g(f->ac->device), lease(f->ac) {}
  Scratch *sc() { return lease.get(); }
};

// the arguments of a call as every family takes them; what is its own (key_counts, accumulate, back, out) the family sets
FeedArgs feed_args(const uint8_t *text, const uint64_t *off, const uint32_t *ids, uint64_t D, uint64_t n_bytes, uint64_t *pho,
                   uint64_t *bases) {
  FeedArgs F{};
  F.text = text;
  F.off = off;
  F.ids = ids;
  F.D = D;
  F.n_bytes = n_bytes;
  F.pho = pho;
  F.bases = bases;
  return F;
}

// the ids a call names: each below n_seqs and only once (what kfd_check asks of them)
struct SeenIds {
  std::vector<uint8_t> seen;
  bool init(uint32_t n_seqs) {
    try {
      seen.assign(n_seqs, 0);
    } catch (...) {
      return false;
    }
    return true;
  }
  bool take(uint32_t id) { return id < seen.size() && !seen[id]++; }
};

// the checks kfd_check makes, on the host (the host entries)
int32_t check_pieces_host(const aha_feed *f, const uint64_t *piece_offsets, const uint32_t *seq_ids, uint64_t n_pieces) {
  if (piece_offsets[0] != 0) return AHA_E_INVALID;
  const uint64_t max_piece = (1ull << 31) - std::max<uint64_t>(f->ac->aut.max_key_len, 1);
  SeenIds seen;
  if (!seen.init(f->n_seqs)) return AHA_E_NOMEM;
  for (uint64_t d = 0; d < n_pieces; d++) {
    if (piece_offsets[d + 1] < piece_offsets[d] || !seen.take(seq_ids[d])) return AHA_E_INVALID;
    if (piece_offsets[d + 1] - piece_offsets[d] >= max_piece) return AHA_E_TOO_LONG;
  }
  return AHA_OK;
}

// ... and of a finish call's ids
int32_t check_ids_host(const aha_feed *f, const uint32_t *seq_ids, uint64_t n_named) {
  SeenIds seen;
  if (!seen.init(f->n_seqs)) return AHA_E_NOMEM;
  for (uint64_t d = 0; d < n_named; d++)
    if (!seen.take(seq_ids[d])) {
      tls_err = "feed finish: need seq_ids below n_seqs and each once";
      return AHA_E_INVALID;
    }
  return AHA_OK;
}

int32_t overlap_refused(const char *what, const uint8_t *corpus, uint64_t n_bytes, const uint8_t *out, uint64_t cap_bytes) {
  if (cap_bytes && n_bytes && corpus) {
    const uintptr_t o0 = reinterpret_cast<uintptr_t>(out), c0 = reinterpret_cast<uintptr_t>(corpus);
    if (o0 < c0 + n_bytes && c0 < o0 + cap_bytes) {
      tls_err = std::string("feed ") + what + " calls have no in-place form: out overlaps the corpus";
      return AHA_E_INVALID;
    }
  }
  return AHA_OK;
}

// what a host entry stages beside the pieces (stage_pieces): the per-piece arrays of its family, and for grep the caller's
// result buffer, which must not overlap the corpus
enum { kWantHold = 1, kWantBack = 2, kWantCov = 4, kWantGrep = 8 };
struct StageAsk {
  unsigned want = 0;
  const uint8_t *out = nullptr;
  uint64_t cap_bytes = 0;
};
// the staged pieces of a host call, on the device.  pho stands for the family's (D + 1)-entry offsets
struct Staged {
  uint64_t n_bytes;
  uint8_t *corpus;
  uint64_t *off;
  uint32_t *ids;
  uint64_t *pho, *bases;
  uint32_t *hold, *back;                                // kWantHold, kWantBack
  uint64_t *cov;                                        // kWantCov
  uint64_t *piece_rec, *piece_kept, *head, *rec_bases;  // kWantGrep
};

// the host entries' prologue: the pieces checked as kfd_check checks them -- before the lock is taken -- then the call's scope,
// the staging buffers and the upload over the feed's stream
int32_t stage_pieces(aha_feed *f, std::optional<FeedCall> &call, const uint8_t *corpus, const uint64_t *piece_offsets,
                     const uint32_t *seq_ids, uint64_t n_pieces, const StageAsk &ask, Staged &B) {
  int32_t rc = check_pieces_host(f, piece_offsets, seq_ids, n_pieces);
  if (rc) return rc;
  const uint64_t n_bytes = piece_offsets[n_pieces], D = n_pieces;
  if (n_bytes && !corpus) return AHA_E_INVALID;
  if ((rc = overlap_refused("grep", corpus, n_bytes, ask.out, ask.cap_bytes))) return rc;
  call.emplace(f);
  hipStream_t s = f->hs;
  B = Staged{};
  B.n_bytes = n_bytes;
  uint8_t *d_corpus = B.corpus = (uint8_t *)reserve(f, kHCorpus, n_bytes + 64);
  uint64_t *d_off = B.off = (uint64_t *)reserve(f, kHOff, (D + 1) * 8);
  uint32_t *d_ids = B.ids = (uint32_t *)reserve(f, kHIds, D * 4);
  B.pho = (uint64_t *)reserve(f, kHPho, (D + 1) * 8);
  B.bases = (uint64_t *)reserve(f, kHBases, D * 8);
  bool ok = d_corpus && d_off && d_ids && B.pho && B.bases;
  if (ask.want & kWantHold) ok &= (B.hold = (uint32_t *)reserve(f, kHHold, D * 4)) != nullptr;
  if (ask.want & kWantBack) ok &= (B.back = (uint32_t *)reserve(f, kHBack, D * 4)) != nullptr;
  if (ask.want & kWantCov) ok &= (B.cov = (uint64_t *)reserve(f, kHCov, D * 8)) != nullptr;
  if (ask.want & kWantGrep) {
    ok &= (B.piece_rec = (uint64_t *)reserve(f, kHPieceRec, (D + 1) * 8)) != nullptr;
    ok &= (B.piece_kept = (uint64_t *)reserve(f, kHPieceKept, (D + 1) * 8)) != nullptr;
    ok &= (B.head = (uint64_t *)reserve(f, kHHead, D * 8)) != nullptr;
    ok &= (B.rec_bases = (uint64_t *)reserve(f, kHRecBases, D * 8)) != nullptr;
  }
  if (!ok) return no_memory("staging buffers");
  // (the names HIPCHK quotes in aha_last_error, as the entries had them)
  if (n_bytes) HIPCHK(f->ac, hipMemcpyAsync(d_corpus, corpus, n_bytes, hipMemcpyHostToDevice, s));
  HIPCHK(f->ac, hipMemcpyAsync(d_off, piece_offsets, (D + 1) * 8, hipMemcpyHostToDevice, s));
  if (D) HIPCHK(f->ac, hipMemcpyAsync(d_ids, seq_ids, D * 4, hipMemcpyHostToDevice, s));
  return AHA_OK;
}

// the host entries' epilogue: what the caller asked for comes back over the feed's stream, then the stream is awaited.  A null
// array and an empty one are skipped: a per-piece array where D == 0 (the (D + 1)-entry offsets are never empty)
struct Back {
  void *dst;
  const void *src;
  size_t bytes;
};
int32_t fetch(aha_feed *f, std::initializer_list<Back> back) {
  hipStream_t s = f->hs;
  for (const Back &b : back)
    if (b.dst && b.bytes) HIPCHK(f->ac, hipMemcpyAsync(b.dst, b.src, b.bytes, hipMemcpyDeviceToHost, s));
  HIPCHK(f->ac, hipStreamSynchronize(s));
  return AHA_OK;
}

// the argument checks both entries of a family share, before any device work.  no_corpus: a device entry's n_bytes && !d_corpus
// (a host entry knows n_bytes only from the offsets it has yet to check: stage_pieces)
int32_t feed_match_args(const aha_feed *f, const uint64_t *piece_offsets, const uint32_t *seq_ids, uint64_t n_pieces, const aha_hit *out,
                        uint64_t cap, const uint64_t *n_hits, bool no_corpus) {
  if (!f || !n_hits || !piece_offsets || (n_pieces && !seq_ids) || (cap && !out) || no_corpus) return AHA_E_INVALID;
  if (bad_feed(f)) return AHA_E_NO_DEVICE;
  return AHA_OK;
}

int32_t feed_finish_args(const aha_feed *f, const uint32_t *seq_ids, uint64_t n_named, const aha_hit *out, uint64_t cap,
                         const uint64_t *n_hits) {
  if (!f || !n_hits || (n_named && !seq_ids) || (cap && !out)) return AHA_E_INVALID;
  if (bad_feed(f)) return AHA_E_NO_DEVICE;
  if (!f->sep && !f->longest) {
    tls_err = "feed finish: the feed has neither a separator filter nor match_longest (aha_feed_open_params); its sequences end with "
              "aha_feed_reset";
    return AHA_E_INVALID;
  }
  return AHA_OK;
}

int32_t feed_count_args(const aha_feed *f, const uint64_t *piece_offsets, const uint32_t *seq_ids, uint64_t n_pieces, uint32_t flags,
                        const uint64_t *n_hits, bool no_corpus) {
  if (!f || !n_hits || !piece_offsets || (n_pieces && !seq_ids) || no_corpus || (flags & ~AHA_COUNT_ACCUMULATE)) return AHA_E_INVALID;
  if (bad_feed(f)) return AHA_E_NO_DEVICE;
  if (f->longest) return longest_refused("count");
  return AHA_OK;
}

int32_t feed_cover_args(const aha_feed *f, const uint64_t *piece_offsets, const uint32_t *seq_ids, uint64_t n_pieces, uint32_t flags,
                        const uint64_t *n_covered, bool no_corpus) {
  if (!f || !n_covered || !piece_offsets || (n_pieces && !seq_ids) || no_corpus || flags) return AHA_E_INVALID;
  if (bad_feed(f)) return AHA_E_NO_DEVICE;
  if (f->sep) return sep_refused("cover");
  if (f->longest) return longest_refused("cover");
  return AHA_OK;
}

// a family that works in bytes (select, replace, grep) on a char feed, a feed with a separator filter or a longest feed
int32_t bytes_only_refused(const aha_feed *f, const char *what) {
  if (f->chars) {
    tls_err = std::string("feed ") + what + ": a char feed (AHA_FEED_CHARS); " + what + " is in bytes";
    return AHA_E_INVALID;
  }
  if (f->sep) return sep_refused(what);
  if (f->longest) return longest_refused(what);
  if (f->fold) {
    tls_err = std::string("feed ") + what + ": the feed was opened with AHA_FEED_FOLD on a handle folded beyond ASCII, which feed " + what +
              " calls do not take yet (a follow-up: what they keep between calls is derived from hits, and a hit that ends in a "
              "character still open is decided on its unfolded byte); feed match, count and cover calls do";
    return AHA_E_INVALID;
  }
  return AHA_OK;
}

int32_t feed_select_args(const aha_feed *f, const uint64_t *piece_offsets, const uint32_t *seq_ids, uint64_t n_pieces, uint32_t flags,
                         const aha_hit *out, uint64_t cap, const uint64_t *n_selected, bool no_corpus) {
  if (!f || !n_selected || !piece_offsets || (n_pieces && !seq_ids) || (cap && !out) || no_corpus ||
      (flags & ~(AHA_FEED_SELECT_FINAL | AHA_FEED_SELECT_TOKENS | AHA_FEED_SELECT_GAP_RUNS)) ||
      ((flags & AHA_FEED_SELECT_GAP_RUNS) && !(flags & AHA_FEED_SELECT_TOKENS)))
    return AHA_E_INVALID;
  if (bad_feed(f)) return AHA_E_NO_DEVICE;
  return bytes_only_refused(f, "select");
}

int32_t feed_replace_args(const aha_feed *f, const aha_repl *table, const uint64_t *piece_offsets, const uint32_t *seq_ids,
                          uint64_t n_pieces, uint32_t flags, const uint8_t *out, uint64_t cap_bytes, const uint64_t *n_out_bytes) {
  if (!f || !table || !n_out_bytes || !piece_offsets || (n_pieces && !seq_ids) || (cap_bytes && !out) ||
      (flags & ~AHA_FEED_REPLACE_FINAL))
    return AHA_E_INVALID;
  if (bad_feed(f)) return AHA_E_NO_DEVICE;
  if (table->owner != f->ac->serial) {
    tls_err = "the replacement table was made for another handle";
    return AHA_E_INVALID;
  }
  int32_t rc = bytes_only_refused(f, "replace");
  if (rc) return rc;
  if (!table->d_ent) return no_device();
  return AHA_OK;
}

int32_t feed_grep_args(const aha_feed *f, const uint64_t *piece_offsets, const uint32_t *seq_ids, uint64_t n_pieces, uint32_t flags,
                       const uint64_t *kept_recs, const uint64_t *rec_out_offsets, uint64_t cap_recs, const uint8_t *out,
                       uint64_t cap_bytes, const uint64_t *n_kept) {
  if (!f || !n_kept || !piece_offsets || (n_pieces && !seq_ids) || (flags & ~(AHA_GREP_INVERT | AHA_FEED_GREP_FINAL)))
    return AHA_E_INVALID;
  if ((cap_recs && !kept_recs && !rec_out_offsets) || (cap_bytes && !out)) return AHA_E_INVALID;
  if (bad_feed(f)) return AHA_E_NO_DEVICE;
  return bytes_only_refused(f, "grep");
}

// all records of a per-sequence array cleared (seq == UINT32_MAX), or the first `bytes` bytes of one; an array not allocated yet
// has nothing to clear
int32_t clear_seqs(aha_feed *f, void *base, size_t stride, size_t bytes, uint32_t seq) {
  if (!base) return AHA_OK;
  if (seq == UINT32_MAX)
    HIPCHK(f->ac, hipMemsetAsync(base, 0, (size_t)f->n_seqs * stride, f->hs));
  else
    HIPCHK(f->ac, hipMemsetAsync((uint8_t *)base + (size_t)seq * stride, 0, bytes, f->hs));
  return AHA_OK;
}
}  // namespace

int32_t aha_feed_open(aha_ac *ac, uint32_t n_seqs, uint32_t flags, aha_feed **out) {
  return aha_feed_open_params(ac, n_seqs, flags, nullptr, out);
}

int32_t aha_feed_open_params(aha_ac *ac, uint32_t n_seqs, uint32_t flags, const aha_match_params *params, aha_feed **out) {
  if (!ac || !out || n_seqs == 0 || (flags & ~(AHA_FEED_CHARS | AHA_FEED_FOLD))) return AHA_E_INVALID;
  *out = nullptr;
  const bool sep = params && params->sep_size > 0;
  int longest = 0;
  if (params) {
    if (params->sep_size > 256) {
      tls_err = "sep BitArray size > 256 is not supported";
      return AHA_E_SEP_SIZE;
    }
    const bool has_longest = params->struct_size >= offsetof(aha_match_params, longest) + sizeof(int32_t);
    longest = has_longest ? params->longest : 0;
    if (longest < 0 || longest > 2) {
      tls_err = "aha_feed_open_params: longest is 0 (match), 1 (match_longest, intersectable = false) or 2 (intersectable = true)";
      return AHA_E_INVALID;
    }
    if (longest && sep) {
      tls_err = "aha_feed_open_params: match_longest has no separator overload (longest != 0 with sep_size > 0)";
      return AHA_E_INVALID;
    }
    if (longest && params->char_offsets) {
      tls_err = "aha_feed_open_params: a longest feed reports byte offsets (longest != 0 with char_offsets != 0)";
      return AHA_E_INVALID;
    }
    if (longest && (flags & AHA_FEED_CHARS)) {
      tls_err = "aha_feed_open_params: a longest feed on a char feed (AHA_FEED_CHARS) is not supported yet (a follow-up)";
      return AHA_E_INVALID;
    }
    if (params->char_offsets) {
      tls_err = "aha_feed_open_params: the separator filter and longest only; a feed counts in characters with AHA_FEED_CHARS";
      return AHA_E_INVALID;
    }
    if (sep && (flags & AHA_FEED_CHARS)) {
      tls_err = "aha_feed_open_params: a separator filter on a char feed (AHA_FEED_CHARS) is not supported";
      return AHA_E_INVALID;
    }
  }
  // AHA_FEED_FOLD on a handle folded beyond ASCII: a folded feed.  On any other handle the flag changes nothing.
  const int fold = (flags & AHA_FEED_FOLD) && ac->fold_mode() >= 2 ? ac->fold_mode() : 0;
  if (fold && (sep || longest)) {  // (before any device work, host-only handles included)
    tls_err = std::string("aha_feed_open_params: AHA_FEED_FOLD on a handle folded beyond ASCII takes neither ") +
              (sep ? "a separator filter" : "longest != 0") + " yet (a follow-up)";
    return AHA_E_INVALID;
  }
  if (const int mode = ac->fold_mode(); !fold && mode >= 2 && mode <= 4) {  // (before any device work, host-only handles included)
    const char *option = mode == 2 ? "SIMPLE" : mode == 3 ? "BMP" : "KANA";
    tls_err = std::string("aha_feed_open: no feed on a handle compiled with AHA_OPT_FOLD_") + option + " yet: a " +
              (mode == 2 ? "two-byte" : "two- or three-byte") +
              " character may be cut between two calls, and the context a feed keeps would have to carry " +
              (mode == 2 ? "half" : "part") +
              " of it (a follow-up; fold the pieces' sequences whole, or use AHA_OPT_FOLD_ASCII); AHA_FEED_FOLD opens a feed that does, "
              "with Lmax + 1 bytes of context and a character still open at a call's end matched unfolded";
    return AHA_E_INVALID;
  }
  if (ac->device < 0) {
    tls_err = aha_strerror(AHA_E_NO_DEVICE);
    return AHA_E_NO_DEVICE;
  }
  DeviceGuard g(ac->device);
  std::unique_ptr<aha_feed> f(new (std::nothrow) aha_feed());
  if (!f) return AHA_E_NOMEM;
  f->ac = ac;
  f->n_seqs = n_seqs;
  f->W = ac->aut.max_key_len ? ac->aut.max_key_len - 1 : 0;
  f->chars = (flags & AHA_FEED_CHARS) != 0;
  if (sep) {  // a hit that ends on the context's last byte and its left neighbour lie in the context: Lmax + 1 bytes
    f->sep = true;
    f->W = ac->aut.max_key_len + 1;
    for (int c = 0; c < params->sep_size; c++)
      if (!((params->sep_bits[c >> 3] >> (c & 7)) & 1)) f->blocked[c >> 5] |= 1u << (c & 31);
  }
  if (fold) {  // the first two bytes of a window may be folded differently from the sequence's: a hit that touches them must end
               // inside the context, so Lmax + 1 bytes -- what a feed with a separator filter keeps (scan_feedfold.hip)
    f->fold = fold;
    f->W = ac->aut.max_key_len + 1;
  }
  f->longest = longest;
  // (a longest feed carries its state in d_long and never reads a context)
  const size_t ctx_bytes = longest ? 16 : std::max<size_t>(2ull * n_seqs * f->W, 16);
  const size_t long_bytes = (size_t)n_seqs * sizeof(FeedLongSeq);
  int32_t rc = AHA_OK;
  if (hipMalloc((void **)&f->d_seqs, (size_t)n_seqs * sizeof(FeedSeq)) != hipSuccess ||
      hipMalloc((void **)&f->d_ctx, ctx_bytes) != hipSuccess || (longest && hipMalloc((void **)&f->d_long, long_bytes) != hipSuccess) || hipHostMalloc((void **)&f->h_pin, 32) != hipSuccess ||
      hipStreamCreateWithFlags(&f->hs, hipStreamNonBlocking) != hipSuccess) {
    tls_err = "aha_feed_open: device allocation failed";
    rc = AHA_E_HIP;
  } else if (hipMemsetAsync(f->d_seqs, 0, (size_t)n_seqs * sizeof(FeedSeq), f->hs) != hipSuccess ||
             (longest && hipMemsetAsync(f->d_long, 0, long_bytes, f->hs) != hipSuccess) || hipStreamSynchronize(f->hs) != hipSuccess) {
    tls_err = "aha_feed_open: clearing the sequences failed";
    rc = AHA_E_HIP;
  }
  if (rc) {
    aha_feed_free(f.release());
    return rc;
  }
  *out = f.release();
  return AHA_OK;
}

void aha_feed_free(aha_feed *f) {
  if (!f) return;
  {
    std::lock_guard<std::mutex> lk(f->mu);  // (waits for a call in flight)
    DeviceGuard g(f->ac->device);
    for (auto &b : f->buf)
      if (b.p) (void)hipFree(b.p);
    if (f->d_seqs) (void)hipFree(f->d_seqs);
    if (f->d_ctx) (void)hipFree(f->d_ctx);
    if (f->d_sel) (void)hipFree(f->d_sel);
    if (f->d_tail) (void)hipFree(f->d_tail);
    if (f->d_tok) (void)hipFree(f->d_tok);
    if (f->d_grep) (void)hipFree(f->d_grep);
    if (f->d_long) (void)hipFree(f->d_long);
    if (f->h_pin) (void)hipHostFree(f->h_pin);
    if (f->hs) (void)hipStreamDestroy(f->hs);
  }
  delete f;
}

int32_t aha_feed_reset(aha_feed *f, uint32_t seq) {
  if (!f) return AHA_E_INVALID;
  if (seq != UINT32_MAX && seq >= f->n_seqs) return AHA_E_INVALID;
  std::lock_guard<std::mutex> lk(f->mu);
  aha_ac *ac = f->ac;
  DeviceGuard g(ac->device);
  int32_t rc;
  // a sequence of length 0 has an empty context: only the counters are cleared (a stamp of 0 is never a call's)
  if ((rc = clear_seqs(f, f->d_seqs, sizeof(FeedSeq), 2 * sizeof(uint64_t), seq))) return rc;
  // the select state too: a sequence of length 0 has no open hits (its tail is never read) and its cursor is 0
  if ((rc = clear_seqs(f, f->d_sel, sizeof(FeedSelSeq), sizeof(FeedSelSeq), seq))) return rc;
  // ... and the token state: no token is open
  if ((rc = clear_seqs(f, f->d_tok, sizeof(FeedTokSeq), sizeof(FeedTokSeq), seq))) return rc;
  // ... and the grep state: no record is open, none is closed
  if ((rc = clear_seqs(f, f->d_grep, sizeof(FeedGrepSeq), sizeof(FeedGrepSeq), seq))) return rc;
  // ... and a longest feed's carried state: the root, nothing pending
  if ((rc = clear_seqs(f, f->d_long, sizeof(FeedLongSeq), sizeof(FeedLongSeq), seq))) return rc;
  HIPCHK(ac, hipStreamSynchronize(f->hs));
  return AHA_OK;
}

int32_t aha_feed_position(const aha_feed *cf, uint32_t seq, uint64_t *bytes, uint64_t *chars) {
  aha_feed *f = const_cast<aha_feed *>(cf);
  if (!f || seq >= f->n_seqs) return AHA_E_INVALID;
  std::lock_guard<std::mutex> lk(f->mu);
  aha_ac *ac = f->ac;
  DeviceGuard g(ac->device);
  HIPCHK(ac, hipMemcpyAsync(f->h_pin, f->d_seqs + seq, 2 * sizeof(uint64_t), hipMemcpyDeviceToHost, f->hs));
  HIPCHK(ac, hipStreamSynchronize(f->hs));
  if (bytes) *bytes = f->h_pin[0];
  if (chars) *chars = f->h_pin[1];
  return AHA_OK;
}

int32_t aha_feed_match_batch_device(aha_feed *f, const uint8_t *d_corpus, const uint64_t *d_piece_offsets,
                                    const uint32_t *d_seq_ids, uint64_t n_pieces, uint64_t n_bytes, aha_hit *d_out,
                                    uint64_t cap, uint64_t *d_piece_hit_offsets, uint64_t *d_piece_bases, uint64_t *n_hits,
                                    void *stream) {
  int32_t rc = feed_match_args(f, d_piece_offsets, d_seq_ids, n_pieces, d_out, cap, n_hits, n_bytes && !d_corpus);
  if (rc) return rc;
  FeedCall call(f);
  FeedArgs F = feed_args(d_corpus, d_piece_offsets, d_seq_ids, n_pieces, n_bytes, d_piece_hit_offsets, d_piece_bases);
  uint64_t total = 0;
  *n_hits = 0;
  rc = feed_match(f, call.sc(), F, d_out, -1, cap, (hipStream_t)stream, &total);
  if (rc == AHA_OK || rc == AHA_E_CAPACITY) *n_hits = total;
  return rc;
}

int32_t aha_feed_match_batch(aha_feed *f, const uint8_t *corpus, const uint64_t *piece_offsets, const uint32_t *seq_ids,
                             uint64_t n_pieces, aha_hit *out, uint64_t cap, uint64_t *piece_hit_offsets,
                             uint64_t *piece_bases, uint64_t *n_hits) {
  int32_t rc = feed_match_args(f, piece_offsets, seq_ids, n_pieces, out, cap, n_hits, false);
  if (rc) return rc;
  std::optional<FeedCall> call;
  Staged B;
  if ((rc = stage_pieces(f, call, corpus, piece_offsets, seq_ids, n_pieces, {}, B))) return rc;
  const uint64_t D = n_pieces;
  FeedArgs F = feed_args(B.corpus, B.off, B.ids, D, B.n_bytes, B.pho, B.bases);
  uint64_t total = 0;
  *n_hits = 0;
  rc = feed_match(f, call->sc(), F, nullptr, kHOut, cap, f->hs, &total);
  if (rc == AHA_E_CAPACITY) *n_hits = total;
  if (rc) return rc;
  if ((rc = fetch(f, {{out, F.out, total * sizeof(aha_hit)}, {piece_hit_offsets, B.pho, (D + 1) * 8}, {piece_bases, B.bases, D * 8}})))
    return rc;
  *n_hits = total;
  return AHA_OK;
}

int32_t aha_feed_finish_batch_device(aha_feed *f, const uint32_t *d_seq_ids, uint64_t n_named, aha_hit *d_out, uint64_t cap,
                                     uint64_t *d_seq_hit_offsets, uint64_t *d_bases, uint64_t *n_hits, void *stream) {
  int32_t rc = feed_finish_args(f, d_seq_ids, n_named, d_out, cap, n_hits);
  if (rc) return rc;
  FeedCall call(f);
  uint64_t total = 0;
  *n_hits = 0;
  rc = feed_finish(f, call.sc(), d_seq_ids, n_named, d_out, cap, d_seq_hit_offsets, d_bases, (hipStream_t)stream, &total);
  if (rc == AHA_OK || rc == AHA_E_CAPACITY) *n_hits = total;
  return rc;
}

int32_t aha_feed_finish_batch(aha_feed *f, const uint32_t *seq_ids, uint64_t n_named, aha_hit *out, uint64_t cap,
                              uint64_t *seq_hit_offsets, uint64_t *bases, uint64_t *n_hits) {
  int32_t rc = feed_finish_args(f, seq_ids, n_named, out, cap, n_hits);
  if (rc) return rc;
  if ((rc = check_ids_host(f, seq_ids, n_named))) return rc;
  FeedCall call(f);
  aha_ac *ac = f->ac;
  hipStream_t s = f->hs;
  const uint64_t D = n_named;
  // (a sequence ends at most Lmax hits: one per key length)
  const uint64_t cap_d = std::min<uint64_t>(cap, D * std::max<uint64_t>(ac->aut.max_key_len, 1));
  uint32_t *d_ids = (uint32_t *)reserve(f, kHIds, D * 4);
  uint64_t *d_sho = (uint64_t *)reserve(f, kHPho, (D + 1) * 8);
  uint64_t *d_bases = (uint64_t *)reserve(f, kHBases, D * 8);
  aha_hit *d_out = (aha_hit *)reserve(f, kHOut, cap_d * sizeof(aha_hit));
  if (!d_ids || !d_sho || !d_bases || !d_out) return no_memory("staging buffers");
  if (D) HIPCHK(ac, hipMemcpyAsync(d_ids, seq_ids, D * 4, hipMemcpyHostToDevice, s));
  uint64_t total = 0;
  *n_hits = 0;
  rc = feed_finish(f, call.sc(), d_ids, D, d_out, cap_d, d_sho, d_bases, s, &total);
  if (rc == AHA_E_CAPACITY) *n_hits = total;
  if (rc) return rc;
  if ((rc = fetch(f, {{out, d_out, total * sizeof(aha_hit)}, {seq_hit_offsets, d_sho, (D + 1) * 8}, {bases, d_bases, D * 8}}))) return rc;
  *n_hits = total;
  return AHA_OK;
}

int32_t aha_feed_count_batch_device(aha_feed *f, const uint8_t *d_corpus, const uint64_t *d_piece_offsets,
                                    const uint32_t *d_seq_ids, uint64_t n_pieces, uint64_t n_bytes, uint32_t flags,
                                    uint64_t *d_key_counts, uint64_t *d_piece_hit_offsets, uint64_t *d_piece_bases,
                                    uint64_t *n_hits, void *stream) {
  int32_t rc = feed_count_args(f, d_piece_offsets, d_seq_ids, n_pieces, flags, n_hits, n_bytes && !d_corpus);
  if (rc) return rc;
  FeedCall call(f);
  FeedArgs F = feed_args(d_corpus, d_piece_offsets, d_seq_ids, n_pieces, n_bytes, d_piece_hit_offsets, d_piece_bases);
  F.key_counts = d_key_counts;
  F.accumulate = (flags & AHA_COUNT_ACCUMULATE) ? 1u : 0u;
  uint64_t total = 0;
  *n_hits = 0;
  if ((rc = feed_count(f, call.sc(), F, (hipStream_t)stream, &total))) return rc;
  *n_hits = total;
  return AHA_OK;
}

int32_t aha_feed_count_batch(aha_feed *f, const uint8_t *corpus, const uint64_t *piece_offsets, const uint32_t *seq_ids,
                             uint64_t n_pieces, uint32_t flags, uint64_t *key_counts, uint64_t *piece_hit_offsets,
                             uint64_t *piece_bases, uint64_t *n_hits) {
  int32_t rc = feed_count_args(f, piece_offsets, seq_ids, n_pieces, flags, n_hits, false);
  if (rc) return rc;
  std::optional<FeedCall> call;
  Staged B;
  if ((rc = stage_pieces(f, call, corpus, piece_offsets, seq_ids, n_pieces, {}, B))) return rc;
  aha_ac *ac = f->ac;
  hipStream_t s = f->hs;
  const uint64_t D = n_pieces;
  const size_t kc_bytes = (size_t)ac->aut.n_keys * 8;
  uint64_t *d_kc = key_counts ? (uint64_t *)reserve(f, kHKc, kc_bytes) : nullptr;
  if (key_counts && !d_kc) return no_memory("staging buffers");
  // running totals: the caller's vector goes up first and comes back only from a call that succeeded
  if (d_kc && (flags & AHA_COUNT_ACCUMULATE) && kc_bytes)
    HIPCHK(ac, hipMemcpyAsync(d_kc, key_counts, kc_bytes, hipMemcpyHostToDevice, s));
  FeedArgs F = feed_args(B.corpus, B.off, B.ids, D, B.n_bytes, B.pho, B.bases);
  F.key_counts = d_kc;
  F.accumulate = (flags & AHA_COUNT_ACCUMULATE) ? 1u : 0u;
  uint64_t total = 0;
  *n_hits = 0;
  if ((rc = feed_count(f, call->sc(), F, s, &total))) return rc;
  if ((rc = fetch(f, {{key_counts, d_kc, kc_bytes}, {piece_hit_offsets, B.pho, (D + 1) * 8}, {piece_bases, B.bases, D * 8}}))) return rc;
  *n_hits = total;
  return AHA_OK;
}

int32_t aha_feed_cover_batch_device(aha_feed *f, const uint8_t *d_corpus, const uint64_t *d_piece_offsets,
                                    const uint32_t *d_seq_ids, uint64_t n_pieces, uint64_t n_bytes, uint32_t flags,
                                    uint32_t *d_mask, uint8_t *d_redacted, uint8_t fill, uint32_t *d_piece_back,
                                    uint64_t *d_piece_covered, uint64_t *d_piece_hit_offsets, uint64_t *d_piece_bases,
                                    uint64_t *n_covered, uint64_t *n_hits, void *stream) {
  int32_t rc = feed_cover_args(f, d_piece_offsets, d_seq_ids, n_pieces, flags, n_covered, n_bytes && !d_corpus);
  if (rc) return rc;
  FeedCall call(f);
  FeedArgs F = feed_args(d_corpus, d_piece_offsets, d_seq_ids, n_pieces, n_bytes, d_piece_hit_offsets, d_piece_bases);
  F.back = d_piece_back;
  uint64_t total = 0, covered = 0;
  *n_covered = 0;
  if (n_hits) *n_hits = 0;
  if ((rc = feed_cover(f, call.sc(), F, (hipStream_t)stream, d_mask, d_redacted, fill, d_piece_covered, &total, &covered))) return rc;
  *n_covered = covered;
  if (n_hits) *n_hits = total;
  return AHA_OK;
}

// The host entry: the pieces go up into the feed's staging buffers and are redacted in place there; what was asked for comes
// back once the call has succeeded.
int32_t aha_feed_cover_batch(aha_feed *f, const uint8_t *corpus, const uint64_t *piece_offsets, const uint32_t *seq_ids,
                             uint64_t n_pieces, uint32_t flags, uint32_t *mask, uint8_t *redacted, uint8_t fill,
                             uint32_t *piece_back, uint64_t *piece_covered, uint64_t *piece_hit_offsets, uint64_t *piece_bases,
                             uint64_t *n_covered, uint64_t *n_hits) {
  int32_t rc = feed_cover_args(f, piece_offsets, seq_ids, n_pieces, flags, n_covered, false);
  if (rc) return rc;
  std::optional<FeedCall> call;
  Staged B;
  const unsigned want = (piece_back ? kWantBack : 0) | (piece_covered ? kWantCov : 0);
  if ((rc = stage_pieces(f, call, corpus, piece_offsets, seq_ids, n_pieces, {want}, B))) return rc;
  const uint64_t D = n_pieces, n_bytes = B.n_bytes, n_words = (n_bytes + 31) / 32;
  FeedArgs F = feed_args(B.corpus, B.off, B.ids, D, n_bytes, B.pho, B.bases);
  F.back = B.back;
  uint64_t total = 0, covered = 0;
  *n_covered = 0;
  if (n_hits) *n_hits = 0;
  if ((rc = feed_cover(f, call->sc(), F, f->hs, nullptr, redacted ? B.corpus : nullptr, fill, B.cov, &total, &covered))) return rc;
  if ((rc = fetch(f, {{mask, F.mask, n_words * 4}, {redacted, B.corpus, n_bytes}, {piece_back, B.back, D * 4},
                      {piece_covered, B.cov, D * 8}, {piece_hit_offsets, B.pho, (D + 1) * 8}, {piece_bases, B.bases, D * 8}})))
    return rc;
  *n_covered = covered;
  if (n_hits) *n_hits = total;
  return AHA_OK;
}

int32_t aha_feed_select_batch_device(aha_feed *f, const uint8_t *d_corpus, const uint64_t *d_piece_offsets,
                                     const uint32_t *d_seq_ids, uint64_t n_pieces, uint64_t n_bytes, uint32_t flags,
                                     aha_hit *d_out, uint64_t cap, uint64_t *d_piece_sel_offsets, uint64_t *d_piece_bases,
                                     uint32_t *d_piece_hold, uint64_t *n_selected, uint64_t *n_hits, void *stream) {
  int32_t rc = feed_select_args(f, d_piece_offsets, d_seq_ids, n_pieces, flags, d_out, cap, n_selected, n_bytes && !d_corpus);
  if (rc) return rc;
  FeedCall call(f);
  FeedArgs F = feed_args(d_corpus, d_piece_offsets, d_seq_ids, n_pieces, n_bytes, nullptr, d_piece_bases);
  *n_selected = 0;
  if (n_hits) *n_hits = 0;
  auto *run = (flags & AHA_FEED_SELECT_TOKENS) ? feed_tokens : feed_select;
  return run(f, call.sc(), F, flags, d_out, cap, d_piece_sel_offsets, d_piece_hold, (hipStream_t)stream, n_selected, n_hits);
}

int32_t aha_feed_select_batch(aha_feed *f, const uint8_t *corpus, const uint64_t *piece_offsets, const uint32_t *seq_ids,
                              uint64_t n_pieces, uint32_t flags, aha_hit *out, uint64_t cap, uint64_t *piece_sel_offsets,
                              uint64_t *piece_bases, uint32_t *piece_hold, uint64_t *n_selected, uint64_t *n_hits) {
  int32_t rc = feed_select_args(f, piece_offsets, seq_ids, n_pieces, flags, out, cap, n_selected, false);
  if (rc) return rc;
  std::optional<FeedCall> call;
  Staged B;
  if ((rc = stage_pieces(f, call, corpus, piece_offsets, seq_ids, n_pieces, {kWantHold}, B))) return rc;
  const uint64_t D = n_pieces;
  // (the selection is at most the caller's cap, and at most one hit per extended position; a token call adds a carried token
  // per piece)
  aha_hit *d_out = (aha_hit *)reserve(f, kHOut, std::min<uint64_t>(cap, B.n_bytes + D * f->W + D) * sizeof(aha_hit));
  if (!d_out) return no_memory("staging buffers");
  FeedArgs F = feed_args(B.corpus, B.off, B.ids, D, B.n_bytes, nullptr, B.bases);
  *n_selected = 0;
  if (n_hits) *n_hits = 0;
  uint64_t total = 0;
  auto *run = (flags & AHA_FEED_SELECT_TOKENS) ? feed_tokens : feed_select;
  rc = run(f, call->sc(), F, flags, d_out, cap, B.pho, B.hold, f->hs, &total, n_hits);
  if (rc == AHA_E_CAPACITY) *n_selected = total;
  if (rc) return rc;
  if ((rc = fetch(f, {{out, d_out, total * sizeof(aha_hit)}, {piece_sel_offsets, B.pho, (D + 1) * 8}, {piece_bases, B.bases, D * 8},
                      {piece_hold, B.hold, D * 4}})))
    return rc;
  *n_selected = total;
  return AHA_OK;
}

int32_t aha_feed_replace_batch_device(aha_feed *f, const aha_repl *table, const uint8_t *d_corpus, const uint64_t *d_piece_offsets,
                                      const uint32_t *d_seq_ids, uint64_t n_pieces, uint64_t n_bytes, uint32_t flags,
                                      uint8_t *d_out, uint64_t cap_bytes, uint64_t *d_piece_out_offsets, uint64_t *d_piece_bases,
                                      uint32_t *d_piece_hold, uint64_t *n_out_bytes, uint64_t *n_selected, uint64_t *n_hits,
                                      void *stream) {
  int32_t rc = feed_replace_args(f, table, d_piece_offsets, d_seq_ids, n_pieces, flags, d_out, cap_bytes, n_out_bytes);
  if (rc) return rc;
  if (n_bytes && !d_corpus) return AHA_E_INVALID;
  if ((rc = overlap_refused("replace", d_corpus, n_bytes, d_out, cap_bytes))) return rc;
  FeedCall call(f);
  FeedArgs F = feed_args(d_corpus, d_piece_offsets, d_seq_ids, n_pieces, n_bytes, nullptr, d_piece_bases);
  *n_out_bytes = 0;
  if (n_selected) *n_selected = 0;
  if (n_hits) *n_hits = 0;
  return feed_replace(f, call.sc(), table, F, flags, d_out, -1, cap_bytes, d_piece_out_offsets, d_piece_hold, (hipStream_t)stream,
                      n_out_bytes, n_selected, n_hits);
}

// The host entry: the pieces go up into the feed's staging buffers; the result, sized once its total is known, and the offsets
// come back once the call has succeeded.
int32_t aha_feed_replace_batch(aha_feed *f, const aha_repl *table, const uint8_t *corpus, const uint64_t *piece_offsets,
                               const uint32_t *seq_ids, uint64_t n_pieces, uint32_t flags, uint8_t *out, uint64_t cap_bytes,
                               uint64_t *piece_out_offsets, uint64_t *piece_bases, uint32_t *piece_hold, uint64_t *n_out_bytes,
                               uint64_t *n_selected, uint64_t *n_hits) {
  int32_t rc = feed_replace_args(f, table, piece_offsets, seq_ids, n_pieces, flags, out, cap_bytes, n_out_bytes);
  if (rc) return rc;
  std::optional<FeedCall> call;
  Staged B;
  if ((rc = stage_pieces(f, call, corpus, piece_offsets, seq_ids, n_pieces, {kWantHold}, B))) return rc;
  const uint64_t D = n_pieces;
  FeedArgs F = feed_args(B.corpus, B.off, B.ids, D, B.n_bytes, nullptr, B.bases);
  *n_out_bytes = 0;
  if (n_selected) *n_selected = 0;
  if (n_hits) *n_hits = 0;
  uint64_t nb = 0, ns = 0, nh = 0;
  rc = feed_replace(f, call->sc(), table, F, flags, nullptr, kHOut, cap_bytes, B.pho, B.hold, f->hs, &nb, &ns, &nh);
  if (rc == AHA_OK || rc == AHA_E_CAPACITY) {  // (the required size and the counts, as the device entry gives them)
    *n_out_bytes = nb;
    if (n_selected) *n_selected = ns;
    if (n_hits) *n_hits = nh;
  }
  if (rc) return rc;
  return fetch(f, {{out, f->buf[kHOut].p, nb}, {piece_out_offsets, B.pho, (D + 1) * 8}, {piece_bases, B.bases, D * 8},
                   {piece_hold, B.hold, D * 4}});
}

int32_t aha_feed_grep_batch_device(aha_feed *f, const uint8_t *d_corpus, const uint64_t *d_piece_offsets, const uint32_t *d_seq_ids,
                                   uint64_t n_pieces, uint64_t n_bytes, uint8_t delim, uint32_t flags, uint64_t *d_kept_recs,
                                   uint64_t *d_rec_out_offsets, uint64_t cap_recs, uint8_t *d_out, uint64_t cap_bytes,
                                   uint64_t *d_piece_rec_offsets, uint64_t *d_piece_kept_offsets, uint32_t *d_piece_hold,
                                   uint64_t *d_piece_head, uint64_t *d_piece_bases, uint64_t *d_piece_rec_bases, uint64_t *n_recs,
                                   uint64_t *n_kept, uint64_t *n_out_bytes, uint64_t *n_hits, void *stream) {
  int32_t rc = feed_grep_args(f, d_piece_offsets, d_seq_ids, n_pieces, flags, d_kept_recs, d_rec_out_offsets, cap_recs, d_out, cap_bytes,
                              n_kept);
  if (rc) return rc;
  if (n_bytes && !d_corpus) return AHA_E_INVALID;
  if ((rc = overlap_refused("grep", d_corpus, n_bytes, d_out, cap_bytes))) return rc;
  FeedCall call(f);
  FeedArgs F = feed_args(d_corpus, d_piece_offsets, d_seq_ids, n_pieces, n_bytes, nullptr, d_piece_bases);
  GrepOut O;
  O.kept = d_kept_recs;
  O.rec_out = d_rec_out_offsets;
  O.out = d_out;
  O.cap_recs = cap_recs;
  O.cap_bytes = cap_bytes;
  O.piece_rec = d_piece_rec_offsets;
  O.piece_kept = d_piece_kept_offsets;
  O.hold = d_piece_hold;
  O.head = d_piece_head;
  O.rec_bases = d_piece_rec_bases;
  if (n_recs) *n_recs = 0;
  *n_kept = 0;
  if (n_out_bytes) *n_out_bytes = 0;
  if (n_hits) *n_hits = 0;
  return feed_grep(f, call.sc(), F, delim, flags, O, (hipStream_t)stream, n_recs, n_kept, n_out_bytes, n_hits);
}

// The host entry: the pieces go up into the feed's staging buffers; the kept fragments, their offsets and their bytes, sized
// once the totals are known, and the per-piece arrays come back once the call has succeeded.
int32_t aha_feed_grep_batch(aha_feed *f, const uint8_t *corpus, const uint64_t *piece_offsets, const uint32_t *seq_ids,
                            uint64_t n_pieces, uint8_t delim, uint32_t flags, uint64_t *kept_recs, uint64_t *rec_out_offsets,
                            uint64_t cap_recs, uint8_t *out, uint64_t cap_bytes, uint64_t *piece_rec_offsets,
                            uint64_t *piece_kept_offsets, uint32_t *piece_hold, uint64_t *piece_head, uint64_t *piece_bases,
                            uint64_t *piece_rec_bases, uint64_t *n_recs, uint64_t *n_kept, uint64_t *n_out_bytes, uint64_t *n_hits) {
  int32_t rc = feed_grep_args(f, piece_offsets, seq_ids, n_pieces, flags, kept_recs, rec_out_offsets, cap_recs, out, cap_bytes, n_kept);
  if (rc) return rc;
  std::optional<FeedCall> call;
  Staged B;
  if ((rc = stage_pieces(f, call, corpus, piece_offsets, seq_ids, n_pieces, {kWantHold | kWantGrep, out, cap_bytes}, B))) return rc;
  const uint64_t D = n_pieces;
  FeedArgs F = feed_args(B.corpus, B.off, B.ids, D, B.n_bytes, nullptr, B.bases);
  GrepOut O;
  if (kept_recs) O.kept_slot = kHKept;
  if (rec_out_offsets) O.rec_out_slot = kHRecOut;
  if (out) O.out_slot = kHOut;
  O.cap_recs = cap_recs;
  O.cap_bytes = cap_bytes;
  O.piece_rec = B.piece_rec;
  O.piece_kept = B.piece_kept;
  O.hold = B.hold;
  O.head = B.head;
  O.rec_bases = B.rec_bases;
  if (n_recs) *n_recs = 0;
  *n_kept = 0;
  if (n_out_bytes) *n_out_bytes = 0;
  if (n_hits) *n_hits = 0;
  uint64_t nr = 0, nk = 0, nb = 0, nh = 0;
  rc = feed_grep(f, call->sc(), F, delim, flags, O, f->hs, &nr, &nk, &nb, &nh);
  if (rc == AHA_OK || rc == AHA_E_CAPACITY) {  // (both required numbers and the counts, as the device entry gives them)
    if (n_recs) *n_recs = nr;
    *n_kept = nk;
    if (n_out_bytes) *n_out_bytes = nb;
    if (n_hits) *n_hits = nh;
  }
  if (rc) return rc;
  return fetch(f, {{kept_recs, O.kept, nk * 8}, {rec_out_offsets, O.rec_out, (nk + 1) * 8}, {out, O.out, nb},
                   {piece_rec_offsets, B.piece_rec, (D + 1) * 8}, {piece_kept_offsets, B.piece_kept, (D + 1) * 8},
                   {piece_hold, B.hold, D * 4}, {piece_head, B.head, D * 8}, {piece_bases, B.bases, D * 8},
                   {piece_rec_bases, B.rec_bases, D * 8}});
}

