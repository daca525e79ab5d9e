// feed.hpp -- what feed.cpp (the feed entry points of the C ABI) and its kernels (scan_feed.hip, scan_feedselect.hip,
// scan_feedreplace.hip, scan_feedsep.hip, scan_feedgrep.hip, scan_feedlongest.hip, scan_feedfold.hip, scan_feedtokens.hip) share.
// Library-internal.
#pragma once
#include <cstdint>

namespace aha {
struct DevAut;
struct MatchArgs;
// one open sequence of a feed, on the device (24 bytes)
struct FeedSeq {
  unsigned long long bytes;  // bytes consumed since open / reset
  unsigned long long chars;  // lead bytes among them (char feeds)
  uint32_t stamp;            // the last call that named the sequence (kfd_check: duplicates within a call)
  uint32_t bank;             // which of the two context banks holds its last min(W, bytes) bytes
};

// what a feed keeps per sequence for select and replace calls (aha_feed_select_batch*, aha_feed_replace_batch*), allocated by
// the feed's first one (16 bytes)
struct FeedSelSeq {
  unsigned long long seen;    // bytes that went through select or replace calls since open / reset / a FINAL call
  unsigned long long cursor;  // c: everything in front of it is final -- inside a reported hit or in no selected hit ever
};

// what a feed keeps per sequence for token calls (aha_feed_select_batch* with AHA_FEED_SELECT_TOKENS), allocated by the feed's
// first one (16 bytes).  A token call is a select call too: it keeps the select state as a select call does
struct FeedTokSeq {
  unsigned long long seen;  // bytes that went through token calls since open / reset / a FINAL call
  unsigned long long t;     // the token cursor, t <= c: everything in front of it has been reported as tokens
};

// what a feed keeps per sequence for grep calls (aha_feed_grep_batch*), allocated by the feed's first one (32 bytes).  The
// record that is open -- its delimiter has not arrived -- is the last open_len bytes of the sequence; the caller holds them.
struct FeedGrepSeq {
  unsigned long long seen;      // bytes that went through grep calls since open / reset / a FINAL call
  unsigned long long open_len;  // bytes of the open record
  unsigned long long recs;      // records closed so far
  uint32_t open_hit;            // the open record, matched as its own document, has a hit already
  uint32_t pad;
};

// what a longest feed (aha_feed_open_params with longest = 1 | 2; scan_feedlongest.hip) carries per sequence across calls: the
// whole state of match_longest_'s loop at the sequence's current end (16 bytes).  All zero: a sequence of length 0.
struct FeedLongSeq {
  uint32_t state;  // 0: the root; else B + 1, B the state in the numbering of the handle's match_longest image (kValueNode included)
  uint32_t back;   // the pending end lies `back` bytes in front of the sequence's current end (1: its last byte); 0: none
  uint32_t key;    // its key (kNoKey: it yields nothing)
  uint32_t prev;   // the sequence's last byte | the one before << 8, as the kernels saw them (folded on a folded handle)
};

// the arguments every feed kernel takes (by value)
struct FeedArgs {
  const uint8_t *text;         // the caller's pieces
  const uint64_t *off;         // [D+1] piece offsets
  const uint32_t *ids;         // [D] sequence ids
  uint64_t D, n_bytes, n_seqs;
  uint32_t W;                  // max(Lmax - 1, 0); Lmax + 1 on a feed with a separator filter and on a folded feed (AHA_FEED_FOLD)
  uint32_t Wp;                 // bytes of the piece in the head windows X and P': W, or 2 W for a cover call
  uint32_t stamp;              // this call's stamp (never 0)
  uint64_t max_piece;          // a piece must be shorter than this
  int32_t chars;
  FeedSeq *seqs;               // [n_seqs]
  uint8_t *ctx;                // [2][n_seqs][W]
  uint32_t *verdict;           // [1]: bit 0 invalid offsets or ids, bit 1 a piece too long, bit 2 / 3 / 4 the select / grep / token
                               // state is behind
  uint64_t *win_total;         // [1]: bytes of the window batch
  uint8_t *win;                // the window batch [X_0..X_{D-1} | ctx_0.. | P'_0..]
  uint64_t *woff;              // [3D+1] its document offsets
  const uint64_t *wdho;        // [3D+1] its per-document hit offsets
  const int32_t *whits;        // its hits (3 words each)
  const uint64_t *mdho;        // [D+1] the main pass's per-document hit offsets
  const int32_t *mhits;        // its hits
  uint64_t *lead_ctx;          // [D] leads(ctx_d) (char feeds)
  unsigned long long *lead_p;  // [D] leads(P_d) (char feeds)
  uint64_t *pho;               // [D+1] hits per piece, scanned (the caller's piece_hit_offsets or feed scratch)
  uint64_t *bases;             // [D] the sequence's length before the piece, or null
  int32_t *out;                // the caller's hits
  uint64_t total;              // hits of the call
  // count calls (aha_feed_count_batch*)
  uint64_t n_whits;            // hits of the window batch: [0, wdho[D]) count +1, the rest -1
  uint32_t K;                  // keys
  uint32_t accumulate;         // kfd_count_finish adds into key_counts instead of copying
  unsigned long long *kc;      // [K] the feed's per-key sums: the main pass's, then the window hits added
  uint64_t *key_counts;        // [K] the caller's, or null
  // cover calls (aha_feed_cover_batch*): the head windows are X2 = ctx || P[0 .. min(2 W, |P|)) and P'2 = P[0 .. min(2 W, |P|))
  uint32_t *mask;              // bit j = byte j of the batch: the main pass's cover of the pieces, then corrected at the cuts
  uint32_t *back;              // [D] bytes in front of the piece inside a hit that ends in it, or null (cleared by the host)
  // select calls (aha_feed_select_batch*): kfd_check refuses a sequence whose bytes did not all go through select calls
  const FeedSelSeq *sel;       // [n_seqs], or null (every other call); verdict bit 2
  // token calls: kfd_check also refuses a sequence of length > 0 whose bytes did not all go through token calls
  const FeedTokSeq *tok;       // [n_seqs], or null (every other call); verdict bit 4
  // calls on a feed with a separator filter (aha_feed_open_params; scan_feedsep.hip): the call's true hits also hold the hits
  // that end on the context's last byte -- the last edge[d] hits of ctx_d alone
  uint64_t *edge;              // [D], or null (every call on a plain feed)
  // grep calls (aha_feed_grep_batch*): kfd_check refuses a sequence whose bytes did not all go through grep calls
  const FeedGrepSeq *grep;     // [n_seqs], or null (every other call); verdict bit 3
  // calls on a folded feed (AHA_FEED_FOLD on a handle folded beyond ASCII; scan_feedfold.hip): the pieces as the engines take
  // them, every piece folded as the end of its sequence.  `text` stays the caller's: the new contexts, leads(P) and a cover
  // call's redaction read it
  uint8_t *ftext;              // [n_bytes] in the feed's scratch, or null (every call on another feed)
};

// what the kernels of a grep call take beside FeedArgs (scan_feedgrep.hip).  The pieces are split into R fragments as a records
// call splits documents; the window batch is [X_0.. | Y_0.. | Z_0..] at F.win / F.woff with the hit offsets F.wdho.
struct FeedGrepArgs {
  FeedGrepSeq *gseq;           // [n_seqs]
  uint32_t delim, invert, final;
  uint64_t R;
  const uint64_t *frag;        // [R+1] the fragments' offsets into the pieces' bytes
  const uint64_t *pro;         // [D+1] the pieces' offsets into the fragments (piece_rec_offsets)
  const uint64_t *fdho;        // [R+1] the fragments' hit offsets, each matched from the root
  uint8_t *flag;               // [R] bit 0 keep, bit 1 has, bit 2 closed
  uint32_t *keep, *S, *T;      // ceil(R / 32) words each (scan_grep.hip kgr_flag's masks)
  uint32_t *hold;              // [D] the caller's piece_hold, or null
  uint64_t *head;              // [D] the caller's piece_head, or null
  uint64_t *rec_bases;         // [D] the caller's piece_rec_bases, or null
};

// what the kernels of a call on a feed with a separator filter take beside FeedArgs (scan_feedsep.hip).  The call's true hits
// are those of the sequence with an end in [n0, n1], relative to the piece (end = 0: the hit ended with the piece before); a
// finish call's are the hits of the named sequences' contexts alone (the X block of a window batch of empty pieces).
struct FeedSepArgs {
  const int32_t *hits;         // the true hits, piece by piece (kfd_merge into scratch; a finish call: the window hits)
  const uint64_t *tho;         // [D+1] where each piece's lie
  uint64_t n_true;
  uint32_t blocked[8];         // bit c: byte c does not pass (c < sep_size && !sep[c])
  uint32_t fold;               // the handle folds (AHA_OPT_FOLD_ASCII): the neighbours are folded before the test
  unsigned long long *keep;    // one bit per true hit: it survives and its end lies in [n0, n1) (a finish call: end = n)
  unsigned long long *blk;     // the rank blocks of the keep mask (scan_select.hip)
  int32_t *out;                // the caller's hits
  uint64_t *bases;             // a finish call: [D] the sequences' lengths, or null
};

// what the kernels of a select call take beside FeedArgs (scan_feedselect.hip).  The extended positions of piece d are
// [eoff[d], eoff[d+1]): the last W'_d = min(W, n0[d]) bytes in front of the piece, then the piece.
struct FeedSelArgs {
  FeedSelSeq *sseq;            // [n_seqs]
  unsigned long long *tail;    // [n_seqs][W]: entry j = the longest known hit (len << 32 | value) that starts at byte seen - W + j
  uint32_t final;              // AHA_FEED_SELECT_FINAL
  uint64_t *eoff;              // [D+1]
  uint64_t *n0;                // [D] the sequence's length before the piece
  uint64_t NE;                 // eoff[D]
  const int32_t *hits;         // the call's true hits, piece by piece, relative to the piece (kfd_merge into scratch)
  const uint64_t *pho;         // [D+1] where each piece's lie
  uint64_t n_hits;
  unsigned long long *L;       // [NE]
  uint32_t *cover, *start, *select;  // NE bits each
  unsigned long long *blk;     // the rank blocks of the select mask (scan_select.hip)
  unsigned long long *cend;    // [D] the end of the piece's last selected hit as an extended position, 0: none
  uint64_t *pso;               // [D+1] the pieces' offsets into the selection (scratch until the call is known to succeed)
  uint32_t *hold;              // [D] the caller's piece_hold, or null
  int32_t *out;                // the caller's hits
  FeedTokSeq *tseq;            // [n_seqs] the token state, or null (no token call yet): a FINAL call clears the sequence's
};

// what a token call keeps per piece between its passes (32 bytes; scan_feedtokens.hip)
constexpr uint32_t kFeedTokCarried = 1u;  // t0 < c0: the piece's tokens begin with the open token carried in
constexpr uint32_t kFeedTokOpen = 2u;     // the last token of T[t0 .. c1) stays open: it is not reported
struct FeedTokPiece {
  unsigned long long t0, t1;  // the token cursor the call finds and leaves
  uint32_t c0, c1;            // the select cursor the call finds and leaves, as extended positions of the piece
  uint32_t flags;             // kFeedTokCarried | kFeedTokOpen
  uint32_t count;             // tokens the call reports for the piece
};

// what the kernels of a token call take beside FeedArgs and FeedSelArgs (scan_feedtokens.hip)
struct FeedTokArgs {
  FeedTokSeq *tseq;            // [n_seqs]
  uint32_t gap_runs;           // AHA_FEED_SELECT_GAP_RUNS
  uint64_t bound;              // a non-final call may leave at most this many bytes behind the token cursor (AHA_FEED_TOKEN_OPEN)
  FeedTokPiece *piece;         // [D]
  uint32_t *inside, *starts;   // S and T of scan_tokens.hip: ceil(NE / 32) whole words each; S clear
  unsigned long long *blk;     // the rank blocks of T
  uint64_t *raw;               // [D+1] the starts in front of every piece's extended positions
  uint64_t *pto;               // [D+1] the pieces' offsets into the tokens (scratch until the call is known to succeed)
  uint64_t *total;             // [1] pto[D]
  uint32_t *verdict;           // [1] bit 0: a token would stay open beyond the bound
  uint32_t *hold;              // [D] the caller's piece_hold, or null
  int32_t *out;                // the caller's tokens
};

// what the kernels of a replace call take beside FeedArgs and FeedSelArgs (scan_feedreplace.hip).  Piece d stages
// T[c0 .. c1) of its sequence -- c0 the cursor the call finds, c1 the one it leaves -- at ext[ext_off[d], ext_off[d+1]): the
// last hold0[d] = n0 - c0 bytes in front of the piece (from the sequence's context), then the piece up to c1.
struct FeedRepArgs {
  uint32_t *hold0;    // [D]
  uint64_t *ext_off;  // [D+1] the exclusive scan of c1 - c0
  uint64_t *bias;     // [D+1] ext_off[d] + hold0[d]: where the piece's own first byte lies, so a row's start (relative to the
                      // piece, possibly negative) is a staged position by one addition (krp_delta's document offsets)
  uint8_t *ext;       // the staged text, at most n_bytes + D W bytes
};

// what the kernels of a call on a longest feed take beside FeedArgs (scan_feedlongest.hip); the two-pass scratch (counts, block
// sums, totals) is the batch match_longest's (MatchArgs)
struct FeedLongArgs {
  FeedLongSeq *lseq;      // [n_seqs] the carried states
  FeedLongSeq *end;       // [D] scratch: the state at every non-empty piece's end (pass 1 writes it, kfl_commit moves it)
  uint64_t *sho;          // a finish call: [D + 1] the named sequences' hit offsets, or null
};

#ifdef __HIP__
// The cursor a select or replace call leaves behind piece d (kfs_commit stores it, kfr_layout sizes the staged text by it):
// everything in front of it is final.  cursor: the one the call finds; wb = min(W, n0); cend: the end of the last hit the call
// settles as an extended position (0: none); under FINAL everything settles.
__device__ inline uint64_t feedsel_cursor(uint64_t cursor, uint64_t n0, uint64_t wb, uint64_t cend, uint64_t n1, uint64_t W,
                                      uint32_t final) {
  if (final) return n1;
  const uint64_t front = n1 > W ? n1 - W : 0, last = n0 - wb + cend;
  const uint64_t c = cursor > last ? cursor : last;
  return c > front ? c : front;
}
#endif

void feed_launch_check(const FeedArgs &F, void *stream);    // kfd_check, then kfd_scan of the window lengths
void feed_launch_check_only(const FeedArgs &F, void *stream);  // kfd_check alone (a grep call lays out windows of its own)
void feed_launch_windows(const FeedArgs &F, void *stream);  // kfd_windows (+ kfd_leads on char feeds)
void feed_launch_leads(const FeedArgs &F, void *stream);    // kfd_leads alone, on char feeds (a folded feed cuts its own windows)
// a folded feed (scan_feedfold.hip; mode: the handle's fold, 2 simple, 3 BMP, 4 kana): kff_heads -- the first two bytes of every
// piece of F.ftext, behind the staged copy's fix-up -- and kff_windows in kfd_windows' place
void feedfold_launch_heads(const FeedArgs &F, int mode, void *stream);
void feedfold_launch_windows(const FeedArgs &F, int mode, void *stream);
void feed_launch_merge(const FeedArgs &F, void *stream);    // kfd_scan of the hits per piece, kfd_merge
void feed_launch_commit(const FeedArgs &F, void *stream);   // kfd_commit: bases, counters, the new contexts
// a feed with a separator filter: kfd_edge (F.edge) and kfd_scan of the true hits per piece into F.pho; then, with F.total read
// back from F.pho[D], kfd_merge of the true hits, the edge hits in front of every piece's
void feed_launch_edge(const FeedArgs &F, void *stream);
void feed_launch_merge_edge(const FeedArgs &F, void *stream);
// count calls: kfd_count_windows (F.kc), kfd_scan of the hits per piece, kfd_count_finish (F.key_counts)
void feed_launch_count(const FeedArgs &F, void *stream);
// cover calls: kfd_cover_clear (the first min(W, |P|) bits of every piece), kfd_cover_windows (the spans of the X2 hits that
// end in the piece, F.back), kfd_scan of the hits per piece
void feed_launch_cover(const FeedArgs &F, void *stream);
// select calls (scan_feedselect.hip), in this order; masks, L and cend clear before feedsel_launch_longest
void feedsel_launch_layout(const FeedArgs &F, const FeedSelArgs &S, void *stream);   // eoff, n0 (after the check)
void feedsel_launch_longest(const FeedArgs &F, const FeedSelArgs &S, uint32_t max_blocks, void *stream);  // L: the tails, then the hits
void feedsel_launch_walk(const FeedArgs &F, const FeedSelArgs &S, uint32_t max_blocks, void *stream);     // select, cend
void feedsel_launch_emit(const FeedArgs &F, const FeedSelArgs &S, uint32_t max_blocks, void *stream);     // out
void feedsel_launch_commit(const FeedArgs &F, const FeedSelArgs &S, void *stream);   // behind feed_launch_commit: tails, cursors, hold
// token calls (scan_feedtokens.hip), in this order behind feed_select_settle; the spans between bounds and starts are
// tokens_launch_spans (scan_tokens.hip), the ranks between starts and edge select_launch_rank and select_launch_rank_docs
void feedtok_launch_bounds(const FeedArgs &F, const FeedSelArgs &S, const FeedTokArgs &K, uint32_t max_blocks, void *stream);  // piece
void feedtok_launch_starts(const FeedArgs &F, const FeedSelArgs &S, const FeedTokArgs &K, uint32_t max_blocks, void *stream);  // T
// t1, the counts, the verdict (kft_edge); pto and the total (kft_offsets)
void feedtok_launch_edge(const FeedArgs &F, const FeedSelArgs &S, const FeedTokArgs &K, uint32_t max_blocks, void *stream);
void feedtok_launch_emit(const FeedArgs &F, const FeedSelArgs &S, const FeedTokArgs &K, uint32_t max_blocks, void *stream);  // out
// behind feedsel_launch_commit: the token state, hold
void feedtok_launch_commit(const FeedArgs &F, const FeedSelArgs &S, const FeedTokArgs &K, uint32_t max_blocks, void *stream);
// replace calls (scan_feedreplace.hip): behind the walk and kfs_emit into scratch, in front of both commits
void feedrep_launch_layout(const FeedArgs &F, const FeedSelArgs &S, const FeedRepArgs &R, void *stream);  // hold0, ext_off, bias
// ext; max_bytes: a bound of ext_off[D] known to the host (it sizes the grid)
void feedrep_launch_stage(const FeedArgs &F, const FeedRepArgs &R, uint64_t max_bytes, uint32_t max_blocks, void *stream);
// calls on a feed with a separator filter (scan_feedsep.hip), in this order; the rank between flag and compact is
// select_launch_rank, the filtered offsets select_launch_rank_docs (scan_select.hip)
void feedsep_launch_flag(const FeedArgs &F, const FeedSepArgs &P, uint32_t max_blocks, void *stream);         // keep
void feedsep_launch_flag_finish(const FeedArgs &F, const FeedSepArgs &P, uint32_t max_blocks, void *stream);  // keep (a finish call)
void feedsep_launch_compact(const FeedSepArgs &P, bool finish, uint32_t max_blocks, void *stream);            // out
void feedsep_launch_count(const FeedArgs &F, const FeedSepArgs &P, uint32_t max_blocks, void *stream);  // F.kc (cleared by the host)
void feedsep_launch_count_finish(const FeedArgs &F, uint32_t max_blocks, void *stream);                 // F.key_counts
// grep calls (scan_feedgrep.hip), in this order; the ranks between flag and commit are select_launch_rank, the runs, the kept
// fragments and the copy scan_grep.hip's and scan_replace.hip's
void feedgrep_launch_layout(const FeedArgs &F, const FeedGrepArgs &G, void *stream);  // F.woff, F.win_total (after the check and the fragments)
void feedgrep_launch_windows(const FeedArgs &F, const FeedGrepArgs &G, void *stream);  // F.win
void feedgrep_launch_flag(const FeedArgs &F, const FeedGrepArgs &G, uint32_t max_blocks, void *stream);  // flag, then keep, S, T
void feedgrep_launch_commit(const FeedArgs &F, const FeedGrepArgs &G, uint32_t max_blocks, void *stream);  // behind feed_launch_commit
void feedsep_launch_restart(const FeedArgs &F, const FeedSepArgs &P, void *stream);  // a finish call: bases, the sequences at length 0
// calls on a longest feed (scan_feedlongest.hip): kfl_commit behind pass 2 -- bases, lengths, the carried states; a finish call
// is kfl_finish twice: the pending hits counted (F.pho: the exclusive scan, F.pho[D] the total; one workgroup strides the ids),
// then written, with the bases, and the sequences restarted
// the walk: kfl_pieces (a thread per piece: exact for both modes) or kfl_chunks (intersectable only: a thread per chunk of
// M.chunk bytes); write = false counts (M.counts, M.blk_hits) and leaves L.end, true writes M.out and M.doc_hit_off
void feedlong_launch_walk(const DevAut &A, const MatchArgs &M, const FeedArgs &F, const FeedLongArgs &L, bool chunks, bool intersectable,
                          bool write, void *stream);
void feedlong_launch_commit(const FeedArgs &F, const FeedLongArgs &L, void *stream);
void feedlong_launch_finish(const FeedArgs &F, const FeedLongArgs &L, const void *key_ln, bool write, void *stream);
}  // namespace aha
