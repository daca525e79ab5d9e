/*
 * aha_hip.h -- C ABI of libaha_hip.so: MI355X-native Aha::AC#match.
 *
 * Drop-in boundary for ONE path of chenkovsky/aha: batch Aho-Corasick
 * traversal (Aha::AC.compile / #match / Aha::Hit).  The reference has no FFI
 * of its own (pure Crystal); these entry points are what a Crystal
 * `lib LibAhaHip` binding calls (bindings/crystal/aha_hip.cr).
 * Citations are file:line relative to the reference repository root.
 *
 * Conventions: extern "C", plain pointers and sizes, no exceptions across the
 * boundary.  Every function returns an int32 status (AHA_OK = 0, <0 error)
 * unless stated.  The caller owns every buffer it passes; the library never
 * retains caller pointers past return.  The AUTOMATON of a handle is immutable after compile and which pipeline a
 * match call takes is a function of that call alone (its size, its params and its `cap`), never of earlier calls.
 * What a handle does keep between calls is grow-only device scratch (aha_ac_release_scratch frees it,
 * aha_ac_scratch_bytes reports it), organised in sets: a match call leases one set for its duration, so concurrent
 * calls on one handle (one host thread and one stream each) run side by side on up to 8 sets and only then wait.
 * aha_last_error returns the text of the calling thread's last failure.
 *
 * Device scratch of one match call on N input bytes with output capacity `cap` hits (single-traversal engine): the
 * event records.  Region pipeline: 8 bytes each, per chunk (N / 2^18 bytes, at least 192) twice the average the
 * capacity allows for plus 1/64 of the chunk, i.e. 16 bytes per hit of capacity + N/8.  Slab pipeline (capacity
 * below 16 hits per chunk, or a separator filter): 41 bytes per hit of capacity + 80 MB.  One event per input byte
 * (8 N bytes, bounded at 48 GiB) only when `cap` announces more than one hit per 4 input bytes or a chunk
 * overflowed its region (aha_timing.repeats then says that the call ran twice).  Plus ~24 bytes per chunk and 4 bytes per
 * document.  A device corpus that is not 16-byte aligned is first copied into scratch (N bytes).
 * A handle compiled with AHA_OPT_FOLD_ASCII: every engine but the prefix filter reads a folded copy of the batch in scratch
 * (N bytes, aligned or not: the same pass as that copy, not a second one); the prefix-filter engine holds nothing extra.
 * Character-level engine (aha_ac_info_t.unit_enabled; aha_timing.engine = 4): its records are 12 bytes and go straight to
 * the expansion -- 24 bytes per hit of capacity + 3N/16 with the fused expansion (output chains of at most 15 keys), + the
 * 8-byte regions above with the general post passes.
 * Prefix-filter engine (aha_ac_info_t.filter_prefix_bytes; aha_timing.engine = 5): the region pipeline's records in chunks
 * of 4 .. 32 KiB (16 bytes per hit of capacity + N/8 as above) + one bit per input byte (N/8) + 16 bytes per chunk.
 * A count call (aha_ac_count_batch*) has no capacity and holds nothing per hit: the full-size regions of its engine (one
 * record per input byte: 8 N bytes, 12 N with the fused character-level expansion, 20 N with its general passes) + 8 bytes
 * per key (the events per head key) + the per-chunk and per-document words above.  Where those regions are beyond the 48 GiB
 * bound or cannot be allocated, the call counts ranges of whole documents one after another (halved until they fit: the
 * regions of one range + its offsets; aha_timing.repeats = the ranges before the last); only a single document whose regions
 * do not fit goes to the two-pass engine.  With a separator filter, or where a match would take the two-pass engine, it
 * takes that engine's counting pass: ~24 bytes per chunk of 256+ bytes, 8 per document.
 */
#ifndef AHA_HIP_H
#define AHA_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif
/* The library is built with -fvisibility=hidden: what this header declares is all it exports. */
#if defined(__GNUC__)
#pragma GCC visibility push(default)
#endif

#define AHA_ABI_VERSION 8

/* Aha::Hit -- src/aha/matcher.cr:2-11.  Half-open [start,end) offsets
 * relative to the start of the sequence (document); value = key index in
 * compile order (src/aha/ac.cr:64-67). */
typedef struct {
  int32_t start, end, value;
} aha_hit;

typedef struct aha_ac aha_ac;

enum {
  AHA_OK = 0,
  AHA_E_INVALID = -1,     /* bad argument */
  AHA_E_EMPTY_KEY = -2,   /* raise "Cannot insert empty key"        src/aha/cedar.cr:756 */
  AHA_E_ZERO_BYTE = -3,   /* raise "key[pos] is zero"               src/aha/cedar.cr:235 */
  AHA_E_DUP_KEY = -4,     /* raise "key:... appear twice."          src/aha/ac.cr:66     */
  AHA_E_SEP_SIZE = -5,    /* raise "sep BitArray size > 256 ..."    src/aha/ac.cr:322    */
  AHA_E_CAPACITY = -6,    /* out buffer too small; *n_hits = required count */
  AHA_E_NO_DEVICE = -7,   /* no usable HIP device: the product path has NO CPU fallback */
  AHA_E_HIP = -8,         /* a HIP runtime call failed; see aha_last_error */
  AHA_E_TOO_LONG = -9,    /* a sequence is >= 2^31 bytes (Int32 offsets, src/aha/matcher.cr:3-5) */
  AHA_E_NOT_FOUND = -10,  /* key / id lookup miss (IndexError in the reference, src/aha/cedar.cr:830-834) */
  AHA_E_TOO_LARGE = -11,  /* automaton exceeds the device image limits */
  AHA_E_NOMEM = -12       /* host memory exhausted (no exception crosses the boundary) */
};

/* Compile-time options.  Zero-initialise and set struct_size. */
typedef struct {
  uint32_t struct_size;
  int32_t device;        /* HIP device ordinal; -1 = current device */
  uint32_t flags;        /* AHA_OPT_* */
  uint32_t reserved;
} aha_options;

#define AHA_OPT_HOST_ONLY 1u /* build the automaton image but do not touch the GPU (tests of host logic) */
#define AHA_OPT_FORCE_WIDE 2u /* always use the 8-byte slot format (default: compact 4-byte when it fits) */
/* ASCII case-insensitive handle (a pure addition to ABI 8).  fold(b) = b + 32 for 0x41 <= b <= 0x5A ('A' .. 'Z'), b
 * otherwise: bytes >= 0x80, '@', '[', '`' and '{' are untouched, lengths and UTF-8 lead bytes never change, so byte and char
 * offsets are those of the original text.  THE RULE: every call on a handle compiled with the flag gives, bit for bit, what
 * the same call gives on an ordinary handle compiled from fold(keys) and run over fold(text) -- match, match_longest in both
 * modes, a separator filter, char offsets, counts, document counts, cover, feeds and feed counts, the pack / unpack exchange,
 * groups, replicate and export.  Exactly three exceptions:
 *   1. redacted[j] is `fill` where the mask bit is set and the ORIGINAL corpus[j] elsewhere, not the folded byte; redaction
 *      in place (d_redacted == d_corpus) writes the fill bytes only.
 *   2. aha_ac_key(id) and aha_ac_save give the keys as the caller spelled them; aha_ac_id(key) folds its argument first.
 *   3. No device entry ever writes the caller's d_corpus, apart from the fill bytes of exception 1.
 * What the rule means in detail: two keys equal after folding are AHA_E_DUP_KEY, *err_key = the index of the second (where
 * the reference would raise on the folded list); a separator filter tests the FOLDED neighbour bytes (clear a letter's
 * lower-case bit to make it a non-separator); the stale END flags of match_longest come from the Cedar replay of the folded
 * keys; the engine choice (unit image, prefix filter, wide or compact) is the one the folded key set would get.
 * aha_ac_load stores nothing new (container format 1): pass the flag in `opts` again, as for AHA_OPT_FORCE_WIDE.
 * aha_ac_replicate copies the flag; aha_group_compile takes it in `flags` and every shard gets it; a feed opened on a folded
 * handle is folded (a straddling hit matches whatever the case of the bytes on either side of the cut).  aha_ac_flags reads it.
 * Cost: the prefix-filter engine folds inside its own text loads (no copy, no extra scratch); every other engine reads a
 * folded copy made by one streaming pass into scratch (N bytes; aha_amd/csrc/scan_fold.hip). */
#define AHA_OPT_FOLD_ASCII 4u
/* Simple case folding for the characters UTF-8 writes in two bytes (a pure addition to ABI 8; implies AHA_OPT_FOLD_ASCII:
 * 4u | 8u means what 8u means, and aha_ac_flags reports the bits as they were passed).  fold2(buf) is a byte-to-byte map of
 * one buffer, as long as its input: at every j with buf[j] in 0xC2 .. 0xDF, j + 1 < len and buf[j + 1] in 0x80 .. 0xBF the
 * pair -- the UTF-8 of a code point cp in U+0080 .. U+07FF -- becomes the UTF-8 of F(cp); such pairs cannot overlap; every
 * other byte gets the ASCII fold above.  A rule on bytes, not on well-formed text: stray continuation bytes, a lead byte at
 * the end, three- and four-byte sequences, 0xC0 and 0xC1 pass through unchanged.  F (aha_amd/csrc/fold_table.hpp, written by
 * tools/gen_fold_table.py from Unicode 13.0.0): with one(s) = "s is one code point in U+0080 .. U+07FF", u = upper(c) if
 * one(upper(c)) else c, F(c) = lower(u) if one(lower(u)) else c.  F is idempotent, gives one representative per case class
 * and equals full case folding wherever that is one code point; it moves 450 code points (Latin-1 Supplement, Latin
 * Extended-A/B, Greek, Cyrillic, Armenian), 108 of them to another lead byte; U+00DF, U+0130, U+0131 and U+017F stay (their
 * partners are not single two-byte characters).  Lengths never change and a lead byte stays a lead byte, so byte offsets,
 * char offsets, masks, selections and substituted copies are those of the original text.
 * THE RULE is AHA_OPT_FOLD_ASCII's with its three exceptions unchanged: every call gives, bit for bit, what the same call gives
 * on an ordinary handle compiled from fold2(key) of each key and run over the batch in which EACH DOCUMENT is folded on its
 * own, fold2(corpus[off[d] .. off[d + 1])) -- a lead byte that ends document d never pairs with a continuation byte that
 * opens d + 1.  Covered: match, match_longest in both modes, a separator filter (it tests the folded neighbour bytes), char
 * offsets, count, document counts, class counts, cover, redact, select, replace, records, grep, the pack / unpack exchange,
 * replicate and export.  Two keys equal after fold2 are AHA_E_DUP_KEY at the second; aha_ac_id folds its argument with
 * fold2; aha_ac_load takes the flag in `opts` again.
 * NOT supported yet, AHA_E_INVALID before any device work: aha_feed_open / aha_feed_open_params on such a handle (a character
 * may be cut between two calls) and aha_group_compile with the flag (the shards cut the batch).  The same holds with
 * AHA_OPT_FOLD_KANA below.
 * Cost: every engine, the prefix filter included, reads a folded copy made by one streaming pass into scratch (N bytes) and a
 * fix-up of one lane per document boundary (scan_fold.hip). */
#define AHA_OPT_FOLD_SIMPLE 8u
/* ... and for the characters UTF-8 writes in three bytes (a pure addition to ABI 8 again; implies AHA_OPT_FOLD_SIMPLE and
 * AHA_OPT_FOLD_ASCII: 16u alone means what 4u | 8u | 16u means, and aha_ac_flags reports the bits as they were passed).
 * fold3(buf) is a byte-to-byte map of one buffer, as long as its input.  At every j the first of these that applies: buf[j] in
 * 0xE0 .. 0xEF, j + 2 < len and buf[j + 1], buf[j + 2] both in 0x80 .. 0xBF -- the triple becomes the UTF-8 of F3(cp), cp =
 * (b0 & 0xF) << 12 | (b1 & 0x3F) << 6 | (b2 & 0x3F), where 0x800 <= cp <= 0xFFFF and cp is no surrogate; overlong forms and
 * 0xD800 .. 0xDFFF pass through byte for byte --; the pair rule of fold2 above, with the same table; the ASCII fold.  Triples
 * cannot overlap each other or a pair.  A rule on bytes: stray continuation bytes, a truncated triple at the end, four-byte
 * sequences, 0xC0, 0xC1 and 0xF5 .. 0xFF pass through.  F3 (aha_amd/csrc/fold3_table.hpp, written by tools/gen_fold3_table.py
 * from Unicode 13.0.0) is F's construction with one3(s) = "s is one code point in U+0800 .. U+FFFF, no surrogate": u = upper(c) if
 * one3(upper(c)) else c, F3(c) = lower(u) if one3(lower(u)) else c.  F3 is idempotent and gives one representative per case
 * class inside the block; it moves 679 code points in 29 blocks of 64 (Georgian with Mtavruli, Cherokee, Latin Extended Additional with every Vietnamese letter, polytonic Greek, the Roman numerals, the circled letters,
 * Glagolitic, Latin Extended-C/D, Coptic, Cyrillic Extended-B, the full-width Latin letters), 124 of them to another lead byte
 * (U+10A0 Georgian E1 82 A0 -> U+2D00 E2 B4 80, U+13A0 Cherokee E1 8E A0 -> U+AB70 EA AD B0); the lead bytes of moved
 * characters are 0xE1, 0xE2, 0xEA and 0xEF only.  Cherokee lands on its lower-case letters (Unicode's case folding on the
 * upper-case ones: either names the class).  33 code points have their only partner outside the block -- the Kelvin sign
 * U+212A (k), the ohm sign U+2126, the Angstrom sign U+212B, U+1E9E (U+00DF), U+1FBE, U+1C80 .. U+1C87, U+2C62, U+2C64 .. U+2C66,
 * U+2C6D .. U+2C70, U+2C7E, U+2C7F, U+A78D, U+A7AA .. U+A7AE, U+A7B0 .. U+A7B2, U+A7C5 --: folding them would change a length,
 * so they stay.  Lengths never change and a lead byte stays a lead byte: all offsets are those of the original text.
 * THE RULE, what is covered and the three exceptions are AHA_OPT_FOLD_SIMPLE's with fold3 for fold2: keys are folded one by one
 * (two keys equal after fold3 are AHA_E_DUP_KEY at the second, aha_ac_id folds its argument), a batch document by document --
 * a character cut by a document boundary is not folded --, aha_ac_load takes the flag in `opts` again.
 * NOT supported yet, AHA_E_INVALID before any device work: aha_feed_open / aha_feed_open_params on such a handle and
 * aha_group_compile with the flag.  The same holds with AHA_OPT_FOLD_KANA below.
 * Cost: AHA_OPT_FOLD_SIMPLE's -- one streaming pass into scratch (N bytes) and a fix-up of one lane per document boundary; ASCII
 * text costs what it costs there, text of three-byte characters about twice that pass (scan_fold.hip). */
#define AHA_OPT_FOLD_BMP 16u
/* ... and for the three scripts Japanese text spells its kana in (a pure addition to ABI 8 again; implies AHA_OPT_FOLD_BMP and
 * through it AHA_OPT_FOLD_SIMPLE and AHA_OPT_FOLD_ASCII: 32u alone means what 4u | 8u | 16u | 32u means, and aha_ac_flags reports
 * the bits as they were passed): a key list in katakana hits text spelled in hiragana or in half-width katakana.
 * foldk(buf) is fold3(buf) with FK in place of F3 for the triples; pairs, ASCII and everything that passes through are
 * unchanged.  FK(cp) = K(cp) where K moves cp, else F3(cp).  K maps these 144 code points and nothing else:
 *   hiragana U+3041 .. U+3096            -> cp + 0x60, the katakana letters U+30A1 .. U+30F6
 *   the iteration marks U+309D, U+309E   -> U+30FD, U+30FE
 *   half-width katakana U+FF66 .. U+FF9D -> the one code point NFKC gives (U+FF71 -> U+30A2, the long-vowel mark U+FF70 -> U+30FC)
 * FK is committed as data (aha_amd/csrc/foldk_table.hpp, written by tools/gen_foldk_table.py from Unicode 13.0.0, in
 * fold3_table.hpp's two levels: F3's 29 live blocks and those of U+3040, U+3080, U+FF40 and U+FF80).  Every image is a
 * three-byte KATAKANA character, no image is a source of K, no source or image has a case mapping: FK is idempotent, K and F3
 * never meet.  The half-width kana change their lead byte (EF -> E3), hiragana their second or third byte; lengths never change
 * and a lead byte stays a lead byte, so all offsets, masks, selections and substituted copies are those of the original text.
 * Limits: the representative is katakana.  A half-width letter followed by a voiced or semi-voiced mark (U+FF76 U+FF9E, six
 * bytes) does NOT become the voiced letter (U+30AC, three bytes): that would change a length; it folds to U+30AB followed by
 * the unchanged U+FF9E.  U+FF9E and U+FF9F stay.  Small and large kana stay apart.  U+30F7 .. U+30FA, U+309F, U+30FF and the
 * combining marks U+3099, U+309A stay.  No normalisation takes place.
 * THE RULE, what is covered and the three exceptions are AHA_OPT_FOLD_BMP's with foldk for fold3: keys are folded one by one
 * (two keys equal after foldk -- U+3042 and U+30A2, U+FF71 and U+30A2 -- are AHA_E_DUP_KEY at the second, aha_ac_id folds its
 * argument), a batch document by document -- a character cut by a document boundary is not folded --, aha_ac_load takes the
 * flag in `opts` again and aha_ac_replicate copies it.  Every batch call family is covered.
 * NOT supported yet, AHA_E_INVALID before any device work: aha_feed_open / aha_feed_open_params on such a handle and
 * aha_group_compile with the flag.
 * Cost: AHA_OPT_FOLD_BMP's, by a kernel of its own (scan_foldk.hip k_foldk_copy; AHA_FOLDK_HALO=mem|lane chooses how a lane
 * gets the bytes around its piece). */
#define AHA_OPT_FOLD_KANA 32u

/* Per-call options mirroring the reference's overloads:
 *   char_offsets = 0: match(seq : Bytes)        src/aha/ac.cr:280-286  (byte offsets)
 *   char_offsets = 1: match(seq : String)       src/aha/matcher.cr:34-39 (char offsets; valid UTF-8)
 *   sep_size > 0    : match(seq, sep : BitArray) src/aha/ac.cr:321-340, matcher.cr:41-46;
 *                     sep_bits is the BitArray, LSB-first, sep_size <= 256. */
typedef struct {
  uint32_t struct_size;
  int32_t char_offsets;
  int32_t sep_size;
  uint8_t sep_bits[32];
  /* match_longest(seq, intersectable) -- src/aha/ac.cr:118-143, 249-263, 297-319: 0 = plain match (default; also when
   * struct_size stops before this field), 1 = match_longest with intersectable = false, 2 = with intersectable = true.
   * Not combinable with a separator filter (the reference has no such overload): AHA_E_INVALID.
   * intersectable = true is chunk-parallel (a 2 * Lmax warm-up makes the pending-end register exact);
   * intersectable = false resets the state after every yield, so a document is walked in order by one thread
   * (documents in parallel) -- correct at any size, fast only for batches of many documents. */
  int32_t longest;
} aha_match_params;

typedef struct {
  uint32_t struct_size;
  uint32_t n_keys;          /* K */
  uint64_t n_states;        /* trie nodes incl. root */
  uint64_t n_slots;         /* double-array slots in the device image */
  uint64_t image_bytes;     /* bytes resident in HBM for the automaton */
  uint32_t max_key_len;     /* Lmax, bytes */
  uint32_t slot_bytes;      /* 4 (compact) or 8 (wide) */
  uint32_t lds_slots;       /* slots of the image cached in LDS by the match kernel */
  int32_t device;           /* device the image lives on, -1 if host only */
  /* Shadow fail links (all 0 = every state has a fail header at slot[base]).  Otherwise only the root and the
   * states with base >= fail_hdr_lo own one; for the others the fail target follows from the last input bytes:
   * base < fail_s1_lo: root; base < fail_s2_lo: the depth-1 state of the last byte; base < fail_hdr_lo: the
   * deepest state of depth <= 2 spelled by the last two bytes. */
  uint32_t fail_s1_lo;
  uint32_t fail_s2_lo;
  uint32_t fail_hdr_lo;
  uint32_t unit_header_beside;  /* ABI 7 (was reserved): 1 = the character-level traversal requests a state's fail header beside
                                 * its probe instead of in a trip of its own -- chosen when the image is compiled, for key sets
                                 * where at least a fifth of the states own a header (text then falls out of deep matches often:
                                 * -8.5 % on BASELINE config 5, +3.5 % on config 3, which keeps the header trip) */
  /* Character-level image (aha_amd/csrc/unit.hpp), built when every key is a sequence of UTF-8-shaped units, at least
   * 30 % of the key bytes lie in multi-byte characters and the keys' characters fit the symbol table (AHA_ENGINE=unit:
   * for every eligible key set).  1 = this handle's matches without a separator filter -- byte or char offsets -- take
   * one step per character instead of one per byte (bit-exact; aha_timing.engine = 4); on a host-only handle: the image
   * was built (aha_ac_export). */
  uint32_t unit_enabled;
  uint32_t unit_slots;          /* 8-byte slots of its double array */
  uint32_t unit_syms;           /* symbols of its dense alphabet (the root's transitions: 4 bytes each, in LDS) */
  uint32_t unit_multi_permille; /* key bytes in multi-byte units, per 1000 */
  /* ABI 6: how the image's big states are laid out (aha_amd/csrc/unit.hpp, BIG STATES) -- what a reader of
   * AHA_IMG_UNIT_SLOTS needs beside the slots: a state with base >= unit_big_lo owns unit_big_block slots; the symbols
   * below unit_n_low index them directly, the others select a group record at base + unit_n_low - unit_n_low / 32 +
   * (symbol >> 5). */
  uint32_t unit_big_lo;
  uint32_t unit_big_block;
  uint32_t unit_n_low;
  uint32_t unit_n_big;
  uint32_t unit_base_bits;      /* 22, or 23 for an image beyond 2^22 slots: width of the base field of a state word; the
                                 * filter takes the bits from there up to bit 28 (7 or 6 of them) */
  uint32_t unit_headers;        /* ABI 7 (was reserved): states of the character-level image that own a fail header (their fail
                                 * state is neither the root nor a one-character state) */
  /* ABI 7: the prefix-filter engine (aha_amd/csrc/scan_filter.hip; aha_timing.engine = 5).  Built for a key set without a
   * character-level image whose keys are 3 .. 64 bytes long (a keyword list): a blocked Bloom filter over the keys' first
   * filter_prefix_bytes bytes (min(4, shortest key); 0 = this handle has none) of filter_words 32-bit words.  Matches without
   * a separator filter -- byte or char offsets -- then look at every text position
   * through the filter and walk the automaton only from the positions it lets through; a batch whose text is dense with
   * such positions (more than about one in twenty) is handed to the single-traversal engine by the call itself
   * (aha_timing.repeats counts it). */
  uint32_t filter_prefix_bytes;
  uint32_t filter_words;
  /* ABI 8: the skip-ahead traversal (aha_amd/csrc/scan_skip.hip; aha_timing.engine = 6) over the character-level image.
   * While the state of src/aha/ac.cr:176-192 is the root or a one-character state, its next state depends on the next two
   * characters alone and -- when no key is a single character -- nothing can be reported, so the walk may jump to the next
   * position where a two-character trie path starts.  A stateless first kernel marks those positions through a blocked Bloom
   * filter over the image's skip_pairs two-character paths (skip_filter_words 32-bit words, keyed by the characters' raw bytes;
   * 0 = this handle has none: not asked for, a one-character key, 23-bit bases, the header requested beside the probe); the
   * second kernel is the character-level traversal, started only at marked positions.  Byte offsets, no separator filter;
   * every other call of the handle keeps engine 4.  OPT-IN (AHA_ENGINE=skip or AHA_SKIP=1 when the handle is compiled): on
   * BASELINE config 3 it is slower than engine 4 (its lanes' scattered text requests), so no key set gets it by default. */
  uint32_t skip_filter_words;
  uint32_t skip_pairs;
  /* ABI 8: the pair engine (aha_amd/csrc/scan_pair.hip; aha_timing.engine = 7).  The same two-character paths behind the same
   * filter, once more as a perfect hash table keyed by the characters' raw bytes (pair_table_log2: log2 of its 16-byte slots, 0 =
   * none; pair_groups displacement bytes; pair_hash_k1 the multiplier of the second character in the pair hash -- chosen so that
   * no two pairs share the 32-bit value; marks and table use the same hash).  A stateless pass over every character resolves
   * the two-character states itself -- one 16-byte load per filter-positive pair -- and writes their events in position order;
   * only the positions where a THIRD character can continue a path (a few per cent) are walked, by a second kernel that voids
   * the events its walks cover and fills its own into slots the first pass left for them.  pair_engine = 1: this handle's
   * matches with byte offsets and without a separator filter run it (no one-character key, at most three END states of three
   * characters or more on one trie path); every other call keeps the engine it had. */
  uint32_t pair_hash_k1;
  uint32_t pair_table_log2;
  uint32_t pair_groups;
  uint32_t pair_engine;
} aha_ac_info_t;

/* Timing of the most recent device match on this handle (HIP events recorded
 * on the launch stream).  Only filled when profiling is enabled. */
typedef struct {
  uint32_t struct_size;
  uint32_t n_kernels;
  float ms_total;           /* first launch -> hits and offsets final in HBM */
  float ms_count;           /* engines 4, 2: the traversal kernel; engine 5: the filter kernel; engine 6: the marking kernel; engine 1:
                             * traversal pass 1 */
  float ms_scan;            /* scans of per-chunk counts (slab pipeline; the region pipelines have them in ms_aux: no event in
                             * between); engine 5: the candidates' walks (chunk records + kf_walk); engine 6: the traversal */
  float ms_write;           /* engine 2: chain expansion + doc offsets; engine 1: traversal pass 2 */
  float ms_aux;             /* engine 2: hits per chunk + scan (regions) or event sort (slabs); engine 1: char-offset prefix pass */
  uint64_t n_chunks;
  uint64_t n_hits;
  uint32_t engine;          /* 7 = pair engine (stateless pair pass + deep walks), 6 = marks + skip-ahead character-level traversal,
                             * 5 = prefix filter + candidate walks,
                             * 4 = character-level traversal, 2 = single-traversal engine, 1 = two-pass engine */
  uint32_t chunk_bytes;     /* bytes per lane chunk */
  /* ABI 6: passes over the batch that were thrown away before this one: 1 when a chunk's event region overflowed -- the
   * batch was denser than `cap` said -- and the match ran once more with full-size regions (the call took about twice
   * the time: give a capacity nearer to the hits to avoid it); +1 when the event temp overflowed and the two-pass engine
   * took over. */
  uint32_t repeats;
  uint32_t reserved;
} aha_timing;

const char *aha_strerror(int32_t code);
/* Message of the last error of the CALLING THREAD (thread-local: calls on one handle may run concurrently; `ac` may be
 * NULL, e.g. after aha_buffer_* / aha_corpus_upload). */
const char *aha_last_error(const aha_ac *ac);
uint32_t aha_abi_version(void);
/* Number of visible HIP devices (0 when there is none / no driver). */
int32_t aha_device_count(void);

/* Aha::AC.compile(keys) -- src/aha/ac.cr:62-112.  Keys are one blob plus K+1
 * offsets.  On AHA_E_EMPTY_KEY / ZERO_BYTE / DUP_KEY *err_key (optional) is
 * the index of the offending key (the index at which the reference raises). */
int32_t aha_ac_compile(const uint8_t *key_bytes, const uint64_t *key_offsets, uint32_t n_keys,
                       const aha_options *opts, aha_ac **out, uint32_t *err_key);
void aha_ac_free(aha_ac *ac);
/* A second handle for the same keys on `device` (< 0: the current one): the host side of `ac` is copied and uploaded,
 * nothing is compiled again.  What aha_group_compile does for every device after the first -- the reference's compile
 * is one call (src/aha/ac.cr:62-69), so n devices must not cost n compiles. */
int32_t aha_ac_replicate(const aha_ac *ac, int32_t device, aha_ac **out);
int32_t aha_ac_info(const aha_ac *ac, aha_ac_info_t *info);
/* The AHA_OPT_* bits the handle was compiled with (AHA_OPT_FOLD_ASCII among them); 0 for a NULL handle.  A pure addition
 * to ABI 8. */
uint32_t aha_ac_flags(const aha_ac *ac);

/* AC#[](sid : Int) : String and AC#[](key) : Int -- delegated to the trie in
 * the reference (src/aha/ac.cr:41-43, src/aha/cedar.cr:747-749, 817-834).
 * aha_ac_key returns the key length (copies min(len,cap) bytes) or <0. */
int32_t aha_ac_key(const aha_ac *ac, int32_t id, uint8_t *buf, int32_t cap);
int32_t aha_ac_id(const aha_ac *ac, const uint8_t *key, int32_t len);

/* The batch entry below with the hits left on the device: host corpus and offsets in (uploaded range by range beside
 * the matches, like aha_ac_match_batch), hits into d_hits[0 .. cap) -- device memory of the handle's device --, per-document
 * offsets (optional) and the count to the host.  For callers that go on working with the hits on the GPU; each shard of
 * aha_group_match_batch is one such call.  AHA_E_CAPACITY: *n_hits is the required count. */
int32_t aha_ac_match_batch_keep(aha_ac *ac, const uint8_t *corpus, const uint64_t *doc_offsets, uint64_t n_docs,
                                const aha_match_params *params, aha_hit *d_hits, uint64_t cap,
                                uint64_t *doc_hit_offsets, uint64_t *n_hits);

/* AC#match on ONE sequence held in host memory (uploads, matches on the GPU,
 * downloads).  Hits come back in the reference's order: ascending end
 * position, and per position own key first, then the output chain
 * (src/aha/ac.cr:176-192, 265-278).  params may be NULL (plain byte match). */
int32_t aha_ac_match_bytes(aha_ac *ac, const uint8_t *text, uint64_t n,
                           const aha_match_params *params, aha_hit *out, uint64_t cap,
                           uint64_t *n_hits);

/* Batch entry (new; the reference is one-sequence-per-call): D documents,
 * document d = corpus[doc_offsets[d] .. doc_offsets[d+1]); doc_offsets[0]
 * must be 0.  Equivalent to D independent #match calls concatenated;
 * doc_hit_offsets (D+1 entries, optional) delimits each document's hits. */
int32_t aha_ac_match_batch(aha_ac *ac, const uint8_t *corpus, const uint64_t *doc_offsets,
                           uint64_t n_docs, const aha_match_params *params, aha_hit *out,
                           uint64_t cap, uint64_t *doc_hit_offsets, uint64_t *n_hits);

/* Device-resident variant: every pointer prefixed d_ is HBM on the handle's
 * device; nothing crosses PCIe except the 8-byte hit count.  `stream` is a
 * hipStream_t (NULL = default stream).  Blocks until the hits are final.
 * On AHA_E_CAPACITY the first `cap` hits and all offsets are still valid.
 * d_doc_offsets must hold n_docs + 1 ascending offsets with [0] = 0 and [n_docs] = n_bytes, every document shorter
 * than 2^31 bytes: checked on the device before anything is indexed with them (AHA_E_INVALID / AHA_E_TOO_LONG) -- by a
 * small kernel in front of the traversal whose verdict every later kernel of the call looks at first, so a valid call
 * pays no read-back for it (match_longest and the two-pass engine read the verdict back before they start). */
int32_t aha_ac_match_batch_device(aha_ac *ac, const uint8_t *d_corpus,
                                  const uint64_t *d_doc_offsets, uint64_t n_docs,
                                  uint64_t n_bytes, const aha_match_params *params,
                                  aha_hit *d_out, uint64_t cap, uint64_t *d_doc_hit_offsets,
                                  uint64_t *n_hits, void *stream);

/* ABI 7 -- aha_ac_match_batch_device that leaves the hits ALSO as the 4-byte exchange stream (below: the format of
 * aha_ac_hits_pack4_device, bit-compatible with aha_ac_hits_unpack4_*): d_words[0 .. *d_n_words) on the device, capacity
 * cap_words >= 2 cap + ceil(cap / 1024) + 1 words: the pack kernels run behind the match on the same stream, one call instead
 * of two (what every resident shard of a group calls).  Final when the call returns. */
int32_t aha_ac_match_batch_device_stream(aha_ac *ac, const uint8_t *d_corpus, const uint64_t *d_doc_offsets, uint64_t n_docs,
                                         uint64_t n_bytes, const aha_match_params *params, aha_hit *d_out, uint64_t cap,
                                         uint64_t *d_doc_hit_offsets, uint64_t *n_hits, uint32_t *d_words, uint64_t cap_words,
                                         uint64_t *d_n_words, void *stream);

/* Exchange format for the multi-GPU all-gatherv of hit buffers (SURVEY.md
 * section 8 e): Hit#start = Hit#end - length of key[value] (src/aha/ac.cr:270-272;
 * with char offsets: - number of chars of the key), so ranks send {end, value}
 * pairs (8 B per hit instead of 12 on the xGMI links) and rebuild the triples
 * on arrival.  All pointers are HBM on the handle's device; the calls are
 * asynchronous on `stream`.  d_pairs holds 2*n int32, d_hits n triples. */
int32_t aha_ac_hits_pack_device(aha_ac *ac, const aha_hit *d_hits, uint64_t n, int32_t *d_pairs,
                                void *stream);
int32_t aha_ac_hits_unpack_device(aha_ac *ac, const int32_t *d_pairs, uint64_t n, int32_t char_offsets,
                                  aha_hit *d_hits, void *stream);

/* The 4-byte form of the same exchange.  Hits of a batch come in per-document order with ascending `end`, so the stream
 * carries one word per hit, value << (step_bits + len_bits) | len << step_bits | step, with step = end - previous end
 * and len = end - start (the key's length in the batch's offsets), and the absolute `end` only for the first hit of
 * every 1024, for a document change and for a gap of 2^step_bits - 1 or more:
 *   d_words = words[n] . first_exception[ceil(n/1024)] . exception_end[...]
 * The widths follow from the automaton (aha_ac_stream_format; every rank holds the same one): key ids take
 * bit_width(n_keys - 1) bits, lengths bit_width(longest key in bytes); with at least 10 bits left the step gets what is
 * left (at most 12) and the receiver rebuilds Hit#start without a table lookup; else len_bits = 0, step_bits = 12
 * (key ids below 2^20) and the length is looked up on arrival (a narrower step would turn every gap of a few hundred
 * bytes into an exception, 4 more bytes on the link).
 * pack4 needs cap_words >= 2 n + ceil(n/1024) (the worst case) and writes the real length -- what has to travel --
 * into *d_n_words (device memory); unpack4 takes the stream and n.  Asynchronous on `stream`. */
int32_t aha_ac_stream_format(const aha_ac *ac, uint32_t *step_bits, uint32_t *len_bits);
int32_t aha_ac_hits_pack4_device(aha_ac *ac, const aha_hit *d_hits, uint64_t n, uint32_t *d_words,
                                 uint64_t cap_words, uint64_t *d_n_words, void *stream);
int32_t aha_ac_hits_unpack4_device(aha_ac *ac, const uint32_t *d_words, uint64_t n, int32_t char_offsets,
                                   aha_hit *d_hits, void *stream);
/* Several streams rebuilt by ONE launch (an 8-GPU step receives seven peers' streams): stream k starts at word
 * word_offset of d_words, holds n_hits hits and is written to d_hits[out_offset ..].  At most 64 segments. */
typedef struct {
  uint64_t word_offset;
  uint64_t n_hits;
  uint64_t out_offset;
} aha_stream_seg;
int32_t aha_ac_hits_unpack4_segs_device(aha_ac *ac, const uint32_t *d_words, const aha_stream_seg *segs,
                                        uint32_t n_segs, int32_t char_offsets, aha_hit *d_hits, void *stream);

/* Copies one array of the automaton image (as uploaded to HBM) into buf;
 * returns its size in bytes (call with cap_bytes = 0 to size the buffer).
 * Data only -- used by host-logic tests and debugging tools. */
enum {
  AHA_IMG_SLOTS = 0,   /* uint32[n_slots] (compact) or uint64[n_slots] (wide) */
  AHA_IMG_END_KEY = 1, /* int32[n_slots], compact only */
  AHA_IMG_KEY_LN = 2,  /* {uint32 len, int32 next}[K] */
  AHA_IMG_KEY_CNT = 3, /* uint32[K] */
  AHA_IMG_KEY_KC = 4,  /* uint32[K] */
  AHA_IMG_UNIT_SLOTS = 6,     /* uint64[unit_slots]: a transition is lo = child base (22 bits) | filter (7) << 22 | F1 << 29 |
                                 NFR << 30 | END << 31, hi = symbol (16 bits) | min(hits, 255) << 16; slots[base] of a state with
                                 NFR and without F1 is its header {word of the fail state, 0}; group records and child runs of
                                 the big states: aha_amd/csrc/unit.hpp, IMAGE and BIG STATES */
  AHA_IMG_UNIT_ROOT = 7,      /* uint32[unit_syms]: the root's transitions by symbol */
  AHA_IMG_UNIT_END_KEY = 8,   /* int32[unit_slots]: key id at the base of an END state, else -1 */
  AHA_IMG_UNIT_TABLES = 9,    /* uint32[2816]: the decode tables (unit.hpp, SYMBOLS) */
  AHA_IMG_UNIT_MARKS = 10,    /* uint32[skip_filter_words]: the Bloom filter over the two-character paths (unit.hpp, MARKS) */
  AHA_IMG_UNIT_PAIRS = 11,    /* uint32[4 << pair_table_log2]: the pair table {raw0 | hits << 24, raw1, event payload, child filter} */
  AHA_IMG_UNIT_PAIR_DISP = 12, /* uint8[pair_groups]: its displacement bytes (unit.hpp, PAIR TABLE) */
  AHA_IMG_STALE_ENDS = 5     /* {uint32 key id, uint32 prefix length}[]: the states (a prefix of a key each) whose node in
                                 the reference's Cedar keeps a stale END flag (src/aha/cedar.cr:642-648); match_longest
                                 treats them as ends that yield nothing (src/aha/ac.cr:126-128, 249-263) */
};
int64_t aha_ac_export(const aha_ac *ac, int32_t which, void *buf, uint64_t cap_bytes);

/* AC#to_io / AC.from_io -- src/aha/ac.cr:45-60 (`save`/`load` in the reference's
 * README).  The reference's on-disk framing goes through the un-vendored
 * `super_io` shard and no reference test reads a loaded automaton back
 * (parity unpinned), so this is the library's OWN
 * container, not the Crystal byte stream: little endian
 *   "AHAHIP01" | u32 format=1 | u32 K | u64 blob_bytes | u64 offs[K+1] | blob |
 *   u64 FNV-1a of everything before it.
 * It stores the keys in `compile` order; aha_ac_load re-derives the automaton
 * (deterministic, same key ids), so a file written by one build loads in any
 * later one.  aha_ac_save returns the size in bytes (cap_bytes = 0 sizes the
 * buffer) or <0; aha_ac_load returns AHA_E_INVALID for a truncated/corrupt
 * buffer, else whatever aha_ac_compile returns. */
int64_t aha_ac_save(const aha_ac *ac, void *buf, uint64_t cap_bytes);
int32_t aha_ac_load(const void *buf, uint64_t n_bytes, const aha_options *opts, aha_ac **out);

/* ---- counts without the hit list (pure additions to ABI 8) ---------------------------------------------------------
 * The same batch, params and results as aha_ac_match_batch, but instead of the hits: key_counts[k] = hits with value k
 * (k < K; uint64, exactly K entries written), doc_hit_offsets (D+1 entries, optional) = the match call's offsets, *n_hits =
 * its hit count.  key_counts == NULL: only the total and the offsets (no per-key pass).  No capacity, so no AHA_E_CAPACITY.
 * char_offsets changes no count (the call takes the byte-offset route); a separator filter counts the filtered hits;
 * longest != 0 is AHA_E_INVALID.  AHA_COUNT_ACCUMULATE adds into key_counts instead of overwriting it: running totals over
 * a corpus streamed through in batches.  Errors, device validation of d_doc_offsets, threading (a call leases a scratch
 * set) and the host entry's range-by-range uploads are those of the match entries.  A device call refused for its offsets
 * (AHA_E_INVALID / AHA_E_TOO_LONG) writes no doc_hit_offsets but may already have cleared d_key_counts (without
 * AHA_COUNT_ACCUMULATE): the verdict comes from the device, behind the clear -- unlike aha_feed_count_batch*, which leaves
 * key_counts as it was.  A count call changes nothing a later
 * match call of the handle depends on.  Pipeline: the match's engine with full-size event regions (document ranges where
 * they do not fit: device scratch above); one add per EVENT (END position) into an LDS table per workgroup instead of the
 * expansion, then the keys' output chains (aha_amd/csrc/scan_count.hip).  A separator filter -- a test per hit -- and
 * whatever a match would give the two-pass engine take that engine's counting pass: one traversal with per-key adds, the
 * documents' offsets noted on the way (a match with a separator filter takes the slab pipeline instead).  aha_ac_last_timing: engine = the engine that traversed, n_hits = the
 * total, ms_write = the counting passes. */
#define AHA_COUNT_ACCUMULATE 1u /* add into key_counts / d_key_counts instead of overwriting them */
int32_t aha_ac_count_batch(aha_ac *ac, const uint8_t *corpus, const uint64_t *doc_offsets, uint64_t n_docs,
                           const aha_match_params *params, uint32_t flags, uint64_t *key_counts /* K or NULL */,
                           uint64_t *doc_hit_offsets /* D+1 or NULL */, uint64_t *n_hits);
/* Device-resident form: d_ pointers are HBM on the handle's device; *n_hits is host memory; blocks until final. */
int32_t aha_ac_count_batch_device(aha_ac *ac, const uint8_t *d_corpus, const uint64_t *d_doc_offsets, uint64_t n_docs,
                                  uint64_t n_bytes, const aha_match_params *params, uint32_t flags,
                                  uint64_t *d_key_counts /* K or NULL */, uint64_t *d_doc_hit_offsets /* or NULL */,
                                  uint64_t *n_hits, void *stream);

/* ---- feeds: sequences that arrive in pieces across calls (pure additions to ABI 8) ----------------------------------
 * A feed is n_seqs open sequences bound to one device handle.  A call matches a batch of D pieces: piece d =
 * corpus[piece_offsets[d] .. piece_offsets[d+1]) is the next part of sequence seq_ids[d].  Its hits are exactly those that one
 * plain match over the whole sequence so far (every piece since open or reset, concatenated) reports with an end inside the
 * piece, in the same order, bit for bit; the hits of piece d are out[piece_hit_offsets[d] .. piece_hit_offsets[d+1]).
 * Offsets are int32 and relative to the piece's first byte -- or, on a char feed (AHA_FEED_CHARS at open), its first
 * character under the lead-byte rule, as the whole sequence's char map has it where a piece begins inside a character --;
 * start may be negative down to -(Lmax-1): the hit began in an earlier piece.  piece_bases[d] (uint64) = the sequence's length
 * before the piece (bytes, or lead bytes on a char feed): absolute offset = base + relative.  A sequence has no length
 * limit; a piece must be shorter than 2^31 bytes minus Lmax (AHA_E_TOO_LONG).  Within one call a sequence appears at most
 * once (AHA_E_INVALID); pieces may come in any order and a call may name any subset of the sequences.  A call that fails
 * changes nothing, AHA_E_CAPACITY included: *n_hits is then the exact count and the same call with a larger buffer gives what
 * the first would have.  Counts: aha_feed_count_batch* below.  Separator filter: match and count calls take one fixed when the
 * feed is opened (aha_feed_open_params, "feed separator filter" below); cover and select calls do not yet (follow-ups).
 * match_longest: a longest feed, opened with aha_feed_open_params ("feed match_longest" below); its match and finish calls
 * report match_longest's hits, the other call families do not take such a feed yet (follow-ups).
 * Errors: aha_last_error(ac).  Calls
 * on one feed are serialised (a mutex in the feed); different feeds and plain calls on the handle run side by side.
 * Pipeline (aha_amd/csrc/feed.cpp, scan_feed.hip): with W = max(Lmax-1, 0) the feed keeps the last
 * min(W, length) bytes of every sequence on the device.  A call matches one window batch of at most 4 W bytes per piece (the
 * hits that straddle or follow a cut), then the pieces as they are (the engine a plain match of them takes: aha_ac_last_timing
 * reports it), and merges the two by count.  Device memory of a feed: 2 W + 24 bytes per sequence; per call, the window
 * batch, 12 bytes per hit of (cap + the hits of the pieces' first W bytes) for the main pass, ~100 bytes per piece, and the
 * handle's scratch set for the two matches; the host entry stages the corpus and the hits on the device as well. */
typedef struct aha_feed aha_feed;
#define AHA_FEED_CHARS 1u /* offsets and bases in characters (the lead-byte rule) instead of bytes */
/* A FOLDED FEED: AHA_FEED_FOLD on a handle compiled with AHA_OPT_FOLD_SIMPLE, _BMP or _KANA (without the flag such a handle has
 * no feeds: AHA_E_INVALID; on any other handle the flag changes nothing).  Let fold be the handle's fold of ONE document -- a
 * truncated character at its end passes through.  A call that takes a sequence S from n0 to n1 bytes reports exactly the hits
 * with n0 < end <= n1 of fold(S[0 .. n1)) matched as one document by a plain handle of the folded keys: every call answers as if
 * the sequence ended with its piece.  A character cut between two calls is folded whole and hits that run through it are found;
 * a character still open at the end of a call is not folded yet, and only a hit that ENDS on one of its bytes is decided on the
 * unfolded byte (the feed's form of "a character cut by a document boundary is not folded").  Such a hit needs a key that ends
 * in a truncated UTF-8 sequence: for keys that are whole characters the feed is bit-exact with the batch call on the whole
 * sequence as one document.  Offsets, bases, piece_hit_offsets, char offsets (AHA_FEED_CHARS), counts and cover masks follow
 * from that hit list as on a plain feed.  Opt-in because the feed keeps W = Lmax + 1 bytes of context (ORIGINAL bytes) and has
 * the open-character rule.  Calls: aha_feed_match_batch*, aha_feed_count_batch* and aha_feed_cover_batch* (the redacted copy
 * keeps the caller's bytes outside hits); aha_feed_select_batch*, _replace_ and _grep_ answer AHA_E_INVALID and leave the feed
 * as it was (follow-ups), aha_feed_finish_batch* as on every plain feed.  With a separator filter or longest != 0:
 * AHA_E_INVALID before any device work (follow-ups).  Pipeline (aha_amd/csrc/scan_feedfold.hip; DESIGN.md 4.13 "Feeds on
 * handles folded beyond ASCII"): per call the pieces are folded once into feed scratch (n_bytes + 64 bytes), the first two bytes
 * of each with the sequence's context in view, the windows are cut from the fold of context || piece, and both matches read
 * text that is already folded. */
#define AHA_FEED_FOLD 4u /* (2u is refused: the value is not taken) */
/* AHA_E_NO_DEVICE on a host-only handle; AHA_E_INVALID for NULL arguments, n_seqs = 0, unknown flags, or a handle folded
 * beyond ASCII without AHA_FEED_FOLD. */
int32_t aha_feed_open(aha_ac *ac, uint32_t n_seqs, uint32_t flags, aha_feed **out);
/* Frees the feed (waits for a call in flight); before aha_ac_free of its handle. */
void aha_feed_free(aha_feed *f);
/* The sequence starts again from length 0; UINT32_MAX: every sequence. */
int32_t aha_feed_reset(aha_feed *f, uint32_t seq);
/* Length of a sequence so far, in bytes and in lead bytes (the latter counted on char feeds only); either may be NULL. */
int32_t aha_feed_position(const aha_feed *f, uint32_t seq, uint64_t *bytes, uint64_t *chars);
/* Host buffers (the pieces are uploaded to feed scratch; offsets and ids are checked on the host). */
int32_t aha_feed_match_batch(aha_feed *f, const uint8_t *corpus, const uint64_t *piece_offsets, const uint32_t *seq_ids,
                             uint64_t n_pieces, aha_hit *out, uint64_t cap, uint64_t *piece_hit_offsets /* D+1 or NULL */,
                             uint64_t *piece_bases /* D or NULL */, uint64_t *n_hits);
/* Device-resident form: d_ pointers are HBM on the handle's device, validated on the device before anything is indexed with
 * them; *n_hits is host memory; blocks until final. */
int32_t aha_feed_match_batch_device(aha_feed *f, const uint8_t *d_corpus, const uint64_t *d_piece_offsets,
                                    const uint32_t *d_seq_ids, uint64_t n_pieces, uint64_t n_bytes, aha_hit *d_out,
                                    uint64_t cap, uint64_t *d_piece_hit_offsets /* D+1 or NULL */,
                                    uint64_t *d_piece_bases /* D or NULL */, uint64_t *n_hits, void *stream);
/* Feed counts: the same pieces as aha_feed_match_batch*, and what a match call of them would give as hits per key --
 * key_counts[k] = its hits with value k (uint64, exactly K entries written) -- with its piece_hit_offsets, piece_bases and
 * *n_hits, but without the hit list.  The sequences move on exactly as the match call would move them, so match and count
 * calls may be mixed freely on one feed (a char feed counts its lead bytes here too).  AHA_COUNT_ACCUMULATE adds into
 * key_counts instead of overwriting it: running totals over a stream of any length; any other flag bit is AHA_E_INVALID.
 * key_counts == NULL: only the total, the offsets and the bases (no per-key pass; the feed still moves on).  No capacity, so
 * no AHA_E_CAPACITY.  A call that fails changes nothing: neither the feed nor key_counts.  Errors and validation are those of
 * the match entries.  Like a count call it writes none of the handle's back-off state; aha_ac_last_timing reports the main
 * pass, which takes the engine aha_ac_count_batch of the same pieces takes.  Pipeline: the window batch
 * matched as for a match call; the pieces counted as by aha_ac_count_batch_device into the feed's own K-word vector; the
 * window hits added with sign (+1 for the context-and-head windows, -1 for the context alone and the head alone); only then
 * the caller's key_counts, offsets and bases, and the feed's state.  Device memory beyond a match call's: 8 bytes per key
 * (16 for the host entry), and no hit buffer for the pieces. */
int32_t aha_feed_count_batch(aha_feed *f, const uint8_t *corpus, const uint64_t *piece_offsets, const uint32_t *seq_ids,
                             uint64_t n_pieces, uint32_t flags, uint64_t *key_counts /* K or NULL */,
                             uint64_t *piece_hit_offsets /* D+1 or NULL */, uint64_t *piece_bases /* D or NULL */,
                             uint64_t *n_hits);
/* Device-resident form: d_ pointers are HBM on the handle's device, validated on the device before anything is indexed with
 * them; *n_hits is host memory; blocks until final. */
int32_t aha_feed_count_batch_device(aha_feed *f, const uint8_t *d_corpus, const uint64_t *d_piece_offsets,
                                    const uint32_t *d_seq_ids, uint64_t n_pieces, uint64_t n_bytes, uint32_t flags,
                                    uint64_t *d_key_counts /* K or NULL */, uint64_t *d_piece_hit_offsets /* D+1 or NULL */,
                                    uint64_t *d_piece_bases /* D or NULL */, uint64_t *n_hits, void *stream);

/* ---- feed separator filter: whole-word hits for sequences in pieces (pure additions to ABI 8) ---------------------------
 * aha_feed_open_params opens a feed whose match and count calls apply the reference's separator filter, match(seq, sep :
 * BitArray) src/aha/ac.cr:321-340, to the whole sequence: with pass(c) = c >= sep_size || sep_bits[c] -- applied to fold(c) on a
 * handle with AHA_OPT_FOLD_ASCII -- a hit {start, end, value} of a sequence T survives when (end == |T| || pass(T[end])) and
 * (start == 0 || pass(T[start-1])).  The survivors keep the order of the unfiltered list.  params == NULL or sep_size == 0:
 * exactly aha_feed_open (longest != 0 without a separator filter: a longest feed, below).  sep_size > 256: AHA_E_SEP_SIZE;
 * char_offsets != 0, longest != 0 with a separator filter (the reference has no such overload), or AHA_FEED_CHARS together with a
 * separator filter (the reference's char overload tests code points: out of scope): AHA_E_INVALID; these checks come before
 * the device check, so a host-only handle answers AHA_E_NO_DEVICE only for valid arguments.
 * The byte behind a hit that ends with a piece is not there yet, so such a feed reports a hit ONE BYTE LATE and a sequence has
 * an explicit end.  Stream law: a match call that takes a sequence from n0 to n1 > n0 bytes reports the surviving hits of the
 * sequence with absolute end in [n0, n1): a hit that ended exactly at the previous cut is reported now, tested against this
 * piece's first byte; a hit that ends with this piece is not reported yet; a zero-length piece reports nothing.
 * aha_feed_finish_batch names sequences that end here: it reports their surviving hits with end == n, the sequence's length
 * (the right-hand test passes there), and starts each named sequence again at length 0.  The hits of all of a sequence's calls
 * made absolute (base + relative), concatenated, with the finish call's appended, are aha_ac_match_batch of the whole sequence
 * with the same sep, bit for bit and in the same order.  aha_feed_reset drops the hits that ended with the last byte (nothing
 * is held anywhere: they are found again from the context).
 * Offsets stay relative to the piece's first byte; a carried-over hit has end == 0 and start == -len, so on such a feed start
 * goes down to -Lmax, not -(Lmax-1).  A finish call reports relative to the sequence's end: end == 0, start == -len, and
 * bases[d] = n, the length of sequence seq_ids[d]; its hits are out[seq_hit_offsets[d] .. seq_hit_offsets[d+1]).
 * aha_feed_count_batch* on such a feed gives key_counts, piece_hit_offsets, piece_bases and *n_hits of what the match call of
 * the same pieces would report and moves the feed on exactly as that call would: match and count calls still mix freely.  It
 * does build the call's unfiltered hit list in scratch (12 bytes per unfiltered hit of the pieces), unlike the plain feed
 * count.  A failing call changes nothing; on AHA_E_CAPACITY *n_hits is the exact filtered count, the sequences of a finish call
 * have NOT restarted, and the same call with a larger buffer gives what the first would have.
 * aha_feed_finish_batch*: AHA_E_INVALID on a plain feed (neither a separator filter nor longest), for a sequence named twice or an id >= n_seqs
 * (the device form checks both on the device).  aha_feed_cover_batch* and aha_feed_select_batch* on a feed with a separator
 * filter: AHA_E_INVALID, the feed as it was (follow-ups).
 * Pipeline (aha_amd/csrc/feed.cpp, scan_feedsep.hip; DESIGN.md 4.10 "Feed separator filter"): the feed keeps W = Lmax + 1 bytes
 * of context per sequence (2 W + 24 bytes of device memory), so a hit that ended with the piece before is a hit of the context
 * alone and its left neighbour lies in the context too.  A call runs the window batch and the main pass unfiltered, merges the
 * call's true hits into scratch, flags each (12 B read, two neighbour bytes), ranks the flags, and writes the kept hits -- or
 * adds their values per key -- once the filtered total is known to fit.
 *
 * ---- feed match_longest: longest hits for sequences in pieces (no new symbol: ABI 8 as it is) ------------------------------
 * aha_feed_open_params(ac, n_seqs, 0, params, &feed) with params->longest = 1 (intersectable = false) or 2 (true) and
 * sep_size == 0 opens a LONGEST FEED: the reference's match_longest(seq, intersectable), src/aha/ac.cr:118-143, for sequences
 * that arrive in pieces.  Let Y(T) be what aha_ac_match_batch with the same longest reports for the one-document batch T, in
 * order.  Every hit of Y(T) has a yield position: the index j >= end of the first byte that finds no goto while the hit is the
 * pending end (ac.cr:131-133); if the sequence ends first it has none.
 * Stream law: a match call that takes a sequence from n0 to n1 bytes reports the hits whose yield position lies in [n0, n1); a
 * zero-length piece reports nothing and changes nothing.  aha_feed_finish_batch* on a named sequence reports the one hit that is
 * still pending, if there is one, and starts the sequence again at length 0.  A sequence's match calls, made absolute (base +
 * relative) and concatenated, with the finish call's hit appended, are Y(T) bit for bit and in order; the hits of the calls up
 * to length n plus a finish at n are Y(T[0..n)) for every n.
 * Offsets are relative to the piece's first byte, piece_bases[d] = n0.  A hit may lie wholly in earlier pieces: a pending end is
 * followed by direct gotos only, so start >= -Lmax and end >= -(Lmax - 1), and both bounds are reached.  A finish call reports
 * relative to the sequence's end as on a feed with a separator filter: end <= 0, bases[d] = n, at most one hit per named
 * sequence.
 * As on the other feeds: a sequence appears at most once per call, pieces may come in any order, a call may name any subset of
 * the sequences, a piece is shorter than 2^31 bytes minus Lmax; a failing call changes nothing, AHA_E_CAPACITY included (*n_hits
 * is then the exact count, the same call with a larger buffer gives what the first would have, the sequences of a finish call
 * have NOT restarted); aha_feed_reset drops the carried state, the pending end with it; calls on one feed are serialised.  On a
 * handle with AHA_OPT_FOLD_ASCII everything the kernels see is the folded text, the two bytes the state carries included.
 * Cedar's stale END flags and NUL bytes (the value node of a key that has children) behave as in the batch call: that is the
 * point of Y(T).
 * Refused, AHA_E_INVALID before any device work, nothing changed, each with its own aha_last_error text: longest outside 0..2;
 * longest != 0 with sep_size > 0, with char_offsets != 0, or with AHA_FEED_CHARS (a follow-up); aha_feed_count_batch*,
 * _cover_, _select_, _replace_ and _grep_ on a longest feed (follow-ups).  The argument checks come before the device check: a
 * host-only handle answers AHA_E_NO_DEVICE for longest = 1 | 2 with valid arguments.  Handles folded beyond ASCII stay refused,
 * with AHA_FEED_FOLD too.
 * Pipeline (aha_amd/csrc/feed.cpp, scan_feedlongest.hip; DESIGN.md 4.10 "Feed match_longest"): match_longest's state at a cut
 * depends on the whole sequence (intersectable = false resets it at every yield), so the feed carries it: 16 bytes per sequence
 * -- the automaton state, the pending end as a distance back from the sequence's end, its key, the last two bytes (all that the
 * shadow fail links ever read in front of the current byte) -- and no context.  A call checks offsets and ids, walks the pieces
 * as the documents of a two-pass batch (count, block scan, write: the batch match_longest's scratch) that start from the carried
 * state and do not flush at their end, one thread per piece, or for longest = 2 and pieces of a chunk or more on average one
 * thread per chunk with the batch kernel's warm-up, and commits the new states once the total is known to fit.
 * aha_ac_last_timing reports what a batch match_longest reports.  Device memory: 40 bytes per sequence; per call 16 bytes per
 * piece beside the batch match_longest's scratch. */
int32_t aha_feed_open_params(aha_ac *ac, uint32_t n_seqs, uint32_t flags, const aha_match_params *params, aha_feed **out);
/* Host buffers (the ids are checked on the host).  Any output array may be NULL; n_named = 0 is valid. */
int32_t aha_feed_finish_batch(aha_feed *f, const uint32_t *seq_ids, uint64_t n_named, aha_hit *out, uint64_t cap,
                              uint64_t *seq_hit_offsets /* n_named+1 or NULL */, uint64_t *bases /* n_named or NULL */,
                              uint64_t *n_hits);
/* Device-resident form: d_ pointers are HBM on the handle's device; *n_hits is host memory; blocks until final. */
int32_t aha_feed_finish_batch_device(aha_feed *f, const uint32_t *d_seq_ids, uint64_t n_named, aha_hit *d_out, uint64_t cap,
                                     uint64_t *d_seq_hit_offsets /* n_named+1 or NULL */,
                                     uint64_t *d_bases /* n_named or NULL */, uint64_t *n_hits, void *stream);

/* ---- document counts: hits per key within each document, no hit list (pure additions to ABI 8) -----------------------
 * The same batch, params, validation and errors as aha_ac_match_batch / _device.  For document d,
 * out[doc_pair_offsets[d] .. doc_pair_offsets[d+1]) holds one pair per distinct `value` among the hits the match call
 * reports for d, ASCENDING BY KEY ID, count = the number of those hits (numpy: np.unique(values, return_counts=True));
 * documents in order; two calls give identical bytes.  count is uint32: a key ends at most once per byte and a document
 * is shorter than 2^31 bytes.  *n_pairs = all pairs; *n_hits (optional) = the match call's hit count.  Summing count per
 * key over all pairs gives aha_ac_count_batch's key_counts, summing it per document the differences of its
 * doc_hit_offsets.  cap is in pairs.  AHA_E_CAPACITY: *n_pairs is the required count, all offsets are valid, the first
 * cap pairs are valid; out == NULL with cap == 0 is a sizing call.  char_offsets changes no count (the byte route); a
 * separator filter counts the filtered hits; longest != 0 is AHA_E_INVALID.  n_pairs == NULL or a NULL handle:
 * AHA_E_INVALID; a host-only handle: AHA_E_NO_DEVICE; the argument checks come before any device work.  The call reads
 * the handle's back-off state and never writes it: a later match call behaves as if it had not happened.
 * Pipeline (aha_amd/csrc/scan_doccount.hip): a count call without key counts (hits per document), the
 * match with cap = hits into the call's scratch, then per document one of three forms chosen from its hit count: a sort
 * in LDS (up to 4096 hits), counting passes over ranges of 8192 key ids in LDS (up to K / 8 hits), a row of K counts in
 * scratch (above).  Device scratch: the match's + 12 bytes per hit (+ 8 per pair of the middle form) + 4 K per dense
 * document in flight (1 GiB at most) + ~40 bytes per document.  Where the hits are beyond 48 GiB the call works through
 * ranges of whole documents one after another (aha_timing.repeats = the ranges before the last); a single document
 * beyond the bound is counted per key instead of matched.  The host entry uploads the batch in one piece.
 * aha_ac_last_timing: engine = the engine that traversed, n_hits, ms_write = the passes after the match.
 * Feeds and groups have no such call yet. */
typedef struct {
  int32_t key;
  uint32_t count;
} aha_key_count;
int32_t aha_ac_doc_counts_batch(aha_ac *ac, const uint8_t *corpus, const uint64_t *doc_offsets, uint64_t n_docs,
                                const aha_match_params *params, aha_key_count *out, uint64_t cap,
                                uint64_t *doc_pair_offsets /* D+1 or NULL */, uint64_t *n_pairs, uint64_t *n_hits /* or NULL */);
/* Device-resident form: d_ pointers are HBM on the handle's device; *n_pairs, *n_hits are host memory; blocks until final. */
int32_t aha_ac_doc_counts_batch_device(aha_ac *ac, const uint8_t *d_corpus, const uint64_t *d_doc_offsets, uint64_t n_docs,
                                       uint64_t n_bytes, const aha_match_params *params, aha_key_count *d_out, uint64_t cap,
                                       uint64_t *d_doc_pair_offsets /* D+1 or NULL */, uint64_t *n_pairs,
                                       uint64_t *n_hits /* or NULL */, void *stream);

/* ---- cover: which bytes lie inside a hit, and a redacted copy, no hit list (pure additions to ABI 8) --------------------
 * The same batch, params, validation and errors as aha_ac_count_batch / _device.
 * mask: bit j of the batch (word j >> 5, bit j & 31) = 1 iff corpus byte j lies in [start, end) of at least one hit that
 * aha_ac_match_batch reports for this batch and these params (byte offsets).  ceil(N / 32) words, every bit >= N is 0.  It
 * is in 32-bit words so that the kernels may use word atomics without touching a byte the caller does not own; read as bytes
 * it is LSB-first (numpy: np.unpackbits(mask.view(np.uint8), bitorder="little")[:N]).
 * redacted[j] = fill where bit j is set, corpus[j] elsewhere.  In the device entry d_redacted == d_corpus is allowed
 * (redaction in place); any other overlap is the caller's error.
 * doc_covered[d] = set bits in document d's range (D entries); *n_covered = their sum; *n_hits (optional) = the match call's
 * hit count.  Any of mask, redacted, doc_covered may be NULL; with all three NULL the call still gives the two totals.
 * n_covered == NULL, a NULL handle, unknown flag bits (flags is 0): AHA_E_INVALID; sep_size > 256: AHA_E_SEP_SIZE;
 * longest != 0: AHA_E_INVALID (a follow-up); a host-only handle: AHA_E_NO_DEVICE; all before any device work.
 * char_offsets changes nothing (the byte route, as for counts).  A separator filter covers the hits that survive it.  No
 * capacity, so no AHA_E_CAPACITY.  A call that fails writes none of the caller's buffers.  Threading (a call leases a scratch
 * set), the device-side checking of d_doc_offsets and the host entry's staging are those of the count and document-count
 * entries (the host entry uploads the batch in one piece and redacts it in place there).  Like a count call it reads the
 * handle's back-off state and never writes it.  N = 0, D = 0 and empty documents are valid.  Hits never cross a document
 * boundary, so neither does a span.  Two calls give identical bytes.
 * Pipeline (aha_amd/csrc/scan_cover.hip): all hits of one END position end at the same byte and the first --
 * the END state's own key -- is the longest, so the union of the hits' spans is the union of one span per event.  The call
 * is a count call without key counts (the engine a match would take, full-size event regions, document ranges where they do
 * not fit: aha_timing.repeats) whose events each OR [end - len(head key), end) into the mask: a bit tile in LDS per group of
 * chunks, vector atomicOr for what lies outside it.  A separator filter and keys beyond 4096 bytes take the two-pass engine's
 * counting traversal, where the first key on an event's chain that passes the left-neighbour test gives the span.  Then a
 * streaming pass writes redacted and popcounts give doc_covered and the total, each only when asked for.
 * Device scratch: the count call's + N / 8 bytes when the caller gives no mask + 8 bytes per chunk; NOTHING proportional to
 * the hits (a match of a dense batch holds 16 bytes per hit of capacity).  The host entry stages the corpus, the offsets, the
 * mask and the D counts on the device as well.
 * aha_ac_last_timing: engine = the engine that traversed, n_hits, ms_write = the passes after the traversal.
 * Feeds: aha_feed_cover_batch* below.  Out of scope so far: groups, coverage of match_longest, masks indexed by character. */
int32_t aha_ac_cover_batch(aha_ac *ac, const uint8_t *corpus, const uint64_t *doc_offsets, uint64_t n_docs,
                           const aha_match_params *params, uint32_t flags /* 0 */, uint32_t *mask /* ceil(N/32) words or NULL */,
                           uint8_t *redacted /* N bytes or NULL */, uint8_t fill, uint64_t *doc_covered /* D or NULL */,
                           uint64_t *n_covered, uint64_t *n_hits /* or NULL */);
/* Device-resident form: d_ pointers are HBM on the handle's device; *n_covered, *n_hits are host memory; blocks until final. */
int32_t aha_ac_cover_batch_device(aha_ac *ac, const uint8_t *d_corpus, const uint64_t *d_doc_offsets, uint64_t n_docs,
                                  uint64_t n_bytes, const aha_match_params *params, uint32_t flags, uint32_t *d_mask,
                                  uint8_t *d_redacted, uint8_t fill, uint64_t *d_doc_covered /* D or NULL */,
                                  uint64_t *n_covered, uint64_t *n_hits /* or NULL */, void *stream);

/* ---- select: leftmost-longest, non-overlapping hits per document (pure additions to ABI 8) ------------------------------
 * The same batch, validation and errors as aha_ac_match_batch / _device.  H_d = the hits that aha_ac_match_batch reports
 * for document d with the same params (byte offsets; a separator filter is allowed) on the same handle (AHA_OPT_FOLD_ASCII
 * included).  The selection S_d: p = 0; among the hits of H_d with start >= p take those with the smallest start, of these
 * the one with the largest end (keys are distinct: it is unique); emit it, p = its end; repeat until no hit has start >= p.
 * out[doc_sel_offsets[d] .. doc_sel_offsets[d+1]) = S_d, ascending by start, no two hits overlap, each an aha_hit
 * {start, end, value} relative to the document exactly as the match writes it; documents in order; two calls give identical
 * bytes.  A selected hit need not be the first hit at its end: keys ab, bcd, cd, d over "abcd" give (0,2,ab), (2,4,cd).
 * *n_selected = all selected hits; *n_hits (optional) = the match call's hit count.  cap is in hits.
 * AHA_E_CAPACITY: *n_selected is the required count and NONE of the caller's buffers is written (out == NULL with cap == 0
 * is a sizing call).  Every failing call leaves the caller's buffers untouched.
 * params->char_offsets != 0, params->longest != 0, any flag bit but the token bits below, n_selected == NULL, a NULL handle:
 * AHA_E_INVALID; sep_size > 256: AHA_E_SEP_SIZE; a host-only handle: AHA_E_NO_DEVICE; all before any device work.  Bad
 * offsets: AHA_E_INVALID / AHA_E_TOO_LONG (the device entry finds them on the device).  N = 0, D = 0 and empty documents are
 * valid.  Like the count, cover and document-count calls it reads the handle's back-off state and never writes it.
 * Pipeline (aha_amd/csrc/scan_select.hip): a count call without key counts (hits per document), the match
 * with cap = hits into the call's scratch, then over the hit list: L[p] = the longest hit that starts at text byte p (a
 * 64-bit atomicMax of len << 32 | value per hit), a cover mask (the union of the longest spans is the union of all hits) and
 * a document-start mask, one walker per run (a maximal covered stretch inside one document: the greedy rule never jumps over
 * an uncovered byte or a document start, so runs are independent; within a run the walk is sequential), the rank of the
 * select mask (the documents' offsets, the total), and the emit once the total is known to fit.
 * Device scratch: the count call's and the match's + 12 bytes per hit + 8 bytes per text byte + 3 N / 8 bytes of masks
 * + N / 256 + 16 bytes per document.  Where the hits are beyond 48 GiB (AHA_SELECT_HIT_BYTES, read when the handle is
 * compiled) the call works through ranges of whole documents (aha_timing.repeats = the ranges before the last; a document
 * beyond the bound is a range of its own) -- twice, since nothing is written before the total is known.
 * aha_ac_last_timing: engine = the engine of the match, n_hits = all hits, ms_write = everything after the match.
 * Out of scope so far: char offsets, groups (the substituted copy: the replace calls below; sequences in pieces: the feed
 * select calls below). */
int32_t aha_ac_select_batch(aha_ac *ac, const uint8_t *corpus, const uint64_t *doc_offsets, uint64_t n_docs,
                            const aha_match_params *params, uint32_t flags /* 0 or AHA_SELECT_* */, aha_hit *out, uint64_t cap,
                            uint64_t *doc_sel_offsets /* D+1 or NULL */, uint64_t *n_selected, uint64_t *n_hits /* or NULL */);
/* Device-resident form: d_ pointers are HBM on the handle's device; *n_selected, *n_hits are host memory; blocks until final. */
int32_t aha_ac_select_batch_device(aha_ac *ac, const uint8_t *d_corpus, const uint64_t *d_doc_offsets, uint64_t n_docs,
                                   uint64_t n_bytes, const aha_match_params *params, uint32_t flags, aha_hit *d_out, uint64_t cap,
                                   uint64_t *d_doc_sel_offsets /* D+1 or NULL */, uint64_t *n_selected,
                                   uint64_t *n_hits /* or NULL */, void *stream);

/* ---- tokens: dictionary segmentation (forward maximum matching) of every document, through the select entries -----------
 * No entry point of their own: the two select calls above with AHA_SELECT_TOKENS in flags.  flags == 0 is select as it was.
 * AHA_SELECT_GAP_RUNS without AHA_SELECT_TOKENS, bits 1 and 2 and every other bit: AHA_E_INVALID, like every refusal of
 * select (char_offsets, longest, NULL arguments, a host-only handle ...), all before any device work.
 * For document d with bytes b[0..n) -- the CALLER's bytes, also on a folded handle -- and the selection S_d exactly as the
 * flag-less call reports it on the same handle with the same params (a separator filter is allowed):
 *   - position p is INSIDE when start <= p < end for some hit of S_d;
 *   - p is a TOKEN START iff (a) p is the start of a hit of S_d, or (b) p is not inside and p == 0, or p - 1 is inside, or --
 *     without AHA_SELECT_GAP_RUNS only -- (b[p] & 0xC0) != 0x80 (the lead-byte rule of AHA_FEED_CHARS);
 *   - a token runs from its start to the next token start, to n for the last one;
 *   - value = the key index for a token of kind (a), whose end is the hit's end; -1 for kind (b).
 * So a token is the longest key that starts here or, where none starts, one character; with AHA_SELECT_GAP_RUNS a whole gap
 * between two selected hits is ONE token.  The rule is bytewise and total: invalid UTF-8 is legal input, a stray run of
 * continuation bytes joins the token in front of it, a document cut in the middle of a character starts a token there, and so
 * does a hit that starts on a continuation byte (byte-level keys).  The tokens of a non-empty document partition it: the
 * first starts at 0, each ends where the next starts, the last ends at n; an empty document has none.
 * out[doc_sel_offsets[d] .. doc_sel_offsets[d+1]) = the tokens of document d as {start, end, value} relative to it, documents
 * in order; *n_selected = all tokens, cap is in tokens, *n_hits = the match's hit count.  AHA_E_CAPACITY, the sizing call
 * (out == NULL, cap == 0), "a failing call writes none of the caller's buffers", determinism, threading and neutrality
 * towards the handle's back-off state are select's.  A batch without any hit is still tokenized; D = 0, N = 0 and batches
 * of empty documents succeed with 0 tokens.
 * Pipeline (aha_amd/csrc/scan_tokens.hip, DESIGN.md 4.14 "Tokens"): select's passes up to the walk; S = the selected spans
 * ORed into a mask; T = the token starts, per mask word from the select, S and document-start words and the word's 32 text
 * bytes (aha_amd/csrc/token_rule.hpp); the rank of T; the emit, in which a token's start and value come from its own bit and
 * its end from the next one.  Device scratch: select's + 2 N / 8 bytes (S, T), nothing per token.  The ranges of whole
 * documents tile ALL documents here, hits or none, and a range holds at most AHA_SELECT_HIT_BYTES bytes of hits and at most an
 * eighth as many bytes of text (8 bytes of scratch per text byte; a document beyond either is a range of its own); a range
 * without a hit is not matched.
 * aha_ac_last_timing: as for select; ms_write = everything after the match.
 * Feeds: aha_feed_select_batch* with AHA_FEED_SELECT_TOKENS below.  Out of scope: character offsets, groups, tokens of
 * match_longest, and id remapping for unknown characters, which callers do on the value column. */
#define AHA_SELECT_TOKENS   4u  /* out receives the tokens of every document instead of the selection */
#define AHA_SELECT_GAP_RUNS 8u  /* only with AHA_SELECT_TOKENS: a gap is ONE token, not one per character */

/* ---- replace: the substituted copy of a batch, built on the device (pure additions to ABI 8) --------------------------------
 * The same batch, params, validation and errors as aha_ac_select_batch / _device; S_d = the selection of document d as those
 * calls report it (AHA_OPT_FOLD_ASCII included; a separator filter is allowed; offsets are bytes).
 * A replacement table (aha_repl) gives for every key k of ONE handle either a byte string R_k -- blob[offsets[k] ..
 * offsets[k+1]); it may be empty (deletion) and may hold NUL bytes -- or "keep" (bit k of keep_bits).  aha_repl_create
 * validates and uploads once: a NULL handle / offsets / out, offsets[0] != 0, descending offsets, one replacement of 2^32 bytes
 * or more: AHA_E_INVALID, *out stays NULL.  On a host-only handle the table is made with a host copy only.  A table is
 * immutable (concurrent calls may share it) and may be freed before or after its handle; aha_repl_free(NULL) is a no-op.
 * The result of document d: its text with every hit of S_d whose key is not kept replaced by R_value; kept hits stay as they
 * are and still take part in the selection -- the table never changes S_d.  On a folded handle the bytes outside replaced hits
 * are the caller's, not the folded copy's (the rule of redact).
 * out = the documents' results one behind the other, doc_out_offsets[0 .. D] where each lies, *n_out_bytes the total;
 * *n_selected, *n_hits (optional) as select reports them.  cap_bytes is in bytes.  AHA_E_CAPACITY: *n_out_bytes is the
 * required size (*n_selected and *n_hits are set too, by both entries) and NONE of the caller's buffers is written -- out,
 * doc_out_offsets, the bytes behind cap_bytes (out == NULL with cap_bytes == 0 is a sizing call; a total of 0 succeeds with
 * cap_bytes == 0).  Every failing call leaves the caller's buffers untouched.  Two calls give identical bytes.
 * params->char_offsets != 0, params->longest != 0, any flag bit, n_out_bytes == NULL, a NULL handle or table, a table made for
 * another handle, out overlapping the corpus (the device entry: its address ranges, when cap_bytes > 0; there is no in-place
 * form): AHA_E_INVALID; a host-only handle: AHA_E_NO_DEVICE; all before any device work.  Bad offsets as in select.  N = 0,
 * D = 0, empty documents and documents without a hit are valid.  The handle's back-off state is read and never written.
 * d_out and d_corpus may have any alignment: no load touches an aligned 16-byte piece without a byte of the corpus or of the
 * blob, no store a byte outside [out, out + total).  Documents stay below 2 GiB; output offsets are 64-bit.
 * Pipeline (aha_amd/csrc/scan_replace.hip): select into the call's scratch (one count and one match per
 * document range, as select itself); per selected hit j its first corpus byte A[j] and its change of length delta[j]; a
 * device-wide exclusive scan shift = scan(delta), signed 64-bit; the documents' output offsets doc_offsets[d] + shift[first
 * selected hit of d]; the total comes to the host; once it fits, the copy, driven by the output: a wave owns 1024 output bytes,
 * a lane 16; the segment of an output position q is the last j with A[j] + shift[j] <= q (deletions make ties); a tile inside
 * one gap is two aligned 16-byte loads, a byte alignment and one aligned 16-byte store per lane, any other tile is walked
 * segment by segment.
 * Device scratch: select's + per selected hit 12 bytes of selection, 8 of A, 8 of shift, the scan's block sums (8 bytes per
 * 256 selected hits) + 8 bytes per document; nothing per text byte beyond select's.  AHA_REPLACE_BLOCKS (read when the handle
 * is compiled) caps the scan's and the copy's grids.
 * aha_ac_last_timing: as select; ms_write = everything after the match.
 * Out of scope so far: replacements indexed by character, groups, an in-place form, computed replacements.  (The substituted
 * stream of sequences in pieces: the feed replace calls below.) */
typedef struct aha_repl aha_repl;
int32_t aha_repl_create(aha_ac *ac, const uint8_t *blob, const uint64_t *offsets /* K+1, offsets[0] == 0, ascending */,
                        const uint32_t *keep_bits /* ceil(K/32) words, bit k = keep key k; NULL: none kept */, aha_repl **out);
void aha_repl_free(aha_repl *table);
int32_t aha_ac_replace_batch(aha_ac *ac, const aha_repl *table, const uint8_t *corpus, const uint64_t *doc_offsets, uint64_t n_docs,
                             const aha_match_params *params, uint32_t flags /* 0 */, uint8_t *out, uint64_t cap_bytes,
                             uint64_t *doc_out_offsets /* D+1 or NULL */, uint64_t *n_out_bytes,
                             uint64_t *n_selected /* or NULL */, uint64_t *n_hits /* or NULL */);
/* Device-resident form: d_ pointers are HBM on the handle's device; *n_out_bytes, *n_selected, *n_hits are host memory; blocks
 * until final. */
int32_t aha_ac_replace_batch_device(aha_ac *ac, const aha_repl *table, const uint8_t *d_corpus, const uint64_t *d_doc_offsets,
                                    uint64_t n_docs, uint64_t n_bytes, const aha_match_params *params, uint32_t flags /* 0 */,
                                    uint8_t *d_out, uint64_t cap_bytes, uint64_t *d_doc_out_offsets /* D+1 or NULL */,
                                    uint64_t *n_out_bytes, uint64_t *n_selected /* or NULL */, uint64_t *n_hits /* or NULL */,
                                    void *stream);

/* ---- records and grep: split a batch into records, keep those with a hit (pure additions to ABI 8) -----------------------
 * RECORDS.  The same batch as aha_ac_match_batch / _device and a delimiter byte.  E = {doc_offsets[d] : 1 <= d <= D} united
 * with {p + 1 : corpus[p] == delim}, without 0.  rec_offsets[0 .. R] = 0 followed by the elements of E, ascending, without
 * repeats; *n_records = R.  So every record is non-empty; it ends behind a delimiter (the delimiter belongs to its record)
 * or at a document's end; a document boundary behind a delimiter is counted once; empty documents have no record.
 * doc_rec_offsets[d] (optional, D + 1 entries) = the elements of E that are <= doc_offsets[d]: document d's records are
 * rec_offsets[doc_rec_offsets[d] .. doc_rec_offsets[d+1]].  rec_offsets is a valid doc_offsets for every batch call of this
 * header: it starts at 0, ascends and ends at N -- records are documents from then on (select per line, grep below).
 * cap_records is in records: the buffer holds cap_records + 1 entries.  AHA_E_CAPACITY: *n_records is the required count and
 * NONE of the caller's buffers is written (rec_offsets == NULL with cap_records == 0 is a sizing call).  N = 0: R = 0,
 * rec_offsets[0] = 0 is written where a buffer is given, doc_rec_offsets is all zero.  A record of 2 GiB or more is not this
 * call's business: the match that follows answers AHA_E_TOO_LONG.
 * A NULL handle / doc_offsets / n_records, rec_offsets == NULL with cap_records != 0, any flag bit (flags is 0):
 * AHA_E_INVALID; a host-only handle: AHA_E_NO_DEVICE; all before any device work.  Bad offsets as in the match (the device
 * entry finds them on the device).  The handle's key set plays no part: the call uses its device, scratch and stream.
 * d_corpus may have any alignment; no load touches a byte outside [corpus, corpus + N).
 * Pipeline (aha_amd/csrc/scan_grep.hip): one pass over the text with aligned 16-byte loads writes a record-end
 * mask, one bit per byte; one lane per document ORs the documents' ends in; the mask is ranked as select's (set bits per 64
 * words, their scan, the rank of every document's first byte); the total comes to the host; once it fits, every set bit p
 * writes rec_offsets[rank + 1] = p + 1.  Device scratch: N / 8 bytes of mask + 8 bytes per 2048 text bytes.
 *
 * GREP.  The same batch, params, validation and errors as aha_ac_count_batch / _device.  h_d = the hits aha_ac_match_batch
 * reports for document d with the same params on the same handle (a separator filter -- whole-word grep -- and
 * AHA_OPT_FOLD_ASCII included).  Document d is KEPT when (h_d >= 1) != invert (flags & AHA_GREP_INVERT).
 * kept_docs[0 .. n_kept) (optional) = the kept documents' indices, ascending; doc_out_offsets[0 .. n_kept] (optional) = where
 * each lies in out; out (optional) = the kept documents' bytes one behind the other -- the caller's own bytes, on a folded
 * handle the original spelling (the rule of redact and replace); *n_kept, *n_out_bytes (optional), *n_hits (optional; all
 * hits of the batch).  Kept empty documents appear in kept_docs with equal neighbouring offsets (under AHA_GREP_INVERT).
 * cap_docs bounds both per-document buffers (doc_out_offsets holds cap_docs + 1), cap_bytes bounds out.  AHA_E_CAPACITY
 * when n_kept > cap_docs and either per-document buffer was given, or when n_out_bytes > cap_bytes and out was given: BOTH
 * required numbers are reported and NONE of the caller's buffers is written.  Every failing call leaves them untouched.
 * All three buffers NULL with capacities 0 is a sizing call that succeeds; out == NULL with cap_bytes == 0 never launches
 * the copy (the "which documents" and "how many" forms).  Two calls give identical bytes.
 * params->char_offsets != 0, params->longest != 0, an unknown flag, n_kept == NULL, a NULL handle, a NULL buffer with a
 * non-zero capacity, out overlapping the corpus (there is no in-place form): AHA_E_INVALID; a host-only handle:
 * AHA_E_NO_DEVICE; all before any device work.  N = 0, D = 0 and empty documents are valid.  The handle's back-off state is
 * read and never written, as in the count call.
 * Example: keys "ab", "b\n" over the one document "xab\nq\n\nb" with delimiter '\n'.  Records gives rec_offsets
 * 0, 4, 6, 7, 8: the records "xab\n", "q\n", "\n", "b".  Grep over rec_offsets keeps record 0 only: kept_docs = {0},
 * doc_out_offsets = {0, 4}, out = "xab\n".  The key "b\n" anchors at a record's end: it hits in "xab\n" and does not hit in the
 * last record, which has no delimiter.  With AHA_GREP_INVERT: kept_docs = {1, 2, 3}, out = "q\n\nb".
 * Pipeline (scan_grep.hip): the count call without key counts (hit offsets per document into scratch); one lane
 * per document writes three masks over documents -- keep, S (a dropped document whose predecessor is kept or which is the
 * first) and T (a dropped document whose successor is kept or which is the last); the three are ranked as above; the j-th bit
 * of S and the j-th bit of T delimit the j-th maximal run of dropped documents, so A[j] = doc_offsets[a_j] and delta[j] =
 * -(doc_offsets[b_j + 1] - A[j]) without a walk along the run; replace's scan gives shift, n_out_bytes = N + shift[n_runs];
 * both totals come to the host; once they fit, kept document d of rank r writes kept_docs[r] = d and doc_out_offsets[r] =
 * doc_offsets[d] + shift[runs in front of d], and replace's copy (above) runs over the dropped runs as deleted hits.
 * Device scratch beside the count call's: 8 bytes per document of hit offsets, 3 bits per document of masks and their block
 * ranks, 28 bytes per dropped run and the scan's block sums.  AHA_GREP_BLOCKS (read when the handle is compiled) caps the grids
 * of these calls' kernels, the reused rank, scan and copy launches included.
 * aha_ac_last_timing (grep): engine = the engine that traversed, n_hits = all hits, ms_write = everything after the count.
 * The host entries stage the batch on the device; a host sizing call followed by the real call runs the device work twice.
 * Out of scope so far: char offsets, match_longest, groups, multi-byte delimiters, an in-place form (feeds:
 * aha_feed_grep_batch* below; the hits in their context instead of whole documents: EXCERPTS below).
 *
 * RULE GREP (AHA_GREP_RULE, flag 4, combinable with AHA_GREP_INVERT: flags 5; 2 and 3 stay refused).  `params` points to an
 * aha_grep_params whose first member is the call's aha_match_params with match.struct_size = sizeof(aha_grep_params); the
 * documents are kept by a rule over their CLASS COUNTS (aha_ac_class_counts_batch* below) instead of "at least one hit".
 * count[d][c] = what aha_ac_class_counts_batch writes for the same batch, match params, handle and class table (a separator
 * filter and a folded handle included); len_d = doc_offsets[d+1] - doc_offsets[d].  A term is
 *   den_bytes == 0:  count[d][class_id] OP num
 *   den_bytes  > 0:  (uint64)count[d][class_id] * den_bytes OP (uint64)num * len_d     ("num hits per den_bytes bytes")
 * with OP >= (AHA_RULE_GE) or < (AHA_RULE_LT); both products fit 64 bits (counts are below 2^32, documents below 2^31
 * bytes); an empty document follows the formula (0 >= 0 holds, 0 < 0 does not).  A document PASSES when some `group` value has
 * all its terms true: OR over groups, AND inside a group; group ids are arbitrary and terms need not be sorted.  Document d is
 * KEPT when passes(d) != invert.  Everything else is grep's contract above, word for word: kept_docs, doc_out_offsets, out,
 * cap_docs, cap_bytes, AHA_E_CAPACITY with both required numbers and nothing written, out == NULL never launches the copy,
 * *n_hits = all hits of the batch, two calls give identical bytes, the handle's back-off state is read and never written.
 * rows (optional): the D x C table itself, as class counts writes it -- host memory in the host entry, HBM in the device
 * entry; every entry is written and nothing outside it, and nothing on a capacity failure.  terms is host memory in both
 * entries (it travels as a kernel argument).
 * AHA_E_INVALID before any device work and with every buffer untouched: match.struct_size < sizeof(aha_grep_params), a NULL
 * table or a table made for another handle, NULL terms, n_terms == 0 or n_terms > 64, reserved != 0, an op above 1, a
 * class_id >= the table's n_classes, and everything grep refuses; a host-only handle answers AHA_E_NO_DEVICE after these.
 * Without AHA_GREP_RULE the call is the one above, whatever struct_size says.
 * Where rows is NULL the table lives in device scratch, at most AHA_RULE_TABLE_BYTES (read when the handle is compiled;
 * default 1 GiB): a batch whose D x C x 4 exceeds it fails with AHA_E_TOO_LARGE and writes nothing (give rows, or smaller
 * batches).  In the device entry rows takes the table at once only where no capacity can fail the call any more (cap_docs >= D
 * or no per-document buffer, cap_bytes >= N or no out); otherwise the table is built in the same bounded scratch and copied
 * into rows once the call is known to fit.
 * Example: the class-counts example below -- keys "he", "she", "hers" with classes {0}, {0, 1}, {} over the documents "ushers"
 * and "he" -- has the rows {2, 1} and {1, 0}.  The rule {c0 >= 2} keeps document 0; {c0 >= 1 AND c1 < 1} keeps document 1;
 * {c0 >= 1 per 3 bytes} keeps both (2 * 3 >= 1 * 6 and 1 * 3 >= 1 * 2).
 * Pipeline (scan_greprule.hip, DESIGN.md 4.16 "Rule grep"): the class-counts call as it is, into rows or scratch; kgq_keep, a
 * wave per 64 documents, stages the columns the rule names through LDS, 32 at a time, evaluates the rule (a kernel argument)
 * and writes the keep mask by ballot; kgq_edges, a lane per mask word, derives S and T from keep alone; then grep's tail above,
 * unchanged.  aha_ac_last_timing: engine, n_hits and repeats as class counts reports them, ms_write = everything after the
 * class-counts call's match.
 * Out of scope so far: weighted sums and comparisons between two classes, tables restricted to the classes a rule names,
 * slabs of documents, feeds, groups, char offsets, match_longest, a rule object on the device.
 *
 * EXCERPTS (AHA_GREP_CONTEXT, flag 8, alone: flags == 8 exactly).  The text around every hit, cut out on the device: `before`
 * bytes in front of every hit and `after` bytes behind it, neighbouring contexts merged into one piece and nothing else copied
 * (grep -o with a byte context, keyword in context, a search-result snippet).  `params` points to an aha_excerpt_params whose
 * first member is the call's aha_match_params with match.struct_size = sizeof(aha_excerpt_params).
 * Document d is the bytes [a, b) of the corpus; H_d = the hits aha_ac_match_batch reports for d with the same match params on
 * the same handle, in byte offsets (a separator filter and every fold option included).  For a hit (start, end) of H_d, in
 * 64-bit arithmetic:
 *   w0 = snapL(max(a, a + start - before))        w1 = snapR(min(b, a + end + after))
 *   snapL(x): at most three times, if x > a and (corpus[x] & 0xC0) == 0x80 then x -= 1
 *   snapR(x): at most three times, if x < b and (corpus[x] & 0xC0) == 0x80 then x += 1
 * The rule is bytewise and reads the caller's own bytes.  On valid UTF-8 no excerpt begins or ends inside a character; on
 * anything else the rule is still defined, and a run of stray continuation bytes moves an edge by at most 3.
 * E = the union of all [w0, w1).  The EXCERPTS are the maximal intervals of E that lie inside one document: windows of one
 * document that overlap or touch ([x, y) and [y, z)) are one excerpt; two excerpts that meet at a document boundary stay two.
 * They are numbered in ascending position, r = 0 .. R-1, [p_r, q_r).  In grep's parameters:
 *   kept_docs[r]        p_r, the excerpt's first byte as an offset into the corpus (not into its document), ascending
 *   doc_out_offsets[r]  where excerpt r lies in out; entry R is the total
 *   out                 the excerpts' bytes one behind the other -- the caller's bytes, on a folded handle the original spelling
 *   *n_kept = R, *n_out_bytes = the sum of q_r - p_r, *n_hits = all hits of the batch
 * Everything else is grep's contract word for word: cap_docs and cap_bytes bound the buffers, AHA_E_CAPACITY reports both
 * required numbers and writes none of the caller's buffers, the sizing call succeeds, out == NULL never launches the copy, two
 * calls give identical bytes, N = 0, D = 0 and empty documents are valid, the handle's back-off state is read and never
 * written, aha_ac_last_timing reports ms_write as everything after the count.  The document of excerpt r is the d with
 * doc_offsets[d] <= p_r < doc_offsets[d+1] (excerpts are never empty, so the search is unambiguous); the library does not
 * compute it on the device.  rec_offsets of aha_ac_records_batch* are valid doc_offsets: contexts clipped to lines.
 * AHA_E_INVALID before any device work, with every buffer and every count untouched: flags that contain AHA_GREP_CONTEXT
 * together with any other bit, match.struct_size < sizeof(aha_excerpt_params), params == NULL, the struct's own flags != 0 or
 * reserved != 0, before or after above 0x7FFFFFFF, and everything plain grep refuses.  A bad sep_size answers
 * AHA_E_SEP_SIZE; a host-only handle answers AHA_E_NO_DEVICE after all of these.  Without the flag the two entry points
 * behave exactly as above, whatever struct_size says.
 * Examples.
 *   1. Key "ab"; documents "xxabxxxxabx" and "ab" (offsets 0, 11, 13).  before = 1, after = 2: the windows are [1,6), [7,11)
 *      and [11,13); starts {1, 7, 11}, out = "xabxx" "xabx" "ab", offsets {0, 5, 9, 11}, n_hits = 3 -- the second and third
 *      excerpts touch at the document boundary and stay two.  before = 1, after = 3: [1,7) and [7,11) touch inside one
 *      document and merge; starts {1, 11}, out = "xabxxxxabx" "ab".
 *   2. Key U+662F over the single document U+6211 U+662F U+4E2D (9 bytes, hit [3,6)), before = after = 1: w0 goes 2 -> 1 -> 0
 *      and w1 goes 7 -> 8 -> 9: one excerpt, the whole document.
 *   3. before = after = 0: the excerpts are the maximal covered runs of the cover call, split at document boundaries;
 *      n_out_bytes equals the cover call's n_covered.
 *   4. before = after = 0x7FFFFFFF: the excerpts are exactly the non-empty documents plain grep keeps; out equals grep's out
 *      and the starts equal doc_offsets[kept_docs].
 * Pipeline (aha_amd/csrc/scan_excerpt.hip, DESIGN.md 4.16 "Excerpts"): the count call with a cover mask M in scratch; a lane
 * per mask word writes S and T (a covered run starts / ends at the bit), a lane per inner document boundary splits the runs
 * that cross it; both are ranked as select's masks; the j-th bits delimit run j, whose document (a binary search), w0 and w1
 * (excerpt_window.hpp, at most six text bytes) are written; first[j] = j is the first run of its document or w0[j] >
 * w1[j-1], last[j] the same seen from j + 1, by wave ballot, ranked again; the R + 1 stretches outside the excerpts become
 * deleted hits for replace's scan and copy; the verdict is given on the host before anything is written.  No pass looks at a
 * hit: the snaps are monotone, so a run's window is the union of its hits' windows.
 * Device scratch beside the count call's: N / 8 bytes for M, 2 N / 8 for S and T and 16 bytes per 2048 text bytes for their
 * block ranks; 24 bytes and 2 bits per run and their block ranks; 28 bytes per excerpt and the scan's block sums.
 * AHA_GREP_BLOCKS caps the grids.
 * Out of scope so far: contexts counted in characters or in lines (whole neighbouring records: CONTEXT LINES below), a
 * separator string between excerpts, combining with AHA_GREP_RULE or invert, match_longest, char offsets, feeds and groups, the
 * excerpt's document index written on the device, an in-place form.
 *
 * CONTEXT LINES (AHA_GREP_LINES, flag 16, combinable with AHA_GREP_INVERT: flags 16 and 17).  grep -A n, -B n and -C n: the
 * records around a matching record are kept with it, and context never crosses a group (a file).  `params` points to an
 * aha_grep_lines_params whose first member is the call's aha_match_params with match.struct_size =
 * sizeof(aha_grep_lines_params).  group_offsets and is_match are host memory in the host entry and HBM in the device entry.
 * The call's "documents" are the records r = 0 .. D-1; any doc_offsets is allowed, not only lines.  The records
 * [group_offsets[g], group_offsets[g+1]) form group g of G; the doc_rec_offsets that aha_ac_records_batch* writes is a valid
 * group_offsets with G = the number of documents, which is the intended use.  NULL means one group, [0, D).  Empty groups are
 * allowed and hold nothing; n_groups may exceed D + 1.  Empty records count as records.
 *   m_r = (h_r >= 1) != invert: exactly plain grep's keep for the same params, flags and handle (a separator filter and every
 *   fold option included).  Record r of group [lo, hi) is KEPT when some s in that group has m_s and r - after <= s <= r + before,
 *   in 64-bit arithmetic.  Stated from the match: m_s keeps [max(lo, s - before), min(hi, s + 1 + after)).
 * Everything else is grep's contract word for word: kept_docs holds the ascending indices, doc_out_offsets[0 .. n_kept] and out
 * the kept records' own bytes (the original spelling on a folded handle); cap_docs, cap_bytes, the sizing call and
 * AHA_E_CAPACITY with both required numbers and nothing written -- is_match included -- behave as in grep; out == NULL never
 * launches the copy; *n_hits = all hits of the batch; two calls give identical bytes; N = 0 and D = 0 are valid; the handle's
 * back-off state is read and never written; aha_ac_last_timing reports ms_write as everything after the count.
 * is_match (optional, cap_docs entries): is_match[i] = m of record kept_docs[i], grep's ':' against '-'.  It is written only
 * where the call fits, and a non-NULL is_match counts as a per-document buffer in the cap_docs verdict.
 * grep's "--" line is not produced on the device: a chunk ends behind kept record i exactly when kept_docs[i+1] !=
 * kept_docs[i] + 1 or the two lie in different groups.
 * Identities.  before = after = 0 equals plain grep with the same flags byte for byte, with is_match all 1.  before = after =
 * 0x7FFFFFFF with G groups keeps exactly the groups that hold a matching record, whole.  With NULL groups and at least one
 * match every record is kept.
 * AHA_E_INVALID before any device work, with every buffer and every count untouched: flag 16 together with 2, 4, 8 or an
 * unknown bit, params == NULL, match.struct_size < sizeof(aha_grep_lines_params), the struct's flags != 0 or reserved != 0,
 * before or after above 0x7FFFFFFF, group_offsets == NULL with n_groups != 0 or the reverse, is_match != NULL with cap_docs ==
 * 0, and everything plain grep refuses.  A bad sep_size answers AHA_E_SEP_SIZE; a host-only handle answers AHA_E_NO_DEVICE
 * after all of these.  Without the flag the two entry points behave exactly as above, whatever struct_size says.
 * The group offsets are validated on the device before anything indexes with them: first entry 0, ascending (equal neighbours
 * allowed), last entry D; a violation answers AHA_E_INVALID as bad doc_offsets do, and nothing is written.  A group may hold any
 * number of records.
 * Example.  Keys "ab"; the one document "x\nab\ny\nz\nab\nw\n" split by records into six lines (offsets 0, 2, 5, 7, 9, 12,
 * 14); lines 1 and 4 match.  before = 1, after = 0, no groups: kept {0, 1, 3, 4}, is_match {0, 1, 0, 1}, out =
 * "x\nab\nz\nab\n".  The same with group_offsets = {0, 4, 6}: line 3 lies in the other group, so it is not context of line 4:
 * kept {0, 1, 4}.  With AHA_GREP_INVERT, before = after = 0: kept {0, 2, 3, 5}.
 * Pipeline (aha_amd/csrc/scan_greplines.hip, DESIGN.md 4.16 "Context lines"): grep's count and flag passes give m; a lane per
 * mask word writes Sm and Tm (a run of matching records starts / ends at the bit), a lane per inner group boundary splits the
 * runs that cross it; both are ranked; the j-th bits delimit run j, whose group (a binary search) and window are written; the
 * first and last run of every merged window XOR one bit each into a toggle mask of D + 1 bits (two windows of different groups
 * that touch cancel there, and both sides are kept); the toggle mask is ranked and a prefix XOR per word fills the keep mask;
 * rule grep's edges and grep's tail take it from there.  Every lane does O(1) work whatever before and after are.
 * Device scratch beside plain grep's: 4 bits per record of masks, 24 bytes per 2048 records of block ranks, 24 bytes per
 * matching run.  AHA_GREP_BLOCKS caps the grids.
 * Out of scope so far: feeds (aha_feed_grep_batch* has no context lines yet: the follow-up), groups of GPUs, combining with
 * AHA_GREP_RULE or AHA_GREP_CONTEXT, char offsets and match_longest, a separator written on the device, contexts in characters,
 * an in-place form, a copy kernel of grep's own. */
#define AHA_GREP_INVERT 1u /* keep the documents WITHOUT a hit */
#define AHA_GREP_RULE 4u   /* params points to an aha_grep_params; keep = the rule over the class counts (2u is refused) */
#define AHA_GREP_CONTEXT 8u /* params points to an aha_excerpt_params; the result is the excerpts, not documents */
#define AHA_GREP_LINES 16u /* params points to an aha_grep_lines_params; the records around a matching record are kept too */
#define AHA_RULE_GE 0u     /* lhs >= rhs */
#define AHA_RULE_LT 1u     /* lhs <  rhs */
typedef struct aha_classes aha_classes;
typedef struct {
  uint32_t class_id;
  uint16_t op;        /* AHA_RULE_GE | AHA_RULE_LT */
  uint16_t group;     /* the terms of one group are AND-ed, the groups OR-ed */
  uint32_t num;
  uint32_t den_bytes; /* 0: a plain count; else "num per den_bytes bytes" */
} aha_rule_term;      /* 16 bytes */
typedef struct {
  aha_match_params match;     /* first member: match.struct_size = sizeof(aha_grep_params) */
  const aha_classes *classes; /* of this handle */
  const aha_rule_term *terms; /* host memory, in both entries */
  uint32_t n_terms;           /* 1 .. 64 */
  uint32_t reserved;          /* 0 */
  uint32_t *rows;             /* optional D x C table, as class counts writes it: host memory in the host entry, HBM in the
                                 device entry */
} aha_grep_params;
typedef struct {
  aha_match_params match; /* first member: match.struct_size = sizeof(aha_excerpt_params) */
  uint32_t before;        /* bytes of context in front of a hit, 0 .. 0x7FFFFFFF */
  uint32_t after;         /* bytes of context behind a hit,     0 .. 0x7FFFFFFF */
  uint32_t flags;         /* 0 */
  uint32_t reserved;      /* 0 */
} aha_excerpt_params;     /* 64 bytes */
typedef struct {
  aha_match_params match;        /* first member: match.struct_size = sizeof(aha_grep_lines_params) */
  uint32_t before;               /* records of context in front of a matching record, 0 .. 0x7FFFFFFF (grep -B) */
  uint32_t after;                /* records of context behind it,                     0 .. 0x7FFFFFFF (grep -A) */
  uint32_t flags;                /* 0 */
  uint32_t reserved;             /* 0 */
  const uint64_t *group_offsets; /* G + 1 entries or NULL: the records [group_offsets[g], group_offsets[g+1]) form group g */
  uint64_t n_groups;             /* G; 0 with NULL */
  uint8_t *is_match;             /* optional, cap_docs entries: 1 where the kept record matched, 0 where it is context */
} aha_grep_lines_params;         /* 88 bytes: match 0, before 48, after 52, flags 56, reserved 60, group_offsets 64,
                                    n_groups 72, is_match 80 */
int32_t aha_ac_records_batch(aha_ac *ac, const uint8_t *corpus, const uint64_t *doc_offsets, uint64_t n_docs, uint8_t delim,
                             uint32_t flags /* 0 */, uint64_t *rec_offsets /* cap_records + 1 */, uint64_t cap_records,
                             uint64_t *doc_rec_offsets /* D+1 or NULL */, uint64_t *n_records);
/* Device-resident form: d_ pointers are HBM on the handle's device; *n_records is host memory; blocks until final. */
int32_t aha_ac_records_batch_device(aha_ac *ac, const uint8_t *d_corpus, const uint64_t *d_doc_offsets, uint64_t n_docs,
                                    uint64_t n_bytes, uint8_t delim, uint32_t flags /* 0 */,
                                    uint64_t *d_rec_offsets /* cap_records + 1 */, uint64_t cap_records,
                                    uint64_t *d_doc_rec_offsets /* D+1 or NULL */, uint64_t *n_records, void *stream);
int32_t aha_ac_grep_batch(aha_ac *ac, const uint8_t *corpus, const uint64_t *doc_offsets, uint64_t n_docs,
                          const aha_match_params *params, uint32_t flags /* AHA_GREP_INVERT */, uint64_t *kept_docs /* or NULL */,
                          uint64_t *doc_out_offsets /* cap_docs + 1 or NULL */, uint64_t cap_docs, uint8_t *out /* or NULL */,
                          uint64_t cap_bytes, uint64_t *n_kept, uint64_t *n_out_bytes /* or NULL */, uint64_t *n_hits /* or NULL */);
/* Device-resident form: d_ pointers are HBM on the handle's device; *n_kept, *n_out_bytes, *n_hits are host memory; blocks
 * until final. */
int32_t aha_ac_grep_batch_device(aha_ac *ac, const uint8_t *d_corpus, const uint64_t *d_doc_offsets, uint64_t n_docs,
                                 uint64_t n_bytes, const aha_match_params *params, uint32_t flags /* AHA_GREP_INVERT */,
                                 uint64_t *d_kept_docs /* or NULL */, uint64_t *d_doc_out_offsets /* cap_docs + 1 or NULL */,
                                 uint64_t cap_docs, uint8_t *d_out /* or NULL */, uint64_t cap_bytes, uint64_t *n_kept,
                                 uint64_t *n_out_bytes /* or NULL */, uint64_t *n_hits /* or NULL */, void *stream);

/* Class counts: hits per key CLASS within each document, as a dense table.  The K keys of a handle belong to a few lexicons
 * (blocklist categories, PII types, topic word lists) and the caller wants one row of C numbers per document -- the feature
 * matrix of a curation pipeline -- without the hit list, without {key, count} pairs and without a capacity to negotiate: the
 * size of the result, D x C, is known before the call.
 * A class table (aha_classes) names for every key k of ONE handle its classes class_ids[offsets[k] .. offsets[k+1]): none,
 * one or several ("apple" may be a fruit and a company).  aha_classes_create validates and uploads it once; it is immutable
 * (concurrent calls may share it), tied to its handle by that handle's serial number, and may be freed before or after its
 * handle; aha_classes_free(NULL) is a no-op.  AHA_E_INVALID with *out left NULL: a NULL handle / offsets / out, offsets[0]
 * != 0 or descending offsets, n_classes == 0 or n_classes > 65536, a class id >= n_classes, one key's ids not strictly
 * ascending (no class twice for a key), class_ids == NULL with offsets[K] != 0.  On a host-only handle the table is made
 * with a host copy only.
 * The calls take the same batch, params, validation and errors as aha_ac_match_batch / _device.  out holds D x C uint32
 * entries, row-major, C = the table's n_classes:
 *   out[d*C + c] = the number of pairs (h, c) where h is a hit aha_ac_match_batch reports for document d with the same params
 *   on the same handle (a separator filter and AHA_OPT_FOLD_ASCII included) and c is among the classes of h.value.
 * EVERY entry of out[0 .. D*C) is written -- the rows of empty documents, of documents without a hit, and every row when no
 * key has a class are zero -- and nothing outside it.  *n_hits (optional) = all hits of the batch.  Two calls give identical
 * bytes.  The handle's back-off state is read and never written, as in the select call.
 * params->char_offsets != 0, params->longest != 0, any flag bit (flags is 0), a NULL handle / doc_offsets / table, a table made
 * for another handle, out == NULL with D > 0: AHA_E_INVALID, before any device work and with every buffer untouched; a
 * host-only handle: AHA_E_NO_DEVICE.  D = 0 and N = 0 succeed.
 * Counts are uint32.  A class count of a document is at most that document's hit count (a key names a class at most once), so
 * a call whose total hit count is below 2^32 cannot overflow; otherwise the documents' hit counts are looked at and a document
 * with 2^32 hits or more fails the call with AHA_E_TOO_LONG before out is written (aha_amd/csrc/class_overflow.hpp).
 * Example: keys "he", "she", "hers" with classes {0}, {0, 1}, {} and C = 2 over the documents "ushers" and "he": the hits
 * are she, he, hers and he, so out = {2, 1, 1, 0}.
 * Pipeline (aha_amd/csrc/scan_classcount.hip): the count call without key counts (hit offsets per document);
 * out is cleared; per range of whole documents whose hit list stays below AHA_CLASS_HIT_BYTES (read when the handle is
 * compiled; one range as a rule) the match into scratch and kcc_add -- a workgroup takes slices of 2048 consecutive hits, sums
 * a slice in an LDS table of 8192 words where (documents of the slice) x C fits it and flushes the non-zero slots with one
 * global add each, and adds to HBM directly otherwise.  A single document beyond the bound is never matched: a count call
 * over it alone gives its key counts, which go into its row through the table.  Integer adds only: no order shows.
 * Device scratch beside the count call's and the match's: 12 bytes per hit of the range in flight, 8 bytes per document of hit
 * offsets, K x 8 bytes for an oversized document; nothing per text byte or per class.  AHA_CLASS_BLOCKS (read when the handle
 * is compiled) caps the grids of these calls' kernels.
 * aha_ac_last_timing: engine = the engine that traversed, n_hits = all hits, ms_write = everything after the match, repeats =
 * the ranges before the last.  The host entry stages the batch on the device and downloads out.
 * Keeping documents by a rule over their row is grep's business: AHA_GREP_RULE above.
 * Out of scope so far: feeds, groups, weights, accumulating into an existing table, char offsets, match_longest. */
/* (aha_classes is declared above, with aha_grep_params) */
int32_t aha_classes_create(aha_ac *ac, const uint32_t *class_ids /* offsets[K] */,
                           const uint64_t *offsets /* K+1, offsets[0] == 0, ascending */, uint32_t n_classes, aha_classes **out);
void aha_classes_free(aha_classes *table);
int32_t aha_ac_class_counts_batch(aha_ac *ac, const aha_classes *table, const uint8_t *corpus, const uint64_t *doc_offsets,
                                  uint64_t n_docs, const aha_match_params *params, uint32_t flags /* 0 */,
                                  uint32_t *out /* D x n_classes */, uint64_t *n_hits /* or NULL */);
/* Device-resident form: d_ pointers are HBM on the handle's device; *n_hits is host memory; blocks until final. */
int32_t aha_ac_class_counts_batch_device(aha_ac *ac, const aha_classes *table, const uint8_t *d_corpus, const uint64_t *d_doc_offsets,
                                         uint64_t n_docs, uint64_t n_bytes, const aha_match_params *params, uint32_t flags /* 0 */,
                                         uint32_t *d_out /* D x n_classes */, uint64_t *n_hits /* or NULL */, void *stream);

/* Feed cover: the same pieces as aha_feed_match_batch*, and the cover of what a match call of them on a BYTE feed in the same
 * state would report (H_d: the hits of piece d, offsets relative to the piece, start possibly negative), without the hit list.
 * mask: the layout of aha_ac_cover_batch over the batch of pieces; bit j = 1 iff byte j lies in [max(start, 0), end) of a hit
 * of its piece's H_d; every bit >= N is 0.  redacted[j] = fill where bit j is set, else corpus[j] -- the caller's bytes on a
 * folded handle; the device entry allows d_redacted == d_corpus.
 * piece_back[d] = max(0, max over H_d of -start): the bytes immediately in front of the piece, in its sequence, that lie inside
 * a hit ending in this piece.  Every straddling hit reaches up to the cut, so they are one run [-back, 0);
 * 0 <= back <= min(Lmax - 1, bytes of the sequence before the piece); in bytes on char feeds too.
 * piece_covered[d] = the set bits inside piece d; *n_covered = their sum (the back bytes belong to earlier pieces and are not
 * counted).  piece_hit_offsets, piece_bases (chars on a char feed) and *n_hits: what the feed match or count of the same pieces
 * gives.  The feed moves on exactly as a match or count call moves it: the three kinds mix freely on one feed.
 * The stream law: cut a sequence into pieces anywhere, write each piece's redacted behind the previous one, then overwrite the
 * last piece_back bytes already written with fill -- the result is, byte for byte, redacted of aha_ac_cover_batch over the
 * whole sequence as one document (and so for the mask bits).
 * n_covered == NULL, a NULL feed, any flag bit (flags is 0): AHA_E_INVALID; a sequence named twice, bad offsets, an id out of
 * range: AHA_E_INVALID (the device entry finds these on the device); a piece of 2^31 - Lmax bytes or more: AHA_E_TOO_LONG; no
 * capacity, so no AHA_E_CAPACITY.  A call that fails changes nothing -- neither the feed nor a caller buffer; in place, no
 * fill byte is written before the verdict is known.  Any output array may be NULL; N = 0, D = 0 and empty pieces are valid.
 * Two calls on feeds in the same state give identical bytes.  Like count and cover calls it reads the handle's back-off state
 * and never writes it.  No separator filter (a feed opened with one refuses the call: AHA_E_INVALID, the feed unchanged; a
 * follow-up); a longest feed refuses the call too (AHA_E_INVALID, the feed unchanged; a follow-up).
 * Pipeline (feed.cpp, scan_feed.hip; DESIGN.md 4.10 "Feed cover"): with W = Lmax - 1 and W' = min(W, |P|), the head windows
 * are widened to X2 = ctx || P[0 .. min(2 W, |P|)) and P'2 = P[0 .. min(2 W, |P|)) (the window batch: at most 6 W bytes per
 * piece, matched quietly, in bytes); the pieces are covered alone as by aha_ac_cover_batch_device into a mask in feed scratch
 * (aha_ac_last_timing reports this pass); bits [0, W') of every piece are cleared and the spans of the X2 hits that end in the
 * piece are ORed in, clipped to the piece (vector atomics); then the totals, piece_covered, the mask's copy, the new contexts
 * and last the redaction.  Device memory beyond a feed count's: N / 8 bytes of mask and the window batch's hit list (12 bytes
 * per hit of at most 3 W bytes of text per piece) -- nothing per hit of the main pass. */
int32_t aha_feed_cover_batch(aha_feed *f, const uint8_t *corpus, const uint64_t *piece_offsets, const uint32_t *seq_ids,
                             uint64_t n_pieces, uint32_t flags /* 0 */, uint32_t *mask /* ceil(N/32) words or NULL */,
                             uint8_t *redacted /* N bytes or NULL */, uint8_t fill, uint32_t *piece_back /* D or NULL */,
                             uint64_t *piece_covered /* D or NULL */, uint64_t *piece_hit_offsets /* D+1 or NULL */,
                             uint64_t *piece_bases /* D or NULL */, uint64_t *n_covered, uint64_t *n_hits /* or NULL */);
/* Device-resident form: d_ pointers are HBM on the handle's device, validated on the device before anything is indexed with
 * them; *n_covered, *n_hits are host memory; blocks until final. */
int32_t aha_feed_cover_batch_device(aha_feed *f, const uint8_t *d_corpus, const uint64_t *d_piece_offsets,
                                    const uint32_t *d_seq_ids, uint64_t n_pieces, uint64_t n_bytes, uint32_t flags,
                                    uint32_t *d_mask, uint8_t *d_redacted, uint8_t fill, uint32_t *d_piece_back,
                                    uint64_t *d_piece_covered, uint64_t *d_piece_hit_offsets, uint64_t *d_piece_bases,
                                    uint64_t *n_covered, uint64_t *n_hits, void *stream);

/* Feed select: the leftmost-longest, non-overlapping hits of sequences that arrive in pieces (pure additions to ABI 8).  The
 * same pieces as aha_feed_match_batch*, on a BYTE feed.  T = one sequence, every piece since open, reset or a FINAL call,
 * concatenated; S(T) = the selection aha_ac_select_batch reports for T as one document with default params on the same handle
 * (AHA_OPT_FOLD_ASCII included); W = max(Lmax - 1, 0), F(n) = max(0, n - W).  A hit that starts at s ends at or before
 * s + Lmax, so once a sequence is n bytes long every hit with a start below F(n) is known and so is the greedy choice there:
 * the hits of S(T[0..n)) with a start below F(n) belong to S(T') for every extension T' of T, and no later text adds a selected
 * hit in front of F(n).  A hit with a start at or behind F(n) may still lose to a longer key from the same start that only
 * completes later (keys ab, abcde: "ab" reports nothing; "cde" then reports (0,5), as start -2).
 * For piece d, which takes its sequence from n0 to n1 bytes, the call reports the hits of S(T[0..n1)) with a start in
 * [F(n0), F(n1)), ascending by start: out[piece_sel_offsets[d] .. piece_sel_offsets[d+1]), each an aha_hit {start, end, value}
 * with int32 offsets relative to the piece's first byte; start lies in [-W, |P| - W), end may be <= 0 (the hit lay wholly in
 * earlier pieces and only now became final).  piece_bases[d] = n0: absolute = base + relative.  cap is in hits.
 * AHA_FEED_SELECT_FINAL (bit 0 of flags): the pieces of this call are the last of their sequences -- everything settles, the
 * starts in [F(n0), n1) are reported, and those sequences start again from length 0 as after aha_feed_reset.  A piece may be
 * empty: "finish sequence q" is a FINAL call with one empty piece.  Any other flag bit: AHA_E_INVALID.
 * The stream law: cut a sequence anywhere into pieces, empty ones included, feed them in order, the last call with FINAL, turn
 * every reported hit to absolute offsets and concatenate -- the result is S(whole sequence), hit for hit, bit for bit.
 * piece_hold[d] (uint32) = n1 - c, in [0, W], with c = max(end of the last selected hit reported so far for the sequence,
 * F(n1)), absolute: the bytes at the end of the sequence whose fate is still open.  Everything in front of c is final -- inside a
 * reported hit, or in no selected hit ever; 0 after FINAL.  *n_selected = all hits reported by the call; *n_hits (optional) = what
 * aha_feed_match_batch of the same pieces would count.  Any output array may be NULL; N = 0, D = 0 and empty pieces are valid.
 * Validation is that of the other feed entries (a sequence named twice, bad offsets, an id out of range: AHA_E_INVALID; a piece
 * too long: AHA_E_TOO_LONG; the device entry finds these on the device).  n_selected == NULL, a NULL feed, a feed opened with
 * AHA_FEED_CHARS (select is bytes only): AHA_E_INVALID.  AHA_E_CAPACITY: *n_selected is the required count, NONE of the
 * caller's buffers is written and the feed is unchanged; the same call with a larger buffer gives what the first would have
 * (out == NULL with cap == 0 is a sizing call).  Every failing call changes nothing.  Two feeds in the same state give
 * identical bytes.  No separator filter (a feed opened with one refuses the call: AHA_E_INVALID, the feed unchanged; a
 * follow-up); a longest feed refuses the call too (AHA_E_INVALID, the feed unchanged; a follow-up).
 * Mixing: select keeps state per sequence that match, count and cover calls do not maintain (they stay exactly as they are).
 * A select call is valid for a sequence only if every byte of it since open, reset or a FINAL call went through select calls;
 * otherwise AHA_E_INVALID (found on the device, next to the duplicate check; aha_last_error says so) and nothing changes.  Such
 * a sequence is usable for select again from its next aha_feed_reset, which clears the select state too.  Other sequences of
 * the feed are not affected.
 * Pipeline (feed.cpp, scan_feedselect.hip; DESIGN.md 4.10 "Feed select"): the context cannot give back a hit that ends inside
 * it, so the open hits are carried: per sequence a tail of W 64-bit words len << 32 | value -- the longest known hit that
 * starts at each of the last min(W, n) bytes --, the cursor c and the bytes seen by select.  A call runs the window batch and
 * the main pass of a feed match with the true hits into scratch (the main pass is retried once with the exact count where the
 * feed's hit buffer is too small; aha_ac_last_timing reports it; the handle's back-off state is read and never written), lays
 * out the extended positions [F(n0), n1) of every piece, fills L from the tails and the hits (a 64-bit atomicMax per hit; what
 * starts in front of c is ignored), builds the cover and piece-start masks, walks every run as select does but takes no start
 * at or behind the piece's frontier (F(n1), or n1 under FINAL), ranks the select mask (the total comes to the host), and once
 * the total fits emits and commits: the feed's ordinary commit, then the new tails, cursors and piece_hold.
 * Device memory: 8 W + 16 bytes per sequence from the feed's first select call on (a feed that never selects keeps 2 W + 24);
 * per call a feed match's with the hits in feed scratch, + 12 bytes per hit + 8 bytes and 3 bits per extended position (at most
 * N + D W of them) + 40 bytes per piece in the handle's scratch set.  Nothing is proportional to W x hits. */
#define AHA_FEED_SELECT_FINAL 1u /* the pieces named in this call are the last of their sequences */
int32_t aha_feed_select_batch(aha_feed *f, const uint8_t *corpus, const uint64_t *piece_offsets, const uint32_t *seq_ids,
                              uint64_t n_pieces, uint32_t flags, aha_hit *out, uint64_t cap,
                              uint64_t *piece_sel_offsets /* D+1 or NULL */, uint64_t *piece_bases /* D or NULL */,
                              uint32_t *piece_hold /* D or NULL */, uint64_t *n_selected, uint64_t *n_hits /* or NULL */);
/* Device-resident form: d_ pointers are HBM on the handle's device, validated on the device before anything is indexed with
 * them; *n_selected, *n_hits are host memory; blocks until final. */
int32_t aha_feed_select_batch_device(aha_feed *f, const uint8_t *d_corpus, const uint64_t *d_piece_offsets,
                                     const uint32_t *d_seq_ids, uint64_t n_pieces, uint64_t n_bytes, uint32_t flags,
                                     aha_hit *d_out, uint64_t cap, uint64_t *d_piece_sel_offsets /* D+1 or NULL */,
                                     uint64_t *d_piece_bases /* D or NULL */, uint32_t *d_piece_hold /* D or NULL */,
                                     uint64_t *n_selected, uint64_t *n_hits /* or NULL */, void *stream);

/* Feed tokens: dictionary segmentation (AHA_SELECT_TOKENS: forward maximum matching) of sequences that arrive in pieces.  No
 * new entry point: the two feed select entries with AHA_FEED_SELECT_TOKENS (bit 2 of flags) report tokens instead of the
 * selection; AHA_FEED_SELECT_GAP_RUNS (bit 3, only with bit 2) leaves gaps whole instead of cutting them into characters.  The
 * values are those of the batch call's flags.  flags & ~(1 | 4 | 8), or 8 without 4: AHA_E_INVALID before any device work; bit
 * 1 stays refused.  Without bit 2 the entries behave exactly as above.  aha_feed_replace_batch* takes FINAL only.
 * T, S(T), W, F(n) and the select cursor c as for feed select.  A token call IS a select call for the feed's select state: it
 * keeps seen bytes, cursor and tails as a select call with the same FINAL bit does.  Beside them the feed keeps a token cursor
 * t <= c per sequence, 0 at open, at reset and after FINAL: everything in front of t has been reported as tokens, and [t, c) is
 * the front part of a gap token (value -1) that is still open; t == c: none.  A selected hit is a whole token the moment it is
 * reported.  A call takes a sequence from n0 to n1 bytes, finds (c0, t0) and leaves (c1, t1): c1 is the cursor feed select
 * leaves, max(c0, end of the last hit the call settles, F(n1)), n1 under FINAL; S1 = the hits of S(T[0..n1)) with a start in
 * [t0, F(n1)) ([t0, n1) under FINAL), all inside [t0, c1); Tok1 = the tokens the batch rule (aha_ac_select_batch with
 * AHA_SELECT_TOKENS and the call's GAP_RUNS bit) gives for T[t0..c1) as one document under S1, shifted by t0.  c1 is a certain
 * boundary iff the call is FINAL, or GAP_RUNS is set, or c1 is the end of the last hit of S1, or c1 < n1 and
 * (T[c1] & 0xC0) != 0x80.  If c1 is certain the call reports all of Tok1 and t1 = c1; otherwise Tok1 without its last token,
 * and t1 = that token's start (a gap token that ends at c1, and nothing yet says that it ends there).  Tok1 empty: nothing,
 * t1 = t0.  The reported tokens tile [t0, t1).
 * Tokens are aha_hit {start, end, value} relative to the piece's first byte (start may be far below -W: a character whose bytes
 * arrive one by one), value = the key or -1.  piece_bases[d] = n0; piece_hold[d] = n1 - t1 (0 after FINAL; it may exceed W: the
 * select cursor's own hold is not reported by a token call); piece_sel_offsets = the tokens of each piece; *n_selected = the
 * tokens of the call, cap is in tokens; *n_hits as for feed select.
 * The stream laws: cut a sequence anywhere into pieces, empty ones included, feed them through token calls with the same
 * GAP_RUNS bit, the last with FINAL, turn the tokens to absolute offsets and concatenate.  Character mode: the result is the
 * batch token call on the whole sequence as one document, token for token, bit for bit, invalid UTF-8 included.  GAP_RUNS: the
 * same after joining -1 tokens that touch -- a gap is handed out up to c1 at every call and never held (the batch call never
 * has two gap tokens that touch, so the join is unambiguous).
 * Examples (absolute offsets).  Keys ab (0), abcde (1), W = 4: "xab" -> [], hold 3; "cd" -> [(0,1,-1)] (relative (-3,-2,-1)),
 * hold 4; "eab" -> [(1,6,1)], hold 2; FINAL, empty -> [(6,8,0)], hold 0.  Key U+662F over U+6211 U+662F U+4E2D (9 bytes, W = 2)
 * cut 4 | 4 | 1: [], hold 4; [(0,3,-1),(3,6,0)], hold 2; [], hold 3 (byte 7 is a continuation byte: the character from 6
 * stays open); FINAL -> [(6,9,-1)].  Key a (W = 0), "xa\xC3" | "\xA9" | "y": [(0,1,-1),(1,2,0)], hold 1; [], hold 2;
 * [(2,4,-1)], hold 1; FINAL -> [(4,5,-1)].  GAP_RUNS, key ab, "zzzzzz" | "zzab" | "zz" FINAL: [(0,5,-1)], hold 1;
 * [(5,8,-1),(8,10,0)], hold 0; [(10,12,-1)] -- joined, the gap is (0,8,-1).
 * State and mixing: 16 bytes per sequence (bytes seen by token calls, t), allocated by the feed's first token call;
 * aha_feed_reset clears it with the select state.  A token call is valid for a sequence iff the sequence has length 0 (it is
 * fresh then, with t = 0) or all of its bytes since open, reset or FINAL went through token calls; otherwise AHA_E_INVALID,
 * found on the device beside select's own check (aha_last_error names "tokens"), and nothing changes.  Select and replace
 * calls are valid after token calls -- the select state is theirs -- and leave the token state as it is (their FINAL restarts
 * the sequence and with it t); after one of them the sequence takes token calls again from its next reset or FINAL.  Calls
 * with and without GAP_RUNS may alternate on one sequence: each applies its own bit from t0 on (the laws are stated for a
 * constant bit).
 * Everything feed select refuses is refused the same way (AHA_FEED_CHARS, a separator filter, a longest feed, a feed folded
 * beyond ASCII).  On an AHA_OPT_FOLD_ASCII handle the lead-byte rule reads the caller's bytes.  Every failing call changes
 * nothing, AHA_E_CAPACITY included (*n_selected = the required token count; out == NULL with cap == 0 is a sizing call).
 * start and end are int32 and a run of stray continuation bytes keeps a character-mode token open without bound: a call that
 * would leave n1 - t1 > 0x3FFFFFFF answers AHA_E_TOO_LONG (found on the device before anything is written; nothing changes).
 * A FINAL call closes the token and GAP_RUNS never holds, so neither meets the bound.  (The bound is read from
 * AHA_FEED_TOKEN_OPEN when the handle is compiled: tests lower it.)
 * Pipeline (feed.cpp feed_tokens, scan_feedtokens.hip; DESIGN.md 4.10 "Feed tokens"): a select call up to its rank; then per
 * piece c0, c1 and t0; the inside mask of the settled selection (ktk_spans); the start mask by the rule of token_rule.hpp with
 * c0 for the document's start where t0 == c0, the continuation bits from the sequence's context bank and from the piece
 * (16-byte loads aligned to the address, nothing outside [corpus, corpus + N) read; with GAP_RUNS no text at all); its rank;
 * per piece the edge decision (feedtok_edge.hpp) and the token count; the pieces' offsets and the total (one read-back with
 * the verdict); then the tokens by ranked slots, the two commits of a select call and the token state.  Device memory beyond a
 * feed select call's: 2 bits per extended position, their rank blocks and 48 bytes per piece.  Nothing per token.
 * Out of scope: token calls on char, separator-filter, longest and folded feeds; groups; character offsets; a device-side
 * hold buffer; id remapping. */
#define AHA_FEED_SELECT_TOKENS 4u   /* out receives the tokens this call settles instead of the selection */
#define AHA_FEED_SELECT_GAP_RUNS 8u /* only with AHA_FEED_SELECT_TOKENS: gaps are not cut into characters */

/* Feed replace: the substituted stream of sequences that arrive in pieces, built on the device (pure additions to ABI 8).  The
 * same pieces and flags as aha_feed_select_batch*, on a BYTE feed, and a replacement table of the feed's handle as for
 * aha_ac_replace_batch*.  T, S(T), W and F(n) as for feed select; c = the sequence's select cursor.  A call takes a sequence
 * from n0 to n1 bytes; it finds the cursor at c0 -- the bytes T[c0..n0) are still open, n0 - c0 is the previous piece_hold --
 * and leaves it at c1 = max(c0, end of the last hit this call settles, F(n1)); c1 = n1 under FINAL.  "Settles" means what
 * aha_feed_select_batch with the same flags would report for the piece; all such hits lie inside [c0, c1).
 * The piece's result is T[c0..c1) with every hit this call settles replaced as the table says: kept keys stay as they are, an
 * empty replacement deletes, and on a folded handle the bytes outside replaced hits are the caller's.  out = the pieces'
 * results one behind the other, piece_out_offsets[0 .. D] where each lies (a piece may give 0 bytes), *n_out_bytes the total;
 * piece_bases[d] = n0; piece_hold[d] = n1 - c1 (0 after FINAL, and those sequences start again from length 0); *n_selected,
 * *n_hits (optional) as feed select reports them.  cap_bytes is in bytes.
 * The stream law: cut a sequence anywhere into pieces, empty ones included, feed them through replace calls, the last with
 * FINAL, and concatenate the results -- that is, byte for byte, aha_ac_replace_batch of the whole sequence as one document with
 * the same table.  Example (keys ab -> "<AB>", abcde -> "", so W = 4): "xab" gives "" (hold 3: nothing lies in front of
 * F(3) = 0), "cd" gives "x" (hold 4), "eab" gives "" (the longer key completed at (1, 6) and is deleted; hold 2), a FINAL call
 * with an empty piece gives "<AB>".
 * State: a replace call is a select call for the feed's state -- it maintains the bytes seen, the cursor and the tail exactly
 * as a select call does and is valid under the same condition (every byte of the sequence since open, reset or FINAL went
 * through select or replace calls; otherwise AHA_E_INVALID, found on the device, nothing changes, until the next reset).
 * Select and replace calls may be mixed on one sequence: a replace call gives the substituted T[c0..c1) from wherever the
 * cursor stands; the stream law is stated for sequences fed by replace calls only.
 * AHA_E_CAPACITY: *n_out_bytes is the required size (*n_selected and *n_hits are set too), NONE of the caller's buffers is
 * written and the feed is unchanged; the same call with a larger buffer gives what the first would have (out == NULL with
 * cap_bytes == 0 is a sizing call; a total of 0 succeeds with cap_bytes == 0).  Every failing call changes nothing.
 * A NULL feed, table or n_out_bytes, a table made for another handle, any flag bit but AHA_FEED_REPLACE_FINAL, a feed opened
 * with AHA_FEED_CHARS, a feed opened with a separator filter (a follow-up), the device entry with out overlapping the corpus
 * (its address ranges, when cap_bytes > 0): AHA_E_INVALID, all before any device work.  Piece and id validation is that of the
 * other feed entries.  The handle's back-off state is read and never written; two feeds in the same state give identical bytes.
 * d_out and d_corpus may have any alignment: no load touches an aligned 16-byte piece that holds no byte of its source buffer,
 * no store a byte outside [out, out + total).
 * Pipeline (feed.cpp feed_replace, scan_feedreplace.hip; DESIGN.md 4.10 "Feed replace"): a select call up to its total, the
 * selection into the call's scratch; per piece hold0 = n0 - c0 and the staged length c1 - c0, scanned; the staged text ext --
 * hold0 bytes from the sequence's context bank (the caller's bytes: the banks are filled from the caller's text), then the
 * piece up to c1; a wave owns 1024 staged bytes, a lane 16, a tile inside one piece is two aligned 16-byte loads, a byte
 * alignment and one aligned 16-byte store per lane --; then replace's own passes over (ext, its offsets, the selection), the
 * byte total to the host, and once it fits the copy, the offsets and the two commits of a select call.
 * Device scratch beyond a feed select call's: the staged text (at most N + D W bytes), per settled hit 12 bytes of selection, 8
 * of A, 8 of shift, the scan's block sums, 28 bytes per piece.  AHA_REPLACE_BLOCKS caps the grids of the stage and of
 * replace's passes. */
#define AHA_FEED_REPLACE_FINAL AHA_FEED_SELECT_FINAL /* the same bit: the pieces are the last of their sequences */
int32_t aha_feed_replace_batch(aha_feed *f, const aha_repl *table, const uint8_t *corpus, const uint64_t *piece_offsets,
                               const uint32_t *seq_ids, uint64_t n_pieces, uint32_t flags, uint8_t *out, uint64_t cap_bytes,
                               uint64_t *piece_out_offsets /* D+1 or NULL */, uint64_t *piece_bases /* D or NULL */,
                               uint32_t *piece_hold /* D or NULL */, uint64_t *n_out_bytes, uint64_t *n_selected /* or NULL */,
                               uint64_t *n_hits /* or NULL */);
/* Device-resident form: d_ pointers are HBM on the handle's device, validated on the device before anything is indexed with
 * them; *n_out_bytes, *n_selected, *n_hits are host memory; blocks until final. */
int32_t aha_feed_replace_batch_device(aha_feed *f, const aha_repl *table, const uint8_t *d_corpus, const uint64_t *d_piece_offsets,
                                      const uint32_t *d_seq_ids, uint64_t n_pieces, uint64_t n_bytes, uint32_t flags,
                                      uint8_t *d_out, uint64_t cap_bytes, uint64_t *d_piece_out_offsets /* D+1 or NULL */,
                                      uint64_t *d_piece_bases /* D or NULL */, uint32_t *d_piece_hold /* D or NULL */,
                                      uint64_t *n_out_bytes, uint64_t *n_selected /* or NULL */, uint64_t *n_hits /* or NULL */,
                                      void *stream);

/* Feed grep: records and grep (aha_ac_records_batch*, aha_ac_grep_batch* above) for sequences that arrive in pieces whose ends
 * fall in the middle of lines.  The same pieces as aha_feed_match_batch*, on a BYTE feed, and a delimiter byte.
 * The whole-sequence definition.  T = a sequence: all its pieces since open, reset or a FINAL call, concatenated.  Its records
 * are aha_ac_records_batch of the one document T with `delim`; a record is KEPT when (aha_ac_match_batch of the record AS ITS
 * OWN DOCUMENT has >= 1 hit) != invert -- aha_ac_grep_batch over those record offsets, on a plain or a folded handle.  A record
 * CLOSES in the call that delivers its delimiter byte; the trailing record without a delimiter closes in the sequence's FINAL
 * call.  Concatenated over a sequence's calls (the last with AHA_FEED_GREP_FINAL), what the feed reports as kept -- the held
 * bytes it tells the caller to emit included -- is aha_ac_grep_batch's `out` for the whole sequence, byte for byte, in order.
 * The open line has no length limit and the feed's state per sequence is bounded, so -- as with piece_hold of
 * aha_feed_select_batch -- the CALLER keeps the bytes of the record that is still open; the call says how many to keep and when
 * to emit or drop them.
 * The pieces are split into FRAGMENTS exactly as aha_ac_records_batch(corpus, piece_offsets, delim) splits them: R fragments,
 * piece_rec_offsets[0 .. D] = that call's doc_rec_offsets.  Only a piece's last fragment can be open (it has no delimiter and
 * the call is not FINAL); only a piece's first fragment can continue a record from earlier pieces.  Outputs, optional unless
 * noted:
 *   kept_recs[0 .. n_kept)        the kept CLOSED fragments' indices in that numbering, ascending; an open fragment is never listed
 *   rec_out_offsets[0 .. n_kept], out   the kept fragments' bytes that lie in this call's pieces, one behind the other -- the
 *                                 caller's own bytes, on a folded handle too.  cap_recs bounds kept_recs and rec_out_offsets
 *                                 (which holds cap_recs + 1 entries), cap_bytes bounds out
 *   piece_kept_offsets[0 .. D]    kept fragments per piece, scanned
 *   piece_hold[d] (uint32)        the bytes at the end of piece d that belong to the record left open: 0 under FINAL; outside
 *                                 FINAL it equals |P_d| exactly when nothing closed in the piece
 *   piece_head[d] (uint64)        the bytes IN FRONT of the piece that belong to a record which closes in this piece and is
 *                                 kept -- the length of the record that was open before the call: the caller emits that many
 *                                 held bytes in front of the piece's first kept fragment.  0 when no record was open, when it
 *                                 stays open, or when it closes and is dropped.  One case is irregular: an EMPTY piece under
 *                                 FINAL with a record open closes that record without any fragment -- it appears only as
 *                                 piece_head[d], not in kept_recs, *n_kept or piece_kept_offsets
 *   piece_bases[d]                the sequence's length before the piece
 *   piece_rec_bases[d]            the records of the sequence closed before the call: fragment j of piece d is line
 *                                 piece_rec_bases[d] + (j - piece_rec_offsets[d]) of its sequence
 *   *n_recs = R; *n_kept (required); *n_out_bytes; *n_hits = the hits of the fragments, each matched as its own document.
 * The caller's holding rule, per sequence: emit piece_head held bytes (else drop them when hold < |P| or under FINAL), then the
 * piece's kept bytes; then, under FINAL, hold nothing; else if hold == |P|: held += piece; else held = the piece's last hold bytes.
 * A call takes the sequence from n0 to n1 as a match call does.  Under FINAL the named sequences start again at length 0, as
 * after aha_feed_reset.
 * THE TRAP.  The hits of a record are those of the record matched as its own document: the automaton reports by state (only
 * where the longest suffix that is a trie path ends a key), so they are neither the hits of the sequence that lie inside the
 * record nor the hits of a fragment from the root.  Keys "abc", "b", pieces "a" | "b\n": the record "ab\n" has no hit (the
 * state at b is "ab"); the fragment "b\n" from the root has one.  Keys "x\nabc", "b", sequence "x\nab\n": the record "ab\n" has
 * a hit; a feed match of the sequence reports none there (its state at b is "x\nab").  A key "\nb" never hits in a record; a
 * key "b\n" hits only at a record's end.  The call applies the feed's two facts to the record as the sequence (DESIGN.md 4.10
 * "Feed grep"): for a piece whose first fragment continues an open record of open_len bytes that already has a hit or not
 * (open_hit), with W = max(Lmax - 1, 0), c = min(W, open_len), e0 = the first fragment's length, g = min(W, e0),
 * X = ctx[-c:] || P[0 .. g), Y = ctx[-c:], Z = P[0 .. g):
 *   has(record) = open_hit  ||  hits(X) - hits(Y) > 0  ||  hits(fragment from the root) - hits(Z) > 0
 * Every other fragment begins a record, so its own count from the root is exact.
 * Validity: a grep call is valid on a sequence only if all its bytes since open, reset or FINAL went through grep calls
 * (otherwise AHA_E_INVALID, found on the device, nothing changes, until its reset).  `delim` is fixed by the feed's first
 * successful grep call; another value later is AHA_E_INVALID.  A NULL feed or n_kept, a feed opened with AHA_FEED_CHARS or with a
 * separator filter (a follow-up), an unknown flag, a NULL buffer with a non-zero capacity (cap_recs with neither kept_recs nor
 * rec_out_offsets; cap_bytes without out), out overlapping the corpus: AHA_E_INVALID, all before any device work.  Piece and id
 * validation is that of the other feed entries.
 * AHA_E_CAPACITY when n_kept > cap_recs and kept_recs or rec_out_offsets was given, or when n_out_bytes > cap_bytes and out was
 * given: BOTH required numbers are reported.  No failing call writes a caller buffer or moves any sequence, AHA_E_CAPACITY
 * included: the same call with larger buffers gives what the first would have.  A call whose buffers are all NULL succeeds and
 * moves the sequences: size with a non-NULL buffer of capacity 0.  out == NULL never launches the copy.  Two identical call
 * sequences give identical bytes.  aha_feed_reset clears the grep state.  The handle's back-off state is read, never written.
 * Pipeline (feed.cpp feed_grep, scan_feedgrep.hip): kfd_check; the records call over the pieces in two halves (the total sizes
 * the fragment offsets); the window batch [X | Y | Z], at most 4 W bytes per piece; the count call without key counts over the
 * windows, then over the fragments as documents (aha_ac_last_timing reports this pass); keep, S and T over the fragments (an
 * open tail counts as dropped); grep's rank, runs, scan, emit and copy as they are; kfd_commit and kfg_commit.  Device scratch:
 * a records call's and a count call's, 17 bytes and 3 bits per fragment, 28 bytes per dropped run, 56 bytes and 4 W per piece;
 * 32 bytes of state per sequence.  AHA_GREP_BLOCKS caps the grids.
 * Out of scope so far: separator-filter feeds, char feeds, match_longest, a device-side hold buffer, rules over class counts
 * (AHA_GREP_RULE is a batch call), context lines (AHA_GREP_LINES is a batch call too; a feed form is the follow-up). */
#define AHA_FEED_GREP_FINAL 2u /* the pieces named in this call are the last of their sequences (beside AHA_GREP_INVERT, bit 0) */
int32_t aha_feed_grep_batch(aha_feed *f, const uint8_t *corpus, const uint64_t *piece_offsets, const uint32_t *seq_ids,
                            uint64_t n_pieces, uint8_t delim, uint32_t flags /* AHA_GREP_INVERT | AHA_FEED_GREP_FINAL */,
                            uint64_t *kept_recs /* or NULL */, uint64_t *rec_out_offsets /* cap_recs + 1 or NULL */,
                            uint64_t cap_recs, uint8_t *out /* or NULL */, uint64_t cap_bytes,
                            uint64_t *piece_rec_offsets /* D+1 or NULL */, uint64_t *piece_kept_offsets /* D+1 or NULL */,
                            uint32_t *piece_hold /* D or NULL */, uint64_t *piece_head /* D or NULL */,
                            uint64_t *piece_bases /* D or NULL */, uint64_t *piece_rec_bases /* D or NULL */,
                            uint64_t *n_recs /* or NULL */, uint64_t *n_kept, uint64_t *n_out_bytes /* or NULL */,
                            uint64_t *n_hits /* or NULL */);
/* Device-resident form: d_ pointers are HBM on the handle's device, validated on the device before anything is indexed with
 * them; the n_ pointers are host memory; blocks until final. */
int32_t aha_feed_grep_batch_device(aha_feed *f, const uint8_t *d_corpus, const uint64_t *d_piece_offsets, const uint32_t *d_seq_ids,
                                   uint64_t n_pieces, uint64_t n_bytes, uint8_t delim,
                                   uint32_t flags /* AHA_GREP_INVERT | AHA_FEED_GREP_FINAL */, uint64_t *d_kept_recs /* or NULL */,
                                   uint64_t *d_rec_out_offsets /* cap_recs + 1 or NULL */, uint64_t cap_recs,
                                   uint8_t *d_out /* or NULL */, uint64_t cap_bytes, uint64_t *d_piece_rec_offsets /* D+1 or NULL */,
                                   uint64_t *d_piece_kept_offsets /* D+1 or NULL */, uint32_t *d_piece_hold /* D or NULL */,
                                   uint64_t *d_piece_head /* D or NULL */, uint64_t *d_piece_bases /* D or NULL */,
                                   uint64_t *d_piece_rec_bases /* D or NULL */, uint64_t *n_recs /* or NULL */, uint64_t *n_kept,
                                   uint64_t *n_out_bytes /* or NULL */, uint64_t *n_hits /* or NULL */, void *stream);

/* Frees the handle's device scratch (it grows with the largest batch seen and is otherwise kept for reuse). */
int32_t aha_ac_release_scratch(aha_ac *ac);
/* Device bytes currently held as scratch by the handle (all sets); waits for running calls. */
int64_t aha_ac_scratch_bytes(aha_ac *ac);

/* Enable/disable HIP-event timing of device matches on this handle.  aha_timing.engine tells which engine answered the
 * last call: keys longer than 4096 bytes, a NULL-capacity sizing call and event-temp overflow take the two-pass
 * engine (1), which is an order of magnitude slower than the single-traversal engine (2). */
int32_t aha_ac_set_profiling(aha_ac *ac, int32_t enabled);
int32_t aha_ac_last_timing(const aha_ac *ac, aha_timing *t);

/* ---- device memory for callers without a GPU framework (SURVEY.md section 8 b: aha_corpus_upload / _free) ----------
 * aha_ac_match_batch_device takes HBM pointers; these give a C, C++ or Crystal caller a way to obtain them, so that a
 * corpus is uploaded once and matched many times (or by several automata) and the hits stay on the device until they
 * are wanted.  Copies run on a private stream of the library and block the calling thread only.  Buffers are 256-byte
 * aligned.  Errors: AHA_E_HIP / AHA_E_INVALID / AHA_E_NO_DEVICE, text through aha_last_error(NULL). */
int32_t aha_buffer_alloc(int32_t device, uint64_t bytes, void **d_ptr);
int32_t aha_buffer_free(int32_t device, void *d_ptr);
int32_t aha_buffer_upload(int32_t device, void *d_dst, const void *src, uint64_t bytes);
int32_t aha_buffer_download(int32_t device, void *dst, const void *d_src, uint64_t bytes);
/* A batch resident in HBM: the bytes of all documents and their D + 1 offsets (validated like aha_ac_match_batch
 * validates them: ascending from 0, every document below 2^31 bytes). */
typedef struct aha_corpus aha_corpus;
int32_t aha_corpus_upload(int32_t device, const uint8_t *corpus, const uint64_t *doc_offsets, uint64_t n_docs,
                          aha_corpus **out);
void aha_corpus_free(aha_corpus *c);
const uint8_t *aha_corpus_bytes(const aha_corpus *c);         /* device pointer */
const uint64_t *aha_corpus_doc_offsets(const aha_corpus *c);  /* device pointer, n_docs + 1 entries */
uint64_t aha_corpus_n_docs(const aha_corpus *c);
uint64_t aha_corpus_n_bytes(const aha_corpus *c);
int32_t aha_corpus_device(const aha_corpus *c);

/* ---- several GPUs of one node behind one handle (SURVEY.md section 8 b / e) -------------------------------------
 * The batch is cut into contiguous, byte-balanced document ranges, one per entry of `devices` (documents are
 * independent: src/aha/ac.cr:177; contiguous ranges make the global hit order the range order); the automaton is
 * replicated; every device matches its range; the hit buffers are exchanged with an all-gatherv, so every device
 * holds the whole ordered hit stream, and come back to the caller exactly as aha_ac_match_batch would return them.
 * Between distinct devices the exchange is RCCL over xGMI (all-pairs ncclSend/ncclRecv in one group; librccl.so is
 * loaded on first use); entries that name the same device twice -- several shards on one GPU, the form a 1-GPU box
 * can run -- exchange with device-to-device copies.  Buffers are host memory; the calls block; calls on one group
 * are serialised inside the library.  The capacity is checked before the exchange: on AHA_E_CAPACITY the devices
 * hold their own shards' hits only. */
typedef struct aha_group aha_group;

typedef struct {
  uint32_t struct_size;
  uint32_t n_devices;
  float ms_match;            /* upload + match of all shards, wall clock (shards run concurrently) */
  float ms_match_max_shard;  /* the slowest shard's device match alone */
  float ms_exchange;         /* the all-gatherv of the hit buffers */
  float ms_download;         /* gathered hits -> caller's buffer */
  uint64_t n_hits;
  uint32_t exchange;         /* 1 = RCCL between distinct devices, 0 = device-to-device copies on one device,
                                2 = the rehearsal AHA_GROUP_RCCL=self: every shard's own stream through RCCL (one
                                communicator of one rank per shard), the peers' by copies */
  uint32_t packed;           /* 1 = the 4-byte exchange stream travelled, 0 = the 12-byte triples (2^20 keys or more) */
  uint64_t wire_bytes;       /* payload bytes of all shards together (each goes to every other shard) */
} aha_group_timing;

int32_t aha_group_compile(const uint8_t *key_bytes, const uint64_t *key_offsets, uint32_t n_keys,
                          const int32_t *devices, int32_t n_devices, uint32_t flags, aha_group **out,
                          uint32_t *err_key);
void aha_group_free(aha_group *g);
int32_t aha_group_size(const aha_group *g);
const char *aha_group_last_error(const aha_group *g);
/* bounds[0..n_parts]: shard r holds documents bounds[r] .. bounds[r+1]-1 (the boundary nearest to r * N / n_parts). */
int32_t aha_group_partition(const uint64_t *doc_offsets, uint64_t n_docs, int32_t n_parts, uint64_t *bounds);
/* Same contract as aha_ac_match_batch (AHA_E_CAPACITY: *n_hits = required count, offsets valid). */
int32_t aha_group_match_batch(aha_group *g, const uint8_t *corpus, const uint64_t *doc_offsets, uint64_t n_docs,
                              const aha_match_params *params, aha_hit *out, uint64_t cap,
                              uint64_t *doc_hit_offsets, uint64_t *n_hits);
/* The gathered hit stream as device `shard` holds it after the last aha_group_match_batch (every device holds the
 * whole ordered stream: this is how a test, or a caller that wants a particular device's copy, reads it back). */
int32_t aha_group_download_shard(aha_group *g, int32_t shard, aha_hit *out, uint64_t cap, uint64_t *n_hits);
int32_t aha_group_last_timing(const aha_group *g, aha_group_timing *t);
/* ABI 7 -- the batch RESIDENT on the group's devices (the group counterpart of aha_corpus_upload + aha_ac_match_batch_device;
 * keeps the reference's one call per batch, src/aha/ac.cr:280-286): aha_group_corpus_upload partitions the documents like
 * aha_group_match_batch does and leaves every shard's range on its device (each over its own PCIe link);
 * aha_group_match_batch_device matches the resident ranges, every device its own, and runs the same all-gatherv -- nothing of
 * the batch crosses PCIe any more.  The hits stay on the devices: every device holds the whole ordered stream
 * (aha_group_download_shard reads one device's copy); *n_hits and doc_hit_offsets (n_docs + 1 entries, optional) are host
 * memory.  A corpus belongs to the group it was uploaded for and must be freed before that group. */
typedef struct aha_group_corpus aha_group_corpus;
int32_t aha_group_corpus_upload(aha_group *g, const uint8_t *corpus, const uint64_t *doc_offsets, uint64_t n_docs,
                                aha_group_corpus **out);
void aha_group_corpus_free(aha_group_corpus *c);
int32_t aha_group_match_batch_device(aha_group *g, const aha_group_corpus *c, const aha_match_params *params,
                                     uint64_t *doc_hit_offsets, uint64_t *n_hits);

#if defined(__GNUC__)
#pragma GCC visibility pop
#endif
#ifdef __cplusplus
}
#endif
#endif /* AHA_HIP_H */
