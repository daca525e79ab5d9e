# aha_hip.cr -- Crystal binding that re-backs Aha::AC with libaha_hip.so
# (MI355X).  Drop this file next to the reference's src/aha/ac.cr and require
# it INSTEAD of ac.cr; the public surface is unchanged:
#
#   Aha::AC.compile(keys)            (reference: src/aha/ac.cr:62-69)
#   AC#match(seq : Bytes, &block)    (src/aha/ac.cr:280-286)
#   AC#match(seq : String, &block)   (src/aha/matcher.cr:34-39)
#   AC#match(seq, sep : BitArray)    (src/aha/ac.cr:321-340, matcher.cr:41-46)
#   AC#match(seq : Array(Char))      (src/aha/ac.cr:288-295)
#   AC#match(Array(Char), sep)       (src/aha/ac.cr:342-364: the neighbour tests look at code points)
#   AC#match_longest(seq, intersectable)   (src/aha/ac.cr:297-319)
#   AC#[](Int) / AC#[](String)       (src/aha/ac.cr:41-43)
#   Aha::Hit                         (src/aha/matcher.cr:2-11, unchanged)
# plus the batch surface the reference does not have (one sequence per call there):
#   AC#match_batch(docs)             -> Array(Array(Aha::Hit)), one GPU round trip for all documents
#   Aha::ACGroup                     the same over several GPUs of one node (aha_group_*)
#
# AC.compile(da : Cedar) (src/aha/ac.cr:71) is provided for tries built by `insert` only: the keys are read back in
# id order (Cedar#[](id), cedar.cr:747-749) and compiled by the library; ids freed by Cedar#delete are rejected,
# because the library numbers keys densely (Hit#value = index in compile order).
#
# Written for the Crystal the reference pins (shard.yml: 0.23.1): integer division is `/`.
#
# UNVERIFIED: no Crystal toolchain exists in the build container or on the GPU
# box, so this file has never been compiled.  The same .so is exercised
# through the identical C ABI by the Python and C++ mirrors (aha_amd/ac.py,
# include/aha/ac.hpp).
require "bit_array"
require "./matcher"

@[Link("aha_hip")]
lib LibAhaHip
  type Ac = Void*

  struct Hit
    start : Int32
    end_ : Int32
    value : Int32
  end

  OPT_FOLD_ASCII = 4_u32 # compile-time flag: 'A'..'Z' of keys and text match as 'a'..'z' (include/aha_hip.h)
  OPT_FOLD_SIMPLE = 8_u32 # ... and the two-byte UTF-8 characters by their simple case fold, document by document; no feeds, no groups yet
  OPT_FOLD_BMP = 16_u32 # ... and the three-byte ones (full-width Latin, Vietnamese, polytonic Greek, Georgian, Cherokee ..); implies both; no feeds, no groups yet
  OPT_FOLD_KANA = 32_u32 # ... and hiragana and half-width katakana as katakana (length-preserving; no voiced half-width sequences); implies all three; no feeds, no groups yet

  struct Options
    struct_size : UInt32
    device : Int32
    flags : UInt32
    reserved : UInt32
  end

  struct MatchParams
    struct_size : UInt32
    char_offsets : Int32
    sep_size : Int32
    sep_bits : UInt8[32]
    longest : Int32 # 0 = #match, 1 = #match_longest(intersectable: false), 2 = #match_longest(intersectable: true)
  end

  # aha_ac_info_t (ABI 8)
  struct Info
    struct_size : UInt32
    n_keys : UInt32
    n_states : UInt64
    n_slots : UInt64
    image_bytes : UInt64
    max_key_len : UInt32
    slot_bytes : UInt32
    lds_slots : UInt32
    device : Int32
    fail_s1_lo : UInt32
    fail_s2_lo : UInt32
    fail_hdr_lo : UInt32
    unit_header_beside : UInt32 # ABI 7: the traversal requests a fail header beside its probe
    unit_enabled : UInt32
    unit_slots : UInt32
    unit_syms : UInt32
    unit_multi_permille : UInt32
    unit_big_lo : UInt32
    unit_big_block : UInt32
    unit_n_low : UInt32
    unit_n_big : UInt32
    unit_base_bits : UInt32
    unit_headers : UInt32       # ABI 7: states that own a fail header
    filter_prefix_bytes : UInt32 # ABI 7: the prefix-filter engine looks at this many first bytes of a key (0: none)
    filter_words : UInt32       # ABI 7: 32-bit words of its Bloom filter
    skip_filter_words : UInt32  # ABI 8: words of the mark filter of the skip-ahead traversal (engine 6; 0: none)
    skip_pairs : UInt32         # ABI 8: two-character trie paths it holds
    pair_hash_k1 : UInt32       # ABI 8: multiplier of the second character in the pair hash
    pair_table_log2 : UInt32    # ABI 8: log2 of the pair table's 16-byte slots (0: none)
    pair_groups : UInt32        # ABI 8: its displacement bytes
    pair_engine : UInt32        # ABI 8: 1 = byte-offset matches run the pair engine (engine 7)
  end

  # aha_timing (ABI 6): filled when profiling is on
  struct Timing
    struct_size : UInt32
    n_kernels : UInt32
    ms_total : Float32
    ms_count : Float32
    ms_scan : Float32
    ms_write : Float32
    ms_aux : Float32
    n_chunks : UInt64
    n_hits : UInt64
    engine : UInt32      # 4 = character-level traversal, 2 = single-traversal engine, 1 = two-pass engine
    chunk_bytes : UInt32
    repeats : UInt32     # passes thrown away: 1 = a region overflowed and the match ran again with full-size regions
    reserved : UInt32
  end

  struct StreamSeg
    word_offset : UInt64
    n_hits : UInt64
    out_offset : UInt64
  end

  struct GroupTiming
    struct_size : UInt32
    n_devices : UInt32
    ms_match : Float32
    ms_match_max_shard : Float32
    ms_exchange : Float32
    ms_download : Float32
    n_hits : UInt64
    exchange : UInt32
    packed : UInt32
    wire_bytes : UInt64
  end

  fun aha_abi_version : UInt32
  fun aha_device_count : Int32
  fun aha_strerror(code : Int32) : UInt8*
  fun aha_last_error(ac : Ac) : UInt8*
  fun aha_ac_compile(key_bytes : UInt8*, key_offsets : UInt64*, n_keys : UInt32,
                     opts : Options*, out : Ac*, err_key : UInt32*) : Int32
  fun aha_ac_free(ac : Ac) : Void
  # a second handle for the same keys on another device: nothing is compiled again (what aha_group_compile does)
  fun aha_ac_replicate(ac : Ac, device : Int32, out : Ac*) : Int32
  fun aha_ac_info(ac : Ac, info : Info*) : Int32
  # the AHA_OPT_* bits the handle was compiled with (OPT_FOLD_ASCII: an ASCII case-insensitive handle)
  fun aha_ac_flags(ac : Ac) : UInt32
  fun aha_ac_set_profiling(ac : Ac, enabled : Int32) : Int32
  fun aha_ac_last_timing(ac : Ac, t : Timing*) : Int32
  # ABI 7: the device match that also leaves the hits as the 4-byte exchange stream
  fun aha_ac_match_batch_device_stream(ac : Ac, d_corpus : UInt8*, d_doc_offsets : UInt64*, n_docs : UInt64, n_bytes : UInt64,
                                       params : MatchParams*, d_out : Hit*, cap : UInt64, d_doc_hit_offsets : UInt64*,
                                       n_hits : UInt64*, d_words : UInt32*, cap_words : UInt64, d_n_words : UInt64*,
                                       stream : Void*) : Int32
  fun aha_ac_release_scratch(ac : Ac) : Int32
  fun aha_ac_scratch_bytes(ac : Ac) : Int64
  fun aha_ac_export(ac : Ac, which : Int32, buf : Void*, cap_bytes : UInt64) : Int64
  fun aha_ac_key(ac : Ac, id : Int32, buf : UInt8*, cap : Int32) : Int32
  fun aha_ac_id(ac : Ac, key : UInt8*, len : Int32) : Int32
  fun aha_ac_save(ac : Ac, buf : Void*, cap_bytes : UInt64) : Int64
  fun aha_ac_load(buf : Void*, n_bytes : UInt64, opts : Options*, out : Ac*) : Int32
  fun aha_ac_match_bytes(ac : Ac, text : UInt8*, n : UInt64, params : MatchParams*,
                         out : Hit*, cap : UInt64, n_hits : UInt64*) : Int32
  fun aha_ac_match_batch(ac : Ac, corpus : UInt8*, doc_offsets : UInt64*, n_docs : UInt64,
                         params : MatchParams*, out : Hit*, cap : UInt64,
                         doc_hit_offsets : UInt64*, n_hits : UInt64*) : Int32

  # host corpus in, hits left on the device (d_hits: device memory of the handle's device)
  fun aha_ac_match_batch_keep(ac : Ac, corpus : UInt8*, doc_offsets : UInt64*, n_docs : UInt64,
                              params : MatchParams*, d_hits : Hit*, cap : UInt64,
                              doc_hit_offsets : UInt64*, n_hits : UInt64*) : Int32
  # exchange formats of the hit lists (all on device memory, asynchronous on `stream`)
  fun aha_ac_stream_format(ac : Ac, step_bits : UInt32*, len_bits : UInt32*) : Int32
  fun aha_ac_hits_pack_device(ac : Ac, d_hits : Hit*, n : UInt64, d_pairs : Int32*, stream : Void*) : Int32
  fun aha_ac_hits_unpack_device(ac : Ac, d_pairs : Int32*, n : UInt64, char_offsets : Int32, d_hits : Hit*,
                                stream : Void*) : Int32
  fun aha_ac_hits_pack4_device(ac : Ac, d_hits : Hit*, n : UInt64, d_words : UInt32*, cap_words : UInt64,
                               d_n_words : UInt64*, stream : Void*) : Int32
  fun aha_ac_hits_unpack4_device(ac : Ac, d_words : UInt32*, n : UInt64, char_offsets : Int32, d_hits : Hit*,
                                 stream : Void*) : Int32
  fun aha_ac_hits_unpack4_segs_device(ac : Ac, d_words : UInt32*, segs : StreamSeg*, n_segs : UInt32,
                                      char_offsets : Int32, d_hits : Hit*, stream : Void*) : Int32
  # device-resident batches: upload a corpus once, match it many times, keep the hits in HBM until they are wanted
  fun aha_ac_match_batch_device(ac : Ac, d_corpus : UInt8*, d_doc_offsets : UInt64*, n_docs : UInt64, n_bytes : UInt64,
                                params : MatchParams*, d_out : Hit*, cap : UInt64, d_doc_hit_offsets : UInt64*,
                                n_hits : UInt64*, stream : Void*) : Int32
  # hits per key and per document without the hit list (flags: COUNT_ACCUMULATE adds into key_counts)
  COUNT_ACCUMULATE = 1_u32
  fun aha_ac_count_batch(ac : Ac, corpus : UInt8*, doc_offsets : UInt64*, n_docs : UInt64, params : MatchParams*,
                         flags : UInt32, key_counts : UInt64*, doc_hit_offsets : UInt64*, n_hits : UInt64*) : Int32
  fun aha_ac_count_batch_device(ac : Ac, d_corpus : UInt8*, d_doc_offsets : UInt64*, n_docs : UInt64, n_bytes : UInt64,
                                params : MatchParams*, flags : UInt32, d_key_counts : UInt64*, d_doc_hit_offsets : UInt64*,
                                n_hits : UInt64*, stream : Void*) : Int32
  # document counts: per document one {key, count} pair per distinct hit value, ascending by key (cap in pairs)
  struct KeyCount
    key : Int32
    count : UInt32
  end
  fun aha_ac_doc_counts_batch(ac : Ac, corpus : UInt8*, doc_offsets : UInt64*, n_docs : UInt64, params : MatchParams*,
                              out : KeyCount*, cap : UInt64, doc_pair_offsets : UInt64*, n_pairs : UInt64*,
                              n_hits : UInt64*) : Int32
  fun aha_ac_doc_counts_batch_device(ac : Ac, d_corpus : UInt8*, d_doc_offsets : UInt64*, n_docs : UInt64, n_bytes : UInt64,
                                     params : MatchParams*, d_out : KeyCount*, cap : UInt64, d_doc_pair_offsets : UInt64*,
                                     n_pairs : UInt64*, n_hits : UInt64*, stream : Void*) : Int32
  # cover: which bytes lie inside a hit (bit j = word j >> 5, bit j & 31), and a redacted copy; no hit list
  fun aha_ac_cover_batch(ac : Ac, corpus : UInt8*, doc_offsets : UInt64*, n_docs : UInt64, params : MatchParams*,
                         flags : UInt32, mask : UInt32*, redacted : UInt8*, fill : UInt8, doc_covered : UInt64*,
                         n_covered : UInt64*, n_hits : UInt64*) : Int32
  fun aha_ac_cover_batch_device(ac : Ac, d_corpus : UInt8*, d_doc_offsets : UInt64*, n_docs : UInt64, n_bytes : UInt64,
                                params : MatchParams*, flags : UInt32, d_mask : UInt32*, d_redacted : UInt8*, fill : UInt8,
                                d_doc_covered : UInt64*, n_covered : UInt64*, n_hits : UInt64*, stream : Void*) : Int32
  # select: per document the leftmost-longest, non-overlapping hits of the match (byte offsets)
  fun aha_ac_select_batch(ac : Ac, corpus : UInt8*, doc_offsets : UInt64*, n_docs : UInt64, params : MatchParams*,
                          flags : UInt32, out : Hit*, cap : UInt64, doc_sel_offsets : UInt64*, n_selected : UInt64*,
                          n_hits : UInt64*) : Int32
  fun aha_ac_select_batch_device(ac : Ac, d_corpus : UInt8*, d_doc_offsets : UInt64*, n_docs : UInt64, n_bytes : UInt64,
                                 params : MatchParams*, flags : UInt32, d_out : Hit*, cap : UInt64,
                                 d_doc_sel_offsets : UInt64*, n_selected : UInt64*, n_hits : UInt64*, stream : Void*) : Int32
  # replace: the substituted copy of a batch, built on the device from its selection; a table per handle
  type Repl = Void*
  fun aha_repl_create(ac : Ac, blob : UInt8*, offsets : UInt64*, keep_bits : UInt32*, out : Repl*) : Int32
  fun aha_repl_free(table : Repl) : Void
  fun aha_ac_replace_batch(ac : Ac, table : Repl, corpus : UInt8*, doc_offsets : UInt64*, n_docs : UInt64, params : MatchParams*,
                           flags : UInt32, out : UInt8*, cap_bytes : UInt64, doc_out_offsets : UInt64*, n_out_bytes : UInt64*,
                           n_selected : UInt64*, n_hits : UInt64*) : Int32
  fun aha_ac_replace_batch_device(ac : Ac, table : Repl, d_corpus : UInt8*, d_doc_offsets : UInt64*, n_docs : UInt64,
                                  n_bytes : UInt64, params : MatchParams*, flags : UInt32, d_out : UInt8*, cap_bytes : UInt64,
                                  d_doc_out_offsets : UInt64*, n_out_bytes : UInt64*, n_selected : UInt64*, n_hits : UInt64*,
                                  stream : Void*) : Int32
  # records: a batch split at a delimiter byte and at the documents' ends; grep: the documents with a hit (GREP_INVERT: without)
  GREP_INVERT = 1_u32
  fun aha_ac_records_batch(ac : Ac, corpus : UInt8*, doc_offsets : UInt64*, n_docs : UInt64, delim : UInt8, flags : UInt32,
                           rec_offsets : UInt64*, cap_records : UInt64, doc_rec_offsets : UInt64*, n_records : UInt64*) : Int32
  fun aha_ac_records_batch_device(ac : Ac, d_corpus : UInt8*, d_doc_offsets : UInt64*, n_docs : UInt64, n_bytes : UInt64,
                                  delim : UInt8, flags : UInt32, d_rec_offsets : UInt64*, cap_records : UInt64,
                                  d_doc_rec_offsets : UInt64*, n_records : UInt64*, stream : Void*) : Int32
  fun aha_ac_grep_batch(ac : Ac, corpus : UInt8*, doc_offsets : UInt64*, n_docs : UInt64, params : MatchParams*, flags : UInt32,
                        kept_docs : UInt64*, doc_out_offsets : UInt64*, cap_docs : UInt64, out : UInt8*, cap_bytes : UInt64,
                        n_kept : UInt64*, n_out_bytes : UInt64*, n_hits : UInt64*) : Int32
  fun aha_ac_grep_batch_device(ac : Ac, d_corpus : UInt8*, d_doc_offsets : UInt64*, n_docs : UInt64, n_bytes : UInt64,
                               params : MatchParams*, flags : UInt32, d_kept_docs : UInt64*, d_doc_out_offsets : UInt64*,
                               cap_docs : UInt64, d_out : UInt8*, cap_bytes : UInt64, n_kept : UInt64*, n_out_bytes : UInt64*,
                               n_hits : UInt64*, stream : Void*) : Int32
  type Classes = Void*
  # rule grep: with GREP_RULE (beside GREP_INVERT) `params` of the grep entries points to a GrepParams -- cast its address to
  # MatchParams* --, and the documents are kept by the rule over their class counts.  A term: count[class_id] OP num, or with
  # den_bytes > 0 "num hits per den_bytes bytes"; the terms of a group are AND-ed, the groups OR-ed; 1 to 64 terms
  GREP_RULE = 4_u32
  RULE_GE   = 0_u32 # lhs >= rhs
  RULE_LT   = 1_u32 # lhs <  rhs
  struct RuleTerm
    class_id : UInt32
    op : UInt16
    group : UInt16
    num : UInt32
    den_bytes : UInt32
  end
  struct GrepParams
    match : MatchParams # first member: match.struct_size = sizeof(GrepParams)
    classes : Classes   # of this handle
    terms : RuleTerm*   # host memory, in both entries
    n_terms : UInt32    # 1 .. 64
    reserved : UInt32   # 0
    rows : UInt32*      # optional D x C table, as class counts writes it (host entry: host memory; device entry: HBM)
  end
  # excerpts: with GREP_CONTEXT (alone) `params` of the grep entries points to an ExcerptParams -- cast its address to
  # MatchParams* --, and the result is the text around every hit: kept_docs takes the excerpts' first bytes (corpus offsets),
  # doc_out_offsets their offsets into out.  Contexts are byte counts, clipped to the document and snapped to UTF-8 boundaries
  GREP_CONTEXT = 8_u32
  struct ExcerptParams
    match : MatchParams # first member: match.struct_size = sizeof(ExcerptParams)
    before : UInt32     # bytes of context in front of a hit, 0 .. 0x7FFFFFFF
    after : UInt32      # bytes of context behind a hit, 0 .. 0x7FFFFFFF
    flags : UInt32      # 0
    reserved : UInt32   # 0
  end
  # context lines: with GREP_LINES (beside GREP_INVERT) `params` of the grep entries points to a GrepLinesParams -- cast its
  # address to MatchParams* --, and the records around a matching record are kept with it (grep -B, -A, -C), inside the groups
  GREP_LINES = 16_u32
  struct GrepLinesParams
    match : MatchParams     # first member: match.struct_size = sizeof(GrepLinesParams), 88 bytes
    before : UInt32         # records of context in front of a matching record, 0 .. 0x7FFFFFFF
    after : UInt32          # records of context behind it, 0 .. 0x7FFFFFFF
    flags : UInt32          # 0
    reserved : UInt32       # 0
    group_offsets : UInt64* # G + 1 entries or null (host entry: host memory; device entry: HBM)
    n_groups : UInt64       # G; 0 with null
    is_match : UInt8*       # optional, cap_docs entries: 1 where the kept record matched, 0 where it is context
  end
  fun aha_classes_create(ac : Ac, class_ids : UInt32*, offsets : UInt64*, n_classes : UInt32, out : Classes*) : Int32
  fun aha_classes_free(table : Classes) : Void
  fun aha_ac_class_counts_batch(ac : Ac, table : Classes, corpus : UInt8*, doc_offsets : UInt64*, n_docs : UInt64,
                                params : MatchParams*, flags : UInt32, out : UInt32*, n_hits : UInt64*) : Int32
  fun aha_ac_class_counts_batch_device(ac : Ac, table : Classes, d_corpus : UInt8*, d_doc_offsets : UInt64*, n_docs : UInt64,
                                       n_bytes : UInt64, params : MatchParams*, flags : UInt32, d_out : UInt32*, n_hits : UInt64*,
                                       stream : Void*) : Int32
  # feeds: sequences that arrive in pieces across calls (offsets relative to the piece; FEED_CHARS: in characters)
  type Feed = Void*
  FEED_CHARS = 1_u32
  # on a handle folded beyond ASCII (FOLD_SIMPLE, _BMP, _KANA): a folded feed -- every call answers as if the sequence ended with
  # its piece, Lmax + 1 bytes of context; match, count and cover calls (aha_hip.h AHA_FEED_FOLD)
  FEED_FOLD  = 4_u32
  fun aha_feed_open(ac : Ac, n_seqs : UInt32, flags : UInt32, out : Feed*) : Int32
  # a feed with a separator filter: match and count calls report a hit one byte late, finish ends a sequence
  fun aha_feed_open_params(ac : Ac, n_seqs : UInt32, flags : UInt32, params : MatchParams*, out : Feed*) : Int32
  fun aha_feed_finish_batch(f : Feed, seq_ids : UInt32*, n_named : UInt64, out : Hit*, cap : UInt64, seq_hit_offsets : UInt64*,
                            bases : UInt64*, n_hits : UInt64*) : Int32
  fun aha_feed_finish_batch_device(f : Feed, d_seq_ids : UInt32*, n_named : UInt64, d_out : Hit*, cap : UInt64,
                                   d_seq_hit_offsets : UInt64*, d_bases : UInt64*, n_hits : UInt64*, stream : Void*) : Int32
  fun aha_feed_free(f : Feed) : Void
  fun aha_feed_reset(f : Feed, seq : UInt32) : Int32
  fun aha_feed_position(f : Feed, seq : UInt32, bytes : UInt64*, chars : UInt64*) : Int32
  fun aha_feed_match_batch(f : Feed, corpus : UInt8*, piece_offsets : UInt64*, seq_ids : UInt32*, n_pieces : UInt64,
                           out : Hit*, cap : UInt64, piece_hit_offsets : UInt64*, piece_bases : UInt64*,
                           n_hits : UInt64*) : Int32
  fun aha_feed_match_batch_device(f : Feed, d_corpus : UInt8*, d_piece_offsets : UInt64*, d_seq_ids : UInt32*,
                                  n_pieces : UInt64, n_bytes : UInt64, d_out : Hit*, cap : UInt64,
                                  d_piece_hit_offsets : UInt64*, d_piece_bases : UInt64*, n_hits : UInt64*,
                                  stream : Void*) : Int32
  # feed counts: hits per key of the same pieces, the sequences moved on as a match call moves them
  fun aha_feed_count_batch(f : Feed, corpus : UInt8*, piece_offsets : UInt64*, seq_ids : UInt32*, n_pieces : UInt64,
                           flags : UInt32, key_counts : UInt64*, piece_hit_offsets : UInt64*, piece_bases : UInt64*,
                           n_hits : UInt64*) : Int32
  fun aha_feed_count_batch_device(f : Feed, d_corpus : UInt8*, d_piece_offsets : UInt64*, d_seq_ids : UInt32*,
                                  n_pieces : UInt64, n_bytes : UInt64, flags : UInt32, d_key_counts : UInt64*,
                                  d_piece_hit_offsets : UInt64*, d_piece_bases : UInt64*, n_hits : UInt64*,
                                  stream : Void*) : Int32
  # feed cover: the mask and the redacted copy of the same pieces, straddling hits included
  fun aha_feed_cover_batch(f : Feed, corpus : UInt8*, piece_offsets : UInt64*, seq_ids : UInt32*, n_pieces : UInt64,
                           flags : UInt32, mask : UInt32*, redacted : UInt8*, fill : UInt8, piece_back : UInt32*,
                           piece_covered : UInt64*, piece_hit_offsets : UInt64*, piece_bases : UInt64*,
                           n_covered : UInt64*, n_hits : UInt64*) : Int32
  fun aha_feed_cover_batch_device(f : Feed, d_corpus : UInt8*, d_piece_offsets : UInt64*, d_seq_ids : UInt32*,
                                  n_pieces : UInt64, n_bytes : UInt64, flags : UInt32, d_mask : UInt32*,
                                  d_redacted : UInt8*, fill : UInt8, d_piece_back : UInt32*, d_piece_covered : UInt64*,
                                  d_piece_hit_offsets : UInt64*, d_piece_bases : UInt64*, n_covered : UInt64*,
                                  n_hits : UInt64*, stream : Void*) : Int32
  # feed select: the leftmost-longest, non-overlapping hits of the same pieces as far as they are settled (byte feeds)
  FEED_SELECT_FINAL = 1_u32
  FEED_SELECT_TOKENS   = 4_u32 # AHA_FEED_SELECT_TOKENS: the tokens the call settles instead of the selection
  FEED_SELECT_GAP_RUNS = 8_u32 # AHA_FEED_SELECT_GAP_RUNS: only with FEED_SELECT_TOKENS, gaps are not cut into characters
  fun aha_feed_select_batch(f : Feed, corpus : UInt8*, piece_offsets : UInt64*, seq_ids : UInt32*, n_pieces : UInt64,
                            flags : UInt32, out : Hit*, cap : UInt64, piece_sel_offsets : UInt64*, piece_bases : UInt64*,
                            piece_hold : UInt32*, n_selected : UInt64*, n_hits : UInt64*) : Int32
  fun aha_feed_select_batch_device(f : Feed, d_corpus : UInt8*, d_piece_offsets : UInt64*, d_seq_ids : UInt32*,
                                   n_pieces : UInt64, n_bytes : UInt64, flags : UInt32, d_out : Hit*, cap : UInt64,
                                   d_piece_sel_offsets : UInt64*, d_piece_bases : UInt64*, d_piece_hold : UInt32*,
                                   n_selected : UInt64*, n_hits : UInt64*, stream : Void*) : Int32
  # feed replace: the substituted stream of the same pieces, built on the device (byte feeds; a table of the feed's handle)
  FEED_REPLACE_FINAL = FEED_SELECT_FINAL
  fun aha_feed_replace_batch(f : Feed, table : Repl, corpus : UInt8*, piece_offsets : UInt64*, seq_ids : UInt32*,
                             n_pieces : UInt64, flags : UInt32, out : UInt8*, cap_bytes : UInt64, piece_out_offsets : UInt64*,
                             piece_bases : UInt64*, piece_hold : UInt32*, n_out_bytes : UInt64*, n_selected : UInt64*,
                             n_hits : UInt64*) : Int32
  fun aha_feed_replace_batch_device(f : Feed, table : Repl, d_corpus : UInt8*, d_piece_offsets : UInt64*, d_seq_ids : UInt32*,
                                    n_pieces : UInt64, n_bytes : UInt64, flags : UInt32, d_out : UInt8*, cap_bytes : UInt64,
                                    d_piece_out_offsets : UInt64*, d_piece_bases : UInt64*, d_piece_hold : UInt32*,
                                    n_out_bytes : UInt64*, n_selected : UInt64*, n_hits : UInt64*, stream : Void*) : Int32
  # feed grep: the lines of the same pieces that close in the call and have a hit (byte feeds; the caller holds the open line)
  FEED_GREP_FINAL = 2_u32 # (beside GREP_INVERT in the same flags word)
  fun aha_feed_grep_batch(f : Feed, corpus : UInt8*, piece_offsets : UInt64*, seq_ids : UInt32*, n_pieces : UInt64,
                          delim : UInt8, flags : UInt32, kept_recs : UInt64*, rec_out_offsets : UInt64*, cap_recs : UInt64,
                          out : UInt8*, cap_bytes : UInt64, piece_rec_offsets : UInt64*, piece_kept_offsets : UInt64*,
                          piece_hold : UInt32*, piece_head : UInt64*, piece_bases : UInt64*, piece_rec_bases : UInt64*,
                          n_recs : UInt64*, n_kept : UInt64*, n_out_bytes : UInt64*, n_hits : UInt64*) : Int32
  fun aha_feed_grep_batch_device(f : Feed, d_corpus : UInt8*, d_piece_offsets : UInt64*, d_seq_ids : UInt32*,
                                 n_pieces : UInt64, n_bytes : UInt64, delim : UInt8, flags : UInt32, d_kept_recs : UInt64*,
                                 d_rec_out_offsets : UInt64*, cap_recs : UInt64, d_out : UInt8*, cap_bytes : UInt64,
                                 d_piece_rec_offsets : UInt64*, d_piece_kept_offsets : UInt64*, d_piece_hold : UInt32*,
                                 d_piece_head : UInt64*, d_piece_bases : UInt64*, d_piece_rec_bases : UInt64*,
                                 n_recs : UInt64*, n_kept : UInt64*, n_out_bytes : UInt64*, n_hits : UInt64*,
                                 stream : Void*) : Int32
  fun aha_buffer_alloc(device : Int32, bytes : UInt64, d_ptr : Void**) : Int32
  fun aha_buffer_free(device : Int32, d_ptr : Void*) : Int32
  fun aha_buffer_upload(device : Int32, d_dst : Void*, src : Void*, bytes : UInt64) : Int32
  fun aha_buffer_download(device : Int32, dst : Void*, d_src : Void*, bytes : UInt64) : Int32
  type Corpus = Void*
  fun aha_corpus_upload(device : Int32, corpus : UInt8*, doc_offsets : UInt64*, n_docs : UInt64, out : Corpus*) : Int32
  fun aha_corpus_free(c : Corpus) : Void
  fun aha_corpus_bytes(c : Corpus) : UInt8*
  fun aha_corpus_doc_offsets(c : Corpus) : UInt64*
  fun aha_corpus_n_docs(c : Corpus) : UInt64
  fun aha_corpus_n_bytes(c : Corpus) : UInt64
  fun aha_corpus_device(c : Corpus) : Int32

  type Group = Void*
  fun aha_group_compile(key_bytes : UInt8*, key_offsets : UInt64*, n_keys : UInt32,
                        devices : Int32*, n_devices : Int32, flags : UInt32,
                        out : Group*, err_key : UInt32*) : Int32
  fun aha_group_free(g : Group) : Void
  fun aha_group_size(g : Group) : Int32
  fun aha_group_last_error(g : Group) : UInt8*
  fun aha_group_partition(doc_offsets : UInt64*, n_docs : UInt64, n_parts : Int32, bounds : UInt64*) : Int32
  fun aha_group_download_shard(g : Group, shard : Int32, out : Hit*, cap : UInt64, n_hits : UInt64*) : Int32
  fun aha_group_last_timing(g : Group, t : GroupTiming*) : Int32
  # ABI 7: the batch resident on the group's devices
  type GroupCorpus = Void*
  fun aha_group_corpus_upload(g : Group, corpus : UInt8*, doc_offsets : UInt64*, n_docs : UInt64, out_c : GroupCorpus*) : Int32
  fun aha_group_corpus_free(c : GroupCorpus) : Void
  fun aha_group_match_batch_device(g : Group, c : GroupCorpus, params : MatchParams*, doc_hit_offsets : UInt64*,
                                   n_hits : UInt64*) : Int32
  fun aha_group_match_batch(g : Group, corpus : UInt8*, doc_offsets : UInt64*, n_docs : UInt64,
                            params : MatchParams*, out : Hit*, cap : UInt64,
                            doc_hit_offsets : UInt64*, n_hits : UInt64*) : Int32
end

module Aha
  class AC
    E_DUP_KEY  = -4
    E_CAPACITY = -6
    SELECT_TOKENS   = 4_u32 # AHA_SELECT_TOKENS: the tokens of every document instead of the selection
    SELECT_GAP_RUNS = 8_u32 # AHA_SELECT_GAP_RUNS: a gap is one token, not one per character

    getter handle : LibAhaHip::Ac

    def initialize(@handle : LibAhaHip::Ac)
    end

    def finalize
      LibAhaHip.aha_ac_free(@handle)
    end

    # fold_ascii: an ASCII case-insensitive handle -- every call gives what a plain handle compiled from the lower-cased keys
    # gives over the lower-cased text ('A'..'Z' only); ac[id] keeps the spelling given here
    def self.compile(keys : Array(String) | Array(Array(UInt8)) | Array(Bytes), fold_ascii : Bool = false) : self
      blob, offs = pack_keys(keys)
      opts = LibAhaHip::Options.new
      opts.struct_size = sizeof(LibAhaHip::Options).to_u32
      opts.device = -1
      opts.flags = fold_ascii ? LibAhaHip::OPT_FOLD_ASCII : 0_u32
      rc = LibAhaHip.aha_ac_compile(blob.to_slice.to_unsafe, offs.to_unsafe, keys.size.to_u32,
        pointerof(opts), out handle, out bad)
      if rc == E_DUP_KEY
        raise "key:#{keys[bad]} appear twice."
      elsif rc != 0
        raise String.new(LibAhaHip.aha_strerror(rc))
      end
      new(handle)
    end

    # ACX.compile(da : Cedar) src/aha/ac.cr:71 -- see the header for the restriction
    def self.compile(da : Cedar) : self
      keys = Array(String).new
      (0...da.size).each do |id|
        keys << da[id]  # raises for an id freed by Cedar#delete
      end
      compile(keys)
    end

    protected def self.pack_keys(keys)
      blob = IO::Memory.new
      offs = Array(UInt64).new(keys.size + 1)
      offs << 0_u64
      keys.each do |k|
        bytes = k.is_a?(String) ? k.to_slice : (k.is_a?(Bytes) ? k : Slice.new(k.to_unsafe, k.size))
        blob.write bytes
        offs << blob.pos.to_u64
      end
      {blob, offs}
    end

    protected def self.params(chars : Bool, sep : BitArray?, longest : Int32 = 0) : LibAhaHip::MatchParams
      params = LibAhaHip::MatchParams.new
      params.struct_size = sizeof(LibAhaHip::MatchParams).to_u32
      params.char_offsets = chars ? 1 : 0
      params.longest = longest
      if sep
        raise "sep BitArray size > 256 is not supported" if sep.size > 256
        params.sep_size = sep.size
        bits = StaticArray(UInt8, 32).new(0_u8)
        sep.each_with_index { |b, i| bits[i >> 3] |= (1_u8 << (i & 7)) if b }
        params.sep_bits = bits
      end
      params
    end

    # New: all documents in one call (the reference is one sequence per call).  Returns the hits of every document
    # in the reference's order; `chars` selects the String overload's char offsets.
    def match_batch(docs : Array(String) | Array(Bytes), chars : Bool = false, sep : BitArray? = nil) : Array(Array(Hit))
      corpus = IO::Memory.new
      offs = Array(UInt64).new(docs.size + 1)
      offs << 0_u64
      docs.each do |d|
        corpus.write(d.is_a?(String) ? d.to_slice : d)
        offs << corpus.pos.to_u64
      end
      params = AC.params(chars, sep)
      dho = Array(UInt64).new(docs.size + 1, 0_u64)
      cap = (corpus.pos / 4 + 64).to_u64
      result = Array(Array(Hit)).new(docs.size)
      loop do
        out_buf = Pointer(LibAhaHip::Hit).malloc(cap)
        rc = LibAhaHip.aha_ac_match_batch(@handle, corpus.to_slice.to_unsafe, offs.to_unsafe, docs.size.to_u64,
          pointerof(params), out_buf, cap, dho.to_unsafe, out n)
        if rc == E_CAPACITY
          cap = n
          next
        end
        raise String.new(LibAhaHip.aha_last_error(@handle)) if rc != 0
        docs.size.times do |d|
          hits = Array(Hit).new((dho[d + 1] - dho[d]).to_i32)
          (dho[d]...dho[d + 1]).each { |i| hits << Hit.new(out_buf[i].start, out_buf[i].end_, out_buf[i].value) }
          result << hits
        end
        break
      end
      result
    end

    # K: the number of keys (the length of a key-count array)
    def n_keys : Int32
      info = LibAhaHip::Info.new
      info.struct_size = sizeof(LibAhaHip::Info).to_u32
      rc = LibAhaHip.aha_ac_info(@handle, pointerof(info))
      raise String.new(LibAhaHip.aha_strerror(rc)) if rc != 0
      info.n_keys.to_i32
    end

    # Hits per key of match_batch(docs, sep: sep) without the hit list: {key_counts (K entries), doc_hit_offsets}.
    # accumulate: a K-entry array the counts are added to (running totals over many batches); it is what is returned.
    def count_batch(docs : Array(String) | Array(Bytes), sep : BitArray? = nil,
                    accumulate : Array(UInt64)? = nil) : {Array(UInt64), Array(UInt64)}
      corpus = IO::Memory.new
      offs = Array(UInt64).new(docs.size + 1)
      offs << 0_u64
      docs.each do |d|
        corpus.write(d.is_a?(String) ? d.to_slice : d)
        offs << corpus.pos.to_u64
      end
      params = AC.params(false, sep)
      dho = Array(UInt64).new(docs.size + 1, 0_u64)
      kc = accumulate || Array(UInt64).new(n_keys, 0_u64)
      raise ArgumentError.new("accumulate holds #{n_keys} counts") if kc.size != n_keys
      flags = accumulate ? LibAhaHip::COUNT_ACCUMULATE : 0_u32
      rc = LibAhaHip.aha_ac_count_batch(@handle, corpus.to_slice.to_unsafe, offs.to_unsafe, docs.size.to_u64,
        pointerof(params), flags, kc.to_unsafe, dho.to_unsafe, out n)
      raise String.new(LibAhaHip.aha_last_error(@handle)) if rc != 0
      {kc, dho}
    end

    # The documents with every byte inside a hit of match_batch(docs, sep: sep) replaced by `fill`, without the hit list
    # (Aha::AC has no such method; CedarX#gsub is the reference's nearest): -> {redacted documents, covered bytes per document}
    def redact_batch(docs : Array(String) | Array(Bytes), fill : UInt8 = 0x2A_u8, sep : BitArray? = nil) : {Array(Bytes), Array(UInt64)}
      corpus = IO::Memory.new
      offs = Array(UInt64).new(docs.size + 1)
      offs << 0_u64
      docs.each do |d|
        corpus.write(d.is_a?(String) ? d.to_slice : d)
        offs << corpus.pos.to_u64
      end
      params = AC.params(false, sep)
      red = Bytes.new(corpus.pos + 1)
      cov = Array(UInt64).new(docs.size + 1, 0_u64)
      rc = LibAhaHip.aha_ac_cover_batch(@handle, corpus.to_slice.to_unsafe, offs.to_unsafe, docs.size.to_u64,
        pointerof(params), 0_u32, Pointer(UInt32).null, red.to_unsafe, fill, cov.to_unsafe, out n_covered,
        Pointer(UInt64).null)
      raise String.new(LibAhaHip.aha_last_error(@handle)) if rc != 0
      cov.pop
      {(0...docs.size).map { |d| red[offs[d], offs[d + 1] - offs[d]] }, cov}
    end

    # The document x key table of match_batch(docs, sep: sep) without the hit list: per document its {key id, count} pairs,
    # ascending by key id.
    def doc_counts_batch(docs : Array(String) | Array(Bytes), sep : BitArray? = nil) : Array(Array({Int32, UInt32}))
      corpus = IO::Memory.new
      offs = Array(UInt64).new(docs.size + 1)
      offs << 0_u64
      docs.each do |d|
        corpus.write(d.is_a?(String) ? d.to_slice : d)
        offs << corpus.pos.to_u64
      end
      params = AC.params(false, sep)
      dpo = Array(UInt64).new(docs.size + 1, 0_u64)
      rc = LibAhaHip.aha_ac_doc_counts_batch(@handle, corpus.to_slice.to_unsafe, offs.to_unsafe, docs.size.to_u64,
        pointerof(params), Pointer(LibAhaHip::KeyCount).null, 0_u64, dpo.to_unsafe, out n, Pointer(UInt64).null)
      pairs = Pointer(LibAhaHip::KeyCount).malloc(n + 1)
      if rc == E_CAPACITY # n is the required count
        rc = LibAhaHip.aha_ac_doc_counts_batch(@handle, corpus.to_slice.to_unsafe, offs.to_unsafe, docs.size.to_u64,
          pointerof(params), pairs, n, dpo.to_unsafe, out n2, Pointer(UInt64).null)
      end
      raise String.new(LibAhaHip.aha_last_error(@handle)) if rc != 0
      Array.new(docs.size) do |d|
        Array.new((dpo[d + 1] - dpo[d]).to_i) { |i| p = pairs[dpo[d] + i]; {p.key, p.count} }
      end
    end

    # Per document the leftmost-longest, non-overlapping hits of match_batch(docs, sep: sep), ascending by start, as
    # {start, end, value} in byte offsets (Aha::AC has no such method; CedarX#gsub walks the text the same way).
    def select_batch(docs : Array(String) | Array(Bytes), sep : BitArray? = nil, flags : UInt32 = 0_u32) : Array(Array({Int32, Int32, Int32}))
      corpus = IO::Memory.new
      offs = Array(UInt64).new(docs.size + 1)
      offs << 0_u64
      docs.each do |d|
        corpus.write(d.is_a?(String) ? d.to_slice : d)
        offs << corpus.pos.to_u64
      end
      params = AC.params(false, sep)
      dso = Array(UInt64).new(docs.size + 1, 0_u64)
      rc = LibAhaHip.aha_ac_select_batch(@handle, corpus.to_slice.to_unsafe, offs.to_unsafe, docs.size.to_u64,
        pointerof(params), flags, Pointer(LibAhaHip::Hit).null, 0_u64, dso.to_unsafe, out n, Pointer(UInt64).null)
      hits = Pointer(LibAhaHip::Hit).malloc(n + 1)
      if rc == E_CAPACITY # n is the required count; nothing was written
        rc = LibAhaHip.aha_ac_select_batch(@handle, corpus.to_slice.to_unsafe, offs.to_unsafe, docs.size.to_u64,
          pointerof(params), flags, hits, n, dso.to_unsafe, out n2, Pointer(UInt64).null)
      end
      raise String.new(LibAhaHip.aha_last_error(@handle)) if rc != 0
      Array.new(docs.size) do |d|
        Array.new((dso[d + 1] - dso[d]).to_i) { |i| h = hits[dso[d] + i]; {h.start, h.end_, h.value} }
      end
    end

    def select(seq : String | Bytes, sep : BitArray? = nil) : Array({Int32, Int32, Int32})
      select_batch([seq.is_a?(String) ? seq.to_slice : seq], sep)[0]
    end

    # The tokens of seq (aha_ac_select_batch with AHA_SELECT_TOKENS): the selected hits with their key index as value and,
    # between them, one token per character (gap_runs: one per gap) with value -1; {start, end, value} in byte offsets, gap-free.
    def tokens(seq : String | Bytes, sep : BitArray? = nil, gap_runs : Bool = false) : Array({Int32, Int32, Int32})
      flags = SELECT_TOKENS | (gap_runs ? SELECT_GAP_RUNS : 0_u32)
      select_batch([seq.is_a?(String) ? seq.to_slice : seq], sep, flags)[0]
    end

    # A replacement table of this handle (aha_repl_create): validated and uploaded once, used by any number of replace_batch
    # calls.  It may outlive the handle.
    class Replacements
      getter handle : LibAhaHip::Repl

      def initialize(@handle : LibAhaHip::Repl)
      end

      def finalize
        LibAhaHip.aha_repl_free(@handle)
      end
    end

    # repl[k] is key k's replacement (String or Bytes; empty: the hit is deleted), nil keeps the key's hits as they are.  One
    # entry per key.
    def replacements(repl : Array(String | Bytes | Nil)) : Replacements
      blob = IO::Memory.new
      roffs = Array(UInt64).new(repl.size + 1)
      roffs << 0_u64
      keep = Array(UInt32).new((repl.size + 31) // 32, 0_u32)
      repl.each_with_index do |r, k|
        if r.nil?
          keep[k >> 5] |= 1_u32 << (k & 31)
        else
          blob.write(r.is_a?(String) ? r.to_slice : r)
        end
        roffs << blob.pos.to_u64
      end
      rc = LibAhaHip.aha_repl_create(@handle, blob.to_slice.to_unsafe, roffs.to_unsafe, keep.to_unsafe, out table)
      raise String.new(LibAhaHip.aha_last_error(@handle)) if rc != 0
      Replacements.new(table)
    end

    # Every document with the hits of select_batch replaced, built on the device.  Pass the table of `replacements` to use it
    # for many batches; an array makes a table for this call alone.
    def replace_batch(docs : Array(String) | Array(Bytes), repl : Replacements | Array(String | Bytes | Nil),
                      sep : BitArray? = nil) : Array(Bytes)
      table = repl.is_a?(Replacements) ? repl : replacements(repl)
      corpus = IO::Memory.new
      offs = Array(UInt64).new(docs.size + 1)
      offs << 0_u64
      docs.each do |d|
        corpus.write(d.is_a?(String) ? d.to_slice : d)
        offs << corpus.pos.to_u64
      end
      params = AC.params(false, sep)
      doo = Array(UInt64).new(docs.size + 1, 0_u64)
      n = 0_u64
      rc = LibAhaHip.aha_ac_replace_batch(@handle, table.handle, corpus.to_slice.to_unsafe, offs.to_unsafe, docs.size.to_u64,
        pointerof(params), 0_u32, Pointer(UInt8).null, 0_u64, doo.to_unsafe, pointerof(n), Pointer(UInt64).null,
        Pointer(UInt64).null)
      bytes = Bytes.empty
      if rc == E_CAPACITY # n is the required size; nothing was written
        bytes = Bytes.new(n)
        rc = LibAhaHip.aha_ac_replace_batch(@handle, table.handle, corpus.to_slice.to_unsafe, offs.to_unsafe, docs.size.to_u64,
          pointerof(params), 0_u32, bytes.to_unsafe, n, doo.to_unsafe, pointerof(n), Pointer(UInt64).null, Pointer(UInt64).null)
      end
      raise String.new(LibAhaHip.aha_last_error(@handle)) if rc != 0
      Array.new(docs.size) { |d| bytes[doo[d], doo[d + 1] - doo[d]] }
    end

    # The offsets of the records of one sequence: split at the delimiter byte, every record with its delimiter, none empty
    # (aha_ac_records_batch).  R + 1 offsets, 0 first: a doc_offsets for the batch entry points.
    def records(seq : String | Bytes, delim : UInt8 = 10_u8) : Array(UInt64)
      bytes = seq.is_a?(String) ? seq.to_slice : seq
      offs = [0_u64, bytes.size.to_u64]
      n = 0_u64
      rc = LibAhaHip.aha_ac_records_batch(@handle, bytes.to_unsafe, offs.to_unsafe, 1_u64, delim, 0_u32, Pointer(UInt64).null,
        0_u64, Pointer(UInt64).null, pointerof(n))
      rec = Array(UInt64).new(n + 1, 0_u64)
      if rc == E_CAPACITY || rc == 0 # n is the required count; nothing was written
        rc = LibAhaHip.aha_ac_records_batch(@handle, bytes.to_unsafe, offs.to_unsafe, 1_u64, delim, 0_u32, rec.to_unsafe, n,
          Pointer(UInt64).null, pointerof(n))
      end
      raise String.new(LibAhaHip.aha_last_error(@handle)) if rc != 0
      rec
    end

    # The records of seq that have a hit of match(record, sep: sep), each with its delimiter; invert: those that have none
    # (aha_ac_records_batch, then aha_ac_grep_batch over the records; Aha::AC has no such method).
    # before, after (context: both): grep -B, -A, -C -- that many records around a matching one are kept with it
    # (aha_ac_grep_batch with GREP_LINES; the sequence is one group).  Without them the call is plain grep's.
    def grep(seq : String | Bytes, delim : UInt8 = 10_u8, invert : Bool = false, sep : BitArray? = nil, before : UInt32 = 0_u32,
             after : UInt32 = 0_u32, context : UInt32? = nil) : Array(Bytes)
      bytes = seq.is_a?(String) ? seq.to_slice : seq
      rec = records(bytes, delim)
      n_rec = (rec.size - 1).to_u64
      if c = context
        raise ArgumentError.new("context sets both sides: give it, or before and after") if before != 0 || after != 0
        before = after = c
      end
      return grep_lines(bytes, rec, n_rec, invert, sep, before, after) if before != 0 || after != 0
      params = AC.params(false, sep)
      flags = invert ? LibAhaHip::GREP_INVERT : 0_u32
      nk = 0_u64
      nb = 0_u64
      # a sizing call: no buffer, no capacity -- it succeeds and gives both counts
      rc = LibAhaHip.aha_ac_grep_batch(@handle, bytes.to_unsafe, rec.to_unsafe, n_rec, pointerof(params), flags,
        Pointer(UInt64).null, Pointer(UInt64).null, 0_u64, Pointer(UInt8).null, 0_u64, pointerof(nk), pointerof(nb),
        Pointer(UInt64).null)
      raise String.new(LibAhaHip.aha_last_error(@handle)) if rc != 0
      doo = Array(UInt64).new(nk + 1, 0_u64)
      out_bytes = Bytes.new(nb)
      rc = LibAhaHip.aha_ac_grep_batch(@handle, bytes.to_unsafe, rec.to_unsafe, n_rec, pointerof(params), flags,
        Pointer(UInt64).null, doo.to_unsafe, nk, nb > 0 ? out_bytes.to_unsafe : Pointer(UInt8).null, nb, pointerof(nk),
        pointerof(nb), Pointer(UInt64).null)
      raise String.new(LibAhaHip.aha_last_error(@handle)) if rc != 0
      Array.new(nk.to_i32) { |i| out_bytes[doo[i], doo[i + 1] - doo[i]] }
    end

    # grep's context form over the records rec of bytes (one group): the sizing call, then the kept records' bytes
    private def grep_lines(bytes : Bytes, rec : Array(UInt64), n_rec : UInt64, invert : Bool, sep : BitArray?, before : UInt32,
                           after : UInt32) : Array(Bytes)
      lp = LibAhaHip::GrepLinesParams.new
      lp.match = AC.params(false, sep)
      lp.match.struct_size = sizeof(LibAhaHip::GrepLinesParams).to_u32
      lp.before = before
      lp.after = after
      lp.flags = 0_u32
      lp.reserved = 0_u32
      lp.group_offsets = Pointer(UInt64).null
      lp.n_groups = 0_u64
      lp.is_match = Pointer(UInt8).null
      params = pointerof(lp).as(LibAhaHip::MatchParams*)
      flags = LibAhaHip::GREP_LINES | (invert ? LibAhaHip::GREP_INVERT : 0_u32)
      nk = 0_u64
      nb = 0_u64
      rc = LibAhaHip.aha_ac_grep_batch(@handle, bytes.to_unsafe, rec.to_unsafe, n_rec, params, flags, Pointer(UInt64).null,
        Pointer(UInt64).null, 0_u64, Pointer(UInt8).null, 0_u64, pointerof(nk), pointerof(nb), Pointer(UInt64).null)
      raise String.new(LibAhaHip.aha_last_error(@handle)) if rc != 0
      doo = Array(UInt64).new(nk + 1, 0_u64)
      out_bytes = Bytes.new(nb)
      rc = LibAhaHip.aha_ac_grep_batch(@handle, bytes.to_unsafe, rec.to_unsafe, n_rec, params, flags, Pointer(UInt64).null,
        doo.to_unsafe, nk, nb > 0 ? out_bytes.to_unsafe : Pointer(UInt8).null, nb, pointerof(nk), pointerof(nb),
        Pointer(UInt64).null)
      raise String.new(LibAhaHip.aha_last_error(@handle)) if rc != 0
      Array.new(nk.to_i32) { |i| out_bytes[doo[i], doo[i + 1] - doo[i]] }
    end

    # The records of seq whose class counts pass a rule (aha_ac_grep_batch with GREP_RULE over the records); invert: those that
    # do not.  table: a LibAhaHip::Classes of this handle (aha_classes_create); terms: {class_id, op, group, num, den_bytes}
    # each, op RULE_GE or RULE_LT.  A record passes when some group has all its terms true.
    def grep_rule(seq : String | Bytes, table : LibAhaHip::Classes,
                  terms : Array({UInt32, UInt32, UInt16, UInt32, UInt32}), delim : UInt8 = 10_u8, invert : Bool = false,
                  sep : BitArray? = nil) : Array(Bytes)
      bytes = seq.is_a?(String) ? seq.to_slice : seq
      rec = records(bytes, delim)
      n_rec = (rec.size - 1).to_u64
      packed = terms.map do |t|
        rt = LibAhaHip::RuleTerm.new
        rt.class_id = t[0]
        rt.op = t[1].to_u16
        rt.group = t[2]
        rt.num = t[3]
        rt.den_bytes = t[4]
        rt
      end
      gp = LibAhaHip::GrepParams.new
      gp.match = AC.params(false, sep)
      gp.match.struct_size = sizeof(LibAhaHip::GrepParams).to_u32
      gp.classes = table
      gp.terms = packed.to_unsafe
      gp.n_terms = packed.size.to_u32
      gp.reserved = 0_u32
      gp.rows = Pointer(UInt32).null
      params = pointerof(gp).as(LibAhaHip::MatchParams*)
      flags = LibAhaHip::GREP_RULE | (invert ? LibAhaHip::GREP_INVERT : 0_u32)
      nk = 0_u64
      nb = 0_u64
      rc = LibAhaHip.aha_ac_grep_batch(@handle, bytes.to_unsafe, rec.to_unsafe, n_rec, params, flags,
        Pointer(UInt64).null, Pointer(UInt64).null, 0_u64, Pointer(UInt8).null, 0_u64, pointerof(nk), pointerof(nb),
        Pointer(UInt64).null)
      raise String.new(LibAhaHip.aha_last_error(@handle)) if rc != 0
      doo = Array(UInt64).new(nk + 1, 0_u64)
      out_bytes = Bytes.new(nb)
      rc = LibAhaHip.aha_ac_grep_batch(@handle, bytes.to_unsafe, rec.to_unsafe, n_rec, params, flags,
        Pointer(UInt64).null, doo.to_unsafe, nk, nb > 0 ? out_bytes.to_unsafe : Pointer(UInt8).null, nb, pointerof(nk),
        pointerof(nb), Pointer(UInt64).null)
      raise String.new(LibAhaHip.aha_last_error(@handle)) if rc != 0
      Array.new(nk.to_i32) { |i| out_bytes[doo[i], doo[i + 1] - doo[i]] }
    end

    # The hits of match(seq, sep) in their context (aha_ac_grep_batch with GREP_CONTEXT over the one document seq): `before`
    # bytes in front of every hit and `after` behind it, snapped outwards to UTF-8 character boundaries, neighbouring contexts
    # merged; {first byte, bytes} per excerpt, ascending.
    def excerpts(seq : String | Bytes, before : UInt32, after : UInt32 = before, sep : BitArray? = nil) : Array({UInt64, Bytes})
      bytes = seq.is_a?(String) ? seq.to_slice : seq
      offs = [0_u64, bytes.size.to_u64]
      ep = LibAhaHip::ExcerptParams.new
      ep.match = AC.params(false, sep)
      ep.match.struct_size = sizeof(LibAhaHip::ExcerptParams).to_u32
      ep.before = before
      ep.after = after
      ep.flags = 0_u32
      ep.reserved = 0_u32
      params = pointerof(ep).as(LibAhaHip::MatchParams*)
      nk = 0_u64
      nb = 0_u64
      rc = LibAhaHip.aha_ac_grep_batch(@handle, bytes.to_unsafe, offs.to_unsafe, 1_u64, params, LibAhaHip::GREP_CONTEXT,
        Pointer(UInt64).null, Pointer(UInt64).null, 0_u64, Pointer(UInt8).null, 0_u64, pointerof(nk), pointerof(nb),
        Pointer(UInt64).null)
      raise String.new(LibAhaHip.aha_last_error(@handle)) if rc != 0
      starts = Array(UInt64).new(nk + 1, 0_u64)
      oo = Array(UInt64).new(nk + 1, 0_u64)
      out_bytes = Bytes.new(nb)
      rc = LibAhaHip.aha_ac_grep_batch(@handle, bytes.to_unsafe, offs.to_unsafe, 1_u64, params, LibAhaHip::GREP_CONTEXT,
        starts.to_unsafe, oo.to_unsafe, nk, nb > 0 ? out_bytes.to_unsafe : Pointer(UInt8).null, nb, pointerof(nk),
        pointerof(nb), Pointer(UInt64).null)
      raise String.new(LibAhaHip.aha_last_error(@handle)) if rc != 0
      Array.new(nk.to_i32) { |i| {starts[i], out_bytes[oo[i], oo[i + 1] - oo[i]]} }
    end

    private def run(seq : Bytes, chars : Bool, sep : BitArray?, longest : Int32 = 0, &block)
      params = AC.params(chars, sep, longest)
      cap = (seq.size / 4 + 64).to_u64
      loop do
        out_buf = Pointer(LibAhaHip::Hit).malloc(cap)
        rc = LibAhaHip.aha_ac_match_bytes(@handle, seq.to_unsafe, seq.size.to_u64, pointerof(params),
          out_buf, cap, out n)
        if rc == E_CAPACITY
          cap = n
          next
        end
        raise String.new(LibAhaHip.aha_last_error(@handle)) if rc != 0
        n.times { |i| yield Hit.new(out_buf[i].start, out_buf[i].end_, out_buf[i].value) }
        break
      end
    end

    def match(seq : Bytes | Array(UInt8), &block)
      bytes = seq.is_a?(Bytes) ? seq : Slice.new(seq.to_unsafe, seq.size)
      run(bytes, false, nil) { |hit| yield hit }
    end

    def match(seq : String, &block)
      run(seq.to_slice, true, nil) { |hit| yield hit }
    end

    def match(seq : Array(Char) | Slice(Char), &block)
      run(String.build { |s| seq.each { |c| s << c } }.to_slice, true, nil) { |hit| yield hit }
    end

    def match(seq : Bytes | Array(UInt8), sep : BitArray, &block)
      bytes = seq.is_a?(Bytes) ? seq : Slice.new(seq.to_unsafe, seq.size)
      run(bytes, false, sep) { |hit| yield hit }
    end

    def match(seq : String, sep : BitArray, &block)
      run(seq.to_slice, true, sep) { |hit| yield hit }
    end

    # ACX#match_longest src/aha/ac.cr:297-319.  Cedar's stale END flags (cedar.cr:642-648) ARE reproduced: the library
    # replays Cedar's inserts from the keys on the first match_longest call of a handle (aha_amd/csrc/cedar_replay.cpp);
    # NUL bytes in the text behave as in the reference (value nodes, kernels.hip)
    def match_longest(seq : Bytes | Array(UInt8), intersectable = false, &block)
      bytes = seq.is_a?(Bytes) ? seq : Slice.new(seq.to_unsafe, seq.size)
      run(bytes, false, nil, intersectable ? 2 : 1) { |hit| yield hit }
    end

    def match_longest(seq : String, intersectable = false, &block)
      run(seq.to_slice, true, nil, intersectable ? 2 : 1) { |hit| yield hit }
    end

    def match_longest(seq : Array(Char) | Slice(Char), intersectable = false, &block)
      run(String.build { |s| seq.each { |c| s << c } }.to_slice, true, nil, intersectable ? 2 : 1) { |hit| yield hit }
    end

    # src/aha/ac.cr:342-364: unlike the String overload the neighbour tests look at the neighbouring CHAR's code
    # point (`chr.ord < sep.size && !sep[chr.ord]`), so they are applied here to the unfiltered byte hits.
    def match(seq : Array(Char) | Slice(Char), sep : BitArray, &block)
      raise "sep BitArray size > 256 is not supported" if sep.size > 256
      str = String.build { |s| seq.each { |c| s << c } }
      char_of_byte = Array(Int32).new(str.bytesize)
      seq.each_with_index { |c, i| c.bytesize.times { char_of_byte << i } }
      run(str.to_slice, false, nil) do |hit|
        chr_idx = char_of_byte[hit.end - 1]
        if chr_idx + 1 < seq.size
          chr = seq[chr_idx + 1]
          next if chr.ord < sep.size && !sep[chr.ord]
        end
        if hit.start > 0
          chr = seq[char_of_byte[hit.start] - 1]
          next if chr.ord < sep.size && !sep[chr.ord]
        end
        yield Hit.new(char_of_byte[hit.start], char_of_byte[hit.end - 1] + 1, hit.value)
      end
    end

    # AC#to_io / AC.from_io (src/aha/ac.cr:45-60) on the library's own container
    def to_io(io : IO, format : IO::ByteFormat = IO::ByteFormat::LittleEndian)
      n = LibAhaHip.aha_ac_save(@handle, Pointer(Void).null, 0_u64)
      raise "save failed" if n < 0
      buf = Bytes.new(n)
      LibAhaHip.aha_ac_save(@handle, buf.to_unsafe.as(Void*), n.to_u64)
      io.write buf
    end

    # (the container stores the keys as spelled and no options: say fold_ascii again)
    def self.from_io(io : IO, format : IO::ByteFormat = IO::ByteFormat::LittleEndian, fold_ascii : Bool = false) : self
      data = io.gets_to_end.to_slice
      opts = LibAhaHip::Options.new
      opts.struct_size = sizeof(LibAhaHip::Options).to_u32
      opts.device = -1
      opts.flags = fold_ascii ? LibAhaHip::OPT_FOLD_ASCII : 0_u32
      rc = LibAhaHip.aha_ac_load(data.to_unsafe.as(Void*), data.size.to_u64, pointerof(opts), out h)
      raise String.new(LibAhaHip.aha_strerror(rc)) if rc != 0
      new(h)
    end

    def fold_ascii? : Bool
      (LibAhaHip.aha_ac_flags(@handle) & LibAhaHip::OPT_FOLD_ASCII) != 0
    end

    def [](sid : Int) : String
      n = LibAhaHip.aha_ac_key(@handle, sid.to_i32, Pointer(UInt8).null, 0)
      raise IndexError.new if n < 0
      buf = Bytes.new(n)
      LibAhaHip.aha_ac_key(@handle, sid.to_i32, buf.to_unsafe, n)
      String.new(buf)
    end

    def [](key : String) : Int32
      r = LibAhaHip.aha_ac_id(@handle, key.to_unsafe, key.bytesize)
      raise IndexError.new if r < 0
      r
    end
  end

  # `Aha::ACBig = ACX(Int64)` (src/aha/ac.cr:9) differs from `Aha::AC` only in the width of its node ids: what `#match` yields
  # is the same `Hit` with an Int32 value (`val.to_i32`, ac.cr:273).  The library's own numbering has no such limit below
  # 2^31 keys, so one class answers for both names.
  alias ACBig = AC

  # n_seqs sequences matched piece by piece (aha_feed_*): #match(seq, piece) yields exactly the hits one match over the whole
  # sequence so far reports with an end inside the piece, with absolute offsets.  (Uncompiled: no Crystal toolchain was at
  # hand when it was written; tests/test_feed_host.py checks that the lib block binds every entry point.)  Hit holds Int32
  # offsets: past 2^31 bytes of a sequence use aha_feed_match_batch, whose offsets are relative to the piece.
  class Feed
    def initialize(ac : AC, n_seqs : Int, chars : Bool = false, fold : Bool = false)
      @ac = ac
      flags = (chars ? LibAhaHip::FEED_CHARS : 0_u32) | (fold ? LibAhaHip::FEED_FOLD : 0_u32)
      rc = LibAhaHip.aha_feed_open(ac.handle, n_seqs.to_u32, flags, out h)
      raise String.new(LibAhaHip.aha_strerror(rc)) if rc != 0
      @handle = h
    end

    # A feed whose #match and #count apply the separator filter of match(seq, sep) to the whole sequence
    # (aha_feed_open_params): a hit is reported once the byte behind it is known, #finish ends a sequence.
    def initialize(ac : AC, n_seqs : Int, sep : BitArray)
      @ac = ac
      raise "sep BitArray size > 256 is not supported" if sep.size > 256
      params = LibAhaHip::MatchParams.new
      params.struct_size = sizeof(LibAhaHip::MatchParams).to_u32
      params.sep_size = sep.size
      bits = StaticArray(UInt8, 32).new(0_u8)
      sep.each_with_index { |b, i| bits[i >> 3] |= (1_u8 << (i & 7)) if b }
      params.sep_bits = bits
      rc = LibAhaHip.aha_feed_open_params(ac.handle, n_seqs.to_u32, 0_u32, pointerof(params), out h)
      raise String.new(LibAhaHip.aha_last_error(ac.handle)) if rc != 0
      @handle = h
    end

    # A longest feed (aha_feed_open_params with longest = 1 | 2), the mirror of AC#match_longest(seq, intersectable) for a
    # sequence in pieces: #match gives the hits of match_longest(whole sequence) that are yielded at a byte of the piece -- a
    # hit may lie wholly in earlier pieces --, #finish the one hit still pending; #count, #select and the other call families
    # raise on such a feed.  Feed.match_longest(ac, n_seqs, intersectable)
    def initialize(ac : AC, n_seqs : Int, *, longest : Int32)
      @ac = ac
      params = LibAhaHip::MatchParams.new
      params.struct_size = sizeof(LibAhaHip::MatchParams).to_u32
      params.longest = longest
      rc = LibAhaHip.aha_feed_open_params(ac.handle, n_seqs.to_u32, 0_u32, pointerof(params), out h)
      raise String.new(LibAhaHip.aha_last_error(ac.handle)) if rc != 0
      @handle = h
    end

    def self.match_longest(ac : AC, n_seqs : Int, intersectable : Bool = false) : Feed
      new(ac, n_seqs, longest: intersectable ? 2 : 1)
    end

    # The sequence ends here (a feed with a separator filter: the surviving hits that end with it; a longest feed: the hit
    # still pending), with absolute offsets; it starts again at length 0.
    def finish(seq : Int) : Array(Hit)
      ids = [seq.to_u32]
      cap = 16_u64
      loop do
        buf = Slice(LibAhaHip::Hit).new(cap.to_i32)
        base = 0_u64
        rc = LibAhaHip.aha_feed_finish_batch(@handle, ids.to_unsafe, 1_u64, buf.to_unsafe, cap, Pointer(UInt64).null,
          pointerof(base), out n)
        if rc == -6 # AHA_E_CAPACITY: n is the exact count, the sequence has not restarted
          cap = n
          next
        end
        raise String.new(LibAhaHip.aha_last_error(@ac.handle)) if rc != 0
        b = base.to_i32 # (raises OverflowError past 2^31)
        return Array(Hit).new(n.to_i32) { |i| Hit.new(buf[i].start + b, buf[i].end_ + b, buf[i].value) }
      end
    end

    def finalize
      LibAhaHip.aha_feed_free(@handle)
    end

    def reset(seq : Int? = nil)
      rc = LibAhaHip.aha_feed_reset(@handle, seq ? seq.to_u32 : UInt32::MAX)
      raise String.new(LibAhaHip.aha_strerror(rc)) if rc != 0
    end

    # {bytes, chars} fed to the sequence so far
    def position(seq : Int) : {UInt64, UInt64}
      rc = LibAhaHip.aha_feed_position(@handle, seq.to_u32, out b, out c)
      raise String.new(LibAhaHip.aha_strerror(rc)) if rc != 0
      {b, c}
    end

    def match(seq : Int, piece : Bytes | String) : Array(Hit)
      bytes = piece.is_a?(String) ? piece.to_slice : piece
      offs = [0_u64, bytes.size.to_u64]
      ids = [seq.to_u32]
      cap = (bytes.size / 4 + 64).to_u64
      loop do
        buf = Slice(LibAhaHip::Hit).new(cap.to_i32)
        base = 0_u64
        rc = LibAhaHip.aha_feed_match_batch(@handle, bytes.to_unsafe, offs.to_unsafe, ids.to_unsafe, 1_u64, buf.to_unsafe,
          cap, nil, pointerof(base), out n)
        if rc == -6 # AHA_E_CAPACITY: n is the exact count, the feed is unchanged
          cap = n
          next
        end
        raise String.new(LibAhaHip.aha_last_error(@ac.handle)) if rc != 0
        b = base.to_i32 # (raises OverflowError past 2^31)
        return Array(Hit).new(n.to_i32) { |i| Hit.new(buf[i].start + b, buf[i].end_ + b, buf[i].value) }
      end
    end

    # The selected hits (leftmost-longest, non-overlapping, as AC#select of the whole sequence) that the next piece of one
    # sequence settles, with absolute offsets: {hits, hold} -- hold: the bytes at the end of the sequence whose fate is still
    # open.  final: the piece is the last of its sequence; everything settles and the sequence starts again from length 0.
    # Byte feeds only, and only for sequences fed through select since their reset.  (Uncompiled, as the rest of this class;
    # tests/test_feed_select_host.py checks that the lib block binds both entry points.)
    def select(seq : Int, piece : Bytes | String, final : Bool = false) : {Array(Hit), UInt32}
      select_flags(seq, piece, final ? LibAhaHip::FEED_SELECT_FINAL : 0_u32)
    end

    # The tokens (dictionary segmentation, as AC#tokens of the whole sequence) that the next piece of one sequence settles
    # (aha_feed_select_batch with AHA_FEED_SELECT_TOKENS), with absolute offsets: {tokens, hold} -- value: the key or -1;
    # hold: the bytes behind the token cursor, which no token holds yet (a character whose next lead byte has not arrived).
    # gap_runs: gaps are not cut into characters and come in parts.  final: everything is reported and the sequence starts
    # again from length 0.  Byte feeds only, and only for sequences fed through token calls since their reset or final call.
    def tokens(seq : Int, piece : Bytes | String, final : Bool = false, gap_runs : Bool = false) : {Array(Hit), UInt32}
      flags = LibAhaHip::FEED_SELECT_TOKENS | (final ? LibAhaHip::FEED_SELECT_FINAL : 0_u32) |
              (gap_runs ? LibAhaHip::FEED_SELECT_GAP_RUNS : 0_u32)
      select_flags(seq, piece, flags)
    end

    private def select_flags(seq : Int, piece : Bytes | String, flags : UInt32) : {Array(Hit), UInt32}
      bytes = piece.is_a?(String) ? piece.to_slice : piece
      offs = [0_u64, bytes.size.to_u64]
      ids = [seq.to_u32]
      cap = 64_u64
      loop do
        buf = Slice(LibAhaHip::Hit).new(cap.to_i32)
        base = 0_u64
        hold = 0_u32
        rc = LibAhaHip.aha_feed_select_batch(@handle, bytes.to_unsafe, offs.to_unsafe, ids.to_unsafe, 1_u64, flags,
          buf.to_unsafe, cap, Pointer(UInt64).null, pointerof(base), pointerof(hold), out n, Pointer(UInt64).null)
        if rc == -6 # AHA_E_CAPACITY: n is the exact count, the feed is unchanged
          cap = n
          next
        end
        raise String.new(LibAhaHip.aha_last_error(@ac.handle)) if rc != 0
        b = base.to_i32 # (raises OverflowError past 2^31)
        return {Array(Hit).new(n.to_i32) { |i| Hit.new(buf[i].start + b, buf[i].end_ + b, buf[i].value) }, hold}
      end
    end

    # The next piece of one sequence substituted on the device: {bytes, hold} -- the substituted bytes that can no longer
    # change (the sequence from the old select cursor to the new one, every hit settled in between replaced as the table
    # says) and the bytes at the end of the sequence that no result holds yet.  final: the piece is the last of its
    # sequence; the rest comes out and the sequence starts again from length 0.  The results of a sequence's pieces,
    # concatenated, are AC#replace_batch of the whole.  (Uncompiled, as the rest of this class;
    # tests/test_feed_replace_host.py checks that the lib block binds both entry points.)
    def replace(seq : Int, piece : Bytes | String, table : AC::Replacements, final : Bool = false) : {Bytes, UInt32}
      bytes = piece.is_a?(String) ? piece.to_slice : piece
      offs = [0_u64, bytes.size.to_u64]
      ids = [seq.to_u32]
      flags = final ? LibAhaHip::FEED_REPLACE_FINAL : 0_u32
      hold = 0_u32
      # a sizing call: AHA_E_CAPACITY (-6) gives the exact size and changes nothing
      rc = LibAhaHip.aha_feed_replace_batch(@handle, table.handle, bytes.to_unsafe, offs.to_unsafe, ids.to_unsafe, 1_u64, flags,
        Pointer(UInt8).null, 0_u64, Pointer(UInt64).null, Pointer(UInt64).null, pointerof(hold), out n,
        Pointer(UInt64).null, Pointer(UInt64).null)
      buf = Bytes.new(n.to_i32)
      if rc == -6
        rc = LibAhaHip.aha_feed_replace_batch(@handle, table.handle, bytes.to_unsafe, offs.to_unsafe, ids.to_unsafe, 1_u64, flags,
          buf.to_unsafe, n, Pointer(UInt64).null, Pointer(UInt64).null, pointerof(hold), out n2,
          Pointer(UInt64).null, Pointer(UInt64).null)
      end
      raise String.new(LibAhaHip.aha_last_error(@ac.handle)) if rc != 0
      {buf, hold}
    end

    # The next piece of one sequence grepped on the device: {lines, head, hold} -- the piece's fragments that close with it and
    # are kept (each with its delimiter), the held bytes to emit in front of the first of them (the line that was open), and
    # the bytes at the end of the piece that belong to the line left open: the caller keeps those (held += piece when
    # hold == piece.size, else held = the piece's last hold bytes).  final: the piece is the last of its sequence; the open
    # line closes and the sequence starts again from length 0.  (Uncompiled, as the rest of this class;
    # tests/test_feed_grep_host.py checks that the lib block binds both entry points.)
    def grep(seq : Int, piece : Bytes | String, delim : UInt8 = 10_u8, invert : Bool = false,
             final : Bool = false) : {Array(Bytes), UInt64, UInt32}
      bytes = piece.is_a?(String) ? piece.to_slice : piece
      offs = [0_u64, bytes.size.to_u64]
      ids = [seq.to_u32]
      flags = (invert ? LibAhaHip::GREP_INVERT : 0_u32) | (final ? LibAhaHip::FEED_GREP_FINAL : 0_u32)
      hold = 0_u32
      head = 0_u64
      # a call with no room: AHA_E_CAPACITY (-6) gives both sizes and changes nothing
      none = Bytes.new(1)
      roo = Array(UInt64).new(1, 0_u64)
      rc = LibAhaHip.aha_feed_grep_batch(@handle, bytes.to_unsafe, offs.to_unsafe, ids.to_unsafe, 1_u64, delim, flags,
        Pointer(UInt64).null, roo.to_unsafe, 0_u64, none.to_unsafe, 0_u64, Pointer(UInt64).null, Pointer(UInt64).null,
        pointerof(hold), pointerof(head), Pointer(UInt64).null, Pointer(UInt64).null, Pointer(UInt64).null, out nk, out nb,
        Pointer(UInt64).null)
      buf = Bytes.new(nb.to_i32)
      if rc == -6
        roo = Array(UInt64).new(nk.to_i32 + 1, 0_u64)
        rc = LibAhaHip.aha_feed_grep_batch(@handle, bytes.to_unsafe, offs.to_unsafe, ids.to_unsafe, 1_u64, delim, flags,
          Pointer(UInt64).null, roo.to_unsafe, nk, buf.to_unsafe, nb, Pointer(UInt64).null, Pointer(UInt64).null,
          pointerof(hold), pointerof(head), Pointer(UInt64).null, Pointer(UInt64).null, Pointer(UInt64).null, out nk2, out nb2,
          Pointer(UInt64).null)
      end
      raise String.new(LibAhaHip.aha_last_error(@ac.handle)) if rc != 0
      {Array(Bytes).new(roo.size - 1) { |i| buf[roo[i].to_i32, (roo[i + 1] - roo[i]).to_i32] }, head, hold}
    end

    # Hits per key of match on the same pieces, without the hit list: {key_counts (K entries), piece_hit_offsets,
    # piece_bases}.  pieces: {seq, piece} pairs, each sequence at most once.  accumulate: a K-entry array the counts are
    # added to (running totals over a stream); it is what is returned, and a call that raises leaves it as it was.
    def count_batch(pieces : Array({Int32, Bytes | String}),
                    accumulate : Array(UInt64)? = nil) : {Array(UInt64), Array(UInt64), Array(UInt64)}
      corpus = IO::Memory.new
      offs = Array(UInt64).new(pieces.size + 1)
      offs << 0_u64
      ids = Array(UInt32).new(pieces.size)
      pieces.each do |(seq, piece)|
        corpus.write(piece.is_a?(String) ? piece.to_slice : piece)
        offs << corpus.pos.to_u64
        ids << seq.to_u32
      end
      k = @ac.n_keys
      kc = accumulate ? accumulate.dup : Array(UInt64).new(k, 0_u64)
      raise ArgumentError.new("accumulate holds #{k} counts") if kc.size != k
      pho = Array(UInt64).new(pieces.size + 1, 0_u64)
      bases = Array(UInt64).new(pieces.size, 0_u64)
      flags = accumulate ? LibAhaHip::COUNT_ACCUMULATE : 0_u32
      rc = LibAhaHip.aha_feed_count_batch(@handle, corpus.to_slice.to_unsafe, offs.to_unsafe, ids.to_unsafe,
        pieces.size.to_u64, flags, kc.to_unsafe, pho.to_unsafe, bases.to_unsafe, out n)
      raise String.new(LibAhaHip.aha_last_error(@ac.handle)) if rc != 0
      accumulate.replace(kc) if accumulate
      {accumulate || kc, pho, bases}
    end

    # (the call behind cover_batch / redact_batch) -> {mask, redacted, piece_back, piece_covered}
    private def cover_call(pieces : Array({Int32, Bytes | String}), want_mask : Bool, want_redacted : Bool,
                           fill : UInt8) : {Array(UInt32), Bytes, Array(UInt32), Array(UInt64)}
      corpus = IO::Memory.new
      offs = Array(UInt64).new(pieces.size + 1)
      offs << 0_u64
      ids = Array(UInt32).new(pieces.size)
      pieces.each do |(seq, piece)|
        corpus.write(piece.is_a?(String) ? piece.to_slice : piece)
        offs << corpus.pos.to_u64
        ids << seq.to_u32
      end
      n = corpus.pos
      mask = Array(UInt32).new(want_mask ? (n + 31) // 32 : 0, 0_u32)
      red = Bytes.new(want_redacted ? n : 0)
      back = Array(UInt32).new(pieces.size, 0_u32)
      cov = Array(UInt64).new(pieces.size, 0_u64)
      rc = LibAhaHip.aha_feed_cover_batch(@handle, corpus.to_slice.to_unsafe, offs.to_unsafe, ids.to_unsafe,
        pieces.size.to_u64, 0_u32, want_mask ? mask.to_unsafe : Pointer(UInt32).null,
        want_redacted ? red.to_unsafe : Pointer(UInt8).null, fill, back.to_unsafe, cov.to_unsafe,
        Pointer(UInt64).null, Pointer(UInt64).null, out n_covered, out n_hits)
      raise String.new(LibAhaHip.aha_last_error(@ac.handle)) if rc != 0
      {mask, red, back, cov}
    end

    # Which bytes of the pieces lie inside a hit of their sequences, without the hit list: {mask, piece_back,
    # piece_covered}.  Bit j of the batch is word j >> 5, bit j & 31; piece_back[d]: the bytes in front of piece d that lie
    # inside a hit ending in it.  pieces: {seq, piece} pairs, each sequence at most once.
    def cover_batch(pieces : Array({Int32, Bytes | String})) : {Array(UInt32), Array(UInt32), Array(UInt64)}
      mask, _, back, cov = cover_call(pieces, true, false, 0_u8)
      {mask, back, cov}
    end

    # The pieces with every byte inside a hit replaced by fill: {redacted, piece_back, piece_covered}.  Written one behind
    # the other, with the last piece_back[d] bytes already written overwritten by fill, the pieces of a sequence give
    # AC#redact of the whole.
    def redact_batch(pieces : Array({Int32, Bytes | String}), fill : UInt8 = 0x2A_u8) : {Bytes, Array(UInt32), Array(UInt64)}
      _, red, back, cov = cover_call(pieces, false, true, fill)
      {red, back, cov}
    end
  end

  # Several GPUs of one node behind one object: the batch is cut into contiguous, byte-balanced document ranges (one
  # per device), every device matches its range, the hit buffers are exchanged with an all-gatherv (RCCL over xGMI
  # between distinct devices) and come back in document order -- the same hits as AC#match_batch.
  class ACGroup
    def initialize(@group : LibAhaHip::Group)
    end

    def finalize
      LibAhaHip.aha_group_free(@group)
    end

    def self.compile(keys : Array(String) | Array(Bytes), devices : Array(Int32), fold_ascii : Bool = false) : self
      blob, offs = AC.pack_keys(keys)
      rc = LibAhaHip.aha_group_compile(blob.to_slice.to_unsafe, offs.to_unsafe, keys.size.to_u32,
        devices.to_unsafe, devices.size, fold_ascii ? LibAhaHip::OPT_FOLD_ASCII : 0_u32, out group, out bad)
      if rc == AC::E_DUP_KEY
        raise "key:#{keys[bad]} appear twice."
      elsif rc != 0
        raise String.new(LibAhaHip.aha_strerror(rc))
      end
      new(group)
    end

    def match_batch(docs : Array(String) | Array(Bytes), chars : Bool = false) : Array(Array(Hit))
      corpus = IO::Memory.new
      offs = Array(UInt64).new(docs.size + 1)
      offs << 0_u64
      docs.each do |d|
        corpus.write(d.is_a?(String) ? d.to_slice : d)
        offs << corpus.pos.to_u64
      end
      params = AC.params(chars, nil)
      dho = Array(UInt64).new(docs.size + 1, 0_u64)
      cap = (corpus.pos / 4 + 64).to_u64
      result = Array(Array(Hit)).new(docs.size)
      loop do
        out_buf = Pointer(LibAhaHip::Hit).malloc(cap)
        rc = LibAhaHip.aha_group_match_batch(@group, corpus.to_slice.to_unsafe, offs.to_unsafe, docs.size.to_u64,
          pointerof(params), out_buf, cap, dho.to_unsafe, out n)
        if rc == AC::E_CAPACITY
          cap = n
          next
        end
        raise String.new(LibAhaHip.aha_strerror(rc)) if rc != 0
        docs.size.times do |d|
          hits = Array(Hit).new((dho[d + 1] - dho[d]).to_i32)
          (dho[d]...dho[d + 1]).each { |i| hits << Hit.new(out_buf[i].start, out_buf[i].end_, out_buf[i].value) }
          result << hits
        end
        break
      end
      result
    end

    # The batch resident on the devices (aha_group_corpus_upload): every shard's documents on its device, uploaded once.
    class Corpus
      getter handle : LibAhaHip::GroupCorpus
      getter n_docs : Int32

      def initialize(@handle, @n_docs)
      end

      def finalize
        LibAhaHip.aha_group_corpus_free(@handle)
      end
    end

    def upload(docs : Array(String) | Array(Bytes)) : Corpus
      corpus = IO::Memory.new
      offs = Array(UInt64).new(docs.size + 1)
      offs << 0_u64
      docs.each do |d|
        corpus.write(d.is_a?(String) ? d.to_slice : d)
        offs << corpus.pos.to_u64
      end
      rc = LibAhaHip.aha_group_corpus_upload(@group, corpus.to_slice.to_unsafe, offs.to_unsafe, docs.size.to_u64, out c)
      raise String.new(LibAhaHip.aha_strerror(rc)) if rc != 0
      Corpus.new(c, docs.size)
    end

    # Every device matches its resident range, then the all-gatherv; the hits stay on the devices (every device holds the
    # whole ordered stream).  Returns the hit count and the per-document hit offsets; `shard_hits` reads one device's copy.
    def match_resident(c : Corpus, chars : Bool = false) : {UInt64, Array(UInt64)}
      params = AC.params(chars, nil)
      dho = Array(UInt64).new(c.n_docs + 1, 0_u64)
      rc = LibAhaHip.aha_group_match_batch_device(@group, c.handle, pointerof(params), dho.to_unsafe, out n)
      raise String.new(LibAhaHip.aha_strerror(rc)) if rc != 0
      {n, dho}
    end

    def shard_hits(shard : Int32) : Array(Hit)
      LibAhaHip.aha_group_download_shard(@group, shard, Pointer(LibAhaHip::Hit).null, 0_u64, out n)
      buf = Pointer(LibAhaHip::Hit).malloc(n + 1)
      rc = LibAhaHip.aha_group_download_shard(@group, shard, buf, n + 1, out got)
      raise String.new(LibAhaHip.aha_strerror(rc)) if rc != 0
      Array(Hit).new(got.to_i32) { |i| Hit.new(buf[i].start, buf[i].end_, buf[i].value) }
    end
  end
end
