"""GPU tests of the kana fold (AHA_OPT_FOLD_KANA, include/aha_hip.h).  THE RULE: every call on a handle compiled with the flag
gives, bit for bit, what the same call gives on an ordinary handle compiled from foldk(key) of each key over the batch in which
each document is folded on its own.  The yardstick everywhere is that ordinary handle -- and the oracle beside it --, given
tests/foldksim.py's fold of the keys and of the corpus (plain Python from unicodedata; it does not read the committed tables).
The exceptions are the ASCII fold's: redact, replace and grep give the caller's bytes, keys keep their spelling.  Every test runs
under both forms of k_foldk_copy's halo (AHA_FOLDK_HALO=mem|lane, read at every launch)."""
import numpy as np
import pytest
import torch

import coversim
import fold3sim
import foldksim
import foldsim
import replacesim
from aha_amd import AC, BitArray
from engine_variants import VARIANTS, use_variant

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
HALOS = ("mem", "lane")


def u8(b):
    return np.frombuffer(bytes(b), dtype=np.uint8).copy()


def offsets_of(docs):
    return np.concatenate([[0], np.cumsum([len(d) for d in docs])]).astype(np.uint64)


def folded(corpus, doc):
    return u8(foldksim.foldk_docs(corpus, doc))


def as_list(h):
    return [(int(s), int(e), int(v)) for s, e, v in np.asarray(h).tolist()]


def on_device(corpus, align):
    """the corpus as a slice of a larger device tensor whose address is `align` modulo 16; the bytes around the slice would join
    its ends (a kana's lead and first continuation byte in front, continuation bytes behind) if a kernel looked at them"""
    n = corpus.size
    big = torch.full((n + 64,), 0x82, dtype=torch.uint8, device=DEV)
    shift = (align - big.data_ptr()) % 16 + 16
    big[:shift] = 0x81
    big[shift - 2] = 0xE3
    dc = big[shift:shift + n]
    dc.copy_(torch.from_numpy(corpus))
    assert dc.data_ptr() % 16 == align
    return dc


def dev_match(m, dc, doc, cap, **kw):
    dd = torch.from_numpy(np.asarray(doc).astype(np.int64)).to(DEV)
    out = torch.zeros((cap + 8, 3), dtype=torch.int32, device=DEV)
    dho = torch.zeros(dd.numel(), dtype=torch.int64, device=DEV)
    n = m.match_batch_device(dc, dd, out, dho, **kw)
    return out[:n].cpu().numpy(), dho.cpu().numpy().astype(np.uint64)


def same_match(f, p, corpus, doc, aligns=(0,), fold=folded, **kw):
    """f over the corpus == p over the per-document fold, hits and per-document offsets, at every alignment; -> p's hits"""
    want_h, want_d = p.match_batch(fold(corpus, doc), doc, **kw)
    want = np.asarray(want_h).view(np.int32).reshape(-1, 3)
    for a in aligns:
        dc = on_device(corpus, a)
        before = dc.clone()
        got, gd = dev_match(f, dc, doc, len(want), **kw)
        assert got.tobytes() == want.tobytes(), (a, kw, len(got), len(want))
        assert np.array_equal(gd, np.asarray(want_d, dtype=np.uint64))
        assert torch.equal(dc, before)  # the caller's corpus is only read
    return want_h


def oracle_hits(keys, text, doc):
    import pyoracle as orc  # checker only

    hits, _ = orc.AC.compile(keys).match_batch(text, doc)
    return sorted(as_list(hits))


def oracle_counts(keys, text, doc):
    return np.bincount([v for _, _, v in oracle_hits(keys, text, doc)], minlength=len(keys)).tolist()


# A handle that reads bytes: one key per byte value (NUL is no key; upper-case letters equal their lower case after folding).
# Every byte of the folded text is one hit whose value names it, so a match compares the staged copy byte for byte.
BYTE_KEYS = [bytes([b]) for b in range(1, 256) if not 0x41 <= b <= 0x5A]
_READERS = []


def byte_readers():
    if not _READERS:
        _READERS.append((AC.compile(BYTE_KEYS, fold_kana=True), AC.compile(BYTE_KEYS)))
    return _READERS[0]


def one_doc(c):
    return np.array([0, c.size], dtype=np.uint64)


# ---- every moved character at every phase --------------------------------------------------------------------------------------
_PHASES = []


def phases_case():
    """each of the 144 characters K moves, and kana it does not move, once at every phase 0 .. 15 of a 16-byte piece"""
    if _PHASES:
        return _PHASES[0]
    chars = [foldksim.enc3(cp) for cp in sorted(foldksim.K())]
    assert len(chars) == 144
    chars += [c.encode() for c in "アヷゟﾞ漢Ａ"]  # katakana itself, kana that stay, a mark, a kanji, a full-width letter (F3's)
    assert len(set(chars)) == len(chars)
    first = {}
    for c in chars:  # one key per class, spelled as its first member: the ordinary handle has the folded spellings in the same order
        first.setdefault(foldksim.foldk(c), c)
    spelled = [first[r] for r in sorted(first)]
    assert sum(foldksim.foldk(k) != k for k in spelled) > 80
    pad = b"aZbYcXdWeVfUgThSi"
    parts, at, met = [], 0, set()
    for phase in range(16):
        for k, c in enumerate(chars):
            g = (phase - at) % 16
            if g == 0 and k % 5 == 0:
                g = 16
            parts.append(pad[:g] + c)
            at += g + 3
            met.add((k, (at - 3) % 16))
    assert len(met) == len(chars) * 16
    base = b"".join(parts) + b"q" * (-at % 16)
    assert len(base) % 16 == 0
    A = "あ".encode()
    # n % 16 = 0; 1 and 2: the tail is the continuation byte(s) of a triple whose lead is in the last piece; 15
    texts = [base, base + b"Q" * 14 + A, base + b"Q" * 15 + A, base + "ぴｭゞｱあ".encode()]
    assert [len(t) % 16 for t in texts] == [0, 1, 2, 15]
    _PHASES.append((chars, spelled, texts))
    return _PHASES[0]


@pytest.mark.parametrize("halo", HALOS)
def test_every_moved_character_at_every_phase_matched_and_redacted(halo, monkeypatch):
    monkeypatch.setenv("AHA_FOLDK_HALO", halo)
    chars, spelled, texts = phases_case()
    f = AC.compile(spelled, fold_kana=True)
    p = AC.compile(foldksim.foldk_keys(spelled))
    for t in texts:
        corpus = u8(t)
        doc = one_doc(corpus)
        fc = folded(corpus, doc)
        assert fc.tobytes() != fold3sim.fold3(t)
        want = same_match(f, p, corpus, doc, aligns=(0, 1, 15))
        assert len(want) >= len(chars) * 16  # every character was found under its class's key
        # redacted: the mask of the folded match, the caller's bytes outside it
        mask, dcov = p.cover_batch(fc, doc)
        red, dcov2 = f.redact_batch(corpus, doc)
        assert np.array_equal(red, coversim.redacted(corpus, coversim.unpack(mask, corpus.size), 0x2A)) and np.array_equal(dcov2, dcov)
    c0 = u8(texts[0])  # the yardstick against the oracle, once
    assert sorted(as_list(p.match_batch(folded(c0, one_doc(c0)), one_doc(c0))[0])) == oracle_hits(foldksim.foldk_keys(spelled), folded(c0, one_doc(c0)), one_doc(c0))
    # ... and the same bytes read one by one
    fb, pb = byte_readers()
    for t in texts[1:3]:
        corpus = u8(t)
        want = same_match(fb, pb, corpus, one_doc(corpus), aligns=(0, 5, 15))
        assert len(want) == corpus.size


# ---- boundaries the kernel can get wrong ---------------------------------------------------------------------------------------
def fold_grid(n_bytes, max_blocks):
    """the staged copy's grid (scan_fold.hip): a workgroup of 256 lanes per 1024 pieces, max_blocks at the most"""
    return max(1, min((n_bytes // 16 + 1023) // 1024, max_blocks))


MOVERS = [c.encode() for c in "あｱぴｭゞｶがﾝ"]  # hiragana and half-width katakana: every one moves


def triples_cut_on(n, edges, cuts):
    """n bytes of MOVERS such that edge e (a byte offset) lies inside a triple, cuts[i] bytes of it in front of edges[i]; a few
    ASCII bytes behind the previous edge set the phase"""
    assert all(c in (1, 2) for c in cuts)
    out, k = bytearray(), 0
    for e, c in zip(list(edges) + [None], list(cuts) + [None]):
        if e is not None:
            out += b"x" * ((e - c - len(out)) % 3)
        while len(out) < (n if e is None else e):
            out += MOVERS[k % len(MOVERS)]
            k += 1
    t = bytes(out[:n])
    for e, c in zip(edges, cuts):
        assert foldksim.is_lead3(t[e - c]) and all(foldksim.is_cont(x) for x in t[e - c + 1:e - c + 3]), (e, c)
    return t


@pytest.mark.parametrize("halo", HALOS)
def test_wave_edges_grid_strides_partial_waves_and_short_buffers(halo, monkeypatch):
    monkeypatch.setenv("AHA_FOLDK_HALO", halo)
    fb, pb = byte_readers()
    # 3 KiB + 5 on one workgroup: a triple across each 1 KiB wave edge, cut 1|2 (bytes 1023 .. 1025), 2|1 (1022 .. 1024), 1|2
    n = 3 * 1024 + 5
    corpus = u8(triples_cut_on(n, (1024, 2048, 3072), (1, 2, 1)))
    assert fold_grid(n, 512) == 1 and n // 16 <= 256
    assert folded(corpus, one_doc(corpus)).tobytes() not in (corpus.tobytes(), fold3sim.fold3(corpus.tobytes()))
    same_match(fb, pb, corpus, one_doc(corpus), aligns=(0, 1, 15))
    corpus = u8(triples_cut_on(n, (1024, 2048, 3072), (2, 1, 2)))
    same_match(fb, pb, corpus, one_doc(corpus), aligns=(0, 5))  # (5: a source view 5 bytes into a buffer)
    # 1800 pieces on 2 workgroups (a workgroup per 1024 pieces: the grid is capped at 2), stride 512: lanes take up to four
    # pieces, both the unrolled loop and the remainder loop run -- in the lane form waves 0 .. 3 take the unrolled step and the
    # wave at piece 1792 is left with 8 lanes --, and a triple lies across every stride edge, in both cut positions
    n = 1800 * 16 + 5
    g = fold_grid(n, 512)
    assert g == 2 and n // 16 > g * 256 and 3 * g * 256 < n // 16
    corpus = u8(triples_cut_on(n, (512 * 16, 1024 * 16, 1536 * 16, 1792 * 16), (2, 1, 2, 1)))
    same_match(fb, pb, corpus, one_doc(corpus), aligns=(0, 15))
    # a last wave that is partial: 64 + 37 pieces and a tail of 5; the last piece ends inside a triple
    n = 16 * (64 + 37) + 5
    corpus = u8(triples_cut_on(n, (1024, 16 * (64 + 37)), (1, 2)))
    same_match(fb, pb, corpus, one_doc(corpus), aligns=(0, 1, 15))
    corpus = u8(triples_cut_on(n, (1024, 16 * (64 + 37)), (2, 1)))
    same_match(fb, pb, corpus, one_doc(corpus), aligns=(0, 5))
    # a buffer that ends with a lead byte, with a lead and one continuation byte, continuation bytes only, lead bytes only
    for t in (b"Hello \xe3", "あｱ".encode() + b"\xe3", b"Hello W\xe3\x81", "あｱぴｭゞ".encode() + b"\xef\xbd", b"\x82", b"\x81\x82",
              b"\x81" * 40, b"\xe3" * 33):
        corpus = u8(t)
        want = same_match(fb, pb, corpus, one_doc(corpus), aligns=(0, 1, 15))
        assert len(want) == corpus.size
    src = "ぴｭ".encode() * 5
    for n in (0, 1, 2, 15, 16, 17):
        for lead_in in (0, 1, 2):  # (cut in front of a lead byte, of a first continuation byte and of a second)
            corpus = u8(src[lead_in:lead_in + n])
            if n == 0:
                h, d = fb.match_batch(corpus, one_doc(corpus))
                assert len(h) == 0 and list(d) == [0, 0]
                continue
            same_match(fb, pb, corpus, one_doc(corpus), aligns=(0, 5, 15))


# ---- documents -----------------------------------------------------------------------------------------------------------------
DOC_KEYS = [b"a\xe3", b"\x81\x82b", b"\x82", "ア".encode(), b"c\xd0", "Р".encode(), b"\xe3", b"\xb1y", b"x\xef\xbd"]
DOCS = [b"a\xe3", b"\x81\x82b",               # "あ" cut 1|2
        b"",
        b"x\xef\xbd", b"\xb1y",               # "ｱ" cut 2|1
        b"\xe3", b"", b"\x81", b"\x82",       # "あ" cut 1|1|1, an empty document between the cuts
        b"c\xd0", b"\xa0b",                   # a pair cut
        "あアｱРр".encode()]


def sep_not_82():
    """every byte a separator but 0x82, the second byte the folded hiragana get (0x81 is the original of most)"""
    sep = BitArray(256)
    for c in range(256):
        sep[c] = c != 0x82
    return sep


def check_documents(f, p):
    corpus, doc = u8(b"".join(DOCS)), offsets_of(DOCS)
    fc = folded(corpus, doc)
    fkeys = foldksim.foldk_keys(DOC_KEYS)
    assert fc.tobytes() != foldksim.foldk(corpus.tobytes())  # the buffer folded whole joins doc 0's end with doc 1's start
    assert fc.tobytes()[:int(doc[11])] == corpus.tobytes()[:int(doc[11])]  # nothing folds in the cut documents
    # the oracle: the keys made of the cut characters' fragments hit, which they would not had the pass folded across the cuts
    counts = oracle_counts(fkeys, fc, doc)
    blind = oracle_counts(fkeys, u8(foldksim.foldk(corpus.tobytes())), doc)
    assert counts[0] == 1 and counts[1] == 1 and counts[7] == 1 and counts[8] == 1 and counts[3] == 3 and counts != blind
    want = same_match(f, p, corpus, doc, aligns=(0, 1, 15))
    assert sorted(as_list(want)) == oracle_hits(fkeys, fc, doc)
    sep = sep_not_82()
    want_s = same_match(f, p, corpus, doc, aligns=(0, 1, 15), sep=sep)
    assert 0 < len(want_s) < len(want)
    # every family that has its own way into the text, against the yardstick
    kc, cd = f.count_batch(corpus, doc)
    wkc, wcd = p.count_batch(fc, doc)
    assert np.array_equal(kc, wkc) and np.array_equal(cd, wcd) and list(kc) == counts
    kc, cd = f.count_batch(corpus, doc, sep=sep)
    wkc, wcd = p.count_batch(fc, doc, sep=sep)
    assert np.array_equal(kc, wkc) and np.array_equal(cd, wcd)
    a, b = f.doc_counts_batch(corpus, doc), p.doc_counts_batch(fc, doc)
    assert a[0].tobytes() == b[0].tobytes() and np.array_equal(a[1], b[1])
    classes = [0, 1, (0, 2), 1, 2, (0, 1), 2, 0, 1]
    assert np.array_equal(f.class_counts_batch(corpus, doc, classes), p.class_counts_batch(fc, doc, classes))
    a, b = f.select_batch(corpus, doc), p.select_batch(fc, doc)
    assert a[0].tobytes() == b[0].tobytes() and np.array_equal(a[1], b[1]) and len(a[0]) > 8
    a, b = f.cover_batch(corpus, doc), p.cover_batch(fc, doc)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    kept, _, _ = f.grep_batch(corpus, doc)
    wd = p.match_batch(fc, doc)[1]
    assert list(kept) == list(p.grep_batch(fc, doc)[0]) == [d for d in range(len(DOCS)) if wd[d + 1] > wd[d]] == [0, 1, 3, 4, 5, 8, 9, 11]
    for chars in (False, True):
        for longest in (1, 2):
            a, b = f.match_batch(corpus, doc, chars=chars, longest=longest), p.match_batch(fc, doc, chars=chars, longest=longest)
            assert np.asarray(a[0]).tobytes() == np.asarray(b[0]).tobytes() and np.array_equal(a[1], b[1])


@pytest.mark.parametrize("halo", HALOS)
def test_documents_are_folded_on_their_own(halo, monkeypatch):
    monkeypatch.setenv("AHA_FOLDK_HALO", halo)
    f = AC.compile(DOC_KEYS, fold_kana=True)
    p = AC.compile(foldksim.foldk_keys(DOC_KEYS))
    assert f.fold_kana and f[3] == "ア" and f[5] == "Р"  # (the caller's spelling)
    check_documents(f, p)


@pytest.mark.parametrize("halo", HALOS)
def test_documents_through_the_ranges_paths(halo, monkeypatch):
    """the same batch with the bounds of a range's hit bytes at their minimum (12 bytes, one hit: AHA_CLASS_HIT_BYTES and its
    siblings of DESIGN.md section 7, read when a handle is compiled): class counts, document counts and select (with it replace
    and grep) each split the batch into ranges of whole documents, every range folded on its own with its rebased offsets --
    ranges start with the continuation bytes of a cut character"""
    monkeypatch.setenv("AHA_FOLDK_HALO", halo)
    for name in ("AHA_CLASS_HIT_BYTES", "AHA_DOCCOUNT_HIT_BYTES", "AHA_SELECT_HIT_BYTES"):
        monkeypatch.setenv(name, "12")
    f = AC.compile(DOC_KEYS, fold_kana=True)
    p = AC.compile(foldksim.foldk_keys(DOC_KEYS))
    check_documents(f, p)


# ---- every family, small ---------------------------------------------------------------------------------------------------
WORDS = ("コンピュータ こんぴゅーた ｺﾝﾋﾟｭｰﾀ ひらがな ヒラガナ ﾋﾗｶﾞﾅ カタカナ かたかな ｶﾀｶﾅ らーめん ラーメン ﾗｰﾒﾝ すし スシ ｽｼ とうきょう トウキョウ "
         "東京タワー 東京たわー 日本語 にほんご ニホンゴ 漢字かな交じり文 カンジ ゝゞ ヽヾ ｶﾞ ガ が ぁあ ァア "
         "ＥＲＲＯＲ ｅｒｒｏｒ Ｗａｒｎｉｎｇ Việt VIỆT Привет МИР мир école ÉCOLE error ERROR Warning the THE 你好 世界").split()


def family_case():
    rng = np.random.default_rng(11)
    docs = []
    for d in range(24):
        if d in (3, 8, 17):
            docs.append(b"")
            continue
        parts, size = [], 0
        while size < 2000:
            w = WORDS[rng.integers(len(WORDS))]
            r = rng.random()
            w = w.upper() if r < 0.2 else w.lower() if r < 0.4 else w
            sep = "" if rng.random() < 0.3 else " " if rng.random() < 0.8 else "\n"  # (Japanese text runs words together)
            b = (w + sep).encode()
            if rng.random() < 0.05:  # random bytes: broken sequences, stray lead and continuation bytes
                b = bytes(rng.integers(0, 256, size=len(b), dtype=np.uint8))
            parts.append(b)
            size += len(b)
        t = b"".join(parts)
        docs.append(t[:len(t) - (d % 4)])  # (some documents end inside a word, perhaps inside a character)
    keys, seen = [], set()
    pool = [w for w in WORDS] + [w[:2] for w in WORDS if len(w) > 3] + [w[-2:] for w in WORDS if len(w) > 4] + ["ｰ", "ん", "ヲ", "Я", "ｒ"]
    for w in pool:
        k = w.encode()
        if foldksim.foldk(k) not in seen and len(keys) < 50:
            seen.add(foldksim.foldk(k))
            keys.append(k)
    assert len(keys) == 50 and sum(foldksim.foldk(k) != fold3sim.fold3(k) for k in keys) > 10
    corpus, doc = u8(b"".join(docs)), offsets_of(docs)
    return keys, corpus, doc, folded(corpus, doc)


_FAMILY = []


def family():
    if not _FAMILY:
        _FAMILY.append(family_case())
    return _FAMILY[0]


@pytest.mark.parametrize("variant", VARIANTS)
def test_every_family_on_every_engine_variant(variant, monkeypatch):
    use_variant(variant, monkeypatch)
    keys, corpus, doc, fc = family()
    assert 30_000 < corpus.size < 60_000 and len(doc) - 1 == 24
    # the inputs do exercise the kana fold
    assert fc.tobytes() != fold3sim.fold3_docs(corpus, doc) and fc.tobytes() != corpus.tobytes()
    f = AC.compile(keys, fold_kana=True)
    p = AC.compile(foldksim.foldk_keys(keys))
    assert f.info == p.info  # the engine choice is the one the folded key set gets
    N_ = corpus.size

    def same(a, b):
        assert len(a) == len(b)
        for x, y in zip(a, b):
            assert np.asarray(x).tobytes() == np.asarray(y).tobytes()

    # the yardstick's own results, once: they do not depend on the halo form
    want_chars = p.match_batch(fc, doc, chars=True)
    want_longest = [p.match_batch(fc, doc, longest=longest) for longest in (1, 2)]
    want_sep = None
    sep = BitArray(256)
    for c in b" \n":
        sep[c] = True
    want_count, want_dc = p.count_batch(fc, doc), p.doc_counts_batch(fc, doc)
    classes = [(k % 5,) if k % 7 else (0, 4) for k in range(len(keys))]
    want_cc = p.class_counts_batch(fc, doc, classes)
    mask, dcov = p.cover_batch(fc, doc)
    want_red = coversim.redacted(corpus, coversim.unpack(mask, N_), 0x2A)
    assert not np.array_equal(want_red, coversim.redacted(fc, coversim.unpack(mask, N_), 0x2A))
    sel, dso = p.select_batch(fc, doc)
    repl = {k: ("<%d>" % k).encode() for k in range(0, len(keys), 2)}
    want_out, want_doo = replacesim.replace(corpus, doc, as_list(sel), dso, repl)
    assert not np.array_equal(want_out, replacesim.replace(fc, doc, as_list(sel), dso, repl)[0])
    want_rec = p.records(corpus, doc)
    want_grep = [p.grep_batch(fc, doc, invert=invert) for invert in (False, True)]
    want_lines = p.grep_batch(fc, want_rec[0], text=False)[::2]
    n_bmp = len(AC.compile(keys, fold_bmp=True).match_batch(corpus, doc)[0])
    for halo in HALOS:
        monkeypatch.setenv("AHA_FOLDK_HALO", halo)
        # match with byte offsets and with char offsets, the separator filter, match_longest in both modes; an unaligned
        # corpus goes through once
        want = same_match(f, p, corpus, doc, aligns=(0, 5))
        assert len(want) > 2000 and n_bmp < len(want)  # (strictly more than the three-byte case fold finds)
        want_sep = same_match(f, p, corpus, doc, sep=sep)
        assert 0 < len(want_sep) < len(want)
        same(f.match_batch(corpus, doc, chars=True), want_chars)
        for k, longest in enumerate((1, 2)):
            same(f.match_batch(corpus, doc, longest=longest), want_longest[k])
        # count, doc counts and class counts
        same(f.count_batch(corpus, doc), want_count)
        same(f.doc_counts_batch(corpus, doc), want_dc)
        same([f.class_counts_batch(corpus, doc, classes)], [want_cc])
        # cover and redact: the mask of the folded match, the ORIGINAL bytes outside it
        same(f.cover_batch(corpus, doc), (mask, dcov))
        red, dcov2 = f.redact_batch(corpus, doc)
        assert np.array_equal(red, want_red) and np.array_equal(dcov2, dcov)
        # select and replace: the selection of the folded match, the caller's spelling outside the replaced hits
        same(f.select_batch(corpus, doc), (sel, dso))
        out, doo = f.replace_batch(corpus, doc, repl)
        assert np.array_equal(out, want_out) and np.array_equal(doo, want_doo)
        # records (no key takes part: the caller's bytes are split) and grep: the kept documents with the caller's spelling
        same(f.records(corpus, doc), want_rec)
        for k, invert in enumerate((False, True)):
            kept, _, wdoo = want_grep[k]
            gk, gout, gdoo = f.grep_batch(corpus, doc, invert=invert)
            assert np.array_equal(gk, kept) and np.array_equal(gdoo, wdoo)
            assert gout.tobytes() == b"".join(corpus[int(doc[d]):int(doc[d + 1])].tobytes() for d in kept)
        same(f.grep_batch(corpus, want_rec[0], text=False)[::2], want_lines)  # (lines, as grep takes them)
    if variant == "auto":  # the yardstick against the oracle, once
        assert sorted(as_list(p.match_batch(fc, doc)[0])) == oracle_hits(foldksim.foldk_keys(keys), fc, doc)


# ---- nothing else moved ----------------------------------------------------------------------------------------------------
def fold8_np(a):
    a = np.asarray(a, dtype=np.uint8)
    return np.where((a >= 65) & (a <= 90), a + 32, a).astype(np.uint8)


@pytest.mark.parametrize("halo", HALOS)
def test_plain_ascii_simple_and_bmp_handles_are_what_they_were(halo, monkeypatch):
    monkeypatch.setenv("AHA_FOLDK_HALO", halo)  # (it must not matter to them)
    keys, corpus, doc, fc = family()
    texts = [(corpus, doc)]
    t = u8(triples_cut_on(3 * 1024 + 5, (1024, 2048, 3072), (1, 2, 1)) + "Привет HELLO ＡＢＣ".encode())
    texts.append((t, np.array([0, 1024, 1024, t.size], dtype=np.uint64)))
    modes = [({}, lambda c, d: np.asarray(c), lambda k: k),
             ({"fold_ascii": True}, lambda c, d: fold8_np(c), lambda k: fold8_np(u8(k)).tobytes()),
             ({"fold_simple": True}, lambda c, d: u8(foldsim.fold2_docs(c, d)), foldsim.fold2),
             ({"fold_bmp": True}, lambda c, d: u8(fold3sim.fold3_docs(c, d)), fold3sim.fold3)]
    found = []
    for kw, fold_text, fold_key in modes:
        own, seen = [], set()
        for k in keys:
            if fold_key(k) not in seen:
                seen.add(fold_key(k))
                own.append(k)
        m = AC.compile(own, **kw)
        p = AC.compile([fold_key(k) for k in own])
        assert not m.fold_kana
        n = 0
        for c, d in texts:
            n += len(same_match(m, p, c, d, aligns=(0, 1, 15), fold=fold_text))
        found.append(n)
    fk = AC.compile(keys, fold_kana=True)
    nk = sum(len(fk.match_batch(c, d)[0]) for c, d in texts)
    assert 0 < found[0] < found[1] < found[2] < found[3] < nk  # each fold finds strictly more than the one before it
