"""GPU tests of case folding for three-byte UTF-8 characters (AHA_OPT_FOLD_BMP, include/aha_hip.h).  THE RULE: every call on a
handle compiled with the flag gives, bit for bit, what the same call gives on an ordinary handle compiled from fold3(key) of
each key over the batch in which each document is folded on its own.  The yardstick everywhere is that ordinary handle, given
tests/fold3sim.py's fold of the keys and of the corpus (plain Python from str.upper / str.lower; it does not read the committed
tables).  The exceptions are the ASCII fold's: redact, replace and grep give the caller's bytes, keys keep their spelling."""
import numpy as np
import pytest
import torch

import coversim
import fold3sim
import foldsim
import replacesim
from aha_amd import AC, BitArray
from engine_variants import VARIANTS, use_variant

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def u8(b):
    return np.frombuffer(bytes(b), dtype=np.uint8).copy()


def offsets_of(docs):
    return np.concatenate([[0], np.cumsum([len(d) for d in docs])]).astype(np.uint64)


def folded(corpus, doc):
    return u8(fold3sim.fold3_docs(corpus, doc))


def as_list(h):
    return [(int(s), int(e), int(v)) for s, e, v in np.asarray(h).tolist()]


def on_device(corpus, align):
    """the corpus as a slice of a larger device tensor whose address is `align` modulo 16; the bytes around the slice would join
    its ends (a triple's lead and first continuation byte in front, continuation bytes behind) if a kernel looked at them"""
    n = corpus.size
    big = torch.full((n + 64,), 0xA1, dtype=torch.uint8, device=DEV)
    shift = (align - big.data_ptr()) % 16 + 16
    big[:shift] = 0xBC
    big[shift - 2] = 0xEF
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


# A handle that reads bytes: one key per byte value (NUL is no key; upper-case letters equal their lower case after folding).
# Every byte of the folded text is one hit whose value names it, so a match compares the staged copy byte for byte.
BYTE_KEYS = [bytes([b]) for b in range(1, 256) if not 0x41 <= b <= 0x5A]
_READERS = []


def byte_readers():
    if not _READERS:
        _READERS.append((AC.compile(BYTE_KEYS, fold_bmp=True), AC.compile(BYTE_KEYS)))
    return _READERS[0]


# ---- every live character at every phase -------------------------------------------------------------------------------------
def test_every_live_character_at_every_phase_of_a_piece():
    blocks = fold3sim.live_blocks()
    assert len(blocks) == 29
    chars = [fold3sim.enc3(cp) for b in blocks for cp in range(b << 6, (b << 6) + 64)]
    chars += ["你".encode(), fold3sim.enc3(0x800), fold3sim.enc3(0xFFFF), b"\xe0\x80\x80", b"\xed\xa0\x80"]  # .. an overlong form, a surrogate
    assert len(chars) == 29 * 64 + 5 and len(set(chars)) == len(chars)
    # one key per case class, spelled as its first member (the folded spelling is another one for most): the ordinary handle
    # has the folded spellings in the same order, so ids map one to one
    first = {}
    for c in chars:
        first.setdefault(fold3sim.fold3(c), c)
    spelled = [first[r] for r in sorted(first)]
    assert len(spelled) == len({fold3sim.fold3(k) for k in spelled}) and sum(fold3sim.fold3(k) != k for k in spelled) > 300
    f = AC.compile(spelled, fold_bmp=True)
    p = AC.compile(fold3sim.fold3_keys(spelled))
    # the text: for every phase 0 .. 15 each character once, with 0 .. 16 ASCII bytes (both cases) in front so that it starts
    # at that phase of a 16-byte piece -- phases 14 and 15 are the straddles 14|15.0 and 15|0.1
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
    A = "Ａ".encode()
    # n % 16 = 0; 1 and 2: the tail is the continuation byte(s) of a triple whose lead is in the last piece; 15
    texts = [base, base + b"Q" * 14 + A, base + b"Q" * 15 + A, base + "ẤＢỆＣỘ".encode()]
    assert [len(t) % 16 for t in texts] == [0, 1, 2, 15]
    for t in texts:
        corpus = u8(t)
        doc = np.array([0, corpus.size], dtype=np.uint64)
        assert folded(corpus, doc).tobytes() != foldsim.fold2(t)
        want = same_match(f, p, corpus, doc, aligns=(0, 1, 15))
        assert len(want) >= len(chars) * 16  # every character was found under its class's key
    # ... and the same bytes read one by one
    fb, pb = byte_readers()
    for t in texts[1:3]:
        corpus = u8(t)
        want = same_match(fb, pb, corpus, np.array([0, corpus.size], dtype=np.uint64), aligns=(0, 1, 15))
        assert len(want) == corpus.size


# ---- boundaries the kernel can get wrong ---------------------------------------------------------------------------------------
def fold_grid(n_bytes, max_blocks):
    """the staged copy's grid (scan_fold.hip): a workgroup of 256 lanes per 1024 pieces, max_blocks at the most"""
    return max(1, min((n_bytes // 16 + 1023) // 1024, max_blocks))


UPPER = [c.encode() for c in "ＡẤＢỆＣỘＤỪＥỴ"]  # upper-case full-width and Vietnamese letters: every one moves


def triples_cut_on(n, edges, cuts):
    """n bytes of UPPER such that edge e (a byte offset) lies inside a triple, cuts[i] bytes of it in front of edges[i]; a few
    ASCII bytes behind the previous edge set the phase"""
    assert all(c in (1, 2) for c in cuts)
    out, k = bytearray(), 0
    for e, c in zip(list(edges) + [None], list(cuts) + [None]):
        if e is not None:
            out += b"x" * ((e - c - len(out)) % 3)
        while len(out) < (n if e is None else e):
            out += UPPER[k % len(UPPER)]
            k += 1
    t = bytes(out[:n])
    for e, c in zip(edges, cuts):
        assert fold3sim.is_lead3(t[e - c]) and all(fold3sim.is_cont(x) for x in t[e - c + 1:e - c + 3]), (e, c)
    return t


@pytest.mark.parametrize("reserve", [None, "1"])
def test_wave_edges_grid_strides_and_short_buffers(reserve, monkeypatch):
    if reserve:
        monkeypatch.setenv("AHA_RESERVE_CUS", reserve)
    fb, pb = byte_readers() if not reserve else (AC.compile(BYTE_KEYS, fold_bmp=True), AC.compile(BYTE_KEYS))
    one_doc = lambda c: np.array([0, c.size], dtype=np.uint64)
    # 3 KiB + 5: a triple across each 1 KiB wave edge, cut 1|2, 2|1 and 1|2; one workgroup, every lane at most one piece -- no
    # stride, with or without a reserved CU (the grid is ceil(pieces / 1024) workgroups for any cap of 512 or more, and the cap
    # is 8 * max(grid, 64))
    n = 3 * 1024 + 5
    corpus = u8(triples_cut_on(n, (1024, 2048, 3072), (1, 2, 1)))
    assert n // 16 <= fold_grid(n, 512) * 256
    assert folded(corpus, one_doc(corpus)).tobytes() not in (corpus.tobytes(), foldsim.fold2(corpus.tobytes()))
    same_match(fb, pb, corpus, one_doc(corpus), aligns=(0, 1, 15))
    # 1800 pieces on 2 workgroups, stride 512: lanes take up to four pieces, both the unrolled loop (i + 3 * 512 < 1800) and the
    # remainder loop run, and a triple lies across every stride edge, in both cut positions
    n = 1800 * 16 + 5
    g = fold_grid(n, 512)
    assert g == 2 and n // 16 > g * 256 and 3 * g * 256 < n // 16
    corpus = u8(triples_cut_on(n, (512 * 16, 1024 * 16, 1536 * 16), (2, 1, 2)))
    same_match(fb, pb, corpus, one_doc(corpus), aligns=(0, 15))
    # a buffer that ends with a lead byte, with a lead and one continuation byte, continuation bytes only, lead bytes only
    for t in (b"Hello \xe1", "ẤＢ".encode() + b"\xe1", b"Hello W\xe1\xba", "ẤＢỆＣỘ".encode() + b"\xe1\xba", b"\xa1", b"\xbc\xa1",
              b"\xa0" * 40, b"\xef" * 33):
        corpus = u8(t)
        want = same_match(fb, pb, corpus, one_doc(corpus), aligns=(0, 1, 15))
        assert len(want) == corpus.size
    src = "ＺỆ".encode() * 5
    for n in (0, 1, 2, 3, 15, 16, 17, 18):
        for lead_in in (0, 1, 2):  # (cut in front of a lead byte, of a first continuation byte and of a second)
            corpus = u8(src[lead_in:lead_in + n])
            if n == 0:
                h, d = fb.match_batch(corpus, one_doc(corpus))
                assert len(h) == 0 and list(d) == [0, 0]
                continue
            same_match(fb, pb, corpus, one_doc(corpus), aligns=(0, 1, 15))


# ---- documents -----------------------------------------------------------------------------------------------------------------
DOC_KEYS = [b"a\xef", b"\xbc\xa1b", b"\xa1", "ａ".encode(), b"c\xd0", "Р".encode(), b"\xef"]
DOCS = [b"a\xef", b"\xbc\xa1b",               # "Ａ" cut 1|2
        b"",
        b"x\xef\xbc", b"\xa1y",               # cut 2|1
        b"\xef", b"", b"\xbc", b"\xa1",       # cut 1|1|1, an empty document between the cuts
        b"c\xd0", b"\xa0b",                   # a pair cut
        "ＡａРр".encode()]
# hits per key over the batch folded document by document: by hand, and checked against the oracle in the test (the "\xa1"
# inside document 1's "\xbc\xa1b" is no hit of its own in the reference's semantics, as the oracle states them)
DOC_KEY_COUNTS = [1, 1, 2, 2, 1, 2, 5]


def oracle_counts(keys, text, doc):
    import pyoracle as orc  # checker only

    hits, _ = orc.AC.compile(keys).match_batch(text, doc)
    return np.bincount([int(r[2]) for r in np.asarray(hits).tolist()], minlength=len(keys)).tolist()


def sep_not_bd():
    """every byte a separator but 0xBD, the folded second byte of the full-width letters (0xBC is the original)"""
    sep = BitArray(256)
    for c in range(256):
        sep[c] = c != 0xBD
    return sep


def check_documents(f, p):
    corpus, doc = u8(b"".join(DOCS)), offsets_of(DOCS)
    fc = folded(corpus, doc)
    assert fc.tobytes() != fold3sim.fold3(corpus.tobytes())  # the buffer folded whole joins doc 0's end with doc 1's start
    assert fc.tobytes()[:int(doc[11])] == corpus.tobytes()[:int(doc[11])]  # nothing folds in the cut documents
    assert oracle_counts(fold3sim.fold3_keys(DOC_KEYS), fc, doc) == DOC_KEY_COUNTS
    want = same_match(f, p, corpus, doc, aligns=(0, 1, 15))
    got = as_list(want)
    wd = p.match_batch(fc, doc)[1]
    assert sorted(got[int(wd[0]):int(wd[1])]) == [(0, 2, 0), (1, 2, 6)]  # without the fix-up: neither of these ..
    assert got[int(wd[1]):int(wd[2])] == [(0, 3, 1)]                     # .. nor this one
    assert got[int(wd[4]):int(wd[5])] == [(0, 1, 2)] and got[int(wd[8]):int(wd[9])] == [(0, 1, 2)]
    assert got[int(wd[9]):int(wd[10])] == [(0, 2, 4)] and got[int(wd[10]):int(wd[11])] == []
    # a separator filter whose bit for 0xBD is clear: the "\xef" of document 3 ("x\xef\xbc") is followed by the original 0xBC
    # and stays; folded across the boundary it would be followed by 0xBD, as the two in the last document are
    sep = sep_not_bd()
    want_s = same_match(f, p, corpus, doc, aligns=(0, 1, 15), sep=sep)
    assert 0 < len(want_s) < len(want)
    ws = p.match_batch(fc, doc, sep=sep)[1]
    assert as_list(want_s)[int(ws[3]):int(ws[4])] == [(1, 2, 6)] and all(v != 6 for _, _, v in as_list(want_s)[int(ws[11]):int(ws[12])])
    # every family that has its own way into the text, against the yardstick
    kc, cd = f.count_batch(corpus, doc)
    wkc, wcd = p.count_batch(fc, doc)
    assert np.array_equal(kc, wkc) and np.array_equal(cd, wcd) and list(kc) == DOC_KEY_COUNTS
    kc, cd = f.count_batch(corpus, doc, sep=sep)
    wkc, wcd = p.count_batch(fc, doc, sep=sep)
    assert np.array_equal(kc, wkc) and np.array_equal(cd, wcd)
    a, b = f.doc_counts_batch(corpus, doc), p.doc_counts_batch(fc, doc)
    assert a[0].tobytes() == b[0].tobytes() and np.array_equal(a[1], b[1])
    classes = [0, 1, (0, 2), 1, 2, (0, 1), 2]
    assert np.array_equal(f.class_counts_batch(corpus, doc, classes), p.class_counts_batch(fc, doc, classes))
    a, b = f.select_batch(corpus, doc), p.select_batch(fc, doc)
    assert a[0].tobytes() == b[0].tobytes() and np.array_equal(a[1], b[1]) and len(a[0]) > 8
    a, b = f.cover_batch(corpus, doc), p.cover_batch(fc, doc)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    kept, _, _ = f.grep_batch(corpus, doc)
    assert list(kept) == [0, 1, 3, 4, 5, 8, 9, 11]
    for chars in (False, True):
        for longest in (1, 2):
            a, b = f.match_batch(corpus, doc, chars=chars, longest=longest), p.match_batch(fc, doc, chars=chars, longest=longest)
            assert np.asarray(a[0]).tobytes() == np.asarray(b[0]).tobytes() and np.array_equal(a[1], b[1])


def test_documents_are_folded_on_their_own():
    f = AC.compile(DOC_KEYS, fold_bmp=True)
    p = AC.compile(fold3sim.fold3_keys(DOC_KEYS))
    assert f.fold_bmp and f[3] == "ａ" and f[5] == "Р"  # (the caller's spelling)
    check_documents(f, p)


def test_documents_through_the_ranges_paths(monkeypatch):
    """the same batch with the bounds of a range's hit bytes at their minimum (12 bytes, one hit: AHA_CLASS_HIT_BYTES and its
    siblings of DESIGN.md section 7, read when a handle is compiled): class counts, document counts and select (with it replace
    and grep) each split the batch into ranges of whole documents, every range folded on its own with its rebased offsets --
    ranges start with the continuation bytes of a cut character"""
    for name in ("AHA_CLASS_HIT_BYTES", "AHA_DOCCOUNT_HIT_BYTES", "AHA_SELECT_HIT_BYTES"):
        monkeypatch.setenv(name, "12")
    f = AC.compile(DOC_KEYS, fold_bmp=True)
    p = AC.compile(fold3sim.fold3_keys(DOC_KEYS))
    check_documents(f, p)


# ---- every family, small ---------------------------------------------------------------------------------------------------
WORDS = ("ＥＲＲＯＲ ｅｒｒｏｒ Ｗａｒｎｉｎｇ ＡＢＣ Việt VIỆT Nam NAM Nguyễn NGUYỄN Đường phở PHỞ Hà Nội HÀ NỘI "
         "ᾼδης ἈΘΗΝΑ ἀθηνᾶ Ἑλλάς ἑλλάς ὙΠΝΟΣ ქართული ᲥᲐᲠᲗᲣᲚᲘ ႠႡႢ ⴀⴁⴂ Ⅻ ⅻ Ⓚⓚ "
         "Привет МИР мир Σοφία ΣΟΦΙΑ école ÉCOLE straße error ERROR Warning the THE 你好 世界 中文ＡＢ 漢字ａｂ").split()


def family_case():
    rng = np.random.default_rng(7)
    docs = []
    for d in range(24):
        if d in (3, 8, 17):
            docs.append(b"")
            continue
        parts, size = [], 0
        while size < 2000:
            w = WORDS[rng.integers(len(WORDS))]
            r = rng.random()
            w = w.upper() if r < 0.3 else w.lower() if r < 0.6 else w
            sep = " " if rng.random() < 0.8 else "\n"
            b = (w + sep).encode()
            if rng.random() < 0.05:  # random bytes: broken sequences, stray lead and continuation bytes
                b = bytes(rng.integers(0, 256, size=len(b), dtype=np.uint8))
            parts.append(b)
            size += len(b)
        t = b"".join(parts)
        docs.append(t[:len(t) - (d % 4)])  # (some documents end inside a word, perhaps inside a character)
    keys, seen = [], set()
    pool = [w for w in WORDS] + [w[:3] for w in WORDS if len(w) > 4] + [w[-3:] for w in WORDS if len(w) > 5] + ["ｒ", "ệ", "ἀ", "Я", "ქ"]
    for w in pool:
        k = w.encode()
        if fold3sim.fold3(k) not in seen and len(keys) < 50:
            seen.add(fold3sim.fold3(k))
            keys.append(k)
    assert len(keys) == 50 and sum(fold3sim.fold3(k) != foldsim.fold2(k) for k in keys) > 10
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
    # the inputs do exercise the three-byte fold
    assert fc.tobytes() != foldsim.fold2_docs(corpus, doc) and fc.tobytes() != corpus.tobytes()
    f = AC.compile(keys, fold_bmp=True)
    p = AC.compile(fold3sim.fold3_keys(keys))
    assert f.info == p.info  # the engine choice is the one the folded key set gets
    N_ = corpus.size

    def same(a, b):
        assert len(a) == len(b)
        for x, y in zip(a, b):
            assert np.asarray(x).tobytes() == np.asarray(y).tobytes()

    # match with byte offsets and with char offsets, match_longest in both modes; an unaligned corpus goes through once
    want = same_match(f, p, corpus, doc, aligns=(0, 5))
    assert len(want) > 2000
    assert len(AC.compile(keys, fold_simple=True).match_batch(corpus, doc)[0]) < len(want)  # (strictly more than the two-byte fold finds)
    same(f.match_batch(corpus, doc, chars=True), p.match_batch(fc, doc, chars=True))
    for longest in (1, 2):
        same(f.match_batch(corpus, doc, longest=longest), p.match_batch(fc, doc, longest=longest))
    # count, doc counts and class counts
    same(f.count_batch(corpus, doc), p.count_batch(fc, doc))
    same(f.doc_counts_batch(corpus, doc), p.doc_counts_batch(fc, doc))
    classes = [(k % 5,) if k % 7 else (0, 4) for k in range(len(keys))]
    same([f.class_counts_batch(corpus, doc, classes)], [p.class_counts_batch(fc, doc, classes)])
    # cover and redact: the mask of the folded match, the ORIGINAL bytes outside it
    mask, dcov = p.cover_batch(fc, doc)
    same(f.cover_batch(corpus, doc), (mask, dcov))
    red, dcov2 = f.redact_batch(corpus, doc)
    want_red = coversim.redacted(corpus, coversim.unpack(mask, N_), 0x2A)
    assert np.array_equal(red, want_red) and np.array_equal(dcov2, dcov)
    assert not np.array_equal(want_red, coversim.redacted(fc, coversim.unpack(mask, N_), 0x2A))
    # select and replace: the selection of the folded match, the caller's spelling outside the replaced hits
    sel, dso = p.select_batch(fc, doc)
    same(f.select_batch(corpus, doc), (sel, dso))
    repl = {k: ("<%d>" % k).encode() for k in range(0, len(keys), 2)}
    want_out, want_doo = replacesim.replace(corpus, doc, as_list(sel), dso, repl)
    out, doo = f.replace_batch(corpus, doc, repl)
    assert np.array_equal(out, want_out) and np.array_equal(doo, want_doo)
    assert not np.array_equal(want_out, replacesim.replace(fc, doc, as_list(sel), dso, repl)[0])
    # records (no key takes part: the caller's bytes are split) and grep: the kept documents with the caller's spelling
    same(f.records(corpus, doc), p.records(corpus, doc))
    for invert in (False, True):
        kept, _, wdoo = p.grep_batch(fc, doc, invert=invert)
        gk, gout, gdoo = f.grep_batch(corpus, doc, invert=invert)
        assert np.array_equal(gk, kept) and np.array_equal(gdoo, wdoo)
        want_bytes = b"".join(corpus[int(doc[d]):int(doc[d + 1])].tobytes() for d in kept)
        assert gout.tobytes() == want_bytes
    rec, _ = f.records(corpus, doc)
    same(f.grep_batch(corpus, rec, text=False)[::2], p.grep_batch(fc, rec, text=False)[::2])  # (lines, as grep takes them)


# ---- nothing else moved ----------------------------------------------------------------------------------------------------
def fold8_np(a):
    a = np.asarray(a, dtype=np.uint8)
    return np.where((a >= 65) & (a <= 90), a + 32, a).astype(np.uint8)


def test_plain_ascii_and_simple_handles_are_what_they_were():
    keys, corpus, doc, fc = family()
    texts = [(corpus, doc)]
    t = u8(triples_cut_on(3 * 1024 + 5, (1024, 2048, 3072), (1, 2, 1)) + "Привет HELLO".encode())
    texts.append((t, np.array([0, 1024, 1024, t.size], dtype=np.uint64)))
    modes = [({}, lambda c, d: np.asarray(c), lambda k: k),
             ({"fold_ascii": True}, lambda c, d: fold8_np(c), lambda k: fold8_np(u8(k)).tobytes()),
             ({"fold_simple": True}, lambda c, d: u8(foldsim.fold2_docs(c, d)), foldsim.fold2)]
    found = []
    for kw, fold_text, fold_key in modes:
        own, seen = [], set()
        for k in keys:  # (keys that collide under a weaker fold's model do not occur; keep the check honest)
            if fold_key(k) not in seen:
                seen.add(fold_key(k))
                own.append(k)
        m = AC.compile(own, **kw)
        p = AC.compile([fold_key(k) for k in own])
        assert not m.fold_bmp
        n = 0
        for c, d in texts:
            n += len(same_match(m, p, c, d, aligns=(0, 1, 15), fold=fold_text))
        found.append(n)
    f3 = AC.compile(keys, fold_bmp=True)
    n3 = sum(len(f3.match_batch(c, d)[0]) for c, d in texts)
    assert 0 < found[0] < found[1] < found[2] < n3  # each fold finds strictly more than the one before it
