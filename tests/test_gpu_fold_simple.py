"""GPU tests of simple case folding for two-byte UTF-8 characters (AHA_OPT_FOLD_SIMPLE, include/aha_hip.h).  THE RULE: every
call on a handle compiled with the flag gives, bit for bit, what the same call gives on an ordinary handle compiled from
fold2(key) of each key over the batch in which each document is folded on its own.  The yardstick everywhere is that ordinary
handle, given tests/foldsim.py's fold of the keys and of the corpus (plain Python from str.upper / str.lower; it does not read
the committed table).  The exceptions are the ASCII fold's: redact, replace and grep give the caller's bytes, keys keep their
spelling."""
import numpy as np
import pytest
import torch

import coversim
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
    return u8(foldsim.fold2_docs(corpus, doc))


def as_list(h):
    return [(int(s), int(e), int(v)) for s, e, v in np.asarray(h).tolist()]


def on_device(corpus, align):
    """the corpus as a slice of a larger device tensor whose address is `align` modulo 16; the bytes around the slice would pair
    with its ends (a lead byte in front, continuation bytes behind) if a kernel looked at them"""
    n = corpus.size
    big = torch.full((n + 64,), 0xA0, dtype=torch.uint8, device=DEV)
    shift = (align - big.data_ptr()) % 16 + 16
    big[:shift] = 0xD0
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


def same_match(f, p, corpus, doc, aligns=(0,), **kw):
    """f over the corpus == p over the per-document fold, hits and per-document offsets, at every alignment; -> p's hits"""
    want_h, want_d = p.match_batch(folded(corpus, doc), doc, **kw)
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


def byte_readers():
    return AC.compile(BYTE_KEYS, fold_simple=True), AC.compile(BYTE_KEYS)


# ---- every pair at every phase ---------------------------------------------------------------------------------------------
def test_every_pair_at_every_phase_of_a_piece():
    chars = [chr(cp) for cp in range(0x80, 0x800)]
    # one key per case class, spelled as its first member (the folded spelling is another one for most): the ordinary handle
    # has the folded spellings in the same order, so ids map one to one
    first = {}
    for c in chars:
        first.setdefault(foldsim.F(c), c)
    spelled = [first[r].encode() for r in sorted(first)]
    assert len(spelled) == len({foldsim.fold2(k) for k in spelled}) and any(foldsim.fold2(k) != k for k in spelled)
    f = AC.compile(spelled, fold_simple=True)
    p = AC.compile(foldsim.fold2_keys(spelled))
    # the text: for every phase 0 .. 15 each of the 1920 characters once, with 0 .. 16 ASCII bytes (both cases) in front so
    # that it starts at that phase of a 16-byte piece -- phase 15 is the straddle
    pad = b"aZbYcXdWeVfUgThSi"
    parts, at, met = [], 0, set()
    for phase in range(16):
        for k, c in enumerate(chars):
            g = (phase - at) % 16
            if g == 0 and k % 5 == 0:
                g = 16
            parts.append(pad[:g] + c.encode())
            at += g + 2
            met.add((k, (at - 2) % 16))
    assert len(met) == 1920 * 16
    base = b"".join(parts) + b"q" * (-at % 16)
    assert len(base) % 16 == 0
    texts = [base, base + b"Q" * 15 + "Я".encode(), base + "Я".encode() * 7 + b"Q"]  # n % 16 = 0, 1 (a tail of one
    assert [len(t) % 16 for t in texts] == [0, 1, 15]                                # continuation byte), 15
    for t in texts:
        corpus = u8(t)
        doc = np.array([0, corpus.size], dtype=np.uint64)
        want = same_match(f, p, corpus, doc, aligns=(0, 1, 15))
        assert len(want) >= 1920 * 16  # every character was found under its class's key
    # ... and the same bytes read one by one
    fb, pb = byte_readers()
    corpus = u8(texts[1])
    want = same_match(fb, pb, corpus, np.array([0, corpus.size], dtype=np.uint64), aligns=(0, 1, 15))
    assert len(want) == corpus.size


# ---- boundaries the kernel can get wrong ---------------------------------------------------------------------------------------
def fold_grid(n_bytes, max_blocks):
    """the staged copy's grid (scan_fold.hip): a workgroup of 256 lanes per 1024 pieces, max_blocks at the most"""
    return max(1, min((n_bytes // 16 + 1023) // 1024, max_blocks))


def cyrillic_on_every_edge(n):
    """n bytes of upper-case Cyrillic at an odd phase: every 16-byte piece, so every wave's 1 KiB, ends with a lead byte"""
    t = b"x" + "РСТУФХЦЧШЩ".encode() * (n // 20 + 1)
    return t[:n]


@pytest.mark.parametrize("reserve", [None, "1"])
def test_wave_edges_grid_strides_and_short_buffers(reserve, monkeypatch):
    if reserve:
        monkeypatch.setenv("AHA_RESERVE_CUS", reserve)
    fb, pb = byte_readers()
    one_doc = lambda c: np.array([0, c.size], dtype=np.uint64)
    # 3 KiB + 5: pairs on each 1 KiB wave edge; one workgroup, every lane at most one piece -- no stride, with or without a
    # reserved CU (the grid is ceil(pieces / 1024) workgroups for any cap of 512 or more, and the cap is 8 * max(grid, 64))
    n = 3 * 1024 + 5
    corpus = u8(cyrillic_on_every_edge(n))
    assert all(corpus[e - 1] in (0xD0, 0xD1) and 0x80 <= corpus[e] <= 0xBF for e in (1024, 2048, 3072))
    assert n // 16 <= fold_grid(n, 512) * 256
    same_match(fb, pb, corpus, one_doc(corpus), aligns=(0, 1, 15))
    # AHA_RESERVE_CUS does not make lanes stride (it only lowers the cap, which this size is far below): the buffer that does
    # is long enough by the grid formula -- 1800 pieces on 2 workgroups, stride 512: lanes take up to four pieces, both the
    # unrolled loop (i + 3 * 512 < 1800) and the remainder loop run, and a pair sits on every stride edge
    n = 1800 * 16 + 5
    g = fold_grid(n, 512)
    assert g == 2 and n // 16 > g * 256 and 3 * g * 256 < n // 16
    corpus = u8(cyrillic_on_every_edge(n))
    assert all(corpus[e - 1] in (0xD0, 0xD1) and 0x80 <= corpus[e] <= 0xBF for e in (512 * 16, 1024 * 16, 1536 * 16))
    same_match(fb, pb, corpus, one_doc(corpus), aligns=(0, 15))
    # a last byte that is a lead byte, a buffer of continuation bytes only, and the lengths around one piece
    for t in (b"Hello \xd0", "ПРИВЕТ".encode() + b"\xd0", b"\xa0", b"\xa0" * 40, b"\xd0" * 33):
        corpus = u8(t)
        want = same_match(fb, pb, corpus, one_doc(corpus), aligns=(0, 1, 15))
        assert len(want) == corpus.size
    src = ("ЩЯ".encode() * 5)
    for n in (0, 1, 2, 15, 16, 17):
        for lead_in in (0, 1):  # (cut in front of a lead byte, and in front of a continuation byte)
            corpus = u8(src[lead_in:lead_in + n])
            if n == 0:
                h, d = fb.match_batch(corpus, one_doc(corpus))
                assert len(h) == 0 and list(d) == [0, 0]
                continue
            same_match(fb, pb, corpus, one_doc(corpus), aligns=(0, 1, 15))


# ---- documents -----------------------------------------------------------------------------------------------------------------
DOC_KEYS = [b"a\xd0", b"\xa0b", "Р".encode()]
DOCS = [b"a\xd0", b"\xa0b", b"", b"\xd0", b"\xa0", "Рр".encode()]


def sep_d0_not_d1():
    sep = BitArray(256)
    for c in range(256):
        sep[c] = c != 0xD1
    return sep


def check_documents(f, p):
    corpus, doc = u8(b"".join(DOCS)), offsets_of(DOCS)
    fc = folded(corpus, doc)
    assert fc.tobytes() != foldsim.fold2(corpus.tobytes())  # the buffer folded whole pairs doc 0's end with doc 1's start
    want = same_match(f, p, corpus, doc, aligns=(0, 1, 15))
    got = as_list(want)
    wd = p.match_batch(fc, doc)[1]
    assert got[int(wd[0]):int(wd[1])] == [(0, 2, 0)] and got[int(wd[1]):int(wd[2])] == [(0, 2, 1)]  # without the fix-up: neither
    assert got[int(wd[5]):int(wd[6])] == [(0, 2, 2), (2, 4, 2)]
    # a separator filter whose bit for 0xD0 is set and for 0xD1 clear: "Р" in "Рр" is followed by 0xD1 (blocked) and the
    # second "р" by the document's end; the hit "\xa0b" of document 1 has document 0's 0xD0 in front of it in the buffer --
    # it must not be looked at, and folded with it it would be 0xD1
    sep = sep_d0_not_d1()
    want_s = same_match(f, p, corpus, doc, aligns=(0, 1, 15), sep=sep)
    assert 0 < len(want_s) < len(want)
    # every family that has its own way into the text, against the yardstick
    kc, cd = f.count_batch(corpus, doc)
    wkc, wcd = p.count_batch(fc, doc)
    assert np.array_equal(kc, wkc) and np.array_equal(cd, wcd) and list(kc) == [1, 1, 2]
    kc, cd = f.count_batch(corpus, doc, sep=sep)
    wkc, wcd = p.count_batch(fc, doc, sep=sep)
    assert np.array_equal(kc, wkc) and np.array_equal(cd, wcd)
    a, b = f.doc_counts_batch(corpus, doc), p.doc_counts_batch(fc, doc)
    assert a[0].tobytes() == b[0].tobytes() and np.array_equal(a[1], b[1])
    classes = [0, 1, (0, 2)]
    assert np.array_equal(f.class_counts_batch(corpus, doc, classes), p.class_counts_batch(fc, doc, classes))
    a, b = f.select_batch(corpus, doc), p.select_batch(fc, doc)
    assert a[0].tobytes() == b[0].tobytes() and np.array_equal(a[1], b[1]) and len(a[0]) == 4
    a, b = f.cover_batch(corpus, doc), p.cover_batch(fc, doc)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    kept, _, _ = f.grep_batch(corpus, doc)
    assert list(kept) == [0, 1, 5]
    for chars in (False, True):
        for longest in (1, 2):
            a, b = f.match_batch(corpus, doc, chars=chars, longest=longest), p.match_batch(fc, doc, chars=chars, longest=longest)
            assert np.asarray(a[0]).tobytes() == np.asarray(b[0]).tobytes() and np.array_equal(a[1], b[1])


def test_documents_are_folded_on_their_own():
    f = AC.compile(DOC_KEYS, fold_simple=True)
    p = AC.compile(foldsim.fold2_keys(DOC_KEYS))
    assert f.fold_simple and f[2] == "Р"  # (the caller's spelling)
    check_documents(f, p)


def test_documents_through_the_ranges_paths(monkeypatch):
    """the same batch with the bounds of a range's hit bytes at their minimum (12 bytes, one hit: AHA_CLASS_HIT_BYTES and its
    siblings of DESIGN.md section 7, read when a handle is compiled): the batch has four hits in three documents, so class
    counts, document counts and select (with it replace and grep) each split it into ranges of whole documents, every range
    folded on its own with its rebased offsets -- the second range starts with document 1's continuation byte"""
    for name in ("AHA_CLASS_HIT_BYTES", "AHA_DOCCOUNT_HIT_BYTES", "AHA_SELECT_HIT_BYTES"):
        monkeypatch.setenv(name, "12")
    f = AC.compile(DOC_KEYS, fold_simple=True)
    p = AC.compile(foldsim.fold2_keys(DOC_KEYS))
    check_documents(f, p)


# ---- every family, small ---------------------------------------------------------------------------------------------------
WORDS = ("Привет МИР мир Москва ЁЛКА ёж Ёж съезд ПОДЪЕЗД Σοφία ΣΟΦΙΑ λόγος ΛΌΓΟΣ Άλφα ωμέγα école ÉCOLE Élève français FRANÇAIS "
         "Ærø straße STRASSE µm error ERROR Warning naïve NAÏVE Őz ǅ ǆ Ԁԁ Ֆֆ the THE quick").split()


def family_case():
    rng = np.random.default_rng(5)
    docs = []
    for d in range(12):
        if d in (3, 8):
            docs.append(b"")
            continue
        parts, size = [], 0
        while size < 4000:
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
        docs.append(t[:len(t) - (d % 3)])  # (some documents end inside a word, perhaps inside a character)
    keys, seen = [], set()
    pool = [w for w in WORDS] + [w[:3] for w in WORDS if len(w) > 4] + [w[-3:] for w in WORDS if len(w) > 5] + ["ё", "σο", "éc", "Я"]
    for w in pool:
        k = w.encode()
        if foldsim.fold2(k) not in seen and len(keys) < 50:
            seen.add(foldsim.fold2(k))
            keys.append(k)
    assert len(keys) == 50 and any(foldsim.fold2(k) != k for k in keys)
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
    assert 30_000 < corpus.size < 60_000
    f = AC.compile(keys, fold_simple=True)
    p = AC.compile(foldsim.fold2_keys(keys))
    assert f.info == p.info  # the engine choice is the one the folded key set gets
    N_ = corpus.size

    def same(a, b):
        assert len(a) == len(b)
        for x, y in zip(a, b):
            assert np.asarray(x).tobytes() == np.asarray(y).tobytes()

    # match with byte offsets and with char offsets, match_longest in both modes; an unaligned corpus goes through once
    want = same_match(f, p, corpus, doc, aligns=(0, 5))
    assert len(want) > 2000
    assert len(want) > len(AC.compile(keys).match_batch(corpus, doc)[0])  # (the fold found more than the spelling does)
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


def test_ascii_fold_and_plain_handles_are_what_they_were():
    text = "Привет, МИР! Hello WORLD, привет мир. ÉCOLE école Σοφία".encode() * 50
    corpus = u8(text)
    doc = np.array([0, 7 * len(text) // 50, 7 * len(text) // 50, corpus.size], dtype=np.uint64)  # (cut between two repetitions)
    keys = ["привет", "МИР", "hello", "World", "école"]
    # only FOLD_ASCII: fold8 of every byte -- keys and text -- and nothing else
    a = AC.compile(keys, fold_ascii=True)
    pa = AC.compile([fold8_np(u8(k.encode())).tobytes() for k in keys])
    assert a.fold_ascii and not a.fold_simple
    want, wd = pa.match_batch(fold8_np(corpus), doc)
    for align in (0, 3):
        got, gd = dev_match(a, on_device(corpus, align), doc, len(want))
        assert got.tobytes() == np.asarray(want).view(np.int32).tobytes() and np.array_equal(gd, wd)
    by_key = np.bincount(np.asarray(want)["value"], minlength=len(keys))
    assert by_key[0] > 0 and by_key[2] > 0 and by_key[3] > 0 and by_key[4] > 0 and by_key[1] > 0
    assert by_key[0] == 50 and by_key[1] == 50 and by_key[4] == 50  # "Привет", "мир" and "ÉCOLE" are not found: bytes >= 0x80 stay
    # no flag: case is ignored nowhere
    plain = AC.compile(keys)
    got, _ = plain.match_batch(corpus, doc)
    assert np.array_equal(np.bincount(np.asarray(got)["value"], minlength=len(keys)), [50, 50, 0, 0, 50])
    # ... and the simple fold finds all of them
    s = AC.compile(keys, fold_simple=True)
    got, _ = s.match_batch(corpus, doc)
    assert np.array_equal(np.bincount(np.asarray(got)["value"], minlength=len(keys)), [100, 100, 50, 50, 100])
