"""Excerpts (aha_ac_grep_batch* with AHA_GREP_CONTEXT) bit-exact against excerptsim.excerpts over the CPU ORACLE's hits (never
the library's own match).  Each case makes the device call twice with guard words around every buffer and compares the bytes,
then starts only, then out only, then the host entry.  Gap edges on mask-word, rank-block and 8192 boundaries; contexts from 0
to 0x7FFFFFFF; documents of every awkward kind; UTF-8 and stray continuation bytes; engines and options; alignment; capacity;
one-block grids; one handle through a sequence of calls that share scratch.  Every case is a few KiB of text."""
import random
import zlib

import numpy as np
import pytest

import excerptsim
import pyoracle as orc
from aha_amd import AC, AhaError
from aha_amd import _native as N
from test_excerpt_host import oracle_hits_per_doc
from test_gpu_doc_counts import KEYSETS, SEP_BITS, _batch, _sep

pytestmark = pytest.mark.gpu

GUARD8 = 0x5A
GUARD64 = 0x5A5A5A5A5A5A5A5A
PAD = 16
DEV = "cuda:0"
MAXC = 0x7FFFFFFF
SEP_PAIR = (40, [i for i in range(40) if i not in SEP_BITS])


def _tensors(corpus, offs, shift=0):
    import torch

    buf = torch.zeros(corpus.size + shift + 16, dtype=torch.uint8, device=DEV)
    ct = buf[shift:shift + corpus.size]
    if corpus.size:
        ct.copy_(torch.from_numpy(np.ascontiguousarray(corpus)))
    return ct, torch.from_numpy(np.asarray(offs, dtype=np.uint64).view(np.int64)).to(DEV)


def _want(o, corpus, offs, before, after, sep_pair=None, oracle_corpus=None):
    """the twin over the oracle's hits (of oracle_corpus where the handle folds: the bytes cut out are the caller's)
    -> (starts, out, out_offsets, n_hits)"""
    per, n_hits = oracle_hits_per_doc(o, corpus if oracle_corpus is None else oracle_corpus, offs, sep_pair)
    starts, out, oo = excerptsim.excerpts(per, offs, corpus, before, after)
    return starts, out, oo, n_hits


def _device(m, ct, ot, cap, cap_bytes, before, after, sep=None, ids=True, text=True):
    """the device entry with guard words around every buffer -> (starts, oo, out, R, nb, nh, rc); after a failing call every
    buffer is still all guard"""
    import torch

    st = torch.full((cap + PAD,), GUARD64, dtype=torch.int64, device=DEV)
    oo = torch.full((cap + 1 + PAD,), GUARD64, dtype=torch.int64, device=DEV)
    big = torch.full((cap_bytes + 2 * PAD,), GUARD8, dtype=torch.uint8, device=DEV)
    out = big[PAD:PAD + cap_bytes] if text else None
    rc, nh = N.AHA_OK, None
    try:
        nk, nb, nh = m.excerpts_batch_device(ct, ot, st if ids else None, oo if ids else None, out, before=before, after=after,
                                             sep=sep, cap=cap)
    except AhaError as e:
        if e.code == N.AHA_E_CAPACITY:
            rc, nk, nb = e.code, e.n_required, e.bytes_required
        else:
            rc, nk, nb = e.code, None, None
    torch.cuda.synchronize()
    st_h, oo_h, big_h = st.cpu().numpy(), oo.cpu().numpy(), big.cpu().numpy()
    assert (st_h[cap:] == GUARD64).all() and (oo_h[cap + 1:] == GUARD64).all(), "the call wrote behind cap"
    assert (big_h[:PAD] == GUARD8).all() and (big_h[PAD + cap_bytes:] == GUARD8).all(), "the call wrote outside out"
    if rc != N.AHA_OK or not text:
        assert (big_h == GUARD8).all()
    if rc != N.AHA_OK or not ids:
        assert (st_h == GUARD64).all() and (oo_h == GUARD64).all()
    return st_h[:cap], oo_h[:cap + 1], big_h[PAD:PAD + cap_bytes], nk, nb, nh, rc


def _check(m, o, corpus, offs, before, after, sep_pair=None, sep=None, oracle_corpus=None, host=True, shift=0, want=None):
    """the device entry twice (identical bytes), starts only, out only, the sizing call and the host entry, against the twin"""
    want = want or _want(o, corpus, offs, before, after, sep_pair, oracle_corpus)
    w_st, w_out, w_oo, w_hits = want
    R, nb0 = w_st.size, w_out.size
    ct, ot = _tensors(corpus, offs, shift)
    first = None
    for _ in range(2):
        st, oo, out, nk, nb, nh, rc = _device(m, ct, ot, R + 2, nb0 + 5, before, after, sep)
        assert rc == N.AHA_OK and (nk, nb, nh) == (R, nb0, w_hits), (nk, nb, nh, R, nb0, w_hits)
        assert np.array_equal(st[:R].astype(np.uint64), w_st) and (st[R:] == GUARD64).all()
        assert np.array_equal(oo[:R + 1].astype(np.uint64), w_oo) and (oo[R + 1:] == GUARD64).all()
        assert out[:nb].tobytes() == w_out.tobytes() and (out[nb:] == GUARD8).all()
        got = (st.tobytes(), oo.tobytes(), out.tobytes())
        assert first is None or got == first
        first = got
    st, oo, _, nk, nb, nh, rc = _device(m, ct, ot, R, 0, before, after, sep, text=False)
    assert rc == N.AHA_OK and (nk, nb, nh) == (R, nb0, w_hits)
    assert np.array_equal(st.astype(np.uint64), w_st) and np.array_equal(oo.astype(np.uint64), w_oo)
    _, _, out, nk, nb, nh, rc = _device(m, ct, ot, 0, nb0, before, after, sep, ids=False)
    assert rc == N.AHA_OK and (nk, nb, nh) == (R, nb0, w_hits) and out.tobytes() == w_out.tobytes()
    assert m.excerpts_batch_device(ct, ot, before=before, after=after, sep=sep) == (R, nb0, w_hits)  # the sizing call
    if host:
        h_st, h_out, h_oo, h_deo = m.excerpts_batch(corpus, offs, before, after, sep=sep)
        assert np.array_equal(h_st, w_st) and h_out.tobytes() == w_out.tobytes() and np.array_equal(h_oo, w_oo)
        assert np.array_equal(h_deo, np.searchsorted(w_st, np.asarray(offs, dtype=np.uint64)).astype(np.uint64))
        assert int(h_deo[-1]) == R
    return want


@pytest.fixture(scope="module")
def plain():
    keys = [b"KEY", b"ab"]
    return AC.compile(keys), orc.AC.compile(keys)


# ---- the header's examples, by the library ---------------------------------------------------------------------------------
def test_the_header_examples_on_the_device(plain):
    m, o = plain
    corpus, offs = _batch([b"xxabxxxxabx", b"ab"])
    st, out, oo, nh = _check(m, o, corpus, offs, 1, 2)
    assert st.tolist() == [1, 7, 11] and out.tobytes() == b"xabxxxabxab" and oo.tolist() == [0, 5, 9, 11] and nh == 3
    st, out, oo, nh = _check(m, o, corpus, offs, 1, 3)
    assert st.tolist() == [1, 11] and out.tobytes() == b"xabxxxxabxab" and oo.tolist() == [0, 10, 12]
    keys = ["是".encode()]
    m2, o2 = AC.compile(keys), orc.AC.compile(keys)
    text = "我是中".encode()
    st, out, oo, nh = _check(m2, o2, *_batch([text]), 1, 1)
    assert st.tolist() == [0] and out.tobytes() == text and nh == 1
    assert m.excerpts(b"xxabxxxxabx", 1, 2) == [(1, b"xabxx"), (7, b"xabx")]
    assert m2.excerpts("我是中国人 是", 0) == [(1, "是"), (6, "是")]
    assert m2.excerpts("我是中国人", 1, 4) == [(0, "我是中国")]


# ---- gap edges ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("edge", [96, 2048, 8192])
@pytest.mark.parametrize("off", [-1, 0, 1])
@pytest.mark.parametrize("gap", [-1, 0, 1])
def test_neighbouring_windows_overlap_touch_and_miss_on_an_edge(plain, edge, off, gap):
    """two planted keys whose windows overlap by one byte (gap -1), touch (0) and miss by one byte (1), the seam -- the first
    window's end -- just below, on and just above a mask word's, a rank block's and 8192's boundary"""
    m, o = plain
    before, after = 5, 7
    seam = edge + off
    text = bytearray(b"x" * (edge + 300))
    for h in (seam - after - 3, seam + gap + before, edge + 200):
        text[h:h + 3] = b"KEY"
    corpus, offs = _batch([b"", bytes(text)])
    st, out, oo, nh = _check(m, o, corpus, offs, before, after, host=(edge == 96))
    assert nh == 3 and st.size == (3 if gap == 1 else 2)
    assert int(st[0]) == seam - after - 3 - before
    if gap == 1:
        assert int(st[1]) == seam + 1 and int(oo[1]) == before + 3 + after


@pytest.mark.parametrize("n", [0, 1, 31, 32, 33, 2047, 2048, 2049, 4097])
def test_batch_sizes_on_the_edges(plain, n):
    m, o = plain
    rng = random.Random(n)
    text = bytearray(b"x" * n)
    for h in range(0, max(n - 2, 0), 37):
        text[h:h + 3] = b"KEY"
    if n >= 3:
        text[n - 3:n] = b"KEY"
    free = [p for p in range(n - 2) if p % 37 >= 3]  # (no cut inside a planted key)
    cuts = sorted({0, n} | {rng.choice(free) for _ in range(9 if free else 0)})
    offs = np.array(cuts if n else [0, 0], dtype=np.uint64)
    corpus = np.frombuffer(bytes(text), dtype=np.uint8).copy()
    st, out, oo, nh = _check(m, o, corpus, offs, 2, 3)
    assert (nh > 0) == (n >= 3) and (st.size > 0) == (nh > 0)


# ---- contexts ----------------------------------------------------------------------------------------------------------------
def _mixed_docs(rng, n_docs=60):
    docs = []
    for d in range(n_docs):
        n = rng.choice([0, 1, 1, 7, 40, 130, 400])
        out = bytearray()
        while len(out) < n:
            out += rng.choice([b"KEY", b"ab"]) if rng.random() < 0.06 else rng.choice([b" ", b"q", b"zz", "中".encode(), b"x" * 9])
        docs.append(bytes(out[:n]))
    return docs


CONTEXTS = [0, 1, 3, 31, 32, 33, 4096, MAXC]


@pytest.fixture(scope="module")
def mixed_batch():
    return _batch(_mixed_docs(random.Random(11)))


@pytest.mark.parametrize("pair", [(c, c) for c in CONTEXTS] + [(0, 33), (31, 0), (1, 4096), (MAXC, 0), (0, MAXC), (3, 32), (32, 1)])
def test_contexts(plain, mixed_batch, pair):
    m, o = plain
    corpus, offs = mixed_batch
    st, out, oo, nh = _check(m, o, corpus, offs, pair[0], pair[1], host=pair in ((3, 3), (MAXC, 0)))
    assert nh > 20 and st.size > 5


def test_no_context_equals_cover_and_the_largest_equals_grep(plain, mixed_batch):
    import torch

    m, o = plain
    corpus, offs = mixed_batch
    ct, ot = _tensors(corpus, offs)
    D = len(offs) - 1
    n_cov, n_hits = m.cover_batch_device(ct, ot)
    R, nb, nh = m.excerpts_batch_device(ct, ot, before=0)
    assert (nb, nh) == (n_cov, n_hits) and R > 0  # example 3
    kept = torch.zeros(D, dtype=torch.int64, device=DEV)
    doo = torch.zeros(D + 1, dtype=torch.int64, device=DEV)
    g_out = torch.zeros(corpus.size, dtype=torch.uint8, device=DEV)
    nk, g_nb, g_nh = m.grep_batch_device(ct, ot, kept, doo, g_out)
    st, oo, out, R, nb, nh, rc = _device(m, ct, ot, D, corpus.size, MAXC, MAXC)
    assert rc == N.AHA_OK and (R, nb, nh) == (nk, g_nb, g_nh) and 0 < nk < D  # example 4
    assert out[:nb].tobytes() == g_out.cpu().numpy()[:g_nb].tobytes()
    assert np.array_equal(st[:R].astype(np.uint64), np.asarray(offs)[kept.cpu().numpy()[:nk]])
    assert np.array_equal(oo[:R + 1], doo.cpu().numpy()[:nk + 1])


# ---- documents ---------------------------------------------------------------------------------------------------------------
def test_empty_batches_and_batches_without_a_hit(plain):
    m, o = plain
    for docs in ([], [b""], [b"", b"", b""], [b"xxxx", b"", b"nothing here"], [b"x"] * 40):
        corpus = np.frombuffer(b"".join(docs), dtype=np.uint8).copy()
        offs = np.cumsum([0] + [len(d) for d in docs]).astype(np.uint64)
        st, out, oo, nh = _check(m, o, corpus, offs, 3, 3)
        assert st.size == 0 and out.size == 0 and oo.tolist() == [0] and nh == 0
        ct, ot = _tensors(corpus, offs)
        st, oo, out, R, nb, nh, rc = _device(m, ct, ot, 4, 8, 3, 3)
        assert rc == N.AHA_OK and (R, nb, nh) == (0, 0, 0)
        assert (st == GUARD64).all() and (out == GUARD8).all() and oo[0] == 0 and (oo[1:] == GUARD64).all()  # entry R is the total


def test_every_byte_covered_and_one_byte_documents():
    keys = [b"a", b"ab"]
    m, o = AC.compile(keys), orc.AC.compile(keys)
    for docs in ([b"a" * 100], [b"a"] * 70, [b"a", b"", b"a", b"b", b"a", b"a"] * 12, [b"aaaa"] * 33 + [b""] + [b"a" * 31, b"a"]):
        corpus, offs = _batch(docs)
        for c in (0, 1, 40):
            st, out, oo, nh = _check(m, o, corpus, offs, c, c, host=c == 1)
            if b"b" not in b"".join(docs):  # neighbouring documents fully inside windows stay apart: one excerpt per non-empty document
                assert st.tolist() == [int(offs[d]) for d in range(len(docs)) if docs[d]]
                assert out.tobytes() == corpus.tobytes()


def test_4097_short_documents_with_runs_on_word_and_block_edges(plain):
    m, o = plain
    D = 4097
    hit = np.zeros(D, dtype=bool)
    for a, b in ((0, 1), (30, 33), (63, 65), (2040, 2050), (2047, 2048), (4090, 4097), (100, 101), (1000, 1032)):
        hit[a:b] = True
    hit[200:1000:3] = True
    docs = [b"KEY" if h else (b"xx" if d % 7 else b"") for d, h in enumerate(hit)]
    corpus, offs = _batch(docs)
    for c in (0, 1, 2, 5):  # 1: an excerpt takes a byte of nothing (documents of 3 bytes); 2 and 5: clipped to the documents
        st, out, oo, nh = _check(m, o, corpus, offs, c, c, host=c == 2)
        assert nh == int(hit.sum()) and st.size == nh and out.size == 3 * nh


def test_contexts_far_larger_than_the_documents(plain):
    m, o = plain
    docs = [b"xKEYx", b"KEY", b"xxxxxxKEY", b"", b"KEYxxxxxxxxxxab", b"nothing", b"ab"]
    corpus, offs = _batch(docs)
    for pair in ((1000, 1000), (0, 5000), (MAXC, 3), (MAXC - 1, MAXC)):
        st, out, oo, nh = _check(m, o, corpus, offs, *pair)
        assert st.size == 5


# ---- UTF-8 -------------------------------------------------------------------------------------------------------------------
def test_contexts_end_inside_characters_at_every_phase():
    keys = ["是".encode(), "é".encode(), b"k", "😀".encode()]
    m, o = AC.compile(keys), orc.AC.compile(keys)
    docs = ["我是中国人，é和😀都在这里 k 末尾", "ñaé😀😀k中", "k", "中k中", "😀是😀", "éé k éé" * 3, "aaaa是aaaa😀aaaak"]
    corpus, offs = _batch([d.encode() for d in docs])
    for before in range(0, 6):
        for after in (0, 1, 2, 3):
            st, out, oo, nh = _check(m, o, corpus, offs, before, after, host=(before, after) == (2, 3))
            for r in range(st.size):  # on valid UTF-8 no excerpt begins or ends inside a character
                out[int(oo[r]):int(oo[r + 1])].tobytes().decode("utf-8")


def test_stray_continuation_bytes_move_an_edge_by_three_at_most():
    keys = [b"k"]
    m, o = AC.compile(keys), orc.AC.compile(keys)
    five = b"\x80\xBF\x81\x80\xBF"
    docs = [b"A" + five + b"k" + five + b"A", five + b"k" + five, b"AA" + five * 2 + b"k" + five * 2 + b"AA"]
    corpus, offs = _batch(docs)
    for c in range(0, 12):
        st, out, oo, nh = _check(m, o, corpus, offs, c, c, host=c == 2)
    st, out, oo, nh = _check(m, o, corpus, offs, 1, 1)
    assert out[int(oo[0]):int(oo[1])].tobytes() == five[1:] + b"k" + five[:4]  # 1 of context + 3 snapped, on either side


def test_continuation_bytes_at_document_edges_are_not_read_across():
    """a document that starts (ends) with continuation bytes beside one that ends (starts) with another class of byte: the snap
    stops at the document's edge whatever lies beyond it"""
    keys = [b"k"]
    m, o = AC.compile(keys), orc.AC.compile(keys)
    tails = [b"\x80\x80", b"\xE6", b"A", b"\x80\x80\x80\x80"]
    seen = set()
    for left in tails:
        for right in tails:
            docs = [b"Ak" + left, right + b"k" + left, right + b"kA", b"\x80k\x80", b"k"]
            corpus, offs = _batch(docs)
            for c in (0, 1, 2, 3):
                st, out, oo, nh = _check(m, o, corpus, offs, c, c, host=False)
                assert nh == 5 and st.size == 5  # clipped: never merged across a boundary
                seen.add((int(st[1]) - int(offs[1]), c))
    assert len(seen) > 4


# ---- engines and options -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("keyset", ["utf8", "keywords"])
def test_a_unit_image_key_set_and_a_keyword_list(keyset):
    from aha_amd import synth

    rng = random.Random(zlib.crc32(keyset.encode()))
    if keyset == "utf8":
        keys = KEYSETS["utf8"](rng)
    else:
        blob, koffs, _ = synth.keys(2)
        keys = [bytes(blob[koffs[i]:koffs[i + 1]]) for i in range(koffs.size - 1)]
    m, o = AC.compile(keys), orc.AC.compile(keys)
    if keyset == "utf8":
        assert m.info["unit_enabled"]
    docs = []
    for d in range(100):
        n = rng.choice([0, 5, 30, 90, 250])
        out = bytearray()
        while len(out) < n:
            out += rng.choice(keys) if rng.random() < 0.05 else rng.choice([b" ", b"q", "中".encode(), b"\n", b"zzzz"])
        docs.append(bytes(out[:n]))  # (cut anywhere: characters may be cut at a document's end)
    corpus, offs = _batch(docs)
    for pair in ((0, 0), (4, 9), (33, 2)):
        st, out, oo, nh = _check(m, o, corpus, offs, *pair, host=pair == (4, 9))
        assert nh > 10 and 5 < st.size


def test_a_separator_filter(plain, mixed_batch):
    m, o = plain
    corpus, offs = mixed_batch
    filtered = _check(m, o, corpus, offs, 4, 6, sep_pair=SEP_PAIR, sep=_sep())
    unfiltered = _check(m, o, corpus, offs, 4, 6, host=False)
    assert 0 < filtered[3] < unfiltered[3] and 0 < filtered[0].size < unfiltered[0].size  # (the filter drops hits)


def test_folded_handles_cut_out_the_original_spelling():
    keys = [b"key", b"word", "é".encode(), "жук".encode()]
    o = orc.AC.compile(keys)
    docs_lower = ["a key and a word", "", "жук é word", "nothing", "keykey é", "xx жукжук key"] * 8
    docs_mixed = [d.upper() if i % 3 == 2 else d.replace("key", "KeY") for i, d in enumerate(docs_lower)]
    assert all(len(a.encode()) == len(b.encode()) for a, b in zip(docs_lower, docs_mixed))
    lower, offs = _batch([d.encode() for d in docs_lower])
    mixed, _ = _batch([d.encode() for d in docs_mixed])
    ascii_lower = mixed.copy()  # what fold_ascii sees of the mixed text: only A-Z folded
    ascii_lower[(mixed >= ord("A")) & (mixed <= ord("Z"))] += 32
    for opts, folded in (({"fold_ascii": True}, ascii_lower), ({"fold_simple": True}, lower)):
        m = AC.compile(keys, **opts)
        st, out, oo, nh = _check(m, o, mixed, offs, 3, 2, oracle_corpus=folded)
        assert nh > 20 and b"KeY" in out.tobytes() and b"WORD" in out.tobytes()
        if "fold_simple" in opts:
            assert "ЖУК".encode() in out.tobytes()


def test_record_offsets_as_documents_clip_the_contexts_to_lines(plain):
    import torch

    m, o = plain
    text = (b"a KEY here\n" + b"nothing\n" + b"\n" + b"KEY\nKEY at the start\n" + b"x" * 50 + b"ab" + b"y" * 50 + b"\nlast line ab") * 5
    corpus = np.frombuffer(text, dtype=np.uint8).copy()
    ct, ot = _tensors(corpus, np.array([0, corpus.size], dtype=np.uint64))
    with pytest.raises(AhaError) as e:  # (the sizing call of records reports the number it needs)
        m.records_device(ct, ot, None)
    n_rec = e.value.n_required
    rec = torch.zeros(n_rec + 1, dtype=torch.int64, device=DEV)
    assert m.records_device(ct, ot, rec) == n_rec
    rec_h = rec.cpu().numpy().astype(np.uint64)
    want = _want(o, corpus, rec_h, 6, 20)
    st, oo, out, R, nb, nh, rc = _device(m, ct, rec, want[0].size, want[1].size, 6, 20)
    assert rc == N.AHA_OK and np.array_equal(st.astype(np.uint64), want[0]) and out.tobytes() == want[1].tobytes()
    pieces = [out[int(oo[r]):int(oo[r + 1])].tobytes() for r in range(R)]
    assert b"a KEY here\n" in pieces and b"KEY\n" in pieces and all(p.count(b"\n") <= 1 for p in pieces)


# ---- alignment ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shift", [1, 7, 15])
def test_the_corpus_may_start_anywhere(plain, mixed_batch, shift):
    m, o = plain
    corpus, offs = mixed_batch
    _check(m, o, corpus, offs, 5, 40, host=False, shift=shift)


# ---- capacity ----------------------------------------------------------------------------------------------------------------
def test_capacity_failures_report_both_numbers_and_write_nothing(plain, mixed_batch):
    m, o = plain
    corpus, offs = mixed_batch
    w_st, w_out, w_oo, w_hits = _want(o, corpus, offs, 4, 4)
    R, nb0 = w_st.size, w_out.size
    assert R > 3 and nb0 > 30
    ct, ot = _tensors(corpus, offs)
    for cap, cap_bytes in ((R - 1, nb0), (R, nb0 - 1), (R - 1, nb0 - 1), (0, 0)):
        st, oo, out, nk, nb, nh, rc = _device(m, ct, ot, cap, cap_bytes, 4, 4)  # (asserts that every guard is intact)
        assert rc == N.AHA_E_CAPACITY and (nk, nb) == (R, nb0)
    st, oo, out, nk, nb, nh, rc = _device(m, ct, ot, R, nb0, 4, 4)  # exactly enough
    assert rc == N.AHA_OK and (nk, nb, nh) == (R, nb0, w_hits) and out.tobytes() == w_out.tobytes()
    # a buffer that is not given cannot fail the call
    assert _device(m, ct, ot, R, 0, 4, 4, text=False)[6] == N.AHA_OK
    assert _device(m, ct, ot, 0, nb0, 4, 4, ids=False)[6] == N.AHA_OK


# ---- small grids -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("knob", ["AHA_GREP_BLOCKS", "AHA_POST_BLOCKS"])
def test_one_block_grids(monkeypatch, knob):
    """one workgroup of 256 lanes loops: more runs than lanes, more mask words than it covers in one trip (256), more rank blocks
    than its four waves; the excerpts of the later trips are there"""
    monkeypatch.setenv(knob, "1")
    keys = [b"KEY", b"ab"]
    m, o = AC.compile(keys), orc.AC.compile(keys)
    docs = []
    rng = random.Random(3)
    for d in range(1000):
        docs.append(b"x" * rng.randint(0, 9) + b"KEY" + b"y" * rng.randint(6, 30) if d % 2 else b"q" * rng.randint(0, 12))
    corpus, offs = _batch(docs)
    n_words = (corpus.size + 31) // 32
    assert n_words > 256 and (n_words + 63) // 64 > 4
    for pair in ((0, 0), (2, 3), (20, 20)):
        st, out, oo, nh = _check(m, o, corpus, offs, *pair, host=False)
        assert nh == 500 and st.size > 256  # more runs and excerpts than lanes
        late = st >= np.uint64(256 * 32)  # excerpts from mask words of later trips
        assert late.sum() > 100 and (np.diff(oo.astype(np.int64))[late] > 0).all()


# ---- one handle through a sequence ------------------------------------------------------------------------------------------
def test_one_handle_through_a_sequence_of_calls_that_share_scratch(mixed_batch):
    import torch

    keys = [b"KEY", b"ab"]
    m, o = AC.compile(keys), orc.AC.compile(keys)
    corpus, offs = mixed_batch
    ct, ot = _tensors(corpus, offs)
    D = len(offs) - 1
    per, n_hits = oracle_hits_per_doc(o, corpus, offs)
    has = np.array([len(p) > 0 for p in per])

    def grep():
        kept = torch.zeros(D, dtype=torch.int64, device=DEV)
        nk, nb, nh = m.grep_batch_device(ct, ot, kept, None, None)
        assert nh == n_hits and np.array_equal(kept.cpu().numpy()[:nk], np.nonzero(has)[0])

    def rule_grep():
        table = m.classes([[0], [1]], n_classes=2)
        kept = torch.zeros(D, dtype=torch.int64, device=DEV)
        nk, nb, nh = m.grep_batch_device(ct, ot, kept, None, None, rule=[[(0, ">=", 1)]], classes=table)
        want = np.array([any(corpus[int(offs[d]) + s:int(offs[d]) + e].tobytes() == b"KEY" for s, e in per[d]) for d in range(D)])
        assert nh == n_hits and np.array_equal(kept.cpu().numpy()[:nk], np.nonzero(want)[0])

    def cover():
        n_cov, nh = m.cover_batch_device(ct, ot)
        assert nh == n_hits and n_cov == int(excerptsim.cover_bits(per, offs).sum())

    grep()
    _check(m, o, corpus, offs, 3, 3, host=False)
    rule_grep()
    cover()
    _check(m, o, corpus, offs, 40, 0, host=False)
    m.release_scratch()
    _check(m, o, corpus, offs, 3, 3)
    grep()
