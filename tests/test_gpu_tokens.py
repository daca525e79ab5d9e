"""Token calls (aha_ac_select_batch* with AHA_SELECT_TOKENS, with and without AHA_SELECT_GAP_RUNS) against tokensim over
selectsim over the CPU ORACLE's hits (never the library's own match or select): device and host entry bit for bit, with guard
words behind cap tokens and behind the D + 1 offsets.  Every case is a few KiB of text: ragged documents on every engine
variant, characters and hits on mask-word and rank-block borders, documents and keys that cut characters, degenerate runs and
batches, small grids, document ranges, capacity, filters and folded handles, neutrality, the Python wrappers."""
import ctypes as C
import random
import zlib

import numpy as np
import pytest

import foldsim
import pyoracle as orc
import selectsim
import tokensim
from aha_amd import AC, AhaError, DeviceCorpus, Hit
from aha_amd import _native as N
from engine_variants import VARIANTS, use_variant
from test_gpu_doc_counts import KEYSETS, SEP_BITS, _batch, _sep
from test_gpu_fold_simple import on_device
from test_gpu_select import GUARD, PAD, SIZES, _as_hits, _ragged_docs, _tensors, _want

pytestmark = pytest.mark.gpu

MODES = (False, True)  # gap_runs


def _want_tokens(o, corpus, offs, gap_runs, sep_pair=None, seen=None):
    """tokensim over selectsim over the oracle's hits of `seen` (the text as the handle matches it; default: the corpus),
    cut out of the caller's bytes -> (tokens, doc_tok_offsets, selection, doc_sel_offsets, n_hits)"""
    sel, dso, hits, _ = _want(o, corpus if seen is None else seen, offs, sep_pair)
    toks, dto = tokensim.tokens(corpus, offs, sel, dso, gap_runs)
    tokensim.check_invariants(toks, dto, corpus, offs, sel, dso, gap_runs)
    return toks, dto, sel, dso, hits.size


def _device(m, ct, ot, D, cap, gap_runs, sep=None):
    """the device entry with guard words behind cap tokens and behind the D + 1 offsets -> (raw out, raw dto, n, n_hits, rc)"""
    import torch

    out = torch.full((cap + PAD, 3), GUARD, dtype=torch.int32, device=ct.device)
    dto = torch.full((D + 1 + PAD,), GUARD, dtype=torch.int64, device=ct.device)
    rc, nh = N.AHA_OK, None
    try:
        n, nh = m.tokens_batch_device(ct, ot, out, dto, sep=sep, gap_runs=gap_runs, cap=cap)
    except AhaError as e:
        if e.code != N.AHA_E_CAPACITY:
            raise
        rc, n = e.code, e.n_required
    torch.cuda.synchronize()
    out_h, dto_h = out.cpu().numpy(), dto.cpu().numpy()
    assert (out_h[cap:] == GUARD).all(), "the call wrote behind cap tokens"
    assert (dto_h[D + 1:] == GUARD).all(), "the call wrote behind the D + 1 offsets"
    return out_h[:cap], dto_h[:D + 1], n, nh, rc


def _check_all_entries(m, o, corpus, offs, sep_pair=None, sep=None, seen=None):
    """both gap modes, device entry and host entry: the same bytes, those of the twin -> the character-mode tokens"""
    D = offs.size - 1
    ct, ot = _tensors(corpus, offs)
    first = None
    for gap_runs in MODES:
        want, want_dto, sel, _, n_hits = _want_tokens(o, corpus, offs, gap_runs, sep_pair, seen)
        rows, dto, n, nh, rc = _device(m, ct, ot, D, want.size + 3, gap_runs, sep=sep)
        got = _as_hits(rows, n)
        assert rc == N.AHA_OK and n == want.size and nh == n_hits, (gap_runs, n, want.size, nh, n_hits)
        assert np.array_equal(dto.astype(np.uint64), want_dto), gap_runs
        assert got.tobytes() == want.tobytes(), (gap_runs, [x for x in zip(got.tolist(), want.tolist()) if x[0] != x[1]][:5])
        assert (rows[n:] == GUARD).all(), "the call wrote behind the tokens"
        rows2, dto2, n2, _, _ = _device(m, ct, ot, D, want.size + 3, gap_runs, sep=sep)  # two calls: identical bytes
        assert rows2.tobytes() == rows.tobytes() and dto2.tobytes() == dto.tobytes() and n2 == n
        h_tok, h_dto = m.tokens_batch(corpus, offs, sep=sep, gap_runs=gap_runs)  # the host entry
        assert h_tok.tobytes() == want.tobytes() and np.array_equal(h_dto, want_dto), gap_runs
        first = want if first is None else first
    return first


@pytest.fixture(params=VARIANTS)
def variant(request, monkeypatch):
    return use_variant(request.param, monkeypatch)


# ---- ragged documents ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("keyset", ["ascii", "utf8", "nested"])
def test_tokens_parity_every_engine_variant(variant, keyset):
    rng = random.Random(zlib.crc32(f"tok/{keyset}".encode()))
    keys = KEYSETS[keyset](rng)
    m, o = AC.compile(keys), orc.AC.compile(keys)
    docs = _ragged_docs(rng, keys)
    assert sorted({len(d) for d in docs}) == SIZES and docs[0] == docs[-1] == b""
    corpus, offs = _batch(docs)
    want = _check_all_entries(m, o, corpus, offs)
    assert (want["value"] >= 0).any() and (want["value"] < 0).any()


def test_tokens_at_every_alignment_of_the_text():
    """the text as a slice of a larger tensor at every address modulo 16; the bytes around it would change the tokens at its
    ends if a kernel looked at them"""
    rng = random.Random(16)
    keys = KEYSETS["utf8"](rng)
    m, o = AC.compile(keys), orc.AC.compile(keys)
    docs = [d for d in _ragged_docs(rng, keys) if len(d) in (0, 1, 33, 65, 300)]
    docs[1] = b"\x80" + docs[1]  # the batch starts and ends inside a character
    docs[-2] = docs[-2] + "中".encode()[:1]
    corpus, offs = _batch(docs)
    _, ot = _tensors(corpus, offs)
    for gap_runs in MODES:
        want, want_dto, _, _, _ = _want_tokens(o, corpus, offs, gap_runs)
        for align in range(16):
            rows, dto, n, _, rc = _device(m, on_device(corpus, align), ot, offs.size - 1, want.size, gap_runs)
            assert rc == N.AHA_OK and _as_hits(rows, n).tobytes() == want.tobytes(), (gap_runs, align)
            assert np.array_equal(dto.astype(np.uint64), want_dto)


# ---- characters and hits over word and rank-block borders --------------------------------------------------------------------
@pytest.mark.parametrize("border", [32, 2048])
def test_tokens_character_over_a_border(border):
    """a three-byte character whose lead is the last byte of a mask word (of a rank block) and whose continuation bytes are in
    the next: no token starts there"""
    keys = [b"key"]
    m, o = AC.compile(keys), orc.AC.compile(keys)
    doc = b"x" * (border - 1) + "中".encode() + b"y" * 40
    corpus, offs = _batch([doc])
    want = _check_all_entries(m, o, corpus, offs)
    starts = set(want["start"].tolist())
    assert border - 1 in starts and border not in starts and border + 1 not in starts and border + 2 in starts
    assert want.size == len(doc) - 2


@pytest.mark.parametrize("border", [32, 2048])
def test_tokens_hit_that_ends_on_a_border(border):
    """a selected hit that ends exactly on the border, followed by a gap (a continuation byte: only "p - 1 is inside" starts the
    token) -- and followed at once by another hit"""
    keys = [b"abc", b"de"]
    m, o = AC.compile(keys), orc.AC.compile(keys)
    gap = b"x" * (border - 3) + b"abc" + b"\x80\x80z" + b"x" * 30
    hit = b"x" * (border - 3) + b"abc" + b"de" + b"\x80x" * 15
    want = _check_all_entries(m, o, *_batch([gap])).tolist()  # (each alone in its batch: the border is the masks' own)
    assert want[border - 3] == (border - 3, border, 0) and want[border - 2] == (border, border + 2, -1)
    want = _check_all_entries(m, o, *_batch([hit, gap])).tolist()
    assert want[border - 3: border] == [(border - 3, border, 0), (border, border + 2, 1), (border + 2, border + 3, -1)]


# ---- documents and hits that cut characters ----------------------------------------------------------------------------------
def test_tokens_documents_and_keys_that_cut_characters():
    zhong = "中".encode()
    keys = [zhong[1:] + b"a", b"ab", zhong]  # a byte-level key that starts on a continuation byte
    m, o = AC.compile(keys), orc.AC.compile(keys)
    docs = [zhong[1:] + b"xy", zhong[:2], zhong + b"a" + zhong, b"q" + zhong[:1], zhong[2:]]
    corpus, offs = _batch(docs)
    want = _check_all_entries(m, o, corpus, offs)
    dto = tokensim.tokens(corpus, offs, *_want(o, corpus, offs)[:2])[1].tolist()
    assert want[dto[0]:dto[1]].tolist() == [(0, 2, -1), (2, 3, -1), (3, 4, -1)]  # the document starts on a continuation byte
    # 中 a 中: the longest hit at 0 is 中 itself; then "a", then 中
    assert want[dto[2]:dto[3]].tolist() == [(0, 3, 2), (3, 4, -1), (4, 7, 2)]
    m2, o2 = AC.compile(keys[:2]), orc.AC.compile(keys[:2])  # without the key 中 the byte-level key cuts the character
    want2 = _check_all_entries(m2, o2, corpus, offs)
    assert want2[dto[2]:dto[2] + 3].tolist() == [(0, 1, -1), (1, 4, 0), (4, 7, -1)]


# ---- degenerate runs and batches ----------------------------------------------------------------------------------------------
def test_tokens_degenerate_runs():
    keys = [b"a", b"aa", b"aaa"]
    m, o = AC.compile(keys), orc.AC.compile(keys)
    stray = b"q" + b"\x80" * 100 + b"r"
    corpus, offs = _batch([stray, b"aaa", b"a" * 5000, b"\x80" * 100])
    want = _check_all_entries(m, o, corpus, offs)
    assert want[:3].tolist() == [(0, 101, -1), (101, 102, -1), (0, 3, 2)]  # the stray run is one token; a document that is one hit
    assert want[3:-1]["value"].tolist() == [2] * 1666 + [1] and want[-1].tolist() == (0, 100, -1)


def test_tokens_batches_without_a_hit_and_without_a_byte():
    keys = [b"needle"]
    m, o = AC.compile(keys), orc.AC.compile(keys)
    corpus, offs = _batch([b"", "我是中国人".encode(), b"", b"hay " * 20, b""])  # no hit: still tokenized
    want = _check_all_entries(m, o, corpus, offs)
    assert want.size == 5 + 80 and (want["value"] == -1).all()
    assert m.tokens_batch(corpus, offs, gap_runs=True)[0].tolist() == [(0, 15, -1), (0, 80, -1)]
    for offs_e in ([0], [0, 0, 0, 0]):  # D = 0; only empty documents (N = 0)
        c_e, o_e = np.zeros(0, dtype=np.uint8), np.array(offs_e, dtype=np.uint64)
        ct_e, ot_e = _tensors(c_e, o_e)
        for gap_runs in MODES:
            toks, dto = m.tokens_batch(c_e, o_e, gap_runs=gap_runs)
            assert toks.size == 0 and dto.tolist() == [0] * len(offs_e)
            rows, dto_d, n, nh, rc = _device(m, ct_e, ot_e, len(offs_e) - 1, 0, gap_runs)
            assert (n, nh, rc) == (0, 0, N.AHA_OK) and dto_d.tolist() == [0] * len(offs_e)


# ---- small grids ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("blocks", [1, 2])
def test_tokens_on_small_grids(monkeypatch, blocks):
    """AHA_POST_BLOCKS = 1 and 2 over a 5000-byte document and a 12000-byte one: every lane strides over the mask words, and
    the batch has more rank blocks (2048 positions each) than the grid has waves (4 per workgroup), so a wave owns several"""
    monkeypatch.setenv("AHA_POST_BLOCKS", str(blocks))
    rng = random.Random(blocks)
    keys = KEYSETS["utf8"](rng)
    m, o = AC.compile(keys), orc.AC.compile(keys)
    docs = [d for d in _ragged_docs(rng, keys) if len(d) != 300]
    fill = [b" ", "中".encode(), b"\x80", b"x"]
    for at, size in ((3, 5000), (9, 12000)):
        out = bytearray()
        while len(out) < size:
            out += rng.choice(keys) if rng.random() < 0.5 else rng.choice(fill)
        docs.insert(at, bytes(out[:size]))
    corpus, offs = _batch(docs)
    assert corpus.size > 2 * 4 * 2048 and corpus.size / 32 > 2 * 256
    want = _check_all_entries(m, o, corpus, offs)
    assert (want["value"] >= 0).any() and (want["value"] < 0).any()


# ---- document ranges --------------------------------------------------------------------------------------------------------------
def test_tokens_in_document_ranges(monkeypatch):
    """the bound of a range lowered: several ranges of whole documents, cut by their hits and by their text, with documents
    without a hit before, between and behind them; the single-range result, bit for bit"""
    rng = random.Random(9)
    keys = KEYSETS["ascii"](rng)
    o = orc.AC.compile(keys)
    quiet = [b"-" * 40, "无".encode() * 30, b"", b"=" * 700]
    docs = quiet + _ragged_docs(rng, keys) + quiet + _ragged_docs(rng, keys) + quiet
    docs[9] = b"".join(rng.choice(keys) for _ in range(300))
    corpus, offs = _batch(docs)
    BOUND = 100
    single = AC.compile(keys)
    monkeypatch.setenv("AHA_SELECT_HIT_BYTES", str(12 * BOUND))
    m = AC.compile(keys)
    m.set_profiling(True)
    _check_all_entries(m, o, corpus, offs)
    ct, ot = _tensors(corpus, offs)
    for gap_runs in MODES:
        want, want_dto, _, _, n_hits = _want_tokens(o, corpus, offs, gap_runs)
        s_tok, s_dto = single.tokens_batch(corpus, offs, gap_runs=gap_runs)
        rows, dto, n, nh, rc = _device(m, ct, ot, offs.size - 1, want.size, gap_runs)
        t = m.last_timing()
        assert t["repeats"] > 0 and t["n_hits"] == n_hits == nh and n_hits > 3 * BOUND, t
        assert _as_hits(rows, n).tobytes() == want.tobytes() == s_tok.tobytes() and np.array_equal(s_dto, want_dto)
        rows, dto, n, _, rc = _device(m, ct, ot, offs.size - 1, want.size - 1, gap_runs)  # capacity across ranges
        assert rc == N.AHA_E_CAPACITY and n == want.size and (rows == GUARD).all() and (dto == GUARD).all()
        tok_c, dto_c, nh_c = m.tokens_corpus(DeviceCorpus(corpus, offs), gap_runs=gap_runs)
        assert tok_c.tobytes() == want.tobytes() and np.array_equal(dto_c, want_dto) and nh_c == n_hits
    # no hit at all: the ranges are cut by the text alone
    m2, o2 = AC.compile([b"needle"]), orc.AC.compile([b"needle"])
    m2.set_profiling(True)
    _check_all_entries(m2, o2, corpus, offs)
    assert m2.last_timing()["repeats"] > 0


# ---- capacity -----------------------------------------------------------------------------------------------------------------------
def test_tokens_capacity_writes_nothing():
    rng = random.Random(21)
    keys = KEYSETS["ascii"](rng)
    m, o = AC.compile(keys), orc.AC.compile(keys)
    corpus, offs = _batch(_ragged_docs(rng, keys))
    D = offs.size - 1
    ct, ot = _tensors(corpus, offs)
    for gap_runs in MODES:
        want, want_dto, sel, _, n_hits = _want_tokens(o, corpus, offs, gap_runs)
        assert want.size > sel.size > 2
        rows, dto, n, _, rc = _device(m, ct, ot, D, want.size - 1, gap_runs)
        assert rc == N.AHA_E_CAPACITY and n == want.size
        assert (rows == GUARD).all() and (dto == GUARD).all(), "a failing call wrote a caller's buffer"
        rows, dto, n, nh, rc = _device(m, ct, ot, D, want.size, gap_runs)  # cap == total
        assert rc == N.AHA_OK and n == want.size and nh == n_hits
        assert _as_hits(rows, n).tobytes() == want.tobytes() and np.array_equal(dto.astype(np.uint64), want_dto)
        with pytest.raises(AhaError) as e:  # the sizing call: out == NULL, cap == 0
            m.tokens_batch_device(ct, ot, None, gap_runs=gap_runs)
        assert e.value.code == N.AHA_E_CAPACITY and e.value.n_required == want.size
        # the host entry, one short
        flags = N.AHA_SELECT_TOKENS | (N.AHA_SELECT_GAP_RUNS if gap_runs else 0)
        n64 = C.c_uint64(0)
        out = np.full((want.size, 3), GUARD, dtype=np.int32)
        dto_h = np.full(D + 1, GUARD, dtype=np.uint64)
        rc = N.lib().aha_ac_select_batch(m._h, corpus.ctypes.data, offs.ctypes.data, D, None, flags, out.ctypes.data, want.size - 1,
                                         dto_h.ctypes.data, C.byref(n64), None)
        assert rc == N.AHA_E_CAPACITY and n64.value == want.size and (out == GUARD).all() and (dto_h == GUARD).all()


# ---- handles and filters --------------------------------------------------------------------------------------------------------
def test_tokens_with_a_separator_filter():
    rng = random.Random(77)
    keys = KEYSETS["ascii"](rng)
    m, o = AC.compile(keys), orc.AC.compile(keys)
    corpus, offs = _batch(_ragged_docs(rng, keys, 0.5))
    bits = [i for i in range(40) if i not in SEP_BITS]
    want = _check_all_entries(m, o, corpus, offs, (40, bits), _sep())
    plain = _want_tokens(o, corpus, offs, False)[0]
    assert want.tobytes() != plain.tobytes() and (want["value"] >= 0).any()


def test_tokens_on_folded_handles():
    """the selection is the folded handle's; the tokens are cut from the caller's bytes and the offsets are the original's"""
    rng = random.Random(5)
    words = sorted({"".join(rng.choice("abcdEFGH") for _ in range(rng.randint(2, 6))) for _ in range(200)}, key=str.lower)
    keys = [w.encode() for w in {w.lower(): w for w in words}.values()]  # distinct after folding
    m = AC.compile(keys, fold_ascii=True)
    o = orc.AC.compile([k.lower() for k in keys])
    corpus, offs = _batch(_ragged_docs(rng, [k.swapcase() for k in keys] + keys))
    low = np.frombuffer(corpus.tobytes().lower(), dtype=np.uint8).copy()
    want = _check_all_entries(m, o, corpus, offs, seen=low)
    assert (want["value"] >= 0).any() and _want_tokens(o, corpus, offs, False)[0].tobytes() != want.tobytes()
    # two-byte characters: Привет matches привет; the gaps hold upper-case two-byte characters, one token each
    keys2 = ["Привет".encode(), "Мир".encode(), b"ok"]
    m2 = AC.compile(keys2, fold_simple=True)
    o2 = orc.AC.compile(foldsim.fold2_keys(keys2))
    docs = ["ПРИВЕТ, мир! Ok ЖЖЖ".encode(), b"", "привет".encode() * 6 + "Я".encode(), "ЖМИР".encode()[1:]]
    corpus2, offs2 = _batch(docs)
    seen = np.frombuffer(bytes(foldsim.fold2_docs(corpus2, offs2)), dtype=np.uint8).copy()
    want2 = _check_all_entries(m2, o2, corpus2, offs2, seen=seen)
    assert want2[0].tolist() == (0, 12, 0) and (want2["value"] == 1).sum() == 2


def test_tokens_text_with_nul_bytes():
    keys = [b"ab", b"abc", b"bc", b"c\x01"]
    m, o = AC.compile(keys), orc.AC.compile(keys)
    corpus, offs = _batch([b"\x00abc\x00\x00abc\x01\x00", b"\x00" * 40, b"ab\x00c\x01abc", b"\x00"])
    want = _check_all_entries(m, o, corpus, offs)
    assert (want["value"] >= 0).sum() >= 4 and want.size > 45


# ---- neutrality -------------------------------------------------------------------------------------------------------------------
def test_tokens_leave_select_and_the_back_off_as_they_were(monkeypatch):
    """select -> tokens -> select on one handle gives the same bytes (the scratch slots do not clash); match -> tokens -> match
    on a handle whose first match is handed back by the prefix-filter engine: every later match gives the hits, the engine and
    the repeats of a twin handle that never saw the call in between."""
    rng = random.Random(3)
    keys = KEYSETS["nested"](rng)
    m = AC.compile(keys)
    corpus, offs = _batch(_ragged_docs(rng, keys))
    before = m.select_batch(corpus, offs)
    for gap_runs in MODES:
        toks, _ = m.tokens_batch(corpus, offs, gap_runs=gap_runs)
        assert toks.size > before[0].size
        after = m.select_batch(corpus, offs)
        assert after[0].tobytes() == before[0].tobytes() and after[1].tobytes() == before[1].tobytes()
    monkeypatch.delenv("AHA_ENGINE", raising=False)
    dense = b"abcd" * 3000
    sparse = b"-" * 5000 + b"abcd"

    def run(with_tokens):
        h = AC.compile(["abc", "bcd"])
        assert h.info["filter_prefix_bytes"] == 3
        h.set_profiling(True)
        seen = []
        for text in [dense] + [sparse] * 6 + [dense] + [sparse] * 3:
            hits = h.match_array(text)
            t = h.last_timing()
            seen.append((t["engine"], t["repeats"], hits.tobytes()))
            if with_tokens:
                assert len(h.tokens(dense)) == 6000 and len(h.tokens(sparse, gap_runs=True)) == 3
        h.release_scratch()
        assert h.scratch_bytes() == 0
        return seen

    plain = run(False)
    assert plain[0][0] == 2 and plain[1][0] == 2 and plain[6][0] == 5, [p[:2] for p in plain]
    assert run(True) == plain


# ---- the Python wrappers ------------------------------------------------------------------------------------------------------------
def test_tokens_python_wrappers_on_the_readme_example():
    m = AC.compile(["我是", "中国"])
    text = "我是中国人"
    assert m.segment(text) == ["我是", "中国", "人"]
    assert m.tokens(text) == [("我是", 0), ("中国", 1), ("人", -1)]
    assert m.tokens(text.encode()) == [Hit(0, 6, 0), Hit(6, 12, 1), Hit(12, 15, -1)]
    assert m.segment(text.encode()) == [text.encode()[:6], text.encode()[6:12], text.encode()[12:]]
    assert m.segment("我是x中y国z") == ["我是", "x", "中", "y", "国", "z"]
    assert m.segment("我是x中y国z", gap_runs=True) == ["我是", "x中y国z"]
    assert m.segment("") == [] and m.tokens(b"") == []
    corpus, offs = _batch([text.encode(), b"", "中国".encode()])
    toks, dto, n_hits = m.tokens_corpus(DeviceCorpus(corpus, offs))
    assert toks.tolist() == [(0, 6, 0), (6, 12, 1), (12, 15, -1), (0, 6, 1)] and dto.tolist() == [0, 3, 3, 4] and n_hits == 3
