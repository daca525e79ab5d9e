"""Select calls (aha_ac_select_batch, aha_ac_select_batch_device) against selectsim over the CPU ORACLE's hits (never the
library's own match): every engine variant on documents whose starts and run ends fall on, before and behind mask-word
boundaries, one long run, the chain case, a separator filter, a folded handle, NUL bytes, capacity, document ranges, neutrality
towards the handle's back-off state, determinism and the host entry.  Every case is a few KiB of text."""
import random
import zlib

import numpy as np
import pytest

import pyoracle as orc
import selectsim
from aha_amd import AC, AhaError, BitArray, DeviceCorpus, Hit
from aha_amd import _native as N
from engine_variants import VARIANTS, use_variant
from test_gpu_doc_counts import KEYSETS, SEP_BITS, _batch, _sep

pytestmark = pytest.mark.gpu

GUARD = 0x5A5A5A5A
PAD = 16
DEV = "cuda:0"
SIZES = [0, 1, 31, 32, 33, 63, 64, 65, 300]


def _oracle_hits(o, corpus, offs, sep=None):
    """(hits HIT_DTYPE, doc hit offsets) of the oracle's match of the batch, document by document; sep = (size, set bits)"""
    parts, dho = [], [0]
    for d in range(offs.size - 1):
        h = o.match(corpus[int(offs[d]):int(offs[d + 1])].tobytes(), chars=False, sep=sep)
        a = np.zeros(h.size, dtype=selectsim.HIT_DTYPE)
        if h.size:
            a["start"], a["end"], a["value"] = h["start"], h["end"], h["value"]
        parts.append(a)
        dho.append(dho[-1] + h.size)
    return (np.concatenate(parts) if parts else np.zeros(0, selectsim.HIT_DTYPE)), np.array(dho, dtype=np.uint64)


def _want(o, corpus, offs, sep=None):
    """selectsim over the oracle's hits -> (selection, doc_sel_offsets, all hits, their offsets)"""
    hits, dho = _oracle_hits(o, corpus, offs, sep)
    sel, dso = selectsim.select(hits, dho)
    return sel, dso, hits, dho


def _tensors(corpus, offs):
    import torch

    ct = torch.from_numpy(corpus).to(DEV) if corpus.size else torch.zeros(0, dtype=torch.uint8, device=DEV)
    return ct, torch.from_numpy(offs.view(np.int64)).to(DEV)


def _device(m, ct, ot, D, cap, sep=None):
    """the device entry with guard words behind cap hits and behind the D + 1 offsets -> (raw out, raw dso, n, n_hits, rc)"""
    import torch

    out = torch.full((cap + PAD, 3), GUARD, dtype=torch.int32, device=ct.device)
    dso = torch.full((D + 1 + PAD,), GUARD, dtype=torch.int64, device=ct.device)
    rc, nh = N.AHA_OK, None
    try:
        n, nh = m.select_batch_device(ct, ot, out, dso, sep=sep, cap=cap)
    except AhaError as e:
        if e.code != N.AHA_E_CAPACITY:
            raise
        rc, n = e.code, e.n_required
    torch.cuda.synchronize()
    out_h, dso_h = out.cpu().numpy(), dso.cpu().numpy()
    assert (out_h[cap:] == GUARD).all(), "the call wrote behind cap hits"
    assert (dso_h[D + 1:] == GUARD).all(), "the call wrote behind the D + 1 offsets"
    return out_h[:cap], dso_h[:D + 1], n, nh, rc


def _as_hits(rows, n):
    return np.ascontiguousarray(rows[:n]).view(selectsim.HIT_DTYPE).reshape(-1)


def _check_all_entries(m, o, corpus, offs, sep_pair=None, sep=None):
    """device entry and host entry: the same bytes, those of selectsim over the oracle's hits, and its invariants"""
    want, want_dso, hits, dho = _want(o, corpus, offs, sep_pair)
    D = offs.size - 1
    ct, ot = _tensors(corpus, offs)
    rows, dso, n, nh, rc = _device(m, ct, ot, D, want.size + 3, sep=sep)
    got = _as_hits(rows, n)
    assert rc == N.AHA_OK and n == want.size and nh == hits.size
    selectsim.check_invariants(got, dso.astype(np.uint64), hits, dho)
    assert np.array_equal(dso.astype(np.uint64), want_dso) and got.tobytes() == want.tobytes()
    assert (rows[n:] == GUARD).all(), "the call wrote behind the selection"
    rows2, dso2, n2, _, _ = _device(m, ct, ot, D, want.size + 3, sep=sep)  # two calls: identical bytes
    assert rows2.tobytes() == rows.tobytes() and dso2.tobytes() == dso.tobytes() and n2 == n
    h_sel, h_dso = m.select_batch(corpus, offs, sep=sep)  # the host entry
    assert h_sel.tobytes() == want.tobytes() and np.array_equal(h_dso, want_dso)
    return want, want_dso, hits, dho


def _ragged_docs(rng, keys, density=0.6):
    """documents of the SIZES (each twice, shuffled) cut anywhere, empty ones first, in the middle and last"""
    pieces = [k for k in keys if len(k) < 64]
    fill = [b" ", b"q", b"\x00", b"zz", "中".encode(), b"a", b"x"]
    sizes = SIZES[1:] * 2
    rng.shuffle(sizes)
    docs = []
    for n in sizes:
        out = bytearray()
        while len(out) < n:
            out += rng.choice(pieces) if rng.random() < density else rng.choice(fill)
        docs.append(bytes(out[:n]))
    mid = len(docs) // 2
    return [b""] + docs[:mid] + [b"", b""] + docs[mid:] + [b""]


@pytest.fixture(params=VARIANTS)
def variant(request, monkeypatch):
    return use_variant(request.param, monkeypatch)


@pytest.mark.parametrize("keyset", ["ascii", "utf8", "nested"])
def test_select_parity_every_engine_variant(variant, keyset):
    rng = random.Random(zlib.crc32(f"sel/{keyset}".encode()))
    keys = KEYSETS[keyset](rng)
    m, o = AC.compile(keys), orc.AC.compile(keys)
    docs = _ragged_docs(rng, keys)
    assert sorted({len(d) for d in docs}) == SIZES and docs[0] == docs[-1] == b""
    corpus, offs = _batch(docs)
    want, _, hits, _ = _check_all_entries(m, o, corpus, offs)
    assert 0 < want.size <= hits.size


def test_select_one_long_run():
    """one document that is one run, longer than any workgroup's share of the positions; twice in a batch: split at the start"""
    keys = [b"a", b"aa", b"aaa"]
    m, o = AC.compile(keys), orc.AC.compile(keys)
    doc = b"a" * 20000
    corpus, offs = _batch([doc])
    want, _, _, _ = _check_all_entries(m, o, corpus, offs)
    assert want.size == 6667 and want[-1].tolist() == (19998, 20000, 1)
    corpus, offs = _batch([doc, doc])
    want, want_dso, _, _ = _check_all_entries(m, o, corpus, offs)
    assert want_dso.tolist() == [0, 6667, 13334] and want[6667].tolist() == (0, 3, 2)


def test_select_chain_hit_is_not_the_first_at_its_end():
    m, o = AC.compile(["ab", "bcd", "cd", "d"]), orc.AC.compile(["ab", "bcd", "cd", "d"])
    assert m.select(b"abcd") == [Hit(0, 2, 0), Hit(2, 4, 2)]
    corpus, offs = _batch([b"abcd", b"", b"xabcdd", b"bcdabcd"])
    want, _, _, _ = _check_all_entries(m, o, corpus, offs)
    assert want.tolist()[:2] == [(0, 2, 0), (2, 4, 2)]
    # the str form: character offsets by a running count of lead bytes; replace on top of it
    m2 = AC.compile(["我", "我是", "是中", "国"])
    assert m2.select("我是中国人") == [Hit(0, 2, 1), Hit(3, 4, 3)]
    assert m2.replace("我是中国人", {1: "I am ", 3: "CN"}) == "I am 中CN人"
    assert m2.replace("我是中国人".encode(), ["a", "b", "c", "d"]) == "b中d人".encode()


def test_select_with_a_separator_filter():
    rng = random.Random(77)
    keys = KEYSETS["ascii"](rng)
    m, o = AC.compile(keys), orc.AC.compile(keys)
    corpus, offs = _batch(_ragged_docs(rng, keys, 0.5))
    bits = [i for i in range(40) if i not in SEP_BITS]
    want, _, hits, _ = _check_all_entries(m, o, corpus, offs, (40, bits), _sep())
    plain, _, all_hits, _ = _want(o, corpus, offs)
    assert 0 < hits.size < all_hits.size and want.tobytes() != plain.tobytes()


def test_select_on_a_folded_handle():
    rng = random.Random(5)
    words = sorted({"".join(rng.choice("abcdEFGH") for _ in range(rng.randint(2, 6))) for _ in range(200)}, key=str.lower)
    keys = [w.encode() for w in {w.lower(): w for w in words}.values()]  # distinct after folding
    m = AC.compile(keys, fold_ascii=True)
    folded = [k.lower() for k in keys]
    o = orc.AC.compile(folded)
    docs = _ragged_docs(rng, [k.swapcase() for k in keys] + keys)
    corpus, offs = _batch(docs)
    low = np.frombuffer(corpus.tobytes().lower(), dtype=np.uint8).copy()
    want, want_dso, hits, dho = _want(o, low, offs)
    assert want.size > 0
    ct, ot = _tensors(corpus, offs)
    rows, dso, n, nh, rc = _device(m, ct, ot, offs.size - 1, want.size)
    assert rc == N.AHA_OK and nh == hits.size
    assert _as_hits(rows, n).tobytes() == want.tobytes() and np.array_equal(dso.astype(np.uint64), want_dso)
    plain = AC.compile(folded)  # a plain handle over folded keys and text: the same bytes
    p_sel, p_dso = plain.select_batch(low, offs)
    assert p_sel.tobytes() == want.tobytes() and np.array_equal(p_dso, want_dso)


def test_select_text_with_nul_bytes():
    keys = [b"ab", b"abc", b"bc", b"c\x01"]
    m, o = AC.compile(keys), orc.AC.compile(keys)
    corpus, offs = _batch([b"\x00abc\x00\x00abc\x01\x00", b"\x00" * 40, b"ab\x00c\x01abc", b"\x00"])
    want, _, _, _ = _check_all_entries(m, o, corpus, offs)
    assert want.size >= 4


def test_select_capacity_writes_nothing():
    import ctypes as C

    rng = random.Random(21)
    keys = KEYSETS["ascii"](rng)
    m, o = AC.compile(keys), orc.AC.compile(keys)
    corpus, offs = _batch(_ragged_docs(rng, keys))
    want, want_dso, hits, _ = _want(o, corpus, offs)
    D = offs.size - 1
    assert want.size > 2
    ct, ot = _tensors(corpus, offs)
    rows, dso, n, _, rc = _device(m, ct, ot, D, want.size - 1)
    assert rc == N.AHA_E_CAPACITY and n == want.size
    assert (rows == GUARD).all() and (dso == GUARD).all(), "a failing call wrote a caller's buffer"
    rows, dso, n, nh, rc = _device(m, ct, ot, D, want.size)
    assert rc == N.AHA_OK and n == want.size and nh == hits.size
    assert _as_hits(rows, n).tobytes() == want.tobytes() and np.array_equal(dso.astype(np.uint64), want_dso)
    with pytest.raises(AhaError) as e:  # the sizing call: out == NULL, cap == 0
        m.select_batch_device(ct, ot, None)
    assert e.value.code == N.AHA_E_CAPACITY and e.value.n_required == want.size
    # the host entry, one short
    L = N.lib()
    n64 = C.c_uint64(0)
    out = np.full((want.size, 3), GUARD, dtype=np.int32)
    dso_h = np.full(D + 1, GUARD, dtype=np.uint64)
    rc = L.aha_ac_select_batch(m._h, corpus.ctypes.data, offs.ctypes.data, D, None, 0, out.ctypes.data, want.size - 1,
                               dso_h.ctypes.data, C.byref(n64), None)
    assert rc == N.AHA_E_CAPACITY and n64.value == want.size and (out == GUARD).all() and (dso_h == GUARD).all()
    # no hits: cap = 0 succeeds, the offsets are written
    corpus0, offs0 = _batch([b"", b"----", b""])
    ct0, ot0 = _tensors(corpus0, offs0)
    rows, dso, n, nh, rc = _device(m, ct0, ot0, 3, 0)
    assert rc == N.AHA_OK and n == 0 and nh == 0 and dso.tolist() == [0, 0, 0, 0]
    for offs_e in ([0], [0, 0, 0]):  # D = 0; N = 0
        c_e, o_e = np.zeros(0, dtype=np.uint8), np.array(offs_e, dtype=np.uint64)
        sel, dso = m.select_batch(c_e, o_e)
        assert sel.size == 0 and dso.tolist() == [0] * len(offs_e)
        ct_e, ot_e = _tensors(c_e, o_e)
        assert _device(m, ct_e, ot_e, len(offs_e) - 1, 0)[2:] == (0, 0, N.AHA_OK)


def test_select_in_document_ranges(monkeypatch):
    """the hit buffer's bound lowered: three or more ranges of whole documents, one document alone beyond the bound"""
    rng = random.Random(9)
    keys = KEYSETS["ascii"](rng)
    o = orc.AC.compile(keys)
    docs = _ragged_docs(rng, keys) + _ragged_docs(rng, keys) + _ragged_docs(rng, keys)
    docs[7] = b"".join(rng.choice(keys) for _ in range(700))
    corpus, offs = _batch(docs)
    want, want_dso, hits, dho = _want(o, corpus, offs)
    h = np.diff(dho.astype(np.int64))
    BOUND = 100
    assert h[7] > BOUND and h.sum() - h[7] > 3 * BOUND and h[-1] == 0 and h[0] == 0  # (from the oracle)
    single = AC.compile(keys)
    s_sel, s_dso = single.select_batch(corpus, offs)
    monkeypatch.setenv("AHA_SELECT_HIT_BYTES", str(12 * BOUND))
    m = AC.compile(keys)
    m.set_profiling(True)
    _check_all_entries(m, o, corpus, offs)
    ct, ot = _tensors(corpus, offs)
    rows, dso, n, nh, rc = _device(m, ct, ot, offs.size - 1, want.size)
    t = m.last_timing()
    assert t["repeats"] >= 2 and t["n_hits"] == hits.size, t
    assert _as_hits(rows, n).tobytes() == want.tobytes() == s_sel.tobytes() and np.array_equal(s_dso, want_dso)
    rows, dso, n, _, rc = _device(m, ct, ot, offs.size - 1, want.size - 1)  # capacity across ranges: nothing written
    assert rc == N.AHA_E_CAPACITY and n == want.size and (rows == GUARD).all() and (dso == GUARD).all()
    sel_c, dso_c, nh_c = m.select_corpus(DeviceCorpus(corpus, offs))
    assert sel_c.tobytes() == want.tobytes() and np.array_equal(dso_c, want_dso) and nh_c == hits.size


def test_select_leaves_no_trace_in_the_back_off(monkeypatch):
    """match -> select -> match on a handle whose first match is handed back by the prefix-filter engine: every later match
    gives the hits, the engine and the repeats of a twin handle that never saw the call in between."""
    monkeypatch.delenv("AHA_ENGINE", raising=False)
    dense = b"abcd" * 3000
    sparse = b"-" * 5000 + b"abcd"

    def run(with_select):
        m = AC.compile(["abc", "bcd"])
        assert m.info["filter_prefix_bytes"] == 3
        m.set_profiling(True)
        seen = []
        for text in [dense] + [sparse] * 6 + [dense] + [sparse] * 3:
            hits = m.match_array(text)
            t = m.last_timing()
            seen.append((t["engine"], t["repeats"], hits.tobytes()))
            if with_select:
                for t2 in (dense, sparse):
                    sel = m.select_array(t2)
                    assert sel.size == (3000 if t2 is dense else 1) and set(sel["value"].tolist()) == {0}
        m.release_scratch()
        assert m.scratch_bytes() == 0
        return seen

    plain = run(False)
    assert plain[0][0] == 2 and plain[1][0] == 2 and plain[6][0] == 5, [p[:2] for p in plain]
    assert run(True) == plain
