"""Count calls (aha_ac_count_batch, aha_ac_count_batch_device) on every engine variant, against the CPU oracle: hits per key
= np.bincount of the oracle's hit values, per-document offsets and the total = the oracle's.  Beside the plain checks: the
separator filter, char offsets (byte-offset counts), running totals (AHA_COUNT_ACCUMULATE), NULL key counts, sentinels
behind what a call may write, bad device offsets, the engine a count call reports against the match call's, call sequences
on one handle (a count call leaves nothing a later match depends on), two threads on one handle, and cfg 5 at 1 M keys."""
import random
import threading
import zlib

import numpy as np
import pytest

import pyoracle as orc
from aha_amd import AC, AhaError, BitArray, DeviceCorpus, synth
from aha_amd import _native as N
from engine_variants import VARIANTS, use_variant

pytestmark = pytest.mark.gpu

S64 = 0xFFFFFFFFFFFFFFFB  # sentinel behind the K counts and the D + 1 offsets
PAD = 16
SEP_BITS = [32, 0]  # a space and a NUL separate


# ---- key sets and their batches ------------------------------------------------------------------------------------

def _keys_ascii(rng):
    words = sorted({"".join(rng.choice("abcdefgh") for _ in range(rng.randint(3, 9))) for _ in range(600)})
    return [w.encode() for w in words]


def _keys_utf8(rng):
    blob, offs, _ = synth.keys(3, K=3000, seed=7)
    return [bytes(blob[offs[i]:offs[i + 1]]) for i in range(offs.size - 1)]


def _keys_nested(rng):
    # output chains longer than 15 (the general post passes), in bytes and in characters
    return [b"a" * i for i in range(1, 24)] + [("我" * i).encode() for i in range(1, 21)] + [b"ba", b"bab", b"abab"]


def _keys_single(rng):
    return [b"a", b"b", b" ", "是".encode(), b"ab", b"ba", "我是".encode(), b"abc", b"c"]


def _keys_long(rng):
    return [b"x" * 5000, b"xx", b"xy", b"y", b"yx" * 3]


KEYSETS = {"ascii": _keys_ascii, "utf8": _keys_utf8, "nested": _keys_nested, "single": _keys_single, "long": _keys_long}


def _docs(rng, keys, n_docs, size, density):
    pieces = [k for k in keys if len(k) < 64] or [b"x"]
    fill = [b" ", b"q", b"\x00", b"zz", "中".encode(), b"a", b"x"]
    docs = []
    for _ in range(n_docs):
        n = rng.choice([0, size // 4, size, size * 2]) if rng.random() < 0.3 else size
        out = bytearray()
        while len(out) < n:
            out += rng.choice(pieces) if rng.random() < density else rng.choice(fill)
        docs.append(bytes(out[:n]))  # (cut anywhere: keys cross document boundaries, characters may be cut)
    docs[0] = b""
    if n_docs > 2:
        docs[n_docs // 2] = b""
    return docs


def _batch(docs):
    corpus = np.frombuffer(b"".join(docs), dtype=np.uint8).copy()
    offs = np.cumsum([0] + [len(d) for d in docs]).astype(np.uint64)
    return corpus, offs


def _sep():
    sep = BitArray(40)
    for i in range(40):
        sep[i] = i not in SEP_BITS
    return sep


def _oracle(o, corpus, offs, K, sep=False):
    """(key counts, doc offsets, total) of the oracle's match of the batch"""
    if not sep:
        hits, dho = o.match_batch(corpus, offs)
    else:
        parts, dho = [], [0]
        bits = [i for i in range(40) if i not in SEP_BITS]
        for d in range(offs.size - 1):
            h = o.match(corpus[int(offs[d]):int(offs[d + 1])].tobytes(), chars=False, sep=(40, bits))
            parts.append(h["value"] if h.size else np.zeros(0, np.int32))
            dho.append(dho[-1] + h.size)
        hits = {"value": np.concatenate(parts) if parts else np.zeros(0, np.int32)}
        dho = np.array(dho, dtype=np.uint64)
    v = np.asarray(hits["value"], dtype=np.int64)
    return np.bincount(v, minlength=K).astype(np.uint64), np.asarray(dho, dtype=np.uint64), int(v.size)


def _compile(keys):
    return AC.compile(keys), orc.AC.compile(keys)


def _device_count(m, corpus_t, offs_t, D, sep=None, chars=False, per_key=True, accumulate=None):
    import torch

    K = m.n_keys
    kc = None
    if per_key:
        kc = torch.full((K + PAD,), 0, dtype=torch.int64, device=corpus_t.device)
        kc[K:] = torch.tensor(np.array([S64] * PAD, dtype=np.uint64).view(np.int64))
        if accumulate is not None:
            kc[:K] = torch.from_numpy(accumulate.view(np.int64)).to(corpus_t.device)
    dho = torch.tensor(np.array([S64] * (D + 1 + PAD), dtype=np.uint64).view(np.int64), device=corpus_t.device)
    n = m.count_batch_device(corpus_t, offs_t, kc, dho, sep=sep, chars=chars, accumulate=accumulate is not None)
    torch.cuda.synchronize()
    kc_h = kc.cpu().numpy().view(np.uint64) if per_key else None
    dho_h = dho.cpu().numpy().view(np.uint64)
    if per_key:
        assert (kc_h[K:] == S64).all(), "a count call wrote behind the K entries"
    assert (dho_h[D + 1:] == S64).all(), "a count call wrote behind the D + 1 offsets"
    return (kc_h[:K] if per_key else None), dho_h[:D + 1], n


@pytest.fixture(params=VARIANTS)
def variant(request, monkeypatch):
    return use_variant(request.param, monkeypatch)


@pytest.mark.parametrize("keyset", sorted(KEYSETS))
def test_count_matches_oracle(variant, keyset):
    import torch

    rng = random.Random(zlib.crc32(f"{variant}/{keyset}".encode()))  # (stable across processes)
    keys = KEYSETS[keyset](rng)
    m, o = _compile(keys)
    K = m.n_keys
    dev = "cuda:0"
    for n_docs, size, density in ((7, 300, 0.3), (40, 2000, 0.6), (3, 70000, 0.9)):
        docs = _docs(rng, keys, n_docs, size, density)
        corpus, offs = _batch(docs)
        want_kc, want_dho, want_n = _oracle(o, corpus, offs, K)
        # host entry
        kc, dho = m.count_batch(corpus, offs)
        assert np.array_equal(kc, want_kc) and np.array_equal(dho, want_dho)
        # device entry, with and without key counts, byte and char offsets
        ct = torch.from_numpy(corpus).to(dev)
        ot = torch.from_numpy(offs.view(np.int64)).to(dev)
        kc, dho, n = _device_count(m, ct, ot, n_docs)
        assert n == want_n and np.array_equal(kc, want_kc) and np.array_equal(dho, want_dho)
        _, dho, n = _device_count(m, ct, ot, n_docs, per_key=False)
        assert n == want_n and np.array_equal(dho, want_dho)
        kc, dho, n = _device_count(m, ct, ot, n_docs, chars=True)
        assert n == want_n and np.array_equal(kc, want_kc) and np.array_equal(dho, want_dho)
        # an unaligned device corpus (a view one byte into a larger buffer)
        big = torch.zeros(corpus.size + 1, dtype=torch.uint8, device=dev)
        big[1:] = ct
        kc, dho, n = _device_count(m, big[1:], ot, n_docs)
        assert n == want_n and np.array_equal(kc, want_kc) and np.array_equal(dho, want_dho)
        # separator filter: the filtered hits
        swant_kc, swant_dho, swant_n = _oracle(o, corpus, offs, K, sep=True)
        kc, dho, n = _device_count(m, ct, ot, n_docs, sep=_sep())
        assert n == swant_n and np.array_equal(kc, swant_kc) and np.array_equal(dho, swant_dho)
        kc, dho = m.count_batch(corpus, offs, sep=_sep())
        assert np.array_equal(kc, swant_kc) and np.array_equal(dho, swant_dho)


def test_count_accumulates_over_batches(variant):
    import torch

    rng = random.Random(11)
    keys = _keys_utf8(rng) if variant in ("u", "ur", "u23", "uh", "k", "p") else _keys_ascii(rng)
    m, o = _compile(keys)
    K = m.n_keys
    parts = [_docs(rng, keys, 5, 3000, 0.5) for _ in range(3)]
    corpus, offs = _batch([d for p in parts for d in p])
    want_kc, _, want_n = _oracle(o, corpus, offs, K)
    acc = np.zeros(K, dtype=np.uint64)
    total = 0
    for p in parts:
        c, of = _batch(p)
        ct = torch.from_numpy(c).to("cuda:0")
        ot = torch.from_numpy(of.view(np.int64)).to("cuda:0")
        acc, _, n = _device_count(m, ct, ot, len(p), accumulate=acc)
        total += n
    assert total == want_n and np.array_equal(acc, want_kc)
    host = np.zeros(K, dtype=np.uint64)
    for p in parts:
        c, of = _batch(p)
        m.count_batch(c, of, accumulate_into=host)
    assert np.array_equal(host, want_kc)


def test_count_engine_and_bad_offsets(variant):
    import torch

    rng = random.Random(5)
    keys = _keys_utf8(rng) if variant in ("u", "ur", "u23", "uh", "k", "p") else _keys_ascii(rng)
    m, o = _compile(keys)
    K = m.n_keys
    docs = _docs(rng, keys, 20, 20000, 0.5)
    corpus, offs = _batch(docs)
    want_kc, want_dho, want_n = _oracle(o, corpus, offs, K)
    ct = torch.from_numpy(corpus).to("cuda:0")
    ot = torch.from_numpy(offs.view(np.int64)).to("cuda:0")
    m.set_profiling(True)
    out = torch.zeros((want_n + 8, 3), dtype=torch.int32, device="cuda:0")
    assert m.match_batch_device(ct, ot, out) == want_n
    engine = m.last_timing()["engine"]
    kc, dho, n = _device_count(m, ct, ot, 20)
    t = m.last_timing()
    assert t["engine"] == engine, (t["engine"], engine)  # the fast path is the match's path, not the two-pass engine
    assert t["n_hits"] == want_n and np.array_equal(kc, want_kc) and np.array_equal(dho, want_dho)
    _, _, n = _device_count(m, ct, ot, 20, per_key=False)
    assert m.last_timing()["engine"] == engine and n == want_n
    # offsets the device rejects: AHA_E_INVALID, and the handle goes on
    bad = ot.clone()
    bad[3] = bad[4] + 5
    with pytest.raises(AhaError) as e:
        _device_count(m, ct, bad, 20)
    assert e.value.code == N.AHA_E_INVALID
    kc, dho, n = _device_count(m, ct, ot, 20)
    assert n == want_n and np.array_equal(kc, want_kc) and np.array_equal(dho, want_dho)


def test_count_between_matches_on_one_handle(variant):
    import torch

    rng = random.Random(3)
    keys = _keys_utf8(rng) if variant in ("u", "ur", "u23", "uh", "k", "p") else _keys_ascii(rng)
    m, o = _compile(keys)
    K = m.n_keys
    docs = _docs(rng, keys, 12, 9000, 0.6)
    corpus, offs = _batch(docs)
    want_hits, want_dho = o.match_batch(corpus, offs)
    want_kc, _, _ = _oracle(o, corpus, offs, K)
    swant_kc, _, _ = _oracle(o, corpus, offs, K, sep=True)
    ct = torch.from_numpy(corpus).to("cuda:0")
    ot = torch.from_numpy(offs.view(np.int64)).to("cuda:0")

    def match():
        out = torch.zeros((want_hits.size + 8, 3), dtype=torch.int32, device="cuda:0")
        dho = torch.zeros(offs.size, dtype=torch.int64, device="cuda:0")
        n = m.match_batch_device(ct, ot, out, dho)
        assert n == want_hits.size
        assert out[:n].cpu().numpy().tobytes() == want_hits.tobytes()
        assert np.array_equal(dho.cpu().numpy().view(np.uint64), want_dho)
        gh, gd = m.match_batch(corpus, offs)
        assert np.asarray(gh).tobytes() == want_hits.tobytes()

    match()
    kc, _, _ = _device_count(m, ct, ot, offs.size - 1)
    assert np.array_equal(kc, want_kc)
    match()
    kc, _, _ = _device_count(m, ct, ot, offs.size - 1, sep=_sep())
    assert np.array_equal(kc, swant_kc)
    match()
    kc, _ = m.count_batch(corpus, offs)
    assert np.array_equal(kc, want_kc)
    match()


def test_count_two_threads_one_handle():
    import torch

    rng = random.Random(9)
    keys = _keys_utf8(rng)
    m, o = _compile(keys)
    K = m.n_keys
    batches = []
    for i in range(2):
        corpus, offs = _batch(_docs(rng, keys, 10, 30000, 0.5))
        batches.append((corpus, offs, _oracle(o, corpus, offs, K)))
    errors = []

    def run(i):
        try:
            torch.cuda.set_device(0)
            corpus, offs, (wk, wd, wn) = batches[i]
            s = torch.cuda.Stream()
            with torch.cuda.stream(s):
                ct = torch.from_numpy(corpus).to("cuda:0")
                ot = torch.from_numpy(offs.view(np.int64)).to("cuda:0")
                s.synchronize()
                for _ in range(5):
                    kc, dho, n = _device_count(m, ct, ot, offs.size - 1)
                    assert n == wn and np.array_equal(kc, wk) and np.array_equal(dho, wd)
                    kc, dho = m.count_batch(corpus, offs)
                    assert np.array_equal(kc, wk) and np.array_equal(dho, wd)
        except Exception as e:  # noqa: BLE001 (reported below)
            errors.append(repr(e))

    ts = [threading.Thread(target=run, args=(i,)) for i in range(2)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    assert not errors, errors


def test_count_hand_back_leaves_no_trace(monkeypatch):
    """A batch that is nothing but key starts: the prefix-filter engine hands it back inside the count call (repeats 1, then
    engine 2), the counts of the abandoned pass are not added, and the handle's back-off is not touched: a later match of
    sparse text still takes the filter, as it would had the count call not happened."""
    monkeypatch.delenv("AHA_ENGINE", raising=False)
    m = AC.compile(["abc", "bcd"])
    assert m.info["filter_prefix_bytes"] == 3
    m.set_profiling(True)
    text = np.frombuffer(b"abcd" * 3000, dtype=np.uint8)
    offs = np.array([0, text.size], dtype=np.uint64)
    for _ in range(2):
        kc, dho = m.count_batch(text, offs)
        t = m.last_timing()
        assert t["engine"] == 2 and t["repeats"] == 1, t
        assert kc.tolist() == [3000, 3000] and dho.tolist() == [0, 6000]
    acc = np.array([5, 7], dtype=np.uint64)
    m.count_batch(text, offs, accumulate_into=acc)
    assert acc.tolist() == [3005, 3007] and m.last_timing()["repeats"] == 1
    sparse = b"-" * 5000 + b"abcd"
    assert len(m.match_array(sparse)) == 2 and m.last_timing()["engine"] == 5


@pytest.mark.parametrize("keyset", ["ascii", "utf8"])
def test_count_in_document_ranges(variant, keyset, monkeypatch):
    """Full-size regions beyond the bound (lowered for the test): the call counts document ranges one after another -- the
    counts add up, the offsets are rebased -- and a document that alone does not fit takes the two-pass engine's counting
    form.  The same results as one pass."""
    import torch

    rng = random.Random(zlib.crc32(f"ranges/{variant}/{keyset}".encode()))
    keys = KEYSETS[keyset](rng)
    m, o = _compile(keys)
    K = m.n_keys
    docs = _docs(rng, keys, 30, 6000, 0.5)
    docs[7] = b"".join(rng.choice(keys) for _ in range(8000))[:120000]  # (alone beyond the bound)
    corpus, offs = _batch(docs)
    want_kc, want_dho, want_n = _oracle(o, corpus, offs, K)
    ct = torch.from_numpy(corpus).to("cuda:0")
    ot = torch.from_numpy(offs.view(np.int64)).to("cuda:0")
    m.set_profiling(True)
    monkeypatch.setenv("AHA_COUNT_REGION_BYTES", str(1 << 20))
    for per_key in (True, False):
        kc, dho, n = _device_count(m, ct, ot, offs.size - 1, per_key=per_key)
        assert n == want_n and np.array_equal(dho, want_dho)
        assert not per_key or np.array_equal(kc, want_kc)
        if variant != "v1":
            assert m.last_timing()["repeats"] >= 1  # (the ranges before the last)
    acc = np.full(K, 3, dtype=np.uint64)
    kc, _, _ = _device_count(m, ct, ot, offs.size - 1, accumulate=acc)
    assert np.array_equal(kc, want_kc + 3)
    kc, dho = m.count_batch(corpus, offs)
    assert np.array_equal(kc, want_kc) and np.array_equal(dho, want_dho)
    monkeypatch.delenv("AHA_COUNT_REGION_BYTES")
    kc, dho, n = _device_count(m, ct, ot, offs.size - 1)
    assert n == want_n and np.array_equal(kc, want_kc) and np.array_equal(dho, want_dho)


def test_count_rejects_bad_buffers():
    import torch

    m = AC.compile(["he", "she"])
    with pytest.raises(ValueError):
        m.count_batch(b"ushers", [0, 6], accumulate_into=np.zeros(1, dtype=np.uint64))
    with pytest.raises(ValueError):
        m.count_batch(b"ushers", [0, 6], accumulate_into=np.zeros(2, dtype=np.int32))
    ct = torch.frombuffer(bytearray(b"ushers"), dtype=torch.uint8).to("cuda:0")
    ot = torch.tensor([0, 6], dtype=torch.int64, device="cuda:0")
    with pytest.raises(ValueError):
        m.count_batch_device(ct, ot, torch.zeros(1, dtype=torch.int64, device="cuda:0"))
    with pytest.raises(ValueError):
        m.count_batch_device(ct, ot, None, torch.zeros(1, dtype=torch.int64, device="cuda:0"))


def test_count_corpus_and_count():
    m, o = _compile([b"he", b"she", b"his", b"hers"])
    kc = m.count("ushers")
    assert kc.tolist() == [1, 1, 0, 1]
    corpus, offs = _batch([b"ushers", b"", b"his hers she"])
    dc = DeviceCorpus(corpus, offs)
    want_kc, want_dho, want_n = _oracle(o, corpus, offs, 4)
    kc, dho, n = m.count_corpus(dc)
    assert n == want_n and np.array_equal(kc, want_kc) and np.array_equal(dho, want_dho)
    kc, dho, n = m.count_corpus(dc, per_key=False)
    assert kc is None and n == want_n and np.array_equal(dho, want_dho)


def test_count_cfg5_full_keys():
    """cfg 5 at its full 1 M keys on 8 MiB: the counts are the bincount of the match call's hits"""
    import torch

    blob, offs, nf = synth.keys(5)
    corpus, doc = synth.corpus(5, blob, offs, nf, n_bytes=8 << 20, doc_bytes=1 << 20)
    m = AC.compile_packed(blob, offs)
    K = m.n_keys
    ct = torch.from_numpy(corpus).to("cuda:0")
    ot = torch.from_numpy(doc.astype(np.int64)).to("cuda:0")
    m.set_profiling(True)
    kc, dho, n = _device_count(m, ct, ot, doc.size - 1)
    count_engine = m.last_timing()["engine"]
    out = torch.zeros((n + 8, 3), dtype=torch.int32, device="cuda:0")
    mdho = torch.zeros(doc.size, dtype=torch.int64, device="cuda:0")
    assert m.match_batch_device(ct, ot, out, mdho) == n
    assert m.last_timing()["engine"] == count_engine
    vals = out[:n, 2].cpu().numpy().astype(np.int64)
    assert np.array_equal(kc, np.bincount(vals, minlength=K).astype(np.uint64))
    assert np.array_equal(dho, mdho.cpu().numpy().view(np.uint64))
