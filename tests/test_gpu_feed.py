"""Feeds (aha_feed_*) on the GPU: sequences fed in pieces over several calls give, piece by piece, exactly the hits one plain
match over the whole sequence reports -- against the CPU oracle and against match_batch of the whole documents -- on every
engine variant, in bytes and in characters.  Beside parity: the engine of the main pass, failed calls that leave the feed as
it was (capacity, bad ids and offsets checked on the device, a piece too long), reset, feed calls between plain match and
count calls (the window pass leaves no trace in the prefix filter's back-off), two feeds in two threads, a non-default
stream, a reduced grid, and one sequence longer than 2^31 bytes."""
import ctypes as C
import random
import threading
import zlib

import numpy as np
import pytest

import pyoracle as orc
from aha_amd import AC, AhaError, HIT_DTYPE, synth
from aha_amd import _native as N
from engine_variants import VARIANTS, use_variant
from feedsim import FeedSim, absolute, leads

pytestmark = pytest.mark.gpu


def _keys_ascii(rng):
    words = sorted({"".join(rng.choice("abcdefgh") for _ in range(rng.randint(3, 9))) for _ in range(600)})
    return [w.encode() for w in words]


def _keys_cjk(rng):
    blob, offs, _ = synth.keys(3, K=3000, seed=7)
    return [bytes(blob[offs[i]:offs[i + 1]]) for i in range(offs.size - 1)]


def _keys_nested(rng):
    return [b"a" * i for i in range(1, 24)] + [("我" * i).encode() for i in range(1, 21)] + [b"ba", b"bab"]


def _keys_single(rng):  # W = 0
    return [b"a", b"b", b" ", b"\x80", b"\xe6"]


def _keys_long(rng):
    return [b"x" * 100, bytes(rng.choice(b"xy") for _ in range(97)), b"xx", b"xy", b"y", b"yx" * 3, ("是" * 33).encode()]


KEYSETS = {"ascii": _keys_ascii, "cjk": _keys_cjk, "nested": _keys_nested, "single": _keys_single, "long": _keys_long}


def _text(rng, keys, n):
    pieces = [k for k in keys if len(k) < 128]
    fill = [b" ", b"q", b"\x00", b"zz", "中".encode(), "我是".encode(), b"a", b"x", b"\x80"]
    out = bytearray()
    while len(out) < n:
        out += rng.choice(pieces) if rng.random() < 0.45 else rng.choice(fill)
    return bytes(out[:n])


def _next_len(rng, text, pos, W):
    """a piece length: empty, 1 byte, shorter than W, up to a NUL, inside a character, or a large part"""
    left = len(text) - pos
    r = rng.random()
    if r < 0.1:
        n = 0
    elif r < 0.2:
        n = 1
    elif r < 0.35:
        n = rng.randint(0, max(W - 1, 0))
    elif r < 0.45:
        z = text.find(b"\x00", pos)
        n = (z - pos + rng.randint(0, 1)) if z >= 0 else left
    elif r < 0.55:
        n = next((i - pos + 1 for i in range(pos, min(len(text), pos + 64)) if text[i] >= 0xC0), rng.randint(1, 64))
    else:
        n = rng.randint(1, max(1, len(text) // 3))
    return max(0, min(n, left))


def _device(arr, dtype=None):
    import torch

    a = np.ascontiguousarray(arr)
    if dtype is not None:
        a = a.astype(dtype)
    return torch.from_numpy(a).to("cuda:0")


def _call(f, pieces, ids, use_device, cap=None, stream=None):
    """one feed call on pieces (bytes) of sequences ids -> (hits, piece_hit_offsets, piece_bases)"""
    import torch

    corpus = np.frombuffer(b"".join(pieces), dtype=np.uint8).copy()
    offs = np.cumsum([0] + [len(p) for p in pieces]).astype(np.uint64)
    ids = np.array(ids, dtype=np.uint32)
    if not use_device:
        return f.match_batch(corpus, offs, ids, cap=cap)
    D = len(pieces)
    ct, ot, it = _device(corpus), _device(offs.view(np.int64)), _device(ids.view(np.int32))
    pho = torch.zeros(D + 1, dtype=torch.int64, device="cuda:0")
    bases = torch.zeros(max(D, 1), dtype=torch.int64, device="cuda:0")
    cap = max(16, corpus.size // 2) if cap is None else cap
    while True:
        out = torch.zeros((max(cap, 1), 3), dtype=torch.int32, device="cuda:0")
        try:
            n = f.match_batch_device(ct, ot, it, out, pho, bases, stream=stream)
            break
        except AhaError as e:
            assert e.code == N.AHA_E_CAPACITY
            cap = e.required
    torch.cuda.synchronize()
    hits = out[:n].cpu().numpy().view(HIT_DTYPE).reshape(-1).copy()
    return hits, pho.cpu().numpy().view(np.uint64), bases.cpu().numpy().view(np.uint64)[:D]


def _feed_all(m, sim, texts, chars, rng, f=None, device_every=2, stream=None):
    """feeds texts over several calls (shuffled subsets of the sequences, random cuts); checks every call's offsets, bases and
    positions against the CPU twin and returns the absolute hits per sequence"""
    S = len(texts)
    f = f or m.feed(S, chars=chars)
    pos = [0] * S
    got = [[] for _ in range(S)]
    W = sim.W
    call = 0
    while any(pos[s] < len(texts[s]) for s in range(S)) or call < 2:
        ids = [s for s in range(S) if rng.random() < 0.75]
        rng.shuffle(ids)
        pieces = []
        for s in ids:
            n = _next_len(rng, texts[s], pos[s], W)
            pieces.append(texts[s][pos[s]:pos[s] + n])
            pos[s] += n
        hits, pho, bases = _call(f, pieces, ids, use_device=(call % device_every == 1), stream=stream)
        assert pho[0] == 0 and pho[-1] == len(hits)
        for d, s in enumerate(ids):
            want, base = sim.piece(s, pieces[d])
            assert int(bases[d]) == base, (call, d)
            part = hits[int(pho[d]):int(pho[d + 1])]
            assert np.array_equal(part, want), (call, d, s)
            got[s].append(absolute(part, base))
        for s in set(ids):
            nb, nc = f.position(s)
            assert nb == pos[s] and (not chars or nc == leads(texts[s][:pos[s]]))
        call += 1
    return f, [np.concatenate(g) if g else np.zeros(0, dtype=HIT_DTYPE) for g in got]


def _check_whole(m, o, texts, got, chars):
    corpus = np.frombuffer(b"".join(texts), dtype=np.uint8).copy()
    offs = np.cumsum([0] + [len(t) for t in texts]).astype(np.uint64)
    mh, mdho = m.match_batch(corpus, offs, chars=chars)
    for s, t in enumerate(texts):
        want = o.match(t, chars=chars) if t else np.zeros(0, dtype=HIT_DTYPE)
        assert np.array_equal(got[s], want), s
        assert np.array_equal(got[s], mh[int(mdho[s]):int(mdho[s + 1])]), s


@pytest.fixture(params=VARIANTS)
def variant(request, monkeypatch):
    return use_variant(request.param, monkeypatch)


@pytest.mark.parametrize("chars", [False, True], ids=["bytes", "chars"])
@pytest.mark.parametrize("keyset", sorted(KEYSETS))
def test_feed_parity(variant, keyset, chars):
    rng = random.Random(zlib.crc32(f"feed/{variant}/{keyset}/{chars}".encode()))
    keys = KEYSETS[keyset](rng)
    m, o = AC.compile(keys), orc.AC.compile(keys)
    S = rng.randint(4, 8)
    texts = [_text(rng, keys, rng.choice([0, 37, 5000, 60000, 300000])) for _ in range(S)]
    sim = FeedSim(o, S, chars)
    assert sim.W == max(max(len(k) for k in keys) - 1, 0)
    f, got = _feed_all(m, sim, texts, chars, rng)
    _check_whole(m, o, texts, got, chars)
    f.close()


def test_feed_engine_and_whole_documents(monkeypatch):
    """A fresh feed given whole documents equals match_batch bit for bit, and its main pass takes the engine the plain match of
    the same pieces takes."""
    import torch

    monkeypatch.delenv("AHA_ENGINE", raising=False)
    blob, offs, nf = synth.keys(3, K=5000)
    corpus, doc = synth.corpus(3, blob, offs, nf, n_bytes=4 << 20, doc_bytes=1 << 16)
    for chars in (False, True):
        m = AC.compile_packed(blob, offs)
        m.set_profiling(True)
        D = doc.size - 1
        ct, dt = _device(corpus), _device(doc.view(np.int64))
        cap = corpus.size // 2
        out = torch.zeros((cap, 3), dtype=torch.int32, device="cuda:0")
        dho = torch.zeros(D + 1, dtype=torch.int64, device="cuda:0")
        n = m.match_batch_device(ct, dt, out, dho, chars=chars)
        plain = m.last_timing()["engine"]
        want = out[:n].cpu().numpy().view(HIT_DTYPE).reshape(-1).copy()
        want_dho = dho.cpu().numpy().view(np.uint64).copy()
        f = m.feed(D, chars=chars)
        it = _device(np.arange(D, dtype=np.int32))
        pho = torch.zeros(D + 1, dtype=torch.int64, device="cuda:0")
        bases = torch.zeros(D, dtype=torch.int64, device="cuda:0")
        out.zero_()
        n2 = f.match_batch_device(ct, dt, it, out, pho, bases)
        assert m.last_timing()["engine"] == plain
        assert n2 == n and np.array_equal(out[:n].cpu().numpy().view(HIT_DTYPE).reshape(-1), want)
        assert np.array_equal(pho.cpu().numpy().view(np.uint64), want_dho) and not bases.any()
        f.close()


def _small_case(seed, chars=False):
    rng = random.Random(seed)
    keys = _keys_ascii(rng) + [b"x" * 40]
    m, o = AC.compile(keys), orc.AC.compile(keys)
    texts = [_text(rng, keys, 20000) for _ in range(4)]
    return rng, keys, m, o, texts


def test_feed_capacity_leaves_feed_unchanged():
    rng, keys, m, o, texts = _small_case(11)
    f = m.feed(4)
    sim = FeedSim(o, 4)
    # a first call so that the sequences have context
    first = [t[:777] for t in texts]
    _, _, _ = f.match_batch(np.frombuffer(b"".join(first), np.uint8), np.cumsum([0] + [777] * 4).astype(np.uint64),
                            np.arange(4, dtype=np.uint32))
    for s in range(4):
        sim.piece(s, first[s])
    pieces = [texts[s][777:777 + 3001 * (s + 1)] for s in (2, 0, 3)]
    ids = [2, 0, 3]
    want = [sim.piece(s, p)[0] for s, p in zip(ids, pieces)]
    required = sum(len(w) for w in want)
    for use_device in (False, True):
        corpus = np.frombuffer(b"".join(pieces), np.uint8).copy()
        offs = np.cumsum([0] + [len(p) for p in pieces]).astype(np.uint64)
        if use_device:
            import torch

            out = torch.zeros((required - 1, 3), dtype=torch.int32, device="cuda:0")
            with pytest.raises(AhaError) as e:
                f.match_batch_device(_device(corpus), _device(offs.view(np.int64)), _device(np.array(ids, np.int32)), out)
            assert e.value.code == N.AHA_E_CAPACITY and e.value.required == required
        else:
            out = np.zeros(required, dtype=HIT_DTYPE)
            n = C.c_uint64(0)
            ids_a = np.array(ids, np.uint32)
            rc = N.lib().aha_feed_match_batch(f._h, corpus.ctypes.data, offs.ctypes.data, ids_a.ctypes.data, 3,
                                              out.ctypes.data, required - 1, None, None, C.byref(n))
            assert rc == N.AHA_E_CAPACITY and n.value == required
        assert [f.position(s)[0] for s in range(4)] == [777] * 4
    hits, pho, bases = _call(f, pieces, ids, use_device=True, cap=required)
    assert np.array_equal(hits, np.concatenate(want)) and bases.tolist() == [777] * 3


def test_feed_bad_arguments_checked_on_device():
    import torch

    rng, keys, m, o, texts = _small_case(12)
    f = m.feed(4)
    f.match(1, texts[1][:500])
    piece = np.frombuffer(texts[0][:1000], np.uint8).copy()
    ct = _device(piece)
    out = torch.zeros((4096, 3), dtype=torch.int32, device="cuda:0")
    bad = [
        ([0, 500, 1000], [0, 4]),   # an id >= n_seqs
        ([0, 500, 1000], [1, 1]),   # an id twice
        ([0, 600, 500, 1000], [0, 1, 2]),  # not ascending
        ([0, 500, 999], [0, 1]),    # [D] != n_bytes
        ([1, 500, 1000], [0, 1]),   # [0] != 0
    ]
    for offs, ids in bad:
        with pytest.raises(AhaError) as e:
            f.match_batch_device(ct, _device(np.array(offs, np.int64)), _device(np.array(ids, np.int32)), out)
        assert e.value.code == N.AHA_E_INVALID, (offs, ids)
        assert f.position(1)[0] == 500 and f.position(0)[0] == 0
    # a piece that claims 2^31 bytes: refused before anything reads the corpus
    offs = _device(np.array([0, 1 << 31], np.int64))
    ids = _device(np.array([0], np.int32))
    n = C.c_uint64(0)
    rc = N.lib().aha_feed_match_batch_device(f._h, ct.data_ptr(), offs.data_ptr(), ids.data_ptr(), 1, 1 << 31, out.data_ptr(),
                                             4096, None, None, C.byref(n), None)
    assert rc == N.AHA_E_TOO_LONG
    assert f.position(1)[0] == 500 and f.position(0)[0] == 0
    # and the feed goes on as if nothing had happened
    sim = FeedSim(o, 4)
    sim.piece(1, texts[1][:500])
    hits, _, _ = _call(f, [texts[1][500:3000]], [1], use_device=True)
    assert np.array_equal(hits, sim.piece(1, texts[1][500:3000])[0])


def test_feed_reset():
    rng, keys, m, o, texts = _small_case(13, chars=True)
    f = m.feed(4, chars=True)
    sim = FeedSim(o, 4, chars=True)
    _feed_all(m, sim, texts, True, rng, f=f)
    f.reset(2)
    sim.reset(2)
    assert f.position(2) == (0, 0) and f.position(1)[0] == len(texts[1])
    hits, pho, bases = _call(f, [texts[0][:3000], texts[2][:5000]], [2, 1], use_device=False)
    want2, _ = FeedSim(o, 1, chars=True).piece(0, texts[0][:3000])
    assert np.array_equal(hits[:int(pho[1])], want2) and int(bases[0]) == 0
    assert int(bases[1]) == leads(texts[1])
    f.reset()
    assert all(f.position(s) == (0, 0) for s in range(4))


def test_feed_between_match_and_count_calls(monkeypatch):
    """Feed calls leave what plain match and count calls give, and their engines, as they were; the window pass does not touch
    the prefix filter's back-off: a dense match hands back (the next two calls skip the filter), a feed call takes one of the
    two, as a plain match of its pieces would, and the sparse match behind it takes the other."""
    monkeypatch.delenv("AHA_ENGINE", raising=False)
    m = AC.compile(["abc", "bcd"])
    assert m.info["filter_prefix_bytes"] == 3
    m.set_profiling(True)
    dense = np.frombuffer(b"abcd" * 3000, dtype=np.uint8)
    doffs = np.array([0, dense.size], dtype=np.uint64)
    sparse = b"-" * 5000 + b"abcd"

    def run(with_feed):
        m2 = AC.compile(["abc", "bcd"])
        m2.set_profiling(True)
        engines = []
        h, _ = m2.match_batch(dense, doffs)
        engines.append((m2.last_timing()["engine"], m2.last_timing()["repeats"]))
        assert len(h) == 6000
        if with_feed:
            f = m2.feed(2)
            assert [(x.start, x.end) for x in f.match(1, sparse[:2500])] == []
        else:
            m2.match_array(sparse[:2500])
        engines.append(m2.last_timing()["engine"])
        assert len(m2.match_array(sparse)) == 2
        engines.append(m2.last_timing()["engine"])
        kc, dho = m2.count_batch(dense, doffs)
        assert kc.tolist() == [3000, 3000]
        assert len(m2.match_array(sparse)) == 2
        engines.append(m2.last_timing()["engine"])
        return engines

    assert run(True) == run(False)
    f = m.feed(1)
    seq = b"--ab" + b"cd" * 5
    got = []
    for a in range(0, len(seq), 3):
        got += f.match(0, seq[a:a + 3])
    assert [(h.start, h.end, h.value) for h in got] == [(2, 5, 0), (3, 6, 1)]


def test_feed_two_threads_one_handle():
    rng, keys, m, o, texts = _small_case(14)
    errors = []

    def worker(k):
        try:
            r = random.Random(100 + k)
            ts = [_text(r, keys, 30000) for _ in range(3)]
            sim = FeedSim(o, 3, chars=bool(k))
            _, got = _feed_all(m, sim, ts, bool(k), r)
            _check_whole(m, o, ts, got, bool(k))
        except Exception as e:  # noqa: BLE001 -- reported below
            errors.append(e)

    th = [threading.Thread(target=worker, args=(k,)) for k in range(2)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert not errors, errors


def test_feed_on_a_side_stream():
    import torch

    rng, keys, m, o, texts = _small_case(15)
    s = torch.cuda.Stream()
    sim = FeedSim(o, 4)
    with torch.cuda.stream(s):
        _, got = _feed_all(m, sim, texts, False, rng, device_every=1, stream=s.cuda_stream)
    _check_whole(m, o, texts, got, False)


def test_feed_reduced_grid(monkeypatch):
    monkeypatch.setenv("AHA_RESERVE_CUS", "1")
    rng, keys, m, o, texts = _small_case(16)
    for chars in (False, True):
        sim = FeedSim(o, 4, chars)
        _, got = _feed_all(m, sim, texts, chars, rng)
        _check_whole(m, o, texts, got, chars)


def test_feed_sequence_longer_than_2g():
    """One sequence of 5 x 512 MiB of cfg 3 text, fed a piece per call from one device buffer: the bases are exact past 2^31,
    the hits within 1 MiB of each cut equal the oracle on that stretch (with a W-byte lead-in), and the others equal the plain
    match of the piece."""
    import torch

    P, R, n_pieces = 512 << 20, 1 << 20, 5
    blob, koffs, nf = synth.keys(3)
    m, o = AC.compile_packed(blob, koffs), orc.AC.compile_packed(blob, koffs)
    W = o.max_key_len - 1
    buf = torch.empty(n_pieces * P, dtype=torch.uint8, device="cuda:0")
    tails, heads = [], []
    for k in range(n_pieces):
        text, _ = synth.corpus(3, blob, koffs, nf, n_bytes=P, rank=k)
        buf[k * P:(k + 1) * P].copy_(torch.from_numpy(text))
        heads.append(bytes(text[:R]))
        tails.append(bytes(text[-(R + W):]))
        del text
    torch.cuda.synchronize()
    f = m.feed(1)
    offs = _device(np.array([0, P], np.int64))
    ids = _device(np.array([0], np.int32))
    one = _device(np.array([0, P], np.int64))
    out = torch.empty((48 << 20, 3), dtype=torch.int32, device="cuda:0")
    pout = torch.empty((48 << 20, 3), dtype=torch.int32, device="cuda:0")
    bases = torch.zeros(1, dtype=torch.int64, device="cuda:0")
    prev = None
    for k in range(n_pieces):
        piece = buf[k * P:(k + 1) * P]
        n = f.match_batch_device(piece, offs, ids, out, None, bases)
        assert int(bases[0]) == k * P
        hits = out[:n].cpu().numpy().view(HIT_DTYPE).reshape(-1).copy()
        pn = m.match_batch_device(piece, one, pout)
        plain = pout[:pn].cpu().numpy().view(HIT_DTYPE).reshape(-1)
        far = hits["end"] > R
        assert np.array_equal(hits[far], plain[plain["end"] > R]), k
        if prev is not None:  # the stretch of 1 MiB on each side of the cut
            want = o.match(tails[k - 1] + heads[k])
            want = want[want["end"] > W].copy()
            want["start"] -= R + W
            want["end"] -= R + W
            before = prev[prev["end"] > P - R].copy()
            before["start"] -= P
            before["end"] -= P
            got = np.concatenate([before, hits[~far]])
            assert np.array_equal(got, want), k
        prev = hits
    assert f.position(0)[0] == n_pieces * P > (1 << 31)
    f.close()
