"""Feed counts (aha_feed_count_batch*) on the GPU: sequences fed in pieces over several calls give, call by call, the hits per
key, per-piece offsets and bases of the CPU twin (tests/feedsim.py), and over all calls the oracle's count of each whole
sequence -- on every engine variant, in bytes and in characters.  Beside parity: running totals and key_counts = NULL, count
and match calls mixed on one feed, failed calls that change neither the feed nor the caller's totals, the engine of the main
pass and no trace in the prefix filter's back-off, one sequence longer than 2^31 bytes, two feeds in two threads, a side
stream and a reduced grid."""
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
from feedsim import FeedSim, leads
from test_gpu_feed import KEYSETS, _call, _device, _keys_ascii, _next_len, _text

pytestmark = pytest.mark.gpu


def _bc(hits, K):
    return np.bincount(hits["value"], minlength=K).astype(np.uint64) if len(hits) else np.zeros(K, dtype=np.uint64)


def _whole(o, t, chars=False):
    return o.match(t, chars=chars) if t else np.zeros(0, dtype=HIT_DTYPE)


def _count_call(f, pieces, ids, use_device, K, per_key=True, acc=None, stream=None):
    """one feed count call -> (key_counts or None, piece_hit_offsets, piece_bases, n_hits); acc: running totals (uint64[K])
    added to in place"""
    import torch

    corpus = np.frombuffer(b"".join(pieces), dtype=np.uint8).copy()
    offs = np.cumsum([0] + [len(p) for p in pieces]).astype(np.uint64)
    ids = np.array(ids, dtype=np.uint32)
    D = len(pieces)
    if not use_device:
        kc, pho, bases = f.count_batch(corpus, offs, ids, per_key=per_key, accumulate_into=acc)
        return kc, pho, bases, int(pho[-1])
    ct, ot, it = _device(corpus), _device(offs.view(np.int64)), _device(ids.view(np.int32))
    pho = torch.zeros(D + 1, dtype=torch.int64, device="cuda:0")
    bases = torch.zeros(max(D, 1), dtype=torch.int64, device="cuda:0")
    kct = None
    if acc is not None:
        kct = _device(acc.view(np.int64))
    elif per_key:
        kct = torch.full((K,), 7, dtype=torch.int64, device="cuda:0")  # (overwritten without ACCUMULATE)
    n = f.count_batch_device(ct, ot, it, kct, pho, bases, accumulate=acc is not None, stream=stream)
    torch.cuda.synchronize()
    kc = kct.cpu().numpy().view(np.uint64).copy() if kct is not None else None
    if acc is not None:
        acc[:] = kc
    return kc, pho.cpu().numpy().view(np.uint64), bases.cpu().numpy().view(np.uint64)[:D], n


def _count_all(m, sim, texts, chars, rng, f=None, device_every=2, stream=None):
    """counts texts over several calls (shuffled subsets of the sequences, random cuts); checks every call's key counts,
    offsets, bases and positions against the CPU twin and the running totals against the oracle on the whole sequences"""
    S, K, W = len(texts), m.n_keys, sim.W
    f = f or m.feed(S, chars=chars)
    pos = [0] * S
    running = np.zeros(K, dtype=np.uint64)
    call = 0
    while any(pos[s] < len(texts[s]) for s in range(S)) or call < 2:
        ids = [s for s in range(S) if rng.random() < 0.75]
        rng.shuffle(ids)
        pieces = []
        for s in ids:
            n = _next_len(rng, texts[s], pos[s], W)
            pieces.append(texts[s][pos[s]:pos[s] + n])
            pos[s] += n
        use_device = call % device_every == 1
        before = running.copy()
        kc, pho, bases, n = _count_call(f, pieces, ids, use_device, K, acc=running if call % 3 == 2 else None, stream=stream)
        want_kc = np.zeros(K, dtype=np.uint64)
        want_pho = [0]
        for d, s in enumerate(ids):
            hits, base = sim.piece(s, pieces[d])
            assert int(bases[d]) == base, (call, d)
            want_kc += _bc(hits, K)
            want_pho.append(want_pho[-1] + len(hits))
        assert pho.tolist() == want_pho and n == want_pho[-1], call
        if call % 3 == 2:
            assert np.array_equal(kc, before + want_kc), call
        else:
            assert np.array_equal(kc, want_kc), call
            running += kc
        for s in set(ids):
            nb, nc = f.position(s)
            assert nb == pos[s] and (not chars or nc == leads(texts[s][:pos[s]]))
        call += 1
    return f, running


def _check_whole(o, texts, running, chars):
    want = np.zeros(running.size, dtype=np.uint64)
    for t in texts:
        want += _bc(_whole(o, t, chars), running.size)
    assert np.array_equal(running, want)


@pytest.fixture(params=VARIANTS)
def variant(request, monkeypatch):
    return use_variant(request.param, monkeypatch)


@pytest.mark.parametrize("chars", [False, True], ids=["bytes", "chars"])
@pytest.mark.parametrize("keyset", sorted(KEYSETS))
def test_feed_count_parity(variant, keyset, chars):
    rng = random.Random(zlib.crc32(f"feedcount/{variant}/{keyset}/{chars}".encode()))
    keys = KEYSETS[keyset](rng)
    m, o = AC.compile(keys), orc.AC.compile(keys)
    S = rng.randint(4, 8)
    texts = [_text(rng, keys, rng.choice([0, 37, 5000, 60000, 300000])) for _ in range(S)]
    sim = FeedSim(o, S, chars)
    f, running = _count_all(m, sim, texts, chars, rng)
    _check_whole(o, texts, running, chars)
    f.close()


def _small_case(seed):
    rng = random.Random(seed)
    keys = _keys_ascii(rng) + [b"x" * 40]
    m, o = AC.compile(keys), orc.AC.compile(keys)
    texts = [_text(rng, keys, 20000) for _ in range(4)]
    return rng, keys, m, o, texts


def test_feed_count_accumulate_and_null():
    import torch

    rng, keys, m, o, texts = _small_case(21)
    K = m.n_keys
    f = m.feed(4)
    sim = FeedSim(o, 4)
    prior = np.arange(K, dtype=np.uint64) * 1000 + 5
    for use_device in (False, True):
        # ACCUMULATE: the prior values plus the counts
        pieces, ids = [texts[0][:3000], texts[3][:100]], [0, 3]
        acc = prior.copy()
        kc, pho, bases, n = _count_call(f, pieces, ids, use_device, K, acc=acc)
        want = [sim.piece(s, p)[0] for s, p in zip(ids, pieces)]
        assert np.array_equal(acc, prior + _bc(np.concatenate(want), K))
        assert n == sum(len(w) for w in want)
        # without it: overwritten (the device form starts from a vector of 7s)
        pieces, ids = [texts[0][3000:6000]], [0]
        kc, pho, bases, n = _count_call(f, pieces, ids, use_device, K)
        assert np.array_equal(kc, _bc(sim.piece(0, pieces[0])[0], K))
        # key_counts = NULL: totals, offsets and bases, and the feed moves on
        pieces, ids = [texts[1][:2000], texts[0][6000:7000]], [1, 0]
        kc, pho, bases, n = _count_call(f, pieces, ids, use_device, K, per_key=False)
        want = [sim.piece(s, p) for s, p in zip(ids, pieces)]
        assert kc is None
        assert pho.tolist() == [0, len(want[0][0]), len(want[0][0]) + len(want[1][0])] and n == int(pho[-1])
        assert bases.tolist() == [w[1] for w in want]
        hits, _, _ = _call(f, [texts[0][7000:9000]], [0], use_device)
        assert np.array_equal(hits, sim.piece(0, texts[0][7000:9000])[0])
        texts = [t[9000:] for t in texts]
        f.reset()
        sim = FeedSim(o, 4)
    # NULL n_hits and unknown flags on a real feed
    L = N.lib()
    pos0 = f.position(0)
    offs = np.array([0, 0], dtype=np.uint64)
    ids = np.array([0], dtype=np.uint32)
    kc = np.zeros(K, dtype=np.uint64)
    n = C.c_uint64(0)
    assert L.aha_feed_count_batch(f._h, None, offs.ctypes.data, ids.ctypes.data, 1, 0, kc.ctypes.data, None, None,
                                  None) == N.AHA_E_INVALID
    assert L.aha_feed_count_batch(f._h, None, offs.ctypes.data, ids.ctypes.data, 1, 2, kc.ctypes.data, None, None,
                                  C.byref(n)) == N.AHA_E_INVALID
    dofs, dids = _device(offs.view(np.int64)), _device(ids.view(np.int32))
    dkc = torch.zeros(K, dtype=torch.int64, device="cuda:0")
    for flags, nh in ((0, None), (2, C.byref(n)), (0x80000001, C.byref(n))):
        assert L.aha_feed_count_batch_device(f._h, None, dofs.data_ptr(), dids.data_ptr(), 1, 0, flags, dkc.data_ptr(), None,
                                             None, nh, None) == N.AHA_E_INVALID
    assert f.position(0) == pos0
    f.close()


@pytest.mark.parametrize("chars", [False, True], ids=["bytes", "chars"])
def test_feed_count_and_match_mixed(chars):
    rng, keys, m, o, texts = _small_case(22)
    K = m.n_keys
    f = m.feed(4, chars=chars)
    sim = FeedSim(o, 4, chars)
    pos = [0] * 4
    call = 0
    while any(pos[s] < len(texts[s]) for s in range(4)):
        ids = [s for s in range(4) if rng.random() < 0.75]
        rng.shuffle(ids)
        pieces = []
        for s in ids:
            n = _next_len(rng, texts[s], pos[s], sim.W)
            pieces.append(texts[s][pos[s]:pos[s] + n])
            pos[s] += n
        use_device = (call // 2) % 2 == 1
        want = [sim.piece(s, p) for s, p in zip(ids, pieces)]
        if call % 2 == 0:
            hits, pho, bases = _call(f, pieces, ids, use_device)
            assert np.array_equal(hits, np.concatenate([w[0] for w in want])) if want else len(hits) == 0
        else:
            kc, pho, bases, n = _count_call(f, pieces, ids, use_device, K)
            assert np.array_equal(kc, _bc(np.concatenate([w[0] for w in want]) if want else np.zeros(0, HIT_DTYPE), K))
        assert np.diff(pho.astype(np.int64)).tolist() == [len(w[0]) for w in want]
        assert bases.tolist() == [w[1] for w in want]
        for s in range(4):
            nb, nc = f.position(s)
            assert nb == pos[s] and (not chars or nc == leads(texts[s][:pos[s]]))
        call += 1
    f.close()


def test_feed_count_failed_calls_change_nothing():
    import torch

    rng, keys, m, o, texts = _small_case(23)
    K = m.n_keys
    f = m.feed(4)
    sim = FeedSim(o, 4)
    f.match(1, texts[1][:500])
    sim.piece(1, texts[1][:500])
    prior = (np.arange(K, dtype=np.uint64) * 3 + 1)
    piece = np.frombuffer(texts[0][:1000], np.uint8).copy()
    ct = _device(piece)
    # host entry: a sequence named twice
    acc = prior.copy()
    with pytest.raises(AhaError) as e:
        f.count_batch(piece, np.array([0, 500, 1000], np.uint64), np.array([1, 1], np.uint32), accumulate_into=acc)
    assert e.value.code == N.AHA_E_INVALID and np.array_equal(acc, prior)
    # device entry: checked on the device
    bad = [
        ([0, 500, 1000], [1, 1]),   # an id twice
        ([0, 600, 500, 1000], [0, 1, 2]),  # not ascending
        ([0, 500, 1000], [0, 4]),   # an id >= n_seqs
    ]
    for offs, ids in bad:
        kct = _device(prior.view(np.int64))
        with pytest.raises(AhaError) as e:
            f.count_batch_device(ct, _device(np.array(offs, np.int64)), _device(np.array(ids, np.int32)), kct, accumulate=True)
        assert e.value.code == N.AHA_E_INVALID, (offs, ids)
        assert np.array_equal(kct.cpu().numpy().view(np.uint64), prior)
        assert f.position(1)[0] == 500 and f.position(0)[0] == 0
    # a piece that claims 2^31 bytes: refused before anything reads the corpus
    kct = _device(prior.view(np.int64))
    offs = _device(np.array([0, 1 << 31], np.int64))
    ids = _device(np.array([0], np.int32))
    n = C.c_uint64(0)
    rc = N.lib().aha_feed_count_batch_device(f._h, ct.data_ptr(), offs.data_ptr(), ids.data_ptr(), 1, 1 << 31,
                                             N.AHA_COUNT_ACCUMULATE, kct.data_ptr(), None, None, C.byref(n), None)
    assert rc == N.AHA_E_TOO_LONG
    torch.cuda.synchronize()
    assert np.array_equal(kct.cpu().numpy().view(np.uint64), prior)
    assert f.position(1)[0] == 500 and f.position(0)[0] == 0
    # the same pieces afterwards give the right counts
    acc = prior.copy()
    pieces, ids = [texts[0][:500], texts[1][500:1000]], [0, 1]
    _count_call(f, pieces, ids, True, K, acc=acc)
    want = np.concatenate([sim.piece(s, p)[0] for s, p in zip(ids, pieces)])
    assert np.array_equal(acc, prior + _bc(want, K))
    f.close()


def test_feed_count_engine_and_back_off(monkeypatch):
    """The main pass takes the engine count_batch of the same pieces takes; a feed count between plain calls leaves what they
    give, and their engines, as they were: a dense match hands back (the next two calls skip the prefix filter), and a feed
    count takes neither of the two."""
    import torch

    monkeypatch.delenv("AHA_ENGINE", raising=False)
    blob, offs, nf = synth.keys(3, K=5000)
    corpus, doc = synth.corpus(3, blob, offs, nf, n_bytes=4 << 20, doc_bytes=1 << 16)
    m = AC.compile_packed(blob, offs)
    m.set_profiling(True)
    D = doc.size - 1
    ct, dt = _device(corpus), _device(doc.view(np.int64))
    kc = torch.zeros(m.n_keys, dtype=torch.int64, device="cuda:0")
    n = m.count_batch_device(ct, dt, kc)
    plain = m.last_timing()["engine"]
    want = kc.cpu().numpy().copy()
    f = m.feed(D)
    it = _device(np.arange(D, dtype=np.int32))
    kc.zero_()
    pho = torch.zeros(D + 1, dtype=torch.int64, device="cuda:0")
    assert f.count_batch_device(ct, dt, it, kc, pho) == n
    assert m.last_timing()["engine"] == plain
    assert np.array_equal(kc.cpu().numpy(), want)
    f.close()

    dense = np.frombuffer(b"abcd" * 3000, dtype=np.uint8)
    doffs = np.array([0, dense.size], dtype=np.uint64)
    sparse = b"-" * 5000 + b"abcd"

    def run(with_feed):
        m2 = AC.compile(["abc", "bcd"])
        assert m2.info["filter_prefix_bytes"] == 3
        m2.set_profiling(True)
        engines = []
        h, _ = m2.match_batch(dense, doffs)
        assert len(h) == 6000
        engines.append((m2.last_timing()["engine"], m2.last_timing()["repeats"]))
        if with_feed:
            f2 = m2.feed(2)
            assert f2.count(1, dense.tobytes()).tolist() == [3000, 3000]
            assert f2.count(1, sparse).tolist() == [1, 1]
        m2.match_array(sparse[:2500])
        engines.append(m2.last_timing()["engine"])
        assert len(m2.match_array(sparse)) == 2
        engines.append(m2.last_timing()["engine"])
        assert len(m2.match_array(sparse)) == 2
        engines.append(m2.last_timing()["engine"])
        return engines

    assert run(True) == run(False)


def test_feed_count_sequence_longer_than_2g():
    """One sequence of 5 x 512 MiB of cfg 3 text counted a piece per call from one device buffer: each call's counts are the
    piece's own count corrected at the cut (the hits that end in the piece's first 1 MiB, with the previous piece's last
    1 MiB + W bytes as lead-in, in place of those of that 1 MiB alone).  The same 2.5 GiB as one document is too long for a
    plain count."""
    import torch

    P, R, n_pieces = 512 << 20, 1 << 20, 5
    blob, koffs, nf = synth.keys(3)
    m, o = AC.compile_packed(blob, koffs), orc.AC.compile_packed(blob, koffs)
    K, W = m.n_keys, o.max_key_len - 1
    buf = torch.empty(n_pieces * P, dtype=torch.uint8, device="cuda:0")
    tails, heads = [], []
    for k in range(n_pieces):
        text, _ = synth.corpus(3, blob, koffs, nf, n_bytes=P, rank=k)
        buf[k * P:(k + 1) * P].copy_(torch.from_numpy(text))
        heads.append(bytes(text[:R]))
        tails.append(bytes(text[-(R + W):]))
        del text
    torch.cuda.synchronize()
    whole = _device(np.array([0, n_pieces * P], np.int64))
    with pytest.raises(AhaError) as e:
        m.count_batch_device(buf, whole)
    assert e.value.code == N.AHA_E_TOO_LONG
    f = m.feed(1)
    offs = _device(np.array([0, P], np.int64))
    ids = _device(np.array([0], np.int32))
    kc = torch.zeros(K, dtype=torch.int64, device="cuda:0")
    pkc = torch.zeros(K, dtype=torch.int64, device="cuda:0")
    bases = torch.zeros(1, dtype=torch.int64, device="cuda:0")
    for k in range(n_pieces):
        piece = buf[k * P:(k + 1) * P]
        n = f.count_batch_device(piece, offs, ids, kc, None, bases)
        assert int(bases[0]) == k * P
        pn = m.count_batch_device(piece, offs, pkc)
        want = pkc.cpu().numpy().view(np.uint64).copy()
        if k:
            cut = o.match(tails[k - 1] + heads[k])
            want += _bc(cut[cut["end"] > R + W], K)
            want -= _bc(o.match(heads[k]), K)
        got = kc.cpu().numpy().view(np.uint64)
        assert np.array_equal(got, want), k
        assert n == int(want.sum()) and (k or n == pn)
    assert f.position(0)[0] == n_pieces * P > (1 << 31)
    f.close()


def test_feed_count_two_threads_one_handle():
    rng, keys, m, o, texts = _small_case(24)
    errors = []

    def worker(k):
        try:
            r = random.Random(200 + k)
            ts = [_text(r, keys, 30000) for _ in range(3)]
            sim = FeedSim(o, 3, chars=bool(k))
            _, running = _count_all(m, sim, ts, bool(k), r)
            _check_whole(o, ts, running, bool(k))
        except Exception as e:  # noqa: BLE001 -- reported below
            errors.append(e)

    th = [threading.Thread(target=worker, args=(k,)) for k in range(2)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert not errors, errors


def test_feed_count_on_a_side_stream():
    import torch

    rng, keys, m, o, texts = _small_case(25)
    s = torch.cuda.Stream()
    sim = FeedSim(o, 4)
    with torch.cuda.stream(s):
        _, running = _count_all(m, sim, texts, False, rng, device_every=1, stream=s.cuda_stream)
    _check_whole(o, texts, running, False)


def test_feed_count_reduced_grid(monkeypatch):
    monkeypatch.setenv("AHA_RESERVE_CUS", "1")
    rng, keys, m, o, texts = _small_case(26)
    for chars in (False, True):
        sim = FeedSim(o, 4, chars)
        _, running = _count_all(m, sim, texts, chars, rng)
        _check_whole(o, texts, running, chars)
