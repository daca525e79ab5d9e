"""Feeds with a separator filter (aha_feed_open_params, aha_feed_finish_batch*) on the GPU, exact against the model
(feedsepsim: the oracle's match(text, sep) of the whole sequence, partitioned by the stream law): random cuts on every engine
variant, every cut of one text around keys that end at the cut, a folded handle, count calls, failed and refused calls that
leave the feed as it was, one call of more than 2^20 unfiltered hits (many workgroups and rank blocks; once more on a reduced
grid), and a non-default stream."""
import ctypes as C
import random
import zlib

import numpy as np
import pytest

import pyoracle as orc
from aha_amd import AC, AhaError, HIT_DTYPE
from aha_amd import _native as N
from engine_variants import VARIANTS, use_variant
from feedsepsim import SEPS, FeedSepSim, absolute, bitarray
from test_gpu_feed import KEYSETS, _call, _device, _text
from test_gpu_feed_count import _count_call

pytestmark = pytest.mark.gpu

# the key sets that drive each variant's engine (character-level engines want the CJK keys)
VARIANT_KEYSET = {"v2": "nested", "v1": "long", "v2p": "single", "u": "cjk", "ur": "cjk", "u23": "cjk", "uh": "cjk", "k": "cjk",
                  "p": "cjk", "f": "ascii", "auto": "ascii"}


def _finish(f, ids, use_device, cap=None):
    """one finish call -> (hits, seq_hit_offsets, bases)"""
    import torch

    if not use_device:
        return f.finish_batch(np.array(ids, dtype=np.uint32), cap=cap)
    D = len(ids)
    it = _device(np.array(ids, dtype=np.int32)) if D else torch.zeros(0, dtype=torch.int32, device="cuda:0")
    sho = torch.zeros(D + 1, dtype=torch.int64, device="cuda:0")
    bases = torch.zeros(max(D, 1), dtype=torch.int64, device="cuda:0")
    cap = 16 if cap is None else cap
    while True:
        out = torch.zeros((max(cap, 1), 3), dtype=torch.int32, device="cuda:0")
        try:
            n = f.finish_batch_device(it, out, sho, bases)
            break
        except AhaError as e:
            assert e.code == N.AHA_E_CAPACITY
            cap = e.required
    torch.cuda.synchronize()
    return (out[:n].cpu().numpy().view(HIT_DTYPE).reshape(-1).copy(), sho.cpu().numpy().view(np.uint64),
            bases.cpu().numpy().view(np.uint64)[:D])


def _piece_len(rng, left, W):
    r = rng.random()
    if r < 0.1:
        n = 0
    elif r < 0.25:
        n = 1
    elif r < 0.55:
        n = rng.choice([W - 1, W, W + 1])  # around the context's width (W = Lmax + 1)
    else:
        n = rng.randint(1, 1500)
    return max(0, min(n, left))


def _feed_all(f, sim, texts, rng, W, stream=None, device_every=2, counts=None):
    """feeds texts over several calls (shuffled subsets, random cuts), then finishes every sequence; every call is compared
    with the model; counts: a uint64[K] array -- every third call is then a count call (checked against the model's hits) ->
    the absolute hits per sequence"""
    S = len(texts)
    pos = [0] * S
    got = [[] for _ in range(S)]
    call = 0
    while any(pos[s] < len(texts[s]) for s in range(S)) or call < 2:
        ids = [s for s in range(S) if rng.random() < 0.75]
        rng.shuffle(ids)
        pieces = []
        for s in ids:
            n = _piece_len(rng, len(texts[s]) - pos[s], W)
            pieces.append(texts[s][pos[s]:pos[s] + n])
            pos[s] += n
        want = [sim.piece(s, p) for s, p in zip(ids, pieces)]
        if counts is not None and call % 3 == 2:
            kc, pho, bases, n = _count_call(f, pieces, ids, call % 2 == 1, counts.size)
            assert n == sum(len(w[0]) for w in want)
            vals = np.concatenate([w[0]["value"] for w in want] + [np.zeros(0, np.int32)])
            assert np.array_equal(kc, np.bincount(vals, minlength=counts.size).astype(np.uint64)), call
            assert pho.tolist() == np.cumsum([0] + [len(w[0]) for w in want]).tolist(), call
            for d, s in enumerate(ids):
                got[s].append(absolute(want[d][0], want[d][1]))  # (the count call moved the feed on: the model's hits stand in)
        else:
            hits, pho, bases = _call(f, pieces, ids, use_device=(call % device_every == 1), stream=stream)
            assert pho[0] == 0 and pho[-1] == len(hits)
            for d, s in enumerate(ids):
                part = hits[int(pho[d]):int(pho[d + 1])]
                assert np.array_equal(part, want[d][0]), (call, d, s)
                got[s].append(absolute(part, want[d][1]))
        assert [int(b) for b in bases] == [w[1] for w in want], call
        call += 1
    ids = list(range(S))
    rng.shuffle(ids)
    for part_ids, use_device in ((ids[:S // 2], False), (ids[S // 2:], True)):
        hits, sho, bases = _finish(f, part_ids, use_device)
        for d, s in enumerate(part_ids):
            want, n = sim.finish(s)
            assert np.array_equal(hits[int(sho[d]):int(sho[d + 1])], want), s
            assert int(bases[d]) == n == len(texts[s])
            got[s].append(absolute(want, n))
    assert all(f.position(s) == (0, 0) for s in range(S))
    return [np.concatenate(g) for g in got]


def _check_whole(m, sim, texts, got, sep):
    corpus = np.frombuffer(b"".join(texts), dtype=np.uint8).copy()
    offs = np.cumsum([0] + [len(t) for t in texts]).astype(np.uint64)
    mh, mdho = m.match_batch(corpus, offs, sep=bitarray(sep))
    for s, t in enumerate(texts):
        assert np.array_equal(got[s], sim.whole(t)), s
        assert np.array_equal(got[s], mh[int(mdho[s]):int(mdho[s + 1])]), s  # aha_ac_match_batch of the whole, same sep


@pytest.fixture(params=VARIANTS)
def variant(request, monkeypatch):
    return use_variant(request.param, monkeypatch)


def test_feed_sep_parity(variant):
    rng = random.Random(zlib.crc32(f"feedsep/{variant}".encode()))
    keys = KEYSETS[VARIANT_KEYSET[variant]](rng)
    sep = SEPS[sorted(SEPS)[VARIANTS.index(variant) % len(SEPS)]]
    m, o = AC.compile(keys), orc.AC.compile(keys)
    W = o.max_key_len + 1
    texts = [_text(rng, keys, rng.randint(1024, 4096)) for _ in range(4)]
    sim = FeedSepSim(o, 4, sep)
    f = m.feed(4, sep=bitarray(sep))
    got = _feed_all(f, sim, texts, rng, W)
    _check_whole(m, sim, texts, got, sep)
    f.close()


def test_feed_sep_every_cut():
    """keys that end exactly at the cut, followed by a separator, by a non-separator, or by the sequence's end"""
    keys = [b"error", b"err", b"or", b"terrors", b"rr", b"s", b"warn: error"]
    sep = SEPS["punct"]
    m, o = AC.compile(keys), orc.AC.compile(keys)
    unit = b"error: terrors or errs warn: error,error err.s rr "
    text = (unit * 6)[:297] + b"err"  # (the sequence ends with a key)
    sim = FeedSepSim(o, 1, sep)
    want = sim.whole(text)
    assert 0 < len(want) < len(o.match(text)) and want["end"][-1] == len(text)
    f = m.feed(1, sep=bitarray(sep))
    for cut in range(len(text) + 1):
        a, pa, ba = _call(f, [text[:cut]], [0], use_device=bool(cut & 1))
        b, pb, bb = _call(f, [text[cut:]], [0], use_device=not (cut & 1))
        c, sho, bc = _finish(f, [0], use_device=bool(cut & 2))
        for h, piece in ((a, text[:cut]), (b, text[cut:])):
            assert np.array_equal(h, sim.piece(0, piece)[0]), cut
        assert np.array_equal(c, sim.finish(0)[0]) and len(c) >= 1, cut
        assert (int(ba[0]), int(bb[0]), int(bc[0])) == (0, cut, len(text)) and sho.tolist() == [0, len(c)]
        assert np.array_equal(np.concatenate([a, absolute(b, cut), absolute(c, len(text))]), want), cut


def test_feed_sep_folded_handle():
    """mixed-case neighbours either side of a cut: the filter tests fold(c), so with 'e' a non-separator 'E' is none either"""
    keys = ["Error", "WARN", "rr"]
    sep = (0x60, sorted(set(b" :.") | set(range(0x41, 0x5B))))  # 'A'..'Z' are set, but fold(c) -- lower case, >= 0x60 -- is tested
    sep_lower = (0x80, sorted(set(b" :.")))
    m = AC.compile(keys, fold_ascii=True)
    o = orc.AC.compile([k.lower() for k in keys])
    text = b"ERROR: tErrors Warn.warN xERRORx error:WARNerror Error"
    for sp in (sep, sep_lower):
        sim = FeedSepSim(o, 1, sp, fold=True)
        want = sim.whole(text)
        assert len(want) > 3
        f = m.feed(1, sep=bitarray(sp))
        for cut in range(len(text) + 1):
            a, _, _ = _call(f, [text[:cut]], [0], use_device=bool(cut & 1))
            b, _, _ = _call(f, [text[cut:]], [0], use_device=not (cut & 1))
            c, _, _ = _finish(f, [0], use_device=False)
            assert np.array_equal(np.concatenate([a, absolute(b, cut), absolute(c, len(text))]), want), cut
        mh, _ = m.match_batch(np.frombuffer(text, np.uint8), np.array([0, len(text)], np.uint64), sep=bitarray(sp))
        assert np.array_equal(mh, want)


def _small_case(seed, sep="punct"):
    rng = random.Random(seed)
    keys = KEYSETS["ascii"](rng) + [b"x" * 40, b"a", b"q"]
    m, o = AC.compile(keys), orc.AC.compile(keys)
    texts = [_text(rng, keys, 4000) for _ in range(4)]
    return rng, keys, m, o, texts, SEPS[sep]


def test_feed_sep_count_equals_match_and_accumulates():
    import torch

    rng, keys, m, o, texts, sep = _small_case(21)
    K = len(keys)
    sim = FeedSepSim(o, 4, sep)
    f = m.feed(4, sep=bitarray(sep))
    got = _feed_all(f, sim, texts, rng, o.max_key_len + 1, counts=np.zeros(K, np.uint64))  # mixed match and count calls
    _check_whole(m, sim, texts, got, sep)
    # AHA_COUNT_ACCUMULATE: running totals over calls, host and device form; finish hits are not counted by count calls
    total = np.zeros(K, dtype=np.uint64)
    dkc = torch.zeros(K, dtype=torch.int64, device="cuda:0")
    want = np.zeros(K, dtype=np.uint64)
    for a in range(0, 4000, 1000):
        pieces = [t[a:a + 1000] for t in texts]
        hs = [sim.piece(s, p)[0] for s, p in enumerate(pieces)]
        want += np.bincount(np.concatenate(hs)["value"], minlength=K).astype(np.uint64)
        corpus = np.frombuffer(b"".join(pieces), np.uint8).copy()
        offs = np.cumsum([0] + [len(p) for p in pieces]).astype(np.uint64)
        if a % 2000 == 0:
            kc, pho, _ = f.count_batch(corpus, offs, np.arange(4, dtype=np.uint32), accumulate_into=total)
            assert kc is total and pho.tolist() == np.cumsum([0] + [len(h) for h in hs]).tolist()
        else:
            n = f.count_batch_device(_device(corpus), _device(offs.view(np.int64)), _device(np.arange(4, dtype=np.int32)), dkc,
                                     accumulate=True)
            assert n == sum(len(h) for h in hs)
    assert np.array_equal(total + dkc.cpu().numpy().view(np.uint64), want) and want.sum() > 0
    # without key counts: the total and the offsets only
    n = C.c_uint64(0)
    piece = np.frombuffer(b" a q ", np.uint8).copy()
    offs = np.array([0, piece.size], np.uint64)
    ids = np.array([2], np.uint32)
    pho = np.zeros(2, np.uint64)
    assert N.lib().aha_feed_count_batch(f._h, piece.ctypes.data, offs.ctypes.data, ids.ctypes.data, 1, 0, None, pho.ctypes.data, None,
                                        C.byref(n)) == 0
    assert n.value == len(sim.piece(2, b" a q ")[0]) == pho[1]


def test_feed_sep_capacity_leaves_feed_unchanged():
    import torch

    rng, keys, m, o, texts, sep = _small_case(22)
    sim = FeedSepSim(o, 4, sep)
    f = m.feed(4, sep=bitarray(sep))
    first = [t[:777] + b" q" for t in texts]  # (a key ends with every piece: an edge hit for the next call)
    _call(f, first, [0, 1, 2, 3], use_device=False)
    for s in range(4):
        sim.piece(s, first[s])
    pieces = [b" " + texts[s][777:777 + 701 * (s + 1)] + b" a" for s in (2, 0, 3)]  # (the separator lets " q" survive)
    ids = [2, 0, 3]
    want = [sim.piece(s, p)[0] for s, p in zip(ids, pieces)]
    required = sum(len(w) for w in want)
    assert all(len(w) and w["end"][0] == 0 for w in want)
    corpus = np.frombuffer(b"".join(pieces), np.uint8).copy()
    offs = np.cumsum([0] + [len(p) for p in pieces]).astype(np.uint64)
    ids_a = np.array(ids, np.uint32)
    for cap in (required - 1, 0):
        out = torch.full((max(cap, 1), 3), 0x5A5A5A5A, dtype=torch.int32, device="cuda:0")
        pho_t = torch.full((4,), 0x5A5A5A5A, dtype=torch.int64, device="cuda:0")
        with pytest.raises(AhaError) as e:
            f.match_batch_device(_device(corpus), _device(offs.view(np.int64)), _device(ids_a.view(np.int32)), out[:cap], pho_t)
        assert e.value.code == N.AHA_E_CAPACITY and e.value.required == required
        assert (out == 0x5A5A5A5A).all() and (pho_t == 0x5A5A5A5A).all()
        hout = np.full(3 * max(cap, 1), 0x5A5A5A5A, dtype=np.int32)
        n = C.c_uint64(0)
        rc = N.lib().aha_feed_match_batch(f._h, corpus.ctypes.data, offs.ctypes.data, ids_a.ctypes.data, 3, hout.ctypes.data, cap,
                                          None, None, C.byref(n))
        assert rc == N.AHA_E_CAPACITY and n.value == required and (hout == 0x5A5A5A5A).all()
        assert [f.position(s)[0] for s in range(4)] == [779] * 4
    hits, pho, bases = _call(f, pieces, ids, use_device=True, cap=required)
    assert np.array_equal(hits, np.concatenate(want)) and bases.tolist() == [779] * 3
    # finish: every sequence ends with a key
    wantf = [sim.finish(s) for s in (1, 3, 0)]
    need = sum(len(w[0]) for w in wantf)
    assert need >= 3
    lens = [f.position(s)[0] for s in range(4)]
    it = _device(np.array([1, 3, 0], np.int32))
    out = torch.full((need, 3), 0x5A5A5A5A, dtype=torch.int32, device="cuda:0")
    with pytest.raises(AhaError) as e:
        f.finish_batch_device(it, out[:need - 1])
    assert e.value.code == N.AHA_E_CAPACITY and e.value.required == need and (out == 0x5A5A5A5A).all()
    n = C.c_uint64(0)
    ids_f = np.array([1, 3, 0], np.uint32)
    hout = np.zeros(need, dtype=HIT_DTYPE)
    assert N.lib().aha_feed_finish_batch(f._h, ids_f.ctypes.data, 3, hout.ctypes.data, need - 1, None, None, C.byref(n)) == N.AHA_E_CAPACITY
    assert n.value == need and [f.position(s)[0] for s in range(4)] == lens  # the sequences have not restarted
    hits, sho, bases = _finish(f, [1, 3, 0], use_device=True, cap=need)
    assert np.array_equal(hits, np.concatenate([w[0] for w in wantf])) and bases.tolist() == [w[1] for w in wantf]
    assert [f.position(s)[0] for s in range(4)] == [0, 0, lens[2], 0]


def test_feed_sep_refusals_and_reset():
    import torch

    rng, keys, m, o, texts, sep = _small_case(23)
    sim = FeedSepSim(o, 4, sep)
    f = m.feed(4, sep=bitarray(sep))
    first = [t[:500] + b" q" for t in texts]
    _call(f, first, [0, 1, 2, 3], use_device=True)
    for s in range(4):
        sim.piece(s, first[s])
    # a sequence named twice, an id out of range: host and device form, nothing restarts
    out = torch.zeros((64, 3), dtype=torch.int32, device="cuda:0")
    for ids in ([1, 1], [0, 4], [2, 3, 2]):
        with pytest.raises(AhaError) as e:
            f.finish_batch(np.array(ids, np.uint32))
        assert e.value.code == N.AHA_E_INVALID
        with pytest.raises(AhaError) as e:
            f.finish_batch_device(_device(np.array(ids, np.int32)), out)
        assert e.value.code == N.AHA_E_INVALID
        assert [f.position(s)[0] for s in range(4)] == [502] * 4
    # cover and select calls are refused, host and device form, and name the follow-up
    piece = np.frombuffer(texts[0][500:900], np.uint8).copy()
    offs = np.array([0, piece.size], np.uint64)
    ids = np.array([0], np.uint32)
    for call in (lambda: f.cover_batch(piece, offs, ids), lambda: f.select_batch(piece, offs, ids),
                 lambda: f.cover_batch_device(_device(piece), _device(offs.view(np.int64)), _device(ids.view(np.int32)),
                                              mask=torch.zeros(16, dtype=torch.int32, device="cuda:0")),
                 lambda: f.select_batch_device(_device(piece), _device(offs.view(np.int64)), _device(ids.view(np.int32)), out)):
        with pytest.raises(AhaError) as e:
            call()
        assert e.value.code == N.AHA_E_INVALID and "follow-up" in str(e.value)
        assert f.position(0)[0] == 502
    # ... and the feed goes on as if nothing had happened: the edge hit " q" left is still found
    hits, _, _ = _call(f, [texts[0][500:900]], [0], use_device=False)
    want = sim.piece(0, texts[0][500:900])[0]
    assert np.array_equal(hits, want)
    # finish on a plain feed is refused
    g = m.feed(2)
    with pytest.raises(AhaError) as e:
        g.finish_batch(np.array([0], np.uint32))
    assert e.value.code == N.AHA_E_INVALID
    with pytest.raises(AhaError) as e:
        g.finish_batch_device(_device(np.array([0], np.int32)), out)
    assert e.value.code == N.AHA_E_INVALID
    # reset drops the hits that ended with the last byte: sequence 1 ends with " q"
    assert sim.piece(1, b" ")[0].tolist() == [(-1, 0, keys.index(b"q"))]  # (what the next call would have reported)
    f.reset(1)
    sim.reset(1)
    hits, _, bases = _call(f, [b" a "], [1], use_device=True)
    assert np.array_equal(hits, sim.piece(1, b" a ")[0]) and hits.tolist() == [(1, 2, keys.index(b"a"))] and int(bases[0]) == 0
    # n_named = 0 and a sequence of length 0
    hits, sho, _ = _finish(f, [], use_device=False)
    assert len(hits) == 0 and sho.tolist() == [0]
    f.reset(3)
    hits, sho, bases = _finish(f, [3], use_device=True)
    assert len(hits) == 0 and sho.tolist() == [0, 0] and bases.tolist() == [0]


def _many_hits():
    """23 nested a-keys over runs of a: 3 pieces with more than 2^20 unfiltered hits; a space every 29 bytes keeps the keys
    that span a whole run or touch the sequence's ends.  The expected hits come from the oracle, once."""
    keys = [b"a" * i for i in range(1, 24)]
    sep = SEPS["punct"]
    m, o = AC.compile(keys), orc.AC.compile(keys)
    unit = b"a" * 23 + b" " + b"a" * 4 + b" "  # whole runs of 23 and of 4 survive
    texts = [(unit * 1400)[:n] for n in (42001, 41411, 40999)]
    first = 5000
    sim = FeedSepSim(o, 3, sep)
    want1 = [sim.piece(s, t[:first])[0] for s, t in enumerate(texts)]
    want2 = [sim.piece(s, t[first:])[0] for s, t in enumerate(texts)]
    n_true = sum(len(o.match(t)) - len(o.match(t[:first])) for t in texts)
    assert n_true >= 1 << 20
    return keys, sep, texts, first, want1, want2, [sim.finish(s)[0] for s in range(3)]


@pytest.fixture(scope="module")
def many_hits():
    return _many_hits()


@pytest.mark.parametrize("reduced", [False, True], ids=["full", "reserve_cus"])
def test_feed_sep_many_hits(many_hits, reduced, monkeypatch):
    if reduced:
        monkeypatch.setenv("AHA_RESERVE_CUS", "1")
    keys, sep, texts, first, want1, want2, wantf = many_hits
    m = AC.compile(keys)
    f = m.feed(3, sep=bitarray(sep))
    hits, pho, _ = _call(f, [t[:first] for t in texts], [0, 1, 2], use_device=True)
    assert np.array_equal(hits, np.concatenate(want1))
    tails = [t[first:] for t in texts]
    kc, cpho, _, _ = _count_call(m.feed(3, sep=bitarray(sep)), texts, [0, 1, 2], True, len(keys))  # (a second feed, whole sequences)
    hits, pho, bases = _call(f, tails, [0, 1, 2], use_device=True)  # one call: > 2^20 true hits over 3 pieces
    assert pho.tolist() == np.cumsum([0] + [len(w) for w in want2]).tolist() and bases.tolist() == [first] * 3
    assert np.array_equal(hits, np.concatenate(want2))
    allh = np.concatenate(want1 + want2)
    assert np.array_equal(kc, np.bincount(allh["value"], minlength=len(keys)).astype(np.uint64))
    assert cpho.tolist() == np.cumsum([0] + [len(a) + len(b) for a, b in zip(want1, want2)]).tolist()
    hits, sho, _ = _finish(f, [0, 1, 2], use_device=True)
    assert np.array_equal(hits, np.concatenate(wantf)) and sho[-1] == len(hits)


def test_feed_sep_on_a_side_stream():
    import torch

    rng, keys, m, o, texts, sep = _small_case(24, sep="low")
    s = torch.cuda.Stream()
    sim = FeedSepSim(o, 4, sep)
    f = m.feed(4, sep=bitarray(sep))
    with torch.cuda.stream(s):
        got = _feed_all(f, sim, texts, rng, o.max_key_len + 1, device_every=1, stream=s.cuda_stream)
        ids = _device(np.array([0], np.int32))
        out = torch.zeros((8, 3), dtype=torch.int32, device="cuda:0")
        assert f.finish_batch_device(ids, out, stream=s.cuda_stream) == 0  # (already finished: length 0)
    _check_whole(m, sim, texts, got, sep)
