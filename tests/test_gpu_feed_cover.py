"""Feed cover (aha_feed_cover_batch*) on the GPU: sequences fed in pieces give, call by call, the mask, the redacted bytes,
piece_back, piece_covered, offsets, bases and totals that the contract derives from the oracle's hits of each WHOLE sequence
(tests/feedcoversim.py piece_truth), and by the stream law the oracle's redaction of the whole -- on every engine variant, on
byte and char feeds, through host and device entries.  Beside parity: pieces that share mask words, a piece beyond one bit
tile of the main pass, a folded handle, redaction in place, all outputs NULL, one-byte keys, match / count / cover calls mixed
on one feed, failed calls that change nothing, no hit list of the main pass, a side stream, two threads, and Feed.redactor."""
import ctypes as C
import random
import threading
import zlib

import numpy as np
import pytest

import pyoracle as orc
from aha_amd import AC, AhaError, HIT_DTYPE
from aha_amd import _native as N
from coversim import mask_words, redacted as redact_np, unpack
from engine_variants import VARIANTS, use_variant
from feedcoversim import piece_truth, reassemble, spans_cover
from feedsim import FeedSim, leads
from test_gpu_feed import _call, _device, _keys_nested, _keys_single, _next_len, _text
from test_gpu_feed_count import _count_call

pytestmark = pytest.mark.gpu

FILL = 0x2A
GUARD = 0x5A5A5A5A
PAD = 8


def _keys16(rng):
    """keys of at most 16 bytes: W = 15"""
    words = sorted({"".join(rng.choice("abcdefgh") for _ in range(rng.randint(3, 9))) for _ in range(300)})
    keys = ([w.encode() for w in words] + [b"a" * i for i in range(1, 17)] + [("我" * i).encode() for i in range(1, 6)]
            + [b"ba", b"bab", b"q\x80"])
    return list(dict.fromkeys(keys))


def _whole(o, t):
    return o.match(bytes(t)) if t else np.zeros(0, dtype=HIT_DTYPE)


def _cover_call(f, pieces, ids, use_device, fill=FILL, stream=None, in_place=False):
    """one feed cover call with every output asked for -> dict; the device form checks the words behind each output"""
    import torch

    corpus = np.frombuffer(b"".join(pieces), dtype=np.uint8).copy()
    offs = np.cumsum([0] + [len(p) for p in pieces]).astype(np.uint64)
    ids = np.array(ids, dtype=np.uint32)
    D, n = len(pieces), corpus.size
    nw = (n + 31) // 32
    if not use_device:
        L = N.lib()
        mask = np.zeros(nw, dtype=np.uint32)
        red = np.zeros(n, dtype=np.uint8)
        back = np.zeros(max(D, 1), dtype=np.uint32)
        cov = np.zeros(max(D, 1), dtype=np.uint64)
        pho = np.zeros(D + 1, dtype=np.uint64)
        bases = np.zeros(max(D, 1), dtype=np.uint64)
        nc, nh = C.c_uint64(0), C.c_uint64(0)
        rc = L.aha_feed_cover_batch(f._h, corpus.ctypes.data, offs.ctypes.data, ids.ctypes.data, D, 0, mask.ctypes.data,
                                    red.ctypes.data, fill, back.ctypes.data, cov.ctypes.data, pho.ctypes.data, bases.ctypes.data,
                                    C.byref(nc), C.byref(nh))
        f._check(rc)
        return dict(mask=mask, red=red, back=back[:D], cov=cov[:D], pho=pho, bases=bases[:D], nc=nc.value, nh=nh.value)
    dev = "cuda:0"
    ct, ot, it = _device(corpus), _device(offs.view(np.int64)), _device(ids.view(np.int32))
    mask = torch.full((nw + PAD,), GUARD, dtype=torch.int32, device=dev)
    red = ct if in_place else torch.full((n + PAD,), 0x5A, dtype=torch.uint8, device=dev)
    back = torch.full((D + PAD,), GUARD, dtype=torch.int32, device=dev)
    cov = torch.full((D + PAD,), GUARD, dtype=torch.int64, device=dev)
    pho = torch.full((D + 1 + PAD,), GUARD, dtype=torch.int64, device=dev)
    bases = torch.full((D + PAD,), GUARD, dtype=torch.int64, device=dev)
    nc, nh = f.cover_batch_device(ct, ot, it, mask=mask, redacted=red, fill=fill, piece_back=back, piece_covered=cov,
                                  piece_hit_offsets=pho, piece_bases=bases, stream=stream)
    torch.cuda.synchronize()
    for t, k in ((mask, nw), (back, D), (cov, D), (pho, D + 1), (bases, D)):
        assert bool((t[k:] == GUARD).all()), "a word behind an output was written"
    if not in_place:
        assert bool((red[n:] == 0x5A).all())
    return dict(mask=mask[:nw].cpu().numpy().view(np.uint32), red=red[:n].cpu().numpy(),
                back=back[:D].cpu().numpy().view(np.uint32), cov=cov[:D].cpu().numpy().view(np.uint64),
                pho=pho[:D + 1].cpu().numpy().view(np.uint64), bases=bases[:D].cpu().numpy().view(np.uint64), nc=nc, nh=nh)


def _want_call(wholes, texts, pos, pieces, ids, chars=False, fill=FILL):
    """the contract for one call, from the whole sequences' hits; pos[s]: bytes of sequence s before the call"""
    covs, backs, counts, bases = [], [], [], []
    for d, s in enumerate(ids):
        cov, back, n = piece_truth(wholes[s], pos[s], len(pieces[d]))
        covs.append(cov)
        backs.append(back)
        counts.append(n)
        bases.append(leads(texts[s][:pos[s]]) if chars else pos[s])
    cover = np.concatenate(covs) if covs else np.zeros(0, dtype=bool)
    corpus = np.frombuffer(b"".join(pieces), dtype=np.uint8)
    return dict(mask=mask_words(cover), red=redact_np(corpus, cover, fill), back=backs, cov=[int(c.sum()) for c in covs],
                pho=np.cumsum([0] + counts).tolist(), bases=bases, nc=int(cover.sum()), nh=sum(counts))


def _assert_call(got, want, where=None):
    assert np.array_equal(got["mask"], want["mask"]), where
    assert np.array_equal(got["red"], want["red"]), where
    assert got["back"].tolist() == want["back"], where
    assert got["cov"].tolist() == want["cov"], where
    assert got["pho"].tolist() == want["pho"], where
    assert got["bases"].tolist() == want["bases"], where
    assert (got["nc"], got["nh"]) == (want["nc"], want["nh"]), where


def _adversarial(W):
    return [max(v, 0) for v in (0, 1, W - 1, W, W + 1, 2 * W - 1, 2 * W, 2 * W + 1)]


def _cover_all(m, o, texts, chars, rng, f=None, device_every=2, stream=None, fill=FILL):
    """covers texts over several calls (shuffled subsets of the sequences; the adversarial lengths, a run of pieces shorter than
    a key, then random cuts); checks every call against the contract and the whole against the stream law"""
    S, W = len(texts), max(o.max_key_len - 1, 0)
    f = f or m.feed(S, chars=chars)
    wholes = [_whole(o, t) for t in texts]
    pos = [0] * S
    steps = [0] * S
    reds, backs = [[] for _ in range(S)], [[] for _ in range(S)]
    fixed = _adversarial(W) + [rng.randint(1, 5) for _ in range(12)]
    call = 0
    while any(pos[s] < len(texts[s]) for s in range(S)) or call < 2:
        ids = [s for s in range(S) if rng.random() < 0.75]
        rng.shuffle(ids)
        pieces = []
        for s in ids:
            n = fixed[steps[s]] if steps[s] < len(fixed) else _next_len(rng, texts[s], pos[s], W)
            steps[s] += 1
            pieces.append(texts[s][pos[s]:pos[s] + n])
        want = _want_call(wholes, texts, pos, pieces, ids, chars, fill)
        got = _cover_call(f, pieces, ids, use_device=(call % device_every == 1), fill=fill, stream=stream)
        _assert_call(got, want, call)
        a = 0
        for d, s in enumerate(ids):
            reds[s].append(got["red"][a:a + len(pieces[d])])
            backs[s].append(int(got["back"][d]))
            a += len(pieces[d])
            pos[s] += len(pieces[d])
        for s in set(ids):
            nb, nc = f.position(s)
            assert nb == pos[s] and (not chars or nc == leads(texts[s][:pos[s]]))
        call += 1
    for s, t in enumerate(texts):
        cover = spans_cover(wholes[s]["start"], wholes[s]["end"], len(t))
        assert reassemble(reds[s], backs[s], fill) == redact_np(np.frombuffer(t, dtype=np.uint8), cover, fill).tobytes(), s
    return f


@pytest.fixture(params=VARIANTS)
def variant(request, monkeypatch):
    return use_variant(request.param, monkeypatch)


@pytest.mark.parametrize("chars", [False, True], ids=["bytes", "chars"])
def test_feed_cover_parity(variant, chars):
    rng = random.Random(zlib.crc32(f"feedcover/{variant}/{chars}".encode()))
    keys = _keys16(rng)
    m, o = AC.compile(keys), orc.AC.compile(keys)
    assert o.max_key_len == 16
    S = rng.randint(3, 5)
    texts = [_text(rng, keys, rng.choice([700, 5000, 40000, 200000])) for _ in range(S)]
    texts[0] = b"\x80\x00" + "中国".encode()[:4] + texts[0] + b"\xbf"
    f = _cover_all(m, o, texts, chars, rng)
    m.redact(texts[0])  # (the plain call on the same handle still answers)
    f.close()


def _small_case(seed, n=20000, S=4):
    rng = random.Random(seed)
    keys = _keys16(rng)
    m, o = AC.compile(keys), orc.AC.compile(keys)
    texts = [_text(rng, keys, n) for _ in range(S)]
    return rng, keys, m, o, texts


def test_feed_cover_neighbours_share_mask_words():
    """24 pieces of 1 to 40 bytes, each of another sequence with a context of its own: wholly covered, not at all, mixed.  The
    clear of one piece's first W bits and the window spans of its neighbour meet in the same mask words."""
    rng = random.Random(31)
    keys = _keys16(rng)
    m, o = AC.compile(keys), orc.AC.compile(keys)
    S = 24
    kinds = [b"a", b"Q", None]
    ctxs, nexts = [], []
    for s in range(S):
        kind = kinds[s % 3]
        n = rng.randint(1, 40)
        ctxs.append(_text(rng, keys, rng.randint(0, 30)) + (b"aaaaaaa" if s % 2 else b"abcdefg"[:rng.randint(0, 7)]))
        nexts.append(kind * n if kind else _text(rng, keys, n))
    texts = [c + p for c, p in zip(ctxs, nexts)]
    wholes = [_whole(o, t) for t in texts]
    for use_device in (False, True):
        f = m.feed(S)
        order = list(range(S))
        rng.shuffle(order)
        got = _cover_call(f, [ctxs[s] for s in order], order, use_device)
        _assert_call(got, _want_call(wholes, texts, [0] * S, [ctxs[s] for s in order], order))
        rng.shuffle(order)
        pos = [len(c) for c in ctxs]
        got = _cover_call(f, [nexts[s] for s in order], order, use_device)
        want = _want_call(wholes, texts, pos, [nexts[s] for s in order], order)
        _assert_call(got, want)
        assert any(c == len(nexts[s]) for c, s in zip(want["cov"], order)) and any(c == 0 for c in want["cov"])
        assert any(want["back"])
        n = sum(len(p) for p in nexts)
        assert not np.unpackbits(got["mask"].view(np.uint8), bitorder="little")[n:].any()
        f.close()


def test_feed_cover_piece_beyond_one_bit_tile():
    """one piece of about 300 KiB beside small ones: the main pass's spans cross a 256 KiB tile group; hits within W of the
    piece's start (straddling the cut) and of its end"""
    rng, keys, m, o, _ = _small_case(32, n=10)
    big = b"aaaaaaaaaa" + _text(rng, keys, 300 * 1024 + 77) + b"abcaaaaaaaaaaaa"
    texts = [b"zz" + b"a" * 9 + big + b"aaaa q", _text(rng, keys, 900), _text(rng, keys, 50)]
    wholes = [_whole(o, t) for t in texts]
    f = m.feed(3)
    calls = [([texts[0][:11], texts[1][:400]], [0, 1]),
             ([texts[1][400:], texts[0][11:11 + len(big)], texts[2]], [1, 0, 2]),
             ([texts[0][11 + len(big):]], [0])]
    pos = [0, 0, 0]
    for k, (pieces, ids) in enumerate(calls):
        got = _cover_call(f, pieces, ids, use_device=True)
        want = _want_call(wholes, texts, pos, pieces, ids)
        _assert_call(got, want, k)
        for p, s in zip(pieces, ids):
            pos[s] += len(p)
        if k:
            assert want["back"][ids.index(0)] > 0
    f.close()


def test_feed_cover_folded_handle():
    """a folded handle: the hits are those of the folded text, a hit straddles the cut, and outside the mask redacted holds the
    caller's bytes as they were spelled"""
    keys = [b"Secret", b"pass WORD", b"k"]
    m = AC.compile(keys, fold_ascii=True)
    o = orc.AC.compile([k.lower() for k in keys])
    text = b"My SeCrEt is a PASS word, Ok? The pAsS wOrD: seCRET. KkK MIXED Case stays"
    whole = _whole(o, text.lower())
    cover = spans_cover(whole["start"], whole["end"], len(text))
    want = redact_np(np.frombuffer(text, dtype=np.uint8), cover, FILL).tobytes()
    for use_device in (False, True):
        for cut in (5, 17, 19, 37, 40):  # inside "SeCrEt", "PASS word", "pAsS wOrD"
            f = m.feed(1)
            pieces = [text[:cut], text[cut:cut + 3], text[cut + 3:]]
            pos, reds, backs = 0, [], []
            for p in pieces:
                got = _cover_call(f, [p], [0], use_device)
                _assert_call(got, _want_call([whole], [text], [pos], [p], [0]), (cut, pos))
                keep = ~unpack(got["mask"], len(p))
                assert np.array_equal(got["red"][keep], np.frombuffer(p, dtype=np.uint8)[keep])
                reds.append(got["red"])
                backs.append(int(got["back"][0]))
                pos += len(p)
            assert reassemble(reds, backs, FILL) == want
            assert any(backs)
            f.close()


def test_feed_cover_in_place_on_the_device():
    import torch

    rng, keys, m, o, texts = _small_case(33)
    wholes = [_whole(o, t) for t in texts]
    f, g = m.feed(4), m.feed(4)
    pos = [0] * 4
    for k in range(3):
        ids = [2, 0, 3]
        pieces = [texts[s][pos[s]:pos[s] + 3000 + 17 * s] for s in ids]
        a = _cover_call(f, pieces, ids, use_device=True)
        b = _cover_call(g, pieces, ids, use_device=True, in_place=True)
        _assert_call(a, _want_call(wholes, texts, pos, pieces, ids), k)
        _assert_call(b, a | {k2: a[k2].tolist() for k2 in ("back", "cov", "pho", "bases")}, k)
        for p, s in zip(pieces, ids):
            pos[s] += len(p)
    # a call that fails (a sequence named twice) leaves the corpus buffer as it was
    piece = np.frombuffer(texts[1][:2000], dtype=np.uint8).copy()
    ct = _device(piece)
    with pytest.raises(AhaError) as e:
        g.cover_batch_device(ct, _device(np.array([0, 1000, 2000], np.int64)), _device(np.array([1, 1], np.int32)), redacted=ct)
    assert e.value.code == N.AHA_E_INVALID
    torch.cuda.synchronize()
    assert np.array_equal(ct.cpu().numpy(), piece) and g.position(1)[0] == 0
    f.close()
    g.close()


def test_feed_cover_null_outputs_and_w0():
    rng, keys, m, o, texts = _small_case(34)
    wholes = [_whole(o, t) for t in texts]
    L = N.lib()
    f = m.feed(4)
    pos = [0] * 4
    for use_device in (False, True):
        ids = [1, 3]
        pieces = [texts[s][pos[s]:pos[s] + 2500] for s in ids]
        want = _want_call(wholes, texts, pos, pieces, ids)
        corpus = np.frombuffer(b"".join(pieces), dtype=np.uint8).copy()
        offs = np.array([0, 2500, 5000], dtype=np.uint64)
        idv = np.array(ids, dtype=np.uint32)
        nc, nh = C.c_uint64(0), C.c_uint64(0)
        if use_device:
            ct, ot, it = _device(corpus), _device(offs.view(np.int64)), _device(idv.view(np.int32))
            rc = L.aha_feed_cover_batch_device(f._h, ct.data_ptr(), ot.data_ptr(), it.data_ptr(), 2, 5000, 0, None, None, FILL,
                                               None, None, None, None, C.byref(nc), C.byref(nh), None)
        else:
            rc = L.aha_feed_cover_batch(f._h, corpus.ctypes.data, offs.ctypes.data, idv.ctypes.data, 2, 0, None, None, FILL, None,
                                        None, None, None, C.byref(nc), C.byref(nh))
        assert rc == N.AHA_OK and (nc.value, nh.value) == (want["nc"], want["nh"])
        for s in ids:
            pos[s] += 2500
            assert f.position(s)[0] == pos[s]
        # n_hits may be NULL; N = 0 and D = 0 are valid
        rc = L.aha_feed_cover_batch(f._h, None, np.zeros(1, np.uint64).ctypes.data, None, 0, 0, None, None, FILL, None, None,
                                    None, None, C.byref(nc), None)
        assert rc == N.AHA_OK and nc.value == 0
    # the feed is where a feed that covered with every output would be
    got = _cover_call(f, [texts[1][pos[1]:pos[1] + 900], b""], [1, 0], True)
    _assert_call(got, _want_call(wholes, texts, pos, [texts[1][pos[1]:pos[1] + 900], b""], [1, 0]))
    f.close()
    # W = 0: one-byte keys, back is always 0
    keys1 = _keys_single(rng)
    m1, o1 = AC.compile(keys1), orc.AC.compile(keys1)
    t1 = [_text(rng, keys1, 3000) for _ in range(3)]
    w1 = [_whole(o1, t) for t in t1]
    f1 = m1.feed(3)
    pos = [0] * 3
    for k in range(6):
        ids = [2, 0, 1]
        pieces = [t1[s][pos[s]:pos[s] + (k * 211) % 700 + s] for s in ids]
        got = _cover_call(f1, pieces, ids, use_device=bool(k % 2))
        _assert_call(got, _want_call(w1, t1, pos, pieces, ids), k)
        assert not got["back"].any()
        for p, s in zip(pieces, ids):
            pos[s] += len(p)
    f1.close()


@pytest.mark.parametrize("chars", [False, True], ids=["bytes", "chars"])
def test_feed_cover_match_and_count_mixed(chars):
    """match, count and cover calls interleaved on one feed, match alone on a twin: the positions, the contexts' effect and
    every later result agree"""
    rng, keys, m, o, texts = _small_case(35)
    wholes = [_whole(o, t) for t in texts]
    K = m.n_keys
    f, twin = m.feed(4, chars=chars), m.feed(4, chars=chars)
    sim = FeedSim(o, 4, chars)
    pos = [0] * 4
    call = 0
    while any(pos[s] < len(texts[s]) for s in range(4)):
        ids = [s for s in range(4) if rng.random() < 0.75]
        rng.shuffle(ids)
        pieces = [texts[s][pos[s]:pos[s] + _next_len(rng, texts[s], pos[s], sim.W)] for s in ids]
        use_device = (call // 3) % 2 == 1
        want = [sim.piece(s, p) for s, p in zip(ids, pieces)]
        want_hits = np.concatenate([w[0] for w in want]) if want else np.zeros(0, HIT_DTYPE)
        t_hits, t_pho, t_bases = _call(twin, pieces, ids, use_device)
        assert np.array_equal(t_hits, want_hits)
        if call % 3 == 0:
            hits, pho, bases = _call(f, pieces, ids, use_device)
            assert np.array_equal(hits, t_hits)
        elif call % 3 == 1:
            kc, pho, bases, n = _count_call(f, pieces, ids, use_device, K)
            assert n == len(t_hits)
        else:
            got = _cover_call(f, pieces, ids, use_device)
            _assert_call(got, _want_call(wholes, texts, pos, pieces, ids, chars), call)
            pho, bases = got["pho"], got["bases"]
        assert pho.tolist() == t_pho.tolist() and bases.tolist() == t_bases.tolist()
        for p, s in zip(pieces, ids):
            pos[s] += len(p)
        for s in range(4):
            assert f.position(s) == twin.position(s)
        call += 1
    f.close()
    twin.close()


def test_feed_cover_failed_calls_change_nothing():
    import torch

    rng, keys, m, o, texts = _small_case(36)
    wholes = [_whole(o, t) for t in texts]
    f = m.feed(4)
    first = _cover_call(f, [texts[1][:500]], [1], True)
    _assert_call(first, _want_call(wholes, texts, [0] * 4, [texts[1][:500]], [1]))
    piece = np.frombuffer(texts[0][:1000], np.uint8).copy()
    # host entry: a sequence named twice
    mask = np.full(32, GUARD, np.uint32)
    red = np.full(1000, 0x5A, np.uint8)
    back = np.full(2, GUARD, np.uint32)
    cov = np.full(2, GUARD, np.uint64)
    pho = np.full(3, GUARD, np.uint64)
    bases = np.full(2, GUARD, np.uint64)
    nc, nh = C.c_uint64(0), C.c_uint64(0)
    rc = N.lib().aha_feed_cover_batch(f._h, piece.ctypes.data, np.array([0, 500, 1000], np.uint64).ctypes.data,
                                      np.array([1, 1], np.uint32).ctypes.data, 2, 0, mask.ctypes.data, red.ctypes.data, FILL,
                                      back.ctypes.data, cov.ctypes.data, pho.ctypes.data, bases.ctypes.data, C.byref(nc), C.byref(nh))
    assert rc == N.AHA_E_INVALID
    for a in (mask, back, cov, pho, bases):
        assert (a == GUARD).all()
    assert (red == 0x5A).all()
    # device entry: checked on the device, before anything is indexed with the offsets or ids
    bad = [
        ([0, 500, 1000], [1, 1]),   # an id twice
        ([0, 600, 500, 1000], [0, 1, 2]),  # not ascending
        ([0, 500, 900], [0, 2]),    # the last offset is not n_bytes
        ([0, 500, 1000], [0, 4]),   # an id >= n_seqs
    ]
    dev = "cuda:0"
    for offs, ids in bad:
        ct = _device(piece)
        D = len(ids)
        outs = dict(mask=torch.full((32,), GUARD, dtype=torch.int32, device=dev),
                    redacted=torch.full((1000,), 0x5A, dtype=torch.uint8, device=dev),
                    piece_back=torch.full((D,), GUARD, dtype=torch.int32, device=dev),
                    piece_covered=torch.full((D,), GUARD, dtype=torch.int64, device=dev),
                    piece_hit_offsets=torch.full((D + 1,), GUARD, dtype=torch.int64, device=dev),
                    piece_bases=torch.full((D,), GUARD, dtype=torch.int64, device=dev))
        with pytest.raises(AhaError) as e:
            f.cover_batch_device(ct, _device(np.array(offs, np.int64)), _device(np.array(ids, np.int32)), **outs)
        assert e.value.code == N.AHA_E_INVALID, (offs, ids)
        torch.cuda.synchronize()
        for k, t in outs.items():
            assert bool((t == (0x5A if k == "redacted" else GUARD)).all()), (offs, ids, k)
        assert np.array_equal(ct.cpu().numpy(), piece)
        assert f.position(1)[0] == 500 and f.position(0)[0] == 0 and f.position(2)[0] == 0
    # a piece that claims 2^31 bytes: refused before anything reads the corpus
    ct = _device(piece)
    rc = N.lib().aha_feed_cover_batch_device(f._h, ct.data_ptr(), _device(np.array([0, 1 << 31], np.int64)).data_ptr(),
                                             _device(np.array([0], np.int32)).data_ptr(), 1, 1 << 31, 0, None, None, FILL, None,
                                             None, None, None, C.byref(nc), C.byref(nh), None)
    assert rc == N.AHA_E_TOO_LONG and f.position(0)[0] == 0
    # the next valid call gives what it would have given without the failed ones
    pos = [0, 500, 0, 0]
    pieces, ids = [texts[0][:500], texts[1][500:1000]], [0, 1]
    _assert_call(_cover_call(f, pieces, ids, True), _want_call(wholes, texts, pos, pieces, ids))
    f.close()


def test_feed_cover_holds_no_main_pass_hit_list():
    """all-'a' pieces under the nested key set: about 23 hits per byte.  The device memory a feed cover call takes (fresh feed,
    scratch released first) stays below what a plain cover of the same pieces takes + 4 N + 4 MiB; a hit list of the main pass
    would be at least 192 N."""
    import torch

    n = 8 << 20
    keys = _keys_nested(random.Random(0))
    o = orc.AC.compile(keys)
    assert o.match(b"a" * 4096).size / 4096 >= 16
    m = AC.compile(keys)
    cuts = [0, 1 << 20, (1 << 20) + 77, 3 << 20, (5 << 20) + 1, (7 << 20) + 4093, n]
    D = len(cuts) - 1
    ct = torch.full((n,), ord("a"), dtype=torch.uint8, device="cuda:0")
    ot = _device(np.array(cuts, np.int64))
    it = _device(np.arange(D, dtype=np.int32))
    torch.cuda.synchronize()

    def growth(call):
        m.release_scratch()
        torch.cuda.synchronize()
        free0 = torch.cuda.mem_get_info()[0]
        out = call()
        torch.cuda.synchronize()
        return free0 - torch.cuda.mem_get_info()[0], out

    plain, (nc, nh) = growth(lambda: m.cover_batch_device(ct, ot))
    assert nc == n and nh >= 16 * n
    f = m.feed(D)
    feed, (fc, fh) = growth(lambda: f.cover_batch_device(ct, ot, it))
    assert (fc, fh) == (nc, nh)
    print(f"device memory: plain cover {plain}, feed cover {feed}, N {n}")
    assert feed <= plain + 4 * n + (4 << 20), (feed, plain)
    f.close()


def test_feed_cover_on_a_side_stream():
    import torch

    rng, keys, m, o, texts = _small_case(37)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        _cover_all(m, o, texts, False, rng, device_every=1, stream=s.cuda_stream).close()


def test_feed_cover_two_threads_one_handle():
    rng, keys, m, o, texts = _small_case(38)
    errors = []

    def worker(k):
        try:
            r = random.Random(300 + k)
            ts = [_text(r, keys, 30000) for _ in range(3)]
            _cover_all(m, o, ts, bool(k), r).close()
        except Exception as e:  # noqa: BLE001 -- reported below
            errors.append(e)

    th = [threading.Thread(target=worker, args=(k,)) for k in range(2)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert not errors, errors


def test_feed_redactor():
    """random cuts of a 10 KiB text: the joined output is matcher.redact(whole), and no push returns a byte that later changes
    (what is handed out is a prefix of the final answer)"""
    rng, keys, m, o, texts = _small_case(39, n=10240, S=2)
    want = [m.redact(t) for t in texts]
    W = o.max_key_len - 1
    f = m.feed(2)
    r = f.redactor()
    out = [b"", b""]
    pos = [0, 0]
    while any(pos[s] < len(texts[s]) for s in range(2)):
        s = rng.randrange(2)
        n = _next_len(rng, texts[s], pos[s], W)
        out[s] += r.push(s, texts[s][pos[s]:pos[s] + n])
        pos[s] += n
        assert want[s].startswith(out[s]) and len(out[s]) >= pos[s] - W
    for s in range(2):
        assert out[s] + r.finish(s) == want[s]
        assert f.position(s)[0] == 0 and r.finish(s) == b""
    assert f.cover(0, b"xxaaa")[1] == 0 and f.redact(1, "bab")[0] == b"***"
    f.close()
