"""Longest feeds (aha_feed_open_params with longest = 1 | 2, aha_feed_finish_batch*) on the GPU, exact against the model
(feedlongestsim: a resumable restatement of match_longest's loop, itself checked against the oracle at every cut in
test_feed_longest_host.py) and against the oracle's match_longest of the whole sequences: every two-piece cut as one feed with
a sequence per cut, byte by byte, the chunked walk with cuts inside chunks and long keys, NULs at value nodes and on cuts, the
give-up to the per-piece walk, stale END flags, a folded handle, failed and refused calls that leave the feed as it was."""
import ctypes as C
import os
import random
import subprocess

import numpy as np
import pytest

import pyoracle as orc
from aha_amd import AC, AhaError, HIT_DTYPE
from aha_amd import _native as N
from feedlongestsim import CASES, FeedLongestSim, absolute, case_keys, case_text, stale_keys
from test_gpu_feed import _call, _device
from test_gpu_feed_sep import _finish

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_CACHE = {}


def cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def rows(h):
    return [(int(x["start"]), int(x["end"]), int(x["value"])) for x in h]


def handle(name):
    def make():
        keys, stale = case_keys(name)
        return keys, stale, AC.compile(keys), orc.AC.compile(keys)
    return cached(("handle", name), make)


def check_call(f, sim, pieces, ids, use_device):
    """one match call against the model: hits, piece_hit_offsets, piece_bases; -> the absolute hits per piece"""
    hits, pho, bases = _call(f, pieces, ids, use_device)
    want = [sim.piece(s, p) for s, p in zip(ids, pieces)]
    assert pho.tolist() == np.cumsum([0] + [len(w[0]) for w in want]).tolist()
    assert bases.tolist() == [w[1] for w in want]
    assert rows(hits) == [r for w in want for r in rows(w[0])]
    return [absolute(hits[int(pho[d]):int(pho[d + 1])], int(bases[d])) for d in range(len(pieces))]


def check_finish(f, sim, ids, use_device):
    hits, sho, bases = _finish(f, ids, use_device)
    want = [sim.finish(s) for s in ids]
    assert sho.tolist() == np.cumsum([0] + [len(w[0]) for w in want]).tolist()
    assert bases.tolist() == [w[1] for w in want]
    assert rows(hits) == [r for w in want for r in rows(w[0])]
    return [absolute(hits[int(sho[d]):int(sho[d + 1])], int(bases[d])) for d in range(len(ids))]


# ---- 1: parity at every cut ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("use_device", [False, True])
@pytest.mark.parametrize("mode", [1, 2])
@pytest.mark.parametrize("name", CASES)
def test_parity_at_every_cut(name, mode, use_device):
    """every two-piece cut of the text as ONE feed with one sequence per cut: two calls of len + 1 pieces and one finish call,
    so the many-pieces-per-call path and the per-piece state work together; then byte by byte on one sequence"""
    keys, stale, m, o = handle(name)
    text = case_text(name, keys)
    isect = mode == 2
    want = rows(o.match_longest(text, intersectable=isect, chars=False))
    S = len(text) + 1
    f = m.feed(S, longest=mode)
    assert f.longest == mode
    sim = FeedLongestSim(keys, S, isect, stale)
    ids = list(range(S))
    a = check_call(f, sim, [text[:c] for c in ids], ids, use_device)
    order = ids[::-1]  # (pieces in any order)
    b = check_call(f, sim, [text[c:] for c in order], order, use_device)
    assert all(f.position(s)[0] == len(text) for s in (0, S // 2, S - 1))
    fin = check_finish(f, sim, ids, use_device)
    for c in ids:
        assert rows(a[c]) + rows(b[S - 1 - c]) + rows(fin[c]) == want, c
    assert f.position(S // 2)[0] == 0  # the sequences started again
    # byte by byte, with an empty piece now and then; the calls up to n plus a finish at n are the oracle on the prefix
    g = m.feed(1, longest=mode)
    gsim = FeedLongestSim(keys, 1, isect, stale)
    got = []
    for i in range(len(text)):
        if i % 7 == 3:
            assert rows(check_call(g, gsim, [b""], [0], use_device)[0]) == []
        got += rows(check_call(g, gsim, [text[i:i + 1]], [0], use_device)[0])
    assert got + rows(check_finish(g, gsim, [0], use_device)[0]) == want


# ---- 2, 3: the chunked walk --------------------------------------------------------------------------------------------------
def dense_text(keys, n, seed, nul=0.0):
    """text dense in hits, so that a pending end sits on most cuts"""
    rng = random.Random(seed)
    keyset = set(keys)
    parents = [k for k in keys if any(o != k and o.startswith(k) for o in keyset)]
    out = bytearray()
    while len(out) < n:
        r = rng.random()
        if r < 0.8:
            out += rng.choice(keys)
        elif r < 0.8 + nul and parents:
            out += rng.choice(parents) + b"\x00"
        else:
            out += bytes([rng.choice(b"abcq ")])
    return bytes(out[:n])


def short_keys():
    rng = random.Random(5)
    keys = sorted({bytes(rng.choice(b"abc") for _ in range(rng.randint(1, 8))) for _ in range(160)})
    assert max(len(k) for k in keys) == 8
    return keys


def long_keys():
    rng = random.Random(6)
    keys = sorted({bytes(rng.choice(b"ab") for _ in range(rng.randint(2, 12))) for _ in range(80)} | {b"ab" * 150, b"a" * 40 + b"b" * 17})
    assert max(len(k) for k in keys) == 300
    return keys


def chunk_handle(kind):
    def make():
        keys = short_keys() if kind == "short" else long_keys()
        o = orc.AC.compile(keys)
        return keys, o.stale_paths(), AC.compile(keys), o
    return cached(("chunk", kind), make)


def feed_in_pieces(f, sim, text, lens, use_device, seq=0):
    got, pos = [], 0
    for n in lens:
        got += rows(check_call(f, sim, [text[pos:pos + n]], [seq], use_device)[0])
        pos += n
    assert pos == len(text)
    return got


PIECES_9K = [0, 1, 1023, 1024, 1025, 3000, 0, 4143]


@pytest.mark.parametrize("use_device", [False, True])
def test_chunks_short_keys(use_device):
    """Lmax = 8: chunks of 1024 bytes.  One sequence fed 9 KiB in pieces of 0 .. 4143 bytes (a call of one long piece takes the
    chunked walk), then a call of 16 sequences with 700-byte pieces, whose cuts fall inside chunks (the per-piece walk by the
    switch rule), then 16 pieces of 2100 bytes: chunks with cuts inside them."""
    keys, stale, m, o = chunk_handle("short")
    text = dense_text(keys, sum(PIECES_9K), 21)
    f = m.feed(17, longest=2)
    sim = FeedLongestSim(keys, 17, True, stale)
    got = feed_in_pieces(f, sim, text, PIECES_9K, use_device, seq=16)
    got += rows(check_finish(f, sim, [16], use_device)[0])
    assert got == rows(o.match_longest(text, intersectable=True, chars=False))
    texts = [dense_text(keys, 700 + 2100, 100 + s) for s in range(16)]
    ids = list(range(16))
    a = check_call(f, sim, [t[:700] for t in texts], ids, use_device)
    b = check_call(f, sim, [t[700:] for t in texts], ids, use_device)
    fin = check_finish(f, sim, ids, use_device)
    for s in ids:
        assert rows(a[s]) + rows(b[s]) + rows(fin[s]) == rows(o.match_longest(texts[s], intersectable=True, chars=False)), s


@pytest.mark.parametrize("use_device", [False, True])
def test_chunks_long_keys(use_device):
    """Lmax = 300: the chunk grows to 8192 bytes and the warm-up to 600; 40 KiB in pieces with cuts inside chunks, pieces
    shorter than the warm-up, and two sequences in one call"""
    keys, stale, m, o = chunk_handle("long")
    assert m.info["max_key_len"] == 300
    text = dense_text(keys, 40 << 10, 22)
    f = m.feed(2, longest=2)
    sim = FeedLongestSim(keys, 2, True, stale)
    lens = [8192, 8191, 300, 1, 599, 10000, 0]
    lens.append(len(text) - sum(lens))
    got = feed_in_pieces(f, sim, text, lens, use_device)
    got += rows(check_finish(f, sim, [0], use_device)[0])
    assert got == rows(o.match_longest(text, intersectable=True, chars=False))
    a = check_call(f, sim, [text[:20000], text[5:17000]], [0, 1], use_device)
    b = check_call(f, sim, [text[17000:], text[20000:]], [1, 0], use_device)
    fin = check_finish(f, sim, [0, 1], use_device)
    assert rows(a[0]) + rows(b[1]) + rows(fin[0]) == rows(o.match_longest(text, intersectable=True, chars=False))
    assert rows(a[1]) + rows(b[0]) + rows(fin[1]) == rows(o.match_longest(text[5:], intersectable=True, chars=False))


@pytest.mark.parametrize("mode", [1, 2])
def test_nuls(mode):
    """a NUL at a value node as a piece's last byte (the next piece's first byte vanishes), two NULs in a row across a cut, NULs
    sprinkled over the chunked text, and a 6 KiB stretch with a NUL every third byte where the chunks give up"""
    keys, stale, m, o = chunk_handle("short")
    isect = mode == 2
    keyset = set(keys)
    parent = next(k for k in keys if len(k) >= 2 and any(x != k and x.startswith(k) for x in keyset))
    body = dense_text(keys, 5000, 31, nul=0.1)
    every_third = b"".join(bytes([c, d, 0]) for c, d in zip(dense_text(keys, 2048, 32), dense_text(keys, 2048, 33)))
    assert len(every_third) == 6144
    head = parent + b"\x00"
    text = head + body[:2000] + parent + b"\x00" + b"\x00" + body[2000:] + every_third + body[:3000] + parent + b"\x00" + keys[0] + body[:1500]
    cut1 = len(head)                                   # behind a value node
    cut2 = len(head) + 2000 + len(parent) + 1          # between two NULs
    cut3 = cut2 + 1 + 3000 - 1000                      # 1000 bytes in front of the stretch with a NUL every third byte: the piece
                                                       # holds all 6 KiB of it, so a chunk 4 KiB into it finds no clean warm-up
    cut4 = len(text) - 1500 - len(keys[0])             # behind a value node again
    cuts = [0, cut1, cut2, cut3, cut4, len(text)]
    assert text[cut1 - 1] == 0 and text[cut2 - 1] == 0 and text[cut2] == 0 and text[cut4 - 1] == 0
    want = rows(o.match_longest(text, intersectable=isect, chars=False))
    for use_device in (False, True):
        f = m.feed(1, longest=mode)
        sim = FeedLongestSim(keys, 1, isect, stale)
        got = feed_in_pieces(f, sim, text, [b - a for a, b in zip(cuts, cuts[1:])], use_device)
        got += rows(check_finish(f, sim, [0], use_device)[0])
        assert got == want


# ---- 4: stale END flags ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [1, 2])
def test_stale_end_flags_at_every_cut(mode):
    keys, stale = stale_keys()
    assert stale
    m, o = cached(("stale",), lambda: (AC.compile(keys), orc.AC.compile(keys)))
    isect = mode == 2
    for seed in range(41, 141):  # the first text on which the stale flags are observable in this mode
        rng = random.Random(seed)
        text = bytes(rng.choice(b"ab") for _ in range(80))
        want = rows(o.match_longest(text, intersectable=isect, chars=False))
        blind = FeedLongestSim(keys, 1, isect)  # (the model without the stale set)
        if want != rows(blind.piece(0, text)[0]) + rows(absolute(*blind.finish(0))):
            break
    else:
        raise AssertionError("no text shows the stale flags")
    S = len(text) + 1
    f = m.feed(S, longest=mode)
    sim = FeedLongestSim(keys, S, isect, stale)
    ids = list(range(S))
    a = check_call(f, sim, [text[:c] for c in ids], ids, True)
    b = check_call(f, sim, [text[c:] for c in ids], ids, False)
    fin = check_finish(f, sim, ids, True)
    for c in ids:
        assert rows(a[c]) + rows(b[c]) + rows(fin[c]) == want, c


# ---- 5: a folded handle ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [1, 2])
def test_folded_handle(mode):
    keys = [b"Error", b"ERRORS", b"err", b"Warning", b"warn", b"rs"]
    low = [k.lower() for k in keys]
    m = cached(("fold",), lambda: AC.compile(keys, fold_ascii=True))
    plain, o = cached(("fold-plain",), lambda: (AC.compile(low), orc.AC.compile(low)))
    isect = mode == 2
    text = b"an ERRor, eRRORS and WARNings; errORs warn ErrorS"
    want = rows(o.match_longest(text.lower(), intersectable=isect, chars=False))
    assert want
    S = len(text) + 1
    ids = list(range(S))
    f, g = m.feed(S, longest=mode), plain.feed(S, longest=mode)
    sim = FeedLongestSim(low, S, isect, o.stale_paths(), fold=True)
    for use_device, part in ((False, lambda c: text[:c]), (True, lambda c: text[c:])):
        mixed = check_call(f, sim, [part(c) for c in ids], ids, use_device)  # a key cut at every byte, in every case combination
        lowered = _call(g, [part(c).lower() for c in ids], ids, use_device)
        assert rows(np.concatenate(mixed) if mixed else []) == rows(np.concatenate(
            [absolute(lowered[0][int(lowered[1][d]):int(lowered[1][d + 1])], int(lowered[2][d])) for d in ids]))
    fin = check_finish(f, sim, ids, True)
    assert rows(_finish(g, ids, False)[0]) == [(a - len(text), e - len(text), v) for x in fin for a, e, v in rows(x)]


# ---- 6: capacity and atomicity -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [1, 2])
def test_capacity_and_atomicity(mode):
    import torch

    keys, stale, m, o = chunk_handle("short")
    isect = mode == 2
    texts = [dense_text(keys, 3000, 50 + s) for s in range(4)]
    f = m.feed(4, longest=mode)
    sim = FeedLongestSim(keys, 4, isect, stale)
    check_call(f, sim, [t[:779] for t in texts], [0, 1, 2, 3], True)
    pieces, ids = [texts[s][779:779 + 701 * (s + 1)] for s in (2, 0, 3)], [2, 0, 3]
    want = [sim.piece(s, p)[0] for s, p in zip(ids, pieces)]
    required = sum(len(w) for w in want)
    assert required > 3
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
    hits, pho, bases = _call(f, pieces, ids, use_device=True, cap=required)  # the same call with room: what the first would have given
    assert np.array_equal(hits, np.concatenate(want)) and bases.tolist() == [779] * 3
    # a finish call one short: the sequences have not restarted
    for s in range(4):  # (every sequence ends with a key read from the root: something is pending)
        check_call(f, sim, [b"q" + keys[-1]], [s], False)
    lens = [f.position(s)[0] for s in range(4)]
    wantf = [sim.finish(s) for s in (1, 3, 0)]
    need = sum(len(w[0]) for w in wantf)
    assert need == 3
    it = _device(np.array([1, 3, 0], np.int32))
    out = torch.full((need, 3), 0x5A5A5A5A, dtype=torch.int32, device="cuda:0")
    with pytest.raises(AhaError) as e:
        f.finish_batch_device(it, out[:need - 1])
    assert e.value.code == N.AHA_E_CAPACITY and e.value.required == need and (out == 0x5A5A5A5A).all()
    n = C.c_uint64(0)
    ids_f = np.array([1, 3, 0], np.uint32)
    hout = np.zeros(need, dtype=HIT_DTYPE)
    assert N.lib().aha_feed_finish_batch(f._h, ids_f.ctypes.data, 3, hout.ctypes.data, need - 1, None, None, C.byref(n)) == N.AHA_E_CAPACITY
    assert n.value == need and [f.position(s)[0] for s in range(4)] == lens
    hits, sho, bases = _finish(f, [1, 3, 0], use_device=True, cap=need)
    assert np.array_equal(hits, np.concatenate([w[0] for w in wantf])) and bases.tolist() == [w[1] for w in wantf]
    assert sho.tolist() == [0, 1, 2, 3] and all(h[1] <= 0 for h in rows(hits))
    assert [f.position(s)[0] for s in range(4)] == [0, 0, lens[2], 0]
    # bad ids change nothing
    for bad in ([2, 2], [0, 4]):
        with pytest.raises(AhaError) as e:
            f.finish_batch(np.array(bad, np.uint32))
        assert e.value.code == N.AHA_E_INVALID
        with pytest.raises(AhaError) as e:
            f.match_batch(np.zeros(2, np.uint8), np.array([0, 1, 2], np.uint64), np.array(bad, np.uint32))
        assert e.value.code == N.AHA_E_INVALID
    assert f.position(2)[0] == lens[2]
    assert rows(check_finish(f, sim, [2], False)[0])


# ---- 7: refusals, reset, mixing ----------------------------------------------------------------------------------------------
def test_refusals_reset_and_mixing():
    import torch

    keys, stale, m, o = chunk_handle("short")
    f = m.feed(3, longest=1)
    sim = FeedLongestSim(keys, 3, False, stale)
    text = dense_text(keys, 1200, 61)
    check_call(f, sim, [text[:500]], [0], True)
    piece = np.frombuffer(text[500:900], np.uint8).copy()
    offs = np.array([0, piece.size], np.uint64)
    ids = np.array([0], np.uint32)
    out = torch.zeros((64, 3), dtype=torch.int32, device="cuda:0")
    dev = lambda: (_device(piece), _device(offs.view(np.int64)), _device(ids.view(np.int32)))
    table = m.replacements({0: b"-"})
    calls = [lambda: f.count_batch(piece, offs, ids), lambda: f.cover_batch(piece, offs, ids), lambda: f.select_batch(piece, offs, ids),
             lambda: f.replace_batch(piece, offs, ids, table), lambda: f.grep_batch(piece, offs, ids),
             lambda: f.count_batch_device(*dev()), lambda: f.select_batch_device(*dev(), out),
             lambda: f.cover_batch_device(*dev(), mask=torch.zeros(16, dtype=torch.int32, device="cuda:0"))]
    for call in calls:
        with pytest.raises(AhaError) as e:
            call()
        assert e.value.code == N.AHA_E_INVALID and "follow-up" in str(e.value)
        assert f.position(0)[0] == 500
    check_call(f, sim, [text[500:900]], [0], False)  # the feed goes on as if nothing had happened
    # reset drops a pending end
    check_call(f, sim, [keys[-1]], [1], True)
    assert len(FeedLongestSim(keys, 1, False, stale).piece(0, keys[-1] + b"q")[0]) == 1  # (something was pending)
    f.reset(1)
    sim.reset(1)
    assert rows(check_call(f, sim, [b"q"], [1], True)[0]) == [] and f.position(1)[0] == 1
    assert rows(check_finish(f, sim, [1], True)[0]) == []
    f.reset()
    for s in range(3):
        sim.reset(s)
    assert [f.position(s)[0] for s in range(3)] == [0, 0, 0]
    # finish on a plain feed is still refused
    g = m.feed(2)
    with pytest.raises(AhaError) as e:
        g.finish_batch(np.array([0], np.uint32))
    assert e.value.code == N.AHA_E_INVALID
    # a plain feed and a longest feed on one handle, interleaved with a batch match_longest: each still exact
    from feedsim import FeedSim

    gsim = FeedSim(o, 2, False)
    corpus = np.frombuffer(text, np.uint8).copy()
    doc = np.array([0, 400, 1200], np.uint64)
    got_l, got_p = [], []
    for a, b in ((0, 300), (300, 301), (301, 1000), (1000, 1200)):
        got_l += rows(check_call(f, sim, [text[a:b]], [2], a % 2 == 0)[0])
        hp, _, bp = _call(g, [text[a:b]], [1], a % 2 == 1)
        wp, wb = gsim.piece(1, text[a:b])
        assert np.array_equal(hp, wp) and int(bp[0]) == wb
        got_p += rows(absolute(hp, int(bp[0])))
        bh, bd = m.match_batch(corpus, doc, longest=1)
        assert rows(bh) == [r for d in range(2) for r in rows(o.match_longest(text[int(doc[d]):int(doc[d + 1])], intersectable=False, chars=False))]
    assert got_l + rows(check_finish(f, sim, [2], False)[0]) == rows(o.match_longest(text, intersectable=False, chars=False))
    assert got_p == rows(o.match(text, chars=False))


# ---- 8: the C++ mirror -------------------------------------------------------------------------------------------------------
def build_spec_feed_longest(tmp_path):
    exe = str(tmp_path / "spec_feed_longest_gpu")
    cmd = ["g++", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "cpp", "spec_feed_longest_gpu.cpp"), "-L", os.path.join(ROOT, "aha_amd"), "-laha_hip",
           "-Wl,-rpath," + os.path.join(ROOT, "aha_amd"), "-Wl,-rpath,/opt/rocm/lib", "-o", exe]
    subprocess.check_call(cmd)
    return exe


def test_cpp_mirror(tmp_path):
    exe = build_spec_feed_longest(tmp_path)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "spec_feed_longest_gpu: ok" in r.stdout
