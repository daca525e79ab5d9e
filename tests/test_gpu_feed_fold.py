"""GPU tests of folded feeds (AHA_FEED_FOLD: feeds on handles compiled with fold_simple, fold_bmp or fold_kana): match, count and
cover calls, device and host entries, bit-exact against the rule of DESIGN.md 4.13 "Feeds on handles folded beyond ASCII" stated
with the oracle -- the hits with n0 < end <= n1 of fold(S[:n1]), folded in Python, matched as one document by the oracle of the
folded keys (tests/feedfoldsim.py rule_hits) -- and everything that follows from that hit list: piece_hit_offsets, bases, key
counts, masks, piece_back, piece_covered, redacted bytes."""
import os
import random
import re

import numpy as np
import pytest

import pyoracle as orc
from aha_amd import AC, AhaError, BitArray
from aha_amd import _native as N
from feedfoldsim import FOLD_KEYS, FOLD_OPTS, cover_of, rule_hits

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIT = orc.HIT_DTYPE

# keys of whole characters, keys cut inside a character, a key that ends in a lead byte: unique under every fold
KEYS = ["Привет", "ПРИ", "école", "ｅｒｒ", "việt", "ラーメン", "ⴀⴁ", "он", "ab", "B", "我是",
        "ệ".encode()[1:] + b"t", "Ж".encode()[:1], b"a" + "ệ".encode()[:2], "ー".encode()[1:]]
# 48 bytes: ASCII, Cyrillic, Latin-1, full-width, Vietnamese, kana in all three scripts, a stray continuation and a stray lead
TEXT48 = ("aB ПрИ" + "É" + "ＥｒＲ" + "viỆt" + "らーﾒﾝ" + "Он").encode() + b"\x96\xe1" + "我".encode() + b"b"
MIX = ["привет ", "ПРИВЕТ", "École ", "ＥＲＲ ｅｒｒ", "VIỆT việt ", "らーめん ラーメン ﾗｰﾒﾝ", "ႠႡ ⴀⴁ", "ОН он", "aB Ab", "我是中", "\x00", "xyz "]
STRAY = [b"\x96", b"\xe1", b"\xd0", b"\xe1\xbb", b"\xef\xbd", b"\xc3"]

_CACHE = {}


def handle(mode):
    """-> (the folded handle, the oracle of the folded keys), one per mode for the whole file"""
    if mode not in _CACHE:
        keys = [k.encode() if isinstance(k, str) else k for k in KEYS]
        _CACHE[mode] = (AC.compile(keys, **{FOLD_OPTS[mode]: True}), orc.AC.compile(FOLD_KEYS[mode](keys)))
    return _CACHE[mode]


def mixed(rng, n):
    out = bytearray()
    while len(out) < n:
        out += rng.choice(STRAY) if rng.random() < 0.08 else rng.choice(MIX).encode()
    return bytes(out[:n])


class Ref:
    """the sequences as the test fed them, and what the rule says a call on them reports"""

    def __init__(self, oracle, mode, n_seqs, chars):
        self.o, self.mode, self.chars = oracle, mode, chars
        self.S = [b""] * n_seqs

    def call(self, ids, pieces):
        hits, pho, bases, bits, back, cov = [], [0], [], [], [], []
        kc = np.zeros(self.o.n_keys, dtype=np.uint64)
        for seq, P in zip(ids, pieces):
            n0 = len(self.S[seq])
            S = self.S[seq] + P
            h, hb, base = rule_hits(self.o, self.mode, S, n0, len(S), chars=self.chars)
            m, bk = cover_of(hb, len(P))
            hits.append(h)
            pho.append(pho[-1] + len(h))
            bases.append(base)
            bits.append(m)
            back.append(bk)
            cov.append(int(m.sum()))
            np.add.at(kc, h["value"].astype(np.int64), 1)
            self.S[seq] = S
        allbits = np.concatenate(bits + [np.zeros(0, dtype=bool)])
        words = np.zeros((allbits.size + 31) // 32 * 4, dtype=np.uint8)
        packed = np.packbits(allbits, bitorder="little")
        words[:packed.size] = packed
        return {"hits": np.concatenate(hits + [np.zeros(0, dtype=HIT)]), "pho": np.array(pho, dtype=np.uint64),
                "bases": np.array(bases, dtype=np.uint64), "kc": kc, "mask": words.view(np.uint32), "bits": allbits,
                "back": np.array(back, dtype=np.uint32), "cov": np.array(cov, dtype=np.uint64)}

    def reset(self, seq=None):
        for s in range(len(self.S)) if seq is None else [seq]:
            self.S[s] = b""


def batch(ids, pieces, lead=0):
    """-> (corpus uint8 as a view `lead` bytes into a buffer, piece offsets, ids)"""
    blob = b"".join(pieces)
    buf = np.frombuffer(b"\xd0" * lead + blob + b"\x96" * 3, dtype=np.uint8)  # (bytes around it that would pair with its ends)
    off = np.cumsum([0] + [len(p) for p in pieces]).astype(np.uint64)
    return buf[lead:lead + len(blob)], off, np.array(ids, dtype=np.uint32)


def check_call(feed, kind, entry, ids, pieces, want, lead=0):
    """one call of `kind` (match, count, cover) through the host or the device entry, everything it gives held against want"""
    import torch

    corpus, off, sid = batch(ids, pieces, lead)
    D, n = len(pieces), corpus.size
    if entry == "host":
        if kind == "match":
            hits, pho, bases = feed.match_batch(corpus, off, sid)
            assert hits.tobytes() == want["hits"].tobytes()
        elif kind == "count":
            kc, pho, bases = feed.count_batch(corpus, off, sid)
            assert np.array_equal(kc, want["kc"])
        else:
            mask, red, info = feed._cover_host(corpus, off, sid, True, True, 0x2A)
            pho, bases = info["piece_hit_offsets"], info["piece_bases"]
            assert np.array_equal(mask, want["mask"])
            assert np.array_equal(red, np.where(want["bits"], np.uint8(0x2A), corpus))
            assert np.array_equal(info["piece_back"], want["back"]) and np.array_equal(info["piece_covered"], want["cov"])
            assert info["n_covered"] == int(want["cov"].sum()) and info["n_hits"] == len(want["hits"])
        assert np.array_equal(pho, want["pho"]) and np.array_equal(bases, want["bases"])
        return
    dev = "cuda:0"
    big = torch.from_numpy(np.concatenate([np.zeros(lead, dtype=np.uint8), corpus, np.zeros(3, dtype=np.uint8)])).to(dev)
    dc = big[lead:lead + n]
    do = torch.from_numpy(off.astype(np.int64)).to(dev)
    di = torch.from_numpy(sid.astype(np.int32)).to(dev)
    dpho = torch.full((D + 1,), -1, dtype=torch.int64, device=dev)
    dbases = torch.full((max(D, 1),), -1, dtype=torch.int64, device=dev)
    if kind == "match":
        out = torch.zeros((len(want["hits"]) + 3, 3), dtype=torch.int32, device=dev)
        got = feed.match_batch_device(dc, do, di, out, dpho, dbases)
        assert got == len(want["hits"])
        assert out[:got].cpu().numpy().tobytes() == want["hits"].tobytes()
    elif kind == "count":
        dk = torch.zeros(len(want["kc"]), dtype=torch.int64, device=dev)
        got = feed.count_batch_device(dc, do, di, dk, dpho, dbases)
        assert got == len(want["hits"]) and np.array_equal(dk.cpu().numpy().astype(np.uint64), want["kc"])
    else:
        dm = torch.zeros(max((n + 31) // 32, 1), dtype=torch.int32, device=dev)
        dback = torch.full((max(D, 1),), -1, dtype=torch.int32, device=dev)
        dcov = torch.full((max(D, 1),), -1, dtype=torch.int64, device=dev)
        nc, nh = feed.cover_batch_device(dc, do, di, mask=dm, redacted=dc, piece_back=dback, piece_covered=dcov,
                                         piece_hit_offsets=dpho, piece_bases=dbases)  # (redacted in place)
        assert nc == int(want["cov"].sum()) and nh == len(want["hits"])
        assert np.array_equal(dm.cpu().numpy().view(np.uint32)[:(n + 31) // 32], want["mask"])
        assert np.array_equal(dc.cpu().numpy(), np.where(want["bits"], np.uint8(0x2A), corpus))
        assert np.array_equal(dback.cpu().numpy()[:D].view(np.uint32), want["back"])
        assert np.array_equal(dcov.cpu().numpy()[:D].astype(np.uint64), want["cov"])
    assert np.array_equal(dpho.cpu().numpy().astype(np.uint64), want["pho"])
    assert np.array_equal(dbases.cpu().numpy()[:D].astype(np.uint64), want["bases"])


# ---- the flag ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [2, 3, 4])
def test_open_needs_the_flag_and_takes_it(mode):
    m, o = handle(mode)
    with pytest.raises(AhaError) as e:
        m.feed(1)
    assert e.value.code == N.AHA_E_INVALID and "follow-up" in str(e.value)
    for kw in ({"sep": orc_sep()}, {"longest": 1}, {"longest": 2}):
        with pytest.raises(AhaError) as e:
            m.feed(1, fold=True, **kw)
        assert e.value.code == N.AHA_E_INVALID and "follow-up" in str(e.value)
    feed = m.feed(2, fold=True)
    ref = Ref(o, mode, 2, False)
    check_call(feed, "match", "host", [1], ["ПРИВ".encode()], ref.call([1], ["ПРИВ".encode()]))
    check_call(feed, "match", "host", [1], ["ЕТ".encode()], ref.call([1], ["ЕТ".encode()]))
    assert len(ref.S[1]) == 12 and feed.position(1) == (12, 0) and feed.position(0) == (0, 0)


def orc_sep():
    sep = BitArray(64)
    sep[32] = True
    return sep


def test_the_flag_on_a_plain_handle_changes_nothing():
    m = AC.compile(["Error", "rro"], fold_ascii=True)
    a, b = m.feed(1), m.feed(1, fold=True)
    for piece in (b"an ER", b"ROR, err", b"or"):
        ha, hb = a.match(0, piece), b.match(0, piece)
        assert ha == hb
    assert a.position(0) == b.position(0) == (15, 0)


# ---- a cut at every byte -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("entry", ["device", "host"])
@pytest.mark.parametrize("chars", [False, True])
@pytest.mark.parametrize("mode", [2, 3, 4])
def test_a_cut_at_every_byte(mode, chars, entry):
    """48 one-byte pieces: every pair is cut once and every triple twice.  Sequence 0 of one feed takes match calls; on a second
    feed count and cover calls take turns."""
    assert len(TEXT48) == 48
    m, o = handle(mode)
    fa, fb = m.feed(1, chars=chars, fold=True), m.feed(1, chars=chars, fold=True)
    ra, rb = Ref(o, mode, 1, chars), Ref(o, mode, 1, chars)
    n_hits = 0
    for i in range(48):
        P = [TEXT48[i:i + 1]]
        want = ra.call([0], P)
        n_hits += len(want["hits"])
        check_call(fa, "match", entry, [0], P, want)
        check_call(fb, "count" if i % 2 == 0 else "cover", entry, [0], P, rb.call([0], P))
    assert n_hits >= 6  # (the text holds the keys in the other case)


# ---- many pieces, odd boundaries, an unaligned view ----------------------------------------------------------------------------
@pytest.mark.parametrize("mode,chars", [(2, False), (3, True), (4, False)])
def test_300_pieces_of_as_many_sequences_in_a_view(mode, chars):
    m, o = handle(mode)
    rng = random.Random(7 + mode)
    D = 300
    feed, ref = m.feed(D, chars=chars, fold=True), Ref(o, mode, D, chars)
    whole = [mixed(rng, rng.choice([0, 1, 2, 3, 5, 17, 31, 33, 64, 90])) for _ in range(D)]
    for kind, entry in (("match", "device"), ("cover", "device"), ("count", "host"), ("match", "host"), ("cover", "host")):
        ids = list(range(D))
        rng.shuffle(ids)
        pieces = []
        for s in ids:  # the next part of every sequence: empty, one byte, two bytes, or more -- wherever that falls
            done = len(ref.S[s])
            pieces.append(whole[s][done:done + rng.choice([0, 1, 2, 2, 7, 19])])
        check_call(feed, kind, entry, ids, pieces, ref.call(ids, pieces), lead=5)


# ---- one long piece: the staged copy's unrolled loop, remainder loop and byte tail ---------------------------------------------
@pytest.mark.parametrize("mode", [2, 3, 4])
def test_a_piece_of_70_kib(mode):
    m, o = handle(mode)
    rng = random.Random(70 + mode)
    body = mixed(rng, 70 * 1024 + 7)
    feed, ref = m.feed(2, fold=True), Ref(o, mode, 2, False)
    # both sequences are cut inside a character: the long piece begins with the second byte of "т", the short one with the last
    # two bytes of "Ệ"
    heads = ["x Приве".encode() + "т".encode()[:1], b"vi" + "Ệ".encode()[:1]]
    check_call(feed, "match", "device", [1, 0], heads, ref.call([1, 0], heads))
    pieces = ["т".encode()[1:] + b" " + body, "Ệ".encode()[1:] + b"t ab"]
    want = ref.call([1, 0], pieces)
    assert len(want["hits"]) > 1000 and want["hits"]["start"].min() == -11  # "Привет" across the cut
    assert mode == 2 or -3 in want["hits"]["start"]  # ... and "việt" (the simple fold leaves "Ệ" alone)
    check_call(feed, "match", "device", [1, 0], pieces, want, lead=5)
    feed.reset()
    ref.reset()
    check_call(feed, "cover", "host", [1], heads[:1], ref.call([1], heads[:1]))
    want = ref.call([1], pieces[:1])
    assert want["back"][0] == 11
    check_call(feed, "cover", "host", [1], pieces[:1], want)


# ---- more pieces than the two kernels start workgroups or lanes for ------------------------------------------------------------
def launcher_caps():
    src = open(os.path.join(ROOT, "aha_amd", "csrc", "scan_feedfold.hip")).read()
    threads = int(re.search(r"constexpr int kFfThreads = (\d+);", src).group(1))
    windows = int(re.search(r"constexpr uint32_t kFfWindowBlocks = (\d+);", src).group(1))
    heads = int(re.search(r"constexpr uint32_t kFfHeadBlocks = (\d+);", src).group(1))
    assert "ff_grid(F.D, kFfThreads, kFfHeadBlocks)" in src and "ff_grid(F.D, 1, kFfWindowBlocks)" in src
    return windows, heads * threads  # a workgroup per piece; a lane per piece


def test_the_piece_loops_take_a_second_trip():
    mode = 3
    m, o = handle(mode)
    D = max(launcher_caps()) + 37
    rng = random.Random(41)
    feed, ref = m.feed(D, fold=True), Ref(o, mode, D, False)
    word = "ViỆt ПРИвет ＥＲr".encode()
    starts = [rng.randrange(len(word)) for _ in range(D)]
    ids = list(range(D))
    first = [word[a:a + rng.choice([1, 2, 3, 4])] for a in starts]
    check_call(feed, "match", "device", ids, first, ref.call(ids, first), lead=5)
    second = [word[a + len(p):a + len(p) + rng.choice([0, 1, 2, 9])] for a, p in zip(starts, first)]
    want = ref.call(ids, second)
    tail = np.nonzero(np.diff(want["pho"])[max(launcher_caps()):])[0]
    assert tail.size and want["back"][max(launcher_caps()):].max() > 0  # (pieces of the second trip have hits across the cut)
    check_call(feed, "cover", "device", ids, second, want, lead=5)


# ---- the call families mixed on one feed, then reset and the same again --------------------------------------------------------
@pytest.mark.parametrize("mode,chars", [(2, True), (3, False), (4, True)])
def test_match_count_and_cover_calls_mix_and_reset_starts_again(mode, chars):
    m, o = handle(mode)
    feed, ref = m.feed(4, chars=chars, fold=True), Ref(o, mode, 4, chars)
    rng = random.Random(5 * mode)
    script = []
    streams = [mixed(rng, 120) for _ in range(4)]
    at = [0] * 4
    for kind, entry in (("match", "device"), ("count", "device"), ("cover", "device"), ("count", "host"), ("match", "host"),
                        ("cover", "host"), ("match", "device")):
        ids = rng.sample(range(4), rng.randint(1, 4))
        pieces = []
        for s in ids:
            k = rng.choice([0, 1, 2, 5, 11, 23])
            pieces.append(streams[s][at[s]:at[s] + k])
            at[s] += len(pieces[-1])
        script.append((kind, entry, ids, pieces))
    firsts = []
    for kind, entry, ids, pieces in script:
        firsts.append(ref.call(ids, pieces))
        check_call(feed, kind, entry, ids, pieces, firsts[-1])
    assert feed.position(0)[0] == len(ref.S[0]) > 0
    feed.reset()
    ref.reset()
    assert feed.position(0) == (0, 0)
    for (kind, entry, ids, pieces), before in zip(script, firsts):
        want = ref.call(ids, pieces)
        assert want["hits"].tobytes() == before["hits"].tobytes()
        check_call(feed, kind, entry, ids, pieces, want)
    # one sequence alone starts again: the others go on
    feed.reset(2)
    ref.reset(2)
    ids, pieces = [2, 1], [streams[2][:9], streams[1][at[1]:at[1] + 9]]
    check_call(feed, "match", "host", ids, pieces, ref.call(ids, pieces))


# ---- the families that are follow-ups ------------------------------------------------------------------------------------------
def test_select_replace_grep_and_finish_are_refused_and_change_nothing():
    import torch

    mode = 2
    m, o = handle(mode)
    feed, ref = m.feed(2, fold=True), Ref(o, mode, 2, False)
    check_call(feed, "match", "host", [0], ["x ПРИ".encode()], ref.call([0], ["x ПРИ".encode()]))
    corpus, off, sid = batch([0], ["вет он".encode()])
    dev = "cuda:0"
    dc, do, di = torch.from_numpy(corpus.copy()).to(dev), torch.from_numpy(off.astype(np.int64)).to(dev), torch.from_numpy(sid.astype(np.int32)).to(dev)
    out = torch.zeros((16, 3), dtype=torch.int32, device=dev)
    calls = [lambda: feed.select_batch(corpus, off, sid), lambda: feed.select_batch_device(dc, do, di, out),
             lambda: feed.replace_batch(corpus, off, sid, {0: "x"}), lambda: feed.grep_batch(corpus, off, sid),
             lambda: feed.grep_batch_device(dc, do, di)]
    for call in calls:
        with pytest.raises(AhaError) as e:
            call()
        assert e.value.code == N.AHA_E_INVALID and "follow-up" in str(e.value), str(e.value)
        assert feed.position(0) == (8, 0)  # (the feed as the first call left it)
    with pytest.raises(AhaError) as e:
        feed.finish_batch(np.array([0], dtype=np.uint32))
    assert e.value.code == N.AHA_E_INVALID
    want = ref.call([0], ["вет он".encode()])
    assert len(want["hits"]) >= 2 and want["hits"]["start"].min() < 0  # "Привет" across the cut, "он"
    check_call(feed, "match", "device", [0], ["вет он".encode()], want)


# ---- the README's caller -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [2, 3])
def test_redactor_blanks_a_word_cut_inside_a_character(mode):
    m = AC.compile(["ПРИВЕТ"], **{FOLD_OPTS[mode]: True})
    text = "Ой, Привет мир".encode()
    cut = text.index("в".encode()) + 1  # between the two bytes of "в"
    r = m.feed(1, fold=True).redactor()
    got = r.push(0, text[:cut]) + r.push(0, text[cut:]) + r.finish(0)
    a = text.index("Привет".encode())
    assert got == text[:a] + b"*" * 12 + text[a + 12:]  # the whole word, the original's bytes around it
