"""CPU tests of the feed select calls (aha_feed_select_batch, aha_feed_select_batch_device): exported, declared and bound; the
argument checks that come before any device work; the stream law and the settled prefix on the model (feedselectsim) over the
CPU oracle's hits; and the arithmetic of the Python Replacer against `substitute` on the whole sequence, with a stand-in feed
that answers from the model."""
import ctypes as C
import os
import random
import re

import numpy as np
import pytest

import feedselectsim as fss
import pyoracle as orc
import selectsim
from aha_amd import AC, Replacer
from aha_amd import _native as N
from aha_amd import ac as acmod

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("aha_feed_select_batch", "aha_feed_select_batch_device")


def test_feed_select_symbols_exported_declared_and_bound():
    hdr = open(os.path.join(ROOT, "include", "aha_hip.h")).read()
    listed = open(os.path.join(ROOT, "aha_amd", "csrc", "exports.map")).read()
    crystal = open(os.path.join(ROOT, "bindings", "crystal", "aha_hip.cr")).read()
    cxx = open(os.path.join(ROOT, "include", "aha", "ac.hpp")).read()
    L = C.CDLL(N.LIB_PATH)
    for name in ENTRIES:
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert re.search(r"^\s+%s;" % name, listed, re.M), name
        assert name in N.SIGNATURES and hasattr(L, name), name
        assert re.search(r"^\s*fun %s\(" % name, crystal, re.M), name
    assert "aha_feed_select_batch(" in cxx  # (the C++ mirror wraps the host entries of the feed calls)
    assert re.search(r"#define\s+AHA_FEED_SELECT_FINAL\s+1u", hdr) and N.AHA_FEED_SELECT_FINAL == 1
    assert N.lib().aha_abi_version() == 8  # a pure addition


def _both(feed, n=True, flags=0):
    """rc of the host entry and of the device entry on the same arguments; the buffers stay untouched"""
    corpus = np.frombuffer(b"ushers", dtype=np.uint8).copy()
    offs = np.array([0, corpus.size], dtype=np.uint64)
    ids = np.zeros(1, dtype=np.uint32)
    out = np.full(16 * 3, 0x5A5A5A5A, dtype=np.int32)
    pso = np.full(2, 0x5A5A5A5A, dtype=np.uint64)
    bases = np.full(1, 0x5A5A5A5A, dtype=np.uint64)
    hold = np.full(1, 0x5A5A5A5A, dtype=np.uint32)
    ns = C.c_uint64(7)
    pn = C.byref(ns) if n else None
    L = N.lib()
    rc_h = L.aha_feed_select_batch(feed, corpus.ctypes.data, offs.ctypes.data, ids.ctypes.data, 1, flags, out.ctypes.data, 16,
                                   pso.ctypes.data, bases.ctypes.data, hold.ctypes.data, pn, None)
    rc_d = L.aha_feed_select_batch_device(feed, corpus.ctypes.data, offs.ctypes.data, ids.ctypes.data, 1, corpus.size, flags,
                                          out.ctypes.data, 16, pso.ctypes.data, bases.ctypes.data, hold.ctypes.data, pn, None,
                                          None)
    for a in (out, pso, bases, hold):
        assert (a == 0x5A5A5A5A).all()
    return rc_h, rc_d


def test_feed_select_argument_checks_before_any_device_work():
    m = AC.compile(["he", "she", "hers"], host_only=True)
    h = C.c_void_p()
    assert N.lib().aha_feed_open(m._h, 4, 0, C.byref(h)) == N.AHA_E_NO_DEVICE and not h.value  # no feed on such a handle
    assert _both(None) == (N.AHA_E_INVALID, N.AHA_E_INVALID)  # a NULL feed
    assert _both(None, n=False) == (N.AHA_E_INVALID, N.AHA_E_INVALID)  # ... and a NULL n_selected
    for flags in (2, 3, 0x80000000):
        assert _both(None, flags=flags) == (N.AHA_E_INVALID, N.AHA_E_INVALID)


# ---- the model against select_doc of the whole sequence, on the oracle's hits ---------------------------------------------
def _keys(rng, alphabet=b"abc", max_len=6):
    n = min(rng.randint(1, 6), sum(len(alphabet) ** k for k in range(1, max_len + 1)))
    keys = set()
    while len(keys) < n:
        keys.add(bytes(rng.choice(alphabet) for _ in range(rng.randint(1, max_len))))
    return sorted(keys)


def _cut(text, cuts):
    at = [0] + sorted(cuts) + [len(text)]
    return [text[at[i]:at[i + 1]] for i in range(len(at) - 1)]


def _law(keys, text, cuts):
    o = orc.AC.compile(keys)
    match, W = fss.oracle_match(o), fss.window(keys)
    want = selectsim.select_doc(match(text))
    got = fss.stream(match, W, _cut(text, cuts))
    assert got == want, (keys, text, cuts)


def test_stream_law_every_cut_of_short_sequences():
    cases = [([b"ab", b"abcde"], b"abcdeabab"), ([b"ab", b"bcd", b"cd", b"d"], b"abcdabcd"), ([b"a", b"aa", b"aaa"], b"aaaaabaaa"),
             ([b"a", b"b"], b"abcab"), ([b"abc", b"bc", b"ca"], b"abc\x00abcabc"), ([b"aaaa"], b"aaaaaaaaa")]
    for keys, text in cases:
        for i in range(len(text) + 1):
            _law(keys, text, [i])
            for j in range(i, len(text) + 1):
                _law(keys, text, [i, j])  # (i == j: an empty piece)


def test_stream_law_random():
    rng = random.Random(20260)
    for case in range(3000):
        keys = _keys(rng, b"abc", max_len=1 if case % 11 == 0 else 6)  # (every 11th: W = 0)
        alphabet = b"abc" + (b"\x00" if case % 5 == 0 else b"") + (b"x" if case % 3 == 0 else b"")  # (a key holds no NUL; text may)
        text = bytes(rng.choice(alphabet) for _ in range(rng.randint(0, 60)))
        cuts = [rng.randint(0, len(text)) for _ in range(rng.randint(0, 6))]
        _law(keys, text, cuts)


def test_settled_hits_never_change_when_the_sequence_grows():
    rng = random.Random(7)
    for _ in range(300):
        keys = _keys(rng)
        o = orc.AC.compile(keys)
        match, W = fss.oracle_match(o), fss.window(keys)
        text = bytes(rng.choice(b"abc") for _ in range(rng.randint(1, 40)))
        settled = []
        for n in range(len(text) + 1):
            sel = selectsim.select_doc(match(text[:n]))
            now = [h for h in sel if h[0] < fss.frontier(n, W)]
            assert now[: len(settled)] == settled, (keys, text, n)  # what was settled stays, in place
            assert all(h[0] >= fss.frontier(n - 1, W) for h in now[len(settled):])  # what is new starts behind the old frontier
            settled = now
        assert selectsim.select_doc(match(text))[: len(settled)] == settled


def test_model_hold_and_offsets():
    keys = [b"ab", b"abcde"]
    q = fss.Sequence(fss.oracle_match(orc.AC.compile(keys)), fss.window(keys))
    assert q.push(b"ab") == ([], 2, 0)  # "ab" may still lose to "abcde"
    assert q.push(b"cde") == ([(-2, 3, 1)], 0, 2)  # it did; the cursor stands behind the hit
    assert q.push(b"abx") == ([], 3, 5)
    assert q.push(b"", final=True) == ([(-3, -1, 0)], 0, 8)  # only now final: end <= 0
    assert q.push(b"ab", final=True) == ([(0, 2, 0)], 0, 0)  # the sequence started again


# ---- the Replacer's arithmetic, on a stand-in feed ---------------------------------------------------------------------------
class _ModelFeed:
    """what Replacer needs of a Feed, answered by the model"""

    class _Ac:
        def __init__(self, n_keys):
            self.n_keys = n_keys

    def __init__(self, keys):
        self._ac = self._Ac(len(keys))
        self._m = fss.Feed(fss.oracle_match(orc.AC.compile(keys)), fss.window(keys), 4)
        self.max_held = 0

    def select_batch(self, corpus, piece_offsets, seq_ids, final=False, cap=None):
        assert len(seq_ids) == 1 and int(piece_offsets[0]) == 0
        hits, pso, bases, hold = self._m.call([np.asarray(corpus, dtype=np.uint8).tobytes()], [int(seq_ids[0])], final)
        return hits.view(acmod.HIT_DTYPE), {"piece_sel_offsets": pso, "piece_bases": bases, "piece_hold": hold, "n_hits": 0}


def test_replacer_arithmetic_against_substitute():
    rng = random.Random(99)
    for case in range(400):
        keys = _keys(rng)
        K, W = len(keys), fss.window(keys)
        repl = {}
        for k in range(K):
            r = rng.random()
            if r < 0.4:
                repl[k] = bytes(rng.choice(b"XYZ") for _ in range(rng.randint(1, 8)))
            elif r < 0.6:
                repl[k] = ""  # deletion
            elif r < 0.7:
                repl[k] = None  # kept, said aloud; the rest: kept, not named
        text = bytes(rng.choice(b"abcx") for _ in range(rng.randint(0, 50)))
        o = orc.AC.compile(keys)
        want = acmod.substitute(text, fss.as_array(selectsim.select_doc(fss.oracle_match(o)(text))), repl, K)
        feed = _ModelFeed(keys)
        r = Replacer(feed, repl)
        seq = case % 4
        got = b""
        for p in _cut(text, [rng.randint(0, len(text)) for _ in range(rng.randint(0, 5))]):
            got += r.push(seq, p)
            assert len(r._held.get(seq, b"")) <= W
        got += r.finish(seq)
        assert got == want, (keys, repl, text)
        assert seq not in r._held
    # str pieces and replacements are UTF-8
    feed = _ModelFeed(["中".encode(), "中国".encode()])
    r = Replacer(feed, {0: "Z", 1: "中华"})
    assert r.push(0, "我是中") + r.push(0, "国人中") + r.finish(0) == "我是中华人Z".encode()
    with pytest.raises(ValueError):
        Replacer(_ModelFeed([b"a", b"b"]), ["x"]).push(0, b"ab")  # a sequence must have one entry per key
