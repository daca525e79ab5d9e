"""CPU tests of the feed replace calls (aha_feed_replace_batch, aha_feed_replace_batch_device): the contract's model
(feedreplacesim) against replace_doc of the whole sequence over select_doc of the CPU oracle's hits, at every cut and every pair
of cuts less than a key apart; the numpy model of the device path's arithmetic against the contract's model; both entry points
exported, declared, listed and bound; the argument checks that come before any device work."""
import ctypes as C
import os
import random
import re

import numpy as np

import feedreplacesim as frs
import feedselectsim as fss
import pyoracle as orc
import replacesim
import selectsim
from aha_amd import AC
from aha_amd import _native as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("aha_feed_replace_batch", "aha_feed_replace_batch_device")

# (keys, replacements, text): deletions, kept keys (None, or not named), replacements longer and shorter than the key, NUL
# bytes in text and replacement, W = 0
CASES = [
    ([b"ab", b"abcde"], {0: b"<AB>", 1: b""}, b"abcdeabab"),
    ([b"ab", b"abcde"], {0: b"", 1: b"a longer replacement"}, b"xabcdabcdeab"),
    ([b"ab", b"abcde"], {0: None, 1: b"Q"}, b"abcdeababcd"),
    ([b"ab", b"bcd", b"cd", b"d"], {0: b"1", 1: b"22", 2: b"", 3: b"four"}, b"abcdabcd"),
    ([b"ab", b"bcd", b"cd", b"d"], {1: b"x", 3: b""}, b"dabcdbcdd"),
    ([b"ab", b"bcd", b"cd", b"d"], [b"", b"", b"", b""], b"abcdabcdxd"),
    ([b"abc", b"bc", b"ca"], {0: b"\x00\x00", 1: b"B", 2: None}, b"abc\x00abcabc\x00ca"),
    ([b"a", b"b"], {0: b"", 1: b"bb"}, b"abcab"),
    ([b"a", b"b", b"c"], {0: b"A", 2: b""}, b"\x00abcab"),
]


def _cut(text, cuts):
    at = [0] + sorted(cuts) + [len(text)]
    return [text[at[i]:at[i + 1]] for i in range(len(at) - 1)]


def _whole(match, text, repl):
    return replacesim.replace_doc(text, selectsim.select_doc(match(text)), repl)


def test_stream_law_every_cut_and_close_pairs_of_cuts():
    for keys, repl, text in CASES:
        match, W = fss.oracle_match(orc.AC.compile(keys)), fss.window(keys)
        assert (W == 0) == all(len(k) == 1 for k in keys)
        want = _whole(match, text, repl)
        assert want != text
        lmax = max(len(k) for k in keys)
        for i in range(len(text) + 1):
            assert frs.stream(match, W, _cut(text, [i]), repl) == want, (keys, text, i)
            for j in range(i, min(i + lmax, len(text) + 1)):  # (i == j: an empty piece)
                assert frs.stream(match, W, _cut(text, [i, j]), repl) == want, (keys, text, i, j)
    assert any(fss.window(k) == 0 for k, _, _ in CASES)


def _random_repl(rng, K):
    repl = {}
    for k in range(K):
        r = rng.random()
        if r < 0.4:
            repl[k] = bytes(rng.choice(b"XYZ\x00") for _ in range(rng.randint(1, 9)))
        elif r < 0.6:
            repl[k] = b""
        elif r < 0.7:
            repl[k] = None
    return repl


def _random_keys(rng, max_len):
    keys = set()
    n = min(rng.randint(1, 6), 3 if max_len == 1 else 6)
    while len(keys) < n:
        keys.add(bytes(rng.choice(b"abc") for _ in range(rng.randint(1, max_len))))
    return sorted(keys)


def test_stream_law_random():
    rng = random.Random(8100)
    for case in range(1500):
        keys = _random_keys(rng, 1 if case % 11 == 0 else 6)
        repl = _random_repl(rng, len(keys))
        text = bytes(rng.choice(b"abcx\x00") for _ in range(rng.randint(0, 60)))
        match, W = fss.oracle_match(orc.AC.compile(keys)), fss.window(keys)
        cuts = [rng.randint(0, len(text)) for _ in range(rng.randint(0, 6))]
        assert frs.stream(match, W, _cut(text, cuts), repl) == _whole(match, text, repl), (keys, repl, text, cuts)


def test_model_example_of_the_header():
    keys = [b"ab", b"abcde"]
    q = frs.Sequence(fss.oracle_match(orc.AC.compile(keys)), fss.window(keys))
    repl = {0: b"<AB>", 1: b""}
    assert q.push(b"xab", repl)[:3] == (b"", 3, 0)  # nothing lies in front of F(3) = 0
    assert q.push(b"cd", repl)[:3] == (b"x", 4, 3)
    assert q.push(b"eab", repl)[:3] == (b"", 2, 5)  # the longer key completed at (1, 6): deleted
    assert q.push(b"", repl, final=True)[:3] == (b"<AB>", 0, 8)
    assert q.push(b"ab", repl, final=True)[:3] == (b"<AB>", 0, 0)  # the sequence started again


def test_mixing_select_and_replace_on_the_model():
    keys = [b"ab", b"abcde"]
    q = frs.Sequence(fss.oracle_match(orc.AC.compile(keys)), fss.window(keys))
    repl = {0: b"<AB>", 1: b"!"}
    assert q.select(b"xabc") == ([], 4, 0)
    assert q.select(b"deab") == ([(-3, 2, 1)], 2, 4)  # settled by a select call: no replace call will substitute it
    assert q.push(b"yzw", repl)[:3] == (b"<AB>", 3, 8)  # T[6..8) from where the cursor stood
    assert q.push(b"", repl, final=True)[:3] == (b"yzw", 0, 11)


def test_device_arithmetic_model_against_the_contract():
    rng = random.Random(515)
    for case in range(250):
        keys = _random_keys(rng, 1 if case % 9 == 0 else 6)
        repl = _random_repl(rng, len(keys))
        match, W = fss.oracle_match(orc.AC.compile(keys)), fss.window(keys)
        n_seqs = rng.randint(1, 5)
        a, b = frs.Feed(match, W, n_seqs), frs.DeviceModel(match, W, n_seqs)
        for call in range(rng.randint(1, 6)):
            ids = rng.sample(range(n_seqs), rng.randint(1, n_seqs))
            pieces = [bytes(rng.choice(b"abcx\x00") for _ in range(rng.choice([0, 1, 2, W, W + 1, rng.randint(0, 40)]))) for _ in ids]
            final = call % 3 == 2
            out, poo, bases, hold, n_sel = a.call(pieces, ids, repl, final)
            mout, mpoo, mhold, mn = b.call(pieces, ids, repl, final)
            assert out.tobytes() == mout.tobytes() and np.array_equal(poo, mpoo), (keys, repl, pieces, ids)
            assert np.array_equal(hold, mhold) and n_sel == mn


def test_feed_replace_symbols_exported_declared_listed_and_bound():
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
    assert "aha_feed_replace_batch(" in cxx  # (the C++ mirror wraps the host entries of the feed calls)
    assert re.search(r"#define\s+AHA_FEED_REPLACE_FINAL\s+AHA_FEED_SELECT_FINAL\b", hdr)
    assert N.AHA_FEED_REPLACE_FINAL == N.AHA_FEED_SELECT_FINAL == 1
    assert len(N.SIGNATURES["aha_feed_replace_batch"][1]) == 15 and len(N.SIGNATURES["aha_feed_replace_batch_device"][1]) == 17
    assert N.lib().aha_abi_version() == 8  # a pure addition


def _both(feed, table, n=True, flags=0):
    """rc of the host entry and of the device entry on the same arguments; the buffers stay untouched"""
    corpus = np.frombuffer(b"ushers", dtype=np.uint8).copy()
    offs = np.array([0, corpus.size], dtype=np.uint64)
    ids = np.zeros(1, dtype=np.uint32)
    out = np.full(64, 0x5A, dtype=np.uint8)
    poo = np.full(2, 0x5A5A5A5A, dtype=np.uint64)
    bases = np.full(1, 0x5A5A5A5A, dtype=np.uint64)
    hold = np.full(1, 0x5A5A5A5A, dtype=np.uint32)
    nb = C.c_uint64(7)
    pn = C.byref(nb) if n else None
    L = N.lib()
    rc_h = L.aha_feed_replace_batch(feed, table, corpus.ctypes.data, offs.ctypes.data, ids.ctypes.data, 1, flags, out.ctypes.data,
                                    64, poo.ctypes.data, bases.ctypes.data, hold.ctypes.data, pn, None, None)
    rc_d = L.aha_feed_replace_batch_device(feed, table, corpus.ctypes.data, offs.ctypes.data, ids.ctypes.data, 1, corpus.size,
                                           flags, out.ctypes.data, 64, poo.ctypes.data, bases.ctypes.data, hold.ctypes.data, pn,
                                           None, None, None)
    assert (out == 0x5A).all()
    for a in (poo, bases, hold):
        assert (a == 0x5A5A5A5A).all()
    assert nb.value == 7
    return rc_h, rc_d


def test_feed_replace_argument_checks_before_any_device_work():
    m = AC.compile(["he", "she", "hers"], host_only=True)
    h = C.c_void_p()
    assert N.lib().aha_feed_open(m._h, 4, 0, C.byref(h)) == N.AHA_E_NO_DEVICE and not h.value  # no feed on such a handle
    table = m.replacements({0: "HE"})  # (a table exists on a host-only handle: a host copy only)
    bad = (N.AHA_E_INVALID, N.AHA_E_INVALID)
    assert _both(None, table._h) == bad  # a NULL feed
    assert _both(None, None) == bad  # ... and a NULL table
    assert _both(None, table._h, n=False) == bad  # ... and a NULL n_out_bytes
    for flags in (2, 3, 0x80000000):
        assert _both(None, table._h, flags=flags) == bad
