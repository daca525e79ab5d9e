"""CPU tests of the feed grep calls (aha_feed_grep_batch, aha_feed_grep_batch_device): exported, declared, listed and bound; the
argument checks that come before any device work; the call-by-call model (feedgrepsim: the X / Y / Z arithmetic and the state
transitions) against the whole-sequence definition for EVERY cut of short texts into two and into three pieces, on the CPU
oracle's hits; and the arithmetic of the Python Grepper with a stand-in feed that answers from the model."""
import ctypes as C
import os
import random
import re

import numpy as np

import feedgrepsim as fgs
import pyoracle as orc
from aha_amd import AC, Grepper
from aha_amd import _native as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("aha_feed_grep_batch", "aha_feed_grep_batch_device")


def test_feed_grep_symbols_exported_declared_and_bound():
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
    assert "aha_feed_grep_batch(" in cxx  # (the C++ mirror wraps the host entries of the feed calls)
    # the two flags share one word: FINAL stands beside INVERT
    assert re.search(r"#define\s+AHA_FEED_GREP_FINAL\s+2u", hdr) and N.AHA_FEED_GREP_FINAL == 2 and N.AHA_GREP_INVERT == 1
    assert N.lib().aha_abi_version() == 8  # a pure addition
    from aha_amd import Feed

    for method in ("grep_batch", "grep_batch_device", "grepper"):
        assert callable(getattr(Feed, method))
    for method in ("push", "finish"):
        assert callable(getattr(Grepper, method))


def _both(feed, n=True, flags=0):
    """rc of the host entry and of the device entry on the same arguments; the buffers stay untouched"""
    corpus = np.frombuffer(b"ab\ncd", dtype=np.uint8).copy()
    offs = np.array([0, corpus.size], dtype=np.uint64)
    ids = np.zeros(1, dtype=np.uint32)
    G = 0x5A5A5A5A
    kept, roo = np.full(8, G, dtype=np.uint64), np.full(9, G, dtype=np.uint64)
    out = np.full(16, 0x5A, dtype=np.uint8)
    per = [np.full(2, G, dtype=np.uint64) for _ in range(5)]
    hold = np.full(1, G, dtype=np.uint32)
    nr, nk, nb = C.c_uint64(7), C.c_uint64(7), C.c_uint64(7)
    pn = C.byref(nk) if n else None
    L = N.lib()
    p = [a.ctypes.data for a in per]
    rc_h = L.aha_feed_grep_batch(feed, corpus.ctypes.data, offs.ctypes.data, ids.ctypes.data, 1, 10, flags, kept.ctypes.data,
                                 roo.ctypes.data, 8, out.ctypes.data, 16, p[0], p[1], hold.ctypes.data, p[2], p[3], p[4],
                                 C.byref(nr), pn, C.byref(nb), None)
    rc_d = L.aha_feed_grep_batch_device(feed, corpus.ctypes.data, offs.ctypes.data, ids.ctypes.data, 1, corpus.size, 10, flags,
                                        kept.ctypes.data, roo.ctypes.data, 8, out.ctypes.data, 16, p[0], p[1], hold.ctypes.data,
                                        p[2], p[3], p[4], C.byref(nr), pn, C.byref(nb), None, None)
    for a in [kept, roo, hold] + per:
        assert (a == G).all()
    assert (out == 0x5A).all() and nr.value == 7 and nk.value == 7 and nb.value == 7
    return rc_h, rc_d


def test_feed_grep_argument_checks_before_any_device_work():
    m = AC.compile(["ab", "b\n"], host_only=True)
    h = C.c_void_p()
    assert N.lib().aha_feed_open(m._h, 4, 0, C.byref(h)) == N.AHA_E_NO_DEVICE and not h.value  # no feed on such a handle
    assert _both(None) == (N.AHA_E_INVALID, N.AHA_E_INVALID)  # a NULL feed
    assert _both(None, n=False) == (N.AHA_E_INVALID, N.AHA_E_INVALID)  # ... and a NULL n_kept
    for flags in (1, 2, 3, 4, 0x80000000):
        assert _both(None, flags=flags) == (N.AHA_E_INVALID, N.AHA_E_INVALID)


# ---- the model against the whole-sequence definition, on the oracle's hits -------------------------------------------------
def _cut(text, cuts):
    at = [0] + sorted(cuts) + [len(text)]
    return [text[at[i]:at[i + 1]] for i in range(len(at) - 1)]


class _Law:
    def __init__(self, keys, fold=False):
        self.keys = keys
        self.count = fgs.oracle_count(orc.AC.compile([k.lower() for k in keys] if fold else keys), fold)
        self.W = fgs.window(keys)
        self._want = {}

    def check(self, text, cuts, delim=b"\n", invert=False):
        key = (text, delim, invert)
        if key not in self._want:
            self._want[key] = fgs.whole(self.count, text, delim, invert)
        got = fgs.stream(self.count, self.W, _cut(text, cuts), delim, invert)
        assert got == self._want[key], (self.keys, text, cuts, delim, invert, got, self._want[key])

    def every_cut(self, text, delim=b"\n", inverts=(False, True)):
        for invert in inverts:
            for i in range(len(text) + 1):
                self.check(text, [i], delim, invert)
                for j in range(i, len(text) + 1):
                    self.check(text, [i, j], delim, invert)  # (i == j: an empty piece; j == len: an empty piece under FINAL)


def test_the_three_traps_whole_sequence():
    c = fgs.oracle_count(orc.AC.compile([b"abc", b"b"]))
    assert c(b"ab\n") == 0 and c(b"b\n") == 1  # the record has no hit, the fragment from the root has one
    assert fgs.whole(c, b"ab\n") == [] and fgs.stream(c, 2, [b"a", b"b\n"]) == []
    o = orc.AC.compile([b"x\nabc", b"b"])
    c = fgs.oracle_count(o)
    assert c(b"ab\n") == 1 and len(o.match(b"x\nab\n", chars=False)) == 0  # the record has a hit, the sequence has none
    assert fgs.whole(c, b"x\nab\n") == [b"ab\n"]
    assert fgs.stream(c, 4, [b"x\na", b"b\n"]) == [b"ab\n"] and fgs.stream(c, 4, [b"x\n", b"ab", b"\n"]) == [b"ab\n"]
    c = fgs.oracle_count(orc.AC.compile([b"\nb"]))
    assert fgs.whole(c, b"a\nb\nb") == [] and fgs.stream(c, 1, [b"a\n", b"b\nb"]) == []  # never inside a record
    c = fgs.oracle_count(orc.AC.compile([b"b\n"]))
    assert fgs.whole(c, b"ab\nb") == [b"ab\n"] and fgs.stream(c, 1, [b"ab", b"\nb"]) == [b"ab\n"]  # only at a record's end


def test_model_equals_the_definition_for_every_cut_into_two_and_three():
    cases = [
        ([b"abc", b"b"], [b"ab\nab\nabc\n", b"a\nb\nab"]),               # trap 1
        ([b"x\nabc", b"b"], [b"x\nab\nx\nabc\n", b"x\nab"]),              # trap 2
        ([b"\nb"], [b"a\nb\nb\n", b"\nb\n\nb"]),                          # trap 3: never in a record
        ([b"b\n"], [b"ab\nb", b"b\n\nb\n"]),                              # ... only at a record's end
        ([b"abcabcab"], [b"xabcabcab\nabcabca\nb", b"abcabcabcabcab\n"]),  # a key longer than a piece
        ([b"a", b"c"], [b"b\na\n\ncb\nb", b"\n\n\n"]),                    # W = 0
        ([b"a\x01b", b"b"], [b"a\x00b\n\x00a\x01\n\x00\x00", b"\x00\na\x01b\x00"]),  # NUL bytes in the text
        ([b"ab", b"bca", b"c"], [b"abca\n", b"abca", b"", b"\n", b"c"]),    # with and without a trailing delimiter, tiny texts
        ([b"aab", b"ba"], [b"aabaab\nxx\nbaab\n"]),
    ]
    for keys, texts in cases:
        law = _Law(keys)
        for text in texts:
            law.every_cut(text)
    law = _Law([b"abc", b"b"])  # (a key holds no NUL; the delimiter may be NUL)
    law.every_cut(b"ab\x00b\x00\x00abc", delim=b"\x00")
    law = _Law([b"aBc", b"B"], fold=True)  # a folded handle: ABC = abc
    for text in (b"Ab\naB\nABc\n", b"a\nb\nAbC"):
        law.every_cut(text)


def test_a_record_over_four_pieces_and_the_carried_hit():
    law = _Law([b"abc", b"cab"])
    law.check(b"xxabcxxxxxxx\nq\n", [3, 6, 9])  # the hit lies in the first two pieces only: open_hit carried over two calls
    law.check(b"xxabcxxxxxxx\nq\n", [3, 6, 9], invert=True)
    law.check(b"xxxxxxxxxcab\n", [3, 6, 10])  # a hit only in the last straddle
    law.check(b"xxxxxxxxxxxx", [3, 6, 9])  # never closed before FINAL
    q = fgs.Sequence(law.count, law.W)
    assert q.push(b"xa")[2:4] == (2, 0) and not q.open_hit
    assert q.push(b"bc")[2:4] == (2, 0) and q.open_hit and q.open_len == 4  # the straddle "abc"
    assert q.push(b"")[2:4] == (0, 0) and q.open_hit and q.open_len == 4  # an empty piece in the middle of a record
    assert q.push(b"yyyy")[2:4] == (4, 0) and q.open_hit and q.open_len == 8 and q.recs == 0
    frags, keep, hold, head, base, rec_base = q.push(b"z\nq")
    assert (frags, keep, hold, head, base, rec_base) == ([b"z\n", b"q"], [True, False], 1, 8, 8, 0)
    assert (q.open_len, q.open_hit, q.recs, q.seen) == (1, False, 1, 11)
    assert q.push(b"", final=True)[1:4] == ([], 0, 0)  # the open record "q" closes without a fragment and is dropped
    assert (q.open_len, q.recs, q.seen) == (0, 0, 0)
    q.push(b"cab")
    assert q.push(b"", final=True)[1:4] == ([], 0, 3)  # ... and kept: it appears only as piece_head


def test_model_random_cuts_and_invariants():
    rng = random.Random(20261)
    for case in range(1500):
        alphabet = b"abc\n" + (b"\x00" if case % 3 == 0 else b"")
        lmax = 1 if case % 11 == 0 else rng.choice([2, 3, 5])
        keys = sorted({bytes(rng.choice(b"abc\n") for _ in range(rng.randint(1, lmax))) for _ in range(rng.randint(1, 5))})
        law = _Law(keys)
        text = bytes(rng.choices(alphabet, [4, 3, 2, 2, 1][: len(alphabet)])[0] for _ in range(rng.randint(0, 40)))
        cuts = [rng.randint(0, len(text)) for _ in range(rng.randint(0, 6))]
        invert = case % 2 == 1
        law.check(text, cuts, invert=invert)
        # what the outputs promise
        q = fgs.Sequence(law.count, law.W)
        pieces = _cut(text, cuts)
        for i, p in enumerate(pieces):
            final = i == len(pieces) - 1
            open_before = q.open_len
            frags, keep, hold, head, base, rec_base = q.push(p, b"\n", invert, final)
            closed = sum(1 for f in frags if final or f.endswith(b"\n"))
            assert hold == 0 if final else (hold == len(p)) == (closed == 0)
            assert head in (0, open_before) and b"".join(frags) == p
            assert base == sum(len(x) for x in pieces[:i]) and rec_base == text[:base].count(b"\n")


# ---- the Grepper's arithmetic, on a stand-in feed --------------------------------------------------------------------------
class _ModelFeed:
    """what Grepper needs of a Feed, answered by the model"""

    def __init__(self, keys):
        self._m = fgs.Feed(fgs.oracle_count(orc.AC.compile(keys)), fgs.window(keys), 4)

    def grep_batch(self, corpus, piece_offsets, seq_ids, delim=b"\n", invert=False, final=False):
        assert len(seq_ids) == 1 and int(piece_offsets[0]) == 0
        return self._m.call([np.asarray(corpus, dtype=np.uint8).tobytes()], [int(seq_ids[0])], delim, invert, final)


def test_grepper_arithmetic_against_the_definition():
    rng = random.Random(77)
    for case in range(400):
        keys = sorted({bytes(rng.choice(b"abc\n") for _ in range(rng.randint(1, 4))) for _ in range(rng.randint(1, 4))})
        count = fgs.oracle_count(orc.AC.compile(keys))
        text = bytes(rng.choices(b"abc\n", [4, 3, 2, 2])[0] for _ in range(rng.randint(0, 50)))
        invert = case % 3 == 0
        g = Grepper(_ModelFeed(keys), b"\n", invert)
        seq = case % 4
        got = []
        for p in _cut(text, [rng.randint(0, len(text)) for _ in range(rng.randint(0, 5))]):
            got += g.push(seq, p)
            assert len(g._held.get(seq, b"")) == g._feed._m.seqs[seq].open_len
        got += g.finish(seq)
        assert got == fgs.whole(count, text, b"\n", invert), (keys, text, invert)
        assert seq not in g._held
    # str pieces are UTF-8
    g = Grepper(_ModelFeed(["中".encode()]))
    assert g.push(0, "我是\n中") + g.push(0, "国\n人") + g.finish(0) == ["中国\n".encode()]
