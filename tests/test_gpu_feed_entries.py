"""The two entries of every feed family (aha_feed_*_batch and aha_feed_*_batch_device) give the same answer: the same small
batches go through the host entry on one feed and the device entry on a second feed of the same handle, and every returned
array, every count and every status must be equal -- with all optional outputs given, and with all of them null.  A capacity
round trip per family that has one: a cap one below the required size is AHA_E_CAPACITY with the same required size from both
entries, and aha_feed_position is unchanged afterwards.  Nothing here is compared with a model (the other feed tests do that):
this pins what the entries share -- staging, read-backs, the order of refusals -- whatever shape their code has."""
import ctypes as C
from collections import namedtuple

import numpy as np
import pytest

from aha_amd import AC, BitArray
from aha_amd import _native as N

pytestmark = pytest.mark.gpu

KEYS = [b"a", b"ab", b"bcd", b"cdefg", b"e f"]  # 1 to 5 bytes, "a" a prefix of "ab"
P7 = b"g e f a"  # after P40: "cdef|g"; before it: "a|b", and the sequence so far ends with a key
P40 = b"bcd ab\ncdefg e f\n\nxa ab e f abcd\n a cdef"
assert len(P7) == 7 and len(P40) == 40
A = (b"", P7, P40)
# (pieces, sequence ids, last): the same three pieces to every sequence in turn, so keys straddle the cuts between calls; then
# no piece at all; then empty pieces alone -- with the family's FINAL flag where it has one
BATCHES = [(A, [1, 2, 0], False), (A, [2, 0, 1], False), (A, [0, 1, 2], False), ((), [], False), ((b"", b"", b""), [0, 1, 2], True)]
HITS, BYTES = 256, 1024  # room for whatever these batches give

Result = namedtuple("Result", "rc counts arrays")
_TORCH = {1: np.uint8, 4: np.int32, 8: np.int64}


def _run(name, f, dev, mid, n_counts, pre=(), pieces=None, ids=()):
    """one call of entry `name` (dev: its _device form).  mid: the arguments between the pieces and the counts -- a number goes
    as it is, None is a null pointer, (dtype, n) is an output array of n zeroed entries -> (status, the counts, the arrays)"""
    import torch

    def mem(a):  # -> (what keeps the memory alive, its address); never a null pointer
        a = np.ascontiguousarray(a)
        a = a if a.size else np.zeros(1, dtype=a.dtype)
        if not dev:
            return a, a.ctypes.data
        t = torch.from_numpy(a.view(_TORCH[a.itemsize]).copy()).to("cuda:0")
        return t, t.data_ptr()

    held = [mem(np.array(ids, dtype=np.uint32))]
    args = [f._h, *pre]
    if pieces is None:  # a finish call names sequences only
        args += [held[0][1] if len(ids) else None, len(ids)]
    else:
        corpus = np.frombuffer(b"".join(pieces), dtype=np.uint8)
        held += [mem(corpus), mem(np.cumsum([0] + [len(p) for p in pieces]).astype(np.uint64))]
        args += [held[1][1] if corpus.size else None, held[2][1], held[0][1] if len(ids) else None, len(pieces)]
        if dev:
            args.append(corpus.size)
    outs = []
    for m in mid:
        if isinstance(m, tuple):
            outs.append(mem(np.zeros(max(m[1], 1), dtype=m[0])))
            args.append(outs[-1][1])
        else:
            args.append(m)
    counts = [C.c_uint64(0) for _ in range(n_counts)]
    args += [C.byref(c) for c in counts]
    if dev:
        args.append(None)  # the null stream
    rc = getattr(N.lib(), name + ("_device" if dev else ""))(*args)
    if dev:
        torch.cuda.synchronize()
    return Result(rc, [int(c.value) for c in counts], [o[0].cpu().numpy() if dev else o[0] for o in outs])


def _positions(f):
    out = []
    for s in range(f.n_seqs):
        b, c = C.c_uint64(0), C.c_uint64(0)
        assert N.lib().aha_feed_position(f._h, s, C.byref(b), C.byref(c)) == N.AHA_OK
        out.append((b.value, c.value))
    return out


# per family: mid(D, N, w, cap, last) -> the middle arguments (w: the optional outputs are given; cap: the capacities),
# n_counts, and per capacity (the count that reports what is required, room for any of these batches)
def _opt(w, dtype, n):
    return (dtype, n) if w else None


FAMILIES = {
    "match": (lambda D, N_, w, cap, last: [("i4", 3 * cap[0]), cap[0], _opt(w, "u8", D + 1), _opt(w, "u8", D)], 1, [(0, HITS)]),
    "finish": (lambda D, N_, w, cap, last: [("i4", 3 * cap[0]), cap[0], _opt(w, "u8", D + 1), _opt(w, "u8", D)], 1, [(0, HITS)]),
    "count": (lambda D, N_, w, cap, last: [0, _opt(w, "u8", len(KEYS)), _opt(w, "u8", D + 1), _opt(w, "u8", D)], 1, []),
    "cover": (lambda D, N_, w, cap, last: [0, _opt(w, "u4", (N_ + 31) // 32), _opt(w, "u1", N_), 0x2A, _opt(w, "u4", D),
                                           _opt(w, "u8", D), _opt(w, "u8", D + 1), _opt(w, "u8", D)], 2, []),
    "select": (lambda D, N_, w, cap, last: [N.AHA_FEED_SELECT_FINAL if last else 0, ("i4", 3 * cap[0]), cap[0],
                                            _opt(w, "u8", D + 1), _opt(w, "u8", D), _opt(w, "u4", D)], 2, [(0, HITS)]),
    "replace": (lambda D, N_, w, cap, last: [N.AHA_FEED_REPLACE_FINAL if last else 0, ("u1", cap[0]), cap[0], _opt(w, "u8", D + 1),
                                             _opt(w, "u8", D), _opt(w, "u4", D)], 3, [(0, BYTES)]),
    # (null: no kept list, no offsets and no bytes either, so no capacity)
    "grep": (lambda D, N_, w, cap, last: [0x0A, N.AHA_FEED_GREP_FINAL if last else 0, _opt(w, "u8", cap[0]), _opt(w, "u8", cap[0] + 1),
                                          cap[0] if w else 0, _opt(w, "u1", cap[1]), cap[1] if w else 0, _opt(w, "u8", D + 1),
                                          _opt(w, "u8", D + 1), _opt(w, "u4", D), _opt(w, "u8", D), _opt(w, "u8", D),
                                          _opt(w, "u8", D)], 4, [(1, HITS), (2, BYTES)]),
}


def _both(family, fh, fd, w, cap, pieces, ids, last, pre):
    """the same call through the host entry on fh and the device entry on fd; everything they return must be equal"""
    mid, n_counts, _ = FAMILIES[family]
    D = len(ids)
    m = mid(D, sum(len(p) for p in pieces or ()), w, cap, last)
    h = _run("aha_feed_%s_batch" % family, fh, False, m, n_counts, pre, pieces, ids)
    d = _run("aha_feed_%s_batch" % family, fd, True, m, n_counts, pre, pieces, ids)
    assert h.rc == d.rc and h.counts == d.counts, (family, ids, cap, h.rc, d.rc, h.counts, d.counts)
    assert len(h.arrays) == len(d.arrays)
    for i, (x, y) in enumerate(zip(h.arrays, d.arrays)):
        assert x.tobytes() == y.tobytes(), (family, ids, cap, i)
    assert _positions(fh) == _positions(fd)
    return h


def _round_trip(family, fh, fd, pieces, ids, last, pre):
    """a sizing call, then for each capacity a call one below what is required: AHA_E_CAPACITY with the same required sizes
    from both entries, and no sequence has moved; then the call that fits"""
    caps = FAMILIES[family][2]
    before = _positions(fh)
    r = _both(family, fh, fd, True, [0] * len(caps), pieces, ids, last, pre)
    assert r.rc == N.AHA_E_CAPACITY, (family, r)
    need = [r.counts[i] for i, _ in caps]
    assert all(n >= 1 for n in need), (family, need)
    for k in range(len(caps)):
        r = _both(family, fh, fd, True, [n - (j == k) for j, n in enumerate(need)], pieces, ids, last, pre)
        assert r.rc == N.AHA_E_CAPACITY and [r.counts[i] for i, _ in caps] == need, (family, k, r)
        assert _positions(fh) == before and _positions(fd) == before
    r = _both(family, fh, fd, True, need, pieces, ids, last, pre)
    assert r.rc == N.AHA_OK and [r.counts[i] for i, _ in caps] == need, (family, r)
    assert _positions(fh) != before


@pytest.fixture(scope="module")
def handle():
    return AC.compile(KEYS)


def _feed(m, kind):
    if kind == "sep":
        sep = BitArray(128)
        for c in range(128):
            sep[c] = not chr(c).isalnum()
        return m.feed(3, sep=sep)
    return m.feed(3, longest=1 if kind == "longest" else 0)


@pytest.mark.parametrize("family,kind", [("match", "plain"), ("count", "plain"), ("cover", "plain"), ("select", "plain"),
                                         ("replace", "plain"), ("grep", "plain"), ("match", "sep"), ("count", "sep"),
                                         ("match", "longest")])
@pytest.mark.parametrize("w", [True, False], ids=["given", "null"])
def test_host_and_device_entries_agree(handle, family, kind, w):
    fh, fd = _feed(handle, kind), _feed(handle, kind)
    table = handle.replacements({0: b"X", 2: b"", 3: b"a longer text"})  # (the name keeps it alive)
    pre = (table._h,) if family == "replace" else ()
    room = [c for _, c in FAMILIES[family][2]]
    for b, (pieces, ids, last) in enumerate(BATCHES):
        if b == 0 and w and room:
            _round_trip(family, fh, fd, pieces, ids, last, pre)
        else:
            r = _both(family, fh, fd, w, room, pieces, ids, last, pre)
            assert r.rc == N.AHA_OK, (family, kind, b, r)


@pytest.mark.parametrize("kind", ["sep", "longest"])
@pytest.mark.parametrize("w", [True, False], ids=["given", "null"])
def test_finish_entries_agree(handle, kind, w):
    fh, fd = _feed(handle, kind), _feed(handle, kind)
    for pieces, ids, last in BATCHES:
        assert _both("match", fh, fd, True, [HITS], pieces, ids, last, ()).rc == N.AHA_OK
    assert _both("finish", fh, fd, w, [HITS], None, [], False, ()).rc == N.AHA_OK  # no sequence named
    if w:  # (sequences 0 and 1 end with a key: something is reported)
        _round_trip("finish", fh, fd, None, [1, 0], False, ())
    else:
        assert _both("finish", fh, fd, w, [HITS], None, [1, 0], False, ()).rc == N.AHA_OK
    assert [p[0] for p in _positions(fh)] == [0, 0, 47]  # (a finished sequence starts again)
    assert _both("finish", fh, fd, w, [HITS], None, [2], False, ()).rc == N.AHA_OK
    assert [p[0] for p in _positions(fh)] == [0, 0, 0]
