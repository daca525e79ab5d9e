"""The fold of AHA_OPT_FOLD_BMP (include/aha_hip.h) in plain Python: F3 from str.upper / str.lower, fold3 of one buffer, a batch
folded document by document, and a model of the device pass (aha_amd/csrc/scan_fold.hip: k_fold3_copy, k_fold3_fix) lane by
lane.  Nothing here reads the committed tables (aha_amd/csrc/fold3_table.hpp, fold_table.hpp): the tests compare the two."""
import numpy as np

import foldsim

LO, HI = 0x800, 0x10000  # the code points UTF-8 writes in three bytes
LIVE_LEADS = (0xE1, 0xE2, 0xEA, 0xEF)  # the lead bytes of the characters F3 moves


def surrogate(cp):
    return 0xD800 <= cp < 0xE000


def one3(s):
    return len(s) == 1 and LO <= ord(s) < HI and not surrogate(ord(s))


def F3(c):
    """one character of U+0800 .. U+FFFF (no surrogate) -> its representative, as foldsim.F does it for two bytes"""
    u = c.upper() if one3(c.upper()) else c
    lo = u.lower()
    return lo if one3(lo) else c


_DENSE = []


def dense():
    """F3(cp) at index cp - 0x800, the surrogates as themselves"""
    if not _DENSE:
        _DENSE.extend(cp if surrogate(cp) else ord(F3(chr(cp))) for cp in range(LO, HI))
    return _DENSE


def live_blocks():
    """the blocks cp >> 6 in which some code point moves"""
    t = dense()
    return sorted({(i + LO) >> 6 for i, x in enumerate(t) if x != i + LO})


def enc3(cp):
    return bytes((0xE0 | (cp >> 12), 0x80 | ((cp >> 6) & 0x3F), 0x80 | (cp & 0x3F)))


def is_lead3(b):
    return 0xE0 <= b <= 0xEF


is_lead2, is_cont, fold8 = foldsim.is_lead, foldsim.is_cont, foldsim.fold8


def f3_of(b0, b1, b2):
    """F3 of the triple's code point; an overlong form is itself (and a surrogate, through dense())"""
    cp = ((b0 & 0xF) << 12) | ((b1 & 0x3F) << 6) | (b2 & 0x3F)
    return cp if cp < LO else dense()[cp - LO]


def fold3(buf):
    """bytes -> bytes of the same length: at every position the first of triple, pair, fold8 that applies"""
    b = bytes(buf)
    n = len(b)
    out = bytearray(n)
    j = 0
    while j < n:
        if is_lead3(b[j]) and j + 2 < n and is_cont(b[j + 1]) and is_cont(b[j + 2]):
            out[j:j + 3] = enc3(f3_of(b[j], b[j + 1], b[j + 2]))
            j += 3
        elif is_lead2(b[j]) and j + 1 < n and is_cont(b[j + 1]):
            out[j:j + 2] = foldsim.fold2(b[j:j + 2])
            j += 2
        else:
            out[j] = fold8(b[j])
            j += 1
    return bytes(out)


def fold3_docs(corpus, off):
    """the batch in which each document is folded on its own; corpus: bytes or a uint8 array, off: D + 1 offsets"""
    b = bytes(np.asarray(corpus, dtype=np.uint8).tobytes()) if not isinstance(corpus, (bytes, bytearray)) else bytes(corpus)
    off = [int(x) for x in off]
    out = bytearray(b)
    for d in range(len(off) - 1):
        out[off[d]:off[d + 1]] = fold3(b[off[d]:off[d + 1]])
    return bytes(out)


def fold3_keys(keys):
    return [fold3(k.encode() if isinstance(k, str) else k) for k in keys]


def fold3_byte(prev2, prev, cur, nxt, nxt2):
    """one byte of fold3 from the byte and its two neighbours on each side (0 where there is none), as every lane that owns a
    byte of a triple computes it"""
    if is_lead3(cur) and is_cont(nxt) and is_cont(nxt2):
        return 0xE0 | (f3_of(cur, nxt, nxt2) >> 12)
    if is_cont(cur):
        if is_lead3(prev) and is_cont(nxt):
            return 0x80 | ((f3_of(prev, cur, nxt) >> 6) & 0x3F)
        if is_cont(prev) and is_lead3(prev2):
            return 0x80 | (f3_of(prev2, prev, cur) & 0x3F)
    return foldsim.fold2_byte(foldsim.table(), prev, cur, nxt)


def live_lead(b):
    return is_lead2(b) or b in LIVE_LEADS


def kernel_model(buf, off, piece=16, wave=64, grid=1, block=256, live_test=False):
    """k_fold3_copy + k_fold3_fix as the lanes do them.  buf: the n source bytes (nothing outside [0, n) is ever indexed: the
    loads go through `load`, which asserts it); off: the documents' offsets (off[0] is subtracted).  Lane g = blockIdx * block +
    threadIdx owns the pieces g, g + grid * block, ..; it loads its own piece; the two bytes before it only when the piece opens
    with a continuation byte; the byte after it only when the piece ends with a lead byte or with the first two bytes of a
    triple, the second byte after it only when the piece ends with a triple's lead byte; with live_test (the kernel's opt-in instantiation) it is then done (fold8
    of every byte) when neither the piece nor the two bytes before it hold a lead byte of a character that can move; and it
    writes its own bytes only.  Lanes 0 .. piece - 1 of block 0 own the n % piece tail, byte by byte.  Then a lane per interior document
    boundary puts the source bytes back where a pair or a triple lay across it.
    -> (dst as bytes, stats: neighbour loads in all, those that cross a wave's edge, those that reach a piece a stride away,
    pieces that took the fast way out of the live-lead test)"""
    src = bytes(buf)
    n = len(src)
    dst = [None] * n
    stats = {"neighbour_loads": 0, "cross_wave": 0, "cross_stride": 0, "not_live": 0}

    def load(j):
        assert 0 <= j < n, j
        return src[j]

    def neighbour(j, own_piece):
        stats["neighbour_loads"] += 1
        other = j // piece  # (the piece that holds the neighbour; none: it lies in the tail)
        if other < n // piece and other // wave != own_piece // wave:
            stats["cross_wave"] += 1
        if other < n // piece and other // (grid * block) != own_piece // (grid * block):
            stats["cross_stride"] += 1
        return load(j)

    pieces, stride = n // piece, grid * block
    for lane in range(min(stride, pieces)):
        for i in range(lane, pieces, stride):
            j0 = i * piece
            v = [load(j0 + k) for k in range(piece)]
            if not any(x & 0x80 for x in v):
                out = [fold8(x) for x in v]
            else:
                prev2 = prev = nxt = nxt2 = 0  # kc_fold3_halo: all four decided and loaded before anything is folded
                if is_cont(v[0]) and j0 > 0:
                    prev, prev2 = neighbour(j0 - 1, i), neighbour(j0 - 2, i)
                b14, b15 = v[piece - 2], v[piece - 1]
                if (is_lead2(b15) or is_lead3(b15) or (is_lead3(b14) and is_cont(b15))) and j0 + piece < n:
                    nxt = neighbour(j0 + piece, i)
                if is_lead3(b15) and j0 + piece + 1 < n:
                    nxt2 = neighbour(j0 + piece + 1, i)
                if live_test and not any(live_lead(x) for x in v) and not live_lead(prev) and not live_lead(prev2):
                    stats["not_live"] += 1
                    out = [fold8(x) for x in v]
                else:
                    w = [prev2, prev] + v + [nxt, nxt2]
                    out = [fold3_byte(w[k], w[k + 1], w[k + 2], w[k + 3], w[k + 4]) for k in range(piece)]
            for k in range(piece):
                assert dst[j0 + k] is None  # every byte has one owner
                dst[j0 + k] = out[k]
    for t in range(piece):  # the tail: block 0, lanes 0 .. piece - 1
        j = pieces * piece + t
        if j < n:
            assert dst[j] is None
            dst[j] = fold3_byte(load(j - 2) if j > 1 else 0, load(j - 1) if j > 0 else 0, load(j), load(j + 1) if j + 1 < n else 0,
                                load(j + 2) if j + 2 < n else 0)
    assert all(x is not None for x in dst)
    off = [int(x) for x in off]
    for d in range(1, len(off) - 1):  # k_fold3_fix: a lane per interior boundary
        b = off[d] - off[0]
        if not 0 < b < n:
            continue
        before, at = load(b - 1), load(b)
        if not is_cont(at):
            continue
        if is_lead2(before):
            dst[b - 1], dst[b] = before, at
        elif is_lead3(before):
            if b + 1 < n and is_cont(load(b + 1)):
                dst[b - 1], dst[b], dst[b + 1] = before, at, load(b + 1)
        elif is_cont(before) and b >= 2 and is_lead3(load(b - 2)):
            dst[b - 2], dst[b - 1], dst[b] = load(b - 2), before, at
    return bytes(dst), stats
