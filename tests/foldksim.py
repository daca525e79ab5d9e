"""The fold of AHA_OPT_FOLD_KANA (include/aha_hip.h) in plain Python: K from unicodedata, FK = K over fold3sim's F3, foldk of one
buffer, a batch folded document by document, and a model of the device pass (aha_amd/csrc/scan_foldk.hip: k_foldk_copy in both
halo forms, then scan_fold.hip's k_fold3_fix) lane by lane.  Nothing here reads the committed tables (aha_amd/csrc/foldk_table.hpp): the tests
compare the two."""
import unicodedata

import numpy as np

import fold3sim
import foldsim

LO, HI = fold3sim.LO, fold3sim.HI
enc3, is_lead3 = fold3sim.enc3, fold3sim.is_lead3
is_lead2, is_cont, fold8 = foldsim.is_lead, foldsim.is_cont, foldsim.fold8

_K = {}


def K():
    """the 144 code points the kana fold moves, as a dict cp -> katakana cp"""
    if not _K:
        for cp in range(0x3041, 0x3097):  # hiragana -> katakana
            _K[cp] = cp + 0x60
        _K[0x309D], _K[0x309E] = 0x30FD, 0x30FE  # the iteration marks
        for cp in range(0xFF66, 0xFF9E):  # half-width katakana -> the one code point NFKC gives
            s = unicodedata.normalize("NFKC", chr(cp))
            assert len(s) == 1, hex(cp)
            _K[cp] = ord(s)
    return _K


def FK(c):
    """one character of U+0800 .. U+FFFF (no surrogate) -> its representative"""
    k = K().get(ord(c))
    return chr(k) if k is not None else fold3sim.F3(c)


_DENSE = []


def dense():
    """FK(cp) at index cp - 0x800, the surrogates as themselves"""
    if not _DENSE:
        t = list(fold3sim.dense())
        for cp, v in K().items():
            t[cp - LO] = v
        _DENSE.extend(t)
    return _DENSE


def live_blocks():
    t = dense()
    return sorted({(i + LO) >> 6 for i, x in enumerate(t) if x != i + LO})


def fk_of(b0, b1, b2):
    """FK of the triple's code point; an overlong form is itself (and a surrogate, through dense())"""
    cp = ((b0 & 0xF) << 12) | ((b1 & 0x3F) << 6) | (b2 & 0x3F)
    return cp if cp < LO else dense()[cp - LO]


def foldk(buf):
    """bytes -> bytes of the same length: at every position the first of triple, pair, fold8 that applies"""
    b = bytes(buf)
    n = len(b)
    out = bytearray(n)
    j = 0
    while j < n:
        if is_lead3(b[j]) and j + 2 < n and is_cont(b[j + 1]) and is_cont(b[j + 2]):
            out[j:j + 3] = enc3(fk_of(b[j], b[j + 1], b[j + 2]))
            j += 3
        elif is_lead2(b[j]) and j + 1 < n and is_cont(b[j + 1]):
            out[j:j + 2] = foldsim.fold2(b[j:j + 2])
            j += 2
        else:
            out[j] = fold8(b[j])
            j += 1
    return bytes(out)


def foldk_docs(corpus, off):
    """the batch in which each document is folded on its own; corpus: bytes or a uint8 array, off: D + 1 offsets"""
    b = bytes(np.asarray(corpus, dtype=np.uint8).tobytes()) if not isinstance(corpus, (bytes, bytearray)) else bytes(corpus)
    off = [int(x) for x in off]
    out = bytearray(b)
    for d in range(len(off) - 1):
        out[off[d]:off[d + 1]] = foldk(b[off[d]:off[d + 1]])
    return bytes(out)


def foldk_keys(keys):
    return [foldk(k.encode() if isinstance(k, str) else k) for k in keys]


def foldk_byte(prev2, prev, cur, nxt, nxt2):
    """one byte of foldk from the byte and its two neighbours on each side (0 where there is none)"""
    if is_lead3(cur) and is_cont(nxt) and is_cont(nxt2):
        return 0xE0 | (fk_of(cur, nxt, nxt2) >> 12)
    if is_cont(cur):
        if is_lead3(prev) and is_cont(nxt):
            return 0x80 | ((fk_of(prev, cur, nxt) >> 6) & 0x3F)
        if is_cont(prev) and is_lead3(prev2):
            return 0x80 | (fk_of(prev2, prev, cur) & 0x3F)
    return foldsim.fold2_byte(foldsim.table(), prev, cur, nxt)


def kernel_model(buf, off, halo="mem", piece=16, wave=64, grid=1, block=256):
    """k_foldk_copy<halo> + k_fold3_fix as the lanes do them.  buf: the n source bytes (nothing outside [0, n) is ever indexed:
    every load goes through `load`, which asserts it); off: the documents' offsets (off[0] is subtracted).

    Lane g = blockIdx * block + threadIdx starts at piece g and moves by stride = grid * block.
    halo == "mem": a lane takes its pieces while it has one (four at a time, then one at a time: the same pieces) and loads the
    bytes around a piece from src where they decide something (kc_fold3_halo).
    halo == "lane": a WAVE takes a step with all its lanes or not at all -- four pieces per lane while the wave's last lane
    has its fourth one, then one piece per lane while the wave's first lane has one; a lane past the end loads and stores
    nothing but hands over zeros.  The two bytes in front of a piece are bytes 14, 15 of the lane below, the two behind it bytes
    0, 1 of the lane above, whatever they are; only lane 0 of a wave loads the bytes in front from src, only lane wave - 1 and a
    lane whose neighbour above has no piece the bytes behind, under kc_fold3_halo's conditions.  The model asserts that every
    lane of a wave is present at every exchange and that a lane reads only lanes of its own wave.

    Lanes 0 .. piece - 1 of block 0 own the n % piece tail, byte by byte.  Then a lane per interior document boundary puts the
    source bytes back where a pair or a triple lay across it.
    -> (dst as bytes, stats: neighbour loads from src, pieces whose halo came from the neighbouring lanes alone, unrolled and
    remainder steps taken by waves, lanes that stood by without a piece)"""
    assert halo in ("mem", "lane") and block % wave == 0
    src = bytes(buf)
    n = len(src)
    dst = [None] * n
    stats = {"neighbour_loads": 0, "from_lanes": 0, "unrolled": 0, "remainder": 0, "idle_lanes": 0}

    def load(j):
        assert 0 <= j < n, j
        return src[j]

    def neighbour(j):
        stats["neighbour_loads"] += 1
        return load(j)

    pieces, stride = n // piece, grid * block

    def front(i, v):
        if is_cont(v[0]) and i > 0:
            return [neighbour(i * piece - 2), neighbour(i * piece - 1)]
        return [0, 0]

    def back(i, v):
        j0 = i * piece
        b14, b15 = v[piece - 2], v[piece - 1]
        h = [0, 0]
        if (is_lead2(b15) or is_lead3(b15) or (is_lead3(b14) and is_cont(b15))) and j0 + piece < n:
            h[0] = neighbour(j0 + piece)
        if is_lead3(b15) and j0 + piece + 1 < n:
            h[1] = neighbour(j0 + piece + 1)
        return h

    def apply(v, h):
        if not any(x & 0x80 for x in v):
            return [fold8(x) for x in v]
        w = h[:2] + v + h[2:]
        return [foldk_byte(w[k], w[k + 1], w[k + 2], w[k + 3], w[k + 4]) for k in range(piece)]

    def store(i, out):
        for k in range(piece):
            assert dst[i * piece + k] is None  # every byte has one owner
            dst[i * piece + k] = out[k]

    def wave_step(i0):
        """the `wave` lanes whose first lane is on piece i0 (which may be past the end for some of them) do one piece each"""
        own = [i0 + t < pieces for t in range(wave)]
        vs = [[load((i0 + t) * piece + k) for k in range(piece)] if own[t] else [0] * piece for t in range(wave)]
        stats["idle_lanes"] += own.count(False)
        for t in range(wave):  # the exchange: all lanes present, lane t reads lanes t - 1 and t + 1 of this wave only
            below = vs[t - 1][piece - 2:] if t > 0 else vs[t][piece - 2:]      # (__shfl_up hands lane 0 its own value)
            above = vs[t + 1][:2] if t < wave - 1 else vs[t][:2]               # (__shfl_down: lane 63 its own)
            if not own[t] or not any(x & 0x80 for x in vs[t]):
                h = [0, 0, 0, 0]
            else:
                edge = False
                if t == 0:
                    below, edge = front(i0 + t, vs[t]), True
                if t == wave - 1 or i0 + t + 1 >= pieces:
                    above, edge = back(i0 + t, vs[t]), True
                stats["from_lanes"] += not edge
                h = list(below) + list(above)
            if own[t]:
                store(i0 + t, apply(vs[t], h))

    if halo == "mem":
        for lane in range(min(stride, pieces)):
            for i in range(lane, pieces, stride):
                v = [load(i * piece + k) for k in range(piece)]
                h = front(i, v) + back(i, v) if any(x & 0x80 for x in v) else [0, 0, 0, 0]
                store(i, apply(v, h))
    else:
        for w0 in range(0, stride, wave):  # a wave: lanes w0 .. w0 + wave - 1 of the grid
            i0 = w0
            while i0 + wave - 1 + 3 * stride < pieces:
                for s in range(4):
                    wave_step(i0 + s * stride)
                stats["unrolled"] += 1
                i0 += 4 * stride
            while i0 < pieces:
                wave_step(i0)
                stats["remainder"] += 1
                i0 += stride
    for t in range(piece):  # the tail: block 0, lanes 0 .. piece - 1
        j = pieces * piece + t
        if j < n:
            assert dst[j] is None
            dst[j] = foldk_byte(load(j - 2) if j > 1 else 0, load(j - 1) if j > 0 else 0, load(j), load(j + 1) if j + 1 < n else 0,
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
