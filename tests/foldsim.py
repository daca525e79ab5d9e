"""The simple case fold of AHA_OPT_FOLD_SIMPLE (include/aha_hip.h) in plain Python: F from str.upper / str.lower, fold2 of one
buffer, a batch folded document by document, and a model of the device pass (aha_amd/csrc/scan_fold.hip) lane by lane.  Nothing
here reads the committed table (aha_amd/csrc/fold_table.hpp): the tests compare the two."""
import numpy as np

LO, HI = 0x80, 0x800  # the code points UTF-8 writes in two bytes


def one(s):
    return len(s) == 1 and LO <= ord(s) < HI


def F(c):
    """one character of U+0080 .. U+07FF -> its representative: through upper(), so that a whole case class lands on one"""
    u = c.upper() if one(c.upper()) else c
    lo = u.lower()
    return lo if one(lo) else c


_TABLE = []


def table():
    """F(cp) at index cp - 0x80"""
    if not _TABLE:
        _TABLE.extend(ord(F(chr(cp))) for cp in range(LO, HI))
    return _TABLE


_PAIR = {}
for _cp in range(LO, HI):
    _PAIR[chr(_cp).encode()] = F(chr(_cp)).encode()


def is_lead(b):
    return 0xC2 <= b <= 0xDF


def is_cont(b):
    return 0x80 <= b <= 0xBF


def fold8(b):
    return b + 32 if 0x41 <= b <= 0x5A else b


def fold2(buf):
    """bytes -> bytes of the same length: every (lead 0xC2..0xDF, continuation) pair folded by F, every other byte by fold8"""
    b = bytes(buf)
    out = bytearray(len(b))
    j = 0
    while j < len(b):
        if is_lead(b[j]) and j + 1 < len(b) and is_cont(b[j + 1]):
            out[j:j + 2] = _PAIR[b[j:j + 2]]
            j += 2
        else:
            out[j] = fold8(b[j])
            j += 1
    return bytes(out)


def fold2_docs(corpus, off):
    """the batch in which each document is folded on its own; corpus: bytes or a uint8 array, off: D + 1 offsets"""
    b = bytes(np.asarray(corpus, dtype=np.uint8).tobytes()) if not isinstance(corpus, (bytes, bytearray)) else bytes(corpus)
    off = [int(x) for x in off]
    out = bytearray(b)
    for d in range(len(off) - 1):
        out[off[d]:off[d + 1]] = fold2(b[off[d]:off[d + 1]])
    return bytes(out)


def fold2_keys(keys):
    return [fold2(k.encode() if isinstance(k, str) else k) for k in keys]


def fold2_byte(tab, prev, cur, nxt):
    """one byte of fold2 from the byte and its neighbours (0 where there is none), as both lanes of a pair compute it"""
    if is_lead(cur) and is_cont(nxt):
        return 0xC0 | (tab[(((cur & 0x1F) << 6) | (nxt & 0x3F)) - LO] >> 6)
    if is_cont(cur) and is_lead(prev):
        return 0x80 | (tab[(((prev & 0x1F) << 6) | (cur & 0x3F)) - LO] & 0x3F)
    return fold8(cur)


def kernel_model(buf, off, piece=16, wave=64, grid=1, block=256):
    """k_fold2_copy + k_fold2_fix as the lanes do them.  buf: the n source bytes (nothing outside [0, n) is ever indexed: the
    loads go through `load`, which asserts it); off: the documents' offsets (off[0] is subtracted).  Lane g = blockIdx * block +
    threadIdx owns the pieces g, g + grid * block, ..; it loads its own piece, the byte before it only when the piece opens with
    a continuation byte and the byte after it only when the piece ends with a lead byte, and writes its own bytes only.  Lanes
    0 .. piece - 1 of block 0 own the n % piece tail, byte by byte.  Then a lane per interior document boundary puts the two
    source bytes back where a lead byte met a continuation byte across it.
    -> (dst as bytes, stats: neighbour loads in all, those that cross a wave's edge, those that reach a piece a stride away)"""
    tab = table()
    src = bytes(buf)
    n = len(src)
    dst = [None] * n
    stats = {"neighbour_loads": 0, "cross_wave": 0, "cross_stride": 0}

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
                prev = neighbour(j0 - 1, i) if is_cont(v[0]) and j0 > 0 else 0
                nxt = neighbour(j0 + piece, i) if is_lead(v[piece - 1]) and j0 + piece < n else 0
                out = [fold2_byte(tab, v[k - 1] if k else prev, v[k], v[k + 1] if k + 1 < piece else nxt) for k in range(piece)]
            for k in range(piece):
                assert dst[j0 + k] is None  # every byte has one owner
                dst[j0 + k] = out[k]
    for t in range(piece):  # the tail: block 0, lanes 0 .. piece - 1
        j = pieces * piece + t
        if j < n:
            assert dst[j] is None
            dst[j] = fold2_byte(tab, load(j - 1) if j > 0 else 0, load(j), load(j + 1) if j + 1 < n else 0)
    assert all(x is not None for x in dst)
    off = [int(x) for x in off]
    for d in range(1, len(off) - 1):  # k_fold2_fix: a lane per interior boundary
        b = off[d] - off[0]
        if 0 < b < n and is_lead(load(b - 1)) and is_cont(load(b)):
            dst[b - 1], dst[b] = src[b - 1], src[b]
    return bytes(dst), stats
