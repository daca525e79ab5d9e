"""The twin of the excerpts calls (aha_ac_grep_batch* with AHA_GREP_CONTEXT).  It does not import the library.

excerpts(...)        the contract stated plainly, by hits, with a bit per byte: slow and obvious.
model_excerpts(...)  a numpy model of the device arithmetic (scan_excerpt.hip): the cover mask, the covered runs of each
                     document (S and T), their windows, the merge flags, the gaps as deleted hits, the shift and the copy by
                     last-segment lookup, as grepsim.model_grep does for grep.

hits_per_doc: one (n, 2) array-like of (start, end) byte offsets per document, relative to the document."""
import numpy as np

MAX_CONTEXT = 0x7FFFFFFF


def is_cont(c):
    return (int(c) & 0xC0) == 0x80


def snap_left(text, a, x):
    for _ in range(3):
        if x > a and is_cont(text[x]):
            x -= 1
    return x


def snap_right(text, b, x):
    for _ in range(3):
        if x < b and is_cont(text[x]):
            x += 1
    return x


def window(text, a, b, s, e, before, after):
    """the window of the stretch [s, e) (corpus positions) of the document [a, b)"""
    return snap_left(text, a, max(a, s - before)), snap_right(text, b, min(b, e + after))


def excerpts(hits_per_doc, offs, corpus, before, after):
    """-> (starts uint64[R], out uint8[n_out_bytes], out_offsets uint64[R + 1])"""
    text = np.asarray(corpus, dtype=np.uint8)
    off = [int(x) for x in offs]
    starts, pieces = [], []
    for d in range(len(off) - 1):
        a, b = off[d], off[d + 1]
        inside = np.zeros(b - a + 2, dtype=np.int8)  # a bit per byte of the document, a clear one on either side
        for s, e in np.asarray(hits_per_doc[d], dtype=np.int64).reshape(-1, 2):
            w0, w1 = window(text, a, b, a + int(s), a + int(e), before, after)
            inside[w0 - a + 1:w1 - a + 1] = 1
        step = np.diff(inside)
        for p, q in zip(np.nonzero(step == 1)[0], np.nonzero(step == -1)[0]):  # the maximal runs [p, q) of set bits
            starts.append(a + int(p))
            pieces.append(text[a + int(p):a + int(q)])
    oo = np.cumsum([0] + [x.size for x in pieces]).astype(np.uint64)
    out = np.concatenate(pieces) if pieces else np.zeros(0, dtype=np.uint8)
    return np.array(starts, dtype=np.uint64), out, oo


def cover_bits(hits_per_doc, offs):
    """the byte-level cover mask of the batch as a bool array"""
    off = [int(x) for x in offs]
    M = np.zeros(off[-1] if off else 0, dtype=bool)
    for d in range(len(off) - 1):
        for s, e in np.asarray(hits_per_doc[d], dtype=np.int64).reshape(-1, 2):
            M[off[d] + int(s):off[d] + int(e)] = True
    return M


def model_excerpts(M, offs, corpus, before, after):
    """the excerpts by the device path, from the cover mask alone -> (starts, out, out_offsets, n_runs)"""
    text = np.asarray(corpus, dtype=np.uint8)
    off = np.asarray(offs).astype(np.int64)
    D, n = off.size - 1, int(off[-1]) if off.size else 0
    M = np.asarray(M, dtype=bool)
    empty = (np.zeros(0, dtype=np.uint64), np.zeros(0, dtype=np.uint8), np.zeros(1, dtype=np.uint64), 0)
    if n == 0 or not M.any():
        return empty
    # kex_edges: from the mask alone; kex_doc_edges: the inner boundaries with covered bytes on both sides
    prev = np.concatenate([[False], M[:-1]])
    nxt = np.concatenate([M[1:], [False]])
    S, T = M & ~prev, M & ~nxt
    for q in off[1:D]:
        q = int(q)
        if 0 < q < n and M[q - 1] and M[q]:
            S[q] = True
            T[q - 1] = True
    s, t = np.nonzero(S)[0], np.nonzero(T)[0]
    assert s.size == t.size and (s <= t).all()
    n_runs = s.size
    # kex_windows: owner_of = the last d with off[d] <= p
    doc = np.searchsorted(off[:D], s, side="right") - 1
    assert (doc == np.searchsorted(off[:D], t, side="right") - 1).all()
    w0 = np.array([snap_left(text, int(off[d]), max(int(off[d]), int(p) - before)) for p, d in zip(s, doc)], dtype=np.int64)
    w1 = np.array([snap_right(text, int(off[d + 1]), min(int(off[d + 1]), int(p) + 1 + after)) for p, d in zip(t, doc)],
                  dtype=np.int64)
    # kex_merge
    j = np.arange(n_runs)
    first = (j == 0) | (doc != np.roll(doc, 1)) | (w0 > np.roll(w1, 1))
    last = (j == n_runs - 1) | (np.roll(doc, -1) != doc) | (np.roll(w0, -1) > w1)
    p_r, q_r = w0[first], w1[last]
    R = p_r.size
    assert q_r.size == R and (p_r < q_r).all()
    # kex_gaps, kex_delta, the scan
    A = np.concatenate([[0], q_r])
    end = np.concatenate([p_r, [n]])
    delta = A - end
    shift = np.zeros(R + 2, dtype=np.int64)
    np.cumsum(delta, out=shift[1:])
    total = int(n + shift[R + 1])
    # kex_emit
    o = A + shift[:R + 1]
    starts = (o[:R] - shift[1:R + 1]).astype(np.uint64)
    assert np.array_equal(starts, p_r.astype(np.uint64)) and int(o[R]) == total
    # the copy: the LAST j with O[j] <= q, text at the distance shift[j + 1]
    q = np.arange(total, dtype=np.int64)
    seg = np.searchsorted(o, q, side="right") - 1
    out = text[q - shift[seg + 1]] if total else np.zeros(0, dtype=np.uint8)
    return starts, out, o.astype(np.uint64), n_runs
