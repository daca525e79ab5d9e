"""The records and grep contracts (aha_ac_records_batch*, aha_ac_grep_batch*) in plain Python, and a numpy model of the device
arithmetic (scan_grep.hip).  Slow and obvious on purpose; the tests give it the CPU oracle's hits per document.
It does not import the library."""
import numpy as np


def _delim(delim):
    return delim[0] if isinstance(delim, (bytes, bytearray)) else int(delim)


# ---- the contracts, stated plainly ---------------------------------------------------------------------------------------
def records(corpus, offs, delim):
    """-> (rec_offsets uint64[R+1], doc_rec_offsets uint64[D+1]): E = the documents' ends and the positions behind a
    delimiter, without 0; rec_offsets = 0 and E ascending without repeats; doc_rec_offsets[d] = the elements of E that are
    <= offs[d]"""
    text = bytes(np.asarray(corpus, dtype=np.uint8).tobytes())
    off = [int(x) for x in offs]
    dl = _delim(delim)
    E = {q for q in off[1:]} | {p + 1 for p in range(len(text)) if text[p] == dl}
    E.discard(0)
    E = sorted(E)
    dro = [sum(1 for e in E if e <= q) for q in off]
    return np.array([0] + E, dtype=np.uint64), np.array(dro, dtype=np.uint64)


def grep(hits_per_doc, offs, corpus, invert):
    """-> (kept_docs uint64[n_kept], out uint8, doc_out_offsets uint64[n_kept+1]): document d is kept when
    (hits_per_doc[d] >= 1) != invert; out = the kept documents' bytes one behind the other"""
    text = bytes(np.asarray(corpus, dtype=np.uint8).tobytes())
    off = [int(x) for x in offs]
    kept, parts, doo = [], [], [0]
    for d in range(len(off) - 1):
        if (int(hits_per_doc[d]) >= 1) != bool(invert):
            kept.append(d)
            parts.append(text[off[d]:off[d + 1]])
            doo.append(doo[-1] + len(parts[-1]))
    return (np.array(kept, dtype=np.uint64), np.frombuffer(b"".join(parts), dtype=np.uint8).copy(),
            np.array(doo, dtype=np.uint64))


# ---- the device arithmetic ------------------------------------------------------------------------------------------------
def eq4(w, b4):
    """kgr_ends' byte compare on one 32-bit word: bit k = (byte k of w == the byte b4 repeats)"""
    m = 0xFFFFFFFF
    x = (w ^ b4) & m
    z = ~((((x & 0x7F7F7F7F) + 0x7F7F7F7F) & m) | x) & 0x80808080
    return ((((z >> 7) * 0x00204081) & m) >> 21) & 0xF


def ends_words(corpus, delim, head):
    """kgr_ends: the mask words of a text whose first 16-byte aligned address lies `head` bytes in (head < 16, at most the
    text): the aligned words (32 text bytes behind the head each, bytes behind the text give no bit), and every mask word as
    the funnel of two neighbours -- the last `head` bits of the one in front, the first 32 - head bits of its own"""
    text = np.asarray(corpus, dtype=np.uint8)
    dl = _delim(delim)
    n = text.size
    head = min(head, n)
    n_words = (n + 31) // 32
    b4 = dl * 0x01010101
    body = np.zeros(n_words * 32, dtype=np.uint8)
    body[: n - head] = text[head:]
    valid = np.zeros(n_words * 32, dtype=bool)
    valid[: n - head] = True
    aligned = []
    for j in range(n_words):
        w = 0
        for k in range(8):  # eight dwords of two 16-byte pieces
            lo = j * 32 + k * 4
            dword = int.from_bytes(body[lo:lo + 4].tobytes(), "little")
            bits = eq4(dword, b4)
            for i in range(4):
                if not valid[lo + i]:
                    bits &= ~(1 << i)
            w |= bits << (4 * k)
        aligned.append(w)
    front = 0  # the head bytes as the top bits of the word in front of the first
    for k in range(head):
        if text[k] == dl:
            front |= 1 << (32 - head + k)
    out = []
    for j in range(n_words):
        prev = aligned[j - 1] if j else front
        out.append((((aligned[j] << 32) | prev) >> (32 - head)) & 0xFFFFFFFF)
    return np.array(out, dtype=np.uint32)


def _bits_of(words, n):
    return np.unpackbits(np.asarray(words, dtype="<u4").view(np.uint8), bitorder="little")[:n].astype(bool)


def model_records(corpus, offs, delim, head=0):
    """records by the device path: the end mask (ends_words) with the documents' ends OR-ed in, its exclusive rank, an end per
    set bit, the documents' offsets as the rank of their first byte"""
    text = np.asarray(corpus, dtype=np.uint8)
    off = np.asarray(offs).astype(np.int64)
    n = text.size
    mask = _bits_of(ends_words(text, delim, head), n)
    q = off[1:]
    mask[q[q > 0] - 1] = True
    rank = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(mask, out=rank[1:])
    rec = np.zeros(int(rank[n]) + 1, dtype=np.uint64)
    p = np.nonzero(mask)[0]
    rec[rank[p] + 1] = p + 1
    return rec, rank[off].astype(np.uint64)


def model_grep(hits_per_doc, offs, corpus, invert):
    """grep by the device path: keep, S and T, their ranks, A, delta, shift, the kept documents' offsets and the copy by
    last-segment lookup.  -> (kept_docs, out, doc_out_offsets, n_runs)"""
    text = np.asarray(corpus, dtype=np.uint8)
    off = np.asarray(offs).astype(np.int64)
    D = off.size - 1
    h = np.asarray(hits_per_doc).astype(np.int64)[:D]
    keep = (h >= 1) != bool(invert)
    drop = ~keep
    prev_keep = np.concatenate([[True], keep[:-1]]) if D else keep
    next_keep = np.concatenate([keep[1:], [True]]) if D else keep
    S, T = drop & prev_keep, drop & next_keep
    a, b = np.nonzero(S)[0], np.nonzero(T)[0]
    assert a.size == b.size and (a <= b).all() and a.size <= min(int(drop.sum()), int(keep.sum()) + 1)
    n = a.size
    A = off[a]
    delta = -(off[b + 1] - A)
    shift = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(delta, out=shift[1:])
    total = int(off[D] + shift[n])
    rank_s = np.zeros(D + 1, dtype=np.int64)
    np.cumsum(S, out=rank_s[1:])
    kept = np.nonzero(keep)[0]
    doo = np.concatenate([off[kept] + shift[rank_s[kept]], [total]])
    O = A + shift[:n]
    q = np.arange(total, dtype=np.int64)
    j = np.searchsorted(O, q, side="right") - 1  # the LAST j with O[j] <= q (adjacent runs tie); -1: in front of the first
    out = text[q - shift[j + 1]] if total else np.zeros(0, dtype=np.uint8)
    return kept.astype(np.uint64), out, doo.astype(np.uint64), n


def kernel_model(corpus, offs, delim, hits_of, invert, head=0):
    """records, then grep over the records, both by the device arithmetic.  hits_of(rec_offsets) -> hits per record.
    -> (rec_offsets, doc_rec_offsets, kept_docs, out, doc_out_offsets, n_runs)"""
    rec, dro = model_records(corpus, offs, delim, head)
    kept, out, doo, n_runs = model_grep(hits_of(rec), rec, corpus, invert)
    return rec, dro, kept, out, doo, n_runs
