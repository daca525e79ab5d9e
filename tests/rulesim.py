"""Rule grep (aha_ac_grep_batch* with AHA_GREP_RULE, include/aha_hip.h) in plain numpy.

passes is the contract: per document whether the rule holds over its class counts (classsim.class_counts) and its length, with
Python integers for the products.  grep composes it with grepsim's grep statement.  kernel_model is scan_greprule.hip's
kgq_edges, word by word: S and T from the keep mask alone.
"""
import numpy as np

import classsim
import grepsim

GE, LT = 0, 1


def term_holds(count, length, op, num, den):
    lhs, rhs = (int(count) * int(den), int(num) * int(length)) if den else (int(count), int(num))
    return lhs < rhs if op == LT else lhs >= rhs


def passes(rows, doc_offsets, terms):
    """rows: (D, C) class counts; terms: (class_id, op, group, num, den_bytes) each -> bool[D]: some group has all its terms
    true (OR over groups, AND inside one; group ids are arbitrary, the terms in any order)"""
    off = [int(x) for x in doc_offsets]
    rows = np.asarray(rows)
    groups = {}
    for c, op, g, num, den in terms:
        groups.setdefault(int(g), []).append((int(c), int(op), int(num), int(den)))
    out = np.zeros(len(off) - 1, dtype=bool)
    for d in range(len(off) - 1):
        length = off[d + 1] - off[d]
        out[d] = any(all(term_holds(rows[d, c], length, op, num, den) for c, op, num, den in ts) for ts in groups.values())
    return out


def grep(hits_per_doc, class_ids, offsets, C, doc_offsets, corpus, terms, invert):
    """hits_per_doc as classsim.class_counts takes them -> (kept_docs, out, doc_out_offsets, rows, passes)"""
    rows = classsim.class_counts(hits_per_doc, class_ids, offsets, C)
    ok = passes(rows, doc_offsets, terms)
    kept, out, doo = grepsim.grep(ok.astype(np.int64), doc_offsets, corpus, invert)
    return kept, out, doo, rows, ok


def pack_bits(bits):
    """bool[D] -> the mask words, the bits from D on 0"""
    bits = np.asarray(bits, dtype=bool)
    padded = np.zeros(((bits.size + 31) // 32) * 32, dtype=np.uint8)
    padded[:bits.size] = bits
    return np.packbits(padded, bitorder="little").view("<u4").copy()


def kernel_model(keep_words, D):
    """kgq_edges: a lane per mask word -> (S words, T words).  dropped = ~keep inside D; S = dropped and not (dropped << 1 | the
    top bit of the word in front); T = dropped and not (dropped >> 1 | the low bit of the next word << 31)"""
    M = 0xFFFFFFFF
    keep = [int(w) for w in keep_words]
    n_words = (D + 31) // 32
    assert len(keep) == n_words
    tail = D & 31
    S, T = [], []
    for w in range(n_words):
        valid = (1 << tail) - 1 if (w + 1 == n_words and tail) else M
        dropped = ~keep[w] & valid & M
        before = ((~keep[w - 1] & M) >> 31) if w else 0
        behind = (~keep[w + 1] & 1) if w + 1 < n_words else 0
        S.append(dropped & ~((dropped << 1) | before) & M)
        T.append(dropped & ~((dropped >> 1) | (behind << 31)) & M)
    return np.array(S, dtype=np.uint32), np.array(T, dtype=np.uint32)


def edges(keep_bits):
    """the direct definition: S[d] = d is dropped and d - 1 is kept or there is none; T[d] = d is dropped and d + 1 is kept or
    there is none -> (S words, T words)"""
    keep = np.asarray(keep_bits, dtype=bool)
    D = keep.size
    S = np.array([not keep[d] and (d == 0 or keep[d - 1]) for d in range(D)], dtype=bool)
    T = np.array([not keep[d] and (d + 1 == D or keep[d + 1]) for d in range(D)], dtype=bool)
    return pack_bits(S), pack_bits(T)
