"""The feed select contract (aha_feed_select_batch*) straight from its definition, on selectsim.select_doc: a sequence T grows
piece by piece from n0 to n1 bytes; with W = max(Lmax - 1, 0) and F(n) = max(0, n - W) a call reports the hits of
select_doc(hits of T[0..n1)) whose start lies in [F(n0), F(n1)) -- [F(n0), n1) under FINAL, after which T is empty again --
relative to the piece's first byte.  piece_hold = n1 - max(end of the last hit reported so far, F(n1)), 0 after FINAL.  Plain
Python, slow and obvious on purpose; `match` is the CPU oracle's (bytes -> (start, end, value) triples, byte offsets)."""
import numpy as np

import selectsim


def window(keys):
    """W of a key set (bytes)"""
    return max(max((len(k) for k in keys), default=0) - 1, 0)


def frontier(n, W):
    return max(0, n - W)


def oracle_match(o):
    """a `match` over a pyoracle.AC"""
    return lambda t: [(int(s), int(e), int(v)) for s, e, v in o.match(bytes(t), chars=False).tolist()]


class Sequence:
    """one sequence of a feed"""

    def __init__(self, match, W):
        self.match, self.W = match, W
        self.text, self.last_end = b"", 0

    def push(self, piece, final=False):
        """-> (hits relative to the piece [(start, end, value)], piece_hold, piece_base)"""
        n0 = len(self.text)
        self.text += bytes(piece)
        n1 = len(self.text)
        lo, hi = frontier(n0, self.W), (n1 if final else frontier(n1, self.W))
        rep = [h for h in selectsim.select_doc(self.match(self.text)) if lo <= h[0] < hi]
        if rep:
            self.last_end = rep[-1][1]
        hold = n1 - max(self.last_end, frontier(n1, self.W))
        if final:
            self.text, self.last_end, hold = b"", 0, 0
        return [(s - n0, e - n0, v) for s, e, v in rep], hold, n0


def stream(match, W, pieces):
    """the pieces of ONE sequence in order, the last call with FINAL -> the reported hits with absolute offsets, concatenated"""
    q, out = Sequence(match, W), []
    for i, p in enumerate(pieces):
        hits, _, base = q.push(p, final=i == len(pieces) - 1)
        out += [(s + base, e + base, v) for s, e, v in hits]
    return out


def as_array(hits):
    out = np.zeros(len(hits), dtype=selectsim.HIT_DTYPE)
    for i, h in enumerate(hits):
        out[i] = h
    return out


class Feed:
    """n_seqs sequences: what one call on (pieces, seq_ids) gives -- the C entry's outputs"""

    def __init__(self, match, W, n_seqs):
        self.seqs = [Sequence(match, W) for _ in range(n_seqs)]

    def call(self, pieces, seq_ids, final=False):
        """-> (hits HIT_DTYPE, piece_sel_offsets uint64[D+1], piece_bases uint64[D], piece_hold uint32[D])"""
        hits, pso, bases, hold = [], [0], [], []
        for p, q in zip(pieces, seq_ids):
            h, ho, b = self.seqs[q].push(p, final)
            hits += h
            pso.append(len(hits))
            bases.append(b)
            hold.append(ho)
        return as_array(hits), np.array(pso, dtype=np.uint64), np.array(bases, dtype=np.uint64), np.array(hold, dtype=np.uint32)
