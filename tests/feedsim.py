"""CPU twin of a feed (aha_feed_*): the two facts of DESIGN.md 4.10 applied with the oracle, piece by piece.  With
W = max(Lmax - 1, 0) and ctx = the last min(W, consumed) bytes of the sequence, the hits of piece P are
  boundary  the hits of ctx || P[:W] matched alone without the first len(match(ctx)), shifted by |ctx| (leads(ctx) in chars);
  main      the hits of P matched alone without the first len(match(P[:W])).
Both selections are by count, never by comparing offsets."""
import numpy as np

from pyoracle import HIT_DTYPE


def leads(b):
    a = np.frombuffer(bytes(b), dtype=np.uint8)
    return int(np.count_nonzero((a & 0xC0) != 0x80))


class FeedSim:
    def __init__(self, oracle, n_seqs, chars=False):
        self.o, self.chars = oracle, chars
        self.W = max(oracle.max_key_len - 1, 0)
        self.ctx = [b""] * n_seqs
        self.pos = [(0, 0)] * n_seqs

    def _m(self, b):
        return self.o.match(bytes(b), chars=self.chars) if b else np.zeros(0, dtype=HIT_DTYPE)

    def piece(self, seq, P):
        """-> (hits relative to the piece, base) and the sequence moves on by P"""
        P = bytes(P)
        ctx, W = self.ctx[seq], self.W
        head = P[:W]
        bnd = self._m(ctx + head)[len(self._m(ctx)):].copy()
        sh = leads(ctx) if self.chars else len(ctx)
        bnd["start"] -= sh
        bnd["end"] -= sh
        main = self._m(P)[len(self._m(head)):]
        nb, nc = self.pos[seq]
        base = nc if self.chars else nb
        self.pos[seq] = (nb + len(P), nc + (leads(P) if self.chars else 0))
        self.ctx[seq] = (ctx + P)[len(ctx) + len(P) - min(W, len(ctx) + len(P)):]
        return np.concatenate([bnd, main]), base

    def reset(self, seq):
        self.ctx[seq] = b""
        self.pos[seq] = (0, 0)


def absolute(hits, base):
    out = hits.copy()
    out["start"] += base
    out["end"] += base
    return out
