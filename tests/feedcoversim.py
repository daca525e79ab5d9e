"""CPU twin of a feed cover call (aha_feed_cover_batch*), two ways, both with the oracle.

The contract (piece_truth): H_d = the whole sequence's hits (byte offsets) whose end lies inside piece d, relative to the piece;
bit j = byte j of the piece lies in [max(start, 0), end) of one of them; back = max(0, max -start).

The pipeline (FeedCoverSim; DESIGN.md 4.10 "Feed cover"): with W = max(Lmax - 1, 0), ctx = the sequence's last min(W, consumed)
bytes and W' = min(W, |P|),
    mask(P) = (cover(P matched alone) with bits [0, W') cleared) OR the spans of {h in hits(X2): end > |ctx|}, clipped to P
    back(P) = max(0, |ctx| - the least start among those window hits)
    hits(P) = |hits(X2)| - |hits(ctx)| + |hits(P)| - |hits(P'2)|
with X2 = ctx || P[:2 W] and P'2 = P[:2 W].  tests/test_feed_cover_host.py holds the two against each other."""
import numpy as np

from pyoracle import HIT_DTYPE


def _m(o, b):
    return o.match(bytes(b)) if b else np.zeros(0, dtype=HIT_DTYPE)


def spans_cover(start, end, n):
    """bool[n]: byte j lies in [max(start, 0), min(end, n)) of a span"""
    diff = np.zeros(n + 1, dtype=np.int64)
    s = np.clip(np.asarray(start, dtype=np.int64), 0, n)
    e = np.clip(np.asarray(end, dtype=np.int64), 0, n)
    keep = e > s
    np.add.at(diff, s[keep], 1)
    np.add.at(diff, e[keep], -1)
    return np.cumsum(diff)[:n] > 0


def piece_truth(whole_hits, base, length):
    """the contract, from the whole sequence's hits (byte offsets): -> (cover bool[length], back, n_hits)"""
    h = whole_hits[(whole_hits["end"] > base) & (whole_hits["end"] <= base + length)]
    start = h["start"].astype(np.int64) - base
    end = h["end"].astype(np.int64) - base
    back = int(max(0, (-start).max())) if len(h) else 0
    return spans_cover(start, end, length), back, len(h)


class FeedCoverSim:
    def __init__(self, oracle, n_seqs):
        self.o = oracle
        self.W = max(oracle.max_key_len - 1, 0)
        self.ctx = [b""] * n_seqs
        self.pos = [0] * n_seqs

    def piece(self, seq, P):
        """-> (cover bool[len(P)], back, n_hits, base) by the pipeline, and the sequence moves on by P"""
        P = bytes(P)
        ctx, W = self.ctx[seq], self.W
        lc, L = len(ctx), len(P)
        head2 = P[:2 * W]
        main = _m(self.o, P)
        cov = spans_cover(main["start"], main["end"], L)
        cov[:min(W, L)] = False
        x2 = _m(self.o, ctx + head2)
        kept = x2[x2["end"] > lc]
        cov |= spans_cover(kept["start"].astype(np.int64) - lc, kept["end"].astype(np.int64) - lc, L)
        back = int(max(0, lc - int(kept["start"].min()))) if len(kept) else 0
        n_hits = len(x2) - len(_m(self.o, ctx)) + len(main) - len(_m(self.o, head2))
        base = self.pos[seq]
        self.pos[seq] += L
        self.ctx[seq] = (ctx + P)[lc + L - min(W, lc + L):]
        return cov, back, n_hits, base


def reassemble(redacted_pieces, backs, fill):
    """the stream law: each piece's redacted bytes behind the previous one, then the last `back` bytes already written
    overwritten with fill"""
    out = bytearray()
    for red, back in zip(redacted_pieces, backs):
        assert 0 <= back <= len(out)
        out[len(out) - back:] = bytes([fill]) * back
        out += bytes(red)
    return bytes(out)
