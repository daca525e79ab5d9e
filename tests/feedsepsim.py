"""CPU model of a feed with a separator filter (aha_feed_open_params, aha_feed_finish_batch), written from the definition: the
oracle's match(text, sep=...) of the whole sequence so far, partitioned by the stream law.  A call that takes a sequence from
n0 to n1 > n0 bytes reports the surviving hits with absolute end in [n0, n1) -- the bytes up to n1 decide their right-hand test
--, relative to the piece's first byte; finish reports those with end == n, relative to the sequence's end, and the sequence
starts again.  fold: the handle folds ASCII case (the oracle was compiled from folded keys; the text is folded here)."""
import numpy as np

from pyoracle import HIT_DTYPE

EMPTY = np.zeros(0, dtype=HIT_DTYPE)

_PUNCT = b" \t\n.,;:!?-()[]\"'/"
SEPS = {
    "punct": (256, sorted(set(_PUNCT))),                        # space and punctuation
    "low": (0x60, sorted(set(_PUNCT) | {0x00, 0x41, 0x5A})),    # bytes >= 0x60 always pass
    "none": (256, []),                                          # all false: only the sequence's two ends pass
    "all": (256, list(range(256))),                             # all true: nothing is filtered
}


def bitarray(sep):
    """the aha_amd BitArray of a (size, set bits) pair"""
    from aha_amd import BitArray

    b = BitArray(sep[0])
    for i in sep[1]:
        b[i] = True
    return b


def relative(hits, base):
    out = hits.copy()
    out["start"] -= base
    out["end"] -= base
    return out


def absolute(hits, base):
    return relative(hits, -base)


class FeedSepSim:
    def __init__(self, oracle, n_seqs, sep, fold=False):
        self.o, self.sep, self.fold = oracle, sep, fold
        self.text = [b""] * n_seqs

    def whole(self, text):
        """the oracle's filtered hits of a whole sequence"""
        text = bytes(text)
        if self.fold:
            text = text.lower()  # (bytes.lower folds ASCII only)
        return self.o.match(text, sep=self.sep) if text else EMPTY

    def piece(self, seq, P):
        """-> (hits relative to the piece, base) and the sequence moves on by P"""
        n0 = len(self.text[seq])
        self.text[seq] += bytes(P)
        n1 = len(self.text[seq])
        if n1 == n0:
            return EMPTY, n0
        h = self.whole(self.text[seq])
        return relative(h[(h["end"] >= n0) & (h["end"] < n1)], n0), n0

    def finish(self, seq):
        """-> (hits relative to the sequence's end, its length) and the sequence starts again"""
        n = len(self.text[seq])
        h = self.whole(self.text[seq])
        self.text[seq] = b""
        return relative(h[h["end"] == n], n), n

    def reset(self, seq):
        self.text[seq] = b""
