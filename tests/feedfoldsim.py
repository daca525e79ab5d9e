"""CPU twin of a folded feed (AHA_FEED_FOLD on a handle compiled with fold_simple, fold_bmp or fold_kana; DESIGN.md 4.13 "Feeds on
handles folded beyond ASCII") and the rule it is held against.

The rule: with fold = the handle's fold of ONE document (a truncated character at its end passes through), a call that takes a
sequence S from n0 to n1 bytes reports exactly the hits with n0 < end <= n1 of fold(S[:n1]) matched as one document by a plain
matcher of the folded keys (rule_hits).

The twin (FeedFoldSim) is the pipeline of feed.cpp / scan_feedfold.hip step by step.  The feed keeps W = Lmax + 1 ORIGINAL bytes
of context; per piece
  P~   fold(P) alone (the staged copy), bytes 0 and 1 recomputed from ctx || P (kff_heads);
  X~   fold(ctx || P)[: |ctx| + |P'|], P' = P[:Wp] (kff_windows: the fold looks two bytes past the cut); the ctx and P' blocks
       are its two parts, copied;
  boundary = match(X~) without the first len(match(ctx~)), main = match(P~) without the first len(match(P'~)) -- by count."""
import numpy as np

import fold3sim
import foldksim
import foldsim
from feedsim import leads
from pyoracle import HIT_DTYPE

FOLDS = {2: foldsim.fold2, 3: fold3sim.fold3, 4: foldksim.foldk}
FOLD_KEYS = {2: foldsim.fold2_keys, 3: fold3sim.fold3_keys, 4: foldksim.foldk_keys}
FOLD_OPTS = {2: "fold_simple", 3: "fold_bmp", 4: "fold_kana"}


def _m(o, b, chars):
    return o.match(bytes(b), chars=chars) if b else np.zeros(0, dtype=HIT_DTYPE)


def rule_hits(o, mode, S, n0, n1, chars=False):
    """-> (the call's hits relative to the piece in the feed's unit, the same hits in bytes, the base in the feed's unit); o: the
    oracle of the folded keys"""
    T = FOLDS[mode](bytes(S[:n1]))
    hb = _m(o, T, False)
    keep = (hb["end"] > n0) & (hb["end"] <= n1)
    byte_hits = hb[keep].copy()
    byte_hits["start"] -= n0
    byte_hits["end"] -= n0
    if not chars:
        return byte_hits.copy(), byte_hits, n0
    hc = _m(o, T, True)  # (the same hits in the same order, in characters)
    base = leads(S[:n0])
    out = hc[keep].copy()
    out["start"] -= base
    out["end"] -= base
    return out, byte_hits, base


def cover_of(byte_hits, L):
    """-> (bool[L]: the piece's bytes inside one of its hits, piece_back: the most bytes one reaches in front of the piece)"""
    m = np.zeros(L, dtype=bool)
    back = 0
    for h in byte_hits:
        m[max(int(h["start"]), 0):int(h["end"])] = True
        back = max(back, -int(h["start"]))
    return m, back


class FeedFoldSim:
    def __init__(self, oracle, n_seqs, mode, chars=False, W=None, wide=False):
        """oracle: of the FOLDED keys.  W: the context kept (the design's Lmax + 1; a test passes Lmax - 1 to show why).  wide: a
        cover call's windows, 2 W bytes of the piece"""
        self.o, self.mode, self.chars, self.fold = oracle, mode, chars, FOLDS[mode]
        self.W = oracle.max_key_len + 1 if W is None else W
        self.Wp = 2 * self.W if wide else self.W
        self.ctx = [b""] * n_seqs
        self.pos = [(0, 0)] * n_seqs

    def piece(self, seq, P):
        """-> (hits relative to the piece, base) and the sequence moves on by P"""
        P = bytes(P)
        ctx, W = self.ctx[seq], self.W
        lc, lp = len(ctx), min(self.Wp, len(P))
        run = self.fold(ctx + P)  # every byte from its two neighbours on each side: what feedfold_byte computes
        Pf = bytearray(self.fold(P))
        Pf[:min(2, len(P))] = run[lc:lc + min(2, len(P))]
        assert bytes(Pf) == run[lc:]  # (behind its first two bytes the piece's fold needs nothing of the context)
        X = self.fold(ctx + P[:lp + 2])[:lc + lp]
        assert X == run[:lc + lp]
        cw, pw = X[:lc], X[lc:]
        assert pw == bytes(Pf[:lp])
        bnd = _m(self.o, X, self.chars)[len(_m(self.o, cw, self.chars)):].copy()
        sh = leads(cw) if self.chars else lc
        bnd["start"] -= sh
        bnd["end"] -= sh
        main = _m(self.o, Pf, self.chars)[len(_m(self.o, pw, self.chars)):]
        nb, nc = self.pos[seq]
        base = nc if self.chars else nb
        self.pos[seq] = (nb + len(P), nc + (leads(P) if self.chars else 0))
        self.ctx[seq] = (ctx + P)[lc + len(P) - min(W, lc + len(P)):]
        return np.concatenate([bnd, main]), base

    def reset(self, seq):
        self.ctx[seq] = b""
        self.pos[seq] = (0, 0)


def same(a, b):
    return a.shape == b.shape and a.tobytes() == b.tobytes()
