"""The feed token contract (aha_feed_select_batch* with AHA_FEED_SELECT_TOKENS) straight from its definition, on
selectsim.select_doc and tokensim.tokens_doc.  A sequence T grows piece by piece from n0 to n1 bytes; beside the select cursor c
of feed select it keeps a token cursor t <= c.  A call finds (c0, t0); c1 = max(c0, end of the last hit the call settles, F(n1)),
n1 under FINAL; S1 = the hits of select_doc(hits of T[0..n1)) with a start in [t0, F(n1)) ([t0, n1) under FINAL); Tok1 =
tokens_doc(T[t0..c1), S1 shifted by -t0), shifted back.  c1 is a certain boundary iff FINAL, or gap_runs, or the last hit of S1
ends there, or c1 < n1 and T[c1] is no continuation byte.  Certain: all of Tok1 is reported and t1 = c1; else Tok1 without its
last token, whose start is t1.  piece_hold = n1 - t1.  Plain Python, slow and obvious on purpose; `match` is the CPU oracle's."""
import numpy as np

import selectsim
import tokensim
from feedselectsim import as_array, frontier, oracle_match, window  # noqa: F401  (the tests take them from here)


class Sequence:
    """one sequence of a feed"""

    def __init__(self, match, W):
        self.match, self.W = match, W
        self.text, self.c, self.t = b"", 0, 0

    def push(self, piece, final=False, gap_runs=False):
        """-> (tokens relative to the piece [(start, end, value)], piece_hold, piece_base)"""
        n0 = len(self.text)
        self.text += bytes(piece)
        T, n1, W = self.text, len(self.text), self.W
        c0, t0 = self.c, self.t
        hi = n1 if final else frontier(n1, W)
        sel = selectsim.select_doc(self.match(T))
        settled = [h for h in sel if c0 <= h[0] < hi]  # (feed select: starts in front of c0 were settled before)
        c1 = n1 if final else max([c0, frontier(n1, W)] + [h[1] for h in settled[-1:]])
        S1 = [h for h in sel if t0 <= h[0] < hi]
        assert all(t0 <= s and e <= c1 for s, e, _ in S1) and S1 == settled  # ([t0, c0) is an open gap token: no hit starts in it)
        tok1 = [(s + t0, e + t0, v) for s, e, v in tokensim.tokens_doc(T[t0:c1], [(s - t0, e - t0, v) for s, e, v in S1], gap_runs)]
        certain = final or gap_runs or (bool(S1) and S1[-1][1] == c1) or (c1 < n1 and (T[c1] & 0xC0) != 0x80)
        if not tok1:
            rep, t1 = [], t0
        elif certain:
            rep, t1 = tok1, c1
        else:
            assert tok1[-1][2] == -1 and tok1[-1][1] == c1
            rep, t1 = tok1[:-1], tok1[-1][0]
        assert (not rep and t1 == t0) or (rep[0][0] == t0 and rep[-1][1] == t1 and all(a[1] == b[0] for a, b in zip(rep, rep[1:])))
        self.c, self.t = c1, t1
        hold = n1 - t1
        if final:
            self.text, self.c, self.t, hold = b"", 0, 0, 0
        return [(s - n0, e - n0, v) for s, e, v in rep], hold, n0


def join_gaps(toks):
    """-1 tokens that touch, joined (the GAP_RUNS law)"""
    out = []
    for s, e, v in toks:
        if out and v == -1 and out[-1][2] == -1 and out[-1][1] == s:
            out[-1] = (out[-1][0], e, -1)
        else:
            out.append((s, e, v))
    return out


def stream(match, W, pieces, gap_runs=False, holds=None):
    """the pieces of ONE sequence in order, the last call with FINAL -> the reported tokens with absolute offsets, concatenated
    (not joined); holds: a list that receives every call's piece_hold"""
    q, out = Sequence(match, W), []
    for i, p in enumerate(pieces):
        toks, hold, base = q.push(p, final=i == len(pieces) - 1, gap_runs=gap_runs)
        out += [(s + base, e + base, v) for s, e, v in toks]
        if holds is not None:
            holds.append(hold)
    return out


class Feed:
    """n_seqs sequences: what one call on (pieces, seq_ids) gives -- the C entry's outputs"""

    def __init__(self, match, W, n_seqs):
        self.seqs = [Sequence(match, W) for _ in range(n_seqs)]

    def call(self, pieces, seq_ids, final=False, gap_runs=False):
        """-> (tokens HIT_DTYPE, piece_tok_offsets uint64[D+1], piece_bases uint64[D], piece_hold uint32[D])"""
        toks, pto, bases, hold = [], [0], [], []
        for p, q in zip(pieces, seq_ids):
            t, ho, b = self.seqs[q].push(p, final, gap_runs)
            toks += t
            pto.append(len(toks))
            bases.append(b)
            hold.append(ho)
        return as_array(toks), np.array(pto, dtype=np.uint64), np.array(bases, dtype=np.uint64), np.array(hold, dtype=np.uint32)
