"""The feed replace contract (aha_feed_replace_batch*) straight from its definition, on feedselectsim.Sequence and
replacesim.replace_doc: a sequence T grows piece by piece from n0 to n1 bytes; a call finds the select cursor at c0 and leaves it
at c1 = n1 - piece_hold (n1 under FINAL), and the piece's result is T[c0..c1) with the hits the select call of the same piece
settles -- all of them inside [c0, c1) -- replaced.  Plain Python, slow and obvious on purpose.  `DeviceModel` states the
arithmetic of the device path beside it with numpy: hold0, the staged lengths and their scan, the gather of the staged text from
the context and the piece, the biased offsets, then replacesim.kernel_model."""
import numpy as np

import feedselectsim as fss
import replacesim


class Sequence:
    """one sequence of a feed: select and replace calls may be mixed on it"""

    def __init__(self, match, W):
        self.q = fss.Sequence(match, W)
        self.cursor = 0  # c, absolute

    def select(self, piece, final=False):
        """a select call: -> what feedselectsim.Sequence.push gives; the cursor moves as for a replace call"""
        n1 = len(self.q.text) + len(piece)
        hits, hold, n0 = self.q.push(piece, final)
        self.cursor = 0 if final else n1 - hold
        return hits, hold, n0

    def push(self, piece, repl, final=False):
        """a replace call: -> (the piece's result bytes, piece_hold, piece_base, settled hits)"""
        text = self.q.text + bytes(piece)
        c0, n1 = self.cursor, len(text)
        hits, hold, n0 = self.q.push(piece, final)
        c1 = n1 - hold
        assert n0 - c0 <= self.q.W and c0 <= c1 <= n1
        sel = [(s + n0 - c0, e + n0 - c0, v) for s, e, v in hits]  # relative to c0
        assert all(0 <= s < e <= c1 - c0 for s, e, _ in sel), "a settled hit lies outside [c0, c1)"
        out = replacesim.replace_doc(text[c0:c1], sel, repl)
        self.cursor = 0 if final else c1
        return out, hold, n0, len(hits)


def stream(match, W, pieces, repl):
    """the pieces of ONE sequence in order through replace calls, the last with FINAL -> the results concatenated"""
    q = Sequence(match, W)
    return b"".join(q.push(p, repl, final=i == len(pieces) - 1)[0] for i, p in enumerate(pieces))


class Feed:
    """n_seqs sequences: what one call on (pieces, seq_ids) gives -- the C entry's outputs"""

    def __init__(self, match, W, n_seqs):
        self.match, self.W = match, W
        self.seqs = [Sequence(match, W) for _ in range(n_seqs)]

    def reset(self, q):
        self.seqs[q] = Sequence(self.match, self.W)

    def select(self, pieces, seq_ids, final=False):
        return [self.seqs[q].select(p, final) for p, q in zip(pieces, seq_ids)]

    def call(self, pieces, seq_ids, repl, final=False):
        """-> (out uint8, piece_out_offsets uint64[D+1], piece_bases uint64[D], piece_hold uint32[D], n_selected)"""
        parts, poo, bases, hold, n_sel = [], [0], [], [], 0
        for p, q in zip(pieces, seq_ids):
            out, ho, b, n = self.seqs[q].push(p, repl, final)
            parts.append(out)
            poo.append(poo[-1] + len(out))
            bases.append(b)
            hold.append(ho)
            n_sel += n
        return (np.frombuffer(b"".join(parts), dtype=np.uint8).copy(), np.array(poo, dtype=np.uint64),
                np.array(bases, dtype=np.uint64), np.array(hold, dtype=np.uint32), n_sel)


class DeviceModel:
    """The same outputs from what the device holds, by the device path's arithmetic.  Per sequence: its length, its select
    cursor and its context (the last min(W, length) bytes, left-aligned in a row of W).  The settled selection of a call comes
    from feedselectsim (the device takes it from the select pipeline); everything behind it is modelled here."""

    def __init__(self, match, W, n_seqs):
        self.W = W
        self.sel = [fss.Sequence(match, W) for _ in range(n_seqs)]
        self.n = [0] * n_seqs
        self.cursor = [0] * n_seqs
        self.ctx = [b""] * n_seqs

    def call(self, pieces, seq_ids, repl, final=False):
        W, D = self.W, len(pieces)
        pieces = [bytes(p) for p in pieces]
        off = np.cumsum([0] + [len(p) for p in pieces]).astype(np.int64)
        text = np.frombuffer(b"".join(pieces), dtype=np.uint8)
        rows, pso, hold0, length, hold1 = [], [0], [], [], []
        for p, q in zip(pieces, seq_ids):
            n0, c0 = self.n[q], self.cursor[q]
            hits, hold, base = self.sel[q].push(p, final)
            assert base == n0
            n1 = n0 + len(p)
            # kfs_commit's expression: max(c0, the end of the last hit settled, F(n1)); n1 under FINAL
            c1 = n1 if final else max(c0, max((e + n0 for _, e, _ in hits), default=0), fss.frontier(n1, W))
            assert n1 - c1 == hold
            rows += hits
            pso.append(len(rows))
            hold0.append(n0 - c0)
            hold1.append(n1 - c1)
            length.append(n0 - c0 + len(p) - (n1 - c1))
        hold0, length = np.array(hold0, dtype=np.int64), np.array(length, dtype=np.int64)
        ext_off = np.zeros(D + 1, dtype=np.int64)
        np.cumsum(length, out=ext_off[1:])
        bias = ext_off[:D] + hold0
        # kfr_stage, driven by the staged positions: the owner of position x, then the context row or the piece
        ext = np.zeros(int(ext_off[D]), dtype=np.uint8)
        for x in range(ext.size):
            d = int(np.searchsorted(ext_off[1:], x, side="right"))  # the last d with ext_off[d] <= x among non-empty ones
            i = x - int(ext_off[d])
            q = seq_ids[d]
            lc = min(W, self.n[q])
            row = self.ctx[q]
            assert len(row) == lc and hold0[d] <= lc
            ext[x] = row[lc - int(hold0[d]) + i] if i < hold0[d] else text[int(off[d]) + i - int(hold0[d])]
        # the rows are relative to the piece: bias stands for the document offsets where A is made (krp_delta), the true
        # offsets where the results' offsets are made (krp_doc_offsets).  The same by rebasing the rows.
        rebased = [(s + int(hold0[d]), e + int(hold0[d]), v) for d in range(D) for s, e, v in rows[pso[d]:pso[d + 1]]]
        for d in range(D):
            for j in range(pso[d], pso[d + 1]):
                assert bias[d] + rows[j][0] == ext_off[d] + rebased[j][0] >= ext_off[d]
                assert ext_off[d] + rebased[j][1] <= ext_off[d + 1]
        out, poo = replacesim.kernel_model(ext, ext_off.astype(np.uint64), rebased, np.array(pso, dtype=np.uint64), repl)
        # both commits
        for d, q in enumerate(seq_ids):
            n1 = self.n[q] + len(pieces[d])
            if final:
                self.n[q], self.cursor[q], self.ctx[q] = 0, 0, b""
            else:
                self.ctx[q] = (self.ctx[q] + pieces[d])[-min(W, n1):] if W else b""
                self.n[q], self.cursor[q] = n1, n1 - hold1[d]
        return out, poo, np.array(hold1, dtype=np.uint32), len(rows)
