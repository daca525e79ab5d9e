"""The feed grep contract (aha_feed_grep_batch*) in plain Python.  Three things, none of which imports the library:
  whole()      the whole-sequence definition: grepsim.records of the sequence as one document, grepsim.grep over those records
               with the hits of every record AS ITS OWN DOCUMENT;
  Sequence / Feed   the call-by-call model: what one call reports and the state it leaves, with the X / Y / Z arithmetic of
               DESIGN.md 4.10 "Feed grep" -- it never looks at more of a sequence than its last W bytes, the open record's
               length and whether that record has a hit already;
  Holder       the caller's holding rule: the lines a caller emits from a call's outputs and the bytes it keeps.
`count` is text -> the number of hits of the text matched as its own document (the CPU oracle's).  Slow and obvious on
purpose."""
import numpy as np

import grepsim


def window(keys):
    """W of a key set (bytes)"""
    return max(max((len(k) for k in keys), default=0) - 1, 0)


def oracle_count(o, fold=False):
    """a `count` over a pyoracle.AC (fold: the oracle holds the lowered keys, the text is lowered before the match)"""
    return lambda t: len(o.match(bytes(t).lower() if fold else bytes(t), chars=False))


def _delim(delim):
    return delim[0] if isinstance(delim, (bytes, bytearray)) else int(delim)


def fragments(piece, delim):
    """a piece split as aha_ac_records_batch splits a document: behind every delimiter and at its end; none of an empty one"""
    dl, out, a = _delim(delim), [], 0
    for i, b in enumerate(piece):
        if b == dl:
            out.append(piece[a:i + 1])
            a = i + 1
    if a < len(piece):
        out.append(piece[a:])
    return out


# ---- the whole-sequence definition ------------------------------------------------------------------------------------------
def whole(count, text, delim=b"\n", invert=False):
    """-> the kept records of the sequence `text`, in order (their concatenation is aha_ac_grep_batch's out)"""
    corpus = np.frombuffer(bytes(text), dtype=np.uint8)
    rec, _ = grepsim.records(corpus, [0, len(text)], delim)
    h = [count(bytes(text[int(rec[r]):int(rec[r + 1])])) for r in range(rec.size - 1)]
    kept, out, doo = grepsim.grep(h, rec, corpus, invert)
    raw = out.tobytes()
    lines = [raw[int(doo[i]):int(doo[i + 1])] for i in range(kept.size)]
    assert lines == [bytes(text[int(rec[r]):int(rec[r + 1])]) for r in kept.tolist()]
    return lines


# ---- the call-by-call model ------------------------------------------------------------------------------------------------
class Sequence:
    """one sequence of a feed: FeedSeq's context and FeedGrepSeq (seen, open_len, recs, open_hit)"""

    def __init__(self, count, W):
        self.count, self.W = count, W
        self.ctx, self.seen, self.open_len, self.recs, self.open_hit = b"", 0, 0, 0, False

    def push(self, piece, delim=b"\n", invert=False, final=False):
        """-> (frags [bytes], keep [bool per fragment], hold, head, base, rec_base)"""
        piece = bytes(piece)
        dl, W, count = _delim(delim), self.W, self.count
        frags = fragments(piece, dl)
        base, rec_base = self.seen, self.recs
        closed = [final or f[-1] == dl for f in frags]
        has = [count(f) > 0 for f in frags]
        if self.open_len and piece:  # the first fragment continues the open record: the two facts, the record as the sequence
            c = min(W, self.open_len)
            g = min(W, len(frags[0]))
            Y = self.ctx[len(self.ctx) - c:] if c else b""
            Z = piece[:g]
            X = Y + Z
            has[0] = self.open_hit or count(X) - count(Y) > 0 or count(frags[0]) - count(Z) > 0
        keep = [c_ and (h != bool(invert)) for c_, h in zip(closed, has)]
        tail_open = bool(frags) and not closed[-1]
        n_closed = len(frags) - (1 if tail_open else 0)
        head = 0
        if piece:
            if self.open_len and keep[0]:
                head = self.open_len
        elif final and self.open_len:  # the open record closes without a fragment
            if self.open_hit != bool(invert):
                head = self.open_len
        hold = len(frags[-1]) if tail_open else 0
        if final:
            self.ctx, self.seen, self.open_len, self.recs, self.open_hit = b"", 0, 0, 0, False
        else:
            if n_closed:
                self.open_len, self.open_hit = hold, bool(tail_open and has[-1])
                self.recs += n_closed
            else:
                self.open_len += len(piece)
                if frags:
                    self.open_hit = has[0]
            self.seen += len(piece)
            both = self.ctx + piece
            self.ctx = both[max(0, len(both) - W):] if W else b""
        return frags, keep, hold, head, base, rec_base


class Feed:
    """n_seqs sequences: what one call on (pieces, seq_ids) gives -- the C entry's outputs"""

    def __init__(self, count, W, n_seqs):
        self.seqs = [Sequence(count, W) for _ in range(n_seqs)]

    def call(self, pieces, seq_ids, delim=b"\n", invert=False, final=False):
        """-> (kept_recs uint64[n_kept], out uint8, rec_out_offsets uint64[n_kept+1], info) with info = {piece_rec_offsets,
        piece_kept_offsets uint64[D+1], piece_hold uint32[D], piece_head, piece_bases, piece_rec_bases uint64[D], n_recs}"""
        assert len(set(int(q) for q in seq_ids)) == len(seq_ids)
        kept, parts, roo, pro, pko, hold, head, bases, rbases = [], [], [0], [0], [0], [], [], [], []
        for p, q in zip(pieces, seq_ids):
            frags, keep, ho, he, b, rb = self.seqs[int(q)].push(p, delim, invert, final)
            for j, (f, k) in enumerate(zip(frags, keep)):
                if k:
                    kept.append(pro[-1] + j)
                    parts.append(f)
                    roo.append(roo[-1] + len(f))
            pro.append(pro[-1] + len(frags))
            pko.append(len(kept))
            hold.append(ho)
            head.append(he)
            bases.append(b)
            rbases.append(rb)
        u64 = lambda x: np.array(x, dtype=np.uint64)  # noqa: E731
        info = {"piece_rec_offsets": u64(pro), "piece_kept_offsets": u64(pko), "piece_hold": np.array(hold, dtype=np.uint32),
                "piece_head": u64(head), "piece_bases": u64(bases), "piece_rec_bases": u64(rbases), "n_recs": pro[-1]}
        return u64(kept), np.frombuffer(b"".join(parts), dtype=np.uint8).copy(), u64(roo), info


# ---- the caller's holding rule ---------------------------------------------------------------------------------------------
class Holder:
    """what a caller keeps of one sequence: the bytes of the record that is still open"""

    def __init__(self):
        self.held = b""

    def step(self, piece, kept_bytes, head, hold, final):
        """kept_bytes: the piece's kept fragments [bytes].  -> the lines the caller emits for this piece"""
        piece = bytes(piece)
        lines = [bytes(x) for x in kept_bytes]
        if head:
            assert head == len(self.held)
            if lines and piece:
                lines[0] = self.held + lines[0]
            else:  # an empty piece under FINAL: the open record closes without a fragment
                assert not piece and final and not lines
                lines = [self.held]
        if final:
            self.held = b""
        elif hold == len(piece):
            self.held += piece
        else:
            self.held = piece[len(piece) - hold:]
        return lines


def stream(count, W, pieces, delim=b"\n", invert=False):
    """the pieces of ONE sequence in order, the last call with FINAL -> the lines a caller emits, by the model and the rule"""
    q, h, out = Sequence(count, W), Holder(), []
    for i, p in enumerate(pieces):
        final = i == len(pieces) - 1
        frags, keep, hold, head, _, _ = q.push(p, delim, invert, final)
        out += h.step(p, [f for f, k in zip(frags, keep) if k], head, hold, final)
        assert len(h.held) == q.open_len
    return out
