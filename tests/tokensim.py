"""The token contract (aha_ac_select_batch* with AHA_SELECT_TOKENS) applied literally, byte by byte, to a selection: position
p of a document is INSIDE when a selected hit holds it; it STARTS a token iff (a) a selected hit starts there, or (b) it is not
inside and p == 0, or p - 1 is inside, or -- in character mode only -- its byte is no UTF-8 continuation byte.  A token runs to
the next start, or to the document's end; value = the key for kind (a), -1 for kind (b).  Plain Python, slow and obvious on
purpose; the tests give it selectsim.select over the CPU oracle's hits."""
import numpy as np

from selectsim import HIT_DTYPE, _triples


def tokens_doc(doc, sel, gap_runs=False):
    """the tokens of ONE document (bytes) under its selection (triples, ascending) as a list of (start, end, value)"""
    n = len(doc)
    inside = [False] * n
    key_at = {}
    for s, e, v in sel:
        key_at[s] = (e, v)
        for p in range(s, e):
            inside[p] = True
    starts = []
    for p in range(n):
        a = p in key_at
        b = (not inside[p]) and (p == 0 or inside[p - 1] or (not gap_runs and (doc[p] & 0xC0) != 0x80))
        if a or b:
            starts.append(p)
    out = []
    for i, p in enumerate(starts):
        end = starts[i + 1] if i + 1 < len(starts) else n
        if p in key_at:
            assert key_at[p][0] == end, "a selected hit ends where the next token starts"
            out.append((p, end, key_at[p][1]))
        else:
            out.append((p, end, -1))
    return out


def tokens(corpus, doc_offsets, sel, doc_sel_offsets, gap_runs=False):
    """(tokens HIT_DTYPE, doc_tok_offsets uint64[D+1]) of a batch under its selection"""
    offs = [int(x) for x in doc_offsets]
    dso = [int(x) for x in doc_sel_offsets]
    raw = bytes(np.asarray(corpus, dtype=np.uint8).tobytes())
    toks, dto = [], [0]
    for d in range(len(offs) - 1):
        toks += tokens_doc(raw[offs[d]:offs[d + 1]], _triples(sel[dso[d]:dso[d + 1]]), gap_runs)
        dto.append(len(toks))
    out = np.zeros(len(toks), dtype=HIT_DTYPE)
    for i, t in enumerate(toks):
        out[i] = t
    return out, np.array(dto, dtype=np.uint64)


def check_invariants(toks, doc_tok_offsets, corpus, doc_offsets, sel, doc_sel_offsets, gap_runs=False):
    """per document: the tokens partition it (none for an empty one); those with value >= 0 are exactly the selection; in
    character mode no token of value -1 holds a non-continuation byte other than its first (with gap_runs: no two tokens of
    value -1 touch)"""
    offs = [int(x) for x in doc_offsets]
    dso = [int(x) for x in doc_sel_offsets]
    dto = [int(x) for x in doc_tok_offsets]
    raw = bytes(np.asarray(corpus, dtype=np.uint8).tobytes())
    assert len(dto) == len(offs) and dto[0] == 0 and dto[-1] == len(toks)
    for d in range(len(offs) - 1):
        doc = raw[offs[d]:offs[d + 1]]
        T = _triples(toks[dto[d]:dto[d + 1]])
        if not doc:
            assert not T, d
            continue
        assert T and T[0][0] == 0 and T[-1][1] == len(doc), (d, T[:1], T[-1:])
        for (s, e, v), nxt in zip(T, T[1:] + [None]):
            assert e > s, (d, s, e)
            if nxt is not None:
                assert nxt[0] == e, (d, e, nxt)
        assert [t for t in T if t[2] >= 0] == _triples(sel[dso[d]:dso[d + 1]]), d
        for i, (s, e, v) in enumerate(T):
            if v >= 0:
                continue
            assert v == -1
            if gap_runs:
                assert i == 0 or T[i - 1][2] >= 0, (d, s)
            else:
                assert all((doc[p] & 0xC0) == 0x80 for p in range(s + 1, e)), (d, s, e)
