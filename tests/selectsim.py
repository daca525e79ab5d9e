"""The select contract (aha_ac_select_batch*) over a hit list, straight from the greedy definition: per document, p = 0;
among the hits with start >= p take the smallest start, of those the largest end; emit it, p = its end; repeat.  Plain Python
over (start, end, value) triples -- slow and obvious on purpose; the tests give it the CPU oracle's hits."""
import numpy as np

HIT_DTYPE = np.dtype([("start", "<i4"), ("end", "<i4"), ("value", "<i4")])


def _triples(hits):
    return [(int(s), int(e), int(v)) for s, e, v in np.asarray(hits).tolist()]


def select_doc(hits):
    """the selection of ONE document's hits (any order) as a list of (start, end, value)"""
    hits = _triples(hits)
    out, p = [], 0
    while True:
        cand = [h for h in hits if h[0] >= p]
        if not cand:
            return out
        s = min(h[0] for h in cand)
        best = max((h for h in cand if h[0] == s), key=lambda h: h[1])
        assert sum(1 for h in cand if h[0] == s and h[1] == best[1]) == 1, "keys are distinct: one hit per (start, end)"
        out.append(best)
        p = best[1]


def select(hits, doc_hit_offsets):
    """(selected hits HIT_DTYPE, doc_sel_offsets uint64[D+1]) of a batch's hit list and its per-document offsets"""
    dho = [int(x) for x in doc_hit_offsets]
    sel, dso = [], [0]
    for d in range(len(dho) - 1):
        sel += select_doc(hits[dho[d]:dho[d + 1]])
        dso.append(len(sel))
    out = np.zeros(len(sel), dtype=HIT_DTYPE)
    for i, (s, e, v) in enumerate(sel):
        out[i] = (s, e, v)
    return out, np.array(dso, dtype=np.uint64)


def check_invariants(sel, doc_sel_offsets, hits, doc_hit_offsets):
    """per document: ascending, non-overlapping; every selected hit is one of the document's hits; no hit of the document
    starts in a gap -- at or behind the previous selected end (0 at first) and before the next selected start (or at all,
    behind the last)"""
    dso = [int(x) for x in doc_sel_offsets]
    dho = [int(x) for x in doc_hit_offsets]
    assert len(dso) == len(dho) and dso[0] == 0 and dso[-1] == len(sel)
    for d in range(len(dho) - 1):
        H = _triples(hits[dho[d]:dho[d + 1]])
        S = _triples(sel[dso[d]:dso[d + 1]])
        members = set(H)
        p = 0
        for s, e, v in S:
            assert (s, e, v) in members, (d, s, e, v)
            assert s >= p and e > s, (d, s, e, p)
            assert not any(p <= h[0] < s for h in H), (d, p, s)
            assert not any(h[0] == s and h[1] > e for h in H), (d, s, e)
            p = e
        assert not any(h[0] >= p for h in H), (d, p)
