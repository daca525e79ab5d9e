"""The replace contract (aha_ac_replace_batch*) over a selection, in plain Python: per document the text's slices between the
selected hits joined with the replacements; a kept key's hit stays as it is.  Slow and obvious on purpose; the tests give it
selectsim's selection of the CPU oracle's hits.  It does not import the library.

repl: a mapping from key index to bytes / str / None (a key it does not name is kept) or a sequence with one entry per key
(None: keep)."""
import numpy as np


def _bytes(r):
    return r.encode("utf-8") if isinstance(r, str) else bytes(r)


def replacement_of(repl, key):
    """the replacement of `key` as bytes, None where the key is kept"""
    r = repl.get(key) if hasattr(repl, "keys") else repl[key]
    return None if r is None else _bytes(r)


def replace_doc(text, sel, repl):
    """one document: text (bytes), sel = its selection as (start, end, value) triples, ascending and non-overlapping"""
    text = bytes(text)
    out, at = [], 0
    for s, e, v in sel:
        s, e, v = int(s), int(e), int(v)
        assert at <= s < e <= len(text), (at, s, e, len(text))
        r = replacement_of(repl, v)
        out.append(text[at:s])
        out.append(text[s:e] if r is None else r)
        at = e
    out.append(text[at:])
    return b"".join(out)


def replace(corpus, doc_offsets, sel, doc_sel_offsets, repl):
    """(result uint8, doc_out_offsets uint64[D+1]) of a batch, its selection and the selection's per-document offsets"""
    corpus = bytes(np.asarray(corpus, dtype=np.uint8).tobytes())
    off = [int(x) for x in doc_offsets]
    dso = [int(x) for x in doc_sel_offsets]
    rows = np.asarray(sel).tolist()
    parts, doo = [], [0]
    for d in range(len(off) - 1):
        parts.append(replace_doc(corpus[off[d]:off[d + 1]], rows[dso[d]:dso[d + 1]], repl))
        doo.append(doo[-1] + len(parts[-1]))
    return np.frombuffer(b"".join(parts), dtype=np.uint8).copy(), np.array(doo, dtype=np.uint64)


def kernel_model(corpus, doc_offsets, sel, doc_sel_offsets, repl):
    """The same result by the arithmetic of the device path, stated with numpy: A, delta, the exclusive scan, O, the last-j tie
    rule and a gather driven by the output positions.  -> (result uint8, doc_out_offsets uint64[D+1])"""
    text = np.asarray(corpus, dtype=np.uint8)
    off = np.asarray(doc_offsets).astype(np.int64)
    dso = np.asarray(doc_sel_offsets).astype(np.int64)
    rows = np.asarray(sel).tolist()
    n = len(rows)
    start = np.array([r[0] for r in rows], dtype=np.int64)
    end = np.array([r[1] for r in rows], dtype=np.int64)
    reps = [replacement_of(repl, int(r[2])) for r in rows]
    # the document of hit j: the largest d with dso[d] <= j
    doc = np.searchsorted(dso[:-1], np.arange(n), side="right") - 1
    A = off[doc] + start
    rlen = np.array([0 if r is None else len(r) for r in reps], dtype=np.int64)  # a kept hit: gap text
    delta = np.array([0 if r is None else len(r) - (e - s) for r, s, e in zip(reps, start, end)], dtype=np.int64)
    shift = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(delta, out=shift[1:])
    doo = off + shift[dso]
    total = int(doo[-1])
    O = A + shift[:n]
    q = np.arange(total, dtype=np.int64)
    j = np.searchsorted(O, q, side="right") - 1  # the LAST j with O[j] <= q; -1: in front of the first
    out = np.zeros(total, dtype=np.uint8)
    jj = np.maximum(j, 0)
    in_rep = (j >= 0) & (q - O[jj] < rlen[jj]) if n else np.zeros(total, dtype=bool)
    gap = ~in_rep
    out[gap] = text[q[gap] - shift[j[gap] + 1]]
    for i in np.nonzero(in_rep)[0].tolist():
        out[i] = reps[j[i]][q[i] - O[j[i]]]
    return out, doo.astype(np.uint64)
