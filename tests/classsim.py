"""Class counts (aha_ac_class_counts_batch*, include/aha_hip.h) in plain numpy.

class_counts is the contract: per document one row of C numbers, the document's hits counted by the classes of their keys.
kernel_model is step 4 of the pipeline as scan_classcount.hip's kcc_add works it -- slices of consecutive hits, the owner search
that steps over documents without hits, the choice between the LDS form and the direct form, the LDS slot indices, the waves'
ballot for equal pairs, the flushes -- with the slice and table sizes as arguments, so that small cases reach every branch.
"""
import numpy as np


def split_hits(values, doc_hit_offsets):
    """the hit values of a batch, document by document -> one array per document"""
    v = np.asarray(values, dtype=np.int64)
    o = np.asarray(doc_hit_offsets, dtype=np.int64)
    return [v[o[d]:o[d + 1]] for d in range(o.size - 1)]


def class_counts(hits_per_doc, class_ids, offsets, C):
    """hits_per_doc: per document the key ids (hit.value) of the hits the match reports for it, in any order; key k belongs to
    the classes class_ids[offsets[k]:offsets[k+1]] -> uint32 (D, C): entry [d, c] = the pairs (hit of d, class of its key)"""
    class_ids = np.asarray(class_ids, dtype=np.int64)
    offsets = np.asarray(offsets, dtype=np.int64)
    out = np.zeros((len(hits_per_doc), C), dtype=np.uint32)
    for d, values in enumerate(hits_per_doc):
        for k in np.asarray(values, dtype=np.int64).tolist():
            for c in class_ids[offsets[k]:offsets[k + 1]].tolist():
                out[d, c] += 1
    return out


def pack_classes(per_key):
    """per key a list of class ids -> (class_ids uint32, offsets uint64[K+1]) as aha_classes_create takes them"""
    offs = np.zeros(len(per_key) + 1, dtype=np.uint64)
    offs[1:] = np.cumsum([len(c) for c in per_key])
    ids = np.array([c for cs in per_key for c in sorted(cs)], dtype=np.uint32)
    return ids, offs


def owner(off, n, sub, x):
    """the largest d in [0, n) with off[d] - sub <= x (off ascends, off[0] - sub <= x): the device's binary search"""
    lo, hi = 1, n
    while lo < hi:
        mid = (lo + hi) >> 1
        if off[mid] - sub <= x:
            lo = mid + 1
        else:
            hi = mid
    return lo - 1


def kernel_model(values, doc_hit_offsets, class_ids, offsets, C, slice_hits, table_words, threads=256, wave=64):
    """kcc_add over one range: values[i] = the key of hit i, the hits document by document, doc_hit_offsets[d] - doc_hit_offsets[0]
    = the first hit of document d.  -> (uint32 (D, C), seen) where seen names what came up: 'lds', 'direct', 'a slice inside one
    document', 'a slice over several documents', 'documents without hits inside a slice', 'a document straddling three slices
    or more', 'a key with no class', 'a key with several classes', 'a row flushed by several slices', 'equal pairs in a wave'"""
    values = np.asarray(values, dtype=np.int64)
    hit_off = [int(x) for x in np.asarray(doc_hit_offsets, dtype=np.uint64)]
    class_ids = np.asarray(class_ids, dtype=np.int64)
    offsets = np.asarray(offsets, dtype=np.int64)
    nd = len(hit_off) - 1
    n_hits = int(values.size)
    assert nd == 0 or hit_off[nd] - hit_off[0] == n_hits
    out = np.zeros(nd * C, dtype=np.uint64)  # (wide: the model adds without wrapping; the result is narrowed at the end)
    seen = set()
    slices_of_doc = np.zeros(max(nd, 1), dtype=np.int64)
    flushes_of_doc = np.zeros(max(nd, 1), dtype=np.int64)
    h0 = hit_off[0] if nd else 0
    n_slices = (n_hits + slice_hits - 1) // slice_hits
    for sl in range(n_slices):
        i0, i1 = sl * slice_hits, min((sl + 1) * slice_hits, n_hits)
        d_lo, d_hi = owner(hit_off, nd, h0, i0), owner(hit_off, nd, h0, i1 - 1)
        span = d_hi - d_lo + 1
        lds = span * C <= table_words
        seen.add("lds" if lds else "direct")
        seen.add("a slice inside one document" if span == 1 else "a slice over several documents")
        if any(hit_off[d + 1] == hit_off[d] for d in range(d_lo + 1, d_hi)):
            seen.add("documents without hits inside a slice")
        table = np.zeros(table_words, dtype=np.uint64) if lds else None
        rows = d_lo * C  # out + d_lo * C

        def add(slot, v):
            if lds:
                assert 0 <= slot < span * C <= table_words
                table[slot] += v
            else:
                assert 0 <= rows + slot < nd * C
                out[rows + slot] += v

        docs_here = set()
        for b in range(i0, i1, threads):
            for w0 in range(0, threads, wave):  # one wave: lanes w0 .. w0 + wave of this round
                lanes = []
                for lane in range(w0, w0 + wave):
                    i = b + lane
                    if i >= i1:
                        continue
                    k = int(values[i])
                    row = owner(hit_off[d_lo:], span, h0, i)
                    d = d_lo + row
                    assert hit_off[d] - h0 <= i < hit_off[d + 1] - h0, "the owner search found another document"
                    docs_here.add(d)
                    j0, n = int(offsets[k]), int(offsets[k + 1] - offsets[k])
                    seen.add("a key with no class" if n == 0 else "a key with several classes" if n > 1 else "a key with one class")
                    lanes.append((row, j0, n))
                j = 0
                while any(j < n for _, _, n in lanes):
                    live = [row * C + int(class_ids[j0 + j]) for row, j0, n in lanes if j < n]
                    first = live[0]  # the wave's first live lane: its pair is taken out by ballot
                    same = sum(1 for s in live if s == first)
                    if same > 1:
                        seen.add("equal pairs in a wave")
                    add(first, same)
                    for s in live:
                        if s != first:
                            add(s, 1)
                    j += 1
        for d in docs_here:
            slices_of_doc[d] += 1
        if lds:
            for k in range(span * C):
                if table[k]:
                    out[rows + k] += table[k]
                    flushes_of_doc[d_lo + k // C] += 1
    if (slices_of_doc >= 3).any():
        seen.add("a document straddling three slices or more")
    if nd and C and (flushes_of_doc > C).any():
        seen.add("a row flushed by several slices")
    assert (out < (1 << 32)).all()
    return out.astype(np.uint32).reshape(nd, C), seen
