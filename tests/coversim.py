"""The contract of the cover calls (aha_ac_cover_batch*) in numpy, from a batch's hits: a difference array and a cumulative
sum give the bytes that lie inside a hit; from them the mask words, the redacted bytes and the covered bytes per document."""
import numpy as np


def byte_cover(start, end, doc_offsets, hits_doc_offsets):
    """bool[N]: byte j of the batch lies in [start, end) of a hit.  start / end: per hit, byte offsets in the hit's document;
    hits_doc_offsets[d] .. [d + 1]: the hits of document d."""
    doc_offsets = np.asarray(doc_offsets, dtype=np.int64)
    hdo = np.asarray(hits_doc_offsets, dtype=np.int64)
    n = int(doc_offsets[-1])
    start = np.asarray(start, dtype=np.int64)
    end = np.asarray(end, dtype=np.int64)
    base = np.repeat(doc_offsets[:-1], np.diff(hdo))
    diff = np.zeros(n + 1, dtype=np.int64)
    np.add.at(diff, base + start, 1)
    np.add.at(diff, base + end, -1)
    return np.cumsum(diff)[:n] > 0


def mask_words(cover):
    """uint32[ceil(N / 32)]: bit j of the batch = word j >> 5, bit j & 31"""
    n = cover.size
    bits = np.zeros(((n + 31) // 32) * 32, dtype=np.uint8)
    bits[:n] = cover
    return np.packbits(bits, bitorder="little").view(np.uint32).copy() if n else np.zeros(0, dtype=np.uint32)


def unpack(mask, n):
    """bool[n] from the mask words"""
    return np.unpackbits(np.ascontiguousarray(mask, dtype=np.uint32).view(np.uint8), bitorder="little")[:n].astype(bool)


def redacted(corpus, cover, fill):
    out = np.array(corpus, dtype=np.uint8, copy=True)
    out[cover] = fill
    return out


def doc_covered(cover, doc_offsets):
    c = np.concatenate([[0], np.cumsum(cover, dtype=np.int64)])
    doc_offsets = np.asarray(doc_offsets, dtype=np.int64)
    return (c[doc_offsets[1:]] - c[doc_offsets[:-1]]).astype(np.uint64)


def cover_all(start, end, corpus, doc_offsets, hits_doc_offsets, fill=0x2A):
    """-> (mask uint32, redacted uint8, doc_covered uint64[D], n_covered)"""
    cov = byte_cover(start, end, doc_offsets, hits_doc_offsets)
    dc = doc_covered(cov, doc_offsets)
    return mask_words(cov), redacted(corpus, cov, fill), dc, int(cov.sum())


def check_invariants(mask, red, dc, n_covered, corpus, doc_offsets, start, end, hits_doc_offsets, fill):
    """what holds for every answer, whatever the hits are"""
    corpus = np.asarray(corpus, dtype=np.uint8)
    doc_offsets = np.asarray(doc_offsets, dtype=np.int64)
    n = corpus.size
    assert mask.size == (n + 31) // 32
    all_bits = np.unpackbits(np.ascontiguousarray(mask).view(np.uint8), bitorder="little")
    assert not all_bits[n:].any(), "a bit behind the batch is set"
    cov = all_bits[:n].astype(bool)
    assert int(cov.sum()) == int(np.asarray(dc, dtype=np.uint64).sum()) == int(n_covered)
    if red is not None:
        assert np.array_equal(red[~cov], corpus[~cov]), "redacted differs from the corpus outside the mask"
        assert (red[cov] == fill).all()
    h = np.diff(np.asarray(hits_doc_offsets, dtype=np.int64))
    assert not np.asarray(dc)[h == 0].any(), "a set bit in a document without hits"
    assert int(n_covered) <= int((np.asarray(end, dtype=np.int64) - np.asarray(start, dtype=np.int64)).sum())
