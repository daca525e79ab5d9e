"""The contract of the document counts (aha_ac_doc_counts_batch*) stated in numpy, from a hit list: for document d one
{key, count} pair per distinct value among hits[dho[d]:dho[d+1]], ascending by key -- np.unique(values, return_counts=True)."""
import numpy as np

KEY_COUNT_DTYPE = np.dtype([("key", "<i4"), ("count", "<u4")])


def doc_counts(values, doc_hit_offsets):
    """values: the hits' `value` field in document order; doc_hit_offsets: D + 1 offsets into it.
    -> (pairs KEY_COUNT_DTYPE[], doc_pair_offsets uint64[D + 1])"""
    values = np.asarray(values, dtype=np.int64)
    dho = np.asarray(doc_hit_offsets, dtype=np.int64)
    parts, dpo = [], [0]
    for d in range(dho.size - 1):
        k, c = np.unique(values[dho[d]:dho[d + 1]], return_counts=True)
        p = np.zeros(k.size, dtype=KEY_COUNT_DTYPE)
        p["key"], p["count"] = k, c
        parts.append(p)
        dpo.append(dpo[-1] + k.size)
    pairs = np.concatenate(parts) if parts else np.zeros(0, dtype=KEY_COUNT_DTYPE)
    return pairs, np.array(dpo, dtype=np.uint64)


def check_invariants(pairs, dpo, values, dho, n_keys):
    """what must hold between the pairs and the two marginals of the count call"""
    values = np.asarray(values, dtype=np.int64)
    dho = np.asarray(dho, dtype=np.int64)
    dpo = np.asarray(dpo, dtype=np.int64)
    assert dpo[0] == 0 and dpo[-1] == pairs.size and (np.diff(dpo) >= 0).all()
    per_key = np.bincount(pairs["key"].astype(np.int64), weights=pairs["count"].astype(np.float64), minlength=n_keys)
    assert np.array_equal(per_key.astype(np.int64), np.bincount(values, minlength=n_keys))
    csum = np.concatenate([[0], np.cumsum(pairs["count"].astype(np.int64))])
    assert np.array_equal(csum[dpo[1:]] - csum[dpo[:-1]], np.diff(dho))
    for d in range(dpo.size - 1):
        k = pairs["key"][dpo[d]:dpo[d + 1]]
        assert (np.diff(k.astype(np.int64)) > 0).all(), f"document {d}: keys not strictly ascending"
    assert (pairs["count"] > 0).all()
