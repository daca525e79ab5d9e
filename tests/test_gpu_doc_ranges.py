"""The document ranges shared by the doc-count, select, replace and class-count calls (aha_amd/csrc/doc_ranges.hpp and the range
helpers of engine.cpp): one small batch with hitless documents in front, an empty one, a document whose hits alone are beyond
the lowered bound, a run of small documents and a hitless tail, on an unfolded and on a folded handle, with every family's
bound at 12 bytes and at a few documents per range.  Each call against its model over the CPU ORACLE's hits, and the number of
ranges it reports against a transcription of the rule."""
import numpy as np
import pytest

import classsim
import doccountsim
import pyoracle as orc
import replacesim
import test_gpu_class_counts as tcc
import test_gpu_doc_counts as tdc
import test_gpu_replace as trp
import test_gpu_select as tsel
from aha_amd import AC
from aha_amd import _native as N

pytestmark = pytest.mark.gpu

KEYS = [b"ab", b"abc", b"bc", b"bcd", b"cd", b"xyz"]
REPL = [b"X", b"", None, b"longer--", b"yz", b"Q"]
PER_KEY, C = [[0], [1], [], [0, 2], [2], [1]], 3
BOUND_HITS = 20  # the second bound: three or four of the small documents in a range
SMALL = [b"abcd-xyz-q", b"xyz", b"qq-abcd abcd q", b"---", b"bcd.ab.cd"]  # 6, 1, 10, 0 and 5 hits
BIG = 4  # the document whose hits alone are beyond BOUND_HITS


def _docs():
    run = [SMALL[i % 5] + b"." * (i % 4) for i in range(15)]
    return [b"q", b"q--q", b"", b"-abcd"] + [b"abcd" * 30] + run + [b"--", b"q", b""]


def ranges_of(h, bound, cost=lambda x: 12 * x):
    """the rule of doc_ranges.hpp, restated: [(d0, d1, solo)] for the documents' hit counts h"""
    D = len(h)
    if sum(h) == 0:
        return []
    if sum(cost(x) for x in h) <= bound:
        return [(0, D, False)]
    out, d0 = [], 0
    while d0 < D:
        if h[d0] == 0:
            d0 += 1
            continue
        d1, b = d0 + 1, cost(h[d0])
        solo = b > bound
        while not solo and d1 < D and b + cost(h[d1]) <= bound:
            b += cost(h[d1])
            d1 += 1
        out.append((d0, d1, solo))
        d0 = d1
    return out


@pytest.fixture(scope="module")
def ref():
    """the batch in lower case and in mixed case, and every model's answer over the oracle's hits of the lower-case text"""
    low, offs = tdc._batch(_docs())
    assert offs.size - 1 <= 32 and low.size <= 4096 and offs[1] == 1  # (a one-byte first document: every later range is unaligned)
    mixed = low.copy()
    up = (np.arange(mixed.size) % 3 == 0) & (mixed >= ord("a")) & (mixed <= ord("z"))
    mixed[up] -= 32
    o = orc.AC.compile(KEYS)
    sel, dso, hits, dho = tsel._want(o, low, offs)
    h = np.diff(dho.astype(np.int64)).tolist()
    assert h[0] == h[1] == h[2] == 0 and offs[3] == offs[2] and h[-3:] == [0, 0, 0] and h[BIG] > BOUND_HITS
    assert max(h) <= 4096  # (kDcSortMax: every document in the sort form of the doc counts, so its cost is its hits')
    values = np.asarray(hits["value"], dtype=np.int64)
    ids, coffs = classsim.pack_classes(PER_KEY)
    r = {"low": low, "mixed": mixed, "offs": offs, "h": h, "hits": hits, "dho": dho, "sel": sel, "dso": dso,
         "pairs": doccountsim.doc_counts(values, dho), "classes": classsim.class_counts(classsim.split_hits(values, dho), ids, coffs, C),
         "oracle_match": o.match_batch(low, offs)}
    for text in ("low", "mixed"):  # (a folded handle substitutes in the original bytes)
        r["replaced", text] = replacesim.replace(r[text], offs, sel, dso, REPL)
    # what the two bounds make of it, from the oracle's hit counts
    at12, at20 = ranges_of(h, 12), ranges_of(h, 12 * BOUND_HITS)
    assert at12[0][0] == 3 and any(s for _, _, s in at12) and any(not s for _, _, s in at12)  # (one hit: the bound exactly met)
    assert (BIG, BIG + 1, True) in at20 and sum(not s for _, _, s in at20) >= 4
    assert any(sum(x > 0 for x in h[a:b]) in (3, 4) for a, b, s in at20 if not s)
    assert at20[-1][1] == len(h)  # (the hitless tail comes along)
    return r


@pytest.mark.parametrize("bound", [12, 12 * BOUND_HITS])
@pytest.mark.parametrize("fold", [False, True])
def test_every_family_in_document_ranges(ref, fold, bound, monkeypatch):
    for name in ("AHA_DOCCOUNT_HIT_BYTES", "AHA_SELECT_HIT_BYTES", "AHA_CLASS_HIT_BYTES"):
        monkeypatch.setenv(name, str(bound))  # (read when the handle is compiled)
    m = AC.compile(KEYS, fold_ascii=True) if fold else AC.compile(KEYS)
    m.set_profiling(True)
    text, offs, D = ref["mixed" if fold else "low"], ref["offs"], ref["offs"].size - 1
    want_repeats = len(ranges_of(ref["h"], bound)) - 1
    assert want_repeats >= 4
    ct, ot = tsel._tensors(text, offs)
    assert ct.data_ptr() % 16 == 0

    gh, gd = m.match_batch(text, offs)  # the library's own match of the same batch: the hits the models were given
    assert np.asarray(gh).tobytes() == ref["oracle_match"][0].tobytes()
    assert np.array_equal(np.asarray(gd, dtype=np.uint64), ref["dho"])

    want, want_dpo = ref["pairs"]
    pairs, dpo, n, nh, rc = tdc._device(m, ct, ot, D, want.size + 3)
    t = m.last_timing()
    assert rc == N.AHA_OK and n == want.size and nh == ref["hits"].size
    assert np.array_equal(dpo, want_dpo) and pairs.tobytes() == want.tobytes()
    assert t["repeats"] == want_repeats and t["n_hits"] == nh, t

    rows, dso, n, nh, rc = tsel._device(m, ct, ot, D, ref["sel"].size + 3)
    t = m.last_timing()
    assert rc == N.AHA_OK and n == ref["sel"].size and nh == ref["hits"].size
    assert np.array_equal(dso.astype(np.uint64), ref["dso"]) and tsel._as_hits(rows, n).tobytes() == ref["sel"].tobytes()
    assert (rows[n:] == tsel.GUARD).all(), "the call wrote behind the selection"
    assert t["repeats"] == want_repeats and t["n_hits"] == nh, t

    want, want_doo = ref["replaced", "mixed" if fold else "low"]
    got, doo, n, ns, nh, rc = trp._device(m, m.replacements(REPL), ct, ot, D, want.size + 3)
    t = m.last_timing()
    assert rc == N.AHA_OK and (n, ns, nh) == (want.size, ref["sel"].size, ref["hits"].size)
    assert np.array_equal(doo, want_doo) and got[:n].tobytes() == want.tobytes()
    assert t["repeats"] == want_repeats and t["n_hits"] == nh, t

    got, nh = tcc._device(m, m.classes(PER_KEY, n_classes=C), text, offs)
    t = m.last_timing()
    assert nh == ref["hits"].size and np.array_equal(got, ref["classes"])
    assert t["repeats"] == want_repeats and t["n_hits"] == nh, t
