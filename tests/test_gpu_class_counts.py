"""Class counts (aha_ac_class_counts_batch, aha_ac_class_counts_batch_device) against classsim.class_counts over the CPU ORACLE's
hits per document (never the library's own match): every engine variant, narrow and wide C, both forms of kcc_add, slice edges
on and off document boundaries, a separator filter, a folded handle, document ranges and the per-key form, one-block grids,
empty input, determinism, neutrality towards the handle's back-off state, the host entry and the Python forms, cross-checks
against the count and document-count calls, and call sequences on one handle.  Every case is a few KiB of text."""
import random
import zlib

import numpy as np
import pytest

import classsim
import pyoracle as orc
from aha_amd import AC, DeviceCorpus
from engine_variants import VARIANTS, use_variant
from test_gpu_doc_counts import KEYSETS, SEP_BITS, _batch, _docs, _oracle_hits, _sep, _tier_batch

pytestmark = pytest.mark.gpu

GUARD = 0x5A5A5A5A
PAD = 16
DEV = "cuda:0"
SLICE, TABLE = 2048, 8192  # kCcSlice, kCcTable (aha_amd/csrc/image.hpp): the cases below are sized around them


def _deal(n_keys, C):
    """keys dealt so that some have no class, some one and some two (C >= 2), the last class among them"""
    per_key = []
    for k in range(n_keys):
        if k % 4 == 0:
            per_key.append([])
        elif k % 4 == 3 and C >= 2:
            a, b = k % C, (k + 1 + k // 4) % C
            per_key.append(sorted({a, b if b != a else (a + 1) % C}))
        else:
            per_key.append([(k * 7 + k // 4) % C])
    if n_keys > 1:
        per_key[1] = [C - 1]
    return per_key


def _want(o, corpus, offs, per_key, C, sep_pair=None):
    """(the table, all hits, hits per document) from the oracle's hits"""
    v, dho = _oracle_hits(o, corpus, offs, sep_pair)
    ids, coffs = classsim.pack_classes(per_key)
    return classsim.class_counts(classsim.split_hits(v, dho), ids, coffs, C), int(v.size), np.diff(dho.astype(np.int64))


def _tensors(corpus, offs):
    import torch

    ct = torch.from_numpy(corpus).to(DEV) if corpus.size else torch.zeros(0, dtype=torch.uint8, device=DEV)
    return ct, torch.from_numpy(offs.view(np.int64)).to(DEV)


def _device(m, table, corpus, offs, sep=None):
    """the device entry with guard words behind D x C entries, all prefilled with the guard -> (uint32 (D, C), n_hits)"""
    import torch

    ct, ot = _tensors(corpus, offs)
    D, C = offs.size - 1, table.n_classes
    buf = torch.full((D * C + PAD,), GUARD, dtype=torch.int32, device=DEV)
    nh = m.class_counts_batch_device(ct, ot, table, buf[: D * C].view(D, C), sep=sep)
    torch.cuda.synchronize()
    h = buf.cpu().numpy().view(np.uint32)
    assert (h[D * C:] == GUARD).all(), "the call wrote behind D x C entries"
    return h[: D * C].reshape(D, C).copy(), nh


def _check(m, o, corpus, offs, per_key, C, sep_pair=None, sep=None, host=True):
    """device entry (and host entry): the same bytes, and those of classsim over the oracle's hits -> (want, hits per document)"""
    want, n_hits, h = _want(o, corpus, offs, per_key, C, sep_pair)
    assert not (want == GUARD).any()  # (so an entry equal to its expectation has been written)
    table = m.classes(per_key, n_classes=C)
    got, nh = _device(m, table, corpus, offs, sep=sep)
    assert nh == n_hits
    assert got.dtype == want.dtype and got.shape == want.shape and np.array_equal(got, want)
    if host:
        out = m.class_counts_batch(corpus, offs, table, sep=sep)
        assert out.dtype == np.uint32 and out.shape == want.shape and out.tobytes() == want.tobytes()
    return want, h


@pytest.fixture(params=VARIANTS)
def variant(request, monkeypatch):
    return use_variant(request.param, monkeypatch)


def test_class_counts_every_engine_variant(variant):
    """one ragged batch on every engine variant (the variables are read when the handle is compiled), C = 3"""
    rng = random.Random(zlib.crc32(f"ccv/{variant}".encode()))
    keys = KEYSETS["utf8"](rng) if variant in ("u", "ur", "u23", "uh", "k", "p") else KEYSETS["ascii"](rng)
    m, o = AC.compile(keys), orc.AC.compile(keys)
    docs = _docs(rng, keys, 12, 1500, 0.6) + [b"".join(rng.choice(keys) for _ in range(1500))]
    corpus, offs = _batch(docs)
    per_key = _deal(len(keys), 3)
    assert {len(c) for c in per_key} == {0, 1, 2}
    want, h = _check(m, o, corpus, offs, per_key, 3)
    assert want.sum() > 0 and h.sum() > SLICE  # (more than one slice)


@pytest.mark.parametrize("keyset", sorted(KEYSETS))
def test_class_counts_ragged_documents_of_every_key_set(keyset):
    rng = random.Random(zlib.crc32(f"cc/{keyset}".encode()))
    keys = KEYSETS[keyset](rng)
    m, o = AC.compile(keys), orc.AC.compile(keys)
    corpus, offs = _batch(_docs(rng, keys, 9, 900, 0.5))
    _check(m, o, corpus, offs, _deal(len(keys), 3), 3)


@pytest.mark.parametrize("C", [1, 2, 7, 64, 8193])
def test_class_counts_narrow_and_wide_tables(C):
    """C = 8193 cannot fit the LDS table even for one document: the direct form"""
    rng = random.Random(C)
    keys = KEYSETS["ascii"](rng)
    m, o = AC.compile(keys), orc.AC.compile(keys)
    corpus, offs = _batch(_docs(rng, keys, 10, 800, 0.6))
    per_key = _deal(len(keys), C)
    assert max(max(c) for c in per_key if c) == C - 1
    want, h = _check(m, o, corpus, offs, per_key, C)
    assert want[:, C - 1].sum() > 0 and (C <= TABLE) == (C != 8193)


def test_class_counts_many_tiny_documents_take_the_direct_form():
    """C = 64 over 513 documents of one or two hits each: one slice whose span x C is beyond the table"""
    NK = 100
    keys = [b"k%d;" % i for i in range(NK)]
    m, o = AC.compile(keys), orc.AC.compile(keys)
    rng = random.Random(64)
    counts = [rng.choice([1, 2]) for _ in range(513)]
    corpus, offs = _batch(_tier_batch(rng, NK, counts))
    want, h = _check(m, o, corpus, offs, _deal(NK, 64), 64)
    assert h.tolist() == counts and h.sum() <= SLICE and 513 * 64 > TABLE  # (from the oracle)


def test_class_counts_lds_form_over_many_documents():
    """C = 4 over 257 documents of about ten hits each: slices of some two hundred documents, span x C inside the table"""
    NK = 100
    keys = [b"k%d;" % i for i in range(NK)]
    m, o = AC.compile(keys), orc.AC.compile(keys)
    rng = random.Random(4)
    counts = [rng.randint(8, 12) for _ in range(257)]
    corpus, offs = _batch(_tier_batch(rng, NK, counts))
    want, h = _check(m, o, corpus, offs, _deal(NK, 4), 4)
    assert h.tolist() == counts and h.sum() > SLICE and 257 * 4 <= TABLE


def test_class_counts_one_document_over_five_slices():
    """keys a, aa, aaa over one document of 3000 a: about 9000 hits -- five slices in one document, a hot slot, a row flushed by
    several workgroups"""
    keys = [b"a", b"aa", b"aaa"]
    m, o = AC.compile(keys), orc.AC.compile(keys)
    corpus, offs = _batch([b"a" * 3000])
    for per_key, C in (([[0], [1], [0, 2]], 3), ([[0], [0], [0]], 1), ([[], [5], []], 6)):
        want, h = _check(m, o, corpus, offs, per_key, C)
        assert h.tolist() == [8997]
    assert -(-8997 // SLICE) == 5


@pytest.mark.parametrize("n", [2047, 2048, 2049])
def test_class_counts_slice_boundary_at_a_document_boundary(n):
    """key a alone over a first document of n a, an empty document, a document without hits and a document with hits: with n =
    2048 the slice boundary falls on the document boundary and the owner search steps over two hitless documents"""
    m, o = AC.compile([b"a"]), orc.AC.compile([b"a"])
    corpus, offs = _batch([b"a" * n, b"", b"xyz", b"aaxa", b"", b"a"])
    want, h = _check(m, o, corpus, offs, [[1]], 2)
    assert h.tolist() == [n, 0, 0, 3, 0, 1] and want[:, 1].tolist() == h.tolist() and not want[:, 0].any()


def test_class_counts_with_a_separator_filter_and_on_a_folded_handle():
    rng = random.Random(31)
    keys = KEYSETS["ascii"](rng)
    m, o = AC.compile(keys), orc.AC.compile(keys)
    corpus, offs = _batch(_docs(rng, keys, 12, 900, 0.5))
    per_key = _deal(len(keys), 5)
    bits = [i for i in range(40) if i not in SEP_BITS]
    want_sep, h_sep = _check(m, o, corpus, offs, per_key, 5, (40, bits), _sep())
    want, h = _check(m, o, corpus, offs, per_key, 5)
    assert 0 < h_sep.sum() < h.sum()  # (the filter drops hits)
    # a folded handle: text in mixed case; the expectation is the oracle's over the lower-cased text
    mf = AC.compile(keys, fold_ascii=True)
    mixed = corpus.copy()
    up = np.array([rng.random() < 0.4 for _ in range(mixed.size)]) & (mixed >= ord("a")) & (mixed <= ord("z"))
    mixed[up] -= 32
    assert up.sum() > 100
    wf, nf, _ = _want(o, corpus, offs, per_key, 5)
    table = mf.classes(per_key, n_classes=5)
    got, nh = _device(mf, table, mixed, offs)
    assert nh == nf and np.array_equal(got, wf)
    assert mf.class_counts_batch(mixed, offs, table).tobytes() == wf.tobytes()


def test_class_counts_in_document_ranges(monkeypatch):
    """AHA_CLASS_HIT_BYTES lowered: several ranges of whole documents; then below one document's hit list, so that the per-key
    form answers for that document.  Both give the bytes of the unbounded call."""
    rng = random.Random(9)
    keys = KEYSETS["ascii"](rng)
    o = orc.AC.compile(keys)
    docs = _docs(rng, keys, 16, 1200, 0.5)
    docs[5] = b"".join(rng.choice(keys) for _ in range(2500))
    corpus, offs = _batch(docs)
    per_key = _deal(len(keys), 6)
    m0 = AC.compile(keys)  # (the knob is read when the handle is compiled)
    want, h = _check(m0, o, corpus, offs, per_key, 6)
    big = int(h[5])
    assert big > 2000 and h.sum() - big > 3 * 700 and np.delete(h, 5).max() < 700  # (from the oracle)
    for bound_hits, solo in ((big + 10, False), (700, True)):
        monkeypatch.setenv("AHA_CLASS_HIT_BYTES", str(12 * bound_hits))
        m = AC.compile(keys)
        m.set_profiling(True)
        table = m.classes(per_key, n_classes=6)
        got, nh = _device(m, table, corpus, offs)
        t = m.last_timing()
        assert t["repeats"] >= (3 if solo else 1) and t["n_hits"] == int(h.sum()) == nh, t
        assert got.tobytes() == want.tobytes()
        assert m.class_counts_batch(corpus, offs, table).tobytes() == want.tobytes()
    # the oversized document alone, and first / last in its batch
    for batch in ([docs[5]], [docs[5], b"", docs[1]], [docs[1], b"", docs[5]]):
        c2, o2 = _batch(batch)
        _check(m, o, c2, o2, per_key, 6)


def test_class_counts_with_one_block_grids(monkeypatch):
    """AHA_CLASS_BLOCKS=1: one workgroup loops over all slices, in both forms"""
    monkeypatch.setenv("AHA_CLASS_BLOCKS", "1")
    NK = 100
    keys = [b"k%d;" % i for i in range(NK)]
    m, o = AC.compile(keys), orc.AC.compile(keys)
    rng = random.Random(77)
    counts = [rng.choice([0, 1, 2, 30, 500]) for _ in range(60)] + [2500]
    corpus, offs = _batch(_tier_batch(rng, NK, counts))
    for C in (4, 8193):
        want, h = _check(m, o, corpus, offs, _deal(NK, C), C, host=False)
        assert h.tolist() == counts and h.sum() > 3 * SLICE


def test_class_counts_empty_input():
    keys = [b"he", b"she", b"hers"]
    m, o = AC.compile(keys), orc.AC.compile(keys)
    per_key = [[0], [0, 1], []]
    none = np.zeros(0, dtype=np.uint8)
    _check(m, o, none, np.array([0], dtype=np.uint64), per_key, 2)  # D = 0
    want, _ = _check(m, o, none, np.array([0, 0, 0, 0], dtype=np.uint64), per_key, 2)  # N = 0 with D = 3
    assert want.shape == (3, 2) and not want.any()
    corpus, offs = _batch([b"ushers", b"", b"xx", b"he"])
    want, h = _check(m, o, corpus, offs, [[], [], []], 3)  # no key has a class
    assert h.sum() == 4 and not want.any()
    want, _ = _check(m, o, corpus, offs, per_key, 2)
    assert want.tolist() == [[2, 1], [0, 0], [0, 0], [1, 0]]


def test_class_counts_two_calls_give_identical_bytes():
    rng = random.Random(13)
    keys = KEYSETS["nested"](rng)
    m = AC.compile(keys)
    corpus, offs = _batch(_docs(rng, keys, 20, 1500, 0.7))
    table = m.classes(_deal(len(keys), 5), n_classes=5)
    a, na = _device(m, table, corpus, offs)
    b, nb = _device(m, table, corpus, offs)
    assert a.tobytes() == b.tobytes() and na == nb and a.sum() > 0


def test_class_counts_leave_no_trace_in_the_back_off(monkeypatch):
    """match -> class counts -> match on a handle whose first match is handed back by the prefix-filter engine: every later match
    gives the hits, the engine and the repeats of a twin handle that never saw the call in between."""
    monkeypatch.delenv("AHA_ENGINE", raising=False)
    dense = b"abcd" * 3000
    sparse = b"-" * 5000 + b"abcd"

    def run(with_counts):
        m = AC.compile(["abc", "bcd"])
        assert m.info["filter_prefix_bytes"] == 3
        m.set_profiling(True)
        table = m.classes([0, 1])
        seen = []
        for text in [dense] + [sparse] * 6 + [dense] + [sparse] * 3:
            hits = m.match_array(text)
            t = m.last_timing()
            seen.append((t["engine"], t["repeats"], hits.tobytes()))
            if with_counts:
                for t2 in (dense, sparse):
                    rows = m.class_counts_batch(t2, [0, 100, len(t2)], table)
                    assert rows.sum(axis=0).tolist() == ([3000, 3000] if t2 is dense else [1, 1])
                    assert m.last_timing()["n_hits"] == (6000 if t2 is dense else 2)
        m.release_scratch()
        assert m.scratch_bytes() == 0
        return seen

    plain = run(False)
    assert plain[0][0] == 2 and plain[1][0] == 2 and plain[6][0] == 5, [p[:2] for p in plain]
    assert run(True) == plain


def test_class_counts_python_forms():
    keys = ["he", "she", "hers"]
    m = AC.compile(keys)
    t = m.classes({"pronoun": ["he", "she"], "female": ["she"]})
    assert t.names == ["pronoun", "female"]
    assert m.class_counts("ushers", t).tolist() == [2, 1] and m.class_counts(b"he", t).dtype == np.uint32
    assert m.class_counts("ushers", [0, (0, 1), None]).tolist() == [2, 1]  # a spec in place of a table
    corpus, offs = _batch([b"ushers", b"he"])
    assert m.class_counts_batch(corpus, offs, t).tolist() == [[2, 1], [1, 0]]
    assert m.class_counts_batch(b"ushershe", [0, 6, 8], t).tolist() == [[2, 1], [1, 0]]
    rows, nh = m.class_counts_corpus(DeviceCorpus(corpus, offs), t)
    assert rows.tolist() == [[2, 1], [1, 0]] and rows.dtype == np.uint32 and nh == 4
    ct, ot = _tensors(corpus, offs)
    import torch

    with pytest.raises(ValueError):
        m.class_counts_batch_device(ct, ot, t, torch.zeros((2, 3), dtype=torch.int32, device=DEV))
    with pytest.raises(ValueError):
        m.class_counts_batch_device(ct, ot, t, torch.zeros((2, 2), dtype=torch.int64, device=DEV))


def test_class_counts_against_the_count_and_document_count_calls():
    rng = random.Random(55)
    keys = KEYSETS["ascii"](rng)
    m = AC.compile(keys)
    K = len(keys)
    corpus, offs = _batch(_docs(rng, keys, 14, 1200, 0.6))
    D = offs.size - 1
    # every key in exactly one class: the row sums are the documents' hit counts
    one = m.classes([[k % 5] for k in range(K)], n_classes=5)
    rows, nh = _device(m, one, corpus, offs)
    _, dho = m.count_batch(corpus, offs, per_key=False)
    assert np.array_equal(rows.sum(axis=1).astype(np.int64), np.diff(np.asarray(dho).astype(np.int64))) and nh == int(dho[-1]) > 0
    # C = K and the identity table: the row is doc_counts_batch made dense
    ident = m.classes(list(range(K)))
    rows, _ = _device(m, ident, corpus, offs)
    pairs, dpo = m.doc_counts_batch(corpus, offs)
    dense = np.zeros((D, K), dtype=np.uint32)
    docid = np.searchsorted(np.asarray(dpo).astype(np.int64), np.arange(pairs.size), side="right") - 1
    dense[docid, pairs["key"]] = pairs["count"]
    assert np.array_equal(rows, dense) and dense.sum() == nh


def test_class_counts_between_other_calls_on_one_handle():
    """class counts, select, class counts, grep, class counts on one handle: each result equals its stand-alone result"""
    rng = random.Random(88)
    keys = KEYSETS["ascii"](rng)
    corpus, offs = _batch(_docs(rng, keys, 10, 1000, 0.6))
    other, ooffs = _batch(_docs(rng, keys, 25, 300, 0.3))
    per_key = _deal(len(keys), 4)

    def alone(call):
        m = AC.compile(keys)
        return call(m, m.classes(per_key, n_classes=4))

    cc1 = lambda m, t: m.class_counts_batch(corpus, offs, t).tobytes()  # noqa: E731
    cc2 = lambda m, t: m.class_counts_batch(other, ooffs, t).tobytes()  # noqa: E731
    sel = lambda m, t: tuple(a.tobytes() for a in m.select_batch(corpus, offs))  # noqa: E731
    grp = lambda m, t: tuple(np.asarray(a).tobytes() for a in m.grep_batch(other, ooffs))  # noqa: E731
    want = [alone(c) for c in (cc1, sel, cc2, grp, cc1)]
    m = AC.compile(keys)
    t = m.classes(per_key, n_classes=4)
    got = [c(m, t) for c in (cc1, sel, cc2, grp, cc1)]
    assert got == want and got[0] == got[4] and got[0] != got[2]
