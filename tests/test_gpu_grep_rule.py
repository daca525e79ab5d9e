"""Rule grep (aha_ac_grep_batch* with AHA_GREP_RULE) bit-exact against rulesim over the CPU ORACLE's hits per document (never the
library's own match): kept patterns steered by planted keys over document counts on the edges of a mask word, a wave, a
256-lane block and a 2048-document rank block; 1, 3, 64 and 65536 classes (one chunk of staged columns, a partial one, two,
and two far apart); one term and 64 terms in 8 groups, both ops, num = 0, density terms with empty documents, a group that never passes,
invert; rows given and not, ids only, both capacity failures, the host entry, determinism; a separator filter, folded
handles, a unit-image key set and a keyword list, one-block grids, the table bound; and one handle through a sequence of
calls that share scratch.  Every case is a few KiB of text."""
import random
import zlib

import numpy as np
import pytest

import classsim
import grepsim
import pyoracle as orc
import rulesim
from aha_amd import AC, AhaError, DeviceCorpus
from aha_amd import _native as N
from test_gpu_doc_counts import KEYSETS, SEP_BITS, _batch, _oracle_hits, _sep

pytestmark = pytest.mark.gpu

GUARD8 = 0x5A
GUARD32 = 0x5A5A5A5A
GUARD64 = 0x5A5A5A5A5A5A5A5A
PAD = 16
DEV = "cuda:0"
GE, LT = ">=", "<"
OPS = {GE: rulesim.GE, LT: rulesim.LT}


def _tensors(corpus, offs):
    import torch

    ct = torch.from_numpy(np.ascontiguousarray(corpus)).to(DEV) if corpus.size else torch.zeros(0, dtype=torch.uint8, device=DEV)
    return ct, torch.from_numpy(np.asarray(offs, dtype=np.uint64).view(np.int64)).to(DEV)


def _sim_terms(spec):
    """a spec of AC.rule with classes by index -> rulesim's terms"""
    return [(t[0], OPS[t[1]], g, t[2], t[3] if len(t) == 4 else 0) for g, group in enumerate(spec) for t in group]


def _want(o, per_key, C, corpus, offs, spec, invert, sep_pair=None, oracle_corpus=None):
    """rulesim.grep over the oracle's hits (of oracle_corpus where the handle folds: the bytes kept are the caller's)"""
    v, dho = _oracle_hits(o, corpus if oracle_corpus is None else oracle_corpus, offs, sep_pair)
    ids, coff = classsim.pack_classes(per_key)
    kept, out, doo, rows, ok = rulesim.grep(classsim.split_hits(v, dho), ids, coff, C, offs, corpus, _sim_terms(spec), invert)
    return kept, out, doo, rows, ok, int(v.size)


def _device(m, ct, ot, D, C, rule, cap_docs, cap_bytes, invert=False, sep=None, rows=True, ids_only=False):
    """the device entry with guard words around every buffer -> (kept, doo, out, rows or None, nk, nb, nh, rc); after a failing
    call every buffer, rows included, is still all guard"""
    import torch

    kept = torch.full((cap_docs + PAD,), GUARD64, dtype=torch.int64, device=DEV)
    doo = torch.full((cap_docs + 1 + PAD,), GUARD64, dtype=torch.int64, device=DEV)
    big = torch.full((cap_bytes + 2 * PAD,), GUARD8, dtype=torch.uint8, device=DEV)
    flat = torch.full((D * C + 2 * PAD,), GUARD32, dtype=torch.int32, device=DEV)
    out = None if ids_only else big[PAD:PAD + cap_bytes]
    rows_t = flat[PAD:PAD + D * C].view(D, C) if rows else None
    rc, nh = N.AHA_OK, None
    try:
        nk, nb, nh = m.grep_batch_device(ct, ot, kept, doo, out, sep=sep, invert=invert, cap_docs=cap_docs, rule=rule, rows=rows_t)
    except AhaError as e:
        if e.code == N.AHA_E_CAPACITY:
            rc, nk, nb = e.code, e.n_required, e.bytes_required
        else:
            rc, nk, nb = e.code, None, None
    torch.cuda.synchronize()
    kept_h, doo_h, big_h, flat_h = kept.cpu().numpy(), doo.cpu().numpy(), big.cpu().numpy(), flat.cpu().numpy().view(np.uint32)
    assert (kept_h[cap_docs:] == GUARD64).all() and (doo_h[cap_docs + 1:] == GUARD64).all(), "the call wrote behind cap_docs"
    assert (big_h[:PAD] == GUARD8).all() and (big_h[PAD + cap_bytes:] == GUARD8).all(), "the call wrote outside out"
    assert (flat_h[:PAD] == GUARD32).all() and (flat_h[PAD + D * C:] == GUARD32).all(), "the call wrote outside rows"
    if rc != N.AHA_OK or ids_only:
        assert (big_h == GUARD8).all()
    if rc != N.AHA_OK or not rows:
        assert (flat_h == GUARD32).all(), "rows written by a failing call, or without being given"
    if rc != N.AHA_OK:
        assert (kept_h == GUARD64).all() and (doo_h == GUARD64).all()
    return (kept_h[:cap_docs], doo_h[:cap_docs + 1], big_h[PAD:PAD + cap_bytes], flat_h[PAD:PAD + D * C].reshape(D, C) if rows else None,
            nk, nb, nh, rc)


def _check(m, table, o, per_key, corpus, offs, spec, invert=False, sep_pair=None, sep=None, oracle_corpus=None, host=True,
           want=None):
    """the device entry twice with rows (identical bytes), once without, ids only, and the host entry, against the simulation"""
    C = table.n_classes
    D = len(offs) - 1
    want = want or _want(o, per_key, C, corpus, offs, spec, invert, sep_pair, oracle_corpus)
    w_kept, w_out, w_doo, w_rows, _, w_hits = want
    nk0, nb0 = w_kept.size, w_out.size
    rule = m.rule(spec, table)
    ct, ot = _tensors(corpus, offs)
    first = None
    for given in (True, True, False):
        kept, doo, out, rows, nk, nb, nh, rc = _device(m, ct, ot, D, C, rule, nk0 + 2, nb0 + 5, invert, sep, rows=given)
        assert rc == N.AHA_OK and (nk, nb, nh) == (nk0, nb0, w_hits), (nk, nb, nh, nk0, nb0, w_hits)
        assert np.array_equal(kept[:nk].astype(np.uint64), w_kept) and (kept[nk:] == GUARD64).all()
        assert np.array_equal(doo[:nk + 1].astype(np.uint64), w_doo) and (doo[nk + 1:] == GUARD64).all()
        assert out[:nb].tobytes() == w_out.tobytes() and (out[nb:] == GUARD8).all()
        if given:
            assert np.array_equal(rows, w_rows)
        got = (kept.tobytes(), doo.tobytes(), out.tobytes())
        assert first is None or got == first
        first = got
    kept, doo, out, _, nk, nb, nh, rc = _device(m, ct, ot, D, C, rule, nk0, 0, invert, sep, rows=False, ids_only=True)
    assert rc == N.AHA_OK and (nk, nb, nh) == (nk0, nb0, w_hits)
    assert np.array_equal(kept.astype(np.uint64), w_kept) and np.array_equal(doo.astype(np.uint64), w_doo)
    if host:
        h_rows = np.full((D, C), GUARD32, dtype=np.uint32)
        h_kept, h_out, h_doo = m.grep_batch(corpus, offs, sep=sep, invert=invert, rule=rule, rows=h_rows)
        assert np.array_equal(h_kept, w_kept) and h_out.tobytes() == w_out.tobytes() and np.array_equal(h_doo, w_doo)
        assert np.array_equal(h_rows, w_rows)
    return want


# ---- kept patterns over the edges ------------------------------------------------------------------------------------------
PKEYS = ["KEY", "BAD", "ok"]
PCLASSES = {1: [[0], [], []], 3: [[0], [1], [2]], 64: [[0, 63], [1], [62]]}
EDGES = [1, 31, 32, 33, 63, 64, 65, 255, 256, 257, 2047, 2048, 2049, 4097]


def _pattern_docs(keep):
    """one document per entry: two KEYs where keep is set, else one KEY (a hit, but too few), BAD and ok scattered; some of the
    dropped ones are empty, a few documents are a few hundred bytes long"""
    docs = []
    for d, k in enumerate(keep):
        tail = b"y" * (300 if d % 50 == 3 else d % 5) + (b"BAD" if d % 3 == 0 else b"") + (b"ok" if d % 4 == 1 else b"")
        if k:
            docs.append(b"x" * (d % 7) + b"KEY" + b"q" * (d % 3) + b"KEY" + tail)
        else:
            docs.append(b"" if d % 9 == 4 else b"z" * (d % 6) + (b"KEY" if d % 2 else b"") + tail)
    return docs


def _patterns(D):
    idx = np.arange(D)
    p = {"all": idx >= 0, "none": idx < 0}
    if D >= 2:
        p["alternating"] = idx % 2 == 0
        p["alternating, dropped first"] = idx % 2 == 1
        p["first only"] = idx == 0
        p["last only"] = idx == D - 1
    if D >= 40:
        p["a dropped run across a mask word"] = ~((idx >= 27) & (idx < 37))
        p["a kept run across a mask word"] = (idx >= 27) & (idx < 37)
    if D >= 70:
        p["dropped runs that end and start on word edges"] = ~(((idx >= 20) & (idx < 32)) | ((idx >= 64) & (idx < 70)) | (idx == 63))
    if D >= 260:
        p["a dropped run across a 256-lane block"] = ~((idx >= 250) & (idx < 259))
    if D >= 2049:
        p["a dropped run across a rank block"] = ~((idx >= 2040) & (idx < min(D, 2060)))
        p["a kept run across a rank block"] = (idx >= 2040) & (idx < 2049)
        p["only the rank block's last and the next block's first"] = (idx == 2047) | (idx == 2048)
    return p


@pytest.fixture(scope="module")
def pattern_handles():
    m, o = AC.compile(PKEYS), orc.AC.compile([k.encode() for k in PKEYS])
    return m, o, {C: m.classes(per_key, n_classes=C) for C, per_key in PCLASSES.items()}


@pytest.mark.parametrize("D", EDGES)
def test_kept_patterns_on_the_edges(pattern_handles, D):
    m, o, tables = pattern_handles
    C = (1, 3, 64)[EDGES.index(D) % 3]
    spec = [[(0, GE, 2)]]
    for name, keep in _patterns(D).items():
        corpus, offs = _batch(_pattern_docs(keep))
        for invert in (False, True):
            want = _want(o, PCLASSES[C], C, corpus, offs, spec, invert)
            assert np.array_equal(want[4], keep), name  # (from the simulation: the planted keys steer the pattern)
            if name not in ("all", "none"):
                assert 0 < want[0].size < D, name
            else:
                assert want[0].size == (D if (name == "all") != invert else 0)
            _check(m, tables[C], o, PCLASSES[C], corpus, offs, spec, invert, host=(D in (1, 33, 257) and not invert), want=want)


@pytest.mark.parametrize("C", [1, 3, 64])
def test_every_class_count_on_a_block_edge(pattern_handles, C):
    """D = 257 at every C: one chunk of staged columns and two, over more than one workgroup"""
    m, o, tables = pattern_handles
    keep = np.arange(257) % 3 != 1
    corpus, offs = _batch(_pattern_docs(keep))
    last = C - 1
    for spec in ([[(0, GE, 2)]], [[(0, GE, 2), (last, GE, 0)]], [[(last, LT, 1)], [(0, GE, 3)]]):
        want = _check(m, tables[C], o, PCLASSES[C], corpus, offs, spec)
        assert 0 < want[0].size < 257


def test_65536_classes_over_two_documents():
    keys = ["he", "she", "hers"]
    per_key = [[0, 65535], [40000], []]
    m, o = AC.compile(keys), orc.AC.compile([k.encode() for k in keys])
    table = m.classes(per_key, n_classes=65536)
    corpus, offs = _batch([b"ushers", b"he"])
    for spec, kept in (([[(65535, GE, 1), (40000, GE, 1)]], [0]), ([[(40000, LT, 1)]], [1]), ([[(0, GE, 1, 6)]], [0, 1])):
        want = _check(m, table, o, per_key, corpus, offs, spec)
        assert want[0].tolist() == kept


# ---- rules -----------------------------------------------------------------------------------------------------------------
def _deal(K, C):
    return [[k % C] + ([(k * 7 + 3) % C] if k % 5 == 0 and (k * 7 + 3) % C != k % C else []) for k in range(K)]


@pytest.fixture(scope="module")
def word_handles():
    rng = random.Random(77)
    keys = KEYSETS["ascii"](rng)
    docs = []
    for d in range(300):
        n = rng.choice([0, 0, 3, 9, 40, 120, 300])
        out = bytearray()
        while len(out) < n:
            out += rng.choice(keys) if rng.random() < 0.3 else rng.choice([b" ", b"q", b"zz", b"\x00"])
        docs.append(bytes(out[:n]))
    return keys, AC.compile(keys), orc.AC.compile(keys), _batch(docs)


def test_the_header_example_on_the_device():
    keys = ["he", "she", "hers"]
    per_key = [[0], [0, 1], []]
    m, o = AC.compile(keys), orc.AC.compile([k.encode() for k in keys])
    table = m.classes(per_key, n_classes=2)
    corpus, offs = _batch([b"ushers", b"he"])
    for spec, kept in (([[(0, GE, 2)]], [0]), ([[(0, GE, 1), (1, LT, 1)]], [1]), ([[(0, GE, 1, 3)]], [0, 1])):
        want = _check(m, table, o, per_key, corpus, offs, spec)
        assert want[0].tolist() == kept and want[3].tolist() == [[2, 1], [1, 0]]
        _check(m, table, o, per_key, corpus, offs, spec, invert=True)
    assert m.grep(b"ushers\nhe", rule=[[(0, GE, 2)]], classes=table) == [b"ushers\n"]
    assert m.grep("ushers\nhe", rule=[[(1, LT, 1)]], classes=table) == ["he"]
    kept, out, doo, nh = m.grep_corpus(DeviceCorpus(corpus, offs), rule=m.rule([[(0, GE, 2)]], table))
    assert kept.tolist() == [0] and out.tobytes() == b"ushers" and doo.tolist() == [0, 6] and nh == 4


@pytest.mark.parametrize("C", [3, 64])
def test_rules_of_every_kind(word_handles, C):
    keys, m, o, (corpus, offs) = word_handles
    per_key = _deal(len(keys), C)
    table = m.classes(per_key, n_classes=C)
    D = len(offs) - 1
    assert (np.diff(offs.astype(np.int64)) == 0).sum() > 20  # empty documents are present
    rng = random.Random(C)
    # group g: enough of one class, and seven bounds of both kinds on classes drawn at random
    groups8 = [[((g * 5) % C, GE, 2 + g % 2)] +
               [(rng.randrange(C), *rng.choice([(LT, 4), (LT, 6, 50), (GE, 0), (GE, 1, 400), (LT, 9, 100)])) for _ in range(7)]
               for g in range(8)]
    specs = {
        "one term": [[(1, GE, 2)]],
        "less than": [[(0, LT, 1)]],
        "num = 0 with >=: every document": [[(2, GE, 0)]],
        "num = 0 with <: none, a group that can never pass": [[(2, LT, 0)]],
        "a group that can never pass beside one that can": [[(0, GE, 1), (0, LT, 1)], [(1, GE, 1)]],
        "density, at least": [[(0, GE, 1, 40)]],
        "density, less than": [[(0, LT, 1, 40)]],
        "density and count": [[(0, GE, 3, 200), (1, LT, 2)], [(2, GE, 4)]],
        "64 terms in 8 groups": groups8,
    }
    assert sum(len(g) for g in groups8) == 64
    for name, spec in specs.items():
        want = _check(m, table, o, per_key, corpus, offs, spec, host=name in ("one term", "64 terms in 8 groups"))
        n = want[0].size
        if "every document" in name:
            assert n == D
        elif "none" in name:
            assert n == 0
        else:
            assert 0 < n < D, (name, n)
        _check(m, table, o, per_key, corpus, offs, spec, invert=True, host=False)
    # an empty document follows the formula: kept by "at least n per bytes", dropped by "less than n per bytes"
    empty = np.flatnonzero(np.diff(offs.astype(np.int64)) == 0)
    assert np.isin(empty, _want(o, per_key, C, corpus, offs, specs["density, at least"], False)[0]).all()
    assert not np.isin(empty, _want(o, per_key, C, corpus, offs, specs["density, less than"], False)[0]).any()


def test_group_ids_are_arbitrary_and_terms_unsorted(word_handles):
    """the same rule with its terms shuffled and its groups renumbered through the C ABI's terms: the same bytes"""
    keys, m, o, (corpus, offs) = word_handles
    per_key = _deal(len(keys), 3)
    table = m.classes(per_key, n_classes=3)
    from aha_amd import Rule

    spec = [[(0, GE, 3, 200), (1, LT, 2)], [(2, GE, 4)], [(1, GE, 1), (2, LT, 1), (0, GE, 1)]]
    want = _check(m, table, o, per_key, corpus, offs, spec, host=False)
    base = list(m.rule(spec, table).terms)
    renumber = {0: 65535, 1: 7, 2: 300}
    shuffled = [(c, op, renumber[g], num, den) for c, op, g, num, den in base]
    random.Random(3).shuffle(shuffled)
    assert [t[2] for t in shuffled] != sorted(t[2] for t in shuffled)
    ct, ot = _tensors(corpus, offs)
    D = len(offs) - 1
    kept, doo, out, rows, nk, nb, nh, rc = _device(m, ct, ot, D, 3, Rule(table, shuffled), want[0].size, want[1].size)
    assert rc == N.AHA_OK and np.array_equal(kept.astype(np.uint64), want[0]) and out.tobytes() == want[1].tobytes()
    assert np.array_equal(doo.astype(np.uint64), want[2]) and np.array_equal(rows, want[3])


# ---- capacities --------------------------------------------------------------------------------------------------------------
def test_capacity_failures_report_both_numbers_and_write_nothing(pattern_handles):
    m, o, tables = pattern_handles
    keep = np.arange(100) % 3 == 0
    corpus, offs = _batch(_pattern_docs(keep))
    spec = [[(0, GE, 2)]]
    want = _want(o, PCLASSES[3], 3, corpus, offs, spec, False)
    nk0, nb0 = want[0].size, want[1].size
    assert nk0 > 3 and nb0 > 10
    rule = m.rule(spec, tables[3])
    ct, ot = _tensors(corpus, offs)
    for cap_docs, cap_bytes in ((nk0 - 1, nb0), (nk0, nb0 - 1), (0, 0), (nk0 - 1, nb0 - 1)):
        for rows in (True, False):
            *_, nk, nb, nh, rc = _device(m, ct, ot, 100, 3, rule, cap_docs, cap_bytes, rows=rows)  # (asserts every guard)
            assert rc == N.AHA_E_CAPACITY and (nk, nb) == (nk0, nb0)
    # rows with capacities that cannot fail are written in place; with capacities that can, once the call is known to fit
    for cap_docs, cap_bytes in ((100, corpus.size), (nk0, nb0)):
        kept, doo, out, rows, nk, nb, nh, rc = _device(m, ct, ot, 100, 3, rule, cap_docs, cap_bytes)
        assert rc == N.AHA_OK and np.array_equal(rows, want[3]) and out[:nb].tobytes() == want[1].tobytes()
    # a sizing call succeeds and gives both
    assert m.grep_batch_device(ct, ot, rule=rule)[:2] == (nk0, nb0)


def test_rows_equal_class_counts_batch_device(word_handles):
    import torch

    keys, m, o, (corpus, offs) = word_handles
    per_key = _deal(len(keys), 64)
    table = m.classes(per_key, n_classes=64)
    ct, ot = _tensors(corpus, offs)
    D = len(offs) - 1
    a = torch.zeros((D, 64), dtype=torch.int32, device=DEV)
    b = torch.full((D, 64), -1, dtype=torch.int32, device=DEV)
    nh_a = m.class_counts_batch_device(ct, ot, table, a)
    _, _, nh_b = m.grep_batch_device(ct, ot, rule=[[(5, GE, 1)]], classes=table, rows=b)
    assert nh_a == nh_b and torch.equal(a, b) and int(a.sum()) > 0


# ---- handles and knobs -----------------------------------------------------------------------------------------------------
def test_a_separator_filter(word_handles):
    keys, m, o, (corpus, offs) = word_handles
    per_key = _deal(len(keys), 5)
    table = m.classes(per_key, n_classes=5)
    bits = [i for i in range(40) if i not in SEP_BITS]
    spec = [[(0, GE, 1)], [(3, GE, 1, 100)]]
    filtered = _check(m, table, o, per_key, corpus, offs, spec, sep_pair=(40, bits), sep=_sep())
    plain = _check(m, table, o, per_key, corpus, offs, spec, host=False)
    assert 0 < filtered[5] < plain[5] and filtered[3].sum() < plain[3].sum()  # (the filter drops hits)
    assert 0 < filtered[0].size < len(offs) - 1


def test_folded_handles_keep_the_original_bytes(word_handles):
    keys, _, o, (corpus, offs) = word_handles
    per_key = _deal(len(keys), 3)
    rng = random.Random(9)
    mixed = corpus.copy()
    up = np.array([rng.random() < 0.4 for _ in range(mixed.size)]) & (mixed >= ord("a")) & (mixed <= ord("z"))
    mixed[up] -= 32
    assert up.sum() > 100
    spec = [[(0, GE, 2), (1, LT, 3)]]
    for opts in ({"fold_ascii": True}, {"fold_simple": True}):
        mf = AC.compile(keys, **opts)
        table = mf.classes(per_key, n_classes=3)
        want = _want(o, per_key, 3, mixed, offs, spec, False, oracle_corpus=corpus)
        assert 0 < want[0].size < len(offs) - 1 and want[1].tobytes() != grepsim.grep(want[4].astype(np.int64), offs, corpus, False)[1].tobytes()
        _check(mf, table, o, per_key, mixed, offs, spec, oracle_corpus=corpus, want=want)
    # two-byte characters on a fold_simple handle: keys in lower case, the text partly in upper case
    keys2 = ["é", "ñandú", "жук", "ab"]
    per2 = [[0], [1], [0, 1], []]
    docs_lower = ["é жук", "", "ñandú ab", "xx é é", "жукжук ñandú", "ab", "ééé"] * 6
    docs_mixed = [d.upper() if i % 2 else d for i, d in enumerate(docs_lower)]
    assert all(len(a.encode()) == len(b.encode()) for a, b in zip(docs_lower, docs_mixed))
    lower, offs2 = _batch([d.encode() for d in docs_lower])
    mixed2, _ = _batch([d.encode() for d in docs_mixed])
    m2, o2 = AC.compile(keys2, fold_simple=True), orc.AC.compile([k.encode() for k in keys2])
    t2 = m2.classes(per2, n_classes=2)
    want = _check(m2, t2, o2, per2, mixed2, offs2, [[(0, GE, 2)], [(1, GE, 1), (0, LT, 1)]], oracle_corpus=lower)
    assert 0 < want[0].size < len(docs_lower) and "É".encode() in want[1].tobytes()


@pytest.mark.parametrize("keyset", ["utf8", "keywords"])
def test_a_unit_image_key_set_and_a_keyword_list(keyset):
    from aha_amd import synth

    rng = random.Random(zlib.crc32(keyset.encode()))
    if keyset == "utf8":
        keys = KEYSETS["utf8"](rng)
    else:
        blob, koffs, _ = synth.keys(2)
        keys = [bytes(blob[koffs[i]:koffs[i + 1]]) for i in range(koffs.size - 1)]
    m, o = AC.compile(keys), orc.AC.compile(keys)
    if keyset == "utf8":
        assert m.info["unit_enabled"]
    docs = []
    for d in range(130):
        n = rng.choice([0, 5, 30, 90, 250])
        out = bytearray()
        while len(out) < n:
            out += rng.choice(keys) if rng.random() < 0.25 else rng.choice([b" ", b"q", "中".encode(), b"\n"])
        docs.append(bytes(out[:n]))
    corpus, offs = _batch(docs)
    per_key = _deal(len(keys), 8)
    table = m.classes(per_key, n_classes=8)
    want = _check(m, table, o, per_key, corpus, offs, [[(0, GE, 1), (1, LT, 2)], [(7, GE, 1, 60)]])
    assert 0 < want[0].size < 130


def test_one_block_grids(monkeypatch, pattern_handles):
    """AHA_GREP_BLOCKS=1 with AHA_CLASS_BLOCKS=1: one workgroup loops over all documents and mask words, with one chunk of columns and with two"""
    monkeypatch.setenv("AHA_GREP_BLOCKS", "1")
    monkeypatch.setenv("AHA_CLASS_BLOCKS", "1")
    m = AC.compile(PKEYS)
    _, o, _ = pattern_handles
    keep = (np.arange(2049) % 5 < 2) | (np.arange(2049) == 2048)
    corpus, offs = _batch(_pattern_docs(keep))
    for C in (3, 64):
        table = m.classes(PCLASSES[C], n_classes=C)
        want = _check(m, table, o, PCLASSES[C], corpus, offs, [[(0, GE, 2)]], host=False)
        assert np.array_equal(want[4], keep)
        _check(m, table, o, PCLASSES[C], corpus, offs, [[(0, GE, 2)]], invert=True, host=False)


def test_the_table_bound(monkeypatch, pattern_handles):
    """a tiny AHA_RULE_TABLE_BYTES: AHA_E_TOO_LARGE without rows and nothing written; with rows (and capacities that cannot
    fail) the table goes to the caller and the call succeeds"""
    monkeypatch.setenv("AHA_RULE_TABLE_BYTES", "64")
    m = AC.compile(PKEYS)
    _, o, _ = pattern_handles
    keep = np.arange(40) % 2 == 0
    corpus, offs = _batch(_pattern_docs(keep))
    table = m.classes(PCLASSES[3], n_classes=3)
    spec = [[(0, GE, 2)]]
    rule = m.rule(spec, table)
    want = _want(o, PCLASSES[3], 3, corpus, offs, spec, False)
    ct, ot = _tensors(corpus, offs)
    *_, rc = _device(m, ct, ot, 40, 3, rule, 40, corpus.size, rows=False)  # (asserts that nothing was written)
    assert rc == N.AHA_E_TOO_LARGE
    with pytest.raises(AhaError) as e:
        m.grep_batch_device(ct, ot, rule=rule)
    assert e.value.code == N.AHA_E_TOO_LARGE and "AHA_RULE_TABLE_BYTES" in str(e.value)
    kept, doo, out, rows, nk, nb, nh, rc = _device(m, ct, ot, 40, 3, rule, 40, corpus.size, rows=True)
    assert rc == N.AHA_OK and np.array_equal(kept[:nk].astype(np.uint64), want[0]) and np.array_equal(rows, want[3])
    assert out[:nb].tobytes() == want[1].tobytes()
    # five documents of three classes fit the bound
    small, soffs = _batch(_pattern_docs(keep[:5]))
    _check(m, table, o, PCLASSES[3], small, soffs, spec, host=False)


# ---- one handle through a sequence -------------------------------------------------------------------------------------------
def _answers(m, table, ct, ot, D, corpus, step):
    import torch

    if step == "grep":
        return tuple(x.tobytes() for x in m.grep_batch(corpus, np.asarray(ot.cpu().numpy()).view(np.uint64)))
    if step == "class counts":
        out = torch.zeros((D, table.n_classes), dtype=torch.int32, device=DEV)
        nh = m.class_counts_batch_device(ct, ot, table, out)
        return (out.cpu().numpy().tobytes(), nh)
    rule = m.rule(step, table)
    got = _device(m, ct, ot, D, table.n_classes, rule, D, corpus.size)
    assert got[-1] == N.AHA_OK
    return tuple(x.tobytes() for x in got[:4]) + got[4:]


def test_one_handle_through_a_sequence_equals_fresh_handles(word_handles):
    keys, _, o, (corpus, offs) = word_handles
    per_key = _deal(len(keys), 3)
    ct, ot = _tensors(corpus, offs)
    D = len(offs) - 1
    steps = ["grep", [[(0, GE, 2)]], "class counts", [[(1, LT, 1), (2, GE, 1, 100)]], "grep"]
    m = AC.compile(keys)
    table = m.classes(per_key, n_classes=3)
    for step in steps:
        got = _answers(m, table, ct, ot, D, corpus, step)
        fresh = AC.compile(keys)
        assert got == _answers(fresh, fresh.classes(per_key, n_classes=3), ct, ot, D, corpus, step), step
    # ... and the rule answers are the simulation's
    _check(m, table, o, per_key, corpus, offs, steps[1], host=False)


@pytest.mark.parametrize("D", [257, 513])
def test_plain_grep_is_unchanged_before_and_after_a_rule_grep(D):
    """the kept patterns of the grep statement (test_gpu_grep.py): the same arrays before and after a rule grep on the handle,
    and grepsim's over the oracle's hits"""
    from test_gpu_grep import _check_grep, _hits_per_doc
    from test_gpu_grep import _pattern_docs as plain_docs

    m, o = AC.compile(["KEY"]), orc.AC.compile(["KEY"])
    table = m.classes([[0]], n_classes=1)
    idx = np.arange(D)
    patterns = {"alternating": idx % 2 == 0, "all": idx >= 0, "none": idx < 0, "only the first": idx == 0,
                "a dropped run across a mask word": ~((idx >= 20) & (idx < 40)),
                "a dropped run across a 256-document block": ~((idx >= 250) & (idx < 257)), "runs of three": idx % 6 < 3}
    for name, keep in patterns.items():
        corpus, offs = _batch(plain_docs(keep))
        h = _hits_per_doc(o, corpus, offs)
        before = [x.tobytes() for x in _check_grep(m, corpus, offs, h, host=False)]
        ct, ot = _tensors(corpus, offs)
        nk, _, _ = m.grep_batch_device(ct, ot, rule=[[(0, LT, 1)]], classes=table)  # keeps the complement
        assert nk == D - int(keep.sum()), name
        after = [x.tobytes() for x in _check_grep(m, corpus, offs, h, host=False)]
        assert before == after, name
        _check_grep(m, corpus, offs, h, invert=True, host=False)
