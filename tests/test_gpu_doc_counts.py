"""Document counts (aha_ac_doc_counts_batch, aha_ac_doc_counts_batch_device) against doccountsim over the CPU ORACLE's hits
(never the library's own match): the reference KATs, the synthetic configs, UTF-8 with and without a separator filter, every
engine variant, every form of the reduction with its thresholds lowered, document ranges, capacity, neutrality towards the
handle's back-off state, and the configs at size."""
import json
import os
import random
import zlib

import numpy as np
import pytest

import doccountsim
import pyoracle as orc
from aha_amd import AC, AhaError, BitArray, DeviceCorpus, synth
from aha_amd import _native as N
from engine_variants import VARIANTS, use_variant

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = 0x5A5A5A5A
PAD = 16
SEP_BITS = [32, 0]  # a space and a NUL separate
DEV = "cuda:0"


def _keys_ascii(rng):
    words = sorted({"".join(rng.choice("abcdefgh") for _ in range(rng.randint(3, 9))) for _ in range(600)})
    return [w.encode() for w in words]


def _keys_utf8(rng):
    blob, offs, _ = synth.keys(3, K=3000, seed=7)
    return [bytes(blob[offs[i]:offs[i + 1]]) for i in range(offs.size - 1)]


def _keys_nested(rng):
    return [b"a" * i for i in range(1, 24)] + [("我" * i).encode() for i in range(1, 21)] + [b"ba", b"bab", b"abab"]


KEYSETS = {"ascii": _keys_ascii, "utf8": _keys_utf8, "nested": _keys_nested}


def _docs(rng, keys, n_docs, size, density):
    pieces = [k for k in keys if len(k) < 64] or [b"x"]
    fill = [b" ", b"q", b"\x00", b"zz", "中".encode(), b"a", b"x"]
    docs = []
    for _ in range(n_docs):
        n = rng.choice([0, size // 4, size, size * 2]) if rng.random() < 0.3 else size
        out = bytearray()
        while len(out) < n:
            out += rng.choice(pieces) if rng.random() < density else rng.choice(fill)
        docs.append(bytes(out[:n]))  # (cut anywhere: keys cross document boundaries, characters may be cut)
    docs[0] = b""
    if n_docs > 2:
        docs[n_docs // 2] = b""
    return docs


def _batch(docs):
    corpus = np.frombuffer(b"".join(docs), dtype=np.uint8).copy()
    offs = np.cumsum([0] + [len(d) for d in docs]).astype(np.uint64)
    return corpus, offs


def _sep():
    sep = BitArray(40)
    for i in range(40):
        sep[i] = i not in SEP_BITS
    return sep


def _oracle_hits(o, corpus, offs, sep=None):
    """(values, doc hit offsets) of the oracle's match of the batch; sep = (size, set bits) or None"""
    if sep is None:
        hits, dho = o.match_batch(corpus, offs)
        return np.asarray(hits["value"], dtype=np.int64), np.asarray(dho, dtype=np.uint64)
    parts, dho = [], [0]
    for d in range(offs.size - 1):
        h = o.match(corpus[int(offs[d]):int(offs[d + 1])].tobytes(), chars=False, sep=sep)
        parts.append(np.asarray(h["value"], dtype=np.int64) if h.size else np.zeros(0, np.int64))
        dho.append(dho[-1] + h.size)
    return (np.concatenate(parts) if parts else np.zeros(0, np.int64)), np.array(dho, dtype=np.uint64)


def _want(o, corpus, offs, sep=None):
    v, dho = _oracle_hits(o, corpus, offs, sep)
    pairs, dpo = doccountsim.doc_counts(v, dho)
    return pairs, dpo, int(v.size), dho


def _device(m, ct, ot, D, cap, sep=None, chars=False):
    """the device entry with guard words behind cap pairs and behind the D + 1 offsets -> (pairs, dpo, n_pairs, n_hits, rc)"""
    import torch

    out = torch.full((cap + PAD, 2), GUARD, dtype=torch.int32, device=ct.device)
    dpo = torch.full((D + 1 + PAD,), GUARD, dtype=torch.int64, device=ct.device)
    rc = N.AHA_OK
    try:
        n, nh = m.doc_counts_batch_device(ct, ot, out, dpo, sep=sep, chars=chars, cap=cap)
    except AhaError as e:
        if e.code != N.AHA_E_CAPACITY:
            raise
        rc, n, nh = e.code, e.n_required, e.n_hits
    torch.cuda.synchronize()
    out_h = out.cpu().numpy()
    dpo_h = dpo.cpu().numpy()
    assert (out_h[cap:] == GUARD).all(), "the call wrote behind cap pairs"
    assert (dpo_h[D + 1:] == GUARD).all(), "the call wrote behind the D + 1 offsets"
    pairs = np.ascontiguousarray(out_h[:min(n, cap)]).view(doccountsim.KEY_COUNT_DTYPE).reshape(-1)
    return pairs, dpo_h[:D + 1].astype(np.uint64), n, nh, rc


def _check_all_entries(m, o, corpus, offs, sep_pair=None, sep=None):
    """host entry, device entry (byte and char offsets): the same bytes, and those of doccountsim over the oracle's hits"""
    import torch

    want, want_dpo, want_n, _ = _want(o, corpus, offs, sep_pair)
    D = offs.size - 1
    pairs, dpo = m.doc_counts_batch(corpus, offs, sep=sep)
    assert np.array_equal(dpo, want_dpo)
    assert pairs.tobytes() == want.tobytes()
    ct = torch.from_numpy(corpus).to(DEV) if corpus.size else torch.zeros(0, dtype=torch.uint8, device=DEV)
    ot = torch.from_numpy(offs.view(np.int64)).to(DEV)
    for chars in (False, True):
        dp, ddpo, n, nh, rc = _device(m, ct, ot, D, want.size + 3, sep=sep, chars=chars)
        assert rc == N.AHA_OK and n == want.size and nh == want_n
        assert np.array_equal(ddpo, want_dpo) and dp.tobytes() == want.tobytes() == pairs.tobytes()
    return want, want_dpo


def test_doc_counts_reference_kats():
    kats = json.load(open(os.path.join(ROOT, "tests", "golden", "reference_kats.json"), encoding="utf-8"))["ac_match"]
    assert kats
    for kat in kats:
        keys = [k.encode() for k in kat["keys"]]
        m, o = AC.compile(keys), orc.AC.compile(kat["keys"])
        text = kat["text"].encode()
        corpus, offs = _batch([text, b"", text + text, text[: len(text) // 2]])
        sp, sep = None, None
        if kat["sep"] is not None:
            sp = (kat["sep"]["size"], kat["sep"]["set"])
            sep = BitArray(sp[0])
            for i in sp[1]:
                sep[i] = True
        _check_all_entries(m, o, corpus, offs, sp, sep)
    m = AC.compile(["he", "she", "his", "hers"])
    assert m.doc_counts("ushers") == {0: 1, 1: 1, 3: 1}


@pytest.mark.parametrize("cfg", [1, 2, 3, 5])
def test_doc_counts_synthetic_configs(cfg):
    """the configs' key sets at a few MiB (cfg 1: cfg 2's generator at 100 keys)"""
    gen = 2 if cfg == 1 else cfg
    K = {1: 100, 2: 1000, 3: 20000, 5: 50000}[cfg]
    blob, koffs, nf = synth.keys(gen, K=K)
    corpus, doc = synth.corpus(gen, blob, koffs, nf, n_bytes=3 << 20, doc_bytes=1 << 16)
    keys = [bytes(blob[koffs[i]:koffs[i + 1]]) for i in range(koffs.size - 1)]
    m, o = AC.compile_packed(blob, koffs), orc.AC.compile(keys)
    want, want_dpo = _check_all_entries(m, o, corpus, doc)
    assert want.size > 0
    p, dpo, nh = m.doc_counts_corpus(DeviceCorpus(corpus, doc))
    assert p.tobytes() == want.tobytes() and np.array_equal(dpo, want_dpo)


@pytest.mark.parametrize("keyset", sorted(KEYSETS))
def test_doc_counts_random_utf8_with_and_without_separator(keyset):
    rng = random.Random(zlib.crc32(f"dc/{keyset}".encode()))
    keys = KEYSETS[keyset](rng)
    m, o = AC.compile(keys), orc.AC.compile(keys)
    for n_docs, size, density in ((7, 300, 0.3), (40, 2000, 0.6), (3, 70000, 0.9)):
        corpus, offs = _batch(_docs(rng, keys, n_docs, size, density))
        _check_all_entries(m, o, corpus, offs)
        bits = [i for i in range(40) if i not in SEP_BITS]
        _check_all_entries(m, o, corpus, offs, (40, bits), _sep())


@pytest.fixture(params=VARIANTS)
def variant(request, monkeypatch):
    return use_variant(request.param, monkeypatch)


def test_doc_counts_every_engine_variant(variant):
    """one ragged batch on every engine variant (the variables are read when the handle is compiled)"""
    rng = random.Random(zlib.crc32(f"dcv/{variant}".encode()))
    keys = _keys_utf8(rng) if variant in ("u", "ur", "u23", "uh", "k", "p") else _keys_ascii(rng)
    m, o = AC.compile(keys), orc.AC.compile(keys)
    docs = _docs(rng, keys, 24, 3000, 0.6) + [b"".join(rng.choice(keys) for _ in range(4000))]
    corpus, offs = _batch(docs)
    want, _ = _check_all_entries(m, o, corpus, offs)
    assert want.size > 0


def _tier_batch(rng, n_keys_used, counts):
    """documents with exactly the given hit counts: keys 'k<i>;' never overlap, filler matches nothing"""
    docs = []
    for h in counts:
        docs.append(b"".join(b"k%d;" % rng.randrange(n_keys_used) for _ in range(h)) + b"--" * rng.randrange(3))
    return docs


def test_doc_counts_every_form_around_its_threshold(monkeypatch):
    """thresholds lowered by their knobs: sort form up to 16 hits, range form (ranges of 64 key ids: five passes over 300 keys)
    up to 39, dense form from 40 on, two rows in flight.  Asserted from the ORACLE's hit counts before anything is compared."""
    SORT_MAX, DENSE_MIN, NK = 16, 40, 300
    monkeypatch.setenv("AHA_DOCCOUNT_SORT_MAX", str(SORT_MAX))
    monkeypatch.setenv("AHA_DOCCOUNT_DENSE_MIN", str(DENSE_MIN))
    monkeypatch.setenv("AHA_DOCCOUNT_RANGE_KEYS", "64")
    monkeypatch.setenv("AHA_DOCCOUNT_ROW_BYTES", str(2 * NK * 4))
    keys = [b"k%d;" % i for i in range(NK)]
    m, o = AC.compile(keys), orc.AC.compile(keys)
    rng = random.Random(5)
    counts = [0, 0, 0, 1, SORT_MAX - 1, SORT_MAX, SORT_MAX + 1, 0, 0, DENSE_MIN - 1, DENSE_MIN, DENSE_MIN + 1, 2, 700, 0, 90, 41,
              5000, 0, 0]
    corpus, offs = _batch(_tier_batch(rng, NK, counts))
    _, dho = _oracle_hits(o, corpus, offs)
    h = np.diff(dho.astype(np.int64))
    assert h.tolist() == counts
    in_sort = (h > 0) & (h <= SORT_MAX)
    in_range = (h > SORT_MAX) & (h < DENSE_MIN)
    in_dense = h >= DENSE_MIN
    assert in_sort.sum() >= 4 and in_range.sum() >= 2 and in_dense.sum() >= 5  # (five dense documents: three groups of rows)
    for t in (SORT_MAX - 1, SORT_MAX, SORT_MAX + 1, DENSE_MIN - 1, DENSE_MIN, DENSE_MIN + 1, 0, 1):
        assert (h == t).any()
    _check_all_entries(m, o, corpus, offs)
    # one document holding all hits (each form), empty documents first / last / in runs, an empty batch, no bytes
    for one in (SORT_MAX, DENSE_MIN - 1, 3000):
        corpus, offs = _batch([b"", b""] + _tier_batch(rng, NK, [one]) + [b"", b"", b""])
        _check_all_entries(m, o, corpus, offs)
    _check_all_entries(m, o, np.zeros(0, dtype=np.uint8), np.array([0], dtype=np.uint64))
    _check_all_entries(m, o, np.zeros(0, dtype=np.uint8), np.array([0, 0, 0, 0], dtype=np.uint64))
    # the sort form at its full size, the defaults otherwise: K below the sort form's limit, so a document is sorted or dense
    for k in ("AHA_DOCCOUNT_SORT_MAX", "AHA_DOCCOUNT_DENSE_MIN", "AHA_DOCCOUNT_RANGE_KEYS", "AHA_DOCCOUNT_ROW_BYTES"):
        monkeypatch.delenv(k)
    m = AC.compile(keys)
    corpus, offs = _batch(_tier_batch(rng, NK, [4095, 4096, 4097, 3, 2049, 2048, 20000]))
    _check_all_entries(m, o, corpus, offs)


def test_doc_counts_in_document_ranges(monkeypatch):
    """the hit buffer's bound lowered: at least three ranges of whole documents, one document alone beyond the bound"""
    import torch

    monkeypatch.setenv("AHA_DOCCOUNT_HIT_BYTES", str(12 * 2000))
    rng = random.Random(9)
    keys = _keys_ascii(rng)
    m, o = AC.compile(keys), orc.AC.compile(keys)
    docs = _docs(rng, keys, 30, 2500, 0.5)
    docs[7] = b"".join(rng.choice(keys) for _ in range(8000))
    corpus, offs = _batch(docs)
    _, dho = _oracle_hits(o, corpus, offs)
    h = np.diff(dho.astype(np.int64))
    assert h[7] > 2000 and h.sum() - h[7] > 3 * 2000  # (from the oracle: one document beyond the bound, the rest three ranges)
    m.set_profiling(True)
    want, want_dpo = _check_all_entries(m, o, corpus, offs)
    ct = torch.from_numpy(corpus).to(DEV)
    ot = torch.from_numpy(offs.view(np.int64)).to(DEV)
    _device(m, ct, ot, offs.size - 1, want.size)
    t = m.last_timing()
    assert t["repeats"] >= 2 and t["n_hits"] == int(dho[-1]), t
    # capacity across ranges
    dp, ddpo, n, nh, rc = _device(m, ct, ot, offs.size - 1, want.size // 2)
    assert rc == N.AHA_E_CAPACITY and n == want.size and np.array_equal(ddpo, want_dpo)
    assert dp.tobytes() == want[: want.size // 2].tobytes()


def test_doc_counts_capacity_and_sizing():
    import torch

    rng = random.Random(21)
    keys = _keys_ascii(rng)
    m, o = AC.compile(keys), orc.AC.compile(keys)
    corpus, offs = _batch(_docs(rng, keys, 20, 3000, 0.6))
    want, want_dpo, want_n, _ = _want(o, corpus, offs)
    D = offs.size - 1
    ct = torch.from_numpy(corpus).to(DEV)
    ot = torch.from_numpy(offs.view(np.int64)).to(DEV)
    dp, dpo, n, nh, rc = _device(m, ct, ot, D, want.size - 1)
    assert rc == N.AHA_E_CAPACITY and n == want.size and nh == want_n
    assert np.array_equal(dpo, want_dpo) and dp.tobytes() == want[:-1].tobytes()
    dp, dpo, n, nh, rc = _device(m, ct, ot, D, want.size)
    assert rc == N.AHA_OK and n == want.size and dp.tobytes() == want.tobytes() and np.array_equal(dpo, want_dpo)
    # the sizing call: out == NULL, cap == 0
    with pytest.raises(AhaError) as e:
        m.doc_counts_batch_device(ct, ot, None)
    assert e.value.code == N.AHA_E_CAPACITY and e.value.n_required == want.size and e.value.n_hits == want_n
    import ctypes as C

    L = N.lib()
    n64 = C.c_uint64(0)
    dpo_h = np.zeros(D + 1, dtype=np.uint64)
    rc = L.aha_ac_doc_counts_batch(m._h, corpus.ctypes.data, offs.ctypes.data, D, None, None, 0, dpo_h.ctypes.data, C.byref(n64), None)
    assert rc == N.AHA_E_CAPACITY and n64.value == want.size and np.array_equal(dpo_h, want_dpo)
    # host entry with cap one short: the first cap pairs
    out = np.zeros(want.size, dtype=doccountsim.KEY_COUNT_DTYPE)
    rc = L.aha_ac_doc_counts_batch(m._h, corpus.ctypes.data, offs.ctypes.data, D, None, out.ctypes.data, want.size - 1,
                                   dpo_h.ctypes.data, C.byref(n64), None)
    assert rc == N.AHA_E_CAPACITY and n64.value == want.size and out[:-1].tobytes() == want[:-1].tobytes() and out[-1]["count"] == 0


def test_doc_counts_leave_no_trace_in_the_back_off(monkeypatch):
    """match -> doc counts -> match on a handle whose first match is handed back by the prefix-filter engine: every later
    match reports the engine and the repeats it reports on a twin handle that never saw the call in between."""
    monkeypatch.delenv("AHA_ENGINE", raising=False)
    dense = b"abcd" * 3000
    sparse = b"-" * 5000 + b"abcd"

    def run(with_doc_counts):
        m = AC.compile(["abc", "bcd"])
        assert m.info["filter_prefix_bytes"] == 3
        m.set_profiling(True)
        seen = []
        for text in [dense] + [sparse] * 6 + [dense] + [sparse] * 3:
            assert len(m.match_array(text)) == (6000 if text is dense else 2)
            t = m.last_timing()
            seen.append((t["engine"], t["repeats"]))
            if with_doc_counts:
                for t2 in (dense, sparse):
                    assert m.doc_counts(t2) == ({0: 3000, 1: 3000} if t2 is dense else {0: 1, 1: 1})
        m.release_scratch()
        assert m.scratch_bytes() == 0
        return seen

    plain = run(False)
    # the set-up: the first match backs off -- the sparse text behind it stays away from the filter (engine 2), later takes it
    assert plain[0][0] == 2 and plain[1][0] == 2 and plain[6][0] == 5, plain
    assert run(True) == plain


@pytest.mark.parametrize("cfg,n_bytes", [(3, 256 << 20), (5, 64 << 20)])
def test_doc_counts_at_size(cfg, n_bytes):
    """on the device: per-key sums = count_batch_device's key counts, per-document sums = its offsets' differences, keys
    ascending within every document; against the oracle: 32+ whole documents (most hits, fewest hits, a seeded sample)"""
    import torch

    blob, koffs, nf = synth.keys(cfg)
    corpus, doc = synth.corpus(cfg, blob, koffs, nf, n_bytes=n_bytes, doc_bytes=1 << 16)
    m = AC.compile_packed(blob, koffs)
    K, D = m.n_keys, doc.size - 1
    ct = torch.from_numpy(corpus).to(DEV)
    ot = torch.from_numpy(doc.astype(np.int64)).to(DEV)
    kc = torch.zeros(K, dtype=torch.int64, device=DEV)
    dho = torch.zeros(D + 1, dtype=torch.int64, device=DEV)
    n_hits = m.count_batch_device(ct, ot, kc, dho)
    with pytest.raises(AhaError) as e:
        m.doc_counts_batch_device(ct, ot, None)
    n = e.value.n_required
    out = torch.zeros((n, 2), dtype=torch.int32, device=DEV)
    dpo = torch.zeros(D + 1, dtype=torch.int64, device=DEV)
    assert m.doc_counts_batch_device(ct, ot, out, dpo) == (n, n_hits)
    key, cnt = out[:, 0].to(torch.int64), out[:, 1].to(torch.int64)
    assert int(dpo[0]) == 0 and int(dpo[-1]) == n and int(cnt.min()) > 0
    assert torch.equal(torch.zeros(K, dtype=torch.int64, device=DEV).index_add_(0, key, cnt), kc)
    docid = torch.searchsorted(dpo, torch.arange(n, device=DEV), right=True) - 1
    assert torch.equal(torch.zeros(D, dtype=torch.int64, device=DEV).index_add_(0, docid, cnt), dho[1:] - dho[:-1])
    asc = (key[1:] > key[:-1]) | (docid[1:] != docid[:-1])
    assert bool(asc.all())
    out2 = torch.zeros((n, 2), dtype=torch.int32, device=DEV)
    m.doc_counts_batch_device(ct, ot, out2, dpo)
    assert torch.equal(out, out2)  # deterministic
    # whole documents against the oracle
    h = (dho[1:] - dho[:-1]).cpu().numpy()
    rng = random.Random(cfg)
    pick = sorted({int(h.argmax()), int(h.argmin())} | set(rng.sample(range(D), 32)))
    assert len(pick) >= 32
    keys = [bytes(blob[koffs[i]:koffs[i + 1]]) for i in range(koffs.size - 1)]
    o = orc.AC.compile(keys)
    out_h, dpo_h = out.cpu().numpy(), dpo.cpu().numpy()
    for d in pick:
        hits = o.match(corpus[int(doc[d]):int(doc[d + 1])].tobytes(), chars=False)
        v = np.asarray(hits["value"], dtype=np.int64) if hits.size else np.zeros(0, np.int64)
        want, _ = doccountsim.doc_counts(v, [0, v.size])
        got = np.ascontiguousarray(out_h[dpo_h[d]:dpo_h[d + 1]]).view(doccountsim.KEY_COUNT_DTYPE).reshape(-1)
        assert got.tobytes() == want.tobytes(), f"document {d}"
