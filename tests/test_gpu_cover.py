"""Cover calls (aha_ac_cover_batch, aha_ac_cover_batch_device) against coversim over the CPU ORACLE's hits (never the library's
own match): key sets with and without a separator filter, every engine variant, edge sizes, long spans, NULL outputs,
redaction in place, document ranges, neutrality towards the handle's back-off state, the scratch bound that separates the
design from one with a hit list, and the configs at size."""
import os
import random
import threading
import zlib

import numpy as np
import pytest

import coversim
import pyoracle as orc
from aha_amd import AC, BitArray, DeviceCorpus, synth
from engine_variants import VARIANTS, use_variant
from test_gpu_doc_counts import KEYSETS, SEP_BITS, _batch, _docs, _keys_ascii, _keys_nested, _keys_utf8, _sep

pytestmark = pytest.mark.gpu

GUARD = 0x5A5A5A5A
PAD = 16
DEV = "cuda:0"
SEP_PAIR = (40, [i for i in range(40) if i not in SEP_BITS])


def _want(o, corpus, offs, sep_pair=None, fill=0x2A):
    """coversim over the oracle's hits -> (mask, redacted, doc_covered, n_covered, n_hits)"""
    parts, dho = [], [0]
    for d in range(offs.size - 1):
        h = o.match(corpus[int(offs[d]):int(offs[d + 1])].tobytes(), chars=False, sep=sep_pair)
        parts.append(h)
        dho.append(dho[-1] + h.size)
    s = np.concatenate([p["start"] for p in parts]).astype(np.int64) if parts else np.zeros(0, np.int64)
    e = np.concatenate([p["end"] for p in parts]).astype(np.int64) if parts else np.zeros(0, np.int64)
    mask, red, dc, nc = coversim.cover_all(s, e, corpus, offs, dho, fill)
    coversim.check_invariants(mask, red, dc, nc, corpus, offs, s, e, dho, fill)
    return mask, red, dc, nc, dho[-1]


def _tensors(corpus, offs, shift=0):
    import torch

    buf = torch.zeros(corpus.size + shift + 16, dtype=torch.uint8, device=DEV)
    ct = buf[shift:shift + corpus.size]
    if corpus.size:
        ct.copy_(torch.from_numpy(corpus))
    return ct, torch.from_numpy(offs.view(np.int64)).to(DEV)


def _device(m, ct, ot, sep=None, fill=0x2A, want_mask=True, want_red=True, want_cov=True, in_place=False):
    """the device entry with guard words behind ceil(N / 32) mask words, N redacted bytes and D counts
    -> (mask, redacted, doc_covered, n_covered, n_hits), None where not asked for"""
    import torch

    n, D = ct.numel(), ot.numel() - 1
    nw = (n + 31) // 32
    mask = torch.full((nw + PAD,), GUARD, dtype=torch.int32, device=DEV) if want_mask else None
    red = None
    if want_red:
        red = torch.full((n + PAD,), 0x5A, dtype=torch.uint8, device=DEV)
        if in_place:
            red[:n] = ct
    cov = torch.full((D + PAD,), GUARD, dtype=torch.int64, device=DEV) if want_cov else None
    src = red[:n] if (want_red and in_place) else ct
    nc, nh = m.cover_batch_device(src, ot, mask=mask, redacted=red[:n] if want_red else None, fill=fill,
                                  doc_covered=cov[:D] if want_cov else None, sep=sep)
    torch.cuda.synchronize()
    out = [None, None, None, nc, nh]
    if want_mask:
        h = mask.cpu().numpy()
        assert (h[nw:] == GUARD).all(), "the call wrote behind ceil(N / 32) mask words"
        out[0] = h[:nw].view(np.uint32).copy()
    if want_red:
        h = red.cpu().numpy()
        assert (h[n:] == 0x5A).all(), "the call wrote behind N redacted bytes"
        out[1] = h[:n].copy()
    if want_cov:
        h = cov.cpu().numpy()
        assert (h[D:] == GUARD).all(), "the call wrote behind D counts"
        out[2] = h[:D].astype(np.uint64)
    return out


def _check_all_entries(m, o, corpus, offs, sep_pair=None, sep=None, fill=0x2A):
    """host entry, device entry, cover_corpus: identical bytes, equal to coversim over the oracle's hits"""
    wm, wr, wc, wn, wh = _want(o, corpus, offs, sep_pair, fill)
    mask, cov = m.cover_batch(corpus, offs, sep=sep)
    assert mask.tobytes() == wm.tobytes() and np.array_equal(cov, wc)
    red, cov = m.redact_batch(corpus, offs, fill=fill, sep=sep)
    assert red.tobytes() == wr.tobytes() and np.array_equal(cov, wc)
    ct, ot = _tensors(corpus, offs)
    before = ct.clone()
    dm, dr, dc, nc, nh = _device(m, ct, ot, sep=sep, fill=fill)
    assert (nc, nh) == (wn, wh)
    assert dm.tobytes() == wm.tobytes() and dr.tobytes() == wr.tobytes() and np.array_equal(dc, wc)
    assert bool((ct == before).all()), "the corpus was changed"
    if offs.size > 1:
        cm, cr, cc, cn, ch = m.cover_corpus(DeviceCorpus(corpus, offs), sep=sep, redacted=True, fill=fill)
        assert cm.tobytes() == wm.tobytes() and cr.tobytes() == wr.tobytes() and np.array_equal(cc, wc) and (cn, ch) == (wn, wh)
    return wm, wr, wc, wn, wh


def test_cover_reference_kat_and_one_sequence():
    m = AC.compile(["我", "我是", "是中"])
    assert m.redact("我是中国人") == "***国人"
    assert AC.compile(["我是"]).redact("我是中国人") == "**中国人"
    m = AC.compile(["he", "she", "his", "hers"])
    assert m.redact(b"ushers") == b"u*****" and m.redact("ushers", fill="#") == "u#####"
    assert m.cover("ushers").tolist() == [False, True, True, True, True, True]
    assert m.redact(b"") == b"" and m.redact("") == "" and m.cover(b"").size == 0


@pytest.mark.parametrize("keyset", sorted(KEYSETS))
def test_cover_key_sets_with_and_without_separator(keyset):
    rng = random.Random(zlib.crc32(f"cv/{keyset}".encode()))
    keys = KEYSETS[keyset](rng)
    m, o = AC.compile(keys), orc.AC.compile(keys)
    for n_docs, size, density in ((7, 300, 0.3), (40, 2000, 0.6), (3, 70000, 0.9)):
        corpus, offs = _batch(_docs(rng, keys, n_docs, size, density))
        wm, *_ = _check_all_entries(m, o, corpus, offs)
        assert wm.any()
        _check_all_entries(m, o, corpus, offs, SEP_PAIR, _sep(), fill=0)


def test_cover_chars_gives_the_same_bytes():
    import ctypes as C
    from aha_amd import _native as N

    rng = random.Random(3)
    keys = _keys_utf8(rng)
    m, o = AC.compile(keys), orc.AC.compile(keys)
    corpus, offs = _batch(_docs(rng, keys, 9, 2000, 0.6))
    wm, wr, wc, wn, wh = _want(o, corpus, offs)
    p = N.aha_match_params()
    p.struct_size = C.sizeof(N.aha_match_params)
    p.char_offsets = 1
    mask = np.zeros(wm.size, dtype=np.uint32)
    red = np.zeros(corpus.size, dtype=np.uint8)
    cov = np.zeros(offs.size - 1, dtype=np.uint64)
    nc, nh = C.c_uint64(0), C.c_uint64(0)
    rc = N.lib().aha_ac_cover_batch(m._h, corpus.ctypes.data, offs.ctypes.data, offs.size - 1, C.byref(p), 0, mask.ctypes.data,
                                    red.ctypes.data, 0x2A, cov.ctypes.data, C.byref(nc), C.byref(nh))
    assert rc == 0 and (nc.value, nh.value) == (wn, wh)
    assert mask.tobytes() == wm.tobytes() and red.tobytes() == wr.tobytes() and np.array_equal(cov, wc)


@pytest.fixture(params=VARIANTS)
def variant(request, monkeypatch):
    return use_variant(request.param, monkeypatch)


def test_cover_every_engine_variant(variant):
    """one ragged batch on every engine variant (the variables are read when the handle is compiled)"""
    rng = random.Random(zlib.crc32(f"cvv/{variant}".encode()))
    keys = _keys_utf8(rng) if variant in ("u", "ur", "u23", "uh", "k", "p") else _keys_ascii(rng)
    m, o = AC.compile(keys), orc.AC.compile(keys)
    docs = _docs(rng, keys, 24, 3000, 0.6) + [b"".join(rng.choice(keys) for _ in range(4000))] + [b"q"] * 5
    corpus, offs = _batch(docs)
    wm, *_ = _check_all_entries(m, o, corpus, offs)
    assert wm.any()
    corpus, offs = _batch(_docs(rng, _keys_nested(rng), 12, 5000, 0.8))  # (this key set's text: few hits, many documents cut)
    _check_all_entries(m, o, corpus, offs)


@pytest.mark.parametrize("kind,engine", [("utf8", 4), ("ascii", 5), ("bytes", 2)])
def test_cover_takes_the_engine_of_the_match(kind, engine, monkeypatch):
    """the library's own choice: character-level (4), keyword list behind the prefix filter (5), byte-level (2)"""
    monkeypatch.delenv("AHA_ENGINE", raising=False)
    rng = random.Random(11)
    # ("bytes": the nested set's ASCII keys -- no multi-byte character, so no character-level image, and keys below three
    # bytes, so no prefix filter)
    keys = [k for k in _keys_nested(rng) if k.isascii()] if kind == "bytes" else KEYSETS[kind](rng)
    m, o = AC.compile(keys), orc.AC.compile(keys)
    m.set_profiling(True)
    if kind == "ascii":
        docs = [(b"-" * 400 + rng.choice(keys)) * 40 for _ in range(8)]  # (sparse: the prefix filter keeps the batch)
    else:
        docs = _docs(rng, keys, 8, 20000, 0.5)
    corpus, offs = _batch(docs)
    wm, wr, wc, wn, wh = _want(o, corpus, offs)
    ct, ot = _tensors(corpus, offs)
    dm, dr, dc, nc, nh = _device(m, ct, ot)
    t = m.last_timing()
    assert t["engine"] == engine and t["n_hits"] == wh, t
    assert dm.tobytes() == wm.tobytes() and dr.tobytes() == wr.tobytes() and np.array_equal(dc, wc)


@pytest.mark.parametrize("n", [0, 1, 31, 32, 33, 4097])
def test_cover_edge_sizes(n):
    keys = [b"a", b"ab", b"bab", b"q" * 40]
    m, o = AC.compile(keys), orc.AC.compile(keys)
    rng = random.Random(n)
    text = bytes(rng.choice(b"abq-") for _ in range(n))
    corpus, offs = _batch([text])
    _check_all_entries(m, o, corpus, offs)
    _check_all_entries(m, o, corpus, offs, SEP_PAIR, _sep())


def test_cover_empty_documents_single_bytes_and_boundaries():
    keys = [b"ab", b"abc", b"c", b"xyz" * 5]
    m, o = AC.compile(keys), orc.AC.compile(keys)
    _check_all_entries(m, o, np.zeros(0, dtype=np.uint8), np.array([0], dtype=np.uint64))  # D = 0
    _check_all_entries(m, o, np.zeros(0, dtype=np.uint8), np.array([0, 0, 0, 0], dtype=np.uint64))
    for docs in ([b"", b"", b"abcabc", b"", b"", b"xabc", b"", b""],
                 [b"a", b"b", b"c", b"a", b"b", b"c"] * 50,  # documents of one byte
                 [b"xa", b"bc"],  # a key split across a boundary: only "c" is covered
                 [b"xyz" * 4 + b"xy", b"z" + b"xyz" * 4]):
        corpus, offs = _batch(docs)
        _check_all_entries(m, o, corpus, offs)
    corpus, offs = _batch([b"xa", b"b"])
    mask, cov = m.cover_batch(corpus, offs)
    assert not mask.any() and not cov.any()


def test_cover_unaligned_device_corpus():
    rng = random.Random(15)
    keys = _keys_ascii(rng)
    m, o = AC.compile(keys), orc.AC.compile(keys)
    corpus, offs = _batch(_docs(rng, keys, 10, 3000, 0.6))
    wm, wr, wc, wn, wh = _want(o, corpus, offs)
    for shift in range(1, 16):
        ct, ot = _tensors(corpus, offs, shift)
        assert ct.data_ptr() % 16 == shift
        dm, dr, dc, nc, nh = _device(m, ct, ot)
        assert dm.tobytes() == wm.tobytes() and dr.tobytes() == wr.tobytes() and np.array_equal(dc, wc) and (nc, nh) == (wn, wh)
        _, ip, _, _, _ = _device(m, ct, ot, in_place=True, want_mask=False, want_cov=False)
        assert ip.tobytes() == wr.tobytes()


@pytest.mark.parametrize("klen,engine", [(3000, None), (5000, 1)])
def test_cover_long_spans(klen, engine, monkeypatch):
    """a key of 3000 bytes (region engines: its span crosses many words and chunks) and of 5000 (the two-pass engine), each
    ending in the first bytes of a chunk and of a document"""
    monkeypatch.delenv("AHA_ENGINE", raising=False)
    rng = random.Random(klen)
    long_key = bytes(rng.choice(b"lmnop") for _ in range(klen))
    keys = [long_key, long_key[-7:], b"zz"]
    m, o = AC.compile(keys), orc.AC.compile(keys)
    m.set_profiling(True)
    docs = []
    for lead in (0, 1, 2, 63, 64, 65, 191, 192, 193, 4095, 4096 - klen % 4096, 8192 - klen % 8192 + 1):
        docs.append(b"-" * lead + long_key + b"-" * rng.randrange(3))
    docs += [long_key, long_key[1:], long_key + long_key, b"zz" + long_key[:-1]]
    corpus, offs = _batch(docs)
    wm, *_ = _check_all_entries(m, o, corpus, offs)
    assert wm.any()
    if engine:
        assert m.last_timing()["engine"] == engine


def test_cover_null_outputs_in_place_and_fill():
    rng = random.Random(17)
    keys = _keys_ascii(rng)
    m, o = AC.compile(keys), orc.AC.compile(keys)
    corpus, offs = _batch(_docs(rng, keys, 12, 3000, 0.6))
    ct, ot = _tensors(corpus, offs)
    for fill in (0, 255, 0x2A):
        wm, wr, wc, wn, wh = _want(o, corpus, offs, fill=fill)
        for a in (False, True):
            for b in (False, True):
                for c in (False, True):
                    dm, dr, dc, nc, nh = _device(m, ct, ot, fill=fill, want_mask=a, want_red=b, want_cov=c)
                    assert (nc, nh) == (wn, wh)
                    assert dm is None or dm.tobytes() == wm.tobytes()
                    assert dr is None or dr.tobytes() == wr.tobytes()
                    assert dc is None or np.array_equal(dc, wc)
        _, ip, _, nc, _ = _device(m, ct, ot, fill=fill, in_place=True, want_mask=False, want_cov=False)
        assert ip.tobytes() == wr.tobytes() and nc == wn


def test_cover_in_document_ranges(monkeypatch):
    """the bound of the event regions lowered: the batch goes through ranges of whole documents that share mask words"""
    monkeypatch.setenv("AHA_COUNT_REGION_BYTES", str(96 << 10))
    monkeypatch.delenv("AHA_ENGINE", raising=False)
    for kind in ("ascii", "utf8", "nested"):
        rng = random.Random(kind)
        keys = KEYSETS[kind](rng)
        m, o = AC.compile(keys), orc.AC.compile(keys)
        m.set_profiling(True)
        corpus, offs = _batch(_docs(rng, keys, 30, 2501, 0.5))
        assert (np.diff(offs.astype(np.int64)) % 32 != 0).any()
        _check_all_entries(m, o, corpus, offs)
        ct, ot = _tensors(corpus, offs)
        _device(m, ct, ot)
        assert m.last_timing()["repeats"] > 0, m.last_timing()


def test_cover_leaves_no_trace_and_is_deterministic(monkeypatch):
    """match, cover, match on one handle: the second match as the first, in hits and in engine / repeats -- on a handle whose
    first match is handed back by the prefix-filter engine; two cover calls give identical bytes"""
    monkeypatch.delenv("AHA_ENGINE", raising=False)
    dense = b"abcd" * 3000
    sparse = b"-" * 5000 + b"abcd"

    def run(with_cover):
        m = AC.compile(["abc", "bcd"])
        assert m.info["filter_prefix_bytes"] == 3
        m.set_profiling(True)
        seen = []
        for text in [dense] + [sparse] * 6 + [dense] + [sparse] * 3:
            hits = m.match_array(text)
            assert len(hits) == (6000 if text is dense else 2)
            t = m.last_timing()
            seen.append((t["engine"], t["repeats"], np.asarray(hits).tobytes()))
            if with_cover:
                for t2 in (dense, sparse):
                    a, b = m.redact(t2), m.redact(t2)
                    assert a == b == (b"*" * 12000 if t2 is dense else b"-" * 5000 + b"****")
        m.release_scratch()
        assert m.scratch_bytes() == 0
        return seen

    plain = run(False)
    assert plain[0][0] == 2 and plain[1][0] == 2 and plain[6][0] == 5, [p[:2] for p in plain]
    assert run(True) == plain


def test_cover_eight_threads_on_one_handle():
    rng = random.Random(23)
    keys = _keys_ascii(rng)
    m, o = AC.compile(keys), orc.AC.compile(keys)
    batches = [_batch(_docs(rng, keys, 10, 3000, 0.6)) for _ in range(8)]
    wants = [_want(o, c, f) for c, f in batches]
    errs = []

    def work(i):
        try:
            for _ in range(3):
                mask, cov = m.cover_batch(*batches[i])
                red, _ = m.redact_batch(*batches[i])
                assert mask.tobytes() == wants[i][0].tobytes() and np.array_equal(cov, wants[i][2])
                assert red.tobytes() == wants[i][1].tobytes()
        except BaseException as e:  # noqa: BLE001
            errs.append((i, repr(e)))

    ts = [threading.Thread(target=work, args=(i,)) for i in range(8)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    assert not errs, errs


def test_cover_holds_no_hit_list():
    """all-'a' text under the nested key set: about 23 hits per byte.  The scratch of a cover call stays within the count call's
    + N + 1 MiB; a match of the batch needs 16 bytes per hit of capacity -- over 256 N."""
    import torch

    n = 4 << 20
    keys = _keys_nested(random.Random(0))
    corpus = np.full(n, ord("a"), dtype=np.uint8)
    offs = np.array([0, n], dtype=np.uint64)
    o = orc.AC.compile(keys)
    sample = o.match(b"a" * 4096, chars=False)
    assert sample.size / 4096 >= 16
    ct, ot = _tensors(corpus, offs)
    mc = AC.compile(keys)
    n_hits = mc.count_batch_device(ct, ot)
    assert n_hits >= 16 * n
    count_scratch = mc.scratch_bytes()
    mv = AC.compile(keys)
    nc, nh = mv.cover_batch_device(ct, ot)  # (no mask of the caller's: the N / 8 bytes are scratch too)
    assert (nc, nh) == (n, n_hits)
    assert mv.scratch_bytes() <= count_scratch + n + (1 << 20), (mv.scratch_bytes(), count_scratch)
    red = torch.empty_like(ct)
    mv.cover_batch_device(ct, ot, redacted=red)
    assert bool((red == 0x2A).all())
    assert mv.scratch_bytes() <= count_scratch + n + (1 << 20)


def _at_size(cfg, n_bytes):
    """device-side properties (coversim.check_invariants' with torch), then whole documents against the oracle"""
    import torch

    blob, koffs, nf = synth.keys(cfg)
    corpus, doc = synth.corpus(cfg, blob, koffs, nf, n_bytes=n_bytes, doc_bytes=1 << 16)
    m = AC.compile_packed(blob, koffs)
    D, n = doc.size - 1, corpus.size
    nw = (n + 31) // 32
    ct = torch.from_numpy(corpus).to(DEV)
    ot = torch.from_numpy(doc.astype(np.int64)).to(DEV)
    dho = torch.zeros(D + 1, dtype=torch.int64, device=DEV)
    n_hits = m.count_batch_device(ct, ot, None, dho)
    mask = torch.full((nw + PAD,), GUARD, dtype=torch.int32, device=DEV)
    red = torch.full((n + PAD,), 0x5A, dtype=torch.uint8, device=DEV)
    cov = torch.full((D + PAD,), GUARD, dtype=torch.int64, device=DEV)
    nc, nh = m.cover_batch_device(ct, ot, mask=mask, redacted=red[:n], fill=0x2A, doc_covered=cov[:D])
    assert nh == n_hits
    assert bool((mask[nw:] == GUARD).all()) and bool((red[n:] == 0x5A).all()) and bool((cov[D:] == GUARD).all())
    shifts = torch.arange(32, device=DEV, dtype=torch.int32)
    pop = 0
    bits = torch.empty(n, dtype=torch.bool, device=DEV)
    step = 1 << 22  # words at a time
    for w0 in range(0, nw, step):
        w = mask[w0:min(w0 + step, nw)]
        b = ((w[:, None] >> shifts[None, :]) & 1).to(torch.bool).reshape(-1)
        lo, hi = w0 * 32, min((w0 + w.numel()) * 32, n)
        assert not bool(b[hi - lo:].any()), "a bit behind the batch is set"
        bits[lo:hi] = b[:hi - lo]
        pop += int(b.sum())
    assert pop == nc == int(cov[:D].sum())
    assert bool((red[:n][bits] == 0x2A).all()) and torch.equal(red[:n][~bits], ct[~bits])
    h = dho[1:] - dho[:-1]
    assert not bool(cov[:D][h == 0].any()) and nc <= n
    mask2 = torch.zeros(nw, dtype=torch.int32, device=DEV)
    assert m.cover_batch_device(ct, ot, mask=mask2) == (nc, nh) and torch.equal(mask2, mask[:nw])  # deterministic
    # whole documents against the oracle
    hh = h.cpu().numpy()
    rng = random.Random(cfg)
    pick = sorted({int(hh.argmax()), int(hh.argmin()), 0, D - 1} | set(rng.sample(range(D), 32)))
    keys = [bytes(blob[koffs[i]:koffs[i + 1]]) for i in range(koffs.size - 1)]
    o = orc.AC.compile(keys)
    bits_h, cov_h = bits.cpu().numpy(), cov[:D].cpu().numpy()
    for d in pick:
        a, b = int(doc[d]), int(doc[d + 1])
        hits = o.match(corpus[a:b].tobytes(), chars=False)
        want = coversim.byte_cover(hits["start"], hits["end"], [0, b - a], [0, hits.size])
        assert np.array_equal(bits_h[a:b], want), f"document {d}"
        assert cov_h[d] == want.sum()


def test_cover_at_size_cfg2():
    _at_size(2, 64 << 20)


def test_cover_at_size_cfg3():
    _at_size(3, 1 << 30)


def test_cover_at_size_cfg5():
    _at_size(5, 256 << 20)
