"""match_longest (src/aha/ac.cr:118-143, 297-319) on its own device path at the scales where it could go wrong: the wide
image, keys long enough to grow the chunk and its warm-up, batches with more than one scan tile of documents or chunks,
several host ranges, NUL bytes that the chunked form must find, and every entry that accepts `longest`.

The path is engine.cpp match_longest_pass (what device_match hands a `longest` call to): mode 1 (longest = 1) is a thread per document; mode 2
(longest = 2, byte offsets) a thread per chunk with a 2 * Lmax warm-up (k_longest_chunks); mode 3 (longest = 2 with char
offsets, or a mode-2 batch whose warm-ups give up at NULs) a thread per document again.  None of the engine variants of
test_gpu_parity.py applies, so nothing here runs under them.  Every case compares with the oracle's match_longest, one
document at a time, bit for bit: hit triples in order and per-document hit offsets.  Data and oracle answers are cached
at module scope (the oracle is single-threaded, ~30 MB/s for match_longest)."""
import random

import numpy as np
import pytest

import pyoracle as orc
from aha_amd import AC, AhaError, synth
from aha_amd import _native as N
from test_oracle_vs_model import rand_keys

pytestmark = pytest.mark.gpu

MiB = 1 << 20
HOST_RANGE = 64 * MiB     # capi.cpp kHostRange: the host entry's document ranges
SCAN_TILE = 1024 * 256    # k_scan_blocks: one tile holds the sums of 1024 blocks of kBlock = 256 units
NUL_BACK = 4096           # k_longest_chunks kNulBack: a warm-up walks back at most this far past a NUL
MODES = {1: (1, False), 2: (2, False), 3: (2, True)}  # mode -> (longest, chars); intersectable = longest == 2

_C = {}


def cached(key, make):
    if key not in _C:
        _C[key] = make()
    return _C[key]


def longest_chunk(L):
    """match_longest_pass's chunk: the first power of two >= max(1024, 16 L), at most 1 MiB.  The warm-up
    of a chunk is 2 L bytes."""
    c = 1024
    while c < 16 * L and c < MiB:
        c *= 2
    return c


def stale_paths_of(ac, keys):
    """The library's replay of Cedar's stale END flags (AHA_IMG_STALE_ENDS), as a set of byte strings."""
    a = ac.export(N.AHA_IMG_STALE_ENDS, np.uint32).reshape(-1, 2)
    return set(bytes(keys[int(k)][:int(n)]) for k, n in a)


def key_list(blob, offs):
    return [bytes(blob[int(offs[i]):int(offs[i + 1])]) for i in range(offs.size - 1)]


def oracle_docs(o, corpus, doc, mode, docs=None):
    """The oracle's answer per document (a list of hit arrays) for documents `docs` (default: all)."""
    longest, chars = MODES[mode]
    idx = range(doc.size - 1) if docs is None else docs
    return [o.match_longest(corpus[int(doc[d]):int(doc[d + 1])].tobytes(), longest == 2, chars=chars) for d in idx]


def joined(parts):
    """Per-document answers -> (hit bytes of the batch, per-document hit offsets)."""
    dho = np.zeros(len(parts) + 1, dtype=np.uint64)
    dho[1:] = np.cumsum([len(p) for p in parts])
    return b"".join(p.tobytes() for p in parts), dho


def first_diff(a, b):
    x, y = np.frombuffer(a, dtype=np.int32).reshape(-1, 3), np.frombuffer(b, dtype=np.int32).reshape(-1, 3)
    n = min(len(x), len(y))
    bad = np.flatnonzero((x[:n] != y[:n]).any(axis=1))
    i = int(bad[0]) if bad.size else n
    return i, len(x), len(y), x[i:i + 2].tolist(), y[i:i + 2].tolist()


def check_host(g, corpus, doc, mode, want):
    """The host entry (aha_ac_match_batch) against the oracle's answer `want` = joined(...)."""
    raw, dho = want
    longest, chars = MODES[mode]
    gh, gd = g.match_batch(corpus, doc, chars=chars, longest=longest, cap=len(raw) // 12 + 16)
    got = gh.tobytes()
    assert got == raw, (mode, first_diff(got, raw))
    assert np.array_equal(gd, dho), (mode, int(np.flatnonzero(gd != dho)[0]))


def run_device(g, dc, dd, cap, mode):
    """match_batch_device into exactly `cap` rows and D + 1 offsets, with guards behind both that must stay untouched.
    Returns (hit count or required count, error code or None, out rows, per-document offsets) as tensors."""
    import torch

    longest, chars = MODES[mode]
    D = dd.numel() - 1
    out = torch.full((cap + 64, 3), -7, dtype=torch.int32, device="cuda")
    dho = torch.full((D + 1 + 8,), -7, dtype=torch.int64, device="cuda")
    n, err = None, None
    try:
        n = g.match_batch_device(dc, dd, out[:cap], dho[:D + 1], chars=chars, longest=longest)
    except AhaError as e:
        n, err = getattr(e, "required", None), e.code
    assert bool((out[cap:] == -7).all()) and bool((dho[D + 1:] == -7).all()), mode
    return n, err, out[:cap], dho[:D + 1]


def check_device(g, dc, dd, mode, want):
    raw, od = want
    total = len(raw) // 12
    n, err, out, dho = run_device(g, dc, dd, total, mode)
    assert err is None and n == total, (mode, err, n, total)
    got = out.cpu().numpy().tobytes()
    assert got == raw, (mode, first_diff(got, raw))
    assert np.array_equal(dho.cpu().numpy().astype(np.uint64), od), mode


# ---- 1a: the wide image (k_longest_*<false, *>, stale and term bitmaps over 8-byte slots) ------------------------

def random_case(seed):
    """test_gpu_parity.py test_match_longest_random's generator: random keys over small alphabets, ragged documents,
    NULs now and then, densely, and (seed 0) behind every byte."""
    rng = random.Random(600 + seed)
    alphabet = [b"ab", b"abc", "abж中".encode(), bytes(range(0x61, 0x6B))][seed % 4]
    keys = rand_keys(rng, rng.randint(1, 80), alphabet, 1, [4, 9, 30][seed % 3])
    docs = [bytes(rng.choice(alphabet + b" ") for _ in range(rng.choice([0, 1, 2, 7, 100, 1023, 1024, 1025, 5000])))
            for _ in range(40)] + [bytes(rng.choice(alphabet) for _ in range(40000))] + \
           [bytes(rng.choice(alphabet + b"\x00") for _ in range(n)) for n in (3, 50, 3000, 30000)] + \
           [bytes(0 if rng.random() < 1 / 300 else rng.choice(alphabet) for _ in range(40000))]
    if seed == 0:
        docs.append(b"".join(bytes([rng.choice(alphabet), 0]) for _ in range(6000)))
    doc = np.cumsum([0] + [len(d) for d in docs]).astype(np.uint64)
    corpus = np.frombuffer(b"".join(docs), dtype=np.uint8)
    return keys, corpus, doc


@pytest.mark.parametrize("seed", range(6))
def test_random_key_sets_on_the_wide_image(seed):
    keys, corpus, doc = random_case(seed)
    g = AC.compile(keys, force_wide=True)
    assert g.info["slot_bytes"] == 8
    o = orc.AC.compile(keys)
    assert stale_paths_of(g, keys) == o.stale_paths()
    try:
        corpus.tobytes().decode("utf-8")
        utf8 = True
    except UnicodeDecodeError:
        utf8 = False
    for mode in (1, 2, 3):
        if MODES[mode][1] and not utf8:
            continue  # char offsets are defined for valid UTF-8 only
        check_host(g, corpus, doc, mode, joined(oracle_docs(o, corpus, doc, mode)))


def cfg_case(cfg):
    def make():
        blob, offs, nf = synth.keys(cfg)
        g = AC.compile_packed(blob, offs)
        o = orc.AC.compile_packed(blob, offs)
        corpus, doc = synth.corpus(cfg, blob, offs, nf, n_bytes=32 * MiB, doc_bytes=60 << 10)
        return key_list(blob, offs), g, o, corpus, doc
    return cached(("cfg", cfg), make)


@pytest.mark.parametrize("cfg,slot_bytes,n_stale", [(3, 4, 10_826), (5, 8, 108_504)])
def test_full_key_sets_compact_and_wide(cfg, slot_bytes, n_stale):
    """cfg 5's million keys get the wide image by size (8-byte slots); cfg 3's 100 000 keys stay compact: the control.
    Same stale set as the oracle's Cedar, then 32 MiB of their own text in documents of at most 64 KiB, all three modes."""
    keys, g, o, corpus, doc = cfg_case(cfg)
    assert g.info["slot_bytes"] == slot_bytes
    stale = o.stale_paths()
    assert len(stale) == n_stale and stale_paths_of(g, keys) == stale
    assert int(np.diff(doc.astype(np.int64)).max()) <= 64 << 10
    for mode in (1, 2, 3):
        check_host(g, corpus, doc, mode, joined(oracle_docs(o, corpus, doc, mode)))


# ---- 1b: long keys grow the chunk (2 KiB .. 1 MiB) and the warm-up (past kNulBack, past a whole chunk) -----------

LONG_LMAX = [64, 65, 200, 1500, 3000, 70_000, 600_000]


def split_long(cuts, protected, max_doc):
    """Cut every document longer than max_doc, never inside a protected interval [s, e)."""
    out = [cuts[0]]
    for b in cuts[1:]:
        while b - out[-1] > max_doc:
            q = out[-1] + max_doc
            for s, e in protected:
                if s < q < e:
                    q = s
            assert q > out[-1]
            out.append(q)
        out.append(b)
    return np.array(out, dtype=np.uint64)


def long_case(L):
    """Keys: nested prefixes of a few long random strings over 2 or 3 letters (pending ends stay pending over long runs
    of direct gotos), plus short keys.  Text: random over the same letters; at every odd chunk edge e a long string, or a
    copy cut short or changed near its end, planted at e - L + {0, 1, 2, 7} behind a 'z' (no goto anywhere: the root).
    Two document splits: `fine` (modes 1, 2, 3: cuts at even edges, on them or one byte to either side, empty documents
    at edges and at the tail, nothing longer than 1 MiB) and `coarse` (mode 2: documents of six chunks, whose warm-ups
    reach across whole chunks when 2 L > chunk)."""
    def make():
        rng = np.random.default_rng(L)
        alpha = np.frombuffer(b"ab" if L % 2 else b"abc", dtype=np.uint8)

        def rs(n):
            return alpha[rng.integers(0, alpha.size, n)].tobytes()

        longs = [rs(L), rs(L - 3), rs(max(L // 2, 8))]
        keys = set()
        for s in longs:
            n = len(s)
            lens = {n, n - 1, n - 2, n - 3, n - 7, n - 8} | {n >> k for k in range(1, 16)} | \
                   {int(x) for x in rng.integers(1, n, 8)}
            keys |= {s[:m] for m in lens if m > 0}
        keys |= {rs(int(m)) for m in rng.integers(1, 7, 40)}
        keys = sorted(keys)
        random.Random(L).shuffle(keys)
        C = longest_chunk(L)
        n_ch = 14 if C == MiB else 24
        n = n_ch * C + 333
        text = alpha[rng.integers(0, alpha.size, n)].copy()
        s0 = longs[0]

        def mutate(s, i):
            b = bytearray(s)
            b[i] = alpha[(alpha.tolist().index(b[i]) + 1) % alpha.size]
            return bytes(b)

        pieces = [s0, s0[:-1], s0[:-5], mutate(s0, L - 2), longs[1], mutate(s0, L - 9)]
        protected, fine, coarse = [], [0], [0]
        for i in range(1, n_ch):
            e = i * C
            if i % 2:
                k = (0, 1, 2, 7)[(i // 2) % 4]
                piece = pieces[(i // 2) % len(pieces)]
                at = e - L + k
                text[at - 1] = ord("z")
                text[at:at + len(piece)] = np.frombuffer(piece, dtype=np.uint8)
                protected.append((at - 1, at + len(piece) + 1))
            else:
                q = e + (0, -1, 1)[(i // 2) % 3]
                fine += [q] * (2 if (i // 2) % 4 == 1 else 1)  # an empty document now and then
                if i % 6 == 0:
                    coarse += [e, e] if i % 12 == 0 else [e]
        fine = split_long(fine + [n, n, n], protected, MiB)
        coarse = np.array(coarse + [n, n], dtype=np.uint64)
        g = AC.compile(keys)
        o = orc.AC.compile(keys)
        return dict(keys=keys, g=g, o=o, C=C, text=text, fine=fine, coarse=coarse)
    return cached(("long", L), make)


@pytest.mark.parametrize("L", LONG_LMAX)
def test_long_keys_grow_the_chunk_and_the_warm_up(L):
    c = long_case(L)
    g, o, text = c["g"], c["o"], c["text"]
    assert g.info["max_key_len"] == L
    assert c["C"] == {64: 1024, 65: 2048, 200: 4096, 1500: 32768, 3000: 65536}.get(L, MiB)
    fine, coarse = c["fine"], c["coarse"]
    assert int(np.diff(fine.astype(np.int64)).max()) <= MiB
    for mode in (1, 2, 3):
        check_host(g, text, fine, mode, joined(oracle_docs(o, text, fine, mode)))
    base = oracle_docs(o, text, coarse, 2)
    check_host(g, text, coarse, 2, joined(base))
    if L == 3000:  # 2 L = 6000 > kNulBack: one NUL per call, in mode 2 (the only mode that looks for NULs)
        C = c["C"]
        assert 2 * L > NUL_BACK
        for a, back in ((2 * C, 5000), (4 * C, 1000)):  # give up (per document) / walk back past the NUL
            assert a not in set(coarse.tolist())
            t = text.copy()
            t[a - back] = 0
            d = int(np.searchsorted(coarse, a - back, side="right")) - 1
            assert int(coarse[d]) < a - 2 * L
            parts = list(base)
            parts[d] = oracle_docs(o, t, coarse, 2, [d])[0]
            check_host(g, t, coarse, 2, joined(parts))
            assert int(np.diff(coarse.astype(np.int64)).max()) <= MiB  # (the give-up runs each document on one thread)


# ---- 1c: many documents, many chunks, several host ranges --------------------------------------------------------

def many_docs_case():
    def make():
        blob, offs, nf = synth.keys(3)
        corpus, _ = synth.corpus(3, blob, offs, nf, n_bytes=40 * MiB, doc_bytes=64 << 10)
        rng = np.random.default_rng(7)
        starts = np.flatnonzero((corpus & 0xC0) != 0x80)  # character starts: every document stays valid UTF-8
        cuts = rng.choice(starts, 300_000, replace=False)
        k1024 = np.arange(0, corpus.size, 1024)
        k1024 = k1024[(corpus[k1024] & 0xC0) != 0x80]  # documents that start on 1024-byte multiples
        ascii_ = starts[corpus[starts] < 0x80]
        one = rng.choice(ascii_, 5000, replace=False)  # 1-byte documents
        empty = rng.choice(starts, 2000, replace=False)  # runs of four empty documents
        doc = np.sort(np.concatenate([[0], cuts, k1024[::3], one, one + 1, np.repeat(empty, 4),
                                      [corpus.size] * 4])).astype(np.uint64)
        doc = doc[doc <= corpus.size]
        g = AC.compile_packed(blob, offs)
        o = orc.AC.compile_packed(blob, offs)
        return g, o, corpus, doc
    return cached("many", make)


def test_many_documents_in_one_host_range():
    """More than 1024 * 256 documents in one device call: the per-document kernels' block sums span two tiles of
    k_scan_blocks, whose carry joins them."""
    g, o, corpus, doc = many_docs_case()
    D = doc.size - 1
    assert D + 1 > SCAN_TILE and corpus.size < HOST_RANGE
    for mode in (1, 3):
        check_host(g, corpus, doc, mode, joined(oracle_docs(o, corpus, doc, mode)))


def big_case():
    def make():
        blob, offs, nf = synth.keys(3)
        corpus, doc = synth.corpus(3, blob, offs, nf, n_bytes=320 * MiB, doc_bytes=64 << 10)
        g = AC.compile_packed(blob, offs)
        o = orc.AC.compile_packed(blob, offs)
        h = int(np.searchsorted(doc, 200 * MiB))
        return dict(g=g, o=o, corpus=corpus, doc=doc, h=h)
    return cached("big", make)


def test_host_entry_over_several_ranges():
    """~200 MiB through the host entry: four ranges of ~64 MiB, whose hit lists and per-document offsets are stitched
    with the hits of the ranges before (match_batch_host, base[k])."""
    c = big_case()
    h = c["h"]
    doc = c["doc"][:h + 1]
    corpus = c["corpus"][:int(doc[-1])]
    assert corpus.size > 3 * HOST_RANGE
    for mode in (1, 2, 3):
        parts = cached(("big", mode), lambda: oracle_docs(c["o"], c["corpus"], c["doc"], mode, range(h)))
        check_host(c["g"], corpus, doc, mode, joined(parts))


def test_device_entry_with_more_chunks_than_a_scan_tile():
    """Mode 2 on 320 MiB in one device call: 1024-byte chunks (Lmax 24), so more than 1024 * 256 of them; documents
    that start on chunk multiples, empty documents at chunk edges and at the end."""
    import torch

    c = big_case()
    g, o, corpus = c["g"], c["o"], c["corpus"]
    assert longest_chunk(g.info["max_key_len"]) == 1024
    rng = np.random.default_rng(3)
    edges = np.arange(1024, corpus.size, 1024, dtype=np.uint64)
    doc = np.sort(np.concatenate([c["doc"], rng.choice(edges, 3000, replace=False),
                                  np.repeat(rng.choice(edges, 500, replace=False), 2),
                                  [corpus.size] * 2])).astype(np.uint64)
    assert (corpus.size + 1023) // 1024 > SCAN_TILE
    want = joined(oracle_docs(o, corpus, doc, 2))
    dc = torch.from_numpy(corpus).cuda()
    dd = torch.from_numpy(doc.astype(np.int64)).cuda()
    check_device(g, dc, dd, 2, want)


# ---- 1d: NUL detection at scale (k_has_nul) ----------------------------------------------------------------------

def nul_case():
    """cfg 2's keys and text (40 MiB + 7 bytes: 7 tail bytes behind the last 16-byte piece), plus keys over control bytes
    the text never holds: T5, T3, K1, K2 each end a key and have a child (a NUL behind them reaches the value node), K3
    does not.  Lmax = 41: chunks of 1024, warm-ups of 82 bytes."""
    def make():
        blob, offs, nf = synth.keys(2)
        n = 40 * MiB + 7
        corpus, doc = synth.corpus(2, blob, offs, nf, n_bytes=n, doc_bytes=64 << 10)
        assert not (corpus < 9).any()
        rng = np.random.default_rng(11)

        def ctl(k):
            return rng.integers(2, 8, k).astype(np.uint8).tobytes()

        T5, T3, K1, K2, K3 = ctl(5), ctl(3), ctl(40), ctl(40), ctl(41)
        keys = key_list(blob, offs) + [T5, T5 + b"\x08", T3, T3 + b"\x08", K1, K1 + b"\x08", K2, K2 + b"\x08", K3]
        g = AC.compile(keys)
        o = orc.AC.compile(keys)
        L = g.info["max_key_len"]
        assert L == 41 and longest_chunk(L) == 1024
        W = 2 * L

        def inside(a):  # a chunk start well inside a document
            d = int(np.searchsorted(doc, a, side="right")) - 1
            return int(doc[d]) < a - 300 and int(doc[d + 1]) > a + 300

        a1 = next(a for a in range(16 * MiB + 4096, n, 1024) if inside(a))
        a2 = next(a for a in range(a1 + 64 * 1024, n, 1024) if inside(a))
        p0 = a2 - W  # where a warm-up without the walk-back would start
        z1 = p0 + 30
        cases = {
            "byte 5": ([(0, T5)], [5]),
            "tail": ([(n - 6, T3)], [n - 3]),
            "warm-up": ([(a1 - 60, K1)], [a1 - 20]),
            # K1 begins in front of p0 and its NUL lies inside [p0, a2); K2 starts right behind that NUL and has one of
            # its own; K3 starts behind the second and ends past a2.  The state at the first NUL decides whether K2's
            # first byte is swallowed, hence whether the second NUL meets a key's end, hence whether K3 is matched.
            "chain": ([(z1 - 40, K1), (z1 + 1, K2), (a2 - 10, K3)], [z1, a2 - 11]),
        }
        base = oracle_docs(o, corpus, doc, 2)
        return dict(g=g, o=o, corpus=corpus, doc=doc, cases=cases, base=base, a2=a2, p0=p0)
    return cached("nul", make)


def _planted(c, name):
    plants, nuls = c["cases"][name]
    t = c["corpus"].copy()
    for at, piece in plants:
        t[at:at + len(piece)] = np.frombuffer(piece, dtype=np.uint8)
    t[nuls] = 0
    return t, nuls


def _doc_of(doc, q):
    return int(np.searchsorted(doc, q, side="right")) - 1


@pytest.mark.parametrize("case", ["byte 5", "tail", "warm-up", "chain"])
def test_nul_detection_at_scale(case):
    """One NUL per call (two for "chain"), right behind a key that ends a key and has children: at byte 5, in the last
    n % 16 bytes (the kernel's tail loop), past 16 MiB inside a chunk's warm-up window.  A single NUL cannot change what a
    2 * Lmax warm-up without the walk-back yields (the state it meets is exact, and its effect dies within Lmax bytes),
    so "chain" puts a second NUL where the first one's effect reaches: there the walk-back past the NULs is needed."""
    c = nul_case()
    g, o, doc = c["g"], c["o"], c["doc"]
    t, nuls = _planted(c, case)
    n = t.size
    assert int((t == 0).sum()) == len(nuls)
    if case == "tail":
        assert nuls[0] >= n - n % 16
    if case in ("warm-up", "chain"):
        a = nuls[0] + (20 if case == "warm-up" else 52)
        assert a % 1024 == 0 and a > 16 * MiB and a - 82 <= nuls[0] < a
    ds = sorted({_doc_of(doc, q) for q in nuls})
    assert len(ds) == 1
    d = ds[0]
    got = oracle_docs(o, t, doc, 2, [d])[0]
    t1 = t.copy()
    t1[nuls] = 1
    assert got.tobytes() != oracle_docs(o, t1, doc, 2, [d])[0].tobytes()  # the NUL is observable
    if case == "chain":  # ... and so is the walk-back: a warm-up from a2 - 2 Lmax alone owns other hits of chunk a2
        a2, p0, lo, hi = c["a2"], c["p0"], int(doc[d]), int(doc[d + 1])

        def own(h, base):
            e = base + h["end"].astype(np.int64) - 1
            m = (e >= a2) & (e < a2 + 1024)
            return list(zip(e[m].tolist(), h["value"][m].tolist()))

        short = o.match_longest(t[p0:hi].tobytes(), True, chars=False)
        assert own(got, lo) != own(short, p0)
    parts = list(c["base"])
    parts[d] = got
    check_host(g, t, doc, 2, joined(parts))


# ---- 1e: the device entry, replicated and loaded handles, a group -------------------------------------------------

def dev_case():
    def make():
        blob, offs, nf = synth.keys(3, K=20_000)
        corpus, doc = synth.corpus(3, blob, offs, nf, n_bytes=4 * MiB, doc_bytes=64 << 10)
        doc = np.concatenate([doc[:5], doc[4:], [corpus.size] * 2]).astype(np.uint64)  # empty documents
        g = AC.compile_packed(blob, offs)
        o = orc.AC.compile_packed(blob, offs)
        return g, o, corpus, doc
    return cached("dev", make)


def test_device_entry_guards_capacity_and_unaligned_views():
    import torch

    g, o, corpus, doc = dev_case()
    dc = torch.from_numpy(corpus).cuda()
    dd = torch.from_numpy(doc.astype(np.int64)).cuda()
    buf = torch.zeros(corpus.size + 1, dtype=torch.uint8, device="cuda")
    buf[1:] = dc
    view = buf[1:]  # a slice that starts at byte 1
    assert view.data_ptr() % 16 == 1
    for mode in (1, 2, 3):
        want = joined(oracle_docs(o, corpus, doc, mode))
        raw, od = want
        total = len(raw) // 12
        assert total > 1000
        check_device(g, dc, dd, mode, want)
        n, err, out, dho = run_device(g, dc, dd, total - 1, mode)  # one row short: nothing past cap
        assert err == N.AHA_E_CAPACITY and n == total, (mode, err, n)
        assert out.cpu().numpy().tobytes() == raw[:12 * (total - 1)]
        check_device(g, view, dd, mode, want)


def test_device_entry_rejects_bad_offsets_before_writing():
    """longest reads the offsets' verdict back before it starts (no deferred check): a bad batch writes no row and no
    offset."""
    import torch

    g, o, corpus, doc = dev_case()
    dc = torch.from_numpy(corpus).cuda()
    desc = doc.astype(np.int64).copy()
    desc[3], desc[7] = desc[7], desc[3]
    short = doc.astype(np.int64).copy()
    short[-1] -= 1
    huge = torch.empty((1 << 31) + 16, dtype=torch.uint8, device="cuda")  # (never read: the offsets are refused)
    cases = [(dc, desc, N.AHA_E_INVALID), (dc, short, N.AHA_E_INVALID),
             (huge, np.array([0, 16, (1 << 31) + 16], dtype=np.int64), N.AHA_E_TOO_LONG)]
    for corp, offs, code in cases:
        dd = torch.from_numpy(offs).cuda()
        for mode in (1, 2, 3):
            n, err, out, dho = run_device(g, corp, dd, 4096, mode)
            assert err == code, (mode, err, code)
            assert bool((out == -7).all()) and bool((dho == -7).all()), mode
    del huge


def test_longest_beyond_4_gib():
    """Mode 2 on a batch of 4 GiB + 1 MiB (uint64 corpus offsets in k_longest_chunks and k_has_nul): the documents on
    both sides of 2^32 and a sample of the others against the oracle; global invariants over all hits."""
    import torch

    blob, offs, nf = synth.keys(3)
    n_bytes = (1 << 32) + MiB
    corpus, doc = synth.corpus(3, blob, offs, nf, n_bytes=n_bytes)
    D = doc.size - 1
    assert int(doc[-1]) == n_bytes
    g = AC.compile_packed(blob, offs)
    dc = torch.from_numpy(corpus).cuda()
    dd = torch.from_numpy(doc.astype(np.int64)).cuda()
    dho = torch.zeros(D + 1, dtype=torch.int64, device="cuda")
    with pytest.raises(AhaError) as e:
        g.match_batch_device(dc, dd, torch.zeros((1, 3), dtype=torch.int32, device="cuda"), dho, longest=2)
    assert e.value.code == N.AHA_E_CAPACITY
    n = e.value.required
    out = torch.zeros((n + 16, 3), dtype=torch.int32, device="cuda")
    assert g.match_batch_device(dc, dd, out, dho, longest=2) == n
    del dc
    offsets = dho.cpu().numpy()
    assert offsets[0] == 0 and offsets[-1] == n and np.all(np.diff(offsets) >= 0)
    hits = out[:n].cpu().numpy()
    del out
    key_len = np.diff(offs.astype(np.int64))
    assert np.array_equal(hits[:, 1] - hits[:, 0], key_len[hits[:, 2]])
    doc_len = np.diff(doc.astype(np.int64))
    doc_of_hit = np.repeat(np.arange(D), np.diff(offsets))
    assert np.all(hits[:, 0] >= 0) and np.all(hits[:, 1].astype(np.int64) <= doc_len[doc_of_hit])
    assert np.all((np.diff(hits[:, 1]) > 0) | (np.diff(doc_of_hit) > 0))  # one hit per end, in order, per document
    o = orc.AC.compile_packed(blob, offs)
    cross = int(np.searchsorted(doc, 1 << 32, side="right")) - 1
    rng = np.random.default_rng(4)
    for d in sorted(set([0, cross - 1, cross, min(cross + 1, D - 1), D - 1] + [int(x) for x in rng.integers(0, D, 4)])):
        want = oracle_docs(o, corpus, doc, 2, [d])[0]
        assert hits[offsets[d]:offsets[d + 1]].tobytes() == want.tobytes(), d


def test_replicated_and_loaded_handles():
    """ensure_stale builds the stale and term bitmaps per handle on first use: on a replica made before and after the
    source's first longest call, and on a handle loaded from the saved image."""
    blob, offs, nf = synth.keys(2)
    keys = key_list(blob, offs)
    corpus, doc = synth.corpus(2, blob, offs, nf, n_bytes=2 * MiB, doc_bytes=32 << 10)
    o = orc.AC.compile_packed(blob, offs)
    stale = o.stale_paths()
    assert len(stale) == 121
    want = {mode: joined(oracle_docs(o, corpus, doc, mode)) for mode in (1, 2, 3)}
    src = AC.compile_packed(blob, offs)
    early = src.replicate(0)
    loaded = AC.from_bytes(src.to_bytes())
    check_host(src, corpus, doc, 2, want[2])
    late = src.replicate(0)
    for h in (early, late, loaded):
        for mode in (1, 2, 3):
            check_host(h, corpus, doc, mode, want[mode])
        assert stale_paths_of(h, keys) == stale


@pytest.mark.parametrize("transport", ["copies", "self-rccl"])
def test_group_of_shards_with_longest(transport, monkeypatch):
    """aha_group_match_batch with longest: three shards on cuda:0, the exchange rebuilds each hit's start from its end
    and the key's length (bytes or chars), every shard holds the whole ordered stream."""
    from aha_amd import ACGroup

    if transport == "self-rccl":
        monkeypatch.setenv("AHA_GROUP_RCCL", "self")
    else:
        monkeypatch.delenv("AHA_GROUP_RCCL", raising=False)
    blob, offs, nf = synth.keys(3, K=20_000)
    corpus, doc = cached("group data", lambda: synth.corpus(3, blob, offs, nf, n_bytes=1 << 23, doc_bytes=1 << 16))
    o = cached("group oracle", lambda: orc.AC.compile_packed(blob, offs))
    grp = ACGroup.compile_packed(blob, offs, [0, 0, 0])
    for mode in (2, 3, 1):
        longest, chars = MODES[mode]
        raw, od = cached(("group", mode), lambda: joined(oracle_docs(o, corpus, doc, mode)))
        gh, gd = grp.match_batch(corpus, doc, chars=chars, cap=16, longest=longest)  # too small first: the capacity protocol
        assert gh.tobytes() == raw, (mode, first_diff(gh.tobytes(), raw))
        assert np.array_equal(gd, od), mode
        for shard in range(3):
            assert grp.download_shard(shard).tobytes() == raw, (mode, shard)
