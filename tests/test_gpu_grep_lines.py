"""grep's context lines (aha_ac_grep_batch* with AHA_GREP_LINES) bit-exact against greplinesim (the brute-force definition) over
the CPU ORACLE's hits per record (never the library's own match), through the device entry -- with guard words around every
buffer -- and the host entry.  Contexts from 0 to 0x7FFFFFFF around word (32), 256-record and rank-block (2048) edges; every D
around those edges; match patterns with and without invert; groups of every awkward kind, the doc_rec_offsets of a records call
among them; bad group offsets; the identities; empty records; engines and options; alignment; capacity; one-block grids; one
handle through a sequence of calls that share scratch.  Every case is a few thousand records of 1 to 8 bytes."""
import ctypes as C
import random
import zlib

import numpy as np
import pytest

import greplinesim as sim
import pyoracle as orc
from aha_amd import AC, AhaError
from aha_amd import _native as N
from aha_amd.ac import _params
from test_gpu_doc_counts import KEYSETS, SEP_BITS, _batch, _sep

pytestmark = pytest.mark.gpu

GUARD8 = 0x5A
GUARD64 = 0x5A5A5A5A5A5A5A5A
PAD = 16
DEV = "cuda:0"
MAXC = 0x7FFFFFFF
SEP_PAIR = (40, [i for i in range(40) if i not in SEP_BITS])
CONTEXTS = [0, 1, 2, 31, 32, 33, 2047, 2048, 2049, MAXC]


def _tensors(corpus, offs, shift=0):
    import torch

    buf = torch.zeros(corpus.size + shift + 16, dtype=torch.uint8, device=DEV)
    ct = buf[shift:shift + corpus.size]
    if corpus.size:
        ct.copy_(torch.from_numpy(np.ascontiguousarray(corpus)))
    return ct, torch.from_numpy(np.asarray(offs, dtype=np.uint64).view(np.int64)).to(DEV)


def _groups_tensor(groups):
    import torch

    if groups is None or len(groups) < 2:  # (G = 0 goes as NULL)
        return None
    return torch.from_numpy(np.asarray(groups, dtype=np.uint64).view(np.int64)).to(DEV)


def _hits(o, corpus, offs, sep_pair=None):
    """the oracle's hits per record -> (int64[D], n_hits)"""
    D = len(offs) - 1
    if D == 0:
        return np.zeros(0, dtype=np.int64), 0
    if sep_pair is None:
        _, dho = o.match_batch(corpus, np.asarray(offs, dtype=np.uint64))
        dho = np.asarray(dho).astype(np.int64)
        return np.diff(dho), int(dho[-1])
    text = np.asarray(corpus, dtype=np.uint8).tobytes()
    h = np.array([o.match(text[int(offs[d]):int(offs[d + 1])], chars=False, sep=sep_pair).size for d in range(D)], dtype=np.int64)
    return h, int(h.sum())


def _device(m, ct, ot, cap, cap_bytes, invert, before, after, gt=None, sep=None, ids=True, text=True, flags=True):
    """the device entry, raw, with guard words around every buffer -> (kept, doo, out, is_match, n_kept, n_bytes, n_hits, rc);
    after a failing call every buffer is still all guard"""
    import torch

    kept = torch.full((cap + PAD,), GUARD64, dtype=torch.int64, device=DEV)
    doo = torch.full((cap + 1 + PAD,), GUARD64, dtype=torch.int64, device=DEV)
    big = torch.full((cap_bytes + 2 * PAD,), GUARD8, dtype=torch.uint8, device=DEV)
    fl = torch.full((cap + 2 * PAD,), GUARD8, dtype=torch.uint8, device=DEV)
    flags = flags and cap > 0  # (is_match with cap_docs == 0 is refused)
    lp = N.aha_grep_lines_params()
    lp.match = _params(False, sep)
    lp.match.struct_size = C.sizeof(N.aha_grep_lines_params)
    lp.before, lp.after = before, after
    if gt is not None:
        lp.group_offsets, lp.n_groups = gt.data_ptr(), gt.numel() - 1
    if flags:
        lp.is_match = fl.data_ptr() + PAD
    nk, nb, nh = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
    rc = N.lib().aha_ac_grep_batch_device(
        m._h, ct.data_ptr(), ot.data_ptr(), ot.numel() - 1, ct.numel(), C.cast(C.pointer(lp), C.POINTER(N.aha_match_params)),
        N.AHA_GREP_LINES | (N.AHA_GREP_INVERT if invert else 0), kept.data_ptr() if ids else None, doo.data_ptr() if ids else None,
        cap if (ids or flags) else 0, big.data_ptr() + PAD if text else None, cap_bytes if text else 0, C.byref(nk), C.byref(nb),
        C.byref(nh), C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    k_h, d_h, b_h, f_h = kept.cpu().numpy(), doo.cpu().numpy(), big.cpu().numpy(), fl.cpu().numpy()
    assert (k_h[cap:] == GUARD64).all() and (d_h[cap + 1:] == GUARD64).all(), "the call wrote behind cap_docs"
    assert (b_h[:PAD] == GUARD8).all() and (b_h[PAD + cap_bytes:] == GUARD8).all(), "the call wrote outside out"
    assert (f_h[:PAD] == GUARD8).all() and (f_h[PAD + cap:] == GUARD8).all(), "the call wrote outside is_match"
    if rc != N.AHA_OK or not text:
        assert (b_h == GUARD8).all()
    if rc != N.AHA_OK or not ids:
        assert (k_h == GUARD64).all() and (d_h == GUARD64).all()
    if rc != N.AHA_OK or not flags:
        assert (f_h == GUARD8).all()
    return k_h[:cap], d_h[:cap + 1], b_h[PAD:PAD + cap_bytes], f_h[PAD:PAD + cap], nk.value, nb.value, nh.value, rc


def _check(m, hits, n_hits, corpus, offs, invert, before, after, groups=None, sep=None, tensors=None, deep=False, host=False):
    """the device entry against the definition; deep: twice (identical bytes), then is_match alone, ids only, out only and the
    sizing call; host: the host entry through grep_batch"""
    w_kept, w_out, w_doo, w_im = want = sim.grep_lines(hits, offs, corpus, invert, before, after, groups)
    K, nb0 = w_kept.size, w_out.size
    ct, ot = tensors or _tensors(corpus, offs)
    gt = _groups_tensor(groups)
    first = None
    for _ in range(2 if deep else 1):
        kept, doo, out, im, nk, nb, nh, rc = _device(m, ct, ot, K + 2, nb0 + 5, invert, before, after, gt, sep)
        assert rc == N.AHA_OK and (nk, nb, nh) == (K, nb0, n_hits), (rc, nk, nb, nh, K, nb0, n_hits, before, after, invert)
        assert np.array_equal(kept[:K].astype(np.uint64), w_kept) and (kept[K:] == GUARD64).all(), (before, after, invert, groups)
        assert np.array_equal(doo[:K + 1].astype(np.uint64), w_doo) and (doo[K + 1:] == GUARD64).all()
        assert out[:nb].tobytes() == w_out.tobytes() and (out[nb:] == GUARD8).all()
        assert np.array_equal(im[:K], w_im) and (im[K:] == GUARD8).all()
        got = (kept.tobytes(), doo.tobytes(), out.tobytes(), im.tobytes())
        assert first is None or got == first
        first = got
    if deep:
        if K:
            *_, im, nk, nb, nh, rc = _device(m, ct, ot, K, 0, invert, before, after, gt, sep, ids=False, text=False)  # is_match alone
            assert rc == N.AHA_OK and (nk, nb, nh) == (K, nb0, n_hits) and np.array_equal(im, w_im)
        kept, doo, _, _, nk, nb, nh, rc = _device(m, ct, ot, K, 0, invert, before, after, gt, sep, text=False, flags=False)
        assert rc == N.AHA_OK and (nk, nb, nh) == (K, nb0, n_hits)  # out == NULL: no copy, the bytes are still counted
        assert np.array_equal(kept.astype(np.uint64), w_kept) and np.array_equal(doo.astype(np.uint64), w_doo)
        _, _, out, _, nk, nb, nh, rc = _device(m, ct, ot, 0, nb0, invert, before, after, gt, sep, ids=False, flags=False)
        assert rc == N.AHA_OK and (nk, nb, nh) == (K, nb0, n_hits) and out.tobytes() == w_out.tobytes()
        *_, nk, nb, nh, rc = _device(m, ct, ot, 0, 0, invert, before, after, gt, sep, ids=False, text=False, flags=False)
        assert rc == N.AHA_OK and (nk, nb, nh) == (K, nb0, n_hits)  # the sizing call
    if host:
        matched = np.full(K + 3, GUARD8, dtype=np.uint8)
        h_kept, h_out, h_doo = m.grep_batch(corpus, offs, sep=sep, invert=invert, before=before, after=after,
                                            groups=None if groups is None else np.asarray(groups, dtype=np.uint64), matched=matched)
        assert np.array_equal(h_kept, w_kept) and h_out.tobytes() == w_out.tobytes() and np.array_equal(h_doo, w_doo)
        assert np.array_equal(matched[:K], w_im) and (matched[K:] == GUARD8).all()
    return want


@pytest.fixture(scope="module")
def plain():
    keys = [b"KEY", b"ab"]
    return AC.compile(keys), orc.AC.compile(keys)


# ---- the header's examples ---------------------------------------------------------------------------------------------------
TEXT = b"x\nab\ny\nz\nab\nw\n"
OFFS = np.array([0, 2, 5, 7, 9, 12, 14], dtype=np.uint64)


def test_header_examples(plain):
    m, o = plain
    corpus = np.frombuffer(TEXT, dtype=np.uint8)
    hits, nh = _hits(o, corpus, OFFS)
    assert hits.tolist() == [0, 1, 0, 0, 1, 0]
    kept, out, doo, im = _check(m, hits, nh, corpus, OFFS, False, 1, 0, deep=True, host=True)
    assert kept.tolist() == [0, 1, 3, 4] and im.tolist() == [0, 1, 0, 1] and out.tobytes() == b"x\nab\nz\nab\n"
    kept, out, doo, im = _check(m, hits, nh, corpus, OFFS, False, 1, 0, groups=[0, 4, 6], deep=True, host=True)
    assert kept.tolist() == [0, 1, 4]
    kept, *_ = _check(m, hits, nh, corpus, OFFS, True, 0, 0, deep=True, host=True)
    assert kept.tolist() == [0, 2, 3, 5]
    # the conveniences
    assert AC.compile(["Error"]).grep("a\nb\nError x\nc\nd\n", after=1) == ["Error x\n", "c\n"]
    assert m.grep(TEXT, before=1) == [b"x\n", b"ab\n", b"z\n", b"ab\n"]
    assert m.grep(TEXT, before=1, separator="--\n") == [b"x\n", b"ab\n", b"--\n", b"z\n", b"ab\n"]
    assert m.grep(TEXT.decode(), context=1, separator="--\n") == ["x\n", "ab\n", "y\n", "z\n", "ab\n", "w\n"]
    assert m.grep(TEXT, context=0, groups=[0, 2, 6], separator=b"--\n") == [b"ab\n", b"--\n", b"ab\n"]
    flags = np.zeros(6, dtype=np.uint8)
    assert m.grep(TEXT, after=1, matched=flags) == [b"ab\n", b"y\n", b"ab\n", b"w\n"] and flags.tolist() == [1, 0, 1, 0, 0, 0]
    from aha_amd import DeviceCorpus

    flags = np.zeros(4, dtype=np.uint8)
    kept, out, doo, n = m.grep_corpus(DeviceCorpus(TEXT, OFFS), before=1, groups=[0, 4, 6], matched=flags)
    assert kept.tolist() == [0, 1, 4] and out.tobytes() == b"x\nab\nab\n" and doo.tolist() == [0, 2, 5, 8] and n == 2
    assert flags.tolist() == [0, 1, 1, 0]


def test_the_torch_binding(plain):
    import torch

    m, o = plain
    corpus = np.frombuffer(TEXT, dtype=np.uint8)
    ct, ot = _tensors(corpus, OFFS)
    kept = torch.zeros(6, dtype=torch.int64, device=DEV)
    doo = torch.zeros(7, dtype=torch.int64, device=DEV)
    out = torch.zeros(14, dtype=torch.uint8, device=DEV)
    matched = torch.full((6,), 9, dtype=torch.uint8, device=DEV)
    gt = _groups_tensor([0, 4, 6])
    assert m.grep_batch_device(ct, ot, kept, doo, out, context=1, groups=gt, matched=matched) == (5, 12, 2)
    assert kept.cpu().tolist()[:5] == [0, 1, 2, 4, 5] and matched.cpu().tolist() == [0, 1, 0, 1, 0, 9]
    assert bytes(out.cpu().numpy()[:12]) == b"x\nab\ny\nab\nw\n"
    assert m.grep_batch_device(ct, ot, before=1) == (4, 10, 2)  # the sizing call
    with pytest.raises(AhaError) as e:
        m.grep_batch_device(ct, ot, kept[:3], None, None, before=1)
    assert e.value.code == N.AHA_E_CAPACITY and (e.value.n_required, e.value.bytes_required) == (4, 10)


# ---- contexts around every edge ------------------------------------------------------------------------------------------------
def _edge_batch():
    """4200 records of one to three bytes; matches placed so that for the contexts of CONTEXTS windows overlap, touch and miss by
    one, end on word (32), 256-record and rank-block (2048) edges, and fall on both sides of group boundaries"""
    rng = random.Random(4200)
    D = 4200
    at = {5, 8, 12, 16,  # context 1: [4, 10) from two touching windows, 12 and 16 miss by one; context 2: all merge
          31, 33, 64, 95, 96,  # matches and window ends on word edges
          160, 160 + 63, 160 + 63 + 64, 160 + 63 + 64 + 65, 160 + 63 + 64 + 65 + 66,  # contexts 31 / 32 / 33: overlap, touch, miss
          255, 256, 288, 511, 513,
          1000, 1000 + 15,
          2015, 2016, 2046, 2047, 2048, 2049, 2050, 2080, 2081,  # around the rank-block edge, windows of 31 .. 33 end on it
          4100, 4196, 4199}
    at |= {3000 + 70 * i for i in range(6)}
    m = [r in at for r in range(D)]
    docs = [b"ab" + (b"\n" if r % 3 else b"") if m[r] else rng.choice([b"\n", b"x\n", b"xy\n", b"q", b"a\n"]) for r in range(D)]
    corpus, offs = _batch(docs)
    # groups: boundaries between two matches (2047 | 2048, 2049 | 2050), next to one (256, 4100), empty groups at the front, in
    # the middle and at the end; the windows of 2046 .. 2047 and of 2048 .. 2049 touch at 2048 from both sides
    groups = [0, 0, 7, 32, 256, 256, 1000, 2048, 2050, 4100, 4200, 4200]
    return corpus, offs, groups, m


@pytest.fixture(scope="module")
def edge_batch(plain):
    corpus, offs, groups, m = _edge_batch()
    hits, nh = _hits(plain[1], corpus, offs)
    assert [h > 0 for h in hits.tolist()] == m
    return corpus, offs, groups, hits, nh, _tensors(corpus, offs)


@pytest.mark.parametrize("before", CONTEXTS)
def test_contexts_around_word_block_and_group_edges(plain, edge_batch, before):
    m, _ = plain
    corpus, offs, groups, hits, nh, tensors = edge_batch
    sizes = set()
    for after in CONTEXTS:
        for g in (None, groups):
            kept, *_ = _check(m, hits, nh, corpus, offs, False, before, after, g, tensors=tensors,
                              deep=(after, g) == (2, None), host=(after, g) == (33, groups))
            sizes.add(kept.size)
    assert len(sizes) > 4  # the contexts make a difference
    _check(m, hits, nh, corpus, offs, True, before, 1, groups, tensors=tensors)  # invert: nearly everything matches


# ---- every D around the edges, every pattern, every kind of groups -------------------------------------------------------------
def _patterns(D, cuts):
    yield "none", [False] * D
    yield "all", [True] * D
    yield "first", [r == 0 for r in range(D)]
    yield "last", [r == D - 1 for r in range(D)]
    yield "alternating", [r % 2 == 0 for r in range(D)]
    yield "one per group", [r in set(cuts[:-1]) for r in range(D)]
    cross = {q + k for q in cuts[1:-1] for k in (-2, -1, 0, 1)}  # a matching run across every inner boundary
    yield "a run across a boundary", [r in cross for r in range(D)]


@pytest.mark.parametrize("D", [0, 1, 31, 32, 33, 2047, 2048, 2049])
def test_every_size_pattern_and_kind_of_groups(plain, D):
    m, o = plain
    cuts = sorted({0, D} | {q for q in (1, 16, 32, D // 2, D - 1) if 0 < q < D})
    kinds = {"null": None, "one group": [0, D], "one per record": list(range(D + 1)),
             "empty groups": [0, 0] + cuts[1:-1] + ([cuts[len(cuts) // 2]] * 2 if len(cuts) > 2 else []) + [D, D, D],
             "cuts": cuts}
    kinds["empty groups"].sort()
    n = 0
    for name, pat in _patterns(D, cuts):
        docs = [(b"ab\n" if r % 2 else b"ab") if pat[r] else (b"x\n" if r % 5 else b"\n") for r in range(D)]
        corpus, offs = _batch(docs)
        hits, nh = _hits(o, corpus, offs)
        assert [h > 0 for h in hits.tolist()] == pat
        tensors = _tensors(corpus, offs)
        for kind, groups in kinds.items():
            for invert in (False, True):
                before, after = ((1, 2), (2, 0), (0, 33), (MAXC, 1))[n % 4]
                _check(m, hits, nh, corpus, offs, invert, before, after, groups, tensors=tensors, deep=n % 16 == 0, host=n % 16 == 8)
                n += 1
    assert n == 7 * 5 * 2


# ---- the groups a records call writes -----------------------------------------------------------------------------------------
def test_the_doc_rec_offsets_of_a_records_call_are_the_groups(plain):
    """split, grep with context, compare with a host split of each document on its own"""
    import torch

    m, o = plain
    rng = random.Random(7)
    docs = []
    for d in range(40):
        lines = [rng.choice([b"a KEY here", b"nothing", b"", b"ab", b"xx", b"q" * 7]) for _ in range(rng.randint(0, 12))]
        doc = b"\n".join(lines)
        docs.append(doc + (b"\n" if rng.random() < 0.5 and doc else b""))
    docs[3] = docs[17] = b""
    corpus, offs = _batch(docs)
    ct, ot = _tensors(corpus, offs)
    with pytest.raises(AhaError) as e:
        m.records_device(ct, ot, None)
    n_rec = e.value.n_required
    rec = torch.zeros(n_rec + 1, dtype=torch.int64, device=DEV)
    dro = torch.zeros(len(docs) + 1, dtype=torch.int64, device=DEV)
    assert m.records_device(ct, ot, rec, dro) == n_rec
    for invert, before, after in ((False, 1, 2), (False, 3, 0), (True, 0, 1), (False, MAXC, MAXC)):
        want_lines, want_flags = [], []
        for doc in docs:  # every document on its own: its lines, its matches, the definition without groups
            lines = doc.split(b"\n")
            lines = [x + b"\n" for x in lines[:-1]] + ([lines[-1]] if lines[-1] else [])
            mm = [(len(o.match(x, chars=False)) > 0) != invert for x in lines]
            keep = sim.keep_brute(mm, before, after, None)
            want_lines += [x for x, k in zip(lines, keep) if k]
            want_flags += [int(f) for f, k in zip(mm, keep) if k]
        K, nb0 = len(want_lines), sum(len(x) for x in want_lines)
        kept, doo, out, im, nk, nb, nh, rc = _device(m, ct, rec, K, nb0, invert, before, after, dro)
        assert rc == N.AHA_OK and (nk, nb) == (K, nb0) and K > 20
        assert [out[int(doo[i]):int(doo[i + 1])].tobytes() for i in range(K)] == want_lines and im.tolist() == want_flags
    # the same through the host calls
    h_rec, h_dro = m.records(corpus, offs)
    assert np.array_equal(h_rec, rec.cpu().numpy().astype(np.uint64)) and np.array_equal(h_dro, dro.cpu().numpy().astype(np.uint64))
    h_kept, h_out, h_doo = m.grep_batch(corpus, h_rec, before=MAXC, after=MAXC, groups=h_dro)
    assert h_out.tobytes() == b"".join(want_lines)


def test_bad_group_offsets_are_refused_with_nothing_written(plain, edge_batch):
    m, _ = plain
    corpus, offs, groups, hits, nh, (ct, ot) = edge_batch
    D = len(offs) - 1
    for bad in ([0, 10, 9, D], [1, 10, D], [0, 10, D - 1], [0, 10, D + 1], [0, D + 5, D], [D, 0]):
        *_, nk, nb, nh_, rc = _device(m, ct, ot, D, corpus.size, False, 1, 1, _groups_tensor(bad))  # (asserts that every guard is intact)
        assert rc == N.AHA_E_INVALID and (nk, nb, nh_) == (0, 0, 0), bad
        with pytest.raises(AhaError) as e:
            m.grep_batch(corpus, offs, before=1, groups=bad)
        assert e.value.code == N.AHA_E_INVALID
    # equal neighbours are fine: many empty groups, far more than D + 1 entries
    many = [0] * 5000 + [D] * 5000
    _check(m, hits, nh, corpus, offs, False, 2, 2, many, tensors=(ct, ot))


# ---- the identities --------------------------------------------------------------------------------------------------------------
def test_identities(plain, edge_batch):
    import torch

    m, _ = plain
    corpus, offs, groups, hits, nh, (ct, ot) = edge_batch
    D = len(offs) - 1
    for invert in (False, True):
        # no context = plain grep, a real call, byte for byte; is_match all 1
        kept = torch.full((D,), GUARD64, dtype=torch.int64, device=DEV)
        doo = torch.full((D + 1,), GUARD64, dtype=torch.int64, device=DEV)
        out = torch.full((corpus.size,), GUARD8, dtype=torch.uint8, device=DEV)
        nk, nb, n = m.grep_batch_device(ct, ot, kept, doo, out, invert=invert)
        k2, d2, o2, im, nk2, nb2, n2, rc = _device(m, ct, ot, D, corpus.size, invert, 0, 0, _groups_tensor(groups))
        assert rc == N.AHA_OK and (nk2, nb2, n2) == (nk, nb, n) and nk > 30
        assert k2.tobytes() == kept.cpu().numpy().tobytes() and d2.tobytes() == doo.cpu().numpy().tobytes()
        assert o2.tobytes() == out.cpu().numpy().tobytes() and (im[:nk] == 1).all()
        # the largest context: exactly the groups that hold a matching record, whole
        mm = sim.matches(hits, D, invert)
        k2, *_, nk2, nb2, n2, rc = _device(m, ct, ot, D, corpus.size, invert, MAXC, MAXC, _groups_tensor(groups))
        want = [r for lo, hi in zip(groups, groups[1:]) if any(mm[lo:hi]) for r in range(lo, hi)]
        assert rc == N.AHA_OK and k2[:nk2].tolist() == want and 0 < nk2
        # without groups every record
        k2, d2, o2, *_, nk2, nb2, n2, rc = _device(m, ct, ot, D, corpus.size, invert, MAXC, MAXC)
        assert rc == N.AHA_OK and nk2 == D and k2.tolist() == list(range(D)) and o2.tobytes() == corpus.tobytes()
        assert d2.astype(np.uint64).tolist() == offs.tolist()
    # no match at all: nothing, whatever the context
    nomatch = AC.compile([b"never"])
    *_, nk2, nb2, n2, rc = _device(nomatch, ct, ot, D, corpus.size, False, MAXC, MAXC)
    assert rc == N.AHA_OK and (nk2, nb2, n2) == (0, 0, 0)


def test_kept_empty_records_under_invert(plain):
    m, o = plain
    rng = random.Random(11)
    docs = [rng.choice([b"", b"", b"ab", b"x", b"KEY!", b"", b"12345678"]) for _ in range(300)]
    corpus, offs = _batch(docs)
    hits, nh = _hits(o, corpus, offs)
    groups = [0, 0, 50, 51, 200, 300]
    for before, after in ((0, 0), (1, 1), (0, 2)):
        kept, out, doo, im = _check(m, hits, nh, corpus, offs, True, before, after, groups, deep=True, host=True)
        assert (np.diff(doo.astype(np.int64)) == 0).sum() > 50  # kept empty records: equal neighbouring offsets
    _check(m, hits, nh, corpus, offs, False, 2, 2, groups, deep=True)
    # N = 0: only empty records
    corpus0, offs0 = _batch([b""] * 40)
    kept, *_ = _check(m, np.zeros(40, dtype=np.int64), 0, corpus0, offs0, True, 1, 1, [0, 10, 40], deep=True, host=True)
    assert kept.size == 40
    _check(m, np.zeros(40, dtype=np.int64), 0, corpus0, offs0, False, 1, 1, [0, 10, 40], deep=True, host=True)


# ---- engines and options -----------------------------------------------------------------------------------------------------
def _random_docs(rng, keys, n):
    docs = []
    for d in range(n):
        size = rng.choice([0, 2, 5, 8, 8, 30])
        out = bytearray()
        while len(out) < size:
            out += rng.choice(keys) if rng.random() < 0.04 else rng.choice([b" ", b"q", "中".encode(), b"\n", b"zz"])
        docs.append(bytes(out[:size]))  # (cut anywhere: keys and characters may be cut at a record's end)
    return docs


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
    corpus, offs = _batch(_random_docs(rng, keys, 2500))
    hits, nh = _hits(o, corpus, offs)
    D = len(offs) - 1
    groups = sorted([0, D] + [rng.randint(0, D) for _ in range(30)])
    for i, pair in enumerate(((1, 1), (0, 3), (40, 2))):
        kept, out, doo, im = _check(m, hits, nh, corpus, offs, False, *pair, groups, deep=i == 0, host=i == 1)
        assert nh > 20 and 20 < im.sum() < kept.size < D


def test_a_separator_filter(plain):
    m, o = plain
    rng = random.Random(5)
    docs = [rng.choice([b"a KEY b\n", b"aKEYb\n", b"ab\n", b"x ab y\n", b"zabz\n", b"\n", b"no\n", b"no\n", b"no\n"]) for _ in range(700)]
    corpus, offs = _batch(docs)
    hits, nh = _hits(o, corpus, offs, SEP_PAIR)
    hits_all, nh_all = _hits(o, corpus, offs)
    assert 0 < nh < nh_all
    groups = [0, 100, 100, 333, 700]
    filtered = _check(m, hits, nh, corpus, offs, False, 1, 1, groups, sep=_sep(), deep=True, host=True)
    unfiltered = _check(m, hits_all, nh_all, corpus, offs, False, 1, 1, groups)
    assert 0 < filtered[3].sum() < unfiltered[3].sum() and filtered[0].size < unfiltered[0].size


def test_folded_handles_keep_the_original_spelling():
    keys = [b"key", b"word", "é".encode(), "жук".encode()]
    o = orc.AC.compile(keys)
    docs_lower = ["a key\n", "\n", "жук é\n", "nothing\n", "none\n", "no\n", "keykey\n", "xx word\n", "q\n", "q\n", "q\n"] * 30
    docs_mixed = [d.upper() if i % 3 == 2 else d.replace("key", "KeY") for i, d in enumerate(docs_lower)]
    assert all(len(a.encode()) == len(b.encode()) for a, b in zip(docs_lower, docs_mixed))
    lower, offs = _batch([d.encode() for d in docs_lower])
    mixed, _ = _batch([d.encode() for d in docs_mixed])
    ascii_lower = mixed.copy()  # what fold_ascii sees of the mixed text: only A-Z folded
    ascii_lower[(mixed >= ord("A")) & (mixed <= ord("Z"))] += 32
    for opts, folded in (({"fold_ascii": True}, ascii_lower), ({"fold_simple": True}, lower)):
        m = AC.compile(keys, **opts)
        hits, nh = _hits(o, folded, offs)
        kept, out, doo, im = _check(m, hits, nh, mixed, offs, False, 1, 1, [0, 11, 330], deep=True, host=True)
        assert nh > 20 and b"KeY" in out.tobytes() and b"NOTHING" in out.tobytes() and 0 < im.sum() < kept.size
        if "fold_simple" in opts:
            assert "ЖУК".encode() in out.tobytes()


# ---- alignment ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shift", [1, 7, 15])
def test_the_corpus_may_start_at_an_odd_address(plain, edge_batch, shift):
    m, _ = plain
    corpus, offs, groups, hits, nh, _t = edge_batch
    _check(m, hits, nh, corpus, offs, False, 2, 33, groups, tensors=_tensors(corpus, offs, shift), deep=True)


# ---- capacity ----------------------------------------------------------------------------------------------------------------
def test_capacity_failures_report_both_numbers_and_write_nothing(plain, edge_batch):
    m, _ = plain
    corpus, offs, groups, hits, nh, (ct, ot) = edge_batch
    gt = _groups_tensor(groups)
    w_kept, w_out, w_doo, w_im = sim.grep_lines(hits, offs, corpus, False, 2, 1, groups)
    K, nb0 = w_kept.size, w_out.size
    assert K > 100 and nb0 > 200
    for cap, cap_bytes in ((K - 1, nb0), (K, nb0 - 1), (K - 1, nb0 - 1), (1, 1)):
        *_, nk, nb, n, rc = _device(m, ct, ot, cap, cap_bytes, False, 2, 1, gt)  # (asserts that every guard is intact)
        assert rc == N.AHA_E_CAPACITY and (nk, nb, n) == (K, nb0, nh)
    # is_match alone counts as a per-document buffer in the verdict, with and without out
    *_, nk, nb, n, rc = _device(m, ct, ot, K - 1, 0, False, 2, 1, gt, ids=False, text=False)
    assert rc == N.AHA_E_CAPACITY and (nk, nb) == (K, nb0)
    *_, nk, nb, n, rc = _device(m, ct, ot, K - 1, nb0, False, 2, 1, gt, ids=False)
    assert rc == N.AHA_E_CAPACITY and (nk, nb) == (K, nb0)
    kept, doo, out, im, nk, nb, n, rc = _device(m, ct, ot, K, nb0, False, 2, 1, gt)  # exactly enough
    assert rc == N.AHA_OK and (nk, nb, n) == (K, nb0, nh) and out.tobytes() == w_out.tobytes() and np.array_equal(im, w_im)
    # a buffer that is not given cannot fail the call
    assert _device(m, ct, ot, K, 0, False, 2, 1, gt, text=False)[7] == N.AHA_OK
    assert _device(m, ct, ot, 0, nb0, False, 2, 1, gt, ids=False, flags=False)[7] == N.AHA_OK
    # the host entry reports the same
    lp = N.aha_grep_lines_params()
    lp.match = _params(False, None)
    lp.match.struct_size = C.sizeof(lp)
    lp.before, lp.after = 2, 1
    g = np.asarray(groups, dtype=np.uint64)
    lp.group_offsets, lp.n_groups = g.ctypes.data, g.size - 1
    flags = np.full(K, GUARD8, dtype=np.uint8)
    lp.is_match = flags.ctypes.data
    kept_h = np.full(K, GUARD64, dtype=np.uint64)
    nk, nb, n = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
    rc = N.lib().aha_ac_grep_batch(m._h, corpus.ctypes.data, offs.ctypes.data, len(offs) - 1,
                                   C.cast(C.pointer(lp), C.POINTER(N.aha_match_params)), N.AHA_GREP_LINES, kept_h.ctypes.data, None, K - 1,
                                   None, 0, C.byref(nk), C.byref(nb), C.byref(n))
    assert rc == N.AHA_E_CAPACITY and (nk.value, nb.value, n.value) == (K, nb0, nh)
    assert (flags == GUARD8).all() and (kept_h == GUARD64).all()


# ---- small grids -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("knob", ["AHA_GREP_BLOCKS", "AHA_POST_BLOCKS"])
def test_one_block_grids(monkeypatch, edge_batch, knob):
    """one workgroup of 256 lanes loops over 132 mask words, 3 rank blocks and -- under invert -- more than 256 group boundaries"""
    monkeypatch.setenv(knob, "1")
    keys = [b"KEY", b"ab"]
    m = AC.compile(keys)
    corpus, offs, groups, hits, nh, tensors = edge_batch
    D = len(offs) - 1
    per_record = list(range(0, D, 3)) + [D]  # 1400 groups: the lanes of kgl_group_edges stride
    for invert, before, after, g in ((False, 1, 2, groups), (False, 33, 2048, None), (True, 1, 0, per_record), (False, 2, 2, per_record),
                                     (True, 0, 0, groups)):
        kept, *_ = _check(m, hits, nh, corpus, offs, invert, before, after, g, tensors=tensors, deep=True)
        assert kept.size > 100 and kept[-1] > 4000  # the records of the later trips are there


# ---- one handle through a sequence ------------------------------------------------------------------------------------------
def test_one_handle_through_a_sequence_of_calls_that_share_scratch(edge_batch):
    import torch

    keys = [b"KEY", b"ab"]
    m = AC.compile(keys)
    corpus, offs, groups, hits, nh, (ct, ot) = edge_batch
    D = len(offs) - 1
    has = hits > 0

    def grep():
        kept = torch.zeros(D, dtype=torch.int64, device=DEV)
        nk, nb, n = m.grep_batch_device(ct, ot, kept, None, None)
        assert n == nh and np.array_equal(kept.cpu().numpy()[:nk], np.nonzero(has)[0])

    def rule_grep():
        table = m.classes([[0], [1]], n_classes=2)
        kept = torch.zeros(D, dtype=torch.int64, device=DEV)
        nk, nb, n = m.grep_batch_device(ct, ot, kept, None, None, rule=[[(1, ">=", 1)]], classes=table)
        assert n == nh and np.array_equal(kept.cpu().numpy()[:nk], np.nonzero(has)[0])  # (every hit here is "ab", class 1)

    def excerpts():
        n_exc, nb, n = m.excerpts_batch_device(ct, ot, before=0, after=0)
        assert n == nh and nb == 2 * nh

    grep()
    _check(m, hits, nh, corpus, offs, False, 2, 33, groups, tensors=(ct, ot), deep=True)
    excerpts()
    rule_grep()
    _check(m, hits, nh, corpus, offs, False, 31, 1, groups, tensors=(ct, ot), deep=True)
    m.release_scratch()
    _check(m, hits, nh, corpus, offs, True, 1, 1, None, tensors=(ct, ot), deep=True, host=True)
    grep()
