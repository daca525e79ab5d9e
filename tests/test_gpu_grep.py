"""Records and grep calls (aha_ac_records_batch*, aha_ac_grep_batch*) against grepsim over the CPU ORACLE's hits per document
(never the library's own match).  Records: sizes and delimiter positions on the mask-word and rank-block edges, every byte a
delimiter and none, document boundaries on, before and behind delimiters, the corpus at each of the 16 alignments, capacity,
small grids.  Grep: every engine variant on ragged documents, kept patterns over 257 and 513 documents, invert with kept empty
documents, a separator filter, a folded handle, a long kept stretch at each of the 16 output alignments, the ids-only form,
both capacities, determinism, neutrality towards the handle's back-off state, the host entry, small grids and the composition
AC.grep.  Every case is a few KiB of text."""
import ctypes as C
import random
import zlib

import numpy as np
import pytest

import grepsim
import pyoracle as orc
from aha_amd import AC, AhaError, DeviceCorpus
from aha_amd import _native as N
from engine_variants import VARIANTS, use_variant
from test_gpu_doc_counts import KEYSETS, SEP_BITS, _batch, _sep

pytestmark = pytest.mark.gpu

GUARD8 = 0x5A
GUARD64 = 0x5A5A5A5A5A5A5A5A
PAD = 16
DEV = "cuda:0"
NL = 10


def _tensors(corpus, offs):
    import torch

    ct = torch.from_numpy(np.ascontiguousarray(corpus)).to(DEV) if corpus.size else torch.zeros(0, dtype=torch.uint8, device=DEV)
    return ct, torch.from_numpy(np.asarray(offs, dtype=np.uint64).view(np.int64)).to(DEV)


@pytest.fixture(scope="module")
def handle():
    return AC.compile(["ab", "b\n"])


# ---- records ---------------------------------------------------------------------------------------------------------------
def _records_device(m, ct, ot, D, cap, delim=b"\n", sizing=False):
    """the device entry with guard words behind cap + 1 record offsets and behind the D + 1 document offsets
    -> (raw rec, raw dro, n, rc)"""
    import torch

    rec = torch.full((cap + 1 + PAD,), GUARD64, dtype=torch.int64, device=DEV)
    dro = torch.full((D + 1 + PAD,), GUARD64, dtype=torch.int64, device=DEV)
    rc = N.AHA_OK
    try:
        n = m.records_device(ct, ot, None if sizing else rec, dro, delim=delim, cap=cap)
    except AhaError as e:
        if e.code != N.AHA_E_CAPACITY:
            raise
        rc, n = e.code, e.n_required
    torch.cuda.synchronize()
    rec_h, dro_h = rec.cpu().numpy(), dro.cpu().numpy()
    assert (rec_h[cap + 1:] == GUARD64).all(), "the call wrote behind cap + 1 record offsets"
    assert (dro_h[D + 1:] == GUARD64).all(), "the call wrote behind the D + 1 offsets"
    return rec_h[:cap + 1], dro_h[:D + 1], n, rc


def _check_records(m, corpus, offs, delim=b"\n", extra=2):
    want_rec, want_dro = grepsim.records(corpus, offs, delim)
    R, D = want_rec.size - 1, len(offs) - 1
    ct, ot = _tensors(corpus, offs)
    rec, dro, n, rc = _records_device(m, ct, ot, D, R + extra, delim)
    assert rc == N.AHA_OK and n == R
    assert np.array_equal(rec[:R + 1].astype(np.uint64), want_rec), (corpus.size, offs)
    assert (rec[R + 1:] == GUARD64).all(), "the call wrote behind the records"
    assert np.array_equal(dro.astype(np.uint64), want_dro)
    return want_rec, want_dro


def _text(rng, n, p_delim=0.05):
    return np.array([NL if rng.random() < p_delim else rng.choice([97, 98, 0, 138, 11, 9]) for _ in range(n)], dtype=np.uint8)


SIZES = [0, 1, 15, 16, 17, 31, 32, 33, 2047, 2048, 2049, 4097]


@pytest.mark.parametrize("n", SIZES)
def test_records_sizes_on_the_word_and_block_edges(handle, n):
    rng = random.Random(n)
    for p_delim in (0.05, 0.5):
        corpus = _text(rng, n, p_delim)
        _check_records(handle, corpus, [0, n])
        cuts = sorted(rng.randint(0, n) for _ in range(5))
        _check_records(handle, corpus, [0] + cuts + [n])


def test_records_delimiters_exactly_on_the_edges(handle):
    for n in (2048, 2049, 4097):
        for at in ([31], [32], [63], [2047], [2048], [31, 32, 63, 2047, 2048]):
            at = [p for p in at if p < n]
            corpus = np.full(n, 97, dtype=np.uint8)
            corpus[at] = NL
            want_rec, _ = _check_records(handle, corpus, [0, n])
            assert want_rec.tolist() == sorted({0, n} | {p + 1 for p in at})


def test_records_every_byte_a_delimiter_and_none(handle):
    corpus = np.full(300, NL, dtype=np.uint8)
    want_rec, want_dro = _check_records(handle, corpus, [0, 100, 100, 300])
    assert want_rec.tolist() == list(range(301)) and want_dro.tolist() == [0, 100, 100, 300]
    corpus = np.full(300, 97, dtype=np.uint8)
    want_rec, want_dro = _check_records(handle, corpus, [0, 300])
    assert want_rec.tolist() == [0, 300]
    want_rec, want_dro = _check_records(handle, corpus, [0, 0, 7, 7, 300, 300])  # only document ends; empty documents
    assert want_rec.tolist() == [0, 7, 300] and want_dro.tolist() == [0, 0, 1, 1, 2, 2]
    _check_records(handle, corpus, [0, 300], delim=b"a")  # another delimiter byte
    _check_records(handle, np.array([0, 255, 0, 0x80, 0, 1], dtype=np.uint8), [0, 6], delim=b"\x00")


def test_records_empty_batches(handle):
    empty = np.zeros(0, dtype=np.uint8)
    for offs in ([0], [0, 0], [0, 0, 0, 0]):
        want_rec, want_dro = _check_records(handle, empty, offs)
        assert want_rec.tolist() == [0] and want_dro.tolist() == [0] * len(offs)
        ct, ot = _tensors(empty, offs)
        assert _records_device(handle, ct, ot, len(offs) - 1, 0, sizing=True)[2:] == (0, N.AHA_OK)  # R = 0 fits cap 0
        rec, dro = handle.records(empty, offs)
        assert rec.tolist() == [0] and dro.tolist() == [0] * len(offs)


def test_records_document_boundaries_on_before_and_behind_delimiters(handle):
    corpus = np.frombuffer(b"ab\ncd\n\nef\ng" + b"x" * 40 + b"\n" + b"y" * 30, dtype=np.uint8).copy()
    n = corpus.size
    # a boundary behind a delimiter (3, 6, 7) is counted once; on one (2, 5: the delimiter starts the next document); before (1)
    for offs in ([0, 3, 6, 7, n], [0, 2, 5, n], [0, 1, 4, 8, n], [0, 0, 3, 3, 3, 6, n, n], [0, 2, 3, 5, 6, 7, 10, 11, n]):
        want_rec, want_dro = _check_records(handle, corpus, offs)
        assert want_rec[-1] == n and (np.diff(want_rec.astype(np.int64)) > 0).all()
    assert grepsim.records(corpus, [0, 3, 6, 7, n], b"\n")[0].tolist() == grepsim.records(corpus, [0, n], b"\n")[0].tolist()


def test_records_at_each_of_the_16_alignments(handle):
    """the corpus tensor sliced at every offset from an aligned address, delimiter bytes in front of it and behind it: none
    of them reaches a result"""
    import torch

    rng = random.Random(16)
    for n in (5, 40, 2100):
        corpus = _text(rng, n, 0.1)
        want_rec, want_dro = grepsim.records(corpus, [0, n], b"\n")
        R = want_rec.size - 1
        for k in range(16):
            big = torch.full((64 + n + 64,), NL, dtype=torch.uint8, device=DEV)
            big[48 + k:48 + k + n] = torch.from_numpy(corpus).to(DEV)
            ct = big[48 + k:48 + k + n]
            assert ct.data_ptr() % 16 == k and ct.is_contiguous()
            ot = torch.tensor([0, n], dtype=torch.int64, device=DEV)
            rec, dro, got, rc = _records_device(handle, ct, ot, 1, R + 2)
            assert rc == N.AHA_OK and got == R, (n, k)
            assert np.array_equal(rec[:R + 1].astype(np.uint64), want_rec), (n, k)
            assert (rec[R + 1:] == GUARD64).all() and dro.tolist() == [0, R]


def test_records_capacity_writes_nothing(handle):
    rng = random.Random(3)
    corpus = _text(rng, 3000, 0.1)
    offs = [0, 1000, 3000]
    want_rec, want_dro = grepsim.records(corpus, offs, b"\n")
    R = want_rec.size - 1
    ct, ot = _tensors(corpus, offs)
    rec, dro, n, rc = _records_device(handle, ct, ot, 2, R - 1)
    assert rc == N.AHA_E_CAPACITY and n == R
    assert (rec == GUARD64).all() and (dro == GUARD64).all(), "a failing call wrote a caller's buffer"
    rec, dro, n, rc = _records_device(handle, ct, ot, 2, 0, sizing=True)  # the sizing call
    assert rc == N.AHA_E_CAPACITY and n == R and (dro == GUARD64).all()
    rec, dro, n, rc = _records_device(handle, ct, ot, 2, R)  # exactly enough
    assert rc == N.AHA_OK and np.array_equal(rec.astype(np.uint64), want_rec) and np.array_equal(dro.astype(np.uint64), want_dro)
    # the host entry: one short, then the Python form (a sizing call first)
    L = N.lib()
    n64 = C.c_uint64(0)
    rec_h = np.full(R + 1, GUARD64, dtype=np.uint64)
    dro_h = np.full(3, GUARD64, dtype=np.uint64)
    offs_h = np.array(offs, dtype=np.uint64)
    rc = L.aha_ac_records_batch(handle._h, corpus.ctypes.data, offs_h.ctypes.data, 2, NL, 0, rec_h.ctypes.data, R - 1,
                                dro_h.ctypes.data, C.byref(n64))
    assert rc == N.AHA_E_CAPACITY and n64.value == R and (rec_h == GUARD64).all() and (dro_h == GUARD64).all()
    h_rec, h_dro = handle.records(corpus, offs)
    assert np.array_equal(h_rec, want_rec) and np.array_equal(h_dro, want_dro)
    bad = np.array([0, 2000, 1000, 3000], dtype=np.uint64)  # descending offsets: found on the device
    ct, ot = _tensors(corpus, bad)
    with pytest.raises(AhaError) as e:
        handle.records_device(ct, ot, None)
    assert e.value.code == N.AHA_E_INVALID


def test_records_with_one_block_grids(monkeypatch):
    monkeypatch.setenv("AHA_GREP_BLOCKS", "1")
    m = AC.compile(["ab"])
    rng = random.Random(8)
    for n in (4097, 70000):  # more than one trip of the one workgroup's four waves, in every kernel
        corpus = _text(rng, n, 0.03)
        cuts = sorted(rng.randint(0, n) for _ in range(600))
        _check_records(m, corpus, [0] + cuts + [n])


# ---- grep ------------------------------------------------------------------------------------------------------------------
def _hits_per_doc(o, corpus, offs, sep=None):
    """the oracle's hits per document; sep = (size, set bits) or None"""
    offs = np.asarray(offs, dtype=np.uint64)
    if sep is None:
        return np.diff(np.asarray(o.match_batch(corpus, offs)[1]).astype(np.int64))
    return np.array([o.match(corpus[int(offs[d]):int(offs[d + 1])].tobytes(), chars=False, sep=sep).size
                     for d in range(offs.size - 1)], dtype=np.int64)


def _grep_device(m, ct, ot, cap_docs, cap_bytes, invert=False, sep=None, text=True, align=0, ids=True):
    """the device entry with guard words behind cap_docs indices, cap_docs + 1 offsets and cap_bytes bytes (out starts
    `align` bytes behind an aligned address, guard bytes in front of it too) -> (raw kept, raw doo, raw out, n_kept, n_bytes,
    n_hits, rc)"""
    import torch

    kept = torch.full((cap_docs + PAD,), GUARD64, dtype=torch.int64, device=DEV)
    doo = torch.full((cap_docs + 1 + PAD,), GUARD64, dtype=torch.int64, device=DEV)
    big = torch.full((64 + cap_bytes + 64,), GUARD8, dtype=torch.uint8, device=DEV)
    out = big[48 + align:48 + align + cap_bytes]
    rc, nh = N.AHA_OK, None
    try:
        nk, nb, nh = m.grep_batch_device(ct, ot, kept if ids else None, doo if ids else None, out if text else None, sep=sep,
                                         invert=invert, cap_docs=cap_docs)
    except AhaError as e:
        if e.code != N.AHA_E_CAPACITY:
            raise
        rc, nk, nb = e.code, e.n_required, e.bytes_required
    torch.cuda.synchronize()
    kept_h, doo_h, big_h = kept.cpu().numpy(), doo.cpu().numpy(), big.cpu().numpy()
    assert (kept_h[cap_docs:] == GUARD64).all(), "the call wrote behind cap_docs indices"
    assert (doo_h[cap_docs + 1:] == GUARD64).all(), "the call wrote behind cap_docs + 1 offsets"
    assert (big_h[:48 + align] == GUARD8).all() and (big_h[48 + align + cap_bytes:] == GUARD8).all(), "the call wrote outside out"
    return kept_h[:cap_docs], doo_h[:cap_docs + 1], big_h[48 + align:48 + align + cap_bytes], nk, nb, nh, rc


def _check_grep(m, corpus, offs, h, invert=False, sep=None, align=0, host=True):
    """device entry (twice: identical bytes) and host entry against grepsim.grep over the given hits per document"""
    want_kept, want_out, want_doo = grepsim.grep(h, offs, corpus, invert)
    nk0, nb0 = want_kept.size, want_out.size
    ct, ot = _tensors(corpus, offs)
    first = None
    for _ in range(2):
        kept, doo, out, nk, nb, nh, rc = _grep_device(m, ct, ot, nk0 + 2, nb0 + 5, invert, sep, align=align)
        assert rc == N.AHA_OK and (nk, nb, nh) == (nk0, nb0, int(np.sum(h)))
        assert np.array_equal(kept[:nk].astype(np.uint64), want_kept) and (kept[nk:] == GUARD64).all()
        assert np.array_equal(doo[:nk + 1].astype(np.uint64), want_doo) and (doo[nk + 1:] == GUARD64).all()
        assert out[:nb].tobytes() == want_out.tobytes() and (out[nb:] == GUARD8).all()
        got = (kept.tobytes(), doo.tobytes(), out.tobytes())
        assert first is None or got == first
        first = got
    if host:
        h_kept, h_out, h_doo = m.grep_batch(corpus, offs, sep=sep, invert=invert)
        assert np.array_equal(h_kept, want_kept) and h_out.tobytes() == want_out.tobytes() and np.array_equal(h_doo, want_doo)
    return want_kept, want_out, want_doo


def _ragged_docs(rng, keys, density=0.02):
    """documents of many sizes cut anywhere, sparse in keys so that some have a hit and some have none; empty ones first, in
    the middle and last"""
    pieces = [k for k in keys if len(k) < 64]
    fill = [b" ", b"q", b"\x00", b"zz", "中".encode(), b"x", b"\n"]
    sizes = [1, 2, 7, 16, 31, 32, 33, 63, 64, 65, 130, 300] * 3
    rng.shuffle(sizes)
    docs = []
    for n in sizes:
        out = bytearray()
        while len(out) < n:
            out += rng.choice(pieces) if rng.random() < density else rng.choice(fill)
        docs.append(bytes(out[:n]))
    mid = len(docs) // 2
    return [b""] + docs[:mid] + [b"", b""] + docs[mid:] + [b""]


@pytest.fixture(params=VARIANTS)
def variant(request, monkeypatch):
    return use_variant(request.param, monkeypatch)


@pytest.mark.parametrize("keyset", ["ascii", "utf8", "nested"])
def test_grep_parity_every_engine_variant(variant, keyset):
    rng = random.Random(zlib.crc32(f"grep/{keyset}".encode()))
    keys = KEYSETS[keyset](rng)
    m, o = AC.compile(keys), orc.AC.compile(keys)
    corpus, offs = _batch(_ragged_docs(rng, keys, 0.1 if keyset == "nested" else 0.03))
    h = _hits_per_doc(o, corpus, offs)
    assert 0 < np.count_nonzero(h) < h.size - 4  # (from the oracle) some kept, some dropped beside the empty ones
    for invert in (False, True):
        _check_grep(m, corpus, offs, h, invert, host=not invert)


def _pattern_docs(keep):
    """one document per entry, of a length that depends on its index: with the key where keep is set"""
    return [(b"x" * (d % 7) + b"KEY" + b"y" * (d % 5)) if k else b"z" * (d % 9) for d, k in enumerate(keep)]


@pytest.mark.parametrize("D", [257, 513])
def test_grep_kept_patterns_over_words_and_blocks(D):
    m, o = AC.compile(["KEY"]), orc.AC.compile(["KEY"])
    idx = np.arange(D)
    patterns = {
        "alternating": idx % 2 == 0,
        "alternating, dropped first": idx % 2 == 1,
        "all": idx >= 0,
        "none": idx < 0,
        "only the first": idx == 0,
        "only the last": idx == D - 1,
        "a dropped run across a mask word": ~((idx >= 20) & (idx < 40)),
        "dropped runs across words, kept ones between": ~(((idx >= 30) & (idx < 34)) | ((idx >= 62) & (idx < 66)) | (idx == 96)),
        "a dropped run across a 256-document block": ~((idx >= 250) & (idx < 257)),
        "a kept run across a 256-document block": (idx >= 250) & (idx < 257),
        "runs of three": idx % 6 < 3,
    }
    for name, keep in patterns.items():
        corpus, offs = _batch(_pattern_docs(keep))
        h = _hits_per_doc(o, corpus, offs)
        assert np.array_equal(h >= 1, keep), name  # (from the oracle)
        want_kept, _, _ = _check_grep(m, corpus, offs, h, host=False)
        assert np.array_equal(want_kept, idx[keep]), name
        _check_grep(m, corpus, offs, h, invert=True, host=False)


def test_grep_invert_keeps_empty_documents():
    """kept empty documents between dropped ones: adjacent dropped runs whose output positions tie"""
    m, o = AC.compile(["KEY"]), orc.AC.compile(["KEY"])
    docs = [b"", b"aKEY", b"", b"KEYKEY", b"", b"", b"KEY", b"none", b"", b"KEYb", b""]
    corpus, offs = _batch(docs)
    h = _hits_per_doc(o, corpus, offs)
    want_kept, want_out, want_doo = _check_grep(m, corpus, offs, h, invert=True)
    assert want_kept.tolist() == [0, 2, 4, 5, 7, 8, 10] and want_out.tobytes() == b"none"
    assert want_doo.tolist() == [0, 0, 0, 0, 0, 4, 4, 4]
    _check_grep(m, corpus, offs, h)
    corpus, offs = _batch([b"", b"", b""])  # N = 0: nothing can hit, invert keeps all
    h = np.zeros(3, dtype=np.int64)
    assert _check_grep(m, corpus, offs, h, invert=True)[0].tolist() == [0, 1, 2]
    assert _check_grep(m, corpus, offs, h)[0].size == 0
    empty, offs0 = np.zeros(0, dtype=np.uint8), np.array([0], dtype=np.uint64)  # D = 0
    for invert in (False, True):
        want_kept, _, want_doo = _check_grep(m, empty, offs0, np.zeros(0, dtype=np.int64), invert=invert)
        assert want_kept.size == 0 and want_doo.tolist() == [0]


def test_grep_with_a_separator_filter():
    rng = random.Random(77)
    keys = KEYSETS["ascii"](rng)
    m, o = AC.compile(keys), orc.AC.compile(keys)
    corpus, offs = _batch(_ragged_docs(rng, keys, 0.08))
    bits = [i for i in range(40) if i not in SEP_BITS]
    h = _hits_per_doc(o, corpus, offs, (40, bits))
    plain = _hits_per_doc(o, corpus, offs)
    assert 0 < np.count_nonzero(h) < np.count_nonzero(plain)  # whole-word grep keeps fewer documents
    for invert in (False, True):
        _check_grep(m, corpus, offs, h, invert, sep=_sep())


def test_grep_on_a_folded_handle_keeps_the_callers_case():
    rng = random.Random(5)
    words = sorted({"".join(rng.choice("abcdEFGH") for _ in range(rng.randint(3, 6))) for _ in range(100)}, key=str.lower)
    keys = [w.encode() for w in {w.lower(): w for w in words}.values()]  # distinct after folding
    m = AC.compile(keys, fold_ascii=True)
    o = orc.AC.compile([k.lower() for k in keys])
    corpus, offs = _batch(_ragged_docs(rng, [k.swapcase() for k in keys] + keys, 0.05))
    low = np.frombuffer(corpus.tobytes().lower(), dtype=np.uint8).copy()
    h = _hits_per_doc(o, low, offs)
    assert np.count_nonzero(h) > 0 and low.tobytes() != corpus.tobytes()
    _, want_out, _ = _check_grep(m, corpus, offs, h)
    assert want_out.tobytes() != want_out.tobytes().lower()  # the original spelling came through
    _check_grep(m, corpus, offs, h, invert=True)


def test_grep_long_kept_stretch_at_each_output_alignment():
    """kept stretches longer than 3 KiB with position-dependent bytes, between dropped documents of odd lengths: tiles inside
    one stretch take the copy's fixed-distance path at every alignment of out against the corpus"""
    m, o = AC.compile([b"\xfe\xff"]), orc.AC.compile([b"\xfe\xff"])
    long1 = bytes((i * 7 + 3) % 251 for i in range(3500))
    long2 = bytes((i * 13 + 5) % 241 for i in range(4101))
    docs = [b"\xfe\xff" * 3 + b"q", long1, b"a\xfe\xffbc", b"", b"\xfe\xff", long2, b"zz\xfe\xff"]
    corpus, offs = _batch(docs)
    h = _hits_per_doc(o, corpus, offs)
    assert (h >= 1).tolist() == [True, False, True, False, True, False, True]
    for align in range(16):
        _, want_out, _ = _check_grep(m, corpus, offs, h, invert=True, align=align, host=align == 0)
        assert want_out.tobytes() == long1 + long2


def test_grep_ids_only_form_writes_no_text():
    m, o = AC.compile(["KEY"]), orc.AC.compile(["KEY"])
    keep = np.arange(100) % 3 == 1
    corpus, offs = _batch(_pattern_docs(keep))
    h = _hits_per_doc(o, corpus, offs)
    want_kept, want_out, want_doo = grepsim.grep(h, offs, corpus, False)
    ct, ot = _tensors(corpus, offs)
    kept, doo, out, nk, nb, nh, rc = _grep_device(m, ct, ot, want_kept.size, 64, text=False)
    assert rc == N.AHA_OK and (nk, nb, nh) == (want_kept.size, want_out.size, int(h.sum()))
    assert np.array_equal(kept.astype(np.uint64), want_kept) and np.array_equal(doo.astype(np.uint64), want_doo)
    assert (out == GUARD8).all()
    assert m.grep_batch_device(ct, ot) == (want_kept.size, want_out.size, int(h.sum()))  # the sizing call: no buffer at all
    h_kept, h_out, h_doo = m.grep_batch(corpus, offs, text=False)
    assert np.array_equal(h_kept, want_kept) and h_out.size == 0 and np.array_equal(h_doo, want_doo)
    c_kept, c_out, c_doo, c_nh = m.grep_corpus(DeviceCorpus(corpus, offs))
    assert np.array_equal(c_kept, want_kept) and c_out.tobytes() == want_out.tobytes() and np.array_equal(c_doo, want_doo)
    assert c_nh == int(h.sum())


def test_grep_capacity_reports_both_numbers_and_writes_nothing():
    m, o = AC.compile(["KEY"]), orc.AC.compile(["KEY"])
    keep = np.arange(90) % 4 != 2
    corpus, offs = _batch(_pattern_docs(keep))
    h = _hits_per_doc(o, corpus, offs)
    want_kept, want_out, want_doo = grepsim.grep(h, offs, corpus, False)
    nk0, nb0 = want_kept.size, want_out.size
    ct, ot = _tensors(corpus, offs)
    for cap_docs, cap_bytes, ids, text in ((nk0 - 1, nb0, True, True), (nk0, nb0 - 1, True, True), (nk0 - 1, nb0 - 1, True, True),
                                           (0, nb0 - 1, False, True), (nk0 - 1, 0, True, False)):
        kept, doo, out, nk, nb, _, rc = _grep_device(m, ct, ot, cap_docs, cap_bytes, text=text, ids=ids)
        assert rc == N.AHA_E_CAPACITY and (nk, nb) == (nk0, nb0), (cap_docs, cap_bytes)
        assert (kept == GUARD64).all() and (doo == GUARD64).all() and (out == GUARD8).all(), "a failing call wrote a caller's buffer"
    kept, doo, out, nk, nb, _, rc = _grep_device(m, ct, ot, nk0, nb0)  # exactly enough
    assert rc == N.AHA_OK and out.tobytes() == want_out.tobytes() and np.array_equal(doo.astype(np.uint64), want_doo)
    # the host entry, one short each way
    L = N.lib()
    offs_h = np.asarray(offs, dtype=np.uint64)
    for cap_docs, cap_bytes in ((nk0 - 1, nb0), (nk0, nb0 - 1)):
        kept_h = np.full(nk0, GUARD64, dtype=np.uint64)
        doo_h = np.full(nk0 + 1, GUARD64, dtype=np.uint64)
        out_h = np.full(nb0, GUARD8, dtype=np.uint8)
        nk64, nb64 = C.c_uint64(0), C.c_uint64(0)
        rc = L.aha_ac_grep_batch(m._h, corpus.ctypes.data, offs_h.ctypes.data, offs_h.size - 1, None, 0, kept_h.ctypes.data,
                                 doo_h.ctypes.data, cap_docs, out_h.ctypes.data, cap_bytes, C.byref(nk64), C.byref(nb64), None)
        assert rc == N.AHA_E_CAPACITY and (nk64.value, nb64.value) == (nk0, nb0)
        assert (kept_h == GUARD64).all() and (doo_h == GUARD64).all() and (out_h == GUARD8).all()
    import torch

    with pytest.raises(AhaError) as e:  # out inside the corpus: no in-place form
        m.grep_batch_device(ct, ot, out=ct[3:40])
    assert e.value.code == N.AHA_E_INVALID
    bad = torch.tensor([0, 50, 20, corpus.size], dtype=torch.int64, device=DEV)
    with pytest.raises(AhaError) as e:
        m.grep_batch_device(ct, bad)
    assert e.value.code == N.AHA_E_INVALID


def test_grep_leaves_no_trace_in_the_back_off(monkeypatch):
    """match -> grep -> match on a handle whose first match is handed back by the prefix-filter engine: every later match
    gives the hits, the engine and the repeats of a twin handle that never saw the call in between."""
    monkeypatch.delenv("AHA_ENGINE", raising=False)
    dense = b"abcd" * 3000
    sparse = b"-" * 5000 + b"abcd"

    def run(with_grep):
        m = AC.compile(["abc", "bcd"])
        assert m.info["filter_prefix_bytes"] == 3
        m.set_profiling(True)
        seen = []
        for text in [dense] + [sparse] * 6 + [dense] + [sparse] * 3:
            hits = m.match_array(text)
            t = m.last_timing()
            seen.append((t["engine"], t["repeats"], hits.tobytes()))
            if with_grep:
                for t2 in (dense, sparse):
                    kept, out, doo = m.grep_batch(t2, [0, 100, len(t2)])
                    assert kept.tolist() == ([0, 1] if t2 is dense else [1]) and doo[-1] == out.size
                    assert m.last_timing()["n_hits"] == (6000 if t2 is dense else 2)
        m.release_scratch()
        assert m.scratch_bytes() == 0
        return seen

    plain = run(False)
    assert plain[0][0] == 2 and plain[1][0] == 2 and plain[6][0] == 5, [p[:2] for p in plain]
    assert run(True) == plain


def test_grep_with_one_block_grids(monkeypatch):
    monkeypatch.setenv("AHA_GREP_BLOCKS", "1")
    m, o = AC.compile(["KEY"]), orc.AC.compile(["KEY"])
    rng = random.Random(12)
    keep = np.array([rng.random() < 0.5 for _ in range(9000)])  # more than one trip of the one workgroup, in every kernel
    keep[4000:4600] = False
    corpus, offs = _batch(_pattern_docs(keep))
    h = _hits_per_doc(o, corpus, offs)
    for invert in (False, True):
        _check_grep(m, corpus, offs, h, invert, host=False)


def test_grep_composition_equals_the_line_filter():
    keys = ["Error", "WARN", "disk"]
    m = AC.compile(keys)
    rng = random.Random(40)
    words = ["Error", "WARN", "disk", "ok", "info", "Err", "WAR", "\n", "\n\n", " ", "x" * 40, "中文"]
    for trial in range(6):
        text = "".join(rng.choice(words) + rng.choice(["", " ", "\n"]) for _ in range(rng.choice([0, 1, 30, 400])))
        want = [ln for ln in text.splitlines(keepends=True) if any(k in ln for k in keys)]
        assert m.grep(text) == want
        assert m.grep(text.encode()) == [w.encode() for w in want]
        inv = [ln for ln in text.splitlines(keepends=True) if not any(k in ln for k in keys)]
        assert m.grep(text, invert=True) == inv
    assert m.grep("a;Error;b", delim=";") == ["Error;"]
    m2 = AC.compile(["ab", "b\n"])  # the worked example of the header
    assert m2.grep(b"xab\nq\n\nb") == [b"xab\n"] and m2.grep(b"xab\nq\n\nb", invert=True) == [b"q\n", b"\n", b"b"]
    rec, dro = m2.records(b"xab\nq\n\nb")
    assert rec.tolist() == [0, 4, 6, 7, 8] and dro.tolist() == [0, 4]
