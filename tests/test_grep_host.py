"""CPU tests of the records and grep calls (aha_ac_records_batch*, aha_ac_grep_batch*): declared, exported, listed and bound;
their argument checks, which come before any device work -- so they hold on a host-only handle; and the device arithmetic as
grepsim.kernel_model states it (the end mask's word assembly at every alignment, document ends OR-ed in, ranks, S and T, A,
delta, shift, the offsets, the copy by last-segment lookup) against the plain statement of both contracts, on random
small-alphabet batches with the oracle's hits per record."""
import ctypes as C
import os
import random
import re

import numpy as np
import pytest

import grepsim
import pyoracle as orc
from aha_amd import AC, AhaError
from aha_amd import _native as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("aha_ac_records_batch", "aha_ac_records_batch_device", "aha_ac_grep_batch", "aha_ac_grep_batch_device")
GUARD = 0x5A


def test_grep_symbols_exported_declared_and_bound():
    hdr = open(os.path.join(ROOT, "include", "aha_hip.h")).read()
    listed = open(os.path.join(ROOT, "aha_amd", "csrc", "exports.map")).read()
    crystal = open(os.path.join(ROOT, "bindings", "crystal", "aha_hip.cr")).read()
    cpp = open(os.path.join(ROOT, "include", "aha", "ac.hpp")).read()
    L = C.CDLL(N.LIB_PATH)
    for name in ENTRIES:
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert re.search(r"^\s+%s;" % name, listed, re.M), name
        assert name in N.SIGNATURES and hasattr(L, name), name
        assert re.search(r"^\s*fun %s\(" % name, crystal, re.M), name
    assert "aha_ac_records_batch(" in cpp and "aha_ac_grep_batch(" in cpp
    assert re.search(r"#define\s+AHA_GREP_INVERT\s+1u", hdr) and N.AHA_GREP_INVERT == 1
    assert N.lib().aha_abi_version() == 8  # a pure addition
    for method in ("records", "records_device", "grep_batch", "grep_batch_device", "grep_corpus", "grep"):
        assert callable(getattr(AC, method))


def _params(**kw):
    p = N.aha_match_params()
    p.struct_size = C.sizeof(N.aha_match_params)
    for k, v in kw.items():
        setattr(p, k, v)
    return p


class _Buffers:
    def __init__(self):
        self.corpus = np.frombuffer(b"xab\nq\n\nb", dtype=np.uint8).copy()
        self.offs = np.array([0, self.corpus.size], dtype=np.uint64)
        self.rec = np.full(16, GUARD, dtype=np.uint64)
        self.dro = np.full(2, GUARD, dtype=np.uint64)
        self.kept = np.full(16, GUARD, dtype=np.uint64)
        self.doo = np.full(17, GUARD, dtype=np.uint64)
        self.out = np.full(64, GUARD, dtype=np.uint8)

    def untouched(self):
        return all((a == GUARD).all() for a in (self.rec, self.dro, self.kept, self.doo, self.out))


def _records_both(m, flags=0, n=True, rec=True, cap=15):
    """rc of the host entry and of the device entry of records on the same arguments; the buffers stay untouched"""
    b = _Buffers()
    nr = C.c_uint64(7)
    pn = C.byref(nr) if n else None
    prec = b.rec.ctypes.data if rec else None
    L = N.lib()
    rc_h = L.aha_ac_records_batch(m._h, b.corpus.ctypes.data, b.offs.ctypes.data, 1, 10, flags, prec, cap, b.dro.ctypes.data, pn)
    rc_d = L.aha_ac_records_batch_device(m._h, b.corpus.ctypes.data, b.offs.ctypes.data, 1, b.corpus.size, 10, flags, prec, cap,
                                         b.dro.ctypes.data, pn, None)
    assert b.untouched() and nr.value == 7
    return rc_h, rc_d


def _grep_both(m, p, flags=0, n=True, kept=True, doo=True, out=True, cap_docs=16, cap_bytes=64, overlap=False):
    """rc of the host entry and of the device entry of grep on the same arguments; the buffers stay untouched"""
    b = _Buffers()
    nk, nb = C.c_uint64(7), C.c_uint64(7)
    pn = C.byref(nk) if n else None
    pk = b.kept.ctypes.data if kept else None
    pd = b.doo.ctypes.data if doo else None
    po = (b.corpus.ctypes.data + 2 if overlap else b.out.ctypes.data) if out else None
    L = N.lib()
    rc_h = L.aha_ac_grep_batch(m._h, b.corpus.ctypes.data, b.offs.ctypes.data, 1, C.byref(p), flags, pk, pd, cap_docs, po, cap_bytes,
                               pn, C.byref(nb), None)
    rc_d = L.aha_ac_grep_batch_device(m._h, b.corpus.ctypes.data, b.offs.ctypes.data, 1, b.corpus.size, C.byref(p), flags, pk, pd,
                                      cap_docs, po, cap_bytes, pn, C.byref(nb), None, None)
    assert b.untouched() and nk.value == 7 and nb.value == 7
    return rc_h, rc_d


INVALID2 = (N.AHA_E_INVALID, N.AHA_E_INVALID)
NO_DEVICE2 = (N.AHA_E_NO_DEVICE, N.AHA_E_NO_DEVICE)


def test_grep_host_only_handle_has_no_device():
    m = AC.compile(["ab", "b\n"], host_only=True)
    assert _records_both(m) == NO_DEVICE2
    assert _records_both(m, rec=False, cap=0) == NO_DEVICE2  # a sizing call
    assert _grep_both(m, _params()) == NO_DEVICE2
    assert _grep_both(m, _params(), flags=N.AHA_GREP_INVERT) == NO_DEVICE2
    assert _grep_both(m, _params(), kept=False, doo=False, out=False, cap_docs=0, cap_bytes=0) == NO_DEVICE2
    assert _grep_both(m, _params(sep_size=40)) == NO_DEVICE2  # a separator filter is allowed
    for call in (lambda: m.records(b"a\nb"), lambda: m.grep(b"a\nb"), lambda: m.grep("a\nb", invert=True),
                 lambda: m.grep_batch(b"a\nb", [0, 3])):
        with pytest.raises(AhaError) as e:
            call()
        assert e.value.code == N.AHA_E_NO_DEVICE


def test_records_argument_checks_come_before_the_device_check():
    m = AC.compile(["ab", "b\n"], host_only=True)
    for flags in (1, 2, 0x80000000):
        assert _records_both(m, flags=flags) == INVALID2
    assert _records_both(m, n=False) == INVALID2
    assert _records_both(m, rec=False, cap=3) == INVALID2  # a NULL buffer with a capacity
    L = N.lib()
    n = C.c_uint64(0)
    offs = np.array([0, 0], dtype=np.uint64)
    assert L.aha_ac_records_batch(None, None, offs.ctypes.data, 1, 10, 0, None, 0, None, C.byref(n)) == N.AHA_E_INVALID
    assert L.aha_ac_records_batch_device(None, None, offs.ctypes.data, 1, 0, 10, 0, None, 0, None, C.byref(n), None) == N.AHA_E_INVALID
    assert L.aha_ac_records_batch(m._h, None, None, 0, 10, 0, None, 0, None, C.byref(n)) == N.AHA_E_INVALID
    assert L.aha_ac_records_batch_device(m._h, None, None, 0, 0, 10, 0, None, 0, None, C.byref(n), None) == N.AHA_E_INVALID
    with pytest.raises(ValueError):
        m.records(b"a\nb", delim=b"\r\n")


def test_grep_argument_checks_come_before_the_device_check():
    m = AC.compile(["ab", "b\n"], host_only=True)
    assert _grep_both(m, _params(char_offsets=1)) == INVALID2
    for longest in (1, 2):
        assert _grep_both(m, _params(longest=longest)) == INVALID2
    for flags in (2, 3, 0x80000000):
        assert _grep_both(m, _params(), flags=flags) == INVALID2
    assert _grep_both(m, _params(), n=False) == INVALID2
    assert _grep_both(m, _params(), kept=False, doo=False) == INVALID2  # cap_docs without either per-document buffer
    assert _grep_both(m, _params(), out=False) == INVALID2  # cap_bytes without out
    assert _grep_both(m, _params(), overlap=True) == INVALID2  # no in-place form
    assert _grep_both(m, _params(sep_size=257)) == (N.AHA_E_SEP_SIZE, N.AHA_E_SEP_SIZE)
    L = N.lib()
    n = C.c_uint64(0)
    offs = np.array([0, 0], dtype=np.uint64)
    assert L.aha_ac_grep_batch(None, None, offs.ctypes.data, 1, None, 0, None, None, 0, None, 0, C.byref(n), None, None) == N.AHA_E_INVALID
    assert L.aha_ac_grep_batch_device(None, None, offs.ctypes.data, 1, 0, None, 0, None, None, 0, None, 0, C.byref(n), None, None,
                                      None) == N.AHA_E_INVALID
    assert L.aha_ac_grep_batch(m._h, None, None, 0, None, 0, None, None, 0, None, 0, C.byref(n), None, None) == N.AHA_E_INVALID


# ---- the device arithmetic against the plain statement ---------------------------------------------------------------------
def test_eq4_is_an_exact_byte_compare():
    rng = random.Random(4)
    for _ in range(4000):
        b = rng.choice([0, 10, 0x7F, 0x80, 0xFF, rng.randrange(256)])
        by = [rng.choice([b, b ^ 0x80, b ^ 1, (b + 1) & 255, (b - 1) & 255, 0, 0x80, rng.randrange(256)]) for _ in range(4)]
        w = int.from_bytes(bytes(by), "little")
        assert grepsim.eq4(w, b * 0x01010101) == sum(1 << k for k in range(4) if by[k] == b), (b, by)


def test_end_mask_words_at_every_alignment():
    rng = random.Random(11)
    for n in [0, 1, 15, 16, 17, 31, 32, 33, 47, 48, 49, 63, 64, 65, 100, 300]:
        for dense in (0.0, 0.3, 1.0):
            text = np.array([10 if rng.random() < dense else rng.choice([9, 11, 138, 0]) for _ in range(n)], dtype=np.uint8)
            want = np.zeros(((n + 31) // 32) * 32, dtype=np.uint8)
            want[:n] = text == 10
            want = np.packbits(want, bitorder="little").view("<u4")
            for head in range(16):
                assert np.array_equal(grepsim.ends_words(text, 10, head), want), (n, dense, head)


def test_worked_example_of_the_header():
    keys = [b"ab", b"b\n"]
    text = b"xab\nq\n\nb"
    corpus = np.frombuffer(text, dtype=np.uint8)
    rec, dro = grepsim.records(corpus, [0, len(text)], b"\n")
    assert rec.tolist() == [0, 4, 6, 7, 8] and dro.tolist() == [0, 4]
    o = orc.AC.compile(keys)
    h = np.diff(o.match_batch(corpus, rec)[1].astype(np.int64))
    assert h.tolist() == [2, 0, 0, 0]  # ab and b\n in the first record; b\n needs the delimiter the last record lacks
    kept, out, doo = grepsim.grep(h, rec, corpus, False)
    assert kept.tolist() == [0] and out.tobytes() == b"xab\n" and doo.tolist() == [0, 4]
    kept, out, doo = grepsim.grep(h, rec, corpus, True)
    assert kept.tolist() == [1, 2, 3] and out.tobytes() == b"q\n\nb" and doo.tolist() == [0, 2, 3, 4]


def _same(a, b):
    return all(np.array_equal(x, y) and x.dtype == y.dtype for x, y in zip(a, b))


def test_kernel_model_against_the_plain_model_on_random_small_alphabets():
    rng = random.Random(20250)
    seen = set()
    for trial in range(3000):
        if trial % 50 == 0:
            alpha = "ab\n" + "c"[: rng.randint(0, 1)]
            keys = sorted({"".join(rng.choice(alpha) for _ in range(rng.randint(1, 3))) for _ in range(rng.randint(1, 4))})
            o = orc.AC.compile([k.encode() for k in keys])
        weights = rng.choice([(4, 4, 1, 1), (1, 1, 3, 1), (3, 1, 1, 3), (1, 1, 0, 6)])
        docs = [("".join(rng.choices("ab\nc", weights)[0] for _ in range(rng.choice([0, 0, 1, 2, 3, 5, 9, 14])))).encode()
                for _ in range(rng.randint(0, 6))]
        text = b"".join(docs)
        corpus = np.frombuffer(text, dtype=np.uint8)
        offs = np.cumsum([0] + [len(d) for d in docs]).astype(np.uint64)
        hits_of = lambda off: np.diff(o.match_batch(corpus, off)[1].astype(np.int64))  # noqa: E731
        want_rec = grepsim.records(corpus, offs, b"\n")
        R = want_rec[0].size - 1
        # what the batch holds
        for d, doc in enumerate(docs):
            if b"\n\n" in doc:
                seen.add("adjacent delimiters")
            if doc.endswith(b"\n"):
                seen.add("a delimiter at a document's last byte")
            if doc and not doc.endswith(b"\n"):
                seen.add("a document without a trailing delimiter")
            if not doc and len(docs) >= 3 and text:
                seen.add("an empty document %s" % ("first" if d == 0 else "last" if d == len(docs) - 1 else "in the middle"))
        for invert in (False, True):
            # records, then grep over the records
            got = grepsim.kernel_model(corpus, offs, b"\n", hits_of, invert, head=trial % 16)
            assert _same(got[:2], want_rec), (keys, docs)
            h = hits_of(want_rec[0])
            assert _same(got[2:5], grepsim.grep(h, want_rec[0], corpus, invert)), (keys, docs, invert)
            keep = (h >= 1) != invert
            if R:
                seen.add("all kept" if keep.all() else "none kept" if not keep.any() else "some kept")
                if not keep[0]:
                    seen.add("a dropped run at the first document")
                if not keep[-1]:
                    seen.add("a dropped run at the last document")
            if invert and R:
                seen.add("invert")
            # grep over the documents themselves: empty documents take part
            hd = hits_of(offs)
            kept, out, doo, n_runs = grepsim.model_grep(hd, offs, corpus, invert)
            assert _same((kept, out, doo), grepsim.grep(hd, offs, corpus, invert)), (keys, docs, invert)
            keep = (hd >= 1) != invert
            for d in range(1, len(docs) - 1):
                if keep[d] and not docs[d] and not keep[d - 1] and not keep[d + 1] and docs[d - 1] and docs[d + 1]:
                    seen.add("adjacent dropped runs separated by one kept empty document")
                    assert n_runs >= 2
    assert seen == {"adjacent delimiters", "a delimiter at a document's last byte", "a document without a trailing delimiter",
                    "an empty document first", "an empty document in the middle", "an empty document last", "all kept",
                    "none kept", "some kept", "a dropped run at the first document", "a dropped run at the last document",
                    "adjacent dropped runs separated by one kept empty document", "invert"}, seen


def test_cpp_grep_example_compiles(tmp_path):
    from test_gpu_grep_cpp import build_spec_grep

    build_spec_grep(tmp_path)
