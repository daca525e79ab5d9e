"""CPU tests of the class-counts calls (aha_classes_*, aha_ac_class_counts_batch*): declared, exported, listed and bound; the
table's validation and the entries' argument checks, which come before any device work -- so they hold on a host-only handle;
the device arithmetic as classsim.kernel_model states it (slices, owners, the choice of form, LDS slots, flushes) against the
plain statement of the contract, on random small-alphabet batches with the oracle's hits per document; and the overflow
predicate on made-up hit offsets."""
import ctypes as C
import os
import random
import re
import subprocess

import numpy as np
import pytest

import classsim
import pyoracle as orc
from aha_amd import AC, AhaError, Classes
from aha_amd import _native as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("aha_classes_create", "aha_classes_free", "aha_ac_class_counts_batch", "aha_ac_class_counts_batch_device")
GUARD = 0x5A5A5A5A
KEYS = ["he", "she", "hers"]


def test_class_counts_symbols_exported_declared_and_bound():
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
        assert name in cpp, name  # (the device entry: named where the host form points to it)
    assert len(re.findall(r"^\s+aha_\w+;", listed, re.M)) == 90
    assert N.lib().aha_abi_version() == 8  # a pure addition
    for method in ("classes", "class_counts_batch", "class_counts_batch_device", "class_counts_corpus", "class_counts"):
        assert callable(getattr(AC, method))
    import aha_amd

    assert "Classes" in aha_amd.__all__ and aha_amd.Classes is Classes


# ---- the table ----------------------------------------------------------------------------------------------------------
def _create(m, ids, offs, n_classes, null_ids=False, null_offs=False, null_out=False, handle=True):
    ids = np.asarray(ids, dtype=np.uint32)
    offs = np.asarray(offs, dtype=np.uint64)
    h = C.c_void_p(0xDEAD)
    rc = N.lib().aha_classes_create(m._h if handle else None, None if null_ids or not ids.size else ids.ctypes.data,
                                    None if null_offs else offs.ctypes.data, n_classes, None if null_out else C.byref(h))
    return rc, h


def test_class_table_validation_on_a_host_only_handle():
    m = AC.compile(KEYS, host_only=True)
    good_ids, good_offs = [0, 0, 1], [0, 1, 3, 3]  # he: {0}; she: {0, 1}; hers: none
    bad = [
        dict(handle=False), dict(null_offs=True),
        dict(offs=[1, 2, 4, 4], ids=[0, 0, 0, 1]),  # offsets[0] != 0
        dict(offs=[0, 3, 1, 3]),  # descending offsets
        dict(n_classes=0), dict(n_classes=65537), dict(n_classes=0xFFFFFFFF),
        dict(n_classes=1),  # a class id >= n_classes
        dict(ids=[0, 1, 0]),  # descending within a key
        dict(ids=[0, 1, 1]),  # a class twice for a key
        dict(null_ids=True),  # class_ids == NULL with offsets[K] != 0
    ]
    for case in bad:
        kw = dict(ids=good_ids, offs=good_offs, n_classes=2)
        kw.update(case)
        rc, h = _create(m, kw.pop("ids"), kw.pop("offs"), kw.pop("n_classes"), **kw)
        assert rc == N.AHA_E_INVALID and h.value is None, case
    assert _create(m, good_ids, good_offs, 2, null_out=True)[0] == N.AHA_E_INVALID
    # valid tables: empty, single and multiple class lists; the limits of n_classes; no class at all (class_ids may be NULL)
    for ids, offs, n in ((good_ids, good_offs, 2), (good_ids, good_offs, 65536), ([], [0, 0, 0, 0], 1), ([], [0, 0, 0, 0], 7),
                         ([65535, 0, 5, 9], [0, 1, 1, 4], 65536)):
        rc, h = _create(m, ids, offs, n)
        assert rc == N.AHA_OK and h.value, (ids, offs, n)
        N.lib().aha_classes_free(h)
    N.lib().aha_classes_free(None)  # a no-op


def test_class_table_may_be_freed_before_or_after_its_handle():
    m = AC.compile(KEYS, host_only=True)
    t = m.classes([0, (0, 1), None])
    assert isinstance(t, Classes) and t.n_classes == 2 and t.n_keys == 3 and t.names is None
    del t  # before its handle
    t = m.classes([0, (0, 1), None])
    del m  # the handle first
    del t


def test_python_class_specs():
    m = AC.compile(KEYS, host_only=True)
    assert m.classes([None, None, None]).n_classes == 1
    assert m.classes([None, 4, [1, 4]]).n_classes == 5
    assert m.classes([0, 0, 0], n_classes=9).n_classes == 9
    t = m.classes({"pronoun": ["he", b"she", 2], "female": ["she", "hers"]})
    assert t.names == ["pronoun", "female"] and t.n_classes == 2
    t = m.classes({3: [0, 1], 1: ["hers"]})
    assert t.names is None and t.n_classes == 4
    with pytest.raises(ValueError):
        m.classes([0, 1])  # one entry per key
    with pytest.raises(ValueError):
        m.classes({0: [3]})  # no such key
    with pytest.raises(IndexError):
        m.classes({0: ["him"]})
    with pytest.raises(AhaError) as e:
        m.classes([0, 1, 70000])
    assert e.value.code == N.AHA_E_INVALID


# ---- the entries' argument checks ------------------------------------------------------------------------------------------
def _params(**kw):
    p = N.aha_match_params()
    p.struct_size = C.sizeof(N.aha_match_params)
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def _counts_both(m, table, p, flags=0, out=True, offs=True, handle=True, n_docs=2):
    """rc of the host entry and of the device entry on the same arguments; the buffers stay untouched"""
    corpus = np.frombuffer(b"ushershe", dtype=np.uint8).copy()
    doc = np.array([0, 6, 8], dtype=np.uint64)
    buf = np.full(2 * 2 + 16, GUARD, dtype=np.uint32)
    nh = C.c_uint64(7)
    L = N.lib()
    th = table._h if table is not None else None
    h = m._h if handle else None
    po = buf.ctypes.data if out else None
    pd = doc.ctypes.data if offs else None
    before = corpus.copy()
    rc_h = L.aha_ac_class_counts_batch(h, th, corpus.ctypes.data, pd, n_docs, C.byref(p), flags, po, C.byref(nh))
    rc_d = L.aha_ac_class_counts_batch_device(h, th, corpus.ctypes.data, pd, n_docs, corpus.size, C.byref(p), flags, po, C.byref(nh), None)
    assert (buf == GUARD).all() and nh.value == 7 and np.array_equal(corpus, before) and doc.tolist() == [0, 6, 8]
    return rc_h, rc_d


INVALID2 = (N.AHA_E_INVALID, N.AHA_E_INVALID)
NO_DEVICE2 = (N.AHA_E_NO_DEVICE, N.AHA_E_NO_DEVICE)


def test_class_counts_host_only_handle_has_no_device():
    m = AC.compile(KEYS, host_only=True)
    t = m.classes([0, (0, 1), None])
    assert _counts_both(m, t, _params()) == NO_DEVICE2
    assert _counts_both(m, t, _params(sep_size=40)) == NO_DEVICE2  # a separator filter is allowed
    assert _counts_both(m, t, _params(), out=False, n_docs=0) == NO_DEVICE2  # D = 0 needs no out
    for call in (lambda: m.class_counts_batch(b"ushershe", [0, 6, 8], t), lambda: m.class_counts("ushers", t),
                 lambda: m.class_counts(b"ushers", [0, (0, 1), None])):
        with pytest.raises(AhaError) as e:
            call()
        assert e.value.code == N.AHA_E_NO_DEVICE


def test_class_counts_argument_checks_come_before_the_device_check():
    m = AC.compile(KEYS, host_only=True)
    t = m.classes([0, (0, 1), None])
    assert _counts_both(m, t, _params(char_offsets=1)) == INVALID2
    for longest in (1, 2):
        assert _counts_both(m, t, _params(longest=longest)) == INVALID2
    for flags in (1, 2, 0x80000000):
        assert _counts_both(m, t, _params(), flags=flags) == INVALID2
    assert _counts_both(m, None, _params()) == INVALID2  # a NULL table
    other = AC.compile(KEYS, host_only=True)
    assert _counts_both(m, other.classes([0, (0, 1), None]), _params()) == INVALID2  # a table made for another handle
    assert "another handle" in N.lib().aha_last_error(m._h).decode()
    assert _counts_both(m, t, _params(), out=False) == INVALID2  # out == NULL with D > 0
    assert _counts_both(m, t, _params(), offs=False) == INVALID2
    assert _counts_both(m, t, _params(), handle=False) == INVALID2
    assert _counts_both(m, t, _params(sep_size=257)) == (N.AHA_E_SEP_SIZE, N.AHA_E_SEP_SIZE)


# ---- the device arithmetic against the plain statement ---------------------------------------------------------------------
def test_worked_example_of_the_header():
    o = orc.AC.compile(KEYS)
    corpus = np.frombuffer(b"ushershe", dtype=np.uint8)
    hits, dho = o.match_batch(corpus, np.array([0, 6, 8], dtype=np.uint64))
    ids, offs = classsim.pack_classes([[0], [0, 1], []])
    per_doc = classsim.split_hits(hits["value"], dho)
    assert classsim.class_counts(per_doc, ids, offs, 2).tolist() == [[2, 1], [1, 0]]
    got, _ = classsim.kernel_model(hits["value"], dho, ids, offs, 2, 2048, 8192)
    assert got.tolist() == [[2, 1], [1, 0]]


def test_kernel_model_against_the_plain_model_on_random_small_alphabets():
    rng = random.Random(417)
    seen = set()
    for trial in range(3000):
        if trial % 50 == 0:
            alpha = "ab" + "c"[: rng.randint(0, 1)]
            keys = sorted({"".join(rng.choice(alpha) for _ in range(rng.randint(1, 3))) for _ in range(rng.randint(1, 5))})
            o = orc.AC.compile([k.encode() for k in keys])
            C_ = rng.choice([1, 2, 3, 5, 8])
            per_key = [sorted(rng.sample(range(C_), rng.choice([0, 1, 1, min(2, C_), min(3, C_)]))) for _ in keys]
            ids, offs = classsim.pack_classes(per_key)
        docs = [("".join(rng.choice("abcx") for _ in range(rng.choice([0, 0, 1, 2, 3, 5, 9, 14, 40])))).encode()
                for _ in range(rng.randint(0, 7))]
        if trial % 7 == 0:
            docs += [b"x" * rng.randint(0, 3)] * rng.randint(1, 3) + [b"ab"]  # hitless documents between documents with hits
        corpus = np.frombuffer(b"".join(docs), dtype=np.uint8)
        doc = np.cumsum([0] + [len(d) for d in docs]).astype(np.uint64)
        hits, dho = o.match_batch(corpus, doc)
        values = np.asarray(hits["value"], dtype=np.int64)
        want = classsim.class_counts(classsim.split_hits(values, dho), ids, offs, C_)
        # the real constants are arguments: small ones here, so that small cases reach every branch
        slice_hits, table_words = rng.choice([(4, 8), (8, 16), (16, 8), (5, 6), (64, 32)])
        got, s = classsim.kernel_model(values, dho, ids, offs, C_, slice_hits, table_words, threads=rng.choice([4, 8]), wave=4)
        assert got.dtype == want.dtype and got.shape == want.shape and np.array_equal(got, want), (keys, per_key, docs)
        seen |= s
    assert seen >= {"lds", "direct", "a slice inside one document", "a slice over several documents",
                    "documents without hits inside a slice", "a document straddling three slices or more", "a key with no class",
                    "a key with several classes", "a row flushed by several slices", "equal pairs in a wave"}, seen


def test_kernel_model_at_the_real_constants():
    """one document of a repeated key: five slices in one document, a hot slot; and a wide C that no table holds"""
    o = orc.AC.compile([b"a", b"aa", b"aaa"])
    corpus = np.frombuffer(b"a" * 3000, dtype=np.uint8)
    hits, dho = o.match_batch(corpus, np.array([0, 3000], dtype=np.uint64))
    values = np.asarray(hits["value"], dtype=np.int64)
    assert values.size == 3000 + 2999 + 2998
    for C_, per_key in ((3, [[0], [1], [0, 2]]), (8193, [[8192], [], [0, 8192]])):
        ids, offs = classsim.pack_classes(per_key)
        got, s = classsim.kernel_model(values, dho, ids, offs, C_, 2048, 8192)
        assert np.array_equal(got, classsim.class_counts([values], ids, offs, C_))
        assert ("direct" in s) == (C_ == 8193) and ("lds" in s) == (C_ == 3)
        assert "a document straddling three slices or more" in s


# ---- the overflow predicate and the C++ example --------------------------------------------------------------------------
def test_overflow_predicate_on_made_up_hit_offsets(tmp_path):
    exe = str(tmp_path / "spec_class_overflow")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", os.path.join(ROOT, "tests", "cpp", "spec_class_overflow.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "FAIL" not in r.stdout, r.stdout + r.stderr
    assert r.stdout.count("ok  ") >= 10


def test_cpp_class_counts_example_compiles(tmp_path):
    from test_gpu_class_counts_cpp import build_spec_class_counts

    build_spec_class_counts(tmp_path)
