"""CPU tests of the document counts (aha_ac_doc_counts_batch, aha_ac_doc_counts_batch_device): exported, declared and bound;
their argument checks, which come before any device work -- so they hold on a host-only handle; and the numpy statement of
the contract (doccountsim) on the oracle's hits."""
import ctypes as C
import json
import os
import random
import re

import numpy as np
import pytest

import doccountsim
import pyoracle as orc
from aha_amd import AC, AhaError, BitArray
from aha_amd import _native as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("aha_ac_doc_counts_batch", "aha_ac_doc_counts_batch_device")


def test_doc_counts_symbols_exported_declared_and_bound():
    hdr = open(os.path.join(ROOT, "include", "aha_hip.h")).read()
    listed = open(os.path.join(ROOT, "aha_amd", "csrc", "exports.map")).read()
    crystal = open(os.path.join(ROOT, "bindings", "crystal", "aha_hip.cr")).read()
    L = C.CDLL(N.LIB_PATH)
    for name in ENTRIES:
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert re.search(r"^\s+%s;" % name, listed, re.M), name
        assert name in N.SIGNATURES and hasattr(L, name), name
        assert re.search(r"^\s*fun %s\(" % name, crystal, re.M), name
    assert re.search(r"}\s*aha_key_count;", hdr) and C.sizeof(N.aha_key_count) == 8
    assert N.lib().aha_abi_version() == 8  # a pure addition


def _params(**kw):
    p = N.aha_match_params()
    p.struct_size = C.sizeof(N.aha_match_params)
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def _both(m, p, n=True):
    """rc of the host entry and of the device entry on the same arguments (a host-only handle)"""
    corpus = np.frombuffer(b"ushers", dtype=np.uint8).copy()
    offs = np.array([0, corpus.size], dtype=np.uint64)
    out = np.zeros(16, dtype=doccountsim.KEY_COUNT_DTYPE)
    np_ = C.c_uint64(7)
    pn = C.byref(np_) if n else None
    L = N.lib()
    rc_h = L.aha_ac_doc_counts_batch(m._h, corpus.ctypes.data, offs.ctypes.data, 1, C.byref(p), out.ctypes.data, 16, None, pn, None)
    rc_d = L.aha_ac_doc_counts_batch_device(m._h, corpus.ctypes.data, offs.ctypes.data, 1, corpus.size, C.byref(p),
                                            out.ctypes.data, 16, None, pn, None, None)
    return rc_h, rc_d


def test_doc_counts_host_only_handle_has_no_device():
    m = AC.compile(["he", "she", "hers"], host_only=True)
    assert _both(m, _params()) == (N.AHA_E_NO_DEVICE, N.AHA_E_NO_DEVICE)
    assert _both(m, _params(char_offsets=1)) == (N.AHA_E_NO_DEVICE, N.AHA_E_NO_DEVICE)
    with pytest.raises(AhaError) as e:
        m.doc_counts("ushers")
    assert e.value.code == N.AHA_E_NO_DEVICE


def test_doc_counts_rejects_longest():
    m = AC.compile(["he", "she", "hers"], host_only=True)
    for longest in (1, 2):
        assert _both(m, _params(longest=longest)) == (N.AHA_E_INVALID, N.AHA_E_INVALID)


def test_doc_counts_rejects_large_separator():
    m = AC.compile(["he", "she", "hers"], host_only=True)
    assert _both(m, _params(sep_size=257)) == (N.AHA_E_SEP_SIZE, N.AHA_E_SEP_SIZE)
    with pytest.raises(AhaError) as e:
        m.doc_counts_batch(b"ushers", [0, 6], sep=BitArray(300))
    assert e.value.code == N.AHA_E_SEP_SIZE


def test_doc_counts_rejects_null_n_pairs_and_null_handle():
    m = AC.compile(["he", "she", "hers"], host_only=True)
    assert _both(m, _params(), n=False) == (N.AHA_E_INVALID, N.AHA_E_INVALID)
    L = N.lib()
    n = C.c_uint64(0)
    assert L.aha_ac_doc_counts_batch(None, None, None, 0, None, None, 0, None, C.byref(n), None) == N.AHA_E_INVALID
    assert L.aha_ac_doc_counts_batch_device(None, None, None, 0, 0, None, None, 0, None, C.byref(n), None, None) == N.AHA_E_INVALID


def _sim_on_oracle(keys, docs):
    o = orc.AC.compile(keys)
    corpus = np.frombuffer(b"".join(docs), dtype=np.uint8).copy()
    offs = np.cumsum([0] + [len(d) for d in docs]).astype(np.uint64)
    hits, dho = o.match_batch(corpus, offs)
    v = np.asarray(hits["value"], dtype=np.int64)
    pairs, dpo = doccountsim.doc_counts(v, dho)
    doccountsim.check_invariants(pairs, dpo, v, dho, len(keys))
    return pairs, dpo


def test_doccountsim_on_reference_kats():
    kats = json.load(open(os.path.join(ROOT, "tests", "golden", "reference_kats.json"), encoding="utf-8"))["ac_match"]
    assert kats
    for kat in kats:
        text = kat["text"].encode()
        _sim_on_oracle([k.encode() for k in kat["keys"]], [text, b"", text + text])


def test_doccountsim_on_random_key_sets():
    import test_gpu_doc_counts as g

    for name in sorted(g.KEYSETS):
        rng = random.Random(name)
        keys = g.KEYSETS[name](rng)
        pairs, dpo = _sim_on_oracle(keys, g._docs(rng, keys, 12, 1500, 0.5))
        assert pairs.size and dpo[-1] == pairs.size
    pairs, dpo = _sim_on_oracle([b"he", b"she", b"his", b"hers"], [b"ushers", b"", b"his hers she he"])
    assert pairs.tolist() == [(0, 1), (1, 1), (3, 1), (0, 3), (1, 1), (2, 1), (3, 1)] and dpo.tolist() == [0, 3, 3, 7]


def test_cpp_doc_counts_example_compiles(tmp_path):
    from test_gpu_doc_counts_cpp import build_spec_doc_counts

    build_spec_doc_counts(tmp_path)
