"""CPU tests of the count entry points (aha_ac_count_batch, aha_ac_count_batch_device): exported and declared, and their
argument checks, which come before any device work -- so they hold on a host-only handle."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from aha_amd import AC, AhaError, BitArray
from aha_amd import _native as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("aha_ac_count_batch", "aha_ac_count_batch_device")


def test_count_symbols_exported_and_declared():
    hdr = open(os.path.join(ROOT, "include", "aha_hip.h")).read()
    listed = open(os.path.join(ROOT, "aha_amd", "csrc", "exports.map")).read()
    L = C.CDLL(N.LIB_PATH)
    for name in ENTRIES:
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert re.search(r"^\s+%s;" % name, listed, re.M), name
        assert name in N.SIGNATURES and hasattr(L, name), name
    assert re.search(r"#define AHA_COUNT_ACCUMULATE 1u", hdr) and N.AHA_COUNT_ACCUMULATE == 1
    assert N.lib().aha_abi_version() == 8  # a pure addition


def _params(**kw):
    p = N.aha_match_params()
    p.struct_size = C.sizeof(N.aha_match_params)
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def _both(m, p, n=True, flags=0):
    """rc of the host entry and of the device entry on the same arguments (a host-only handle)"""
    corpus = np.frombuffer(b"ushers", dtype=np.uint8).copy()
    offs = np.array([0, corpus.size], dtype=np.uint64)
    kc = np.zeros(m.n_keys, dtype=np.uint64)
    nh = C.c_uint64(7)
    pn = C.byref(nh) if n else None
    L = N.lib()
    rc_h = L.aha_ac_count_batch(m._h, corpus.ctypes.data, offs.ctypes.data, 1, C.byref(p), flags, kc.ctypes.data, None, pn)
    rc_d = L.aha_ac_count_batch_device(m._h, corpus.ctypes.data, offs.ctypes.data, 1, corpus.size, C.byref(p), flags,
                                       kc.ctypes.data, None, pn, None)
    return rc_h, rc_d


def test_count_host_only_handle_has_no_device():
    m = AC.compile(["he", "she", "hers"], host_only=True)
    assert _both(m, _params()) == (N.AHA_E_NO_DEVICE, N.AHA_E_NO_DEVICE)
    assert _both(m, _params(char_offsets=1)) == (N.AHA_E_NO_DEVICE, N.AHA_E_NO_DEVICE)
    with pytest.raises(AhaError) as e:
        m.count("ushers")
    assert e.value.code == N.AHA_E_NO_DEVICE


def test_count_rejects_longest():
    m = AC.compile(["he", "she", "hers"], host_only=True)
    for longest in (1, 2):
        assert _both(m, _params(longest=longest)) == (N.AHA_E_INVALID, N.AHA_E_INVALID)


def test_count_rejects_large_separator():
    m = AC.compile(["he", "she", "hers"], host_only=True)
    assert _both(m, _params(sep_size=257)) == (N.AHA_E_SEP_SIZE, N.AHA_E_SEP_SIZE)
    with pytest.raises(AhaError) as e:
        m.count_batch(b"ushers", [0, 6], sep=BitArray(300))
    assert e.value.code == N.AHA_E_SEP_SIZE


def test_count_rejects_null_n_hits_and_unknown_flags():
    m = AC.compile(["he", "she", "hers"], host_only=True)
    assert _both(m, _params(), n=False) == (N.AHA_E_INVALID, N.AHA_E_INVALID)
    assert _both(m, _params(), flags=2) == (N.AHA_E_INVALID, N.AHA_E_INVALID)
    L = N.lib()
    nh = C.c_uint64(0)
    assert L.aha_ac_count_batch(None, None, None, 0, None, 0, None, None, C.byref(nh)) == N.AHA_E_INVALID


def test_cpp_count_example_compiles(tmp_path):
    from test_gpu_count_cpp import build_spec_count

    build_spec_count(tmp_path)
