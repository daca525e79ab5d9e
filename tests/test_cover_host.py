"""CPU tests of the cover calls (aha_ac_cover_batch, aha_ac_cover_batch_device): exported, declared and bound; their argument
checks, which come before any device work -- so they hold on a host-only handle; the numpy statement of the contract
(coversim) on the oracle's hits; and the premise of the kernels, pinned on the oracle: of the hits of one END position the
first has the smallest start."""
import ctypes as C
import json
import os
import random
import re

import numpy as np
import pytest

import coversim
import pyoracle as orc
from aha_amd import AC, AhaError, BitArray
from aha_amd import _native as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("aha_ac_cover_batch", "aha_ac_cover_batch_device")
SEP_BITS = [32, 0]


def test_cover_symbols_exported_declared_and_bound():
    hdr = open(os.path.join(ROOT, "include", "aha_hip.h")).read()
    listed = open(os.path.join(ROOT, "aha_amd", "csrc", "exports.map")).read()
    crystal = open(os.path.join(ROOT, "bindings", "crystal", "aha_hip.cr")).read()
    L = C.CDLL(N.LIB_PATH)
    for name in ENTRIES:
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert re.search(r"^\s+%s;" % name, listed, re.M), name
        assert name in N.SIGNATURES and hasattr(L, name), name
        assert re.search(r"^\s*fun %s\(" % name, crystal, re.M), name
    assert N.lib().aha_abi_version() == 8  # a pure addition


def _params(**kw):
    p = N.aha_match_params()
    p.struct_size = C.sizeof(N.aha_match_params)
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def _both(m, p, n=True, flags=0):
    """rc of the host entry and of the device entry on the same arguments (a host-only handle); no buffer is written"""
    corpus = np.frombuffer(b"ushers", dtype=np.uint8).copy()
    offs = np.array([0, corpus.size], dtype=np.uint64)
    mask = np.full(1, 0x5A5A5A5A, dtype=np.uint32)
    red = np.full(6, 0x5A, dtype=np.uint8)
    cov = np.full(1, 0x5A, dtype=np.uint64)
    nc = C.c_uint64(7)
    pn = C.byref(nc) if n else None
    L = N.lib()
    rc_h = L.aha_ac_cover_batch(m._h, corpus.ctypes.data, offs.ctypes.data, 1, C.byref(p), flags, mask.ctypes.data, red.ctypes.data,
                                0x2A, cov.ctypes.data, pn, None)
    rc_d = L.aha_ac_cover_batch_device(m._h, corpus.ctypes.data, offs.ctypes.data, 1, corpus.size, C.byref(p), flags,
                                       mask.ctypes.data, red.ctypes.data, 0x2A, cov.ctypes.data, pn, None, None)
    assert mask[0] == 0x5A5A5A5A and (red == 0x5A).all() and cov[0] == 0x5A  # a call that fails writes none of the buffers
    return rc_h, rc_d


def test_cover_host_only_handle_has_no_device():
    m = AC.compile(["he", "she", "hers"], host_only=True)
    assert _both(m, _params()) == (N.AHA_E_NO_DEVICE, N.AHA_E_NO_DEVICE)
    assert _both(m, _params(char_offsets=1)) == (N.AHA_E_NO_DEVICE, N.AHA_E_NO_DEVICE)
    for call in (lambda: m.cover("ushers"), lambda: m.redact("ushers"), lambda: m.redact(b"ushers"),
                 lambda: m.cover_batch(b"ushers", [0, 6]), lambda: m.redact_batch(b"ushers", [0, 6])):
        with pytest.raises(AhaError) as e:
            call()
        assert e.value.code == N.AHA_E_NO_DEVICE


def test_cover_rejects_longest_flags_and_large_separator():
    m = AC.compile(["he", "she", "hers"], host_only=True)
    for longest in (1, 2):
        assert _both(m, _params(longest=longest)) == (N.AHA_E_INVALID, N.AHA_E_INVALID)
    for flags in (1, 2, 0x80000000):
        assert _both(m, _params(), flags=flags) == (N.AHA_E_INVALID, N.AHA_E_INVALID)
    assert _both(m, _params(sep_size=257)) == (N.AHA_E_SEP_SIZE, N.AHA_E_SEP_SIZE)
    with pytest.raises(AhaError) as e:
        m.cover_batch(b"ushers", [0, 6], sep=BitArray(300))
    assert e.value.code == N.AHA_E_SEP_SIZE


def test_cover_rejects_null_n_covered_and_null_handle():
    m = AC.compile(["he", "she", "hers"], host_only=True)
    assert _both(m, _params(), n=False) == (N.AHA_E_INVALID, N.AHA_E_INVALID)
    L = N.lib()
    n = C.c_uint64(0)
    assert L.aha_ac_cover_batch(None, None, None, 0, None, 0, None, None, 0, None, C.byref(n), None) == N.AHA_E_INVALID
    assert L.aha_ac_cover_batch_device(None, None, None, 0, 0, None, 0, None, None, 0, None, C.byref(n), None, None) == N.AHA_E_INVALID


def _oracle_hits(o, docs, sep=None):
    """(start, end, value, doc hit offsets) of the oracle's match of every document; sep = (size, set bits) or None"""
    parts, dho = [], [0]
    for d in docs:
        h = o.match(bytes(d), chars=False, sep=sep)
        parts.append(h)
        dho.append(dho[-1] + h.size)
    h = np.concatenate(parts) if parts else np.zeros(0, dtype=[("start", "<i4"), ("end", "<i4"), ("value", "<i4")])
    return h["start"].astype(np.int64), h["end"].astype(np.int64), h["value"].astype(np.int64), np.array(dho, dtype=np.uint64)


def _sim_on_oracle(keys, docs, sep=None, fill=0x2A):
    o = orc.AC.compile(keys)
    corpus = np.frombuffer(b"".join(docs), dtype=np.uint8).copy()
    offs = np.cumsum([0] + [len(d) for d in docs]).astype(np.uint64)
    s, e, _, dho = _oracle_hits(o, docs, sep)
    mask, red, dc, nc = coversim.cover_all(s, e, corpus, offs, dho, fill)
    coversim.check_invariants(mask, red, dc, nc, corpus, offs, s, e, dho, fill)
    # the definition, byte by byte
    want = np.zeros(corpus.size, dtype=bool)
    doc = np.repeat(np.arange(len(docs)), np.diff(dho.astype(np.int64)))
    for a, b, d in zip(s, e, doc):
        want[int(offs[d]) + a:int(offs[d]) + b] = True
    assert np.array_equal(coversim.unpack(mask, corpus.size), want)
    return mask, red, dc, nc


def test_coversim_on_reference_kats():
    kats = json.load(open(os.path.join(ROOT, "tests", "golden", "reference_kats.json"), encoding="utf-8"))["ac_match"]
    assert kats
    for kat in kats:
        text = kat["text"].encode()
        sep = (kat["sep"]["size"], kat["sep"]["set"]) if kat["sep"] is not None else None
        _sim_on_oracle([k.encode() for k in kat["keys"]], [text, b"", text + text], sep)
    mask, red, dc, nc = _sim_on_oracle([b"he", b"she", b"his", b"hers"], [b"ushers", b"", b"his hers she he"])
    assert red.tobytes() == b"u*****" + b"*** **** *** **" and dc.tolist() == [5, 0, 12] and nc == 17
    assert mask.tolist() == [sum(1 << j for j, c in enumerate("u*****" "*** **** *** **") if c == "*")]  # bit j = byte j


def test_coversim_on_random_key_sets():
    import test_gpu_doc_counts as g

    bits = [i for i in range(40) if i not in SEP_BITS]
    for name in sorted(g.KEYSETS):
        rng = random.Random(name)
        keys = g.KEYSETS[name](rng)
        docs = g._docs(rng, keys, 12, 1500, 0.5)
        _, _, dc, nc = _sim_on_oracle(keys, docs)
        assert nc and dc.sum() == nc
        _sim_on_oracle(keys, docs, (40, bits), fill=0)


def test_first_hit_of_an_end_position_has_the_smallest_start():
    """The kernels' premise (one span per event): in the oracle's order the hits of one END position stand together and
    the first of them -- with a separator filter the first that survives -- starts leftmost, so its span holds the others."""
    import test_gpu_doc_counts as g

    bits = [i for i in range(40) if i not in SEP_BITS]
    checked = 0
    for name in sorted(g.KEYSETS):
        rng = random.Random("premise/" + name)
        keys = g.KEYSETS[name](rng)
        o = orc.AC.compile(keys)
        for doc in g._docs(rng, keys, 10, 2000, 0.6) + [b"a" * 300, ("我" * 90).encode()]:
            for sep in (None, (40, bits)):
                h = o.match(doc, chars=False, sep=sep)
                if not h.size:
                    continue
                end, start = h["end"].astype(np.int64), h["start"].astype(np.int64)
                assert (np.diff(end) >= 0).all()  # the hits of one END position are one run
                first = np.flatnonzero(np.concatenate([[True], end[1:] != end[:-1]]))
                run_min = np.minimum.reduceat(start, first)
                assert np.array_equal(start[first], run_min), (name, sep)
                checked += int((np.diff(np.append(first, end.size)) > 1).sum())
    assert checked > 1000  # (runs of more than one hit: the nested key set has them at nearly every position)


def test_redact_str_replaces_whole_characters():
    # (host-only: the calls fail before the host-side character mapping; the mapping itself is checked on the GPU)
    m = AC.compile(["我是"], host_only=True)
    with pytest.raises(AhaError):
        m.redact("我是中国人")


def test_cpp_cover_example_compiles(tmp_path):
    from test_gpu_cover_cpp import build_spec_cover

    build_spec_cover(tmp_path)
