"""CPU tests of the select calls (aha_ac_select_batch, aha_ac_select_batch_device): exported, declared and bound; their
argument checks, which come before any device work -- so they hold on a host-only handle; the greedy statement of the contract
(selectsim) on the oracle's hits against an independent formulation (the L array and runs, as the kernels work); and the host
side arithmetic of AC.select on str and of AC.replace."""
import ctypes as C
import json
import os
import random
import re

import numpy as np
import pytest

import pyoracle as orc
import selectsim
from aha_amd import AC, AhaError, BitArray
from aha_amd import _native as N
from aha_amd import ac as acmod

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("aha_ac_select_batch", "aha_ac_select_batch_device")


def test_select_symbols_exported_declared_and_bound():
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
    """rc of the host entry and of the device entry on the same arguments (a host-only handle); the buffers stay untouched"""
    corpus = np.frombuffer(b"ushers", dtype=np.uint8).copy()
    offs = np.array([0, corpus.size], dtype=np.uint64)
    out = np.full(16 * 3, 0x5A5A5A5A, dtype=np.int32)
    dso = np.full(2, 0x5A5A5A5A, dtype=np.uint64)
    ns = C.c_uint64(7)
    pn = C.byref(ns) if n else None
    L = N.lib()
    rc_h = L.aha_ac_select_batch(m._h, corpus.ctypes.data, offs.ctypes.data, 1, C.byref(p), flags, out.ctypes.data, 16,
                                 dso.ctypes.data, pn, None)
    rc_d = L.aha_ac_select_batch_device(m._h, corpus.ctypes.data, offs.ctypes.data, 1, corpus.size, C.byref(p), flags,
                                        out.ctypes.data, 16, dso.ctypes.data, pn, None, None)
    assert (out == 0x5A5A5A5A).all() and (dso == 0x5A5A5A5A).all()
    return rc_h, rc_d


def test_select_host_only_handle_has_no_device():
    m = AC.compile(["he", "she", "hers"], host_only=True)
    assert _both(m, _params()) == (N.AHA_E_NO_DEVICE, N.AHA_E_NO_DEVICE)
    for call in (lambda: m.select("ushers"), lambda: m.select(b"ushers"), lambda: m.replace("ushers", {0: "x"}),
                 lambda: m.select_batch(b"ushers", [0, 6])):
        with pytest.raises(AhaError) as e:
            call()
        assert e.value.code == N.AHA_E_NO_DEVICE


def test_select_rejects_char_offsets_longest_and_flags():
    m = AC.compile(["he", "she", "hers"], host_only=True)
    assert _both(m, _params(char_offsets=1)) == (N.AHA_E_INVALID, N.AHA_E_INVALID)
    for longest in (1, 2):
        assert _both(m, _params(longest=longest)) == (N.AHA_E_INVALID, N.AHA_E_INVALID)
    for flags in (1, 2, 0x80000000):
        assert _both(m, _params(), flags=flags) == (N.AHA_E_INVALID, N.AHA_E_INVALID)


def test_select_rejects_large_separator():
    m = AC.compile(["he", "she", "hers"], host_only=True)
    assert _both(m, _params(sep_size=257)) == (N.AHA_E_SEP_SIZE, N.AHA_E_SEP_SIZE)
    with pytest.raises(AhaError) as e:
        m.select_batch(b"ushers", [0, 6], sep=BitArray(300))
    assert e.value.code == N.AHA_E_SEP_SIZE


def test_select_rejects_null_n_selected_and_null_handle():
    m = AC.compile(["he", "she", "hers"], host_only=True)
    assert _both(m, _params(), n=False) == (N.AHA_E_INVALID, N.AHA_E_INVALID)
    L = N.lib()
    n = C.c_uint64(0)
    assert L.aha_ac_select_batch(None, None, None, 0, None, 0, None, 0, None, C.byref(n), None) == N.AHA_E_INVALID
    assert L.aha_ac_select_batch_device(None, None, None, 0, 0, None, 0, None, 0, None, C.byref(n), None, None) == N.AHA_E_INVALID


# ---- selectsim against an independent formulation ------------------------------------------------------------------------
def _by_runs(hits, n):
    """one document of n bytes the way the kernels work: L[p] = the longest hit that starts at p, the cover of the longest
    spans, one walk per run (a maximal covered stretch)"""
    L = [None] * n
    for s, e, v in hits:
        if L[s] is None or e - s > L[s][0]:
            L[s] = (e - s, v)
    cover = [False] * n
    for p in range(n):
        if L[p]:
            for j in range(p, p + L[p][0]):
                cover[j] = True
    out = []
    for p0 in range(n):
        if not L[p0] or (p0 and cover[p0 - 1]):
            continue
        p = p0
        while p < n and cover[p]:
            if L[p]:
                out.append((p, p + L[p][0], L[p][1]))
                p += L[p][0]
            else:
                p += 1
    return out


def _oracle_docs(keys, docs, sep=None):
    """the oracle's hits of every document, as one list and its offsets"""
    o = orc.AC.compile(keys)
    hits, dho = [], [0]
    for d in docs:
        h = o.match(d, chars=False, sep=sep)
        hits += [(int(s), int(e), int(v)) for s, e, v in zip(h["start"], h["end"], h["value"])] if h.size else []
        dho.append(len(hits))
    arr = np.zeros(len(hits), dtype=selectsim.HIT_DTYPE)
    for i, t in enumerate(hits):
        arr[i] = t
    return arr, np.array(dho, dtype=np.uint64)


def _sim_against_runs(keys, docs, sep=None):
    hits, dho = _oracle_docs(keys, docs, sep)
    sel, dso = selectsim.select(hits, dho)
    selectsim.check_invariants(sel, dso, hits, dho)
    not_first = 0
    for d, doc in enumerate(docs):
        H = [tuple(x) for x in hits[int(dho[d]):int(dho[d + 1])].tolist()]
        S = [tuple(x) for x in sel[int(dso[d]):int(dso[d + 1])].tolist()]
        assert S == _by_runs(H, len(doc)), (keys, doc)
        first_at_end = {}
        for s, e, v in H:  # (the oracle lists the hits of one end with the END state's own key -- the longest -- first)
            first_at_end.setdefault(e, (s, e, v))
        not_first += sum(1 for h in S if first_at_end[h[1]] != h)
    return sel, dso, not_first


def test_selectsim_on_reference_kats():
    kats = json.load(open(os.path.join(ROOT, "tests", "golden", "reference_kats.json"), encoding="utf-8"))["ac_match"]
    assert kats
    for kat in kats:
        text = kat["text"].encode()
        sep = (kat["sep"]["size"], kat["sep"]["set"]) if kat["sep"] is not None else None
        _sim_against_runs([k.encode() for k in kat["keys"]], [text, b"", text + text], sep)


def test_selectsim_chain_case_and_nested_keys():
    sel, dso, not_first = _sim_against_runs([b"ab", b"bcd", b"cd", b"d"], [b"abcd", b"", b"abcdabcd"])
    assert sel.tolist()[:2] == [(0, 2, 0), (2, 4, 2)] and dso.tolist() == [0, 2, 2, 6]
    assert not_first == 3  # cd is behind bcd at its end, every time
    keys = [b"a" * i for i in range(1, 24)]
    sel, dso, _ = _sim_against_runs(keys, [b"a" * 50, b"a" * 23 + b"b" + b"a" * 5, b"b"])
    assert sel.tolist() == [(0, 23, 22), (23, 46, 22), (46, 50, 3), (0, 23, 22), (24, 29, 4)] and dso.tolist() == [0, 3, 5, 5]
    assert selectsim.select_doc([(0, 2, 0), (1, 3, 1), (2, 3, 2)]) == [(0, 2, 0), (2, 3, 2)]


def test_selectsim_on_random_small_alphabets():
    rng = random.Random(20240)
    not_first = 0
    sep = (128, [i for i in range(128) if chr(i) not in "ab"])  # (a neighbour a or b drops a hit, c and d do not)
    for trial in range(150):
        alpha = "abcd"[: rng.randint(2, 4)]
        keys = sorted({"".join(rng.choice(alpha) for _ in range(rng.randint(1, 5))) for _ in range(rng.randint(1, 9))})
        keys = [k.encode() for k in keys]
        docs = [("".join(rng.choice(alpha) for _ in range(rng.randint(0, 40)))).encode() for _ in range(4)]
        not_first += _sim_against_runs(keys, docs)[2]
        _sim_against_runs(keys, docs, sep)
    assert not_first > 0  # (the shortcut "one span per event" would not do)


# ---- the host-side arithmetic of AC.select (str) and AC.replace ----------------------------------------------------------
def _char_hits_plain(text, hits):
    """byte offsets over text.encode() as character offsets, the plain way: decode the prefix"""
    b = text.encode()
    return [(len(b[:s].decode()), len(b[:e].decode()), v) for s, e, v in hits]


def _replace_plain(b, sel, repl):
    out, at = b"", 0
    for s, e, v in sel:
        r = repl.get(v) if isinstance(repl, dict) else repl[v]
        if r is None:
            continue
        out += b[at:s] + (r.encode() if isinstance(r, str) else r)
        at = e
    return out + b[at:]


def test_select_str_offsets_and_replace_arithmetic():
    keys = ["我", "我是", "是中", "he", "hers", "é", "éa", "🙂", "a🙂"]
    texts = ["我是中国人 ushers", "", "éaé🙂a🙂héhers我", "plain ascii hers", "🙂🙂我是"]
    for text in texts:
        b = text.encode()
        hits, dho = _oracle_docs([k.encode() for k in keys], [b])
        sel, _ = selectsim.select(hits, dho)
        triples = [tuple(x) for x in sel.tolist()]
        got = acmod.char_offsets_of(b, sel)
        assert [tuple(x) for x in got.tolist()] == _char_hits_plain(text, triples)
        for s, e, v in got.tolist():
            assert text[s:e] == keys[v]
        repl_map = {0: "I", 1: "I am", 3: b"HE", 7: "", 5: None}
        repl_seq = ["<%d>" % i for i in range(len(keys))]
        for repl in (repl_map, repl_seq, {}):
            want = _replace_plain(b, triples, repl)
            assert acmod.substitute(b, sel, repl, len(keys)) == want
            want.decode()  # (whole characters in, whole characters out)
    sel = np.array([(0, 2, 0)], dtype=selectsim.HIT_DTYPE)
    with pytest.raises(ValueError):
        acmod.substitute(b"he", sel, ["only one"], 9)


def test_cpp_select_example_compiles(tmp_path):
    from test_gpu_select_cpp import build_spec_select

    build_spec_select(tmp_path)
