"""CPU tests of the replace calls (aha_repl_create, aha_repl_free, aha_ac_replace_batch, aha_ac_replace_batch_device): exported,
declared and bound; the table's validation; the entries' argument checks, which come before any device work -- so they hold
on a host-only handle, where a table is made with a host copy only; and the contract in plain Python (replacesim over selectsim
over the oracle's hits) against AC.replace's `substitute` and against an independent numpy statement of the kernels' arithmetic
(A, delta, the exclusive scan, O, the last-j tie rule, the output-driven gather)."""
import ctypes as C
import os
import random
import re

import numpy as np
import pytest

import pyoracle as orc
import replacesim
import selectsim
from aha_amd import AC, AhaError
from aha_amd import _native as N
from aha_amd import ac as acmod

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("aha_repl_create", "aha_repl_free", "aha_ac_replace_batch", "aha_ac_replace_batch_device")
GUARD8, GUARD64 = 0xA5, 0x5A5A5A5A5A5A5A5A
KEYS = ["he", "she", "hers"]


def test_replace_symbols_exported_declared_and_bound():
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


def _create(m, blob, offs, keep=None):
    """(rc, handle) of aha_repl_create on raw arrays"""
    blob = np.frombuffer(bytes(blob), dtype=np.uint8).copy() if blob is not None else None
    offs = np.array(offs, dtype=np.uint64) if offs is not None else None
    keep = np.array(keep, dtype=np.uint32) if keep is not None else None
    h = C.c_void_p(0xDEAD)
    rc = N.lib().aha_repl_create(m._h if m is not None else None, blob.ctypes.data if blob is not None and blob.size else None,
                                 offs.ctypes.data if offs is not None else None,
                                 keep.ctypes.data if keep is not None else None, C.byref(h))
    return rc, h


def test_repl_create_validation():
    m = AC.compile(KEYS, host_only=True)
    L = N.lib()
    rc, h = _create(m, b"abcdef", [0, 1, 3, 6])
    assert rc == N.AHA_OK and h.value
    L.aha_repl_free(h)
    rc, h = _create(m, b"", [0, 0, 0, 0], [0b101])  # everything deleted or kept: no blob at all
    assert rc == N.AHA_OK and h.value
    L.aha_repl_free(h)
    L.aha_repl_free(None)  # a no-op
    for offs in ([1, 1, 3, 6], [0, 3, 1, 6], [0, 1, 3, 2]):  # offsets[0] != 0; descending
        rc, h = _create(m, b"abcdef", offs)
        assert rc == N.AHA_E_INVALID and not h.value, offs
    rc, h = _create(m, b"abcdef", [0, 1, 1 + (1 << 32), 2 + (1 << 32)])  # one replacement of 2^32 bytes (refused before any read)
    assert rc == N.AHA_E_INVALID and not h.value
    rc, h = _create(None, b"abcdef", [0, 1, 3, 6])
    assert rc == N.AHA_E_INVALID and not h.value
    rc, h = _create(m, b"abcdef", None)
    assert rc == N.AHA_E_INVALID and not h.value
    rc, h = _create(m, None, [0, 1, 3, 6])  # bytes named, no blob
    assert rc == N.AHA_E_INVALID and not h.value
    offs = np.array([0, 1, 3, 6], dtype=np.uint64)
    assert L.aha_repl_create(m._h, None, offs.ctypes.data, None, None) == N.AHA_E_INVALID


def test_repl_table_outlives_its_handle_and_the_other_way_round():
    m = AC.compile(KEYS, host_only=True)
    t = m.replacements({0: "HE"})
    del m
    del t
    m = AC.compile(KEYS, host_only=True)
    t = m.replacements(["a", None, ""])
    del t
    assert m.n_keys == 3


def test_replacements_packs_mappings_and_sequences():
    blob, offs, keep = acmod._pack_replacements({0: "HE", 2: b""}, 3)
    assert blob.tobytes() == b"HE" and offs.tolist() == [0, 2, 2, 2] and keep.tolist() == [0b010]
    blob, offs, keep = acmod._pack_replacements(["a", None, "é\x00"], 3)
    assert blob.tobytes() == "aé\x00".encode() and offs.tolist() == [0, 1, 1, 4] and keep.tolist() == [0b010]
    with pytest.raises(ValueError):
        acmod._pack_replacements(["only one"], 3)
    with pytest.raises(ValueError):
        acmod._pack_replacements({7: "x"}, 3)
    blob, offs, keep = acmod._pack_replacements({}, 40)
    assert blob.size == 0 and keep.tolist() == [0xFFFFFFFF, 0xFF]


def _both(m, table, p=None, n=True, flags=0, overlap=False, handle=True):
    """rc of the host entry and of the device entry on the same arguments (a host-only handle); the guard-filled buffers stay
    untouched"""
    buf = np.full(64, GUARD8, dtype=np.uint8)
    buf[:6] = np.frombuffer(b"ushers", dtype=np.uint8)
    corpus = buf[:6]
    offs = np.array([0, 6], dtype=np.uint64)
    out = buf[3:35] if overlap else np.full(32, GUARD8, dtype=np.uint8)
    doo = np.full(2, GUARD64, dtype=np.uint64)
    nb = C.c_uint64(7)
    pn = C.byref(nb) if n else None
    pp = C.byref(p) if p is not None else None
    L = N.lib()
    h = m._h if handle else None
    t = table._h if table is not None else None
    rc_h = L.aha_ac_replace_batch(h, t, corpus.ctypes.data, offs.ctypes.data, 1, pp, flags, out.ctypes.data, 32, doo.ctypes.data, pn,
                                  None, None)
    rc_d = L.aha_ac_replace_batch_device(h, t, corpus.ctypes.data, offs.ctypes.data, 1, 6, pp, flags, out.ctypes.data, 32,
                                         doo.ctypes.data, pn, None, None, None)
    assert buf[:6].tobytes() == b"ushers" and (buf[6:] == GUARD8).all() and (doo == GUARD64).all()
    assert overlap or (out == GUARD8).all()
    return rc_h, rc_d


def _params(**kw):
    p = N.aha_match_params()
    p.struct_size = C.sizeof(N.aha_match_params)
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def test_replace_argument_checks_hold_on_a_host_only_handle():
    m = AC.compile(KEYS, host_only=True)
    t = m.replacements({0: "HE", 1: ""})  # creation succeeds without a device
    inv = (N.AHA_E_INVALID, N.AHA_E_INVALID)
    assert _both(m, t) == (N.AHA_E_NO_DEVICE, N.AHA_E_NO_DEVICE)
    assert _both(m, t, _params()) == (N.AHA_E_NO_DEVICE, N.AHA_E_NO_DEVICE)
    assert _both(m, t, _params(char_offsets=1)) == inv
    for longest in (1, 2):
        assert _both(m, t, _params(longest=longest)) == inv
    for flags in (1, 2, 0x80000000):
        assert _both(m, t, _params(), flags=flags) == inv
    assert _both(m, t, n=False) == inv  # n_out_bytes == NULL
    assert _both(m, t, handle=False) == inv
    assert _both(m, None) == inv
    other = AC.compile(KEYS, host_only=True)
    assert _both(m, other.replacements({0: "HE"})) == inv  # a table made for another handle
    assert _both(m, t, overlap=True) == inv  # there is no in-place form
    assert _both(m, t, _params(sep_size=257)) == (N.AHA_E_SEP_SIZE, N.AHA_E_SEP_SIZE)
    for call in (lambda: m.replace_batch(b"ushers", [0, 6], t), lambda: m.replace_batch(b"ushers", [0, 6], {0: "x"})):
        with pytest.raises(AhaError) as e:
            call()
        assert e.value.code == N.AHA_E_NO_DEVICE


# ---- the contract in plain Python against substitute and against the kernels' arithmetic ----------------------------------
def _oracle_docs(o, docs):
    hits, dho = [], [0]
    for d in docs:
        h = o.match(d, chars=False)
        hits += [(int(s), int(e), int(v)) for s, e, v in zip(h["start"], h["end"], h["value"])] if h.size else []
        dho.append(len(hits))
    arr = np.zeros(len(hits), dtype=selectsim.HIT_DTYPE)
    for i, t in enumerate(hits):
        arr[i] = t
    return arr, np.array(dho, dtype=np.uint64)


def _models_agree(keys, docs, repl, seen):
    o = orc.AC.compile(keys)
    hits, dho = _oracle_docs(o, docs)
    sel, dso = selectsim.select(hits, dho)
    corpus = np.frombuffer(b"".join(docs), dtype=np.uint8)
    offs = np.cumsum([0] + [len(d) for d in docs]).astype(np.uint64)
    want, want_doo = replacesim.replace(corpus, offs, sel, dso, repl)
    for d, doc in enumerate(docs):  # AC.replace's host arithmetic, document by document
        S = sel[int(dso[d]):int(dso[d + 1])]
        assert acmod.substitute(doc, S, repl, len(keys)) == want[int(want_doo[d]):int(want_doo[d + 1])].tobytes()
        rows = S.tolist()
        for i, (s, e, v) in enumerate(rows):
            r = replacesim.replacement_of(repl, v)
            seen["kept"] += r is None
            seen["empty"] += r == b""
            seen["longer"] += r is not None and len(r) > e - s
            seen["shorter"] += r is not None and 0 < len(r) < e - s
            seen["at_start"] += s == 0
            seen["at_end"] += e == len(doc)
            if i + 1 < len(rows) and rows[i + 1][0] == e:
                seen["adjacent"] += 1
                seen["tie"] += r == b""  # O[j] == O[j + 1]: the tie of the last-j rule
        seen["empty_doc"] += len(doc) == 0
        seen["no_hit_doc"] += len(doc) > 0 and not rows
    got, got_doo = replacesim.kernel_model(corpus, offs, sel, dso, repl)
    assert np.array_equal(got_doo, want_doo), (keys, docs, repl)
    assert got.tobytes() == want.tobytes(), (keys, docs, repl)
    seen["all_deleted"] += want.size == 0 and corpus.size > 0
    return want


def test_replace_models_agree_on_fixed_cases():
    seen = dict.fromkeys(("kept", "empty", "longer", "shorter", "at_start", "at_end", "adjacent", "tie", "empty_doc", "no_hit_doc",
                          "all_deleted"), 0)
    chain = [b"ab", b"bcd", b"cd", b"d"]
    assert _models_agree(chain, [b"abcd", b"", b"xabcdd"], {0: "<AB>", 2: ""}, seen).tobytes() == b"<AB>x<AB>d"
    assert _models_agree([b"a"], [b"aaaa", b"aa"], [b""], seen).size == 0
    assert _models_agree([b"a"], [b"aaab"], [b""], seen).tobytes() == b"b"
    assert _models_agree([b"a", b"b"], [b"aaab-", b"-"], [b"", b"XY\x00"], seen).tobytes() == b"XY\x00--"
    assert _models_agree([b"a", b"b"], [b"ab"], [None, None], seen).tobytes() == b"ab"
    assert _models_agree([b"a"], [b"", b""], {}, seen).size == 0
    assert seen["tie"] and seen["all_deleted"] and seen["kept"]


def test_replace_models_agree_on_random_small_alphabets():
    rng = random.Random(4150)
    seen = dict.fromkeys(("kept", "empty", "longer", "shorter", "at_start", "at_end", "adjacent", "tie", "empty_doc", "no_hit_doc",
                          "all_deleted"), 0)
    for trial in range(3000):
        alpha = "abcd"[: rng.randint(2, 4)]
        keys = sorted({"".join(rng.choice(alpha) for _ in range(rng.randint(1, 4))) for _ in range(rng.randint(1, 7))})
        keys = [k.encode() for k in keys]
        docs = [("".join(rng.choice(alpha + "-") for _ in range(rng.choice((0, 0, 1, 3, 9, 20))))).encode()
                for _ in range(rng.randint(1, 4))]
        choices = [None, b"", b"", b"X", b"YZ", b"\x00", b"longer than any key"]
        if rng.random() < 0.5:
            repl = [rng.choice(choices) for _ in keys]
        else:
            repl = {k: rng.choice(choices) for k in range(len(keys)) if rng.random() < 0.6}
        _models_agree(keys, docs, repl, seen)
    assert all(seen.values()), seen  # every situation the kernels' index arithmetic has to get right came up


def test_cpp_replace_example_compiles(tmp_path):
    from test_gpu_replace_cpp import build_spec_replace

    build_spec_replace(tmp_path)
