"""CPU tests of the excerpts calls (aha_ac_grep_batch* with AHA_GREP_CONTEXT): the header's four examples on the twin
(excerptsim.excerpts over the oracle's hits); the twin against the numpy model of the device arithmetic over a few thousand
random batches with stray continuation bytes; every refusal before any device work -- so it holds on a host-only handle, through
both entries, with guarded buffers and counts untouched; the Python argument checks; the constant and the struct in every
binding, 90 exports, ABI 8; the Makefile's lists; excerpt_window.hpp against a brute-force loop under ASan and UBSan."""
import ctypes as C
import os
import random
import re
import subprocess

import numpy as np
import pytest

import excerptsim
import pyoracle as orc
from aha_amd import AC, AhaError
from aha_amd import _native as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = 0x5A
MAXC = 0x7FFFFFFF


def oracle_hits_per_doc(o, corpus, offs, sep_pair=None):
    """the oracle's hits of every document as (n, 2) arrays of (start, end), relative to the document -> (list, n_hits)"""
    per, n = [], 0
    for d in range(len(offs) - 1):
        h = o.match(np.asarray(corpus[int(offs[d]):int(offs[d + 1])], dtype=np.uint8).tobytes(), chars=False, sep=sep_pair)
        per.append(np.stack([np.asarray(h["start"], dtype=np.int64), np.asarray(h["end"], dtype=np.int64)], axis=1)
                   if h.size else np.zeros((0, 2), np.int64))
        n += int(h.size)
    return per, n


def _twin(keys, docs, before, after):
    o = orc.AC.compile([k if isinstance(k, bytes) else k.encode() for k in keys])
    corpus = np.frombuffer(b"".join(docs), dtype=np.uint8)
    offs = np.cumsum([0] + [len(d) for d in docs]).astype(np.uint64)
    per, n_hits = oracle_hits_per_doc(o, corpus, offs)
    starts, out, oo = excerptsim.excerpts(per, offs, corpus, before, after)
    m_starts, m_out, m_oo, _ = excerptsim.model_excerpts(excerptsim.cover_bits(per, offs), offs, corpus, before, after)
    assert np.array_equal(starts, m_starts) and out.tobytes() == m_out.tobytes() and np.array_equal(oo, m_oo)
    return starts.tolist(), out.tobytes(), oo.tolist(), n_hits, per, offs, corpus


# ---- the header's examples ---------------------------------------------------------------------------------------------------
def test_example_1_touching_at_a_boundary_stays_two_touching_inside_merges():
    docs = [b"xxabxxxxabx", b"ab"]
    starts, out, oo, n_hits, *_ = _twin(["ab"], docs, 1, 2)
    assert starts == [1, 7, 11] and out == b"xabxx" b"xabx" b"ab" and oo == [0, 5, 9, 11] and n_hits == 3
    starts, out, oo, n_hits, *_ = _twin(["ab"], docs, 1, 3)
    assert starts == [1, 11] and out == b"xabxxxxabx" b"ab" and oo == [0, 10, 12] and n_hits == 3


def test_example_2_edges_inside_characters_are_snapped_outwards():
    text = "我是中".encode()
    assert len(text) == 9
    starts, out, oo, n_hits, per, *_ = _twin(["是"], [text], 1, 1)
    assert per[0].tolist() == [[3, 6]]
    assert starts == [0] and out == text and oo == [0, 9] and n_hits == 1
    t = np.frombuffer(text, dtype=np.uint8)
    assert [excerptsim.snap_left(t, 0, x) for x in (2, 1, 0)] == [0, 0, 0]
    assert [excerptsim.snap_right(t, 9, x) for x in (7, 8, 9)] == [9, 9, 9]


def test_example_3_no_context_gives_the_covered_runs():
    docs = [b"xxabxxxxabx", b"ab", b"", b"abab", b"xx"]
    starts, out, oo, n_hits, per, offs, corpus = _twin(["ab", "ba"], docs, 0, 0)
    M = excerptsim.cover_bits(per, offs)
    assert len(out) == int(M.sum())  # the cover call's n_covered
    assert starts == [2, 8, 11, 13] and out == b"ab" b"ab" b"ab" b"abab"  # split at the document boundary 13


def test_example_4_the_largest_context_gives_the_documents_with_a_hit():
    docs = [b"xxabxxxxabx", b"", b"nothing", b"ab", b"\x80\x80ab\x80", b"q"]
    starts, out, oo, n_hits, per, offs, corpus = _twin(["ab"], docs, MAXC, MAXC)
    kept = [d for d in range(len(docs)) if len(per[d])]
    assert kept == [0, 3, 4]
    assert starts == [int(offs[d]) for d in kept] and out == b"".join(docs[d] for d in kept)


# ---- the twin against the model of the device arithmetic ---------------------------------------------------------------------
ALPHABET = [ord("A"), ord(" "), 0x80, 0xBF, 0xE6, 0xC3, 0x81]
BEFORE = [0, 1, 2, 3, 4, 7, 100]
AFTER = [0, 1, 2, 3, 5, 100]


def test_the_twin_equals_the_device_model_over_random_batches():
    rng = random.Random(20)
    n = 0
    for trial in range(3000):
        D = rng.randint(0, 6)
        lens = [rng.choice([0, 0, 1, 1, 2, 3, 5, 8, 13, 21]) for _ in range(D)]
        offs = np.cumsum([0] + lens).astype(np.uint64)
        corpus = np.array([rng.choice(ALPHABET) for _ in range(int(offs[-1]))], dtype=np.uint8)
        per = []
        for L in lens:  # any hits inside the document: the twin takes them as given
            hits = []
            for _ in range(rng.choice([0, 0, 1, 1, 2, 4]) if L else 0):
                s = rng.randrange(L)
                hits.append((s, rng.randint(s + 1, min(L, s + 4))))
            per.append(np.array(sorted(hits), dtype=np.int64).reshape(-1, 2))
        M = excerptsim.cover_bits(per, offs)
        before, after = rng.choice(BEFORE), rng.choice(AFTER)
        if trial % 50 == 0:
            before, after = rng.choice([MAXC, before]), rng.choice([MAXC, after])
        starts, out, oo = excerptsim.excerpts(per, offs, corpus, before, after)
        m_starts, m_out, m_oo, n_runs = excerptsim.model_excerpts(M, offs, corpus, before, after)
        assert np.array_equal(starts, m_starts), (trial, lens, per, before, after)
        assert out.tobytes() == m_out.tobytes() and np.array_equal(oo, m_oo), (trial, lens, per, before, after)
        assert starts.size <= n_runs
        n += starts.size
    assert n > 3000  # the batches are not mostly empty


# ---- refusals, before any device work ----------------------------------------------------------------------------------------
class _Buffers:
    def __init__(self):
        self.corpus = np.frombuffer(b"xxabxxxxabxab", dtype=np.uint8).copy()
        self.offs = np.array([0, 11, 13], dtype=np.uint64)
        self.kept = np.full(16, GUARD, dtype=np.uint64)
        self.doo = np.full(17, GUARD, dtype=np.uint64)
        self.out = np.full(64, GUARD, dtype=np.uint8)

    def untouched(self):
        return all((a == GUARD).all() for a in (self.kept, self.doo, self.out))


def _ep(before=1, after=2, flags=0, reserved=0, struct_size=None, **match):
    ep = N.aha_excerpt_params()
    ep.match.struct_size = C.sizeof(N.aha_excerpt_params) if struct_size is None else struct_size
    for k, v in match.items():
        setattr(ep.match, k, v)
    ep.before, ep.after, ep.flags, ep.reserved = before, after, flags, reserved
    return ep


def _both(m, ep, flags=N.AHA_GREP_CONTEXT):
    """rc of the host entry and of the device entry on the same arguments; the buffers and the counts stay untouched"""
    b = _Buffers()
    nk, nb, nh = C.c_uint64(7), C.c_uint64(7), C.c_uint64(7)
    p = C.cast(C.pointer(ep), C.POINTER(N.aha_match_params)) if ep is not None else None
    L = N.lib()
    rc_h = L.aha_ac_grep_batch(m._h, b.corpus.ctypes.data, b.offs.ctypes.data, 2, p, flags, b.kept.ctypes.data, b.doo.ctypes.data, 16,
                               b.out.ctypes.data, 64, C.byref(nk), C.byref(nb), C.byref(nh))
    rc_d = L.aha_ac_grep_batch_device(m._h, b.corpus.ctypes.data, b.offs.ctypes.data, 2, b.corpus.size, p, flags, b.kept.ctypes.data,
                                      b.doo.ctypes.data, 16, b.out.ctypes.data, 64, C.byref(nk), C.byref(nb), C.byref(nh), None)
    assert b.untouched() and (nk.value, nb.value, nh.value) == (7, 7, 7)
    return rc_h, rc_d


INVALID2 = (N.AHA_E_INVALID, N.AHA_E_INVALID)
NO_DEVICE2 = (N.AHA_E_NO_DEVICE, N.AHA_E_NO_DEVICE)


@pytest.fixture(scope="module")
def host():
    return AC.compile(["ab"], host_only=True)


def test_a_correct_call_answers_no_device_on_a_host_only_handle(host):
    m = host
    assert _both(m, _ep()) == NO_DEVICE2
    assert _both(m, _ep(0, 0)) == NO_DEVICE2
    assert _both(m, _ep(MAXC, MAXC)) == NO_DEVICE2
    assert _both(m, _ep(sep_size=40)) == NO_DEVICE2  # a separator filter is allowed
    assert _both(m, _ep(struct_size=C.sizeof(N.aha_excerpt_params) + 8)) == NO_DEVICE2  # a later, larger struct
    for call in (lambda: m.excerpts_batch(b"xxab", [0, 4], 1), lambda: m.excerpts(b"xxab", 1, 2), lambda: m.excerpts("xxab", 0)):
        with pytest.raises(AhaError) as e:
            call()
        assert e.value.code == N.AHA_E_NO_DEVICE


def test_refusals_come_before_the_device_check(host):
    m = host
    # the flag stands alone
    for flags in (8 | 1, 8 | 4, 8 | 4 | 1, 8 | 2, 8 | 16, 8 | 0x80000000):
        assert _both(m, _ep(), flags=flags) == INVALID2, flags
    # the struct
    assert _both(m, _ep(struct_size=C.sizeof(N.aha_match_params))) == INVALID2
    assert _both(m, _ep(struct_size=C.sizeof(N.aha_excerpt_params) - 1)) == INVALID2
    assert _both(m, _ep(struct_size=0)) == INVALID2
    assert _both(m, None) == INVALID2
    assert _both(m, _ep(flags=1)) == INVALID2
    assert _both(m, _ep(reserved=1)) == INVALID2
    assert _both(m, _ep(before=MAXC + 1)) == INVALID2
    assert _both(m, _ep(after=MAXC + 1)) == INVALID2
    assert _both(m, _ep(before=0xFFFFFFFF, after=0xFFFFFFFF)) == INVALID2
    # everything plain grep refuses
    assert _both(m, _ep(char_offsets=1)) == INVALID2
    for longest in (1, 2):
        assert _both(m, _ep(longest=longest)) == INVALID2
    assert _both(m, _ep(sep_size=257)) == (N.AHA_E_SEP_SIZE, N.AHA_E_SEP_SIZE)
    L = N.lib()
    b = _Buffers()
    n = C.c_uint64(0)
    ep = _ep()
    p = C.cast(C.pointer(ep), C.POINTER(N.aha_match_params))
    cp, op = b.corpus.ctypes.data, b.offs.ctypes.data
    # n_kept NULL, a NULL handle; a NULL buffer with a capacity; out overlapping the corpus
    assert L.aha_ac_grep_batch(m._h, cp, op, 2, p, 8, None, None, 0, None, 0, None, None, None) == N.AHA_E_INVALID
    assert L.aha_ac_grep_batch_device(m._h, cp, op, 2, 13, p, 8, None, None, 0, None, 0, None, None, None, None) == N.AHA_E_INVALID
    assert L.aha_ac_grep_batch(None, cp, op, 2, p, 8, None, None, 0, None, 0, C.byref(n), None, None) == N.AHA_E_INVALID
    assert L.aha_ac_grep_batch_device(None, cp, op, 2, 13, p, 8, None, None, 0, None, 0, C.byref(n), None, None,
                                      None) == N.AHA_E_INVALID
    assert L.aha_ac_grep_batch(m._h, cp, op, 2, p, 8, None, None, 3, None, 0, C.byref(n), None, None) == N.AHA_E_INVALID
    assert L.aha_ac_grep_batch(m._h, cp, op, 2, p, 8, None, None, 0, None, 9, C.byref(n), None, None) == N.AHA_E_INVALID
    assert L.aha_ac_grep_batch_device(m._h, cp, op, 2, 13, p, 8, None, None, 0, cp + 2, 8, C.byref(n), None, None,
                                      None) == N.AHA_E_INVALID
    # the sizing call is a correct call
    assert L.aha_ac_grep_batch(m._h, cp, op, 2, p, 8, None, None, 0, None, 0, C.byref(n), None, None) == N.AHA_E_NO_DEVICE
    assert b.untouched()


def test_without_the_flag_struct_size_changes_nothing(host):
    # a plain grep call whose params claim the larger struct (and hold rubbish behind the match params) is the call it was
    ep = _ep(before=0xFFFFFFFF, after=0xFFFFFFFF, flags=9, reserved=5)
    assert _both(host, ep, flags=0) == NO_DEVICE2
    assert _both(host, ep, flags=N.AHA_GREP_INVERT) == NO_DEVICE2


def test_python_argument_checks_come_before_the_library(host):
    m = host
    for before, after in ((-1, 0), (0, -1), (MAXC + 1, 0), (0, MAXC + 1), (1.5, 0), (None, 1), ("3", 0), (True, 0)):
        with pytest.raises(ValueError):
            m.excerpts_batch(b"xxab", [0, 4], before, after)
        with pytest.raises(ValueError):
            m.excerpts(b"xxab", before, after)
        with pytest.raises(ValueError):
            m.excerpts_corpus(None, before, after)  # (the check comes first: no corpus is touched)
        with pytest.raises(ValueError):
            m.excerpts_batch_device(None, None, before=before, after=after)
    with pytest.raises(TypeError):
        m.excerpts_batch_device(None, None, None, None, None, 1)  # before is keyword-only


# ---- the bindings, the exports, the build -----------------------------------------------------------------------------------
def test_constant_and_struct_declared_and_bound():
    hdr = open(os.path.join(ROOT, "include", "aha_hip.h")).read()
    listed = open(os.path.join(ROOT, "aha_amd", "csrc", "exports.map")).read()
    crystal = open(os.path.join(ROOT, "bindings", "crystal", "aha_hip.cr")).read()
    cpp = open(os.path.join(ROOT, "include", "aha", "ac.hpp")).read()
    assert re.search(r"#define\s+AHA_GREP_CONTEXT\s+8u", hdr) and N.AHA_GREP_CONTEXT == 8
    assert re.search(r"}\s*aha_excerpt_params;", hdr)
    assert C.sizeof(N.aha_match_params) == 48  # the mirror did not move
    assert C.sizeof(N.aha_excerpt_params) == 64
    assert [(f, getattr(N.aha_excerpt_params, f).offset) for f in ("match", "before", "after", "flags", "reserved")] == [
        ("match", 0), ("before", 48), ("after", 52), ("flags", 56), ("reserved", 60)]
    assert "GREP_CONTEXT = 8_u32" in crystal and "struct ExcerptParams" in crystal and "def excerpts(" in crystal
    assert "AHA_GREP_CONTEXT" in cpp and "aha_excerpt_params" in cpp and "excerpts_batch(" in cpp and "excerpts_batch_device(" in cpp
    assert len(re.findall(r"^\s+aha_\w+;", listed, re.M)) == 90  # no new entry point
    lib = os.path.join(ROOT, "aha_amd", "libaha_hip.so")
    nm = subprocess.run(["nm", "-D", "--defined-only", lib], capture_output=True, text=True, check=True).stdout
    assert len([ln for ln in nm.splitlines() if re.search(r" T aha_\w+$", ln)]) == 90
    assert N.lib().aha_abi_version() == 8 and re.search(r"#define\s+AHA_ABI_VERSION\s+8\b", hdr)
    for method in ("excerpts_batch", "excerpts_batch_device", "excerpts_corpus", "excerpts"):
        assert callable(getattr(AC, method))
    # the examples and what is out of scope are in the header
    for phrase in ("xabxx", "0x7FFFFFFF", "snapL", "snapR", "contexts counted in characters or in lines"):
        assert phrase in hdr, phrase


def test_makefile_lists_the_new_sources():
    mk = open(os.path.join(ROOT, "aha_amd", "csrc", "Makefile")).read()
    assert mk.count("scan_excerpt.hip") == 1 and mk.count("excerpt_window.hpp") == 1
    assert mk.count("excerpt_stubs.cpp") == 2
    stubs = open(os.path.join(ROOT, "tests", "cpp", "excerpt_stubs.cpp")).read()
    decl = open(os.path.join(ROOT, "aha_amd", "csrc", "image.hpp")).read()
    names = set(re.findall(r"\bvoid (excerpt_launch_\w+)\(", decl))
    assert len(names) == 4 and names == set(re.findall(r"\bvoid (excerpt_launch_\w+)\(", stubs))


def test_spec_excerpt_window_runs_clean_under_asan_and_ubsan(tmp_path):
    exe = str(tmp_path / "spec_excerpt_window")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           os.path.join(ROOT, "tests", "cpp", "spec_excerpt_window.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert " 0 failure(s)" in r.stdout


def test_cpp_excerpt_example_compiles(tmp_path):
    from test_gpu_excerpt_cpp import build_spec_excerpt

    build_spec_excerpt(tmp_path)
