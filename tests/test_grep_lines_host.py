"""CPU tests of grep's context lines (aha_ac_grep_batch* with AHA_GREP_LINES): the header's examples on the twin
(greplinesim over the oracle's hits per record); the brute-force definition against the model of the device passes (runs,
windows, toggles) over a few thousand random cases with empty groups, empty records and contexts beyond D; the three
identities against plain grep's twin; every refusal before any device work -- so it holds on a host-only handle, through both
entries, with guarded buffers and counts untouched; the Python argument checks; the constant and the struct in every binding,
90 exports, ABI 8; the Makefile's lists; the C++ example compiles."""
import ctypes as C
import os
import random
import re
import subprocess

import numpy as np
import pytest

import greplinesim as sim
import grepsim
import pyoracle as orc
from aha_amd import AC, AhaError
from aha_amd import _native as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = 0x5A
MAXC = 0x7FFFFFFF
LINES = 16


def hits_per_record(keys, corpus, offs):
    o = orc.AC.compile([k if isinstance(k, bytes) else k.encode() for k in keys])
    text = np.asarray(corpus, dtype=np.uint8).tobytes()
    return [int(o.match(text[int(offs[d]):int(offs[d + 1])], chars=False).size) for d in range(len(offs) - 1)]


# ---- the header's examples ---------------------------------------------------------------------------------------------------
TEXT = b"x\nab\ny\nz\nab\nw\n"
OFFS = [0, 2, 5, 7, 9, 12, 14]


def _example(invert, before, after, groups):
    corpus = np.frombuffer(TEXT, dtype=np.uint8)
    h = hits_per_record(["ab"], corpus, OFFS)
    assert h == [0, 1, 0, 0, 1, 0]
    a = sim.grep_lines(h, OFFS, corpus, invert, before, after, groups)
    b = sim.grep_lines(h, OFFS, corpus, invert, before, after, groups, model=True)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))
    kept, out, doo, im = a
    return kept.tolist(), im.tolist(), out.tobytes(), doo.tolist()


def test_header_examples():
    assert _example(False, 1, 0, None) == ([0, 1, 3, 4], [0, 1, 0, 1], b"x\nab\nz\nab\n", [0, 2, 5, 7, 10])
    assert _example(False, 1, 0, [0, 4, 6])[:2] == ([0, 1, 4], [0, 1, 1])  # line 3 lies in the other group
    assert _example(True, 0, 0, None)[:2] == ([0, 2, 3, 5], [1, 1, 1, 1])
    assert sim.chunk_ends([0, 1, 3, 4], None, 6) == [False, True, False]
    assert sim.chunk_ends([3, 4], [0, 4, 6], 6) == [True]  # neighbours in different groups


# ---- brute force against the model of the device passes -----------------------------------------------------------------------
def _random_groups(rng, D):
    G = rng.randint(1, 6)
    cuts = sorted(rng.randint(0, D) for _ in range(G - 1))
    if rng.random() < 0.3:  # empty groups at the front, in the middle, at the end
        cuts = sorted(cuts + rng.choice([[0], [D], [0, 0], [D, D], [cuts[0]] if cuts else [0]]))
    return [0] + cuts + [D]


def test_brute_force_equals_the_model_over_random_cases():
    rng = random.Random(16)
    n_kept = n_ctx = 0
    for trial in range(4000):
        D = rng.randint(0, 40)
        p = rng.choice([0.0, 0.05, 0.2, 0.5, 0.9, 1.0])
        m = [rng.random() < p for _ in range(D)]
        groups = None if rng.random() < 0.2 else _random_groups(rng, D)
        before, after = (rng.choice([0, 0, 1, 1, 2, 3, 5, 8, D, D + 1, 100, MAXC]) for _ in range(2))
        a, b = sim.keep_brute(m, before, after, groups), sim.keep_model(m, before, after, groups)
        assert a == b, (trial, m, groups, before, after)
        assert all(k for k, mm in zip(a, m) if mm)  # a match is kept
        n_kept += sum(a)
        n_ctx += sum(1 for k, mm in zip(a, m) if k and not mm)
    assert n_kept > 20000 and n_ctx > 5000  # the cases are not mostly empty


def test_results_over_random_batches_with_empty_records():
    rng = random.Random(17)
    for trial in range(300):
        D = rng.randint(0, 24)
        lens = [rng.choice([0, 0, 1, 2, 3]) for _ in range(D)]
        offs = np.cumsum([0] + lens).astype(np.uint64)
        corpus = np.array([rng.choice(b"ab\n") for _ in range(int(offs[-1]))], dtype=np.uint8)
        h = [rng.choice([0, 0, 1, 3]) for _ in range(D)]
        groups = None if trial % 3 == 0 else _random_groups(rng, D)
        invert, before, after = trial % 2 == 1, rng.choice([0, 1, 2, 30]), rng.choice([0, 1, 2, 30])
        kept, out, doo, im = sim.grep_lines(h, offs, corpus, invert, before, after, groups)
        again = sim.grep_lines(h, offs, corpus, invert, before, after, groups, model=True)
        assert all(np.array_equal(x, y) for x, y in zip((kept, out, doo, im), again))
        assert doo.size == kept.size + 1 and int(doo[-1]) == out.size and im.size == kept.size
        assert out.tobytes() == b"".join(corpus[int(offs[r]):int(offs[r + 1])].tobytes() for r in kept.tolist())


# ---- the three identities --------------------------------------------------------------------------------------------------------
def test_identities_against_plain_grep():
    rng = random.Random(18)
    for trial in range(200):
        D = rng.randint(0, 30)
        lens = [rng.choice([0, 1, 2, 3]) for _ in range(D)]
        offs = np.cumsum([0] + lens).astype(np.uint64)
        corpus = np.array([rng.choice(b"xy\n") for _ in range(int(offs[-1]))], dtype=np.uint8)
        h = [rng.choice([0, 0, 0, 2]) for _ in range(D)]
        groups = _random_groups(rng, D)
        for invert in (False, True):
            m = sim.matches(h, D, invert)
            # no context = plain grep, is_match all 1
            kept, out, doo, im = sim.grep_lines(h, offs, corpus, invert, 0, 0, groups)
            g_kept, g_out, g_doo = grepsim.grep(h, offs, corpus, invert)
            assert np.array_equal(kept, g_kept) and out.tobytes() == g_out.tobytes() and np.array_equal(doo, g_doo)
            assert im.tolist() == [1] * kept.size
            # the largest context keeps exactly the groups that hold a matching record, whole
            kept, *_ = sim.grep_lines(h, offs, corpus, invert, MAXC, MAXC, groups)
            want = [r for lo, hi in zip(groups, groups[1:]) if any(m[lo:hi]) for r in range(lo, hi)]
            assert kept.tolist() == want
            # without groups and with at least one match every record is kept
            kept, *_ = sim.grep_lines(h, offs, corpus, invert, MAXC, MAXC, None)
            assert kept.tolist() == (list(range(D)) if any(m) else [])


# ---- refusals, before any device work ----------------------------------------------------------------------------------------
class _Buffers:
    def __init__(self):
        self.corpus = np.frombuffer(TEXT, dtype=np.uint8).copy()
        self.offs = np.array(OFFS, dtype=np.uint64)
        self.groups = np.array([0, 4, 6], dtype=np.uint64)
        self.kept = np.full(16, GUARD, dtype=np.uint64)
        self.doo = np.full(17, GUARD, dtype=np.uint64)
        self.out = np.full(64, GUARD, dtype=np.uint8)
        self.flags = np.full(16, GUARD, dtype=np.uint8)

    def untouched(self):
        return all((a == GUARD).all() for a in (self.kept, self.doo, self.out, self.flags))


def _lp(b, before=1, after=2, flags=0, reserved=0, struct_size=None, groups=True, n_groups=None, is_match=True, **match):
    lp = N.aha_grep_lines_params()
    lp.match.struct_size = C.sizeof(N.aha_grep_lines_params) if struct_size is None else struct_size
    for k, v in match.items():
        setattr(lp.match, k, v)
    lp.before, lp.after, lp.flags, lp.reserved = before, after, flags, reserved
    lp.group_offsets = b.groups.ctypes.data if groups else None
    lp.n_groups = (2 if groups else 0) if n_groups is None else n_groups
    lp.is_match = b.flags.ctypes.data if is_match else None
    return lp


def _both(m, call_flags=LINES, cap_docs=16, no_params=False, **kw):
    """rc of the host entry and of the device entry on the same arguments; the buffers and the counts stay untouched"""
    b = _Buffers()
    lp = _lp(b, **kw)
    flags = call_flags
    nk, nb, nh = C.c_uint64(7), C.c_uint64(7), C.c_uint64(7)
    p = None if no_params else C.cast(C.pointer(lp), C.POINTER(N.aha_match_params))
    L = N.lib()
    kp, dp = (b.kept.ctypes.data, b.doo.ctypes.data) if cap_docs else (None, None)
    rc_h = L.aha_ac_grep_batch(m._h, b.corpus.ctypes.data, b.offs.ctypes.data, 6, p, flags, kp, dp, cap_docs, b.out.ctypes.data, 64,
                               C.byref(nk), C.byref(nb), C.byref(nh))
    rc_d = L.aha_ac_grep_batch_device(m._h, b.corpus.ctypes.data, b.offs.ctypes.data, 6, b.corpus.size, p, flags, kp, dp, cap_docs,
                                      b.out.ctypes.data, 64, C.byref(nk), C.byref(nb), C.byref(nh), None)
    assert b.untouched() and (nk.value, nb.value, nh.value) == (7, 7, 7)
    return rc_h, rc_d


INVALID2 = (N.AHA_E_INVALID, N.AHA_E_INVALID)
NO_DEVICE2 = (N.AHA_E_NO_DEVICE, N.AHA_E_NO_DEVICE)


@pytest.fixture(scope="module")
def host():
    return AC.compile(["ab"], host_only=True)


def test_a_correct_call_answers_no_device_on_a_host_only_handle(host):
    m = host
    assert _both(m) == NO_DEVICE2
    assert _both(m, call_flags=LINES | 1) == NO_DEVICE2
    assert _both(m, before=0, after=0) == NO_DEVICE2
    assert _both(m, before=MAXC, after=MAXC) == NO_DEVICE2
    assert _both(m, groups=False) == NO_DEVICE2
    assert _both(m, is_match=False) == NO_DEVICE2
    assert _both(m, n_groups=1000) == NO_DEVICE2  # n_groups > D + 1 is no error: empty groups may be many
    assert _both(m, sep_size=40) == NO_DEVICE2  # a separator filter is allowed
    assert _both(m, struct_size=C.sizeof(N.aha_grep_lines_params) + 8) == NO_DEVICE2  # a later, larger struct
    assert _both(m, cap_docs=0, is_match=False) == NO_DEVICE2
    for call in (lambda: m.grep_batch(TEXT, OFFS, before=1), lambda: m.grep_batch(TEXT, OFFS, context=2, groups=[0, 4, 6]),
                 lambda: m.grep_batch(TEXT, OFFS, matched=np.zeros(6, np.uint8))):
        with pytest.raises(AhaError) as e:
            call()
        assert e.value.code == N.AHA_E_NO_DEVICE


def test_refusals_come_before_the_device_check(host):
    m = host
    for flags in (16 | 2, 16 | 4, 16 | 8, 16 | 0x80000000, 16 | 1 | 2, 16 | 1 | 4, 16 | 32):
        assert _both(m, call_flags=flags) == INVALID2, flags
    assert _both(m, no_params=True) == INVALID2
    assert _both(m, struct_size=C.sizeof(N.aha_match_params)) == INVALID2
    assert _both(m, struct_size=C.sizeof(N.aha_excerpt_params)) == INVALID2
    assert _both(m, struct_size=C.sizeof(N.aha_grep_lines_params) - 1) == INVALID2
    assert _both(m, struct_size=0) == INVALID2
    assert _both(m, flags=1) == INVALID2
    assert _both(m, reserved=1) == INVALID2
    assert _both(m, before=MAXC + 1) == INVALID2
    assert _both(m, after=MAXC + 1) == INVALID2
    assert _both(m, before=0xFFFFFFFF, after=0xFFFFFFFF) == INVALID2
    assert _both(m, groups=False, n_groups=2) == INVALID2
    assert _both(m, groups=True, n_groups=0) == INVALID2
    assert _both(m, cap_docs=0, is_match=True) == INVALID2
    # everything plain grep refuses
    assert _both(m, char_offsets=1) == INVALID2
    for longest in (1, 2):
        assert _both(m, longest=longest) == INVALID2
    assert _both(m, sep_size=257) == (N.AHA_E_SEP_SIZE, N.AHA_E_SEP_SIZE)
    L = N.lib()
    b = _Buffers()
    n = C.c_uint64(0)
    lp = _lp(b, is_match=False)
    p = C.cast(C.pointer(lp), C.POINTER(N.aha_match_params))
    cp, op = b.corpus.ctypes.data, b.offs.ctypes.data
    # n_kept NULL, a NULL handle; a NULL buffer with a capacity; out overlapping the corpus
    assert L.aha_ac_grep_batch(m._h, cp, op, 6, p, 16, None, None, 0, None, 0, None, None, None) == N.AHA_E_INVALID
    assert L.aha_ac_grep_batch_device(m._h, cp, op, 6, 14, p, 16, None, None, 0, None, 0, None, None, None, None) == N.AHA_E_INVALID
    assert L.aha_ac_grep_batch(None, cp, op, 6, p, 16, None, None, 0, None, 0, C.byref(n), None, None) == N.AHA_E_INVALID
    assert L.aha_ac_grep_batch(m._h, cp, op, 6, p, 16, None, None, 3, None, 0, C.byref(n), None, None) == N.AHA_E_INVALID
    assert L.aha_ac_grep_batch(m._h, cp, op, 6, p, 16, None, None, 0, None, 9, C.byref(n), None, None) == N.AHA_E_INVALID
    assert L.aha_ac_grep_batch_device(m._h, cp, op, 6, 14, p, 16, None, None, 0, cp + 2, 8, C.byref(n), None, None,
                                      None) == N.AHA_E_INVALID
    # is_match alone is a per-document buffer: a capacity with it and nothing else is a correct call, as is the sizing call
    lp.is_match = b.flags.ctypes.data
    assert L.aha_ac_grep_batch(m._h, cp, op, 6, p, 16, None, None, 3, None, 0, C.byref(n), None, None) == N.AHA_E_NO_DEVICE
    lp.is_match = None
    assert L.aha_ac_grep_batch(m._h, cp, op, 6, p, 16, None, None, 0, None, 0, C.byref(n), None, None) == N.AHA_E_NO_DEVICE
    assert b.untouched()


def test_without_the_flag_struct_size_and_the_other_fields_change_nothing(host):
    # a plain grep call whose params claim the larger struct (and hold rubbish behind the match params) is the call it was
    kw = dict(before=0xFFFFFFFF, after=0xFFFFFFFF, reserved=5, groups=False, n_groups=99)
    assert _both(host, call_flags=0, **kw) == NO_DEVICE2
    assert _both(host, call_flags=N.AHA_GREP_INVERT, **kw) == NO_DEVICE2


def test_python_argument_checks_come_before_the_library(host):
    m = host
    for before, after in ((-1, 0), (0, -1), (MAXC + 1, 0), (0, MAXC + 1), (1.5, 0), (None, 1), ("3", 0), (True, 0)):
        with pytest.raises(ValueError):
            m.grep_batch(TEXT, OFFS, before=before, after=after)
        with pytest.raises(ValueError):
            m.grep(TEXT, before=before, after=after)
        with pytest.raises(ValueError):
            m.grep_corpus(None, before=before, after=after)  # (the check comes first: no corpus is touched)
        with pytest.raises(ValueError):
            m.grep_batch_device(None, None, before=before, after=after)
    for kw in (dict(context=1, before=1), dict(context=1, after=2), dict(context=-1), dict(context=MAXC + 1), dict(context="1")):
        with pytest.raises(ValueError):
            m.grep_batch(TEXT, OFFS, **kw)
        with pytest.raises(ValueError):
            m.grep_batch_device(None, None, **kw)
        with pytest.raises(ValueError):
            m.grep_corpus(None, **kw)
        with pytest.raises(ValueError):
            m.grep(TEXT, **kw)
    # not with a rule: the rule is never looked at
    for kw in (dict(before=1), dict(after=1), dict(context=0), dict(groups=[0, 6]), dict(matched=np.zeros(6, np.uint8))):
        with pytest.raises(ValueError, match="rule"):
            m.grep_batch(TEXT, OFFS, rule=object(), **kw)
        with pytest.raises(ValueError, match="rule"):
            m.grep_batch_device(None, None, rule=object(), **kw)
        with pytest.raises(ValueError, match="rule"):
            m.grep_corpus(None, rule=object(), **kw)
        with pytest.raises(ValueError, match="rule"):
            m.grep(TEXT, rule=object(), **kw)
    with pytest.raises(ValueError):
        m.grep_batch(TEXT, OFFS, before=1, matched=np.zeros(6, np.int32))
    with pytest.raises(ValueError):
        m.grep_batch(TEXT, OFFS, before=1, groups=np.zeros((2, 2), np.uint64))
    with pytest.raises(ValueError):
        m.grep_batch(TEXT, OFFS, before=1, rows=np.zeros((6, 1), np.uint32))


def test_with_no_keyword_the_calls_pass_what_they_passed(host, monkeypatch):
    """grep_batch without a context keyword (or with the defaults spelled out) reaches the library with plain grep's flags and
    a plain aha_match_params"""
    seen = []
    real = N.lib().aha_ac_grep_batch

    def spy(h, corpus, offs, D, p, flags, *rest):
        seen.append((flags, p.contents.struct_size if p else None))
        return real(h, corpus, offs, D, p, flags, *rest)

    real_lib = N.lib()

    class _Lib:
        def __getattr__(self, name):
            return spy if name == "aha_ac_grep_batch" else getattr(real_lib, name)

    monkeypatch.setattr(N, "lib", lambda: _Lib())
    for kw in ({}, dict(before=0, after=0), dict(invert=True)):
        with pytest.raises(AhaError):
            host.grep_batch(TEXT, OFFS, **kw)
    with pytest.raises(AhaError):
        host.grep_batch(TEXT, OFFS, before=1, invert=True)
    assert seen == [(0, 48), (0, 48), (1, 48), (17, 88)]


# ---- the bindings, the exports, the build -----------------------------------------------------------------------------------
def test_constant_and_struct_declared_and_bound():
    hdr = open(os.path.join(ROOT, "include", "aha_hip.h")).read()
    listed = open(os.path.join(ROOT, "aha_amd", "csrc", "exports.map")).read()
    crystal = open(os.path.join(ROOT, "bindings", "crystal", "aha_hip.cr")).read()
    cpp = open(os.path.join(ROOT, "include", "aha", "ac.hpp")).read()
    assert re.search(r"#define\s+AHA_GREP_LINES\s+16u", hdr) and N.AHA_GREP_LINES == 16
    assert re.search(r"}\s*aha_grep_lines_params;", hdr)
    assert C.sizeof(N.aha_match_params) == 48  # the mirror did not move
    assert C.sizeof(N.aha_grep_lines_params) == 88
    fields = ("match", "before", "after", "flags", "reserved", "group_offsets", "n_groups", "is_match")
    assert [(f, getattr(N.aha_grep_lines_params, f).offset) for f in fields] == [
        ("match", 0), ("before", 48), ("after", 52), ("flags", 56), ("reserved", 60), ("group_offsets", 64), ("n_groups", 72),
        ("is_match", 80)]
    assert "GREP_LINES = 16_u32" in crystal and "struct GrepLinesParams" in crystal
    assert re.search(r"def grep\([^)]*before : UInt32[^)]*after : UInt32[^)]*context :", crystal)
    assert "AHA_GREP_LINES" in cpp and "aha_grep_lines_params" in cpp and "grep_lines_batch(" in cpp and "grep_lines_batch_device(" in cpp
    assert len(re.findall(r"^\s+aha_\w+;", listed, re.M)) == 90  # no new entry point
    lib = os.path.join(ROOT, "aha_amd", "libaha_hip.so")
    nm = subprocess.run(["nm", "-D", "--defined-only", lib], capture_output=True, text=True, check=True).stdout
    assert len([ln for ln in nm.splitlines() if re.search(r" T aha_\w+$", ln)]) == 90
    assert N.lib().aha_abi_version() == 8 and re.search(r"#define\s+AHA_ABI_VERSION\s+8\b", hdr)
    # the section, the example, the identities and what is out of scope are in the header
    for phrase in ("CONTEXT LINES", "kept {0, 1, 3, 4}", "is_match {0, 1, 0, 1}", "kept {0, 1, 4}", "kept {0, 2, 3, 5}",
                   "equals plain grep", "every record is kept", "a separator written on the device"):
        assert phrase in hdr, phrase


def test_makefile_lists_the_new_sources():
    mk = open(os.path.join(ROOT, "aha_amd", "csrc", "Makefile")).read()
    assert mk.count("scan_greplines.hip") == 1
    assert mk.count("grep_lines_stubs.cpp") == 2
    stubs = open(os.path.join(ROOT, "tests", "cpp", "grep_lines_stubs.cpp")).read()
    decl = open(os.path.join(ROOT, "aha_amd", "csrc", "image.hpp")).read()
    names = set(re.findall(r"\bvoid (greplines_launch_\w+)\(", decl))
    assert len(names) == 4 and names == set(re.findall(r"\bvoid (greplines_launch_\w+)\(", stubs))


def test_cpp_grep_lines_example_compiles(tmp_path):
    from test_gpu_grep_lines_cpp import build_spec_grep_lines

    build_spec_grep_lines(tmp_path)
