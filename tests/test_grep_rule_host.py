"""CPU tests of rule grep (aha_ac_grep_batch* with AHA_GREP_RULE): the constants and structs are declared and bound in every
binding, the ABI stays 8 with 90 exports; every refusal comes before any device work -- so it holds on a host-only handle,
through both entries, with guarded buffers untouched; AC.rule validates on the host; the header's worked example through
rulesim over the oracle's hits; and kgq_edges' word arithmetic (rulesim.kernel_model) against the direct definition of S and T."""
import ctypes as C
import itertools
import os
import random
import re

import numpy as np
import pytest

import classsim
import pyoracle as orc
import rulesim
from aha_amd import AC, AhaError, Rule
from aha_amd import _native as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = 0x5A
KEYS = ["he", "she", "hers"]
CLASSES = [[0], [0, 1], []]


def test_rule_constants_and_structs_declared_and_bound():
    hdr = open(os.path.join(ROOT, "include", "aha_hip.h")).read()
    listed = open(os.path.join(ROOT, "aha_amd", "csrc", "exports.map")).read()
    crystal = open(os.path.join(ROOT, "bindings", "crystal", "aha_hip.cr")).read()
    cpp = open(os.path.join(ROOT, "include", "aha", "ac.hpp")).read()
    assert re.search(r"#define\s+AHA_GREP_RULE\s+4u", hdr) and N.AHA_GREP_RULE == 4
    assert re.search(r"#define\s+AHA_RULE_GE\s+0u", hdr) and N.AHA_RULE_GE == 0
    assert re.search(r"#define\s+AHA_RULE_LT\s+1u", hdr) and N.AHA_RULE_LT == 1
    assert re.search(r"}\s*aha_rule_term;", hdr) and re.search(r"}\s*aha_grep_params;", hdr)
    assert C.sizeof(N.aha_rule_term) == 16
    assert C.sizeof(N.aha_match_params) == 48  # the mirror did not move
    assert N.aha_grep_params.match.offset == 0 and N.aha_grep_params.classes.offset == 48
    assert C.sizeof(N.aha_grep_params) == 48 + 8 + 8 + 4 + 4 + 8
    assert "GREP_RULE" in crystal and "struct RuleTerm" in crystal and "struct GrepParams" in crystal
    assert "AHA_GREP_RULE" in cpp and "aha_grep_params" in cpp and "aha_rule_term" in cpp
    assert len(re.findall(r"^\s+aha_\w+;", listed, re.M)) == 90  # no new entry point
    assert N.lib().aha_abi_version() == 8 and re.search(r"#define\s+AHA_ABI_VERSION\s+8\b", hdr)
    assert callable(AC.rule)
    import inspect
    for method in ("grep_batch", "grep_batch_device", "grep_corpus", "grep"):
        ps = inspect.signature(getattr(AC, method)).parameters
        assert all(ps[k].default is None for k in ("classes", "rule", "rows")), method


class _Buffers:
    def __init__(self):
        self.corpus = np.frombuffer(b"ushershe", dtype=np.uint8).copy()
        self.offs = np.array([0, 6, 8], dtype=np.uint64)
        self.kept = np.full(16, GUARD, dtype=np.uint64)
        self.doo = np.full(17, GUARD, dtype=np.uint64)
        self.out = np.full(64, GUARD, dtype=np.uint8)
        self.rows = np.full(8, GUARD, dtype=np.uint32)

    def untouched(self):
        return all((a == GUARD).all() for a in (self.kept, self.doo, self.out, self.rows))


def _terms(*ts):
    arr = (N.aha_rule_term * max(len(ts), 1))()
    for i, (c, op, g, num, den) in enumerate(ts):
        arr[i] = N.aha_rule_term(c, op, g, num, den)
    return arr


def _gp(table, terms, n_terms=None, struct_size=None, reserved=0, **match):
    gp = N.aha_grep_params()
    gp.match.struct_size = C.sizeof(N.aha_grep_params) if struct_size is None else struct_size
    for k, v in match.items():
        setattr(gp.match, k, v)
    gp.classes = table
    gp.terms = C.cast(terms, C.POINTER(N.aha_rule_term)) if terms is not None else None
    gp.n_terms = len(terms) if n_terms is None else n_terms
    gp.reserved = reserved
    return gp


def _rule_both(m, gp, flags=N.AHA_GREP_RULE, rows=True):
    """rc of the host entry and of the device entry on the same arguments; the buffers, rows included, stay untouched"""
    b = _Buffers()
    nk, nb = C.c_uint64(7), C.c_uint64(7)
    gp.rows = b.rows.ctypes.data if rows else None
    p = C.cast(C.pointer(gp), C.POINTER(N.aha_match_params))
    L = N.lib()
    rc_h = L.aha_ac_grep_batch(m._h, b.corpus.ctypes.data, b.offs.ctypes.data, 2, p, flags, b.kept.ctypes.data, b.doo.ctypes.data, 16,
                               b.out.ctypes.data, 64, C.byref(nk), C.byref(nb), None)
    rc_d = L.aha_ac_grep_batch_device(m._h, b.corpus.ctypes.data, b.offs.ctypes.data, 2, b.corpus.size, p, flags, b.kept.ctypes.data,
                                      b.doo.ctypes.data, 16, b.out.ctypes.data, 64, C.byref(nk), C.byref(nb), None, None)
    assert b.untouched() and nk.value == 7 and nb.value == 7
    return rc_h, rc_d


INVALID2 = (N.AHA_E_INVALID, N.AHA_E_INVALID)
NO_DEVICE2 = (N.AHA_E_NO_DEVICE, N.AHA_E_NO_DEVICE)


@pytest.fixture(scope="module")
def host():
    m = AC.compile(KEYS, host_only=True)
    return m, m.classes(CLASSES)


def test_a_valid_rule_answers_no_device_on_a_host_only_handle(host):
    m, t = host
    one = _terms((0, N.AHA_RULE_GE, 0, 2, 0))
    assert _rule_both(m, _gp(t._h, one)) == NO_DEVICE2
    assert _rule_both(m, _gp(t._h, one), flags=N.AHA_GREP_RULE | N.AHA_GREP_INVERT) == NO_DEVICE2
    assert _rule_both(m, _gp(t._h, one), rows=False) == NO_DEVICE2
    assert _rule_both(m, _gp(t._h, one, sep_size=40)) == NO_DEVICE2  # a separator filter is allowed
    full = _terms(*[(i & 1, i & 1, i // 8, i, i % 3) for i in range(64)])
    assert _rule_both(m, _gp(t._h, full)) == NO_DEVICE2
    assert _rule_both(m, _gp(t._h, one, struct_size=C.sizeof(N.aha_grep_params) + 8)) == NO_DEVICE2  # a later, larger struct
    rule = m.rule([[(0, ">=", 2)]], t)
    for call in (lambda: m.grep_batch(b"ushershe", [0, 6, 8], rule=rule), lambda: m.grep(b"ushers\nhe", rule=rule),
                 lambda: m.grep_batch(b"ushershe", [0, 6, 8], rule=[[(1, "<", 1)]], classes=t, invert=True)):
        with pytest.raises(AhaError) as e:
            call()
        assert e.value.code == N.AHA_E_NO_DEVICE


def test_rule_refusals_come_before_the_device_check(host):
    m, t = host
    one = _terms((0, N.AHA_RULE_GE, 0, 2, 0))
    # flag 4 with a struct that is too small; 2 and 3 stay refused, and so do they beside 4
    assert _rule_both(m, _gp(t._h, one, struct_size=C.sizeof(N.aha_match_params))) == INVALID2
    assert _rule_both(m, _gp(t._h, one, struct_size=C.sizeof(N.aha_grep_params) - 1)) == INVALID2
    for flags in (2, 3, 6, 7, 8 | 4, 0x80000000 | 4):
        assert _rule_both(m, _gp(t._h, one), flags=flags) == INVALID2
    # the table
    assert _rule_both(m, _gp(None, one)) == INVALID2
    other = AC.compile(KEYS, host_only=True)
    t2 = other.classes(CLASSES)
    assert _rule_both(m, _gp(t2._h, one)) == INVALID2
    assert "the class table was made for another handle" in N.lib().aha_last_error(None).decode()
    # the terms
    assert _rule_both(m, _gp(t._h, None, n_terms=1)) == INVALID2
    assert _rule_both(m, _gp(t._h, one, n_terms=0)) == INVALID2
    big = _terms(*[(0, 0, 0, 1, 0)] * 65)
    assert _rule_both(m, _gp(t._h, big)) == INVALID2
    assert _rule_both(m, _gp(t._h, big, n_terms=64)) == NO_DEVICE2
    assert _rule_both(m, _gp(t._h, one, reserved=1)) == INVALID2
    assert _rule_both(m, _gp(t._h, _terms((0, 2, 0, 1, 0)))) == INVALID2  # an op above 1
    assert _rule_both(m, _gp(t._h, _terms((0, 0, 0, 1, 0), (1, 0xFFFF, 0, 1, 0)))) == INVALID2
    assert _rule_both(m, _gp(t._h, _terms((2, 0, 0, 1, 0)))) == INVALID2  # class_id >= n_classes
    assert _rule_both(m, _gp(t._h, _terms((1, 0, 0, 1, 0), (0xFFFFFFFF, 1, 9, 1, 0)))) == INVALID2
    # everything grep refuses
    assert _rule_both(m, _gp(t._h, one, char_offsets=1)) == INVALID2
    for longest in (1, 2):
        assert _rule_both(m, _gp(t._h, one, longest=longest)) == INVALID2
    assert _rule_both(m, _gp(t._h, one, sep_size=257)) == (N.AHA_E_SEP_SIZE, N.AHA_E_SEP_SIZE)
    L = N.lib()
    b = _Buffers()
    n = C.c_uint64(0)
    gp = _gp(t._h, one)
    p = C.cast(C.pointer(gp), C.POINTER(N.aha_match_params))
    # NULL params, n_kept, handle; a NULL buffer with a capacity; out overlapping the corpus
    assert L.aha_ac_grep_batch(m._h, b.corpus.ctypes.data, b.offs.ctypes.data, 2, None, 4, None, None, 0, None, 0, C.byref(n), None,
                               None) == N.AHA_E_INVALID
    assert L.aha_ac_grep_batch_device(m._h, b.corpus.ctypes.data, b.offs.ctypes.data, 2, 8, None, 4, None, None, 0, None, 0, C.byref(n),
                                      None, None, None) == N.AHA_E_INVALID
    assert L.aha_ac_grep_batch(m._h, b.corpus.ctypes.data, b.offs.ctypes.data, 2, p, 4, None, None, 0, None, 0, None, None,
                               None) == N.AHA_E_INVALID
    assert L.aha_ac_grep_batch(None, b.corpus.ctypes.data, b.offs.ctypes.data, 2, p, 4, None, None, 0, None, 0, C.byref(n), None,
                               None) == N.AHA_E_INVALID
    assert L.aha_ac_grep_batch(m._h, b.corpus.ctypes.data, b.offs.ctypes.data, 2, p, 4, None, None, 3, None, 0, C.byref(n), None,
                               None) == N.AHA_E_INVALID
    assert L.aha_ac_grep_batch(m._h, b.corpus.ctypes.data, b.offs.ctypes.data, 2, p, 4, None, None, 0, None, 9, C.byref(n), None,
                               None) == N.AHA_E_INVALID
    assert L.aha_ac_grep_batch_device(m._h, b.corpus.ctypes.data, b.offs.ctypes.data, 2, 8, p, 4, None, None, 0,
                                      b.corpus.ctypes.data + 2, 8, C.byref(n), None, None, None) == N.AHA_E_INVALID
    assert b.untouched()


def test_without_the_flag_struct_size_changes_nothing(host):
    m, t = host
    # a plain grep call whose params claim a larger struct (and hold rubbish behind the match params) is the call it was
    gp = _gp(None, None, n_terms=99, reserved=5)
    assert _rule_both(m, gp, flags=0) == NO_DEVICE2
    assert _rule_both(m, gp, flags=N.AHA_GREP_INVERT) == NO_DEVICE2


def test_ac_rule_validates_on_the_host(host):
    m, t = host
    r = m.rule([[(0, ">=", 2)], [(0, ">=", 1), (1, "<", 1, 1000)]], t)
    assert isinstance(r, Rule) and r.classes is t
    assert r.terms == ((0, 0, 0, 2, 0), (0, 0, 1, 1, 0), (1, 1, 1, 1, 1000))
    with pytest.raises(AttributeError):
        r.terms = ()
    named = m.classes({"pron": ["he", "she"], "fem": ["she"]})
    assert m.rule([[("fem", "<", 1), ("pron", ">=", 1)]], named).terms == ((1, 1, 0, 1, 0), (0, 0, 0, 1, 0))
    assert m.rule([[(0, ">=", 1)]], CLASSES).classes.n_classes == 2  # a spec of AC.classes is taken too
    for bad in ([[(0, ">", 1)]], [[(0, "==", 1)]], [[(0, 0, 1)]],  # an unknown op
                [[(2, ">=", 1)]], [[(-1, ">=", 1)]], [[("nope", ">=", 1)]],  # a class out of range
                [], [[]], [[(0, ">=", 1)] * 65], [[(0, ">=", 1)] * 33, [(1, "<", 1)] * 32],  # 0 or 65 terms
                [[(0, ">=")]], [[(0, ">=", -1)]], [[(0, ">=", 1 << 32)]], [[(0, ">=", 1, -5)]], [(0, ">=", 1)]):
        with pytest.raises(ValueError):
            m.rule(bad, t)
    assert len(m.rule([[(0, ">=", 1)] * 64], t).terms) == 64
    with pytest.raises(ValueError):
        m.grep_batch(b"he", [0, 2], classes=t)  # classes without a rule
    with pytest.raises(ValueError):
        m.grep_batch(b"he", [0, 2], rows=np.zeros((1, 2), np.uint32))
    with pytest.raises(ValueError):
        m.grep_batch(b"he", [0, 2], rule=[[(0, ">=", 1)]])  # a spec without classes
    with pytest.raises(ValueError):
        m.grep_batch(b"he", [0, 2], rule=r, rows=np.zeros((2, 2), np.uint32))  # rows of another shape
    with pytest.raises(ValueError):
        m.grep_batch(b"he", [0, 2], rule=r, classes=named)


def test_worked_example_of_the_header():
    o = orc.AC.compile([k.encode() for k in KEYS])
    text = b"ushershe"
    corpus = np.frombuffer(text, dtype=np.uint8)
    offs = np.array([0, 6, 8], dtype=np.uint64)
    hits, dho = o.match_batch(corpus, offs)
    per_doc = classsim.split_hits(hits["value"], dho)
    ids, coff = classsim.pack_classes(CLASSES)
    want = {  # the rule -> the kept documents
        ((0, rulesim.GE, 0, 2, 0),): [0],
        ((0, rulesim.GE, 0, 1, 0), (1, rulesim.LT, 0, 1, 0)): [1],
        ((0, rulesim.GE, 0, 1, 3),): [0, 1],
    }
    for terms, kept_want in want.items():
        kept, out, doo, rows, ok = rulesim.grep(per_doc, ids, coff, 2, offs, corpus, terms, False)
        assert rows.tolist() == [[2, 1], [1, 0]]
        assert kept.tolist() == kept_want, terms
        assert out.tobytes() == b"".join([b"ushers", b"he"][d] for d in kept_want)
        inv = rulesim.grep(per_doc, ids, coff, 2, offs, corpus, terms, True)[0]
        assert inv.tolist() == [d for d in (0, 1) if d not in kept_want]
    # OR over groups with arbitrary ids in any order: {c0 >= 2} (group 7) or {c0 >= 1 and c1 < 1} (group 3) keeps both
    mixed = ((0, rulesim.GE, 3, 1, 0), (0, rulesim.GE, 7, 2, 0), (1, rulesim.LT, 3, 1, 0))
    assert rulesim.passes([[2, 1], [1, 0]], offs, mixed).tolist() == [True, True]
    # an empty document follows the formula: 0 * den >= num * 0 holds, 0 * den < num * 0 does not
    assert rulesim.passes([[0, 0]], [0, 0], ((0, rulesim.GE, 0, 5, 1000),)).tolist() == [True]
    assert rulesim.passes([[0, 0]], [0, 0], ((0, rulesim.LT, 0, 5, 1000),)).tolist() == [False]
    # the products do not wrap: a count of 2^32 - 1 per 2^32 - 1 bytes against num 2^32 - 1 over 2^31 - 1 bytes
    top = (1 << 32) - 1
    assert rulesim.passes(np.array([[top]], dtype=np.uint64), [0, (1 << 31) - 1], ((0, rulesim.GE, 0, top, top),)).tolist() == [True]


def test_edges_model_equals_the_direct_definition():
    """kgq_edges reads a word and one bit of each neighbour, so a bit of S or T depends on three neighbouring documents, on D
    and on where the word ends.  Every mask for D <= 12; for every D up to 70 every 6-document pattern at every position in an
    all-kept and in an all-dropped batch (every neighbourhood at every position, word ends and the batch's ends included) and
    random masks; random masks at the rank block's edge."""
    def same(keep):
        got = rulesim.kernel_model(rulesim.pack_bits(keep), len(keep))
        want = rulesim.edges(keep)
        return np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])

    for D in range(1, 13):
        for bits in itertools.product((False, True), repeat=D):
            assert same(np.array(bits)), bits
    rng = random.Random(5)
    pats = [np.array(p) for p in itertools.product((False, True), repeat=6)]
    for D in range(13, 71):
        for back in (False, True):
            for at in range(0, D - 5):
                for p in pats[:: 1 if at % 8 in (0, 5, 6, 7) or at > D - 9 else 7]:
                    keep = np.full(D, back)
                    keep[at:at + 6] = p
                    assert same(keep), (D, at, p)
        for _ in range(20):
            assert same(np.array([rng.random() < 0.5 for _ in range(D)]))
    for D in (2047, 2048, 2049):
        for dense in (0.02, 0.5, 0.98):
            for _ in range(4):
                assert same(np.random.RandomState(rng.randrange(1 << 30)).rand(D) < dense), D
        assert same(np.zeros(D, dtype=bool)) and same(np.ones(D, dtype=bool))


def test_cpp_grep_rule_example_compiles(tmp_path):
    from test_gpu_grep_rule_cpp import build_spec_grep_rule

    build_spec_grep_rule(tmp_path)
