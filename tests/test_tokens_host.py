"""CPU tests of the token calls (aha_ac_select_batch* with AHA_SELECT_TOKENS): no new entry point -- the exports and the ABI
stay; the flag table and select's refusals with the token bit set, all before any device work, so they hold on a host-only
handle; the constants; the bytewise statement of the contract (tokensim) against an independent formulation (a sequential
forward-maximum-matching loop over the oracle's hits); the per-word rule of token_rule.hpp and the tiling rule of
doc_ranges.hpp as stand-alone programs under AddressSanitizer and UBSan; the build lists."""
import ctypes as C
import os
import random
import re
import subprocess

import numpy as np
import pytest

import selectsim
import tokensim
from aha_amd import AC, AhaError, BitArray
from aha_amd import _native as N
from test_select_host import _both, _oracle_docs, _params

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOK, RUNS = 4, 8


def test_tokens_add_no_entry_point_and_constants_match_the_header():
    listed = open(os.path.join(ROOT, "aha_amd", "csrc", "exports.map")).read()
    assert len(re.findall(r"^\s+aha_\w+;", listed, re.M)) == 90
    assert N.lib().aha_abi_version() == 8
    hdr = open(os.path.join(ROOT, "include", "aha_hip.h")).read()
    for name, value in (("AHA_SELECT_TOKENS", TOK), ("AHA_SELECT_GAP_RUNS", RUNS)):
        m = re.search(r"^#define %s\s+(\d+)u\b" % name, hdr, re.M)
        assert m and int(m.group(1)) == value == getattr(N, name), name
    crystal = open(os.path.join(ROOT, "bindings", "crystal", "aha_hip.cr")).read()
    assert re.search(r"SELECT_TOKENS\s*=\s*4_u32", crystal) and re.search(r"SELECT_GAP_RUNS\s*=\s*8_u32", crystal)
    assert re.search(r"^\s*def tokens\(", crystal, re.M)


def test_token_flag_table():
    m = AC.compile(["he", "she", "hers"], host_only=True)
    for flags in (TOK, TOK | RUNS):  # accepted as far as a host-only handle goes
        assert _both(m, _params(), flags=flags) == (N.AHA_E_NO_DEVICE, N.AHA_E_NO_DEVICE)
    for flags in (RUNS, TOK | 1, TOK | 2, TOK | 0x80000000, TOK | RUNS | 16):
        assert _both(m, _params(), flags=flags) == (N.AHA_E_INVALID, N.AHA_E_INVALID), flags


def test_token_flag_keeps_the_refusals_of_select():
    m = AC.compile(["he", "she", "hers"], host_only=True)
    for flags in (TOK, TOK | RUNS):
        assert _both(m, _params(char_offsets=1), flags=flags) == (N.AHA_E_INVALID, N.AHA_E_INVALID)
        for longest in (1, 2):
            assert _both(m, _params(longest=longest), flags=flags) == (N.AHA_E_INVALID, N.AHA_E_INVALID)
        assert _both(m, _params(sep_size=257), flags=flags) == (N.AHA_E_SEP_SIZE, N.AHA_E_SEP_SIZE)
        assert _both(m, _params(), n=False, flags=flags) == (N.AHA_E_INVALID, N.AHA_E_INVALID)
        L = N.lib()
        n = C.c_uint64(0)
        assert L.aha_ac_select_batch(None, None, None, 0, None, flags, None, 0, None, C.byref(n), None) == N.AHA_E_INVALID
        assert L.aha_ac_select_batch_device(None, None, None, 0, 0, None, flags, None, 0, None, C.byref(n), None, None) == N.AHA_E_INVALID
    for call in (lambda: m.tokens("ushers"), lambda: m.tokens(b"ushers"), lambda: m.segment("ushers"),
                 lambda: m.tokens_batch(b"ushers", [0, 6], gap_runs=True)):
        with pytest.raises(AhaError) as e:
            call()
        assert e.value.code == N.AHA_E_NO_DEVICE
    with pytest.raises(AhaError) as e:
        m.tokens_batch(b"ushers", [0, 6], sep=BitArray(300))
    assert e.value.code == N.AHA_E_SEP_SIZE


# ---- tokensim against an independent formulation ---------------------------------------------------------------------------
def _fmm(doc, hits, gap_runs):
    """forward maximum matching of ONE document, sequentially: at p take the longest hit that starts at p; where none starts,
    one character (the byte at p and the continuation bytes behind it) -- or, with gap_runs, everything up to the next
    position where a hit starts -- as an unknown token.  hits: the document's (start, end, value), any order."""
    longest = {}
    for s, e, v in hits:
        if s not in longest or e > longest[s][0]:
            longest[s] = (e, v)
    out, p, n = [], 0, len(doc)
    while p < n:
        if p in longest:
            e, v = longest[p]
            out.append((p, e, v))
            p = e
            continue
        q = p + 1
        while q < n and q not in longest and (gap_runs or (doc[q] & 0xC0) == 0x80):
            q += 1
        out.append((p, q, -1))
        p = q
    return out


def _sim_against_fmm(keys, docs, sep=None):
    hits, dho = _oracle_docs(keys, docs, sep)
    sel, dso = selectsim.select(hits, dho)
    corpus = np.frombuffer(b"".join(docs), dtype=np.uint8)
    offs = np.cumsum([0] + [len(d) for d in docs]).astype(np.uint64)
    n_unknown = 0
    for gap_runs in (False, True):
        toks, dto = tokensim.tokens(corpus, offs, sel, dso, gap_runs)
        tokensim.check_invariants(toks, dto, corpus, offs, sel, dso, gap_runs)
        for d, doc in enumerate(docs):
            H = [tuple(x) for x in hits[int(dho[d]):int(dho[d + 1])].tolist()]
            T = [tuple(x) for x in toks[int(dto[d]):int(dto[d + 1])].tolist()]
            assert T == _fmm(doc, H, gap_runs), (keys, doc, gap_runs)
            n_unknown += sum(1 for t in T if t[2] < 0)
    return n_unknown


def test_tokensim_on_the_readme_example_and_named_cases():
    keys = ["我是", "中国"]
    b = "我是中国人".encode()
    assert tokensim.tokens_doc(b, [(0, 6, 0), (6, 12, 1)]) == [(0, 6, 0), (6, 12, 1), (12, 15, -1)]
    assert _sim_against_fmm([k.encode() for k in keys], [b, b"", b[1:], b[:-1]]) > 0
    # a stray run of continuation bytes joins the token in front; a document cut inside a character starts a token there
    assert tokensim.tokens_doc(b"a" + b"\x80" * 5 + b"b", []) == [(0, 6, -1), (6, 7, -1)]
    assert tokensim.tokens_doc(b"\x80\x80a", []) == [(0, 2, -1), (2, 3, -1)]
    assert tokensim.tokens_doc(b"\x80\x80a", [], gap_runs=True) == [(0, 3, -1)]
    # a byte-level key that starts on a continuation byte starts a token there, and a gap follows it at once
    assert tokensim.tokens_doc("我x".encode(), [(1, 3, 0)]) == [(0, 1, -1), (1, 3, 0), (3, 4, -1)]
    assert tokensim.tokens_doc(b"ab\x80\x80c", [(0, 2, 7)]) == [(0, 2, 7), (2, 4, -1), (4, 5, -1)]


def test_tokensim_on_random_small_alphabets():
    rng = random.Random(4242)
    unknown = 0
    sep = (256, [i for i in range(256) if chr(i) not in "ab"])
    units = ["a", "b", "c", "中", "é", "\x80", "\xff"]
    for trial in range(120):
        alpha = units[: rng.randint(2, len(units))]

        def word(lo, hi):
            return b"".join(u.encode("latin-1") if ord(u) in (0x80, 0xFF) else u.encode() for u in
                            (rng.choice(alpha) for _ in range(rng.randint(lo, hi))))

        keys = sorted({word(1, 4) for _ in range(rng.randint(1, 8))})
        if rng.random() < 0.3:  # byte-level keys: cut inside a character
            keys = sorted(set(keys) | {"中".encode()[1:], "é".encode()[:1]})
        docs = [word(0, 30) for _ in range(4)]
        unknown += _sim_against_fmm(keys, docs)
        _sim_against_fmm(keys, docs, sep)
    assert unknown > 0


# ---- the per-word rule and the build -----------------------------------------------------------------------------------------
def test_spec_token_rule_runs_clean_under_asan_and_ubsan(tmp_path):
    exe = str(tmp_path / "spec_token_rule")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           os.path.join(ROOT, "tests", "cpp", "spec_token_rule.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert " 0 failure(s)" in r.stdout


def test_spec_doc_tiles_runs_clean_under_asan_and_ubsan(tmp_path):
    """the ranges of a token call (doc_ranges.hpp doc_tiles): they tile every document and keep both bounds"""
    exe = str(tmp_path / "spec_doc_tiles")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           os.path.join(ROOT, "tests", "cpp", "spec_doc_tiles.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert " 0 failure(s)" in r.stdout


def test_makefile_lists_the_new_sources():
    mk = open(os.path.join(ROOT, "aha_amd", "csrc", "Makefile")).read()
    assert mk.count("scan_tokens.hip") == 1 and mk.count("token_rule.hpp") == 1
    assert mk.count("token_stubs.cpp") == 2
    stubs = open(os.path.join(ROOT, "tests", "cpp", "token_stubs.cpp")).read()
    decl = open(os.path.join(ROOT, "aha_amd", "csrc", "image.hpp")).read()
    names = set(re.findall(r"\bvoid (tokens_launch_\w+)\(", decl))
    assert len(names) == 3 and names == set(re.findall(r"\bvoid (tokens_launch_\w+)\(", stubs))


def test_cpp_tokens_example_compiles(tmp_path):
    from test_gpu_tokens_cpp import build_spec_tokens

    build_spec_tokens(tmp_path)
