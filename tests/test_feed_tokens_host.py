"""CPU tests of the feed token calls (aha_feed_select_batch* with AHA_FEED_SELECT_TOKENS): the stream laws on the model
(feedtokensim) against tokensim on whole sequences, over the CPU oracle's hits; the header's examples; the constants; the flag
refusals that come before any device work; the bindings; the build lists; and the edge decision of feedtok_edge.hpp as a
stand-alone program under AddressSanitizer and UBSan."""
import os
import random
import re
import subprocess

import feedtokensim as fts
import pyoracle as orc
import selectsim
import tokensim
from aha_amd import Feed, Segmenter
from aha_amd import _native as N
from test_feed_select_host import _both, _cut

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
UNITS = [b"a", b"b", b"c", "中".encode(), "é".encode(), b"\x80", b"\xff"]


def _word(rng, alpha, lo, hi):
    return b"".join(rng.choice(alpha) for _ in range(rng.randint(lo, hi)))


def _law(keys, text, cuts):
    """both laws for one cut sequence -> (a token was held beyond W, a gap arrived in parts)"""
    match, W = fts.oracle_match(orc.AC.compile(keys)), fts.window(keys)
    sel = selectsim.select_doc(match(text))
    pieces = _cut(text, cuts)
    holds = []
    got = fts.stream(match, W, pieces, holds=holds)
    assert got == tokensim.tokens_doc(text, sel), (keys, text, cuts)
    assert holds[-1] == 0
    runs = fts.stream(match, W, pieces, gap_runs=True)
    assert fts.join_gaps(runs) == tokensim.tokens_doc(text, sel, gap_runs=True), (keys, text, cuts)
    assert b"".join(text[s:e] for s, e, _ in got) == text == b"".join(text[s:e] for s, e, _ in runs)
    return any(h > W for h in holds), fts.join_gaps(runs) != runs


def test_stream_laws_random_small_alphabets():
    rng = random.Random(20261)
    held_beyond, in_parts = 0, 0
    for case in range(1200):
        alpha = UNITS[: rng.randint(2, len(UNITS))]
        if case % 7 == 0:  # W = 0: keys of one byte
            keys = sorted({bytes([rng.choice(b"abc\x80\xa9")]) for _ in range(rng.randint(1, 3))})
        else:
            keys = sorted({_word(rng, alpha, 1, 4) for _ in range(rng.randint(1, 6))})
        if case % 3 == 0:  # byte-level keys that cut a character
            keys = sorted(set(keys) | {"中".encode()[1:], "é".encode()[:1]})
        text = _word(rng, alpha, 0, 24)
        cuts = [rng.randint(0, len(text)) for _ in range(rng.randint(0, 6))]  # (equal cuts: empty pieces)
        a, b = _law(keys, text, cuts)
        held_beyond += a
        in_parts += b
    assert held_beyond > 50 and in_parts > 50, (held_beyond, in_parts)


def test_stream_laws_every_cut_of_short_sequences():
    cases = [([b"ab", b"abcde"], b"xabcdeabab"), ([b"a"], b"xa\xc3\xa9y"), (["是".encode()], "我是中".encode()),
             ([b"\x98"], "我是".encode()), ([b"ab"], b"a\x80\x80\x80b\x80ab")]
    for keys, text in cases:
        for i in range(len(text) + 1):
            for j in range(i, len(text) + 1):
                _law(keys, text, [i, j])


def _run(keys, pieces, gap_runs=False):
    q = fts.Sequence(fts.oracle_match(orc.AC.compile(keys)), fts.window(keys))
    out = []
    for i, p in enumerate(pieces):
        toks, hold, base = q.push(p, final=i == len(pieces) - 1, gap_runs=gap_runs)
        out.append(([(s + base, e + base, v) for s, e, v in toks], hold))
    return out


def test_the_examples_of_the_header():
    assert _run([b"ab", b"abcde"], [b"xab", b"cd", b"eab", b""]) == [([], 3), ([(0, 1, -1)], 4), ([(1, 6, 1)], 2), ([(6, 8, 0)], 0)]
    q = fts.Sequence(fts.oracle_match(orc.AC.compile([b"ab", b"abcde"])), 4)
    q.push(b"xab")
    assert q.push(b"cd")[0] == [(-3, -2, -1)]  # relative to the piece
    u = "我是中".encode()
    assert _run(["是".encode()], [u[:4], u[4:8], u[8:], b""]) == [([], 4), ([(0, 3, -1), (3, 6, 0)], 2), ([], 3), ([(6, 9, -1)], 0)]
    assert _run([b"a"], [b"xa\xc3", b"\xa9", b"y", b""]) == [([(0, 1, -1), (1, 2, 0)], 1), ([], 2), ([(2, 4, -1)], 1), ([(4, 5, -1)], 0)]
    got = _run([b"ab"], [b"zzzzzz", b"zzab", b"zz"], gap_runs=True)
    assert got == [([(0, 5, -1)], 1), ([(5, 8, -1), (8, 10, 0)], 0), ([(10, 12, -1)], 0)]
    assert fts.join_gaps(sum((t for t, _ in got), []))[0] == (0, 8, -1)


def test_constants_agree_and_no_entry_point_is_added():
    hdr = open(os.path.join(ROOT, "include", "aha_hip.h")).read()
    crystal = open(os.path.join(ROOT, "bindings", "crystal", "aha_hip.cr")).read()
    for name, value in (("AHA_FEED_SELECT_TOKENS", 4), ("AHA_FEED_SELECT_GAP_RUNS", 8)):
        m = re.search(r"^#define %s\s+(\d+)u\b" % name, hdr, re.M)
        assert m and int(m.group(1)) == value == getattr(N, name), name
        assert re.search(r"%s\s*=\s*%d_u32" % (name[len("AHA_"):], value), crystal), name
    assert N.AHA_FEED_SELECT_TOKENS == N.AHA_SELECT_TOKENS and N.AHA_FEED_SELECT_GAP_RUNS == N.AHA_SELECT_GAP_RUNS
    listed = open(os.path.join(ROOT, "aha_amd", "csrc", "exports.map")).read()
    assert len(re.findall(r"^\s+aha_\w+;", listed, re.M)) == 90 and N.lib().aha_abi_version() == 8


def test_flag_refusals_before_any_device_work():
    for flags in (8, 8 | 1, 16, 2 | 4):
        assert _both(None, flags=flags) == (N.AHA_E_INVALID, N.AHA_E_INVALID), flags


def test_bindings_have_the_token_calls():
    for name in ("tokens_batch", "tokens_batch_device", "tokens", "segmenter"):
        assert callable(getattr(Feed, name)), name
    assert callable(Segmenter.push) and callable(Segmenter.finish)
    crystal = open(os.path.join(ROOT, "bindings", "crystal", "aha_hip.cr")).read()
    cxx = open(os.path.join(ROOT, "include", "aha", "ac.hpp")).read()
    assert len(re.findall(r"^\s*def tokens\(", crystal, re.M)) == 2  # (AC#tokens and Feed#tokens)
    assert "AHA_FEED_SELECT_TOKENS" in cxx and len(re.findall(r"\bstd::vector<Hit> tokens_batch\(std::string_view corpus", cxx)) == 2


class _ModelFeed:
    """what Segmenter needs of a Feed, answered by the model"""

    def __init__(self, keys):
        self._m = fts.Feed(fts.oracle_match(orc.AC.compile(keys)), fts.window(keys), 4)

    def tokens_batch(self, corpus, piece_offsets, seq_ids, final=False, gap_runs=False, cap=None):
        toks, pto, bases, hold = self._m.call([bytes(corpus)], [int(seq_ids[0])], final, gap_runs)
        return toks, {"piece_tok_offsets": pto, "piece_bases": bases, "piece_hold": hold, "n_hits": 0}


def test_segmenter_arithmetic_on_the_model():
    rng = random.Random(5)
    for case in range(200):
        alpha = UNITS[: rng.randint(2, len(UNITS))]
        keys = sorted({_word(rng, alpha, 1, 4) for _ in range(rng.randint(1, 5))})
        text = _word(rng, alpha, 0, 24)
        sel = selectsim.select_doc(fts.oracle_match(orc.AC.compile(keys))(text))
        for gap_runs in (False, True):
            g = Segmenter(_ModelFeed(keys), gap_runs)
            got = []
            for p in _cut(text, [rng.randint(0, len(text)) for _ in range(rng.randint(0, 5))]):
                got += g.push(case % 4, p)
            got += g.finish(case % 4)
            assert b"".join(b for b, _ in got) == text and not g._held
            if not gap_runs:
                assert got == [(text[s:e], v) for s, e, v in tokensim.tokens_doc(text, sel)], (keys, text)


def test_makefile_lists_the_new_sources():
    mk = open(os.path.join(ROOT, "aha_amd", "csrc", "Makefile")).read()
    assert mk.count("scan_feedtokens.hip") == 1 and mk.count("feedtok_edge.hpp") == 1
    assert mk.count("feedtok_stubs.cpp") == 2
    stubs = open(os.path.join(ROOT, "tests", "cpp", "feedtok_stubs.cpp")).read()
    decl = open(os.path.join(ROOT, "aha_amd", "csrc", "feed.hpp")).read()
    names = set(re.findall(r"\bvoid (feedtok_launch_\w+)\(", decl))
    assert len(names) == 5 and names == set(re.findall(r"\bvoid (feedtok_launch_\w+)\(", stubs))


def test_spec_feedtok_edge_runs_clean_under_asan_and_ubsan(tmp_path):
    exe = str(tmp_path / "spec_feedtok_edge")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           os.path.join(ROOT, "tests", "cpp", "spec_feedtok_edge.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert " 0 failure(s)" in r.stdout


def test_cpp_feed_tokens_example_compiles(tmp_path):
    from test_gpu_feed_tokens_cpp import build_spec_feed_tokens

    build_spec_feed_tokens(tmp_path)
