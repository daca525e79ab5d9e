"""Longest feeds without a GPU (aha_feed_open_params with longest = 1 | 2): the CPU model against the oracle at every cut, the
argument checks of the open call on a host-only handle, the shared step under the sanitizers as its own process, and the
surface (exports, ABI, stubs, documents)."""
import ctypes as C
import os
import re
import subprocess

import pytest

import pyoracle as orc
from aha_amd import AC, AhaError
from aha_amd import _native as N
from feedlongestsim import CASES, FeedLongestSim, absolute, case_keys, case_text

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "aha_amd", "csrc")


def rows(h):
    return [(int(x["start"]), int(x["end"]), int(x["value"])) for x in h]


@pytest.mark.parametrize("mode", [1, 2])
@pytest.mark.parametrize("name", CASES)
def test_model_is_the_oracle_at_every_cut(name, mode):
    keys, stale = case_keys(name)
    if name == "stale":
        assert stale
    o = orc.AC.compile(keys)
    text = case_text(name, keys)
    assert len(text) == (230 if name == "long" else 60) and b"\x00" in text
    isect = mode == 2
    want = rows(o.match_longest(text, intersectable=isect, chars=False))
    assert want
    lmax = max(len(k) for k in keys)
    prefix = {n: rows(o.match_longest(text[:n], intersectable=isect, chars=False)) if n else [] for n in range(len(text) + 1)}

    def bounded(h):
        assert all(a >= -lmax and e >= -(lmax - 1) for a, e, _ in rows(h)), rows(h)

    for cut in range(len(text) + 1):
        sim = FeedLongestSim(keys, 2, isect, stale)
        h0, b0 = sim.piece(0, text[:cut])
        assert b0 == 0
        # the calls up to the cut plus a finish there are the oracle on the prefix: on a second sequence, so the first goes on
        sim.piece(1, text[:cut])
        f1, n1 = sim.finish(1)
        assert n1 == cut and len(f1) <= 1 and all(e <= 0 for _, e, _ in rows(f1))
        assert rows(h0) + rows(absolute(f1, n1)) == prefix[cut], cut
        h1, b1 = sim.piece(0, text[cut:])
        assert b1 == cut
        bounded(h1)
        f0, n0 = sim.finish(0)
        assert n0 == len(text) and len(f0) <= 1
        assert rows(h0) + rows(absolute(h1, b1)) + rows(absolute(f0, n0)) == want, cut
        assert sim.position(0) == 0  # it started again
    sim = FeedLongestSim(keys, 1, isect, stale)
    got = []
    for i in range(len(text)):
        assert rows(sim.piece(0, b"")[0]) == []  # a zero-length piece reports nothing and changes nothing
        h, b = sim.piece(0, text[i:i + 1])
        assert b == i
        bounded(h)
        got += rows(absolute(h, b))
        assert len(h) <= 1
    f, n = sim.finish(0)
    assert got + rows(absolute(f, n)) == want


def test_model_folds_and_resets():
    sim = FeedLongestSim([b"he", b"hers"], 1, False, fold=True)
    assert rows(sim.piece(0, b"HeR")[0]) == []
    assert rows(sim.piece(0, b"Sx")[0]) == [(-3, 1, 1)]  # yielded at 'x'
    sim.piece(0, b"he")
    sim.reset(0)
    assert rows(sim.finish(0)[0]) == []  # reset drops the pending end
    sim.piece(0, b"he")
    assert rows(sim.finish(0)[0]) == [(-2, 0, 0)]


def _params(**kw):
    p = N.aha_match_params()
    p.struct_size = C.sizeof(N.aha_match_params)
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def _open(m, n_seqs, flags, p):
    h = C.c_void_p()
    rc = N.lib().aha_feed_open_params(m._h, n_seqs, flags, C.byref(p), C.byref(h))
    assert not h.value
    return rc, N.lib().aha_last_error(None).decode()


def test_longest_feed_open_checks():
    m = AC.compile(["he", "she", "hers"], host_only=True)
    # valid arguments: the handle without a device is noticed, and only then
    assert _open(m, 4, 0, _params(longest=1))[0] == N.AHA_E_NO_DEVICE
    assert _open(m, 4, 0, _params(longest=2))[0] == N.AHA_E_NO_DEVICE
    refused = [_open(m, 4, 0, _params(longest=3)), _open(m, 4, 0, _params(longest=-1)), _open(m, 4, 0, _params(longest=1, char_offsets=1)),
               _open(m, 4, N.AHA_FEED_CHARS, _params(longest=1)), _open(m, 4, 0, _params(sep_size=16, longest=1))]
    assert [rc for rc, _ in refused] == [N.AHA_E_INVALID] * 5
    texts = [t for _, t in refused]
    assert texts[0] == texts[1] and len(set(texts[1:])) == 4 and all(texts)
    assert _open(m, 4, 0, _params(char_offsets=1))[0] == N.AHA_E_INVALID  # as before
    with pytest.raises(AhaError) as e:
        m.feed(4, longest=2)
    assert e.value.code == N.AHA_E_NO_DEVICE
    for kw in (dict(longest=3), dict(longest=1, chars=True)):
        with pytest.raises(AhaError) as e:
            m.feed(4, **kw)
        assert e.value.code == N.AHA_E_INVALID
    # a handle folded beyond ASCII stays refused as it is
    with pytest.raises(AhaError) as e:
        AC.compile(["he"], host_only=True, fold_simple=True).feed(4, longest=1)
    assert e.value.code == N.AHA_E_INVALID
    # no new symbol, no ABI bump
    assert N.lib().aha_abi_version() == 8
    listed = open(os.path.join(CSRC, "exports.map")).read()
    assert len(re.findall(r"^\s+aha_\w+;", listed, re.M)) == 90


def test_spec_feed_longest_runs_clean_under_asan_and_ubsan(tmp_path):
    exe = str(tmp_path / "spec_feed_longest")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           os.path.join(ROOT, "tests", "cpp", "spec_feed_longest.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "spec_feed_longest: ok" in r.stdout


def test_cpp_feed_longest_spec_compiles(tmp_path):
    from test_gpu_feed_longest import build_spec_feed_longest

    assert os.path.exists(build_spec_feed_longest(tmp_path))


def test_host_only_sanitizer_library_lists_the_new_stub():
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert mk.count("../../tests/cpp/feed_longest_stubs.cpp") == 2 and os.path.exists(os.path.join(ROOT, "tests", "cpp", "feed_longest_stubs.cpp"))
    assert "scan_feedlongest.hip" in mk and "longest_step.hpp" in mk


def test_feed_kernels_take_the_step_from_the_header():
    """the feed's kernels and the sanitizer spec build on longest_step.hpp; kernels.hip keeps its own copy (the batch kernels
    measured slower on the header: DESIGN 4.10) with the same constants"""
    feed = open(os.path.join(CSRC, "scan_feedlongest.hip")).read()
    assert '#include "longest_step.hpp"' in feed and "longest_step<Probe<COMPACT>>" in feed and "tp[-1]" not in feed
    assert '#include "../../aha_amd/csrc/longest_step.hpp"' in open(os.path.join(ROOT, "tests", "cpp", "spec_feed_longest.cpp")).read()
    hdr, batch = open(os.path.join(CSRC, "longest_step.hpp")).read(), open(os.path.join(CSRC, "kernels.hip")).read()
    for line in ("constexpr uint32_t kNoKey = 0xFFFFFFFFu;", "constexpr uint32_t kValueNode = 0xFFFFFFFEu;"):
        assert line in hdr and line in batch, line


def test_documents_describe_the_longest_feed():
    hdr = open(os.path.join(ROOT, "include", "aha_hip.h")).read()
    assert "longest feed" in hdr and "no feed call has match_longest" not in hdr
    for doc in ("README.md", "INTEGRATION.md", "DESIGN.md"):
        assert "longest" in open(os.path.join(ROOT, doc)).read(), doc
    assert "Feed match_longest" in open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "longest" in open(os.path.join(ROOT, "include", "aha", "ac.hpp")).read()
    assert "longest" in open(os.path.join(ROOT, "bindings", "crystal", "aha_hip.cr")).read()
