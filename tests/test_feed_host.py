"""CPU tests of feeds (aha_feed_*): the entry points are declared, exported, listed and bound; their argument checks come
before any device work, so they hold on a host-only handle; and the CPU twin of the feed pipeline (tests/feedsim.py: the two
facts of DESIGN.md 4.10) equals the oracle on whole sequences, whatever the cuts, in both offset modes."""
import ctypes as C
import os
import random
import re
import zlib

import numpy as np
import pytest

import pyoracle as orc
from aha_amd import AC, AhaError
from aha_amd import _native as N
from feedsim import FeedSim, absolute, leads

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("aha_feed_open", "aha_feed_free", "aha_feed_reset", "aha_feed_position", "aha_feed_match_batch",
           "aha_feed_match_batch_device")


def test_feed_symbols_exported_declared_and_bound():
    hdr = open(os.path.join(ROOT, "include", "aha_hip.h")).read()
    listed = open(os.path.join(ROOT, "aha_amd", "csrc", "exports.map")).read()
    cr = open(os.path.join(ROOT, "bindings", "crystal", "aha_hip.cr")).read()
    L = C.CDLL(N.LIB_PATH)
    for name in ENTRIES:
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert re.search(r"^\s+%s;" % name, listed, re.M), name
        assert re.search(r"fun %s\b" % name, cr), name
        assert name in N.SIGNATURES and hasattr(L, name), name
    assert "#define AHA_FEED_CHARS 1u" in hdr and N.AHA_FEED_CHARS == 1
    assert N.lib().aha_abi_version() == 8  # a pure addition


def test_feed_open_checks():
    L = N.lib()
    m = AC.compile(["he", "she", "hers"], host_only=True)
    f = C.c_void_p(1)
    assert L.aha_feed_open(m._h, 4, 0, C.byref(f)) == N.AHA_E_NO_DEVICE and not f.value
    assert L.aha_feed_open(m._h, 4, N.AHA_FEED_CHARS, C.byref(f)) == N.AHA_E_NO_DEVICE
    assert L.aha_feed_open(None, 4, 0, C.byref(f)) == N.AHA_E_INVALID
    assert L.aha_feed_open(m._h, 4, 0, None) == N.AHA_E_INVALID
    assert L.aha_feed_open(m._h, 0, 0, C.byref(f)) == N.AHA_E_INVALID
    assert L.aha_feed_open(m._h, 4, 2, C.byref(f)) == N.AHA_E_INVALID
    with pytest.raises(AhaError) as e:
        m.feed(4)
    assert e.value.code == N.AHA_E_NO_DEVICE


def test_feed_null_feed_is_invalid():
    L = N.lib()
    n = C.c_uint64(0)
    b = C.c_uint64(0)
    offs = np.zeros(1, dtype=np.uint64)
    assert L.aha_feed_reset(None, 0) == N.AHA_E_INVALID
    assert L.aha_feed_position(None, 0, C.byref(b), None) == N.AHA_E_INVALID
    assert L.aha_feed_match_batch(None, None, offs.ctypes.data, None, 0, None, 0, None, None, C.byref(n)) == N.AHA_E_INVALID
    assert L.aha_feed_match_batch_device(None, None, offs.ctypes.data, None, 0, 0, None, 0, None, None, C.byref(n),
                                         None) == N.AHA_E_INVALID
    L.aha_feed_free(None)  # (a no-op)


KEYSETS = {
    "ascii": [b"he", b"she", b"his", b"hers", b"abc", b"bcd", b"abcdefg", b"c d"],
    "utf8": ["我", "我是", "是中", "中国人", "国"],
    "nested": [b"a" * i for i in range(1, 12)] + [("我" * i).encode() for i in range(1, 6)] + [b"ba"],
    "single": [b"a", b"b", "是".encode(), b"\x80"],
    "long": [b"x" * 100, b"xx", b"xy", b"y", b"yx" * 3],
}


def _text(rng, keys, n):
    fill = [b" ", b"\x00", "中".encode(), b"\x80", b"\xe6", b"a", b"x", b"q"]
    out = bytearray()
    while len(out) < n:
        out += rng.choice(keys) if rng.random() < 0.5 else rng.choice(fill)
    return bytes(out[:n])


@pytest.mark.parametrize("keyset", sorted(KEYSETS))
@pytest.mark.parametrize("chars", [False, True])
def test_feedsim_equals_oracle_on_whole_sequences(keyset, chars):
    keys = [k.encode() if isinstance(k, str) else k for k in KEYSETS[keyset]]
    o = orc.AC.compile(keys)
    rng = random.Random(zlib.crc32(f"{keyset}/{chars}".encode()))
    for trial in range(12):
        text = _text(rng, keys, rng.choice([0, 1, 7, 60, 400, 1500]))
        sim = FeedSim(o, 1, chars)
        if trial == 0:  # a cut at every byte
            cuts = list(range(len(text) + 1))
        else:
            cuts = sorted({0, len(text)} | {rng.randint(0, len(text)) for _ in range(rng.randint(0, 12))})
        got = []
        for a, b in zip(cuts, cuts[1:]):
            hits, base = sim.piece(0, text[a:b])
            assert base == (leads(text[:a]) if chars else a)
            assert (hits["end"] >= 0).all() and (hits["start"] >= -sim.W).all()
            got.append(absolute(hits, base))
        got = np.concatenate(got) if got else np.zeros(0, dtype=orc.HIT_DTYPE)
        want = o.match(text, chars=chars) if text else np.zeros(0, dtype=orc.HIT_DTYPE)
        assert np.array_equal(got, want), (keyset, chars, trial)


def test_cpp_feed_example_compiles(tmp_path):
    from test_gpu_feed_cpp import build_spec_feed

    build_spec_feed(tmp_path)
