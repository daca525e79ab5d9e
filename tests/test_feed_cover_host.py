"""CPU tests of feed cover (aha_feed_cover_batch*): the entry points are declared, exported, listed and bound; their argument
checks come before any device work; and, on the oracle, for every keyset of the GPU feed suite: the stream law (the redacted
pieces with their back-fills are the redaction of the whole sequence) and the identity the device pipeline rests on
(tests/feedcoversim.py: clear + the widened windows = the contract's mask, back and hit count)."""
import ctypes as C
import os
import random
import re
import zlib

import numpy as np
import pytest

import pyoracle as orc
from aha_amd import _native as N
from coversim import redacted as redact_np
from feedcoversim import FeedCoverSim, piece_truth, reassemble, spans_cover
from test_gpu_feed import KEYSETS, _next_len, _text

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("aha_feed_cover_batch", "aha_feed_cover_batch_device")
FILL = 0x2A


def test_feed_cover_symbols_exported_declared_and_bound():
    hdr = open(os.path.join(ROOT, "include", "aha_hip.h")).read()
    listed = open(os.path.join(ROOT, "aha_amd", "csrc", "exports.map")).read()
    cr = open(os.path.join(ROOT, "bindings", "crystal", "aha_hip.cr")).read()
    hpp = open(os.path.join(ROOT, "include", "aha", "ac.hpp")).read()
    L = C.CDLL(N.LIB_PATH)
    for name in ENTRIES:
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert re.search(r"^\s+%s;" % name, listed, re.M), name
        assert re.search(r"fun %s\b" % name, cr), name
        assert name in N.SIGNATURES and hasattr(L, name), name
    feed_cr = cr.split("class Feed", 1)[1].split("class ACGroup", 1)[0]
    assert "def cover_batch" in feed_cr and "def redact_batch" in feed_cr
    assert "aha_feed_cover_batch(" in hpp
    assert N.lib().aha_abi_version() == 8  # a pure addition


def test_feed_cover_argument_checks():
    """A NULL feed, a NULL n_covered and a flag bit are AHA_E_INVALID from both entries, before anything else."""
    L = N.lib()
    nc, nh = C.c_uint64(0), C.c_uint64(0)
    offs = np.zeros(1, dtype=np.uint64)
    for flags in (0, 1, 0x80000000):
        for pnc in (C.byref(nc), None):
            assert L.aha_feed_cover_batch(None, None, offs.ctypes.data, None, 0, flags, None, None, FILL, None, None, None, None,
                                          pnc, C.byref(nh)) == N.AHA_E_INVALID
            assert L.aha_feed_cover_batch_device(None, None, offs.ctypes.data, None, 0, 0, flags, None, None, FILL, None, None,
                                                 None, None, pnc, C.byref(nh), None) == N.AHA_E_INVALID
    assert nc.value == 0 and nh.value == 0


def _whole(o, t):
    return o.match(bytes(t)) if t else np.zeros(0, dtype=orc.HIT_DTYPE)


def _case(keyset, tag):
    rng = random.Random(zlib.crc32(f"feedcover/{tag}/{keyset}".encode()))
    keys = KEYSETS[keyset](rng)
    o = orc.AC.compile(keys)
    return rng, keys, o, max(o.max_key_len - 1, 0)


def _check_cuts(o, W, text, cuts):
    """the sequence cut at `cuts`: the contract's pieces obey the stream law and the bounds on back, and the pipeline gives
    the contract's mask, back and hit count"""
    whole = _whole(o, text)
    raw = np.frombuffer(text, dtype=np.uint8)
    want = redact_np(raw, spans_cover(whole["start"], whole["end"], len(text)), FILL).tobytes()
    sim = FeedCoverSim(o, 1)
    bounds = [0] + list(cuts) + [len(text)]
    reds, backs, n_hits = [], [], 0
    for a, b in zip(bounds[:-1], bounds[1:]):
        cov, back, n = piece_truth(whole, a, b - a)
        assert 0 <= back <= min(W, a), (a, b)
        s_cov, s_back, s_n, s_base = sim.piece(0, text[a:b])
        assert np.array_equal(s_cov, cov) and s_back == back and s_n == n and s_base == a, (a, b)
        reds.append(redact_np(raw[a:b], cov, FILL))
        backs.append(back)
        n_hits += n
    assert reassemble(reds, backs, FILL) == want, cuts
    assert n_hits == len(whole)


@pytest.mark.parametrize("keyset", sorted(KEYSETS))
def test_stream_law_and_pipeline_at_every_cut(keyset):
    rng, keys, o, W = _case(keyset, "cuts")
    n = 260 if keyset == "long" else 90
    text = _text(rng, keys, n)
    for c in range(n + 1):
        _check_cuts(o, W, text, [c])
        for gap in sorted({1, 2, max(W // 2, 1), max(W - 1, 1)}):  # two cuts less than a key length apart
            if c + gap <= n:
                _check_cuts(o, W, text, [c, c + gap])
    for _ in range(20):  # pieces shorter than a key throughout: one hit spans three pieces and more
        cuts = sorted(rng.sample(range(n + 1), min(n, 40)))
        _check_cuts(o, W, text, cuts)


@pytest.mark.parametrize("keyset", sorted(KEYSETS))
def test_pipeline_identity_on_the_oracle(keyset):
    """several sequences fed piece by piece: the lengths 0, 1, W-1, W, W+1, 2W-1, 2W, 2W+1, then random ones; texts with NUL
    bytes, stray continuation bytes and characters cut anywhere; W = 0 with the one-byte keys"""
    rng, keys, o, W = _case(keyset, "pipeline")
    S = 3
    texts = [_text(rng, keys, n) for n in (37, 3000, 12000)]
    texts[0] = b"\x80\x00" + "中国".encode()[:4] + texts[0] + b"\xbf"
    whole = [_whole(o, t) for t in texts]
    sim = FeedCoverSim(o, S)
    pos = [0] * S
    fixed = [max(v, 0) for v in (0, 1, W - 1, W, W + 1, 2 * W - 1, 2 * W, 2 * W + 1)]
    step = 0
    while any(pos[s] < len(texts[s]) for s in range(S)):
        for s in range(S):
            n = fixed[step] if step < len(fixed) else _next_len(rng, texts[s], pos[s], W)
            n = min(n, len(texts[s]) - pos[s])
            cov, back, nh = piece_truth(whole[s], pos[s], n)
            s_cov, s_back, s_n, s_base = sim.piece(s, texts[s][pos[s]:pos[s] + n])
            assert np.array_equal(s_cov, cov) and s_back == back and s_n == nh and s_base == pos[s], (keyset, s, pos[s], n)
            assert 0 <= back <= min(W, pos[s])
            pos[s] += n
        step += 1
    if keyset == "single":
        assert W == 0


def test_cpp_feed_cover_example_compiles(tmp_path):
    from test_gpu_feed_cover_cpp import build_spec_feed_cover

    build_spec_feed_cover(tmp_path)
