"""CPU tests of feed counts (aha_feed_count_batch*): the entry points are declared, exported, listed and bound; their argument
checks come before any device work; and the identity the count pipeline rests on holds on the oracle, per
key, for every cut of every keyset of the GPU feed suite:
    bincount(hits of piece P) = bincount(X) - bincount(ctx) + bincount(P) - bincount(P')
with ctx the sequence's last min(W, consumed) bytes, P' = P[:W] and X = ctx || P'."""
import ctypes as C
import os
import random
import re
import zlib

import numpy as np
import pytest

import pyoracle as orc
from aha_amd import _native as N
from feedsim import FeedSim
from test_gpu_feed import KEYSETS, _next_len, _text

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("aha_feed_count_batch", "aha_feed_count_batch_device")


def test_feed_count_symbols_exported_declared_and_bound():
    hdr = open(os.path.join(ROOT, "include", "aha_hip.h")).read()
    listed = open(os.path.join(ROOT, "aha_amd", "csrc", "exports.map")).read()
    cr = open(os.path.join(ROOT, "bindings", "crystal", "aha_hip.cr")).read()
    L = C.CDLL(N.LIB_PATH)
    for name in ENTRIES:
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert re.search(r"^\s+%s;" % name, listed, re.M), name
        assert re.search(r"fun %s\b" % name, cr), name
        assert name in N.SIGNATURES and hasattr(L, name), name
    assert "def count_batch" in cr.split("class Feed", 1)[1].split("class ACGroup", 1)[0]
    assert N.lib().aha_abi_version() == 8  # a pure addition


def test_feed_count_argument_checks():
    """A NULL feed, a NULL n_hits and an unknown flag bit are AHA_E_INVALID from both entries, before anything else."""
    L = N.lib()
    n = C.c_uint64(0)
    offs = np.zeros(1, dtype=np.uint64)
    kc = np.zeros(4, dtype=np.uint64)
    for flags in (0, N.AHA_COUNT_ACCUMULATE, 2, 0x80000000):
        for nh in (C.byref(n), None):
            assert L.aha_feed_count_batch(None, None, offs.ctypes.data, None, 0, flags, kc.ctypes.data, None, None,
                                          nh) == N.AHA_E_INVALID
            assert L.aha_feed_count_batch_device(None, None, offs.ctypes.data, None, 0, 0, flags, None, None, None, nh,
                                                 None) == N.AHA_E_INVALID
    assert not kc.any() and n.value == 0


def _bc(hits, K):
    return np.bincount(hits["value"], minlength=K).astype(np.int64) if len(hits) else np.zeros(K, dtype=np.int64)


def _hits(o, b, chars):
    return o.match(bytes(b), chars=chars) if b else np.zeros(0, dtype=orc.HIT_DTYPE)


@pytest.mark.parametrize("chars", [False, True], ids=["bytes", "chars"])
@pytest.mark.parametrize("keyset", sorted(KEYSETS))
def test_counting_identity_on_the_oracle(keyset, chars):
    rng = random.Random(zlib.crc32(f"feedcount/{keyset}/{chars}".encode()))
    keys = KEYSETS[keyset](rng)
    o = orc.AC.compile(keys)
    K, W = len(keys), max(o.max_key_len - 1, 0)
    S = 4
    texts = [_text(rng, keys, n) for n in (0, 37, 3000, 20000)]
    if keyset == "ascii":  # stray continuation bytes, NULs and characters cut anywhere
        texts[1] = b"\x80\x00" + "中国".encode()[:4] + texts[1] + b"\xbf"
    sim = FeedSim(o, S, chars)
    pos = [0] * S
    sums = np.zeros((S, K), dtype=np.int64)
    while any(pos[s] < len(texts[s]) for s in range(S)):
        for s in range(S):
            n = _next_len(rng, texts[s], pos[s], W)
            P = texts[s][pos[s]:pos[s] + n]
            pos[s] += n
            ctx = sim.ctx[s]
            head = P[:W]
            terms = (_bc(_hits(o, ctx + head, chars), K) - _bc(_hits(o, ctx, chars), K) + _bc(_hits(o, P, chars), K)
                     - _bc(_hits(o, head, chars), K))
            hits, _ = sim.piece(s, P)
            want = _bc(hits, K)
            assert np.array_equal(terms, want), (keyset, s, pos[s])
            sums[s] += want
    for s in range(S):
        assert np.array_equal(sums[s], _bc(_hits(o, texts[s], chars), K)), (keyset, s)


def test_cpp_feed_count_example_compiles(tmp_path):
    from test_gpu_feed_count_cpp import build_spec_feed_count

    build_spec_feed_count(tmp_path)
