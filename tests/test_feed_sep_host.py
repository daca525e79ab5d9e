"""CPU tests of feeds with a separator filter (aha_feed_open_params, aha_feed_finish_batch, aha_feed_finish_batch_device): the
model the GPU tests compare against (feedsepsim) gives, concatenated, the oracle's filtered hits of the whole sequence at every
cut; the entry points are exported, declared and bound; the argument checks come before the device check; the C++ example
compiles."""
import ctypes as C
import os
import random
import re

import numpy as np
import pytest

import pyoracle as orc
from aha_amd import AC, AhaError
from aha_amd import _native as N
from aha_amd import ac as acmod
from feedsepsim import SEPS, FeedSepSim, absolute, bitarray
from test_gpu_feed import KEYSETS, _text

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("aha_feed_open_params", "aha_feed_finish_batch", "aha_feed_finish_batch_device")
KEYSET_NAMES = ("nested", "single", "long", "ascii")  # (single: W = 0 without a filter)


def _stream(sim, pieces):
    got = []
    for p in pieces:
        h, base = sim.piece(0, p)
        assert ((h["end"] >= 0) & (h["end"] < max(len(p), 1))).all()
        got.append(absolute(h, base))
    h, n = sim.finish(0)
    assert (h["end"] == 0).all() and n == sum(len(p) for p in pieces)
    got.append(absolute(h, n))
    return np.concatenate(got)


@pytest.mark.parametrize("sep", sorted(SEPS))
@pytest.mark.parametrize("keyset", KEYSET_NAMES)
def test_model_is_the_oracle_at_every_cut(keyset, sep):
    rng = random.Random(f"feedsep/{keyset}/{sep}")
    keys = KEYSETS[keyset](rng)
    o = orc.AC.compile(keys)
    sim = FeedSepSim(o, 1, SEPS[sep])
    n = 230 if keyset == "long" else 60  # (long: keys of 100 bytes)
    for t in range(3):
        text = _text(rng, keys, n) if t else (b" " + keys[0] + b"\x00" + keys[-1] + b"\x80" + _text(rng, keys, n))[:n]
        want = o.match(text, sep=SEPS[sep])
        for cut in range(len(text) + 1):  # every two-piece cut (an empty piece at both ends)
            assert np.array_equal(_stream(sim, [text[:cut], text[cut:]]), want), (keyset, sep, cut)
        assert np.array_equal(_stream(sim, [text[i:i + 1] for i in range(len(text))]), want), (keyset, sep)  # byte by byte
    assert np.array_equal(_stream(sim, []), np.zeros(0, dtype=orc.HIT_DTYPE))  # an empty sequence


def test_model_reports_a_hit_one_byte_late():
    keys = [b"error", b"err"]
    sim = FeedSepSim(orc.AC.compile(keys), 2, SEPS["punct"])
    assert sim.piece(1, b"an error")[0].tolist() == []  # it ends with the piece: the byte behind it is not there yet
    assert sim.piece(1, b"")[0].tolist() == []  # a zero-length piece reports nothing
    assert sim.piece(1, b": terrors")[0].tolist() == [(-5, 0, 0)]  # carried over: end == 0, start == -len
    assert sim.piece(1, b" err")[0].tolist() == []
    h, n = sim.finish(1)
    assert h.tolist() == [(-3, 0, 1)] and n == 21  # the sequence's end passes on the right
    assert sim.piece(1, b"error ")[0].tolist() == [(0, 5, 0)]  # it started again: the sequence's start passes on the left
    sim.piece(0, b"x error")
    sim.reset(0)
    assert sim.piece(0, b" ")[0].tolist() == []  # reset drops the hit that ended with the last byte


def test_feed_sep_symbols_exported_declared_and_bound():
    hdr = open(os.path.join(ROOT, "include", "aha_hip.h")).read()
    listed = open(os.path.join(ROOT, "aha_amd", "csrc", "exports.map")).read()
    crystal = open(os.path.join(ROOT, "bindings", "crystal", "aha_hip.cr")).read()
    cxx = open(os.path.join(ROOT, "include", "aha", "ac.hpp")).read()
    L = C.CDLL(N.LIB_PATH)
    for name in ENTRIES:
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert re.search(r"^\s+%s;" % name, listed, re.M), name
        assert name in N.SIGNATURES and hasattr(L, name), name
        assert re.search(r"^\s*fun %s\(" % name, crystal, re.M), name
    assert "aha_feed_open_params(" in cxx and "aha_feed_finish_batch(" in cxx  # (the C++ mirror wraps the host entries)
    for method in ("finish_batch", "finish_batch_device", "finish"):
        assert callable(getattr(acmod.Feed, method))
    assert N.lib().aha_abi_version() == 8  # a pure addition


def _params(**kw):
    p = N.aha_match_params()
    p.struct_size = C.sizeof(N.aha_match_params)
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def _open(m, n_seqs, flags, p):
    h = C.c_void_p()
    rc = N.lib().aha_feed_open_params(m._h, n_seqs, flags, C.byref(p) if p is not None else None, C.byref(h))
    assert not h.value
    return rc


def test_feed_open_params_argument_checks_before_the_device_check():
    m = AC.compile(["he", "she", "hers"], host_only=True)
    assert _open(m, 4, 0, _params(sep_size=257)) == N.AHA_E_SEP_SIZE
    assert _open(m, 4, 0, _params(sep_size=16, char_offsets=1)) == N.AHA_E_INVALID
    assert _open(m, 4, 0, _params(sep_size=16, longest=1)) == N.AHA_E_INVALID
    assert _open(m, 4, N.AHA_FEED_CHARS, _params(sep_size=16)) == N.AHA_E_INVALID  # a char feed with a filter
    assert _open(m, 0, 0, _params(sep_size=16)) == N.AHA_E_INVALID and _open(m, 4, 2, _params(sep_size=16)) == N.AHA_E_INVALID
    # valid arguments: only now the handle without a device is noticed
    for flags, p in ((0, _params(sep_size=16)), (0, _params(sep_size=256)), (0, None), (N.AHA_FEED_CHARS, _params(sep_size=0))):
        assert _open(m, 4, flags, p) == N.AHA_E_NO_DEVICE
    with pytest.raises(AhaError) as e:
        m.feed(4, sep=bitarray(SEPS["punct"]))
    assert e.value.code == N.AHA_E_NO_DEVICE
    with pytest.raises(AhaError) as e:
        m.feed(4, chars=True, sep=bitarray(SEPS["punct"]))
    assert e.value.code == N.AHA_E_INVALID


def test_feed_finish_argument_checks_on_a_null_feed():
    ids = np.zeros(1, dtype=np.uint32)
    out = np.full(16 * 3, 0x5A5A5A5A, dtype=np.int32)
    n = C.c_uint64(7)
    L = N.lib()
    assert L.aha_feed_finish_batch(None, ids.ctypes.data, 1, out.ctypes.data, 16, None, None, C.byref(n)) == N.AHA_E_INVALID
    assert L.aha_feed_finish_batch_device(None, ids.ctypes.data, 1, out.ctypes.data, 16, None, None, C.byref(n), None) == N.AHA_E_INVALID
    assert (out == 0x5A5A5A5A).all()


def test_cpp_feed_sep_spec_compiles(tmp_path):
    from test_gpu_feed_sep_cpp import build_spec_feed_sep

    assert os.path.exists(build_spec_feed_sep(tmp_path))
