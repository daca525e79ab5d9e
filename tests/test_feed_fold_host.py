"""CPU tests of folded feeds (AHA_FEED_FOLD: feeds on handles compiled with fold_simple, fold_bmp or fold_kana; DESIGN.md 4.13
"Feeds on handles folded beyond ASCII"): the CPU twin of the pipeline (tests/feedfoldsim.py) against the rule -- a call reports
the hits with n0 < end <= n1 of fold(S[:n1]) matched as one document -- for modes 2, 3 and 4, in bytes and in characters, with
cuts at every byte and random cuts, keys that are whole characters, keys cut inside a character and stray bytes, texts with
NULs; for keys of whole characters also against the whole sequence folded as one document; one recorded case in which the plain
feed's context of Lmax - 1 bytes is too short; the refusals, on a host-only handle; the constant in the header and the bindings
with the ABI untouched; and the stand-alone sanitizer program of the byte both kernels compute."""
import ctypes as C
import os
import random
import re
import subprocess

import numpy as np
import pytest

import pyoracle as orc
from aha_amd import AC, AhaError
from aha_amd import _native as N
from feedfoldsim import FOLD_KEYS, FOLD_OPTS, FOLDS, FeedFoldSim, rule_hits, same
from feedsim import absolute

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "aha_amd", "csrc")

# characters of every kind the folds move (and some they do not), in both cases
CHARS = list("aBcXyZ09 ") + list("ПриветЖжЯя") + list("ÉéÀàßÿ") + list("ＡａＺｚ") + list("ႠⴀႥ") + list("ỆệẠạ") + list("我是中") + \
    list("らラﾗーｰあアｱ")
STRAY = [b"\x80", b"\xbf", b"\xd0", b"\xc3", b"\xe1", b"\xe1\xbb", b"\xef", b"\xe3\x81", b"\xc1", b"\xf0\x9f", b"\x96"]


def other_case(k):
    """the key spelled in the other case where it is text (a key cut inside a character stays as it is)"""
    try:
        return k.decode().swapcase().encode()
    except UnicodeDecodeError:
        return k


def random_text(rng, n_items, nul=False, keys=()):
    out = bytearray()
    for _ in range(n_items):
        r = rng.random()
        if keys and r > 0.7:  # (so that hits, and hits across cuts, do occur)
            k = rng.choice(keys)
            out += other_case(k) if rng.random() < 0.6 else k
        elif r < 0.12:
            out += rng.choice(STRAY)
        elif nul and r < 0.18:
            out += b"\x00"
        else:
            out += rng.choice(CHARS).encode()
    return bytes(out)


def random_keys(rng, mode, kind):
    """kind 'whole': keys of whole characters; 'cut': slices of such strings at any byte; 'stray': with stray bytes as well.
    -> the keys as spelled, unique and non-empty after the fold"""
    fold, keys, seen = FOLDS[mode], [], set()
    for _ in range(rng.randint(1, 6)):
        k = "".join(rng.choice(CHARS) for _ in range(rng.randint(1, 3))).encode()
        if kind != "whole":
            a = rng.randint(0, len(k) - 1)
            k = k[a:rng.randint(a + 1, len(k))]
        if kind == "stray" and rng.random() < 0.5:
            k = (rng.choice(STRAY) if rng.random() < 0.5 else b"") + k + (rng.choice(STRAY) if rng.random() < 0.7 else b"")
        if k and fold(k) not in seen:
            seen.add(fold(k))
            keys.append(k)
    return keys


def cuts_of(rng, n, every):
    if every:
        return list(range(n + 1))
    inner = sorted(rng.randint(0, n) for _ in range(rng.randint(0, 5)))  # (equal cuts: empty pieces)
    return [0] + inner + [n]


def run_twin(o, mode, chars, S, cuts, W=None):
    """-> the pieces' (twin hits, rule hits, twin base, rule base)"""
    sim = FeedFoldSim(o, 1, mode, chars=chars, W=W)
    out = []
    for a, b in zip(cuts, cuts[1:]):
        got, base = sim.piece(0, S[a:b])
        want, _, wbase = rule_hits(o, mode, S, a, b, chars=chars)
        out.append((got, want, base, wbase))
    return out


@pytest.mark.parametrize("mode", [2, 3, 4])
@pytest.mark.parametrize("chars", [False, True])
def test_twin_is_the_rule(mode, chars):
    rng = random.Random(100 * mode + chars)
    n_cut_hits = 0
    for trial in range(150):
        kind = ("whole", "cut", "stray")[trial % 3]
        keys = random_keys(rng, mode, kind)
        if not keys:
            continue
        o = orc.AC.compile(FOLD_KEYS[mode](keys))
        S = random_text(rng, rng.randint(0, 14), nul=trial % 5 == 0, keys=keys)
        cuts = cuts_of(rng, len(S), every=trial % 3 == 0)
        whole = []
        for (got, want, base, wbase), a in zip(run_twin(o, mode, chars, S, cuts), cuts):
            assert same(got, want) and base == wbase, (mode, chars, keys, S, cuts, a, got, want)
            whole.append(absolute(got, base))
            n_cut_hits += int(np.count_nonzero(got["start"] < 0))
        if kind == "whole":  # bit-exact with the batch call on the whole sequence folded as one document, in order
            ref = o.match(FOLDS[mode](S), chars=chars) if S else np.zeros(0, dtype=orc.HIT_DTYPE)
            assert same(np.concatenate(whole + [ref[:0]]), ref), (mode, chars, keys, S, cuts)
    assert n_cut_hits > 100  # hits that began in an earlier piece did occur


def test_a_character_cut_between_calls_is_folded_whole_and_an_open_one_is_not():
    # "Ệ" = E1 BB 86, "ệ" = E1 BB 87: the key's last byte differs
    o = orc.AC.compile([b"\xe1\xbb\x87"])
    for cuts in ([0, 1, 2, 3], [0, 2, 3], [0, 1, 3], [0, 3]):
        sim = FeedFoldSim(o, 1, 3)
        hits = [sim.piece(0, "Ệ".encode()[a:b])[0] for a, b in zip(cuts, cuts[1:])]
        assert [len(h) for h in hits] == [0] * (len(cuts) - 2) + [1] and int(hits[-1]["end"][0]) == 3 - cuts[-2]
    # a key that ends in a truncated sequence is decided on the unfolded byte while the character is open: "あ" = E3 81 82 folds
    # to "ア" = E3 82 A2 under the kana fold, the key is E3 82.  Cut behind E3 81 the first call sees the open character
    # unfolded -- no hit -- and the second call reports ends in (2, 3] only: the feed never reports what the whole sequence
    # folded as one document has at end 2.  Uncut, the character is whole when its second byte is judged: the hit is there.
    o2 = orc.AC.compile([b"\xe3\x82"])
    S = "あ".encode()
    assert len(o2.match(FOLDS[4](S), chars=False)) == 1
    for cuts, n_hits in (([0, 2, 3], [0, 0]), ([0, 1, 2, 3], [0, 0, 0]), ([0, 3], [1]), ([0, 1, 3], [0, 1])):
        pieces = run_twin(o2, 4, False, S, cuts)
        assert [len(got) for got, _, _, _ in pieces] == n_hits
        assert all(same(got, want) for got, want, _, _ in pieces)


def test_a_context_of_lmax_minus_one_bytes_is_too_short():
    # "Ệa" = E1 BB 86 61 folds to E1 BB 87 61; the key is the last three of those bytes (Lmax = 3).  Cut in front of "a", a
    # context of Lmax - 1 = 2 bytes is BB 86: two continuation bytes without their lead, which no fold touches, so the window
    # holds BB 86 61 and the hit is lost.  With Lmax + 1 bytes the lead byte is in the context.
    keys, S, cuts = [b"\xbb\x87a"], "Ệa".encode(), [0, 3, 4]
    o = orc.AC.compile(keys)
    assert FOLDS[3](S) == b"\xe1\xbb\x87a" and o.max_key_len == 3
    short = run_twin(o, 3, False, S, cuts, W=o.max_key_len - 1)
    assert len(short[1][0]) == 0 and len(short[1][1]) == 1  # the twin with the plain feed's context misses the rule's hit
    for got, want, base, wbase in run_twin(o, 3, False, S, cuts):
        assert same(got, want)


# ---- the refusals, before any device work ------------------------------------------------------------------------------------
def _params(**kw):
    p = N.aha_match_params()
    p.struct_size = C.sizeof(N.aha_match_params)
    for k, v in kw.items():
        setattr(p, k, v)
    return p


@pytest.mark.parametrize("mode", [2, 3, 4])
def test_open_checks_on_a_host_only_handle(mode):
    L = N.lib()
    m = AC.compile(["Привет", "ｅｒｒｏｒ", "ラーメン"], host_only=True, **{FOLD_OPTS[mode]: True})
    h = C.c_void_p()
    # without the flag: refused as before, in the same words; the message names the flag
    assert L.aha_feed_open(m._h, 1, 0, C.byref(h)) == N.AHA_E_INVALID and not h.value
    msg = L.aha_last_error(m._h).decode()
    assert "AHA_OPT_FOLD_" in msg and "follow-up" in msg and "AHA_FEED_FOLD" in msg
    assert L.aha_feed_open(m._h, 1, N.AHA_FEED_CHARS, C.byref(h)) == N.AHA_E_INVALID
    with pytest.raises(AhaError) as e:
        m.feed(1)
    assert e.value.code == N.AHA_E_INVALID and "follow-up" in str(e.value)
    # with it: past the refusal, as far as a host-only handle gets
    for flags in (N.AHA_FEED_FOLD, N.AHA_FEED_FOLD | N.AHA_FEED_CHARS):
        assert L.aha_feed_open(m._h, 1, flags, C.byref(h)) == N.AHA_E_NO_DEVICE and not h.value
        assert L.aha_feed_open_params(m._h, 1, flags, None, C.byref(h)) == N.AHA_E_NO_DEVICE
    with pytest.raises(AhaError) as e:
        m.feed(1, fold=True)
    assert e.value.code == N.AHA_E_NO_DEVICE
    with pytest.raises(AhaError) as e:
        m.feed(1, chars=True, fold=True)
    assert e.value.code == N.AHA_E_NO_DEVICE
    # the flag with a separator filter or longest: follow-ups, refused before the device check
    for p in (_params(sep_size=16), _params(longest=1), _params(longest=2)):
        assert L.aha_feed_open_params(m._h, 1, N.AHA_FEED_FOLD, C.byref(p), C.byref(h)) == N.AHA_E_INVALID and not h.value
        assert "follow-up" in L.aha_last_error(m._h).decode()
    # flag value 2 is not taken, alone or beside the flag
    for flags in (2, 2 | N.AHA_FEED_FOLD, 8, 8 | N.AHA_FEED_FOLD):
        assert L.aha_feed_open(m._h, 1, flags, C.byref(h)) == N.AHA_E_INVALID


def test_the_flag_on_a_plain_handle_behaves_as_if_absent():
    L = N.lib()
    h = C.c_void_p()
    for kw in ({}, {"fold_ascii": True}):
        m = AC.compile(["he", "she"], host_only=True, **kw)
        for flags in (0, N.AHA_FEED_FOLD, N.AHA_FEED_FOLD | N.AHA_FEED_CHARS):
            assert L.aha_feed_open(m._h, 2, flags, C.byref(h)) == N.AHA_E_NO_DEVICE
            # a separator filter and longest stay what they are on such a handle: valid arguments, so the device check answers
            for p in (_params(sep_size=16), _params(longest=1)):
                want = N.AHA_E_INVALID if flags & N.AHA_FEED_CHARS else N.AHA_E_NO_DEVICE
                assert L.aha_feed_open_params(m._h, 2, flags, C.byref(p), C.byref(h)) == want
        assert L.aha_feed_open(m._h, 2, 2, C.byref(h)) == N.AHA_E_INVALID


def test_constant_in_header_and_bindings_abi_untouched():
    hdr = open(os.path.join(ROOT, "include", "aha_hip.h")).read()
    assert re.search(r"^#define AHA_FEED_FOLD 4u\b", hdr, re.M) and N.AHA_FEED_FOLD == 4
    assert "AHA_FEED_FOLD" in open(os.path.join(ROOT, "include", "aha", "ac.hpp")).read()
    assert re.search(r"^\s*FEED_FOLD\s*=\s*4_u32", open(os.path.join(ROOT, "bindings", "crystal", "aha_hip.cr")).read(), re.M)
    listed = open(os.path.join(CSRC, "exports.map")).read()
    assert len(re.findall(r"^\s+aha_\w+;", listed, re.M)) == 90
    assert N.lib().aha_abi_version() == 8 and re.search(r"#define AHA_ABI_VERSION 8\b", hdr)
    out = subprocess.run(["nm", "-D", "--defined-only", N.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert len([ln for ln in out.splitlines() if re.search(r" T aha_\w+$", ln)]) == 90
    import inspect

    assert "fold" in inspect.signature(AC.feed).parameters
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert "scan_feedfold.hip" in mk and mk.count("../../tests/cpp/feed_fold_stubs.cpp") == 2
    for doc in ("README.md", "INTEGRATION.md", "DESIGN.md"):
        assert "AHA_FEED_FOLD" in open(os.path.join(ROOT, doc)).read() or "fold=True" in open(os.path.join(ROOT, doc)).read(), doc


# ---- the byte both kernels compute, under the sanitizers, as its own process -------------------------------------------------
def test_spec_feed_fold_runs_clean_under_asan_and_ubsan(tmp_path):
    exe = str(tmp_path / "spec_feed_fold")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           os.path.join(ROOT, "tests", "cpp", "spec_feed_fold.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "spec_feed_fold: ok" in r.stdout
