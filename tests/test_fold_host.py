"""CPU tests of ASCII case-insensitive handles (AHA_OPT_FOLD_ASCII, include/aha_hip.h): the flag and aha_ac_flags are
declared, exported, listed and bound; the word form of the fold (aha_amd/csrc/fold.hpp) is the bytewise rule; a folded
host-only handle is, image for image, the plain handle compiled from the folded keys, while it keeps the keys as spelled."""
import ctypes as C
import io
import os
import random
import re
import subprocess

import numpy as np
import pytest

import pyoracle as orc
from aha_amd import AC, ACGroup, AhaError
from aha_amd import _native as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXPORTS = [N.AHA_IMG_SLOTS, N.AHA_IMG_END_KEY, N.AHA_IMG_KEY_LN, N.AHA_IMG_KEY_CNT, N.AHA_IMG_KEY_KC, N.AHA_IMG_STALE_ENDS,
           N.AHA_IMG_UNIT_SLOTS, N.AHA_IMG_UNIT_ROOT, N.AHA_IMG_UNIT_END_KEY, N.AHA_IMG_UNIT_TABLES, N.AHA_IMG_UNIT_MARKS,
           N.AHA_IMG_UNIT_PAIRS, N.AHA_IMG_UNIT_PAIR_DISP]


def fold(a):
    a = np.frombuffer(a, dtype=np.uint8) if isinstance(a, (bytes, bytearray)) else np.asarray(a, dtype=np.uint8)
    return np.where((a >= 65) & (a <= 90), a + 32, a).astype(np.uint8)


def fold_b(b):
    return fold(b).tobytes()


def test_fold_flag_and_entry_declared_exported_listed_and_bound():
    hdr = open(os.path.join(ROOT, "include", "aha_hip.h")).read()
    listed = open(os.path.join(ROOT, "aha_amd", "csrc", "exports.map")).read()
    crystal = open(os.path.join(ROOT, "bindings", "crystal", "aha_hip.cr")).read()
    assert re.search(r"#define\s+AHA_OPT_FOLD_ASCII\s+4u\b", hdr)
    assert N.AHA_OPT_FOLD_ASCII == 4
    assert re.search(r"OPT_FOLD_ASCII\s*=\s*4_u32", crystal)
    assert re.search(r"\buint32_t\s+aha_ac_flags\s*\(\s*const aha_ac \*ac\s*\)", hdr)
    assert re.search(r"^\s+aha_ac_flags;", listed, re.M)
    assert "aha_ac_flags" in N.SIGNATURES and hasattr(C.CDLL(N.LIB_PATH), "aha_ac_flags")
    assert re.search(r"^\s*fun aha_ac_flags\(", crystal, re.M)
    assert "fold_ascii" in open(os.path.join(ROOT, "include", "aha", "ac.hpp")).read()
    assert N.lib().aha_abi_version() == 8 and re.search(r"#define AHA_ABI_VERSION 8\b", hdr)  # a pure addition
    assert C.sizeof(N.aha_ac_info_t) == 136
    assert N.lib().aha_ac_flags(None) == 0


def test_fold32_is_the_bytewise_rule(tmp_path):
    exe = str(tmp_path / "spec_fold32")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", os.path.join(ROOT, "tests", "cpp", "spec_fold32.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr


def test_cpp_fold_spec_compiles(tmp_path):
    from test_gpu_fold_cpp import build_spec_fold
    assert os.path.exists(build_spec_fold(tmp_path))


def _same_handle(folded, plain):
    ia, ib = folded.info, plain.info
    assert ia == ib, {k: (ia[k], ib[k]) for k in ia if ia[k] != ib[k]}
    for which in EXPORTS:
        a, b = folded.export(which, np.uint8), plain.export(which, np.uint8)
        assert a.tobytes() == b.tobytes(), which


def _mixed(rng, b):
    return bytes((c - 32) if 97 <= c <= 122 and rng.random() < 0.5 else c for c in b)


def test_folded_handle_is_the_plain_handle_of_the_folded_keys():
    rng = random.Random(7)
    words = set()
    while len(words) < 400:
        words.add("".join(rng.choice("abcdefghijklmnopqrstuvwxyz0123456789_") for _ in range(rng.randint(3, 14))).encode())
    ascii_keys = [_mixed(rng, w) for w in sorted(words)]
    cjk = ["我", "我是", "是中", "中国人", "Error", "ERR", "国aB", "人Z"] + ["字典词语%dX解释" % i for i in range(40)]
    cjk_keys = [k.encode() for k in cjk]
    for keys, kw, engine_field in ((ascii_keys, {}, "filter_prefix_bytes"), (cjk_keys, {}, "unit_enabled"),
                                   (ascii_keys, {"force_wide": True}, None)):
        f = AC.compile(keys, host_only=True, fold_ascii=True, **kw)
        p = AC.compile([fold_b(k) for k in keys], host_only=True, **kw)
        assert f.fold_ascii and not p.fold_ascii
        _same_handle(f, p)
        if engine_field:
            assert f.info[engine_field], engine_field
        if kw:
            assert f.info["slot_bytes"] == 8
        assert N.lib().aha_ac_flags(f._h) == N.AHA_OPT_HOST_ONLY | N.AHA_OPT_FOLD_ASCII | (N.AHA_OPT_FORCE_WIDE if kw else 0)
        assert N.lib().aha_ac_flags(p._h) == N.AHA_OPT_HOST_ONLY | (N.AHA_OPT_FORCE_WIDE if kw else 0)


def test_stale_ends_come_from_the_folded_keys():
    keys = ["Bbc", "bcc", "b", "X", "xy", "Xyz", "我A", "我a是"]
    f = AC.compile(keys, host_only=True, fold_ascii=True)
    p = AC.compile([k.lower() for k in keys], host_only=True)
    a, b = f.export(N.AHA_IMG_STALE_ENDS, np.uint32), p.export(N.AHA_IMG_STALE_ENDS, np.uint32)
    assert a.tobytes() == b.tobytes()
    o = orc.AC.compile([k.lower() for k in keys])
    assert a.size // 2 == o.stale_ends() > 0
    assert AC.compile(keys, host_only=True).export(N.AHA_IMG_STALE_ENDS, np.uint32).tobytes() != a.tobytes()  # only after folding


def test_keys_equal_after_folding_are_duplicates():
    with pytest.raises(AhaError) as e:
        AC.compile(["Foo", "bar", "fOO"], host_only=True, fold_ascii=True)
    assert e.value.code == N.AHA_E_DUP_KEY and e.value.key_index == 2
    assert AC.compile(["Foo", "bar", "fOO"], host_only=True).n_keys == 3
    with pytest.raises(AhaError) as e:
        ACGroup.compile(["Foo", "bar", "fOO"], [0, 0], host_only=True, fold_ascii=True)
    assert e.value.code == N.AHA_E_DUP_KEY and e.value.key_index == 2
    with pytest.raises(orc.OracleError):  # where the reference raises on the folded list
        orc.AC.compile(["foo", "bar", "foo"])


def test_keys_keep_their_spelling_and_ids_fold_their_argument():
    m = AC.compile(["Foo", "bAr", "baz@[`{", "我Q"], host_only=True, fold_ascii=True)
    assert [m[i] for i in range(4)] == ["Foo", "bAr", "baz@[`{", "我Q"]
    assert m["FOO"] == m["foo"] == m["Foo"] == 0
    assert m["BAR"] == 1 and m["BAZ@[`{"] == 2 and m["我q"] == 3
    for miss in ("fo", "fooo", "baz`{@[", "BAZ\x00[`{"):
        with pytest.raises(IndexError):
            m[miss]
    plain = AC.compile(["Foo", "bAr"], host_only=True)
    assert plain["Foo"] == 0
    with pytest.raises(IndexError):
        plain["foo"]


def test_boundary_bytes_and_high_bytes_are_not_folded():
    # '@' 0x40 / '`' 0x60, '[' 0x5B / '{' 0x7B differ by 0x20 like a letter's two cases; 0xC1 .. 0xDA are 'A' .. 'Z' + 0x80
    keys = [b"@@@", b"```", b"[[[", b"{{{", bytes(range(0xC1, 0xDB)), "Éé".encode(), "ÀB".encode()]
    m = AC.compile(keys, host_only=True, fold_ascii=True)
    assert m.n_keys == len(keys)  # no two of them are equal after folding
    for i, k in enumerate(keys):
        assert m[k] == i
    assert m["Àb".encode()] == 6
    for miss in (b"@@`", b"[[{", bytes(range(0xE1, 0xFB)), "éé".encode(), "àb".encode()):
        with pytest.raises(IndexError):
            m[miss]
    _same_handle(m, AC.compile([fold_b(k) for k in keys], host_only=True))


def test_save_and_load():
    keys = ["Error", "WARN", "info", "Déjà", "x@Y"]
    m = AC.compile(keys, host_only=True, fold_ascii=True)
    data = m.to_bytes()
    assert data == AC.compile(keys, host_only=True).to_bytes()  # the container: format 1, the keys as spelled, nothing new
    again = AC.from_bytes(data, host_only=True, fold_ascii=True)
    assert again.fold_ascii and [again[i] for i in range(len(keys))] == keys
    assert [again[k.upper()] for k in ("error", "warn", "info")] == [0, 1, 2]
    _same_handle(again, m)
    again2 = AC.load(io.BytesIO(data), host_only=True, fold_ascii=True)
    assert again2.fold_ascii and again2["ERROR"] == 0
    sensitive = AC.from_bytes(data, host_only=True)
    assert not sensitive.fold_ascii and sensitive["Error"] == 0
    with pytest.raises(IndexError):
        sensitive["error"]
    # two spellings of one word: a case-sensitive key set that no folded handle can load
    two = AC.compile(["Foo", "foo"], host_only=True).to_bytes()
    with pytest.raises(AhaError) as e:
        AC.from_bytes(two, host_only=True, fold_ascii=True)
    assert e.value.code == N.AHA_E_DUP_KEY


def test_host_only_group_accepts_the_flag():
    """aha_group_compile takes the flag in its `flags` (a host-only group compiles every shard with them: the duplicate check
    above is shard 0's); that every shard FOLDS is checked where shards can match: tests/test_gpu_fold.py."""
    g = ACGroup.compile(["Foo", "bar"], [0, 0, 0], host_only=True, fold_ascii=True)
    assert N.lib().aha_group_size(g._h) == 3
    plain = ACGroup.compile(["Foo", "bar", "fOO"], [0, 0, 0], host_only=True)  # (without the flag: no duplicate)
    assert N.lib().aha_group_size(plain._h) == 3


def test_replicate_keeps_the_flag_where_there_is_a_device():
    """aha_ac_replicate always uploads (there is no host-only replica): with a device the replica is checked here, without one
    the call has nothing to give and tests/test_gpu_fold.py::test_replicate_load_and_group is where the flag is followed."""
    m = AC.compile(["Foo", "bar"], host_only=True, fold_ascii=True)
    if N.lib().aha_device_count() > 0:
        r = m.replicate(0)
        assert r.fold_ascii and r[0] == "Foo" and r["FOO"] == 0
    else:
        with pytest.raises(AhaError) as e:
            m.replicate(0)
        assert e.value.code == N.AHA_E_NO_DEVICE
