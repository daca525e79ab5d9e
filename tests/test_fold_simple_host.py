"""CPU tests of simple case folding for two-byte UTF-8 characters (AHA_OPT_FOLD_SIMPLE, include/aha_hip.h): the committed table
against the rule stated in tests/foldsim.py, the flag in the header and the bindings with the ABI untouched, host-only handles
(duplicates after folding, aha_ac_id, the caller's spelling), the refusals of feeds and groups, the device pass's arithmetic
as a lane-by-lane model against the plain per-document fold, and the stand-alone sanitizer program of fold2_bytes."""
import ctypes as C
import os
import random
import re
import struct
import subprocess
import unicodedata
import zlib

import numpy as np
import pytest

import foldsim
from aha_amd import AC, AhaError
from aha_amd import _native as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "aha_amd", "csrc")


def committed_table():
    text = open(os.path.join(CSRC, "fold_table.hpp")).read()
    body = text[text.index("#define AHA_FOLD2_TABLE"):text.index("/* end */")]
    return [int(x, 16) for x in re.findall(r"0x([0-9a-f]{4}),", body)]


# ---- the table -------------------------------------------------------------------------------------------------------------
def test_committed_table_has_the_stated_crc_and_shape():
    t = committed_table()
    assert len(t) == 1920
    assert zlib.crc32(struct.pack("<1920H", *t)) == 0x13BB525D
    assert sum(1 for i, x in enumerate(t) if x != i + 0x80) == 450
    assert sum(1 for i, x in enumerate(t) if (x >> 6) != ((i + 0x80) >> 6)) == 108
    assert all(0x80 <= x < 0x800 for x in t) and all(t[x - 0x80] == x for x in t)  # in the block, idempotent


def test_committed_table_is_the_rule_where_python_has_unicode_13():
    if unicodedata.unidata_version != "13.0.0":
        pytest.skip("this interpreter's Unicode is %s: the table is fixed at 13.0.0" % unicodedata.unidata_version)
    assert committed_table() == foldsim.table()


def test_generator_agrees_with_the_committed_header():
    if unicodedata.unidata_version != "13.0.0":
        pytest.skip("this interpreter's Unicode is %s: the table is fixed at 13.0.0" % unicodedata.unidata_version)
    r = subprocess.run(["python3", os.path.join(ROOT, "tools", "gen_fold_table.py"), "--check"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr


def test_rule_properties_of_the_python_statement():
    if unicodedata.unidata_version != "13.0.0":
        pytest.skip("properties checked for Unicode 13.0.0")
    F = foldsim.F
    for cp in range(0x80, 0x800):
        c = chr(cp)
        assert F(F(c)) == F(c)
        for v in (c.lower(), c.upper(), c.title()):
            if foldsim.one(v):
                assert F(v) == F(c), hex(cp)
        if foldsim.one(c.casefold()):  # (a single code point of the block: U+017F casefolds to ASCII 's' and stays)
            assert F(c) == c.casefold(), hex(cp)
    assert [F(c) for c in "ßİıſ"] == list("ßİıſ")
    assert F("µ") == "μ" and F("ς") == "σ" and F("ͅ") == "ι"
    assert [F(c) for c in "ϐϑϕϖϰϱϵ"] == list("βθφπκρε")
    assert foldsim.fold2("Р".encode()) == b"\xd1\x80" and foldsim.fold2("Π".encode()) == b"\xcf\x80"


# ---- the header and the bindings ---------------------------------------------------------------------------------------------
def test_flag_is_declared_and_bound_and_the_abi_did_not_move():
    hdr = open(os.path.join(ROOT, "include", "aha_hip.h")).read()
    assert re.search(r"#define\s+AHA_OPT_FOLD_SIMPLE\s+8u\b", hdr)
    assert N.AHA_OPT_FOLD_SIMPLE == 8
    assert "AHA_OPT_FOLD_SIMPLE" in open(os.path.join(ROOT, "include", "aha", "ac.hpp")).read()
    assert re.search(r"OPT_FOLD_SIMPLE\s*=\s*8_u32", open(os.path.join(ROOT, "bindings", "crystal", "aha_hip.cr")).read())
    listed = open(os.path.join(CSRC, "exports.map")).read()
    assert len(re.findall(r"^\s+aha_\w+;", listed, re.M)) == 90
    assert N.lib().aha_abi_version() == 8 and re.search(r"#define AHA_ABI_VERSION 8\b", hdr)
    assert C.sizeof(N.aha_options) == 16 and C.sizeof(N.aha_ac_info_t) == 136
    out = subprocess.run(["nm", "-D", "--defined-only", N.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert len([ln for ln in out.splitlines() if re.search(r" T aha_\w+$", ln)]) == 90


# ---- host-only handles -------------------------------------------------------------------------------------------------------
def test_keys_equal_after_the_simple_fold_are_duplicates():
    with pytest.raises(AhaError) as e:
        AC.compile(["Привет", "ПРИВЕТ"], host_only=True, fold_simple=True)
    assert e.value.code == N.AHA_E_DUP_KEY and e.value.key_index == 1
    assert AC.compile(["Привет", "ПРИВЕТ"], host_only=True, fold_ascii=True).n_keys == 2  # (the ASCII fold does not see them)
    assert AC.compile(["ß", "SS"], host_only=True, fold_simple=True).n_keys == 2
    with pytest.raises(AhaError) as e:
        AC.compile(["x", "σ", "y", "ς"], host_only=True, fold_simple=True)
    assert e.value.code == N.AHA_E_DUP_KEY and e.value.key_index == 3
    # a key is folded on its own: a lead byte that ends one key does not pair with the continuation byte that opens the next
    m = AC.compile([b"a\xd0", b"\xa0b", "р".encode(), b"A\xd0\xa0B"], host_only=True, fold_simple=True)
    assert m.n_keys == 4 and m[b"A\xd0"] == 0 and m[b"\xa0B"] == 1 and m["Р".encode()] == 2 and m[b"a\xd1\x80b"] == 3


def test_ids_fold_their_argument_and_keys_keep_their_spelling():
    keys = ["école", "ПРИВЕТ", "Σοφία", "Foo", "ǅ"]
    m = AC.compile(keys, host_only=True, fold_simple=True)
    assert m.fold_simple and m.fold_ascii is False
    assert N.lib().aha_ac_flags(m._h) == N.AHA_OPT_HOST_ONLY | N.AHA_OPT_FOLD_SIMPLE
    assert m["ÉCOLE"] == 0 and m["École"] == 0 and m["привет"] == 1 and m["ΣΟΦΊΑ"] == 2 and m["σοφία"] == 2 and m["FOO"] == 3
    assert m["Ǆ"] == 4 and m["ǆ"] == 4  # (a digraph's three cases are one class)
    assert [m[i] for i in range(len(keys))] == keys
    with pytest.raises(IndexError):
        m["ecole"]
    both = AC.compile(keys, host_only=True, fold_ascii=True, fold_simple=True)  # 4u | 8u means what 8u means
    assert N.lib().aha_ac_flags(both._h) == N.AHA_OPT_HOST_ONLY | N.AHA_OPT_FOLD_ASCII | N.AHA_OPT_FOLD_SIMPLE  # (as passed)
    assert both["ÉCOLE"] == 0
    ascii_only = AC.compile(keys, host_only=True, fold_ascii=True)
    with pytest.raises(IndexError):
        ascii_only["ÉCOLE"]
    # the container: the caller's spelling, nothing new; the flag is said again at load
    data = m.to_bytes()
    assert data == AC.compile(keys, host_only=True).to_bytes()
    again = AC.from_bytes(data, host_only=True, fold_simple=True)
    assert again.fold_simple and [again[i] for i in range(len(keys))] == keys and again["ПРИВЕТ".lower()] == 1
    with pytest.raises(AhaError) as e:
        AC.from_bytes(AC.compile(["Привет", "ПРИВЕТ"], host_only=True).to_bytes(), host_only=True, fold_simple=True)
    assert e.value.code == N.AHA_E_DUP_KEY


def test_handle_is_the_plain_handle_of_the_folded_keys():
    rng = random.Random(3)
    letters = "abcXYZ" + "абвгдежзийклмнопрстуфхцчшщъыьэюяАБВГДЕЖЗИЙКЛМНОПРСТУФХЦЧШЩЪЫЬЭЮЯ" + "αβγδεζηθλμπρσςΑΒΓΔΠΣ" + "éèêàçÉÈÊÀÇßµ"
    keys, seen = [], set()
    while len(keys) < 300:
        k = "".join(rng.choice(letters) for _ in range(rng.randint(2, 9))).encode()
        if foldsim.fold2(k) not in seen:
            seen.add(foldsim.fold2(k))
            keys.append(k)
    f = AC.compile(keys, host_only=True, fold_simple=True)
    p = AC.compile(foldsim.fold2_keys(keys), host_only=True)
    assert f.info == p.info
    for which in (N.AHA_IMG_SLOTS, N.AHA_IMG_END_KEY, N.AHA_IMG_KEY_LN, N.AHA_IMG_STALE_ENDS, N.AHA_IMG_UNIT_SLOTS, N.AHA_IMG_UNIT_TABLES):
        assert f.export(which, np.uint8).tobytes() == p.export(which, np.uint8).tobytes(), which


# ---- the refusals ------------------------------------------------------------------------------------------------------------
def test_feeds_and_groups_are_refused_before_any_device_work():
    m = AC.compile(["Привет"], host_only=True, fold_simple=True)  # (host-only: a call that reached the device would say NO_DEVICE)
    h = C.c_void_p()
    assert N.lib().aha_feed_open(m._h, 1, 0, C.byref(h)) == N.AHA_E_INVALID and not h.value
    msg = N.lib().aha_last_error(m._h).decode()
    assert "AHA_OPT_FOLD_SIMPLE" in msg and "follow-up" in msg
    p = N.aha_match_params()
    p.struct_size = C.sizeof(N.aha_match_params)
    assert N.lib().aha_feed_open_params(m._h, 1, 0, C.byref(p), C.byref(h)) == N.AHA_E_INVALID and not h.value
    assert N.lib().aha_feed_open_params(m._h, 1, N.AHA_FEED_CHARS, None, C.byref(h)) == N.AHA_E_INVALID
    with pytest.raises(AhaError) as e:
        m.feed(1)
    assert e.value.code == N.AHA_E_INVALID and "follow-up" in str(e.value)
    plain = AC.compile(["Привет"], host_only=True, fold_ascii=True)
    assert N.lib().aha_feed_open(plain._h, 1, 0, C.byref(h)) == N.AHA_E_NO_DEVICE  # (an ASCII-folded handle gets as far as before)
    blob = np.frombuffer("Приветмир".encode(), dtype=np.uint8)
    offs = np.array([0, 12, 18], dtype=np.uint64)
    devs = np.array([0, 0], dtype=np.int32)
    ek = C.c_uint32(0)
    for flags in (N.AHA_OPT_FOLD_SIMPLE, N.AHA_OPT_FOLD_SIMPLE | N.AHA_OPT_HOST_ONLY, N.AHA_OPT_FOLD_SIMPLE | N.AHA_OPT_FOLD_ASCII):
        g = C.c_void_p()
        rc = N.lib().aha_group_compile(blob.ctypes.data, offs.ctypes.data, 2, devs.ctypes.data, 2, flags, C.byref(g), C.byref(ek))
        assert rc == N.AHA_E_INVALID and not g.value
    assert "follow-up" in N.lib().aha_last_error(None).decode()


# ---- the device arithmetic ---------------------------------------------------------------------------------------------------
ALPHABET = [ord(c) for c in "abXY"] + [0xD0, 0xD1, 0xCE, 0xC3, 0xA0, 0x80, 0xBF, 0xE4, 0xC1]


def random_offsets(rng, n):
    """document offsets over n bytes, empty documents included"""
    cuts = sorted(rng.randint(0, n) for _ in range(rng.randint(0, 6)))
    if cuts and rng.random() < 0.5:
        cuts.insert(rng.randrange(len(cuts)), cuts[rng.randrange(len(cuts))])  # an empty document
        cuts.sort()
    return [0] + cuts + [n]


def test_kernel_model_is_the_per_document_fold():
    rng = random.Random(11)
    seen = {"neighbour_loads": 0, "cross_wave": 0, "cross_stride": 0, "fixed": 0}
    for n in list(range(0, 71)) + list(range(1000, 1101)):
        for align in range(16):
            # (the slice of a larger buffer whose bytes around it would pair with its ends: the model never indexes them)
            big = bytes([0xD0] * align) + bytes(rng.choice(ALPHABET) for _ in range(n)) + bytes([0xA0] * 16)
            buf = big[align:align + n]
            off = random_offsets(rng, n)
            want = foldsim.fold2_docs(buf, off)
            for grid in ((1,) if n < 1000 else (1, 2)):
                got, stats = foldsim.kernel_model(buf, off, piece=16, wave=64, grid=grid, block=16 if grid == 2 else 256)
                assert got == want, (n, align, off, grid)
                for k in stats:
                    seen[k] += stats[k]
            seen["fixed"] += want != foldsim.fold2(buf)
    # the cases the model is there for did occur: pairs across pieces, across a wave's edge, across a lane's stride, and
    # boundaries where the blind pass had to be taken back
    assert seen["neighbour_loads"] > 1000 and seen["cross_stride"] > 100 and seen["fixed"] > 100, seen
    # a wave's edge needs more than 64 pieces: Cyrillic text at an odd phase, every piece's last byte a lead byte
    buf = b"x" + "РСТУ".encode() * 300
    got, stats = foldsim.kernel_model(buf, [0, len(buf)], grid=1)
    assert got == foldsim.fold2(buf) and stats["cross_wave"] >= 2 and stats["neighbour_loads"] >= 2 * (len(buf) // 16 - 1)
    got, stats = foldsim.kernel_model(buf, [0, 7, 7, len(buf)], grid=1, block=64)
    assert got == foldsim.fold2_docs(buf, [0, 7, 7, len(buf)]) and stats["cross_stride"] >= 2


# ---- fold2_bytes under the sanitizers, as its own process --------------------------------------------------------------------
def test_spec_fold2_runs_clean_under_asan_and_ubsan(tmp_path):
    exe = str(tmp_path / "spec_fold2")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           os.path.join(ROOT, "tests", "cpp", "spec_fold2.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "spec_fold2: ok" in r.stdout


def test_host_only_sanitizer_library_lists_the_new_stub():
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert mk.count("../../tests/cpp/fold2_stubs.cpp") == 2 and os.path.exists(os.path.join(ROOT, "tests", "cpp", "fold2_stubs.cpp"))
