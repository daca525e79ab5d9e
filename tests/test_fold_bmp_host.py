"""CPU tests of case folding for three-byte UTF-8 characters (AHA_OPT_FOLD_BMP, include/aha_hip.h): the committed two-level table
against the rule stated in tests/fold3sim.py, the flag in the header and the bindings with the ABI untouched, host-only handles
(duplicates after folding, keys folded on their own, aha_ac_id, the caller's spelling, the handle of the folded keys), the
refusals of feeds and groups, the device pass's arithmetic as a lane-by-lane model against the plain per-document fold, and the
stand-alone sanitizer program of fold3_bytes and fold3_byte."""
import ctypes as C
import hashlib
import os
import random
import re
import struct
import subprocess
import sys
import unicodedata
import zlib

import numpy as np
import pytest

import fold3sim
import foldsim
from aha_amd import AC, AhaError
from aha_amd import _native as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "aha_amd", "csrc")
UNICODE_13 = unicodedata.unidata_version == "13.0.0"
needs_unicode_13 = pytest.mark.skipif(not UNICODE_13, reason="the tables are fixed at Unicode 13.0.0, this interpreter has %s" % unicodedata.unidata_version)


def committed_dense():
    """the dense table F3(cp) at cp - 0x800 from the two levels of the committed header"""
    text = open(os.path.join(CSRC, "fold3_table.hpp")).read()
    ibody = text[text.index("#define AHA_FOLD3_INDEX \\"):text.index("/* end of index */")]
    lbody = text[text.index("#define AHA_FOLD3_LIVE \\"):text.index("/* end of live */")]
    index = [int(x) for x in re.findall(r"(?<![\w+])(\d+),", ibody)]
    live = [int(x, 16) for x in re.findall(r"0x([0-9a-f]{4}),", lbody)]
    assert len(index) == 992 == int(re.search(r"#define AHA_FOLD3_INDEX_ENTRIES (\d+)", text).group(1))
    assert len(live) == 29 * 64 == int(re.search(r"#define AHA_FOLD3_LIVE_ENTRIES (\d+)", text).group(1))
    assert sorted(set(index)) == list(range(30))
    t = []
    for b, k in enumerate(index):
        t.extend(live[(k - 1) * 64:k * 64] if k else range(0x800 + b * 64, 0x800 + b * 64 + 64))
    return t


# ---- the table -------------------------------------------------------------------------------------------------------------
def test_committed_table_has_the_stated_crc_and_counts():
    t = committed_dense()
    assert len(t) == 63488
    assert zlib.crc32(struct.pack("<63488H", *t)) == 0x7BD41939
    moved = [i + 0x800 for i, x in enumerate(t) if x != i + 0x800]
    assert len(moved) == 679
    assert sum(1 for cp in moved if t[cp - 0x800] >> 12 != cp >> 12) == 124  # another lead byte
    assert sum(1 for cp in moved if t[cp - 0x800] >> 6 != cp >> 6) == 255    # another second byte (those included)
    assert len({cp >> 6 for cp in moved}) == 29
    assert {0xE0 | cp >> 12 for cp in moved} == {0xE1, 0xE2, 0xEA, 0xEF} == set(fold3sim.LIVE_LEADS)
    assert all(0x800 <= x <= 0xFFFF for x in t) and all(t[x - 0x800] == x for x in t)  # in the block, idempotent
    assert all(t[cp - 0x800] == cp for cp in range(0xD800, 0xE000)) and not any(0xD800 <= t[cp - 0x800] < 0xE000 for cp in moved)
    assert t[0x10A0 - 0x800] == 0x2D00 and t[0x13A0 - 0x800] == 0xAB70 and t[0xFF21 - 0x800] == 0xFF41


@needs_unicode_13
def test_committed_table_is_the_rule():
    assert committed_dense() == fold3sim.dense()
    assert [b for b in fold3sim.live_blocks()] == sorted({(i + 0x800) >> 6 for i, x in enumerate(committed_dense()) if x != i + 0x800})


@needs_unicode_13
def test_generators_agree_with_the_committed_headers():
    for tool in ("gen_fold3_table.py", "gen_fold_table.py"):
        r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", tool), "--check"], capture_output=True, text=True)
        assert r.returncode == 0, r.stdout + r.stderr


def test_two_byte_header_and_generator_are_untouched():
    text = open(os.path.join(CSRC, "fold_table.hpp")).read()
    t = [int(x, 16) for x in re.findall(r"0x([0-9a-f]{4}),", text[text.index("#define AHA_FOLD2_TABLE"):text.index("/* end */")])]
    assert len(t) == 1920 and zlib.crc32(struct.pack("<1920H", *t)) == 0x13BB525D
    assert hashlib.sha256(text.encode()).hexdigest() == "f133241565fa6983f3fdeeefcec0585dd23b4a9b8639ebcdf95cc8733e22f18a"
    assert hashlib.sha256(open(os.path.join(ROOT, "tools", "gen_fold_table.py"), "rb").read()).hexdigest() == "1992e8115328917ea7bada9b85d9c4c2c694a421afb5b0272954a32376a2a536"


@needs_unicode_13
def test_rule_properties_of_the_python_statement():
    F3, one3 = fold3sim.F3, fold3sim.one3
    outside = []
    for cp in range(0x800, 0x10000):
        if fold3sim.surrogate(cp):
            continue
        c = chr(cp)
        assert F3(F3(c)) == F3(c)
        partners = [v for v in (c.lower(), c.upper(), c.title()) if len(v) == 1 and v != c]
        for v in partners:
            if one3(v):
                assert F3(v) == F3(c), hex(cp)  # class-consistent: 0 exceptions
        if partners and not any(one3(v) for v in partners):
            outside.append(cp)
            assert F3(c) == c
    assert len(outside) == 33 and {0x212A, 0x2126, 0x212B, 0x1E9E, 0x2C62}.issubset(outside) and set(range(0x1C80, 0x1C88)).issubset(outside)
    assert F3("Ａ") == "ａ" and F3("Ệ") == "ệ" and F3("Ἀ") == "ἀ" and F3("Ⴀ") == "ⴀ" and F3("Ა") == "ა" and F3("Ⅻ") == "ⅻ" and F3("Ⓐ") == "ⓐ"
    assert F3("Ꭰ") == "ꭰ" == F3("ꭰ")  # (Cherokee lands on the lower-case letters)
    assert F3("你") == "你" and F3("\u212a") == "\u212a" and F3("\u1e9e") == "\u1e9e"
    assert fold3sim.fold3("ＥＲＲＯＲ Привет X".encode()) == "ｅｒｒｏｒ привет x".encode()
    assert fold3sim.fold3(b"\xe0\x80\x80\xed\xa0\x80\xe1\x82") == b"\xe0\x80\x80\xed\xa0\x80\xe1\x82"


# ---- the header and the bindings ---------------------------------------------------------------------------------------------
def test_flag_is_declared_and_bound_and_the_abi_did_not_move():
    hdr = open(os.path.join(ROOT, "include", "aha_hip.h")).read()
    assert re.search(r"#define\s+AHA_OPT_FOLD_BMP\s+16u\b", hdr)
    assert N.AHA_OPT_FOLD_BMP == 16
    assert "AHA_OPT_FOLD_BMP" in open(os.path.join(ROOT, "include", "aha", "ac.hpp")).read()
    assert re.search(r"OPT_FOLD_BMP\s*=\s*16_u32", open(os.path.join(ROOT, "bindings", "crystal", "aha_hip.cr")).read())
    for doc in ("README.md", "INTEGRATION.md", "DESIGN.md", os.path.join("tools", "README.md")):
        text = open(os.path.join(ROOT, doc)).read()
        assert "fold_bmp" in text or "AHA_OPT_FOLD_BMP" in text or "gen_fold3_table" in text, doc
    listed = open(os.path.join(CSRC, "exports.map")).read()
    assert len(re.findall(r"^\s+aha_\w+;", listed, re.M)) == 90
    assert N.lib().aha_abi_version() == 8 and re.search(r"#define AHA_ABI_VERSION 8\b", hdr)
    assert C.sizeof(N.aha_options) == 16 and C.sizeof(N.aha_ac_info_t) == 136
    out = subprocess.run(["nm", "-D", "--defined-only", N.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert len([ln for ln in out.splitlines() if re.search(r" T aha_\w+$", ln)]) == 90


# ---- host-only handles -------------------------------------------------------------------------------------------------------
def test_keys_equal_after_the_fold_are_duplicates():
    with pytest.raises(AhaError) as e:
        AC.compile(["ＡＢＣ", "ａｂｃ"], host_only=True, fold_bmp=True)
    assert e.value.code == N.AHA_E_DUP_KEY and e.value.key_index == 1
    assert AC.compile(["ＡＢＣ", "ａｂｃ"], host_only=True, fold_simple=True).n_keys == 2  # (the two-byte fold does not see them)
    assert AC.compile(["\u212a", "k"], host_only=True, fold_bmp=True).n_keys == 2       # the Kelvin sign stays
    assert AC.compile(["\u1e9e", "ß", "\u2126", "ω", "\u212b", "å"], host_only=True, fold_bmp=True).n_keys == 6
    with pytest.raises(AhaError) as e:
        AC.compile(["x", "Ệ", "y", "ệ"], host_only=True, fold_bmp=True)
    assert e.value.code == N.AHA_E_DUP_KEY and e.value.key_index == 3
    for pair in (["Привет", "ПРИВЕТ"], ["Foo", "fOO"], ["Ꭰ", "ꭰ"], ["Ⴀ", "ⴀ"]):  # it implies the two-byte and the ASCII fold
        with pytest.raises(AhaError) as e:
            AC.compile(pair, host_only=True, fold_bmp=True)
        assert e.value.code == N.AHA_E_DUP_KEY


def test_a_key_is_folded_on_its_own():
    # a lead byte that ends one key never joins the continuation bytes that open the next
    m = AC.compile([b"a\xef", b"\xbc\xa1b", "ａ".encode(), b"A\xef\xbc\xa1B", b"q\xef\xbc", b"\xa1r"], host_only=True, fold_bmp=True)
    assert m.n_keys == 6
    assert m[b"A\xef"] == 0 and m[b"\xbc\xa1B"] == 1 and m["Ａ".encode()] == 2 and m[b"a\xef\xbd\x81b"] == 3
    assert m[b"Q\xef\xbc"] == 4 and m[b"\xa1R"] == 5
    with pytest.raises(IndexError):
        m[b"\xbd\x81b"]  # (what key 1 would be had it been folded behind key 0's lead byte)


def test_ids_fold_their_argument_and_keys_keep_their_spelling():
    keys = ["ＥＲＲＯＲ", "Việt Nam", "ᾼδης", "ქართული", "école", "ПРИВЕТ", "Foo", "你好"]
    m = AC.compile(keys, host_only=True, fold_bmp=True)
    assert m.fold_bmp and m.fold_simple is False and m.fold_ascii is False
    assert N.lib().aha_ac_flags(m._h) == N.AHA_OPT_HOST_ONLY | N.AHA_OPT_FOLD_BMP
    assert m["ｅｒｒｏｒ"] == 0 and m["ＥｒｒＯｒ"] == 0 and m["VIỆT NAM"] == 1 and m["việt nam"] == 1 and m["ᾳΔΗΣ"] == 2
    assert m["ᲥᲐᲠᲗᲣᲚᲘ"] == 3 and m["ÉCOLE"] == 4 and m["привет"] == 5 and m["FOO"] == 6 and m["你好"] == 7
    assert [m[i] for i in range(len(keys))] == keys
    with pytest.raises(IndexError):
        m["error"]
    every = AC.compile(keys, host_only=True, fold_ascii=True, fold_simple=True, fold_bmp=True)  # 4u | 8u | 16u means what 16u means
    assert N.lib().aha_ac_flags(every._h) == N.AHA_OPT_HOST_ONLY | N.AHA_OPT_FOLD_ASCII | N.AHA_OPT_FOLD_SIMPLE | N.AHA_OPT_FOLD_BMP
    assert every.fold_bmp and every.fold_simple and every.fold_ascii and every["ｅｒｒｏｒ"] == 0
    simple = AC.compile(keys, host_only=True, fold_simple=True)
    assert simple.fold_bmp is False and simple["привет"] == 5
    with pytest.raises(IndexError):
        simple["ｅｒｒｏｒ"]
    # the container: the caller's spelling, nothing new; the flag is said again at load
    data = m.to_bytes()
    assert data == AC.compile(keys, host_only=True).to_bytes()
    again = AC.from_bytes(data, host_only=True, fold_bmp=True)
    assert again.fold_bmp and [again[i] for i in range(len(keys))] == keys and again["ｅｒｒｏｒ"] == 0
    with pytest.raises(AhaError) as e:
        AC.from_bytes(AC.compile(["ＡＢＣ", "ａｂｃ"], host_only=True).to_bytes(), host_only=True, fold_bmp=True)
    assert e.value.code == N.AHA_E_DUP_KEY


LETTERS = ("abcXYZ" + "абвгджзАБВГДЖЗ" + "ａｂｃｘｙｚＡＢＣＸＹＺ" + "ạảấầệỉọộụỳẠẢẤẦỆỈỌỘỤỲ" + "ἀἁἂᾳῃῳἈἉἊᾼῌῼ" + "აბგდევႠႡႢႣᲐᲑᲒᲓ" + "你好世界中文")


def test_handle_is_the_plain_handle_of_the_folded_keys():
    rng = random.Random(5)
    keys, seen = [], set()
    while len(keys) < 300:
        k = "".join(rng.choice(LETTERS) for _ in range(rng.randint(2, 9))).encode()
        if fold3sim.fold3(k) not in seen:
            seen.add(fold3sim.fold3(k))
            keys.append(k)
    assert sum(fold3sim.fold3(k) != foldsim.fold2(k) for k in keys) > 100
    f = AC.compile(keys, host_only=True, fold_bmp=True)
    p = AC.compile(fold3sim.fold3_keys(keys), host_only=True)
    assert f.info == p.info
    for which in (N.AHA_IMG_SLOTS, N.AHA_IMG_END_KEY, N.AHA_IMG_KEY_LN, N.AHA_IMG_STALE_ENDS, N.AHA_IMG_UNIT_SLOTS, N.AHA_IMG_UNIT_TABLES):
        assert f.export(which, np.uint8).tobytes() == p.export(which, np.uint8).tobytes(), which


# ---- the refusals ------------------------------------------------------------------------------------------------------------
def test_feeds_and_groups_are_refused_before_any_device_work():
    m = AC.compile(["ＡＢＣ"], host_only=True, fold_bmp=True)  # (host-only: a call that reached the device would say NO_DEVICE)
    h = C.c_void_p()
    assert N.lib().aha_feed_open(m._h, 1, 0, C.byref(h)) == N.AHA_E_INVALID and not h.value
    msg = N.lib().aha_last_error(m._h).decode()
    assert "AHA_OPT_FOLD_BMP" in msg and "follow-up" in msg
    p = N.aha_match_params()
    p.struct_size = C.sizeof(N.aha_match_params)
    assert N.lib().aha_feed_open_params(m._h, 1, 0, C.byref(p), C.byref(h)) == N.AHA_E_INVALID and not h.value
    assert N.lib().aha_feed_open_params(m._h, 1, N.AHA_FEED_CHARS, None, C.byref(h)) == N.AHA_E_INVALID
    with pytest.raises(AhaError) as e:
        m.feed(1)
    assert e.value.code == N.AHA_E_INVALID and "AHA_OPT_FOLD_BMP" in str(e.value)
    blob = np.frombuffer("ＡＢＣabc".encode(), dtype=np.uint8)
    offs = np.array([0, 9, 12], dtype=np.uint64)
    devs = np.array([0, 0], dtype=np.int32)
    ek = C.c_uint32(0)
    for flags in (N.AHA_OPT_FOLD_BMP, N.AHA_OPT_FOLD_BMP | N.AHA_OPT_HOST_ONLY, N.AHA_OPT_FOLD_BMP | N.AHA_OPT_FOLD_SIMPLE | N.AHA_OPT_FOLD_ASCII):
        g = C.c_void_p()
        rc = N.lib().aha_group_compile(blob.ctypes.data, offs.ctypes.data, 2, devs.ctypes.data, 2, flags, C.byref(g), C.byref(ek))
        assert rc == N.AHA_E_INVALID and not g.value
        assert "AHA_OPT_FOLD_BMP" in N.lib().aha_last_error(None).decode()


# ---- the device arithmetic ---------------------------------------------------------------------------------------------------
ALPHABET = [ord(c) for c in "abXY"] + [0xD0, 0xC3, 0xE0, 0xE1, 0xE2, 0xEA, 0xED, 0xEF, 0xE4, 0xA0, 0x80, 0xBC, 0xBA, 0xBF, 0xF0, 0xC1]


TOKENS = [c.encode() for c in "ＡỆႠꭰ你РÉ"]


def random_bytes(rng, n):
    """n bytes, half of them single bytes of the alphabet, half whole characters (the last one perhaps cut)"""
    out = bytearray()
    while len(out) < n:
        out += bytes([rng.choice(ALPHABET)]) if rng.random() < 0.5 else rng.choice(TOKENS)
    return bytes(out[:n])


def random_offsets(rng, n):
    """document offsets over n bytes, empty and one-byte documents included"""
    cuts = sorted(rng.randint(0, n) for _ in range(rng.randint(0, 6)))
    if cuts and rng.random() < 0.5:
        c = cuts[rng.randrange(len(cuts))]
        cuts.extend([c, min(n, c + 1)])  # an empty document and a one-byte one
        cuts.sort()
    return [0] + cuts + [n]


def test_kernel_model_is_the_per_document_fold():
    rng = random.Random(13)
    seen = {"neighbour_loads": 0, "cross_wave": 0, "cross_stride": 0, "not_live": 0, "fixed": 0, "moved": 0}
    for n in list(range(0, 41)) + list(range(1000, 1061)):
        for align in range(0, 16, 1 if n <= 40 else 5):
            # (the slice of a larger buffer whose bytes around it would join its ends: the model never indexes them)
            big = bytes([0xEF, 0xBC] * 8)[:align] + random_bytes(rng, n) + bytes([0xA1] * 16)
            buf = big[align:align + n]
            off = random_offsets(rng, n)
            want = fold3sim.fold3_docs(buf, off)
            for grid in ((1,) if n < 1000 else (1, 2)):
                for live_test in (True, False):
                    got, stats = fold3sim.kernel_model(buf, off, piece=16, wave=64, grid=grid, block=16 if grid == 2 else 256, live_test=live_test)
                    assert got == want, (n, align, off, grid, live_test)
                    for k in stats:
                        seen[k] += stats[k]
            seen["fixed"] += want != fold3sim.fold3(buf)
            seen["moved"] += want != foldsim.fold2_docs(buf, off)
    # the cases the model is there for did occur: triples across pieces and across a lane's stride, pieces the live-lead test
    # let through, boundaries where the blind pass had to be taken back, and text the two-byte fold leaves alone
    assert seen["neighbour_loads"] > 1000 and seen["cross_stride"] > 100 and seen["fixed"] > 50 and seen["moved"] > 100, seen
    # Chinese text with a full-width letter now and then, at every phase: pieces that leave by the live-lead test beside pieces
    # that may not -- the piece behind one that ends with a live lead byte among them
    for phase in range(16):
        buf = b"q" * phase + "".join("你好世界中文"[k % 6] + ("Ａ" if k % 29 == 0 else "") for k in range(300)).encode()
        off = [0, len(buf) // 3, len(buf)]
        got, stats = fold3sim.kernel_model(buf, off, live_test=True)
        assert got == fold3sim.fold3_docs(buf, off) != buf
        assert 0 < stats["not_live"] < len(buf) // 16
        assert fold3sim.kernel_model(buf, off)[0] == got
    # strides and a wave's edge: full-width text at each phase, grid 1 with 64-lane blocks and with 256
    for lead_in in (b"", b"x", b"xy"):
        buf = lead_in + "ＡＢＣＤＥ".encode() * 240
        for off in ([0, len(buf)], [0, 7, 7, 8, 1024, 1025, 1027, len(buf)]):
            want = fold3sim.fold3_docs(buf, off)
            got, stats = fold3sim.kernel_model(buf, off, grid=1, block=64)
            assert got == want and stats["cross_stride"] >= 2 and stats["neighbour_loads"] >= len(buf) // 16 - 1
            got, stats = fold3sim.kernel_model(buf, off, grid=1, block=256)
            assert got == want and stats["cross_wave"] >= 2
    # Chinese text: with the live-lead test no piece goes byte by byte, and the result is the text
    buf = "你好世界，中文。".replace("，", "、").encode() * 40
    got, stats = fold3sim.kernel_model(buf, [0, len(buf)], live_test=True)
    assert got == buf == fold3sim.fold3(buf) and stats["not_live"] == len(buf) // 16
    got, stats = fold3sim.kernel_model(buf, [0, len(buf)])
    assert got == buf and stats["not_live"] == 0
    # one- and zero-byte documents inside one triple: two boundaries, the same bytes put back
    buf = b"a" + "Ａ".encode() + b"b"
    for off in ([0, 2, 3, 5], [0, 2, 2, 3, 3, 5], [0, 1, 2, 3, 4, 5], [0, 3, 5], [0, 2, 5]):
        assert fold3sim.kernel_model(buf, off)[0] == fold3sim.fold3_docs(buf, off) == buf
    assert fold3sim.kernel_model(buf, [0, 1, 4, 5])[0] == b"a" + "ａ".encode() + b"b"


def test_fold3_byte_is_the_rule_at_every_position():
    rng = random.Random(17)
    for _ in range(400):
        buf = bytes(rng.choice(ALPHABET) for _ in range(rng.randint(0, 24)))
        n = len(buf)
        at = lambda j: buf[j] if 0 <= j < n else 0
        assert bytes(fold3sim.fold3_byte(at(j - 2), at(j - 1), buf[j], at(j + 1), at(j + 2)) for j in range(n)) == fold3sim.fold3(buf)


# ---- fold3_bytes and fold3_byte under the sanitizers, as their own process ---------------------------------------------------
def test_spec_fold3_runs_clean_under_asan_and_ubsan(tmp_path):
    exe = str(tmp_path / "spec_fold3")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           os.path.join(ROOT, "tests", "cpp", "spec_fold3.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "spec_fold3: ok" in r.stdout


def test_host_only_sanitizer_library_lists_the_new_stub():
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert mk.count("../../tests/cpp/fold3_stubs.cpp") == 2 and os.path.exists(os.path.join(ROOT, "tests", "cpp", "fold3_stubs.cpp"))
    assert mk.count("../../tests/cpp/fold2_stubs.cpp") == 2
