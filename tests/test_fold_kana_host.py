"""CPU tests of the kana fold (AHA_OPT_FOLD_KANA, include/aha_hip.h): the committed two-level table against the rule stated in
tests/foldksim.py, the flag in the header and the bindings with the ABI untouched, host-only handles (duplicates after folding,
aha_ac_id, the caller's spelling, load and replicate, the handle of the folded keys), the refusals of feeds and groups, the
device pass's arithmetic in both halo forms as a lane-by-lane model against the plain per-document fold, and the stand-alone
sanitizer program of foldk_bytes and foldk_byte."""
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
import foldksim
from aha_amd import AC, AhaError
from aha_amd import _native as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "aha_amd", "csrc")
UNICODE_13 = unicodedata.unidata_version == "13.0.0"
needs_unicode_13 = pytest.mark.skipif(not UNICODE_13, reason="the tables are fixed at Unicode 13.0.0, this interpreter has %s" % unicodedata.unidata_version)
CRC = 0x3E50B4E4


def committed_dense():
    """the dense table FK(cp) at cp - 0x800 from the two levels of the committed header"""
    text = open(os.path.join(CSRC, "foldk_table.hpp")).read()
    ibody = text[text.index("#define AHA_FOLDK_INDEX \\"):text.index("/* end of index */")]
    lbody = text[text.index("#define AHA_FOLDK_LIVE \\"):text.index("/* end of live */")]
    index = [int(x) for x in re.findall(r"(?<![\w+])(\d+),", ibody)]
    live = [int(x, 16) for x in re.findall(r"0x([0-9a-f]{4}),", lbody)]
    assert len(index) == 992 == int(re.search(r"#define AHA_FOLDK_INDEX_ENTRIES (\d+)", text).group(1))
    assert len(live) == 33 * 64 == int(re.search(r"#define AHA_FOLDK_LIVE_ENTRIES (\d+)", text).group(1))
    assert sorted(set(index)) == list(range(34))
    t = []
    for b, k in enumerate(index):
        t.extend(live[(k - 1) * 64:k * 64] if k else range(0x800 + b * 64, 0x800 + b * 64 + 64))
    return t


# ---- the table -------------------------------------------------------------------------------------------------------------
def test_committed_table_has_the_stated_crc_and_counts():
    t = committed_dense()
    assert len(t) == 63488
    assert zlib.crc32(struct.pack("<63488H", *t)) == CRC
    assert ("0x%08x" % CRC) in open(os.path.join(ROOT, "DESIGN.md")).read().lower()
    moved = [i + 0x800 for i, x in enumerate(t) if x != i + 0x800]
    assert len(moved) == 679 + 144
    assert all(0x800 <= x <= 0xFFFF for x in t) and all(t[x - 0x800] == x for x in t)  # in the block, idempotent
    # K: what it moves and nothing else
    f3 = fold3sim.dense() if UNICODE_13 else None
    domain = set(range(0x3041, 0x3097)) | {0x309D, 0x309E} | set(range(0xFF66, 0xFF9E))
    assert len(domain) == 144 and domain <= set(moved)
    for cp in domain:
        v = t[cp - 0x800]
        assert v not in domain and 0x30A1 <= v <= 0x30FE and t[v - 0x800] == v
        if f3:
            assert f3[cp - 0x800] == cp and f3[v - 0x800] == v  # K and F3 never meet
    for cp in range(0x3041, 0x3097):
        assert t[cp - 0x800] == cp + 0x60
    assert t[0x309D - 0x800] == 0x30FD and t[0x309E - 0x800] == 0x30FE and t[0xFF71 - 0x800] == 0x30A2 and t[0xFF70 - 0x800] == 0x30FC
    for cp in (0x3040, 0x3097, 0x3099, 0x309A, 0x309F, 0x30F7, 0x30FA, 0x30FF, 0xFF65, 0xFF9E, 0xFF9F, 0x4F60):
        assert t[cp - 0x800] == cp, hex(cp)
    if f3:
        assert all(t[i] == f3[i] for i in range(len(t)) if i + 0x800 not in domain)  # everything else is F3
    assert {cp >> 6 for cp in domain} == {0x3040 >> 6, 0x3080 >> 6, 0xFF40 >> 6, 0xFF80 >> 6}
    assert len({cp >> 6 for cp in moved}) == 33


@needs_unicode_13
def test_committed_table_is_the_rule():
    assert committed_dense() == foldksim.dense()
    K = foldksim.K()
    assert len(K) == 144
    for cp, v in K.items():
        c, i = chr(cp), chr(v)
        assert unicodedata.name(i).startswith("KATAKANA") and len(i.encode()) == 3
        assert v not in K                                                         # no image is in K's domain
        assert c.lower() == c.upper() == c and i.lower() == i.upper() == i        # no source or image has a case mapping
        assert fold3sim.F3(c) == c and fold3sim.F3(i) == i
        if cp >= 0xFF00:
            assert unicodedata.normalize("NFKC", c) == i and c.encode()[0] == 0xEF and i.encode()[0] == 0xE3
        else:
            assert c.encode()[0] == i.encode()[0] == 0xE3 and c.encode()[1:] != i.encode()[1:]
    for cp in range(0x800, 0x10000):
        if not fold3sim.surrogate(cp):
            c = chr(cp)
            assert foldksim.FK(foldksim.FK(c)) == foldksim.FK(c)
    assert foldksim.foldk("こんぴゅーた ｺﾝﾋﾟｭｰﾀ ＡБ X".encode()) == "コンピュータ コンヒﾟュータ ａб x".encode()
    assert foldksim.foldk("ｶﾞ".encode()) == "カﾞ".encode() != "ガ".encode()  # no voiced half-width sequences
    assert foldksim.foldk("ぁあ".encode()) == "ァア".encode()                  # small and large kana stay apart


@needs_unicode_13
def test_generator_agrees_and_the_other_tables_are_untouched():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gen_foldk_table.py"), "--check"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert ("0x%08x" % CRC) in r.stdout
    gen = open(os.path.join(ROOT, "tools", "gen_foldk_table.py")).read()
    assert re.search(r"^CRC = 0x%08X\b" % CRC, gen, re.M) and "refusing to write" in gen
    for tool in ("gen_fold3_table.py", "gen_fold_table.py"):
        r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", tool), "--check"], capture_output=True, text=True)
        assert r.returncode == 0, r.stdout + r.stderr


def test_existing_tables_and_generators_are_byte_for_byte_what_they_were():
    want = {os.path.join(CSRC, "fold_table.hpp"): "f133241565fa6983f3fdeeefcec0585dd23b4a9b8639ebcdf95cc8733e22f18a",
            os.path.join(ROOT, "tools", "gen_fold_table.py"): "1992e8115328917ea7bada9b85d9c4c2c694a421afb5b0272954a32376a2a536"}
    for path, digest in want.items():
        assert hashlib.sha256(open(path, "rb").read()).hexdigest() == digest, path
    t3 = open(os.path.join(CSRC, "fold3_table.hpp")).read()
    assert "0x7bd41939" in t3 and "#define AHA_FOLD3_LIVE_ENTRIES 1856" in t3


# ---- the header and the bindings ---------------------------------------------------------------------------------------------
def test_flag_is_declared_and_bound_and_the_abi_did_not_move():
    hdr = open(os.path.join(ROOT, "include", "aha_hip.h")).read()
    assert re.search(r"#define\s+AHA_OPT_FOLD_KANA\s+32u\b", hdr)
    assert N.AHA_OPT_FOLD_KANA == 32
    assert "AHA_OPT_FOLD_KANA" in open(os.path.join(ROOT, "include", "aha", "ac.hpp")).read()
    assert re.search(r"OPT_FOLD_KANA\s*=\s*32_u32", open(os.path.join(ROOT, "bindings", "crystal", "aha_hip.cr")).read())
    for doc in ("README.md", "INTEGRATION.md", "DESIGN.md", os.path.join("tools", "README.md")):
        text = open(os.path.join(ROOT, doc)).read()
        assert "fold_kana" in text or "AHA_OPT_FOLD_KANA" in text or "gen_foldk_table" in text, doc
    assert "AHA_FOLDK_HALO" in open(os.path.join(ROOT, "DESIGN.md")).read()
    listed = open(os.path.join(CSRC, "exports.map")).read()
    assert len(re.findall(r"^\s+aha_\w+;", listed, re.M)) == 90
    assert N.lib().aha_abi_version() == 8 and re.search(r"#define AHA_ABI_VERSION 8\b", hdr)
    assert C.sizeof(N.aha_options) == 16 and C.sizeof(N.aha_ac_info_t) == 136
    out = subprocess.run(["nm", "-D", "--defined-only", N.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert len([ln for ln in out.splitlines() if re.search(r" T aha_\w+$", ln)]) == 90


# ---- host-only handles -------------------------------------------------------------------------------------------------------
def test_keys_equal_after_the_fold_are_duplicates():
    for pair in (["あ", "ア"], ["ｱ", "ア"], ["ｱ", "あ"], ["ゝ", "ヽ"], ["ｰ", "ー"], ["こんぴゅーた", "コンピュータ"]):
        with pytest.raises(AhaError) as e:
            AC.compile(pair, host_only=True, fold_kana=True)
        assert e.value.code == N.AHA_E_DUP_KEY and e.value.key_index == 1, pair
        assert AC.compile(pair, host_only=True, fold_bmp=True).n_keys == 2  # fold_bmp handles do not merge them
    with pytest.raises(AhaError) as e:
        AC.compile(["x", "か", "y", "ｶ"], host_only=True, fold_kana=True)
    assert e.value.code == N.AHA_E_DUP_KEY and e.value.key_index == 3
    # the limits: a voiced half-width sequence is not the voiced letter, small and large stay apart, the marks stay
    assert AC.compile(["ｶﾞ", "ガ", "ぁ", "あ", "ﾞ", "ﾟ", "゛", "ヷ", "ゟ", "ヿ", "わ"], host_only=True, fold_kana=True).n_keys == 11
    with pytest.raises(AhaError) as e:
        AC.compile(["ｶﾞ", "カﾞ"], host_only=True, fold_kana=True)
    assert e.value.code == N.AHA_E_DUP_KEY
    for pair in (["ＡＢＣ", "ａｂｃ"], ["Привет", "ПРИВЕТ"], ["Foo", "fOO"], ["Ệ", "ệ"]):  # it implies the three case folds
        with pytest.raises(AhaError) as e:
            AC.compile(pair, host_only=True, fold_kana=True)
        assert e.value.code == N.AHA_E_DUP_KEY


def test_a_key_is_folded_on_its_own():
    # a lead byte that ends one key never joins the continuation bytes that open the next
    m = AC.compile([b"a\xe3", b"\x81\x82b", "ア".encode(), b"A\xe3\x81\x82B", b"q\xef\xbd", b"\xb1r"], host_only=True, fold_kana=True)
    assert m.n_keys == 6
    assert m[b"A\xe3"] == 0 and m[b"\x81\x82B"] == 1 and m["あ".encode()] == 2 and m["ｱ".encode()] == 2 and m["aアb".encode()] == 3
    assert m[b"Q\xef\xbd"] == 4 and m[b"\xb1R"] == 5
    with pytest.raises(IndexError):
        m[b"\x82\xa2b"]  # (what key 1 would be had it been folded behind key 0's lead byte)


def test_ids_fold_their_argument_keys_keep_their_spelling_load_and_replicate():
    keys = ["コンピュータ", "ひらがな", "ｶﾀｶﾅ", "ＥＲＲＯＲ", "Việt Nam", "école", "ПРИВЕТ", "Foo", "漢字"]
    m = AC.compile(keys, host_only=True, fold_kana=True)
    assert m.fold_kana and m.fold_bmp is False and m.fold_simple is False and m.fold_ascii is False
    assert N.lib().aha_ac_flags(m._h) == N.AHA_OPT_HOST_ONLY | N.AHA_OPT_FOLD_KANA  # the bits as passed
    assert m["こんぴゅーた"] == 0 and m["ｺﾝﾋﾟｭｰﾀ".replace("ﾋﾟ", "ピ")] == 0 and m["ヒラガナ"] == 1 and m["ﾋﾗｶﾞﾅ".replace("ｶﾞ", "が")] == 1
    assert m["カタカナ"] == 2 and m["かたかな"] == 2 and m["ｅｒｒｏｒ"] == 3 and m["VIỆT NAM"] == 4 and m["ÉCOLE"] == 5
    assert m["привет"] == 6 and m["FOO"] == 7 and m["漢字"] == 8
    assert [m[i] for i in range(len(keys))] == keys
    with pytest.raises(IndexError):
        m["ｺﾝﾋﾟｭｰﾀ"]  # (the half-width voiced sequence is seven characters, not six)
    every = AC.compile(keys, host_only=True, fold_ascii=True, fold_simple=True, fold_bmp=True, fold_kana=True)
    assert N.lib().aha_ac_flags(every._h) == (N.AHA_OPT_HOST_ONLY | N.AHA_OPT_FOLD_ASCII | N.AHA_OPT_FOLD_SIMPLE | N.AHA_OPT_FOLD_BMP |
                                             N.AHA_OPT_FOLD_KANA)
    assert every.fold_kana and every.fold_bmp and every["こんぴゅーた"] == 0
    bmp = AC.compile(keys, host_only=True, fold_bmp=True)
    assert bmp.fold_kana is False and bmp["ｅｒｒｏｒ"] == 3
    with pytest.raises(IndexError):
        bmp["こんぴゅーた"]
    # the container: the caller's spelling, nothing new; the flag is said again at load
    data = m.to_bytes()
    assert data == AC.compile(keys, host_only=True).to_bytes()
    again = AC.from_bytes(data, host_only=True, fold_kana=True)
    assert again.fold_kana and [again[i] for i in range(len(keys))] == keys and again["こんぴゅーた"] == 0
    with pytest.raises(AhaError) as e:
        AC.from_bytes(AC.compile(["あ", "ア"], host_only=True).to_bytes(), host_only=True, fold_kana=True)
    assert e.value.code == N.AHA_E_DUP_KEY
    # replicate copies the flag (a host-only handle has no device to replicate to: the flags of the refusal's source stay)
    h = C.c_void_p()
    rc = N.lib().aha_ac_replicate(m._h, 0, C.byref(h))
    if rc == N.AHA_OK:
        try:
            assert N.lib().aha_ac_flags(h) & N.AHA_OPT_FOLD_KANA
        finally:
            N.lib().aha_ac_free(h)
    else:
        assert not h.value
    src = open(os.path.join(CSRC, "capi.cpp")).read()
    assert "ac->opt_flags = src->opt_flags & ~AHA_OPT_HOST_ONLY" in src  # every option bit travels


LETTERS = ("abcXYZ" + "あいうえおかきくけこがぎぐゃゅょっー" + "アイウエオカキクケコガギグャュョッ" + "ｱｲｳｴｵｶｷｸｹｺｬｭｮｯｰﾞﾟ" + "ａｂｃＡＢＣ" + "абвАБВ" + "漢字日本語")


def test_handle_is_the_plain_handle_of_the_folded_keys():
    rng = random.Random(5)
    keys, seen = [], set()
    while len(keys) < 300:
        k = "".join(rng.choice(LETTERS) for _ in range(rng.randint(2, 9))).encode()
        if foldksim.foldk(k) not in seen:
            seen.add(foldksim.foldk(k))
            keys.append(k)
    assert sum(foldksim.foldk(k) != fold3sim.fold3(k) for k in keys) > 100
    f = AC.compile(keys, host_only=True, fold_kana=True)
    p = AC.compile(foldksim.foldk_keys(keys), host_only=True)
    assert f.info == p.info
    for which in (N.AHA_IMG_SLOTS, N.AHA_IMG_END_KEY, N.AHA_IMG_KEY_LN, N.AHA_IMG_STALE_ENDS, N.AHA_IMG_UNIT_SLOTS, N.AHA_IMG_UNIT_TABLES):
        assert f.export(which, np.uint8).tobytes() == p.export(which, np.uint8).tobytes(), which


# ---- the refusals ------------------------------------------------------------------------------------------------------------
def test_feeds_and_groups_are_refused_before_any_device_work():
    m = AC.compile(["カナ"], host_only=True, fold_kana=True)  # (host-only: a call that reached the device would say NO_DEVICE)
    h = C.c_void_p()
    assert N.lib().aha_feed_open(m._h, 1, 0, C.byref(h)) == N.AHA_E_INVALID and not h.value
    msg = N.lib().aha_last_error(m._h).decode()
    assert "AHA_OPT_FOLD_KANA" in msg and "follow-up" in msg
    p = N.aha_match_params()
    p.struct_size = C.sizeof(N.aha_match_params)
    assert N.lib().aha_feed_open_params(m._h, 1, 0, C.byref(p), C.byref(h)) == N.AHA_E_INVALID and not h.value
    assert N.lib().aha_feed_open_params(m._h, 1, N.AHA_FEED_CHARS, None, C.byref(h)) == N.AHA_E_INVALID
    with pytest.raises(AhaError) as e:
        m.feed(1)
    assert e.value.code == N.AHA_E_INVALID and "AHA_OPT_FOLD_KANA" in str(e.value)
    blob = np.frombuffer("カナabc".encode(), dtype=np.uint8)
    offs = np.array([0, 6, 9], dtype=np.uint64)
    devs = np.array([0, 0], dtype=np.int32)
    ek = C.c_uint32(0)
    for flags in (N.AHA_OPT_FOLD_KANA, N.AHA_OPT_FOLD_KANA | N.AHA_OPT_HOST_ONLY,
                  N.AHA_OPT_FOLD_KANA | N.AHA_OPT_FOLD_BMP | N.AHA_OPT_FOLD_SIMPLE | N.AHA_OPT_FOLD_ASCII):
        g = C.c_void_p()
        rc = N.lib().aha_group_compile(blob.ctypes.data, offs.ctypes.data, 2, devs.ctypes.data, 2, flags, C.byref(g), C.byref(ek))
        assert rc == N.AHA_E_INVALID and not g.value
        assert "AHA_OPT_FOLD_KANA" in N.lib().aha_last_error(None).decode()


# ---- the device arithmetic ---------------------------------------------------------------------------------------------------
# stray bytes: kana lead and continuation bytes, other leads, a four-byte lead, an invalid byte
ALPHABET = [ord(c) for c in "abXY"] + [0xD0, 0xC3, 0xE0, 0xE3, 0xEF, 0xE4, 0xED, 0x81, 0x82, 0x83, 0xBD, 0xBE, 0xB1, 0xA0, 0xF0, 0xC1]
TOKENS = [c.encode() for c in "あぴゅゝゞゖアピヷｱｶﾞｰｦﾝ･ＡａРÉ漢"]


def random_bytes(rng, n):
    """n bytes, four in ten of them single bytes of the alphabet, the rest whole characters (the last one perhaps cut)"""
    out = bytearray()
    while len(out) < n:
        out += bytes([rng.choice(ALPHABET)]) if rng.random() < 0.4 else rng.choice(TOKENS)
    return bytes(out[:n])


def random_offsets(rng, n):
    """document offsets over n bytes, empty and one-byte documents included"""
    cuts = sorted(rng.randint(0, n) for _ in range(rng.randint(0, 6)))
    if cuts and rng.random() < 0.5:
        c = cuts[rng.randrange(len(cuts))]
        cuts.extend([c, min(n, c + 1)])  # an empty document and a one-byte one
        cuts.sort()
    return [0] + cuts + [n]


def test_kernel_model_is_the_per_document_fold_on_random_cases():
    """3000 small cases; the model's piece is 4 bytes and its wave 4 lanes, so that a case of a few dozen bytes has pieces
    across lanes, waves, workgroups and strides, unrolled and remainder steps and partial waves (the arithmetic is the kernel's
    with 16 and 64 for 4 and 4; the tests below use the kernel's own sizes)"""
    rng = random.Random(23)
    seen = {"neighbour_loads": 0, "from_lanes": 0, "unrolled": 0, "remainder": 0, "idle_lanes": 0, "fixed": 0, "moved": 0}
    for case in range(3000):
        n = rng.choice((rng.randint(0, 12), rng.randint(13, 140), rng.randint(100, 400)))
        buf = random_bytes(rng, n)
        off = random_offsets(rng, n)
        want = foldksim.foldk_docs(buf, off)
        grid, block = rng.choice(((1, 4), (1, 8), (2, 4), (2, 8), (3, 4)))
        for halo in ("mem", "lane"):
            got, stats = foldksim.kernel_model(buf, off, halo=halo, piece=4, wave=4, grid=grid, block=block)
            assert got == want, (case, n, off, grid, block, halo)
            for k in stats:
                seen[k] += stats[k]
        seen["fixed"] += want != foldksim.foldk(buf)
        seen["moved"] += want != fold3sim.fold3_docs(buf, off)
    # the cases the model is there for did occur
    assert seen["from_lanes"] > 10000 and seen["neighbour_loads"] > 5000 and seen["unrolled"] > 1000 and seen["remainder"] > 1000, seen
    assert seen["idle_lanes"] > 1000 and seen["fixed"] > 300 and seen["moved"] > 2000, seen


def test_kernel_model_at_the_kernels_own_sizes():
    rng = random.Random(29)
    # wave and grid edges: 3 KiB + 5 on one workgroup; 1800 pieces on two workgroups (unrolled and remainder steps, the last
    # wave of the remainder partial: 1800 = 3 * 512 + 264 = 3 * 512 + 4 * 64 + 8); a last wave of 37 lanes
    for n, grid in ((3 * 1024 + 5, 1), (1800 * 16 + 5, 2), (16 * (64 + 37) + 5, 1)):
        for lead_in in (b"", b"x", b"xy"):
            buf = (lead_in + "あｱア".encode() * (n // 9 + 1))[:n]
            off = [0, 7, 7, 8, 1023, 1024, 1025, n] if n > 2000 else [0, n]
            want = foldksim.foldk_docs(buf, off)
            assert want != buf
            m, ms = foldksim.kernel_model(buf, off, halo="mem", grid=grid)
            l, ls = foldksim.kernel_model(buf, off, halo="lane", grid=grid)
            assert m == want and l == want
            # the lane form loads at a wave's two edges only: at most four bytes per wave step
            waves = -(-(n // 16) // 64)
            assert ls["neighbour_loads"] <= 4 * waves < ms["neighbour_loads"] and ls["from_lanes"] >= (n // 16) - 2 * waves
            if grid == 2:
                assert ls["unrolled"] > 0 and ls["remainder"] > 0 and ls["idle_lanes"] == 64 - 8
            if n == 16 * (64 + 37) + 5:
                assert ls["idle_lanes"] == 64 - 37 and ls["unrolled"] == 0
    for n in (0, 1, 2, 15, 16, 17, 31, 32, 33):
        for lead_in in (0, 1, 2):
            buf = ("ぴｭー".encode() * 6)[lead_in:lead_in + n]
            for halo in ("mem", "lane"):
                assert foldksim.kernel_model(buf, [0, len(buf)], halo=halo)[0] == foldksim.foldk(buf)
    for _ in range(20):  # random text at the kernel's sizes, a few hundred pieces
        n = rng.randint(1024, 6000)
        buf, off = random_bytes(rng, n), random_offsets(rng, n)
        for halo in ("mem", "lane"):
            assert foldksim.kernel_model(buf, off, halo=halo, grid=rng.choice((1, 2)), block=rng.choice((64, 256)))[0] == foldksim.foldk_docs(buf, off)


def test_kernel_model_on_every_cut_of_a_triple_by_a_boundary():
    for c in ("あ", "ｱ", "ゞ", "Ａ", "ア", "漢"):
        t = c.encode()
        for phase in range(16):  # the triple at every phase of a piece, the piece behind the first one
            buf = b"Q" * (16 + phase) + t + b"Zz" * 9
            at = 16 + phase
            whole = foldksim.foldk(buf)
            kept = whole[:at] + t + whole[at + 3:]  # the character not folded
            for off in ([0, at + 1, len(buf)], [0, at + 2, len(buf)], [0, at + 1, at + 2, len(buf)], [0, at + 1, at + 1, at + 2, len(buf)],
                        [0, at, at + 3, len(buf)], [0, at + 3, len(buf)]):
                want = foldksim.foldk_docs(buf, off)
                cut = any(at < b < at + 3 for b in off)
                assert want == (kept if cut else whole)
                for halo in ("mem", "lane"):
                    assert foldksim.kernel_model(buf, off, halo=halo)[0] == want, (c, phase, off, halo)
                    assert foldksim.kernel_model(buf, off, halo=halo, piece=4, wave=4, grid=2, block=4)[0] == want


def test_foldk_byte_is_the_rule_at_every_position():
    rng = random.Random(17)
    for _ in range(400):
        buf = random_bytes(rng, rng.randint(0, 24))
        n = len(buf)
        at = lambda j: buf[j] if 0 <= j < n else 0
        assert bytes(foldksim.foldk_byte(at(j - 2), at(j - 1), buf[j], at(j + 1), at(j + 2)) for j in range(n)) == foldksim.foldk(buf)


# ---- foldk_bytes and foldk_byte under the sanitizers, as their own process ---------------------------------------------------
def test_spec_foldk_runs_clean_under_asan_and_ubsan(tmp_path):
    exe = str(tmp_path / "spec_foldk")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           os.path.join(ROOT, "tests", "cpp", "spec_foldk.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "spec_foldk: ok" in r.stdout


def test_host_only_sanitizer_library_lists_the_new_stub():
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert mk.count("../../tests/cpp/foldk_stubs.cpp") == 2 and os.path.exists(os.path.join(ROOT, "tests", "cpp", "foldk_stubs.cpp"))
    assert mk.count("../../tests/cpp/fold3_stubs.cpp") == 2 and mk.count("../../tests/cpp/fold2_stubs.cpp") == 2
    assert "foldk_table.hpp" in mk
