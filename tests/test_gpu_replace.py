"""Replace calls (aha_ac_replace_batch, aha_ac_replace_batch_device) against replacesim over selectsim over the CPU ORACLE's hits
(never the library's own select): every engine variant on ragged documents, everything deleted, ties of adjacent deletions,
growth over several tiles, the scan's boundaries, the select tests' special cases, every alignment of out and corpus, capacity,
overlap, document ranges, and what a call leaves behind on the handle.  Every case is a few KiB of text."""
import ctypes as C
import random
import zlib

import numpy as np
import pytest

import pyoracle as orc
import replacesim
from aha_amd import AC, AhaError, DeviceCorpus
from aha_amd import _native as N
from engine_variants import VARIANTS, use_variant
from test_gpu_doc_counts import KEYSETS, SEP_BITS, _batch, _sep
from test_gpu_select import SIZES, _ragged_docs, _tensors, _want

pytestmark = pytest.mark.gpu

GUARD8, GUARD64 = 0xA5, 0x5A5A5A5A5A5A5A5A
PAD = 48
SCAN_BLOCK = 256  # selected hits of one block of the scan = block sums one lane of the scan over the sums takes (image.hpp)


def _expect(o, corpus, offs, repl, sep_pair=None, text=None):
    """replacesim over selectsim over the oracle's hits of `corpus` (applied to `text`: a folded handle's original bytes)
    -> (bytes uint8, doc_out_offsets, n_selected, n_hits)"""
    sel, dso, hits, _ = _want(o, corpus, offs, sep_pair)
    want, doo = replacesim.replace(corpus if text is None else text, offs, sel, dso, repl)
    return want, doo, sel.size, hits.size


def _device(m, table, ct, ot, D, cap, sep=None, out_off=0):
    """the device entry with guard bytes in front of out (out_off of them: out's alignment), behind cap bytes and behind the
    D + 1 offsets -> (out[:cap], doo, n_out_bytes, n_selected, n_hits, rc)"""
    import torch

    raw = torch.full((out_off + cap + PAD,), GUARD8, dtype=torch.uint8, device=ct.device)
    assert raw.data_ptr() % 16 == 0
    doo = torch.full((D + 1 + PAD,), GUARD64, dtype=torch.int64, device=ct.device)
    rc, ns, nh = N.AHA_OK, None, None
    try:
        n, ns, nh = m.replace_batch_device(ct, ot, table, raw[out_off:], doo, sep=sep, cap=cap)
    except AhaError as e:
        if e.code != N.AHA_E_CAPACITY:
            raise
        rc, n = e.code, e.n_required
    torch.cuda.synchronize()
    raw_h, doo_h = raw.cpu().numpy(), doo.cpu().numpy().view(np.uint64)
    assert (raw_h[:out_off] == GUARD8).all(), "the call wrote in front of out"
    assert (raw_h[out_off + cap:] == GUARD8).all(), "the call wrote behind cap_bytes"
    assert (doo_h[D + 1:] == GUARD64).all(), "the call wrote behind the D + 1 offsets"
    return raw_h[out_off:out_off + cap], doo_h[:D + 1], n, ns, nh, rc


def _check_device(m, table, o, corpus, offs, repl, out_off=0, ct=None, sep_pair=None, sep=None, text=None, exp=None):
    want, want_doo, n_sel, n_hits = exp or _expect(o, corpus, offs, repl, sep_pair, text)
    src = corpus if text is None else text
    if ct is None:
        ct = _tensors(src, offs)[0]
    ot = _tensors(src, offs)[1]
    D = offs.size - 1
    got, doo, n, ns, nh, rc = _device(m, table, ct, ot, D, want.size + 3, sep=sep, out_off=out_off)
    assert rc == N.AHA_OK and (n, ns, nh) == (want.size, n_sel, n_hits)
    assert np.array_equal(doo, want_doo)
    assert got[:n].tobytes() == want.tobytes()
    assert (got[n:] == GUARD8).all(), "the call wrote behind the total"
    return want, want_doo, got, doo


def _check_all_entries(m, o, corpus, offs, repl, sep_pair=None, sep=None, text=None):
    """device entry (twice: identical bytes) and host entry: the bytes of replacesim over selectsim over the oracle's hits"""
    table = m.replacements(repl)
    exp = _expect(o, corpus, offs, repl, sep_pair, text)  # (computed once: it is the slow part)
    want, want_doo, got, doo = _check_device(m, table, o, corpus, offs, repl, sep=sep, text=text, exp=exp)
    _, _, got2, doo2 = _check_device(m, table, o, corpus, offs, repl, sep=sep, text=text, exp=exp)
    assert got2.tobytes() == got.tobytes() and doo2.tobytes() == doo.tobytes()
    h_out, h_doo = m.replace_batch(corpus if text is None else text, offs, table, sep=sep)  # the host entry
    assert h_out.tobytes() == want.tobytes() and np.array_equal(h_doo, want_doo)
    return want, want_doo


def _gap(n, at=0):
    """n bytes no ASCII key can match, each a function of its position (at + i): a copy from a wrong address, or with its bytes
    in a wrong order, gives other bytes.  (The second term: 7 i alone repeats every 128 bytes, so at every multiple of a tile.)"""
    return bytes(0x80 | ((7 * i + 13 * (i >> 7)) & 0x7F) for i in range(at, at + n))


def _fast_tiles(text_mod, out_mod, offs, sel, dso, repl, total):
    """krp_copy's choice of path, restated: for every 1024-byte tile of the output (from the first 16-byte aligned address of
    out on) that lies inside one gap, the distance of its source from a 16-byte aligned address -- (text + q - shift) & 15, the
    value the fast path's byte alignment turns on"""
    n = sel.shape[0]
    off = offs.astype(np.int64)
    doc = np.searchsorted(dso.astype(np.int64)[:-1], np.arange(n), side="right") - 1
    rep = [replacesim.replacement_of(repl, int(v)) for v in sel["value"]]
    rlen = np.array([0 if r is None else len(r) for r in rep], dtype=np.int64)
    delta = np.array([0 if r is None else len(r) - int(e - s) for r, s, e in zip(rep, sel["start"], sel["end"])], dtype=np.int64)
    shift = np.concatenate([[0], np.cumsum(delta)]).astype(np.int64)
    O = off[doc] + sel["start"].astype(np.int64) + shift[:n]
    ks = []
    head = min((16 - out_mod) & 15, total)
    for q0 in range(head, total - 1023, 1024):
        j = int(np.searchsorted(O, q0, side="right")) - 1
        gap_from = int(O[j] + rlen[j]) if j >= 0 else 0
        gap_to = int(O[j + 1]) if j + 1 < n else total
        if gap_from <= q0 and q0 + 1024 <= gap_to:
            ks.append((text_mod + q0 - int(shift[j + 1])) & 15)
    return ks


def _mixed_table(rng, keys):
    """per key one of: shorter, equal, longer, empty, with NUL bytes, kept (None) -- every kind at least once"""
    kinds = ["shorter", "equal", "longer", "empty", "nul", "keep"]
    order = kinds * (len(keys) // len(kinds) + 1)
    rng.shuffle(order)
    out = []
    for k, kind in zip(keys, order):
        out.append({"shorter": k[:len(k) // 2], "equal": bytes(reversed(k)), "longer": b"<" + k + b"|" + k + b">", "empty": b"",
                    "nul": b"\x00" + k[:1] + b"\x00", "keep": None}[kind])
    return out


@pytest.fixture(params=VARIANTS)
def variant(request, monkeypatch):
    return use_variant(request.param, monkeypatch)


@pytest.mark.parametrize("keyset", ["ascii", "utf8", "nested"])
def test_replace_parity_every_engine_variant(variant, keyset):
    rng = random.Random(zlib.crc32(f"rep/{keyset}".encode()))
    keys = KEYSETS[keyset](rng)
    m, o = AC.compile(keys), orc.AC.compile(keys)
    docs = _ragged_docs(rng, keys)
    assert sorted({len(d) for d in docs}) == SIZES and docs[0] == docs[-1] == b""
    corpus, offs = _batch(docs)
    repl = _mixed_table(rng, keys)
    want, _ = _check_all_entries(m, o, corpus, offs, repl)
    assert want.size and want.tobytes() != corpus.tobytes()


def test_replace_everything_deleted():
    m, o = AC.compile([b"a", b"b"]), orc.AC.compile([b"a", b"b"])
    for docs in ([b"a" * 1000], [b"a" * 700, b"", b"a" * 300], [b"a"]):
        corpus, offs = _batch(docs)
        want, doo = _check_all_entries(m, o, corpus, offs, [b"", None])
        assert want.size == 0 and not doo.any()
    corpus, offs = _batch([b"a" * 999 + b"b", b"a" * 40 + b"-"])  # ... except the last byte
    want, doo = _check_all_entries(m, o, corpus, offs, [b"", None])
    assert want.tobytes() == b"b-" and doo.tolist() == [0, 1, 2]


def test_replace_ties_of_adjacent_deletions():
    """runs of adjacent deleted hits start at one output position: the last of them decides what stands there"""
    keys = [b"a", b"b", b"c", b"de"]
    m, o = AC.compile(keys), orc.AC.compile(keys)
    docs = [b"aaab--", b"aaa-", b"aaac", b"dededeb", b"adeadeb-", b"aaa", b"", b"a" * 70 + b"b" + b"a" * 70 + b"-" + b"de" * 40 + b"c"]
    corpus, offs = _batch(docs)
    want, _ = _check_all_entries(m, o, corpus, offs, [b"", b"XY", None, b""])
    assert want.tobytes() == b"XY--" + b"-" + b"c" + b"XY" + b"XY-" + b"XY-c"


@pytest.mark.parametrize("size", [300, 5000])
def test_replace_growth_over_several_tiles(monkeypatch, size):
    """one replacement longer than a lane's, a wave's and (5000) a pass of the whole grid's share of the output"""
    monkeypatch.setenv("AHA_REPLACE_BLOCKS", "1")
    m, o = AC.compile([b"a", b"q"]), orc.AC.compile([b"a", b"q"])
    big = bytes((7 * i + 3) & 255 for i in range(size))
    corpus, offs = _batch([b"-" * 37 + b"a" + b"-" * 50 + b"a", b"a", b"", b"--a--q", _gap(2100)])  # (whole tiles in one gap)
    want, doo = _check_all_entries(m, o, corpus, offs, [big, b"Q"])
    assert want.size == corpus.size + 4 * (size - 1) and int(doo[1]) == 37 + size + 50 + size


@pytest.mark.parametrize("n", [0, 1, SCAN_BLOCK - 1, SCAN_BLOCK, SCAN_BLOCK + 1, SCAN_BLOCK * SCAN_BLOCK - 1, SCAN_BLOCK * SCAN_BLOCK,
                               SCAN_BLOCK * SCAN_BLOCK + 1])
def test_replace_scan_boundaries(monkeypatch, n):
    """n selected hits, every byte of the text one of them; a grid of one workgroup loops over the scan's blocks"""
    monkeypatch.setenv("AHA_REPLACE_BLOCKS", "1")
    m, o = AC.compile([b"a", b"b", b"c"]), orc.AC.compile([b"a", b"b", b"c"])
    text = (b"abc" * (n // 3 + 1))[:n]
    docs = [text[i:i + 16] for i in range(0, n, 16)] or [b"--"]
    corpus, offs = _batch(docs)
    assert corpus.size < 100 << 10
    table = m.replacements([b"XY", b"", None])
    want, want_doo, n_sel, _ = _expect(o, corpus, offs, [b"XY", b"", None])
    assert n_sel == n
    ct, ot = _tensors(corpus, offs)
    got, doo, nb, ns, _, rc = _device(m, table, ct, ot, offs.size - 1, want.size)
    assert rc == N.AHA_OK and ns == n and nb == want.size
    assert got.tobytes() == want.tobytes() and np.array_equal(doo, want_doo)


def test_replace_chain_hit_is_not_the_first_at_its_end():
    keys = ["ab", "bcd", "cd", "d"]
    m, o = AC.compile(keys), orc.AC.compile(keys)
    corpus, offs = _batch([b"abcd", b"", b"xabcdd", b"bcdabcd"])
    want, _ = _check_all_entries(m, o, corpus, offs, {0: "<AB>", 2: "", 3: "!"})
    assert want.tobytes() == b"<AB>" + b"x<AB>!" + b"bcd<AB>"


def test_replace_one_long_run():
    keys = [b"a", b"aa", b"aaa"]
    m, o = AC.compile(keys), orc.AC.compile(keys)
    doc = b"a" * 1201
    corpus, offs = _batch([doc, doc])
    want, doo = _check_all_entries(m, o, corpus, offs, [b"1", b"22", b"xyzw"])
    assert want.tobytes() == (b"xyzw" * 400 + b"1") * 2 and doo.tolist() == [0, 1601, 3202]


def test_replace_with_a_separator_filter():
    rng = random.Random(77)
    keys = KEYSETS["ascii"](rng)
    m, o = AC.compile(keys), orc.AC.compile(keys)
    corpus, offs = _batch(_ragged_docs(rng, keys, 0.5))
    bits = [i for i in range(40) if i not in SEP_BITS]
    repl = _mixed_table(rng, keys)
    want, _ = _check_all_entries(m, o, corpus, offs, repl, (40, bits), _sep())
    assert want.tobytes() != _expect(o, corpus, offs, repl)[0].tobytes()


def test_replace_nul_bytes_in_text_and_replacements():
    keys = [b"ab", b"abc", b"bc", b"c\x01"]  # (a key itself holds no NUL byte: compile refuses it)
    m, o = AC.compile(keys), orc.AC.compile(keys)
    corpus, offs = _batch([b"\x00abc\x00\x00abc\x01\x00", b"\x00" * 40, b"ab\x00c\x01abc", b"\x00"])
    want, _ = _check_all_entries(m, o, corpus, offs, [b"\x00", b"\x00\x00\x00\x00\x00", None, b"\x00\x01\x00"])
    assert want.tobytes().count(b"\x00") > 50 and b"\x00\x00\x00\x00\x00" * 2 in want.tobytes().replace(b"\x01", b"")


def test_replace_on_a_folded_handle_keeps_the_original_case():
    rng = random.Random(5)
    words = sorted({"".join(rng.choice("abcdEFGH") for _ in range(rng.randint(2, 6))) for _ in range(200)}, key=str.lower)
    keys = [w.encode() for w in {w.lower(): w for w in words}.values()]  # distinct after folding
    m = AC.compile(keys, fold_ascii=True)
    o = orc.AC.compile([k.lower() for k in keys])
    docs = _ragged_docs(rng, [k.swapcase() for k in keys] + keys)
    corpus, offs = _batch(docs)
    low = np.frombuffer(corpus.tobytes().lower(), dtype=np.uint8).copy()
    repl = _mixed_table(rng, keys)
    want, _ = _check_all_entries(m, o, low, offs, repl, text=corpus)  # the oracle over the folded text, the slices of the original
    assert want.tobytes() != replacesim.replace(low, offs, *_want(o, low, offs)[:2], repl)[0].tobytes()
    kept_only, _ = _check_all_entries(m, o, low, offs, [None] * len(keys), text=corpus)  # inside kept hits too
    assert kept_only.tobytes() == corpus.tobytes() != low.tobytes()


@pytest.mark.parametrize("off", [1, 5, 15])
def test_replace_any_alignment_of_out_and_corpus(off):
    import torch

    rng = random.Random(31 + off)
    keys = KEYSETS["ascii"](rng)
    m, o = AC.compile(keys), orc.AC.compile(keys)
    corpus, offs = _batch(_ragged_docs(rng, keys, 0.3) + [_gap(3000)])  # (sparse hits and a long gap: whole tiles in one gap)
    repl = _mixed_table(rng, keys)
    table = m.replacements(repl)
    _check_device(m, table, o, corpus, offs, repl, out_off=off)
    raw = torch.full((corpus.size + 64,), GUARD8, dtype=torch.uint8, device="cuda:0")
    raw[off:off + corpus.size] = torch.from_numpy(corpus).to("cuda:0")
    ct = raw[off:off + corpus.size]
    assert ct.data_ptr() % 16 == off
    _check_device(m, table, o, corpus, offs, repl, ct=ct)
    _check_device(m, table, o, corpus, offs, repl, out_off=16 - off, ct=ct)


def test_replace_whole_tiles_in_a_gap_at_every_source_alignment():
    """The copy's fast path -- two aligned 16-byte loads, a byte alignment, one aligned store -- takes the tiles that lie inside
    one gap.  Gaps of position-dependent bytes, longer than two tiles, behind shifts of 0, +1, +1 (behind a kept hit) and -1,
    the last over two documents; the corpus at each of the 16 byte offsets from an aligned address, out aligned and not.
    Every distance of the source from an aligned address, 0 .. 15, must occur with an aligned out alone and with the others
    alone: asserted here from the tiles."""
    import torch

    keys = [b"ab", b"cd", b"ef"]
    repl = [b"XYZ", None, b""]
    m, o = AC.compile(keys), orc.AC.compile(keys)
    docs = [_gap(2500) + b"ab" + _gap(2500, 2500) + b"cd" + _gap(2500, 5000) + b"ef" + _gap(2100, 7500), b"", _gap(1100, 9600),
            b"ab"]
    corpus, offs = _batch(docs)
    table = m.replacements(repl)
    sel, dso, _, _ = _want(o, corpus, offs)
    exp = _expect(o, corpus, offs, repl)
    assert sel.shape[0] == 4 and exp[0].size == corpus.size + 1 + 0 - 2 + 1
    raw = torch.full((corpus.size + 64,), GUARD8, dtype=torch.uint8, device="cuda:0")
    assert raw.data_ptr() % 16 == 0
    seen = {True: [], False: []}
    for off in range(16):
        raw[off:off + corpus.size] = torch.from_numpy(corpus).to("cuda:0")
        ct = raw[off:off + corpus.size]
        for out_off in (0, (7 * off + 1) % 16 or 9):
            ks = _fast_tiles(off, out_off, offs, sel, dso, repl, exp[0].size)
            assert len(ks) >= 4, ks  # (a gap of 2047 bytes or more holds a whole tile; the last two are one gap of 3200)
            seen[out_off == 0] += ks
            _check_device(m, table, o, corpus, offs, repl, out_off=out_off, ct=ct, exp=exp)
    assert set(seen[True]) == set(range(16)) and set(seen[False]) == set(range(16)), seen


@pytest.mark.parametrize("off", [0, 5, 15])
def test_replace_small_totals_head_and_tail(off):
    """totals of 0 .. 17 and 31 .. 33 bytes at an aligned and two unaligned outs: head only, tail only, both"""
    m, o = AC.compile([b"a", b"b"]), orc.AC.compile([b"a", b"b"])
    repl = [b"", b"BB"]
    table = m.replacements(repl)
    for total in list(range(18)) + [31, 32, 33]:
        body = (b"xyzwvutsrqponmlkjihgfedc" * 2)[:max(total - 2, 0)]
        docs = [b"aaaaa" + body[:len(body) // 2], b"", body[len(body) // 2:] + (b"b" if total >= 2 else b"-" * total) + b"a"]
        corpus, offs = _batch(docs)
        want, _, _, _ = _check_device(m, table, o, corpus, offs, repl, out_off=off)
        assert want.size == total


def test_replace_capacity_writes_nothing():
    rng = random.Random(21)
    keys = KEYSETS["ascii"](rng)
    m, o = AC.compile(keys), orc.AC.compile(keys)
    corpus, offs = _batch(_ragged_docs(rng, keys))
    repl = _mixed_table(rng, keys)
    table = m.replacements(repl)
    want, want_doo, n_sel, n_hits = _expect(o, corpus, offs, repl)
    D = offs.size - 1
    ct, ot = _tensors(corpus, offs)
    for cap in (want.size - 1, 0):
        got, doo, n, _, _, rc = _device(m, table, ct, ot, D, cap)
        assert rc == N.AHA_E_CAPACITY and n == want.size
        assert (got == GUARD8).all() and (doo == GUARD64).all(), "a failing call wrote a caller's buffer"
    got, doo, n, ns, nh, rc = _device(m, table, ct, ot, D, want.size)  # the exact fit
    assert rc == N.AHA_OK and (n, ns, nh) == (want.size, n_sel, n_hits)
    assert got.tobytes() == want.tobytes() and np.array_equal(doo, want_doo)
    with pytest.raises(AhaError) as e:  # the sizing call: out == NULL, cap_bytes == 0
        m.replace_batch_device(ct, ot, table, None)
    assert e.value.code == N.AHA_E_CAPACITY and e.value.n_required == want.size
    # the host entry, one short
    L = N.lib()
    n64, ns64, nh64 = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
    out = np.full(want.size, GUARD8, dtype=np.uint8)
    doo_h = np.full(D + 1, GUARD64, dtype=np.uint64)
    rc = L.aha_ac_replace_batch(m._h, table._h, corpus.ctypes.data, offs.ctypes.data, D, None, 0, out.ctypes.data, want.size - 1,
                                doo_h.ctypes.data, C.byref(n64), C.byref(ns64), C.byref(nh64))
    assert rc == N.AHA_E_CAPACITY and n64.value == want.size and (out == GUARD8).all() and (doo_h == GUARD64).all()
    assert (ns64.value, nh64.value) == (n_sel, n_hits)  # (the counts come with the required size, as from the device entry)
    # a total of 0 succeeds with cap_bytes == 0; N = 0 and D = 0 are valid
    for docs in ([b"", b"", b""], [], [b""]):
        c_e = np.zeros(0, dtype=np.uint8)
        o_e = np.zeros(len(docs) + 1, dtype=np.uint64)
        out_e, doo_e = m.replace_batch(c_e, o_e, table)
        assert out_e.size == 0 and doo_e.tolist() == [0] * (len(docs) + 1)
        ct_e, ot_e = _tensors(c_e, o_e)
        got, doo, n, ns, nh, rc = _device(m, table, ct_e, ot_e, len(docs), 0)
        assert (n, ns, nh, rc) == (0, 0, 0, N.AHA_OK) and not doo.any()


def test_replace_refuses_out_overlapping_the_corpus():
    import torch

    m = AC.compile([b"a"])
    table = m.replacements([b"bb"])
    raw = torch.full((256,), ord("a"), dtype=torch.uint8, device="cuda:0")
    ot = torch.tensor([0, 100], dtype=torch.int64, device="cuda:0")
    for lo, hi in ((0, 200), (99, 256), (50, 60)):
        with pytest.raises(AhaError) as e:
            m.replace_batch_device(raw[:100], ot, table, raw[lo:hi])
        assert e.value.code == N.AHA_E_INVALID
    torch.cuda.synchronize()
    assert (raw.cpu().numpy() == ord("a")).all()
    with pytest.raises(AhaError) as e:  # (a sizing call names no range: it is not refused)
        m.replace_batch_device(raw[:100], ot, table, None)
    assert e.value.code == N.AHA_E_CAPACITY and e.value.n_required == 200
    out = torch.zeros(200, dtype=torch.uint8, device="cuda:0")
    assert m.replace_batch_device(raw[:100], ot, table, out) == (200, 100, 100) and (out.cpu().numpy() == ord("b")).all()


def test_replace_in_document_ranges(monkeypatch):
    """the hit buffer's bound lowered: three or more ranges of whole documents, the selection of all of them in one buffer"""
    rng = random.Random(9)
    keys = KEYSETS["ascii"](rng)
    o = orc.AC.compile(keys)
    docs = _ragged_docs(rng, keys) + _ragged_docs(rng, keys) + _ragged_docs(rng, keys)
    docs[7] = b"".join(rng.choice(keys) for _ in range(700))
    corpus, offs = _batch(docs)
    repl = _mixed_table(rng, keys)
    single = AC.compile(keys)
    s_out, s_doo = single.replace_batch(corpus, offs, repl)
    monkeypatch.setenv("AHA_SELECT_HIT_BYTES", str(12 * 100))
    m = AC.compile(keys)
    m.set_profiling(True)
    want, want_doo = _check_all_entries(m, o, corpus, offs, repl)
    table = m.replacements(repl)
    ct, ot = _tensors(corpus, offs)
    got, doo, n, ns, nh, rc = _device(m, table, ct, ot, offs.size - 1, want.size)
    t = m.last_timing()
    assert rc == N.AHA_OK and t["repeats"] >= 2 and t["n_hits"] == nh, t
    assert got.tobytes() == want.tobytes() == s_out.tobytes() and np.array_equal(s_doo, want_doo)
    got, doo, n, _, _, rc = _device(m, table, ct, ot, offs.size - 1, want.size - 1)  # capacity across ranges: nothing written
    assert rc == N.AHA_E_CAPACITY and n == want.size and (got == GUARD8).all() and (doo == GUARD64).all()
    c_out, c_doo, c_ns, c_nh = m.replace_corpus(DeviceCorpus(corpus, offs), table)
    assert c_out.tobytes() == want.tobytes() and np.array_equal(c_doo, want_doo) and (c_ns, c_nh) == (ns, nh)


def test_replace_leaves_no_trace_in_the_back_off(monkeypatch):
    """match -> replace -> match on a handle whose first match is handed back by the prefix-filter engine: every later match
    gives the hits, the engine and the repeats of a twin handle that never saw the call in between."""
    monkeypatch.delenv("AHA_ENGINE", raising=False)
    dense = b"abcd" * 3000
    sparse = b"-" * 5000 + b"abcd"

    def run(with_replace):
        m = AC.compile(["abc", "bcd"])
        assert m.info["filter_prefix_bytes"] == 3
        m.set_profiling(True)
        table = m.replacements(["X", "Y"])
        seen = []
        for text in [dense] + [sparse] * 6 + [dense] + [sparse] * 3:
            hits = m.match_array(text)
            t = m.last_timing()
            seen.append((t["engine"], t["repeats"], hits.tobytes()))
            if with_replace:
                for t2 in (dense, sparse):
                    out, _ = m.replace_batch(t2, np.array([0, len(t2)], dtype=np.uint64), table)
                    assert out.tobytes() == (b"Xd" * 3000 if t2 is dense else b"-" * 5000 + b"Xd")
        m.release_scratch()
        assert m.scratch_bytes() == 0
        return seen

    plain = run(False)
    assert plain[0][0] == 2 and plain[1][0] == 2 and plain[6][0] == 5, [p[:2] for p in plain]
    assert run(True) == plain


def test_replace_scratch_grows_only_and_a_match_behind_it_is_bit_exact():
    rng = random.Random(3)
    keys = KEYSETS["ascii"](rng)
    m, o = AC.compile(keys), orc.AC.compile(keys)
    repl = _mixed_table(rng, keys)
    table = m.replacements(repl)
    seen = []
    for density in (0.2, 0.9, 0.5, 0.9, 0.1):
        corpus, offs = _batch(_ragged_docs(rng, keys, density))
        m.replace_batch(corpus, offs, table)
        seen.append(m.scratch_bytes())
    assert seen == sorted(seen) and seen[0] > 0, seen
    hits, dho = m.match_batch(corpus, offs)
    o_hits, o_dho = o.match_batch(corpus, offs)
    assert np.asarray(hits).tobytes() == o_hits.tobytes() and np.array_equal(np.asarray(dho, dtype=np.uint64), o_dho)
    m.release_scratch()
    assert m.scratch_bytes() == 0
    out, _ = m.replace_batch(corpus, offs, table)  # ... and the call works again from nothing
    assert out.tobytes() == _expect(o, corpus, offs, repl)[0].tobytes()
