"""The passes after the traversal on grids where every lane strides.  Select (scan_select.hip), feed select
(scan_feedselect.hip) and the cover passes (scan_cover.hip) are grid-stride loops -- `i += gridDim.x * 256`, `b += n_waves`,
`d += gridDim.x` -- whose default grid (at least 512 workgroups) gives the suite's inputs one trip.  AHA_POST_BLOCKS (read when
a handle is compiled) caps that grid: 1 workgroup is 256 lanes and 4 waves, 3 workgroups are 768 lanes and 12 waves, an odd
grid whose last trip is partial.  The loops whose grid is a launcher's constant (a workgroup per piece up to 4 096, one
workgroup of 1 024 lanes for a scan) and kv_spans (its grid follows AHA_RESERVE_CUS) take their second trip by size instead.

Every expected value comes from the CPU oracle and the plain sims (selectsim, replacesim, coversim, feedselectsim,
feedreplacesim, feedcoversim, feedgrepsim), bit for bit, with guard words behind every caller buffer (the family files'
helpers, imported).  Every case asserts from its own input that the item counts of the kernels it is there for exceed the
lanes or waves of the grid, and from the oracle's result that what only a later trip writes is not trivial."""
import os
import random
import re
from collections import namedtuple

import numpy as np
import pytest

import coversim
import feedselectsim as fss
import pyoracle as orc
import replacesim
import test_gpu_cover as tcov
import test_gpu_feed_cover as tfcov
import test_gpu_feed_grep as tfgrep
import test_gpu_feed_replace as tfrep
import test_gpu_feed_select as tfsel
import test_gpu_replace as trep
import test_gpu_select as tsel
from aha_amd import AC, synth
from aha_amd import _native as N
from engine_variants import use_variant
from test_gpu_doc_counts import KEYSETS, _batch, _docs, _keys_utf8
from test_gpu_feed import _text as feed_text
from test_gpu_grid_geometry import char_start, plant, v2_chunk

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RANK = 2048  # positions of one rank block: 64 mask words (scan_select.hip kSlBlockWords)
Grid = namedtuple("Grid", "blocks lanes waves")
KNOBS = ("AHA_POST_BLOCKS", "AHA_REPLACE_BLOCKS", "AHA_GREP_BLOCKS", "AHA_CLASS_BLOCKS", "AHA_SELECT_HIT_BYTES", "AHA_RESERVE_CUS",
         "AHA_V2_BPC")

_CACHE = {}


def cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def use_grid(monkeypatch, blocks):
    """the environment of a handle whose post-pass grids have `blocks` workgroups (0: the default grid)"""
    for v in KNOBS:
        monkeypatch.delenv(v, raising=False)
    if blocks:
        monkeypatch.setenv("AHA_POST_BLOCKS", str(blocks))
    return Grid(blocks, 256 * blocks, 4 * blocks)


@pytest.fixture(params=[1, 3], ids=["post1", "post3"])
def grid(request, monkeypatch):
    return use_grid(monkeypatch, request.param)


def source(name):
    return open(os.path.join(ROOT, "aha_amd", "csrc", name)).read()


def rank_blocks(n):
    return ((n + 31) // 32 + 63) // 64


# ---- select ------------------------------------------------------------------------------------------------------------------
SEL_KEYS = [b"a", b"ab", b"abc", b"bc", b"cab", b"bcabca", b"ca", b"xyzzy", b"zy-"]
# document starts on, before and behind mask-word and rank-block edges (24 576 = 12 rank blocks: the edge of three workgroups'
# first trip); empty documents first, inside and last
SEL_CUTS = [0, 0, 31, 32, 33, 64, 65, 300, 2047, 2048, 2049, 2049, 4000, 4095, 4097, 6143, 6144, 8190, 8193, 10240, 10241, 12000,
            12287, 12288, 14000, 17000, 18431, 18432, 18433, 20000, 20480, 22000, 23000, 24575, 24576, 24577, 26000, 26624, 28000,
            28671, 28673, 30000, 30737, 30737]
SEL_RUN_ENDS = [1024, 1055, 1089, 14336, 16383, 22529]  # a run ends on, before and behind a word edge and a rank-block edge


def _sel_text(rng, n, dense):
    """n bytes: letters of the keys throughout (a hit at nearly every position), or bursts of them in a filler without hits"""
    if dense:
        return bytes(rng.choice(b"abc") for _ in range(n))
    out = bytearray()
    while len(out) < n:
        if rng.random() < 0.16:
            out += bytes(rng.choice(b"abc") for _ in range(rng.randint(3, 12)))
        else:
            out += bytes(rng.choice(b"-._ \x00q") for _ in range(rng.randint(2, 9)))
    return bytes(out[:n])


def _abs_starts(sel, dso, offs):
    """the selected hits' first bytes in the batch"""
    doc = np.searchsorted(dso.astype(np.int64), np.arange(sel.size), side="right") - 1
    return offs.astype(np.int64)[doc] + sel["start"].astype(np.int64)


def ragged_batch():
    """about 30 KiB in 43 ragged documents -> (corpus, offs, (selection, its offsets, hits, their offsets))"""
    def make():
        rng = random.Random(30)
        sizes = np.diff(SEL_CUTS).tolist()
        docs = [_sel_text(rng, n, dense=n <= 400) for n in sizes]
        corpus, offs = _batch(docs)
        assert offs.tolist() == SEL_CUTS
        for e in SEL_RUN_ENDS:
            corpus[e - 4:e + 1] = np.frombuffer(b"-abc-", dtype=np.uint8)
        exp = tsel._want(orc.AC.compile(SEL_KEYS), corpus, offs)
        sel, dso, hits, dho = exp
        assert np.diff(dho.astype(np.int64)).max() < 600  # (selectsim.select_doc is quadratic in a document's hits)
        starts = _abs_starts(sel, dso, offs)
        ends = starts + (sel["end"] - sel["start"])
        for e in SEL_RUN_ENDS:  # (from the oracle: a selected hit ends there and none starts there)
            assert e in ends and e not in starts and not any(int(c) - 4 < e <= int(c) for c in offs[1:-1])
        return corpus, offs, exp
    return cached("ragged", make)


def check_select(m, exp, corpus, offs):
    """test_gpu_select's _check_all_entries with the expectation computed once: the device entry twice, then the host entry"""
    want, want_dso, hits, dho = exp
    D = offs.size - 1
    ct, ot = tsel._tensors(corpus, offs)
    rows, dso, n, nh, rc = tsel._device(m, ct, ot, D, want.size + 3)
    assert rc == N.AHA_OK and n == want.size and nh == hits.size
    assert np.array_equal(dso.astype(np.uint64), want_dso) and tsel._as_hits(rows, n).tobytes() == want.tobytes()
    assert (rows[n:] == tsel.GUARD).all(), "the call wrote behind the selection"
    rows2, dso2, n2, _, _ = tsel._device(m, ct, ot, D, want.size + 3)
    assert rows2.tobytes() == rows.tobytes() and dso2.tobytes() == dso.tobytes() and n2 == n
    h_sel, h_dso = m.select_batch(corpus, offs)
    assert h_sel.tobytes() == want.tobytes() and np.array_equal(h_dso, want_dso)


def select_strides(g, corpus, offs, exp, hits=True, positions=True, blocks=True, docs=True):
    """the second-trip assertions of a one-range select call on grid g: what its kernels loop over exceeds the grid, and what
    the later trips alone write is there"""
    sel, dso, all_hits, dho = exp
    nb, nd = int(corpus.size), offs.size - 1
    starts = _abs_starts(sel, dso, offs)
    per_doc = np.diff(dso.astype(np.int64))
    if hits:  # ksl_longest: a lane per hit
        assert all_hits.size > g.lanes and per_doc[dho[:-1].astype(np.int64) >= g.lanes].any()
    if positions:  # ksl_marks, ksl_walk: a lane per position
        assert nb > g.lanes and (starts >= g.lanes).any()
    if blocks:  # ksl_rank_blocks, ksl_emit: a wave per rank block
        assert rank_blocks(nb) > g.waves and (starts // RANK >= g.waves).any()
    if docs:  # ksl_rank_docs: a wave per document
        assert nd > g.waves and per_doc[g.waves:].any() and dso[g.waves:].any()


def test_select_ragged_batch(grid):
    """every select kernel on a second and third trip: more hits and positions than lanes, more rank blocks and documents than
    waves -- at three workgroups too (30 737 positions > 12 x 2 048)"""
    corpus, offs, exp = ragged_batch()
    assert corpus.size > 12 * RANK and offs.size - 1 >= 40
    select_strides(grid, corpus, offs, exp)
    check_select(AC.compile(SEL_KEYS), exp, corpus, offs)


RUN_KEYS = [b"abcdefghabcdefgh", b"efghab", b"ha", b"cd"]


def test_select_runs_through_later_trips(grid):
    """one run of more than 800 covered bytes that starts in the first trip's positions and is walked through those of later
    trips; further runs that start where only a later trip comes by, one at a document start, two that meet at a boundary"""
    def make():
        P = b"abcdefgh"
        joints = (b"efgh", b"h", b"cd", b"efgh", b"h", b"cd", b"")  # (covered by the short keys: the run goes on in another phase)
        run1 = b"".join(P * k + j for k, j in zip((13, 17, 11, 14, 20, 16, 16), joints))
        docs = [b"-" * 100, b"-" * 20 + run1 + b"--", b"-" * 37 + P * 30 + b"-", P * 12 + b"-", b"", P * 6, b"cd" + P * 5, b""]
        corpus, offs = _batch(docs)
        return corpus, offs, tsel._want(orc.AC.compile(RUN_KEYS), corpus, offs)
    corpus, offs, exp = cached("runs", make)
    sel, dso, hits, dho = exp
    assert np.diff(dho.astype(np.int64)).max() < 600
    cover = coversim.byte_cover(hits["start"], hits["end"], offs, dho).astype(np.int8)
    edge = np.zeros(corpus.size + 1, dtype=bool)  # a run begins at a covered byte behind an uncovered one or at a document start
    edge[offs.astype(np.int64)] = True
    begins = np.nonzero(cover & (edge[:-1] | (np.concatenate([[0], cover[:-1]]) == 0)))[0]
    stops = np.nonzero(cover & (edge[1:] | (np.concatenate([cover[1:], [0]]) == 0)))[0] + 1
    runs = list(zip(begins.tolist(), stops.tolist()))
    assert any(a < 256 and b - a >= 800 and b > grid.lanes for a, b in runs), runs  # (256: the first trip of either grid)
    assert sum(1 for a, b in runs if a >= grid.lanes) >= 2 and any(a in offs.tolist() for a, b in runs)
    select_strides(grid, corpus, offs, exp, hits=False, blocks=False, docs=grid.blocks == 1)
    check_select(AC.compile(RUN_KEYS), exp, corpus, offs)


DOC_KEYS = [b"ab", b"abc", b"c", b"bca"]
DOC_FULL = [3, 4, 11, 12, 13, 100, 254, 257, 300, 301, 400, 509, 510, 513, 600, 700, 765, 766, 769, 770, 771, 800, 801, 850, 870,
            880, 890, 893, 894, 895]


def test_select_more_documents_than_lanes(grid):
    """900 documents, 870 of them empty, about 300 bytes: the launch of ksl_marks is sized by the documents, whose loop strides
    there and in ksl_rank_docs; empty documents first, last and in rows across the stride edges (256, 512, 768; every 4 and 12)"""
    def make():
        rng = random.Random(900)
        docs = [b""] * 900
        for d in DOC_FULL:
            docs[d] = bytes(rng.choice(b"abcx") for _ in range(rng.randint(8, 12)))
        corpus, offs = _batch(docs)
        return corpus, offs, tsel._want(orc.AC.compile(DOC_KEYS), corpus, offs)
    corpus, offs, exp = cached("docs900", make)
    sel, dso, hits, dho = exp
    nd = offs.size - 1
    sizes = np.diff(offs.astype(np.int64))
    assert nd == 900 and (sizes == 0).sum() >= 870 and corpus.size < nd  # (the launch: max(nb, nd) lanes)
    assert sizes[:3].sum() == 0 and sizes[-4:].sum() == 0 and all(sizes[e - 1:e + 1].sum() == 0 for e in (256, 512, 768))
    assert nd > grid.lanes and nd > grid.waves
    assert np.diff(dso.astype(np.int64))[grid.lanes:].any()  # documents only a later trip of ksl_marks' document loop visits
    select_strides(grid, corpus, offs, exp, hits=False, positions=grid.blocks == 1, blocks=False)
    check_select(AC.compile(DOC_KEYS), exp, corpus, offs)


def test_select_range_of_whole_rank_blocks_with_empty_documents_last(grid):
    """13 x 2 048 bytes exactly, a hit that ends with the text, six empty documents behind it: ksl_rank_docs takes their rank
    from blk[n_blk], the total"""
    def make():
        rng = random.Random(13)
        cuts = [0, 1000, 2048, 5000, 5001, 9000, 12288, 15000, 18000, 20000, 22000, 24000, 25000, 26000] + [13 * RANK] * 7
        docs = [_sel_text(rng, n, dense=False) for n in np.diff(cuts).tolist()]
        docs[13] = docs[13][:-3] + b"abc"
        corpus, offs = _batch(docs)
        return corpus, offs, tsel._want(orc.AC.compile(SEL_KEYS), corpus, offs)
    corpus, offs, exp = cached("whole-blocks", make)
    sel, dso, hits, dho = exp
    nb = corpus.size
    assert nb % RANK == 0 and rank_blocks(nb) * RANK == nb and (offs[-7:] == nb).all()
    assert sel.size and (dso[-7:] == sel.size).all() and int(_abs_starts(sel, dso, offs)[-1]) + 3 == nb
    select_strides(grid, corpus, offs, exp)
    check_select(AC.compile(SEL_KEYS), exp, corpus, offs)


def test_select_in_document_ranges(grid, monkeypatch):
    """the ragged batch in three and more ranges of whole documents: the offsets carried from range to range (`total`, `base`)
    with kernels that stride inside every range"""
    corpus, offs, exp = ragged_batch()
    sel, dso, hits, dho = exp
    monkeypatch.setenv("AHA_SELECT_HIT_BYTES", str(12 * (hits.size // 3)))
    m = AC.compile(SEL_KEYS)
    m.set_profiling(True)
    check_select(m, exp, corpus, offs)
    ct, ot = tsel._tensors(corpus, offs)
    rows, got_dso, n, nh, rc = tsel._device(m, ct, ot, offs.size - 1, sel.size)
    t = m.last_timing()
    assert rc == N.AHA_OK and tsel._as_hits(rows, n).tobytes() == sel.tobytes() and t["n_hits"] == hits.size
    n_ranges = t["repeats"] + 1
    assert n_ranges >= 3, t
    # at least one range has more hits and positions than the grid has lanes (their mean does), the last ones' hits are selected
    assert hits.size // n_ranges > grid.lanes and corpus.size // n_ranges > grid.lanes
    assert np.diff(dso.astype(np.int64))[-10:].any()


def test_select_rank_scan_takes_two_blocks_per_lane(monkeypatch):
    """ksl_rank_scan is one workgroup of 1 024 lanes, each with `per` consecutive rank blocks: 2 MiB + 4 097 bytes are 1 027
    blocks, so per = 2 (no knob: the grid is a constant).  The filler holds no hit; hits stand around blocks 0, 1, 2, 1 023 to
    1 026 (the last, of one byte)"""
    use_grid(monkeypatch, 0)
    lanes = int(re.search(r"constexpr int kSlScanThreads = (\d+);", source("scan_select.hip")).group(1))
    n = (2 << 20) + 4097
    n_blk = rank_blocks(n)
    assert n_blk > lanes and -(-n_blk // lanes) == 2
    i = np.arange(n, dtype=np.int64)
    corpus = (0x80 | ((7 * i + 13 * (i >> 7)) & 0x7F)).astype(np.uint8)
    planted = [0, 1, 2, lanes - 1, lanes, lanes + 1]
    for b in planted:
        for at in (5, 1000, RANK - 4):  # (the last one crosses into the next block)
            if b * RANK + at + 7 < n:
                corpus[b * RANK + at:b * RANK + at + 7] = np.frombuffer(b"abcabca", dtype=np.uint8)
    corpus[n - 1] = ord("a")
    offs = np.array([0, lanes * RANK - 3, lanes * RANK, n - 1, n, n], dtype=np.uint64)
    o = orc.AC.compile(SEL_KEYS)
    exp = tsel._want(o, corpus, offs)
    sel, dso, hits, dho = exp
    blocks = _abs_starts(sel, dso, offs) // RANK
    # selected hits in odd and even blocks -- both halves of a lane's pair -- and in the last one
    assert hits.size < 600 and set(blocks.tolist()) >= set(planted) | {n_blk - 1}
    check_select(AC.compile(SEL_KEYS), exp, corpus, offs)


def test_replace_on_one_workgroup(monkeypatch):
    """replace over the ragged batch with AHA_POST_BLOCKS=1 and AHA_REPLACE_BLOCKS=1: the select inside and the scan and the copy
    behind it all loop, against replacesim"""
    g = use_grid(monkeypatch, 1)
    monkeypatch.setenv("AHA_REPLACE_BLOCKS", "1")
    corpus, offs, exp_sel = ragged_batch()
    sel, dso, hits, dho = exp_sel
    select_strides(g, corpus, offs, exp_sel)
    repl = trep._mixed_table(random.Random(4), SEL_KEYS)
    want, want_doo = replacesim.replace(corpus, offs, sel, dso, repl)
    assert sel.size > 2 * trep.SCAN_BLOCK and want.size > 16 * 1024 and want.tobytes() != corpus.tobytes()
    exp = (want, want_doo, sel.size, hits.size)
    m = AC.compile(SEL_KEYS)
    table = m.replacements(repl)
    _, _, got, doo = trep._check_device(m, table, None, corpus, offs, repl, exp=exp)
    _, _, got2, doo2 = trep._check_device(m, table, None, corpus, offs, repl, exp=exp)
    assert got2.tobytes() == got.tobytes() and doo2.tobytes() == doo.tobytes()
    h_out, h_doo = m.replace_batch(corpus, offs, table)
    assert h_out.tobytes() == want.tobytes() and np.array_equal(h_doo, want_doo)


# ---- cover -------------------------------------------------------------------------------------------------------------------
def cover_batch():
    """about 40 KiB in 42 documents that are not word-aligned, one above 2 048 bytes -> (keys, corpus, offs, coversim's answer)"""
    def make():
        rng = random.Random(40)
        keys = KEYSETS["ascii"](rng)
        docs = _docs(rng, keys, 40, 1000, 0.5)
        docs.insert(17, b"".join(rng.choice(keys) + b" " for _ in range(500))[:2500])
        docs.append(b"".join(rng.choice(keys) + b"--" for _ in range(700))[:4001])
        corpus, offs = _batch(docs)
        return keys, corpus, offs, tcov._want(orc.AC.compile(keys), corpus, offs)
    return cached("cover", make)


def test_cover_passes_over_the_mask(grid):
    """kv_clear, kv_total, kv_redact and kv_doc_covered on a second and third trip: aligned buffers (16 bytes per lane), a
    corpus view off by 1 and by 8 bytes (byte by byte), in place"""
    keys, corpus, offs, (wm, wr, wc, wn, wh) = cover_batch()
    n, D = corpus.size, offs.size - 1
    sizes = np.diff(offs.astype(np.int64))
    assert wm.size > grid.lanes and n // 16 > grid.lanes and D > grid.waves  # mask words, 16-byte pieces, documents
    assert sizes.max() > 64 * 32 and ((offs[1:-1] % 32) != 0).sum() > D // 2  # a wave's `w += 64` loop; documents inside words
    assert wm[grid.lanes:].any() and wc[grid.waves:].any()
    tail = slice(16 * grid.lanes, None)
    assert (wr[tail] != corpus[tail]).any() and (wr[tail] == corpus[tail]).any()
    m = AC.compile(keys)
    for shift in (0, 1, 8):
        ct, ot = tcov._tensors(corpus, offs, shift)
        assert ct.data_ptr() % 16 == shift
        before = ct.clone()
        dm, dr, dc, nc, nh = tcov._device(m, ct, ot)
        assert (nc, nh) == (wn, wh), shift
        assert dm.tobytes() == wm.tobytes() and dr.tobytes() == wr.tobytes() and np.array_equal(dc, wc), shift
        assert bool((ct == before).all()), "the corpus was changed"
    ct, ot = tcov._tensors(corpus, offs)
    dm, ip, dc, nc, nh = tcov._device(m, ct, ot, in_place=True)
    assert ip.tobytes() == wr.tobytes() and dm.tobytes() == wm.tobytes() and np.array_equal(dc, wc) and (nc, nh) == (wn, wh)


@pytest.mark.parametrize("variant,engine", [("v2", 2), ("u", 4)])
def test_cover_spans_on_later_groups(variant, engine, monkeypatch):
    """kv_spans with more groups of chunks than workgroups (`g += gridDim.x`; the LDS tile cleared per group): one traversal
    workgroup (AHA_RESERVE_CUS = cus - 1), so the spans' grid is 4 and the chunk is the batch over 1 024 lanes; just above 2 MiB
    there are 9 groups from the byte-level engine's records (kSrcRegions) and 16 from the character-level engine's fused ones
    (kSrcUnit).  The longest key ends 1 byte, Lmax - 1 bytes and exactly at every group edge: its span reaches back into the
    tile of the group before, which that group's workgroup flushes with atomicOr."""
    import torch

    use_grid(monkeypatch, 0)
    use_variant(variant, monkeypatch)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    monkeypatch.setenv("AHA_RESERVE_CUS", str(cus - 1))
    grid_cap = 4 * 1  # engine.cpp device_count: the spans run on 4 * v2_grid workgroups
    keys = _keys_utf8(None)
    longest = max(keys, key=len)
    lmax = len(longest)
    n = (2 << 20) + 4097
    S = v2_chunk(n, 1, lmax)
    G = max(1, min(262144 // S, 256))  # scan_cover.hip cover_launch_spans: chunks of a group
    if engine == 4:
        G = max(64, G // 64 * 64)
    n_groups = -(-(-(-n // S)) // G)
    assert n_groups > 2 * grid_cap

    def make():
        blob, koffs, nf = synth.keys(3, K=3000, seed=7)
        text, _ = synth.corpus(3, blob, koffs, nf, n_bytes=n, doc_bytes=1 << 16)
        buf = text.copy()
        for g in range(1, n_groups):
            plant(buf, g * G * S + (1, lmax - 1, 0)[g % 3] - lmax, longest)
        cuts = [char_start(buf, c) for c in range(300_007, n - lmax, 300_007)]
        assert all(min(abs(c - g * G * S) for g in range(n_groups)) > 2 * lmax for c in cuts)  # (no planted key is cut)
        offs = np.array([0] + cuts + [n, n], dtype=np.uint64)
        return buf, offs, tcov._want(orc.AC.compile(keys), buf, offs)
    corpus, offs, (wm, wr, wc, wn, wh) = cached(("spans", G, S), make)
    bits = coversim.unpack(wm, n)
    for g in range(1, n_groups):  # (from the oracle: the planted key is covered up to its last byte, across the edge or up to it)
        e = g * G * S + (1, lmax - 1, 0)[g % 3]
        assert bits[e - lmax:e].all()
    assert wm[grid_cap * G * S // 32:].any()  # what the groups behind the first trip's cover
    m = AC.compile(keys)
    m.set_profiling(True)
    ct, ot = tcov._tensors(corpus, offs)
    dm, dr, dc, nc, nh = tcov._device(m, ct, ot)
    t = m.last_timing()
    assert t["engine"] == engine and t["chunk_bytes"] == S and t["n_hits"] == wh, t
    assert -(-t["n_chunks"] // G) == n_groups > grid_cap
    assert (nc, nh) == (wn, wh) and dm.tobytes() == wm.tobytes() and dr.tobytes() == wr.tobytes() and np.array_equal(dc, wc)


# ---- feeds -------------------------------------------------------------------------------------------------------------------
FEED_LONG = b"abcde" * 20  # W = 99: three pieces have 297 tail entries
FEED_KEYS = [FEED_LONG, b"ab", b"cde", b"bcdea", b"e-"]
FEED_REPL = {0: b"<L>", 1: b"", 2: None, 3: b"a replacement longer than its key", 4: b"\x00E"}


def _feed_filler(rng, n, every):
    """n bytes of a filler without hits with one of the short keys about every `every` bytes"""
    out = bytearray()
    while len(out) < n:
        out += bytes(rng.choice(b"-_. ") for _ in range(rng.randint(1, 2 * every)))
        out += rng.choice([b"ab", b"cde", b"bcdea", b"e-", b"abcde"])
    return bytes(out[:n])


def feed_calls():
    """three sequences in two calls of about 10 KiB each -> [(pieces, ids)] x 2.  Sequence 0 is cut inside the long key (a run
    across the cut), sequence 2 inside a short one; sequence 1 ends its first piece with short hits in its last 41 bytes --
    the tail entries 256 and up of the second call, where it is the third piece -- and no long key near them"""
    def make():
        rng = random.Random(99)
        body = lambda n: _feed_filler(rng, n, 14)  # noqa: E731
        first = [body(1500) + FEED_LONG + body(1800) + FEED_LONG[:37],
                 body(1700) + FEED_LONG + body(1600) + b"--ab-cde-ab--cde-ab-bcdea-ab",
                 body(3300) + FEED_LONG + b"--bcd"]
        second = [FEED_LONG[37:] + body(1900) + FEED_LONG + body(1400),
                  b"--" + body(1800) + FEED_LONG + body(1500) + b"-ab-cde-",
                  b"ea-" + body(3400)]
        return [(first, [0, 1, 2]), ([second[0], second[2], second[1]], [0, 2, 1])]
    return cached("feed-calls", make)


def feed_strides(rig, calls, g, reported):
    """the second call on grid g: its extended positions, rank blocks, true hits and tail entries exceed the grid, and what
    `reported` (the model's hits of the call, per piece) holds from the later trips is there"""
    W = rig.W
    (first, ids1), (second, ids2) = calls
    n0 = [len(first[ids1.index(q)]) for q in ids2]
    assert W == 99 and min(n0) >= W
    eoff = np.cumsum([0] + [W + len(p) for p in second])
    NE, D = int(eoff[-1]), len(second)
    true = [sum(1 for h in rig.match(first[ids1.index(q)] + p) if h[1] > n) for q, p, n in zip(ids2, second, n0)]
    assert NE > 8192 and rank_blocks(NE) > g.waves and D * W > g.lanes and sum(true) > g.lanes
    # kfs_longest: hits behind the first trip's are selected
    assert sum(true[:-1]) >= g.lanes and any(h[1] > 0 for h in reported[-1])
    # kfs_tail: entry i = d * W + j stands for byte j - W of piece d; the entries behind the first trip's are piece 2's last
    lo = g.lanes - (D - 1) * W - W
    assert lo < 0 and any(lo <= h[0] and h[1] <= 0 for h in reported[-1]), (lo, reported[-1][:5])
    # kfs_walk, kfs_emit: selected hits in rank blocks behind the first trip's; a run across the cut
    assert any((int(eoff[d]) + W + h[0]) // RANK >= g.waves for d in range(D) for h in reported[d])
    assert any(h[0] < 0 < h[1] and h[2] == 0 for h in reported[0])


def _per_piece(hits, pso):
    return [hits[int(pso[d]):int(pso[d + 1])].tolist() for d in range(pso.size - 1)]


def test_feed_select_on_one_workgroup(monkeypatch):
    g = use_grid(monkeypatch, 1)
    calls = feed_calls()
    r = tfsel.Rig(FEED_KEYS, n_seqs=3)
    for pieces, ids in calls:
        hits, _ = tfsel.step(r, pieces, ids, device=True)
        assert hits.size > 100
    feed_strides(r, calls, g, _reported_select(calls))
    tfsel.finish_and_compare(r, device=True)


def _reported_select(calls):
    """feedselectsim's hits of the second call, per piece (a model of its own: the rig's has moved on)"""
    def make():
        rig_match = fss.oracle_match(orc.AC.compile(FEED_KEYS))
        model = fss.Feed(rig_match, fss.window(FEED_KEYS), 3)
        model.call(*calls[0])
        hits, pso, _, _ = model.call(*calls[1])
        return _per_piece(hits, pso)
    return cached("feed-reported", make)


def test_feed_replace_on_one_workgroup(monkeypatch):
    g = use_grid(monkeypatch, 1)
    calls = feed_calls()
    r = tfrep.Rig(FEED_KEYS, FEED_REPL, n_seqs=3)
    for pieces, ids in calls:
        out, _ = tfrep.step(r, pieces, ids, device=True)
        assert len(out) > 8192 and out != b"".join(pieces)
    feed_strides(r, calls, g, _reported_select(calls))
    tfrep.finish_and_compare(r, device=True)


def test_feed_cover_on_one_workgroup(monkeypatch):
    """four sequences, two calls of about 12 KiB: kv_total strides over the call's mask words (the pieces' covered bytes, the
    redacted copy and the mask are the feed's own passes)"""
    g = use_grid(monkeypatch, 1)
    rng = random.Random(12)
    keys = tfcov._keys16(rng)
    m, o = AC.compile(keys), orc.AC.compile(keys)
    texts = [feed_text(rng, keys, 6000 + 7 * s) for s in range(4)]
    wholes = [tfcov._whole(o, t) for t in texts]
    f = m.feed(4)
    pos = [0] * 4
    for ids, cut in (([2, 0, 3, 1], 3001), ([1, 3, 2, 0], 7000)):
        pieces = [texts[s][pos[s]:cut] for s in ids]
        want = tfcov._want_call(wholes, texts, pos, pieces, ids)
        n_words = (sum(len(p) for p in pieces) + 31) // 32
        first_trip = int(np.unpackbits(want["mask"][:g.lanes].view(np.uint8)).sum())  # covered bytes in the words one trip takes
        assert n_words > g.lanes and want["mask"][g.lanes:].any() and want["nc"] > first_trip
        tfcov._assert_call(tfcov._cover_call(f, pieces, ids, use_device=True), want)
        for d, s in enumerate(ids):
            pos[s] += len(pieces[d])
    assert any(want["back"])  # (the second call's windows reach back across the cut)
    f.close()


def piece_caps():
    """the launchers' fixed grids: a workgroup per piece (kfs_commit, kfg_windows), a lane per run of pieces in the one-workgroup
    scans (kfs_layout, kfr_layout, kfg_layout)"""
    sel, rep, grp = source("scan_feedselect.hip"), source("scan_feedreplace.hip"), source("scan_feedgrep.hip")
    per_piece = [int(re.search(r"%s, dim3\(grid_for\(F\.D, 1, (\d+)\)\)" % k, s).group(1))
                 for k, s in (("kfs_commit", sel), ("kfg_windows", grp))]
    scans = [int(re.search(r"constexpr int %s = (\d+);" % k, s).group(1))
             for k, s in (("kFsScanThreads", sel), ("kFrScanThreads", rep), ("kFgScanThreads", grp))]
    return max(per_piece), max(scans)


def many_pieces():
    """more pieces than workgroups a launcher starts, of 1 to 4 bytes and as many sequences, in two calls"""
    def make():
        cap, scan = piece_caps()
        D = cap + 37
        assert D > cap and D > 2 * scan  # a second trip per workgroup; `per` > 1 in the scans
        rng = random.Random(41)
        word = b"abcabcabbbbcabcabxab"
        starts = [rng.randrange(len(word) - 8) for _ in range(D)]
        first = [word[a:a + rng.choice([1, 2, 3, 4])] for a in starts]
        second = [word[a + len(p):a + len(p) + rng.choice([1, 2, 3, 4])] for a, p in zip(starts, first)]
        return cap, D, first, second
    return cached("many-pieces", make)


def test_feed_select_more_pieces_than_workgroups(monkeypatch):
    use_grid(monkeypatch, 0)
    cap, D, first, second = many_pieces()
    r = tfsel.Rig(tfrep.KEYS, n_seqs=D)
    ids = list(range(D))
    tfsel.step(r, first, ids, device=True)
    want, wpso, _, whold = r.model.call(second, ids)  # (the model once: step() would ask it again)
    rc, hits, pso, bases, hold, ns, nh, _ = tfsel._raw(r.feed, second, ids, cap=want.size + 3, device=True)
    assert rc == N.AHA_OK and ns == want.size and hits.tobytes() == want.tobytes()
    assert np.array_equal(pso, wpso) and np.array_equal(hold, whold) and np.array_equal(bases, [len(p) for p in first])
    late = want[int(wpso[cap]):]
    assert (late["start"] < 0).any() and whold[cap:].any()  # pieces of the second trip: hits across the cut, bytes held back
    # FINAL with empty pieces: what is still open, against the model
    want, wpso, _, whold = r.model.call([b""] * D, ids, True)
    rc, hits, pso, _, hold, ns, _, _ = tfsel._raw(r.feed, [b""] * D, ids, final=True, cap=want.size + 3, device=True)
    assert rc == N.AHA_OK and hits.tobytes() == want.tobytes() and np.array_equal(pso, wpso) and not hold.any()
    assert np.diff(wpso.astype(np.int64))[cap:].any() and r.feed.position(D - 1) == (0, 0)


def test_feed_replace_more_pieces_than_workgroups(monkeypatch):
    use_grid(monkeypatch, 0)
    cap, D, first, second = many_pieces()
    r = tfrep.Rig(tfrep.KEYS, tfrep.REPL, n_seqs=D)
    ids = list(range(D))
    tfrep.step(r, first, ids, device=True)
    want = r.model.call(second, ids, r.repl, False)
    wout, wpoo, wbases, whold, wsel = want
    assert whold[cap:].any() and (np.diff(wpoo.astype(np.int64))[cap:] != [len(p) for p in second[cap:]]).any()
    tfrep.step(r, second, ids, device=True, want=want)
    out, hold = tfrep.step(r, [b""] * D, ids, final=True, device=True)
    assert not hold.any() and r.feed.position(D - 1) == (0, 0)
    assert b"".join(r.said[q] for q in ids[cap:]) != b"".join(r.whole[q] for q in ids[cap:])


def test_feed_grep_more_pieces_than_workgroups(monkeypatch):
    use_grid(monkeypatch, 0)
    cap, D = many_pieces()[:2]
    rng = random.Random(43)
    first = [rng.choice([b"a", b"xa", b"b", b"bc", b"\n", b"x", b"ab"]) for _ in range(D)]
    second = [rng.choice([b"b\n", b"b", b"ca\n", b"a\n", b"\n", b"c", b"x\nab"]) for _ in range(D)]
    p = tfgrep.Pair([b"ab", b"bca"], D)
    ids = list(range(D))
    p.step(first, ids)
    kept, out, roo, info = p.step(second, ids, hits=True)
    # pieces of the second trip whose record is kept for a hit across the cut alone: neither side holds one
    across = [d for d in range(cap, D) if info["piece_head"][d] and not p.count(first[d]) and not p.count(second[d])]
    assert across and np.diff(info["piece_kept_offsets"].astype(np.int64))[cap:].any()
    p.step([b""] * D, ids, final=True)
    assert p.feed.position(D - 1) == (0, 0)
