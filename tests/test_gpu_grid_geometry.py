"""GPU parity on reduced persistent grids: every traversal kernel here loops over tiles, chunks or groups (`tile +=
gridDim.x`, `chunk += nw`, `g += gridDim.x`), and the state it carries from one trip to the next -- kf_walk's prefetch of
the next chunk, the per-tile setup of ku_traverse / k2_traverse / ks_traverse, ku_expand_groups' uend cache and s_tot
double buffer, the waves of kp_pairs and ks_mark with several tiles -- only runs on a second trip.  On the full device
the suite's inputs give most of these loops one trip.  Handles compiled with AHA_RESERVE_CUS (and AHA_V2_BPC) get a
smaller grid (engine.cpp, v2_setup / plan_engine), so test-sized inputs take the second trips.

Every case compares the HIP path with the CPU oracle bit for bit (hit triples in order, per-document hit offsets) and
asserts from last_timing() that the call reached the geometry it exists for."""
import random
from collections import namedtuple

import numpy as np
import pytest

import pyoracle as orc
from aha_amd import AC, BitArray, synth
from engine_variants import use_variant

pytestmark = pytest.mark.gpu

THREADS = 1024      # kV2Threads: lanes (and chunks) of one traversal tile
MAX_S = 32768       # kV2MaxS: the chunk cap, the exact width of the 15-bit `rel` and 16-bit `seq` fields (image.hpp)
TILE = THREADS * MAX_S  # bytes of one traversal tile at the chunk cap: 32 MiB
PAIR_TILE = 2048    # kp_pairs: a wave's tile = a chunk of the event regions
SK_PIECE = 64       # ks_mark: bytes per lane; a wave's tile is 64 pieces

Geo = namedtuple("Geo", "name cus grid pf_cus bpc")


@pytest.fixture
def geometry(request, monkeypatch):
    """g1: AHA_RESERVE_CUS = cus - 1, a traversal grid of one workgroup (16 waves).  g3: cus - 3, an odd grid.  ship: 16,
    what bench.py sets for --gpus N > 1.  bpc2: AHA_V2_BPC=2, two workgroups per CU with half the LDS prefix (the
    character-level engines are not built under it).  Read when a handle is compiled."""
    import torch

    cus = torch.cuda.get_device_properties(0).multi_processor_count
    reserve = {"g1": cus - 1, "g3": cus - 3, "ship": 16, "bpc2": 0}[request.param]
    bpc = 2 if request.param == "bpc2" else 1
    assert 0 <= reserve < cus
    if reserve:
        monkeypatch.setenv("AHA_RESERVE_CUS", str(reserve))
    else:
        monkeypatch.delenv("AHA_RESERVE_CUS", raising=False)
    if bpc == 2:
        monkeypatch.setenv("AHA_V2_BPC", "2")
    else:
        monkeypatch.delenv("AHA_V2_BPC", raising=False)
    for v in ("AHA_FILTER_CHUNK", "AHA_EXPAND_BLOCKS", "AHA_GROUP_RCCL", "AHA_PAIR", "AHA_SKIP", "AHA_DIRECT"):
        monkeypatch.delenv(v, raising=False)
    return Geo(request.param, cus, (cus - reserve) * bpc, cus - reserve, bpc)


@pytest.fixture
def engine(request, monkeypatch):
    """One of test_gpu_parity.py's engine variants but v1 (the two-pass engine's grid does not follow v2_grid)."""
    return use_variant(request.param, monkeypatch)


def grids(geos, engines):
    """Parametrize a test over the geometries x engine variants it runs: the two fixtures above take their part of each id."""
    return pytest.mark.parametrize("geometry,engine", [(g, e) for g in geos for e in engines], indirect=True)


# ---- the planner's arithmetic (engine.cpp plan_v2) ----------------------------------------------------------------

def v2_chunk(n, grid, lmax):
    """The chunk of the byte-level, character-level and skip-ahead traversals: the batch over grid * 1024 lanes, rounded
    up to 64, at least 8 * Lmax, at most kV2MaxS."""
    lanes = grid * THREADS
    s = (-(-n // lanes) + 63) // 64 * 64
    return min(max(s, 64, (8 * lmax + 63) // 64 * 64), MAX_S)


def filter_image_in_lds(n_slots, s, chars):  # scan_filter.hip: kf_wave_lds, kfLdsBudget
    w = s // 4096
    wave = 256 * w * 2 + 64 * 4 + 64 * 4 * 8 + (w * 64 * 10 if chars else 0)
    return n_slots * 4 + 16 * wave <= 160 << 10


def filter_waves(n_slots, s, chars, n_chunks, pf_cus):
    """Waves of kf_walk's launch (filter_launch_walk): 16 per block with the image in LDS, else 4."""
    if filter_image_in_lds(n_slots, s, chars):
        return 16 * max(1, min(-(-n_chunks // 16), pf_cus))
    return 4 * max(1, min(-(-n_chunks // 4), 5 * pf_cus))


def want_engines(engine, geo, chars=False, sep=False):
    """Engines that may answer a call over a cfg 3-like key set (a character-level image, skip / pair eligible, no prefix
    filter): 2 byte-level, 4 character-level, 6 skip-ahead, 7 pair (4 after a hand-back)."""
    if sep or geo.bpc == 2 or engine in ("v2", "v2p", "f"):
        return (2,)
    if engine == "k":
        return (4,) if chars else (6,)
    if engine == "p":
        return (4,) if chars else (7, 4)
    return (4,)


# ---- data and the oracle, cached at module scope (the oracle is single-threaded, ~0.1 GB/s) ---------------------

_DATA = {}
_ORACLE = {}


def cached(store, key, make):
    if key not in store:
        store[key] = make()
    return store[key]


def plant(buf, at, piece):
    """Write `piece` at byte `at` of a UTF-8 buffer, blanking the parts of characters it cuts so the text stays valid."""
    a = at
    while a > 0 and (buf[a] & 0xC0) == 0x80:
        a -= 1
    buf[a:at] = 32
    buf[at:at + len(piece)] = np.frombuffer(piece, dtype=np.uint8)
    e = at + len(piece)
    while e < buf.size and (buf[e] & 0xC0) == 0x80:
        buf[e] = 32
        e += 1


def char_start(buf, c):
    while c < buf.size and (buf[c] & 0xC0) == 0x80:
        c += 1
    return c


def with_key(blob, offs, key):
    return np.concatenate([blob, np.frombuffer(key, dtype=np.uint8)]), np.append(offs, offs[-1] + len(key)).astype(np.uint64)


def oracle_batch(name, keys, corpus, doc, chars=False):
    def make():
        o = cached(_ORACLE, ("handle",) + keys[:1], lambda: orc.AC.compile_packed(*keys[1:]))
        oh, od = o.match_batch(corpus, doc, chars=chars, cap=max(1024, corpus.size // 4))
        return oh.tobytes(), np.asarray(od, dtype=np.uint64), len(oh)
    return cached(_ORACLE, (name, chars), make)


def oracle_sep(name, keys, corpus, doc, bits):
    """Per document, the String overload with a separator filter (src/aha/ac.cr:176-192): hits in document offsets."""
    def make():
        o = cached(_ORACLE, ("handle",) + keys[:1], lambda: orc.AC.compile_packed(*keys[1:]))
        parts, dho = [], [0]
        for d in range(doc.size - 1):
            h = o.match(corpus[int(doc[d]):int(doc[d + 1])].tobytes(), chars=False, sep=(256, bits))
            parts.append(h.tobytes())
            dho.append(dho[-1] + len(h))
        return b"".join(parts), np.asarray(dho, dtype=np.uint64), dho[-1]
    return cached(_ORACLE, (name, "sep"), make)


def run_device(g, corpus, doc, cap, chars=False, sep=None):
    """match_batch_device into an output of exactly `cap` rows and per-document offsets, with guards behind both: nothing
    may be written past them.  Returns (n, hit bytes, doc hit offsets)."""
    import torch

    dc = torch.from_numpy(corpus).cuda()
    dd = torch.from_numpy(doc.astype(np.int64)).cuda()
    big = torch.full((cap + 64, 3), -7, dtype=torch.int32, device="cuda")
    dho = torch.full((doc.size + 8,), -7, dtype=torch.int64, device="cuda")
    n = g.match_batch_device(dc, dd, big[:cap], dho[:doc.size], sep=sep, chars=chars)
    assert bool((big[cap:] == -7).all()) and bool((dho[doc.size:] == -7).all())
    return n, big[:n].cpu().numpy().tobytes(), dho[:doc.size].cpu().numpy().astype(np.uint64)


def check_device(g, corpus, doc, want, cap=None, chars=False, sep=None):
    raw, od, total = want
    n, got, dho = run_device(g, corpus, doc, total if cap is None else cap, chars=chars, sep=sep)
    assert n == total and got == raw, (n, total, chars, sep is not None)
    assert np.array_equal(dho, od)
    t = g.last_timing()
    assert t["n_hits"] == total
    return t


def compile_profiled(keys):
    g = AC.compile_packed(*keys[1:])
    g.set_profiling(True)
    return g


# ---- 1. a second tile per traversal workgroup, at the chunk cap ----------------------------------------------------

EDGE_KEY = b"<tile-edge-key>"  # an ASCII key planted across the tile edge (every cut near it falls on a character start)


def cap_keys():
    def make():
        blob, offs, nf = synth.keys(3, K=20_000)
        return ("cfg3+edge",) + with_key(blob, offs, EDGE_KEY) + (nf,)
    return cached(_DATA, "cap_keys", make)[:3]


def cap_corpus():
    """33 MiB + 12 345 bytes of cfg 3 text: on one workgroup the chunk is the cap, 1 057 chunks, a second tile of 33 chunks
    (not a multiple of 64).  Layout A cuts documents at the tile edge (T - 1, T, T + 1) and at chunk edges, with empty
    documents; layout B leaves one document across the tile edge, where the planted key straddles it."""
    def make():
        blob, offs, nf = synth.keys(3, K=20_000)
        n = TILE + (1 << 20) + 12_345
        corpus, doc = synth.corpus(3, blob, offs, nf, n_bytes=n, doc_bytes=1 << 20)
        buf = corpus.copy()
        edges = [MAX_S * k for k in (1, 2, 511, 1023, 1025, 1031)]
        for e in edges:
            plant(buf, e - 1, b"  ")
        plant(buf, TILE - 7, EDGE_KEY)
        cuts = [char_start(buf, int(c)) for c in doc[1:-1]]
        a = sorted(cuts + edges + [TILE - 1, TILE, TILE, TILE + 1] + [0, 0, n, n])
        b = sorted([c for c in cuts + edges if c < TILE - (1 << 20)] + [0, n, n])
        for lay in (a, b):
            assert lay[0] == 0 and lay[-1] == n and all(c == n or (buf[c] & 0xC0) != 0x80 for c in lay)
        assert sum(1 for c in b if TILE - (1 << 20) <= c < n) == 0 and bytes(buf[TILE - 7:TILE + 8]) == EDGE_KEY
        return buf, np.array(a, dtype=np.uint64), np.array(b, dtype=np.uint64)
    return cached(_DATA, "cap_corpus", make)


SEP_BITS = [32] + list(range(0x80, 0x100))  # spaces and every non-ASCII byte: keys between characters stay hits


@grids(("g1",), ("v2", "v2p", "u", "uh", "u23", "k", "auto"))
def test_second_tile_per_traversal_workgroup_at_the_chunk_cap(geometry, engine):
    """One traversal workgroup (g1) over 33 MiB + an odd tail: S = kV2MaxS = 32 768 -- never reached on the full grid
    below 8 GiB -- and 1 057 chunks, so workgroup 0 runs tile 0 and then, on its second trip round `tile += gridDim.x`,
    the partial tile 1 (ku_traverse, k2_traverse, ks_traverse: the per-tile setup and wave event buffers).  Byte offsets
    in two document layouts, char offsets, and a separator call (k2_traverse's slab pipeline on every engine)."""
    keys = cap_keys()
    corpus, doc_a, doc_b = cap_corpus()
    g = compile_profiled(keys)
    lmax = g.info["max_key_len"]
    assert v2_chunk(corpus.size, geometry.grid, lmax) == MAX_S

    def geo_ok(t, want):
        assert t["engine"] in want, (t["engine"], want)
        assert t["chunk_bytes"] == MAX_S and t["n_chunks"] == -(-corpus.size // MAX_S)
        assert t["n_chunks"] > THREADS * geometry.grid and t["n_chunks"] % 64 != 0  # a second, partial tile

    for name, doc in (("cap-a", doc_a), ("cap-b", doc_b)):
        t = check_device(g, corpus, doc, oracle_batch(name, keys, corpus, doc))
        geo_ok(t, want_engines(engine, geometry))
    t = check_device(g, corpus, doc_a, oracle_batch("cap-a", keys, corpus, doc_a, chars=True), chars=True)
    geo_ok(t, want_engines(engine, geometry, chars=True))
    sep = BitArray(256)
    for b in SEP_BITS:
        sep[b] = True
    # (room for every hit before the separator test: the slab pipeline's event temp is sized from the capacity, and a call
    # with more events than that goes to the two-pass engine)
    want_b = oracle_batch("cap-b", keys, corpus, doc_b)
    t = check_device(g, corpus, doc_b, oracle_sep("cap-b", keys, corpus, doc_b, SEP_BITS), cap=2 * want_b[2], sep=sep)
    geo_ok(t, (2,))
    # the planted key across the tile edge is a hit of layout B's spanning document (and cut by layout A's boundaries)
    edge = np.frombuffer(want_b[0], dtype=orc.HIT_DTYPE)
    edge_id = keys[2].size - 2
    d_span = int(np.searchsorted(doc_b, TILE, side="right")) - 1
    assert sum(1 for h in edge.tolist() if h[2] == edge_id) == 1 and int(doc_b[d_span]) < TILE < int(doc_b[d_span + 1])


@grids(("g3",), ("u", "v2"))
def test_one_workgroup_of_an_odd_grid_takes_two_tiles(geometry, engine):
    """Three traversal workgroups (g3) over 3 tiles + 4 097 bytes at the chunk cap: 3 073 chunks, 4 tiles -- workgroup 0
    takes tiles 0 and 3, the others one each."""
    def make():
        blob, offs, nf = synth.keys(3, K=20_000)
        n = 3 * TILE + 4097
        return synth.corpus(3, blob, offs, nf, n_bytes=n, doc_bytes=4 << 20)
    corpus, doc = cached(_DATA, "three_tiles", make)
    keys = cap_keys()
    g = compile_profiled(keys)
    t = check_device(g, corpus, doc, oracle_batch("three-tiles", keys, corpus, doc))
    assert t["engine"] == (4 if engine == "u" else 2) and t["chunk_bytes"] == MAX_S
    n_tiles = -(-t["n_chunks"] // THREADS)
    assert geometry.grid == 3 and n_tiles == 4 and n_tiles % geometry.grid == 1


# ---- 2. the chunk cap's bit fields ---------------------------------------------------------------------------------

@grids(("g1",), ("v2", "v2p", "u", "uh", "u23", "auto"))
def test_an_event_at_every_byte_of_a_capped_chunk(geometry, engine):
    """A one-byte key and keys nested on it over a run of it longer than three chunks: chunks of 32 768 bytes with an
    event at every byte, the largest `rel` (15 bits) and `seq` (16 bits) of an event record (p_y = (seq << 16) | last |
    rel).  A dense capacity (full-size regions, k2d_expand_dense) and an exact one, whose regions overflow on the run:
    the call is repeated once with full-size regions (repeats == 1) and still matches."""

    def make():
        n = TILE + (1 << 20) + 777
        buf = np.full(n, ord("b"), dtype=np.uint8)
        run_at = MAX_S * 500 - 100
        buf[run_at:run_at + 3 * MAX_S + 200] = ord("a")
        blob, offs = orc.pack_keys([b"a", b"aa", b"aaa", b"aaaa"])
        return buf, np.array([0, 12_345_677, n], dtype=np.uint64), ("nested-a", blob, np.asarray(offs, dtype=np.uint64))
    corpus, doc, keys = cached(_DATA, "run_of_a", make)
    want = oracle_batch("run-of-a", keys, corpus, doc)
    assert want[2] > 4 * 3 * MAX_S
    g = compile_profiled(keys)
    e = 4 if engine in ("u", "uh", "u23") else 2
    for cap, repeats in ((corpus.size // 4 + 64, 0), (want[2], 1)):
        t = check_device(g, corpus, doc, want, cap=cap)
        assert t["engine"] == e and t["repeats"] == repeats, (cap, t)
        assert t["chunk_bytes"] == MAX_S and t["n_chunks"] > THREADS * geometry.grid


# ---- 3. several chunks per filter wave -----------------------------------------------------------------------------

def filter_data(image, utf8):
    """A keyword list (cfg 2: keys of 4 to 16 bytes, no character-level image) whose image fits LDS (1 000 keys) or does
    not (4 000 keys: n_slots * 4 > 160 KiB), over 4 MiB + 333 bytes of its text.  At every 4 KiB edge a longest key
    starts 1, 2, 3, 7 or 15 bytes before it (in the warm bytes of every chunk size) and a NUL byte stands in front of a
    key.  Documents start exactly at chunk edges: at every odd multiple of 32 KiB (an edge for every chunk size: the
    boundary cuts the key planted across it) and at every third 4 KiB edge between them, with empty documents at one
    such edge; the other edges keep their keys whole.  utf8: the same text
    with runs of 2-, 3- and 4-byte characters between its words (kf_walk counts a chunk's continuation bytes)."""
    def make():
        blob, offs, nf = synth.keys(2, K=1000 if image == "lds" else 4000)
        corpus, doc = synth.corpus(2, blob, offs, nf, n_bytes=(4 << 20) + 333, doc_bytes=1 << 16)
        keys = [bytes(blob[offs[i]:offs[i + 1]]) for i in range(offs.size - 1)]
        longest, short = max(keys, key=len), min(keys, key=len)
        rng = random.Random(33)
        raw = corpus.tobytes()
        if utf8:
            parts, at = [], 0
            while at < len(raw):
                nxt = raw.find(b" ", at + rng.randint(50, 400))
                nxt = len(raw) if nxt < 0 else nxt
                parts.append(raw[at:nxt])
                parts.append(b" " + (rng.choice(["é", "月", "😁", "я"]) * rng.randint(1, 8)).encode())
                at = nxt
            raw = b"".join(parts)
        buf = np.frombuffer(raw, dtype=np.uint8).copy()
        n = buf.size
        cuts = [char_start(buf, int(c)) for c in doc[1:-1] if c < n]
        edges = []
        for k, e in enumerate(range(4096, n - 200, 4096)):
            plant(buf, e - (1, 2, 3, 7, 15)[k % 5], longest)
            plant(buf, e + 100, b"\x00" + short)
            if (e % MAX_S == 0 and e // MAX_S % 2 == 1) or (e % MAX_S != 0 and k % 3 == 2):
                edges.append(e)
        assert all((buf[e] & 0xC0) != 0x80 for e in edges)  # (inside a planted ASCII key: a character start)
        assert sum(1 for e in edges if e % MAX_S == 0) >= 60 and sum(1 for e in edges if e % 8192 == 4096) >= 100
        cuts = sorted(set(cuts + edges) | {char_start(buf, MAX_S * 5 + 3000)}) + [MAX_S * 9] * 2
        docs = np.array(sorted([0, 0] + cuts + [n, n]), dtype=np.uint64)
        return buf, docs, ("cfg2-%s" % image, blob, offs)
    return cached(_DATA, ("filter", image, utf8), make)


@pytest.mark.parametrize("chunk", [None, "4096", "8192", "16384", "32768"])
@pytest.mark.parametrize("image", ["lds", "hbm"])
@grids(("g1", "g3"), ("f", "auto"))
def test_filter_waves_take_several_chunks(geometry, engine, monkeypatch, image, chunk):
    """The prefix-filter engine (scan_filter.hip) on one and on three CUs: kf_walk<true, ..> (16 waves, the image in LDS)
    or kf_walk<false, ..> (5 x 4 waves per CU), each wave with several chunks -- the prefetch of the next chunk's bitmap
    words and record (nm / nrec) runs on every trip after the first.  Every chunk size, forced like
    test_prefix_filter_engine_edges does."""
    if chunk:
        monkeypatch.setenv("AHA_FILTER_CHUNK", chunk)
    g = compile_profiled(filter_data(image, False)[2])
    n_slots = g.info["n_slots"]
    assert g.info["filter_prefix_bytes"] > 0 and (n_slots * 4 <= 160 << 10) == (image == "lds")
    for text_utf8, chars in ((False, False), (True, True), (True, False)):
        corpus, doc, keys = filter_data(image, text_utf8)
        gh, gd = g.match_batch(corpus, doc, chars=chars)
        raw, od, total = oracle_batch("filter-%s-%s" % (image, text_utf8), keys, corpus, doc, chars=chars)
        assert len(gh) == total and np.asarray(gh).tobytes() == raw and np.array_equal(np.asarray(gd, dtype=np.uint64), od)
        t = g.last_timing()
        assert t["engine"] == 5, (chars, t)
        s = t["chunk_bytes"]
        assert s == int(chunk) if chunk else s in (4096, 8192, 16384, 32768)
        if image == "hbm":
            assert not filter_image_in_lds(n_slots, s, chars)
        elif not chars:
            assert filter_image_in_lds(n_slots, s, chars)
        assert t["n_chunks"] == -(-corpus.size // s)
        assert t["n_chunks"] > filter_waves(n_slots, s, chars, t["n_chunks"], geometry.pf_cus)  # a wave takes a second chunk


# ---- 4. pair and skip engines with few waves -----------------------------------------------------------------------

@pytest.mark.parametrize("geometry,engine,n_bytes",
                         [(g, e, n) for g, grid in (("g1", 1), ("g3", 3)) for e in ("p", "k")
                          for n in ((64 << 10) + 5, (1 << 20) + 77, (3 << 20) + 1) if n // PAIR_TILE > 16 * grid],
                         indirect=["geometry", "engine"])
def test_pair_and_skip_waves_take_several_tiles(geometry, engine, n_bytes):
    """kp_pairs (a wave per 2 KiB tile, `tile += n_waves`) and ks_mark (a wave per 64 pieces of 64 bytes) on 16 or 48
    waves, so every wave takes several tiles.  First a batch of 16 KiB documents, which the pair engine keeps on a fresh
    handle: its multi-tile output is what the oracle sees (engine 7 asserted).  Then the same text with empty documents
    (two boundaries in one 32-byte piece): the pair engine may hand that batch back to engine 4, and either answer must
    match.  (After three hand-backs a handle stops trying the pair engine -- pair_off --, so only the first call of a
    handle can be expected to reach it.)"""
    waves = 16 * geometry.grid
    assert n_bytes // PAIR_TILE > waves

    def make():
        blob, offs, nf = synth.keys(3, K=20_000)
        corpus, doc = synth.corpus(3, blob, offs, nf, n_bytes=n_bytes, doc_bytes=16 << 10)
        empty = np.array(sorted(doc.tolist() + [0, int(doc[doc.size // 2])] + [n_bytes]), dtype=np.uint64)
        return corpus, doc, empty
    corpus, doc, empty = cached(_DATA, ("pair", n_bytes), make)
    keys = cap_keys()
    g = compile_profiled(keys)
    for name, d, allowed in (("plain", doc, (7,)), ("empty", empty, (7, 4))):
        gh, gd = g.match_batch(corpus, d)
        raw, od, total = oracle_batch("pair-%s-%d" % (name, n_bytes), keys, corpus, d)
        assert len(gh) == total and np.asarray(gh).tobytes() == raw and np.array_equal(np.asarray(gd, dtype=np.uint64), od)
        t = g.last_timing()
        if engine == "k":
            assert t["engine"] == 6
            assert (-(-n_bytes // SK_PIECE) + 4 + 63) // 64 > waves  # ks_mark: tiles of 64 pieces, a second per wave
            assert t["chunk_bytes"] == v2_chunk(n_bytes, geometry.grid, g.info["max_key_len"])
        else:
            assert t["engine"] in allowed, (name, t["engine"])
            if t["engine"] == 7:
                assert t["chunk_bytes"] == PAIR_TILE and t["n_chunks"] == -(-n_bytes // PAIR_TILE) and t["n_chunks"] > waves


# ---- 5. multi-group and multi-chunk expansion ----------------------------------------------------------------------

@grids(("g1",), ("u", "ur", "u23"))
def test_expansion_workgroups_take_several_groups(geometry, engine):
    """ku_expand_groups runs on min(n_groups, 2 * v2_grid) workgroups: on one CU two workgroups take the 16 groups of 64
    chunks of a 4 MiB batch in turn, keeping their LDS cache of uend entries and the s_tot[par] double buffer across
    groups.  "ur" takes the general passes instead: ku_regroup has a workgroup per group (its group loop needs more than
    65 536 groups, which no grid reaches) and the k2d expansion behind it.  Byte and char offsets."""

    def make():
        blob, offs, nf = synth.keys(3, K=20_000)
        return synth.corpus(3, blob, offs, nf, n_bytes=(4 << 20) + 999, doc_bytes=1 << 16)
    corpus, doc = cached(_DATA, "groups", make)
    keys = cap_keys()
    g = compile_profiled(keys)
    for chars in (False, True):
        t = check_device(g, corpus, doc, oracle_batch("groups", keys, corpus, doc, chars=chars), chars=chars)
        assert t["engine"] == 4 and t["chunk_bytes"] == v2_chunk(corpus.size, geometry.grid, g.info["max_key_len"])
        n_groups = -(-t["n_chunks"] // 64)
        assert n_groups >= 4 * 2 * geometry.grid  # four groups and more per expansion workgroup


def dense_data(layout):
    def make():
        rng = random.Random(5)
        pieces = [b"a" * k for k in range(1, 10)] + [b"ab", b"bab", b"abc", b"c", b" "]
        parts, size = [], 0
        while size < (1 << 20) + 13:
            p = rng.choice(pieces)
            parts.append(p)
            size += len(p)
        text = b"".join(parts)[:(1 << 20) + 13]
        n = len(text)
        step = 37 if layout == "many" else 4099
        doc = np.array(sorted(list(range(0, n, step)) + [0, 4099 * 7, n, n]), dtype=np.uint64)
        keys = [b"a" * k for k in range(1, 7)] + [b"ab", b"b", b"bab", b"abab", b"abc"]
        blob, offs = orc.pack_keys(keys)
        return np.frombuffer(text, dtype=np.uint8).copy(), doc, ("dense", blob, np.asarray(offs, dtype=np.uint64))
    return cached(_DATA, ("dense", layout), make)


@pytest.mark.parametrize("layout", ["many", "few"])
@pytest.mark.parametrize("blocks", [1, 3, 7])
@grids(("g1",), ("v2", "ur"))
def test_dense_expansion_blocks_take_several_chunks(geometry, engine, monkeypatch, blocks, layout):
    """k2d_expand_dense with AHA_EXPAND_BLOCKS = 1, 3, 7 (read per call): a block walks many chunks (`c += n_blocks`) and
    the per-document offsets' blocks ride behind doc_from.  A hit-dense batch (2+ hits per byte, a capacity that says
    so) of ~28 000 documents of 37 bytes (a lane per document) or of 256 documents (16 lanes per document)."""
    monkeypatch.setenv("AHA_EXPAND_BLOCKS", str(blocks))
    corpus, doc, keys = dense_data(layout)
    want = oracle_batch("dense-" + layout, keys, corpus, doc)
    assert want[2] > 2 * corpus.size
    g = compile_profiled(keys)
    t = check_device(g, corpus, doc, want)
    assert t["engine"] == (4 if engine == "ur" else 2) and t["repeats"] == 0
    assert t["n_chunks"] >= 100 * blocks  # a hundred chunks and more per block
    assert (doc.size > 4 * t["n_chunks"]) == (layout == "many")


# ---- 6. the shipped multi-GPU setting ------------------------------------------------------------------------------

@pytest.mark.parametrize("transport", ["copies", "self-rccl"])
@grids(("ship",), ("v2", "u", "auto"))
def test_group_of_shards_under_the_shipped_reserve(geometry, engine, monkeypatch, transport):
    """AHA_RESERVE_CUS=16 -- what bench.py sets for more than one GPU -- on the group of three shards on one device, with
    the streams copied and through RCCL to itself (AHA_GROUP_RCCL=self), against the oracle.  A single handle compiled
    under the same environment shows the grid took effect: its chunk over 64 * cus * 1024 bytes is the reduced grid's."""
    from aha_amd import ACGroup

    if transport == "self-rccl":
        monkeypatch.setenv("AHA_GROUP_RCCL", "self")
    keys = cap_keys()

    def make():
        blob, offs, nf = synth.keys(3, K=20_000)
        return synth.corpus(3, blob, offs, nf, n_bytes=(8 << 20) + 3, doc_bytes=1 << 16)
    corpus, doc = cached(_DATA, "group", make)
    grp = ACGroup.compile_packed(keys[1], keys[2], [0, 0, 0])
    for chars in (False, True):
        raw, od, total = oracle_batch("group", keys, corpus, doc, chars=chars)
        gh, gd = grp.match_batch(corpus, doc, chars=chars, cap=16)  # too small first: the capacity protocol
        assert np.array_equal(gd, od) and gh.tobytes() == raw
        for shard in range(3):
            assert grp.download_shard(shard).tobytes() == raw, (chars, shard)
        t = grp.last_timing()
        assert t["n_devices"] == 3 and t["n_hits"] == total and t["exchange"] == (2 if transport == "self-rccl" else 0)
    # the grid: S = 64 bytes on the full device, 128 on cus - 16 workgroups
    n = 64 * geometry.cus * THREADS
    small = ("ship-small",) + tuple(np.asarray(x) for x in orc.pack_keys([b"ab", b"b", "中国".encode()]))
    text = np.frombuffer((b"xy ab z " + "中国 ".encode() + b"bb q ") * (n // 20 + 1), dtype=np.uint8)[:n].copy()
    sdoc = np.array([0, n // 3, n], dtype=np.uint64)
    g = compile_profiled(small)
    t = check_device(g, text, sdoc, oracle_batch("ship-small", small, text, sdoc))
    assert t["engine"] in (2, 4) and t["chunk_bytes"] == v2_chunk(n, geometry.grid, 6) == 128 != v2_chunk(n, geometry.cus, 6)


# ---- the reduced grids at the library's own sizes ------------------------------------------------------------------

@grids(("ship", "bpc2"), ("v2", "v2p", "u", "ur", "uh", "u23", "f", "k", "p", "auto"))
def test_parity_on_the_shipped_and_two_per_cu_grids(geometry, engine):
    """Every variant on the shipped reserve (cus - 16 workgroups) and on two workgroups per CU (half the LDS prefix; no
    character-level engines), over 256 * cus * 1024 - 4 095 bytes of cfg 3 text: a batch whose chunk differs between the
    full grid (256 bytes), cus - 16 workgroups (320) and 2 * cus (192), so the assertion on chunk_bytes pins the grid the
    handle was compiled with.  Byte and char offsets."""

    def make():
        blob, offs, nf = synth.keys(3, K=20_000)
        return synth.corpus(3, blob, offs, nf, n_bytes=256 * geometry.cus * THREADS - 4095, doc_bytes=1 << 20)
    corpus, doc = cached(_DATA, ("grids", geometry.cus), make)
    keys = cap_keys()
    g = compile_profiled(keys)
    lmax = g.info["max_key_len"]
    s_geo, s_full = v2_chunk(corpus.size, geometry.grid, lmax), v2_chunk(corpus.size, geometry.cus, lmax)
    assert s_geo != s_full
    for chars in (False, True):
        t = check_device(g, corpus, doc, oracle_batch("grids-%d" % geometry.cus, keys, corpus, doc, chars=chars), chars=chars)
        assert t["engine"] in want_engines(engine, geometry, chars=chars), (t["engine"], chars)
        if t["engine"] == 7:
            assert t["chunk_bytes"] == PAIR_TILE and t["n_chunks"] > 16 * geometry.grid
        else:
            assert t["chunk_bytes"] == s_geo, (t["chunk_bytes"], s_geo, s_full)
