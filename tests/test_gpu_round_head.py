"""ku_traverse's round head (scan_unit.hip): an input line -- 64 bytes, four pieces -- is requested whole, one
round before its first piece is staged, by four plain loads where all of it lies inside the text and through the byte-wise
path where it holds the text's end; lines before the text's start and behind its end are zeros.  The issue priority is set in
the round that requests a line.  Every case against the CPU oracle, hits and document offsets byte for byte, with the fused
and the general post pass ("u", "ur"), the header beside the probe ("uh"), byte and char offsets.

1. the text ends at every phase of a line: N in {1, 15, .. 129} and one chunk more, with a key that ends exactly at N, a
   three-byte unit cut off by N and a key whose last unit starts in the last piece; N = 0 and only empty documents;
2. lines before the text's start: the first chunk's warm-up with longest keys of 2, 17, 64, 65 and 129 bytes, a key across
   every chunk border (the next chunk's lane finds it through its warm-up) and a document that starts in the middle of a
   line, behind a key's first half (the warm-up is clipped there);
3. a hit that ends at every offset modulo 64 over chunks of five lines, document boundaries at 0, 16, 32, 48 and odd offsets
   of a line: the queue's rotation and the request in every phase, a boundary in the round that requests a line;
4. rounds without a trip between a request and its use: a second chunk of a single byte, a wave with one live lane (65
   chunks), chunks of three-byte characters beside chunks that take a trip per byte (their lanes are done with the window
   while the others still walk); the workgroup's other waves have no live lane at all and run every round without a trip;
5. one workgroup over three tiles and a ragged fourth (AHA_RESERVE_CUS = CUs - 1): the first line of every tile is
   requested by the round in front of its first; a tile that ends in events is followed by one that starts clean;
6. case 3 over 4 500 chunks, on the full grid (five workgroups with every wave live, so all four ranks of every SIMD note and
   read progress words) and on one workgroup: the priority words must not change a result."""
import numpy as np
import pytest

import pyoracle as orc
from aha_amd import AC
from engine_variants import use_variant

pytestmark = pytest.mark.gpu

LINE_ENDS = [1, 15, 16, 17, 47, 48, 49, 63, 64, 65, 127, 128, 129]
MOON = "月".encode()


def long_key(n):
    """n bytes without a period: no proper suffix of it is a prefix"""
    return (b"k" + b"lmnopqrstuvwxyz" * (n // 15 + 1))[:n - 1] + b"K"


KEYSETS = {
    "short": [b"ab", b"ba", MOON, b"a" + MOON, "é".encode() + b"a"],
    "abba": [b"ab", b"ba"],
    "w2": [b"ab"],
    "w17": [b"ab", long_key(17)],
    "w64": [b"ab", long_key(64)],
    "w65": [b"ab", long_key(65)],
    "w129": [b"ab", long_key(129)],
    "five": [b"ab", b"ba", long_key(40)],  # chunks of 320 bytes: five lines
}
S_OF = {"short": 64, "abba": 64, "w2": 64, "w17": 192, "w64": 512, "w65": 576, "w129": 1088, "five": 320}  # 8 x the longest key, in whole lines

_CACHE = {}


def cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def packed(ks):
    def make():
        blob, offs = orc.pack_keys(KEYSETS[ks])
        return np.asarray(blob), np.asarray(offs, dtype=np.uint64)
    return cached(("keys", ks), make)


def abab(n):
    return np.frombuffer(b"ab" * (n // 2 + 1), dtype=np.uint8)[:n].copy()


def quiet(n):
    return np.frombuffer(("q" * 11 + "ü" + "qq月").encode() * (n // 16 + 1), dtype=np.uint8)[:n].copy()


def put(buf, at, what):
    w = np.frombuffer(what, dtype=np.uint8)
    buf[at:at + w.size] = w


def texts():
    """name -> (key set, text, document offsets)"""
    def make():
        t = {}
        # ---- 1. the text's end in every phase of a line
        t["end-0"] = ("short", np.zeros(0, dtype=np.uint8), [0])
        t["end-0-empty-docs"] = ("short", np.zeros(0, dtype=np.uint8), [0, 0, 0, 0])
        for base in (0, 64):
            for k in LINE_ENDS:
                n = base + k
                for tail, what in (("key", b"ab"), ("cut", b"a" + MOON[:2]), ("unit", b"a" + MOON)):
                    if len(what) > n:
                        continue
                    buf = quiet(n)
                    if n >= 8:
                        put(buf, 0, b"abab")
                    put(buf, n - len(what), what)
                    t["end-%d-%s" % (n, tail)] = ("short", buf, [0, n] if n % 2 else [0, n, n])
        # ---- 2. lines before the text's start; the warm-up across a chunk border and clipped at a document's start
        for ks in ("w2", "w17", "w64", "w65", "w129"):
            s, key = S_OF[ks], KEYSETS[ks][-1]
            n = 5 * s + 21
            buf = quiet(n)
            put(buf, 0, key)                                   # in the first chunk's first bytes
            put(buf, s - len(key) + 1, key)                    # ends on the second chunk's first byte
            put(buf, 2 * s - 1, key)                           # starts on the second chunk's last byte
            cut = 3 * s - len(key) // 2 - 1                    # a document starts in the warm-up of the fourth chunk, mid-line,
            put(buf, 3 * s - len(key) + 1, key)                # behind the key's first half (no hit: it does not lie in one document)
            put(buf, 4 * s - len(key) // 2, key)
            put(buf, n - len(key), key)                        # ends at N
            t["warm-" + ks] = (ks, buf, [0, cut, n])
        # ---- 3. a hit at every offset modulo 64, boundaries in every phase
        s = S_OF["five"]
        n = 70 * s + 7
        buf = abab(n)
        put(buf, 3 * s - 11, KEYSETS["five"][-1])
        doc = [0] + [c * s + 64 * (c % 5) + o for c, o in zip(range(1, 69, 2), [0, 16, 32, 48, 1, 15, 17, 31, 33, 47, 49, 63] * 3)]
        t["phases"] = ("five", buf, sorted(doc) + [n])
        n = 4500 * s + 7  # ... and the same over several workgroups' worth of chunks (case 6)
        t["phases-wide"] = ("five", abab(n), sorted([0] + [c * s + 64 * (c % 5) + o for c, o in
                                                           zip(range(1, 4499, 7), [0, 16, 32, 48, 1, 15, 17, 31, 33, 47, 49, 63] * 60)]) + [n])
        # ---- 4. rounds without a trip between a request and its use
        t["second-chunk-one-byte"] = ("short", abab(65), [0, 65])
        t["one-live-lane"] = ("short", abab(64 * 64 + 37), [0, 100, 64 * 64 + 37])
        n = 128 * 64
        buf = abab(n)
        moon = np.frombuffer(MOON * 64, dtype=np.uint8)
        for c in range(0, n // 64, 3):  # chunks of three-byte characters: a third of the trips of their neighbours
            buf[c * 64:c * 64 + 63] = moon[:63]
        t["ahead"] = ("short", buf, [0, n])
        return {k: (v[0], v[1], np.array(v[2], dtype=np.uint64)) for k, v in t.items()}
    return cached("texts", make)


def oracle(name, chars):
    def make():
        ks, corpus, doc = texts()[name]
        o = cached(("oracle", ks), lambda: orc.AC.compile_packed(*packed(ks)))
        oh, od = o.match_batch(corpus, doc, chars=chars, cap=2 * corpus.size + 1024)
        return oh.tobytes(), np.asarray(od, dtype=np.uint64), len(oh)
    return cached(("want", name, chars), make)


def ends(name):
    """absolute byte offsets behind the oracle's hits"""
    ks, corpus, doc = texts()[name]
    raw, od, total = oracle(name, False)
    h = np.frombuffer(raw, dtype=orc.HIT_DTYPE)
    per_doc = np.diff(od.astype(np.int64))
    return np.repeat(doc[:-1].astype(np.int64), per_doc) + h["end"].astype(np.int64), h


def run(g, corpus, doc, want, chars):
    import torch

    raw, od, total = want
    cap = total + 4096
    dc = torch.from_numpy(corpus).cuda()
    dd = torch.from_numpy(doc.astype(np.int64)).cuda()
    big = torch.full((cap + 64, 3), -7, dtype=torch.int32, device="cuda")
    dho = torch.full((doc.size + 8,), -7, dtype=torch.int64, device="cuda")
    n = g.match_batch_device(dc, dd, big[:cap], dho[:doc.size], chars=chars)
    assert bool((big[cap:] == -7).all()) and bool((dho[doc.size:] == -7).all())
    assert n == total and big[:n].cpu().numpy().tobytes() == raw
    assert np.array_equal(dho[:doc.size].cpu().numpy().astype(np.uint64), od)
    return g.last_timing()


def handle(variant, ks):
    g = AC.compile_packed(*packed(ks))
    g.set_profiling(True)
    info = g.info
    assert info["unit_enabled"], info
    if variant in ("u", "uh"):
        assert info["unit_header_beside"] == (1 if variant == "uh" else 0)
    return g


@pytest.fixture
def engine(request, monkeypatch):
    monkeypatch.delenv("AHA_RESERVE_CUS", raising=False)
    return use_variant(request.param, monkeypatch)


def one_workgroup(monkeypatch):
    import torch

    monkeypatch.setenv("AHA_RESERVE_CUS", str(torch.cuda.get_device_properties(0).multi_processor_count - 1))


@pytest.mark.parametrize("chars", [False, True], ids=["bytes", "chars"])
@pytest.mark.parametrize("engine", ["u", "ur", "uh"], indirect=True)
def test_line_requests_at_the_texts_edges_and_in_every_phase(engine, chars):
    handles = {}
    for name, (ks, corpus, doc) in texts().items():
        if ks not in handles:
            handles[ks] = handle(engine, ks)
        t = run(handles[ks], corpus, doc, oracle(name, chars), chars)
        if corpus.size:
            assert t["engine"] == 4 and t["chunk_bytes"] == S_OF[ks] and t["repeats"] == 0, (name, t)
            assert t["n_chunks"] == -(-corpus.size // S_OF[ks]), (name, t)


def test_the_texts_are_what_their_names_say():
    """(no GPU work of its own: the oracle's hits show that each text holds the case it is there for)"""
    for n in [b + k for b in (0, 64) for k in LINE_ENDS]:
        for tail, key in (("key", 0), ("unit", 3)):
            if "end-%d-%s" % (n, tail) in texts():
                e, h = ends("end-%d-%s" % (n, tail))
                assert ((e == n) & (h["value"] == key)).any(), (n, tail)  # `ab` / `a月` ends exactly at N
        if "end-%d-cut" % n in texts():
            ks, corpus, doc = texts()["end-%d-cut" % n]
            assert corpus[-2:].tobytes() == MOON[:2] and corpus.size == n
            e, h = ends("end-%d-cut" % n)
            assert not (h["value"] >= 2).any() or (e[h["value"] >= 2] < n - 2).all()
    in_last_piece = [n for n in [b + k for b in (0, 64) for k in LINE_ENDS] if n >= 4 and n - 3 >= 16 * ((n - 1) // 16)]
    assert len(in_last_piece) >= 8, in_last_piece  # N = 15, 16, 47, 48, ..: the key's last unit starts in the text's last piece
    for n in in_last_piece:
        e, h = ends("end-%d-unit" % n)
        hit = (e == n) & (h["value"] == 3)
        assert hit.any() and texts()["end-%d-unit" % n][1][n - 3:].tobytes() == MOON
    for ks in ("w2", "w17", "w64", "w65", "w129"):
        s, key = S_OF[ks], KEYSETS[ks][-1]
        kid = len(KEYSETS[ks]) - 1
        corpus, doc = texts()["warm-" + ks][1:]
        e, h = ends("warm-" + ks)
        got = set(e[h["value"] == kid].tolist())
        across = {3 * s + 1} if int(doc[1]) <= 3 * s - len(key) + 1 else set()  # (a two-byte key lies behind the boundary)
        assert got == {len(key), s + 1, 2 * s - 1 + len(key), 4 * s - len(key) // 2 + len(key), corpus.size} | across, (ks, got)
        assert int(doc[1]) % 64 != 0 and 3 * s - max(len(key) - 1, 2) <= int(doc[1]) < 3 * s  # inside the warm-up, mid-line
    e, h = ends("phases")
    assert np.bincount(e % 64, minlength=64).min() > 0
    ks, corpus, doc = texts()["phases"]
    assert {0, 16, 32, 48, 1, 15, 17, 31, 33, 47, 49, 63} <= set((doc[1:-1] % 64).tolist())
    assert S_OF["five"] == 5 * 64 and (h["value"] == 2).sum() == 1
    assert texts()["second-chunk-one-byte"][1].size == 64 + 1
    assert -(-texts()["one-live-lane"][1].size // 64) == 65
    corpus = texts()["ahead"][1]
    units = ((corpus & 0xC0) != 0x80).reshape(-1, 64).sum(axis=1)  # trips a lane needs for its chunk, at least
    assert (units[0::3] <= 22).all() and (units[1::3] == 64).all() and (units[2::3] == 64).all()  # a third of its neighbours'
    e, h = ends("ahead")
    per_chunk = np.bincount((e - 1) // 64, minlength=128)
    assert (per_chunk[0::3] >= 20).all() and (per_chunk[1::3] >= 62).all()  # and both kinds report
    e, h = ends("phases-wide")
    assert np.bincount(e % 64, minlength=64).min() > 0
    assert {0, 16, 32, 48, 1, 15, 17, 31, 33, 47, 49, 63} <= set((texts()["phases-wide"][2][1:-1] % 64).tolist())


@pytest.mark.parametrize("chars", [False, True], ids=["bytes", "chars"])
@pytest.mark.parametrize("engine", ["u", "ur", "uh"], indirect=True)
def test_every_phase_on_one_workgroup_and_on_the_full_grid(engine, chars, monkeypatch):
    """The priority words order the waves of a SIMD by the lines they have requested: with every wave of several workgroups
    live, and with every wave of a single workgroup live, the result is the oracle's."""
    ks, corpus, doc = texts()["phases-wide"]
    want = oracle("phases-wide", chars)
    t = run(handle(engine, ks), corpus, doc, want, chars)
    assert t["engine"] == 4 and t["chunk_bytes"] == S_OF[ks] and t["n_chunks"] == 4501, t  # four full workgroups and a fifth
    one_workgroup(monkeypatch)
    t = run(handle(engine, ks), corpus, doc, want, chars)
    assert t["engine"] == 4 and 960 < t["n_chunks"] <= 1024, t  # (the chunk grows with the text: one tile, every wave live)


@pytest.mark.parametrize("chars", [False, True], ids=["bytes", "chars"])
@pytest.mark.parametrize("engine", ["u", "ur", "uh"], indirect=True)
def test_one_workgroup_requests_the_first_line_of_every_tile(engine, chars, monkeypatch):
    """One traversal workgroup; its chunk grows with the text up to 32 KiB, so three tiles and a ragged fourth are 96 MiB and
    a little: quiet text (one three-byte character in sixteen bytes) with `abab..` up to the last byte of the first and of
    the second tile, from the first byte of the third and up to its last; the second tile starts clean, and so does the
    fourth (the oracle's hits say so below)."""
    one_workgroup(monkeypatch)
    tile = 1024 * 32768

    def make():
        n = 3 * tile + 65 * 32768 + 11
        buf = quiet(n)
        for at, ln in ((tile - 40_000, 40_000), (2 * tile - 777, 777), (2 * tile, 5001), (3 * tile - 40, 40), (3 * tile + 64 * 32768 - 50, 30_000),
                       (n - 999, 999), (32768 - 7, 70_000)):
            buf[at:at + ln] = abab(ln)
        return buf, np.array([0, tile - 3, tile - 3, 2 * tile + 16, n], dtype=np.uint64)
    corpus, doc = cached("tiles", make)

    def want_():
        o = cached(("oracle", "abba"), lambda: orc.AC.compile_packed(*packed("abba")))
        oh, od = o.match_batch(corpus, doc, chars=chars, cap=1 << 20)
        return oh.tobytes(), np.asarray(od, dtype=np.uint64), len(oh)
    want = cached(("want-tiles", chars), want_)
    t = run(handle(engine, "abba"), corpus, doc, want, chars)
    assert t["engine"] == 4 and t["chunk_bytes"] == 32768 and t["n_chunks"] == 3 * 1024 + 66, t
    assert t["n_chunks"] > 3 * 1024  # three whole tiles and a ragged one
    if not chars:  # what the text is there for, from the oracle's hits: the chunk a hit ends in
        h = np.frombuffer(want[0], dtype=orc.HIT_DTYPE)
        e = np.repeat(doc[:-1].astype(np.int64), np.diff(want[1].astype(np.int64))) + h["end"].astype(np.int64)
        per_chunk = np.bincount((e - 1) // 32768, minlength=3 * 1024 + 66)
        assert per_chunk[1023] > 0 and per_chunk[2047] > 0 and per_chunk[3071] > 0  # every whole tile ends in events
        assert (e == tile).any() and (e == 2 * tile).any() and (e == 3 * tile).any()  # ... up to its last byte
        assert per_chunk[1024] == 0 and per_chunk[3072] == 0 and per_chunk[2048] > 0  # tiles two and four start clean, three does not
