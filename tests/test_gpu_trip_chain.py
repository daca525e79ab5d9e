"""ku_traverse's chain from one probe to the next (scan_unit.hip): a trip works out in the probe's shadow
where a miss goes, the masks of a group record, where the lane stands and whether it reports once the unit is consumed; the
probe's answer only picks among them.  The cases are those where such a hoisted select -- or an event insert that waits for
the next trip's shadow, the variant kept as tools/lab/trip_chain_dropped.patch -- can go wrong, every one against the CPU
oracle, hits and document offsets byte for byte.  The keys are at most three bytes long, so the chunk is 64 bytes and a wave
of 64 chunks covers 4 KiB of text.

Events in every trip, and in the last one:
- `ab`, `ba` over `abab..`: every lane reports in every trip, so every trip has an insert AND a buffer that has to be
  emptied before it; the same behind a first document of 1, 7 and 63 bytes, and with `ab` alone (events every other trip);
- a key that ends in the last trip before the trip loop is left: on the last byte of a 16-byte piece (the round ends), on
  the last byte before a document boundary in the middle of a piece (`..ab|ab..`, also with empty documents there: the
  boundary block reads the lane's counts right behind it), on the last byte of a chunk, on byte N - 1 of a text whose
  length is no multiple of 16, and in a lane that has run ahead to the end of its window, where the next unit -- three
  bytes, split across the window's end -- is not staged yet: the lane parks right behind its event.
What the shadow picks:
- text that walks every way a miss can go -- to the root, through F1 (root[the symbol that led here]), through a header
  (`abc`, `bcd`, `cd`: `abc` fails to `bc`, neither the root nor a one-character state; "pending" on `u`, "beside" on `uh`)
  -- in lanes whose neighbours consume their unit in the same trip, so a lane that tries its unit again has to keep its
  place, its unit and the symbol that led to its state;
- a redirect through the group record of a big state: 600 keys `a` + a two-byte character make `a` a state whose high
  symbols are reached through group records (info: unit_n_big, unit_n_low below the number of symbols).
Geometry: 65 and 127 chunks (a partial last wave), one workgroup that loops over tiles (nothing of one tile's last trips
may reach the next tile), and a capacity so small that a region overflows and the call is repeated."""
import numpy as np
import pytest

import pyoracle as orc
from aha_amd import AC
from engine_variants import use_variant

pytestmark = pytest.mark.gpu

S = 64  # the smallest chunk

KEYSETS = {
    "abba": [b"ab", b"ba"],
    "ab": [b"ab"],
    "mix": [b"ab", b"ba", "月".encode(), "éa".encode()],
    "suffix": [b"abc", b"bcd", b"cd", b"b", "éa".encode(), "aé".encode()],
    "big": [b"a" + chr(c).encode() for c in range(0x400, 0x400 + 600)] + [b"ab", b"ba", chr(0x410).encode() + b"a"],
}

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
    """text outside every key set's alphabet, with two- and three-byte characters in it (char offsets differ from byte offsets)"""
    return np.frombuffer(("q" * 11 + "ü" + "qq月").encode() * (n // 16 + 1), dtype=np.uint8)[:n].copy()


def put(buf, at, what):
    w = np.frombuffer(what, dtype=np.uint8)
    buf[at:at + w.size] = w


def from_alphabet(seed, n, alphabet):
    """n bytes (about) of units drawn from `alphabet` (a list of byte strings), cut at a unit"""
    rng = np.random.default_rng(seed)
    out, size = [], 0
    while size < n:
        u = alphabet[int(rng.integers(len(alphabet)))]
        out.append(u)
        size += len(u)
    return np.frombuffer(b"".join(out), dtype=np.uint8).copy()


def texts():
    """name -> (key set, text, document offsets)"""
    def make():
        t = {}
        # ---- an insert in every trip, and a buffer that is emptied in front of it
        for ks in ("abba", "ab"):
            for chunks in (128, 65, 127):  # whole waves; a partial last wave
                n = chunks * S
                t["%s-abab-%d" % (ks, chunks)] = (ks, abab(n), [0, n // 3, n])
            for p in (1, 7, 63):
                n = p + 128 * S
                t["%s-prefix-%d" % (ks, p)] = (ks, np.concatenate([np.full(p, ord("x"), dtype=np.uint8), abab(n - p)]), [0, p, n])
        # ---- the last trip before the trip loop is left
        n = 3 * 64 * S
        buf = quiet(n)
        buf[buf >= 0x80] = ord("q")  # (one trip per byte: the lanes of a wave stay in step, the round ends for all of them at once)
        for c in range(n // S):      # `ab` on the last two bytes of a piece: which piece depends on the chunk, some chunks none
            if c % 5 != 4:
                put(buf, c * S + 16 * (c % 4) + 14, b"ab")
            if c % 7 == 0:
                put(buf, c * S + 30, b"abab")  # ... and across the piece's end
        t["piece-end"] = ("abba", buf, [0, n])
        n = 2 * 64 * S + 40
        buf, doc = quiet(n), [0]
        for c in range(0, n // S, 3):  # `..ab|ab..` with the boundary in the middle of a piece; every other one with empty documents
            at = c * S + 16 * (c % 4) + 7
            put(buf, at - 4, b"qbabab")  # ends: ..ab at at - 1; the next document starts with `ab`
            put(buf, at - 2, b"abab")
            doc += [at] * (1 + (c % 2) * 2)
        t["boundary"] = ("abba", buf, doc + [n])
        n = 130 * S + 5  # no multiple of 16: the last piece is loaded byte by byte
        buf = quiet(n)
        for c in range(n // S):
            if c % 3 != 2:
                put(buf, c * S + S - 2, b"ab")     # the last byte of the chunk
            if c % 4 == 1:
                put(buf, c * S + S - 1, b"aba")    # ... and a key across the chunks' border, one that starts a chunk
        put(buf, n - 2, b"ab")                     # byte N - 1
        t["chunk-end"] = ("abba", buf, [0, 64 * S + S, n])
        n = 2 * 64 * S
        buf = abab(n)  # a trip per byte -- beside chunks of three-byte characters, whose lanes run ahead to the window's end
        moon = np.frombuffer("月".encode() * (2 * S // 3 + 2), dtype=np.uint8)
        for c in range(0, n // S, 4):
            buf[c * S:(c + 2) * S] = moon[:2 * S] if c % 8 else moon[1:2 * S + 1]  # (also out of step with the chunk's start)
        for c in range(2, n // S, 16):
            put(buf, c * S + 3, "éaéqéa".encode())
        t["parked"] = ("mix", buf, [0, 37 * S + 12, n])
        # ---- every way a miss can go, in lanes beside lanes that consume
        alpha = [b"a", b"b", b"c", b"d", b"q", "é".encode(), "月".encode(), b"abc", b"abcd", b"bcq", b"abq", b"aq", b"\xe6\x9c", b"\xa9"]
        buf = from_alphabet(11, 200 * S + 9, alpha)
        t["misses"] = ("suffix", buf, [0, 5, 5, 3001, buf.size])
        # ---- group records: `a` + a high symbol that continues, one that does not, a low one; keys of the other kind between them
        big = [b"a" + chr(c).encode() for c in range(0x400, 0x400 + 700, 7)] + [b"a", b"ab", b"ba", chr(0x410).encode() + b"a",
                                                                                 chr(0x655).encode(), b"q", b"aa" + chr(0x6FF).encode()]
        buf = from_alphabet(12, 100 * S + 3, big)
        t["groups"] = ("big", buf, [0, 1000, buf.size])
        # ---- regions that overflow
        n = 4 * 64 * S
        few = quiet(n)
        for c in range(0, n // S, 8):  # every eighth chunk reports 63 times, the others never
            few[c * S:(c + 1) * S] = abab(S)
        t["uneven"] = ("abba", few, [0, n])
        return {k: (v[0], v[1], np.array(v[2], dtype=np.uint64)) for k, v in t.items()}
    return cached("texts", make)


def oracle(name, chars):
    def make():
        ks, corpus, doc = texts()[name]
        o = cached(("oracle", ks), lambda: orc.AC.compile_packed(*packed(ks)))
        oh, od = o.match_batch(corpus, doc, chars=chars, cap=2 * corpus.size + 1024)
        return oh.tobytes(), np.asarray(od, dtype=np.uint64), len(oh)
    return cached(("want", name, chars), make)


def run(g, corpus, doc, want, chars, cap=None):
    import torch

    raw, od, total = want
    cap = total if cap is None else cap
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
    assert info["unit_enabled"] and info["max_key_len"] <= 3
    if variant in ("u", "uh"):
        assert info["unit_header_beside"] == (1 if variant == "uh" else 0)
    assert info["unit_base_bits"] == (23 if variant == "u23" else 22)
    if ks == "big":  # group records are in use: a big state, and symbols above the ones it keeps in its direct row
        assert info["unit_n_big"] >= 1 and info["unit_syms"] > info["unit_n_low"], info
    if ks == "suffix":
        assert info["unit_headers"] >= 1, info
    return g


@pytest.fixture
def engine(request, monkeypatch):
    monkeypatch.delenv("AHA_RESERVE_CUS", raising=False)
    return use_variant(request.param, monkeypatch)


@pytest.mark.parametrize("chars", [False, True], ids=["bytes", "chars"])
@pytest.mark.parametrize("engine", ["u", "uh", "u23"], indirect=True)
def test_events_in_every_trip_and_shadow_selects(engine, chars):
    handles = {}
    for name, (ks, corpus, doc) in texts().items():
        if ks not in handles:
            handles[ks] = handle(engine, ks)
        want = oracle(name, chars)
        assert want[2] > 0, name
        t = run(handles[ks], corpus, doc, want, chars, cap=want[2] + 4096)  # (room enough: the regions hold what their chunks report)
        assert t["engine"] == 4 and t["chunk_bytes"] == S and t["repeats"] == 0, (name, t)
        assert t["n_chunks"] == -(-corpus.size // S)


def test_the_texts_are_what_their_names_say():
    """(no GPU work of its own: the oracle's hits show that each text holds the case it is there for)"""
    def ends(name):  # byte offsets behind the hits, per document start
        ks, corpus, doc = texts()[name]
        raw, od, total = oracle(name, False)
        h = np.frombuffer(raw, dtype=np.int32).reshape(-1, 3)
        return ks, corpus, doc, h, od
    ks, corpus, doc, h, od = ends("abba-abab-128")
    assert h.shape[0] == corpus.size - 2  # every byte but a document's first ends a key: 63 or 64 reports per chunk
    ks, corpus, doc, h, od = ends("boundary")
    assert len(set(doc.tolist())) < doc.size  # empty documents
    for d in doc[1:-1].tolist():
        assert corpus[d - 2:d + 2].tobytes() == b"abab" and d % 16 == 7
    ks, corpus, doc, h, od = ends("chunk-end")
    assert corpus.size % 16 and corpus[-2:].tobytes() == b"ab"
    ks, corpus, doc, h, od = ends("piece-end")
    assert h.shape[0] >= 3 * 64 * 4 // 5


@pytest.mark.parametrize("chars", [False, True], ids=["bytes", "chars"])
@pytest.mark.parametrize("engine", ["u", "uh", "u23"], indirect=True)
def test_region_overflow_repeats_the_call_on_dense_events(engine, chars):
    """An exact capacity over a text whose hits sit in every eighth chunk: the regions are sized for twice the average + 16
    events, a reporting chunk sends 63 -- cursor[1] = 2, and the host repeats the call with full-size regions."""
    g = handle(engine, "abba")
    ks, corpus, doc = texts()["uneven"]
    want = oracle("uneven", chars)
    assert 2 * (want[2] // (corpus.size // S)) + 16 < 63
    t = run(g, corpus, doc, want, chars)
    assert t["engine"] == 4 and t["chunk_bytes"] == S and t["repeats"] == 1, t


@pytest.mark.parametrize("chars", [False, True], ids=["bytes", "chars"])
@pytest.mark.parametrize("engine", ["u"], indirect=True)
def test_one_tile_ends_in_events_and_the_next_starts_clean(engine, chars, monkeypatch):
    """AHA_RESERVE_CUS = CUs - 1: one traversal workgroup, which loops over its tiles.  Its chunk grows with the text up to
    32 KiB, so several tiles need more than 32 MiB: quiet text with `abab..` up to the last byte of the first tile and from
    the first byte of the second (the last trips of a tile report; the next tile starts with an empty buffer and no state), in
    the partial last wave and at the very end."""
    import torch

    cus = torch.cuda.get_device_properties(0).multi_processor_count
    monkeypatch.setenv("AHA_RESERVE_CUS", str(cus - 1))
    tile = 1024 * 32768

    def make():
        n = tile + 65 * 32768 + 11
        buf = np.full(n, ord("q"), dtype=np.uint8)
        for at, ln in ((tile - 40_000, 40_000), (tile + 3, 5001), (tile + 64 * 32768 - 50, 30_000), (n - 999, 999), (32768 - 7, 70_000)):
            buf[at:at + ln] = abab(ln)
        return buf, np.array([0, tile - 1, tile - 1, n], dtype=np.uint64)
    corpus, doc = cached("tiles", make)

    def want_():
        o = cached(("oracle", "abba"), lambda: orc.AC.compile_packed(*packed("abba")))
        oh, od = o.match_batch(corpus, doc, chars=chars, cap=1 << 20)
        return oh.tobytes(), np.asarray(od, dtype=np.uint64), len(oh)
    want = cached(("want-tiles", chars), want_)
    g = handle(engine, "abba")
    t = run(g, corpus, doc, want, chars, cap=want[2] + 4096)
    assert t["engine"] == 4 and t["chunk_bytes"] == 32768 and t["n_chunks"] == 1024 + 66, t
