"""ku_traverse's trip (scan_unit.hip) at the edges of its event buffer -- which is emptied before an insert it cannot take
-- and of the set of lanes that probe, every case against the CPU oracle bit for bit.  The keys are at most three bytes
long, so the chunk falls to its 64-byte minimum and a wave of 64 chunks is 4 KiB of text:

- `abab..` with the key `ab`: every lane reports in the same trip (64 events per trip), so every insert meets a buffer that
  cannot take it and is emptied first; the same behind a first document of 1, 7 or 63 bytes: a boundary inside the first
  chunk, whose lane falls out of step with the others, so the fill stops being a multiple of 64;
- text outside the keys' alphabet: no lane probes and nothing is reported; one `abab..` chunk per wave: one lane probes and
  reports, the buffer fills one record at a time (every residue, `fill + events == 64` among them); every eighth chunk:
  eight at a time;
- 65 and 127 chunks (a partial last wave: its part of the event space is smaller than 64 regions), a length that is no
  multiple of 16, several tiles;
- a capacity so small that a region overflows and the call is repeated with full-size regions;
- all of it with char offsets, with the header beside the probe (AHA_UNIT_HEADER_BESIDE) and with 23-bit bases
  (AHA_UNIT_BASE_BITS); and once on a single workgroup, which loops over several tiles."""
import numpy as np
import pytest

import pyoracle as orc
from aha_amd import AC
from engine_variants import use_variant

pytestmark = pytest.mark.gpu

S = 64  # the smallest chunk
KEYS = [b"ab", b"bca", "éa".encode()]  # (the last one: a two-byte unit in the alphabet, so char offsets differ from byte offsets)

_CACHE = {}


def cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def packed():
    def make():
        blob, offs = orc.pack_keys(KEYS)
        return np.asarray(blob), np.asarray(offs, dtype=np.uint64)
    return cached("keys", make)


def abab(n):
    return np.frombuffer(b"ab" * (n // 2 + 1), dtype=np.uint8)[:n].copy()


def texts():
    """name -> (text, document offsets)"""
    def make():
        t = {}
        for chunks in (64, 65, 127, 3 * 1024 + 65):  # whole waves, a partial last wave, three tiles and a partial one
            n = chunks * S
            t["abab-%d" % chunks] = (abab(n), [0, n // 3, n])
        n = 70 * S + 5  # no multiple of 16: the last piece is loaded byte by byte
        t["abab-odd"] = (abab(n), [0, n])
        for p in (1, 7, 63):
            n = p + 128 * S
            t["prefix-%d" % p] = (np.concatenate([np.full(p, ord("x"), dtype=np.uint8), abab(n - p)]), [0, p, n])
        n = 130 * S + 3
        quiet = np.frombuffer(("q" * 37 + "ü" + "qq月").encode() * (n // 40 + 1), dtype=np.uint8)[:n - 3].copy()
        t["no-probe"] = (np.concatenate([quiet, np.frombuffer(b"qqq", dtype=np.uint8)]), [0, n])
        n = 5 * 64 * S + 3 * S
        one = np.full(n, ord("q"), dtype=np.uint8)
        for w in range(-(-n // (64 * S))):  # one chunk of every wave: lane (7 w + 3) % 64
            at = (w * 64 + (7 * w + 3) % 64) * S
            if at + S <= n:
                one[at:at + S] = abab(S)
        t["one-lane"] = (one, [0, n // 2 + 1, n])
        n = 4 * 64 * S
        few = np.full(n, ord("q"), dtype=np.uint8)
        for c in range(0, n // S, 8):  # every eighth chunk reports 32 times, the others never
            few[c * S:(c + 1) * S] = abab(S)
        t["uneven"] = (few, [0, n])
        mixed = ("ab" * 9 + "éa" + "bca" + "q" + "éab").encode()
        n = 200 * S + 1
        t["mixed"] = (np.frombuffer(mixed * (n // len(mixed) + 1), dtype=np.uint8)[:n - 1].copy(), [0, 76, 76, n - 1])
        return {k: (v[0], np.array(v[1], dtype=np.uint64)) for k, v in t.items()}
    return cached("texts", make)


def oracle(name, chars):
    def make():
        o = cached("oracle", lambda: orc.AC.compile_packed(*packed()))
        corpus, doc = texts()[name]
        oh, od = o.match_batch(corpus, doc, chars=chars, cap=corpus.size + 1024)
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


def handle(variant):
    g = AC.compile_packed(*packed())
    g.set_profiling(True)
    info = g.info
    assert info["unit_enabled"]
    if variant in ("u", "uh"):
        assert info["unit_header_beside"] == (1 if variant == "uh" else 0)
    assert info["unit_base_bits"] == (23 if variant == "u23" else 22)
    return g


@pytest.fixture
def engine(request, monkeypatch):
    monkeypatch.delenv("AHA_RESERVE_CUS", raising=False)
    return use_variant(request.param, monkeypatch)


@pytest.mark.parametrize("chars", [False, True], ids=["bytes", "chars"])
@pytest.mark.parametrize("engine", ["u", "uh", "u23"], indirect=True)
def test_event_buffer_and_probe_mask_edges(engine, chars):
    g = handle(engine)
    for name, (corpus, doc) in texts().items():
        want = oracle(name, chars)
        t = run(g, corpus, doc, want, chars, cap=want[2] + 4096)  # (room enough: the regions hold what their chunks report)
        assert t["engine"] == 4 and t["chunk_bytes"] == S and t["repeats"] == 0, (name, t)
        assert t["n_chunks"] == -(-corpus.size // S)
        assert (want[2] == 0) == (name == "no-probe")


@pytest.mark.parametrize("chars", [False, True], ids=["bytes", "chars"])
@pytest.mark.parametrize("engine", ["u", "uh", "u23"], indirect=True)
def test_region_overflow_repeats_the_call(engine, chars):
    """An exact capacity over a text whose hits sit in every eighth chunk: the regions are sized for twice the average + 16
    events, a reporting chunk sends 32 -- cursor[1] = 2, and the host repeats the call with full-size regions."""
    g = handle(engine)
    corpus, doc = texts()["uneven"]
    want = oracle("uneven", chars)
    assert 2 * (want[2] // (corpus.size // S)) + 16 < 32
    t = run(g, corpus, doc, want, chars)
    assert t["engine"] == 4 and t["chunk_bytes"] == S and t["repeats"] == 1, t


@pytest.mark.parametrize("chars", [False, True], ids=["bytes", "chars"])
@pytest.mark.parametrize("engine", ["u"], indirect=True)
def test_one_workgroup_loops_over_tiles(engine, chars, monkeypatch):
    """AHA_RESERVE_CUS = CUs - 1: one traversal workgroup.  Its chunk grows with the text up to 32 KiB, so several tiles need
    more than 32 MiB: quiet text with `abab..` across the tile edge, at the start of the second tile's last wave and at the
    very end -- the wave's buffer and its part of the event space are set up again for every tile."""
    import torch

    cus = torch.cuda.get_device_properties(0).multi_processor_count
    monkeypatch.setenv("AHA_RESERVE_CUS", str(cus - 1))
    tile = 1024 * 32768

    def make():
        n = tile + 65 * 32768 + 11
        buf = np.full(n, ord("q"), dtype=np.uint8)
        for at, ln in ((tile - 3000, 6001), (tile + 64 * 32768 - 50, 30_000), (n - 999, 999), (12_345, 70_000)):
            buf[at:at + ln] = abab(ln)
        return buf, np.array([0, tile + 1, n], dtype=np.uint64)
    corpus, doc = cached("tiles", make)

    def want_():
        o = cached("oracle", lambda: orc.AC.compile_packed(*packed()))
        oh, od = o.match_batch(corpus, doc, chars=chars, cap=1 << 20)
        return oh.tobytes(), np.asarray(od, dtype=np.uint64), len(oh)
    want = cached(("want-tiles", chars), want_)
    g = handle(engine)
    t = run(g, corpus, doc, want, chars, cap=want[2] + 4096)
    assert t["engine"] == 4 and t["chunk_bytes"] == 32768 and t["n_chunks"] == 1024 + 66, t
