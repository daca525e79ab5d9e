"""ku_traverse's waves set their issue priority from the progress of the other waves on their SIMD (scan_unit.hip: a word per
wave in LDS, written and read every round, nobody waits for it).  Priorities change when a wave runs, never what it computes:
every case against the CPU oracle bit for bit -- hits and doc_hit_off -- on the character-level engine with 22-bit and
23-bit bases, the header beside the probe, the general post passes (AHA_UNIT_POST=regroup) and char offsets, on one
workgroup (AHA_RESERVE_CUS = CUs - 1: the 16 waves whose words share the LDS block) and on the whole device.

The keys are at most eight bytes long, so the chunk's minimum is 64 bytes and a wave's group of 64 chunks is 4 KiB of text:

- batches of 1, 15, 16, 17, 33 and 16 * 5 + 1 such groups, the last one partial (1 or 63 chunks; one batch has fewer than 64
  chunks): one live wave on one SIMD, a SIMD with three live waves and one that only stages, every wave live, and -- on
  one workgroup -- chunks of 128, 192 and 384 bytes, so the waves do 9 to 25 rounds per chunk;
- document boundaries on the boundaries between two waves' groups and one byte to either side, empty documents at the very
  start and the very end, one document over many groups;
- call sequences on one handle: the same call three times, after release_scratch(), a sizing call of capacity 1 in front of
  the full call, a count call in front of a match call, a small batch between two large ones;
- a capacity so small that a chunk's region overflows and the host repeats the call with larger regions.

(A workgroup that loops over several tiles -- the round count runs on over them -- needs more than 32 MiB: that is
test_gpu_trip_trim.py's one-workgroup case.)"""
import random

import numpy as np
import pytest

import pyoracle as orc
from aha_amd import AC, AhaError
from aha_amd import _native as N
from engine_variants import use_variant

pytestmark = pytest.mark.gpu

S_MIN = 64        # the smallest chunk: keys of at most 8 bytes
GROUP = 64 * S_MIN
MAX_S = 32768
THREADS = 1024

_CACHE = {}


def cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


CJK = "中国人大学生日本語文字東京北海道"
CYR = "абвгдежзиклмнопрст"
LAT = "abcde"


def key_list():
    rng = random.Random(11)
    keys = {(x + y).encode() for x in LAT for y in LAT}  # every two-letter key: events are dense
    while len(keys) < 25 + 300:
        kind = rng.randrange(4)
        if kind == 0:
            k = "".join(rng.choice(CJK) for _ in range(rng.randint(1, 2)))
        elif kind == 1:
            k = "".join(rng.choice(CYR) for _ in range(rng.randint(1, 4)))
        elif kind == 2:
            k = "".join(rng.choice(LAT + "xyz") for _ in range(rng.randint(3, 8)))
        else:
            k = rng.choice(CJK) + rng.choice(LAT) + rng.choice(CYR)
        assert len(k.encode()) <= 8
        keys.add(k.encode())
    return sorted(keys)


def packed():
    def make():
        blob, offs = orc.pack_keys(key_list())
        return np.asarray(blob), np.asarray(offs, dtype=np.uint64)
    return cached("keys", make)


def mixed_text(n, seed):
    rng = random.Random(seed)
    parts, size = [], 0
    alphabet = [c.encode() for c in LAT * 6 + CJK + CYR + "xyz q\n"] + [b"\xe4\xb8", b"\x80", b"\xff"]  # (and broken units)
    while size < n:
        p = rng.choice(alphabet)
        parts.append(p)
        size += len(p)
    return np.frombuffer(b"".join(parts)[:n], dtype=np.uint8).copy()


def static_chunk(n_bytes, grid):
    """engine.cpp plan_v2: the text over the grid's lanes, in 64s, s_min at least"""
    lanes = grid * THREADS
    return min(max(S_MIN, -(-(-(-n_bytes // lanes)) // 64) * 64), MAX_S)


def batch_of(n_groups, rem):
    """n_groups groups of 4 KiB, the last one of `rem` pieces of 64 bytes, the last piece five bytes short"""
    return mixed_text(((n_groups - 1) * 64 + rem) * S_MIN - 5, 100 * n_groups + rem)


def group_batches():
    def make():
        t = {}
        for n_groups, rem in ((1, 1), (1, 63), (15, 63), (16, 1), (17, 63), (33, 1), (16 * 5 + 1, 63)):
            text = batch_of(n_groups, rem)
            n = text.size
            t["g%d-%d" % (n_groups, rem)] = (text, np.array([0, n // 3, n // 3 + 1, n], dtype=np.uint64))
        return t
    return cached("group-batches", make)


def boundary_batch(grid):
    def make():
        text = batch_of(33, 1)
        n = text.size
        wave_bytes = 64 * static_chunk(n, grid)  # the text of one wave
        last = n // wave_bytes
        assert last >= 10
        cuts = {0, n}
        for g, d in ((1, 0), (2, -1), (3, 1), (5, 0), (5, 1), (6, -1), (last, 0), (last, -1), (last, 1)):
            cuts.add(g * wave_bytes + d)
        # (one document from wave 6 to the last one; empty documents at the very start and the very end)
        doc = np.array(sorted([0, 0] + sorted(cuts) + [6 * wave_bytes - 1, n, n]), dtype=np.uint64)
        return text, doc
    return cached(("boundaries", grid), make)


def uneven_batch():
    def make():
        n_chunks = 16 * 64
        text = np.full(n_chunks * S_MIN, ord("q"), dtype=np.uint8)
        ab = np.frombuffer(b"ab" * (S_MIN // 2), dtype=np.uint8)
        for c in range(0, n_chunks, 8):  # every eighth chunk reports at (almost) every byte, the others never
            text[c * S_MIN:(c + 1) * S_MIN] = ab
        return text, np.array([0, 5 * GROUP + 7, text.size], dtype=np.uint64), n_chunks
    return cached("uneven", make)


def oracle(name, text, doc, chars):
    def make():
        o = cached("oracle", lambda: orc.AC.compile_packed(*packed()))
        oh, od = o.match_batch(text, doc, chars=chars, cap=4 * text.size + 1024)
        return oh.tobytes(), np.asarray(od, dtype=np.uint64), len(oh)
    return cached(("want", name, chars), make)


def run(g, text, doc, want, chars, cap=None):
    import torch

    raw, od, total = want
    cap = total + 4096 if cap is None else cap
    dc = torch.from_numpy(text).cuda()
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
    assert info["unit_enabled"] and info["max_key_len"] <= 8
    if variant in ("u", "uh"):
        assert info["unit_header_beside"] == (1 if variant == "uh" else 0)
    assert info["unit_base_bits"] == (23 if variant == "u23" else 22)
    return g


@pytest.fixture(params=["one-workgroup", "device"])
def grid(request, monkeypatch):
    """workgroups of the traversal"""
    import torch

    cus = torch.cuda.get_device_properties(0).multi_processor_count
    if request.param == "one-workgroup":
        monkeypatch.setenv("AHA_RESERVE_CUS", str(cus - 1))
        return 1
    monkeypatch.delenv("AHA_RESERVE_CUS", raising=False)
    return cus


@pytest.fixture
def engine(request, monkeypatch):
    return use_variant(request.param, monkeypatch)


def planned(t, n_bytes, grid):
    s = static_chunk(n_bytes, grid)
    assert t["engine"] == 4 and t["chunk_bytes"] == s and t["n_chunks"] == -(-n_bytes // s), (t, s)


VARIANTS = ["u", "u23", "uh", "ur"]


@pytest.mark.parametrize("chars", [False, True], ids=["bytes", "chars"])
@pytest.mark.parametrize("engine", VARIANTS, indirect=True)
def test_wave_counts_around_the_workgroup(engine, grid, chars):
    g = handle(engine)
    seen = set()
    for name, (text, doc) in group_batches().items():
        want = oracle(name, text, doc, chars)
        assert text.size < 1000 or want[2] > text.size // 4  # events are dense
        t = run(g, text, doc, want, chars)
        planned(t, text.size, grid)
        assert t["repeats"] == 0, (name, t)
        seen.add((t["chunk_bytes"], -(-t["n_chunks"] // 64)))
    if grid == 1:  # chunks and live waves: one wave, fifteen and sixteen at the smallest chunk, then larger chunks
        assert seen == {(64, 1), (64, 15), (64, 16), (128, 9), (192, 11), (384, 14)}, seen
    else:
        assert {s for s, _ in seen} == {64} and max(w for _, w in seen) == 81


@pytest.mark.parametrize("chars", [False, True], ids=["bytes", "chars"])
@pytest.mark.parametrize("engine", VARIANTS, indirect=True)
def test_document_boundaries_between_waves(engine, grid, chars):
    g = handle(engine)
    text, doc = boundary_batch(grid)
    assert doc[0] == doc[1] == 0 and doc[-1] == doc[-2] == text.size
    assert int(np.diff(doc.astype(np.int64)).max()) >= 4 * 64 * static_chunk(text.size, grid)
    planned(run(g, text, doc, oracle(("boundaries", grid), text, doc, chars), chars), text.size, grid)


@pytest.mark.parametrize("chars", [False, True], ids=["bytes", "chars"])
@pytest.mark.parametrize("engine", VARIANTS, indirect=True)
def test_call_sequences_on_one_handle(engine, grid, chars):
    import torch

    g = handle(engine)
    text, doc = group_batches()["g81-63"]
    want = oracle("g81-63", text, doc, chars)
    for _ in range(3):
        planned(run(g, text, doc, want, chars), text.size, grid)
    g.release_scratch()
    planned(run(g, text, doc, want, chars), text.size, grid)
    # a sizing call (capacity 1), then the full call with exactly what it asked for
    dc, dd = torch.from_numpy(text).cuda(), torch.from_numpy(doc.astype(np.int64)).cuda()
    one = torch.full((1 + 8, 3), -7, dtype=torch.int32, device="cuda")
    with pytest.raises(AhaError) as e:
        g.match_batch_device(dc, dd, one[:1], None, chars=chars)
    assert e.value.code == N.AHA_E_CAPACITY and e.value.required == want[2]
    assert bool((one[1:] == -7).all())
    run(g, text, doc, want, chars, cap=want[2])
    # a count call, then a match call
    v = np.frombuffer(want[0], dtype=np.int32).reshape(-1, 3)[:, 2]
    K = g.n_keys
    kc = torch.zeros(K, dtype=torch.int64, device="cuda")
    dho = torch.zeros(doc.size, dtype=torch.int64, device="cuda")
    assert g.count_batch_device(dc, dd, kc, dho, chars=chars) == want[2]
    assert np.array_equal(kc.cpu().numpy(), np.bincount(v, minlength=K)) and np.array_equal(dho.cpu().numpy().astype(np.uint64), want[1])
    planned(run(g, text, doc, want, chars), text.size, grid)
    small, sdoc = group_batches()["g15-63"]
    planned(run(g, small, sdoc, oracle("g15-63", small, sdoc, chars), chars), small.size, grid)
    planned(run(g, text, doc, want, chars), text.size, grid)


@pytest.mark.parametrize("chars", [False, True], ids=["bytes", "chars"])
@pytest.mark.parametrize("engine", VARIANTS, indirect=True)
def test_region_overflow_repeats_the_call(engine, grid, chars):
    """An exact capacity over a text whose hits sit in every eighth chunk: the regions hold twice the average + 16 events, a
    reporting chunk sends more -- cursor[1] = 2, and the host repeats the call with full-size regions."""
    g = handle(engine)
    text, doc, n_chunks = uneven_batch()
    want = oracle("uneven", text, doc, chars)
    assert 2 * (want[2] // n_chunks) + 16 < 32
    t = run(g, text, doc, want, chars, cap=want[2])
    planned(t, text.size, grid)
    assert t["n_chunks"] == n_chunks and t["repeats"] == 1, t
    planned(run(g, text, doc, want, chars, cap=want[2]), text.size, grid)  # and once more on the same handle
