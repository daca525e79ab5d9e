"""Call sequences on ONE handle, every call against the CPU oracle.

A handle carries state from one call to the next: each leased scratch set keeps its buffers, and v2buf[kCursor] holds two
blocks of counter words -- a call counts in one of them and its last kernel clears the other for the call behind it
(engine.cpp, match_v2); calls that do not publish leave the block dirty, hand-backs retry on the same set, and
release_scratch frees the buffers.  The parity suite compiles fresh handles and makes a call or two on each, so none of
that is exercised there.  Here one handle per engine variant and key set walks through every ordered pair of call kinds
(a de Bruijn walk), and each call is checked bit-exact: hit triples in order, per-document offsets, and the rows and
entries behind what the call may write still hold their sentinels."""
import ctypes as C
import gc
import random
import threading
import time

import numpy as np
import pytest

import grepsim
import pyoracle as orc
import replacesim
import selectsim
from aha_amd import AC, AhaError, BitArray, DeviceBuffer
from aha_amd import _native as N
from aha_amd.ac import _params
from walksim import (ENGINE_VARS, PAD, S32, S64, VARIANTS, Text, ascii_keys, cjk_keys, compile_under, de_bruijn_walk)
from walksim import check_dev as _check_dev, check_dho as _check_dho, check_np as _check_np, dho_dev as _dho_dev, hits_np as _hits_np

pytestmark = pytest.mark.gpu

HOST, DEV_DHO, DEV_NODHO, STREAM, KEEP, CHARS, SEP, LONG1, LONG2, SINGLE, CAP, BADOFF, EMPTY, UNALIGNED, RELEASE, PROFILE = range(16)
KIND_NAMES = ["host", "dev_dho", "dev_nodho", "stream", "keep", "chars", "sep", "longest1", "longest2", "single", "capacity",
              "bad_offsets", "empty", "unaligned", "release", "profiling"]
K = len(KIND_NAMES)
ZERO_HIT_KINDS = {EMPTY}          # their count is 0 whatever the text
NO_DOC_KINDS = {SINGLE}           # one sequence, no document offsets
TIMED = {HOST, DEV_DHO, DEV_NODHO, STREAM, KEEP, CHARS, SEP, SINGLE, UNALIGNED, PROFILE}  # match_longest and empty batches publish no timing

SEP_BITS = [32]                   # a space separates


# ---- key sets and their texts ------------------------------------------------

def _docs(rng, tokens, sep, shape, density, fill):
    out = []
    for n in shape:
        out.append(sep.join(rng.choice(tokens) if rng.random() < density else rng.choice(fill) for _ in range(n)))
    return out


def _pool(rng, tokens, sep, fill, extra=()):
    """Five texts of different size, document count and density (plus extras): consecutive calls can always pick a
    text whose count and document count differ from the call before."""
    return [
        Text(_docs(rng, tokens, sep, [300] * 12, 0.05, fill)),
        Text(_docs(rng, tokens, sep, [60] * 40, 0.3, fill)),
        Text(_docs(rng, tokens, sep, [8000] * 3, 0.6, fill)),
        Text(_docs(rng, tokens, sep, [200, 0, 200, 0, 200, 200, 200], 0.2, fill)),
        Text(_docs(rng, tokens, sep, [rng.randint(0, 8) for _ in range(100)], 0.5, fill)),
    ] + list(extra)


def _ascii_set():
    """(a) a keyword list of ASCII keys of 3 to 64 bytes (the prefix-filter engine's) over text with a few non-ASCII
    characters; keys nested six deep on one walk and a document dense with them: kf_walk hands the batch back."""
    rng = random.Random(31)
    keys, nested = ascii_keys(rng)
    fill = ["zz", "é", "ü9", "0", "mn"]
    dense = Text(["qrstuvwxy " * 3000, "ab qrstuvwxy", "é" * 40 + "qrstuvwxy" * 700])
    return keys, _pool(rng, keys + nested * 4, " ", fill, [dense])


def _cjk_set():
    """(b) CJK / mixed UTF-8 keys of 1 to 4 characters: the character-level image (engine 4) under `auto`."""
    rng = random.Random(32)
    keys, cps = cjk_keys(rng)
    fill = ["ä", "ß", "\U0001F600", "x", "é"]
    return keys, _pool(rng, cps + keys + [" "] * 20, "", fill)


def _nested_set():
    """(c) a small nested alphabet: long output chains, the dense expansion, a batch whose hits crowd the first chunks (a
    region overflows for a capacity near the count: the repeated pass) and, for the capacity kind, 3 MB of "a" (more events
    than the slab pipeline's temp holds: the two-pass engine counts)."""
    rng = random.Random(33)
    keys = ["a", "aa", "ab", "b", "中", "中国"]
    fill = ["x", " ", "y"]
    crowd = Text([("ab" * 20000 + "中国" * 20000), "x" * 3_000_000])
    return keys, _pool(rng, ["a", "b", "中", "国", "aa", "ab", " "], "", fill, [crowd])


KEY_SETS = {"ascii": _ascii_set, "cjk": _cjk_set, "nested": _nested_set}
_SETS = {}
_ORACLE = {}


def key_set(name):
    if name not in _SETS:
        keys, texts = KEY_SETS[name]()
        _SETS[name] = (keys, texts, orc.AC.compile(keys))
    return _SETS[name]


def expect(name, ti, flag, text=None):
    """The oracle's (hits, per-document offsets) of text ti of key set `name`, cached per (key set, text, flag)."""
    key = (name, ti, flag)
    if key not in _ORACLE:
        _, texts, o = key_set(name)
        t = text if text is not None else texts[ti]
        if flag in ("plain", "chars"):
            h, d = o.match_batch(t.corpus, t.offs, chars=flag == "chars")
        elif flag == "single":
            h, d = o.match(t.corpus.tobytes(), chars=False), None
        else:
            parts = []
            for doc in t.docs:
                if flag == "sep":
                    parts.append(o.match(doc, chars=False, sep=(256, SEP_BITS)))
                else:
                    parts.append(o.match_longest(doc, flag == "long2", chars=False))
            d = np.cumsum([0] + [len(p) for p in parts]).astype(np.uint64)
            h = np.concatenate(parts) if parts else np.zeros(0, dtype=orc.HIT_DTYPE)
        _ORACLE[key] = (np.ascontiguousarray(h, dtype=orc.HIT_DTYPE), d)
    return _ORACLE[key]


FLAG_OF = {HOST: "plain", DEV_DHO: "plain", DEV_NODHO: "plain", STREAM: "plain", KEEP: "plain", CHARS: "chars", SEP: "sep",
           LONG1: "long1", LONG2: "long2", SINGLE: "single", CAP: "plain", BADOFF: "plain", UNALIGNED: "plain",
           PROFILE: "plain"}


def expected_nd(name, kind, ti):
    h, _ = expect(name, ti, FLAG_OF[kind])
    return len(h), (None if kind in NO_DOC_KINDS else key_set(name)[1][ti].D)


def plan_walk(name):
    """The walk for key set `name`: (kind, text index) per step.  Consecutive successful calls differ in hit count
    (unless both are empty-batch calls, which have none) and in document count (unless both are single sequences); the
    text rotates over the pool so every text meets every transition."""
    walk = de_bruijn_walk(K)
    pairs = set(zip(walk, walk[1:]))
    assert len(walk) == K * K + 1 and pairs == {(a, b) for a in range(K) for b in range(K)}, "the walk misses a pair"
    texts = key_set(name)[1]
    plan, last, rot = [], None, 0
    n_empty = 0
    for kind in walk:
        if kind == RELEASE:
            plan.append((kind, None))
            continue
        if kind == EMPTY:  # no text: a batch of no document, or of five empty ones, by turns (D = 0 or 5)
            D = 5 * (n_empty % 2)
            n_empty += 1
            assert all(t.D not in (0, 5) for t in texts)
            plan.append((kind, D))
            last = (0, D, kind)
            continue
        chosen = None
        for j in range(len(texts)):
            ti = (rot + j) % len(texts)
            if name == "nested" and ti == len(texts) - 1 and kind not in (DEV_DHO, DEV_NODHO, CAP):
                continue  # (the 3 MB text: through the device entry, where a capacity near the count makes a region overflow)
            if kind in (BADOFF, CAP):
                chosen = ti
                break
            n, D = expected_nd(name, kind, ti)
            if n == 0:
                continue  # (a zero count would not tell a stale counter from a fresh one)
            if last is not None:
                ln, lD, lk = last
                if n == ln and not (kind in ZERO_HIT_KINDS and lk in ZERO_HIT_KINDS):
                    continue
                if D == lD and not (kind in NO_DOC_KINDS and lk in NO_DOC_KINDS):
                    continue
            chosen = ti
            break
        assert chosen is not None, (name, kind, last)
        rot += 1
        plan.append((kind, chosen))
        if kind not in (BADOFF, CAP):
            n, D = expected_nd(name, kind, chosen)
            last = (n, D, kind)
    return plan


# ---- one call of each kind ---------------------------------------------------

def _host_batch(g, t, cap, chars=False, sep=None, longest=0, keep=None):
    """aha_ac_match_batch / _keep on the caller's own buffers (prefilled with sentinels)."""
    p = _params(chars, sep, longest)
    out = _hits_np(cap)
    dho = np.full(t.D + 1 + PAD, S64, dtype=np.uint64)
    n = C.c_uint64(0)
    cp = t.corpus.ctypes.data if t.corpus.size else None
    if keep is None:
        rc = N.lib().aha_ac_match_batch(g._h, cp, t.offs.ctypes.data, t.D, C.byref(p), out.ctypes.data, cap,
                                        dho.ctypes.data, C.byref(n))
    else:
        rc = N.lib().aha_ac_match_batch_keep(g._h, cp, t.offs.ctypes.data, t.D, C.byref(p), keep.data_ptr(), cap,
                                             dho.ctypes.data, C.byref(n))
    return rc, int(n.value), out, dho


def _sep():
    s = BitArray(256)
    for b in SEP_BITS:
        s[b] = True
    return s


def run_kind(g, name, kind, ti, st, state):
    """One step: the call, every check; returns (n, D) of a successful match call, else None."""
    import torch

    keys, texts, o = key_set(name)
    t = texts[ti] if ti is not None and kind != EMPTY else None  # (an empty-batch step carries its document count)
    stream = st.cuda_stream

    def device_call(chars=False, dho=True, words=False, unaligned=False, cap_rows=None, offs=None, text=None):
        tt = text or t
        want, want_off = expect(name, ti, "chars" if chars else "plain")
        cap = cap_rows if cap_rows is not None else len(want) + 37
        with torch.cuda.stream(st):
            dc, dd = tt.dev()
            if offs is not None:
                dd = offs
            if unaligned:
                holder = torch.full((tt.corpus.size + 64,), 0xEE, dtype=torch.uint8, device="cuda")
                dc_u = holder[1:1 + tt.corpus.size]
                dc_u.copy_(dc)
                assert dc_u.data_ptr() % 16 == 1
                dc = dc_u
            big = torch.full((cap + PAD, 3), S32, dtype=torch.int32, device="cuda")
            d_dho = _dho_dev(tt.D) if dho else None
            w = nw = None
            if words:
                w = torch.full((2 * cap + cap // 1024 + 2,), S32, dtype=torch.int32, device="cuda")
                nw = torch.zeros(1, dtype=torch.int64, device="cuda")
        st.synchronize()
        err = None
        try:
            n = g.match_batch_device(dc, dd, big[:cap], d_dho, chars=chars, stream=stream, words=w, n_words=nw)
        except AhaError as e:
            err, n = e, None
        return dict(err=err, n=n, big=big, dho=d_dho, cap=cap, want=want, want_off=want_off, words=w, n_words=nw)

    if kind == RELEASE:
        g.release_scratch()
        assert g.scratch_bytes() == 0
        return None
    if kind == PROFILE:
        state["prof"] = not state["prof"]
        g.set_profiling(state["prof"])
        kind = DEV_DHO  # ... and a device call right behind it (the first profiled call on a set creates its events)
    if kind in (HOST, SEP, LONG1, LONG2):
        flag = FLAG_OF[kind]
        want, want_off = expect(name, ti, flag)
        cap = len(want) + 37
        rc, n, out, dho = _host_batch(g, t, cap, sep=_sep() if kind == SEP else None,
                                      longest={LONG1: 1, LONG2: 2}.get(kind, 0))
        assert rc == N.AHA_OK, (rc, N.lib().aha_last_error(g._h))
        _check_np(out, n, want, n)
        _check_dho(dho, t.D, want_off)
        return n, t.D
    if kind == KEEP:
        want, want_off = expect(name, ti, "plain")
        cap = len(want) + 37
        with torch.cuda.stream(st):
            big = torch.full((cap + PAD, 3), S32, dtype=torch.int32, device="cuda")
        st.synchronize()
        rc, n, _, dho = _host_batch(g, t, cap, keep=big)
        assert rc == N.AHA_OK, (rc, N.lib().aha_last_error(g._h))
        _check_dev(big, n, want, n)
        _check_dho(dho, t.D, want_off)
        return n, t.D
    if kind == SINGLE:
        want, _ = expect(name, ti, "single")
        cap = len(want) + 37
        out = _hits_np(cap)
        n = C.c_uint64(0)
        p = _params(False, None)
        rc = N.lib().aha_ac_match_bytes(g._h, t.corpus.ctypes.data, t.corpus.size, C.byref(p), out.ctypes.data, cap,
                                        C.byref(n))
        assert rc == N.AHA_OK, (rc, N.lib().aha_last_error(g._h))
        _check_np(out, int(n.value), want, int(n.value))
        return int(n.value), None
    if kind in (DEV_DHO, DEV_NODHO, STREAM, CHARS, UNALIGNED):
        r = device_call(chars=kind == CHARS, dho=kind != DEV_NODHO, words=kind == STREAM, unaligned=kind == UNALIGNED)
        assert r["err"] is None, (r["err"], r["err"].code)
        n = r["n"]
        _check_dev(r["big"], n, r["want"], n)
        if r["dho"] is not None:
            _check_dho(r["dho"], t.D, r["want_off"])
        if kind == STREAM:  # the 4-byte exchange stream of the same call, unpacked again
            with torch.cuda.stream(st):
                back = torch.full((n + 1, 3), S32, dtype=torch.int32, device="cuda")
                g.hits_unpack4_device(r["words"], n, back, stream=stream)
            st.synchronize()
            assert n == 0 or int(r["n_words"].item()) > 0
            assert back[:n].cpu().numpy().tobytes() == r["want"].tobytes()
        return n, t.D
    if kind == CAP:
        state["caps"] = state.get("caps", 0) + 1
        if name == "nested" and state["caps"] % 2 == 0:
            # 3 MB of "a" and room for 4 hits: more events than the slab pipeline's temp -- the count comes from the two-pass engine
            big_t = state.setdefault("aaa", np.full(3_000_000, ord("a"), dtype=np.uint8))
            out = _hits_np(4)
            n = C.c_uint64(0)
            rc = N.lib().aha_ac_match_bytes(g._h, big_t.ctypes.data, big_t.size, None, out.ctypes.data, 4, C.byref(n))
            assert rc == N.AHA_E_CAPACITY and n.value == 2 * big_t.size - 1
            assert out[:4].tolist() == [(0, 1, 0), (0, 2, 1), (1, 2, 0), (1, 3, 1)]
            assert (out[4:]["end"] == S32).all()
            return None
        want, _ = expect(name, ti, "plain")
        cap = [len(want) - 1, len(want) // 2, 3][state["caps"] % 3]
        r = device_call(cap_rows=max(cap, 0))
        assert r["err"] is not None and r["err"].code == N.AHA_E_CAPACITY, r["err"]
        assert r["err"].required == len(want)
        assert bool((r["big"][r["cap"]:] == S32).all())  # nothing at or beyond cap
        return None
    if kind == BADOFF:
        state["bad"] = state.get("bad", 0) + 1
        offs = t.offs.astype(np.int64).copy()
        which = state["bad"] % 4
        if which == 0:
            offs[0] = 1
        elif which == 1:
            offs[-1] -= 1
        elif which == 2:
            offs[1] = offs[-1] + 44
        else:
            offs[1] = 1 << 40
        with torch.cuda.stream(st):
            bad = torch.from_numpy(offs).cuda()
        r = device_call(offs=bad)
        assert r["err"] is not None and r["err"].code == N.AHA_E_INVALID, r["err"]
        assert bool((r["big"] == S32).all())  # nothing indexed with the bad offsets
        assert bool((r["dho"] == S64 - (1 << 64)).all())
        return None
    if kind == EMPTY:
        if ti == 0:
            e = Text([])  # no document at all: the host entry
            rc, n, out, dho = _host_batch(g, e, 16)
            assert rc == N.AHA_OK and n == 0
            _check_np(out, 0, np.zeros(0, dtype=orc.HIT_DTYPE), 0)
            _check_dho(dho, 0, np.zeros(1, dtype=np.uint64))
            return 0, 0
        with torch.cuda.stream(st):  # only empty documents: the device entry
            dc = torch.zeros(16, dtype=torch.uint8, device="cuda")[:0]
            dd = torch.zeros(6, dtype=torch.int64, device="cuda")
            big = torch.full((16 + PAD, 3), S32, dtype=torch.int32, device="cuda")
            dho = _dho_dev(5)
        st.synchronize()
        assert g.match_batch_device(dc, dd, big[:16], dho, stream=stream) == 0
        _check_dev(big, 0, np.zeros(0, dtype=orc.HIT_DTYPE), 0)
        _check_dho(dho, 5, np.zeros(6, dtype=np.uint64))
        return 0, 5
    raise AssertionError(kind)


def multi_range_call(g, name):
    """One host call above the host entry's range (64 MiB, capi.cpp kHostRange) made of small documents: two ranges run
    back to back on one scratch set, so the counter block changes halves inside one API call."""
    keys, texts, o = key_set(name)
    rng = random.Random(44)
    pieces = [d for t in texts[:5] for d in t.docs if d]
    doc_bytes = 4096
    n_docs = (68 << 20) // doc_bytes
    filler = b"\x01" * doc_bytes
    docs = []
    for i in range(n_docs):
        p = pieces[rng.randrange(len(pieces))][:200] if i % 3 == 0 else b""
        docs.append(p + filler[: doc_bytes - len(p)])
    t = Text(docs)
    want, want_off = expect(name, "multi", "plain", text=t)
    rc, n, out, dho = _host_batch(g, t, len(want) + 37)
    assert rc == N.AHA_OK, (rc, N.lib().aha_last_error(g._h))
    _check_np(out, n, want, n)
    _check_dho(dho, t.D, want_off)


@pytest.mark.parametrize("name", list(KEY_SETS))
@pytest.mark.parametrize("variant", list(VARIANTS))
def test_call_sequence_on_one_handle(variant, name, monkeypatch):
    """Every ordered pair of call kinds on one handle, each call against the oracle; with profiling on, aha_timing.n_hits is
    the call's own count (not the call's before it)."""
    import torch

    keys, _, _ = key_set(name)
    g = compile_under(monkeypatch, variant, keys)
    plan = plan_walk(name)
    st = torch.cuda.Stream()
    state = {"prof": False}
    t0 = time.perf_counter()
    for i, (kind, ti) in enumerate(plan):
        if variant == "auto" and i == len(plan) // 2:
            multi_range_call(g, name)
        try:
            res = run_kind(g, name, kind, ti, st, state)
        except AssertionError as e:
            raise AssertionError(f"step {i} ({KIND_NAMES[kind]}, text {ti}) after {KIND_NAMES[plan[i - 1][0]] if i else '-'}: {e}") from e
        if res is not None and state["prof"] and kind in TIMED:
            assert g.last_timing()["n_hits"] == res[0], (i, KIND_NAMES[kind])
    print(f"{variant}/{name}: {len(plan)} steps in {time.perf_counter() - t0:.1f} s")


def test_release_resets_the_counter_block(monkeypatch):
    """release_scratch frees the counter block; the block the next call allocates -- possibly at the same address -- holds
    words nobody knows and must be cleared, whatever the call before the release left behind.  The blocks freed just before
    the call hold a bad-offsets verdict (17) in cursor[1] of both halves: every kernel of the region pipelines returns on a
    non-zero cursor[1] before it touches anything else, so a call that trusted the stale block is refused (AHA_E_INVALID)
    instead of writing anywhere."""
    keys, texts, _ = key_set("cjk")
    g = compile_under(monkeypatch, "auto", keys)
    t = texts[1]
    want, want_off = expect("cjk", 1, "plain")

    def call():
        rc, n, out, dho = _host_batch(g, t, len(want) + 37)
        assert rc == N.AHA_OK, (rc, N.lib().aha_last_error(g._h))
        _check_np(out, n, want, n)
        _check_dho(dho, t.D, want_off)

    call()  # a publishing call: it clears the other half and leaves the block clean
    g.release_scratch()
    assert g.scratch_bytes() == 0
    words = (3 * 16 * 8 + 3 * 16 * 8 // 8 + 256) // 8  # what v2_reserve(kCursor, kCursorBytes) allocates: 688 bytes
    poison = np.zeros(words, dtype=np.uint64)
    poison[1] = poison[17] = 17
    bufs = [DeviceBuffer(0, words * 8) for _ in range(16)]
    for b in bufs:
        b.upload(poison)
    del bufs, b
    gc.collect()
    call()


def test_calls_on_one_handle_beside_release(monkeypatch):
    """Two threads run call sequences of their own on one handle (each lease its own scratch set) while a third releases
    the scratch between their calls: every result is the oracle's, and only the steps that expect an error fail."""
    import torch

    keys, texts, _ = key_set("ascii")
    g = compile_under(monkeypatch, "auto", keys)
    kinds = [HOST, DEV_DHO, DEV_NODHO, CHARS, SEP, LONG1, SINGLE, UNALIGNED, STREAM, KEEP, CAP, BADOFF, EMPTY, LONG2]
    for ti in range(5):  # oracle answers and device copies ahead of the threads
        for f in ("plain", "chars", "sep", "long1", "long2", "single"):
            expect("ascii", ti, f)
        texts[ti].dev()
    torch.cuda.synchronize()
    errs, done, counts = [], threading.Event(), [0, 0, 0]
    deadline = time.perf_counter() + 25

    def work(w):
        try:
            st = torch.cuda.Stream()
            state = {"prof": False}
            rng = random.Random(70 + w)
            for r in range(6):
                order = kinds[:]
                rng.shuffle(order)
                for i, kind in enumerate(order):
                    run_kind(g, "ascii", kind, (i + r + w) % 5, st, state)
                    counts[w] += 1
                if time.perf_counter() > deadline:
                    break
        except Exception as e:  # noqa: BLE001
            errs.append((w, repr(e)))

    def releaser():
        while not done.is_set():
            g.release_scratch()
            counts[2] += 1
            time.sleep(0.003)

    ths = [threading.Thread(target=work, args=(w,)) for w in (0, 1)]
    rel = threading.Thread(target=releaser)
    rel.start()
    for th in ths:
        th.start()
    for th in ths:
        th.join()
    done.set()
    rel.join()
    assert not errs, errs
    assert counts[0] >= len(kinds) and counts[1] >= len(kinds) and counts[2] > 1, counts


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_separator_at_a_document_end_on_a_piece_boundary(variant, monkeypatch):
    """match(seq, sep) in a batch: a hit that ends its document has no right neighbour (src/aha/ac.cr:324-329, documents are
    independent: ac.cr:177).  The single-traversal engine stages the text in pieces of 32 bytes and flags an event as its
    document's last by the boundary's offset inside the piece -- a document that ends exactly at the piece's end has none
    there, so the flag must come from the absolute offsets, or the next document's first byte (or the byte behind the text)
    is taken for the neighbour and the hit is dropped."""
    keys = ["ab", "b", "abc"]
    g = compile_under(monkeypatch, variant, keys)
    o = orc.AC.compile(keys)
    docs = [b"ab" + b" " * 28 + b"ab"] * 6 + [b"ab" + b" " * 60 + b"ab", b"b" * 32, b"", b"ab " + b" " * 90 + b"abc"] + \
           [b"ab" + b" " * 28 + b"ab"] * 3
    t = Text(docs)
    assert all(int(x) % 32 == 0 for x in t.offs)  # every document ends on a piece boundary, the last one at the text's end
    want, want_off = [], [0]
    for d in docs:
        h = o.match(d, chars=False, sep=(256, SEP_BITS))
        want.append(h)
        want_off.append(want_off[-1] + len(h))
    want = np.concatenate(want)
    rc, n, out, dho = _host_batch(g, t, len(want) + 8, sep=_sep())
    assert rc == N.AHA_OK
    _check_np(out, n, want, n)
    _check_dho(dho, t.D, np.array(want_off, dtype=np.uint64))


# ---- the scratch allocator's contract, family by family ---------------------------------------------------------------

def _alloc_input():
    """About 40 ASCII keys of 3 to 8 bytes in mixed case, a batch of 256 KiB in about 1000 documents, and its first half
    (whole documents) as the smaller batch: whatever is cut into ranges of documents starts with the same ranges."""
    rng = random.Random(77)
    keys = set()
    while len(keys) < 40:
        keys.add("".join(rng.choice("abcdeFGH") for _ in range(rng.randint(3, 8))))
    keys = sorted(keys)
    words = keys + [k.swapcase() for k in keys[:10]] + ["zz", "q", "tuvwxyz", "0123", "mnop qr"]
    docs, total = [], 0
    while total < 256 << 10:
        n = rng.randint(180, 345)
        d = ""
        while len(d) < n:
            d += rng.choice(words) + rng.choice([" ", "", "-"])
        docs.append(d[:n])
        total += n
    half, acc = 0, 0
    while acc < total // 2:
        acc += len(docs[half])
        half += 1
    return keys, Text(docs), Text(docs[:half])


class _ModelAnswers:
    """What every call kind returns for one batch, from ONE pass of tests/pymodel.py over its documents."""

    def __init__(self, model, t, fold, n_keys, repl):
        from aha_amd.ac import HIT_DTYPE, KEY_COUNT_DTYPE

        hits, pairs, self.dho, self.dpo = [], [], [0], [0]
        sep_hits, self.sep_pho = [], [0]
        covered = np.zeros(t.corpus.size, dtype=np.bool_)
        self.doc_covered = np.zeros(t.D, dtype=np.uint64)
        for d, doc in enumerate(t.docs):
            h = model.match(doc.lower() if fold else doc, chars=False)
            base = int(t.offs[d])
            for s, e, _ in h:
                covered[base + s:base + e] = True
            self.doc_covered[d] = covered[base:base + len(doc)].sum()
            hits += h
            per_key = np.bincount([v for _, _, v in h], minlength=n_keys)
            pairs += [(k, int(c)) for k, c in enumerate(per_key) if c]
            self.dho.append(len(hits))
            self.dpo.append(len(pairs))
            # a first piece on a feed with a separator filter: the surviving hits that end before the piece's last byte
            sep_hits += [x for x in model.match(doc.lower() if fold else doc, sep=(256, ALLOC_SEP), chars=False) if x[1] < len(doc)]
            self.sep_pho.append(len(sep_hits))
        self.hits = np.array(hits, dtype=HIT_DTYPE)
        self.pairs = np.array(pairs, dtype=KEY_COUNT_DTYPE)
        self.key_counts = np.bincount(self.hits["value"], minlength=n_keys).astype(np.uint64)
        self.dho = np.array(self.dho, dtype=np.uint64)
        self.dpo = np.array(self.dpo, dtype=np.uint64)
        self.n_covered = int(covered.sum())
        self.mask = np.packbits(np.concatenate([covered, np.zeros(-covered.size % 32, dtype=np.bool_)]),
                                bitorder="little").view(np.uint32)
        self.redacted = np.where(covered, np.uint8(0x2A), t.corpus)
        # select, replace, records and grep over the same hit list
        self.sel, self.dso = selectsim.select(self.hits, self.dho)
        self.rep, self.doo = replacesim.replace(t.corpus, t.offs, self.sel, self.dso, repl)
        self.rec, self.dro = grepsim.records(t.corpus, t.offs, b"\n")
        self.kept, self.kept_out, self.kept_doo = grepsim.grep(np.diff(self.dho.astype(np.int64)), t.offs, t.corpus, False)
        self.sep_hits = np.array(sep_hits, dtype=HIT_DTYPE)
        self.sep_pho = np.array(self.sep_pho, dtype=np.uint64)


_ALLOC = {}
ALLOC_SEP = [32, 45]              # a space and a hyphen separate (what _alloc_input joins its words with)


def _alloc_repl(keys):
    """grow, shrink, delete, same length, keep -- by the key's index"""
    repl = {}
    for i, k in enumerate(keys):
        r = [k + "++", "_", "", "#" * len(k), None][i % 5]
        if r is not None:
            repl[i] = r.encode()
    return repl


def _alloc_case(fold):
    from pymodel import ModelAC

    if "input" not in _ALLOC:
        _ALLOC["input"] = _alloc_input()
    keys, big, small = _ALLOC["input"]
    if fold not in _ALLOC:
        model = ModelAC([k.lower() for k in keys] if fold else keys)
        _ALLOC[fold] = tuple(_ModelAnswers(model, t, fold, len(keys), _alloc_repl(keys)) for t in (big, small))
    return keys, (big, small), _ALLOC[fold]


@pytest.mark.parametrize("fold", [False, True], ids=["plain", "fold_ascii"])
def test_scratch_only_grows_in_every_call_family(fold, monkeypatch):
    """The allocator's contract (capi.cpp reserve), for every family of scratch buffers a call kind touches: the result is
    the model's, a second identical call and a call on a smaller batch leave scratch_bytes() as it is (the buffers only
    grow), release_scratch() brings it to 0, and the call gives the right answer again on fresh buffers.

    Feed match, select and replace calls keep the rule for an identical call, not for the smaller batch: a feed matches its window batch into a hit buffer
    of its own that only grows (feed.cpp feed_windows), so the smaller batch's windows run with the larger batch's capacity;
    with a capacity above a hit per 4 bytes of text the match plans full-size event regions (engine.cpp plan_v2, `dense`), which
    the larger batch at the same capacity did not need.  Nothing is freed and nothing grows twice: what is asserted there is
    that scratch_bytes() does not shrink on the smaller batch and that the smaller and the larger batch again leave it where
    it then stands."""
    import torch

    keys, texts, answers = _alloc_case(fold)
    for v in ENGINE_VARS + ("AHA_COUNT_REGION_BYTES", "AHA_DOCCOUNT_HIT_BYTES", "AHA_SELECT_HIT_BYTES"):
        monkeypatch.delenv(v, raising=False)
    g = AC.compile(keys, fold_ascii=fold)
    monkeypatch.setenv("AHA_DOCCOUNT_HIT_BYTES", "4096")  # (read when the handle is compiled: ranges of ~340 hits)
    g_dc = AC.compile(keys, fold_ascii=fold)
    monkeypatch.delenv("AHA_DOCCOUNT_HIT_BYTES")
    monkeypatch.setenv("AHA_SELECT_HIT_BYTES", "4096")  # (the same for select and replace calls)
    g_sel = AC.compile(keys, fold_ascii=fold)
    monkeypatch.delenv("AHA_SELECT_HIT_BYTES")
    K = len(keys)
    repl = _alloc_repl(keys)
    tables, feeds = {}, {}

    def table_of(h):
        if id(h) not in tables:
            tables[id(h)] = h.replacements(repl)
        return tables[id(h)]

    def feed_of(h, sep=False):
        """a feed of the handle with a sequence per document of the larger batch, every sequence at length 0: document d is
        the first piece of sequence d, so the call is the same call every time.  What a Feed owns (its sequences' contexts,
        tails, cursors and open records: feed.cpp) is not the handle's scratch; what a feed call builds its answer in --
        fselbuf, frepbuf, fsepbuf, fgrpbuf and the families' own buffers -- is, and falls under the contract."""
        if (id(h), sep) not in feeds:
            b = None
            if sep:
                b = BitArray(256)
                for x in ALLOC_SEP:
                    b[x] = True
            feeds[(id(h), sep)] = h.feed(texts[0].D, sep=b)
        f = feeds[(id(h), sep)]
        f.reset()
        return f

    def ids_of(t):
        return torch.arange(t.D, dtype=torch.int32, device="cuda")

    def rows(n, width):
        return torch.full((n + PAD, width), S32, dtype=torch.int32, device="cuda")

    def raw(n):
        return torch.full((n + PAD,), 0x5A, dtype=torch.uint8, device="cuda")

    def check_raw(buf, n, want):
        got = buf.cpu().numpy()
        assert n == want.size and got[:n].tobytes() == want.tobytes() and (got[n:] == 0x5A).all()

    def zeros_then_sentinels(buf, D):
        got = buf.cpu().numpy()
        assert not got[:D].any() and (got[D:] == S64 - (1 << 64)).all()

    def i64(a):
        return a.cpu().numpy().astype(np.uint64)

    def unaligned(t):
        holder = torch.full((t.corpus.size + 64,), 0xEE, dtype=torch.uint8, device="cuda")
        view = holder[1:1 + t.corpus.size]
        view.copy_(t.dev()[0])
        assert view.data_ptr() % 16 == 1
        return view

    def dev_match(h, t, a, view=None):
        out = torch.full((len(a.hits) + 37, 3), S32, dtype=torch.int32, device="cuda")
        dho = _dho_dev(t.D)
        torch.cuda.synchronize()
        n = h.match_batch_device(view if view is not None else t.dev()[0], t.dev()[1], out, dho)
        _check_dev(out, n, a.hits, n)
        _check_dho(dho, t.D, a.dho)

    def dev_count(h, t, a, region_bytes=None):
        kc = torch.full((K,), -1, dtype=torch.int64, device="cuda")
        dho = _dho_dev(t.D)
        torch.cuda.synchronize()
        if region_bytes:  # (read by every pass: the full-size regions of more than a few documents do not fit)
            monkeypatch.setenv("AHA_COUNT_REGION_BYTES", str(region_bytes))
        try:
            n = h.count_batch_device(t.dev()[0], t.dev()[1], kc, dho)
        finally:
            monkeypatch.delenv("AHA_COUNT_REGION_BYTES", raising=False)
        assert n == len(a.hits) and np.array_equal(i64(kc), a.key_counts)
        _check_dho(dho, t.D, a.dho)

    def dev_doc_counts(h, t, a):
        out = torch.full((len(a.pairs) + 5, 2), S32, dtype=torch.int32, device="cuda")
        dpo = _dho_dev(t.D)
        torch.cuda.synchronize()
        n, nh = h.doc_counts_batch_device(t.dev()[0], t.dev()[1], out, dpo)
        assert (n, nh) == (len(a.pairs), len(a.hits))
        assert out[:n].cpu().numpy().tobytes() == a.pairs.tobytes() and bool((out[n:] == S32).all())
        _check_dho(dpo, t.D, a.dpo)

    def dev_cover(h, t, a, with_mask):
        mask = torch.full((a.mask.size,), -1, dtype=torch.int32, device="cuda") if with_mask else None
        red = torch.zeros(t.corpus.size, dtype=torch.uint8, device="cuda")
        cov = torch.full((t.D,), -1, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        nc, nh = h.cover_batch_device(t.dev()[0], t.dev()[1], mask=mask, redacted=red, doc_covered=cov)
        assert (nc, nh) == (a.n_covered, len(a.hits))
        assert np.array_equal(red.cpu().numpy(), a.redacted) and np.array_equal(i64(cov), a.doc_covered)
        if with_mask:
            assert np.array_equal(mask.cpu().numpy().view(np.uint32), a.mask)

    def dev_select(h, t, a):
        out, dso = rows(len(a.sel), 3), _dho_dev(t.D)
        torch.cuda.synchronize()
        n, nh = h.select_batch_device(t.dev()[0], t.dev()[1], out, dso, cap=len(a.sel))
        assert nh == len(a.hits)
        _check_dev(out, n, a.sel, n)
        _check_dho(dso, t.D, a.dso)

    def dev_replace(h, t, a):
        out, doo = raw(a.rep.size), _dho_dev(t.D)
        torch.cuda.synchronize()
        n, ns, nh = h.replace_batch_device(t.dev()[0], t.dev()[1], table_of(h), out, doo, cap=a.rep.size)
        assert (ns, nh) == (len(a.sel), len(a.hits))
        check_raw(out, n, a.rep)
        _check_dho(doo, t.D, a.doo)

    def dev_records(h, t, a):
        R = a.rec.size - 1
        rec, dro = _dho_dev(R), _dho_dev(t.D)
        torch.cuda.synchronize()
        assert h.records_device(t.dev()[0], t.dev()[1], rec, dro, cap=R) == R
        _check_dho(rec, R, a.rec)
        _check_dho(dro, t.D, a.dro)

    def dev_grep(h, t, a):
        nk = a.kept.size
        kept, doo, out = _dho_dev(nk - 1), _dho_dev(nk), raw(a.kept_out.size)
        torch.cuda.synchronize()
        got = h.grep_batch_device(t.dev()[0], t.dev()[1], kept, doo, out, cap_docs=nk, cap_bytes=a.kept_out.size)
        assert got == (nk, a.kept_out.size, len(a.hits))
        _check_dho(kept, nk - 1, a.kept)
        _check_dho(doo, nk, a.kept_doo)
        check_raw(out, got[1], a.kept_out)

    def host_select(h, t, a):
        sel, dso = h.select_batch(t.corpus, t.offs)
        assert sel.tobytes() == a.sel.tobytes() and np.array_equal(dso, a.dso)

    def host_replace(h, t, a):
        out, doo = h.replace_batch(t.corpus, t.offs, table_of(h))
        assert out.tobytes() == a.rep.tobytes() and np.array_equal(doo, a.doo)

    def host_records(h, t, a):
        rec, dro = h.records(t.corpus, t.offs)
        assert np.array_equal(rec, a.rec) and np.array_equal(dro, a.dro)

    def host_grep(h, t, a):
        kept, out, doo = h.grep_batch(t.corpus, t.offs)
        assert np.array_equal(kept, a.kept) and out.tobytes() == a.kept_out.tobytes() and np.array_equal(doo, a.kept_doo)

    def feed_match(h, t, a, sep=False):
        f = feed_of(h, sep)
        want, want_pho = (a.sep_hits, a.sep_pho) if sep else (a.hits, a.dho)
        out, pho, bases = rows(len(want), 3), _dho_dev(t.D), _dho_dev(t.D - 1)
        torch.cuda.synchronize()
        n = f.match_batch_device(t.dev()[0], t.dev()[1], ids_of(t), out[:len(want)], pho, bases)
        _check_dev(out, n, want, n)
        _check_dho(pho, t.D, want_pho)
        zeros_then_sentinels(bases, t.D)

    def feed_select(h, t, a):
        f = feed_of(h)
        out, pso, bases = rows(len(a.sel), 3), _dho_dev(t.D), _dho_dev(t.D - 1)
        torch.cuda.synchronize()
        n, nh = f.select_batch_device(t.dev()[0], t.dev()[1], ids_of(t), out, pso, bases, final=True, cap=len(a.sel))
        _check_dev(out, n, a.sel, n)
        _check_dho(pso, t.D, a.dso)
        zeros_then_sentinels(bases, t.D)

    def feed_replace(h, t, a):
        f = feed_of(h)
        out, poo, bases = raw(a.rep.size), _dho_dev(t.D), _dho_dev(t.D - 1)
        torch.cuda.synchronize()
        n, ns, nh = f.replace_batch_device(t.dev()[0], t.dev()[1], ids_of(t), table_of(h), out, poo, bases, final=True,
                                           cap=a.rep.size)
        assert ns == len(a.sel)
        check_raw(out, n, a.rep)
        _check_dho(poo, t.D, a.doo)
        zeros_then_sentinels(bases, t.D)

    def feed_grep(h, t, a):
        # (no document of this batch holds a line feed or is empty: under FINAL every piece is one record that closes)
        f = feed_of(h)
        nk = a.kept.size
        kept, roo, out = _dho_dev(nk - 1), _dho_dev(nk), raw(a.kept_out.size)
        torch.cuda.synchronize()
        got = f.grep_batch_device(t.dev()[0], t.dev()[1], ids_of(t), kept, roo, out, final=True, cap_recs=nk,
                                  cap_bytes=a.kept_out.size)
        assert got[:3] == (t.D, nk, a.kept_out.size), got
        _check_dho(kept, nk - 1, a.kept)
        _check_dho(roo, nk, a.kept_doo)
        check_raw(out, got[2], a.kept_out)

    def host_match_count(h, t, a):
        hits, dho = h.match_batch(t.corpus, t.offs, cap=len(a.hits) + 37)
        assert hits.tobytes() == a.hits.tobytes() and np.array_equal(dho, a.dho)
        kc, dho = h.count_batch(t.corpus, t.offs)
        assert np.array_equal(kc, a.key_counts) and np.array_equal(dho, a.dho)

    def host_doc_counts(h, t, a):
        pairs, dpo = h.doc_counts_batch(t.corpus, t.offs)
        assert pairs.tobytes() == a.pairs.tobytes() and np.array_equal(dpo, a.dpo)

    def host_cover(h, t, a):
        mask, cov = h.cover_batch(t.corpus, t.offs)
        assert np.array_equal(mask, a.mask) and np.array_equal(cov, a.doc_covered)
        red, cov = h.redact_batch(t.corpus, t.offs)
        assert np.array_equal(red, a.redacted) and np.array_equal(cov, a.doc_covered)

    views = {}

    def dev_match_unaligned(h, t, a):
        if id(t) not in views:
            views[id(t)] = unaligned(t)
        dev_match(h, t, a, views[id(t)])

    # the kinds named after document ranges must take them: aha_timing.repeats counts a call's ranges before its last
    in_ranges = {"count in document ranges", "doc counts, small hit buffer", "select in document ranges",
                 "replace in document ranges"}
    g.set_profiling(True)
    g_dc.set_profiling(True)
    g_sel.set_profiling(True)
    kinds = [
        ("device match", g, dev_match),
        ("device match, unaligned view", g, dev_match_unaligned),
        ("count", g, dev_count),
        ("count in document ranges", g, lambda h, t, a: dev_count(h, t, a, region_bytes=300_000)),
        ("doc counts", g, dev_doc_counts),
        ("doc counts, small hit buffer", g_dc, dev_doc_counts),
        ("cover, caller's mask", g, lambda h, t, a: dev_cover(h, t, a, True)),
        ("cover, no mask", g, lambda h, t, a: dev_cover(h, t, a, False)),
        ("host match and count", g, host_match_count),
        ("host doc counts", g, host_doc_counts),
        ("host cover", g, host_cover),
        ("select", g, dev_select),
        ("select in document ranges", g_sel, dev_select),
        ("replace", g, dev_replace),
        ("replace in document ranges", g_sel, dev_replace),
        ("records", g, dev_records),
        ("grep", g, dev_grep),
        ("host select", g, host_select),
        ("host replace", g, host_replace),
        ("host records", g, host_records),
        ("host grep", g, host_grep),
        ("feed match", g, feed_match),
        ("feed select", g, feed_select),
        ("feed replace", g, feed_replace),
        ("feed grep", g, feed_grep),
        ("feed match, separator filter", g, lambda h, t, a: feed_match(h, t, a, sep=True)),
    ]
    # the feed kinds whose window batch is matched into the feed's own grow-only hit buffer (feed_windows with hits); a feed
    # grep counts its windows and keeps the strict rule
    windows_with_hits = {"feed match", "feed select", "feed replace", "feed match, separator filter"}
    (big, small), (a_big, a_small) = texts, answers
    assert len(a_big.hits) > 2 * big.D and len(a_small.hits) > 0
    for name, h, call in kinds:
        try:
            h.release_scratch()
            call(h, big, a_big)
            grown = h.scratch_bytes()
            assert grown > 0
            if name in in_ranges:
                assert h.last_timing()["repeats"] >= 1, "the batch was not cut into document ranges"
            call(h, big, a_big)
            assert h.scratch_bytes() == grown, "a second identical call allocated"
            call(h, small, a_small)
            if name in windows_with_hits:
                settled = h.scratch_bytes()
                assert settled >= grown
                call(h, small, a_small)
                call(h, big, a_big)
                assert h.scratch_bytes() == settled, "the buffers did not settle"
            else:
                assert h.scratch_bytes() == grown, "a smaller batch allocated"
            h.release_scratch()
            assert h.scratch_bytes() == 0
            call(h, big, a_big)
        except AssertionError as e:
            raise AssertionError(f"{name}: {e}") from e
