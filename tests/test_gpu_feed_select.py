"""Feed select calls (aha_feed_select_batch, aha_feed_select_batch_device) against feedselectsim over the CPU ORACLE's hits:
every call is compared exactly -- hits, offsets, bases, hold -- and the concatenation with AC.select_batch of the whole
sequences as one batch on the same handle.  Inputs are a few KB."""
import ctypes as C
import random

import numpy as np
import pytest

import feedselectsim as fss
import pyoracle as orc
import selectsim
from aha_amd import AC, AhaError, Hit
from aha_amd import _native as N
from engine_variants import VARIANTS, use_variant

pytestmark = pytest.mark.gpu

GUARD = 0x5A5A5A5A
PAD = 8
DEV = "cuda:0"


def _fold(t):
    return bytes(b + 32 if 0x41 <= b <= 0x5A else b for b in bytes(t))


class Rig:
    """a handle, a feed on it and the model beside it"""

    def __init__(self, keys, n_seqs=4, fold=False, chars=False):
        keys = [k.encode() if isinstance(k, str) else bytes(k) for k in keys]
        self.m = AC.compile(keys, fold_ascii=fold)
        self.o = orc.AC.compile([_fold(k) for k in keys] if fold else keys)
        plain = fss.oracle_match(self.o)
        self.match = (lambda t: plain(_fold(t))) if fold else plain
        self.W = fss.window(keys)
        self.n_seqs = n_seqs
        self.feed = self.m.feed(n_seqs, chars=chars)
        self.model = fss.Feed(self.match, self.W, n_seqs)
        self.said = {}  # seq -> everything reported so far, absolute
        self.whole = {}  # seq -> the sequence so far


def _raw(feed, pieces, ids, final=False, cap=64, device=False, sizing=False):
    """one call through the C entry with guard words in and behind every caller buffer
    -> (rc, hits HIT_DTYPE, pso, bases, hold, n_selected, n_hits, untouched: no caller buffer was written)"""
    corpus = np.frombuffer(b"".join(pieces), dtype=np.uint8).copy()
    offs = np.cumsum([0] + [len(p) for p in pieces]).astype(np.uint64)
    ids = np.asarray(ids, dtype=np.uint32)
    D = len(pieces)
    flags = N.AHA_FEED_SELECT_FINAL if final else 0
    n, nh = C.c_uint64(0), C.c_uint64(0)
    L = N.lib()
    if device:
        import torch

        ct = torch.from_numpy(corpus).to(DEV) if corpus.size else torch.zeros(0, dtype=torch.uint8, device=DEV)
        ot = torch.from_numpy(offs.view(np.int64)).to(DEV)
        it = torch.from_numpy(ids.view(np.int32)).to(DEV) if D else torch.zeros(0, dtype=torch.int32, device=DEV)
        out = torch.full((cap + PAD, 3), GUARD, dtype=torch.int32, device=DEV)
        pso = torch.full((D + 1 + PAD,), GUARD, dtype=torch.int64, device=DEV)
        bases = torch.full((D + PAD,), GUARD, dtype=torch.int64, device=DEV)
        hold = torch.full((D + PAD,), GUARD, dtype=torch.int32, device=DEV)
        s = torch.cuda.current_stream().cuda_stream
        rc = L.aha_feed_select_batch_device(feed._h, ct.data_ptr(), ot.data_ptr(), it.data_ptr(), D, corpus.size, flags,
                                            None if sizing else out.data_ptr(), 0 if sizing else cap, pso.data_ptr(),
                                            bases.data_ptr(), hold.data_ptr(), C.byref(n), C.byref(nh), C.c_void_p(s))
        torch.cuda.synchronize()
        out, pso, bases, hold = (t.cpu().numpy() for t in (out, pso, bases, hold))
    else:
        out = np.full((cap + PAD, 3), GUARD, dtype=np.int32)
        pso = np.full(D + 1 + PAD, GUARD, dtype=np.int64)
        bases = np.full(D + PAD, GUARD, dtype=np.int64)
        hold = np.full(D + PAD, GUARD, dtype=np.int32)
        rc = L.aha_feed_select_batch(feed._h, corpus.ctypes.data, offs.ctypes.data, ids.ctypes.data, D, flags,
                                     None if sizing else out.ctypes.data, 0 if sizing else cap, pso.ctypes.data,
                                     bases.ctypes.data, hold.ctypes.data, C.byref(n), C.byref(nh))
    ns = int(n.value)
    assert (out[cap:] == GUARD).all() and (pso[D + 1:] == GUARD).all() and (bases[D:] == GUARD).all() and (hold[D:] == GUARD).all()
    untouched = all((a == GUARD).all() for a in (out, pso, bases, hold))
    if rc == N.AHA_OK:
        assert (out[ns:] == GUARD).all(), "the call wrote behind the selection"
    hits = np.ascontiguousarray(out[:min(ns, cap)]).view(selectsim.HIT_DTYPE).reshape(-1)
    return rc, hits, pso[:D + 1].astype(np.uint64), bases[:D].astype(np.uint64), hold[:D].astype(np.uint32), ns, int(nh.value), untouched


def step(r, pieces, ids, final=False, device=False):
    """one call on the feed and on the model: identical, hit for hit"""
    pieces = [bytes(p) for p in pieces]
    want, wpso, wbases, whold = r.model.call(pieces, ids, final)
    rc, hits, pso, bases, hold, ns, nh, _ = _raw(r.feed, pieces, ids, final, cap=want.size + 3, device=device)
    assert rc == N.AHA_OK, (rc, r.m.last_error() if hasattr(r.m, "last_error") else "")
    assert ns == want.size and hits.tobytes() == want.tobytes(), (hits.tolist(), want.tolist())
    assert np.array_equal(pso, wpso) and np.array_equal(bases, wbases) and np.array_equal(hold, whold), (hold, whold)
    assert (hold <= r.W).all()
    for d, q in enumerate(ids):
        r.whole[q] = r.whole.get(q, b"") + pieces[d]
        r.said.setdefault(q, []).extend((s + int(bases[d]), e + int(bases[d]), v) for s, e, v in hits[int(pso[d]):int(pso[d + 1])].tolist())
    return hits, hold


def finish_and_compare(r, device=False):
    """FINAL with empty pieces for every sequence that has text, then: what was said = select_batch of the whole sequences"""
    qs = sorted(q for q, t in r.whole.items() if r.model.seqs[q].text or t)
    open_ = [q for q in qs if r.model.seqs[q].text]
    if open_:
        _, hold = step(r, [b""] * len(open_), open_, final=True, device=device)
        assert not hold.any()
        for q in open_:
            assert r.feed.position(q) == (0, 0)
    docs = [r.whole[q] for q in qs]
    sel, dso = r.m.select_batch(np.frombuffer(b"".join(docs), dtype=np.uint8), np.cumsum([0] + [len(d) for d in docs]).astype(np.uint64))
    for i, q in enumerate(qs):
        assert r.said.get(q, []) == [tuple(h) for h in sel[int(dso[i]):int(dso[i + 1])].tolist()], q


def test_longer_key_completes_later():
    r = Rig(["ab", "abcde"])
    hits, hold = step(r, [b"ab"], [0])
    assert hits.size == 0 and hold.tolist() == [2]  # nothing is reported early
    hits, hold = step(r, [b"cde"], [0])
    assert hits.tolist() == [(-2, 3, 1)] and hold.tolist() == [0]  # one hit (0, 5), with a negative start
    assert r.said[0] == [(0, 5, 1)]
    finish_and_compare(r)
    # the Python one-sequence form: absolute offsets
    assert r.feed.select(1, b"ab") == [] and r.feed.select(1, b"x", final=True) == [Hit(0, 2, 0)]
    assert r.feed.position(1) == (0, 0)


@pytest.mark.parametrize("device", [False, True])
def test_settled_hit_hides_tail_starts_every_cut(device):
    for cut in range(5):
        r = Rig(["ab", "bcd", "cd", "d"])
        step(r, [b"abcd"[:cut]], [2], device=device)
        step(r, [b"abcd"[cut:]], [2], device=device)
        finish_and_compare(r, device)
        assert r.said[2] == [(0, 2, 0), (2, 4, 2)]


def test_a_key_longer_than_several_pieces():
    key = bytes(range(0x41, 0x41 + 40))
    r = Rig([key, key[:7], key[3:9], key[38:]])
    text = b"xx" + key + key[:20] + key + b"y"
    at = 0
    for i, n in enumerate([1, 3, 0, 7, 2, 0, 0, 11, 5, 1, 1, 9, 4, 0, 13, 2, 3, 6, 8, 40]):
        step(r, [text[at:at + n]], [1], device=i % 2 == 1)
        at += n
    assert at >= len(text)
    finish_and_compare(r)
    assert (2, 42, 0) in r.said[1] and (62, 102, 0) in r.said[1]


def test_window_zero_everything_settles_at_once():
    r = Rig(["a", "b", "c"])
    assert r.W == 0
    for i, p in enumerate([b"abxc", b"", b"cab", b"x"]):
        hits, hold = step(r, [p, p[::-1]], [0, 3], device=i % 2 == 0)
        assert hold.tolist() == [0, 0] and hits.size == 2 * sum(1 for b in p if b in b"abc")
    finish_and_compare(r)


@pytest.mark.parametrize("lead", [5, 38])
def test_mask_and_rank_boundaries(lead):
    """a hit at nearly every position of ~5000 bytes: the extended positions cross mask words and the 2048-position rank blocks;
    the context makes the piece's first position unaligned.  The context is b + (lead - 1) a's with (lead - 1) % 3 == 1: its
    last a is a hit of its own that the piece's first a's replace by a longer one, so the first reported hit starts at -1"""
    assert (lead - 1) % 3 == 1 and (lead - 2) % 32
    rng = random.Random(lead)
    r = Rig(["a", "aa", "aaa"], n_seqs=2)
    big = bytearray()
    while len(big) < 5000:
        big += b"a" * rng.randint(1, 70) + bytes([rng.choice(b"bx\x00")])
    step(r, [b"b" + b"a" * (lead - 1)], [1])
    hits, _ = step(r, [bytes(big)], [1], device=True)
    assert hits.size > 1500 and hits[0]["start"] < 0
    finish_and_compare(r)


def test_many_pieces_permuted_ids_and_a_subset_call():
    rng = random.Random(600)
    keys = [b"ab", b"abc", b"bca", b"cabcab", b"a", b"bbbb"]
    r = Rig(keys, n_seqs=640)
    ids = rng.sample(range(640), 600)
    mk = lambda: bytes(rng.choice(b"abc") for _ in range(rng.randint(0, 40)))
    step(r, [mk() for _ in ids], ids, device=True)
    sub = rng.sample(ids, 150) + [q for q in range(640) if q not in ids][:5]
    step(r, [mk() for _ in sub], sub, device=True)
    step(r, [mk() for _ in ids], ids[::-1])
    # FINAL with non-empty pieces on some, the rest flushed by empty ones
    some = ids[:200]
    _, hold = step(r, [mk() for _ in some], some, final=True, device=True)
    assert not hold.any() and all(r.feed.position(q) == (0, 0) for q in some[:5])
    finish_and_compare(r)


def test_final_then_the_sequence_starts_again():
    r = Rig(["ab", "abcde", "e"])
    step(r, [b"xab"], [0])
    hits, hold = step(r, [b""], [0], final=True)  # FINAL with an empty piece flushes the open hit
    assert hits.tolist() == [(-2, 0, 0)] and hold.tolist() == [0] and r.feed.position(0) == (0, 0)
    hits, _ = step(r, [b"cdeab"], [0], final=True)  # from 0: no "abcde" across the FINAL call
    assert hits.tolist() == [(2, 3, 2), (3, 5, 0)] and r.feed.position(0) == (0, 0)
    step(r, [b"abcd"], [0])
    assert r.feed.position(0) == (4, 0)


@pytest.mark.parametrize("device", [False, True])
def test_capacity_changes_nothing(device):
    r = Rig(["ab", "abc", "c"], n_seqs=3)
    step(r, [b"abca", b"cc"], [0, 2], device=device)
    pieces, ids = [b"bcabcab", b"", b"cabc"], [2, 1, 0]
    want, wpso, wbases, whold = r.model.call(pieces, ids)
    assert want.size >= 3
    before = [r.feed.position(q) for q in range(3)]
    rc, _, _, _, _, ns, _, untouched = _raw(r.feed, pieces, ids, cap=want.size - 1, device=device)
    assert rc == N.AHA_E_CAPACITY and ns == want.size and untouched
    rc, _, _, _, _, ns, _, untouched = _raw(r.feed, pieces, ids, sizing=True, device=device)  # out = NULL, cap = 0
    assert rc == N.AHA_E_CAPACITY and ns == want.size and untouched
    assert [r.feed.position(q) for q in range(3)] == before
    rc, hits, pso, bases, hold, ns, _, _ = _raw(r.feed, pieces, ids, cap=want.size, device=device)
    assert rc == N.AHA_OK and hits.tobytes() == want.tobytes()
    assert np.array_equal(pso, wpso) and np.array_equal(bases, wbases) and np.array_equal(hold, whold)


def test_mixing_with_match_calls():
    r = Rig(["ab", "abcde"], n_seqs=3)
    step(r, [b"ab", b"xa"], [0, 1])
    r.feed.match(0, b"cd")  # sequence 0 moves on without its select state
    r.feed.match(2, b"ab")  # ... and sequence 2 never had any
    for q in (0, 2):
        before = r.feed.position(q)
        rc, _, _, _, _, _, _, untouched = _raw(r.feed, [b"e"], [q])
        assert rc == N.AHA_E_INVALID and untouched and r.feed.position(q) == before
        with pytest.raises(AhaError) as e:
            r.feed.select(q, b"e")
        assert e.value.code == N.AHA_E_INVALID and "select" in str(e.value)
    hits, _ = step(r, [b"bcde"], [1])  # the neighbour, fed through select only, is unaffected
    assert hits.tolist() == [(-1, 4, 1)]
    for q in (0, 2):
        r.feed.reset(q)
        r.model.seqs[q] = fss.Sequence(r.match, r.W)
        r.whole[q], r.said[q] = b"", []
        step(r, [b"abcde"], [q])  # after reset the sequence works again
    finish_and_compare(r)
    r.feed.reset()  # every sequence at once
    assert r.feed.select(1, b"abcdeab", final=True) == [Hit(0, 5, 1), Hit(5, 7, 0)]


def test_char_feed_is_refused():
    r = Rig(["我", "我是"], chars=True)
    for device in (False, True):
        rc, _, _, _, _, _, _, untouched = _raw(r.feed, ["我是".encode()], [0], device=device)
        assert rc == N.AHA_E_INVALID and untouched and r.feed.position(0) == (0, 0)


def test_folded_handle_cut_inside_a_key():
    r = Rig(["Hello", "hell", "LOW", "o"], fold=True)
    text = b"xHeLLo hELLOW helLo"
    for cut in (3, 5, 11):
        rr = Rig(["Hello", "hell", "LOW", "o"], fold=True)
        step(rr, [text[:cut]], [0])
        step(rr, [text[cut:]], [0], device=True)
        finish_and_compare(rr)
    assert r.feed.select(0, text, final=True)[0] == Hit(1, 6, 0)


@pytest.fixture(params=VARIANTS)
def variant(request, monkeypatch):
    return use_variant(request.param, monkeypatch)


def _random_case(rng, utf8, device):
    if utf8:
        chars = "我是中国人民"
        keys = sorted({"".join(rng.choice(chars) for _ in range(rng.randint(1, 3))).encode() for _ in range(rng.randint(2, 8))})
        alphabet = [c.encode() for c in chars] + [b"a", b"\x00"]
    else:
        n = rng.randint(1, 6)
        keys = set()
        while len(keys) < n:
            keys.add(bytes(rng.choice(b"abc") for _ in range(rng.randint(1, 6))))
        keys = sorted(keys)
        alphabet = [b"a", b"b", b"c", b"a", b"b", b"x", b"\x00"]
    n_seqs = rng.randint(1, 8)
    r = Rig(keys, n_seqs=n_seqs)
    texts = [b"".join(rng.choice(alphabet) for _ in range(rng.randint(0, 300)))[:300] for _ in range(n_seqs)]
    at = [0] * n_seqs
    for _ in range(rng.randint(1, 5)):
        qs = rng.sample(range(n_seqs), rng.randint(1, n_seqs))
        pieces = []
        for q in qs:
            n = rng.choice([0, 1, 2, 5, rng.randint(0, 120)])
            pieces.append(texts[q][at[q]:at[q] + n])
            at[q] += len(pieces[-1])
        step(r, pieces, qs, device=device)
    finish_and_compare(r, device)


@pytest.mark.parametrize("part", range(6))
def test_random(part):
    """300 cases in six parts: key sets over {a,b,c} and, every fifth, a UTF-8 key set; both entries"""
    rng = random.Random(4100 + part)
    for case in range(50):
        _random_case(rng, utf8=case % 5 == 4, device=case % 2 == 1)


@pytest.mark.parametrize("utf8", [False, True])
def test_engine_variants(variant, utf8):
    rng = random.Random(17 + utf8)
    for device in (False, True):
        _random_case(rng, utf8, device)


def test_device_entry_finds_bad_offsets_and_duplicates():
    import torch

    r = Rig(["ab", "abc"])
    step(r, [b"ab"], [0])
    corpus = torch.from_numpy(np.frombuffer(b"cabcab", dtype=np.uint8).copy()).to(DEV)
    out = torch.full((16, 3), GUARD, dtype=torch.int32, device=DEV)
    bad = [([0, 4, 3, 6], [0, 1, 2]), ([1, 3, 6], [0, 1]), ([0, 3, 5], [0, 1]), ([0, 3, 6], [1, 1]), ([0, 3, 6], [0, 4])]
    for offs, ids in bad:
        ot = torch.tensor(offs, dtype=torch.int64, device=DEV)
        it = torch.tensor(ids, dtype=torch.int32, device=DEV)
        with pytest.raises(AhaError) as e:
            r.feed.select_batch_device(corpus, ot, it, out)
        assert e.value.code == N.AHA_E_INVALID
        torch.cuda.synchronize()
        assert (out.cpu().numpy() == GUARD).all() and r.feed.position(0) == (2, 0) and r.feed.position(1) == (0, 0)
    hits, _ = step(r, [b"cab"], [0], device=True)  # the feed is as it was
    assert hits.tolist() == [(-2, 1, 1)]


def test_two_feeds_in_the_same_state_give_identical_bytes():
    rng = random.Random(3)
    a, b = Rig(["ab", "abc", "bca", "c"], n_seqs=5), None
    b = a.m.feed(5)
    said = 0
    for i in range(4):
        ids = rng.sample(range(5), 3)
        pieces = [bytes(rng.choice(b"abc") for _ in range(rng.randint(0, 30))) for _ in ids]
        x = _raw(a.feed, pieces, ids, final=i == 3, cap=128, device=i % 2 == 0)
        y = _raw(b, pieces, ids, final=i == 3, cap=128, device=i % 2 == 0)
        assert x[0] == y[0] == N.AHA_OK and all(np.asarray(p).tobytes() == np.asarray(q).tobytes() for p, q in zip(x[1:5], y[1:5]))
        assert x[5:7] == y[5:7]
        said += x[5]
    assert said > 0


def test_python_replacer_end_to_end():
    keys = ["ab", "abcde", "cd", "e", "xy"]
    r = Rig(keys)
    repl = {0: "<AB>", 1: "", 2: "Q", 3: None}  # replacement, deletion, kept aloud, kept by omission
    text = b"abcdxabcdeecdabxyabcdabcdecd e"
    assert len(text) == 30
    want = r.m.replace(text, repl)
    assert want != text
    for cut in range(31):
        rep = r.feed.replacer(repl)
        got = rep.push(1, text[:cut]) + rep.push(1, text[cut:]) + rep.finish(1)
        assert got == want, cut
        assert r.feed.position(1) == (0, 0)
    rep = r.feed.replacer(repl)
    got = b"".join(rep.push(3, text[i:i + 1]) for i in range(30)) + rep.finish(3)  # byte by byte
    assert got == want
    assert rep.push(0, "xab") + rep.finish(0) == b"x<AB>"  # str is UTF-8; bytes come back
