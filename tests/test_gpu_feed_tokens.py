"""Feed token calls (aha_feed_select_batch* with AHA_FEED_SELECT_TOKENS) against feedtokensim over the CPU ORACLE's hits: every
call is compared exactly -- tokens, offsets, bases, hold -- through both entries, with guard words behind every caller buffer;
the concatenation against tokensim on the whole sequences and against AC.tokens_batch on the same handle.  The device entry's
corpus ends with its allocation and starts at a chosen alignment.  Inputs are a few KB."""
import ctypes as C
import random

import numpy as np
import pytest

import feedtokensim as fts
import pyoracle as orc
import selectsim
import tokensim
from aha_amd import AC, AhaError, BitArray, Hit
from aha_amd import _native as N
from engine_variants import VARIANTS, use_variant

pytestmark = pytest.mark.gpu

GUARD = 0x5A5A5A5A
PAD = 8
DEV = "cuda:0"
TOK, RUNS, FINAL = N.AHA_FEED_SELECT_TOKENS, N.AHA_FEED_SELECT_GAP_RUNS, N.AHA_FEED_SELECT_FINAL


def _fold(t):
    return bytes(b + 32 if 0x41 <= b <= 0x5A else b for b in bytes(t))


class Rig:
    """a handle, a feed on it and the model beside it"""

    def __init__(self, keys, n_seqs=4, fold=False, gap_runs=False, **feed_args):
        keys = [k.encode() if isinstance(k, str) else bytes(k) for k in keys]
        self.m = AC.compile(keys, fold_ascii=fold)
        self.o = orc.AC.compile([_fold(k) for k in keys] if fold else keys)
        plain = fts.oracle_match(self.o)
        self.match = (lambda t: plain(_fold(t))) if fold else plain
        self.W = fts.window(keys)
        self.gap_runs = gap_runs
        self.feed = self.m.feed(n_seqs, **feed_args)
        self.model = fts.Feed(self.match, self.W, n_seqs)
        self.restart(reset=False)

    def restart(self, reset=True):
        """every sequence from length 0 again"""
        if reset:
            self.feed.reset()
        self.model = fts.Feed(self.match, self.W, len(self.model.seqs))
        self.said = {}  # seq -> everything reported so far, absolute
        self.whole = {}  # seq -> the sequence so far


def _raw(feed, pieces, ids, flags=TOK, cap=64, device=False, sizing=False, align=0):
    """one call through the C entry with guard words in and behind every caller buffer; the device entry's corpus starts `align`
    bytes behind a 16-byte border and ends with its allocation
    -> (rc, tokens HIT_DTYPE, pto, bases, hold, n_tokens, n_hits, untouched: no caller buffer was written)"""
    corpus = np.frombuffer(b"".join(pieces), dtype=np.uint8).copy()
    offs = np.cumsum([0] + [len(p) for p in pieces]).astype(np.uint64)
    ids = np.asarray(ids, dtype=np.uint32)
    D = len(pieces)
    n, nh = C.c_uint64(0), C.c_uint64(0)
    L = N.lib()
    if device:
        import torch

        room = torch.zeros(align + corpus.size, dtype=torch.uint8, device=DEV)
        assert room.data_ptr() % 16 == 0
        ct = room[align:]
        if corpus.size:
            ct.copy_(torch.from_numpy(corpus))
        ot = torch.from_numpy(offs.view(np.int64)).to(DEV)
        it = torch.from_numpy(ids.view(np.int32)).to(DEV) if D else torch.zeros(0, dtype=torch.int32, device=DEV)
        out = torch.full((cap + PAD, 3), GUARD, dtype=torch.int32, device=DEV)
        pto = torch.full((D + 1 + PAD,), GUARD, dtype=torch.int64, device=DEV)
        bases = torch.full((D + PAD,), GUARD, dtype=torch.int64, device=DEV)
        hold = torch.full((D + PAD,), GUARD, dtype=torch.int32, device=DEV)
        s = torch.cuda.current_stream().cuda_stream
        rc = L.aha_feed_select_batch_device(feed._h, ct.data_ptr(), ot.data_ptr(), it.data_ptr(), D, corpus.size, flags,
                                            None if sizing else out.data_ptr(), 0 if sizing else cap, pto.data_ptr(),
                                            bases.data_ptr(), hold.data_ptr(), C.byref(n), C.byref(nh), C.c_void_p(s))
        torch.cuda.synchronize()
        assert ct.cpu().numpy().tobytes() == corpus.tobytes()
        out, pto, bases, hold = (t.cpu().numpy() for t in (out, pto, bases, hold))
    else:
        out = np.full((cap + PAD, 3), GUARD, dtype=np.int32)
        pto = np.full(D + 1 + PAD, GUARD, dtype=np.int64)
        bases = np.full(D + PAD, GUARD, dtype=np.int64)
        hold = np.full(D + PAD, GUARD, dtype=np.int32)
        rc = L.aha_feed_select_batch(feed._h, corpus.ctypes.data, offs.ctypes.data, ids.ctypes.data, D, flags,
                                     None if sizing else out.ctypes.data, 0 if sizing else cap, pto.ctypes.data,
                                     bases.ctypes.data, hold.ctypes.data, C.byref(n), C.byref(nh))
    nt = int(n.value)
    assert (out[cap:] == GUARD).all() and (pto[D + 1:] == GUARD).all() and (bases[D:] == GUARD).all() and (hold[D:] == GUARD).all()
    untouched = all((a == GUARD).all() for a in (out, pto, bases, hold))
    if rc == N.AHA_OK:
        assert (out[nt:] == GUARD).all(), "the call wrote behind the tokens"
    toks = np.ascontiguousarray(out[:min(nt, cap)]).view(selectsim.HIT_DTYPE).reshape(-1)
    return rc, toks, pto[:D + 1].astype(np.uint64), bases[:D].astype(np.uint64), hold[:D].astype(np.uint32), nt, int(nh.value), untouched


def step(r, pieces, ids, final=False, device=False, align=0, gap_runs=None, twin=None):
    """one call on the feed and on the model: identical, token for token; twin: a second feed in the same state, which gives
    identical bytes through the other entry"""
    pieces = [bytes(p) for p in pieces]
    gap_runs = r.gap_runs if gap_runs is None else gap_runs
    want, wpto, wbases, whold = r.model.call(pieces, ids, final, gap_runs)
    flags = TOK | (FINAL if final else 0) | (RUNS if gap_runs else 0)
    rc, toks, pto, bases, hold, nt, nh, _ = _raw(r.feed, pieces, ids, flags, cap=want.size + 3, device=device, align=align)
    assert rc == N.AHA_OK, (rc, N.lib().aha_last_error(r.m._h))
    assert nt == want.size and toks.tobytes() == want.tobytes(), (toks.tolist(), want.tolist())
    assert np.array_equal(pto, wpto) and np.array_equal(bases, wbases) and np.array_equal(hold, whold), (hold, whold)
    if twin is not None:
        y = _raw(twin, pieces, ids, flags, cap=want.size + 3, device=not device)
        assert y[0] == N.AHA_OK and y[5:7] == (nt, nh)
        assert all(np.asarray(a).tobytes() == np.asarray(b).tobytes() for a, b in zip((toks, pto, bases, hold), y[1:5]))
    for d, q in enumerate(ids):
        r.whole[q] = r.whole.get(q, b"") + pieces[d]
        r.said.setdefault(q, []).extend((s + int(bases[d]), e + int(bases[d]), v) for s, e, v in toks[int(pto[d]):int(pto[d + 1])].tolist())
    return toks, hold


def finish_and_compare(r, device=False):
    """FINAL with empty pieces for every sequence that has text, then: what was said = the tokens of the whole sequences, by
    tokensim over the oracle and by AC.tokens_batch on the same handle"""
    qs = sorted(q for q, t in r.whole.items() if r.model.seqs[q].text or t)
    open_ = [q for q in qs if r.model.seqs[q].text]
    if open_:
        _, hold = step(r, [b""] * len(open_), open_, final=True, device=device)
        assert not hold.any()
        for q in open_:
            assert r.feed.position(q) == (0, 0)
    docs = [r.whole[q] for q in qs]
    toks, dto = r.m.tokens_batch(np.frombuffer(b"".join(docs), dtype=np.uint8), np.cumsum([0] + [len(d) for d in docs]).astype(np.uint64),
                                 gap_runs=r.gap_runs)
    for i, q in enumerate(qs):
        said = fts.join_gaps(r.said.get(q, [])) if r.gap_runs else r.said.get(q, [])
        assert said == tokensim.tokens_doc(docs[i], selectsim.select_doc(r.match(docs[i])), r.gap_runs), q
        assert said == [tuple(t) for t in toks[int(dto[i]):int(dto[i + 1])].tolist()], q


# ---- the header's examples ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("device", [False, True])
@pytest.mark.parametrize("gap_runs", [False, True])
def test_example_one_at_every_cut(device, gap_runs):
    text = b"xabcdeab"
    r = Rig(["ab", "abcde"], gap_runs=gap_runs)
    for i in range(len(text) + 1):
        for j in range(i, len(text) + 1, 2):
            r.restart()
            for p in (text[:i], text[i:j], text[j:]):
                step(r, [p], [1], device=device)
            finish_and_compare(r, device)
            assert fts.join_gaps(r.said[1]) == [(0, 1, -1), (1, 6, 1), (6, 8, 0)]


def test_examples_call_by_call():
    r = Rig(["ab", "abcde"])
    expect = [(b"xab", False, [], 3), (b"cd", False, [(-3, -2, -1)], 4), (b"eab", False, [(-4, 1, 1)], 2), (b"", True, [(-2, 0, 0)], 0)]
    for p, final, want, hold in expect:
        toks, h = step(r, [p], [0], final=final)
        assert toks.tolist() == want and h.tolist() == [hold]
    u = "我是中".encode()
    r = Rig(["是"])
    for p, final, want, hold in [(u[:4], False, [], 4), (u[4:8], False, [(-4, -1, -1), (-1, 2, 0)], 2), (u[8:], False, [], 3),
                                 (b"", True, [(-3, 0, -1)], 0)]:
        toks, h = step(r, [p], [0], final=final, device=True)
        assert toks.tolist() == want and h.tolist() == [hold]
    r = Rig(["a"])
    for p, final, want, hold in [(b"xa\xc3", False, [(0, 1, -1), (1, 2, 0)], 1), (b"\xa9", False, [], 2), (b"y", False, [(-2, 0, -1)], 1),
                                 (b"", True, [(-1, 0, -1)], 0)]:
        toks, h = step(r, [p], [0], final=final)
        assert toks.tolist() == want and h.tolist() == [hold]
    r = Rig(["ab"], gap_runs=True)
    for p, final, want, hold in [(b"zzzzzz", False, [(0, 5, -1)], 1), (b"zzab", False, [(-1, 2, -1), (2, 4, 0)], 0),
                                 (b"zz", True, [(0, 2, -1)], 0)]:
        toks, h = step(r, [p], [0], final=final, device=True)
        assert toks.tolist() == want and h.tolist() == [hold]
    assert fts.join_gaps(r.said[0])[0] == (0, 8, -1)
    # the Python one-sequence form: absolute offsets
    r = Rig(["ab", "abcde"])
    assert r.feed.tokens(1, b"xab") == [] and r.feed.tokens(1, b"cd") == [Hit(0, 1, -1)]
    assert r.feed.tokens(1, b"", final=True) == [Hit(1, 3, 0), Hit(3, 4, -1), Hit(4, 5, -1)] and r.feed.position(1) == (0, 0)


@pytest.mark.parametrize("keys", [["是"], ["我是"], [b"\x98\xaf"], ["a"]])
def test_a_character_cut_at_each_of_its_bytes(keys):
    """three-, two- and four-byte characters and stray continuation bytes, two cuts anywhere: every byte of a character is a
    piece's last, and F(n1) lands inside a character"""
    text = "我是中é𝄞".encode() + b"\x80\x80z"
    hit_f = False
    r = Rig(keys)
    for i in range(len(text) + 1):
        for j in range(i, len(text) + 1):
            r.restart()
            for k, p in enumerate((text[:i], text[i:j], text[j:])):
                n1 = len(r.whole.get(0, b"")) + len(p)
                f = fts.frontier(n1, r.W)
                hit_f = hit_f or (0 < f < len(text) and (text[f] & 0xC0) == 0x80)
                step(r, [p], [0], device=(i + j + k) % 2 == 1)
            finish_and_compare(r)
    assert hit_f


def test_a_key_longer_than_several_pieces_and_pieces_shorter_than_the_window():
    key = bytes(range(0x41, 0x41 + 40))
    r = Rig([key, key[:7], key[3:9], key[38:]])
    text = "我".encode() + key + key[:20] + "é是".encode() + key + b"y\x80"
    at = 0
    for i, n in enumerate([1, 3, 0, 7, 2, 0, 0, 11, 5, 1, 1, 9, 4, 0, 13, 2, 3, 6, 8, 40, 30]):
        step(r, [text[at:at + n]], [1], device=i % 2 == 1)
        at += n
    assert at >= len(text)
    finish_and_compare(r)
    assert (3, 43, 0) in r.said[1]


@pytest.mark.parametrize("gap_runs", [False, True])
def test_window_zero_and_empty_pieces(gap_runs):
    r = Rig(["a", "b", "c"], gap_runs=gap_runs)
    assert r.W == 0
    for i, p in enumerate([b"abxc", b"", "x中".encode()[:3], "x中".encode()[3:] + b"cab", b"", b"x\xc3"]):
        step(r, [p, p[::-1]], [0, 3], device=i % 2 == 0)
    step(r, [b"", b""], [3, 1], final=True)  # FINAL with empty pieces: one closes a token, one names a sequence that has none
    finish_and_compare(r)


# ---- masks, ranks, alignments -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lead", [5, 38])
@pytest.mark.parametrize("gap_runs", [False, True])
def test_mask_and_rank_boundaries(lead, gap_runs):
    """~5000 bytes behind a context of `lead` bytes: c0 and c1 fall on both sides of a 32-position mask word, the extended
    positions cross the 2048-position rank blocks"""
    rng = random.Random(lead)
    r = Rig(["a", "aa", "aaa"], n_seqs=2, gap_runs=gap_runs)
    big = bytearray()
    while len(big) < 5000:
        big += b"a" * rng.randint(1, 70) + rng.choice([b"b", b"x", "中".encode(), b"\x80\x80"])
    step(r, [b"b" + b"a" * (lead - 1)], [1])
    toks, _ = step(r, [bytes(big)], [1], device=True)
    assert toks.size > 1500
    finish_and_compare(r)


def test_a_token_start_on_both_sides_of_a_rank_block():
    """W = 0 and no continuation byte: every position starts a token, the last of rank block 0 and the first of block 1 included;
    a second sequence behind it starts inside a block"""
    rng = random.Random(1)
    r = Rig(["q"])
    text = bytes(rng.choice(b"abcq") for _ in range(4200))
    toks, _ = step(r, [text, b"xyq"], [0, 2], device=True)
    assert toks.size == 4203 and toks[2047]["start"] == 2047 and toks[2048]["start"] == 2048
    finish_and_compare(r)


@pytest.mark.parametrize("align", range(16))
def test_every_alignment_of_the_corpus_and_the_pieces(align):
    """the corpus starts `align` bytes behind a 16-byte border and ends with its allocation; the pieces' lengths put their first
    bytes on other offsets again and the last piece's end anywhere in an aligned piece"""
    rng = random.Random(align)
    units = [b"a", b"b", "中".encode(), "é".encode(), b"\x80", b"z"]
    r = Rig(["ab", "中a", "b"], n_seqs=5)
    for rnd in range(3):
        pieces = [b"".join(rng.choice(units) for _ in range(n)) for n in (17 + align, 33 + rnd, 5, 0, 48 - align)]
        step(r, pieces, [4, 0, 2, 3, 1], device=True, align=align)
    finish_and_compare(r, device=True)


def test_many_pieces_permuted_ids_a_subset_call_and_two_feeds():
    rng = random.Random(600)
    units = [b"a", b"b", b"c", "中".encode(), b"\x80"]
    r = Rig([b"ab", b"abc", b"bca", b"cabcab", "中a".encode(), b"bbbb"], n_seqs=340)
    twin = r.m.feed(340)
    ids = rng.sample(range(340), 300)
    mk = lambda: b"".join(rng.choice(units) for _ in range(rng.randint(0, 40)))
    sub = rng.sample(ids, 150) + [q for q in range(340) if q not in ids][:5]
    calls = [(ids, False), (sub, False), (ids[::-1], False), (ids[:200], True)]  # (the last: FINAL with non-empty pieces on some)
    for i, (qs, final) in enumerate(calls):
        step(r, [mk() for _ in qs], qs, final=final, device=i % 2 == 0, twin=twin)
    finish_and_compare(r)


def test_two_feeds_in_the_same_state_give_identical_bytes():
    rng = random.Random(3)
    a = Rig(["ab", "abc", "bca", "c"], n_seqs=5)
    b = a.m.feed(5)
    said = 0
    for i in range(4):
        ids = rng.sample(range(5), 3)
        pieces = [b"".join(rng.choice([b"a", b"b", b"c", "é".encode(), b"\xa9"]) for _ in range(rng.randint(0, 30))) for _ in ids]
        flags = TOK | (FINAL if i == 3 else 0)
        x = _raw(a.feed, pieces, ids, flags, cap=256, device=i % 2 == 0)
        y = _raw(b, pieces, ids, flags, cap=256, device=i % 2 == 0)
        assert x[0] == y[0] == N.AHA_OK and all(np.asarray(p).tobytes() == np.asarray(q).tobytes() for p, q in zip(x[1:5], y[1:5]))
        assert x[5:7] == y[5:7]
        said += x[5]
    assert said > 0


# ---- state ---------------------------------------------------------------------------------------------------------------------
def test_final_then_the_sequence_starts_again():
    r = Rig(["ab", "abcde", "e"])
    step(r, [b"xab\xc3"], [0])
    toks, hold = step(r, [b""], [0], final=True)
    assert toks.tolist() == [(-4, -3, -1), (-3, -1, 0), (-1, 0, -1)] and hold.tolist() == [0] and r.feed.position(0) == (0, 0)
    toks, _ = step(r, [b"\xa9cdeab"], [0], final=True)  # from 0: no character and no "abcde" across the FINAL call
    assert toks.tolist() == [(0, 1, -1), (1, 2, -1), (2, 3, -1), (3, 4, 2), (4, 6, 0)] and r.feed.position(0) == (0, 0)
    step(r, [b"abcd"], [0])
    assert r.feed.position(0) == (4, 0)


@pytest.mark.parametrize("device", [False, True])
def test_capacity_and_sizing_calls_change_nothing(device):
    r = Rig(["ab", "abc", "c"], n_seqs=3)
    _, hold0 = step(r, [b"abca\xc3", b"cc"], [0, 2], device=device)
    pieces, ids = [b"bcabcab", b"", b"\xa9cabc"], [2, 1, 0]
    want, wpto, wbases, whold = r.model.call(pieces, ids)
    assert want.size >= 3
    before = [r.feed.position(q) for q in range(3)]
    rc, _, _, _, _, nt, _, untouched = _raw(r.feed, pieces, ids, cap=want.size - 1, device=device)
    assert rc == N.AHA_E_CAPACITY and nt == want.size and untouched
    rc, _, _, _, _, nt, _, untouched = _raw(r.feed, pieces, ids, sizing=True, device=device)  # out = NULL, cap = 0
    assert rc == N.AHA_E_CAPACITY and nt == want.size and untouched
    assert [r.feed.position(q) for q in range(3)] == before
    rc, toks, pto, bases, hold, nt, _, _ = _raw(r.feed, pieces, ids, cap=want.size, device=device)
    assert rc == N.AHA_OK and toks.tobytes() == want.tobytes()
    assert np.array_equal(pto, wpto) and np.array_equal(bases, wbases) and np.array_equal(hold, whold)
    rc, _, _, _, hold, _, _, _ = _raw(r.feed, [b"", b""], [0, 2], device=device)  # the holds are those the model kept
    assert rc == N.AHA_OK and hold.tolist() == [int(whold[2]), int(whold[0])]


def test_mixing_with_select_calls():
    r = Rig(["ab", "abcde"], n_seqs=3)
    step(r, [b"ab", b"xa"], [0, 1])
    assert r.feed.select(0, b"cd") == []  # select after tokens is valid: the select state is its own
    r.feed.select(2, b"ab")  # ... and sequence 2 never had token state
    for q in (0, 2):
        before = r.feed.position(q)
        rc, _, _, _, _, _, _, untouched = _raw(r.feed, [b"e"], [q])
        assert rc == N.AHA_E_INVALID and untouched and r.feed.position(q) == before
        with pytest.raises(AhaError) as e:
            r.feed.tokens(q, b"e")
        assert e.value.code == N.AHA_E_INVALID and "tokens" in str(e.value)
    assert r.feed.select(0, b"e") == [Hit(0, 5, 1)]  # the feed is unchanged: select goes on where it was
    toks, _ = step(r, [b"bcde"], [1])  # the neighbour, fed through token calls only, is unaffected
    assert toks.tolist() == [(-2, -1, -1), (-1, 4, 1)]
    for q in (0, 2):
        r.feed.reset(q)
        r.model.seqs[q] = fts.Sequence(r.match, r.W)
        r.whole[q], r.said[q] = b"", []
        step(r, [b"abcde"], [q])  # after reset the sequence takes token calls again
    # a select FINAL restarts the sequence too, and the same length reached through select calls is not mistaken for token state
    r.feed.select(1, b"", final=True)
    assert len(r.whole[1]) == 6
    r.feed.select(1, b"xabcdx")
    rc, _, _, _, _, _, _, untouched = _raw(r.feed, [b"e"], [1])
    assert rc == N.AHA_E_INVALID and untouched
    r.feed.select(1, b"", final=True)
    r.model.seqs[1] = fts.Sequence(r.match, r.W)
    r.whole[1], r.said[1] = b"", []
    step(r, [b"xab"], [1])
    finish_and_compare(r)
    r.feed.reset()  # every sequence at once
    assert r.feed.tokens(1, b"abcdeab", final=True) == [Hit(0, 5, 1), Hit(5, 7, 0)]
    # both gap modes on one sequence: each call applies its own bit from t0 on
    r = Rig(["a"])
    _, hold = step(r, [b"zz\xc3"], [1])
    assert hold.tolist() == [1]
    toks, hold = step(r, [b"\xa9z"], [1], gap_runs=True)
    assert toks.tolist() == [(-1, 2, -1)] and hold.tolist() == [0]
    toks, _ = step(r, [b"\xc3\xa9"], [1], final=True)
    assert toks.tolist() == [(0, 2, -1)]


def test_refusals_of_feed_select_hold_for_tokens():
    m = AC.compile(["我", "我是"])
    sep = BitArray(256)
    feeds = [m.feed(2, chars=True), m.feed(2, sep=sep), m.feed(2, longest=1), AC.compile(["straße"], fold_simple=True).feed(2, fold=True)]
    for feed in feeds:
        for device in (False, True):
            for flags in (TOK, TOK | RUNS, TOK | FINAL):
                rc, _, _, _, _, _, _, untouched = _raw(feed, ["我是".encode()], [0], flags, device=device)
                assert rc == N.AHA_E_INVALID and untouched and feed.position(0)[0] == 0
    feed = m.feed(2)
    for flags in (RUNS, RUNS | FINAL, 16 | TOK, 2 | TOK):
        rc, _, _, _, _, _, _, untouched = _raw(feed, [b"x"], [0], flags)
        assert rc == N.AHA_E_INVALID and untouched


def test_folded_handle_cut_inside_a_key():
    text = "xHeLLo hELLOW é helLo".encode()
    for cut in (3, 5, 11, 15):
        rr = Rig(["Hello", "hell", "LOW", "o"], fold=True)
        step(rr, [text[:cut]], [0])
        step(rr, [text[cut:]], [0], device=True)
        finish_and_compare(rr)
        assert rr.said[0][:2] == [(0, 1, -1), (1, 6, 0)]


def test_a_token_open_beyond_the_bound_is_refused(monkeypatch):
    monkeypatch.setenv("AHA_FEED_TOKEN_OPEN", "8")
    r = Rig(["a"])
    piece = b"a" + b"\x80" * 20
    for device in (False, True):
        rc, _, _, _, _, nt, _, untouched = _raw(r.feed, [piece], [0], device=device)
        assert rc == N.AHA_E_TOO_LONG and untouched and r.feed.position(0) == (0, 0)
    rc, _, _, _, _, _, _, _ = _raw(r.feed, [piece], [0], TOK | RUNS)  # gaps as runs never hold
    assert rc == N.AHA_OK and r.feed.position(0) == (21, 0)
    r.feed.reset(0)
    toks, hold = step(r, [b"\x80" * 8], [0])  # at the bound: held
    assert toks.size == 0 and hold.tolist() == [8]
    rc, _, _, _, _, _, _, untouched = _raw(r.feed, [b"\x80"], [0])
    assert rc == N.AHA_E_TOO_LONG and untouched and r.feed.position(0) == (8, 0)
    toks, hold = step(r, [b"\x80" * 13], [0], final=True)  # FINAL closes the token
    assert toks.tolist() == [(-8, 13, -1)] and hold.tolist() == [0]
    toks, _ = step(r, [piece], [0], final=True)
    assert toks.tolist() == [(0, 1, 0), (1, 21, -1)]


# ---- random --------------------------------------------------------------------------------------------------------------------
@pytest.fixture(params=VARIANTS)
def variant(request, monkeypatch):
    return use_variant(request.param, monkeypatch)


def _random_case(rng, utf8, device, gap_runs):
    if utf8:
        chars = "我是中国人民"
        keys = sorted({"".join(rng.choice(chars) for _ in range(rng.randint(1, 3))).encode() for _ in range(rng.randint(2, 8))})
        if rng.random() < 0.3:
            keys = sorted(set(keys) | {"中".encode()[1:], "我".encode()[:2]})  # byte-level keys that cut a character
        alphabet = [c.encode() for c in chars] + [b"a", b"\x00", b"\x80", "é".encode()]
    else:
        n = rng.randint(1, 6)
        keys = set()
        while len(keys) < n:
            keys.add(bytes(rng.choice(b"abc") for _ in range(rng.randint(1, 6))))
        keys = sorted(keys)
        alphabet = [b"a", b"b", b"c", b"a", b"b", b"x", b"\x00", "中".encode(), b"\xbf"]
    n_seqs = rng.randint(1, 8)
    r = Rig(keys, n_seqs=n_seqs, gap_runs=gap_runs)
    texts = [b"".join(rng.choice(alphabet) for _ in range(rng.randint(0, 300)))[:300] for _ in range(n_seqs)]
    at = [0] * n_seqs
    for _ in range(rng.randint(1, 5)):
        qs = rng.sample(range(n_seqs), rng.randint(1, n_seqs))
        pieces = []
        for q in qs:
            n = rng.choice([0, 1, 2, 5, rng.randint(0, 120)])
            pieces.append(texts[q][at[q]:at[q] + n])
            at[q] += len(pieces[-1])
        step(r, pieces, qs, device=device, align=rng.randrange(16))
    finish_and_compare(r, device)


@pytest.mark.parametrize("part", range(6))
def test_random(part):
    """150 cases in six parts: key sets over {a,b,c} and, every third, a UTF-8 key set; both entries, both gap modes"""
    rng = random.Random(5100 + part)
    for case in range(25):
        _random_case(rng, utf8=case % 3 == 2, device=case % 2 == 1, gap_runs=case % 4 >= 2)


@pytest.mark.parametrize("utf8", [False, True])
def test_engine_variants(variant, utf8):
    rng = random.Random(17 + utf8)
    for device in (False, True):
        _random_case(rng, utf8, device, gap_runs=False)


@pytest.mark.parametrize("blocks", [1, 3])
def test_small_grids_where_every_lane_strides(blocks, monkeypatch):
    """AHA_POST_BLOCKS (read when the handle is compiled) caps every grid of the token passes: the mask words (a lane each in
    kft_starts), the rank blocks (a wave each in kft_emit) and the pieces (a lane each in kft_bounds, kft_edge, kft_commit)
    exceed the grid's lanes and waves"""
    monkeypatch.setenv("AHA_POST_BLOCKS", str(blocks))
    lanes, waves = 256 * blocks, 4 * blocks
    rng = random.Random(blocks)
    n_seqs = lanes + 40
    units = [b"a", b"b", b"c", "中".encode(), "é".encode(), b"\x80"]
    r = Rig(["ab", "abc", "中a", "c"], n_seqs=n_seqs)
    ids = rng.sample(range(n_seqs), n_seqs)
    for rnd in range(2):
        pieces = [b"".join(rng.choice(units) for _ in range(rng.randint(40, 90) if d % 3 else rng.randint(0, 2))) for d in range(n_seqs)]
        n_ext = sum(len(p) for p in pieces)
        assert len(pieces) > lanes and (n_ext + 31) // 32 > lanes and (n_ext + 2047) // 2048 > waves
        step(r, pieces, ids, device=rnd == 1, align=rnd * 7)
    finish_and_compare(r, device=True)


def test_python_segmenter_end_to_end():
    keys = ["ab", "abcde", "中国", "e"]
    r = Rig(keys)
    text = "abcdx我是中国人abcdeé".encode() + b"\x80ab e"
    want = [(text[s:e], v) for s, e, v in tokensim.tokens_doc(text, selectsim.select_doc(r.match(text)))]
    for cut in range(len(text) + 1):
        g = r.feed.segmenter()
        got = g.push(1, text[:cut]) + g.push(1, text[cut:]) + g.finish(1)
        assert got == want, cut
        assert r.feed.position(1) == (0, 0)
    g = r.feed.segmenter()
    got = sum((g.push(3, text[i:i + 1]) for i in range(len(text))), []) + g.finish(3)  # byte by byte
    assert got == want
    g = r.feed.segmenter(gap_runs=True)
    parts = g.push(0, "我是中") + g.push(0, "国人") + g.finish(0)  # str is UTF-8; bytes come back, a gap in parts
    assert b"".join(b for b, _ in parts) == "我是中国人".encode() and ("中国".encode(), 2) in parts
