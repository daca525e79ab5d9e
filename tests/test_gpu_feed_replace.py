"""Feed replace calls (aha_feed_replace_batch, aha_feed_replace_batch_device) against feedreplacesim over the CPU ORACLE's
hits: every call is compared exactly -- bytes, offsets, bases, hold, counts -- and the concatenation with AC.replace of the
whole sequence on the same handle.  Inputs are a few KB."""
import ctypes as C
import random

import numpy as np
import pytest

import feedreplacesim as frs
import feedselectsim as fss
import pyoracle as orc
from aha_amd import AC, AhaError, BitArray
from aha_amd import _native as N

pytestmark = pytest.mark.gpu

GUARD8, GUARD32, GUARD64 = 0x5A, 0x5A5A5A5A, 0x5A5A5A5A5A5A5A5A
PAD = 32  # guard bytes in front of out and behind it; guard entries behind every array
DEV = "cuda:0"


def _fold(t):
    return bytes(b + 32 if 0x41 <= b <= 0x5A else b for b in bytes(t))


class Rig:
    """a handle, a replacement table, a feed on it and the model beside it"""

    def __init__(self, keys, repl, n_seqs=4, fold=False):
        keys = [k.encode() if isinstance(k, str) else bytes(k) for k in keys]
        self.m = AC.compile(keys, fold_ascii=fold)
        self.repl = repl
        self.table = self.m.replacements(repl)
        self.o = orc.AC.compile([_fold(k) for k in keys] if fold else keys)
        plain = fss.oracle_match(self.o)
        self.match = (lambda t: plain(_fold(t))) if fold else plain
        self.W = fss.window(keys)
        self.n_seqs = n_seqs
        self.feed = self.m.feed(n_seqs)
        self.model = frs.Feed(self.match, self.W, n_seqs)
        self.said = {}  # seq -> the results so far, concatenated
        self.whole = {}  # seq -> the sequence so far


def _raw(feed, table, pieces, ids, final=False, cap=64, device=False, sizing=False, out_mod=0, corpus_mod=0):
    """one call through the C entry with 0x5A in, in front of and behind every caller buffer; out and the corpus start out_mod /
    corpus_mod bytes behind a 16-byte aligned address
    -> (rc, out uint8[cap], poo, bases, hold, n_out_bytes, n_selected, n_hits, untouched: no caller buffer was written)"""
    blob = b"".join(pieces)
    offs = np.cumsum([0] + [len(p) for p in pieces]).astype(np.uint64)
    ids = np.asarray(ids, dtype=np.uint32)
    D = len(pieces)
    flags = N.AHA_FEED_REPLACE_FINAL if final else 0
    n, ns, nh = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
    L = N.lib()
    craw = np.zeros(16 + len(blob) + 16, dtype=np.uint8)
    craw[corpus_mod:corpus_mod + len(blob)] = np.frombuffer(blob, dtype=np.uint8)
    lo = PAD + out_mod
    if device:
        import torch

        ct = torch.from_numpy(craw).to(DEV)
        ot = torch.from_numpy(offs.view(np.int64)).to(DEV)
        it = torch.from_numpy(ids.view(np.int32)).to(DEV) if D else torch.zeros(0, dtype=torch.int32, device=DEV)
        raw = torch.full((lo + cap + PAD,), GUARD8, dtype=torch.uint8, device=DEV)
        assert raw.data_ptr() % 16 == 0 and ct.data_ptr() % 16 == 0
        poo = torch.full((D + 1 + PAD,), GUARD64, dtype=torch.int64, device=DEV)
        bases = torch.full((D + PAD,), GUARD64, dtype=torch.int64, device=DEV)
        hold = torch.full((D + PAD,), GUARD32, dtype=torch.int32, device=DEV)
        s = torch.cuda.current_stream().cuda_stream
        rc = L.aha_feed_replace_batch_device(feed._h, table._h, ct.data_ptr() + corpus_mod, ot.data_ptr(), it.data_ptr(), D, len(blob),
                                             flags, None if sizing else raw.data_ptr() + lo, 0 if sizing else cap, poo.data_ptr(),
                                             bases.data_ptr(), hold.data_ptr(), C.byref(n), C.byref(ns), C.byref(nh), C.c_void_p(s))
        torch.cuda.synchronize()
        raw, poo, bases, hold = (t.cpu().numpy() for t in (raw, poo, bases, hold))
    else:
        raw = np.full(lo + cap + PAD, GUARD8, dtype=np.uint8)
        poo = np.full(D + 1 + PAD, GUARD64, dtype=np.int64)
        bases = np.full(D + PAD, GUARD64, dtype=np.int64)
        hold = np.full(D + PAD, GUARD32, dtype=np.int32)
        rc = L.aha_feed_replace_batch(feed._h, table._h, craw.ctypes.data + corpus_mod, offs.ctypes.data, ids.ctypes.data, D, flags,
                                      None if sizing else raw.ctypes.data + lo, 0 if sizing else cap, poo.ctypes.data,
                                      bases.ctypes.data, hold.ctypes.data, C.byref(n), C.byref(ns), C.byref(nh))
    nb = int(n.value)
    assert (raw[:lo] == GUARD8).all(), "the call wrote in front of out"
    assert (raw[lo + cap:] == GUARD8).all(), "the call wrote behind cap_bytes"
    assert (poo[D + 1:] == GUARD64).all() and (bases[D:] == GUARD64).all() and (hold[D:] == GUARD32).all()
    untouched = (raw == GUARD8).all() and (poo == GUARD64).all() and (bases == GUARD64).all() and (hold == GUARD32).all()
    return (rc, raw[lo:lo + cap], poo[:D + 1].astype(np.uint64), bases[:D].astype(np.uint64), hold[:D].astype(np.uint32), nb,
            int(ns.value), int(nh.value), untouched)


def step(r, pieces, ids, final=False, device=False, want=None, **where):
    """one call on the feed and on the model: identical, byte for byte.  want: the model's answer where it is already known"""
    pieces = [bytes(p) for p in pieces]
    wout, wpoo, wbases, whold, wsel = want if want is not None else r.model.call(pieces, ids, r.repl, final)
    rc, out, poo, bases, hold, nb, ns, _, _ = _raw(r.feed, r.table, pieces, ids, final, cap=wout.size + 5, device=device, **where)
    assert rc == N.AHA_OK, (rc, N.lib().aha_last_error(None))
    assert nb == wout.size and ns == wsel and out[:nb].tobytes() == wout.tobytes(), (out[:nb].tobytes(), wout.tobytes())
    assert (out[nb:] == GUARD8).all(), "the call wrote behind the total"
    assert np.array_equal(poo, wpoo) and np.array_equal(bases, wbases) and np.array_equal(hold, whold), (hold, whold)
    assert (hold <= r.W).all()
    for d, q in enumerate(ids):
        r.whole[q] = r.whole.get(q, b"") + pieces[d]
        r.said[q] = r.said.get(q, b"") + out[int(poo[d]):int(poo[d + 1])].tobytes()
    return out[:nb].tobytes(), hold


def finish_and_compare(r, device=False):
    """FINAL with empty pieces for every sequence that is open, then: what was said = AC.replace_batch of the whole sequences"""
    open_ = [q for q in sorted(r.whole) if r.model.seqs[q].q.text]
    if open_:
        _, hold = step(r, [b""] * len(open_), open_, final=True, device=device)
        assert not hold.any()
        for q in open_[:8]:
            assert r.feed.position(q) == (0, 0)
    qs = sorted(r.whole)
    docs = [r.whole[q] for q in qs]
    out, doo = r.m.replace_batch(np.frombuffer(b"".join(docs), dtype=np.uint8), np.cumsum([0] + [len(d) for d in docs]).astype(np.uint64),
                                 r.table)
    for i, q in enumerate(qs):
        assert r.said.get(q, b"") == out[int(doo[i]):int(doo[i + 1])].tobytes(), q


KEYS = [b"ab", b"abc", b"bca", b"cabcab", b"a", b"bbbb"]  # W = 5
REPL = {0: b"<AB>", 1: b"", 2: b"\x00Q", 3: None, 5: b"a far longer replacement"}  # key 4: kept by omission


def _text(rng, n, alphabet=b"abcabx\x00"):
    return bytes(rng.choice(alphabet) for _ in range(n))


@pytest.mark.parametrize("device", [False, True])
def test_every_cut_with_small_pieces_behind_it(device):
    """a text of 100 bytes cut at every position -- one sequence per cut, all in one call --, then pieces of 0, 1, W - 1, W and
    W + 1 bytes, then the rest with FINAL: every call against the model, the stream against replace of the whole"""
    rng = random.Random(11)
    text = _text(rng, 100)
    r = Rig(KEYS, REPL, n_seqs=101)
    assert r.W == 5
    at = list(range(101))
    ids = list(range(101))
    step(r, [text[:c] for c in at], ids, device=device)
    for n in (0, 1, r.W - 1, r.W, r.W + 1):
        step(r, [text[a:a + n] for a in at], ids, device=device)
        at = [min(a + n, 100) for a in at]
    step(r, [text[a:] for a in at], ids, final=True, device=device)
    assert all(r.whole[q] == text for q in ids)
    finish_and_compare(r, device)
    assert len({r.said[q] for q in ids}) == 1 and r.said[0] != text


def _big_call(rng, W):
    """the pieces of the large call: lengths 0 .. 3 W, and a few that hold whole 1024-byte tiles"""
    lens = [rng.randint(0, 3 * W) for _ in range(294)] + [1023, 1024, 1025 + W, 5000, 0, 0]
    rng.shuffle(lens)
    pieces = []
    for n in lens:
        if n >= 1023:  # a long stretch without a hit in the middle: whole tiles of the copy lie in one gap
            k = n // 4
            pieces.append(_text(rng, k) + bytes(0x80 | (7 * i + 13 * (i >> 7)) & 0xFF for i in range(n - 2 * k)) + _text(rng, k))
        else:
            pieces.append(_text(rng, n))
    return pieces


def test_one_large_call_at_every_alignment():
    """300 pieces in one call (a call names a sequence once: 300 sequences, in random order, about 100 of them with text and
    open bytes from a call before), with out and the corpus at each of the 16 byte alignments.  Fast tiles, partial tiles and
    pieces whose result is empty all occur; the guard bytes either side of out are intact (_raw)."""
    rng = random.Random(300)
    n_seqs = 320
    primed = rng.sample(range(n_seqs), 100)
    first = [_text(rng, rng.randint(1, 12)) for _ in primed]
    ids = rng.sample(range(n_seqs), 300)
    pieces = _big_call(rng, 5)
    model = Rig(KEYS, REPL, n_seqs=n_seqs)
    want0 = model.model.call(first, primed, REPL)
    want1 = model.model.call(pieces, ids, REPL)
    poo = want1[1].astype(np.int64)
    sizes = poo[1:] - poo[:-1]
    assert (sizes == 0).sum() >= 2 and want1[3].max() == 5 and want1[0].size > 8000
    assert any(len(p) == 0 and int(want1[3][d]) > 0 for d, p in enumerate(pieces))  # an empty piece on a sequence with open bytes
    m, table = model.m, model.table
    for a in range(16):
        r = model
        r.feed = m.feed(n_seqs)
        r.said, r.whole = {}, {}
        step(r, first, primed, device=True, want=want0)
        step(r, pieces, ids, device=True, want=want1, out_mod=a, corpus_mod=(5 * a + 3) % 16)
    # the host entry, once; then the streams against replace of the whole sequences
    r.feed = m.feed(n_seqs)
    r.said, r.whole = {}, {}
    step(r, first, primed, want=want0)
    step(r, pieces, ids, want=want1)
    finish_and_compare(r)


@pytest.mark.parametrize("device", [False, True])
def test_capacity_changes_nothing(device):
    r = Rig(["ab", "abc", "c"], {0: b"12345", 1: b"", 2: b"CC"}, n_seqs=3)
    step(r, [b"abca", b"cc"], [0, 2], device=device)
    pieces, ids = [b"bcabcab", b"", b"cabc"], [2, 1, 0]
    want = r.model.call(pieces, ids, r.repl)
    need = want[0].size
    assert need >= 8 and want[4] >= 3
    before = [r.feed.position(q) for q in range(3)]
    rc, _, _, _, _, nb, ns, nh, untouched = _raw(r.feed, r.table, pieces, ids, cap=need - 1, device=device)
    assert rc == N.AHA_E_CAPACITY and nb == need and ns == want[4] and nh >= ns and untouched
    rc, _, _, _, _, nb, ns, _, untouched = _raw(r.feed, r.table, pieces, ids, sizing=True, device=device)  # out = NULL, cap = 0
    assert rc == N.AHA_E_CAPACITY and nb == need and ns == want[4] and untouched
    assert [r.feed.position(q) for q in range(3)] == before
    step(r, pieces, ids, device=device, want=want)  # the larger call gives what the first would have
    # a total of 0 succeeds with cap 0: everything deleted, nothing else there
    rr = Rig(["ab"], {0: b""}, n_seqs=2)
    rc, _, poo, bases, hold, nb, ns, _, _ = _raw(rr.feed, rr.table, [b"abab", b""], [1, 0], final=True, sizing=True, device=device)
    assert rc == N.AHA_OK and nb == 0 and ns == 2 and poo.tolist() == [0, 0, 0] and hold.tolist() == [0, 0] and bases.tolist() == [0, 0]


def _refused(r, table, pieces, ids, device, word=None):
    before = [r.feed.position(q) for q in range(r.n_seqs)]
    rc, _, _, _, _, _, _, _, untouched = _raw(r.feed, table, pieces, ids, device=device)
    assert rc == N.AHA_E_INVALID and untouched
    assert [r.feed.position(q) for q in range(r.n_seqs)] == before
    if word:
        assert word in N.lib().aha_last_error(None).decode()


@pytest.mark.parametrize("device", [False, True])
def test_refusals_leave_the_feed_as_it_was(device):
    import torch

    r = Rig(["ab", "abcde"], {0: b"<AB>", 1: b"!"}, n_seqs=3)
    step(r, [b"xab", b"ab"], [0, 1], device=device)
    # a char feed, a feed with a separator filter
    chars = r.m.feed(2, chars=True)
    sep = BitArray(256)
    sep[0x20] = True
    filtered = r.m.feed(2, sep=sep)
    for f in (chars, filtered):
        rc, _, _, _, _, _, _, _, untouched = _raw(f, r.table, [b"ab ab"], [0], device=device)
        assert rc == N.AHA_E_INVALID and untouched and f.position(0) == (0, 0)
    assert "separator filter" in N.lib().aha_last_error(None).decode()
    # a table made for another handle
    other = AC.compile(["ab", "abcde"])
    _refused(r, other.replacements({0: b"no"}), [b"cde"], [0], device, "another handle")
    # the device entry with out overlapping the corpus
    if device:
        buf = torch.full((64,), 0x61, dtype=torch.uint8, device=DEV)
        ot = torch.tensor([0, 32], dtype=torch.int64, device=DEV)
        it = torch.zeros(1, dtype=torch.int32, device=DEV)
        for lo in (0, 16, 31):
            with pytest.raises(AhaError) as e:
                r.feed.replace_batch_device(buf[:32], ot, it, r.table, buf[lo:lo + 32])
            assert e.value.code == N.AHA_E_INVALID and "overlaps" in str(e.value)
        torch.cuda.synchronize()
        assert (buf.cpu().numpy() == 0x61).all() and r.feed.position(0) == (3, 0)
    # a sequence a match call touched, until its reset
    r.feed.match(1, b"c")
    _refused(r, r.table, [b"de"], [1], device, "select")
    _refused(r, r.table, [b"cde", b"de"], [0, 1], device)  # ... and a call that names it beside a good one
    r.feed.reset(1)
    r.model.reset(1)
    r.whole[1], r.said[1] = b"", b""
    out, _ = step(r, [b"cdeab", b"abcdex"], [0, 1], device=device)  # the feed is as it was: sequence 0 goes on, 1 from 0
    assert out == b"x!!"
    finish_and_compare(r, device)
    assert r.said[0] == b"x!<AB>" and r.said[1] == b"!x"


def test_select_and_replace_calls_mixed_on_one_sequence():
    r = Rig(["ab", "abcde"], {0: b"<AB>", 1: b"!"}, n_seqs=2)
    hits, info = r.feed.select_batch(b"xabc", [0, 4], [1])
    assert hits.size == 0 and info["piece_hold"].tolist() == [4]
    r.model.select([b"xabc"], [1])
    out, hold = step(r, [b"deab"], [1])  # the replace call starts where the select call left the cursor: T[0..6)
    assert out == b"x!" and hold.tolist() == [2]
    hits, info = r.feed.select_batch(b"yzw", [0, 3], [1])  # "ab" at (6, 8) is settled by a select call: no result will hold it
    r.model.select([b"yzw"], [1])
    assert hits.tolist() == [(-2, 0, 0)] and info["piece_hold"].tolist() == [3]
    out, hold = step(r, [b"ab"], [1], final=True, device=True)
    assert out == b"yzw<AB>" and hold.tolist() == [0] and r.feed.position(1) == (0, 0)
    assert r.feed.replace(0, b"abcdeab", r.table, final=True) == b"!<AB>"  # the Python one-sequence form
    assert r.feed.replace(0, "xab", {0: "é"}) == b"" and r.feed.replace(0, b"", {0: "é"}, final=True) == "xé".encode()


@pytest.mark.parametrize("device", [False, True])
def test_folded_handle_keeps_the_callers_bytes(device):
    """a hit that straddles a cut on a folded handle: outside the replaced hits the original case survives, in the bytes the
    feed held back too (they come from its context, which holds the caller's text)"""
    text = b"xxHeLLo WoRLD hELLOW heLLo"
    for cut in (3, 5, 6, 9, 21):
        r = Rig(["Hello", "LOW", "world"], {0: b"[hi]", 1: None, 2: b""}, fold=True)
        step(r, [text[:cut]], [0], device=device)
        step(r, [text[cut:]], [0], device=device)
        finish_and_compare(r, device)
        assert r.said[0] == b"xx[hi]  [hi]W [hi]"
    r = Rig(["abcdefgh"], {0: b"-"}, fold=True)
    out, hold = step(r, [b"QrStAbC"], [0], device=device)
    assert out == b"" and hold.tolist() == [7]
    out, _ = step(r, [b"xYz"], [0], final=True, device=device)
    assert out == b"QrStAbCxYz"  # no hit after all: the held bytes come back as the caller wrote them


def test_utf8_keys_and_a_keyword_list():
    """the character-level engine and the prefix-filter engine under the feed's passes"""
    rng = random.Random(77)
    cjk = ["中", "中国", "国人", "人民共和", "我是"]
    r = Rig(cjk, {0: "Z", 1: "中华", 2: "", 3: None, 4: "I am "})
    assert r.m.info["unit_enabled"] == 1
    words = ["alpha", "alphabet", "bet", "betray", "ray", "trayful"]
    k = Rig(words, {0: b"A", 1: b"", 2: b"wager", 4: b"\x00", 5: None})
    assert k.m.info["filter_prefix_bytes"] == 3
    alphabets = [[c.encode() for c in "我是中国人民共和"] + [b"a", b"\x00"], [w.encode() for w in words] + [b" ", b"tr", b"al", b"ful"]]
    for rig, alphabet in zip((r, k), alphabets):
        texts = [b"".join(rng.choice(alphabet) for _ in range(rng.randint(5, 80))) for _ in range(4)]
        at = [0] * 4
        for call in range(5):
            qs = rng.sample(range(4), rng.randint(1, 4))
            pieces = []
            for q in qs:
                n = rng.choice([0, 1, 3, 7, rng.randint(0, 60)])
                pieces.append(texts[q][at[q]:at[q] + n])
                at[q] += len(pieces[-1])
            step(rig, pieces, qs, device=call % 2 == 1)
        finish_and_compare(rig, device=True)
        assert any(rig.said[q] != rig.whole[q] for q in rig.whole)


def test_every_new_kernel_loops_on_a_grid_of_one(monkeypatch):
    """AHA_REPLACE_BLOCKS=1 (read when the handle is compiled): the stage, the scan and the copy run on one workgroup each, which
    strides over all tiles"""
    monkeypatch.setenv("AHA_REPLACE_BLOCKS", "1")
    rng = random.Random(5)
    r = Rig(KEYS, REPL, n_seqs=40)
    ids = rng.sample(range(40), 30)
    step(r, [_text(rng, rng.randint(0, 9)) for _ in ids], ids, device=True)
    ids = rng.sample(range(40), 36)
    pieces = [_text(rng, rng.randint(0, 40)) for _ in ids]
    pieces[3] = _text(rng, 9000, b"ab\x80\x81\x82")  # 9 tiles of staged text in one piece, hits all over it
    pieces[7] = _text(rng, 700) + bytes(0x80 | (i & 0x7F) for i in range(6000)) + _text(rng, 300)  # fast tiles of both kernels
    out, _ = step(r, pieces, ids, device=True)
    assert len(out) > 16 * 1024
    finish_and_compare(r, device=True)


def test_final_with_empty_pieces_and_all_deleted_runs():
    r = Rig(["a", "aa", "aaa", "b"], {0: b"", 1: b"", 2: b"", 3: b""}, n_seqs=6)
    out, hold = step(r, [b"aaaa", b"bab", b"", b"aaaaaaaab" * 200], [0, 1, 2, 5], device=True)
    assert out == b"" and hold.tolist() == [1, 2, 0, 1]  # everything settled is deleted: every piece gives 0 bytes
    out, hold = step(r, [b"", b"", b""], [1, 0, 2], final=True)  # FINAL with empty pieces: the held bytes, deleted too
    assert out == b"" and not hold.any()
    out, _ = step(r, [b"xaay", b"", b"aab"], [3, 4, 0], final=True, device=True)  # a survivor between deleted runs
    assert out == b"xy"
    for q in range(6):
        assert r.feed.position(q) == ((1800, 0) if q == 5 else (0, 0))
    finish_and_compare(r)
    assert r.said[5] == b"" and r.said[3] == b"xy"


def test_two_feeds_in_the_same_state_give_identical_bytes():
    rng = random.Random(3)
    a = Rig(["ab", "abc", "bca", "c"], {0: b"<>", 1: b"", 3: b"cc"}, n_seqs=5)
    b = a.m.feed(5)
    said = 0
    for i in range(4):
        ids = rng.sample(range(5), 3)
        pieces = [_text(rng, rng.randint(0, 30), b"abc") for _ in ids]
        x = _raw(a.feed, a.table, pieces, ids, final=i == 3, cap=256, device=i % 2 == 0)
        y = _raw(b, a.table, pieces, ids, final=i == 3, cap=256, device=i % 2 == 0)
        assert x[0] == y[0] == N.AHA_OK and all(np.asarray(p).tobytes() == np.asarray(q).tobytes() for p, q in zip(x[1:5], y[1:5]))
        assert x[5:8] == y[5:8]
        said += x[5]
    assert said > 0
