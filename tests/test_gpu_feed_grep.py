"""Feed grep calls (aha_feed_grep_batch*) against feedgrepsim -- the call-by-call model over the CPU ORACLE's hits, which
tests/test_feed_grep_host.py proves equal to the whole-sequence definition -- never against the library's own match.  Every
output of every call is compared, with guard words behind what a call may write.  Shapes: piece and fragment boundaries on
either side of 32 bytes (a mask word) and 2048 bytes (a rank block), 32 and 2048 fragments, more than 256 dropped runs, 1 / 2 /
33 / 257 pieces over 1 / 3 / 257 sequences with permuted ids and subsets, Lmax 1 / 3 / 64, pieces of 0 and 1 byte, the three
traps, the carried hit, FINAL in every form, invert over empty lines, every misalignment, one-block grids, a folded handle, a
few hundred random sequences, and the laws (capacity, refusals, ids-only, mixing, the Grepper)."""
import ctypes as C
import random

import numpy as np
import pytest

import feedgrepsim as fgs
import pyoracle as orc
from aha_amd import AC, AhaError
from aha_amd import _native as N

pytestmark = pytest.mark.gpu

G64 = 0x5A5A5A5A5A5A5A5A
G32 = 0x5A5A5A5A
G8 = 0x5A
NL = b"\n"


def _cuda(a, dtype):
    import torch

    return torch.from_numpy(np.ascontiguousarray(np.asarray(a).astype(dtype))).cuda()


class Pair:
    """a feed of the library and the model in the same state; step() makes one call on both and compares every output"""

    def __init__(self, keys, n_seqs, fold=False, delim=NL):
        self.keys = [k if isinstance(k, bytes) else k.encode() for k in keys]
        self.m = AC.compile(self.keys, fold_ascii=fold)
        self.count = fgs.oracle_count(orc.AC.compile([k.lower() for k in self.keys] if fold else self.keys), fold)
        self.W = fgs.window(self.keys)
        self.feed = self.m.feed(n_seqs)
        self.model = fgs.Feed(self.count, self.W, n_seqs)
        self.delim = delim

    def device(self, pieces, ids, invert=False, final=False, align=0, cap_recs=None, cap_bytes=None, ids_only=False, room=(0, 0)):
        """the device entry with guards -> dict of what came back (arrays trimmed to what the call may write)"""
        import torch

        text = b"".join(pieces)
        n, D = len(text), len(pieces)
        offs = np.cumsum([0] + [len(p) for p in pieces]).astype(np.int64)
        raw = torch.full((n + 48,), 0x7E, dtype=torch.uint8, device="cuda")
        corpus = raw[align:align + n]
        if n:
            corpus.copy_(torch.from_numpy(np.frombuffer(text, dtype=np.uint8).copy()))
        kept = torch.full((room[0] + 2,), G64, dtype=torch.int64, device="cuda")
        roo = torch.full((room[0] + 3,), G64, dtype=torch.int64, device="cuda")
        outraw = torch.full((room[1] + 40,), G8, dtype=torch.uint8, device="cuda")
        out = outraw[16 + align:16 + align + room[1] + 3]
        per = {k: torch.full((D + 2,), G64, dtype=torch.int64, device="cuda")
               for k in ("piece_rec_offsets", "piece_kept_offsets", "piece_head", "piece_bases", "piece_rec_bases")}
        hold = torch.full((D + 2,), G32, dtype=torch.int32, device="cuda")
        res = {"rc": 0}
        try:
            nr, nk, nb, nh = self.feed.grep_batch_device(
                corpus, _cuda(offs, np.int64), _cuda(ids, np.int32), kept_recs=kept, rec_out_offsets=roo,
                out=None if ids_only else out, delim=self.delim, invert=invert, final=final, piece_hold=hold,
                cap_recs=room[0] if cap_recs is None else cap_recs, cap_bytes=room[1] if cap_bytes is None else cap_bytes, **per)
        except AhaError as e:
            res.update(rc=e.code, n_required=getattr(e, "n_required", None), bytes_required=getattr(e, "bytes_required", None))
            nr = nk = nb = nh = 0
        res.update(n_recs=nr, n_kept=nk, n_out_bytes=nb, n_hits=nh)
        res["kept_raw"] = kept.cpu().numpy().astype(np.uint64)
        res["roo_raw"] = roo.cpu().numpy().astype(np.uint64)
        res["out_raw"] = outraw.cpu().numpy()
        res["out_at"] = 16 + align
        for k, t in per.items():
            res[k] = t.cpu().numpy().astype(np.uint64)
        res["piece_hold"] = hold.cpu().numpy().astype(np.uint32)
        assert (raw.cpu().numpy()[align + n:] == 0x7E).all() and (raw.cpu().numpy()[:align] == 0x7E).all()
        return res

    @staticmethod
    def untouched(res):
        ok = (res["kept_raw"] == G64).all() and (res["roo_raw"] == G64).all() and (res["out_raw"] == G8).all()
        ok = ok and (res["piece_hold"] == G32).all()
        return ok and all((res[k] == G64).all() for k in ("piece_rec_offsets", "piece_kept_offsets", "piece_head", "piece_bases",
                                                            "piece_rec_bases"))

    def compare(self, res, want, D, ids_only=False):
        wk, wo, wr, info = want
        nk, nb = wk.size, wo.size
        assert res["rc"] == 0, res
        assert (res["n_recs"], res["n_kept"], res["n_out_bytes"]) == (info["n_recs"], nk, nb), (res, info)
        assert np.array_equal(res["kept_raw"][:nk], wk) and (res["kept_raw"][nk:] == G64).all()
        assert np.array_equal(res["roo_raw"][:nk + 1], wr) and (res["roo_raw"][nk + 1:] == G64).all()
        a = res["out_at"]
        got = res["out_raw"]
        if ids_only:
            assert (got == G8).all()
        else:
            assert got[a:a + nb].tobytes() == wo.tobytes()
            assert (got[:a] == G8).all() and (got[a + nb:] == G8).all()
        for k in ("piece_rec_offsets", "piece_kept_offsets"):
            assert np.array_equal(res[k][:D + 1], info[k]) and (res[k][D + 1:] == G64).all(), k
        for k in ("piece_head", "piece_bases", "piece_rec_bases"):
            assert np.array_equal(res[k][:D], info[k]) and (res[k][D:] == G64).all(), (k, res[k][:D], info[k])
        assert np.array_equal(res["piece_hold"][:D], info["piece_hold"]) and (res["piece_hold"][D:] == G32).all()

    def step(self, pieces, ids, invert=False, final=False, align=0, ids_only=False, hits=False):
        want = self.model.call(pieces, ids, self.delim, invert, final)
        res = self.device(pieces, ids, invert, final, align, ids_only=ids_only, room=(want[0].size, want[1].size))
        self.compare(res, want, len(pieces), ids_only)
        if hits:
            assert res["n_hits"] == sum(self.count(f) for p in pieces for f in fgs.fragments(p, self.delim))
        return want

    def host(self, pieces, ids, invert=False, final=False):
        """the host entry through Feed.grep_batch, against the model"""
        want = self.model.call(pieces, ids, self.delim, invert, final)
        offs = np.cumsum([0] + [len(p) for p in pieces]).astype(np.uint64)
        kept, out, roo, info = self.feed.grep_batch(np.frombuffer(b"".join(pieces), dtype=np.uint8), offs, np.array(ids, dtype=np.uint32),
                                                    delim=self.delim, invert=invert, final=final)
        assert np.array_equal(kept, want[0]) and out.tobytes() == want[1].tobytes() and np.array_equal(roo, want[2])
        for k, v in want[3].items():
            assert np.array_equal(np.asarray(info[k]), np.asarray(v)), k
        return want


def _cut(text, cuts):
    at = [0] + sorted(cuts) + [len(text)]
    return [text[at[i]:at[i + 1]] for i in range(len(at) - 1)]


def _feed_one(p, text, cuts, seq=0, invert=False, align=0):
    """one sequence cut at `cuts`, a call per piece, the last with FINAL -> the kept bytes by the caller's holding rule"""
    h, lines = fgs.Holder(), []
    pieces = _cut(text, cuts)
    for i, piece in enumerate(pieces):
        final = i == len(pieces) - 1
        kept, out, roo, info = p.step([piece], [seq], invert, final, align)
        raw = out.tobytes()
        lines += h.step(piece, [raw[int(roo[j]):int(roo[j + 1])] for j in range(kept.size)], int(info["piece_head"][0]),
                        int(info["piece_hold"][0]), final)
    assert lines == fgs.whole(p.count, text, p.delim, invert)
    return lines


# ---- the traps, the carried hit, FINAL -------------------------------------------------------------------------------------
def test_the_three_traps_on_the_device():
    p = Pair([b"abc", b"b"], 2)
    assert _feed_one(p, b"ab\n", [1]) == [] and _feed_one(p, b"ab\n", [1], invert=True) == [b"ab\n"]
    p = Pair([b"x\nabc", b"b"], 2)
    for cut in range(7):
        assert _feed_one(p, b"x\nab\n", [cut], seq=cut % 2) == [b"ab\n"]
    assert _feed_one(p, b"x\nab\nx\nabc\n", [3, 4, 9]) == [b"ab\n", b"abc\n"]
    p = Pair([b"\nb"], 1)
    assert _feed_one(p, b"a\nb\nb", [2]) == [] and _feed_one(p, b"a\nb\nb", [1, 3]) == []
    p = Pair([b"b\n"], 1)
    assert _feed_one(p, b"ab\nb", [2]) == [b"ab\n"] and _feed_one(p, b"ab\nb", [3]) == [b"ab\n"]
    assert _feed_one(p, b"ab\nb\n", [2, 5]) == [b"ab\n", b"b\n"]


def test_the_hit_in_a_straddle_and_the_hit_carried_over_two_calls():
    p = Pair([b"abc", b"cab"], 3)
    w = p.step([b"xxab"], [1], hits=True)
    assert w[3]["piece_hold"][0] == 4 and w[0].size == 0
    p.step([b"cxx"], [1], hits=True)  # "abc" only in the straddle: open_hit from now on
    p.step([b"yyyy"], [1])
    p.step([b""], [1])  # an empty piece in the middle of a record
    w = p.step([b"z\nq"], [1], hits=True)  # the hit lies three calls back
    assert w[3]["piece_head"][0] == 11 and w[1].tobytes() == b"z\n" and w[3]["piece_hold"][0] == 1
    w = p.step([b"\n"], [1])  # a piece that is only the delimiter closes "q\n", dropped
    assert w[0].size == 0 and w[3]["piece_head"][0] == 0 and w[3]["piece_hold"][0] == 0 and w[3]["piece_rec_bases"][0] == 1
    p.step([b"c"], [1]), p.step([b"a"], [1]), p.step([b"b"], [1])  # pieces of one byte: "cab" over three calls
    w = p.step([b""], [1], final=True)  # FINAL with an empty piece: the record closes without a fragment
    assert w[3]["piece_head"][0] == 3 and w[0].size == 0 and w[3]["n_recs"] == 0
    assert p.feed.position(1) == (0, 0)
    # the same under invert, and FINAL with and without a trailing delimiter
    for text in (b"xxabcxx\nno\n", b"xxabcxx\nno", b"\n\n\n", b"cab", b""):
        for invert in (False, True):
            for cuts in ([], [3], [2, 5], [0], [len(text)]):
                _feed_one(p, text, [min(c, len(text)) for c in cuts], seq=2, invert=invert)


# ---- the edges of the masks and the rank blocks ------------------------------------------------------------------------------
def _lines_text(rng, n_lines, keys, p_key=0.5, width=(0, 6)):
    out = []
    for _ in range(n_lines):
        body = bytes(rng.choice(b"xyz") for _ in range(rng.randint(*width)))
        out.append(body + (rng.choice(keys) if rng.random() < p_key else b"") + NL)
    return b"".join(out)


@pytest.mark.parametrize("edge", [32, 2048])
def test_piece_and_fragment_boundaries_around_a_mask_word_and_a_rank_block(edge):
    rng = random.Random(edge)
    p = Pair([b"abc", b"b\n"], 4)
    for delta_d in (-2, -1, 0, 1):  # a delimiter at edge + delta_d ...
        text = bytearray(rng.choice(b"axyz") for _ in range(2 * edge + 40))
        text[edge + delta_d] = 10
        text[5] = 10
        text[edge - 10:edge - 7] = b"abc"
        text[2 * edge:2 * edge + 2] = b"b\n"
        for delta_c in (-1, 0, 1):  # ... and a cut at edge + delta_c, in one call as two pieces of two sequences and in two calls
            c = edge + delta_c
            p.step([bytes(text[:c]), bytes(text[c:])], [1, 3], invert=delta_c == 0)
            p.step([b"", b""], [3, 1], final=True)
            _feed_one(p, bytes(text), [c], seq=0, align=(edge + delta_d) % 16)


def test_32_and_2048_fragments_and_more_than_256_dropped_runs():
    rng = random.Random(3)
    p = Pair([b"abc", b"c\n"], 3)
    for n_lines in (31, 32, 33, 2047, 2048, 2049):
        text = _lines_text(rng, n_lines, [b"abc"], 0.5, (0, 3))  # kept and dropped lines alternate at random: ~n / 4 runs
        text = text[:-1] if n_lines % 2 else text
        cuts = sorted(rng.randint(0, len(text)) for _ in range(3))
        pieces = _cut(text, cuts)
        w = p.step([text], [1], final=True)  # one piece: exactly n_lines fragments in one call
        assert w[3]["n_recs"] == n_lines and (n_lines < 2000 or 256 < w[0].size < n_lines - 256)
        p.step(pieces[:2] + [b""], [2, 0, 1])
        p.step(pieces[2:], [2, 0], invert=True, hits=True)
        p.step([b"", b"", b""], [0, 1, 2], final=True)
        _feed_one(p, text, cuts, seq=1)


def test_invert_with_kept_empty_stretches():
    p = Pair([b"a"], 2)
    text = b"\n\n\na\n\n" + b"\n" * 70 + b"a\n\n"
    for cuts in ([1], [2, 3], [40, 41], [4, 5]):
        assert _feed_one(p, text, cuts, invert=True) == [NL] * 3 + [NL] * 71 + [NL]
        _feed_one(p, text, cuts)


# ---- many pieces, many sequences ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D,n_seqs", [(1, 1), (2, 3), (33, 257), (257, 257), (3, 3)])
def test_pieces_over_sequences_with_permuted_ids_and_subsets(D, n_seqs):
    rng = random.Random(D * 1000 + n_seqs)
    p = Pair([b"ab", b"bca", b"c\n"], n_seqs)
    for call in range(4):
        ids = rng.sample(range(n_seqs), D if call != 2 else max(1, D // 2))  # (the third call names a subset)
        pieces = [bytes(rng.choices(b"abc\n\x00", [4, 3, 2, 2, 1])[0] for _ in range(rng.choice([0, 0, 1, 1, 2, 5, 9, 40])))
                  for _ in ids]
        if call == 1:
            pieces[0] = NL
        p.step(pieces, ids, invert=call == 1, final=call == 3, hits=call == 0)
    assert all(p.feed.position(i) == (0, 0) for i in ids)


@pytest.mark.parametrize("lmax", [1, 3, 64])
def test_key_sets_of_lmax_1_3_and_64(lmax):
    rng = random.Random(lmax)
    long_key = bytes(rng.choice(b"abc") for _ in range(lmax))
    keys = sorted({long_key, long_key[: max(1, lmax // 2)], b"c"[:1] if lmax > 1 else long_key})
    p = Pair(keys, 2)
    for trial in range(6):
        body = [bytes(rng.choice(b"abx") for _ in range(rng.randint(0, 90))) + (long_key if rng.random() < 0.6 else b"") + NL
                for _ in range(6)]
        text = b"".join(body) + b"tail" + long_key
        k = text.find(long_key)
        cuts = sorted({max(0, k + rng.randint(0, lmax)), rng.randint(0, len(text)), rng.randint(0, len(text))})
        _feed_one(p, text, cuts, seq=trial % 2, invert=trial % 3 == 0)
    # a key longer than every piece: 64 bytes over pieces of 7
    text = b"xx" + long_key + b"yy\nno\n" + long_key[:-1] + NL
    _feed_one(p, text, list(range(7, len(text), 7)))


def test_corpus_slices_at_every_misalignment():
    rng = random.Random(15)
    p = Pair([b"abc", b"b\n"], 2)
    text = _lines_text(rng, 12, [b"abc", b"b"], 0.5, (0, 9)) + b"open ab"
    for align in range(1, 16):
        _feed_one(p, text, [align, 17 + align, len(text) - align], seq=align % 2, invert=align % 4 == 0, align=align)


def test_with_one_block_grids(monkeypatch):
    monkeypatch.setenv("AHA_GREP_BLOCKS", "1")  # every workgroup loops
    rng = random.Random(9)
    p = Pair([b"abc", b"c\n"], 300)
    text = _lines_text(rng, 2100, [b"abc"], 0.5, (0, 3))
    _feed_one(p, text, sorted(rng.randint(0, len(text)) for _ in range(3)))
    ids = rng.sample(range(300), 290)
    for call in range(3):
        p.step([bytes(rng.choices(b"abc\n", [3, 2, 3, 2])[0] for _ in range(rng.randint(0, 12))) for _ in ids], ids, final=call == 2)


def test_a_folded_handle_gives_the_callers_spelling():
    p = Pair([b"aBc", b"B\n"], 2, fold=True)
    assert _feed_one(p, b"xAbC\nno\nAB\nab", [3, 9]) == [b"xAbC\n", b"AB\n"]
    assert _feed_one(p, b"xAbC\nno\nAB\nab", [2, 12], invert=True) == [b"no\n", b"ab"]
    rng = random.Random(2)
    for _ in range(10):
        text = bytes(rng.choice(b"aAbBcC\n") for _ in range(rng.randint(0, 80)))
        _feed_one(p, text, [rng.randint(0, len(text)) for _ in range(3)], seq=1)


def test_random_sequences_over_a_small_alphabet():
    """a few hundred sequences, a few hundred bytes each, cut at random: the sequences of one key set share a feed, call t
    feeds piece t of every sequence that still has one (FINAL calls apart: the flag is the call's)"""
    rng = random.Random(20262)
    n_cases = 0
    for group in range(6):
        lmax = [1, 2, 3, 4, 6, 3][group]
        keys = sorted({bytes(rng.choice(b"abc\n") for _ in range(rng.randint(1, lmax))) for _ in range(rng.randint(1, 5))})
        S = 50
        p = Pair(keys, S)
        texts = [bytes(rng.choices(b"abc\n\x00", [4, 3, 2, 2, 1])[0] for _ in range(rng.randint(0, 300))) for _ in range(S)]
        cut = [_cut(t, [rng.randint(0, len(t)) for _ in range(rng.randint(0, 5))]) for t in texts]
        holders = [fgs.Holder() for _ in range(S)]
        lines = [[] for _ in range(S)]
        invert = group % 2 == 1
        for t in range(6):
            for final in (False, True):
                ids = [s for s in range(S) if t < len(cut[s]) and (t == len(cut[s]) - 1) == final]
                if not ids:
                    continue
                rng.shuffle(ids)
                pieces = [cut[s][t] for s in ids]
                kept, out, roo, info = p.step(pieces, ids, invert, final, align=(t * 5 + group) % 16)
                raw = out.tobytes()
                pko = info["piece_kept_offsets"]
                for d, s in enumerate(ids):
                    mine = [raw[int(roo[j]):int(roo[j + 1])] for j in range(int(pko[d]), int(pko[d + 1]))]
                    lines[s] += holders[s].step(pieces[d], mine, int(info["piece_head"][d]), int(info["piece_hold"][d]), final)
        for s in range(S):
            assert lines[s] == fgs.whole(p.count, texts[s], NL, invert), (keys, texts[s], [len(x) for x in cut[s]])
            n_cases += 1
    assert n_cases == 300


# ---- the laws ----------------------------------------------------------------------------------------------------------------
def test_capacity_reports_both_numbers_writes_nothing_and_the_retry_is_a_first_call():
    p = Pair([b"abc"], 2)
    p.step([b"xxab"], [0])
    pieces, ids = [b"c\nq\nabc\nw", b"abc\nabc\nz"], [0, 1]
    want = fgs.Feed(p.count, p.W, 2)
    want.seqs[0].push(b"xxab")
    wk, wo, wr, info = want.call(pieces, ids)
    assert (wk.size, wo.size) == (4, 14)
    for cap_recs, cap_bytes in ((3, 14), (4, 13), (0, 0), (3, 13)):
        res = p.device(pieces, ids, cap_recs=cap_recs, cap_bytes=cap_bytes, room=(4, 14))
        assert res["rc"] == N.AHA_E_CAPACITY and (res["n_required"], res["bytes_required"]) == (4, 14), res
        assert Pair.untouched(res)
        assert p.feed.position(0) == (4, 0) and p.feed.position(1) == (0, 0)  # no sequence moved
    p.step(pieces, ids)  # with room: what the model gives for a first call
    assert p.feed.position(0) == (13, 0)


def test_refusals_change_nothing_and_reset_restores():
    p = Pair([b"abc", b"b\n"], 4)
    p.step([b"xab", b"q\nab"], [0, 1])
    res = p.device([b"c\n", b"c\n"], [0, 0], room=(2, 4))  # a duplicate id
    assert res["rc"] == N.AHA_E_INVALID and Pair.untouched(res)
    res = p.device([b"c\n"], [4], room=(2, 4))  # an id beyond the feed
    assert res["rc"] == N.AHA_E_INVALID and Pair.untouched(res)
    other = Pair([b"abc", b"b\n"], 4, delim=b";")
    other.feed, other.model = p.feed, p.model
    res = other.device([b"c;"], [2], room=(2, 4))  # another delimiter
    assert res["rc"] == N.AHA_E_INVALID and Pair.untouched(res)
    assert p.feed.position(0) == (3, 0) and p.feed.position(2) == (0, 0)
    p.step([b"c\n", b"c\n"], [0, 1])  # nothing changed: the open records close as the model says
    # a match call in between: grep is refused on that sequence, and on no other
    p.step([b"ab"], [3])
    hits, _, _ = p.feed.match_batch(np.frombuffer(b"c", dtype=np.uint8), np.array([0, 1], dtype=np.uint64), np.array([3], dtype=np.uint32))
    assert len(hits) == 1
    res = p.device([b"\n", b"abc\n"], [3, 2], room=(2, 5))
    assert res["rc"] == N.AHA_E_INVALID and Pair.untouched(res) and p.feed.position(3) == (3, 0) and p.feed.position(2) == (0, 0)
    p.step([b"abc\n"], [2])
    p.feed.reset(3)
    p.model.seqs[3] = fgs.Sequence(p.count, p.W)
    p.step([b"c\nabc", b"x"], [3, 2])
    p.feed.reset()  # all of them: the grep state is cleared with the rest
    p.model = fgs.Feed(p.count, p.W, 4)
    p.step([b"c\n", b"c\n"], [2, 3], invert=True)


def test_argument_errors_before_any_device_work():
    import torch

    m = AC.compile([b"ab"])
    L = N.lib()
    corpus = torch.zeros(8, dtype=torch.uint8, device="cuda")
    offs, ids = _cuda([0, 8], np.int64), _cuda([0], np.int32)
    buf = torch.zeros(64, dtype=torch.int64, device="cuda")
    nk = C.c_uint64(9)

    def call(f, flags=0, kept=None, roo=None, cap_recs=0, out=None, cap_bytes=0, n=True):
        return L.aha_feed_grep_batch_device(f._h, corpus.data_ptr(), offs.data_ptr(), ids.data_ptr(), 1, 8, 10, flags, kept, roo,
                                            cap_recs, out, cap_bytes, None, None, None, None, None, None, None,
                                            C.byref(nk) if n else None, None, None, None)

    f = m.feed(2)
    for bad in (dict(flags=4), dict(flags=0x80000000), dict(n=False), dict(cap_recs=3), dict(cap_bytes=5),
                dict(out=corpus.data_ptr() + 2, cap_bytes=4)):
        assert call(f, **bad) == N.AHA_E_INVALID, bad
        assert nk.value == 9 and f.position(0) == (0, 0)
    assert call(m.feed(2, chars=True)) == N.AHA_E_INVALID
    from aha_amd import BitArray

    bits = BitArray(256)
    for c in range(256):
        bits[c] = c in (32, 10)
    assert call(m.feed(2, sep=bits)) == N.AHA_E_INVALID  # a feed with a separator filter: a follow-up
    assert call(f, kept=buf.data_ptr(), cap_recs=8) == 0 and nk.value == 0 and f.position(0) == (8, 0)  # (the call as such is fine)


def test_ids_only_gives_the_same_ids_and_twice_the_same_bytes():
    rng = random.Random(4)
    text = _lines_text(rng, 40, [b"abc"], 0.5)
    cuts = [50, 90]
    a, b = Pair([b"abc"], 1), Pair([b"abc"], 1)
    for i, piece in enumerate(_cut(text, cuts)):
        wa = a.step([piece], [0], final=i == 2)
        wb = b.step([piece], [0], final=i == 2, ids_only=True)  # out == NULL: the same ids and offsets, no byte written
        assert np.array_equal(wa[0], wb[0]) and np.array_equal(wa[2], wb[2])
    c = Pair([b"abc"], 1)
    for i, piece in enumerate(_cut(text, cuts)):  # an identical call sequence: identical bytes (the model is deterministic)
        c.step([piece], [0], final=i == 2)


def test_grep_match_and_count_calls_on_different_sequences_mix():
    p = Pair([b"abc", b"b\n"], 4)
    o = orc.AC.compile(p.keys)
    one = lambda b: (np.frombuffer(b, dtype=np.uint8), np.array([0, len(b)], dtype=np.uint64))  # noqa: E731
    p.step([b"xab"], [0])
    hits, _, bases = p.feed.match_batch(*one(b"xxab"), np.array([1], dtype=np.uint32))
    assert len(hits) == 0
    p.step([b"c\nb"], [0])
    hits, _, bases = p.feed.match_batch(*one(b"c\nb\n"), np.array([1], dtype=np.uint32))
    assert [(int(h["start"]) + 4, int(h["end"]) + 4) for h in hits] == [(int(s), int(e)) for s, e, _ in o.match(b"xxabc\nb\n", chars=False).tolist()]
    kc, _, _ = p.feed.count_batch(*one(b"abcabc"), np.array([2], dtype=np.uint32))
    assert kc.tolist() == [2, 0]
    p.step([b"\nab", b"q"], [0, 3], final=True)
    kc, _, _ = p.feed.count_batch(*one(b"b\n"), np.array([2], dtype=np.uint32))
    assert kc.tolist() == [0, 1]


def test_host_entry_against_the_model():
    rng = random.Random(6)
    p = Pair([b"ab", b"bca", b"c\n"], 5)
    for call in range(5):
        ids = rng.sample(range(5), rng.randint(1, 5))
        pieces = [bytes(rng.choices(b"abc\n", [4, 3, 2, 2])[0] for _ in range(rng.choice([0, 1, 3, 30, 70]))) for _ in ids]
        p.host(pieces, ids, invert=call % 2 == 1, final=call == 4)
    p.host([], [])  # a call of no pieces
    p.step([], [])


def test_grepper_over_random_pushes_equals_grep_of_the_joined_text():
    rng = random.Random(12)
    m = AC.compile([b"abc", b"b\n", b"ca"])
    for invert in (False, True):
        feed = m.feed(3)
        g = feed.grepper(invert=invert)
        texts, got = [b"", b"", b""], [[], [], []]
        for _ in range(40):
            s = rng.randrange(3)
            piece = bytes(rng.choices(b"abc\n", [4, 3, 3, 2])[0] for _ in range(rng.choice([0, 1, 2, 5, 17, 60])))
            texts[s] += piece
            got[s] += g.push(s, piece)
        for s in range(3):
            got[s] += g.finish(s)
            assert got[s] == m.grep(texts[s], invert=invert), (s, invert)
            assert feed.position(s) == (0, 0)
