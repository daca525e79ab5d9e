"""GPU tests of ASCII case-insensitive handles (AHA_OPT_FOLD_ASCII, include/aha_hip.h).  THE RULE: every call on a folded
handle gives, bit for bit, what the same call gives on an ordinary handle compiled from fold(keys) over fold(text).  Expected
values come from the CPU oracle compiled from fold(keys) and run over fold(text) -- the oracle is never given the flag, it has
none -- and from the numpy statements of the count / cover contracts on the oracle's hits.  The three exceptions: redaction
keeps the ORIGINAL bytes outside the mask, keys keep their spelling, the caller's device corpus is never written."""
import ctypes as C
import os
import random

import numpy as np
import pytest
import torch

import coversim
import doccountsim
import pyoracle as orc
from aha_amd import AC, ACGroup, BitArray, synth
from aha_amd import _native as N
from engine_variants import VARIANTS, use_variant

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def fold(a):
    a = np.frombuffer(a, dtype=np.uint8) if isinstance(a, (bytes, bytearray)) else np.asarray(a, dtype=np.uint8)
    return np.where((a >= 65) & (a <= 90), a + 32, a).astype(np.uint8)


def mix_case(a, seed):
    """each ASCII letter upper-cased with probability 1/2"""
    a = np.array(a, dtype=np.uint8, copy=True)
    flip = np.random.default_rng(seed).random(a.size) < 0.5
    low = (a >= 97) & (a <= 122)
    a[low & flip] -= 32
    return a


def as_list(h):
    return [(int(x["start"]), int(x["end"]), int(x["value"])) for x in h]


def hits_list(hs):
    return [(h.start, h.end, h.value) for h in hs]


def dev_match(m, d_corpus, d_doc, cap, **kw):
    out = torch.zeros((cap + 8, 3), dtype=torch.int32, device=DEV)
    dho = torch.zeros(d_doc.numel(), dtype=torch.int64, device=DEV)
    n = m.match_batch_device(d_corpus, d_doc, out, dho, **kw)
    return out[:n].cpu().numpy(), dho.cpu().numpy().astype(np.uint64), n


def mixed_cfg(cfg, n_bytes, K=None, doc_bytes=1 << 16):
    blob, koffs, nf = synth.keys(cfg, K=K)
    corpus, doc = synth.corpus(cfg, blob, koffs, nf, n_bytes=n_bytes, doc_bytes=doc_bytes)
    assert np.array_equal(fold(blob), blob)  # (the synthetic keys are lower case: mixing cannot make two of them equal)
    return mix_case(blob, 11), koffs, mix_case(corpus, 12), doc


def test_he_she_hers_in_any_case():
    m = AC.compile(["He", "SHE", "hers"], fold_ascii=True)
    o = orc.AC.compile(["he", "she", "hers"])
    assert m.fold_ascii
    assert hits_list(m.match("uSHerS")) == as_list(o.match("ushers")) == [(1, 4, 1), (2, 4, 0), (2, 6, 2)]
    assert hits_list(m.match(b"uSHerS")) == as_list(o.match(b"ushers"))
    assert m[1] == "SHE" and m["she"] == 1
    # neutrality: a plain handle matches the bytes as they are
    assert hits_list(AC.compile(["He", "SHE", "hers"]).match("uSHerS")) == [(2, 4, 0)]
    assert hits_list(AC.compile(["he", "she", "hers"]).match("uSHerS")) == []


@pytest.mark.parametrize("n_bytes", [1 << 20, 1 << 26])
def test_cfg2_filter_engine_fused(n_bytes):
    blob, koffs, corpus, doc = mixed_cfg(2, n_bytes)
    N_ = corpus.size
    f = AC.compile_packed(blob, koffs, fold_ascii=True)
    p = AC.compile_packed(fold(blob), koffs)
    o = orc.AC.compile_packed(fold(blob), koffs)
    oh, od = o.match_batch(fold(corpus), doc)
    assert len(oh) > 0
    assert f.info == p.info and f.info["filter_prefix_bytes"] > 0
    # host entry
    gh, gd = f.match_batch(corpus, doc)
    assert np.asarray(gh).tobytes() == oh.tobytes() and np.array_equal(np.asarray(gd, dtype=np.uint64), od)
    # device entry: engine 5, nothing thrown away, no staging copy, the caller's corpus untouched
    dc = torch.from_numpy(corpus).to(DEV)
    dd = torch.from_numpy(doc.astype(np.int64)).to(DEV)
    dcf = torch.from_numpy(fold(corpus)).to(DEV)
    before = dc.clone()
    for m in (f, p):
        m.release_scratch()
        m.set_profiling(True)
    def fused_no_copy(what):
        """the last device call of f: the filter engine, nothing handed back, and nothing of N bytes held (no staged copy)"""
        t = f.last_timing()
        assert t["engine"] == 5 and t["repeats"] == 0, (what, t)
        assert f.scratch_bytes() < p.scratch_bytes() + N_, (what, f.scratch_bytes(), p.scratch_bytes(), N_)

    hits, dho, n = dev_match(f, dc, dd, len(oh))
    assert n == len(oh) and hits.tobytes() == oh.tobytes() and np.array_equal(dho, od)
    t = f.last_timing()
    assert t["engine"] == 5 and t["repeats"] == 0, t
    hits_p, _, _ = dev_match(p, dcf, dd, len(oh))
    assert hits_p.tobytes() == oh.tobytes()
    assert p.last_timing()["engine"] == 5
    assert f.scratch_bytes() < p.scratch_bytes() + N_, (f.scratch_bytes(), p.scratch_bytes(), N_)
    # char offsets (plain ASCII: the same numbers) through the filter engine's CHARS form
    hits_c, dho_c, _ = dev_match(f, dc, dd, len(oh), chars=True)
    ohc, odc = o.match_batch(fold(corpus), doc, chars=True)
    assert hits_c.tobytes() == ohc.tobytes() and np.array_equal(dho_c, odc)
    # counts
    K = f.n_keys
    want_kc = np.bincount(oh["value"], minlength=K).astype(np.uint64)
    kc, cd = f.count_batch(corpus, doc)
    assert np.array_equal(kc, want_kc) and np.array_equal(cd, od)
    dkc = torch.zeros(K, dtype=torch.int64, device=DEV)
    ddho = torch.zeros(doc.size, dtype=torch.int64, device=DEV)
    p.release_scratch()
    p.count_batch_device(dcf, dd, dkc, ddho)  # (the plain handle's scratch for the same call: full-size regions)
    f.release_scratch()
    assert f.count_batch_device(dc, dd, dkc, ddho) == len(oh)
    fused_no_copy("count")
    assert np.array_equal(dkc.cpu().numpy().astype(np.uint64), want_kc) and np.array_equal(ddho.cpu().numpy().astype(np.uint64), od)
    # document counts
    want_pairs, want_dpo = doccountsim.doc_counts(oh["value"], od)
    pairs, dpo = f.doc_counts_batch(corpus, doc)
    assert pairs.tobytes() == want_pairs.tobytes() and np.array_equal(dpo, want_dpo)
    dout = torch.zeros((want_pairs.size + 4, 2), dtype=torch.int32, device=DEV)
    ddpo = torch.zeros(doc.size, dtype=torch.int64, device=DEV)
    p.release_scratch()
    p.doc_counts_batch_device(dcf, dd, dout, ddpo)  # (the plain handle's scratch for the same call: the hits are held there too)
    f.release_scratch()
    npairs, nh = f.doc_counts_batch_device(dc, dd, dout, ddpo)
    assert (npairs, nh) == (want_pairs.size, len(oh))
    fused_no_copy("doc_counts")
    assert dout[:npairs].cpu().numpy().tobytes() == want_pairs.tobytes()
    assert np.array_equal(ddpo.cpu().numpy().astype(np.uint64), want_dpo)
    # cover and redaction: the mask of the folded match, the ORIGINAL bytes outside it
    want_mask, _, want_dc, want_nc = coversim.cover_all(oh["start"], oh["end"], corpus, doc, od, 0x2A)
    cov = coversim.unpack(want_mask, N_)
    want_red = coversim.redacted(corpus, cov, 0x2A)  # (of the mixed-case corpus)
    assert not np.array_equal(want_red, coversim.redacted(fold(corpus), cov, 0x2A))
    mask, dcov = f.cover_batch(corpus, doc)
    assert np.array_equal(mask, want_mask) and np.array_equal(dcov, want_dc)
    red, dcov = f.redact_batch(corpus, doc)
    assert np.array_equal(red, want_red) and np.array_equal(dcov, want_dc)
    dmask = torch.zeros(want_mask.size, dtype=torch.int32, device=DEV)
    dred = torch.zeros(N_, dtype=torch.uint8, device=DEV)
    ddc = torch.zeros(doc.size - 1, dtype=torch.int64, device=DEV)
    p.release_scratch()
    p.cover_batch_device(dcf, dd, dmask, dred, 0x2A, ddc)
    f.release_scratch()
    assert f.cover_batch_device(dc, dd, dmask, dred, 0x2A, ddc) == (want_nc, len(oh))
    fused_no_copy("cover")
    assert np.array_equal(dmask.cpu().numpy().view(np.uint32), want_mask)
    assert np.array_equal(dred.cpu().numpy(), want_red)
    assert np.array_equal(ddc.cpu().numpy().astype(np.uint64), want_dc)
    # no device entry above wrote the caller's corpus
    assert torch.equal(dc, before)
    # in place: the fill bytes only
    inplace = dc.clone()
    assert f.cover_batch_device(inplace, dd, None, inplace, 0x2A, None) == (want_nc, len(oh))
    assert np.array_equal(inplace.cpu().numpy(), want_red)


@pytest.mark.parametrize("cfg,n_bytes,K", [(3, 1 << 24, None), (5, 1 << 22, 200_000)])
def test_staged_engines_aligned_and_unaligned(cfg, n_bytes, K, monkeypatch):
    if cfg == 5:  # the byte-level engine over the wide image (the key set by itself gets a character-level image)
        monkeypatch.setenv("AHA_ENGINE", "v2")
    blob, koffs, corpus, doc = mixed_cfg(cfg, n_bytes, K=K)
    assert (blob != fold(blob)).any() and (corpus != fold(corpus)).any()
    N_ = corpus.size
    f = AC.compile_packed(blob, koffs, fold_ascii=True, force_wide=cfg == 5)
    o = orc.AC.compile_packed(fold(blob), koffs)
    oh, od = o.match_batch(fold(corpus), doc)
    ohc, odc = o.match_batch(fold(corpus), doc, chars=True)
    assert f.info["filter_prefix_bytes"] == 0
    if cfg == 3:
        assert f.info["unit_enabled"] == 1
    else:
        assert f.info["slot_bytes"] == 8 and f.info["unit_enabled"] == 0
    f.set_profiling(True)
    K_ = f.n_keys
    want_kc = np.bincount(oh["value"], minlength=K_).astype(np.uint64)
    want_mask, _, want_dc, want_nc = coversim.cover_all(oh["start"], oh["end"], corpus, doc, od, 0x23)
    want_red = coversim.redacted(corpus, coversim.unpack(want_mask, N_), 0x23)
    big = torch.zeros(N_ + 64, dtype=torch.uint8, device=DEV)
    dd = torch.from_numpy(doc.astype(np.int64)).to(DEV)
    for shift in (0, 5):
        dc = big[shift:shift + N_]
        dc.copy_(torch.from_numpy(corpus))
        assert dc.data_ptr() % 16 == (5 if shift else 0)
        before = dc.clone()
        hits, dho, n = dev_match(f, dc, dd, len(oh))
        assert n == len(oh) and hits.tobytes() == oh.tobytes() and np.array_equal(dho, od)
        assert f.last_timing()["engine"] == (4 if cfg == 3 else 2)
        hits, dho, n = dev_match(f, dc, dd, len(ohc), chars=True)
        assert hits.tobytes() == ohc.tobytes() and np.array_equal(dho, odc)
        dkc = torch.zeros(K_, dtype=torch.int64, device=DEV)
        assert f.count_batch_device(dc, dd, dkc, None) == len(oh)
        assert np.array_equal(dkc.cpu().numpy().astype(np.uint64), want_kc)
        dmask = torch.zeros(want_mask.size, dtype=torch.int32, device=DEV)
        dred = torch.zeros(N_, dtype=torch.uint8, device=DEV)
        assert f.cover_batch_device(dc, dd, dmask, dred, 0x23, None) == (want_nc, len(oh))
        assert np.array_equal(dmask.cpu().numpy().view(np.uint32), want_mask)
        assert np.array_equal(dred.cpu().numpy(), want_red)
        assert torch.equal(dc, before)


def test_count_and_cover_in_document_ranges_stay_fused(monkeypatch):
    """full-size regions beyond the bound: the call counts ranges of whole documents.  A folded handle's aligned ranges go to
    the filter engine as the caller's bytes (no copy); an unaligned range is folded on its way into the range's scratch."""
    blob, koffs, corpus, doc = mixed_cfg(2, 1 << 20, doc_bytes=(1 << 14) + 16 * 3)
    N_ = corpus.size
    f = AC.compile_packed(blob, koffs, fold_ascii=True)
    o = orc.AC.compile_packed(fold(blob), koffs)
    oh, od = o.match_batch(fold(corpus), doc)
    want_kc = np.bincount(oh["value"], minlength=f.n_keys).astype(np.uint64)
    want_mask, _, want_dc, want_nc = coversim.cover_all(oh["start"], oh["end"], corpus, doc, od, 0x2A)
    want_red = coversim.redacted(corpus, coversim.unpack(want_mask, N_), 0x2A)
    monkeypatch.setenv("AHA_COUNT_REGION_BYTES", str(1 << 20))
    # (the host entries: their offsets are checked on the host, which is the way into the ranges)
    f.set_profiling(True)
    kc, cd = f.count_batch(corpus, doc)
    t = f.last_timing()
    assert t["repeats"] >= 2 and t["engine"] == 5, t  # (ranges; the last one through the filter engine)
    assert np.array_equal(kc, want_kc) and np.array_equal(cd, od)
    mask, dcov = f.cover_batch(corpus, doc)
    assert f.last_timing()["repeats"] >= 2
    assert np.array_equal(mask, want_mask) and np.array_equal(dcov, want_dc)
    red, dcov = f.redact_batch(corpus, doc)
    assert np.array_equal(red, want_red) and np.array_equal(dcov, want_dc)


ALPHABET = ["a", "A", "b", "B", "@", "[", "我", "是"]


def small_case(seed, n_keys=60, n_text=6000):
    rng = random.Random(seed)
    keys, seen = [], set()
    while len(keys) < n_keys:
        k = "".join(rng.choice(ALPHABET) for _ in range(rng.randint(1, 6))).encode()[:6]
        try:
            k.decode()
        except UnicodeDecodeError:
            continue
        if k and fold(k).tobytes() not in seen:
            seen.add(fold(k).tobytes())
            keys.append(k)
    docs = ["".join(rng.choice(ALPHABET) for _ in range(rng.randint(0, n_text // 8))).encode() for _ in range(9)]
    corpus = np.frombuffer(b"".join(docs), dtype=np.uint8)
    doc = np.concatenate([[0], np.cumsum([len(d) for d in docs])]).astype(np.uint64)
    return keys, corpus, doc


@pytest.mark.parametrize("variant", VARIANTS)
def test_engine_variants_see_folded_text(variant, monkeypatch):
    use_variant(variant, monkeypatch)
    for seed, min_len in ((1, 1), (2, 3)):
        keys, corpus, doc = small_case(seed)
        keys = [k for k in keys if len(k) >= min_len]
        f = AC.compile(keys, fold_ascii=True)
        o = orc.AC.compile([fold(k).tobytes() for k in keys])
        for chars in (False, True):
            oh, od = o.match_batch(fold(corpus), doc, chars=chars)
            for cap in (None, 8):  # (8: the slab pipeline, then the exact count through the two-pass engine)
                gh, gd = f.match_batch(corpus, doc, chars=chars, cap=cap)
                assert np.asarray(gh).tobytes() == oh.tobytes(), (variant, seed, chars, cap)
                assert np.array_equal(np.asarray(gd, dtype=np.uint64), od)
        oh, od = o.match_batch(fold(corpus), doc)
        kc, cd = f.count_batch(corpus, doc)
        assert np.array_equal(kc, np.bincount(oh["value"], minlength=len(keys)).astype(np.uint64)) and np.array_equal(cd, od)
        want_mask, _, want_dc, _ = coversim.cover_all(oh["start"], oh["end"], corpus, doc, od, 0x2A)
        red, dcov = f.redact_batch(corpus, doc)
        assert np.array_equal(red, coversim.redacted(corpus, coversim.unpack(want_mask, corpus.size), 0x2A))
        assert np.array_equal(dcov, want_dc)


def test_dense_batch_handed_back_by_the_filter_uses_the_staged_copy():
    keys = ["ABcd", "bcDA", "CDab", "dabC", "error", "WARNing"]
    f = AC.compile(keys, fold_ascii=True)
    assert f.info["filter_prefix_bytes"] > 0
    o = orc.AC.compile([k.lower() for k in keys])
    dense = np.frombuffer(b"aBCd" * 8192 + b" ERROR warNING " * 10, dtype=np.uint8)
    doc = np.array([0, dense.size], dtype=np.uint64)
    oh, od = o.match_batch(fold(dense), doc)
    dc = torch.from_numpy(dense.copy()).to(DEV)
    dd = torch.from_numpy(doc.astype(np.int64)).to(DEV)
    f.release_scratch()
    f.set_profiling(True)
    hits, dho, n = dev_match(f, dc, dd, len(oh))
    assert n == len(oh) and hits.tobytes() == oh.tobytes() and np.array_equal(dho, od)
    t = f.last_timing()
    assert t["repeats"] >= 1 and t["engine"] == 2, t
    assert f.scratch_bytes() >= dense.size  # (the folded copy)
    assert np.array_equal(dc.cpu().numpy(), dense)


def test_separator_filter_tests_the_folded_neighbours():
    keys = ["Foo", "BAR", "o", "ba"]
    f = AC.compile(keys, fold_ascii=True)
    o = orc.AC.compile([k.lower() for k in keys])
    # every byte value a separator except the lower-case letters: an upper-case neighbour must block like its lower case
    sep = BitArray(256)
    bits = [c for c in range(256) if not 97 <= c <= 122]
    for c in bits:
        sep[c] = True
    text = b"Foo fooBAR XfOO foo,BAR barX Obar oO o Ba"
    want = as_list(o.match(fold(text).tobytes(), sep=(256, bits)))
    assert want and want != as_list(o.match(fold(text).tobytes()))
    assert as_list(f.match_array(text, sep)) == want
    # ... and differs from the oracle run over the unfolded neighbours (upper case would then count as a separator)
    assert want != as_list(o.match(text, sep=(256, bits)))
    kc = f.count(text, sep=sep)
    assert np.array_equal(kc, np.bincount([v for _, _, v in want], minlength=4).astype(np.uint64))


@pytest.mark.parametrize("intersectable", [False, True])
def test_match_longest_with_stale_ends_that_exist_only_after_folding(intersectable):
    keys = ["Bbc", "bcc", "b", "X", "xy", "Xyz", "我A", "我a是"]
    f = AC.compile(keys, fold_ascii=True)
    low = [fold(k.encode()).tobytes() for k in keys]
    o = orc.AC.compile(low)
    assert o.stale_ends() > 0
    assert orc.AC.compile([k.encode() for k in keys]).stale_paths() != o.stale_paths()
    rng = random.Random(5)
    for _ in range(40):
        text = "".join(rng.choice(["a", "A", "b", "B", "c", "C", "d", "x", "X", "y", "Z", "z", "我", "是", " "]) for _ in range(rng.randint(1, 80)))
        for t in (text, text.encode()):
            tf = t.lower() if isinstance(t, str) else fold(t).tobytes()
            want = as_list(o.match_longest(tf, intersectable))
            got = hits_list(f.match_longest(t, intersectable))
            assert got == want, (t, intersectable)


@pytest.mark.parametrize("chars", [False, True])
def test_feed_pieces_cut_inside_a_key_with_halves_of_different_case(chars):
    keys = ["Error", "WARNING", "rro", "我是Q", "ing"]
    f = AC.compile(keys, fold_ascii=True)
    o = orc.AC.compile([fold(k.encode()).tobytes() for k in keys])
    whole = "xxERror: warnING 我是q eRRor WARning erRoR我是Q!".encode()
    cuts = [0, 4, 5, 13, 14, 21, 23, 30, 37, len(whole)]  # inside "ERr|or", "warn|ING", the CJK character, ...
    oh = o.match(fold(whole).tobytes(), chars=False)
    lead = np.concatenate([[0], np.cumsum((np.frombuffer(whole, dtype=np.uint8) & 0xC0) != 0x80)])
    ohc = o.match(fold(whole).tobytes(), chars=True)
    want_all = as_list(ohc if chars else oh)
    ends_b = oh["end"]
    fd = f.feed(1, chars=chars)
    got_all, counts = [], np.zeros(len(keys), dtype=np.uint64)
    for i in range(len(cuts) - 1):
        piece = whole[cuts[i]:cuts[i + 1]]
        in_piece = (ends_b > cuts[i]) & (ends_b <= cuts[i + 1])
        if i % 2 == 0:
            got = hits_list(fd.match(0, piece))
            got_all += got
            assert got == [h for h, inside in zip(want_all, in_piece) if inside], i
        else:  # a count call moves the feed on like a match call
            kc = fd.count(0, piece)
            assert np.array_equal(kc, np.bincount(oh["value"][in_piece], minlength=len(keys)).astype(np.uint64)), i
            got_all += [h for h, inside in zip(want_all, in_piece) if inside]
    assert got_all == want_all
    nb, nc = fd.position(0)
    assert nb == len(whole) and (not chars or nc == lead[-1])
    fd.close()


def test_replicate_load_and_group():
    blob, koffs, corpus, doc = mixed_cfg(2, 1 << 20)
    f = AC.compile_packed(blob, koffs, fold_ascii=True)
    p = AC.compile_packed(fold(blob), koffs)
    ph, pd = p.match_batch(fold(corpus), doc)
    assert len(ph) > 0
    r = f.replicate(0)
    assert r.fold_ascii and r[3] == f[3]
    ld = AC.from_bytes(f.to_bytes(), fold_ascii=True)
    assert ld.fold_ascii and [ld[i] for i in range(5)] == [f[i] for i in range(5)]
    for m in (r, ld):
        gh, gd = m.match_batch(corpus, doc)
        assert np.asarray(gh).tobytes() == np.asarray(ph).tobytes() and np.array_equal(gd, pd)
    sensitive = AC.from_bytes(f.to_bytes())
    sh, _ = sensitive.match_batch(corpus, doc)
    assert not sensitive.fold_ascii and len(sh) < len(ph)
    g = ACGroup.compile_packed(blob, koffs, [0, 0, 0], fold_ascii=True)
    gh, gd = g.match_batch(corpus, doc)
    assert np.asarray(gh).tobytes() == np.asarray(ph).tobytes() and np.array_equal(np.asarray(gd, dtype=np.uint64), pd)
    gc = g.upload_corpus(corpus, doc)  # ... and resident on the group's devices
    n, gd2 = g.match_corpus(gc)
    assert n == len(ph) and np.array_equal(np.asarray(gd2, dtype=np.uint64), pd)
    assert g.download_shard(2).tobytes() == np.asarray(ph).tobytes()
    del gc
    # the pack / unpack exchange of the folded handle's hits
    dh = torch.from_numpy(np.asarray(ph).view(np.int32).reshape(-1, 3).copy()).to(DEV)
    pairs = torch.zeros((len(ph), 2), dtype=torch.int32, device=DEV)
    back = torch.zeros_like(dh)
    f.hits_pack_device(dh, len(ph), pairs)
    f.hits_unpack_device(pairs, len(ph), back)
    torch.cuda.synchronize()
    assert torch.equal(back, dh)


def test_plain_and_folded_handles_differ_on_upper_case():
    keys = ["error", "warning"]
    text = b"Error ERROR error Warning"
    doc = [0, len(text)]
    plain, folded = AC.compile(keys), AC.compile(keys, fold_ascii=True)
    a, _ = plain.match_batch(text, doc)
    b, _ = folded.match_batch(text, doc)
    assert as_list(a) == [(12, 17, 0)]
    assert as_list(b) == [(0, 5, 0), (6, 11, 0), (12, 17, 0), (18, 25, 1)]
    assert plain.redact(text) == b"Error ERROR ***** Warning" and folded.redact(text) == b"***** ***** ***** *******"
    assert folded.redact("Error: ok") == "*****: ok"
