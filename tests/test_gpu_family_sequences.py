"""Call sequences across EVERY call family and feed on ONE handle, every call against the CPU oracle.

tests/test_gpu_call_sequences.py walks one handle through the ordered pairs of 16 forms of `match`.  The batch families
(count, document counts, cover, select, replace, records, grep) and the feed families (match, count, cover, select, replace,
separator filter, grep) lease the same Scratch set (aha_amd/csrc/handle.hpp) and each leaves state for the next call: the two
halves of v2buf[kCursor] (device_count and device_match run inside document counts, select, grep and the feeds), dc_rows_clear,
kRepSel / kRepSelSpare changing places over document ranges, grpbuf shared by records, grep and feed grep, the back-off
counters no internal pass may write, and a Feed's per-sequence device state, which must survive whatever happens to the
handle's scratch between two pieces.  Here one handle per engine variant and key set, with two feeds open on it, walks through
every ordered pair of 25 kinds (a de Bruijn walk, 626 steps), all device calls over one non-default stream.

References: the CPU oracle's hit list of a text (plain, or with the separator filter), turned into each family's answer by
selectsim, replacesim, grepsim, coversim and doccountsim; the feed sims fed the same pieces.  Nothing is compared with another
GPU call.  Every output a call writes is compared bit for bit, and what lies behind it must still hold its sentinel.  The plan
(the same for every variant; built and checked on the CPU) asserts that two consecutive successful steps differ in text, total
and document / piece count, so a call that returned the previous call's numbers or wrote nothing cannot pass.

The handle is compiled with AHA_DOCCOUNT_HIT_BYTES and AHA_SELECT_HIT_BYTES lowered so that the pool's largest text takes at
least two document ranges in document counts, select and replace and every other text one; with profiling on the walk asserts
both from aha_timing.repeats.

Feed steps: every feed kind owns subgroups of sequences of its feed (of sizes no other subgroup and no batch has); a visit
feeds the next piece of one subgroup's sequences -- never the subgroup of the step before --, the sixth piece closes them
(FINAL, reset, or finish_batch_device on the separator feed: a visit of its own) and the subgroup starts again on the next text.
On a closing step the stream law is asserted over what the GPU reported for each sequence since it started: select hits, made
absolute, are the batch select of the whole; replace bytes, concatenated, the batch replace; grep lines by the caller's
holding rule, the whole-sequence grep; separator-feed hits the filtered match of the whole.  Match, count and cover calls mix
on their sequences (as the contract lets them): there the pieces' hit counts add up to the whole's, and the hits the match
calls reported are the whole's hits that end in those pieces.  Select and replace calls mix on a subgroup of their own, which
has no stream law (include/aha_hip.h states it for sequences fed by one kind only).

Two rules asserted as the header states them, not as "nothing written": a document-count call that fails with AHA_E_CAPACITY
leaves all offsets and the first cap pairs valid; a count call refused for its offsets may have cleared key_counts (the
verdict comes from the device, behind the memset), so only its offsets are checked for sentinels.

aha_timing.n_hits, with profiling on, is asserted after every successful step that matches: a batch call's own hits (device
and host entries, after each of a host step's calls), and for a feed call the hits of its main pass -- the pieces matched as
a plain batch, for a grep call the fragments matched as documents (include/aha_hip.h: the timing of a feed call is its main
pass's).  Exempt: records (no match), empty batches and release (they publish no timing), failing steps, and a finish call
on the separator feed, which matches the sequences' contexts only and has no main pass."""
import copy
import os
import random
import threading
import time

import numpy as np
import pytest

import coversim
import doccountsim
import feedgrepsim as fgs
import feedreplacesim as frs
import grepsim
import pyoracle as orc
import replacesim
import selectsim
from aha_amd import AhaError, BitArray
from aha_amd import _native as N
from feedcoversim import FeedCoverSim
from feedsepsim import FeedSepSim
from feedsim import FeedSim
from walksim import ENGINE_VARS, PAD, S32, S64, VARIANTS, Text, ascii_keys, cjk_keys, compile_under, de_bruijn_walk

pytestmark = pytest.mark.gpu

KIND_NAMES = ["match", "count", "count_ranges", "doc_counts", "cover_mask", "cover", "select", "replace", "records", "grep",
              "grep_invert", "host", "sep", "empty", "release", "capacity", "bad_offsets", "feed_match", "feed_count",
              "feed_cover", "feed_select", "feed_replace", "feed_grep", "feed_sep", "feed_refused"]
(MATCH, COUNT, COUNT_R, DOCC, COVER_M, COVER_N, SELECT, REPLACE, RECORDS, GREP, GREP_INV, HOSTK, SEPK, EMPTYK, RELEASE, CAPF,
 BADOFF, F_MATCH, F_COUNT, F_COVER, F_SELECT, F_REPLACE, F_GREP, F_SEP, F_REFUSED) = range(25)
K = len(KIND_NAMES)
FAMILY_OF = {MATCH: "match", COUNT: "count", COUNT_R: "count", DOCC: "docc", COVER_M: "cover", COVER_N: "cover",
             SELECT: "select", REPLACE: "replace", RECORDS: "records", GREP: "grep", GREP_INV: "grep"}
FAMILIES = ["count", "docc", "cover", "select", "replace", "records", "grep"]
SEP_FAMILIES = ["count", "cover", "select", "replace", "grep"]
CAP_FORMS = ["docc", "select", "replace", "records", "grep_docs", "grep_bytes"]
REFUSALS = ["select_cap", "replace_cap", "grep_cap", "match_cap", "sep_cover", "sep_select", "sep_grep", "select_on_match"]
RANGED = ("docc", "select", "replace")  # the families cut into document ranges by the compile-time bounds
FEED_KINDS = (F_MATCH, F_COUNT, F_COVER, F_SELECT, F_REPLACE, F_GREP, F_SEP)

SEP_BITS = [32, 10]               # a space and a line feed separate
S64I = S64 - (1 << 64)            # the uint64 sentinel as the int64 torch holds
G8 = 0x5A                         # sentinel of byte buffers
FILL = 0x2A
NL = b"\n"
SEQ_BYTES = 600                   # a feed sequence: this many bytes of a pool text, in six pieces
N_PIECES = 6
PROF_SPAN, PROF_OFF = 50, 10     # profiling is off for the first PROF_OFF of every PROF_SPAN steps


def _sep():
    s = BitArray(256)
    for b in SEP_BITS:
        s[b] = True
    return s


# ---- key sets, their texts and every family's answer -----------------------------------------------------------------------

def _docs(rng, tokens, sep, shape, density, fill):
    """documents of shape[d] words: a line feed now and then (records and grep need delimiters inside the documents), keys at
    `density`, filler otherwise; a quarter of the documents has no key at all (grep drops them)"""
    out = []
    for n in shape:
        dens = 0.0 if rng.random() < 0.25 else density
        words = []
        for _ in range(n):
            r = rng.random()
            words.append("\n" if r < 0.08 else rng.choice(tokens) if r < 0.08 + dens else rng.choice(fill))
        out.append(sep.join(words))
    return out


def _pool(rng, tokens, sep, fill, scale):
    """Five texts of 8 to 64 KiB in 20 to 400 documents, some of them empty; the third is the largest by far: the one the
    compile-time bounds cut into document ranges."""
    n = lambda x: max(1, int(x * scale))  # noqa: E731
    return [
        Text(_docs(rng, tokens, sep, [n(100)] * 40, 0.15, fill)),
        Text(_docs(rng, tokens, sep, [n(34)] * 120, 0.3, fill)),
        Text(_docs(rng, tokens, sep, [n(170)] * 64, 0.6, fill)),
        Text(_docs(rng, tokens, sep, [n(420), 0] * 10, 0.2, fill)),
        Text(_docs(rng, tokens, sep, [rng.randint(0, n(18)) for _ in range(400)], 0.5, fill)),
    ]


class _Lowered:
    """the oracle of a fold_ascii handle: compiled from the (lower-case) keys, given the lowered text"""

    def __init__(self, o):
        self.o = o
        self.max_key_len = o.max_key_len

    def match(self, text, chars=None, sep=None):
        return self.o.match(bytes(text).lower(), chars=chars, sep=sep)


class KeySet:
    def __init__(self, name):
        self.name, self.fold = name, name == "fold"
        if name in ("ascii", "fold"):
            rng = random.Random(31)
            keys, nested = ascii_keys(rng)
            texts = _pool(rng, keys + nested * 4, " ", ["zz", "é", "ü9", "0", "mn"], 1.0)
            if self.fold:  # mixed-case text: the reference is the oracle over the lowered text, outputs keep the spelling
                flip = random.Random(35)
                texts = [Text([bytes(b - 32 if 97 <= b <= 122 and flip.random() < 0.3 else b for b in d) for d in t.docs])
                         for t in texts]
        else:
            rng = random.Random(32)
            keys, cps = cjk_keys(rng)
            texts = _pool(rng, cps + keys + [" "] * 100, "", ["ä", "ß", "\U0001F600", "x", "é"], 0.9)
        self.keys, self.texts = keys, texts
        self.kb = [k.encode() for k in keys]
        self.n_keys = len(keys)
        self.W = max(len(k) for k in self.kb) - 1
        raw = orc.AC.compile(keys)
        self.o = _Lowered(raw) if self.fold else raw
        self._raw = raw
        # grow, shrink, delete, same length, keep -- by the key's index
        self.repl = {}
        for i, k in enumerate(self.kb):
            r = [k + b"++", b"_", b"", b"#" * len(k), None][i % 5]
            if r is not None:
                self.repl[i] = r
        self._answers = {}
        for t in texts:
            assert 8 << 10 <= t.corpus.size <= 64 << 10 and 20 <= t.D <= 400, (name, t.corpus.size, t.D)
            assert NL[0] in t.corpus
        assert any(len(d) == 0 for t in texts for d in t.docs)
        self.largest = 2
        small = max(len(self.answers(ti, "plain").hits) for ti in range(len(texts)) if ti != self.largest)
        # a document's hits cost a range 12 to 20 bytes each (engine.cpp, document counts: 8 more per pair of the middle form):
        # every smaller text fits one range whatever its form, the largest does not fit even at 12
        self.hit_bytes = 20 * small
        assert 10 * len(self.answers(self.largest, "plain").hits) > self.hit_bytes, name

    def lowered(self, corpus):
        return np.frombuffer(corpus.tobytes().lower(), dtype=np.uint8) if self.fold else corpus

    def hit_list(self, t, flag):
        """the oracle's (hits, per-document offsets) of a batch, plain or with the separator filter"""
        if t.corpus.size == 0:
            return np.zeros(0, dtype=orc.HIT_DTYPE), np.zeros(t.D + 1, dtype=np.uint64)
        if flag == "plain":
            h, d = self._raw.match_batch(self.lowered(t.corpus), t.offs, chars=False)
            return np.ascontiguousarray(h, dtype=orc.HIT_DTYPE), d
        none = np.zeros(0, dtype=orc.HIT_DTYPE)
        parts = [self.o.match(doc, chars=False, sep=(256, SEP_BITS)) if doc else none for doc in t.docs]
        d = np.cumsum([0] + [len(p) for p in parts]).astype(np.uint64)
        return np.ascontiguousarray(np.concatenate(parts), dtype=orc.HIT_DTYPE), d

    def answers(self, ti, flag):
        """cached per (text, flag); ti may be a Text of its own (the empty batches)"""
        key = (ti if isinstance(ti, int) else id(ti), flag)
        if key not in self._answers:
            self._answers[key] = Answers(self, self.texts[ti] if isinstance(ti, int) else ti, flag)
        return self._answers[key]


class Answers:
    """every family's answer for one batch, from the oracle's hit list (computed when first asked for, then left alone)"""

    def __init__(self, ks, t, flag):
        self.ks, self.t = ks, t
        self.hits, self.dho = ks.hit_list(t, flag)
        self._c = {}

    def _get(self, name, make):
        if name not in self._c:
            self._c[name] = make()
        return self._c[name]

    @property
    def key_counts(self):
        return self._get("kc", lambda: np.bincount(self.hits["value"], minlength=self.ks.n_keys).astype(np.uint64))

    @property
    def docc(self):  # (pairs, doc_pair_offsets)
        return self._get("docc", lambda: doccountsim.doc_counts(self.hits["value"], self.dho))

    @property
    def cover(self):  # (mask, redacted, doc_covered, n_covered)
        return self._get("cover", lambda: coversim.cover_all(self.hits["start"], self.hits["end"], self.t.corpus, self.t.offs,
                                                             self.dho, FILL))

    @property
    def select(self):  # (selected hits, doc_sel_offsets)
        return self._get("select", lambda: selectsim.select(self.hits, self.dho))

    @property
    def replace(self):  # (bytes, doc_out_offsets)
        return self._get("replace", lambda: replacesim.replace(self.t.corpus, self.t.offs, *self.select, self.ks.repl))

    @property
    def records(self):  # (rec_offsets, doc_rec_offsets)
        return self._get("records", lambda: grepsim.records(self.t.corpus, self.t.offs, NL))

    def grep(self, invert):  # (kept_docs, bytes, doc_out_offsets)
        return self._get(("grep", invert), lambda: grepsim.grep(np.diff(self.dho.astype(np.int64)), self.t.offs, self.t.corpus,
                                                                invert))

    def total(self, fam, invert=False):
        """the number a call of the family reports first: what must differ between two consecutive steps"""
        if fam in ("match", "count"):
            return len(self.hits)
        if fam == "docc":
            return len(self.docc[0])
        if fam == "cover":
            return self.cover[3]
        if fam == "select":
            return len(self.select[0])
        if fam == "replace":
            return self.replace[0].size
        if fam == "records":
            return self.records[0].size - 1
        return self.grep(invert)[0].size


_SETS = {}


def key_set(name):
    if name not in _SETS:
        _SETS[name] = KeySet(name)
    return _SETS[name]


# ---- the feeds' model: subgroups of sequences, their pieces, and what every call on them gives ----------------------------

class Sub:
    """a subgroup of sequences of one feed: fed together, piece by piece, through one text after another"""

    def __init__(self, name, feed, ids, base):
        self.name, self.feed, self.ids, self.base = name, feed, list(ids), base
        self.cycle, self.k = 0, 0
        self.texts, self.pieces, self.consumed = None, None, [0] * len(ids)


def _pieces_of(ks, text, j):
    """six pieces at fixed, uneven places: the first cut inside a key where the text has one, an empty piece and a piece of 5
    or 3 bytes (shorter than the window of either key set), at places that alternate with j"""
    hits = ks.o.match(text, chars=False)
    c1 = next((int(h["start"]) + 1 for h in hits if h["start"] >= 3 and h["end"] - h["start"] >= 2 and h["start"] < len(text) // 2), 7)
    n = len(text)
    mids = [n // 4, 3, n // 5, 0] if j % 2 else [0, n // 4, 5, n // 5]  # (a call of two sequences or more never feeds crumbs alone)
    cuts = np.cumsum([0, c1] + mids).tolist() + [len(text)]
    assert cuts[-2] < cuts[-1]
    inside = any(h["start"] < c < h["end"] for h in hits for c in cuts[1:-1])
    return [text[cuts[i]:cuts[i + 1]] for i in range(N_PIECES)], inside


class FeedModels:
    """The state of both feeds as the plan walks: the sims, fed what the GPU feeds will be fed."""

    SIZES = [("mcc_a", 0, 2), ("mcc_b", 0, 3), ("sel", 0, 4), ("mix", 0, 6), ("rep", 0, 7), ("grep_a", 0, 8), ("grep_b", 0, 9),
             ("sep_a", 1, 10), ("sep_b", 1, 11)]
    SUBS_OF = {F_MATCH: ("mcc_a", "mcc_b"), F_COUNT: ("mcc_a", "mcc_b"), F_COVER: ("mcc_a", "mcc_b"), F_SELECT: ("sel", "mix"),
               F_REPLACE: ("rep", "mix"), F_GREP: ("grep_a", "grep_b"), F_SEP: ("sep_a", "sep_b")}

    def __init__(self, ks):
        self.ks = ks
        self.subs, at = {}, [0, 0]
        for b, (name, feed, n) in enumerate(self.SIZES):
            self.subs[name] = Sub(name, feed, range(at[feed], at[feed] + n), b)
            at[feed] += n
        self.n_seqs = at
        assert at[0] >= 12 and len({n for _, _, n in self.SIZES} | {0, 5}) == len(self.SIZES) + 2
        match = lambda t: [(int(s), int(e), int(v)) for s, e, v in ks.o.match(bytes(t), chars=False).tolist()] if t else []  # noqa: E731
        self.match = match
        self.fsim = FeedSim(ks.o, at[0])
        self.csim = FeedCoverSim(ks.o, at[0])
        self.selrep = frs.Feed(match, ks.W, at[0])
        self.count = fgs.oracle_count(ks._raw, ks.fold)
        self.grep = fgs.Feed(self.count, ks.W, at[0])
        self.sep = FeedSepSim(ks._raw, at[1], (256, SEP_BITS), fold=ks.fold)
        self.cut_inside_a_key = False
        self.visits = {k: 0 for k in self.SUBS_OF}

    def choose(self, kind, last_sub, last_total):
        """the kind's subgroups by turns, never the subgroup of the step before, nor one whose call would report that step's
        total"""
        a, b = self.SUBS_OF[kind]
        pick = (a, b)[self.visits[kind] % 2]
        other = b if pick == a else a
        self.visits[kind] += 1
        if pick == last_sub or (other != last_sub and self.expect(kind, self.subs[pick], models=self.sims_copy())["total"] == last_total):
            pick = other
        return self.subs[pick]

    def _start(self, sub):
        t = self.ks.texts[(sub.cycle + sub.base) % len(self.ks.texts)]
        raw = t.corpus.tobytes()
        sub.texts, sub.pieces = [], []
        for j in range(len(sub.ids)):
            at = j * (len(raw) // len(sub.ids))  # (spread over the text: its documents differ in density)
            text = raw[at:at + SEQ_BYTES]
            assert len(text) == SEQ_BYTES
            p, inside = _pieces_of(self.ks, text, j + sub.cycle)
            self.cut_inside_a_key |= inside
            sub.texts.append(text)
            sub.pieces.append(p)
        sub.consumed = [0] * len(sub.ids)

    def next_call(self, sub):
        """(pieces, final): what the subgroup's next visit feeds; the separator feed's seventh visit feeds nothing (finish)"""
        if sub.k == 0 and sub.pieces is None:
            self._start(sub)
        if sub.k == N_PIECES:
            return None, True
        return [p[sub.k] for p in sub.pieces], sub.k == N_PIECES - 1

    def expect(self, kind, sub, models=None):
        """What a call of `kind` on the subgroup's next pieces gives, by the sims -- which move on as the feed will.  models: a
        copy of this object's sims to move instead (a refused call: the feed stays)."""
        m = models or self
        ks = self.ks
        pieces, final = self.next_call(sub)
        ids = sub.ids
        w = {"pieces": pieces, "final": final, "ids": ids, "sub": sub.name, "closing": final}
        if kind == F_SEP:
            if pieces is None:
                res = [m.sep.finish(q) for q in ids]
                w.update(finish=True, bases=np.array([n for _, n in res], dtype=np.uint64))
            else:
                res = [m.sep.piece(q, p) for q, p in zip(ids, pieces)]
                w.update(finish=False, bases=np.array([b for _, b in res], dtype=np.uint64), closing=False)
            w["hits"] = np.concatenate([h for h, _ in res])
            w["pho"] = np.cumsum([0] + [len(h) for h, _ in res]).astype(np.uint64)
            w["total"] = len(w["hits"])
            if pieces is not None:
                w["main_hits"] = self.main_hits(pieces)
        elif kind in (F_MATCH, F_COUNT, F_COVER):
            hs, covs, backs, bases = [], [], [], []
            for q, p in zip(ids, pieces):
                h, base = m.fsim.piece(q, p)  # (ks.o lowers the text of a folding handle)
                cov, back, nh, base2 = m.csim.piece(q, p)
                assert nh == len(h) and base == base2
                hs.append(h), covs.append(cov), backs.append(back), bases.append(base)
            text = np.frombuffer(b"".join(pieces), dtype=np.uint8)
            cov = np.concatenate(covs) if covs else np.zeros(0, dtype=bool)
            w.update(hits=np.concatenate(hs), pho=np.cumsum([0] + [len(h) for h in hs]).astype(np.uint64),
                     bases=np.array(bases, dtype=np.uint64), mask=coversim.mask_words(cov),
                     redacted=coversim.redacted(text, cov, FILL), back=np.array(backs, dtype=np.uint32),
                     covered=np.array([int(c.sum()) for c in covs], dtype=np.uint64), n_covered=int(cov.sum()))
            w["key_counts"] = np.bincount(w["hits"]["value"], minlength=ks.n_keys).astype(np.uint64)
            w["total"] = w["n_covered"] if kind == F_COVER else len(w["hits"])
            w["main_hits"] = self.main_hits(pieces)
            if final and models is None:
                for q in ids:
                    m.fsim.reset(q)
                    m.csim.ctx[q], m.csim.pos[q] = b"", 0
        elif kind == F_SELECT:
            res = m.selrep.select(pieces, ids, final)
            rows = [h for hits, _, _ in res for h in hits]
            w.update(hits=frs.fss.as_array(rows), pso=np.cumsum([0] + [len(r[0]) for r in res]).astype(np.uint64),
                     bases=np.array([r[2] for r in res], dtype=np.uint64), hold=np.array([r[1] for r in res], dtype=np.uint32))
            w["total"] = len(rows)
            w["main_hits"] = self.main_hits(pieces)
        elif kind == F_REPLACE:
            out, poo, bases, hold, n_sel = m.selrep.call(pieces, ids, ks.repl, final)
            w.update(out=out, poo=poo, bases=bases, hold=hold, n_selected=n_sel, total=out.size, main_hits=self.main_hits(pieces))
        elif kind == F_GREP:
            invert = sub.name == "grep_b"
            kept, out, roo, info = m.grep.call(pieces, ids, NL, invert, final)
            w.update(kept=kept, out=out, roo=roo, info=info, invert=invert, total=info["n_recs"])  # (the first number it reports)
            w["main_hits"] = sum(self.count(f) for p in pieces for f in fgs.fragments(p, NL))  # (the fragments as documents)
        return w

    def main_hits(self, pieces):
        """what aha_timing.n_hits is after a feed call: the hits of its main pass, the pieces matched as a plain batch"""
        return sum(len(self.ks.o.match(p, chars=False)) for p in pieces if p)

    def advance(self, sub, w):
        """the subgroup after the call that gave w"""
        if w["pieces"] is not None:
            for j, p in enumerate(w["pieces"]):
                sub.consumed[j] += len(p)
        closing_now = w.get("finish", False) if sub.feed == 1 else w["closing"]
        sub.k += 1
        if closing_now:
            w["law"] = self.law(sub)
            sub.cycle, sub.k, sub.pieces = sub.cycle + 1, 0, None
            sub.consumed = [0] * len(sub.ids)
        w["consumed"] = list(sub.consumed)

    def law(self, sub):
        """the whole-text reference of the closing step's stream law, per sequence"""
        ks = self.ks
        if sub.feed == 1:
            return [self.sep.whole(t) for t in sub.texts]
        if sub.name.startswith("mcc"):
            return [ks.o.match(t, chars=False) for t in sub.texts]
        sel = [selectsim.select_doc(self.match(t)) for t in sub.texts] if sub.name in ("sel", "rep") else None
        if sub.name == "sel":
            return [frs.fss.as_array(s) for s in sel]
        if sub.name == "rep":
            return [replacesim.replace_doc(t, s, ks.repl) for t, s in zip(sub.texts, sel)]
        if sub.name.startswith("grep"):
            return [fgs.whole(self.count, t, NL, sub.name == "grep_b") for t in sub.texts]
        return None  # (select and replace calls mixed: no stream law)

    def sims_copy(self):
        c = copy.copy(self)
        # (the select, replace and grep models hold closures and plain data; the others hold the oracle: their lists alone)
        c.selrep, c.grep = copy.deepcopy(self.selrep), copy.deepcopy(self.grep)
        c.fsim, c.csim, c.sep = copy.copy(self.fsim), copy.copy(self.csim), copy.copy(self.sep)
        c.fsim.ctx, c.fsim.pos = list(self.fsim.ctx), list(self.fsim.pos)
        c.csim.ctx, c.csim.pos = list(self.csim.ctx), list(self.csim.pos)
        c.sep.text = list(self.sep.text)
        return c


# ---- the plan ----------------------------------------------------------------------------------------------------------------

_PLANS = {}


def plan_walk(name):
    """The walk of key set `name`: one dict per step with its kind, its variant, its text and -- for feed steps -- what the
    sims say the call gives.  The same for every engine variant; everything the issue wants asserted about the plan is
    asserted here."""
    if name in _PLANS:
        return _PLANS[name]
    ks = key_set(name)
    walk = de_bruijn_walk(K)
    pairs = set(zip(walk, walk[1:]))
    assert len(walk) == K * K + 1 and pairs == {(a, b) for a in range(K) for b in range(K)}, "the walk misses a pair"
    fm = FeedModels(ks)
    empties = {0: Text([]), 5: Text([b""] * 5)}
    steps, visits, rot = [], [0] * K, 0
    last = None      # (total, D, text id) of the last successful step
    last_sub = None  # the subgroup the last successful step fed, if it was a feed step
    ranged = {f: set() for f in RANGED}
    owed = []        # refusal forms whose turn came while the feeds had nothing of theirs to refuse
    for i, kind in enumerate(walk):
        v = visits[kind]
        visits[kind] += 1
        st = {"i": i, "kind": kind, "variant": "", "ti": None, "prof": i % PROF_SPAN >= PROF_OFF, "sig": None}
        steps.append(st)
        this_sub = None
        if kind == RELEASE:
            pass
        elif kind in FEED_KINDS:
            sub = fm.choose(kind, last_sub, None if last is None else last[0])
            w = fm.expect(kind, sub)
            fm.advance(sub, w)
            st.update(want=w, variant=sub.name + ("/finish" if w.get("finish") else "/final" if w["final"] else ""), ti=sub.name)
            st["sig"] = (w["total"], len(sub.ids), "feed:" + sub.name)
            this_sub = sub.name
        elif kind == F_REFUSED:
            owed.append(REFUSALS[v % len(REFUSALS)])  # by turns; a form the feeds' state cannot refuse now stays owed
            got = None
            for form in owed:
                got = _plan_refusal(fm, form, v)
                if got is not None:
                    owed.remove(form)
                    break
            if got is None:  # nothing owed can be refused now: the next form in turn that can (one on the separator feed always can)
                for turn in range(1, len(REFUSALS)):
                    form = REFUSALS[(v + turn) % len(REFUSALS)]
                    got = _plan_refusal(fm, form, v)
                    if got is not None:
                        break
            assert got is not None
            st.update(want=got, variant=form, ti=got["sub"])
        elif kind == EMPTYK:
            D, fam = 5 * (v % 2), FAMILIES[v % len(FAMILIES)]
            st.update(variant=f"{fam}/D={D}", fam=fam, text=empties[D], flag="plain", invert=v % 3 == 0)
            st["sig"] = (ks.answers(empties[D], "plain").total(fam, st["invert"]), D, f"empty{D}")
        else:
            if kind == HOSTK:
                fam, flag = FAMILIES[v % len(FAMILIES)], "plain"
            elif kind == SEPK:
                fam, flag = SEP_FAMILIES[v % len(SEP_FAMILIES)], "sep"
            elif kind == CAPF:
                form = CAP_FORMS[v % len(CAP_FORMS)]
                fam, flag = form.split("_")[0], "plain"
                st["form"] = form
            elif kind == BADOFF:
                fam, flag = FAMILIES[v % len(FAMILIES)], "plain"
                st["form"] = ("decreasing", "last")[v % 2]
            else:
                fam, flag = FAMILY_OF[kind], "plain"
            invert = kind == GREP_INV or (kind in (HOSTK, SEPK, CAPF) and fam == "grep" and v % 2 == 1)
            chosen = None
            for j in range(len(ks.texts)):
                ti = (rot + j) % len(ks.texts)
                a = ks.answers(ti, flag)
                n, D = a.total(fam, invert), ks.texts[ti].D
                if kind == BADOFF:
                    chosen = ti
                    break
                if kind == CAPF:
                    if n < 2 or (st["form"] == "grep_bytes" and a.grep(invert)[1].size < 2):
                        continue
                    chosen = ti
                    break
                if n == 0:
                    continue  # (a zero total would not tell a stale counter from a fresh one)
                if last is not None and (n == last[0] or D == last[1] or ti == last[2]):
                    continue
                chosen = ti
                break
            assert chosen is not None, (name, i, KIND_NAMES[kind], last)
            rot += 1
            a = ks.answers(chosen, flag)
            st.update(ti=chosen, fam=fam, flag=flag, invert=invert, text=ks.texts[chosen],
                      variant=st.get("form", fam if kind in (HOSTK, SEPK) else "") + ("/invert" if invert and kind != GREP_INV else ""))
            if kind not in (CAPF, BADOFF):
                st["sig"] = (a.total(fam, invert), ks.texts[chosen].D, chosen)
                if fam in RANGED and flag == "plain" and kind != HOSTK and st["prof"]:
                    ranged[fam].add(chosen == ks.largest)
        if st["sig"] is not None:
            # (an empty batch reports 0 whatever went before: beside one, and only there, a call that finds nothing -- a finish
            # call, a piece in which no record closes -- may report 0 too)
            if last is not None and not (st["sig"][0] == 0 == last[0] and "empty" in (str(st["sig"][2])[:5], str(last[2])[:5])):
                assert st["sig"][0] != last[0], f"step {i} ({KIND_NAMES[kind]}): {st['sig']} has the total of the step before, {last}"
            if last is not None:
                assert st["sig"][1] != last[1] and st["sig"][2] != last[2], f"step {i} ({KIND_NAMES[kind]}): {st['sig']} after {last}"
            last = st["sig"]
            last_sub = this_sub  # (of the last successful step, like `last`)
    # what the walk is for
    assert all(r == {True, False} for r in ranged.values()), ("a family never meets both one range and several, profiled", ranged)
    assert fm.cut_inside_a_key
    closing = [s for s in steps if s["kind"] in FEED_KINDS and s["want"].get("law") is not None]
    assert {s["want"]["sub"] for s in closing} >= {"mcc_a", "mcc_b", "sel", "rep", "grep_a", "grep_b", "sep_a", "sep_b"}
    n_refused = [sum(s["variant"] == f for s in steps if s["kind"] == F_REFUSED) for f in REFUSALS]
    assert min(n_refused) >= 2 and max(n_refused) <= 4, dict(zip(REFUSALS, n_refused))
    for kind, forms in ((HOSTK, FAMILIES), (SEPK, SEP_FAMILIES), (CAPF, CAP_FORMS)):
        assert {s["variant"].split("/")[0] for s in steps if s["kind"] == kind} == set(forms)
    _PLANS[name] = (steps, fm.n_seqs)
    return _PLANS[name]


def _plan_refusal(fm, form, v):
    """what a refused call of `form` is made of, or None where the feeds' state has nothing to refuse"""
    subs = fm.subs
    if form.startswith("sep_"):
        sub = subs["sep_a"]
        return {"sub": sub.name, "ids": sub.ids, "pieces": [b"ab cd\n"] * len(sub.ids), "code": N.AHA_E_INVALID,
                "consumed": list(sub.consumed), "feed": 1}
    if form == "select_on_match":
        sub = next((s for s in (subs["mcc_a"], subs["mcc_b"]) if s.k > 0 and min(s.consumed) > 0), None)
        if sub is None:
            return None
        return {"sub": sub.name, "ids": sub.ids, "pieces": [b"ab cd\n"] * len(sub.ids), "code": N.AHA_E_INVALID,
                "consumed": list(sub.consumed), "feed": 0}
    kind, sub = {"select_cap": (F_SELECT, subs["sel"]), "replace_cap": (F_REPLACE, subs["rep"]),
                 "grep_cap": (F_GREP, subs["grep_a"]), "match_cap": (F_MATCH, subs[("mcc_a", "mcc_b")[v % 2]])}[form]
    w = fm.expect(kind, sub, models=fm.sims_copy())  # (the sims stay where they are: so does the feed)
    if w["total"] < 1 or (form == "grep_cap" and (w["kept"].size < 1 or w["out"].size < 1)):
        return None
    short = "bytes" if form == "replace_cap" or (form == "grep_cap" and v % 2) else "rows"
    w.update(code=N.AHA_E_CAPACITY, consumed=list(sub.consumed), feed=0, kind=kind, short=short)
    return w


# ---- guarded buffers -----------------------------------------------------------------------------------------------------------

class Bufs:
    """a call's output buffers on the device, prefilled with sentinels, allocated and filled on the walk's stream"""

    def __init__(self, st):
        self.st, self.b = st, {}

    def new(self, name, shape, dtype, fill):
        import torch

        with torch.cuda.stream(self.st):
            self.b[name] = (torch.full(shape if isinstance(shape, tuple) else (shape,), fill, dtype=dtype, device="cuda"), fill)
        return self.b[name][0]

    def get(self, name):
        return self.b[name][0] if name in self.b else None

    def host(self, name, dtype=None):
        a = self.b[name][0].cpu().numpy()
        return a.astype(dtype) if dtype is not None else a

    def written(self):
        """the buffers that no longer hold their sentinel everywhere"""
        return [n for n, (t, fill) in self.b.items() if not bool((t == fill).all())]

    def check(self, name, n, want, dtype=np.uint64):
        """entries [0, n) are `want`, everything behind still the sentinel"""
        t, fill = self.b[name]
        got = t.cpu().numpy()
        head = got[:n]
        want = np.asarray(want)
        assert head.astype(dtype).tobytes() == want.astype(dtype).tobytes(), f"{name}: {head[:8]} ... for {want[:8]} ..."
        assert (got[n:] == fill).all(), f"{name}: written behind entry {n}"


def _to_dev(st, a, dtype):
    import torch

    with torch.cuda.stream(st):
        return torch.from_numpy(np.ascontiguousarray(np.asarray(a).astype(dtype))).cuda()


def _pieces_dev(st, pieces):
    """the pieces one behind the other on the device (a non-null pointer for an empty batch), and their offsets"""
    import torch

    raw = b"".join(pieces)
    with torch.cuda.stream(st):
        if raw:
            corpus = torch.from_numpy(np.frombuffer(raw, dtype=np.uint8).copy()).cuda()
        else:
            corpus = torch.zeros(16, dtype=torch.uint8, device="cuda")[:0]
    return corpus, _to_dev(st, np.cumsum([0] + [len(p) for p in pieces]), np.int64)


# ---- one batch call of a family ----------------------------------------------------------------------------------------------

def call_family(g, ks, fam, t, a, env, sep=None, invert=False, ids_only=False, with_mask=True, caps=None, dd=None):
    """The device entry of `fam` on text t over env's stream, into sentinel-filled buffers with exactly the room the answer
    `a` needs (caps: other capacities).  -> (AhaError or None, what the call returned, the buffers)"""
    import torch

    st, stream, table = env["st"], env["st"].cuda_stream, env["table"]
    caps = caps or {}
    B = Bufs(st)
    if t.corpus.size:
        dc, d_off = t.dev()
    else:
        dc, d_off = _pieces_dev(st, t.docs)
    if dd is not None:
        d_off = dd
    D, n_bytes = t.D, t.corpus.size
    i64, i32, u8 = torch.int64, torch.int32, torch.uint8
    if fam == "match":
        cap = caps.get("rows", len(a.hits) + 37)
        B.new("out", (cap + PAD, 3), i32, S32), B.new("dho", D + 1 + PAD, i64, S64I)
        call = lambda: g.match_batch_device(dc, d_off, B.get("out")[:cap], B.get("dho"), sep=sep, stream=stream)  # noqa: E731
    elif fam == "count":
        B.new("kc", ks.n_keys + PAD, i64, S64I), B.new("dho", D + 1 + PAD, i64, S64I)
        call = lambda: g.count_batch_device(dc, d_off, B.get("kc"), B.get("dho"), sep=sep, stream=stream)  # noqa: E731
    elif fam == "docc":
        cap = caps.get("rows", len(a.docc[0]))
        B.new("out", (cap + PAD, 2), i32, S32), B.new("dpo", D + 1 + PAD, i64, S64I)
        call = lambda: g.doc_counts_batch_device(dc, d_off, B.get("out"), B.get("dpo"), sep=sep, cap=cap, stream=stream)  # noqa: E731
    elif fam == "cover":
        if with_mask:
            B.new("mask", (n_bytes + 31) // 32 + PAD, i32, S32)
        B.new("red", n_bytes + PAD, u8, G8), B.new("cov", D + PAD, i64, S64I)
        call = lambda: g.cover_batch_device(dc, d_off, mask=B.get("mask"), redacted=B.get("red"), fill=FILL,  # noqa: E731
                                            doc_covered=B.get("cov"), sep=sep, stream=stream)
    elif fam == "select":
        cap = caps.get("rows", len(a.select[0]))
        B.new("out", (cap + PAD, 3), i32, S32), B.new("dso", D + 1 + PAD, i64, S64I)
        call = lambda: g.select_batch_device(dc, d_off, B.get("out"), B.get("dso"), sep=sep, cap=cap, stream=stream)  # noqa: E731
    elif fam == "replace":
        cap = caps.get("bytes", a.replace[0].size)
        B.new("out", cap + PAD, u8, G8), B.new("doo", D + 1 + PAD, i64, S64I)
        call = lambda: g.replace_batch_device(dc, d_off, table, B.get("out"), B.get("doo"), sep=sep, cap=cap, stream=stream)  # noqa: E731
    elif fam == "records":
        cap = caps.get("rows", a.records[0].size - 1)
        B.new("rec", cap + 1 + PAD, i64, S64I), B.new("dro", D + 1 + PAD, i64, S64I)
        call = lambda: g.records_device(dc, d_off, B.get("rec"), B.get("dro"), delim=NL, cap=cap, stream=stream)  # noqa: E731
    else:
        kept, out, _ = a.grep(invert)
        cd, cb = caps.get("rows", kept.size), caps.get("bytes", out.size)
        B.new("kept", cd + PAD, i64, S64I), B.new("doo", cd + 1 + PAD, i64, S64I)
        if not ids_only:
            B.new("out", cb + PAD, u8, G8)
        call = lambda: g.grep_batch_device(dc, d_off, B.get("kept"), B.get("doo"), B.get("out"), sep=sep, invert=invert,  # noqa: E731
                                           cap_docs=cd, cap_bytes=None if ids_only else cb, stream=stream)
    st.synchronize()
    try:
        return None, call(), B
    except AhaError as e:
        return e, None, B


def check_family(ks, fam, t, a, ret, B, invert=False, ids_only=False, with_mask=True):
    """every output of a successful call against the answer; -> the match's hit count where the call reports it"""
    D, nh = t.D, len(a.hits)
    if fam == "match":
        assert ret == nh
        B.check("out", nh, a.hits.view(np.int32).reshape(-1, 3), np.int32)
        B.check("dho", D + 1, a.dho)
    elif fam == "count":
        assert ret == nh
        B.check("kc", ks.n_keys, a.key_counts)
        B.check("dho", D + 1, a.dho)
    elif fam == "docc":
        pairs, dpo = a.docc
        assert ret == (len(pairs), nh), (ret, len(pairs), nh)
        B.check("out", len(pairs), pairs.view(np.int32).reshape(-1, 2), np.int32)
        B.check("dpo", D + 1, dpo)
    elif fam == "cover":
        mask, red, dc, n_cov = a.cover
        assert ret == (n_cov, nh), (ret, n_cov, nh)
        if with_mask:
            B.check("mask", mask.size, mask, np.uint32)  # (the bits behind the batch in its last word are 0 in the answer)
        B.check("red", red.size, red, np.uint8)
        B.check("cov", D, dc)
    elif fam == "select":
        sel, dso = a.select
        assert ret == (len(sel), nh), (ret, len(sel), nh)
        B.check("out", len(sel), sel.view(np.int32).reshape(-1, 3), np.int32)
        B.check("dso", D + 1, dso)
    elif fam == "replace":
        out, doo = a.replace
        assert ret == (out.size, len(a.select[0]), nh), (ret, out.size, len(a.select[0]), nh)
        B.check("out", out.size, out, np.uint8)
        B.check("doo", D + 1, doo)
    elif fam == "records":
        rec, dro = a.records
        assert ret == rec.size - 1
        B.check("rec", rec.size, rec)
        B.check("dro", D + 1, dro)
        return None
    else:
        kept, out, doo = a.grep(invert)
        assert ret == (kept.size, out.size, nh), (ret, kept.size, out.size, nh)
        B.check("kept", kept.size, kept)
        B.check("doo", kept.size + 1, doo)
        if not ids_only:
            B.check("out", out.size, out, np.uint8)
    return nh


def check_timing(g, env, n_hits):
    """with profiling on, aha_timing.n_hits is the call's own"""
    if env.get("prof"):
        got = g.last_timing()["n_hits"]
        assert got == n_hits, f"aha_timing.n_hits is {got}, the call's hits are {n_hits}"


def host_family(g, ks, fam, t, a, invert, env, sep=None):
    """the host-buffer entry of `fam` (they share hostbuf) against the same answer; its timing after every call that matches"""
    c, o = t.corpus, t.offs
    timed = lambda: check_timing(g, env, len(a.hits))  # noqa: E731
    if fam == "count":
        kc, dho = g.count_batch(c, o, sep=sep)
        assert np.array_equal(kc, a.key_counts) and np.array_equal(dho, a.dho)
        timed()
    elif fam == "docc":
        pairs, dpo = g.doc_counts_batch(c, o, sep=sep)
        assert pairs.tobytes() == a.docc[0].tobytes() and np.array_equal(dpo, a.docc[1])
        timed()
    elif fam == "cover":
        mask, cov = g.cover_batch(c, o, sep=sep)
        assert np.array_equal(mask, a.cover[0]) and np.array_equal(cov, a.cover[2])
        timed()
        red, cov = g.redact_batch(c, o, fill=FILL, sep=sep)
        assert np.array_equal(red, a.cover[1]) and np.array_equal(cov, a.cover[2])
        timed()
    elif fam == "select":
        sel, dso = g.select_batch(c, o, sep=sep)
        assert sel.tobytes() == a.select[0].tobytes() and np.array_equal(dso, a.select[1])
        timed()
    elif fam == "replace":
        out, doo = g.replace_batch(c, o, ks.repl, sep=sep)
        assert out.tobytes() == a.replace[0].tobytes() and np.array_equal(doo, a.replace[1])
        timed()
    elif fam == "records":
        rec, dro = g.records(c, o, NL)
        assert np.array_equal(rec, a.records[0]) and np.array_equal(dro, a.records[1])
    else:
        kept, out, doo = g.grep_batch(c, o, sep=sep, invert=invert)
        want = a.grep(invert)
        assert np.array_equal(kept, want[0]) and out.tobytes() == want[1].tobytes() and np.array_equal(doo, want[2])
        timed()


# ---- one feed call -------------------------------------------------------------------------------------------------------------

def call_feed(env, kind, w, caps=None):
    """The device entry of feed kind `kind` on the pieces of w, sentinel-filled buffers with exactly the room w needs.
    -> (AhaError or None, what the call returned, the buffers)"""
    import torch

    st, stream = env["st"], env["st"].cuda_stream
    caps = caps or {}
    feed = env["feeds"][1 if kind == F_SEP else 0]
    B = Bufs(st)
    i64, i32, u8 = torch.int64, torch.int32, torch.uint8
    ids = _to_dev(st, w["ids"], np.int32)
    D = len(w["ids"])
    if kind == F_SEP and w.get("finish"):
        cap = len(w["hits"])
        B.new("out", (cap + PAD, 3), i32, S32), B.new("pho", D + 1 + PAD, i64, S64I), B.new("bases", D + PAD, i64, S64I)
        call = lambda: feed.finish_batch_device(ids, B.get("out")[:cap], B.get("pho"), B.get("bases"), stream=stream)  # noqa: E731
    else:
        corpus, offs = _pieces_dev(st, w["pieces"])
        n_bytes = corpus.numel()
        if kind in (F_MATCH, F_SEP):
            cap = caps.get("rows", len(w["hits"]))
            B.new("out", (cap + PAD, 3), i32, S32), B.new("pho", D + 1 + PAD, i64, S64I), B.new("bases", D + PAD, i64, S64I)
            call = lambda: feed.match_batch_device(corpus, offs, ids, B.get("out")[:cap], B.get("pho"), B.get("bases"),  # noqa: E731
                                                   stream=stream)
        elif kind == F_COUNT:
            B.new("kc", env["ks"].n_keys + PAD, i64, S64I), B.new("pho", D + 1 + PAD, i64, S64I), B.new("bases", D + PAD, i64, S64I)
            call = lambda: feed.count_batch_device(corpus, offs, ids, B.get("kc"), B.get("pho"), B.get("bases"), stream=stream)  # noqa: E731
        elif kind == F_COVER:
            B.new("mask", (n_bytes + 31) // 32 + PAD, i32, S32), B.new("red", n_bytes + PAD, u8, G8)
            B.new("back", D + PAD, i32, S32), B.new("covered", D + PAD, i64, S64I)
            B.new("pho", D + 1 + PAD, i64, S64I), B.new("bases", D + PAD, i64, S64I)
            call = lambda: feed.cover_batch_device(corpus, offs, ids, mask=B.get("mask"), redacted=B.get("red"), fill=FILL,  # noqa: E731
                                                   piece_back=B.get("back"), piece_covered=B.get("covered"),
                                                   piece_hit_offsets=B.get("pho"), piece_bases=B.get("bases"), stream=stream)
        elif kind == F_SELECT:
            cap = caps.get("rows", len(w.get("hits", ())))
            B.new("out", (cap + PAD, 3), i32, S32), B.new("pso", D + 1 + PAD, i64, S64I), B.new("bases", D + PAD, i64, S64I)
            B.new("hold", D + PAD, i32, S32)
            call = lambda: feed.select_batch_device(corpus, offs, ids, B.get("out"), B.get("pso"), B.get("bases"), B.get("hold"),  # noqa: E731
                                                    final=w["final"], cap=cap, stream=stream)
        elif kind == F_REPLACE:
            cap = caps.get("bytes", w["out"].size if "out" in w else 0)
            B.new("out", cap + PAD, u8, G8), B.new("poo", D + 1 + PAD, i64, S64I), B.new("bases", D + PAD, i64, S64I)
            B.new("hold", D + PAD, i32, S32)
            call = lambda: feed.replace_batch_device(corpus, offs, ids, env["table"], B.get("out"), B.get("poo"), B.get("bases"),  # noqa: E731
                                                     B.get("hold"), final=w["final"], cap=cap, stream=stream)
        else:
            cr = caps.get("rows", w["kept"].size if "kept" in w else 0)
            cb = caps.get("bytes", w["out"].size if "kept" in w else 0)
            B.new("kept", cr + PAD, i64, S64I), B.new("roo", cr + 1 + PAD, i64, S64I), B.new("out", cb + PAD, u8, G8)
            for k in ("piece_rec_offsets", "piece_kept_offsets"):
                B.new(k, D + 1 + PAD, i64, S64I)
            for k in ("piece_head", "piece_bases", "piece_rec_bases"):
                B.new(k, D + PAD, i64, S64I)
            B.new("piece_hold", D + PAD, i32, S32)
            per = {k: B.get(k) for k in ("piece_rec_offsets", "piece_kept_offsets", "piece_head", "piece_bases", "piece_rec_bases",
                                         "piece_hold")}
            call = lambda: feed.grep_batch_device(corpus, offs, ids, B.get("kept"), B.get("roo"), B.get("out"), delim=NL,  # noqa: E731
                                                  invert=w.get("invert", False), final=w.get("final", False), cap_recs=cr, cap_bytes=cb,
                                                  stream=stream, **per)
    st.synchronize()
    try:
        return None, call(), B
    except AhaError as e:
        return e, None, B


def check_feed(env, kind, w, ret, B):
    """every output of a successful feed call against the sims' answer"""
    D = len(w["ids"])
    if kind in (F_MATCH, F_SEP):
        assert ret == len(w["hits"]), (ret, len(w["hits"]))
        B.check("out", len(w["hits"]), w["hits"].view(np.int32).reshape(-1, 3), np.int32)
        B.check("pho", D + 1, w["pho"])
        B.check("bases", D, w["bases"])
    elif kind == F_COUNT:
        assert ret == len(w["hits"])
        B.check("kc", env["ks"].n_keys, w["key_counts"])
        B.check("pho", D + 1, w["pho"])
        B.check("bases", D, w["bases"])
    elif kind == F_COVER:
        assert ret == (w["n_covered"], len(w["hits"])), (ret, w["n_covered"], len(w["hits"]))
        B.check("mask", w["mask"].size, w["mask"], np.uint32)
        B.check("red", w["redacted"].size, w["redacted"], np.uint8)
        B.check("back", D, w["back"], np.uint32)
        B.check("covered", D, w["covered"])
        B.check("pho", D + 1, w["pho"])
        B.check("bases", D, w["bases"])
    elif kind == F_SELECT:
        assert ret[0] == len(w["hits"]), (ret, len(w["hits"]))
        B.check("out", len(w["hits"]), w["hits"].view(np.int32).reshape(-1, 3), np.int32)
        B.check("pso", D + 1, w["pso"])
        B.check("bases", D, w["bases"])
        B.check("hold", D, w["hold"], np.uint32)
    elif kind == F_REPLACE:
        assert ret[:2] == (w["out"].size, w["n_selected"]), (ret, w["out"].size, w["n_selected"])
        B.check("out", w["out"].size, w["out"], np.uint8)
        B.check("poo", D + 1, w["poo"])
        B.check("bases", D, w["bases"])
        B.check("hold", D, w["hold"], np.uint32)
    else:
        info = w["info"]
        assert ret[:3] == (info["n_recs"], w["kept"].size, w["out"].size), (ret, info["n_recs"], w["kept"].size, w["out"].size)
        B.check("kept", w["kept"].size, w["kept"])
        B.check("roo", w["kept"].size + 1, w["roo"])
        B.check("out", w["out"].size, w["out"], np.uint8)
        for k in ("piece_rec_offsets", "piece_kept_offsets"):
            B.check(k, D + 1, info[k])
        for k in ("piece_head", "piece_bases", "piece_rec_bases"):
            B.check(k, D, info[k])
        B.check("piece_hold", D, info["piece_hold"], np.uint32)


def note_reported(env, kind, w, B):
    """what the GPU reported for each sequence of the step's subgroup since it started; on a closing step the stream law"""
    acc = env["reported"].setdefault(w["sub"], [[] for _ in w["ids"]])
    D = len(w["ids"])
    if kind in (F_MATCH, F_COUNT, F_COVER, F_SEP):
        pho = B.host("pho", np.uint64)[:D + 1].astype(np.int64)
        bases = B.host("bases", np.uint64)[:D].astype(np.int64)
        rows = B.host("out")[:int(pho[-1])].copy().view(orc.HIT_DTYPE).reshape(-1) if kind in (F_MATCH, F_SEP) else None
        for j in range(D):
            n = 0 if w["pieces"] is None else len(w["pieces"][j])
            hits = None
            if rows is not None:
                hits = rows[pho[j]:pho[j + 1]].copy()
                hits["start"] += bases[j]
                hits["end"] += bases[j]
            acc[j].append((int(pho[j + 1] - pho[j]), int(bases[j]), n, hits))
    elif kind == F_SELECT:
        pso = B.host("pso", np.uint64)[:D + 1].astype(np.int64)
        bases = B.host("bases", np.uint64)[:D].astype(np.int64)
        rows = B.host("out")[:int(pso[-1])].copy().view(orc.HIT_DTYPE).reshape(-1)
        for j in range(D):
            hits = rows[pso[j]:pso[j + 1]].copy()
            hits["start"] += bases[j]
            hits["end"] += bases[j]
            acc[j].append(hits)
    elif kind == F_REPLACE:
        poo = B.host("poo", np.uint64)[:D + 1].astype(np.int64)
        raw = B.host("out")[:int(poo[-1])].tobytes()
        for j in range(D):
            acc[j].append(raw[poo[j]:poo[j + 1]])
    else:
        pko = B.host("piece_kept_offsets", np.uint64)[:D + 1].astype(np.int64)
        roo = B.host("roo", np.uint64)[:int(pko[-1]) + 1].astype(np.int64)
        raw = B.host("out").tobytes()
        head, hold = B.host("piece_head", np.uint64)[:D], B.host("piece_hold", np.uint32)[:D]
        holders = env["holders"].setdefault(w["sub"], [fgs.Holder() for _ in w["ids"]])
        for j in range(D):
            kept = [raw[roo[r]:roo[r + 1]] for r in range(pko[j], pko[j + 1])]
            acc[j] += holders[j].step(w["pieces"][j], kept, int(head[j]), int(hold[j]), w["final"])
    law = w.get("law")
    if "law" not in w:
        return
    got = env["reported"].pop(w["sub"])
    env["holders"].pop(w["sub"], None)
    if law is None:
        return
    for j, (whole, rep) in enumerate(zip(law, got)):
        if w["sub"].startswith("mcc"):
            assert sum(r[0] for r in rep) == len(whole), f"sequence {j}: the pieces' hit counts do not add up to the whole's"
            ends = whole["end"].astype(np.int64)
            for n_hits, base, n, hits in rep:
                if hits is not None:  # (a match call: the whole's hits that end inside the piece)
                    assert hits.tobytes() == whole[(ends > base) & (ends <= base + n)].tobytes(), f"sequence {j} at {base}"
        elif w["sub"].startswith("sep"):
            cat = np.concatenate([r[3] for r in rep])
            assert cat.tobytes() == np.ascontiguousarray(whole).tobytes(), f"sequence {j}: not the filtered match of the whole"
        elif w["sub"] == "sel":
            assert np.concatenate(rep).tobytes() == whole.tobytes(), f"sequence {j}: not the batch select of the whole"
        elif w["sub"] == "rep":
            assert b"".join(rep) == whole, f"sequence {j}: not the batch replace of the whole"
        else:
            assert rep == whole, f"sequence {j}: not the whole-sequence grep"


def check_positions(env, feed_no, ids, consumed):
    feed = env["feeds"][feed_no]
    for q, n in zip(ids, consumed):
        assert feed.position(q)[0] == n, f"sequence {q} of feed {feed_no} stands at {feed.position(q)[0]}, not {n}"


# ---- one step -----------------------------------------------------------------------------------------------------------------

def _bad_offsets(env, t, form):
    offs = t.offs.astype(np.int64).copy()
    if form == "decreasing":
        j = next(d for d in range(1, t.D) if offs[d + 1] > offs[d])  # one decreasing pair: offs[j] > offs[j + 1]
        offs[j] = offs[j + 1] + 3
    else:
        offs[-1] -= 1  # the last offset is not n_bytes
    return _to_dev(env["st"], offs, np.int64)


def run_step(g, env, s):
    """One step of the plan: the call and every check.  -> (the match's hit count the call's timing must report or None, the
    family when it is one the compile-time bounds cut into ranges)"""
    ks, kind = env["ks"], s["kind"]
    if kind == RELEASE:
        g.release_scratch()
        assert g.scratch_bytes() == 0
        return None, None
    if kind in FEED_KINDS:
        w = s["want"]
        err, ret, B = call_feed(env, kind, w)
        assert err is None, (err, getattr(err, "code", None))
        check_feed(env, kind, w, ret, B)
        if "main_hits" in w and sum(len(p) for p in w["pieces"]):  # (a finish call matches contexts only: no main pass)
            check_timing(g, env, w["main_hits"])
        note_reported(env, kind, w, B)
        feed = env["feeds"][1 if kind == F_SEP else 0]
        if w["closing"] and kind in (F_MATCH, F_COUNT, F_COVER):
            for q in w["ids"]:
                feed.reset(q)
        check_positions(env, 1 if kind == F_SEP else 0, w["ids"], w["consumed"])
        return None, None
    if kind == F_REFUSED:
        w, form = s["want"], s["variant"]
        if form in ("sep_cover", "sep_select", "sep_grep", "select_on_match"):
            k2 = {"sep_cover": F_COVER, "sep_select": F_SELECT, "sep_grep": F_GREP, "select_on_match": F_SELECT}[form]
            if w["feed"] == 1:  # (call_feed takes the separator feed for F_SEP only: these go to it by hand)
                env2 = dict(env, feeds=[env["feeds"][1], env["feeds"][1]])
            else:
                env2 = env
            err, ret, B = call_feed(env2, k2, dict(w, final=False))
            assert err is not None and err.code == N.AHA_E_INVALID, (err, ret)
        else:
            rows = w["kept"].size if form == "grep_cap" else w["total"]
            short = {"rows": rows - 1} if w["short"] == "rows" else {"bytes": w["out"].size - 1}
            err, ret, B = call_feed(env, w["kind"], w, caps=short)
            assert err is not None and err.code == N.AHA_E_CAPACITY, (err, ret)
            if form == "match_cap":
                assert err.required == len(w["hits"])
            elif form == "select_cap":
                assert err.n_required == len(w["hits"])
            elif form == "replace_cap":
                assert err.n_required == w["out"].size
            else:
                assert (err.n_required, err.bytes_required) == (w["kept"].size, w["out"].size)
        assert not B.written(), ("a refused call wrote", B.written())
        check_positions(env, w["feed"], w["ids"], w["consumed"])
        return None, None
    fam, t, invert = s["fam"], s["text"], s["invert"]
    a = ks.answers(s["ti"] if kind != EMPTYK else t, s["flag"])
    if kind == HOSTK:
        host_family(g, ks, fam, t, a, invert, env)
        return None, None
    if kind == CAPF:
        form = s["form"]
        if form == "grep_bytes":
            caps = {"bytes": a.grep(invert)[1].size - 1}
        else:
            caps = {"bytes" if fam == "replace" else "rows": a.total(fam, invert) - 1}
        err, ret, B = call_family(g, ks, fam, t, a, env, invert=invert, caps=caps)
        assert err is not None and err.code == N.AHA_E_CAPACITY, (err, ret)
        if fam == "grep":
            assert (err.n_required, err.bytes_required) == (a.grep(invert)[0].size, a.grep(invert)[1].size)
        else:
            assert err.n_required == a.total(fam, invert), (err.n_required, a.total(fam, invert))
        if fam == "docc":  # (the header's rule for this entry: all offsets valid, the first cap pairs valid, nothing behind them)
            pairs, dpo = a.docc
            B.check("out", caps["rows"], pairs[:caps["rows"]].view(np.int32).reshape(-1, 2), np.int32)
            B.check("dpo", t.D + 1, dpo)
        else:
            assert not B.written(), ("a call that did not fit wrote", B.written())
        return None, None
    if kind == BADOFF:
        err, ret, B = call_family(g, ks, fam, t, a, env, invert=invert, dd=_bad_offsets(env, t, s["form"]))
        assert err is not None and err.code == N.AHA_E_INVALID, (err, ret)
        wrote = [n for n in B.written() if not (fam == "count" and n == "kc")]
        assert not wrote, ("a call refused for its offsets wrote", wrote)
        return None, None
    # a successful batch call through the device entry
    sep = _sep() if kind == SEPK else None
    ids_only = kind == GREP_INV
    with_mask = kind != COVER_N
    if kind == COUNT_R:  # (read by every pass: regions of 8 bytes or more per byte of text do not fit twice the text)
        os.environ["AHA_COUNT_REGION_BYTES"] = str(2 * t.corpus.size)
    try:
        err, ret, B = call_family(g, ks, fam, t, a, env, sep=sep, invert=invert, ids_only=ids_only, with_mask=with_mask)
    finally:
        os.environ.pop("AHA_COUNT_REGION_BYTES", None)
    assert err is None, (err, getattr(err, "code", None))
    nh = check_family(ks, fam, t, a, ret, B, invert=invert, ids_only=ids_only, with_mask=with_mask)
    if kind == EMPTYK:  # (an empty batch publishes no timing)
        return None, None
    return nh, (fam if fam in RANGED and kind != SEPK else "count_r" if kind == COUNT_R else None)


def open_env(g, ks, n_seqs, st):
    return {"ks": ks, "st": st, "table": g.replacements(ks.repl), "feeds": [g.feed(n_seqs[0]), g.feed(n_seqs[1], sep=_sep())],
            "reported": {}, "holders": {}}


def compile_bounded(monkeypatch, variant, ks):
    """the handle of the walk: the engine variant, and both hit buffers' bounds lowered (read when the handle is compiled)"""
    monkeypatch.delenv("AHA_COUNT_REGION_BYTES", raising=False)
    monkeypatch.setenv("AHA_DOCCOUNT_HIT_BYTES", str(ks.hit_bytes))
    monkeypatch.setenv("AHA_SELECT_HIT_BYTES", str(ks.hit_bytes))
    g = compile_under(monkeypatch, variant, ks.keys, fold_ascii=ks.fold)
    monkeypatch.delenv("AHA_DOCCOUNT_HIT_BYTES")
    monkeypatch.delenv("AHA_SELECT_HIT_BYTES")
    return g


WALK_VARIANTS = ("auto", "v2", "v1", "u", "f")
assert set(WALK_VARIANTS) <= set(VARIANTS)
CASES = [(v, n) for n in ("ascii", "cjk") for v in WALK_VARIANTS] + [("auto", "fold")]


@pytest.mark.parametrize("variant,name", CASES, ids=[f"{v}-{n}" for v, n in CASES])
def test_family_sequence_on_one_handle(variant, name, monkeypatch):
    """Every ordered pair of the 25 kinds on one handle with two feeds open on it, each call against the oracle; with
    profiling on, aha_timing.n_hits is the call's own (a feed call's: its main pass's; the module's docstring names the steps
    that publish none) and aha_timing.repeats tells one document range from several."""
    import torch

    ks = key_set(name)
    steps, n_seqs = plan_walk(name)
    g = compile_bounded(monkeypatch, variant, ks)
    st = torch.cuda.Stream()
    env = open_env(g, ks, n_seqs, st)
    prof, n_ranged, n_closing = None, 0, 0
    t0 = time.perf_counter()
    for s in steps:
        i, kind = s["i"], s["kind"]
        if s["prof"] != prof:
            prof = env["prof"] = s["prof"]
            g.set_profiling(prof)
        try:
            nh, fam = run_step(g, env, s)
            if prof and nh is not None:
                t = g.last_timing()
                assert t["n_hits"] == nh, f"aha_timing.n_hits is {t['n_hits']}, the call's hits are {nh}"
                if fam == "count_r" and variant != "v1":  # (the two-pass engine counts in one piece)
                    assert t["repeats"] >= 1, "the count was not cut into document ranges"
                    n_ranged += 1
                elif fam in RANGED:
                    if s["ti"] == ks.largest:
                        assert t["repeats"] >= 1, "the largest text was not cut into document ranges"
                        n_ranged += 1
                    else:
                        assert t["repeats"] == 0, f"{t['repeats'] + 1} document ranges for a text that fits one"
        except (AssertionError, AhaError) as e:
            before = steps[i - 1] if i else None
            raise AssertionError(f"step {i} ({KIND_NAMES[kind]} {s['variant']}, text {s['ti']}) after "
                                 f"{KIND_NAMES[before['kind']] + ' ' + before['variant'] if before else '-'}: {e}") from e
        n_closing += kind in FEED_KINDS and "law" in s["want"]
    pairs = {(a["kind"], b["kind"]) for a, b in zip(steps, steps[1:])}
    print(f"{variant}/{name}: {len(steps)} steps, {len(pairs)} ordered pairs, {n_ranged} in document ranges, {n_closing} closing "
          f"a feed sequence, in {time.perf_counter() - t0:.1f} s")
    assert len(pairs) == K * K and n_ranged > 0 and n_closing > 0
    for f in env["feeds"]:
        f.close()


# ---- threads beside release, with every family ---------------------------------------------------------------------------------

def test_family_calls_on_one_handle_beside_release(monkeypatch):
    """Two threads, each with feeds and a stream of its own, run shuffled rounds of the successful kinds on one handle (each
    call leases its own scratch set) while a third releases the scratch every few milliseconds: every result is the
    reference's, no step raises, and each worker completes at least one full round.  A worker's round is the walk's plan
    filtered to its successful kinds -- feed steps in the plan's order, so the sims' answers hold, the batch steps shuffled
    in between."""
    import torch

    ks = key_set("ascii")
    steps, n_seqs = plan_walk("ascii")
    for v in ENGINE_VARS:
        monkeypatch.delenv(v, raising=False)
    g = compile_bounded(monkeypatch, "auto", ks)
    for t in ks.texts:
        t.dev()
    torch.cuda.synchronize()
    ok_kinds = set(range(K)) - {RELEASE, CAPF, BADOFF, F_REFUSED, COUNT_R}  # (COUNT_R sets a process-wide variable)
    # one round: the walk's successful steps, so sequences of every feed family close in it
    round_steps = [s for s in steps if s["kind"] in ok_kinds]
    assert {s["kind"] for s in round_steps} == ok_kinds
    assert {s["want"]["sub"][:3] for s in round_steps if s["kind"] in FEED_KINDS and s["want"].get("law") is not None} == \
        {"mcc", "sel", "rep", "gre", "sep"}
    errs, done, counts = [], threading.Event(), [0, 0, 0]
    deadline = time.perf_counter() + 25

    def work(wk):
        try:
            st = torch.cuda.Stream()
            env = open_env(g, ks, n_seqs, st)
            rng = random.Random(80 + wk)
            for r in range(2):
                # feed steps keep the plan's order; batch steps are shuffled among themselves
                batch = [s for s in round_steps if s["kind"] not in FEED_KINDS]
                rng.shuffle(batch)
                it = iter(batch)
                order = [s if s["kind"] in FEED_KINDS else next(it) for s in round_steps]
                if r:  # (a further round starts the feeds from nothing, as the plan did)
                    for f in env["feeds"]:
                        f.reset()
                    env["reported"], env["holders"] = {}, {}
                for s in order:
                    try:
                        run_step(g, env, s)
                    except (AssertionError, AhaError) as e:
                        raise AssertionError(f"worker {wk}, round {r}, step {s['i']} ({KIND_NAMES[s['kind']]} {s['variant']}): {e}") from e
                counts[wk] += 1
                if time.perf_counter() > deadline:
                    break
        except Exception as e:  # noqa: BLE001
            errs.append((wk, repr(e)))

    def releaser():
        while not done.is_set():
            g.release_scratch()
            counts[2] += 1
            time.sleep(0.003)

    ths = [threading.Thread(target=work, args=(wk,)) for wk in (0, 1)]
    rel = threading.Thread(target=releaser)
    rel.start()
    for th in ths:
        th.start()
    for th in ths:
        th.join()
    done.set()
    rel.join()
    assert not errs, errs
    assert counts[0] >= 1 and counts[1] >= 1 and counts[2] > 1, counts
