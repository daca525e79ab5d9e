"""CPU model of a longest feed (aha_feed_open_params with longest = 1 | 2, aha_feed_finish_batch): a resumable restatement of
pymodel.ModelAC.match_longest's loop (src/aha/ac.cr:118-143, 249-263).  Per sequence it keeps what the loop keeps between two
bytes -- the node, the pending end (its absolute position and node), the length so far -- so a piece continues where the last one
stopped.  is_end? is "ends a key" or "the node's path is in the stale set" (orc.AC.stale_paths(): Cedar's stale END flags are a
property of its slot history); VALUE_NODE is the label-0 child a NUL byte reaches from a node that ends a key and has children.

The stream law: a hit is yielded at the first byte that finds no goto while it is the pending end; a call that takes a sequence
from n0 to n1 bytes reports the hits yielded at a byte in [n0, n1), relative to the piece's first byte; finish reports the hit
still pending, relative to the sequence's end, and the sequence starts again.  fold: the handle folds ASCII case (the keys given
here are the folded ones; the text is folded here).

CASES / case_keys / case_text: the key sets, texts and cuts the host test and the GPU test share."""
import random
import zlib

import numpy as np

from pymodel import ModelAC
from pyoracle import HIT_DTYPE

EMPTY = np.zeros(0, dtype=HIT_DTYPE)
VALUE_NODE = -2


def hits_array(rows):
    out = np.zeros(len(rows), dtype=HIT_DTYPE)
    for i, (a, e, v) in enumerate(rows):
        out[i] = (a, e, v)
    return out


class FeedLongestSim:
    def __init__(self, keys, n_seqs, intersectable, stale=(), fold=False):
        self.m = ModelAC(keys)
        self.lmax = max(len(k) for k in self.m.keys)
        self.intersectable, self.fold = bool(intersectable), fold
        self.stale_nodes = set()
        for path in stale:
            n = 0
            for b in path:
                n = self.m.children[n][b]
            self.stale_nodes.add(n)
        self.state = [(0, -1, -1, 0)] * n_seqs  # node, pending end (absolute, -1: none), its node, bytes so far

    def _hit(self, i, n):
        k = self.m.key_of[n] if n >= 0 else -1
        return [(i - len(self.m.keys[k]) + 1, i + 1, k)] if k >= 0 else []

    def piece(self, seq, P):
        """-> (hits relative to the piece, base) and the sequence moves on by P"""
        m = self.m
        nid, prev_i, prev_nid, n0 = self.state[seq]
        P = bytes(P).lower() if self.fold else bytes(P)  # (bytes.lower folds ASCII only)
        out = []
        for i, b in enumerate(P, n0):
            while True:
                if nid == VALUE_NODE:  # no goto from it, no fail link: the pending (empty) end is yielded, the byte is gone
                    prev_i = -1
                    nid = 0
                    break
                if b == 0 and m.key_of[nid] >= 0 and m.children[nid]:
                    nid = VALUE_NODE
                    prev_i, prev_nid = i, nid
                    break
                nxt = m.children[nid].get(b) if b else None
                if nxt is not None:
                    nid = nxt
                    if m.key_of[nid] >= 0 or nid in self.stale_nodes:
                        prev_i, prev_nid = i, nid
                    break
                if prev_i != -1:
                    out += self._hit(prev_i, prev_nid)
                    prev_i = -1
                    if not self.intersectable:
                        nid = 0
                if nid == 0:
                    break
                nid = m.fail[nid]
        self.state[seq] = (nid, prev_i, prev_nid, n0 + len(P))
        return hits_array([(a - n0, e - n0, v) for a, e, v in out]), n0

    def finish(self, seq):
        """-> (the pending hit relative to the sequence's end, its length) and the sequence starts again"""
        _, prev_i, prev_nid, n = self.state[seq]
        out = self._hit(prev_i, prev_nid) if prev_i != -1 else []
        self.state[seq] = (0, -1, -1, 0)
        return hits_array([(a - n, e - n, v) for a, e, v in out]), n

    def reset(self, seq):
        self.state[seq] = (0, -1, -1, 0)

    def position(self, seq):
        return self.state[seq][3]


def absolute(hits, base):
    out = hits.copy()
    out["start"] += base
    out["end"] += base
    return out


# ---- the cases the host test and the GPU test share ---------------------------------------------------------------------------
CASES = ("nested", "single", "long", "ascii", "stale")


def stale_keys(seed=0):
    """a random two-letter key set whose Cedar holds stale END flags (test_gpu_parity's match_longest generator finds them among
    such sets): the first seed from `seed` on whose oracle census is non-empty -> (keys, stale paths)"""
    import pyoracle as orc

    for s in range(seed, seed + 200):
        rng = random.Random(1000 + s)
        keys = sorted({bytes(rng.choice(b"ab") for _ in range(rng.randint(1, 7))) for _ in range(rng.randint(6, 40))})
        stale = orc.AC.compile(keys).stale_paths()
        if stale:
            return keys, stale
    raise AssertionError("no two-letter key set with stale END flags found")


def case_keys(name):
    """-> (keys, stale paths of the oracle's Cedar)"""
    import pyoracle as orc
    from test_gpu_feed import KEYSETS

    if name == "stale":
        return stale_keys()
    keys = KEYSETS[name](random.Random(zlib.crc32(f"feed-longest/{name}".encode())))
    return keys, orc.AC.compile(keys).stale_paths()


def case_text(name, keys, n=None):
    """n bytes (60; 230 for `long`) dense in keys, with a NUL behind a key that has children (the value node), two NULs in a row
    and a lone NUL"""
    if n is None:
        n = 230 if name == "long" else 60
    rng = random.Random(zlib.crc32(f"feed-longest-text/{name}/{n}".encode()))
    short = [k for k in keys if len(k) <= max(8, n // 2)]
    keyset = set(keys)
    parents = [k for k in short if any(o != k and o.startswith(k) for o in keyset)]
    out = bytearray()
    if parents:
        out += rng.choice(parents) + b"\x00"
    while len(out) < n:
        r = rng.random()
        if r < 0.6:
            out += rng.choice(short)
        elif r < 0.7 and parents:
            out += rng.choice(parents) + b"\x00"
        elif r < 0.78:
            out += b"\x00\x00" if rng.random() < 0.4 else b"\x00"
        else:
            out += bytes([rng.choice(b"abxyq \x80")])
    return bytes(out[:n])
