"""What the call-sequence walks share (tests/test_gpu_call_sequences.py, tests/test_gpu_family_sequences.py): the engine
variants a handle is compiled under, the de Bruijn walk over call kinds, a batch of documents with its device copy, the key
lists of the two key sets, and the sentinel helpers -- buffers prefilled with values no call writes, and the checks that what
lies behind a call's output still holds them."""
import numpy as np

import pyoracle as orc
from aha_amd import AC

# the engine variants of test_gpu_parity.py's fixture (the opt-in skip and pair engines left out); read at compile time
ENGINE_VARS = ("AHA_ENGINE", "AHA_UNIT_HEADER_BESIDE", "AHA_UNIT_BASE_BITS", "AHA_UNIT_POST", "AHA_LDS_SLOTS")
VARIANTS = {
    "auto": {},
    "v2": {"AHA_ENGINE": "v2"},
    "v1": {"AHA_ENGINE": "v1"},
    "u": {"AHA_ENGINE": "unit", "AHA_UNIT_HEADER_BESIDE": "0"},
    "ur": {"AHA_ENGINE": "unit", "AHA_UNIT_POST": "regroup"},
    "uh": {"AHA_ENGINE": "unit", "AHA_UNIT_HEADER_BESIDE": "1"},
    "f": {"AHA_ENGINE": "filter"},
}

S32 = -7                          # sentinel of the int32 hit rows
S64 = 0xFFFFFFFFFFFFFFFB          # sentinel of the uint64 per-document offsets
PAD = 64                          # rows / entries behind what a call may write


def de_bruijn_walk(k):
    """Kinds 0 .. k-1 in an order in which every ordered pair (a, b) stands next to each other once: k^2 + 1 steps."""
    a = [0] * (2 * k)
    seq = []

    def db(t, p):
        if t > 2:
            if 2 % p == 0:
                seq.extend(a[1:p + 1])
        else:
            a[t] = a[t - p]
            db(t + 1, p)
            for j in range(a[t - p] + 1, k):
                a[t] = j
                db(t + 1, t)

    db(1, 1)
    return seq + seq[:1]


class Text:
    def __init__(self, docs):
        self.docs = [d.encode() if isinstance(d, str) else d for d in docs]
        self.corpus = np.frombuffer(b"".join(self.docs), dtype=np.uint8).copy()
        self.offs = np.cumsum([0] + [len(d) for d in self.docs]).astype(np.uint64)
        self.D = len(self.docs)
        self._dev = None

    def dev(self):
        import torch

        if self._dev is None:
            self._dev = (torch.from_numpy(self.corpus).cuda(), torch.from_numpy(self.offs.astype(np.int64)).cuda())
        return self._dev


def ascii_keys(rng):
    """(keys, nested): ASCII keys of 3 to 64 bytes (the prefix-filter engine's), the last six nested on one walk"""
    keys = set()
    while len(keys) < 150:
        keys.add("".join(rng.choice("abcdefghijkl") for _ in range(rng.randint(3, 8))))
    keys = sorted(keys) + ["".join(rng.choice("abcdefghijklmnopqrstuvwxyz") for _ in range(n)) for n in (20, 33, 64)]
    nested = ["qrstuvwxy"[:n] for n in range(4, 10)]
    return list(dict.fromkeys(keys + nested)), nested


def cjk_keys(rng):
    """(keys, code points): CJK / mixed UTF-8 keys of 1 to 4 characters (the character-level image under `auto`)"""
    cps = [chr(c) for c in list(range(0x4E00, 0x4E30)) + list(range(97, 105)) + list(range(0x430, 0x438))]
    keys, seen = [], set()
    while len(keys) < 150:
        k = "".join(rng.choice(cps) for _ in range(rng.randint(1, 4)))
        if k not in seen:
            seen.add(k)
            keys.append(k)
    return keys, cps


def compile_under(monkeypatch, variant, keys, **kw):
    for v in ENGINE_VARS:
        monkeypatch.delenv(v, raising=False)
    for k, v in VARIANTS[variant].items():
        monkeypatch.setenv(k, v)
    return AC.compile(keys, **kw)


# ---- sentinels ------------------------------------------------------------------------------------------------------------

def hits_np(cap):
    out = np.empty(cap + PAD, dtype=orc.HIT_DTYPE)
    out["start"] = out["end"] = out["value"] = S32
    return out


def check_np(out, n, want, limit):
    """hits [0, n) are the oracle's, rows [limit, end) untouched."""
    assert n == len(want)
    assert out[:n].tobytes() == want.tobytes()
    tail = out[limit:]
    assert (tail["start"] == S32).all() and (tail["end"] == S32).all() and (tail["value"] == S32).all()


def check_dev(big, n, want, limit):
    assert n == len(want)
    assert big[:n].cpu().numpy().tobytes() == want.tobytes()
    assert bool((big[limit:] == S32).all())


def dho_dev(D):
    import torch

    return torch.full((D + 1 + PAD,), S64 - (1 << 64), dtype=torch.int64, device="cuda")


def check_dho(dho, D, want):
    got = dho.cpu().numpy().astype(np.uint64) if not isinstance(dho, np.ndarray) else dho
    assert np.array_equal(got[:D + 1], want)
    assert (got[D + 1:] == np.uint64(S64)).all()
