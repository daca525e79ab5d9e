"""Feed match and count calls with a separator filter against the plain feed match of the same pieces, batch resident on the
device (one MI355X), by tools/feed_bench.py's method: cfg 2 at 64 MiB and cfg 3 at 1 GiB, the batch's documents are the pieces
of as many sequences, fed again on every call so that every piece has a context.  The three calls alternate call by call
(plain feed match, filtered feed match, filtered feed count); the medians of --steps rounds after --warmup are recorded, with
the unfiltered and the kept hit counts.  The separator set is chosen from the first 32 MiB of the batch so that roughly half
the hits survive where byte values allow it: every byte value passes except a blocked set, grown greedily among the most
frequent neighbours of hits towards a kept share of a half (keywords between spaces leave little choice: the kept share is
recorded).
Prints one JSON line.  Usage: python tools/feed_sep_bench.py [--steps 10] [--warmup 3] [--configs 2,3]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SIZES = {2: 64 << 20, 3: 1 << 30}


def choose_sep(m, corpus, doc):
    """a BitArray chosen on the hits of the batch's first 32 MiB: every byte value passes except a set of blocked ones, grown
    greedily -- among the 24 most frequent neighbours, the byte whose blocking brings the kept share closest to a half -- until
    no byte brings it closer"""
    from aha_amd import BitArray

    k = max(int(np.searchsorted(doc, 32 << 20, side="right")) - 1, 1)
    hits, dho = m.match_batch(corpus[: int(doc[k])], doc[: k + 1])
    owner = np.repeat(np.arange(k), np.diff(dho.astype(np.int64)))
    a, b = doc[owner].astype(np.int64), doc[owner + 1].astype(np.int64)
    end = a + hits["end"].astype(np.int64)
    left = a + hits["start"].astype(np.int64) - 1
    # 256: the document's end or start, which always passes
    rn = np.where(end < b, corpus[np.minimum(end, corpus.size - 1)].astype(np.int64), 256)
    ln = np.where(left >= a, corpus[np.maximum(left, 0)].astype(np.int64), 256)
    cand = [int(c) for c in np.argsort(-(np.bincount(rn, minlength=257) + np.bincount(ln, minlength=257))[:256])[:24]]
    blocked = np.zeros(257, dtype=bool)

    def kept(bl):
        return float(np.mean(~bl[rn] & ~bl[ln])) if len(hits) else 1.0

    share, chosen = kept(blocked), []
    while True:
        best = None
        for c in cand:
            if blocked[c]:
                continue
            blocked[c] = True
            s = kept(blocked)
            blocked[c] = False
            if abs(s - 0.5) < abs(share - 0.5) and (best is None or abs(s - 0.5) < abs(best[1] - 0.5)):
                best = (c, s)
        if best is None:
            break
        blocked[best[0]] = True
        chosen.append(best[0])
        share = best[1]
    sep = BitArray(256)
    for c in range(256):
        sep[c] = not blocked[c]
    return sep, chosen


def run_cfg(cfg, steps, warmup):
    import torch
    from aha_amd import AC, synth

    blob, offs, nf = synth.keys(cfg)
    corpus, doc = synth.corpus(cfg, blob, offs, nf, n_bytes=SIZES[cfg])
    m = AC.compile_packed(blob, offs)
    sep, blocked = choose_sep(m, corpus, doc)
    dev = "cuda:0"
    ct = torch.from_numpy(corpus).to(dev)
    ot = torch.from_numpy(doc.astype(np.int64)).to(dev)
    D = doc.size - 1
    it = torch.arange(D, dtype=torch.int32, device=dev)
    pho = torch.zeros(D + 1, dtype=torch.int64, device=dev)
    bases = torch.zeros(D, dtype=torch.int64, device=dev)
    kc = torch.zeros(m.n_keys, dtype=torch.int64, device=dev)
    res = {"config": cfg, "bytes": int(corpus.size), "pieces": int(D), "keys": int(m.n_keys), "blocked_bytes": blocked}
    n = m.count_batch_device(ct, ot, None, pho)
    res["hits_plain_match_sep"] = m.count_batch_device(ct, ot, None, pho, sep=sep)
    hits = torch.zeros((n + n // 8 + 1024, 3), dtype=torch.int32, device=dev)
    plain, fm, fc = m.feed(D), m.feed(D, sep=sep), m.feed(D, sep=sep)
    calls = {
        "plain_feed_match": lambda: plain.match_batch_device(ct, ot, it, hits, pho, bases),
        "sep_feed_match": lambda: fm.match_batch_device(ct, ot, it, hits, pho, bases),
        "sep_feed_count": lambda: fc.count_batch_device(ct, ot, it, kc, pho, bases),
    }
    for name, fn in calls.items():  # (every piece has a context from the second call on)
        fn()
        res["hits_" + name] = fn()
    ts = {name: [] for name in calls}
    for step in range(warmup + steps):
        for name, fn in calls.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            if step >= warmup:
                ts[name].append((time.perf_counter() - t0) * 1e3)
    for name in calls:
        res["ms_" + name] = float(np.median(ts[name]))
    res["kept_share"] = round(res["hits_sep_feed_match"] / max(res["hits_plain_feed_match"], 1), 4)
    res["ms_filter_pass_match"] = round(res["ms_sep_feed_match"] - res["ms_plain_feed_match"], 4)
    res["ms_filter_pass_count"] = round(res["ms_sep_feed_count"] - res["ms_plain_feed_match"], 4)
    for f in (plain, fm, fc):
        f.close()
    del hits
    torch.cuda.empty_cache()
    m.release_scratch()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--configs", default="2,3")
    a = ap.parse_args()
    res = {"tool": "feed_sep_bench", "steps": a.steps, "warmup": a.warmup, "results": []}
    for c in a.configs.split(","):
        res["results"].append(run_cfg(int(c), a.steps, a.warmup))
    print(json.dumps(res))
    return 0


if __name__ == "__main__":
    sys.exit(main())
