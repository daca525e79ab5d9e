"""What a folded feed (AHA_FEED_FOLD: a feed on a handle compiled with fold_simple, fold_bmp or fold_kana) costs beside the feed of
an ASCII-folded handle on the same pieces, batch resident on the device (one MI355X).

cfg 3's keys compiled four times -- fold_ascii (the yardstick: its feed is the code as it was), fold_simple, fold_bmp, fold_kana --
and cfg 3's corpus at --mib MiB as the pieces of as many sequences as it has documents.  Every feed is fed the same pieces again
on every call, so every piece after the first call has a context.  Feed match (hits, piece_hit_offsets, bases) and feed cover
(mask, piece_back) are timed for the four feeds in turn, call by call: the median of --steps alternating calls with [min, max]
(after --warmup rounds).  The text holds nothing the folds move, so all four report the same hits; the tool checks that.
The two new kernels' own times (kff_heads, kff_windows) come from a kernel trace, rocprofv3 --kernel-trace --stats, in a run
of its own (--trace-calls N: N match and N cover calls per folded feed and nothing else, for that run).
--plain-only: the gate's half -- a plain handle's feed match on the same pieces alone, which runs on any build.
Prints one JSON line; --out writes it to a file as well.
Usage: python tools/feed_fold_bench.py [--steps 10] [--warmup 2] [--mib 1024] [--out profiles/feed_fold_bench.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
DEV = "cuda:0"
MODES = (("ascii", "fold_ascii"), ("simple", "fold_simple"), ("bmp", "fold_bmp"), ("kana", "fold_kana"))


def _alternate(fns, steps, warmup):
    import torch

    for _ in range(warmup):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    ts = {k: [] for k in fns}
    for _ in range(steps):
        for k, fn in fns.items():
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ts[k].append((time.perf_counter() - t0) * 1e3)
    return {k: {"median_ms": round(float(np.median(v)), 4), "min_ms": round(float(min(v)), 4), "max_ms": round(float(max(v)), 4)}
            for k, v in ts.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--mib", type=int, default=1024)
    ap.add_argument("--trace-calls", type=int, default=0)
    ap.add_argument("--plain-only", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch

    if not torch.cuda.is_available():
        print("feed_fold_bench: no GPU (there is no CPU fallback for a measurement)", file=sys.stderr)
        return 2
    from aha_amd import AC, synth

    blob, offs, nf = synth.keys(3)
    corpus, doc = synth.corpus(3, blob, offs, nf, n_bytes=a.mib << 20)
    n, D = int(corpus.size), int(doc.size - 1)
    ct = torch.from_numpy(corpus).to(DEV)
    ot = torch.from_numpy(doc.astype(np.int64)).to(DEV)
    it = torch.arange(D, dtype=torch.int32, device=DEV)
    pho = torch.zeros(D + 1, dtype=torch.int64, device=DEV)
    bases = torch.zeros(D, dtype=torch.int64, device=DEV)
    back = torch.zeros(D, dtype=torch.int32, device=DEV)
    mask = torch.zeros((n + 31) // 32, dtype=torch.int32, device=DEV)
    res = {"tool": "feed_fold_bench", "steps": a.steps, "warmup": a.warmup, "config": 3, "bytes": n, "pieces": D,
           "keys": int(offs.size - 1)}

    if a.plain_only:
        m = AC.compile_packed(blob, offs)
        f = m.feed(D)
        hits = m.count_batch_device(ct, ot, None, None)
        out = torch.zeros((hits + (1 << 20), 3), dtype=torch.int32, device=DEV)
        f.match_batch_device(ct, ot, it, out, pho, bases)
        res["plain_feed_match"] = _alternate({"x": lambda: f.match_batch_device(ct, ot, it, out, pho, bases)}, a.steps, a.warmup)["x"]
        print(json.dumps(res))
        return 0

    handles, feeds = {}, {}
    for name, opt in MODES:
        handles[name] = AC.compile_packed(blob, offs, **{opt: True})
        feeds[name] = handles[name].feed(D) if name == "ascii" else handles[name].feed(D, fold=True)
    hits0 = handles["ascii"].count_batch_device(ct, ot, None, None)
    out = torch.zeros((hits0 + (1 << 20), 3), dtype=torch.int32, device=DEV)
    res["hits_first_call"], res["hits"], res["covered"], res["engine"] = {}, {}, {}, {}
    for name, f in feeds.items():  # the first call has no contexts; the second is what every later call repeats
        res["hits_first_call"][name] = f.match_batch_device(ct, ot, it, out, pho, bases)
        res["hits"][name] = f.match_batch_device(ct, ot, it, out, pho, bases)
        res["covered"][name] = f.cover_batch_device(ct, ot, it, mask=mask, piece_back=back)[0]
        handles[name].set_profiling(True)
        f.match_batch_device(ct, ot, it, out, pho, bases)
        res["engine"][name] = handles[name].last_timing()["engine"]
        handles[name].set_profiling(False)
    res["equal"] = len(set(res["hits"].values())) == 1 and len(set(res["covered"].values())) == 1
    if a.trace_calls:
        for name, f in feeds.items():
            if name != "ascii":
                for _ in range(a.trace_calls):
                    f.match_batch_device(ct, ot, it, out, pho, bases)
                    f.cover_batch_device(ct, ot, it, mask=mask, piece_back=back)
        torch.cuda.synchronize()
        res["traced_calls_per_folded_feed"] = a.trace_calls
        print(json.dumps(res))
        return 0
    res["feed_match"] = _alternate({k: (lambda f=f: f.match_batch_device(ct, ot, it, out, pho, bases)) for k, f in feeds.items()},
                                   a.steps, a.warmup)
    res["feed_cover"] = _alternate({k: (lambda f=f: f.cover_batch_device(ct, ot, it, mask=mask, piece_back=back)) for k, f in feeds.items()},
                                   a.steps, a.warmup)
    for fam in ("feed_match", "feed_cover"):
        base = res[fam]["ascii"]["median_ms"]
        res[fam + "_less_ascii_ms"] = {k: round(v["median_ms"] - base, 4) for k, v in res[fam].items() if k != "ascii"}
    res["ok"] = bool(res["equal"])
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(res, fh, indent=1)
            fh.write("\n")
    return 0 if res["ok"] else 1


if __name__ == "__main__":
    sys.exit(main())
