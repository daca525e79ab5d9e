"""Feed token calls against the feed select call on the same pieces, batch resident on the device (one MI355X).

The cfg 3 key set over 64 sequences, in two shapes: pieces of 64 KiB and of 1 MiB (--piece-bytes), cut from the cfg 3 corpus
at fixed strides, so a cut falls inside a character and inside a key now and then.  The same pieces are fed again on every
call, so that every piece after the first has a context, open hits and an open token.  Three feeds, one per kind of call, are
timed in turn step by step -- a drift of the clocks between runs is larger than what a token call adds --; records the median
of --steps timed calls (after --warmup) of
  ms_feed_select       aha_feed_select_batch_device (hits, offsets, bases, hold): the yardstick, the parent's code
  ms_feed_tokens       ... with AHA_FEED_SELECT_TOKENS (character mode)
  ms_feed_tokens_runs  ... with AHA_FEED_SELECT_TOKENS | AHA_FEED_SELECT_GAP_RUNS
the two ratios to the yardstick, the selected hits and the tokens of one call, and aha_ac_last_timing behind one call of each:
it times the main pass (the match of the pieces), which the three calls share, so what a token call adds lies outside it, in
the passes behind the rank and in the 12 bytes written per token (DESIGN.md 4.10 "Feed tokens").  No threshold is set.  Writes
one JSON document to --out (default profiles/feed_tokens_bench.json) and prints it.
Usage: python tools/feed_tokens_bench.py [--steps 20] [--warmup 3] [--piece-bytes 65536,1048576] [--seqs 64]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CFG = 3


def _medians_ms(fns, steps, warmup):
    """the median time of every call, the calls taken in turn step by step so that a drift of the clocks meets them all alike"""
    import torch

    for _ in range(warmup):
        for fn in fns:
            fn()
    torch.cuda.synchronize()
    ts = [[] for _ in fns]
    for _ in range(steps):
        for i, fn in enumerate(fns):
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ts[i].append((time.perf_counter() - t0) * 1e3)
    return [float(np.median(t)) for t in ts]


def run_shape(m, ct, piece, D, steps, warmup):
    import torch

    dev = "cuda:0"
    n = piece * D
    W = max(int(m.info["max_key_len"]) - 1, 0)
    ct = ct[:n]
    ot = torch.arange(D + 1, dtype=torch.int64, device=dev) * piece
    it = torch.arange(D, dtype=torch.int32, device=dev)
    off = torch.zeros(D + 1, dtype=torch.int64, device=dev)
    bases = torch.zeros(D, dtype=torch.int64, device=dev)
    hold = torch.zeros(D, dtype=torch.int32, device=dev)
    # (at most a token per extended position and a carried one per piece)
    out = torch.empty((n + D * (W + 1), 3), dtype=torch.int32, device=dev)
    res = {"config": CFG, "piece_bytes": piece, "pieces": D, "bytes": n, "keys": int(m.n_keys), "W": W}
    calls = (("feed_select", lambda f: f.select_batch_device(ct, ot, it, out, off, bases, hold)),
             ("feed_tokens", lambda f: f.tokens_batch_device(ct, ot, it, out, off, bases, hold)),
             ("feed_tokens_runs", lambda f: f.tokens_batch_device(ct, ot, it, out, off, bases, hold, gap_runs=True)))
    feeds = []
    for name, call in calls:
        f = m.feed(D)
        feeds.append(f)
        call(f)
        res["n_" + name], res["hits"] = call(f)  # (with contexts)
        res["held_" + name] = int(hold.sum())
        m.set_profiling(True)  # (event records inside the call: for this one call only, never for the timed ones)
        call(f)
        res["timing_" + name] = {k: round(float(v), 4) for k, v in m.last_timing().items() if k.startswith("ms_")}
        m.set_profiling(False)
    ms = _medians_ms([lambda call=call, f=f: call(f) for (_, call), f in zip(calls, feeds)], steps, warmup)
    for (name, _), t, f in zip(calls, ms, feeds):
        res["ms_" + name] = round(t, 4)
        f.close()
    m.release_scratch()
    res["ratio_tokens_select"] = round(res["ms_feed_tokens"] / res["ms_feed_select"], 3)
    res["ratio_tokens_runs_select"] = round(res["ms_feed_tokens_runs"] / res["ms_feed_select"], 3)
    res["gb_per_s_feed_tokens"] = round(n / res["ms_feed_tokens"] / 1e6, 2)
    del out
    torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--piece-bytes", default="65536,1048576")
    ap.add_argument("--seqs", type=int, default=64)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "feed_tokens_bench.json"))
    a = ap.parse_args()
    import torch
    from aha_amd import AC, synth

    pieces = [int(p) for p in a.piece_bytes.split(",")]
    blob, offs, nf = synth.keys(CFG)
    corpus, _ = synth.corpus(CFG, blob, offs, nf, n_bytes=max(pieces) * a.seqs)
    m = AC.compile_packed(blob, offs)
    ct = torch.from_numpy(corpus).to("cuda:0")
    res = {"tool": "feed_tokens_bench", "steps": a.steps, "warmup": a.warmup, "results": []}
    for piece in pieces:
        res["results"].append(run_shape(m, ct, min(piece, int(ct.numel()) // a.seqs), a.seqs, a.steps, a.warmup))
    text = json.dumps(res)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text + "\n")
    print(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
