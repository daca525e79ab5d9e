"""Feed counts against plain counts and feed matches of the same pieces, batch resident on the device (one MI355X).

For cfg 2 at 64 MiB, cfg 3 at 1 GiB (bytes and chars) and cfg 5 at 256 MiB, in two shapes: the batch's documents as the pieces
of as many sequences (cfg 3: 1024 sequences, one 1 MiB piece each per call), and the whole batch as one piece of one
sequence.  Either is fed again on every call, so that every piece after the first call has a context (tools/feed_bench.py's
method).  Records the median of --steps timed calls (after --warmup) of
  ms_count              aha_ac_count_batch_device of the same pieces as documents, with key counts
  ms_feed_count         aha_feed_count_batch_device, with key counts
  ms_feed_count_totals  the same without key counts (totals, offsets and bases only)
  ms_feed_match         aha_feed_match_batch_device
the engines of the plain count and of the feed count's main pass, and the hit counts (the feed's differ from the plain ones
by the hits that straddle a cut).  The window passes' own times come from a kernel trace: rocprofv3 --kernel-trace --stats.
Prints one JSON line.
Usage: python tools/feed_count_bench.py [--steps 10] [--warmup 3] [--configs 2,3,5]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SIZES = {2: 64 << 20, 3: 1 << 30, 5: 256 << 20}
CHARS = {2: (False,), 3: (False, True), 5: (False,)}


def _median_ms(fn, steps, warmup):
    import torch

    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(steps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts))


def _engine(m, fn):
    m.set_profiling(True)
    fn()
    e = m.last_timing()["engine"]
    m.set_profiling(False)
    return e


def run_shape(m, ct, ot, cfg, chars, shape, steps, warmup):
    import torch

    dev = "cuda:0"
    D = ot.numel() - 1
    it = torch.arange(D, dtype=torch.int32, device=dev)
    dho = torch.zeros(D + 1, dtype=torch.int64, device=dev)
    pho = torch.zeros(D + 1, dtype=torch.int64, device=dev)
    bases = torch.zeros(D, dtype=torch.int64, device=dev)
    kc = torch.zeros(m.n_keys, dtype=torch.int64, device=dev)
    res = {"config": cfg, "chars": chars, "shape": shape, "bytes": int(ct.numel()), "pieces": int(D), "keys": int(m.n_keys)}
    res["hits_count"] = m.count_batch_device(ct, ot, kc, dho)
    res["engine_count"] = _engine(m, lambda: m.count_batch_device(ct, ot, kc, dho))
    res["ms_count"] = _median_ms(lambda: m.count_batch_device(ct, ot, kc, dho), steps, warmup)
    m.release_scratch()
    f = m.feed(D, chars=chars)
    res["hits_feed_first"] = f.count_batch_device(ct, ot, it, kc, pho, bases)
    res["hits_feed"] = f.count_batch_device(ct, ot, it, kc, pho, bases)  # (every piece now has a context)
    res["engine_feed_count"] = _engine(m, lambda: f.count_batch_device(ct, ot, it, kc, pho, bases))
    res["ms_feed_count"] = _median_ms(lambda: f.count_batch_device(ct, ot, it, kc, pho, bases), steps, warmup)
    res["ms_feed_count_totals"] = _median_ms(lambda: f.count_batch_device(ct, ot, it, None, pho, bases), steps, warmup)
    hits = torch.zeros((res["hits_feed"] + 1024, 3), dtype=torch.int32, device=dev)
    assert f.match_batch_device(ct, ot, it, hits, pho, bases) == res["hits_feed"]
    res["ms_feed_match"] = _median_ms(lambda: f.match_batch_device(ct, ot, it, hits, pho, bases), steps, warmup)
    res["ms_feed_count_minus_count"] = round(res["ms_feed_count"] - res["ms_count"], 4)
    res["ratio_feed_count_count"] = round(res["ms_feed_count"] / res["ms_count"], 3)
    res["ratio_feed_count_feed_match"] = round(res["ms_feed_count"] / res["ms_feed_match"], 3)
    f.close()
    del hits
    torch.cuda.empty_cache()
    m.release_scratch()
    return res


def run_cfg(cfg, steps, warmup):
    import torch
    from aha_amd import AC, synth

    blob, offs, nf = synth.keys(cfg)
    corpus, doc = synth.corpus(cfg, blob, offs, nf, n_bytes=SIZES[cfg])
    m = AC.compile_packed(blob, offs)
    ct = torch.from_numpy(corpus).to("cuda:0")
    out = []
    for shape, d in (("many", doc), ("one", np.array([0, corpus.size], dtype=np.uint64))):
        ot = torch.from_numpy(d.astype(np.int64)).to("cuda:0")
        for chars in CHARS[cfg]:
            out.append(run_shape(m, ct, ot, cfg, chars, shape, steps, warmup))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--configs", default="2,3,5")
    a = ap.parse_args()
    res = {"tool": "feed_count_bench", "steps": a.steps, "warmup": a.warmup, "results": []}
    for c in a.configs.split(","):
        res["results"] += run_cfg(int(c), a.steps, a.warmup)
    print(json.dumps(res))
    return 0


if __name__ == "__main__":
    sys.exit(main())
