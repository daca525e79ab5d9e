"""Feed calls against plain match calls of the same batch, batch resident on the device (one MI355X).

For cfg 2 at 64 MiB, cfg 3 at 1 GiB and cfg 5 at 256 MiB, in bytes and in chars: the batch's documents are the pieces of as
many sequences (cfg 3: 1024 sequences, one 1 MiB piece each per call), fed again on every call so that every piece after the
first call has a context.  Records the median of --steps timed calls (after --warmup) of the feed call and of
match_batch_device on the same pieces with the same capacity, both hit counts (they differ by the hits that straddle a
cut), and a device-to-device copy of the hits' bytes (the bound kfd_merge is set against; its own time comes from a
kernel trace: rocprofv3 --kernel-trace --stats).  Prints one JSON line.
Usage: python tools/feed_bench.py [--steps 10] [--warmup 3] [--configs 2,3,5]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SIZES = {2: 64 << 20, 3: 1 << 30, 5: 256 << 20}


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


def run_cfg(cfg, steps, warmup):
    import torch
    from aha_amd import AC, synth

    blob, offs, nf = synth.keys(cfg)
    corpus, doc = synth.corpus(cfg, blob, offs, nf, n_bytes=SIZES[cfg])
    m = AC.compile_packed(blob, offs)
    dev = "cuda:0"
    ct = torch.from_numpy(corpus).to(dev)
    ot = torch.from_numpy(doc.astype(np.int64)).to(dev)
    D = doc.size - 1
    it = torch.arange(D, dtype=torch.int32, device=dev)
    dho = torch.zeros(D + 1, dtype=torch.int64, device=dev)
    pho = torch.zeros(D + 1, dtype=torch.int64, device=dev)
    bases = torch.zeros(D, dtype=torch.int64, device=dev)
    out = []
    for chars in (False, True):
        res = {"config": cfg, "chars": chars, "bytes": int(corpus.size), "pieces": int(D), "keys": int(m.n_keys)}
        n = m.count_batch_device(ct, ot, None, dho)
        hits = torch.zeros((n + 1024, 3), dtype=torch.int32, device=dev)
        res["hits_match"] = m.match_batch_device(ct, ot, hits, dho, chars=chars)
        m.set_profiling(True)
        m.match_batch_device(ct, ot, hits, dho, chars=chars)
        res["engine_match"] = m.last_timing()["engine"]
        m.set_profiling(False)
        res["ms_match"] = _median_ms(lambda: m.match_batch_device(ct, ot, hits, dho, chars=chars), steps, warmup)
        m.release_scratch()
        f = m.feed(D, chars=chars)
        res["hits_feed_first"] = f.match_batch_device(ct, ot, it, hits, pho, bases)
        res["hits_feed"] = f.match_batch_device(ct, ot, it, hits, pho, bases)  # (every piece now has a context)
        m.set_profiling(True)
        f.match_batch_device(ct, ot, it, hits, pho, bases)
        res["engine_feed"] = m.last_timing()["engine"]
        m.set_profiling(False)
        res["ms_feed"] = _median_ms(lambda: f.match_batch_device(ct, ot, it, hits, pho, bases), steps, warmup)
        res["scratch_match_sets"] = int(m.scratch_bytes())
        nh = res["hits_feed"]
        dst = torch.empty_like(hits[:nh])
        res["ms_copy_hits"] = _median_ms(lambda: dst.copy_(hits[:nh]), steps, warmup)
        res["hit_bytes"] = int(nh * 12)
        res["ratio_feed_match"] = round(res["ms_feed"] / res["ms_match"], 3)
        f.close()
        del hits, dst
        torch.cuda.empty_cache()
        m.release_scratch()
        out.append(res)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--configs", default="2,3,5")
    a = ap.parse_args()
    res = {"tool": "feed_bench", "steps": a.steps, "warmup": a.warmup, "results": []}
    for c in a.configs.split(","):
        res["results"] += run_cfg(int(c), a.steps, a.warmup)
    print(json.dumps(res))
    return 0


if __name__ == "__main__":
    sys.exit(main())
