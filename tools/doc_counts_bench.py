"""Document counts against what a caller must do without them, batch resident on the device (one MI355X).

For cfg 2 at 64 MiB, cfg 3 at 1 GiB and cfg 5 at 256 MiB, medians of --steps timed calls (after --warmup):
(a) doc_counts_batch_device; (b) match_batch_device (cap = hits), then torch.unique(doc_id << 32 | value,
return_counts=True) on the device, the doc ids from a searchsorted of the hit index in doc_hit_offsets; (c)
match_batch_device alone and count_batch_device alone (to hold against profiles/count_bench.json).  The pairs of (a) are
checked against (b)'s in the same run.  Prints one JSON line.
Usage: python tools/doc_counts_bench.py [--steps 10] [--warmup 3] [--configs 2,3,5]"""
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
    from aha_amd import AC, AhaError, synth

    blob, offs, nf = synth.keys(cfg)
    corpus, doc = synth.corpus(cfg, blob, offs, nf, n_bytes=SIZES[cfg])
    m = AC.compile_packed(blob, offs)
    K = m.n_keys
    dev = "cuda:0"
    ct = torch.from_numpy(corpus).to(dev)
    ot = torch.from_numpy(doc.astype(np.int64)).to(dev)
    D = doc.size - 1
    dho = torch.zeros(D + 1, dtype=torch.int64, device=dev)
    dpo = torch.zeros(D + 1, dtype=torch.int64, device=dev)
    kc = torch.zeros(K, dtype=torch.int64, device=dev)
    res = {"config": cfg, "bytes": int(corpus.size), "keys": int(K), "docs": int(D)}
    try:
        n_pairs, n_hits = m.doc_counts_batch_device(ct, ot, None)
    except AhaError as e:
        n_pairs, n_hits = e.n_required, e.n_hits
    res["hits"], res["pairs"] = n_hits, n_pairs
    pairs = torch.zeros((n_pairs + 1, 2), dtype=torch.int32, device=dev)
    m.release_scratch()
    res["ms_doc_counts"] = _median_ms(lambda: m.doc_counts_batch_device(ct, ot, pairs, dpo), steps, warmup)
    res["scratch_doc_counts"] = int(m.scratch_bytes())
    m.set_profiling(True)
    m.doc_counts_batch_device(ct, ot, pairs, dpo)
    t = m.last_timing()
    res["doc_counts_timing"] = {k: (round(v, 4) if isinstance(v, float) else v) for k, v in t.items()}
    m.set_profiling(False)
    m.release_scratch()
    out = torch.zeros((n_hits + 1, 3), dtype=torch.int32, device=dev)

    def without():
        m.match_batch_device(ct, ot, out, dho)
        docid = torch.searchsorted(dho, torch.arange(n_hits, device=dev), right=True) - 1
        return torch.unique((docid << 32) | out[:n_hits, 2].to(torch.int64), return_counts=True)

    try:
        res["ms_match_unique"] = _median_ms(without, steps, warmup)
        keys, cnts = without()
        res["pairs_ok"] = bool(keys.numel() == n_pairs and torch.equal(keys & 0xFFFFFFFF, pairs[:n_pairs, 0].to(torch.int64))
                               and torch.equal(cnts, pairs[:n_pairs, 1].to(torch.int64))
                               and torch.equal(torch.searchsorted(keys >> 32, torch.arange(D + 1, device=dev)), dpo))
        del keys, cnts
    except torch.OutOfMemoryError:
        res["ms_match_unique"], res["pairs_ok"] = None, None  # (the general sort does not fit beside the hits)
    torch.cuda.empty_cache()
    res["ms_match"] = _median_ms(lambda: m.match_batch_device(ct, ot, out, dho), steps, warmup)
    del out
    torch.cuda.empty_cache()
    m.release_scratch()
    res["ms_count"] = _median_ms(lambda: m.count_batch_device(ct, ot, kc, dho), steps, warmup)
    res["ms_count_no_keys"] = _median_ms(lambda: m.count_batch_device(ct, ot, None, dho), steps, warmup)
    if res["ms_match_unique"]:
        res["speedup_over_match_unique"] = round(res["ms_match_unique"] / res["ms_doc_counts"], 3)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--configs", default="2,3,5")
    a = ap.parse_args()
    out = {"tool": "doc_counts_bench", "steps": a.steps, "warmup": a.warmup, "results": []}
    for c in a.configs.split(","):
        out["results"].append(run_cfg(int(c), a.steps, a.warmup))
    out["ok"] = all(r["pairs_ok"] is not False for r in out["results"])
    print(json.dumps(out))
    return 0 if out["ok"] else 1


if __name__ == "__main__":
    sys.exit(main())
