"""Cover calls against what a caller must do without them, batch resident on the device (one MI355X).

For cfg 2 at 64 MiB, cfg 3 at 1 GiB and cfg 5 at 256 MiB, medians of --steps timed calls (after --warmup), in one run:
(a) cover_batch_device with the mask only; (b) with mask + redacted; (c) match_batch_device (cap = hits), then the caller's
own byte cover from the hit list in torch -- a difference array over absolute starts and ends and a cumsum --; (d)
match_batch_device alone; (e) count_batch_device without key counts; (f) a bare device copy of the corpus.  (d) and (e) are
to be held against profiles/count_bench.json / doc_counts_bench.json.  The cover of (a) is checked against (c)'s in the same
run; scratch bytes after (a) and after (d).  Prints one JSON line.
Usage: python tools/cover_bench.py [--steps 10] [--warmup 3] [--configs 2,3,5]"""
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
    n, D = int(corpus.size), doc.size - 1
    nw = (n + 31) // 32
    dho = torch.zeros(D + 1, dtype=torch.int64, device=dev)
    mask = torch.zeros(nw, dtype=torch.int32, device=dev)
    red = torch.empty_like(ct)
    res = {"config": cfg, "bytes": n, "keys": int(m.n_keys), "docs": int(D)}
    m.release_scratch()
    res["ms_cover_mask"] = _median_ms(lambda: m.cover_batch_device(ct, ot, mask=mask), steps, warmup)
    res["scratch_cover"] = int(m.scratch_bytes())
    n_covered, n_hits = m.cover_batch_device(ct, ot, mask=mask)
    res["hits"], res["covered"] = n_hits, n_covered
    res["ms_cover_mask_redacted"] = _median_ms(lambda: m.cover_batch_device(ct, ot, mask=mask, redacted=red), steps, warmup)
    m.set_profiling(True)
    m.cover_batch_device(ct, ot, mask=mask, redacted=red)
    t = m.last_timing()
    res["cover_timing"] = {k: (round(v, 4) if isinstance(v, float) else v) for k, v in t.items()}
    m.set_profiling(False)
    m.release_scratch()
    out = torch.zeros((n_hits + 1, 3), dtype=torch.int32, device=dev)

    def without():
        m.match_batch_device(ct, ot, out, dho)
        docid = torch.searchsorted(dho, torch.arange(n_hits, device=dev), right=True) - 1
        base = ot[docid]
        diff = torch.zeros(n + 1, dtype=torch.int32, device=dev)
        one = torch.ones(n_hits, dtype=torch.int32, device=dev)
        diff.index_add_(0, base + out[:n_hits, 0], one)
        diff.index_add_(0, base + out[:n_hits, 1], -one)
        return torch.cumsum(diff[:n], 0, dtype=torch.int32) > 0

    try:
        res["ms_match_own_mask"] = _median_ms(without, steps, warmup)
        cov = without()
        shifts = torch.arange(32, device=dev, dtype=torch.int32)
        ok = int(cov.sum()) == n_covered
        step = 1 << 22
        for w0 in range(0, nw, step):
            w = mask[w0:min(w0 + step, nw)]
            b = ((w[:, None] >> shifts[None, :]) & 1).to(torch.bool).reshape(-1)
            lo, hi = w0 * 32, min((w0 + w.numel()) * 32, n)
            ok = ok and torch.equal(b[:hi - lo], cov[lo:hi]) and not bool(b[hi - lo:].any())
        res["mask_ok"] = bool(ok)
        del cov
    except torch.OutOfMemoryError:
        res["ms_match_own_mask"], res["mask_ok"] = None, None
    torch.cuda.empty_cache()
    m.release_scratch()
    res["ms_match"] = _median_ms(lambda: m.match_batch_device(ct, ot, out, dho), steps, warmup)
    res["scratch_match"] = int(m.scratch_bytes())
    res["hit_buffer_bytes"] = int(out.numel() * 4)
    del out
    torch.cuda.empty_cache()
    m.release_scratch()
    res["ms_count_no_keys"] = _median_ms(lambda: m.count_batch_device(ct, ot, None, dho), steps, warmup)
    res["scratch_count"] = int(m.scratch_bytes())
    res["ms_device_copy"] = _median_ms(lambda: red.copy_(ct), steps, warmup)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--configs", default="2,3,5")
    a = ap.parse_args()
    out = {"tool": "cover_bench", "steps": a.steps, "warmup": a.warmup, "results": []}
    for c in a.configs.split(","):
        out["results"].append(run_cfg(int(c), a.steps, a.warmup))
    out["ok"] = all(r["mask_ok"] is not False for r in out["results"])
    print(json.dumps(out))
    return 0 if out["ok"] else 1


if __name__ == "__main__":
    sys.exit(main())
