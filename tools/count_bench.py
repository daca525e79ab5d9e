"""Count calls against match calls on the BASELINE shapes, batch resident on the device (one MI355X).

For cfg 2 at 64 MiB, cfg 3 at 1 GiB and cfg 5 at 256 MiB: the median of --steps timed calls (after --warmup) of
match_batch_device (cap = hits), count_batch_device with key counts and count_batch_device without them; the handle's
scratch bytes after each; and, in the same run, the key counts against a bincount of the match call's hits.  For
--sep-configs the same three calls with a separator filter (a space separates).  Prints one JSON line.  Usage: python tools/count_bench.py [--steps 10] [--warmup 3] [--configs 2,3,5]"""
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


def run_cfg(cfg, steps, warmup, sep=False):
    import torch
    from aha_amd import AC, synth

    blob, offs, nf = synth.keys(cfg)
    corpus, doc = synth.corpus(cfg, blob, offs, nf, n_bytes=SIZES[cfg])
    m = AC.compile_packed(blob, offs)
    K = m.n_keys
    dev = "cuda:0"
    ct = torch.from_numpy(corpus).to(dev)
    ot = torch.from_numpy(doc.astype(np.int64)).to(dev)
    D = doc.size - 1
    dho = torch.zeros(D + 1, dtype=torch.int64, device=dev)
    kc = torch.zeros(K, dtype=torch.int64, device=dev)
    res = {"config": cfg, "bytes": int(corpus.size), "keys": int(K), "docs": int(D)}
    # counts first: the hit total sizes the match call's buffer
    m.set_profiling(True)
    n = m.count_batch_device(ct, ot, kc, dho)
    res["hits"] = n
    res["engine_count"] = m.last_timing()["engine"]
    m.set_profiling(False)
    out = torch.zeros((n + 1, 3), dtype=torch.int32, device=dev)
    m.release_scratch()
    res["ms_match"] = _median_ms(lambda: m.match_batch_device(ct, ot, out, dho), steps, warmup)
    res["scratch_match"] = int(m.scratch_bytes())
    m.set_profiling(True)
    m.match_batch_device(ct, ot, out, dho)
    res["engine_match"] = m.last_timing()["engine"]
    m.set_profiling(False)
    mdho = dho.clone()
    # the check: counts = bincount of the match call's values, offsets equal
    vals = out[:n, 2].to(torch.int64)
    want = torch.bincount(vals, minlength=K)
    del out, vals
    torch.cuda.empty_cache()
    m.release_scratch()
    res["ms_count"] = _median_ms(lambda: m.count_batch_device(ct, ot, kc, dho), steps, warmup)
    res["scratch_count"] = int(m.scratch_bytes())
    res["counts_ok"] = bool(torch.equal(kc, want)) and bool(torch.equal(dho, mdho))
    m.release_scratch()
    res["ms_count_no_keys"] = _median_ms(lambda: m.count_batch_device(ct, ot, None, dho), steps, warmup)
    res["scratch_count_no_keys"] = int(m.scratch_bytes())
    res["offsets_ok"] = bool(torch.equal(dho, mdho))
    m.set_profiling(True)
    m.count_batch_device(ct, ot, kc, dho)
    t = m.last_timing()
    res["count_timing"] = {k: (round(v, 4) if isinstance(v, float) else v) for k, v in t.items()}
    m.set_profiling(False)
    res["speedup"] = round(res["ms_match"] / res["ms_count"], 3) if res["ms_count"] else None
    m.release_scratch()
    if sep:
        # separator filter (a space separates): the match takes the slab pipeline, the count the two-pass engine's counting form
        from aha_amd import BitArray

        sp = BitArray(33)
        for i in range(32):
            sp[i] = True
        ns = m.count_batch_device(ct, ot, kc, dho, sep=sp)
        sdho = dho.clone()
        skc = kc.clone()
        out = torch.zeros((ns + 1, 3), dtype=torch.int32, device=dev)
        res["sep_hits"] = ns
        res["ms_match_sep"] = _median_ms(lambda: m.match_batch_device(ct, ot, out, dho, sep=sp), steps, warmup)
        want = torch.bincount(out[:ns, 2].to(torch.int64), minlength=K)
        res["sep_counts_ok"] = bool(torch.equal(skc, want)) and bool(torch.equal(sdho, dho))
        del out
        torch.cuda.empty_cache()
        res["ms_count_sep"] = _median_ms(lambda: m.count_batch_device(ct, ot, kc, dho, sep=sp), steps, warmup)
        res["ms_count_sep_no_keys"] = _median_ms(lambda: m.count_batch_device(ct, ot, None, dho, sep=sp), steps, warmup)
        m.release_scratch()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--configs", default="2,3,5")
    ap.add_argument("--sep-configs", default="2,3", help="configs also measured with a separator filter")
    a = ap.parse_args()
    out = {"tool": "count_bench", "steps": a.steps, "warmup": a.warmup, "results": []}
    for c in a.configs.split(","):
        out["results"].append(run_cfg(int(c), a.steps, a.warmup, sep=c in a.sep_configs.split(",")))
    out["ok"] = all(r["counts_ok"] and r["offsets_ok"] and r.get("sep_counts_ok", True) for r in out["results"])
    print(json.dumps(out))
    return 0 if out["ok"] else 1


if __name__ == "__main__":
    sys.exit(main())
