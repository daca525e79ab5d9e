"""Class counts against what a caller must do without them, batch resident on the device (one MI355X).

For cfg 2 at 64 MiB, cfg 3 at 1 GiB and cfg 5 at 256 MiB, each with C = 8 and C = 64 and the keys dealt to the classes
round-robin (key k in class k mod C), medians of --steps timed calls (after --warmup) with min and max:
(a) class_counts_batch_device; (b) doc_counts_batch_device (cap = pairs), then the caller's index_add_ of the pairs' counts into
a (D, C) tensor -- the document of a pair from a searchsorted in doc_pair_offsets, its class from the key; (c)
match_batch_device alone; (d) count_batch_device without key counts; (e) the scratch of (a).  The table of (a) is checked against
(b)'s in the same run.  What the call replaces is (a) against (b); what kcc_add and the clear cost is (a) - (c) - (d).
Prints one JSON line.
Usage: python tools/class_counts_bench.py [--steps 10] [--warmup 3] [--configs 2,3,5] [--classes 8,64]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SIZES = {2: 64 << 20, 3: 1 << 30, 5: 256 << 20}


def _timed(fn, steps, warmup):
    """-> {median, min, max} in ms"""
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
    return {"median": round(float(np.median(ts)), 4), "min": round(float(min(ts)), 4), "max": round(float(max(ts)), 4)}


def run_cfg(cfg, classes, steps, warmup):
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
    res = {"config": cfg, "bytes": int(corpus.size), "keys": int(K), "docs": int(D), "classes": []}
    try:
        n_pairs, n_hits = m.doc_counts_batch_device(ct, ot, None)
    except AhaError as e:
        n_pairs, n_hits = e.n_required, e.n_hits
    res["hits"], res["pairs"] = n_hits, n_pairs
    # (c) and (d): the same for every C
    out = torch.zeros((n_hits + 1, 3), dtype=torch.int32, device=dev)
    res["ms_match"] = _timed(lambda: m.match_batch_device(ct, ot, out, dho), steps, warmup)
    del out
    torch.cuda.empty_cache()
    m.release_scratch()
    res["ms_count_no_keys"] = _timed(lambda: m.count_batch_device(ct, ot, None, dho), steps, warmup)
    pairs = torch.zeros((n_pairs + 1, 2), dtype=torch.int32, device=dev)
    for C in classes:
        r = {"C": C}
        table = m.classes([k % C for k in range(K)], n_classes=C)
        rows = torch.zeros((D, C), dtype=torch.int32, device=dev)
        m.release_scratch()
        r["ms_class_counts"] = _timed(lambda: m.class_counts_batch_device(ct, ot, table, rows), steps, warmup)
        r["scratch_class_counts"] = int(m.scratch_bytes())
        m.set_profiling(True)
        m.class_counts_batch_device(ct, ot, table, rows)
        t = m.last_timing()
        r["class_counts_timing"] = {k: (round(v, 4) if isinstance(v, float) else v) for k, v in t.items()}
        m.set_profiling(False)
        m.release_scratch()
        key_class = (torch.arange(K, device=dev) % C).to(torch.int64)
        rows_b = torch.zeros((D, C), dtype=torch.int64, device=dev)

        def without():
            m.doc_counts_batch_device(ct, ot, pairs, dpo)
            docid = torch.searchsorted(dpo, torch.arange(n_pairs, device=dev), right=True) - 1
            rows_b.zero_()
            rows_b.view(-1).index_add_(0, docid * C + key_class[pairs[:n_pairs, 0].to(torch.int64)], pairs[:n_pairs, 1].to(torch.int64))

        r["ms_doc_counts_index_add"] = _timed(without, steps, warmup)
        without()
        r["rows_ok"] = bool(torch.equal(rows_b, rows.to(torch.int64)))
        r["ratio_b_over_a"] = round(r["ms_doc_counts_index_add"]["median"] / r["ms_class_counts"]["median"], 3)
        r["ms_a_minus_c_minus_d"] = round(r["ms_class_counts"]["median"] - res["ms_match"]["median"] - res["ms_count_no_keys"]["median"], 4)
        res["classes"].append(r)
        del rows, rows_b, table
        torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--configs", default="2,3,5")
    ap.add_argument("--classes", default="8,64")
    a = ap.parse_args()
    out = {"tool": "class_counts_bench", "steps": a.steps, "warmup": a.warmup, "results": []}
    classes = [int(c) for c in a.classes.split(",")]
    for c in a.configs.split(","):
        out["results"].append(run_cfg(int(c), classes, a.steps, a.warmup))
        print("cfg %s done" % c, file=sys.stderr, flush=True)
    out["ok"] = all(r["rows_ok"] for res in out["results"] for r in res["classes"])
    print(json.dumps(out))
    return 0 if out["ok"] else 1


if __name__ == "__main__":
    sys.exit(main())
