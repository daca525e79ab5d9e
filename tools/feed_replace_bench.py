"""Feed replace against feed select of the same pieces and against plain replace of the same bytes as whole documents, batch
resident on the device (one MI355X).

For cfg 2 at 64 MiB and cfg 3 at 1 GiB (tools/feed_count_bench.py's sizes; --max-bytes caps them), in two shapes: the batch's
documents as the pieces of as many sequences, and the whole batch as one piece of one sequence.  Either is fed again on every
call, so that every piece after the first call has a context and open bytes.  The table replaces a third of the keys by a
string of their own length, deletes a third and doubles a third.  Records the median of --steps timed calls (after --warmup) of
  ms_replace       aha_ac_replace_batch_device of the same pieces as documents
  ms_feed_select   aha_feed_select_batch_device (hits, offsets, bases, hold)
  ms_feed_replace  aha_feed_replace_batch_device (bytes, offsets, bases, hold)
and the selected hits, the hits and the bytes of the results.  The expectation is ms_feed_select plus one read and one write of
the staged bytes plus replace's passes behind its select (DESIGN.md 4.10 "Feed replace"); no threshold is set.  Writes one
JSON document to --out (default profiles/feed_replace_bench.json) and prints it.
Usage: python tools/feed_replace_bench.py [--steps 10] [--warmup 3] [--configs 2,3] [--max-bytes N]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SIZES = {2: 64 << 20, 3: 1 << 30}


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


def _table(m, blob, offs):
    """per key: its bytes reversed, nothing, or the key twice"""
    repl = []
    for k in range(m.n_keys):
        key = bytes(blob[int(offs[k]):int(offs[k + 1])])
        repl.append((key[::-1], b"", key + key)[k % 3])
    return m.replacements(repl)


def run_shape(m, table, ct, ot, cfg, shape, steps, warmup):
    import torch
    from aha_amd import AhaError

    dev = "cuda:0"
    n = int(ct.numel())
    D = ot.numel() - 1
    W = max(int(m.info["max_key_len"]) - 1, 0)
    it = torch.arange(D, dtype=torch.int32, device=dev)
    off = torch.zeros(D + 1, dtype=torch.int64, device=dev)
    bases = torch.zeros(D, dtype=torch.int64, device=dev)
    hold = torch.zeros(D, dtype=torch.int32, device=dev)
    res = {"config": cfg, "shape": shape, "bytes": n, "pieces": int(D), "keys": int(m.n_keys), "W": W}
    # plain replace: a sizing call, then the timed one
    try:
        m.replace_batch_device(ct, ot, table, None)
        need = 0
    except AhaError as e:
        need = e.n_required
    out = torch.empty(need + 2 * D * W + 4096 + n // 8, dtype=torch.uint8, device=dev)  # (room for the feed's later calls too)
    res["out_bytes_replace"], res["selected_replace"], res["hits_replace"] = m.replace_batch_device(ct, ot, table, out, off)
    res["ms_replace"] = _median_ms(lambda: m.replace_batch_device(ct, ot, table, out, off), steps, warmup)
    m.release_scratch()
    # feed select: the selection is at most what plain select gives plus one open hit per piece
    hits = torch.empty((res["selected_replace"] + D * (W + 1) + 1024, 3), dtype=torch.int32, device=dev)
    fs = m.feed(D)
    fs.select_batch_device(ct, ot, it, hits, off, bases, hold)
    res["selected_feed"], res["hits_feed"] = fs.select_batch_device(ct, ot, it, hits, off, bases, hold)  # (with contexts)
    res["ms_feed_select"] = _median_ms(lambda: fs.select_batch_device(ct, ot, it, hits, off, bases, hold), steps, warmup)
    fs.close()
    del hits
    m.release_scratch()
    # feed replace
    fr = m.feed(D)
    fr.replace_batch_device(ct, ot, it, table, out, off, bases, hold)
    res["out_bytes_feed"], res["selected_feed_replace"], _ = fr.replace_batch_device(ct, ot, it, table, out, off, bases, hold)
    res["held_bytes"] = int(hold.sum())
    res["ms_feed_replace"] = _median_ms(lambda: fr.replace_batch_device(ct, ot, it, table, out, off, bases, hold), steps, warmup)
    fr.close()
    res["ms_feed_replace_minus_feed_select"] = round(res["ms_feed_replace"] - res["ms_feed_select"], 4)
    res["ratio_feed_replace_feed_select"] = round(res["ms_feed_replace"] / res["ms_feed_select"], 3)
    res["ratio_feed_replace_replace"] = round(res["ms_feed_replace"] / res["ms_replace"], 3)
    res["gb_per_s_feed_replace"] = round(n / res["ms_feed_replace"] / 1e6, 2)
    del out
    torch.cuda.empty_cache()
    m.release_scratch()
    return res


def run_cfg(cfg, steps, warmup, max_bytes):
    import torch
    from aha_amd import AC, synth

    blob, offs, nf = synth.keys(cfg)
    corpus, doc = synth.corpus(cfg, blob, offs, nf, n_bytes=min(SIZES[cfg], max_bytes))
    m = AC.compile_packed(blob, offs)
    table = _table(m, blob, offs)
    ct = torch.from_numpy(corpus).to("cuda:0")
    out = []
    for shape, d in (("many", doc), ("one", np.array([0, corpus.size], dtype=np.uint64))):
        ot = torch.from_numpy(d.astype(np.int64)).to("cuda:0")
        out.append(run_shape(m, table, ct, ot, cfg, shape, steps, warmup))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--configs", default="2,3")
    ap.add_argument("--max-bytes", type=int, default=1 << 62)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "feed_replace_bench.json"))
    a = ap.parse_args()
    res = {"tool": "feed_replace_bench", "steps": a.steps, "warmup": a.warmup, "results": []}
    for c in a.configs.split(","):
        res["results"] += run_cfg(int(c), a.steps, a.warmup, a.max_bytes)
    text = json.dumps(res)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text + "\n")
    print(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
