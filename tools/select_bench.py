"""Select calls beside the calls they are built from, batch resident on the device (one MI355X).

For cfg 2 at 64 MiB, cfg 3 at 1 GiB and cfg 5 at 256 MiB, medians of --steps timed calls (after --warmup):
(a) select_batch_device; (b) match_batch_device alone (cap = hits); (c) count_batch_device without key counts;
(d) doc_counts_batch_device; (e) the scratch of (a); (f) the selected hits beside all hits.  Also the split of (a) from
aha_ac_last_timing (ms_write = everything after the match) and the longest run of the batch -- a maximal stretch of covered bytes
inside one document, which ksl_walk walks with one lane -- from the cover mask.  The selection is checked on the device:
ascending and non-overlapping inside every document, every selected hit a hit of the match.
(b) and (c) are to be held against profiles/doc_counts_bench.json and profiles/cover_bench.json.
Writes profiles/select_bench.json and prints the same JSON line.
Usage: python tools/select_bench.py [--steps 10] [--warmup 3] [--configs 2,3,5]"""
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
    return float(np.median(ts)), float(min(ts)), float(max(ts))


def _longest_run(m, ct, ot, n_bytes, dev):
    """the longest stretch of covered bytes that holds no document start but its first byte"""
    import torch

    mask = torch.zeros((n_bytes + 31) // 32, dtype=torch.int32, device=dev)
    m.cover_batch_device(ct, ot, mask=mask)
    shifts = torch.arange(32, device=dev, dtype=torch.int32)
    covered = ((mask.unsqueeze(1) >> shifts) & 1).reshape(-1)[:n_bytes].to(torch.bool)
    del mask
    # a run ends in front of every uncovered byte and every document start
    cut = ~covered
    cut[ot[:-1][ot[:-1] < n_bytes]] = True
    cuts = torch.nonzero(cut).reshape(-1)
    del cut
    cuts = torch.cat([cuts, torch.tensor([n_bytes], device=dev)])
    span = cuts[1:] - cuts[:-1] - (~covered[cuts[:-1]]).to(torch.int64)  # (an uncovered cut is not part of the run behind it)
    return int(span.max()) if span.numel() else 0


def run_cfg(cfg, steps, warmup):
    import torch
    from aha_amd import AC, AhaError, synth

    blob, offs, nf = synth.keys(cfg)
    corpus, doc = synth.corpus(cfg, blob, offs, nf, n_bytes=SIZES[cfg])
    m = AC.compile_packed(blob, offs)
    dev = "cuda:0"
    ct = torch.from_numpy(corpus).to(dev)
    ot = torch.from_numpy(doc.astype(np.int64)).to(dev)
    D = doc.size - 1
    dho = torch.zeros(D + 1, dtype=torch.int64, device=dev)
    dso = torch.zeros(D + 1, dtype=torch.int64, device=dev)
    res = {"config": cfg, "bytes": int(corpus.size), "keys": int(m.n_keys), "docs": int(D)}
    try:
        n_sel, n_hits = m.select_batch_device(ct, ot, None)
    except AhaError as e:
        n_sel = e.n_required
        n_hits = m.count_batch_device(ct, ot, None, dho)
    res["hits"], res["selected"] = int(n_hits), int(n_sel)
    sel = torch.zeros((n_sel + 1, 3), dtype=torch.int32, device=dev)
    m.release_scratch()
    res["ms_select"], res["ms_select_min"], res["ms_select_max"] = _median_ms(lambda: m.select_batch_device(ct, ot, sel, dso), steps, warmup)
    res["scratch_select"] = int(m.scratch_bytes())
    m.set_profiling(True)
    m.select_batch_device(ct, ot, sel, dso)
    t = m.last_timing()
    res["select_timing"] = {k: (round(v, 4) if isinstance(v, float) else v) for k, v in t.items()}
    m.set_profiling(False)
    m.release_scratch()
    # the selection against the match of the same batch, on the device
    out = torch.zeros((n_hits + 1, 3), dtype=torch.int32, device=dev)
    m.match_batch_device(ct, ot, out, dho)
    s64 = sel[:n_sel].to(torch.int64)
    sdoc = torch.searchsorted(dso, torch.arange(n_sel, device=dev), right=True) - 1
    ok = bool(int(dso[0]) == 0 and int(dso[-1]) == n_sel and (s64[:, 1] > s64[:, 0]).all())
    ok = ok and bool(((s64[1:, 0] >= s64[:-1, 1]) | (sdoc[1:] != sdoc[:-1])).all())
    h64 = out[:n_hits].to(torch.int64)
    hdoc = torch.searchsorted(dho, torch.arange(n_hits, device=dev), right=True) - 1
    # (position in the batch, length) identifies a hit: keys are distinct and shorter than 2^20 bytes
    hkey = torch.sort(((ot[hdoc] + h64[:, 0]) << 20) | (h64[:, 1] - h64[:, 0]))[0] if n_hits else hdoc
    skey = ((ot[sdoc] + s64[:, 0]) << 20) | (s64[:, 1] - s64[:, 0])
    if n_sel:
        at = torch.searchsorted(hkey, skey).clamp(max=max(n_hits - 1, 0))
        ok = ok and bool((hkey[at] == skey).all())
    res["selection_ok"] = ok
    del h64, hdoc, hkey, skey, s64, sdoc
    torch.cuda.empty_cache()
    res["ms_match"], res["ms_match_min"], res["ms_match_max"] = _median_ms(lambda: m.match_batch_device(ct, ot, out, dho), steps, warmup)
    del out
    torch.cuda.empty_cache()
    m.release_scratch()
    res["ms_count_no_keys"], res["ms_count_min"], res["ms_count_max"] = _median_ms(lambda: m.count_batch_device(ct, ot, None, dho), steps, warmup)
    try:
        n_pairs, _ = m.doc_counts_batch_device(ct, ot, None)
    except AhaError as e:
        n_pairs = e.n_required
    pairs = torch.zeros((n_pairs + 1, 2), dtype=torch.int32, device=dev)
    res["ms_doc_counts"], _, _ = _median_ms(lambda: m.doc_counts_batch_device(ct, ot, pairs, dso), steps, warmup)
    del pairs
    m.release_scratch()
    torch.cuda.empty_cache()
    res["longest_run_bytes"] = _longest_run(m, ct, ot, int(corpus.size), dev)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--configs", default="2,3,5")
    a = ap.parse_args()
    out = {"tool": "select_bench", "steps": a.steps, "warmup": a.warmup, "results": []}
    for c in a.configs.split(","):
        out["results"].append(run_cfg(int(c), a.steps, a.warmup))
    out["ok"] = all(r["selection_ok"] for r in out["results"])
    line = json.dumps(out)
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "select_bench.json"), "w") as f:
        f.write(line + "\n")
    print(line)
    return 0 if out["ok"] else 1


if __name__ == "__main__":
    sys.exit(main())
