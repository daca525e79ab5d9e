"""Records and grep calls beside the calls they are to be held against, batch resident on the device (one MI355X).

For cfg 2 at 64 MiB and cfg 3 at 1 GiB, with a newline written over one byte in 100 on average, medians of --steps timed calls
(after --warmup) with min and max:
(a) records_device over the batch, against a plain device-to-device copy of N bytes on the same stream;
(b) grep_batch_device over those records -- with the copy, and the ids-only form -- against count_batch_device without key
    counts (hit offsets per record) on the same batch, at three kept fractions: near 1 % and near 50 % by a prefix of the key
    set (the prefix lengths are searched with the sizing call), near 99 % by inverting the first;
(c) the scratch of (a) and of (b), the records, the kept records and the dropped runs.
(b) - count is what grep adds to the count call; with the copy it is to be held against the copy of the kept bytes.
The result of (b) is checked against numpy over the count call's own hit offsets.
Writes profiles/grep_bench.json (--out) and prints the same JSON line.
Usage: python tools/grep_bench.py [--steps 10] [--warmup 3] [--configs 2,3] [--max-bytes N] [--out PATH]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SIZES = {2: 64 << 20, 3: 1 << 30}
TARGETS = (0.01, 0.5)


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
    return {"median": float(np.median(ts)), "min": float(min(ts)), "max": float(max(ts))}


def _runs(keep):
    """maximal runs of dropped records"""
    drop = ~keep
    return int(np.count_nonzero(drop & np.concatenate([[True], keep[:-1]]))) if keep.size else 0


def run_cfg(cfg, steps, warmup, max_bytes):
    import torch
    from aha_amd import AC, AhaError, synth

    dev = "cuda:0"
    n_bytes = min(SIZES[cfg], max_bytes) if max_bytes else SIZES[cfg]
    blob, offs, nf = synth.keys(cfg)
    corpus, doc = synth.corpus(cfg, blob, offs, nf, n_bytes=n_bytes)
    rng = np.random.default_rng(cfg)
    corpus = corpus.copy()
    corpus[rng.random(corpus.size) < 0.01] = 10
    K, N, D = offs.size - 1, int(corpus.size), doc.size - 1
    ct = torch.from_numpy(corpus).to(dev)
    ot = torch.from_numpy(doc.astype(np.int64)).to(dev)
    res = {"config": cfg, "bytes": N, "keys": int(K), "docs": int(D), "ok": True}

    # (a) records
    full = AC.compile_packed(blob, offs)
    try:
        R = full.records_device(ct, ot, None)
    except AhaError as e:  # the sizing call: the required count
        R = e.n_required
    rt = torch.zeros(R + 1, dtype=torch.int64, device=dev)
    drt = torch.zeros(D + 1, dtype=torch.int64, device=dev)
    full.release_scratch()
    res["records"] = int(R)
    print(f"cfg {cfg}: {N} bytes, {R} records", file=sys.stderr, flush=True)
    res["ms_records"] = _median_ms(lambda: full.records_device(ct, ot, rt, drt), steps, warmup)
    res["scratch_records"] = int(full.scratch_bytes())
    spare = torch.zeros(N, dtype=torch.uint8, device=dev)
    res["ms_copy_d2d"] = _median_ms(lambda: spare.copy_(ct), steps, warmup)
    res["records_over_copy"] = res["ms_records"]["median"] / res["ms_copy_d2d"]["median"]
    rec = rt.cpu().numpy().astype(np.uint64)
    want = np.concatenate([[0], np.union1d(np.nonzero(corpus == 10)[0] + 1, doc[1:][doc[1:] > 0].astype(np.int64))])
    res["ok"] = res["ok"] and np.array_equal(rec, want.astype(np.uint64))
    del full

    # (b) the key prefixes whose kept fractions lie nearest the targets
    def handle(k):
        return AC.compile_packed(blob[: int(offs[k])], offs[: k + 1])

    tried = {}
    k = 1
    while True:
        m = handle(k)
        tried[k] = m.grep_batch_device(ct, rt)[0] / max(R, 1)
        del m
        if k == K or tried[k] > 0.75:
            break
        k = min(K, k * 2)
    cases = []
    for target in TARGETS:
        kk = min(tried, key=lambda x: abs(tried[x] - target))
        cases.append((kk, False))
    cases.append((cases[0][0], True))
    res["prefix_search"] = {str(k): round(v, 5) for k, v in tried.items()}
    dho = torch.zeros(R + 1, dtype=torch.int64, device=dev)
    res["cases"] = []
    for kk, invert in cases:
        m = handle(kk)
        nk, nb, nh = m.grep_batch_device(ct, rt, invert=invert)
        kept = torch.zeros(nk + 1, dtype=torch.int64, device=dev)
        doo = torch.zeros(nk + 2, dtype=torch.int64, device=dev)
        out = torch.zeros(nb + 16, dtype=torch.uint8, device=dev)
        m.release_scratch()
        c = {"keys": int(kk), "invert": invert, "kept": int(nk), "kept_fraction": nk / max(R, 1), "out_bytes": int(nb),
             "hits": int(nh)}
        c["ms_count"] = _median_ms(lambda: m.count_batch_device(ct, rt, doc_hit_offsets=dho), steps, warmup)
        c["scratch_count"] = int(m.scratch_bytes())
        c["ms_grep"] = _median_ms(lambda: m.grep_batch_device(ct, rt, kept, doo, out, invert=invert, cap_docs=nk), steps, warmup)
        c["ms_grep_ids_only"] = _median_ms(lambda: m.grep_batch_device(ct, rt, kept, doo, None, invert=invert, cap_docs=nk), steps,
                                           warmup)
        c["scratch_grep"] = int(m.scratch_bytes())
        c["ms_copy_kept_d2d"] = _median_ms(lambda: spare[:nb].copy_(ct[:nb]), steps, warmup)
        c["grep_minus_count"] = c["ms_grep"]["median"] - c["ms_count"]["median"]
        c["grep_ids_only_minus_count"] = c["ms_grep_ids_only"]["median"] - c["ms_count"]["median"]
        m.set_profiling(True)
        m.grep_batch_device(ct, rt, kept, doo, out, invert=invert, cap_docs=nk)
        c["timing"] = {k: (round(v, 4) if isinstance(v, float) else v) for k, v in m.last_timing().items()}
        m.set_profiling(False)
        # the contract over the count call's own hit offsets
        keep = (np.diff(dho.cpu().numpy()) >= 1) != invert
        c["dropped_runs"] = _runs(keep)
        ids = np.nonzero(keep)[0]
        lens = (rec[1:] - rec[:-1]).astype(np.int64)[ids]
        want_doo = np.concatenate([[0], np.cumsum(lens)])
        ok = np.array_equal(kept[:nk].cpu().numpy(), ids) and np.array_equal(doo[:nk + 1].cpu().numpy(), want_doo)
        out_h = out[:nb].cpu().numpy()
        for i in rng.integers(0, max(nk, 1), size=min(nk, 256)).tolist():
            a, b = int(rec[ids[i]]), int(rec[ids[i] + 1])
            ok = ok and out_h[int(want_doo[i]):int(want_doo[i + 1])].tobytes() == corpus[a:b].tobytes()
        c["ok"] = bool(ok)
        res["ok"] = res["ok"] and c["ok"]
        res["cases"].append(c)
        print(f"cfg {cfg}: {kk} keys, invert {invert}: kept {c['kept_fraction']:.4f}", file=sys.stderr, flush=True)
        del m, kept, doo, out
        torch.cuda.empty_cache()
    res["ok"] = bool(res["ok"])
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--configs", default="2,3")
    ap.add_argument("--max-bytes", type=int, default=0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "grep_bench.json"))
    a = ap.parse_args()
    out = {"tool": "grep_bench", "steps": a.steps, "warmup": a.warmup, "results": []}
    for c in a.configs.split(","):
        out["results"].append(run_cfg(int(c), a.steps, a.warmup, a.max_bytes))
    out["ok"] = all(r["ok"] for r in out["results"])
    line = json.dumps(out)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")
    print(line)
    return 0 if out["ok"] else 1


if __name__ == "__main__":
    sys.exit(main())
