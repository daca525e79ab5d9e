"""Replace calls beside the calls they are to be held against, batch resident on the device (one MI355X).

For cfg 2 at 64 MiB, cfg 3 at 1 GiB and cfg 5 at 256 MiB, medians of --steps timed calls (after --warmup) with min and max:
(a) replace_batch_device with a table of same-length replacements and with one of mixed lengths (shorter, equal, longer, empty,
kept); (b) select_batch_device on the same batch; (c) cover_batch_device with a redacted copy (the fixed-length copy) and the
same call without it (the cover's traversal); (d) a plain device-to-device copy of N bytes on the same stream; (e) the scratch
of (a); (f) output bytes / input bytes and selected hits per KiB.  (a) - (b) is what replace adds to select: it is to be held
against (d) and against (c) less the cover's traversal.  The result of (a) is checked against aha_amd.ac.substitute over the
library's selection on a sample of documents.  The krp_* kernels' own times need a kernel trace in a run of its own
(rocprofv3 --kernel-trace --stats -- python tools/replace_bench.py --configs 2 --steps 3); they are not collected here.
Writes profiles/replace_bench.json and prints the same JSON line.
Usage: python tools/replace_bench.py [--steps 10] [--warmup 3] [--configs 2,3,5]"""
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
    return {"median": float(np.median(ts)), "min": float(min(ts)), "max": float(max(ts))}


def _tables(keys):
    same = [bytes(b ^ 0x20 if 0x41 <= (b & 0xDF) <= 0x5A else b for b in k)[::-1] for k in keys]  # a key's own length
    mixed = []
    for i, k in enumerate(keys):
        mixed.append((k[:len(k) // 2], k[::-1], k + b"/" + k, b"", None)[i % 5])
    return {"same": same, "mixed": mixed}


def run_cfg(cfg, steps, warmup):
    import torch
    from aha_amd import AC, AhaError, synth
    from aha_amd.ac import substitute

    blob, offs, nf = synth.keys(cfg)
    corpus, doc = synth.corpus(cfg, blob, offs, nf, n_bytes=SIZES[cfg])
    keys = [bytes(blob[offs[i]:offs[i + 1]]) for i in range(offs.size - 1)]
    m = AC.compile_packed(blob, offs)
    dev = "cuda:0"
    ct = torch.from_numpy(corpus).to(dev)
    ot = torch.from_numpy(doc.astype(np.int64)).to(dev)
    D, N = doc.size - 1, int(corpus.size)
    dso = torch.zeros(D + 1, dtype=torch.int64, device=dev)
    doo = torch.zeros(D + 1, dtype=torch.int64, device=dev)
    res = {"config": cfg, "bytes": N, "keys": len(keys), "docs": int(D), "ok": True}
    try:
        n_sel, n_hits = m.select_batch_device(ct, ot, None)
    except AhaError as e:
        n_sel, n_hits = e.n_required, None
    sel = torch.zeros((n_sel + 1, 3), dtype=torch.int32, device=dev)
    _, n_hits = m.select_batch_device(ct, ot, sel, dso)
    res["hits"], res["selected"], res["selected_per_kib"] = int(n_hits), int(n_sel), n_sel / (N / 1024)
    m.release_scratch()
    res["ms_select"] = _median_ms(lambda: m.select_batch_device(ct, ot, sel, dso), steps, warmup)
    sel_h, dso_h = sel[:n_sel].cpu().numpy(), dso.cpu().numpy()
    rng = np.random.default_rng(cfg)
    sample = sorted(set(rng.integers(0, D, size=min(D, 64)).tolist()))
    for name, repl in _tables(keys).items():
        table = m.replacements(repl)
        try:
            total = m.replace_batch_device(ct, ot, table, None)[0]
        except AhaError as e:
            total = e.n_required
        out = torch.zeros(total + 16, dtype=torch.uint8, device=dev)
        m.release_scratch()
        res["ms_replace_" + name] = _median_ms(lambda: m.replace_batch_device(ct, ot, table, out, doo), steps, warmup)
        res["scratch_replace_" + name] = int(m.scratch_bytes())
        res["out_over_in_" + name] = total / max(N, 1)
        m.set_profiling(True)
        m.replace_batch_device(ct, ot, table, out, doo)
        res["timing_" + name] = {k: (round(v, 4) if isinstance(v, float) else v) for k, v in m.last_timing().items()}
        m.set_profiling(False)
        doo_h = doo.cpu().numpy()
        for d in sample:  # the contract on a sample of documents, over the library's own selection
            text = corpus[int(doc[d]):int(doc[d + 1])].tobytes()
            rows = [tuple(r) for r in sel_h[int(dso_h[d]):int(dso_h[d + 1])].tolist()]
            want = substitute(text, np.array(rows, dtype=np.int64).reshape(-1, 3), repl, len(keys))
            got = out[int(doo_h[d]):int(doo_h[d + 1])].cpu().numpy().tobytes()
            res["ok"] = res["ok"] and got == want
        del out, table
        torch.cuda.empty_cache()
    m.release_scratch()
    red = torch.zeros(N, dtype=torch.uint8, device=dev)
    res["ms_redact"] = _median_ms(lambda: m.cover_batch_device(ct, ot, redacted=red), steps, warmup)
    mask = torch.zeros((N + 31) // 32, dtype=torch.int32, device=dev)
    res["ms_cover_mask_only"] = _median_ms(lambda: m.cover_batch_device(ct, ot, mask=mask), steps, warmup)
    res["ms_copy_d2d"] = _median_ms(lambda: red.copy_(ct), steps, warmup)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--configs", default="2,3,5")
    a = ap.parse_args()
    out = {"tool": "replace_bench", "steps": a.steps, "warmup": a.warmup, "results": []}
    for c in a.configs.split(","):
        out["results"].append(run_cfg(int(c), a.steps, a.warmup))
    out["ok"] = all(r["ok"] for r in out["results"])
    line = json.dumps(out)
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "replace_bench.json"), "w") as f:
        f.write(line + "\n")
    print(line)
    return 0 if out["ok"] else 1


if __name__ == "__main__":
    sys.exit(main())
