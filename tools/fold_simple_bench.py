"""What AHA_OPT_FOLD_SIMPLE costs, batch resident on the device (one MI355X).  Medians of --steps timed calls (after --warmup)
with [min, max], the sides of a comparison ALTERNATING call by call in one loop.

 pass:<kind>:<MiB>  the staged pass alone, kind = ascii (printable ASCII, no byte >= 0x80: the fast path) or cyrillic (every
                    other byte a lead byte).  The text is a view 5 bytes into a buffer, so every handle stages it: a plain
                    handle by a device-to-device copy, an ASCII-folded one by k_fold_copy (the yardstick), a simple-folded one
                    by k_fold2_copy + k_fold2_fix.  Each less the plain handle's aligned call = the pass; the key set is two
                    words, so the match beside it is as short as a match gets.
 cfg:<n>:<MiB>      a BASELINE config's key list (2: the keyword list of the prefix-filter engine) over its text, aligned:
                    FOLD_SIMPLE (staged copy, then the filter engine on it) against FOLD_ASCII (the filter folds in its loads)
                    and a plain handle; hit counts are compared (ASCII text: the three agree).
Prints one JSON line; --out writes it to a file too (after every case: a long run keeps what is measured so far).
Usage: python tools/fold_simple_bench.py [--steps 10] [--warmup 2] [--cases pass:ascii:1024,pass:cyrillic:1024,cfg:2:64,cfg:2:1024]
                                         [--out profiles/fold_simple_bench.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
DEV = "cuda:0"


def _alternate(fns, steps, warmup):
    import torch

    for _ in range(warmup):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    ts = {k: [] for k in fns}
    for _ in range(steps):
        for k, fn in fns.items():
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ts[k].append((time.perf_counter() - t0) * 1e3)
    return {k: {"median_ms": round(float(np.median(v)), 4), "min_ms": round(float(min(v)), 4), "max_ms": round(float(max(v)), 4)}
            for k, v in ts.items()}


def run_pass(kind, mib, steps, warmup):
    import torch
    from aha_amd import AC

    n = mib << 20
    g = torch.Generator(device=DEV)
    g.manual_seed(7)
    big = torch.zeros(n + 64, dtype=torch.uint8, device=DEV)
    view = big[5:5 + n]
    if kind == "ascii":
        view.copy_(torch.randint(32, 127, (n,), dtype=torch.uint8, device=DEV, generator=g))
        keys = ["error", "Warning"]
    else:  # U+0410 .. U+042F, the upper-case letters: 0xD0 and a continuation byte 0x90 .. 0xAF
        view[0::2] = 0xD0
        view[1::2] = torch.randint(0x90, 0xB0, (n // 2,), dtype=torch.uint8, device=DEV, generator=g)
        keys = ["привет", "МИР"]
    aligned = view.clone()
    assert aligned.data_ptr() % 16 == 0 and view.data_ptr() % 16 == 5
    n_docs = max(n >> 20, 1)
    ot = torch.arange(0, n + 1, n // n_docs, dtype=torch.int64, device=DEV)
    handles = {"plain": AC.compile(keys), "ascii": AC.compile(keys, fold_ascii=True), "simple": AC.compile(keys, fold_simple=True)}
    hits = {k: m.count_batch_device(view, ot, None, None) for k, m in handles.items()}
    cap = max(hits.values()) + 1
    out = torch.zeros((cap, 3), dtype=torch.int32, device=DEV)
    dho = torch.zeros(ot.numel(), dtype=torch.int64, device=DEV)
    spare = torch.empty_like(aligned)
    fns = {"plain_aligned": lambda: handles["plain"].match_batch_device(aligned, ot, out, dho),
           "plain_unaligned_copy": lambda: handles["plain"].match_batch_device(view, ot, out, dho),
           "ascii_unaligned_fold_copy": lambda: handles["ascii"].match_batch_device(view, ot, out, dho),
           "simple_unaligned_fold2_copy": lambda: handles["simple"].match_batch_device(view, ot, out, dho),
           "bare_device_copy": lambda: spare.copy_(view)}
    t = _alternate(fns, steps, warmup)
    base = t["plain_aligned"]["median_ms"]
    res = {"case": "pass:%s:%d" % (kind, mib), "bytes": n, "docs": n_docs, "hits": hits, "match": t,
           "copy_ms": round(t["plain_unaligned_copy"]["median_ms"] - base, 4),
           "fold_copy_ms": round(t["ascii_unaligned_fold_copy"]["median_ms"] - base, 4),
           "fold2_copy_ms": round(t["simple_unaligned_fold2_copy"]["median_ms"] - base, 4)}
    if kind == "ascii":  # (Cyrillic text: the three handles find different hits, so their matches differ beside the pass)
        res["equal"] = hits["ascii"] == hits["simple"]
    else:
        res["equal"] = hits["simple"] >= hits["ascii"] == hits["plain"]
        res["note"] = "the matches beside the passes differ: the simple-folded handle finds hits the others do not"
    return res


def run_cfg(cfg, mib, steps, warmup):
    import torch
    from aha_amd import AC, synth
    from tools.fold_bench import fold, mix_case

    blob, offs, nf = synth.keys(cfg)
    corpus, doc = synth.corpus(cfg, blob, offs, nf, n_bytes=mib << 20)
    mblob, mcorpus = mix_case(blob, 11), mix_case(corpus, 12)
    handles = {"plain_prefolded": AC.compile_packed(fold(mblob), offs), "fold_ascii": AC.compile_packed(mblob, offs, fold_ascii=True),
               "fold_simple": AC.compile_packed(mblob, offs, fold_simple=True)}
    ct = {"plain_prefolded": torch.from_numpy(fold(mcorpus)).to(DEV)}
    ct["fold_ascii"] = ct["fold_simple"] = torch.from_numpy(mcorpus).to(DEV)
    ot = torch.from_numpy(doc.astype(np.int64)).to(DEV)
    dho = torch.zeros(doc.size, dtype=torch.int64, device=DEV)
    hits = {k: m.count_batch_device(ct[k], ot, None, None) for k, m in handles.items()}
    out = torch.zeros((max(hits.values()) + 1, 3), dtype=torch.int32, device=DEV)
    fns = {k: (lambda k=k: handles[k].match_batch_device(ct[k], ot, out, dho)) for k in handles}
    t = _alternate(fns, steps, warmup)
    engines = {}
    for k, m in handles.items():
        m.set_profiling(True)
        m.match_batch_device(ct[k], ot, out, dho)
        engines[k] = m.last_timing()["engine"]
        m.set_profiling(False)
    return {"case": "cfg:%d:%d" % (cfg, mib), "bytes": int(corpus.size), "keys": int(handles["fold_simple"].n_keys), "hits": hits,
            "engines": engines, "match": t, "equal": len(set(hits.values())) == 1,
            "staging_ms": round(t["fold_simple"]["median_ms"] - t["fold_ascii"]["median_ms"], 4),
            "scratch": {k: int(m.scratch_bytes()) for k, m in handles.items()}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--cases", default="pass:ascii:1024,pass:cyrillic:1024,cfg:2:64,cfg:2:1024")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch

    if not torch.cuda.is_available():
        print("fold_simple_bench: no GPU (there is no CPU fallback for a measurement)", file=sys.stderr)
        return 2
    out = {"tool": "fold_simple_bench", "steps": a.steps, "warmup": a.warmup, "results": []}
    for c in a.cases.split(","):
        what, x, mib = c.split(":")
        out["results"].append(run_pass(x, int(mib), a.steps, a.warmup) if what == "pass" else run_cfg(int(x), int(mib), a.steps, a.warmup))
        torch.cuda.empty_cache()
        if a.out:
            with open(a.out, "w") as f:
                json.dump(out, f, indent=1)
    out["ok"] = all(r["equal"] for r in out["results"])
    print(json.dumps(out))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")
    return 0 if out["ok"] else 1


if __name__ == "__main__":
    sys.exit(main())
