"""What AHA_OPT_FOLD_BMP costs, batch resident on the device (one MI355X).  Medians of --steps timed calls (after --warmup) with
[min, max], the sides of a comparison ALTERNATING call by call in one loop.  The yardstick is the simple-folded handle's
staged pass (k_fold2_copy + k_fold2_fix), on the same text in the same process.

 pass:<kind>:<MiB>  the staged pass alone.  kind = ascii (printable ASCII: the fast path), cyrillic (every other byte a lead
                    byte), chinese (the text of BASELINE config 3: three-byte characters, none of which moves) or dense
                    (upper-case full-width letters U+FF21 .. U+FF3A: every character moves).  The text is a view 5 bytes into a
                    buffer, so every handle stages it: a plain handle by a device-to-device copy, a simple-folded one by
                    k_fold2_copy + k_fold2_fix (the yardstick), a BMP-folded one by k_fold3_copy + k_fold3_fix, as it is
                    by default and (AHA_FOLD3_LIVE_TEST=1, read at every launch) with the live-lead test.  Each less the plain handle's
                    aligned call = the pass; the key set is two words, so the match beside it is as short as a match gets.
                    Hits: the BMP-folded handle's equal a plain handle's over the text folded beforehand (dense: on the
                    device, by the rule for that range of characters; elsewhere fold3 = fold2 and the yardstick's hits).
 cfg:<n>:<MiB>      a BASELINE config's key list (2: the keyword list of the prefix-filter engine) over its text in mixed case,
                    aligned: FOLD_BMP against FOLD_SIMPLE (both stage, then the filter engine runs on the copy); hits equal.
Prints one JSON line; --out writes it to a file too (after every case: a long run keeps what is measured so far).
Usage: python tools/fold_bmp_bench.py [--steps 10] [--warmup 2] [--out profiles/fold_bmp_bench.json]
                                      [--cases pass:ascii:1024,pass:cyrillic:1024,pass:chinese:1024,pass:dense:1024,cfg:2:64,cfg:2:1024]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
DEV = "cuda:0"
LIVE_LEADS = (0xE1, 0xE2, 0xEA, 0xEF)


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


def _live_test(on):
    os.environ["AHA_FOLD3_LIVE_TEST"] = "1" if on else "0"


def run_pass(kind, mib, steps, warmup):
    import torch
    from aha_amd import AC, synth

    n = mib << 20
    g = torch.Generator(device=DEV)
    g.manual_seed(7)
    big = torch.zeros(n + 64, dtype=torch.uint8, device=DEV)
    view = big[5:5 + n]
    prefolded = None  # (the text folded beforehand, where fold3 is not fold2)
    if kind == "ascii":
        view.copy_(torch.randint(32, 127, (n,), dtype=torch.uint8, device=DEV, generator=g))
        keys = ["error", "Warning"]
    elif kind == "cyrillic":  # U+0410 .. U+042F, the upper-case letters: 0xD0 and a continuation byte 0x90 .. 0xAF
        view[0::2] = 0xD0
        view[1::2] = torch.randint(0x90, 0xB0, (n // 2,), dtype=torch.uint8, device=DEV, generator=g)
        keys = ["привет", "МИР"]
    elif kind == "chinese":
        blob, offs, nf = synth.keys(3)
        corpus, _ = synth.corpus(3, blob, offs, nf, n_bytes=n)
        view[:min(n, corpus.size)].copy_(torch.from_numpy(corpus[:n]).to(DEV))  # (a shorter corpus leaves NUL bytes behind it)
        keys = ["我是", "中国"]
    else:  # dense: U+FF21 .. U+FF3A, EF BC A1 .. EF BC BA; folded EF BD 81 .. EF BD 9A
        m = n // 3
        view[0:3 * m:3] = 0xEF
        view[1:3 * m:3] = 0xBC
        view[2:3 * m:3] = torch.randint(0xA1, 0xBB, (m,), dtype=torch.uint8, device=DEV, generator=g)
        view[3 * m:] = 0x20
        keys = ["ｅｒｒｏｒ", "ＷＡＲＮ"]
        prefolded = view.clone()
        prefolded[1:3 * m:3] = 0xBD
        prefolded[2:3 * m:3] -= 0x20
    aligned = view.clone()
    assert aligned.data_ptr() % 16 == 0 and view.data_ptr() % 16 == 5
    live = int(sum(int((view == b).sum()) for b in LIVE_LEADS))
    n_docs = max(n >> 20, 1)
    ot = torch.arange(0, n + 1, n // n_docs, dtype=torch.int64, device=DEV)
    handles = {"plain": AC.compile(keys), "simple": AC.compile(keys, fold_simple=True), "bmp": AC.compile(keys, fold_bmp=True)}
    _live_test(False)
    hits = {k: m.count_batch_device(view, ot, None, None) for k, m in handles.items()}
    _live_test(True)
    hits["bmp_live_test"] = handles["bmp"].count_batch_device(view, ot, None, None)
    if prefolded is not None:
        lowered = AC.compile([k.lower() for k in keys])
        hits["plain_on_prefolded"] = lowered.count_batch_device(prefolded, ot, None, None)
        equal = hits["bmp"] == hits["bmp_live_test"] == hits["plain_on_prefolded"] > hits["simple"]
    else:
        equal = hits["bmp"] == hits["bmp_live_test"] == hits["simple"]
    del prefolded
    cap = max(hits.values()) + 1
    out = torch.zeros((cap, 3), dtype=torch.int32, device=DEV)
    dho = torch.zeros(ot.numel(), dtype=torch.int64, device=DEV)
    spare = torch.empty_like(aligned)

    def bmp(on):
        _live_test(on)
        handles["bmp"].match_batch_device(view, ot, out, dho)

    fns = {"plain_aligned": lambda: handles["plain"].match_batch_device(aligned, ot, out, dho),
           "plain_unaligned_copy": lambda: handles["plain"].match_batch_device(view, ot, out, dho),
           "simple_unaligned_fold2_copy": lambda: handles["simple"].match_batch_device(view, ot, out, dho),
           "bmp_unaligned_fold3_copy": lambda: bmp(False),
           "bmp_unaligned_fold3_copy_live_test": lambda: bmp(True),
           "bare_device_copy": lambda: spare.copy_(view)}
    t = _alternate(fns, steps, warmup)
    _live_test(False)
    base = t["plain_aligned"]["median_ms"]
    res = {"case": "pass:%s:%d" % (kind, mib), "bytes": n, "docs": n_docs, "live_lead_bytes": live, "hits": hits, "match": t,
           "copy_ms": round(t["plain_unaligned_copy"]["median_ms"] - base, 4),
           "fold2_copy_ms": round(t["simple_unaligned_fold2_copy"]["median_ms"] - base, 4),
           "fold3_copy_ms": round(t["bmp_unaligned_fold3_copy"]["median_ms"] - base, 4),
           "fold3_copy_live_test_ms": round(t["bmp_unaligned_fold3_copy_live_test"]["median_ms"] - base, 4),
           "equal": bool(equal)}
    if kind == "dense":
        res["note"] = "the matches beside the passes differ: the BMP-folded handle finds hits the others do not"
    return res


def run_cfg(cfg, mib, steps, warmup):
    import torch
    from aha_amd import AC, synth
    from tools.fold_bench import mix_case

    blob, offs, nf = synth.keys(cfg)
    corpus, doc = synth.corpus(cfg, blob, offs, nf, n_bytes=mib << 20)
    mblob, mcorpus = mix_case(blob, 11), mix_case(corpus, 12)
    handles = {"fold_simple": AC.compile_packed(mblob, offs, fold_simple=True), "fold_bmp": AC.compile_packed(mblob, offs, fold_bmp=True)}
    ct = torch.from_numpy(mcorpus).to(DEV)
    ot = torch.from_numpy(doc.astype(np.int64)).to(DEV)
    dho = torch.zeros(doc.size, dtype=torch.int64, device=DEV)
    _live_test(False)
    hits = {k: m.count_batch_device(ct, ot, None, None) for k, m in handles.items()}
    out = torch.zeros((max(hits.values()) + 1, 3), dtype=torch.int32, device=DEV)
    fns = {k: (lambda k=k: handles[k].match_batch_device(ct, ot, out, dho)) for k in handles}
    t = _alternate(fns, steps, warmup)
    engines = {}
    for k, m in handles.items():
        m.set_profiling(True)
        m.match_batch_device(ct, ot, out, dho)
        engines[k] = m.last_timing()["engine"]
        m.set_profiling(False)
    return {"case": "cfg:%d:%d" % (cfg, mib), "bytes": int(corpus.size), "keys": int(handles["fold_bmp"].n_keys), "hits": hits,
            "engines": engines, "match": t, "equal": len(set(hits.values())) == 1,
            "bmp_over_simple_ms": round(t["fold_bmp"]["median_ms"] - t["fold_simple"]["median_ms"], 4),
            "scratch": {k: int(m.scratch_bytes()) for k, m in handles.items()}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--cases", default="pass:ascii:1024,pass:cyrillic:1024,pass:chinese:1024,pass:dense:1024,cfg:2:64,cfg:2:1024")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch

    if not torch.cuda.is_available():
        print("fold_bmp_bench: no GPU (there is no CPU fallback for a measurement)", file=sys.stderr)
        return 2
    out = {"tool": "fold_bmp_bench", "steps": a.steps, "warmup": a.warmup, "results": []}
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
