"""ASCII case-insensitive handles (AHA_OPT_FOLD_ASCII) against the paths they stand beside, batch resident on the device
(one MI355X).  Keys and text are the BASELINE configs' with each ASCII letter upper-cased with probability 1/2 (fixed seeds).

Per config and size, --steps timed calls each (after --warmup), the two sides of a comparison ALTERNATING call by call in one
loop, medians and the [min, max] of the steps:
 1. folded handle on the mixed-case text  vs  plain handle on the pre-folded text (a path the flag does not touch); the spread
    of the baseline itself is its [min, max]; with profiling on, the filter kernel's time (ms_count) of both on cfg 2.
 2. the caller's alternative on cfg 2: a torch lower-casing of the batch on the device + the plain match, vs one folded call.
 3. cfg 3 / cfg 5 (staged engines): the same pair as 1; the difference is the fold copy.
 4. the fold copy against the device-to-device copy it replaces for unaligned views: plain and folded handles on a view 5
    bytes into a buffer (copy, fold copy), each less the plain aligned call; and a bare device copy of the same bytes.
Results are checked against each other in the same run (hits equal).  Prints one JSON line; --out writes it to a file too.
Usage: python tools/fold_bench.py [--steps 20] [--warmup 3] [--cases 2:64,2:1024,3:1024,5:1024] [--out profiles/fold_bench.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def fold(a):
    return np.where((a >= 65) & (a <= 90), a + 32, a).astype(np.uint8)


def mix_case(a, seed):
    a = np.array(a, dtype=np.uint8, copy=True)
    rng = np.random.default_rng(seed)
    step = 64 << 20
    for lo in range(0, a.size, step):
        v = a[lo:lo + step]
        flip = rng.integers(0, 2, v.size, dtype=np.uint8).astype(bool)
        v[(v >= 97) & (v <= 122) & flip] -= 32
    return a


def _alternate(fns, steps, warmup):
    """{name: {median, min, max}} of callables timed in turn, one call of each per round"""
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


def run_case(cfg, mib, steps, warmup):
    import torch
    from aha_amd import AC, synth

    dev = "cuda:0"
    n_bytes = mib << 20
    blob, offs, nf = synth.keys(cfg)
    corpus, doc = synth.corpus(cfg, blob, offs, nf, n_bytes=n_bytes)
    mblob, mcorpus = mix_case(blob, 11), mix_case(corpus, 12)
    plain = AC.compile_packed(fold(mblob), offs)
    folded = AC.compile_packed(mblob, offs, fold_ascii=True)
    n = int(corpus.size)
    big = torch.zeros(n + 64, dtype=torch.uint8, device=dev)
    ct_mixed = torch.from_numpy(mcorpus).to(dev)
    ct_folded = torch.from_numpy(fold(mcorpus)).to(dev)
    ot = torch.from_numpy(doc.astype(np.int64)).to(dev)
    dho = torch.zeros(doc.size, dtype=torch.int64, device=dev)
    res = {"config": cfg, "bytes": n, "keys": int(plain.n_keys), "docs": int(doc.size - 1)}
    n_hits = plain.count_batch_device(ct_folded, ot, None, None)
    res["hits"] = n_hits
    out_p = torch.zeros((n_hits + 1, 3), dtype=torch.int32, device=dev)
    out_f = torch.zeros((n_hits + 1, 3), dtype=torch.int32, device=dev)
    res["equal"] = (plain.match_batch_device(ct_folded, ot, out_p, dho) == folded.match_batch_device(ct_mixed, ot, out_f, dho) == n_hits
                    and bool(torch.equal(out_p, out_f)))

    def lower_then_match():
        up = (ct_mixed >= 65) & (ct_mixed <= 90)
        low = torch.where(up, ct_mixed + 32, ct_mixed)
        return plain.match_batch_device(low, ot, out_p, dho)

    fns = {"plain_prefolded": lambda: plain.match_batch_device(ct_folded, ot, out_p, dho),
           "folded": lambda: folded.match_batch_device(ct_mixed, ot, out_f, dho)}
    if cfg == 2:
        fns["plain_after_torch_lower"] = lower_then_match
    res["match"] = _alternate(fns, steps, warmup)
    res["scratch_plain"], res["scratch_folded"] = int(plain.scratch_bytes()), int(folded.scratch_bytes())
    # the kernels' own times of one profiled call each (cfg 2: ms_count = kf_filter)
    for name, m, t in (("plain", plain, ct_folded), ("folded", folded, ct_mixed)):
        m.set_profiling(True)
        ks = []
        for _ in range(5):
            m.match_batch_device(t, ot, out_p, dho)
            ks.append(m.last_timing())
        m.set_profiling(False)
        res["timing_" + name] = {"engine": ks[-1]["engine"], "repeats": ks[-1]["repeats"],
                                 "ms_count_median": round(float(np.median([k["ms_count"] for k in ks])), 4),
                                 "ms_total_median": round(float(np.median([k["ms_total"] for k in ks])), 4)}
    # unaligned views: the copy of a plain handle, the fold copy of a folded one
    v_folded, v_mixed = big[5:5 + n], None
    v_folded.copy_(ct_folded)
    big2 = torch.zeros(n + 64, dtype=torch.uint8, device=dev)
    v_mixed = big2[5:5 + n]
    v_mixed.copy_(ct_mixed)
    spare = torch.empty_like(ct_mixed)
    res["unaligned"] = _alternate({"plain_aligned": lambda: plain.match_batch_device(ct_folded, ot, out_p, dho),
                                   "plain_unaligned_copy": lambda: plain.match_batch_device(v_folded, ot, out_p, dho),
                                   "folded_unaligned_fold_copy": lambda: folded.match_batch_device(v_mixed, ot, out_f, dho),
                                   "bare_device_copy": lambda: spare.copy_(ct_mixed)}, steps, warmup)
    u = res["unaligned"]
    res["copy_ms"] = round(u["plain_unaligned_copy"]["median_ms"] - u["plain_aligned"]["median_ms"], 4)
    res["fold_copy_ms"] = round(u["folded_unaligned_fold_copy"]["median_ms"] - u["plain_aligned"]["median_ms"], 4)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--cases", default="2:64,2:1024,3:1024,5:1024")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch

    if not torch.cuda.is_available():
        print("fold_bench: no GPU (there is no CPU fallback for a measurement)", file=sys.stderr)
        return 2
    out = {"tool": "fold_bench", "steps": a.steps, "warmup": a.warmup, "results": []}
    for c in a.cases.split(","):
        cfg, mib = c.split(":")
        out["results"].append(run_case(int(cfg), int(mib), a.steps, a.warmup))
        torch.cuda.empty_cache()
        if a.out:  # (a long run: what is measured so far is kept)
            with open(a.out, "w") as f:
                json.dump(out, f, indent=1)
    out["ok"] = all(r["equal"] for r in out["results"])
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")
    return 0 if out["ok"] else 1


if __name__ == "__main__":
    sys.exit(main())
