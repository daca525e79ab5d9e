"""Token calls beside the select call they ride on, batch resident on the device (one MI355X).

For cfg 3 at 256 MiB (and any of --configs at --bytes), medians of --steps timed calls (after --warmup):
(a) select_batch_device, flag-less; (b) tokens_batch_device, a token per character between the hits; (c) the same with
gap_runs.  Of each also the split from aha_ac_last_timing (ms_write = everything after the match), so that (b) - (a) in
ms_write is what the token passes cost: S and T over the positions, the rank of T and 12 bytes written per token.  Beside them
(d) a device-to-device copy of as many bytes as (b) writes, the ceiling of any kernel that writes them.  The tokens are checked
on the device: every document partitioned, the tokens with a key exactly the selection.
--select-only times (a) alone: for a library without the token bits (the parent's build, chosen by AHA_HIP_LIB).
Writes profiles/tokens_bench.json (or --out) and prints the same JSON line.
Usage: python tools/tokens_bench.py [--steps 10] [--warmup 3] [--configs 3] [--bytes N] [--select-only] [--out FILE]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SIZES = {2: 64 << 20, 3: 256 << 20, 5: 256 << 20}


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


def _timed(m, fn, steps, warmup):
    """median / min / max of the call's wall time, and of ms_write over as many profiled calls"""
    ms = _median_ms(fn, steps, warmup)
    m.set_profiling(True)
    writes, t = [], None
    for _ in range(steps):
        fn()
        t = m.last_timing()
        writes.append(t["ms_write"])
    m.set_profiling(False)
    return {"ms": round(ms[0], 4), "ms_min": round(ms[1], 4), "ms_max": round(ms[2], 4),
            "ms_write": round(float(np.median(writes)), 4), "ms_write_min": round(min(writes), 4),
            "ms_write_max": round(max(writes), 4), "engine": t["engine"], "repeats": t["repeats"]}


def _sized(call):
    from aha_amd import AhaError

    try:
        return call()[0]
    except AhaError as e:
        return e.n_required


def _tokens_ok(tok, dto, sel, dso, ot, n_tok):
    """every document partitioned; the tokens with a key are the selection, row for row"""
    import torch

    t64 = tok[:n_tok].to(torch.int64)
    tdoc = torch.searchsorted(dto, torch.arange(n_tok, device=tok.device), right=True) - 1
    lens = ot[1:] - ot[:-1]
    first = torch.ones(n_tok, dtype=torch.bool, device=tok.device)
    first[1:] = tdoc[1:] != tdoc[:-1]
    last = torch.ones(n_tok, dtype=torch.bool, device=tok.device)
    last[:-1] = first[1:]
    ok = bool((t64[:, 1] > t64[:, 0]).all()) and bool((t64[first, 0] == 0).all()) and bool((t64[last, 1] == lens[tdoc[last]]).all())
    ok = ok and bool((t64[1:, 0][~first[1:]] == t64[:-1, 1][~first[1:]]).all())
    ok = ok and bool(((dto[1:] - dto[:-1] > 0) == (lens > 0)).all())
    keyed = tok[:n_tok][tok[:n_tok, 2] >= 0]
    return ok and keyed.shape[0] == sel.shape[0] and bool((keyed == sel).all()) and int(dso[-1]) == sel.shape[0]


def run_cfg(cfg, n_bytes, steps, warmup, select_only):
    import torch
    from aha_amd import AC, synth

    blob, offs, nf = synth.keys(cfg)
    corpus, doc = synth.corpus(cfg, blob, offs, nf, n_bytes=n_bytes)
    m = AC.compile_packed(blob, offs)
    dev = "cuda:0"
    ct = torch.from_numpy(corpus).to(dev)
    ot = torch.from_numpy(doc.astype(np.int64)).to(dev)
    D = doc.size - 1
    dso = torch.zeros(D + 1, dtype=torch.int64, device=dev)
    dto = torch.zeros(D + 1, dtype=torch.int64, device=dev)
    res = {"config": cfg, "bytes": int(corpus.size), "keys": int(m.n_keys), "docs": int(D)}
    n_sel = _sized(lambda: m.select_batch_device(ct, ot, None))
    sel = torch.zeros((n_sel + 1, 3), dtype=torch.int32, device=dev)
    res["selected"] = int(n_sel)
    res["select"] = _timed(m, lambda: m.select_batch_device(ct, ot, sel, dso), steps, warmup)
    res["scratch_select"] = int(m.scratch_bytes())
    res["tokens_ok"] = True
    if select_only:
        return res
    for name, gap_runs in (("tokens", False), ("tokens_gap_runs", True)):
        m.release_scratch()
        n_tok = _sized(lambda: m.tokens_batch_device(ct, ot, None, gap_runs=gap_runs))
        tok = torch.zeros((n_tok + 1, 3), dtype=torch.int32, device=dev)
        r = _timed(m, lambda: m.tokens_batch_device(ct, ot, tok, dto, gap_runs=gap_runs), steps, warmup)
        r["tokens"], r["scratch"] = int(n_tok), int(m.scratch_bytes())
        r["ok"] = _tokens_ok(tok, dto, sel[:n_sel], dso, ot, n_tok)
        res["tokens_ok"] = res["tokens_ok"] and r["ok"]
        # the copy ceiling for the bytes this call writes
        dst = torch.empty_like(tok)
        ms_copy = _median_ms(lambda: dst.copy_(tok), steps, warmup)[0]
        r["ms_copy_same_bytes"] = round(ms_copy, 4)
        r["copy_gb_s"] = round(tok.numel() * 4 / ms_copy / 1e6, 1)
        extra = r["ms_write"] - res["select"]["ms_write"]
        r["ms_write_over_select"] = round(extra, 4)
        r["token_write_gb_s"] = round(n_tok * 12 / extra / 1e6, 1) if extra > 0 else None
        res[name] = r
        del tok, dst
        torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--configs", default="3")
    ap.add_argument("--bytes", type=int, default=None)
    ap.add_argument("--select-only", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tokens_bench.json"))
    a = ap.parse_args()
    out = {"tool": "tokens_bench", "steps": a.steps, "warmup": a.warmup, "select_only": a.select_only, "results": []}
    for c in a.configs.split(","):
        out["results"].append(run_cfg(int(c), a.bytes or SIZES[int(c)], a.steps, a.warmup, a.select_only))
    out["ok"] = all(r["tokens_ok"] for r in out["results"])
    line = json.dumps(out)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")
    print(line)
    return 0 if out["ok"] else 1


if __name__ == "__main__":
    sys.exit(main())
