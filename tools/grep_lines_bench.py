"""grep with context lines (AHA_GREP_LINES) beside plain grep on the same batch and the same matches, batch resident on the
device (one MI355X).

The batches of tools/grep_bench.py: cfg 2 at 64 MiB and cfg 3 at 1 GiB, a newline written over one byte in 100 on average, split
into records on the device; the matches near 1 % and near 50 % of the records by a prefix of the key set.  Medians of --steps
timed calls (after --warmup) with min and max:
(a) plain grep_batch_device over the records, ids only and with the copy;
(b) the lines call with before = after = 0 (the same keep set: what the dilation passes cost by themselves) and with before =
    after = 2 (grep -C 2), groups = the documents (the records call's doc_rec_offsets), ids only (with is_match) and with the copy;
(c) the lines call's extra time over plain grep, the kept fraction it produces, its scratch, the matching runs.
The kept records and is_match are checked against numpy over a count call's own hit offsets.
Writes profiles/grep_lines_bench.json (--out) and prints the same JSON line.
Usage: python tools/grep_lines_bench.py [--steps 10] [--warmup 3] [--configs 2,3] [--max-bytes N] [--out PATH]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from grep_bench import SIZES, TARGETS, _median_ms  # noqa: E402

CONTEXTS = (0, 2)


def _dilate(m, before, after, groups):
    """the contract over a bool array: record r of group [lo, hi) is kept when a match lies in [max(lo, r - after), min(hi, r + before + 1))"""
    D = m.size
    front = np.concatenate([[0], np.cumsum(m)])
    r = np.arange(D, dtype=np.int64)
    g = np.searchsorted(groups, r, side="right") - 1
    lo, hi = groups[g], groups[g + 1]
    return front[np.minimum(hi, r + before + 1)] > front[np.maximum(lo, r - after)]


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
    full = AC.compile_packed(blob, offs)
    try:
        R = full.records_device(ct, ot, None)
    except AhaError as e:  # the sizing call: the required count
        R = e.n_required
    rt = torch.zeros(R + 1, dtype=torch.int64, device=dev)
    drt = torch.zeros(D + 1, dtype=torch.int64, device=dev)
    full.records_device(ct, ot, rt, drt)
    del full
    groups = drt.cpu().numpy().astype(np.int64)
    res["records"] = int(R)
    print(f"cfg {cfg}: {N} bytes, {R} records, {D} groups", file=sys.stderr, flush=True)

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
    res["prefix_search"] = {str(k): round(v, 5) for k, v in tried.items()}
    dho = torch.zeros(R + 1, dtype=torch.int64, device=dev)
    kept = torch.zeros(R + 1, dtype=torch.int64, device=dev)
    doo = torch.zeros(R + 2, dtype=torch.int64, device=dev)
    flags = torch.zeros(R + 1, dtype=torch.uint8, device=dev)
    out = torch.zeros(N + 16, dtype=torch.uint8, device=dev)
    res["cases"] = []
    for target in TARGETS:
        kk = min(tried, key=lambda x: abs(tried[x] - target))
        m = handle(kk)
        m.count_batch_device(ct, rt, doc_hit_offsets=dho)
        match = np.diff(dho.cpu().numpy()) >= 1
        nk, nb, nh = m.grep_batch_device(ct, rt)
        c = {"keys": int(kk), "matching": int(nk), "matching_fraction": nk / max(R, 1), "hits": int(nh),
             "matching_runs": int(np.count_nonzero(match & ~np.concatenate([[False], match[:-1]])))}
        m.release_scratch()
        c["ms_grep_ids_only"] = _median_ms(lambda: m.grep_batch_device(ct, rt, kept, doo, None, cap_docs=R), steps, warmup)
        c["ms_grep"] = _median_ms(lambda: m.grep_batch_device(ct, rt, kept, doo, out, cap_docs=R), steps, warmup)
        c["scratch_grep"] = int(m.scratch_bytes())
        c["lines"] = []
        for ctx in CONTEXTS:
            m.release_scratch()
            kw = dict(before=ctx, after=ctx, groups=drt, matched=flags, cap_docs=R)
            lk, lb, lh = m.grep_batch_device(ct, rt, kept, doo, out, **kw)
            want = np.nonzero(_dilate(match, ctx, ctx, groups))[0]
            ok = lk == want.size and np.array_equal(kept[:lk].cpu().numpy(), want) and lh == nh
            ok = ok and np.array_equal(flags[:lk].cpu().numpy().astype(bool), match[want])
            e = {"context": ctx, "kept": int(lk), "kept_fraction": lk / max(R, 1), "out_bytes": int(lb), "ok": bool(ok)}
            e["ms_lines_ids_only"] = _median_ms(lambda: m.grep_batch_device(ct, rt, kept, doo, None, **kw), steps, warmup)
            e["ms_lines"] = _median_ms(lambda: m.grep_batch_device(ct, rt, kept, doo, out, **kw), steps, warmup)
            e["scratch_lines"] = int(m.scratch_bytes())
            e["ids_only_minus_grep_ids_only"] = e["ms_lines_ids_only"]["median"] - c["ms_grep_ids_only"]["median"]
            e["lines_minus_grep"] = e["ms_lines"]["median"] - c["ms_grep"]["median"]
            c["lines"].append(e)
            res["ok"] = res["ok"] and e["ok"]
            print(f"cfg {cfg}: {kk} keys, -C {ctx}: kept {e['kept_fraction']:.4f}, {e['ms_lines']['median']:.3f} ms "
                  f"(grep {c['ms_grep']['median']:.3f})", file=sys.stderr, flush=True)
        res["cases"].append(c)
        del m
        torch.cuda.empty_cache()
    res["ok"] = bool(res["ok"])
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--configs", default="2,3")
    ap.add_argument("--max-bytes", type=int, default=0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "grep_lines_bench.json"))
    a = ap.parse_args()
    out = {"tool": "grep_lines_bench", "steps": a.steps, "warmup": a.warmup, "results": []}
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
