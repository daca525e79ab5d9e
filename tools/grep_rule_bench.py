"""Rule grep beside what it replaces, batch resident on the device (one MI355X).

For cfg 2 at 64 MiB and cfg 3 at 1 GiB, split into lines as tools/grep_bench.py splits them (a newline written over one byte
in 100 on average), the keys dealt round-robin into C = 8 and C = 64 classes, one count rule and one density rule per C --
the candidate whose kept fraction lies nearest one half, searched with the sizing call (the achieved fraction is reported: a
sparse key set may not reach one half) -- medians of --steps timed calls (after --warmup) with min and max:
(a) grep_batch_device with the rule: ids only, and with the copy;
(b) what it replaces: class_counts_batch_device, then the caller's torch predicate over the table and nonzero;
(c) class_counts_batch_device alone;
(d) (a) - (c): the two new kernels and grep's tail; beside it a device-to-device copy of the D x C table, which reads it once
    and writes it once.
The kept documents of (a) are checked against (b)'s.  --attach NAME=FILE (repeatable) stores the last JSON line of FILE under
"attached": the no-regression figures of bench.py and tools/grep_bench.py on the parent commit and on this one.
AHA_RULE_TABLE_BYTES defaults to 8 GiB here: cfg 3's table at C = 64 is 2.7 GB.
Writes profiles/grep_rule_bench.json (--out) and prints the same JSON line.
Usage: python tools/grep_rule_bench.py [--steps 10] [--warmup 3] [--configs 2,3] [--max-bytes N] [--attach NAME=FILE] [--out PATH]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ.setdefault("AHA_RULE_TABLE_BYTES", str(8 << 30))

SIZES = {2: 64 << 20, 3: 1 << 30}
CLASSES = (8, 64)


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


def _candidates(C, density):
    """rules "some of the first j classes has at least t hits (per den bytes)": j groups of one term"""
    out = []
    for j in (1, 2, 4, 8, 16, 32, 64):
        if j > C:
            break
        for t in (1, 2, 3):
            for den in ((100, 400) if density else (0,)):
                out.append([[(c, ">=", t, den)] for c in range(j)])
    return out


def _torch_predicate(rows, lens, spec):
    """the caller's predicate over the (D, C) table: OR over groups, AND inside one.  The searched rules -- one term per group,
    the same bound on the first j classes -- are written the way a caller would: one comparison over j columns, then any"""
    import torch

    first = spec[0][0]
    if all(len(g) == 1 and g[0][1:] == first[1:] for g in spec) and [g[0][0] for g in spec] == list(range(len(spec))):
        _, op, num, den = first
        cols = rows[:, :len(spec)]
        if den:
            lhs, rhs = cols.to(torch.int64) * den, (lens * num)[:, None]
        else:
            lhs, rhs = cols, num
        return ((lhs >= rhs) if op == ">=" else (lhs < rhs)).any(dim=1)
    keep = torch.zeros(rows.shape[0], dtype=torch.bool, device=rows.device)
    for group in spec:
        ok = torch.ones_like(keep)
        for c, op, num, den in group:
            col = rows[:, c].to(torch.int64)
            lhs, rhs = (col * den, lens * num) if den else (col, num)
            ok &= (lhs >= rhs) if op == ">=" else (lhs < rhs)
        keep |= ok
    return keep


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
    m = AC.compile_packed(blob, offs)
    try:
        R = m.records_device(ct, ot, None)
    except AhaError as e:  # the sizing call: the required count
        R = e.n_required
    rt = torch.zeros(R + 1, dtype=torch.int64, device=dev)
    m.records_device(ct, ot, rt)
    lens = rt[1:] - rt[:-1]
    res = {"config": cfg, "bytes": N, "keys": int(K), "records": int(R), "ok": True, "rows": []}
    print(f"cfg {cfg}: {N} bytes, {R} records", file=sys.stderr, flush=True)
    for C in CLASSES:
        table = m.classes([[k % C] for k in range(K)], n_classes=C)
        rows = torch.zeros((R, C), dtype=torch.int32, device=dev)
        spare = torch.zeros((R, C), dtype=torch.int32, device=dev)
        ms_counts = _median_ms(lambda: m.class_counts_batch_device(ct, rt, table, rows), steps, warmup)
        ms_copy_rows = _median_ms(lambda: spare.copy_(rows), steps, warmup)
        del spare
        for kind in ("count", "density"):
            tried = []
            for spec in _candidates(C, kind == "density"):
                tried.append((abs(m.grep_batch_device(ct, rt, rule=spec, classes=table)[0] / max(R, 1) - 0.5), len(tried), spec))
            spec = min(tried)[2]
            rule = m.rule(spec, table)
            nk, nb, nh = m.grep_batch_device(ct, rt, rule=rule)
            kept = torch.zeros(nk + 1, dtype=torch.int64, device=dev)
            doo = torch.zeros(nk + 2, dtype=torch.int64, device=dev)
            out = torch.zeros(nb + 16, dtype=torch.uint8, device=dev)
            r = {"classes": C, "rule": kind, "terms": len(rule.terms), "spec_first_group": [list(t) for t in spec[0]],
                 "kept": int(nk), "kept_fraction": nk / max(R, 1), "out_bytes": int(nb), "hits": int(nh),
                 "table_bytes": int(R) * C * 4}
            r["ms_rule_grep_ids_only"] = _median_ms(lambda: m.grep_batch_device(ct, rt, kept, doo, None, cap_docs=nk, rule=rule),
                                                    steps, warmup)
            r["ms_rule_grep"] = _median_ms(lambda: m.grep_batch_device(ct, rt, kept, doo, out, cap_docs=nk, rule=rule), steps, warmup)

            def replaced():
                m.class_counts_batch_device(ct, rt, table, rows)
                return _torch_predicate(rows, lens, spec).nonzero()

            r["ms_counts_predicate_nonzero"] = _median_ms(replaced, steps, warmup)
            r["ms_class_counts"] = ms_counts
            r["ms_copy_rows_d2d"] = ms_copy_rows
            r["rule_grep_ids_only_minus_class_counts"] = r["ms_rule_grep_ids_only"]["median"] - ms_counts["median"]
            r["rule_grep_minus_class_counts"] = r["ms_rule_grep"]["median"] - ms_counts["median"]
            r["added_over_copy_rows"] = r["rule_grep_ids_only_minus_class_counts"] / max(ms_copy_rows["median"], 1e-9)
            r["ids_only_not_slower_than_replaced"] = r["ms_rule_grep_ids_only"]["median"] <= r["ms_counts_predicate_nonzero"]["median"]
            m.set_profiling(True)
            m.grep_batch_device(ct, rt, kept, doo, out, cap_docs=nk, rule=rule)
            r["timing"] = {k: (round(v, 4) if isinstance(v, float) else v) for k, v in m.last_timing().items()}
            m.set_profiling(False)
            ids = replaced().flatten()
            r["ok"] = bool(ids.numel() == nk and torch.equal(ids, kept[:nk]))
            res["ok"] = res["ok"] and r["ok"]
            res["rows"].append(r)
            print(f"cfg {cfg}: C {C}, {kind} rule of {len(rule.terms)} terms: kept {r['kept_fraction']:.4f}, ids only "
                  f"{r['ms_rule_grep_ids_only']['median']:.3f} ms, replaced {r['ms_counts_predicate_nonzero']['median']:.3f} ms, "
                  f"class counts {ms_counts['median']:.3f} ms", file=sys.stderr, flush=True)
            del kept, doo, out
        del rows, table
        torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--configs", default="2,3")
    ap.add_argument("--max-bytes", type=int, default=0)
    ap.add_argument("--attach", action="append", default=[], metavar="NAME=FILE")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "grep_rule_bench.json"))
    a = ap.parse_args()
    out = {"tool": "grep_rule_bench", "steps": a.steps, "warmup": a.warmup, "results": []}
    for c in a.configs.split(","):
        out["results"].append(run_cfg(int(c), a.steps, a.warmup, a.max_bytes))
    out["ok"] = all(r["ok"] for r in out["results"])
    out["attached"] = {}
    for item in a.attach:
        name, path = item.split("=", 1)
        lines = [ln for ln in open(path).read().splitlines() if ln.startswith("{")]
        out["attached"][name] = json.loads(lines[-1]) if lines else None
    line = json.dumps(out)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")
    print(line)
    return 0 if out["ok"] else 1


if __name__ == "__main__":
    sys.exit(main())
