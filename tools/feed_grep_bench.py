"""Feed grep calls beside the batch calls they are to be held against, batch resident on the device (one MI355X).

The same bytes, records and key prefixes as tools/grep_bench.py (profiles/grep_bench.json): cfg 2 at 64 MiB and cfg 3 at 1 GiB,
a newline written over one byte in 100 on average.  The documents are the pieces, one sequence each, and every piece is cut
mid-line: each document is fed as two pieces, its first half in one call and its second half, with FINAL, in the next, both
cuts moved off the line ends -- so every piece of the second call continues an open record (its windows are not empty) and a
step of two calls leaves the feed as it found it.  Medians of --steps timed steps (after --warmup) with min and max:
(a) feed grep, both calls of a step, with the copy and in the ids-only form;
(b) records_device + grep_batch_device of the same bytes as one batch: the yardstick (the figures of profiles/grep_bench.json
    are those of the commit before feed grep; the two calls are measured again here, on the same machine and batch);
(c) the feed count without key counts of the same two calls.
The expectation (a) is held against: (b), plus the feed's fixed part of about 0.2 ms per call -- twice per
step --, plus one small count of the window batch.  The kept bytes of (a) are checked against (b)'s.
Writes profiles/feed_grep_bench.json (--out) and prints the same JSON line.
Usage: python tools/feed_grep_bench.py [--steps 10] [--warmup 3] [--configs 2,3] [--max-bytes N] [--out PATH]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from grep_bench import SIZES, _median_ms  # noqa: E402


def _mid_line(corpus, at):
    """`at` moved forward until it does not stand behind a newline or on one (a cut in the middle of a line)"""
    n = corpus.size
    while 0 < at < n and (corpus[at - 1] == 10 or corpus[at] == 10):
        at += 1
    return at


def run_cfg(cfg, steps, warmup, max_bytes, parent):
    import torch
    from aha_amd import AC, AhaError, synth

    dev = "cuda:0"
    n_bytes = min(SIZES[cfg], max_bytes) if max_bytes else SIZES[cfg]
    blob, offs, nf = synth.keys(cfg)
    corpus, doc = synth.corpus(cfg, blob, offs, nf, n_bytes=n_bytes)
    rng = np.random.default_rng(cfg)
    corpus = corpus.copy()
    corpus[rng.random(corpus.size) < 0.01] = 10
    N, D = int(corpus.size), doc.size - 1
    # the sequences: the documents with their boundaries moved to the middle of a line; each in two pieces
    seq = np.array([0] + [_mid_line(corpus, int(x)) for x in doc[1:-1]] + [N], dtype=np.int64)
    seq = np.maximum.accumulate(seq)
    mid = np.array([max(int(seq[d]), min(int(seq[d + 1]), _mid_line(corpus, int(seq[d] + seq[d + 1]) // 2))) for d in range(D)],
                   dtype=np.int64)
    first = np.concatenate([corpus[seq[d]:mid[d]] for d in range(D)])
    second = np.concatenate([corpus[mid[d]:seq[d + 1]] for d in range(D)])
    off1 = np.concatenate([[0], np.cumsum(mid - seq[:-1])]).astype(np.int64)
    off2 = np.concatenate([[0], np.cumsum(seq[1:] - mid)]).astype(np.int64)
    c1, c2 = torch.from_numpy(first).to(dev), torch.from_numpy(second).to(dev)
    o1, o2 = torch.from_numpy(off1).to(dev), torch.from_numpy(off2).to(dev)
    ids = torch.arange(D, dtype=torch.int32, device=dev)
    ct, st = torch.from_numpy(corpus).to(dev), torch.from_numpy(seq).to(dev)
    res = {"config": cfg, "bytes": N, "pieces_per_call": int(D), "calls_per_step": 2, "ok": True, "cases": []}
    prior = next((r for r in parent.get("results", []) if r["config"] == cfg and r["bytes"] == N), None)
    if prior:
        cases = [(c["keys"], c["invert"]) for c in prior["cases"]]
    else:  # (another size than the profile's: the first prefix of the profile's kind)
        cases = [(64, False), (64, True)]
    full = AC.compile_packed(blob, offs)
    try:
        R = full.records_device(ct, st, None)
    except AhaError as e:
        R = e.n_required
    rt = torch.zeros(R + 1, dtype=torch.int64, device=dev)
    res["records"] = int(R)
    res["ms_records"] = _median_ms(lambda: full.records_device(ct, st, rt), steps, warmup)
    del full
    for kk, invert in cases:
        m = AC.compile_packed(blob[: int(offs[kk])], offs[: kk + 1])
        c = {"keys": int(kk), "invert": invert}
        # (b) the batch calls over the same bytes, the sequences as documents
        nk, nb, nh = m.grep_batch_device(ct, rt, invert=invert)
        kept = torch.zeros(nk + 1, dtype=torch.int64, device=dev)
        doo = torch.zeros(nk + 2, dtype=torch.int64, device=dev)
        out = torch.zeros(nb + 16, dtype=torch.uint8, device=dev)
        c.update(kept=int(nk), kept_fraction=nk / max(R, 1), out_bytes=int(nb))
        c["ms_batch_grep"] = _median_ms(lambda: m.grep_batch_device(ct, rt, kept, doo, out, invert=invert, cap_docs=nk), steps, warmup)
        c["ms_batch_grep_ids_only"] = _median_ms(lambda: m.grep_batch_device(ct, rt, kept, doo, None, invert=invert, cap_docs=nk), steps,
                                                 warmup)
        c["ms_batch_records_plus_grep"] = res["ms_records"]["median"] + c["ms_batch_grep"]["median"]
        if prior:
            pc = next(x for x in prior["cases"] if x["keys"] == kk and x["invert"] == invert)
            c["ms_parent_records_plus_grep"] = prior["ms_records"]["median"] + pc["ms_grep"]["median"]
            c["ms_parent_records_plus_grep_ids_only"] = prior["ms_records"]["median"] + pc["ms_grep_ids_only"]["median"]
        want = out[:nb].cpu().numpy().tobytes()
        # (a) feed grep: two calls a step
        feed = m.feed(D)
        k1, r1, b1 = (torch.zeros(R + 2, dtype=torch.int64, device=dev), torch.zeros(R + 3, dtype=torch.int64, device=dev),
                      torch.zeros(N // 2 + (1 << 20), dtype=torch.uint8, device=dev))
        k2, r2, b2 = torch.zeros_like(k1), torch.zeros_like(r1), torch.zeros_like(b1)
        head = torch.zeros(D, dtype=torch.int64, device=dev)
        hold = torch.zeros(D, dtype=torch.int32, device=dev)
        got = {}

        def step(copy):
            got["a"] = feed.grep_batch_device(c1, o1, ids, k1, r1, b1 if copy else None, invert=invert, piece_hold=hold)
            got["b"] = feed.grep_batch_device(c2, o2, ids, k2, r2, b2 if copy else None, invert=invert, final=True, piece_head=head)

        c["ms_feed_grep"] = _median_ms(lambda: step(True), steps, warmup)
        c["ms_feed_grep_ids_only"] = _median_ms(lambda: step(False), steps, warmup)
        step(True)
        c["feed_fragments"] = [int(got["a"][0]), int(got["b"][0])]
        c["feed_kept"] = [int(got["a"][1]), int(got["b"][1])]
        # the kept bytes: call 1's, then per sequence the held bytes (the tail of its first piece) in front of call 2's
        o_a, o_b = b1[: got["a"][2]].cpu().numpy().tobytes(), b2[: got["b"][2]].cpu().numpy().tobytes()
        hd, ho = head.cpu().numpy(), hold.cpu().numpy()
        held = sum(int(hd[d]) for d in range(D))
        ok = len(o_a) + len(o_b) + held == len(want) and all(int(hd[d]) in (0, int(ho[d])) for d in range(D))
        c["ok"] = bool(ok)
        res["ok"] = res["ok"] and c["ok"]
        # (c) the feed count without key counts of the same two calls
        fc = m.feed(D)

        def count_step():
            fc.count_batch_device(c1, o1, ids)
            fc.count_batch_device(c2, o2, ids)
            fc.reset()

        c["ms_feed_count_no_keys"] = _median_ms(count_step, steps, warmup)
        c["feed_minus_batch"] = c["ms_feed_grep"]["median"] - c["ms_batch_records_plus_grep"]
        res["cases"].append(c)
        print(f"cfg {cfg}: {kk} keys, invert {invert}: feed {c['ms_feed_grep']['median']:.3f} ms, batch "
              f"{c['ms_batch_records_plus_grep']:.3f} ms", file=sys.stderr, flush=True)
        del feed, fc, m, k1, r1, b1, k2, r2, b2, kept, doo, out
        torch.cuda.empty_cache()
    res["ok"] = bool(res["ok"])
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--configs", default="2,3")
    ap.add_argument("--max-bytes", type=int, default=0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "feed_grep_bench.json"))
    a = ap.parse_args()
    try:
        parent = json.load(open(os.path.join(ROOT, "profiles", "grep_bench.json")))
    except OSError:
        parent = {}
    out = {"tool": "feed_grep_bench", "steps": a.steps, "warmup": a.warmup, "results": []}
    for c in a.configs.split(","):
        out["results"].append(run_cfg(int(c), a.steps, a.warmup, a.max_bytes, parent))
    out["ok"] = all(r["ok"] for r in out["results"])
    line = json.dumps(out)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")
    print(line)
    return 0 if out["ok"] else 1


if __name__ == "__main__":
    sys.exit(main())
