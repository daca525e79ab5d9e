"""Longest feeds (AC.feed(.., longest=1 | 2)) against the batch match_longest of the same bytes, batch resident on the device
(one MI355X), cfg 3's keys and text.  Every row is the median of --steps calls with [min, max], host clock around calls that end
in a stream synchronise, the two sides of a row alternating call by call after --warmup rounds; every feed call starts from a
reset feed whose sequences were given one warm-up piece, so every piece starts from a carried state.

  chunks   mode 2, one sequence fed 64 MiB as one piece (kfl_chunks) | aha_ac_match_batch_device(longest = 2) of the same 64 MiB
           as one document (k_longest_chunks): the feed pays the carried-state load and store, the check and kfl_commit on top
  pieces   modes 1 and 2, 16384 sequences with 4 KiB pieces (kfl_pieces) | the batch call of the same bytes as 16384 documents
  switch   mode 2 at mean piece lengths of 256 B, 1 KiB and 4 KiB (64 MiB per call) through both walks
           (AHA_FEED_LONGEST_WALK = pieces | chunks): the rows behind the rule in engine.cpp device_feed_longest_count
  --gate   a batch match_longest mode-2 call of the 64 MiB alone (one JSON line; tools run it on two builds, alternating)

Writes profiles/feed_longest_bench.json (--out) and prints it as one JSON line.
Usage: python tools/feed_longest_bench.py [--steps 10] [--warmup 2] [--gate]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N_BYTES = 64 << 20


def stats(ms):
    ms = sorted(ms)
    return {"median_ms": round(float(np.median(ms)), 4), "min_ms": round(ms[0], 4), "max_ms": round(ms[-1], 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--gate", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "feed_longest_bench.json"))
    args = ap.parse_args()
    import torch
    from aha_amd import AC, synth

    assert torch.cuda.is_available(), "this tool measures on the GPU"
    dev = "cuda:0"
    blob, offs, nf = synth.keys(3)
    corpus, _ = synth.corpus(3, blob, offs, nf, n_bytes=N_BYTES)
    corpus = corpus[:N_BYTES]
    m = AC.compile_packed(blob, offs)
    ct = torch.from_numpy(corpus).to(dev)
    cap = N_BYTES // 8
    out = torch.zeros((cap, 3), dtype=torch.int32, device=dev)

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        n = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, n

    def layout(piece):
        D = N_BYTES // piece
        ot = torch.arange(D + 1, dtype=torch.int64, device=dev) * piece
        it = torch.arange(D, dtype=torch.int32, device=dev)
        return D, ot, it, torch.zeros(D + 1, dtype=torch.int64, device=dev)

    def batch_call(mode, ot, dho):
        return lambda: m.match_batch_device(ct, ot, out, dho, longest=mode)

    def run(sides):
        """sides: name -> (prepare or None, call); they alternate call by call"""
        ms = {k: [] for k in sides}
        hits = {}
        for r in range(args.warmup + args.steps):
            for k, (prep, call) in sides.items():
                if prep:
                    prep()
                t, n = timed(call)
                hits[k] = int(n)
                if r >= args.warmup:
                    ms[k].append(t)
        return {k: dict(stats(v), hits=hits[k]) for k, v in ms.items()}

    def feed_side(mode, D, ot, it, pho, walk=None):
        f = m.feed(D, longest=mode)
        warm = torch.arange(D + 1, dtype=torch.int64, device=dev) * 16  # 16 bytes per sequence: a carried state everywhere

        def prep():
            if walk:
                os.environ["AHA_FEED_LONGEST_WALK"] = walk
            else:
                os.environ.pop("AHA_FEED_LONGEST_WALK", None)
            f.reset()
            f.match_batch_device(ct[:16 * D], warm, it, out)

        return prep, lambda: f.match_batch_device(ct, ot, it, out, pho)

    if args.gate:
        D, ot, it, dho = layout(N_BYTES)
        r = run({"batch_longest2": (None, batch_call(2, ot, dho))})
        print(json.dumps({"gate_batch_longest2": r["batch_longest2"]}))
        return
    res = {"bytes_per_call": N_BYTES, "keys": int(m.info["n_keys"]), "max_key_len": int(m.info["max_key_len"]), "steps": args.steps,
           "warmup": args.warmup, "method": "host clock around calls that end in a stream synchronise; sides alternate call by call"}
    D, ot, it, pho = layout(N_BYTES)
    res["chunks"] = run({"feed_mode2_one_piece": feed_side(2, D, ot, it, pho), "batch_longest2_one_doc": (None, batch_call(2, ot, pho))})
    D, ot, it, pho = layout(4096)
    res["pieces"] = run({"feed_mode1_4k": feed_side(1, D, ot, it, pho), "batch_longest1_4k_docs": (None, batch_call(1, ot, pho)),
                         "feed_mode2_4k_pieces": feed_side(2, D, ot, it, pho, "pieces"), "batch_longest2_4k_docs": (None, batch_call(2, ot, pho))})
    res["switch"] = {}
    for piece in (256, 1024, 4096):
        D, ot, it, pho = layout(piece)
        res["switch"][str(piece)] = run({"pieces": feed_side(2, D, ot, it, pho, "pieces"), "chunks": feed_side(2, D, ot, it, pho, "chunks")})
    os.environ.pop("AHA_FEED_LONGEST_WALK", None)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
