"""Feed cover against plain cover and against a feed match with the mask built from its hit list, batch resident on the
device (one MI355X).

For cfg 2 at 64 MiB, cfg 3 at 1 GiB and cfg 5 at 256 MiB (tools/feed_count_bench.py's sizes), in two shapes: the batch's
documents as the pieces of as many sequences, and the whole batch as one piece of one sequence.  Either is fed again on every
call, so that every piece after the first call has a context.  Records the median of --steps timed calls (after --warmup) of
  ms_cover              aha_ac_cover_batch_device of the same pieces as documents, mask only
  ms_feed_cover         aha_feed_cover_batch_device, mask and piece_back
  ms_feed_cover_redact  the same with the redacted copy as well
  ms_feed_match_mask    aha_feed_match_batch_device, then the mask from its hits in torch (a difference array over the batch and
                        a cumulative sum); left out (null) where the hit list is beyond --max-list-hits
the engines of the plain cover and of the feed cover's main pass, the hits and the covered bytes.  The clear and window kernels'
own times come from a kernel trace: rocprofv3 --kernel-trace --stats.  Prints one JSON line.
Usage: python tools/feed_cover_bench.py [--steps 10] [--warmup 3] [--configs 2,3,5]"""
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
    return float(np.median(ts))


def _engine(m, fn):
    m.set_profiling(True)
    fn()
    e = m.last_timing()["engine"]
    m.set_profiling(False)
    return e


def _mask_from_hits(hits, n_hits, pho, ot, n_bytes):
    """bool[N] from a feed match's hit list: +1 at every clipped start, -1 at every end, cumulative sum"""
    import torch

    D = ot.numel() - 1
    base = torch.repeat_interleave(ot[:D], pho[1:] - pho[:D])
    h = hits[:n_hits]
    diff = torch.zeros(n_bytes + 1, dtype=torch.int32, device=hits.device)
    one = torch.ones(n_hits, dtype=torch.int32, device=hits.device)
    diff.index_add_(0, base + h[:, 0].clamp(min=0), one)
    diff.index_add_(0, base + h[:, 1], -one)
    return torch.cumsum(diff[:n_bytes], 0) > 0


def run_shape(m, ct, ot, cfg, shape, steps, warmup, max_list_hits):
    import torch

    dev = "cuda:0"
    n = int(ct.numel())
    D = ot.numel() - 1
    it = torch.arange(D, dtype=torch.int32, device=dev)
    pho = torch.zeros(D + 1, dtype=torch.int64, device=dev)
    bases = torch.zeros(D, dtype=torch.int64, device=dev)
    back = torch.zeros(D, dtype=torch.int32, device=dev)
    mask = torch.zeros((n + 31) // 32, dtype=torch.int32, device=dev)
    red = torch.empty_like(ct)
    res = {"config": cfg, "shape": shape, "bytes": n, "pieces": int(D), "keys": int(m.n_keys)}
    res["covered_cover"], res["hits_cover"] = m.cover_batch_device(ct, ot, mask=mask)
    res["engine_cover"] = _engine(m, lambda: m.cover_batch_device(ct, ot, mask=mask))
    res["ms_cover"] = _median_ms(lambda: m.cover_batch_device(ct, ot, mask=mask), steps, warmup)
    m.release_scratch()
    f = m.feed(D)
    f.cover_batch_device(ct, ot, it, mask=mask, piece_back=back)
    res["covered_feed"], res["hits_feed"] = f.cover_batch_device(ct, ot, it, mask=mask, piece_back=back)  # (with contexts)
    res["back_bytes"] = int(back.sum())
    res["engine_feed_cover"] = _engine(m, lambda: f.cover_batch_device(ct, ot, it, mask=mask, piece_back=back))
    res["ms_feed_cover"] = _median_ms(lambda: f.cover_batch_device(ct, ot, it, mask=mask, piece_back=back), steps, warmup)
    res["ms_feed_cover_redact"] = _median_ms(
        lambda: f.cover_batch_device(ct, ot, it, mask=mask, redacted=red, piece_back=back), steps, warmup)
    res["ms_feed_match_mask"] = None
    if res["hits_feed"] <= max_list_hits:
        nh = res["hits_feed"]
        hits = torch.zeros((nh + 1024, 3), dtype=torch.int32, device=dev)

        def match_and_mask():
            assert f.match_batch_device(ct, ot, it, hits, pho, bases) == nh
            return _mask_from_hits(hits, nh, pho, ot, n)

        want = match_and_mask()
        f.cover_batch_device(ct, ot, it, mask=mask)
        bits = (mask.view(torch.uint8).unsqueeze(1) >> torch.arange(8, device=dev, dtype=torch.uint8)) & 1
        res["mask_equals_hit_list"] = bool(torch.equal(bits.reshape(-1)[:n].bool(), want))
        del bits, want
        res["ms_feed_match_mask"] = _median_ms(match_and_mask, steps, warmup)
        res["ratio_match_mask_feed_cover"] = round(res["ms_feed_match_mask"] / res["ms_feed_cover"], 3)
        del hits
    res["ms_feed_cover_minus_cover"] = round(res["ms_feed_cover"] - res["ms_cover"], 4)
    res["ratio_feed_cover_cover"] = round(res["ms_feed_cover"] / res["ms_cover"], 3)
    f.close()
    torch.cuda.empty_cache()
    m.release_scratch()
    return res


def run_cfg(cfg, steps, warmup, max_list_hits):
    import torch
    from aha_amd import AC, synth

    blob, offs, nf = synth.keys(cfg)
    corpus, doc = synth.corpus(cfg, blob, offs, nf, n_bytes=SIZES[cfg])
    m = AC.compile_packed(blob, offs)
    ct = torch.from_numpy(corpus).to("cuda:0")
    out = []
    for shape, d in (("many", doc), ("one", np.array([0, corpus.size], dtype=np.uint64))):
        ot = torch.from_numpy(d.astype(np.int64)).to("cuda:0")
        out.append(run_shape(m, ct, ot, cfg, shape, steps, warmup, max_list_hits))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--configs", default="2,3,5")
    ap.add_argument("--max-list-hits", type=int, default=1 << 31)
    a = ap.parse_args()
    res = {"tool": "feed_cover_bench", "steps": a.steps, "warmup": a.warmup, "results": []}
    for c in a.configs.split(","):
        res["results"] += run_cfg(int(c), a.steps, a.warmup, a.max_list_hits)
    print(json.dumps(res))
    return 0


if __name__ == "__main__":
    sys.exit(main())
