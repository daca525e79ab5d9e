"""What AHA_OPT_FOLD_KANA costs, batch resident on the device (one MI355X).  Medians of --steps timed calls (after --warmup) with
[min, max], the sides of a comparison ALTERNATING call by call in one loop.  The yardstick is the BMP-folded handle's staged
pass (mode 3: k_fold3_copy + k_fold3_fix), on the same text in the same process.

 pass:<kind>:<MiB>  the staged pass alone.  kind = ascii (printable ASCII: the fast path), chinese (the text of BASELINE config
                    3: three-byte characters, none of which moves) or japanese (a text this tool builds from a seed: hiragana,
                    katakana, half-width katakana and kanji, every character three bytes -- every 16-byte piece goes through the
                    table path and four characters in ten move).  The text is a view 5 bytes into a buffer, so every handle
                    stages it: a plain handle by a device-to-device copy, a simple-folded one by k_fold2_copy (mode 2), a
                    BMP-folded one by k_fold3_copy (mode 3, the yardstick), a kana-folded one by k_foldk_copy with the halo from
                    memory and from the neighbouring lanes (AHA_FOLDK_HALO=mem|lane, read at every launch).  Each less the plain
                    handle's aligned call = the pass; the key set is two words, so the match beside it is as short as a match
                    gets.  Hits: the kana-folded handle's are the same under both halo forms and equal a plain handle's over
                    the text folded beforehand (japanese: on the device, through a table built here from unicodedata; elsewhere
                    foldk = fold3 and the yardstick's hits).
 --no-kana          modes 2 and 3 only (what a library without the flag can run: the gate's parent side).
Prints one JSON line; --out writes it to a file too (after every case: a long run keeps what is measured so far).
Usage: python tools/fold_kana_bench.py [--steps 10] [--warmup 2] [--out profiles/fold_kana_bench.json] [--no-kana]
                                       [--cases pass:ascii:1024,pass:chinese:1024,pass:japanese:1024]"""
import argparse
import json
import os
import sys
import time
import unicodedata

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


def _halo(form):
    os.environ["AHA_FOLDK_HALO"] = form


def kana_map():
    """K of include/aha_hip.h as an int64 array over the BMP: K(cp) where K moves cp, cp elsewhere"""
    t = np.arange(0x10000, dtype=np.int64)
    t[0x3041:0x3097] += 0x60
    t[0x309D], t[0x309E] = 0x30FD, 0x30FE
    for cp in range(0xFF66, 0xFF9E):
        t[cp] = ord(unicodedata.normalize("NFKC", chr(cp)))
    return t


def japanese(n, view):
    """fills view[:n] with n // 3 three-byte characters drawn from a seed -- 40 % hiragana, 25 % katakana, 10 % half-width
    katakana, 25 % kanji -- and spaces behind them; -> the same text folded by the rule, the share of characters that move"""
    import torch

    g = torch.Generator(device=DEV)
    g.manual_seed(11)
    m = n // 3
    kind = torch.rand(m, device=DEV, generator=g)
    r = torch.rand(m, device=DEV, generator=g)
    cp = torch.where(kind < 0.40, 0x3041 + (r * (0x3097 - 0x3041)).long(),
                     torch.where(kind < 0.65, 0x30A1 + (r * (0x30F7 - 0x30A1)).long(),
                                 torch.where(kind < 0.75, 0xFF66 + (r * (0xFF9E - 0xFF66)).long(), 0x4E00 + (r * (0x9FA6 - 0x4E00)).long())))
    del kind, r
    fk = torch.from_numpy(kana_map()).to(DEV)[cp]
    moved = float((fk != cp).float().mean())

    def encode(dst, c):
        dst[0:3 * m:3] = (0xE0 | (c >> 12)).to(torch.uint8)
        dst[1:3 * m:3] = (0x80 | ((c >> 6) & 0x3F)).to(torch.uint8)
        dst[2:3 * m:3] = (0x80 | (c & 0x3F)).to(torch.uint8)
        dst[3 * m:] = 0x20

    encode(view, cp)
    prefolded = torch.empty(n, dtype=torch.uint8, device=DEV)
    encode(prefolded, fk)
    return prefolded, moved


def run_pass(kind, mib, steps, warmup, kana):
    import torch
    from aha_amd import AC, synth

    n = mib << 20
    g = torch.Generator(device=DEV)
    g.manual_seed(7)
    big = torch.zeros(n + 64, dtype=torch.uint8, device=DEV)
    view = big[5:5 + n]
    prefolded, moved = None, 0.0
    if kind == "ascii":
        view.copy_(torch.randint(32, 127, (n,), dtype=torch.uint8, device=DEV, generator=g))
        keys = ["error", "Warning"]
    elif kind == "chinese":
        blob, offs, nf = synth.keys(3)
        corpus, _ = synth.corpus(3, blob, offs, nf, n_bytes=n)
        view[:min(n, corpus.size)].copy_(torch.from_numpy(corpus[:n]).to(DEV))  # (a shorter corpus leaves NUL bytes behind it)
        keys = ["我是", "中国"]
    else:  # japanese
        prefolded, moved = japanese(n, view)
        keys = ["カナ", "コン"]
    aligned = view.clone()
    assert aligned.data_ptr() % 16 == 0 and view.data_ptr() % 16 == 5
    n_docs = max(n >> 20, 1)
    ot = torch.arange(0, n + 1, n // n_docs, dtype=torch.int64, device=DEV)
    handles = {"plain": AC.compile(keys), "simple": AC.compile(keys, fold_simple=True), "bmp": AC.compile(keys, fold_bmp=True)}
    hits = {k: m.count_batch_device(view, ot, None, None) for k, m in handles.items()}
    equal = hits["bmp"] == hits["simple"]  # (no text here has a character only the three-byte case fold moves)
    if kana:
        handles["kana"] = AC.compile(keys, fold_kana=True)
        for form in ("mem", "lane"):
            _halo(form)
            hits["kana_" + form] = handles["kana"].count_batch_device(view, ot, None, None)
        if prefolded is not None:
            hits["plain_on_prefolded"] = handles["plain"].count_batch_device(prefolded, ot, None, None)
            equal = hits["kana_mem"] == hits["kana_lane"] == hits["plain_on_prefolded"] > hits["bmp"]
        else:
            equal = hits["kana_mem"] == hits["kana_lane"] == hits["bmp"]
    del prefolded
    cap = max(hits.values()) + 1
    out = torch.zeros((cap, 3), dtype=torch.int32, device=DEV)
    dho = torch.zeros(ot.numel(), dtype=torch.int64, device=DEV)
    spare = torch.empty_like(aligned)

    def kana_call(form):
        _halo(form)
        handles["kana"].match_batch_device(view, ot, out, dho)

    fns = {"plain_aligned": lambda: handles["plain"].match_batch_device(aligned, ot, out, dho),
           "plain_unaligned_copy": lambda: handles["plain"].match_batch_device(view, ot, out, dho),
           "simple_unaligned_fold2_copy": lambda: handles["simple"].match_batch_device(view, ot, out, dho),
           "bmp_unaligned_fold3_copy": lambda: handles["bmp"].match_batch_device(view, ot, out, dho)}
    if kana:
        fns["kana_unaligned_foldk_copy_mem"] = lambda: kana_call("mem")
        fns["kana_unaligned_foldk_copy_lane"] = lambda: kana_call("lane")
    fns["bare_device_copy"] = lambda: spare.copy_(view)
    t = _alternate(fns, steps, warmup)
    os.environ.pop("AHA_FOLDK_HALO", None)
    base = t["plain_aligned"]

    def less_base(name):  # the pass: the call less the plain handle's aligned call, median and [min, max] of the call's own spread
        return {"median_ms": round(t[name]["median_ms"] - base["median_ms"], 4), "min_ms": round(t[name]["min_ms"] - base["median_ms"], 4),
                "max_ms": round(t[name]["max_ms"] - base["median_ms"], 4)}

    res = {"case": "pass:%s:%d" % (kind, mib), "bytes": n, "docs": n_docs, "moved_share": round(moved, 4), "hits": hits, "match": t,
           "copy_ms": less_base("plain_unaligned_copy"), "fold2_copy_ms": less_base("simple_unaligned_fold2_copy"),
           "fold3_copy_ms": less_base("bmp_unaligned_fold3_copy"), "equal": bool(equal)}
    if kana:
        res["foldk_copy_mem_ms"] = less_base("kana_unaligned_foldk_copy_mem")
        res["foldk_copy_lane_ms"] = less_base("kana_unaligned_foldk_copy_lane")
    if kind == "japanese":
        res["note"] = "the matches beside the passes differ: the kana-folded handle finds hits the others do not"
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--cases", default="pass:ascii:1024,pass:chinese:1024,pass:japanese:1024")
    ap.add_argument("--no-kana", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch

    if not torch.cuda.is_available():
        print("fold_kana_bench: no GPU (there is no CPU fallback for a measurement)", file=sys.stderr)
        return 2
    out = {"tool": "fold_kana_bench", "steps": a.steps, "warmup": a.warmup, "results": []}
    for c in a.cases.split(","):
        _, x, mib = c.split(":")
        out["results"].append(run_pass(x, int(mib), a.steps, a.warmup, not a.no_kana))
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
