"""Per-wave clocks of one ku_traverse launch: when the waves of the persistent grid end, and what the early ones share.

Build the library with tools/lab/wave_clk.patch applied and -DAHA_WAVE_CLK, run one call of 512 MiB or more with
AHA_WAVE_CLK_OUT=<file> (bench.py --steps 2 --warmup 1 will do), then: python tools/lab/wave_clk.py <file> [waves, default 4096].
Four words per wave: the 100 MHz clock at kernel entry, at the head of the tile loop, behind it; HW_ID | XCC_ID << 32."""
import sys

import numpy as np

a = np.fromfile(sys.argv[1], dtype=np.uint64).reshape(-1, 4)
n = int(sys.argv[2]) if len(sys.argv) > 2 else 4096
a = a[:n]
t_in, t_a, t_b, hw = (a[:, i].astype(np.int64) for i in range(4))
live = t_b > 0
print("waves with clocks:", int(live.sum()), "of", n)
t0 = t_in[live].min()
end = t_b.max()
T = (end - t0) / 100.0  # us (100 MHz)
print("kernel, first entry to last wave's end: %.1f us" % T)
print("entry spread: %.1f us; loop head (after the tables) median %.1f us, max %.1f us after the first entry"
      % ((t_in.max() - t0) / 100.0, np.median(t_a - t0) / 100.0, (t_a.max() - t0) / 100.0))
e = (t_b - t0) / 100.0
print("wave end, us after first entry: min %.1f  p1 %.1f  p10 %.1f  p25 %.1f  median %.1f  p75 %.1f  p90 %.1f  p99 %.1f  max %.1f"
      % (e.min(), *np.percentile(e, [1, 10, 25, 50, 75, 90, 99]), e.max()))
print("  as a share of the kernel: min %.3f p10 %.3f median %.3f p90 %.3f" % (e.min() / T, np.percentile(e, 10) / T, np.median(e) / T, np.percentile(e, 90) / T))
idle = (e.max() - e).sum() / (n * e.max())
print("idle share of wave-slot time (wave's end to kernel's end): %.4f" % idle)
d = (t_b - t_a) / 100.0
print("loop time per wave, us: min %.1f median %.1f max %.1f; sd %.1f" % (d.min(), np.median(d), d.max(), d.std()))
hw_id = (hw & 0xFFFFFFFF).astype(np.int64)
xcc = ((hw >> 32) & 0xF).astype(np.int64)
simd = (hw_id >> 4) & 3
cu = (hw_id >> 8) & 15
sh = (hw_id >> 12) & 1
se = (hw_id >> 13) & 7
wiw = np.arange(n) % 16
for name, key in (("xcc", xcc), ("se", se), ("sh", sh), ("cu", cu), ("simd", simd), ("wave in workgroup", wiw)):
    print("by", name)
    for v in np.unique(key):
        m = key == v
        print("   %2d: n %4d  end median %.1f  min %.1f  max %.1f  mean idle %.4f" % (v, m.sum(), np.median(e[m]), e[m].min(), e[m].max(), ((e.max() - e[m]).mean() / e.max())))
# per workgroup: spread inside a workgroup vs between
wg = e.reshape(-1, 16)
print("spread inside a workgroup (max - min of its waves' ends), us: median %.1f max %.1f" % (np.median(wg.max(1) - wg.min(1)), (wg.max(1) - wg.min(1)).max()))
print("spread of workgroup means, us: sd %.1f  min %.1f max %.1f" % (wg.mean(1).std(), wg.mean(1).min(), wg.mean(1).max()))
# variance explained
tot = e.var()
for name, key in (("xcc", xcc), ("xcc*se*cu", xcc * 1000 + se * 100 + sh * 16 + cu), ("simd", simd), ("wave in workgroup", wiw)):
    means = {v: e[key == v].mean() for v in np.unique(key)}
    expl = np.array([means[v] for v in key]).var()
    print("variance of the end times explained by %s: %.3f" % (name, expl / tot))
