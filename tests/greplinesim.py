"""The context-lines contract (aha_ac_grep_batch* with AHA_GREP_LINES) in plain Python, taken from per-record hit counts: the
brute-force definition, and a model of the device passes by runs, windows and toggles (scan_greplines.hip, DESIGN.md 4.16
"Context lines").  Slow and obvious on purpose; the tests give it the CPU oracle's hits per record.  It does not import the
library."""
import numpy as np


def _groups(groups, D):
    """-> the group offsets as a list of G + 1 ints; None: the one group [0, D)"""
    return [0, D] if groups is None else [int(x) for x in groups]


def groups_ok(groups, D):
    """what the device validates: first entry 0, ascending (equal neighbours allowed), last entry D"""
    g = [int(x) for x in groups]
    return len(g) >= 1 and g[0] == 0 and g[-1] == D and all(a <= b for a, b in zip(g, g[1:]))


def matches(hits_per_rec, D, invert):
    """m_r = (h_r >= 1) != invert: plain grep's keep"""
    return [(int(hits_per_rec[r]) >= 1) != bool(invert) for r in range(D)]


# ---- the contract, stated plainly ------------------------------------------------------------------------------------------
def keep_brute(m, before, after, groups):
    """record r of group [lo, hi) is kept when some s in that group has m[s] and r - after <= s <= r + before"""
    D = len(m)
    g = _groups(groups, D)
    front = [0] * (D + 1)  # front[r] = the matches among records [0, r): "some s in [a, b) has m[s]" is front[b] > front[a]
    for r in range(D):
        front[r + 1] = front[r] + (1 if m[r] else 0)
    keep = [False] * D
    for lo, hi in zip(g, g[1:]):
        for r in range(lo, hi):
            keep[r] = front[min(hi, r + before + 1)] > front[max(lo, r - after)]
    return keep


# ---- the device passes -------------------------------------------------------------------------------------------------------
def keep_model(m, before, after, groups):
    """Sm / Tm (a run of matches of one group starts / ends), run j's group (the LAST g with groups[g] <= s: empty groups are
    stepped over) and window, first / last over runs, the toggles XOR-ed into D + 1 bits, the inclusive prefix parity"""
    D = len(m)
    g = _groups(groups, D)
    G = len(g) - 1
    Sm = [m[r] and not (r and m[r - 1]) for r in range(D)]
    Tm = [m[r] and not (r + 1 < D and m[r + 1]) for r in range(D)]
    for q in g[1:-1]:  # the inner group boundaries
        if 0 < q < D and m[q - 1] and m[q]:
            Sm[q] = True
            Tm[q - 1] = True
    s_at = [r for r in range(D) if Sm[r]]
    t_at = [r for r in range(D) if Tm[r]]
    assert len(s_at) == len(t_at) and all(a <= b for a, b in zip(s_at, t_at))
    grp, w0, w1 = [], [], []
    for s, t in zip(s_at, t_at):
        k = max(i for i in range(G) if g[i] <= s)
        assert g[k] <= s <= t < g[k + 1]
        grp.append(k)
        w0.append(max(g[k], s - before))
        w1.append(min(g[k + 1], t + 1 + after))
    n = len(grp)
    tog = [0] * (D + 1)
    for j in range(n):
        first = j == 0 or grp[j - 1] != grp[j] or w0[j] > w1[j - 1]
        last = j + 1 == n or grp[j + 1] != grp[j] or w0[j + 1] > w1[j]
        if first:
            tog[w0[j]] ^= 1
        if last:
            tog[w1[j]] ^= 1
    keep, par = [], 0
    for r in range(D):
        par ^= tog[r]
        keep.append(bool(par))
    assert D == 0 or (par ^ tog[D]) == 0  # every chunk that opens is closed
    return keep


# ---- the results ---------------------------------------------------------------------------------------------------------------
def grep_lines(hits_per_rec, offs, corpus, invert, before, after, groups=None, model=False):
    """-> (kept_docs uint64[n_kept], out uint8, doc_out_offsets uint64[n_kept+1], is_match uint8[n_kept])"""
    text = bytes(np.asarray(corpus, dtype=np.uint8).tobytes())
    off = [int(x) for x in offs]
    D = len(off) - 1
    m = matches(hits_per_rec, D, invert)
    keep = (keep_model if model else keep_brute)(m, int(before), int(after), groups)
    kept = [r for r in range(D) if keep[r]]
    parts = [text[off[r]:off[r + 1]] for r in kept]
    doo = np.zeros(len(kept) + 1, dtype=np.uint64)
    if kept:
        doo[1:] = np.cumsum([len(x) for x in parts], dtype=np.uint64)
    return (np.array(kept, dtype=np.uint64), np.frombuffer(b"".join(parts), dtype=np.uint8).copy(), doo,
            np.array([1 if m[r] else 0 for r in kept], dtype=np.uint8))


def chunk_ends(kept, groups, D):
    """-> bool[n_kept - 1]: a chunk ends behind kept record i (kept[i+1] != kept[i] + 1, or the two lie in different groups)"""
    k = [int(x) for x in kept]
    g = _groups(groups, D)
    own = [max(i for i in range(len(g) - 1) if g[i] <= r) for r in k]
    return [k[i + 1] != k[i] + 1 or own[i + 1] != own[i] for i in range(len(k) - 1)]
