// The partition of a batch into ranges of whole documents (aha_amd/csrc/doc_ranges.hpp) on made-up hit offsets: its real bound
// (about 2 GiB of hits) cannot be reached on a device at test sizes.  The reference is the three loops the rule replaced -- doc
// counts', select's and class counts' -- transcribed as they stood in engine.cpp before doc_ranges.hpp existed; the sweep checks
// the rule against each of them and the properties every caller relies on.  Built and run by tests/test_host_logic.py.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../aha_amd/csrc/doc_ranges.hpp"

using aha::DocRange;
using Offs = std::vector<uint64_t>;
using Ranges = std::vector<DocRange>;
constexpr uint64_t kHit = 12;  // sizeof(aha_hit)

static int fails = 0;
static void check(const char *name, bool ok) {
  std::printf("%s %s\n", ok ? "ok  " : "FAIL", name);
  if (!ok) fails++;
}

// ---- the three loops as they stood (the reference) --------------------------------------------------------------------------
// device_doc_counts: every range is opened at d0, hitless or not; a range without a hit is skipped inline
template <class Cost>
static Ranges old_doc_counts(const Offs &hd, uint64_t D, uint64_t dc_hit_bytes, Cost doc_bytes) {
  Ranges out;
  for (uint64_t d0 = 0; d0 < D;) {
    uint64_t d1 = d0, bytes = 0;
    while (d1 < D && (d1 == d0 || bytes + doc_bytes(hd[d1 + 1] - hd[d1]) <= dc_hit_bytes)) {
      bytes += doc_bytes(hd[d1 + 1] - hd[d1]);
      d1++;
    }
    const uint64_t nd = d1 - d0, rh = hd[d1] - hd[d0];
    const bool solo = nd == 1 && bytes > dc_hit_bytes;
    if (rh == 0) {  // (no hit: the documents' offsets stand as they are)
      d0 = d1;
      continue;
    }
    out.push_back(DocRange{d0, d1, solo});
    d0 = d1;
  }
  return out;
}

// device_select_to: the `bounds` vector; range r is [bounds[r], bounds[r + 1])
static Offs old_select(const Offs &hd, uint64_t D, uint64_t sel_hit_bytes) {
  const uint64_t n_hits = hd[D] - hd[0];
  Offs bounds;
  bounds.push_back(0);
  for (uint64_t d0 = 0; n_hits && d0 < D;) {
    uint64_t d1 = d0, bytes = 0;
    while (d1 < D && (bytes == 0 || bytes + (hd[d1 + 1] - hd[d1]) * kHit <= sel_hit_bytes)) {
      bytes += (hd[d1 + 1] - hd[d1]) * kHit;
      d1++;
    }
    bounds.push_back(d1);
    d0 = d1;
  }
  if (bounds.size() > 2 && hd[bounds.back()] == hd[bounds[bounds.size() - 2]]) bounds.erase(bounds.end() - 2);  // (a hitless tail)
  return bounds;
}

// device_class_counts: the whole-batch pre-check, else a range starts at a document with hits
static Ranges old_class_counts(const Offs &hd, uint64_t D, uint64_t bound) {
  const uint64_t n_hits = hd[D] - hd[0];
  Ranges ranges;
  if (n_hits && n_hits <= bound / kHit && n_hits < (1ull << 32)) {  // (2^32 hits: the documents are looked at)
    ranges.push_back(DocRange{0, D, false});
  } else if (n_hits) {
    for (uint64_t d0 = 0; d0 < D;) {
      if (hd[d0 + 1] == hd[d0]) {
        d0++;
        continue;
      }
      uint64_t d1 = d0 + 1, bytes = (hd[d0 + 1] - hd[d0]) * kHit;
      const bool solo = bytes > bound;
      while (!solo && d1 < D && bytes + (hd[d1 + 1] - hd[d1]) * kHit <= bound) {
        bytes += (hd[d1 + 1] - hd[d1]) * kHit;
        d1++;
      }
      ranges.push_back(DocRange{d0, d1, solo});
      d0 = d1;
    }
  }
  return ranges;
}

// ---- how the callers use the rule ---------------------------------------------------------------------------------------------
static uint64_t hit_cost(uint64_t h) { return h * kHit; }

// select: range r from the end of the one before it (0 for the first), the last to D
static Offs tiled(const Ranges &r, uint64_t D) {
  Offs bounds;
  bounds.push_back(0);
  for (const DocRange &g : r) bounds.push_back(g.d1);
  if (!r.empty()) bounds.back() = D;
  return bounds;
}

static bool same(const Ranges &a, const Ranges &b) {
  if (a.size() != b.size()) return false;
  for (size_t i = 0; i < a.size(); i++)
    if (a[i].d0 != b[i].d0 || a[i].d1 != b[i].d1 || a[i].solo != b[i].solo) return false;
  return true;
}

// the documents with hits of every range, and its solo flag: {first, last + 1 hit-bearing document, solo}
static Ranges hit_groups(const Ranges &r, const Offs &hd) {
  Ranges out;
  for (const DocRange &g : r) {
    uint64_t a = g.d0, b = g.d1;
    while (a < b && hd[a + 1] == hd[a]) a++;
    while (b > a && hd[b] == hd[b - 1]) b--;
    out.push_back(DocRange{a, b, g.solo});
  }
  return out;
}
static bool whole(const Ranges &r, uint64_t D) { return r.size() == 1 && r[0].d0 == 0 && r[0].d1 == D; }

// what every caller relies on
template <class Cost>
static bool sound(const Ranges &r, const Offs &hd, uint64_t D, uint64_t bound, Cost cost) {
  uint64_t at = 0;
  std::vector<int> in(D, 0);
  for (const DocRange &g : r) {
    if (g.d0 < at || g.d1 <= g.d0 || g.d1 > D) return false;  // ascending, disjoint, not empty
    at = g.d1;
    uint64_t sum = 0;
    for (uint64_t d = g.d0; d < g.d1; d++) {
      in[d]++;
      sum += cost(hd[d + 1] - hd[d]);
    }
    if (g.solo ? (g.d1 != g.d0 + 1 || sum <= bound) : sum > bound) return false;
    if (hd[g.d1] == hd[g.d0]) return false;  // (a range holds hits: `repeats` counts it)
  }
  for (uint64_t d = 0; d < D; d++)
    if (hd[d + 1] != hd[d] ? in[d] != 1 : in[d] > 1) return false;
  return true;
}

static Ranges rule(const Offs &hd, uint64_t bound) {
  Ranges r;
  if (!aha::doc_ranges(hd.data(), hd.size() - 1, bound, hit_cost, r)) fails++;
  return r;
}

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;  // fixed seed
static uint64_t rnd() {
  rng_state ^= rng_state << 13;
  rng_state ^= rng_state >> 7;
  rng_state ^= rng_state << 17;
  return rng_state;
}

int main() {
  // ---- the sweep ----
  const uint64_t hits_of[] = {0, 0, 0, 1, 1, 2, 3, 5, 8, 13, 40, 90, 1000, 100000};
  const uint64_t bounds_of[] = {12, 24, 36, 60, 96, 120, 156, 480, 1000, 4096};
  const uint64_t n_cases = 200000;
  uint64_t bad_cls = 0, bad_sel = 0, bad_dc = 0, bad_sound = 0, multi = 0, solos = 0;
  for (uint64_t c = 0; c < n_cases; c++) {
    const uint64_t D = rnd() % 13;
    Offs hd(D + 1);
    hd[0] = rnd() % 3 ? 0 : rnd() % 1000;  // (the offsets need not start at 0)
    for (uint64_t d = 0; d < D; d++) hd[d + 1] = hd[d] + hits_of[rnd() % (sizeof(hits_of) / sizeof(hits_of[0]))];
    const uint64_t pick = rnd() % 14;
    const uint64_t bound = pick < 10 ? bounds_of[pick] : 12 + rnd() % 989;
    // doc counts' cost: the hits, and in the range form (sort_max < h < dense_min) the pairs beside them
    const uint64_t sort_max = rnd() % 4 * 4, dense_min = sort_max + 1 + rnd() % 40, K = 1 + rnd() % 20;
    auto form = [&](uint64_t h) { return h <= sort_max ? 0 : (h < dense_min ? 1 : 2); };
    auto doc_bytes = [&](uint64_t h) { return h * kHit + (form(h) == 1 ? std::min<uint64_t>(h, K) * 8 : 0); };

    const Ranges r = rule(hd, bound);
    if (!same(r, old_class_counts(hd, D, bound))) bad_cls++;
    if (tiled(r, D) != old_select(hd, D, bound)) bad_sel++;
    if (!sound(r, hd, D, bound, hit_cost)) bad_sound++;
    Ranges rd;
    if (!aha::doc_ranges(hd.data(), D, bound, doc_bytes, rd)) fails++;
    const Ranges od = old_doc_counts(hd, D, bound, doc_bytes);
    if (!same(hit_groups(rd, hd), hit_groups(od, hd)) || whole(rd, D) != whole(od, D)) bad_dc++;
    if (!sound(rd, hd, D, bound, doc_bytes)) bad_sound++;
    multi += r.size() > 1;
    for (const DocRange &g : r) solos += g.solo;
  }
  std::printf("%llu cases: %llu with several ranges, %llu solo ranges\n", (unsigned long long)n_cases, (unsigned long long)multi,
              (unsigned long long)solos);
  check("the sweep cuts batches and meets oversized documents", multi > n_cases / 4 && solos > n_cases / 4);
  check("class counts: the range list is the loop's", bad_cls == 0);
  check("select: the tiled range list is the loop's", bad_sel == 0);
  check("doc counts: the groups of documents with hits, the solo flags and the whole-batch cases are the loop's", bad_dc == 0);
  check("ascending, disjoint; a document with hits in exactly one range; solo = one document; a range's cost within the bound",
        bad_sound == 0);

  // ---- by hand ----
  const uint64_t G = 1ull << 32;
  check("D = 0", rule({0}, 12).empty() && rule({7}, 12).empty());
  check("all documents hitless", rule({0, 0, 0, 0}, 12).empty() && rule({5, 5, 5}, 1000).empty());
  check("one oversized document between hitless ones", same(rule({0, 0, 0, 9, 9, 9}, 96), {{2, 3, true}}));
  check("an oversized last document", same(rule({0, 2, 4, 4, 50}, 48), {{0, 3, false}, {3, 4, true}}));
  check("the bound exactly met: one range, the caller's batch",
        same(rule({0, 0, 3, 3, 8}, 96), {{0, 4, false}}) && same(rule({0, 0, 3, 3, 9}, 96), {{1, 3, false}, {3, 4, false}}));
  check("the bound exactly met by one document: not solo", same(rule({0, 1, 2}, 12), {{0, 1, false}, {1, 2, false}}));
  check("hitless documents come along behind, never in front",
        same(rule({0, 0, 5, 5, 5, 10, 10}, 60), {{1, 4, false}, {4, 6, false}}));
  check("hit offsets above 2^32",
        same(rule({G, G + 2, G + 2, 3 * G, 3 * G + 1}, 48), {{0, 2, false}, {2, 3, true}, {3, 4, false}}) &&
            same(rule({0, G, 2 * G + 5}, 12 * G), {{0, 1, false}, {1, 2, true}}) && same(rule({0, G, 2 * G}, 24 * G), {{0, 2, false}}));
  check("select's tiling: every document in a range, the hitless head and tail too",
        tiled(rule({0, 0, 0, 9, 9, 9}, 96), 5) == Offs({0, 5}) && tiled(rule({0, 0, 5, 5, 5, 10, 10}, 60), 6) == Offs({0, 4, 6}) &&
            tiled(rule({0, 0, 0}, 60), 2) == Offs({0}));
  {
    // a cost with pair bytes: 3 hits cost 36 + 24 in the range form, 2 hits 24 in the sort form
    auto cost = [](uint64_t h) { return h * kHit + (h > 2 && h < 6 ? std::min<uint64_t>(h, 7) * 8 : 0); };
    Ranges r;
    aha::doc_ranges(Offs{0, 3, 5, 8}.data(), 3, 84, cost, r);
    check("doc counts' cost counts the pairs", same(r, {{0, 2, false}, {2, 3, false}}));
    aha::doc_ranges(Offs{0, 3, 5, 8}.data(), 3, 59, cost, r);
    check("doc counts' cost makes a document solo", same(r, {{0, 1, true}, {1, 2, false}, {2, 3, true}}));
  }
  if (fails) std::printf("%d FAILED\n", fails);
  return fails ? 1 : 0;
}
