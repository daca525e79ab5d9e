// spec_feed_longest.cpp -- the shared step of match_longest (aha_amd/csrc/longest_step.hpp) as host code, driven the way the
// feed's kernels drive it (scan_feedlongest.hip): piece by piece, with the state, the pending end and the two bytes in front
// carried as values across every cut.  A small automaton image is built by hand here -- states numbered as the library places
// them: depth 1, depth 2, the deeper states whose fail target has depth <= 2 (no fail header: the shadow links of
// longest_fail_of), then the states with a header -- and the piecewise walks are compared with a plain restatement of the loop
// over trie nodes and true fail links that sees the whole text.  Built with -fsanitize=address,undefined by
// tests/test_feed_longest_host.py and run as its own process.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "../../aha_amd/csrc/longest_step.hpp"

using namespace aha;

namespace {

struct Trie {
  std::vector<std::map<uint8_t, int>> kids{1};
  std::vector<int> key{-1}, depth{0}, fail{0};
  std::vector<std::string> keys;
  void add(const std::string &k) {
    int s = 0;
    for (unsigned char c : k) {
      auto it = kids[s].find(c);
      if (it == kids[s].end()) {
        kids.emplace_back();
        key.push_back(-1);
        depth.push_back(depth[s] + 1);
        fail.push_back(0);
        it = kids[s].emplace(c, (int)kids.size() - 1).first;
      }
      s = it->second;
    }
    key[s] = (int)keys.size();
    keys.push_back(k);
  }
  void link() {
    std::vector<int> q;
    for (auto &e : kids[0]) q.push_back(e.second);
    for (size_t h = 0; h < q.size(); h++) {
      const int s = q[h];
      for (auto &e : kids[s]) {
        int f = fail[s];
        while (f && !kids[f].count(e.first)) f = fail[f];
        auto it = kids[f].find(e.first);
        const int t = it == kids[f].end() ? 0 : it->second;
        fail[e.second] = t == e.second ? 0 : t;
        q.push_back(e.second);
      }
    }
  }
};

// the image: state ids in the library's order; 0 is never a state (the root's id is n + 1, so "B == 0" bugs show)
struct Image {
  uint32_t root = 0, s1_lo = 0, s2_lo = 0, s2_hi = 0;
  const uint32_t *term_bits = nullptr, *stale_bits = nullptr;
  std::vector<uint32_t> term, stale, id_of, fail_id;  // fail_id[B]: header states only (others: poisoned)
  std::vector<int> node_of;
  std::map<std::pair<uint32_t, uint8_t>, uint32_t> go;
  std::vector<int> key_of;  // by id
};

struct HostProbe {
  static int go(const Image &A, uint32_t &B, uint32_t b, uint32_t &key) {
    auto it = A.go.find({B, (uint8_t)b});
    if (it == A.go.end()) return 0;
    B = it->second;
    if (A.key_of[B] >= 0) {
      key = (uint32_t)A.key_of[B];
      return 2;
    }
    return 1;
  }
  static uint32_t fail(const Image &A, uint32_t B) {
    if (A.fail_id[B] == 0xDEADu) {
      printf("spec_feed_longest: fail header of a headerless state %u read\n", B);
      exit(1);
    }
    return A.fail_id[B];
  }
  static uint32_t child_or_root(const Image &A, uint32_t B, uint32_t b) {
    auto it = A.go.find({B, (uint8_t)b});
    return it == A.go.end() ? A.root : it->second;
  }
};

Image build(const Trie &t, const std::vector<std::string> &stale_paths) {
  Image A;
  const int n = (int)t.kids.size();
  std::vector<int> order;
  auto cls = [&](int s) { return t.depth[s] == 1 ? 0 : t.depth[s] == 2 ? 1 : t.depth[t.fail[s]] <= 2 ? 2 : 3; };
  for (int c = 0; c < 4; c++)
    for (int s = 1; s < n; s++)
      if (cls(s) == c) order.push_back(s);
  A.id_of.assign(n, 0);
  A.node_of.assign(n + 2, -1);
  uint32_t next = 1, lo[5] = {1, 0, 0, 0, 0};
  int at = 0;
  for (int c = 0; c < 4; c++) {
    lo[c] = next;
    while (at < (int)order.size() && cls(order[at]) == c) {
      A.id_of[order[at]] = next;
      A.node_of[next] = order[at];
      next++;
      at++;
    }
  }
  lo[4] = next;
  A.root = next;  // above every range: the root owns a header
  A.id_of[0] = A.root;
  A.node_of[A.root] = 0;
  A.s1_lo = lo[1];
  A.s2_lo = lo[2];
  A.s2_hi = lo[3];
  A.key_of.assign(n + 2, -1);
  A.fail_id.assign(n + 2, 0xDEADu);
  A.term.assign((n + 2 + 31) / 32 + 1, 0);
  A.stale.assign((n + 2 + 31) / 32 + 1, 0);
  for (int s = 0; s < n; s++) {
    const uint32_t B = A.id_of[s];
    A.key_of[B] = t.key[s];
    if (s == 0 || cls(s) == 3) A.fail_id[B] = A.id_of[t.fail[s]];
    for (auto &e : t.kids[s]) A.go[{B, e.first}] = A.id_of[e.second];
    if (t.key[s] >= 0 && !t.kids[s].empty()) A.term[B >> 5] |= 1u << (B & 31);
  }
  for (auto &p : stale_paths) {
    int s = 0;
    for (unsigned char c : p) s = t.kids[s].at(c);
    const uint32_t B = A.id_of[s];
    A.stale[B >> 5] |= 1u << (B & 31);
  }
  A.term_bits = A.term.data();
  A.stale_bits = A.stale.data();
  return A;
}

struct Hit {
  int64_t start, end;
  int key;
  bool operator==(const Hit &o) const { return start == o.start && end == o.end && key == o.key; }
};

// the loop over trie nodes and true fail links, the whole text at once (tests/pymodel.py match_longest)
std::vector<Hit> whole(const Trie &t, const std::vector<std::string> &stale_paths, const std::string &text, bool isect) {
  std::vector<char> stale(t.kids.size(), 0);
  for (auto &p : stale_paths) {
    int s = 0;
    for (unsigned char c : p) s = t.kids[s].at(c);
    stale[s] = 1;
  }
  std::vector<Hit> out;
  int nid = 0, prev_nid = -1;
  int64_t prev_i = -1;
  auto fetch = [&](int64_t i, int n) {
    if (n >= 0 && t.key[n] >= 0) out.push_back({i - (int64_t)t.keys[t.key[n]].size() + 1, i + 1, t.key[n]});
  };
  for (int64_t i = 0; i < (int64_t)text.size(); i++) {
    const uint8_t b = (uint8_t)text[i];
    for (;;) {
      if (nid == -2) {
        prev_i = -1;
        nid = 0;
        break;
      }
      if (b == 0 && t.key[nid] >= 0 && !t.kids[nid].empty()) {
        nid = -2;
        prev_i = i;
        prev_nid = -2;
        break;
      }
      auto it = b ? t.kids[nid].find(b) : t.kids[nid].end();
      if (it != t.kids[nid].end()) {
        nid = it->second;
        if (t.key[nid] >= 0 || stale[nid]) {
          prev_i = i;
          prev_nid = nid;
        }
        break;
      }
      if (prev_i != -1) {
        fetch(prev_i, prev_nid);
        prev_i = -1;
        if (!isect) nid = 0;
      }
      if (nid == 0) break;
      nid = t.fail[nid];
    }
  }
  if (prev_i != -1) fetch(prev_i, prev_nid);
  return out;
}

// what a feed carries per sequence (FeedLongSeq): the state, the pending end as a distance back, its key, the last two bytes
struct Carried {
  uint32_t B;
  uint32_t back = 0, key = 0;
  LongestPrevRegs prev;
};

constexpr int64_t kBias = 1ll << 32;

// one piece, copied into a buffer of exactly its size so that any look in front of it or behind it is an ASan report
void piece(const Image &A, Carried &c, const std::string &whole_text, size_t n0, size_t n1, bool isect, std::vector<Hit> &out) {
  std::vector<uint8_t> buf(whole_text.begin() + n0, whole_text.begin() + n1);
  uint32_t B = c.B;
  Pending pend, y;
  pend.p = c.back ? kBias - (int64_t)c.back : -1;
  pend.key = c.key;
  LongestPrevRegs prev = c.prev;
  for (size_t p = 0; p < buf.size(); p++) {
    const uint32_t b = buf[p];
    if (longest_step<HostProbe>(A, B, b, prev, kBias + (int64_t)p, 0u, isect, pend, &y) && y.key != kNoKey) {
      const int64_t end = (int64_t)n0 + (y.p - kBias) + 1;
      out.push_back({0, end, (int)y.key});
    }
    prev.push(b);
  }
  c.B = B;
  c.back = pend.p >= 0 ? (uint32_t)(kBias + (int64_t)buf.size() - pend.p) : 0u;
  c.key = pend.p >= 0 ? pend.key : 0u;
  c.prev = prev;
}

void finish(const Carried &c, size_t n, std::vector<Hit> &out) {
  if (c.back && c.key != kNoKey) out.push_back({0, (int64_t)n - (int64_t)c.back + 1, (int)c.key});
}

int check(const char *what, const Trie &t, const std::vector<Hit> &want, std::vector<Hit> got) {
  for (auto &h : got) h.start = h.end - (int64_t)t.keys[h.key].size();
  if (got.size() == want.size() && std::equal(got.begin(), got.end(), want.begin())) return 0;
  printf("spec_feed_longest: %s differs (%zu hits, want %zu)\n", what, got.size(), want.size());
  return 1;
}

int run(const std::vector<std::string> &keys, const std::vector<std::string> &stale_paths, const std::string &text) {
  Trie t;
  for (auto &k : keys) t.add(k);
  t.link();
  const Image A = build(t, stale_paths);
  int bad = 0;
  for (int isect = 0; isect < 2; isect++) {
    const std::vector<Hit> want = whole(t, stale_paths, text, isect != 0);
    for (size_t cut = 0; cut <= text.size(); cut++) {  // every two-piece cut
      Carried c;
      c.B = A.root;
      std::vector<Hit> got;
      piece(A, c, text, 0, cut, isect != 0, got);
      // (the calls up to the cut plus a finish there are the whole of the prefix)
      std::vector<Hit> pre = got;
      finish(c, cut, pre);
      bad += check("prefix", t, whole(t, stale_paths, text.substr(0, cut), isect != 0), pre);
      piece(A, c, text, cut, text.size(), isect != 0, got);
      finish(c, text.size(), got);
      bad += check("two pieces", t, want, got);
    }
    Carried c;  // byte by byte, an empty piece in front of every byte
    c.B = A.root;
    std::vector<Hit> got;
    for (size_t i = 0; i < text.size(); i++) {
      piece(A, c, text, i, i, isect != 0, got);
      piece(A, c, text, i, i + 1, isect != 0, got);
    }
    finish(c, text.size(), got);
    bad += check("byte by byte", t, want, got);
  }
  return bad;
}

}  // namespace

int main() {
  int bad = 0;
  // nested keys: deep states whose fail targets have depth <= 2 (shadow links) and deeper (headers); "ab" ends a key and has
  // children (a NUL behind it reaches the value node); a stale END on "abc" and on "b"
  const std::vector<std::string> keys = {"a", "ab", "abcd", "abcde", "bcdx", "cd", "cde", "bcdeab", "deabc", "eabcdx", "xyz", "zz"};
  const std::vector<std::string> stale = {"abc", "b"};
  const std::string nul(1, '\0');
  bad += run(keys, stale, "abcdeabcdxabcdeabq" + nul + "abcdab" + nul + "cdeabcdx" + nul + nul + "bcdeabcdezzxyzabcab" + nul);
  bad += run(keys, {}, "xabcdeabcdeabcdxyzzzabcbcdeabcdeab");
  bad += run({"a"}, {}, "aaa" + nul + "a" + nul + nul + "a");
  bad += run({"aaaa", "aa", "a", "aaaaaaa"}, {"aaa"}, "aaaaaaaaaaaa" + nul + "aaaab" + nul + "aaaaaaaaa");
  if (bad) {
    printf("spec_feed_longest: %d FAILED\n", bad);
    return 1;
  }
  printf("spec_feed_longest: ok\n");
  return 0;
}
