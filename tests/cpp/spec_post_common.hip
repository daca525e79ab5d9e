// spec_post_common.hip -- every helper of aha_amd/csrc/post_common.hpp in a tiny kernel, against plain host loops.  Exits
// non-zero with a message at the first difference.  Built and run by tests/test_post_common_cpp.py.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../../aha_amd/csrc/post_common.hpp"

using namespace aha;
typedef unsigned long long u64;

#define HIP_OK(x)                                                                         \
  do {                                                                                    \
    const hipError_t e_ = (x);                                                            \
    if (e_ != hipSuccess) {                                                               \
      printf("%s:%d: %s: %s\n", __FILE__, __LINE__, #x, hipGetErrorString(e_));           \
      exit(2);                                                                            \
    }                                                                                     \
  } while (0)

static void fail(const std::string &what) {
  printf("FAIL %s\n", what.c_str());
  exit(1);
}

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t rnd() {  // xorshift64*
  rng_state ^= rng_state >> 12, rng_state ^= rng_state << 25, rng_state ^= rng_state >> 27;
  return rng_state * 0x2545F4914F6CDD1Dull;
}

// a device copy of a host vector (never of size 0), freed with the object
template <class T>
struct Dev {
  T *p = nullptr;
  size_t n;
  explicit Dev(size_t n_) : n(n_) {
    HIP_OK(hipMalloc((void **)&p, (n ? n : 1) * sizeof(T)));
    HIP_OK(hipMemset(p, 0, (n ? n : 1) * sizeof(T)));
  }
  explicit Dev(const std::vector<T> &v) : Dev(v.size()) {
    if (n) HIP_OK(hipMemcpy(p, v.data(), n * sizeof(T), hipMemcpyHostToDevice));
  }
  ~Dev() { (void)hipFree(p); }
  std::vector<T> get() const {
    std::vector<T> v(n);
    HIP_OK(hipDeviceSynchronize());
    if (n) HIP_OK(hipMemcpy(v.data(), p, n * sizeof(T), hipMemcpyDeviceToHost));
    return v;
  }
};

// ------------------------------------------------------------------ owner_of
__global__ void k_owner(const uint64_t *off, uint64_t n, const uint64_t *xs, uint64_t nx, uint64_t sub, uint64_t *out) {
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < nx; i += (uint64_t)gridDim.x * blockDim.x)
    out[i] = sub ? owner_of(off, n, xs[i], sub) : owner_of(off, n, xs[i]);
}

// rel: an ascending table with rel[0] = 0; it is searched as it is (sub = 0) and moved up by `base` (sub = off[0] = base)
static void check_owner(const char *name, const std::vector<uint64_t> &rel, uint64_t base) {
  const uint64_t n = rel.size();
  std::vector<uint64_t> off(n), xs;
  for (uint64_t d = 0; d < n; d++) {
    off[d] = rel[d] + base;
    if (rel[d]) xs.push_back(rel[d] - 1);  // one before, on and one behind every entry
    xs.push_back(rel[d]);
    xs.push_back(rel[d] + 1);
  }
  Dev<uint64_t> d_off(off), d_xs(xs), d_out(xs.size());
  hipLaunchKernelGGL(k_owner, dim3(2), dim3(256), 0, 0, d_off.p, n, d_xs.p, (uint64_t)xs.size(), base, d_out.p);
  const std::vector<uint64_t> got = d_out.get();
  for (size_t i = 0; i < xs.size(); i++) {
    uint64_t want = 0;
    for (uint64_t d = 0; d < n; d++)
      if (off[d] - base <= xs[i]) want = d;
    if (got[i] != want)
      fail(std::string("owner_of ") + name + " sub " + std::to_string(base) + ": x " + std::to_string(xs[i]) + " -> " +
           std::to_string(got[i]) + ", want " + std::to_string(want));
  }
}

static void spec_owner() {
  std::vector<uint64_t> big(1000);
  big[0] = 0, big[1] = 0;  // equal neighbours first ...
  for (size_t d = 2; d < big.size(); d++) big[d] = big[d - 1] + (rnd() % 3 == 0 ? 0 : rnd() % 4 * 2);  // ... in the middle ...
  big[999] = big[998] = big[997];                                                                      // ... and last
  const std::vector<std::pair<const char *, std::vector<uint64_t>>> tables = {
      {"n=1", {0}},           {"n=2", {0, 5}},        {"n=2 equal", {0, 0}},       {"n=3", {0, 2, 5}},
      {"n=3 first", {0, 0, 4}}, {"n=3 last", {0, 3, 3}}, {"n=3 all", {0, 0, 0}},   {"n=4 middle", {0, 3, 3, 6}},
      {"n=1000", big}};
  for (const auto &t : tables) {
    check_owner(t.first, t.second, 0);
    check_owner(t.first, t.second, 77);
  }
}

// --------------------------------------------------------------------- wave
template <class T>
__global__ void k_wave(const T *in, T *sum, T *excl) {
  const T v = in[threadIdx.x];
  sum[threadIdx.x] = wave_sum(v);
  excl[threadIdx.x] = wave_excl_scan(v);
}
__global__ void k_wave_max(const uint32_t *in, uint32_t *mx) { mx[threadIdx.x] = wave_max(in[threadIdx.x]); }

template <class T>
static void check_wave(const char *name, const std::vector<T> &v) {
  Dev<T> d_in(v), d_sum(64), d_excl(64);
  hipLaunchKernelGGL(k_wave<T>, dim3(1), dim3(64), 0, 0, d_in.p, d_sum.p, d_excl.p);
  const std::vector<T> sum = d_sum.get(), excl = d_excl.get();
  T run = 0, total = 0;
  for (int l = 0; l < 64; l++) total += v[l];
  for (int l = 0; l < 64; l++) {
    if (sum[l] != total) fail(std::string("wave_sum ") + name + ": lane " + std::to_string(l) + " has " + std::to_string(sum[l]) + ", want " + std::to_string(total));
    if (excl[l] != run) fail(std::string("wave_excl_scan ") + name + ": lane " + std::to_string(l) + " has " + std::to_string(excl[l]) + ", want " + std::to_string(run));
    run += v[l];
  }
}

static void check_wave_max(const char *name, const std::vector<uint32_t> &v) {
  Dev<uint32_t> d_in(v), d_mx(64);
  hipLaunchKernelGGL(k_wave_max, dim3(1), dim3(64), 0, 0, d_in.p, d_mx.p);
  const std::vector<uint32_t> mx = d_mx.get();
  uint32_t want = 0;
  for (int l = 0; l < 64; l++) want = v[l] > want ? v[l] : want;
  for (int l = 0; l < 64; l++)
    if (mx[l] != want) fail(std::string("wave_max ") + name + ": lane " + std::to_string(l) + " has " + std::to_string(mx[l]) + ", want " + std::to_string(want));
}

static void spec_wave() {
  std::vector<uint32_t> zero(64, 0u), full(64, 0x03FFFFFFu), r32(64), one(64, 0u);  // (64 x 0x03FFFFFF stays below 2^32)
  for (auto &x : r32) x = (uint32_t)rnd() & 0x03FFFFFFu;
  one[37] = 9;  // the maximum in one lane only
  check_wave<uint32_t>("zero", zero), check_wave<uint32_t>("0x03FFFFFF", full), check_wave<uint32_t>("random", r32);
  check_wave_max("zero", zero), check_wave_max("0x03FFFFFF", full), check_wave_max("random", r32), check_wave_max("one lane", one);
  std::vector<u64> r64(64);
  for (auto &x : r64) x = (1ull << 31) + (rnd() & 0xFFFFFFFFull);  // (the sum passes 2^32 after two lanes)
  check_wave<u64>("uint64", r64);
  std::vector<long long> rs(64);
  for (auto &x : rs) x = (long long)(rnd() % 2000001) - 1200000;  // mixed signs, a negative total
  check_wave<long long>("long long", rs);
}

// ----------------------------------------------------------- block_run_scan
template <int THREADS, class T>
__global__ __launch_bounds__(THREADS) void k_run_scan(const T *in, uint64_t n, T *out) {
  __shared__ T lds[THREADS];
  const T total = block_run_scan<THREADS>(
      n, [&](uint64_t i) { return in[i]; }, [&](uint64_t i, T run) { out[i] = run; }, lds);
  if (threadIdx.x == THREADS - 1) out[n] = total;
}

template <int THREADS, class T>
static void check_run_scan(const char *name, uint64_t n, T (*make)()) {
  std::vector<T> v(n);
  for (auto &x : v) x = make();
  Dev<T> d_in(v), d_out(n + 1);
  HIP_OK(hipMemset(d_out.p, 0xA5, (n + 1) * sizeof(T)));
  hipLaunchKernelGGL((k_run_scan<THREADS, T>), dim3(1), dim3(THREADS), 0, 0, d_in.p, n, d_out.p);
  const std::vector<T> got = d_out.get();
  T run = 0;
  for (uint64_t i = 0; i <= n; i++) {  // every prefix, and the total behind them
    if (got[i] != run)
      fail(std::string("block_run_scan<") + std::to_string(THREADS) + "> " + name + " n " + std::to_string(n) + ": [" + std::to_string(i) +
           "] = " + std::to_string(got[i]) + ", want " + std::to_string(run));
    if (i < n) run += v[i];
  }
}

static u64 make_u64() { return (1ull << 32) + (rnd() & 0xFFFFFFull); }                 // (one item passes 2^32)
static long long make_ll() { return (long long)(rnd() % 2000001) - 1500000; }           // mixed signs, negative totals

template <int THREADS>
static void spec_run_scan() {
  // (at 2 THREADS + 37 items per = 3: the lanes from ceil(n / 3) on have empty runs)
  for (uint64_t n : {(uint64_t)0, (uint64_t)1, (uint64_t)THREADS - 1, (uint64_t)THREADS, (uint64_t)THREADS + 1, (uint64_t)2 * THREADS + 37}) {
    check_run_scan<THREADS, u64>("uint64", n, make_u64);
    check_run_scan<THREADS, long long>("long long", n, make_ll);
  }
}

// ---------------------------------------------------------- for_ranked_bits
// pos[rank] = the bit's position, seen[rank] += 1; a rank beyond the total is counted, not stored
__global__ __launch_bounds__(256) void k_ranked(const uint32_t *words, uint64_t n_words, uint64_t n_blk, const u64 *blk, uint64_t total,
                                                u64 *pos, uint32_t *seen, uint32_t *beyond) {
  for_ranked_bits(words, n_words, n_blk, blk, [&](uint64_t w, uint32_t i, uint64_t rank) {
    if (rank < total) {
      pos[rank] = w * 32 + i;
      atomicAdd(seen + rank, 1u);
    } else {
      atomicAdd(beyond, 1u);
    }
  });
}

__global__ void k_bits(const uint32_t *mask, uint32_t *out) { out[threadIdx.x] = bit_at(mask, threadIdx.x) ? 1u : 0u; }

static void check_ranked(uint64_t n_words, uint32_t grid) {
  const uint64_t n_bits = n_words ? n_words * 32 - 13 : 0;  // the last word is partly used
  std::vector<uint32_t> words(n_words);
  for (uint64_t w = 0; w < n_words; w++) {
    const uint64_t b = w / kRankBlockWords;
    words[w] = (uint32_t)rnd() & (uint32_t)rnd();
    if (w == 0 || b == 1 || b == 3) words[w] = 0xFFFFFFFFu;  // an all-ones word; two full blocks ...
    if (b == 2) words[w] = 0u;                                // ... and an all-zero one between them
  }
  if (n_words) words[n_words - 1] &= 0xFFFFFFFFu >> 13;
  const uint64_t n_blk = rank_blocks(n_bits);
  if (n_blk != (n_words + 63) / 64) fail("rank_blocks(" + std::to_string(n_bits) + ") = " + std::to_string(n_blk));
  std::vector<u64> blk(n_blk + 1, 0), want;
  for (uint64_t w = 0; w < n_words; w++) {
    if (w % kRankBlockWords == 0) blk[w / kRankBlockWords] = want.size();
    for (uint32_t i = 0; i < 32; i++)
      if ((words[w] >> i) & 1u) want.push_back(w * 32 + i);
  }
  blk[n_blk] = want.size();
  Dev<uint32_t> d_words(words), d_seen(want.size()), d_beyond(1);
  Dev<u64> d_blk(blk), d_pos(want.size());
  hipLaunchKernelGGL(k_ranked, dim3(grid), dim3(256), 0, 0, d_words.p, n_words, n_blk, d_blk.p, (uint64_t)want.size(), d_pos.p, d_seen.p,
                     d_beyond.p);
  const std::string name = "for_ranked_bits " + std::to_string(n_words) + " words on " + std::to_string(grid) + " workgroups: ";
  if (d_beyond.get()[0]) fail(name + std::to_string(d_beyond.get()[0]) + " visits with a rank beyond the set bits");
  const std::vector<u64> pos = d_pos.get();
  const std::vector<uint32_t> seen = d_seen.get();
  for (size_t r = 0; r < want.size(); r++) {
    if (seen[r] != 1) fail(name + "rank " + std::to_string(r) + " visited " + std::to_string(seen[r]) + " times");
    if (pos[r] != want[r]) fail(name + "rank " + std::to_string(r) + " is bit " + std::to_string(pos[r]) + ", want " + std::to_string(want[r]));
  }
}

static void spec_ranked() {
  // (1 workgroup = 4 waves: at 6 blocks two of them take a second trip)
  for (uint64_t n_words : {0, 1, 63, 64, 65, 64 * 5 + 1})
    for (uint32_t grid : {1u, 3u}) check_ranked(n_words, grid);
  Dev<uint32_t> d_mask(std::vector<uint32_t>{0x80000001u, 0x00010000u}), d_bits(64);
  std::vector<uint32_t> bits(64);
  for (uint64_t p = 0; p < 64; p++) bits[p] = (p == 0 || p == 31 || p == 48) ? 1u : 0u;  // (bit 16 of word 1 is position 48)
  hipLaunchKernelGGL(k_bits, dim3(1), dim3(64), 0, 0, d_mask.p, d_bits.p);
  if (d_bits.get() != bits) fail("bit_at");
}

// ------------------------------------------------------------------ grid_for
static void spec_grid() {
  const struct {
    uint64_t units, per;
    uint32_t cap, want;
  } cases[] = {{0, 256, 1024, 1},     {1, 256, 1024, 1},          {256, 256, 1024, 1},      {257, 256, 1024, 2},
               {512, 256, 1024, 2},   {1024ull * 256, 256, 1024, 1024}, {1024ull * 256 + 1, 256, 1024, 1024}, {7 * 4 + 1, 4, 7, 7},
               {7 * 4, 4, 7, 7},      {6 * 4 + 1, 4, 7, 7},       {5, 1, 4096, 5},          {0, 1, 4096, 1},
               {1ull << 40, 256, 65535, 65535}, {9, 256, 0, 1}};
  for (const auto &c : cases) {
    const uint32_t got = post::grid_for(c.units, c.per, c.cap);
    if (got != c.want)
      fail("grid_for(" + std::to_string(c.units) + ", " + std::to_string(c.per) + ", " + std::to_string(c.cap) + ") = " + std::to_string(got) +
           ", want " + std::to_string(c.want));
  }
}

int main() {
  spec_grid();
  int n_dev = 0;
  HIP_OK(hipGetDeviceCount(&n_dev));
  if (!n_dev) fail("no device");
  spec_owner();
  spec_wave();
  spec_run_scan<256>();
  spec_run_scan<1024>();
  spec_ranked();
  HIP_OK(hipDeviceSynchronize());
  printf("spec_post_common ok\n");
  return 0;
}
