// The overflow predicate of the class-counts calls (aha_amd/csrc/class_overflow.hpp) on made-up hit offsets: the branch it guards
// needs a batch of 2^32 hits, so it is tested here and not on a device.  Built and run by tests/test_class_counts_host.py.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../aha_amd/csrc/class_overflow.hpp"

static int fails = 0;
static void check(const char *name, bool ok) {
  std::printf("%s %s\n", ok ? "ok  " : "FAIL", name);
  if (!ok) fails++;
}

int main() {
  using Offs = std::vector<uint64_t>;
  const uint64_t G = 1ull << 32;
  uint64_t doc = 99;
  auto over = [&](const Offs &o) { return aha::class_counts_overflow(o.data(), o.size() - 1, &doc); };
  check("no document", !over({0}) && doc == 99);
  check("a small batch", !over({0, 5, 5, 9}) && doc == 99);
  check("2^32 - 1 hits in one document", !over({0, G - 1}));
  check("2^32 hits in one document", over({0, G}) && doc == 0);
  doc = 99;
  check("2^32 hits in all, none of the documents has them", !over({0, G - 1, G - 1, 2 * G - 2}) && doc == 99);
  check("the second document of a large batch", over({0, G - 1, 2 * G - 1, 2 * G}) && doc == 1);
  check("the last document", over({7, 8, 8, 9 + G}) && doc == 2);
  check("offsets that do not start at 0", !over({G, G + 3, 2 * G + 2}) && over({G, 2 * G}));
  check("the first of two", over({0, G, 3 * G}) && doc == 0);
  check("without the document asked for", aha::class_counts_overflow(Offs{0, G}.data(), 1));
  if (fails) std::printf("%d FAILED\n", fails);
  return fails ? 1 : 0;
}
