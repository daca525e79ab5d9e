// grep_rule_stubs.cpp -- link-time stand-ins for rule grep's kernel launchers (scan_greprule.hip), beside kernel_stubs.cpp in the
// sanitizer build of the host side (aha_amd/csrc/Makefile, target asan): every test there runs HOST_ONLY, where no launcher is
// ever reached.
#include <cstdio>
#include <cstdlib>

#include <hip/hip_runtime_api.h>

#include "../../aha_amd/csrc/image.hpp"

namespace aha {
[[noreturn]] static void no_gpu(const char *what) {
  fprintf(stderr, "sanitizer build: %s reached (host-only library)\n", what);
  abort();
}
void greprule_launch_keep(const uint32_t *, uint32_t, const uint64_t *, uint64_t, const aha_rule_term *, uint32_t, bool, uint32_t *,
                          uint32_t, void *) {
  no_gpu("greprule_launch_keep");
}
void greprule_launch_edges(const uint32_t *, uint64_t, uint32_t *, uint32_t *, uint32_t, void *) { no_gpu("greprule_launch_edges"); }
}  // namespace aha
