// grep_stubs.cpp -- link-time stand-ins for the records and grep paths' kernel launchers (scan_grep.hip), beside kernel_stubs.cpp
// in the sanitizer build of the host side (aha_amd/csrc/Makefile, target asan): every test there runs HOST_ONLY, where no
// launcher is ever reached.
#include <cstdio>
#include <cstdlib>

#include <hip/hip_runtime_api.h>

#include "../../aha_amd/csrc/image.hpp"

namespace aha {
[[noreturn]] static void no_gpu(const char *what) {
  fprintf(stderr, "sanitizer build: %s reached (host-only library)\n", what);
  abort();
}
void grep_launch_ends(const uint8_t *, uint64_t, uint8_t, const uint64_t *, uint64_t, uint32_t *, uint32_t, void *) {
  no_gpu("grep_launch_ends");
}
void grep_launch_emit_ends(const uint32_t *, uint64_t, const uint64_t *, uint64_t *, uint32_t, void *) { no_gpu("grep_launch_emit_ends"); }
void grep_launch_flag(const uint64_t *, uint64_t, bool, uint32_t *, uint32_t *, uint32_t *, uint32_t, void *) { no_gpu("grep_launch_flag"); }
void grep_launch_runs(const uint32_t *, const uint32_t *, uint64_t, const uint64_t *, const uint64_t *, const uint64_t *, uint64_t,
                      uint64_t *, int64_t *, void *, RepEntry *, uint32_t, void *) {
  no_gpu("grep_launch_runs");
}
void grep_launch_emit_docs(const uint32_t *, const uint32_t *, uint64_t, const uint64_t *, const uint64_t *, const uint64_t *,
                           const int64_t *, uint64_t, uint64_t *, uint64_t *, uint32_t, void *) {
  no_gpu("grep_launch_emit_docs");
}
}  // namespace aha
