// grep_lines_stubs.cpp -- link-time stand-ins for the context-lines path's kernel launchers (scan_greplines.hip), beside
// kernel_stubs.cpp in the sanitizer build of the host side (aha_amd/csrc/Makefile, target asan): every test there runs HOST_ONLY,
// where no launcher is ever reached.
#include <cstdio>
#include <cstdlib>

#include <hip/hip_runtime_api.h>

#include "../../aha_amd/csrc/image.hpp"

namespace aha {
[[noreturn]] static void no_gpu(const char *what) {
  fprintf(stderr, "sanitizer build: %s reached (host-only library)\n", what);
  abort();
}
void greplines_launch_edges(const uint32_t *, uint64_t, const uint64_t *, uint64_t, uint32_t *, uint32_t *, uint32_t, void *) {
  no_gpu("greplines_launch_edges");
}
void greplines_launch_windows(const uint32_t *, const uint32_t *, uint64_t, const uint64_t *, const uint64_t *, const uint64_t *,
                              uint64_t, uint32_t, uint32_t, uint64_t, uint64_t *, uint64_t *, uint64_t *, uint32_t *, uint32_t,
                              void *) {
  no_gpu("greplines_launch_windows");
}
void greplines_launch_fill(const uint32_t *, const uint64_t *, uint64_t, uint32_t *, uint32_t, void *) {
  no_gpu("greplines_launch_fill");
}
void greplines_launch_emit_match(const uint32_t *, const uint64_t *, uint64_t, const uint32_t *, uint8_t *, uint32_t, void *) {
  no_gpu("greplines_launch_emit_match");
}
}  // namespace aha
