// excerpt_stubs.cpp -- link-time stand-ins for the excerpts path's kernel launchers (scan_excerpt.hip), beside kernel_stubs.cpp in
// the sanitizer build of the host side (aha_amd/csrc/Makefile, target asan): every test there runs HOST_ONLY, where no launcher
// is ever reached.
#include <cstdio>
#include <cstdlib>

#include <hip/hip_runtime_api.h>

#include "../../aha_amd/csrc/image.hpp"

namespace aha {
[[noreturn]] static void no_gpu(const char *what) {
  fprintf(stderr, "sanitizer build: %s reached (host-only library)\n", what);
  abort();
}
void excerpt_launch_edges(const uint32_t *, uint64_t, const uint64_t *, uint64_t, uint32_t *, uint32_t *, uint32_t, void *) {
  no_gpu("excerpt_launch_edges");
}
void excerpt_launch_windows(const uint32_t *, const uint32_t *, uint64_t, const uint64_t *, const uint64_t *, const uint8_t *,
                            const uint64_t *, uint64_t, uint32_t, uint32_t, uint64_t, uint64_t *, uint64_t *, uint64_t *, uint32_t *,
                            uint32_t *, uint32_t, void *) {
  no_gpu("excerpt_launch_windows");
}
void excerpt_launch_gaps(const uint32_t *, const uint32_t *, uint64_t, const uint64_t *, const uint64_t *, const uint64_t *,
                         const uint64_t *, uint64_t, uint64_t, uint64_t *, int64_t *, void *, RepEntry *, uint32_t, void *) {
  no_gpu("excerpt_launch_gaps");
}
void excerpt_launch_emit(const uint64_t *, const int64_t *, uint64_t, uint64_t *, uint64_t *, uint32_t, void *) {
  no_gpu("excerpt_launch_emit");
}
}  // namespace aha
