// replace_stubs.cpp -- link-time stand-ins for the replace path's kernel launchers (scan_replace.hip), beside kernel_stubs.cpp in
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
void replace_launch_delta(const void *, uint64_t, const uint64_t *, const uint64_t *, uint64_t, const RepEntry *, uint32_t, uint64_t *,
                          int64_t *, uint32_t, void *) {
  no_gpu("replace_launch_delta");
}
void replace_launch_scan(int64_t *, uint64_t, int64_t *, uint32_t, void *) { no_gpu("replace_launch_scan"); }
void replace_launch_doc_offsets(const uint64_t *, const uint64_t *, const int64_t *, uint64_t, uint64_t *, uint32_t, void *) {
  no_gpu("replace_launch_doc_offsets");
}
void replace_launch_copy(const uint8_t *, const void *, const uint64_t *, const int64_t *, uint64_t, const RepEntry *, uint32_t,
                         const uint8_t *, uint8_t *, uint64_t, uint32_t, void *) {
  no_gpu("replace_launch_copy");
}
}  // namespace aha
