// class_count_stubs.cpp -- link-time stand-ins for the class-counts path's kernel launchers (scan_classcount.hip), beside
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
void classcount_launch_add(const void *, uint64_t, const uint64_t *, uint64_t, const uint64_t *, const uint32_t *, uint32_t, uint32_t,
                           uint32_t *, uint32_t, void *) {
  no_gpu("classcount_launch_add");
}
void classcount_launch_fold_keys(const uint64_t *, uint32_t, const uint64_t *, const uint32_t *, uint32_t *, uint32_t, void *) {
  no_gpu("classcount_launch_fold_keys");
}
}  // namespace aha
