// doc_count_stubs.cpp -- link-time stand-ins for the document counts' kernel launchers (scan_doccount.hip), beside
// kernel_stubs.cpp in the sanitizer build of the host side (aha_amd/csrc/Makefile, target asan): every test there runs
// HOST_ONLY, where no launcher is ever reached.
#include <cstdio>
#include <cstdlib>

#include <hip/hip_runtime_api.h>

#include "../../aha_amd/csrc/image.hpp"

namespace aha {
[[noreturn]] static void no_gpu(const char *what) {
  fprintf(stderr, "sanitizer build: %s reached (host-only library)\n", what);
  abort();
}
void doccount_launch_sort(const DcItem *, uint32_t, const void *, uint32_t *, void *) { no_gpu("doccount_launch_sort"); }
void doccount_launch_range(const DcItem *, uint32_t, const void *, uint32_t, uint32_t, uint32_t *, void *) {
  no_gpu("doccount_launch_range");
}
void doccount_launch_add(const DcItem *, uint32_t, const void *, uint32_t *, uint32_t, uint32_t, void *) {
  no_gpu("doccount_launch_add");
}
void doccount_launch_compact(const DcItem *, uint32_t, uint32_t *, uint32_t, uint32_t *, void *) { no_gpu("doccount_launch_compact"); }
void doccount_launch_compact64(const DcItem *, unsigned long long *, uint32_t, uint32_t *, void *) {
  no_gpu("doccount_launch_compact64");
}
void doccount_launch_gather(const uint64_t *, const uint32_t *const *, uint64_t, uint64_t, void *, void *) {
  no_gpu("doccount_launch_gather");
}
}  // namespace aha
