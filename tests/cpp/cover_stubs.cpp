// cover_stubs.cpp -- link-time stand-ins for the cover path's kernel launchers (scan_cover.hip), beside kernel_stubs.cpp in the
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
void cover_launch_clear(uint32_t *, uint64_t, const unsigned long long *, uint32_t, void *) { no_gpu("cover_launch_clear"); }
void cover_launch_spans(const DevAut &, const V2Args &, const uint2 *, uint64_t *, uint32_t *, uint64_t, uint32_t, void *) {
  no_gpu("cover_launch_spans");
}
void cover_launch_redact(const uint8_t *, uint8_t *, const uint32_t *, uint64_t, uint8_t, uint32_t, void *) {
  no_gpu("cover_launch_redact");
}
void cover_launch_doc_covered(const uint32_t *, const uint64_t *, uint64_t, uint64_t *, uint32_t, void *) {
  no_gpu("cover_launch_doc_covered");
}
void cover_launch_total(const uint32_t *, uint64_t, uint64_t *, uint32_t, void *) { no_gpu("cover_launch_total"); }
}  // namespace aha
