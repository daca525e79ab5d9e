// count_stubs.cpp -- link-time stand-ins for the count path's kernel launchers (scan_count.hip and the count launchers of
// scan_v2.hip / scan_unit.hip), beside kernel_stubs.cpp in the sanitizer build of the host side (aha_amd/csrc/Makefile,
// target asan): every test there runs HOST_ONLY, where no launcher is ever reached.
#include <cstdio>
#include <cstdlib>

#include <hip/hip_runtime_api.h>

#include "../../aha_amd/csrc/image.hpp"

namespace aha {
[[noreturn]] static void no_gpu(const char *what) {
  fprintf(stderr, "sanitizer build: %s reached (host-only library)\n", what);
  abort();
}
void v2_launch_count_post(const DevAut &, const V2Args &, void *, bool) { no_gpu("v2_launch_count_post"); }
void v2_launch_doc_offsets(const DevAut &, const V2Args &, void *) { no_gpu("v2_launch_doc_offsets"); }
void unit_launch_doc_offsets(const V2Args &, void *) { no_gpu("unit_launch_doc_offsets"); }
void count_launch_visits(const DevAut &, const V2Args &, const uint2 *, unsigned long long *, uint32_t, void *) {
  no_gpu("count_launch_visits");
}
void launch_count_doc_offsets(const MatchArgs &, void *) { no_gpu("launch_count_doc_offsets"); }
void count_launch_chain(const uint2 *, uint32_t, const unsigned long long *, unsigned long long *, const unsigned long long *,
                        void *) {
  no_gpu("count_launch_chain");
}
}  // namespace aha
