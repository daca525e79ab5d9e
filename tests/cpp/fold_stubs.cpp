// fold_stubs.cpp -- link-time stand-ins for the launchers a folded handle (AHA_OPT_FOLD_ASCII) adds: the staged copy
// (scan_fold.hip) and the folding forms of the prefix-filter engine's launches (scan_filter.hip), beside kernel_stubs.cpp in the
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
void fold_launch_copy(const uint8_t *, uint8_t *, uint64_t, uint32_t, void *) { no_gpu("fold_launch_copy"); }
void filter_launch_filter_fold(const FilterDev &, const V2Args &, void *, void *, unsigned long long *, uint32_t, void *) {
  no_gpu("filter_launch_filter_fold");
}
void filter_launch_walk_fold(const DevAut &, const V2Args &, const void *, const void *, const unsigned long long *, uint32_t, void *) {
  no_gpu("filter_launch_walk_fold");
}
}  // namespace aha
