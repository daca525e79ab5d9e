// foldk_stubs.cpp -- link-time stand-in for the launcher a handle compiled with AHA_OPT_FOLD_KANA adds: the staged copy that
// folds every document on its own with foldk (scan_foldk.hip), beside fold3_stubs.cpp in the sanitizer build of the host side
// (aha_amd/csrc/Makefile, target asan): every test there runs HOST_ONLY, where no launcher is ever reached.
#include <cstdio>
#include <cstdlib>

#include <hip/hip_runtime_api.h>

#include "../../aha_amd/csrc/image.hpp"

namespace aha {
void foldk_launch_copy(const uint8_t *, uint8_t *, uint64_t, const uint64_t *, uint64_t, uint32_t, void *) {
  fprintf(stderr, "sanitizer build: foldk_launch_copy reached (host-only library)\n");
  abort();
}
}  // namespace aha
