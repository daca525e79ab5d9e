// token_stubs.cpp -- link-time stand-ins for the token path's kernel launchers (scan_tokens.hip), beside kernel_stubs.cpp in
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
void tokens_launch_spans(const uint64_t *, uint64_t, const uint32_t *, uint32_t *, uint32_t, void *) { no_gpu("tokens_launch_spans"); }
void tokens_launch_starts(const uint8_t *, uint64_t, const uint32_t *, const uint32_t *, const uint32_t *, bool, uint32_t *, uint32_t,
                          void *) {
  no_gpu("tokens_launch_starts");
}
void tokens_launch_emit(const uint32_t *, uint64_t, const uint64_t *, const uint32_t *, const uint32_t *, const uint64_t *,
                        const uint64_t *, uint64_t, void *, uint32_t, void *) {
  no_gpu("tokens_launch_emit");
}
}  // namespace aha
