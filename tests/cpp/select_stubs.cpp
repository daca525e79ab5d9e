// select_stubs.cpp -- link-time stand-ins for the select path's kernel launchers (scan_select.hip), beside kernel_stubs.cpp in
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
uint64_t select_rank_blocks(uint64_t n_bytes) { return ((n_bytes + 31) / 32 + 63) / 64; }
void select_launch_longest(const void *, uint64_t, const uint64_t *, const uint64_t *, uint64_t, uint64_t, uint64_t *, uint32_t, void *) {
  no_gpu("select_launch_longest");
}
void select_launch_marks(const uint64_t *, uint64_t, const uint64_t *, uint64_t, uint32_t *, uint32_t *, uint32_t, void *) {
  no_gpu("select_launch_marks");
}
void select_launch_walk(const uint64_t *, uint64_t, const uint32_t *, const uint32_t *, uint32_t *, uint32_t, void *) {
  no_gpu("select_launch_walk");
}
void select_launch_rank(const uint32_t *, uint64_t, uint64_t *, uint32_t, void *) { no_gpu("select_launch_rank"); }
void select_launch_rank_docs(const uint32_t *, const uint64_t *, const uint64_t *, uint64_t, uint64_t, uint64_t *, uint32_t, void *) {
  no_gpu("select_launch_rank_docs");
}
void select_launch_emit(const uint32_t *, uint64_t, const uint64_t *, const uint64_t *, const uint64_t *, uint64_t, void *, uint32_t,
                        void *) {
  no_gpu("select_launch_emit");
}
}  // namespace aha
