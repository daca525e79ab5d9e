// feed_stubs.cpp -- link-time stand-ins for the feed path's kernel launchers (scan_feed.hip), beside kernel_stubs.cpp in the
// sanitizer build of the host side (aha_amd/csrc/Makefile, target asan): every test there runs HOST_ONLY, where no launcher
// is ever reached (aha_feed_open refuses a host-only handle).
#include <cstdio>
#include <cstdlib>

#include "../../aha_amd/csrc/feed.hpp"

namespace aha {
[[noreturn]] static void no_gpu(const char *what) {
  fprintf(stderr, "sanitizer build: %s reached (host-only library)\n", what);
  abort();
}
void feed_launch_check(const FeedArgs &, void *) { no_gpu("feed_launch_check"); }
void feed_launch_windows(const FeedArgs &, void *) { no_gpu("feed_launch_windows"); }
void feed_launch_merge(const FeedArgs &, void *) { no_gpu("feed_launch_merge"); }
void feed_launch_commit(const FeedArgs &, void *) { no_gpu("feed_launch_commit"); }
}  // namespace aha
