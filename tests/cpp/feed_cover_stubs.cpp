// feed_cover_stubs.cpp -- link-time stand-in for the feed cover launcher (scan_feed.hip), beside feed_stubs.cpp in the
// sanitizer build of the host side (aha_amd/csrc/Makefile, target asan): every test there runs HOST_ONLY, where no launcher
// is ever reached (aha_feed_open refuses a host-only handle).
#include <cstdio>
#include <cstdlib>

#include "../../aha_amd/csrc/feed.hpp"

namespace aha {
void feed_launch_cover(const FeedArgs &, void *) {
  fprintf(stderr, "sanitizer build: feed_launch_cover reached (host-only library)\n");
  abort();
}
}  // namespace aha
