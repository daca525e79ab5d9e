// feed_replace_stubs.cpp -- link-time stand-ins for the feed replace launchers (scan_feedreplace.hip), beside
// feed_select_stubs.cpp and replace_stubs.cpp in the sanitizer build of the host side (aha_amd/csrc/Makefile, target asan):
// every test there runs HOST_ONLY, where no launcher is ever reached (aha_feed_open refuses a host-only handle).
#include <cstdio>
#include <cstdlib>

#include "../../aha_amd/csrc/feed.hpp"

namespace aha {
[[noreturn]] static void no_gpu(const char *what) {
  fprintf(stderr, "sanitizer build: %s reached (host-only library)\n", what);
  abort();
}
void feedrep_launch_layout(const FeedArgs &, const FeedSelArgs &, const FeedRepArgs &, void *) { no_gpu("feedrep_launch_layout"); }
void feedrep_launch_stage(const FeedArgs &, const FeedRepArgs &, uint64_t, uint32_t, void *) { no_gpu("feedrep_launch_stage"); }
}  // namespace aha
