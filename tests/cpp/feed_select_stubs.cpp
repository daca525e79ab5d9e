// feed_select_stubs.cpp -- link-time stand-ins for the feed select launchers (scan_feedselect.hip), beside feed_stubs.cpp and
// select_stubs.cpp in the sanitizer build of the host side (aha_amd/csrc/Makefile, target asan): every test there runs
// HOST_ONLY, where no launcher is ever reached (aha_feed_open refuses a host-only handle).
#include <cstdio>
#include <cstdlib>

#include "../../aha_amd/csrc/feed.hpp"

namespace aha {
[[noreturn]] static void no_gpu(const char *what) {
  fprintf(stderr, "sanitizer build: %s reached (host-only library)\n", what);
  abort();
}
void feedsel_launch_layout(const FeedArgs &, const FeedSelArgs &, void *) { no_gpu("feedsel_launch_layout"); }
void feedsel_launch_longest(const FeedArgs &, const FeedSelArgs &, uint32_t, void *) { no_gpu("feedsel_launch_longest"); }
void feedsel_launch_walk(const FeedArgs &, const FeedSelArgs &, uint32_t, void *) { no_gpu("feedsel_launch_walk"); }
void feedsel_launch_emit(const FeedArgs &, const FeedSelArgs &, uint32_t, void *) { no_gpu("feedsel_launch_emit"); }
void feedsel_launch_commit(const FeedArgs &, const FeedSelArgs &, void *) { no_gpu("feedsel_launch_commit"); }
}  // namespace aha
