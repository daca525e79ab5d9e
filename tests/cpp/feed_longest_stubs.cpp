// feed_longest_stubs.cpp -- link-time stand-ins for the launchers of a longest feed (scan_feedlongest.hip), beside
// feed_stubs.cpp and feed_sep_stubs.cpp in the sanitizer build of the host side (aha_amd/csrc/Makefile, target asan): every test
// there runs HOST_ONLY, where no launcher is ever reached (aha_feed_open_params refuses a host-only handle once its arguments are
// checked).
#include <cstdio>
#include <cstdlib>

#include "../../aha_amd/csrc/feed.hpp"

namespace aha {
[[noreturn]] static void no_gpu(const char *what) {
  fprintf(stderr, "sanitizer build: %s reached (host-only library)\n", what);
  abort();
}
void feedlong_launch_walk(const DevAut &, const MatchArgs &, const FeedArgs &, const FeedLongArgs &, bool, bool, bool, void *) {
  no_gpu("feedlong_launch_walk");
}
void feedlong_launch_commit(const FeedArgs &, const FeedLongArgs &, void *) { no_gpu("feedlong_launch_commit"); }
void feedlong_launch_finish(const FeedArgs &, const FeedLongArgs &, const void *, bool, void *) { no_gpu("feedlong_launch_finish"); }
}  // namespace aha
