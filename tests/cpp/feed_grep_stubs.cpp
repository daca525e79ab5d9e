// feed_grep_stubs.cpp -- link-time stand-ins for the feed grep launchers (scan_feedgrep.hip) and the check that stands alone
// (scan_feed.hip), beside feed_stubs.cpp and grep_stubs.cpp in the sanitizer build of the host side (aha_amd/csrc/Makefile,
// target asan): every test there runs HOST_ONLY, where no launcher is ever reached (aha_feed_open refuses a host-only handle).
#include <cstdio>
#include <cstdlib>

#include "../../aha_amd/csrc/feed.hpp"

namespace aha {
[[noreturn]] static void no_gpu(const char *what) {
  fprintf(stderr, "sanitizer build: %s reached (host-only library)\n", what);
  abort();
}
void feed_launch_check_only(const FeedArgs &, void *) { no_gpu("feed_launch_check_only"); }
void feedgrep_launch_layout(const FeedArgs &, const FeedGrepArgs &, void *) { no_gpu("feedgrep_launch_layout"); }
void feedgrep_launch_windows(const FeedArgs &, const FeedGrepArgs &, void *) { no_gpu("feedgrep_launch_windows"); }
void feedgrep_launch_flag(const FeedArgs &, const FeedGrepArgs &, uint32_t, void *) { no_gpu("feedgrep_launch_flag"); }
void feedgrep_launch_commit(const FeedArgs &, const FeedGrepArgs &, uint32_t, void *) { no_gpu("feedgrep_launch_commit"); }
}  // namespace aha
