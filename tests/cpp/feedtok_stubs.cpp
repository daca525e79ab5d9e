// feedtok_stubs.cpp -- link-time stand-ins for the feed token launchers (scan_feedtokens.hip), beside feed_select_stubs.cpp and
// token_stubs.cpp in the sanitizer build of the host side (aha_amd/csrc/Makefile, target asan): every test there runs
// HOST_ONLY, where no launcher is ever reached (aha_feed_open refuses a host-only handle).
#include <cstdio>
#include <cstdlib>

#include "../../aha_amd/csrc/feed.hpp"

namespace aha {
[[noreturn]] static void no_gpu(const char *what) {
  fprintf(stderr, "sanitizer build: %s reached (host-only library)\n", what);
  abort();
}
void feedtok_launch_bounds(const FeedArgs &, const FeedSelArgs &, const FeedTokArgs &, uint32_t, void *) { no_gpu("feedtok_launch_bounds"); }
void feedtok_launch_starts(const FeedArgs &, const FeedSelArgs &, const FeedTokArgs &, uint32_t, void *) { no_gpu("feedtok_launch_starts"); }
void feedtok_launch_edge(const FeedArgs &, const FeedSelArgs &, const FeedTokArgs &, uint32_t, void *) { no_gpu("feedtok_launch_edge"); }
void feedtok_launch_emit(const FeedArgs &, const FeedSelArgs &, const FeedTokArgs &, uint32_t, void *) { no_gpu("feedtok_launch_emit"); }
void feedtok_launch_commit(const FeedArgs &, const FeedSelArgs &, const FeedTokArgs &, uint32_t, void *) { no_gpu("feedtok_launch_commit"); }
}  // namespace aha
