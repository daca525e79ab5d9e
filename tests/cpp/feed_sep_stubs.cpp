// feed_sep_stubs.cpp -- link-time stand-ins for the launchers of a feed with a separator filter (scan_feedsep.hip and the edge
// launchers of scan_feed.hip), beside feed_stubs.cpp and feed_select_stubs.cpp in the sanitizer build of the host side
// (aha_amd/csrc/Makefile, target asan): every test there runs HOST_ONLY, where no launcher is ever reached (aha_feed_open_params
// refuses a host-only handle once its arguments are checked).
#include <cstdio>
#include <cstdlib>

#include "../../aha_amd/csrc/feed.hpp"

namespace aha {
[[noreturn]] static void no_gpu(const char *what) {
  fprintf(stderr, "sanitizer build: %s reached (host-only library)\n", what);
  abort();
}
void feed_launch_edge(const FeedArgs &, void *) { no_gpu("feed_launch_edge"); }
void feed_launch_merge_edge(const FeedArgs &, void *) { no_gpu("feed_launch_merge_edge"); }
void feedsep_launch_flag(const FeedArgs &, const FeedSepArgs &, uint32_t, void *) { no_gpu("feedsep_launch_flag"); }
void feedsep_launch_flag_finish(const FeedArgs &, const FeedSepArgs &, uint32_t, void *) { no_gpu("feedsep_launch_flag_finish"); }
void feedsep_launch_compact(const FeedSepArgs &, bool, uint32_t, void *) { no_gpu("feedsep_launch_compact"); }
void feedsep_launch_count(const FeedArgs &, const FeedSepArgs &, uint32_t, void *) { no_gpu("feedsep_launch_count"); }
void feedsep_launch_count_finish(const FeedArgs &, uint32_t, void *) { no_gpu("feedsep_launch_count_finish"); }
void feedsep_launch_restart(const FeedArgs &, const FeedSepArgs &, void *) { no_gpu("feedsep_launch_restart"); }
}  // namespace aha
