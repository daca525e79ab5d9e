// feed_fold_stubs.cpp -- link-time stand-ins for the launchers a folded feed adds (AHA_FEED_FOLD; scan_feedfold.hip, and
// scan_feed.hip's kfd_leads on its own), beside feed_stubs.cpp in the sanitizer build of the host side (aha_amd/csrc/Makefile,
// target asan): every test there runs HOST_ONLY, where no launcher is ever reached (aha_feed_open refuses a host-only handle).
#include <cstdio>
#include <cstdlib>

#include "../../aha_amd/csrc/feed.hpp"

namespace aha {
[[noreturn]] static void no_gpu(const char *what) {
  fprintf(stderr, "sanitizer build: %s reached (host-only library)\n", what);
  abort();
}
void feed_launch_leads(const FeedArgs &, void *) { no_gpu("feed_launch_leads"); }
void feedfold_launch_heads(const FeedArgs &, int, void *) { no_gpu("feedfold_launch_heads"); }
void feedfold_launch_windows(const FeedArgs &, int, void *) { no_gpu("feedfold_launch_windows"); }
}  // namespace aha
