// joiner.h -- eegfx::Joiner, for every host source that starts threads.  No HIP here: ctx.h and
// rforest_host.h both include it.
#pragma once

#include <thread>
#include <vector>

namespace eegfx {

// Joins the threads it holds when it goes out of scope (an exception from emplace_back or from a
// later call leaves no joinable std::thread behind, which would call std::terminate).
struct Joiner {
  std::vector<std::thread> th;
  ~Joiner() {
    for (auto& t : th)
      if (t.joinable()) t.join();
  }
};

}  // namespace eegfx
