// split_plan.h -- the host arithmetic of eegfx_odp_split_sharded (odp.cpp): which of a shard's
// rows are training rows and which are test rows of the shuffled list, and where in that list each
// one stands.  Host code only (no HIP); eegfx_split_shard_plan exposes it and
// tests/test_split_plan_cases.py checks it against pipeline.reference_split.
#pragma once

#include <cstdint>
#include <vector>

namespace eegfx {

// One shard's part of the split.  perm[p] is the global row at position p of the shuffled list
// (eegfx_java_shuffle); positions [0, cut) are the training part, cut = (int64_t)(n * fraction).
// Of the rows [first, first + count): the training rows first, then the test rows, each part in
// increasing position.  idx: the row within the shard; pos: its position in its part (p for a
// training row, p - cut for a test row).
struct SplitShardPlan {
  int64_t n_train = 0, n_test = 0;
  std::vector<int64_t> idx, pos;  // [n_train + n_test]
};

inline SplitShardPlan split_shard_plan(const int64_t* perm, int64_t n, int64_t cut, int64_t first,
                                       int64_t count) {
  SplitShardPlan s;
  s.idx.resize((size_t)count);
  s.pos.resize((size_t)count);
  for (int64_t p = 0; p < cut; ++p)
    s.n_train += (uint64_t)(perm[p] - first) < (uint64_t)count;
  s.n_test = count - s.n_train;
  int64_t a = 0, b = s.n_train;
  for (int64_t p = 0; p < n; ++p) {
    const int64_t r = perm[p] - first;
    if ((uint64_t)r >= (uint64_t)count) continue;
    int64_t& at = p < cut ? a : b;
    s.idx[(size_t)at] = r;
    s.pos[(size_t)at] = p < cut ? p : p - cut;
    ++at;
  }
  return s;
}

}  // namespace eegfx
