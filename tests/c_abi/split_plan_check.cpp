// split_plan_check.cpp -- csrc/split_plan.h alone, as a plain program for the sanitizers
// (tests/test_split_plan_cases.py builds it with AddressSanitizer + UBSan and runs it directly).
// stdin, one case per line:  n cut first count perm[0] .. perm[n-1]
// stdout per case:           n_train n_test idx[0..count) pos[0..count)
#include <cstdio>
#include <vector>

#include "split_plan.h"

int main() {
  long long n, cut, first, count;
  while (scanf("%lld %lld %lld %lld", &n, &cut, &first, &count) == 4) {
    std::vector<int64_t> perm((size_t)n);
    for (auto& p : perm) {
      long long v;
      if (scanf("%lld", &v) != 1) return 2;
      p = v;
    }
    const eegfx::SplitShardPlan s = eegfx::split_shard_plan(perm.data(), n, cut, first, count);
    if ((long long)s.idx.size() != count || (long long)s.pos.size() != count) return 3;
    printf("%lld %lld", (long long)s.n_train, (long long)s.n_test);
    for (int64_t v : s.idx) printf(" %lld", (long long)v);
    for (int64_t v : s.pos) printf(" %lld", (long long)v);
    printf("\n");
  }
  printf("split_plan_check ok\n");
  return 0;
}
