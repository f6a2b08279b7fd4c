// rforest_host.h -- the host half of the random forest (eegfx_rforest_*): MLlib 1.6.2 RandomForest
// as Classification/RandomForestClassifier.java:101-136 calls it (continuous features, two
// classes), DESIGN.md section 10.2.  The bagging weights (commons-math's PoissonDistribution(1.0)
// on a Well19937c, one sampler per ParallelCollectionRDD slice), the features of a node
// (DecisionTreeMetadata, SamplingUtils.reservoirSampleAndCount), the node queue and its groups
// (RandomForest.selectNodesToSplit), and the check of a forest before prediction.  No HIP here:
// tree_driver.cpp drives the kernels of rforest.hip around these functions, and a stand-alone
// program can compile them (tests/c_abi/rforest_host_check.cpp).  Thresholds, impurities, split
// selection and the per-node rule are dtree_host.h's.
#pragma once

#include <algorithm>
#include <cstdint>
#include <deque>
#include <vector>

#include "dtree_host.h"
#include "joiner.h"
#include "spark_sample.h"

namespace eegfx {
namespace rforest {

// org.apache.commons.math3.random.Well19937c (AbstractWell with k = 19937: 624 words)
struct Well19937c {
  uint32_t v[624];
  int index = 0;
  explicit Well19937c(int64_t seed) { set_seed(seed); }
  // AbstractWell.setSeed(long) -> setSeed(int[]{high, low}): the words after the seed come from
  // the sign-extended word two places back
  void set_seed(int64_t seed) {
    v[0] = (uint32_t)((uint64_t)seed >> 32);
    v[1] = (uint32_t)(uint64_t)seed;
    for (int i = 2; i < 624; ++i) {
      const int64_t l = (int64_t)(int32_t)v[i - 2];
      v[i] = (uint32_t)(1812433253ULL * (uint64_t)(l ^ (l >> 30)) + (uint64_t)i);
    }
    index = 0;
  }
  uint32_t next(int bits) {
    auto at = [](int i) { return i >= 624 ? i - 624 : i; };  // i % 624 for i < 1248
    const int iRm1 = at(index + 623), iRm2 = at(index + 622);
    const uint32_t v0 = v[index], vM1 = v[at(index + 70)], vM2 = v[at(index + 179)],
                   vM3 = v[at(index + 449)];
    const uint32_t z0 = (0x80000000u & v[iRm1]) ^ (0x7FFFFFFFu & v[iRm2]);
    const uint32_t z1 = (v0 ^ (v0 << 25)) ^ (vM1 ^ (vM1 >> 27));
    const uint32_t z2 = (vM2 >> 9) ^ (vM3 ^ (vM3 >> 1));
    const uint32_t z3 = z1 ^ z2;
    uint32_t z4 = z0 ^ (z1 ^ (z1 << 9)) ^ (z2 ^ (z2 << 21)) ^ (z3 ^ (z3 >> 21));
    v[iRm1] = z3;
    v[index] = z4;
    v[iRm2] &= 0x80000000u;
    index = iRm1;
    z4 ^= (z4 << 7) & 0xe46e1700u;
    z4 ^= (z4 << 15) & 0x9b868000u;
    return z4 >> (32 - bits);
  }
  // BitsStreamGenerator.nextDouble
  double next_double() {
    const uint64_t high = (uint64_t)next(26) << 26;
    const uint64_t low = next(26);
    return (double)(high | low) * 0x1.0p-52;
  }
};

// PoissonDistribution(1.0).sample(): the product of uniforms against exp(-1), the correctly
// rounded double as a literal (no libm call enters)
inline int poisson1(Well19937c& rng) {
  const double p = 0x1.78b56362cef38p-2;
  int n = 0;
  double r = 1.0;
  while (n < 1000) {
    r *= rng.next_double();
    if (r >= p)
      ++n;
    else
      return n;
  }
  return n;
}

// BaggedPoint.convertToBaggedRDD with subsamplingRate 1.0, with replacement: w[tree][row] (tree-
// major, n bytes per tree) and each tree's weight sum.  num_trees == 1: every weight 1, no
// sampler.  Otherwise slice p = rows [p n / P, (p + 1) n / P) owns the sampler seeded with
// seed + p + 1 and draws row by row, tree by tree.  The slices are drawn on up to `threads`
// threads; a slice's rows are written by its thread alone and the sums are integers, so the result
// does not depend on `threads`.  Returns false when a draw does not fit a byte.
inline bool poisson_bag(int64_t n, int num_trees, int P, int64_t seed, uint8_t* w,
                        int64_t* tree_sums, int threads) {
  if (num_trees == 1) {
    std::fill(w, w + n, (uint8_t)1);
    tree_sums[0] = n;
    return true;
  }
  const int W = std::max(1, std::min(threads, P));
  std::vector<int64_t> part((size_t)W * num_trees, 0);
  std::vector<char> over((size_t)W, 0);
  auto work = [&](int t) {
    int64_t* sums = part.data() + (size_t)t * num_trees;
    for (int p = t; p < P; p += W) {
      const int64_t a = (int64_t)p * n / P, b = (int64_t)(p + 1) * n / P;
      if (a >= b) continue;
      Well19937c rng((int64_t)((uint64_t)seed + (uint64_t)p + 1u));
      for (int64_t r = a; r < b; ++r)
        for (int k = 0; k < num_trees; ++k) {
          const int c = poisson1(rng);
          if (c > 255) over[t] = 1;
          w[(size_t)k * n + r] = (uint8_t)c;
          sums[k] += c;
        }
    }
  };
  if (W == 1) {
    work(0);
  } else {
    Joiner pool;
    for (int t = 0; t < W; ++t) pool.th.emplace_back(work, t);
  }
  bool ok = true;
  for (int k = 0; k < num_trees; ++k) tree_sums[k] = 0;
  for (int t = 0; t < W; ++t) {
    ok = ok && !over[t];
    for (int k = 0; k < num_trees; ++k) tree_sums[k] += part[(size_t)t * num_trees + k];
  }
  return ok;
}

// DecisionTreeMetadata.buildMetadata: the features a node considers.  subset: EEGFX_SUBSET_*;
// the roots are integer ones (ceil(sqrt d), ceil(log2 d)), so no rounding enters.  -1: unknown.
inline int features_per_node(int subset, int num_trees, int d) {
  if (subset == EEGFX_SUBSET_AUTO) subset = num_trees == 1 ? EEGFX_SUBSET_ALL : EEGFX_SUBSET_SQRT;
  switch (subset) {
    case EEGFX_SUBSET_ALL:
      return d;
    case EEGFX_SUBSET_SQRT: {
      int k = 0;
      while ((int64_t)k * k < d) ++k;
      return k;
    }
    case EEGFX_SUBSET_LOG2: {
      int c = 0;
      while (((int64_t)1 << c) < d) ++c;
      return std::max(1, c);
    }
    case EEGFX_SUBSET_ONETHIRD:
      return (d + 2) / 3;
  }
  return -1;
}

// SamplingUtils.reservoirSampleAndCount over 0..d-1 with an XORShiftRandom(seed): res[k], in
// reservoir order (not sorted).  k == d: no draw.
inline void reservoir(int d, int k, int64_t seed, int32_t* res) {
  for (int i = 0; i < k; ++i) res[i] = i;
  if (k >= d) return;
  spark::XORShiftRandom rand(seed);
  int64_t l = k;
  for (int item = k; item < d; ++item) {
    l += 1;
    const int64_t j = (int64_t)(rand.next_double() * (double)l);
    if (j < k) res[j] = item;
  }
}

// A queued node: its tree, its position in that tree's node array, its level, and its ticket (the
// order it entered the queue: the roots are 0..num_trees-1).  A group leaves the head of the queue,
// so its tickets are consecutive.
struct QNode {
  int32_t tree, pos, level, seq;
};
constexpr int64_t kMaxMemoryBytes = (int64_t)256 << 20;  // Strategy.maxMemoryInMB = 256

// RandomForest.selectNodesToSplit: takes nodes off the head of the queue while the group's
// aggregates stay within maxMemoryInMB; every node looked at draws its feature subset (k of d
// features, subsets[i * k ..]) from rng when `subsample`, the node that does not fit included --
// it stays queued and draws again for the next group.  node_bytes = aggregateSize: numBins * 2 *
// (k or d) doubles.  An empty group (a single node above the limit) is the caller's error.
inline void next_group(std::deque<QNode>* q, spark::JavaRandom* rng, int d, int k, bool subsample,
                       int64_t node_bytes, std::vector<QNode>* group,
                       std::vector<int32_t>* subsets) {
  group->clear();
  subsets->clear();
  std::vector<int32_t> res((size_t)k);
  int64_t mem = 0;
  while (!q->empty() && mem < kMaxMemoryBytes) {
    if (subsample) reservoir(d, k, rng->next_long(), res.data());
    if (mem + node_bytes <= kMaxMemoryBytes) {
      group->push_back(q->front());
      q->pop_front();
      if (subsample) subsets->insert(subsets->end(), res.begin(), res.end());
    }
    mem += node_bytes;
  }
}

// After a group: the children that are not leaves enter the queue by ascending tree, a tree's
// nodes in group order, left then right.  child_pos[2 i + side]: the position of group node i's
// child in its tree, -1: none or a leaf.  Writes the ticket of each queued child (-1 otherwise).
inline void enqueue_children(const std::vector<QNode>& group, const std::vector<int32_t>& child_pos,
                             int32_t* next_seq, std::deque<QNode>* q,
                             std::vector<int32_t>* child_seq) {
  child_seq->assign(child_pos.size(), -1);
  std::vector<int32_t> order(group.size());
  for (size_t i = 0; i < order.size(); ++i) order[i] = (int32_t)i;
  std::stable_sort(order.begin(), order.end(),
                   [&](int32_t a, int32_t b) { return group[a].tree < group[b].tree; });
  for (int32_t i : order)
    for (int side = 0; side < 2; ++side) {
      const int32_t pos = child_pos[2 * (size_t)i + side];
      if (pos < 0) continue;
      (*child_seq)[2 * (size_t)i + side] = *next_seq;
      q->push_back(QNode{group[i].tree, pos, group[i].level + 1, (*next_seq)++});
    }
}

// A node's split over its feature list is the tree's rule under its earlier name here
using dtree::best_split;

// A forest that prediction may walk: the offsets ascend from 0, every tree has a node, and each
// tree's slice is a valid node array of its own (children relative to its first node).
inline bool forest_valid(const eegfx_tree_node* nodes, const int32_t* offsets, int32_t num_trees,
                         int32_t d) {
  if (!nodes || !offsets || num_trees < 1 || offsets[0] != 0) return false;
  for (int32_t t = 0; t < num_trees; ++t)
    if (offsets[t + 1] <= offsets[t]) return false;
  for (int32_t t = 0; t < num_trees; ++t)
    if (!dtree::nodes_valid(nodes + offsets[t], offsets[t + 1] - offsets[t], d)) return false;
  return true;
}

}  // namespace rforest
}  // namespace eegfx
