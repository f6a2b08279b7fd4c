// dtree_host.h -- the host half of the decision tree (eegfx_dtree_*): MLlib 1.6.2 DecisionTree as
// Classification/DecisionTreeClassifier.java:99-127 calls it (continuous features, two classes).
// Threshold search over the sampled rows, impurities, best-split selection over one node's integer
// class histogram, the growth of a node from its split, and the check of a node array before
// prediction.  No HIP here: tree_driver.cpp drives the kernels of dtree.hip and rforest.hip around
// these functions, and a stand-alone program can compile them (tests/c_abi/dtree_host_check.cpp).  Every gain is plain fp64, evaluated left to right and
// unfused (-ffp-contract=off), with libm's log: the tree is bit-defined under both impurities.
#pragma once

#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstdint>
#include <vector>

#include "eegfx.h"

namespace eegfx {
namespace dtree {

// DecisionTreeMetadata: the rows findSplitsBins samples, max(maxBins^2, 10000)
inline int64_t required_samples(int max_bins) {
  return std::max<int64_t>((int64_t)max_bins * max_bins, 10000);
}

// findSplitsForContinuousFeature: the thresholds of one feature from its sampled values (`v` is
// sorted in place).  Distinct values ascending with their counts (-0.0 == 0.0 is one value); all of
// them when there are at most num_splits, else the stride scan, which emits at most num_splits
// (an emission needs cur > target, and cur never passes samples = (num_splits + 1) * stride).
inline void find_thresholds(std::vector<double>& v, int num_splits, std::vector<double>* out) {
  out->clear();
  std::sort(v.begin(), v.end());
  std::vector<double> val;
  std::vector<int64_t> cnt;
  for (double x : v) {
    if (!val.empty() && val.back() == x) {
      ++cnt.back();
    } else {
      val.push_back(x);
      cnt.push_back(1);
    }
  }
  if ((int64_t)val.size() <= num_splits) {
    *out = val;
    return;
  }
  const double stride = (double)v.size() / (double)(num_splits + 1);
  double target = stride;
  int64_t cur = cnt[0];
  for (size_t i = 1; i < val.size(); ++i) {
    const int64_t prev = cur;
    cur += cnt[i];
    if (std::fabs((double)prev - target) < std::fabs((double)cur - target)) {
      out->push_back(val[i - 1]);
      target += stride;
    }
  }
}

// Gini.calculate / Entropy.calculate over the two class counts
inline double impurity(int kind, double c0, double c1) {
  const double t = c0 + c1;
  if (t == 0.0) return 0.0;
  if (kind == EEGFX_GINI) {
    double imp = 1.0;
    double f = c0 / t;
    imp -= f * f;
    f = c1 / t;
    imp -= f * f;
    return imp;
  }
  double imp = 0.0;
  if (c0 != 0.0) {
    const double f = c0 / t;
    imp -= f * (std::log(f) / std::log(2.0));
  }
  if (c1 != 0.0) {
    const double f = c1 / t;
    imp -= f * (std::log(f) / std::log(2.0));
  }
  return imp;
}

struct Best {
  int feature = -1;  // -1: the node has no candidate at all
  int split = -1;
  double gain = -DBL_MAX;
  double tot[2] = {0, 0}, left[2] = {0, 0}, right[2] = {0, 0};  // class counts
};

// binsToBestSplit over a node's feature list: h = uint32 [k][B][2] (list position, bin, label),
// position j is feature feat[j] (feat == nullptr: feature j, the whole tree's k == d) with
// nthr[feature] splits, split s sends bins 0..s left.  The first maximum in list order then split
// order (Scala's maxBy keeps the earlier of equals); an invalid candidate has gain -DBL_MAX.
// Best::feature is the feature itself.
inline Best best_split(const uint32_t* h, int k, int B, const int32_t* feat, const int32_t* nthr,
                       int kind, int min_instances) {
  Best best;
  for (int b = 0; b < B; ++b) {
    best.tot[0] += (double)h[b * 2];
    best.tot[1] += (double)h[b * 2 + 1];
  }
  const double imp_tot = impurity(kind, best.tot[0], best.tot[1]);
  for (int j = 0; j < k; ++j) {
    const int f = feat ? feat[j] : j;
    double l0 = 0, l1 = 0;
    for (int s = 0; s < nthr[f]; ++s) {
      l0 += (double)h[((size_t)j * B + s) * 2];
      l1 += (double)h[((size_t)j * B + s) * 2 + 1];
      const double r0 = best.tot[0] - l0, r1 = best.tot[1] - l1;
      const double lc = l0 + l1, rc = r0 + r1;
      double gain = -DBL_MAX;
      if (!(lc < (double)min_instances || rc < (double)min_instances)) {
        const double t = lc + rc;
        gain = imp_tot - (lc / t) * impurity(kind, l0, l1) - (rc / t) * impurity(kind, r0, r1);
        if (gain < 0.0) gain = -DBL_MAX;
      }
      if (best.feature < 0 || gain > best.gain) {
        best.feature = f;
        best.split = s;
        best.gain = gain;
        best.left[0] = l0;
        best.left[1] = l1;
        best.right[0] = r0;
        best.right[1] = r1;
      }
    }
  }
  return best;
}

// The whole tree's call, as it was before the feature list: every feature, in order.
inline Best best_split(const uint32_t* h, int d, int B, const int32_t* nthr, int kind,
                       int min_instances) {
  return best_split(h, d, B, nullptr, nthr, kind, min_instances);
}

// Predict.predict of a node's class counts: the argmax, class 0 on a tie
inline double predict_of(const double c[2]) { return c[1] > c[0] ? 1.0 : 0.0; }

// What grow_node decided: the split the rows of the node are routed by (feature -1: the node is a
// leaf) and the positions of its children that get a histogram of their own (-1: none, or a leaf).
struct Grown {
  int32_t feature = -1, split = -1;
  int32_t child[2] = {-1, -1};
};

// One node of `tree` (at `pos`, on `level`) from its best split.  The root takes predict and
// impurity from its own counts (a child got them from its parent's split).  The node is a leaf iff
// there is no candidate, the gain is not above 0 or level == max_depth; otherwise it stores
// (feature, threshold thr[feature * T + split], gain) and its children are appended, left then
// right, with ids 2 id and 2 id + 1; a child is a leaf iff level + 1 == max_depth or its impurity
// is 0.0.
inline Grown grow_node(std::vector<eegfx_tree_node>* tree, int32_t pos, int level, int max_depth,
                       const Best& b, const double* thr, int T, int kind) {
  std::vector<eegfx_tree_node>& t = *tree;
  Grown g;
  if (level == 0) {
    t[pos].predict = predict_of(b.tot);
    t[pos].impurity = impurity(kind, b.tot[0], b.tot[1]);
  }
  if (b.feature < 0 || b.gain <= 0.0 || level == max_depth) return g;
  const int32_t id = t[pos].id;
  t[pos].feature = g.feature = b.feature;
  t[pos].threshold = thr[(size_t)b.feature * T + b.split];
  t[pos].gain = b.gain;
  g.split = b.split;
  for (int side = 0; side < 2; ++side) {
    const double* c = side == 0 ? b.left : b.right;
    const double imp = impurity(kind, c[0], c[1]);
    const int32_t child = (int32_t)t.size();
    t.push_back(eegfx_tree_node{2 * id + side, -1, -1, -1, 0.0, predict_of(c), imp, 0.0});
    (side == 0 ? t[pos].left : t[pos].right) = child;
    if (!(level + 1 == max_depth || imp == 0.0)) g.child[side] = child;
  }
  return g;
}

// A node array that prediction may walk: every child position lies inside the array and after its
// parent (so a walk ends), a leaf has no child, and every feature is below d.
inline bool nodes_valid(const eegfx_tree_node* nodes, int32_t n_nodes, int32_t d) {
  if (!nodes || n_nodes < 1) return false;
  for (int32_t i = 0; i < n_nodes; ++i) {
    const eegfx_tree_node& nd = nodes[i];
    if (nd.feature == -1) {
      if (nd.left != -1 || nd.right != -1) return false;
      continue;
    }
    if (nd.feature < 0 || nd.feature >= d) return false;
    if (nd.left <= i || nd.left >= n_nodes || nd.right <= i || nd.right >= n_nodes) return false;
  }
  return true;
}

}  // namespace dtree
}  // namespace eegfx
