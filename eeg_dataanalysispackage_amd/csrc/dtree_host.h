// dtree_host.h -- the host half of the decision tree (eegfx_dtree_*): MLlib 1.6.2 DecisionTree as
// Classification/DecisionTreeClassifier.java:99-127 calls it (continuous features, two classes).
// Threshold search over the sampled rows, impurities, best-split selection over one node's integer
// class histogram, and the check of a node array before prediction.  No HIP here:
// dtree_driver.cpp drives the kernels of dtree.hip around these functions, and a stand-alone
// program can compile them
// (tests/c_abi/dtree_host_check.cpp).  Every gain is plain fp64, evaluated left to right and
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

// binsToBestSplit for one node: h = uint32 [d][B][2] (feature, bin, label), feature f has
// nthr[f] splits, split s sends bins 0..s left.  The first maximum in feature-major then split
// order (Scala's maxBy keeps the earlier of equals); an invalid candidate has gain -DBL_MAX.
inline Best best_split(const uint32_t* h, int d, int B, const int32_t* nthr, int kind,
                       int min_instances) {
  Best best;
  for (int b = 0; b < B; ++b) {
    best.tot[0] += (double)h[b * 2];
    best.tot[1] += (double)h[b * 2 + 1];
  }
  const double imp_tot = impurity(kind, best.tot[0], best.tot[1]);
  for (int f = 0; f < d; ++f) {
    double l0 = 0, l1 = 0;
    for (int s = 0; s < nthr[f]; ++s) {
      l0 += (double)h[((size_t)f * B + s) * 2];
      l1 += (double)h[((size_t)f * B + s) * 2 + 1];
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

// Predict.predict of a node's class counts: the argmax, class 0 on a tie
inline double predict_of(const double c[2]) { return c[1] > c[0] ? 1.0 : 0.0; }

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
