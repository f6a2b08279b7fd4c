// tree_driver.cpp -- the one driver of eegfx_dtree_* and eegfx_rforest_* (and eegfx_poisson_bag):
// MLlib 1.6.2 RandomForest (RandomForestClassifier.java:101-136) and DecisionTree
// (DecisionTreeClassifier.java:99-127), whose run *is* a forest of one tree over every feature
// without a bag.  The passes over the rows run on the device (dtree.hip, rforest.hip); the
// threshold search, the bagging, the feature subsets, the node queue, the split selection and the
// growth of every node are the host's (dtree_host.h, rforest_host.h), DESIGN.md sections 10.1, 10.2.
#include <cmath>
#include <cstring>
#include <deque>
#include <vector>

#include "ctx.h"
#include "rforest_host.h"

// Device memory the histograms of one synchronisation may take (a node's histogram is k * bins * 2
// counters): the launches of a group are issued back to back into it and read back together.
static constexpr size_t kTreeHistBudget = (size_t)16 << 20;

// The front half of a tree or a forest call (DESIGN.md section 10.1 "Bins"): the threshold sample
// to the host, the thresholds of every feature (one sort per feature, on threads), the table to
// the device and the rows binned there.  hist_bytes: what the caller's histograms need of the
// scratch allocation that also holds the gathered sample.
void eegfx::dt_bin_rows(eegfx_ctx* ctx, const double* X, const double* y, int64_t n, int32_t d,
                        int32_t max_bins, int64_t split_seed, int mem, size_t hist_bytes,
                        DtBinned* out) {
  DtBinned& b = *out;
  const hipStream_t st = ctx->stream;
  const int B = b.B = (int)std::min<int64_t>(max_bins, n), T = b.T = B - 1;  // numBins, numSplits
  // ---- the sampled rows, on the host
  const int64_t required = dtree::required_samples(max_bins);
  std::vector<int64_t> rows;  // empty: every row
  if (n > required) {
    std::vector<uint32_t> mask((size_t)((n + 31) / 32));
    spark::sample_mask(n, (double)required / (double)n, 1, split_seed, mask.data());
    for (int64_t r = 0; r < n; ++r)
      if ((mask[r >> 5] >> (r & 31)) & 1u) rows.push_back(r);
  }
  const int64_t m = rows.empty() && n <= required ? n : (int64_t)rows.size();
  if (m < 1) fail(EEGFX_EINVAL, "the split sample is empty");

  const auto [dX, dy] = stage_xy(ctx, X, y, n, d, mem);
  // one allocation for the sample (device X only) and the histograms of a group after it
  const size_t sample_bytes = mem == EEGFX_MEM_DEVICE ? sizeof(double) * (size_t)(m * d) : 0;
  const size_t idx_bytes = sizeof(int64_t) * rows.size();
  b.scratch = ctx->dt_hist.get(std::max(sample_bytes + idx_bytes, hist_bytes));
  std::vector<double> sample;  // [m][d]
  const double* S = X;
  if (mem == EEGFX_MEM_DEVICE) {
    sample.resize((size_t)(m * d));
    if (rows.empty()) {
      HIP_CHECK(hipMemcpyAsync(sample.data(), dX, sample_bytes, hipMemcpyDeviceToHost, st));
    } else {
      int64_t* didx = (int64_t*)((char*)b.scratch + sample_bytes);
      HIP_CHECK(hipMemcpyAsync(didx, rows.data(), idx_bytes, hipMemcpyHostToDevice, st));
      HIP_CHECK(launch_dt_gather(st, dX, d, didx, m, (double*)b.scratch));
      HIP_CHECK(hipMemcpyAsync(sample.data(), b.scratch, sample_bytes, hipMemcpyDeviceToHost, st));
    }
    HIP_CHECK(hipStreamSynchronize(st));
    S = sample.data();
  }

  // ---- thresholds: int32 flags[4], int32 nthr[d] (padded to 8 bytes), double thr[d][T]
  const size_t thr_off = 16 + (((size_t)d * 4 + 7) & ~(size_t)7);
  b.tab.assign(thr_off + sizeof(double) * (size_t)d * T, 0);
  int32_t* nthr = b.nthr = (int32_t*)(b.tab.data() + 16);
  double* thr = b.thr = (double*)(b.tab.data() + thr_off);
  {
    const bool packed = mem == EEGFX_MEM_DEVICE || rows.empty();  // S holds the sample itself
    // Spark 1.6 finds no bin for a non-finite value and throws
    for (int64_t i = 0; i < m; ++i) {
      const double* row = S + (packed ? i : rows[i]) * d;
      for (int f = 0; f < d; ++f)
        if (!std::isfinite(row[f])) fail(EEGFX_EINVAL, "a training feature is not finite");
    }
    // one sort per feature, threads over the features (the sorts are
    // most of a call's time on one thread)
    const int W = std::min({(int)d, 8, available_processors()});
    std::vector<char> failed((size_t)W, 0);  // no exception leaves a thread
    {
      Joiner pool;
      for (int w = 0; w < W; ++w)
        pool.th.emplace_back([&, w] {
          try {
            std::vector<double> col((size_t)m), t;
            for (int f = w; f < d; f += W) {
              for (int64_t i = 0; i < m; ++i) col[i] = S[(packed ? i : rows[i]) * d + f];
              dtree::find_thresholds(col, T, &t);
              // at most T by find_thresholds' argument; never past the feature's table row
              nthr[f] = (int32_t)std::min<size_t>(t.size(), (size_t)T);
              std::copy(t.begin(), t.begin() + nthr[f], thr + (size_t)f * T);
            }
          } catch (...) {
            failed[w] = 1;
          }
        });
    }
    for (char c : failed)
      if (c) fail(EEGFX_ENOMEM, "out of host memory in the threshold search");
  }
  uint8_t* dtab = b.dtab = (uint8_t*)ctx->dt_tab.get(b.tab.size());
  HIP_CHECK(hipMemcpyAsync(dtab, b.tab.data(), b.tab.size(), hipMemcpyHostToDevice, st));
  uint8_t* bins = b.bins = (uint8_t*)ctx->dt_bins.get((size_t)(n * d));
  // int32 slot[n], then uint8 label[n]
  int32_t* slot = b.slot = (int32_t*)ctx->dt_rows.get(5 * (size_t)n);
  uint8_t* label = b.label = (uint8_t*)(slot + n);
  HIP_CHECK(launch_dt_bin(st, dX, dy, n, d, T, (const int32_t*)(dtab + 16),
                          (const double*)(dtab + thr_off), (int32_t*)dtab, bins, label, slot));
}

namespace {

// The argument checks both train entries share, in the order the tests pin: mem before the sizes,
// the sizes before the parameters.  null_arg: one of the entry's own pointers is null.
void check_tree_params(const eegfx_ctx* ctx, int mem, int64_t n, int32_t d, int32_t capacity,
                       bool null_arg, int32_t impurity, int32_t max_depth, int32_t max_bins,
                       int32_t min_instances_per_node) {
  if (!ctx) fail(EEGFX_EINVAL, "null context");
  check_mem(mem);
  // n == 1: numBins = 1 leaves no split, and Spark's assertion fails
  if (n < 2 || n > INT32_MAX) fail(EEGFX_EINVAL, "n=%lld outside [2, 2^31)", (long long)n);
  check_train_d(d);
  if (capacity < 0) fail(EEGFX_EINVAL, "capacity %d", capacity);
  if (null_arg) fail(EEGFX_EINVAL, "null argument");
  if (impurity != EEGFX_GINI && impurity != EEGFX_ENTROPY)
    fail(EEGFX_EINVAL, "impurity %d", impurity);
  if (max_depth < 0 || max_depth > 30)  // DecisionTree.run's require
    fail(EEGFX_EINVAL, "maxDepth %d outside [0, 30]", max_depth);
  if (max_bins < 2) fail(EEGFX_EINVAL, "maxBins %d below 2", max_bins);
  if (max_bins > kDtMaxBins)
    fail(EEGFX_ENOTSUP, "maxBins %d: a bin index is one byte (at most %d bins)", max_bins,
         kDtMaxBins);
  if (min_instances_per_node < 1)
    fail(EEGFX_EINVAL, "minInstancesPerNode %d", min_instances_per_node);
}

using Forest = std::vector<std::vector<eegfx_tree_node>>;

// RandomForest.run: bins the rows, bags them, and grows num_trees trees over k of the d features a
// node, group by group off the node queue.  Returns the trees; *total: their nodes.  The single
// unweighted tree (one tree, every feature: DecisionTree.run) is the case where the loop needs no
// weights: its rows carry dt_bin_kernel's slots and its histograms are dt_hist_kernel's, which
// selects a launch's rows by ticket as rf_hist_kernel does; every other case runs the rf_* kernels.
Forest grow_trees(eegfx_ctx* ctx, const double* X, const double* y, int64_t n, int32_t d,
                  int32_t impurity, int32_t max_depth, int32_t max_bins,
                  int32_t min_instances_per_node, int32_t num_trees, int k, int64_t seed, int P,
                  int64_t split_seed, int mem, int64_t* total_nodes) {
  ctx->activate();
  const hipStream_t st = ctx->stream;
  const bool subsample = k < d;
  const bool plain = num_trees == 1 && !subsample;
  const int B = (int)std::min<int64_t>(max_bins, n);  // numBins
  const size_t node_counters = (size_t)k * B * 2, node_bytes = node_counters * sizeof(uint32_t);
  // nodes per synchronisation, and per histogram launch
  const int C = (int)std::max<size_t>(1, kTreeHistBudget / node_bytes);
  const int G = node_counters <= (size_t)kDtLdsCounters
                    ? std::min(C, (int)(kDtLdsCounters / node_counters)) : C;

  DtBinned binned;
  dt_bin_rows(ctx, X, y, n, d, max_bins, split_seed, mem, (size_t)C * node_bytes, &binned);
  const int T = binned.T;
  uint32_t* dhist = (uint32_t*)binned.scratch;

  // ---- bagging: the weights on the host, the roots' tickets on the device.  The plain tree's
  // rows already sit in ticket 0, tree 0's root (dt_bin_kernel).
  uint8_t* weight = nullptr;
  int32_t* slot = binned.slot;
  if (!plain) {
    const size_t cells = (size_t)num_trees * (size_t)n;  // weights and slots, [tree][row]
    weight = (uint8_t*)ctx->rf_weight.get(cells);
    slot = (int32_t*)ctx->rf_slot.get(cells * sizeof(int32_t));
    std::vector<uint8_t> hw;
    if (num_trees == 1) {
      HIP_CHECK(hipMemsetAsync(weight, 1, cells, st));
    } else {
      hw.resize(cells);
      std::vector<int64_t> sums((size_t)num_trees);
      if (!rforest::poisson_bag(n, num_trees, P, seed, hw.data(), sums.data(),
                                std::min(64, available_processors())))
        fail(EEGFX_ENOTSUP, "a bagging weight above 255");
      for (int64_t s : sums)
        if (s > (int64_t)UINT32_MAX)
          fail(EEGFX_ENOTSUP, "a tree's weights sum to %lld: the counters are 32 bits",
               (long long)s);
      HIP_CHECK(hipMemcpyAsync(weight, hw.data(), cells, hipMemcpyHostToDevice, st));
    }
    HIP_CHECK(launch_rf_init(st, weight, n, num_trees, slot));
  }

  // ---- the forest, group by group
  const eegfx_tree_node root{1, -1, -1, -1, 0.0, 0.0, 0.0, 0.0};
  Forest out((size_t)num_trees, std::vector<eegfx_tree_node>{root});
  std::deque<rforest::QNode> queue;
  for (int32_t t = 0; t < num_trees; ++t) queue.push_back(rforest::QNode{t, 0, 0, t});
  int32_t next_seq = num_trees;
  int64_t total = num_trees;
  spark::JavaRandom rng(seed);
  std::vector<rforest::QNode> group;
  std::vector<int32_t> subsets, tab, sent, child_pos, child_seq;  // sent: the table on the device
  std::vector<uint32_t> hist;
  std::vector<DtDecision> dec;
  bool first = true;
  while (!queue.empty()) {
    rforest::next_group(&queue, &rng, d, k, subsample, (int64_t)B * 2 * k * 8, &group, &subsets);
    // cannot trigger: k <= d <= kLrMaxFeatures = 1024 and B <= 256 give at most 4 MB a node
    if (group.empty()) fail(EEGFX_ENOTSUP, "one node's aggregates exceed maxMemoryInMB");
    const int gn = (int)group.size(), s0 = group[0].seq;
    // the group's device table: the subsets [gn][k], then every launch's distinct trees, then
    // the group's distinct trees
    struct Launch {
      int first, count, trees_at, nt;
    };
    std::vector<Launch> launches;
    tab.assign(subsets.begin(), subsets.end());
    auto distinct_trees = [&](int a, int b) {  // of group nodes [a, b), in order of appearance
      const size_t at = tab.size();
      for (int i = a; i < b; ++i)
        if (std::find(tab.begin() + at, tab.end(), group[i].tree) == tab.end())
          tab.push_back(group[i].tree);
      return (int)(tab.size() - at);
    };
    for (int a = 0; a < gn; a += G) {
      const int cnt = std::min(G, gn - a), at = (int)tab.size();
      launches.push_back(Launch{a, cnt, at, distinct_trees(a, a + cnt)});
    }
    const int group_trees_at = (int)tab.size(), group_nt = distinct_trees(0, gn);
    int32_t* dtab = (int32_t*)ctx->rf_tab.get(sizeof(int32_t) * tab.size());
    if (tab != sent) {  // without subsets the table seldom changes; one tree's never does
      HIP_CHECK(hipMemcpyAsync(dtab, tab.data(), sizeof(int32_t) * tab.size(),
                               hipMemcpyHostToDevice, st));
      sent = tab;
    }

    dec.assign((size_t)gn, DtDecision{-1, -1, -1, -1});
    child_pos.assign(2 * (size_t)gn, -1);
    for (size_t l0 = 0; l0 < launches.size();) {
      // as many launches as the histogram budget holds, then one copy and one synchronisation
      size_t l1 = l0;
      int cn = 0;
      while (l1 < launches.size() && cn + launches[l1].count <= C) cn += launches[l1++].count;
      const int c0 = launches[l0].first;
      HIP_CHECK(hipMemsetAsync(dhist, 0, (size_t)cn * node_bytes, st));
      for (size_t l = l0; l < l1; ++l) {
        const Launch& L = launches[l];
        uint32_t* h = dhist + (size_t)(L.first - c0) * node_counters;
        ctx->tic();
        if (plain) {
          HIP_CHECK(launch_dt_hist(st, binned.bins, binned.label, slot, n, d, B, s0 + L.first,
                                   L.count, h));
          ctx->toc(n * (int64_t)d + 5 * n);
        } else {
          HIP_CHECK(launch_rf_hist(st, binned.bins, binned.label, weight, slot, n, d, B, k,
                                   s0 + L.first, L.count, dtab + L.trees_at, L.nt,
                                   subsample ? dtab + (size_t)L.first * k : nullptr, h));
          ctx->toc(n * (int64_t)d + n + 5 * n * (int64_t)L.nt);
        }
      }
      if (hist.size() < (size_t)cn * node_counters) hist.resize((size_t)cn * node_counters);
      HIP_CHECK(hipMemcpyAsync(hist.data(), dhist, (size_t)cn * node_bytes,
                               hipMemcpyDeviceToHost, st));
      if (first)
        HIP_CHECK(hipMemcpyAsync(binned.tab.data(), binned.dtab, 16, hipMemcpyDeviceToHost, st));
      HIP_CHECK(hipStreamSynchronize(st));
      if (first) {  // the first synchronisation reads dt_bin_kernel's flags
        const int32_t* flags = (const int32_t*)binned.tab.data();
        if (flags[0]) fail(EEGFX_EINVAL, "a training feature is not finite");
        if (flags[1]) fail(EEGFX_EINVAL, "%s", kBadLabels);
        first = false;
      }
      for (int i = c0; i < c0 + cn; ++i) {
        const rforest::QNode& q = group[i];
        const dtree::Best b = dtree::best_split(
            hist.data() + (size_t)(i - c0) * node_counters, k, B,
            subsample ? subsets.data() + (size_t)i * k : nullptr, binned.nthr, impurity,
            min_instances_per_node);
        const dtree::Grown grown = dtree::grow_node(&out[q.tree], q.pos, q.level, max_depth, b,
                                                    binned.thr, T, impurity);
        dec[i].feature = grown.feature;
        dec[i].split = grown.split;
        child_pos[2 * (size_t)i] = grown.child[0];
        child_pos[2 * (size_t)i + 1] = grown.child[1];
        if (grown.feature >= 0) total += 2;
      }
      l0 = l1;
    }
    if (total + 2 * (int64_t)queue.size() > INT32_MAX / 2)
      fail(EEGFX_ENOTSUP, "the forest has more than 2^30 nodes");
    rforest::enqueue_children(group, child_pos, &next_seq, &queue, &child_seq);
    if (queue.empty()) break;
    for (int i = 0; i < gn; ++i) {
      dec[i].left = child_seq[2 * (size_t)i];
      dec[i].right = child_seq[2 * (size_t)i + 1];
    }
    DtDecision* ddec = (DtDecision*)ctx->dt_nodes.get(sizeof(DtDecision) * dec.size());
    HIP_CHECK(hipMemcpyAsync(ddec, dec.data(), sizeof(DtDecision) * dec.size(),
                             hipMemcpyHostToDevice, st));
    HIP_CHECK(launch_rf_route(st, binned.bins, n, d, dtab + group_trees_at, group_nt, s0, gn,
                              ddec, slot));
    HIP_CHECK(hipStreamSynchronize(st));  // `dec` and `tab` are rewritten for the next group
  }
  ctx->drain();
  *total_nodes = total;
  return out;
}

// The back half of both predict entries, after their checks: inside the predict frame, the nodes
// uploaded as DtNode and one walk kernel.
// tree_offsets: num_trees + 1 offsets into `nodes` and the vote over the trees; nullptr: one tree.
void predict_rows(eegfx_ctx* ctx, const double* X, int64_t n, int32_t d,
                  const eegfx_tree_node* nodes, int32_t n_nodes, const int32_t* tree_offsets,
                  int32_t num_trees, double* out, int mem) {
  std::vector<DtNode> hn((size_t)n_nodes);  // outlives the frame's drain
  for (int32_t i = 0; i < n_nodes; ++i)
    hn[i] = DtNode{nodes[i].feature, nodes[i].left, nodes[i].right, 0, nodes[i].threshold,
                   nodes[i].predict};
  predict_frame(ctx, X, n, d, out, mem, [&](const double* dX, double* dout) {
    const hipStream_t st = ctx->stream;
    DtNode* dn = (DtNode*)ctx->dt_nodes.get(sizeof(DtNode) * hn.size());
    HIP_CHECK(hipMemcpyAsync(dn, hn.data(), sizeof(DtNode) * hn.size(), hipMemcpyHostToDevice, st));
    if (tree_offsets) {
      int32_t* doff = (int32_t*)ctx->rf_tab.get(sizeof(int32_t) * ((size_t)num_trees + 1));
      HIP_CHECK(hipMemcpyAsync(doff, tree_offsets, sizeof(int32_t) * ((size_t)num_trees + 1),
                               hipMemcpyHostToDevice, st));
      HIP_CHECK(launch_rf_predict(st, dX, n, d, dn, doff, num_trees, dout));
    } else {
      HIP_CHECK(launch_dt_predict(st, dX, n, d, dn, n_nodes, dout));
    }
  });
}

}  // namespace

extern "C" {

// DecisionTree.run: new RandomForest(strategy, 1, "all", seed).run -- one tree, every feature, no
// bag, no draw from the seed.
int eegfx_dtree_train(eegfx_ctx* ctx, const double* X, const double* y, int64_t n, int32_t d,
                      int32_t impurity, int32_t max_depth, int32_t max_bins,
                      int32_t min_instances_per_node, int64_t split_seed, eegfx_tree_node* nodes,
                      int32_t capacity, int32_t* n_nodes, int mem) {
  return guarded([&] {
    check_tree_params(ctx, mem, n, d, capacity, !X || !y || !n_nodes || (capacity > 0 && !nodes),
                      impurity, max_depth, max_bins, min_instances_per_node);
    int64_t total = 0;
    const Forest out = grow_trees(ctx, X, y, n, d, impurity, max_depth, max_bins,
                                  min_instances_per_node, 1, d, 0, 1, split_seed, mem, &total);
    *n_nodes = (int32_t)total;
    if ((int64_t)capacity < total)
      fail(EEGFX_EINVAL, "the tree has %zu nodes, capacity is %d", out[0].size(), capacity);
    memcpy(nodes, out[0].data(), sizeof(eegfx_tree_node) * out[0].size());
  });
}

int eegfx_dtree_predict(eegfx_ctx* ctx, const double* X, int64_t n, int32_t d,
                        const eegfx_tree_node* nodes, int32_t n_nodes, double* out, int mem) {
  return guarded([&] {
    if (!ctx) fail(EEGFX_EINVAL, "null context");
    check_mem(mem);
    check_predict_dims(n, d);
    if (n_nodes < 1) fail(EEGFX_EINVAL, "n_nodes %d", n_nodes);
    if (!nodes || (n > 0 && (!X || !out))) fail(EEGFX_EINVAL, "null argument");
    if (!dtree::nodes_valid(nodes, n_nodes, d))
      fail(EEGFX_EINVAL, "the node array is not a tree over %d features", d);
    if (n == 0) return;
    predict_rows(ctx, X, n, d, nodes, n_nodes, nullptr, 1, out, mem);
  });
}

int eegfx_rforest_train(eegfx_ctx* ctx, const double* X, const double* y, int64_t n, int32_t d,
                        int32_t impurity, int32_t max_depth, int32_t max_bins,
                        int32_t min_instances_per_node, int32_t num_trees, int32_t feature_subset,
                        int64_t seed, int32_t num_partitions, int64_t split_seed,
                        eegfx_tree_node* nodes, int32_t capacity, int32_t* tree_offsets,
                        int32_t* n_nodes, int mem) {
  return guarded([&] {
    check_tree_params(ctx, mem, n, d, capacity,
                      !X || !y || !n_nodes || !tree_offsets || (capacity > 0 && !nodes), impurity,
                      max_depth, max_bins, min_instances_per_node);
    if (num_trees < 1) fail(EEGFX_EINVAL, "numTrees %d", num_trees);
    const int k = rforest::features_per_node(feature_subset, num_trees, d);
    if (k < 0) fail(EEGFX_EINVAL, "featureSubsetStrategy %d", feature_subset);
    if (num_partitions < 0) fail(EEGFX_EINVAL, "num_partitions %d", num_partitions);
    const int P = num_partitions > 0 ? num_partitions : available_processors();
    int64_t total = 0;
    const Forest out = grow_trees(ctx, X, y, n, d, impurity, max_depth, max_bins,
                                  min_instances_per_node, num_trees, k, seed, P, split_seed, mem,
                                  &total);
    *n_nodes = (int32_t)total;
    if ((int64_t)capacity < total)
      fail(EEGFX_EINVAL, "the forest has %lld nodes, capacity is %d", (long long)total, capacity);
    int32_t at = 0;
    for (int32_t t = 0; t < num_trees; ++t) {
      tree_offsets[t] = at;
      memcpy(nodes + at, out[t].data(), sizeof(eegfx_tree_node) * out[t].size());
      at += (int32_t)out[t].size();
    }
    tree_offsets[num_trees] = at;
  });
}

int eegfx_rforest_predict(eegfx_ctx* ctx, const double* X, int64_t n, int32_t d,
                          const eegfx_tree_node* nodes, const int32_t* tree_offsets,
                          int32_t num_trees, double* out, int mem) {
  return guarded([&] {
    if (!ctx) fail(EEGFX_EINVAL, "null context");
    check_mem(mem);
    check_predict_dims(n, d);
    if (num_trees < 1) fail(EEGFX_EINVAL, "num_trees %d", num_trees);
    if (!nodes || !tree_offsets || (n > 0 && (!X || !out))) fail(EEGFX_EINVAL, "null argument");
    if (!rforest::forest_valid(nodes, tree_offsets, num_trees, d))
      fail(EEGFX_EINVAL, "the node array is not a forest of %d trees over %d features", num_trees,
           d);
    if (n == 0) return;
    predict_rows(ctx, X, n, d, nodes, tree_offsets[num_trees], tree_offsets, num_trees, out, mem);
  });
}

int eegfx_poisson_bag(int64_t n, int32_t num_trees, int32_t num_partitions, int64_t seed,
                      uint8_t* weights) {
  return guarded([&] {
    if (n < 0 || num_trees < 1 || num_partitions < 1 || !weights)
      fail(EEGFX_EINVAL, "bad argument");
    std::vector<int64_t> sums((size_t)num_trees);
    if (!rforest::poisson_bag(n, num_trees, num_partitions, seed, weights, sums.data(),
                              std::min(64, available_processors())))
      fail(EEGFX_ENOTSUP, "a bagging weight above 255");
  });
}

}  // extern "C"
