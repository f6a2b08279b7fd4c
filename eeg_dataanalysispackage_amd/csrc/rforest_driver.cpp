// rforest_driver.cpp -- the drivers of eegfx_rforest_train / eegfx_rforest_predict /
// eegfx_poisson_bag: MLlib 1.6.2 RandomForest (RandomForestClassifier.java:101-136) with the
// passes over every tree's rows on the device (rforest.hip, and dtree.hip's binning) and the
// bagging, the feature subsets, the node queue and the split selection on the host
// (rforest_host.h), DESIGN.md section 10.2.
#include <cstring>
#include <deque>
#include <vector>

#include "ctx.h"
#include "rforest_host.h"

// Device memory the histograms of one synchronisation may take (a node's histogram is k * bins * 2
// counters): the launches of a group are issued back to back into it and read back together.
static constexpr size_t kRfHistBudget = (size_t)16 << 20;

extern "C" {

int eegfx_rforest_train(eegfx_ctx* ctx, const double* X, const double* y, int64_t n, int32_t d,
                        int32_t impurity, int32_t max_depth, int32_t max_bins,
                        int32_t min_instances_per_node, int32_t num_trees, int32_t feature_subset,
                        int64_t seed, int32_t num_partitions, int64_t split_seed,
                        eegfx_tree_node* nodes, int32_t capacity, int32_t* tree_offsets,
                        int32_t* n_nodes, int mem) {
  return guarded([&] {
    if (!ctx) fail(EEGFX_EINVAL, "null context");
    check_mem(mem);
    // n == 1: numBins = 1 leaves no split, and Spark's assertion fails
    if (n < 2 || n > INT32_MAX) fail(EEGFX_EINVAL, "n=%lld outside [2, 2^31)", (long long)n);
    if (d < 1 || d > kLrMaxFeatures) fail(EEGFX_EINVAL, "d=%d outside [1, %d]", d, kLrMaxFeatures);
    if (capacity < 0) fail(EEGFX_EINVAL, "capacity %d", capacity);
    if (!X || !y || !n_nodes || !tree_offsets || (capacity > 0 && !nodes))
      fail(EEGFX_EINVAL, "null argument");
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
    if (num_trees < 1) fail(EEGFX_EINVAL, "numTrees %d", num_trees);
    const int k = rforest::features_per_node(feature_subset, num_trees, d);
    if (k < 0) fail(EEGFX_EINVAL, "featureSubsetStrategy %d", feature_subset);
    if (num_partitions < 0) fail(EEGFX_EINVAL, "num_partitions %d", num_partitions);
    const int P = num_partitions > 0 ? num_partitions : available_processors();
    const size_t cells = (size_t)num_trees * (size_t)n;  // weights and slots, [tree][row]
    ctx->activate();
    const hipStream_t st = ctx->stream;
    const bool subsample = k < d;
    const int B = (int)std::min<int64_t>(max_bins, n);  // numBins
    const size_t node_counters = (size_t)k * B * 2, node_bytes = node_counters * sizeof(uint32_t);
    // nodes per histogram launch, and per synchronisation
    const int C = (int)std::max<size_t>(1, kRfHistBudget / node_bytes);
    const int G = node_counters <= (size_t)kDtLdsCounters
                      ? std::min(C, (int)(kDtLdsCounters / node_counters)) : C;

    DtBinned binned;
    dt_bin_rows(ctx, X, y, n, d, max_bins, split_seed, mem, (size_t)C * node_bytes, &binned);
    const int T = binned.T;
    const int32_t* nthr = binned.nthr;
    const double* thr = binned.thr;
    uint32_t* dhist = (uint32_t*)binned.scratch;

    // ---- bagging: the weights on the host, the roots' tickets on the device
    uint8_t* weight = (uint8_t*)ctx->rf_weight.get(cells);
    int32_t* slot = (int32_t*)ctx->rf_slot.get(cells * sizeof(int32_t));
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

    // ---- the forest, group by group
    const eegfx_tree_node root{1, -1, -1, -1, 0.0, 0.0, 0.0, 0.0};
    std::vector<std::vector<eegfx_tree_node>> out((size_t)num_trees,
                                                  std::vector<eegfx_tree_node>{root});
    std::deque<rforest::QNode> queue;
    for (int32_t t = 0; t < num_trees; ++t) queue.push_back(rforest::QNode{t, 0, 0, t});
    int32_t next_seq = num_trees;
    int64_t total = num_trees;
    spark::JavaRandom rng(seed);
    std::vector<rforest::QNode> group;
    std::vector<int32_t> subsets, tab, child_pos, child_seq;
    std::vector<uint32_t> hist((size_t)C * node_counters);
    std::vector<DtDecision> dec;
    bool first = true;
    while (!queue.empty()) {
      rforest::next_group(&queue, &rng, d, k, subsample, (int64_t)B * 2 * k * 8, &group, &subsets);
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
      HIP_CHECK(hipMemcpyAsync(dtab, tab.data(), sizeof(int32_t) * tab.size(),
                               hipMemcpyHostToDevice, st));

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
          ctx->tic();
          HIP_CHECK(launch_rf_hist(st, binned.bins, binned.label, weight, slot, n, d, B, k,
                                   s0 + L.first, L.count, dtab + L.trees_at, L.nt,
                                   subsample ? dtab + (size_t)L.first * k : nullptr,
                                   dhist + (size_t)(L.first - c0) * node_counters));
          ctx->toc(n * (int64_t)d + n + 5 * n * (int64_t)L.nt);
        }
        HIP_CHECK(hipMemcpyAsync(hist.data(), dhist, (size_t)cn * node_bytes,
                                 hipMemcpyDeviceToHost, st));
        if (first)
          HIP_CHECK(hipMemcpyAsync(binned.tab.data(), binned.dtab, 16, hipMemcpyDeviceToHost, st));
        HIP_CHECK(hipStreamSynchronize(st));
        if (first) {
          const int32_t* flags = (const int32_t*)binned.tab.data();
          if (flags[0]) fail(EEGFX_EINVAL, "a training feature is not finite");
          if (flags[1]) fail(EEGFX_EINVAL, "Input validation failed: labels must be 0.0 or 1.0");
          first = false;
        }
        for (int i = c0; i < c0 + cn; ++i) {
          const rforest::QNode& q = group[i];
          const dtree::Best b = rforest::best_split(
              hist.data() + (size_t)(i - c0) * node_counters, k, B,
              subsample ? subsets.data() + (size_t)i * k : nullptr, nthr, impurity,
              min_instances_per_node);
          std::vector<eegfx_tree_node>& tree = out[q.tree];
          if (q.level == 0) {
            tree[q.pos].predict = dtree::predict_of(b.tot);
            tree[q.pos].impurity = dtree::impurity(impurity, b.tot[0], b.tot[1]);
          }
          if (b.feature < 0 || b.gain <= 0.0 || q.level == max_depth) continue;  // a leaf
          const int32_t id = tree[q.pos].id;
          tree[q.pos].feature = b.feature;
          tree[q.pos].threshold = thr[(size_t)b.feature * T + b.split];
          tree[q.pos].gain = b.gain;
          dec[i].feature = b.feature;
          dec[i].split = b.split;
          for (int side = 0; side < 2; ++side) {
            const double* c = side == 0 ? b.left : b.right;
            const double imp = dtree::impurity(impurity, c[0], c[1]);
            const int32_t child = (int32_t)tree.size();
            tree.push_back(eegfx_tree_node{2 * id + side, -1, -1, -1, 0.0, dtree::predict_of(c),
                                           imp, 0.0});
            (side == 0 ? tree[q.pos].left : tree[q.pos].right) = child;
            if (!(q.level + 1 == max_depth || imp == 0.0)) child_pos[2 * (size_t)i + side] = child;
          }
          total += 2;
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
      DtDecision* ddec = (DtDecision*)ctx->dt_dec.get(sizeof(DtDecision) * dec.size());
      HIP_CHECK(hipMemcpyAsync(ddec, dec.data(), sizeof(DtDecision) * dec.size(),
                               hipMemcpyHostToDevice, st));
      HIP_CHECK(launch_rf_route(st, binned.bins, n, d, dtab + group_trees_at, group_nt, s0, gn,
                                ddec, slot));
      HIP_CHECK(hipStreamSynchronize(st));  // `dec` and `tab` are rewritten for the next group
    }
    ctx->drain();
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
    if (n < 0 || d < 1 || d > kLrMaxFeatures) fail(EEGFX_EINVAL, "n=%lld d=%d", (long long)n, d);
    if (num_trees < 1) fail(EEGFX_EINVAL, "num_trees %d", num_trees);
    if (!nodes || !tree_offsets || (n > 0 && (!X || !out))) fail(EEGFX_EINVAL, "null argument");
    if (!rforest::forest_valid(nodes, tree_offsets, num_trees, d))
      fail(EEGFX_EINVAL, "the node array is not a forest of %d trees over %d features", num_trees,
           d);
    if (n == 0) return;
    ctx->activate();
    const hipStream_t st = ctx->stream;
    const double* dX = X;
    double* dout = out;
    if (mem == EEGFX_MEM_HOST) {
      double* bx = (double*)ctx->lr_x.get(sizeof(double) * (size_t)(n * d));
      HIP_CHECK(hipMemcpyAsync(bx, X, sizeof(double) * (size_t)(n * d), hipMemcpyHostToDevice, st));
      dX = bx;
      dout = (double*)ctx->lr_y.get(sizeof(double) * (size_t)n);
    }
    const int32_t n_nodes = tree_offsets[num_trees];
    std::vector<DtNode> hn((size_t)n_nodes);
    for (int32_t i = 0; i < n_nodes; ++i)
      hn[i] = DtNode{nodes[i].feature, nodes[i].left, nodes[i].right, 0, nodes[i].threshold,
                     nodes[i].predict};
    DtNode* dn = (DtNode*)ctx->dt_dec.get(sizeof(DtNode) * hn.size());
    int32_t* doff = (int32_t*)ctx->rf_tab.get(sizeof(int32_t) * ((size_t)num_trees + 1));
    HIP_CHECK(hipMemcpyAsync(dn, hn.data(), sizeof(DtNode) * hn.size(), hipMemcpyHostToDevice, st));
    HIP_CHECK(hipMemcpyAsync(doff, tree_offsets, sizeof(int32_t) * ((size_t)num_trees + 1),
                             hipMemcpyHostToDevice, st));
    HIP_CHECK(launch_rf_predict(st, dX, n, d, dn, doff, num_trees, dout));
    if (mem == EEGFX_MEM_HOST)
      HIP_CHECK(hipMemcpyAsync(out, dout, sizeof(double) * (size_t)n, hipMemcpyDeviceToHost, st));
    ctx->drain();
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
