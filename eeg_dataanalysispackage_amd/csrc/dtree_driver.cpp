// dtree_driver.cpp -- the drivers of eegfx_dtree_train / eegfx_dtree_predict: MLlib 1.6.2
// DecisionTree (DecisionTreeClassifier.java:99-127) with the O(n d) passes on the device
// (dtree.hip) and the threshold search and split selection on the host (dtree_host.h), DESIGN.md
// section 10.
#include <cmath>
#include <cstring>
#include <vector>

#include "ctx.h"
#include "dtree_host.h"
#include "spark_sample.h"

// Device memory one group of node histograms may take (a node's histogram is d * bins * 2
// counters; a level with more active nodes than fit is histogrammed group by group).
static constexpr size_t kDtHistBudget = (size_t)16 << 20;

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

  const double* dX = X;
  const double* dy = y;
  if (mem == EEGFX_MEM_HOST) {
    double* bx = (double*)ctx->lr_x.get(sizeof(double) * (size_t)(n * d));
    double* by = (double*)ctx->lr_y.get(sizeof(double) * (size_t)n);
    HIP_CHECK(hipMemcpyAsync(bx, X, sizeof(double) * (size_t)(n * d), hipMemcpyHostToDevice, st));
    HIP_CHECK(hipMemcpyAsync(by, y, sizeof(double) * (size_t)n, hipMemcpyHostToDevice, st));
    dX = bx;
    dy = by;
  }
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
    const unsigned hw = std::max(1u, std::thread::hardware_concurrency());
    const int W = (int)std::min({(unsigned)d, 8u, hw});
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

extern "C" {

int eegfx_dtree_train(eegfx_ctx* ctx, const double* X, const double* y, int64_t n, int32_t d,
                      int32_t impurity, int32_t max_depth, int32_t max_bins,
                      int32_t min_instances_per_node, int64_t split_seed, eegfx_tree_node* nodes,
                      int32_t capacity, int32_t* n_nodes, int mem) {
  return guarded([&] {
    if (!ctx) fail(EEGFX_EINVAL, "null context");
    check_mem(mem);
    // n == 1: numBins = 1 leaves no split, and Spark's assertion fails
    if (n < 2 || n > INT32_MAX) fail(EEGFX_EINVAL, "n=%lld outside [2, 2^31)", (long long)n);
    if (d < 1 || d > kLrMaxFeatures) fail(EEGFX_EINVAL, "d=%d outside [1, %d]", d, kLrMaxFeatures);
    if (capacity < 0) fail(EEGFX_EINVAL, "capacity %d", capacity);
    if (!X || !y || !n_nodes || (capacity > 0 && !nodes)) fail(EEGFX_EINVAL, "null argument");
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
    ctx->activate();
    const hipStream_t st = ctx->stream;
    const int B = (int)std::min<int64_t>(max_bins, n), T = B - 1;  // numBins, numSplits
    const size_t node_counters = (size_t)d * B * 2, node_bytes = node_counters * sizeof(uint32_t);
    // active nodes per histogram launch
    int G = (int)std::max<size_t>(1, kDtHistBudget / node_bytes);
    if (node_counters <= (size_t)kDtLdsCounters)
      G = std::min(G, (int)(kDtLdsCounters / node_counters));

    DtBinned binned;
    dt_bin_rows(ctx, X, y, n, d, max_bins, split_seed, mem, (size_t)G * node_bytes, &binned);
    const int32_t* nthr = binned.nthr;
    const double* thr = binned.thr;
    std::vector<uint8_t>& tab = binned.tab;
    uint8_t* const dtab = binned.dtab;
    uint8_t* const bins = binned.bins;
    uint8_t* const label = binned.label;
    int32_t* const slot = binned.slot;
    void* const scratch = binned.scratch;

    // ---- the tree, level by level
    std::vector<eegfx_tree_node> out;
    out.push_back(eegfx_tree_node{1, -1, -1, -1, 0.0, 0.0, 0.0, 0.0});
    std::vector<int32_t> active{0}, next;  // positions in `out`; a node's slot is its index here
    std::vector<uint32_t> hist((size_t)G * node_counters);
    std::vector<DtDecision> dec;
    uint32_t* dhist = (uint32_t*)scratch;
    for (int level = 0; !active.empty(); ++level) {
      dec.assign(active.size(), DtDecision{-1, -1, -1, -1});
      next.clear();
      for (size_t g0 = 0; g0 < active.size(); g0 += (size_t)G) {
        const int g = (int)std::min<size_t>((size_t)G, active.size() - g0);
        HIP_CHECK(hipMemsetAsync(dhist, 0, (size_t)g * node_bytes, st));
        ctx->tic();
        HIP_CHECK(launch_dt_hist(st, bins, label, slot, n, d, B, (int)g0, g, dhist));
        ctx->toc(n * (int64_t)d + 5 * n);
        HIP_CHECK(hipMemcpyAsync(hist.data(), dhist, (size_t)g * node_bytes, hipMemcpyDeviceToHost,
                                 st));
        if (level == 0)
          HIP_CHECK(hipMemcpyAsync(tab.data(), dtab, 16, hipMemcpyDeviceToHost, st));
        HIP_CHECK(hipStreamSynchronize(st));
        if (level == 0) {
          const int32_t* flags = (const int32_t*)tab.data();
          if (flags[0]) fail(EEGFX_EINVAL, "a training feature is not finite");
          if (flags[1]) fail(EEGFX_EINVAL, "Input validation failed: labels must be 0.0 or 1.0");
        }
        for (int k = 0; k < g; ++k) {
          const dtree::Best b = dtree::best_split(hist.data() + (size_t)k * node_counters, d, B,
                                                  nthr, impurity, min_instances_per_node);
          const int32_t pos = active[g0 + k];
          if (level == 0) {
            out[pos].predict = dtree::predict_of(b.tot);
            out[pos].impurity = dtree::impurity(impurity, b.tot[0], b.tot[1]);
          }
          if (b.feature < 0 || b.gain <= 0.0 || level == max_depth) continue;  // a leaf
          const int32_t id = out[pos].id;
          out[pos].feature = b.feature;
          out[pos].threshold = thr[(size_t)b.feature * T + b.split];
          out[pos].gain = b.gain;
          DtDecision& dc = dec[g0 + k];
          dc.feature = b.feature;
          dc.split = b.split;
          for (int side = 0; side < 2; ++side) {
            const double* c = side == 0 ? b.left : b.right;
            const double imp = dtree::impurity(impurity, c[0], c[1]);
            const int32_t child = (int32_t)out.size();
            out.push_back(eegfx_tree_node{2 * id + side, -1, -1, -1, 0.0, dtree::predict_of(c),
                                          imp, 0.0});
            (side == 0 ? out[pos].left : out[pos].right) = child;
            int32_t child_slot = -1;
            if (!(level + 1 == max_depth || imp == 0.0)) {
              child_slot = (int32_t)next.size();
              next.push_back(child);
            }
            (side == 0 ? dc.left : dc.right) = child_slot;
          }
        }
      }
      if (next.empty()) break;
      DtDecision* ddec = (DtDecision*)ctx->dt_dec.get(sizeof(DtDecision) * dec.size());
      HIP_CHECK(hipMemcpyAsync(ddec, dec.data(), sizeof(DtDecision) * dec.size(),
                               hipMemcpyHostToDevice, st));
      HIP_CHECK(launch_dt_route(st, bins, n, d, ddec, slot));
      HIP_CHECK(hipStreamSynchronize(st));  // `dec` is rewritten for the next level
      active.swap(next);
    }
    ctx->drain();
    *n_nodes = (int32_t)out.size();
    if ((size_t)capacity < out.size())
      fail(EEGFX_EINVAL, "the tree has %zu nodes, capacity is %d", out.size(), capacity);
    memcpy(nodes, out.data(), sizeof(eegfx_tree_node) * out.size());
  });
}

int eegfx_dtree_predict(eegfx_ctx* ctx, const double* X, int64_t n, int32_t d,
                        const eegfx_tree_node* nodes, int32_t n_nodes, double* out, int mem) {
  return guarded([&] {
    if (!ctx) fail(EEGFX_EINVAL, "null context");
    check_mem(mem);
    if (n < 0 || d < 1 || d > kLrMaxFeatures) fail(EEGFX_EINVAL, "n=%lld d=%d", (long long)n, d);
    if (n_nodes < 1) fail(EEGFX_EINVAL, "n_nodes %d", n_nodes);
    if (!nodes || (n > 0 && (!X || !out))) fail(EEGFX_EINVAL, "null argument");
    if (!dtree::nodes_valid(nodes, n_nodes, d))
      fail(EEGFX_EINVAL, "the node array is not a tree over %d features", d);
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
    std::vector<DtNode> hn((size_t)n_nodes);
    for (int32_t i = 0; i < n_nodes; ++i)
      hn[i] = DtNode{nodes[i].feature, nodes[i].left, nodes[i].right, 0, nodes[i].threshold,
                     nodes[i].predict};
    DtNode* dn = (DtNode*)ctx->dt_dec.get(sizeof(DtNode) * hn.size());
    HIP_CHECK(hipMemcpyAsync(dn, hn.data(), sizeof(DtNode) * hn.size(), hipMemcpyHostToDevice, st));
    HIP_CHECK(launch_dt_predict(st, dX, n, d, dn, n_nodes, dout));
    if (mem == EEGFX_MEM_HOST)
      HIP_CHECK(hipMemcpyAsync(out, dout, sizeof(double) * (size_t)n, hipMemcpyDeviceToHost, st));
    ctx->drain();
  });
}

}  // extern "C"
