// rforest.hip -- the O(trees n) passes of train_clf=rf on the GPU: MLlib
// 1.6.2 RandomForest as Classification/RandomForestClassifier.java:101-136 runs it.  The rows are
// binned once by dtree.hip's dt_bin_kernel; the host (tree_driver.cpp over rforest_host.h) draws
// the bagging weights and the feature subsets and chooses every split.  Per tree and row there is
// a weight (uint8 [tree][row]) and a slot (int32 [tree][row]): the queue ticket of the node the
// row sits in, -1 when that node is a leaf or the weight is 0.  A group of nodes leaves the queue
// with consecutive tickets, so "slot - s0 < g" selects a launch's rows as dt_hist_kernel does.
//   rf_init_kernel     slot[tree][row] = tree (the root's ticket), or -1 for weight 0.
//   rf_hist_kernel     one launch histograms g consecutive tickets over the trees they belong to.
//                      A wave takes a row, keeps its bins in registers (d <= 64: one byte per lane,
//                      read by a lane shuffle) and its lanes take the (tree, list position j)
//                      pairs: lane p looks up the row's slot in that tree, the node's j-th feature
//                      and adds the weight to h[node][j][bin][label].  Different trees are
//                      different nodes, so the lanes of one LDS atomic hit distinct counters.
//                      Privatised in 128 KB of LDS and merged with integer atomics, non-zero
//                      counters only; a node too large for LDS adds to global memory directly.
//   rf_route_kernel    per (tree, row) of the group's trees: slot -> the child's ticket, or -1
//                      (the single unweighted tree's rows too: one tree, dt_bin_kernel's slots).
//   rf_predict_kernel  one row per lane walks every tree; 1.0 iff more trees say 1 than 0.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "hist_lds.h"
#include "launch.h"

namespace eegfx {
namespace dev {

constexpr int kRfHistThreads = 1024;  // one workgroup per CU (its LDS), 16 waves
constexpr int kRfHistRows = 8;        // consecutive rows per wave: a slot column's line is reused

__global__ __launch_bounds__(256) void rf_init_kernel(const uint8_t* __restrict__ weight,
                                                      int64_t n, int num_trees,
                                                      int32_t* __restrict__ slot) {
  for (int t = blockIdx.y; t < num_trees; t += gridDim.y)
    for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r < n;
         r += (int64_t)gridDim.x * blockDim.x)
      slot[(int64_t)t * n + r] = weight[(int64_t)t * n + r] ? t : -1;
}

// ONE: d <= 64, the row's bins are one byte per lane.  trees[nt]: the distinct trees of the
// launch's nodes; sub[g][k]: the features of local node s (nullptr: feature j, k == d).
template <bool LDS, bool ONE>
__global__ __launch_bounds__(kRfHistThreads) void rf_hist_kernel(
    const uint8_t* __restrict__ bins, const uint8_t* __restrict__ label,
    const uint8_t* __restrict__ weight, const int32_t* __restrict__ slot, int64_t n, int d, int B,
    int k, int s0, int g, const int32_t* __restrict__ trees, int nt,
    const int32_t* __restrict__ sub, uint32_t* __restrict__ hist) {
  __shared__ uint32_t h[LDS ? kDtLdsCounters : 1];
  const int node_counters = k * B * 2;
  const int used = LDS ? g * node_counters : 0;  // <= kDtLdsCounters (launch_rf_hist)
  if (LDS) lds_hist_zero(h, used);
  const int lane = threadIdx.x & 63;
  const int waves = (int)blockDim.x >> 6;
  const int pairs = nt * k;
  const int64_t stride = (int64_t)gridDim.x * waves * kRfHistRows;
  for (int64_t r0 = ((int64_t)blockIdx.x * waves + (threadIdx.x >> 6)) * kRfHistRows; r0 < n;
       r0 += stride) {
    for (int u = 0; u < kRfHistRows && r0 + u < n; ++u) {  // wave-uniform
      const int64_t r = r0 + u;
      const uint8_t* row = bins + r * d;
      const int lab = label[r];
      int mine = 0;
      if (ONE) mine = lane < d ? row[lane] : 0;
      // every lane runs every trip: the shuffle below reads other lanes' registers
      for (int p0 = 0; p0 < pairs; p0 += 64) {
        const int p = p0 + lane;
        const bool in = p < pairs;
        const int ti = in ? p / k : 0;
        const int j = p - ti * k;
        const int64_t at = (int64_t)trees[ti] * n + r;
        const int s = in ? slot[at] - s0 : -1;
        const bool ok = (unsigned)s < (unsigned)g;  // this tree's node of the row is in the launch
        const int f = ok ? (sub ? sub[s * k + j] : j) : 0;  // < d (rforest::reservoir)
        const int bin = ONE ? __shfl(mine, f) : (int)row[f];  // < B (dt_bin_kernel)
        if (ok) {
          const uint32_t w = weight[at];
          const size_t i = (size_t)s * node_counters + (size_t)(j * B + bin) * 2 + lab;
          if (LDS) atomicAdd(&h[i], w); else atomicAdd(&hist[i], w);
        }
      }
    }
  }
  if (LDS) lds_hist_merge(h, used, hist);
}

__global__ __launch_bounds__(256) void rf_route_kernel(const uint8_t* __restrict__ bins, int64_t n,
                                                       int d, const int32_t* __restrict__ trees,
                                                       int nt, int s0, int g,
                                                       const DtDecision* __restrict__ dec,
                                                       int32_t* __restrict__ slot) {
  for (int ti = blockIdx.y; ti < nt; ti += gridDim.y) {
    int32_t* col = slot + (int64_t)trees[ti] * n;
    for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r < n;
         r += (int64_t)gridDim.x * blockDim.x) {
      const int s = col[r] - s0;
      if ((unsigned)s >= (unsigned)g) continue;  // a leaf's row, or a node still queued
      const DtDecision dc = dec[s];
      if (dc.feature < 0)
        col[r] = -1;
      else
        col[r] = (int)bins[r * d + dc.feature] <= dc.split ? dc.left : dc.right;
    }
  }
}

__global__ __launch_bounds__(256) void rf_predict_kernel(const double* __restrict__ X, int64_t n,
                                                         int d, const DtNode* __restrict__ nodes,
                                                         const int32_t* __restrict__ offsets,
                                                         int num_trees, double* __restrict__ out) {
  for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r < n;
       r += (int64_t)gridDim.x * blockDim.x) {
    const double* x = X + r * d;
    int ones = 0;
    for (int t = 0; t < num_trees; ++t) {
      const DtNode* tree = nodes + offsets[t];
      const int count = offsets[t + 1] - offsets[t];
      int i = 0;
      // children lie after their parent (rforest::forest_valid), so a walk takes < count steps
      for (int step = 0; step < count && tree[i].feature >= 0; ++step)
        i = x[tree[i].feature] <= tree[i].threshold ? tree[i].left : tree[i].right;
      ones += tree[i].predict == 1.0 ? 1 : 0;
    }
    out[r] = ones > num_trees - ones ? 1.0 : 0.0;  // a tie is 0.0
  }
}

}  // namespace dev

hipError_t launch_rf_init(hipStream_t st, const uint8_t* weight, int64_t n, int num_trees,
                          int32_t* slot) {
  const dim3 grid(grid_for(n, 256 * 4, 1024), grid_for(num_trees, 1, 1024));
  hipLaunchKernelGGL(dev::rf_init_kernel, grid, dim3(256), 0, st, weight, n, num_trees, slot);
  return hipGetLastError();
}

hipError_t launch_rf_hist(hipStream_t st, const uint8_t* bins, const uint8_t* label,
                          const uint8_t* weight, const int32_t* slot, int64_t n, int d, int B,
                          int k, int s0, int g, const int32_t* trees, int nt, const int32_t* sub,
                          uint32_t* hist) {
  // one workgroup per CU; at least one block of rows for every wave of a workgroup
  const dim3 grid(grid_for(n, (dev::kRfHistThreads / 64) * dev::kRfHistRows, 256));
  const dim3 block(dev::kRfHistThreads);
  const bool lds = (int64_t)g * k * B * 2 <= kDtLdsCounters;
#define EEGFX_RF_HIST(L, O)                                                                      \
  hipLaunchKernelGGL((dev::rf_hist_kernel<L, O>), grid, block, 0, st, bins, label, weight, slot, \
                     n, d, B, k, s0, g, trees, nt, sub, hist)
  if (lds && d <= 64)
    EEGFX_RF_HIST(true, true);
  else if (lds)
    EEGFX_RF_HIST(true, false);
  else  // k <= d <= 64 features of at most 256 bins fit LDS
    EEGFX_RF_HIST(false, false);
#undef EEGFX_RF_HIST
  return hipGetLastError();
}

hipError_t launch_rf_route(hipStream_t st, const uint8_t* bins, int64_t n, int d,
                           const int32_t* trees, int nt, int s0, int g, const DtDecision* dec,
                           int32_t* slot) {
  const dim3 grid(grid_for(n, 256, 2048), grid_for(nt, 1, 1024));
  hipLaunchKernelGGL(dev::rf_route_kernel, grid, dim3(256), 0, st, bins, n, d, trees, nt, s0, g,
                     dec, slot);
  return hipGetLastError();
}

hipError_t launch_rf_predict(hipStream_t st, const double* X, int64_t n, int d,
                             const DtNode* nodes, const int32_t* offsets, int num_trees,
                             double* out) {
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(dev::rf_predict_kernel, dim3(grid_for(n, 256, 8192)), dim3(256), 0, st, X, n,
                     d, nodes, offsets, num_trees, out);
  return hipGetLastError();
}

}  // namespace eegfx
