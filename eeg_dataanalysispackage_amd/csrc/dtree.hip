// dtree.hip -- the O(n d) passes of train_clf=dt on the GPU: MLlib 1.6.2
// DecisionTree as Classification/DecisionTreeClassifier.java:99-127 runs it.  The host
// (tree_driver.cpp over dtree_host.h) finds the thresholds from the sampled rows and chooses
// every split from integer histograms; these kernels do everything that touches all rows (the
// rows are routed to their children by rforest.hip's rf_route_kernel, with one tree):
//   dt_bin_kernel      X double[n][d] -> bins uint8[n][d] by binary search in the per-feature
//                      threshold table (bin = thresholds below the value; bin k is (t[k-1], t[k]]),
//                      labels -> uint8, every row's node slot = 0 (the root); flags a non-finite
//                      feature and a label other than 0.0 / 1.0, as lr_validate_kernel does.
//   dt_hist_kernel     one pass per launch of g queued nodes (tickets g0 .. g0 + g - 1): a row
//                      whose slot lies there adds 1 to hist[slot - g0][feature][bin][label].  A
//                      wave takes a row, its lanes the features (lane k: k, k + 64, ...), so the
//                      lanes of one LDS atomic hit distinct counters.  Privatised in 128 KB of LDS
//                      per workgroup and merged with integer atomics (hist_lds.h; counts: no order
//                      enters the result); a launch whose histograms do not fit LDS adds to global
//                      memory directly.
//   dt_predict_kernel  one row per lane walks the node array: left iff x[feature] <= threshold.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "hist_lds.h"
#include "launch.h"

namespace eegfx {
namespace dev {

constexpr int kDtHistThreads = 1024;  // one workgroup per CU (its LDS), 16 waves
constexpr int kDtHistRows = 4;        // rows per wave whose slots are loaded together
constexpr int kDtHistWide = 8;        // the same when a row is one byte per lane (d <= 64)

__global__ __launch_bounds__(256) void dt_bin_kernel(
    const double* __restrict__ X, const double* __restrict__ y, int64_t n, int d, int T,
    const int32_t* __restrict__ nthr, const double* __restrict__ thr, int32_t* __restrict__ flags,
    uint8_t* __restrict__ bins, uint8_t* __restrict__ label, int32_t* __restrict__ slot) {
  // element e = r * d + f; (r, f) advance with e without a division per element
  const int64_t total = n * d, step = (int64_t)gridDim.x * blockDim.x;
  const int64_t step_r = step / d;
  const int step_f = (int)(step % d);
  int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  int64_t r = e / d;
  int f = (int)(e % d);
  for (; e < total; e += step) {
    const double x = X[e];
    if (!(__builtin_fabs(x) <= __DBL_MAX__)) flags[0] = 1;
    const double* t = thr + (int64_t)f * T;
    int lo = 0, hi = nthr[f];
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (t[mid] < x) lo = mid + 1; else hi = mid;
    }
    bins[e] = (uint8_t)lo;  // <= nthr[f] <= T <= 255
    if (f == 0) {
      const double yy = y[r];
      if (!(yy == 0.0 || yy == 1.0)) flags[1] = 1;
      label[r] = yy == 1.0 ? 1 : 0;
      slot[r] = 0;
    }
    r += step_r;
    f += step_f;
    if (f >= d) {
      f -= d;
      ++r;
    }
  }
}

// ONE: d <= 64, a row is one byte per lane.  The slots of kDtHistWide rows are loaded together,
// then the label and the bin of every row of them that belongs to the group, then the atomics: two
// load latencies per 8 rows instead of three per row.
template <bool LDS, bool ONE>
__global__ __launch_bounds__(kDtHistThreads) void dt_hist_kernel(
    const uint8_t* __restrict__ bins, const uint8_t* __restrict__ label,
    const int32_t* __restrict__ slot, int64_t n, int d, int B, int g0, int g,
    uint32_t* __restrict__ hist) {
  static_assert(LDS || !ONE, "64 features of 256 bins fit LDS");
  __shared__ uint32_t h[LDS ? kDtLdsCounters : 1];
  const int node_counters = d * B * 2;
  const int used = LDS ? g * node_counters : 0;  // <= kDtLdsCounters (launch_dt_hist)
  if (LDS) lds_hist_zero(h, used);
  const int lane = threadIdx.x & 63;
  const int waves = (int)blockDim.x >> 6;
  constexpr int U = ONE ? kDtHistWide : kDtHistRows;
  const int64_t stride = (int64_t)gridDim.x * waves * U;
  for (int64_t r0 = ((int64_t)blockIdx.x * waves + (threadIdx.x >> 6)) * U; r0 < n;
       r0 += stride) {
    int s[U];
#pragma unroll
    for (int u = 0; u < U; ++u) s[u] = r0 + u < n ? slot[r0 + u] - g0 : -1;
    if constexpr (ONE) {
      int at[U];  // the lane's counter of row u, -1: none
#pragma unroll
      for (int u = 0; u < U; ++u) {
        // s[u] in [0, g) only for a row below n that belongs to the group (wave-uniform)
        const bool ok = (unsigned)s[u] < (unsigned)g && lane < d;
        const int64_t r = r0 + u;
        const int lab = ok ? label[r] : 0, bin = ok ? bins[r * d + lane] : 0;  // bin < B
        at[u] = ok ? s[u] * node_counters + (lane * B + bin) * 2 + lab : -1;
      }
#pragma unroll
      for (int u = 0; u < U; ++u)
        if (at[u] >= 0) atomicAdd(&h[at[u]], 1u);
    } else {
#pragma unroll
      for (int u = 0; u < U; ++u) {
        if ((unsigned)s[u] >= (unsigned)g) continue;  // wave-uniform: a leaf's row, another group's
        const int64_t r = r0 + u;
        const uint8_t* row = bins + r * d;
        const size_t base = (size_t)s[u] * node_counters + label[r];
        for (int f = lane; f < d; f += 64) {
          const size_t i = base + (size_t)(f * B + row[f]) * 2;  // row[f] < B (dt_bin_kernel)
          if (LDS) atomicAdd(&h[i], 1u); else atomicAdd(&hist[i], 1u);
        }
      }
    }
  }
  if (LDS) lds_hist_merge(h, used, hist);
}

__global__ __launch_bounds__(256) void dt_gather_kernel(const double* __restrict__ X, int d,
                                                        const int64_t* __restrict__ idx, int64_t m,
                                                        double* __restrict__ out) {
  const int64_t total = m * d;
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total;
       e += (int64_t)gridDim.x * blockDim.x) {
    const int64_t i = e / d;
    out[e] = X[idx[i] * d + (e - i * d)];
  }
}

__global__ __launch_bounds__(256) void dt_predict_kernel(const double* __restrict__ X, int64_t n,
                                                         int d, const DtNode* __restrict__ nodes,
                                                         int n_nodes, double* __restrict__ out) {
  for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r < n;
       r += (int64_t)gridDim.x * blockDim.x) {
    int i = 0;
    // children lie after their parent (dtree::nodes_valid), so a walk takes < n_nodes steps
    for (int step = 0; step < n_nodes && nodes[i].feature >= 0; ++step)
      i = X[r * d + nodes[i].feature] <= nodes[i].threshold ? nodes[i].left : nodes[i].right;
    out[r] = nodes[i].predict;
  }
}

}  // namespace dev

hipError_t launch_dt_bin(hipStream_t st, const double* X, const double* y, int64_t n, int d,
                         int T, const int32_t* nthr, const double* thr, int32_t* flags,
                         uint8_t* bins, uint8_t* label, int32_t* slot) {
  hipLaunchKernelGGL(dev::dt_bin_kernel, dim3(grid_for(n * d, 256 * 8, 8192)), dim3(256), 0, st, X,
                     y, n, d, T, nthr, thr, flags, bins, label, slot);
  return hipGetLastError();
}

hipError_t launch_dt_hist(hipStream_t st, const uint8_t* bins, const uint8_t* label,
                          const int32_t* slot, int64_t n, int d, int B, int g0, int g,
                          uint32_t* hist) {
  // one workgroup per CU; at least one group of rows for every wave of a workgroup
  const dim3 grid(grid_for(n, (dev::kDtHistThreads / 64) * dev::kDtHistWide, 256));
  const dim3 block(dev::kDtHistThreads);
  const bool lds = (int64_t)g * d * B * 2 <= kDtLdsCounters;
  if (lds && d <= 64)
    hipLaunchKernelGGL((dev::dt_hist_kernel<true, true>), grid, block, 0, st, bins, label, slot,
                       n, d, B, g0, g, hist);
  else if (lds)
    hipLaunchKernelGGL((dev::dt_hist_kernel<true, false>), grid, block, 0, st, bins, label, slot,
                       n, d, B, g0, g, hist);
  else
    hipLaunchKernelGGL((dev::dt_hist_kernel<false, false>), grid, block, 0, st, bins, label, slot,
                       n, d, B, g0, g, hist);
  return hipGetLastError();
}

hipError_t launch_dt_gather(hipStream_t st, const double* X, int d, const int64_t* idx, int64_t m,
                            double* out) {
  hipLaunchKernelGGL(dev::dt_gather_kernel, dim3(grid_for(m * d, 256, 4096)), dim3(256), 0, st, X,
                     d, idx, m, out);
  return hipGetLastError();
}

hipError_t launch_dt_predict(hipStream_t st, const double* X, int64_t n, int d,
                             const DtNode* nodes, int n_nodes, double* out) {
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(dev::dt_predict_kernel, dim3(grid_for(n, 256, 8192)), dim3(256), 0, st, X, n,
                     d, nodes, n_nodes, out);
  return hipGetLastError();
}

}  // namespace eegfx
