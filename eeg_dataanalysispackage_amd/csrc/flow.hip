// flow.hip -- the two bandwidth-bound passes of the train/test flow, the
// glue of PipelineBuilder.execute's train_clf branch (:170-223) between the provider's resident
// rows and the classifiers:
//   gather_rows_kernel  dst[i][0:d] = src[idx[i]][0:d]: the shuffled order of Collections.shuffle
//                       applied to the feature rows (and, with d = 1, to the labels).  A row is d
//                       doubles moved as bits (NaN payloads and -0.0 survive), in 16-byte pieces
//                       when src, dst and d allow it (launch_gather_rows decides per launch), else
//                       in 8-byte pieces.  Piece e = i * dv + c; a thread takes kGatherUnroll
//                       pieces a grid stride apart per trip: their indices are loaded together,
//                       then their source pieces, then the stores, so four loads are in flight per
//                       lane.  (i, c) advance with e without a division per piece.  An index
//                       outside [0, n_src) copies nothing; the smallest such i lands in *bad.
//   confusion_kernel    one pass over pred[n] and labels[n]: the four cells of the confusion matrix
//                       as unsigned 64-bit counts, summed per lane, then per wave (shuffles), then
//                       one atomic per wave and non-zero counter.  Which actual classes occur and
//                       whether a label is neither 0.0 nor 1.0 are wave-reduced bits of one word.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "launch.h"

namespace eegfx {
namespace dev {

template <typename V>
__global__ __launch_bounds__(kGatherThreads) void gather_rows_kernel(
    const V* __restrict__ src, int64_t n_src, int dv, const int64_t* __restrict__ idx, int64_t m,
    V* __restrict__ dst, unsigned long long* __restrict__ bad) {
  constexpr int U = kGatherUnroll;
  const int64_t total = m * dv, step = (int64_t)gridDim.x * blockDim.x;
  const int64_t step_i = step / dv;
  const int step_c = (int)(step % dv);
  int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  int64_t i = e / dv;
  int c = (int)(e - i * dv);
  for (; e < total; e += step * U) {
    int64_t row[U], from[U];
    int col[U];
    V v[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      row[u] = i;
      col[u] = c;
      i += step_i;
      c += step_c;
      if (c >= dv) {
        c -= dv;
        ++i;
      }
    }
#pragma unroll
    for (int u = 0; u < U; ++u) from[u] = e + u * step < total ? idx[row[u]] : 0;
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const bool live = e + u * step < total;
      const bool ok = live && (uint64_t)from[u] < (uint64_t)n_src;
      if (live && !ok && col[u] == 0) atomicMin(bad, (unsigned long long)row[u]);
      if (!ok) row[u] = -1;
      v[u] = ok ? src[from[u] * dv + col[u]] : V();
    }
#pragma unroll
    for (int u = 0; u < U; ++u)
      if (row[u] >= 0) dst[row[u] * dv + col[u]] = v[u];
  }
}

__device__ inline unsigned long long wave_sum(unsigned long long v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
  return v;  // lane 0 holds the wave's sum
}

__global__ __launch_bounds__(kConfusionThreads) void confusion_kernel(
    const double* __restrict__ pred, const double* __restrict__ labels, int64_t n,
    ConfusionOut* __restrict__ out) {
  constexpr int U = 4;
  unsigned long long cell[4] = {0, 0, 0, 0};  // tp, tn, fp, fn in the reference's reading
  unsigned seen = 0;
  const int64_t step = (int64_t)gridDim.x * blockDim.x;
  for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r < n; r += step * U) {
    double a[U], p[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const bool live = r + u * step < n;
      a[u] = live ? labels[r + u * step] : 0.0;
      p[u] = live ? pred[r + u * step] : -1.0;  // -1: falls out of the matrix
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      if (r + u * step >= n) continue;
      const bool a1 = a[u] == 1.0, a0 = a[u] == 0.0;
      seen |= a1 ? kSeenOne : a0 ? kSeenZero : kSeenOther;
      const bool p1 = p[u] == 1.0, p0 = p[u] == 0.0;
      // cm[actual][predicted] flattened column-major and read as tn, fp, fn, tp: the reference's
      // "false positives" are actual 1 / predicted 0 (classification.reference_statistics)
      cell[0] += a1 && p1;
      cell[1] += a0 && p0;
      cell[2] += a1 && p0;
      cell[3] += a0 && p1;
    }
  }
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const unsigned long long s = wave_sum(cell[k]);
    if ((threadIdx.x & 63) == 0 && s) atomicAdd(&out->cell[k], s);
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) seen |= __shfl_down(seen, off, 64);
  if ((threadIdx.x & 63) == 0 && seen) atomicOr(&out->seen, seen);
}

}  // namespace dev

hipError_t launch_gather_rows(hipStream_t st, const double* src, int64_t n_src, int d,
                              const int64_t* idx, int64_t m, double* dst,
                              unsigned long long* bad) {
  if (m == 0) return hipSuccess;
  // rows of an odd d, or buffers that start 8 bytes off, are only 8-byte aligned
  const bool wide = d % 2 == 0 && ((uintptr_t)src | (uintptr_t)dst) % 16 == 0;
  const int dv = wide ? d / 2 : d;
  const dim3 grid(grid_for(m * dv, kGatherThreads * kGatherUnroll, kGatherMaxBlocks));
  if (wide)
    hipLaunchKernelGGL(dev::gather_rows_kernel<ulonglong2>, grid, dim3(kGatherThreads), 0, st,
                       (const ulonglong2*)src, n_src, dv, idx, m, (ulonglong2*)dst, bad);
  else
    hipLaunchKernelGGL(dev::gather_rows_kernel<unsigned long long>, grid, dim3(kGatherThreads), 0,
                       st, (const unsigned long long*)src, n_src, dv, idx, m,
                       (unsigned long long*)dst, bad);
  return hipGetLastError();
}

hipError_t launch_confusion(hipStream_t st, const double* pred, const double* labels, int64_t n,
                            ConfusionOut* out) {
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(dev::confusion_kernel, dim3(grid_for(n, kConfusionThreads * 4, 2048)),
                     dim3(kConfusionThreads), 0, st, pred, labels, n, out);
  return hipGetLastError();
}

}  // namespace eegfx
