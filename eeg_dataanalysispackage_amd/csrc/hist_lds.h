// hist_lds.h -- the workgroup-private histogram of dt_hist_kernel (dtree.hip) and rf_hist_kernel
// (rforest.hip): `used` uint32 counters in LDS, zeroed before the rows and merged into device memory
// after them with integer atomics, non-zero counters only (counts: no order enters the result).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace eegfx {
namespace dev {

__device__ inline void lds_hist_zero(uint32_t* h, int used) {
  for (int i = threadIdx.x; i < used; i += blockDim.x) h[i] = 0;
  __syncthreads();
}

__device__ inline void lds_hist_merge(const uint32_t* h, int used, uint32_t* __restrict__ hist) {
  __syncthreads();
  for (int i = threadIdx.x; i < used; i += blockDim.x) {
    const uint32_t v = h[i];
    if (v) atomicAdd(&hist[i], v);
  }
}

}  // namespace dev
}  // namespace eegfx
