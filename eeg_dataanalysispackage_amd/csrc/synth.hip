// synth.hip -- deterministic synthetic recordings for tests and bench.py (gfx950).
//   synth_kernel                 int16 recordings: drift, a 10 Hz sinusoid, noise, saturations
// Compiled with -ffp-contract=off: every fp32/fp64 expression is evaluated as written, one
// correctly rounded IEEE operation at a time, matching the Java (strictfp-equivalent) order.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "launch.h"

namespace eegfx {
namespace dev {

__device__ __forceinline__ uint64_t splitmix64(uint64_t z) {
  z += 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
__device__ __forceinline__ float unit_noise(uint64_t seed, uint64_t key) {  // [-1, 1)
  return (float)(splitmix64(seed ^ splitmix64(key)) >> 40) * (2.0f / 16777216.0f) - 1.0f;
}

// DC -25000 counts, a bounded random walk (piecewise-linear between random knots every 64 and
// 1024 frames), a 10 Hz sinusoid of 200 counts and white noise, clipped to int16; about one
// sample in 65536 is a -32768 saturation.
__global__ __launch_bounds__(256) void synth_kernel(int16_t* __restrict__ dst, int64_t n_frames,
                                                    int ct, uint64_t seed) {
  const int64_t total = n_frames * ct;
  for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total;
       idx += (int64_t)gridDim.x * blockDim.x) {
    const int64_t t = idx / ct;
    const int c = (int)(idx - t * ct);
    const uint64_t ck = (uint64_t)c << 48;
    const int64_t k1 = t >> 6, k2 = t >> 10;
    const float f1 = (float)(t & 63) * (1.0f / 64.0f), f2 = (float)(t & 1023) * (1.0f / 1024.0f);
    const float w1 = unit_noise(seed, ck | (uint64_t)(2 * k1)) * (1.0f - f1) +
                     unit_noise(seed, ck | (uint64_t)(2 * k1 + 2)) * f1;
    const float w2 = unit_noise(seed + 1, ck | (uint64_t)k2) * (1.0f - f2) +
                     unit_noise(seed + 1, ck | (uint64_t)(k2 + 1)) * f2;
    const float sine = 200.0f * __sinf(6.2831853f * 10.0f * (float)(t % 1000) / 1000.0f + (float)c);
    const float noise = 40.0f * unit_noise(seed + 2, (uint64_t)idx);
    float v = -25000.0f + 1500.0f * w1 + 4000.0f * w2 + sine + noise;
    if (unit_noise(seed + 3, (uint64_t)idx) < -0.99997f) v = -40000.0f;
    v = fminf(fmaxf(v, -32768.0f), 32767.0f);
    dst[idx] = (int16_t)__float2int_rn(v);
  }
}

}  // namespace dev

hipError_t launch_synth(hipStream_t st, int16_t* dst, int64_t n_frames, int ct, uint64_t seed) {
  const int64_t total = n_frames * ct;
  if (total == 0) return hipSuccess;
  int64_t blocks = (total + 255) / 256;
  if (blocks > 65536) blocks = 65536;
  hipLaunchKernelGGL(dev::synth_kernel, dim3((unsigned)blocks), dim3(256), 0, st, dst, n_frames,
                     ct, seed);
  return hipGetLastError();
}

}  // namespace eegfx
