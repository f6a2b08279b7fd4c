// pyramid.hip -- the full dwt-8 pyramid: feature sizes 17..512 (WaveletTransform's FEATURE_SIZE,
// WaveletTransform.java:126-137, :205-212).  A channel's features are the first nfeat coefficients
// of the in-place pyramid [a6(8) d6(8) d5(16) d4(32) d3(64) d2(128) d1(256)], the row is the C
// channels' features one after another, L2-normalised (SignalProcessing.java:38-52).
//
//   pyramid_from_epochs_kernel  materialised epochs / packed window rows -> wide feature rows
//
// It runs EXACT under both numerics settings (the fma conditioning guard has no bound for the
// detail bands).  A workgroup is one wave and owns up to 8 epochs.  Their
// signals (epoch m, channel c), numbered m * C + c, are taken 8 at a time, lane = 8 * signal +
// segment (dwt8.h).  A pass runs the pyramid of its 8 signals; every coefficient the feature size
// reaches goes to an LDS tile as it is produced (nothing beyond the cascade's own slices stays in
// registers), and the tile -- 8 consecutive channel blocks of the output, one contiguous run of
// 8 * nfeat doubles -- is stored to `out` unnormalised.  Lane m then adds the squares of epoch
// m's values of this pass to the epoch's sum, in index order: the reference sums Math.pow(f, 2)
// sequentially over the row and fp64 addition does not associate, so the adds form one serial
// chain per epoch (the squares are independent, the chain is not).  After the last pass the wave
// divides its rows in place (they are still in L2).
//
// A row is C * nfeat doubles, up to 256 KB at C = 64: it cannot wait in LDS for its norm, which
// is why the rows pass through `out` twice.
//
// A fused raw -> rows kernel of the same shape (windows staged as window_wide_kernel stages them,
// the decode fused into level 1) was built and measured against cut + this kernel: 37 % faster at
// nfeat = 32, 29 % slower at nfeat = 512, so eegfx_process_recording_fe runs
// the two passes.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <type_traits>

#include "dwt8.h"
#include "launch.h"

namespace eegfx {
namespace dev {

// The tile: signal g's coefficient j at g * ts + j + j / 32.  The pad per 32 coefficients puts
// the 8 segments' simultaneous writes of one band (strides 32, 16, ... doubles) on distinct
// banks, and ts = 8 (mod 32) doubles skews the 8 signals by 16 banks each.
__host__ __device__ constexpr int pyramid_tile_stride(int nfeat) {
  return (((nfeat - 1) + ((nfeat - 1) >> 5) + 1 - 8 + 31) / 32) * 32 + 8;
}
__device__ __forceinline__ int py_slot(int j) { return j + (j >> 5); }
constexpr int kPyMaxFeat = 512;
constexpr int kPyTileMax = 8 * pyramid_tile_stride(kPyMaxFeat);  // doubles

// Stores the tile's nv signals (sig0 .. sig0 + nv) to the block's rows `o` and continues the
// epochs' sums of squares: lane m < ne owns epoch m's sum.
__device__ __forceinline__ void pyramid_flush(const double* tile, int ts, int sig0, int nv, int C,
                                              int nf, int ne, double* __restrict__ o, double& acc,
                                              int lane) {
  double* dst = o + (int64_t)sig0 * nf;
  for (int g = 0; g < nv; ++g) {
    const double* t = tile + g * ts;
    for (int j = lane; j < nf; j += 64) dst[g * nf + j] = t[py_slot(j)];
  }
  if (lane < ne) {
    const int lo = max(sig0, lane * C) - sig0, hi = min(sig0 + nv, (lane + 1) * C) - sig0;
    for (int g = lo; g < hi; ++g) {
      const double* t = tile + g * ts;
#pragma unroll 8
      for (int j = 0; j < nf; ++j) {
        const double f = t[py_slot(j)];
        acc = acc + f * f;  // Math.pow(f, 2) summed in index order
      }
    }
  }
}

// Divides the block's ne rows of F doubles by their norms (lane m holds epoch m's).
__device__ __forceinline__ void pyramid_rescale(double* __restrict__ o, int ne, int F, double norm,
                                                int lane) {
  __threadfence_block();  // this wave's raw rows are complete before it reads them back
  for (int e = 0; e < ne; ++e) {  // eight loads in flight per batch (L2 round trips)
    double* r = o + (int64_t)e * F;
    const double nv = __shfl(norm, e, 64);
    for (int i0 = 0; i0 < F; i0 += 8 * 64) {
      double t[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const int i = i0 + 64 * u + lane;
        t[u] = i < F ? r[i] : 0.0;
      }
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const int i = i0 + 64 * u + lane;
        if (i < F) r[i] = t[u] / nv;
      }
    }
  }
}

// Window rows in LDS as features_from_epochs_kernel stages them (extract.hip): segment s of
// signal g at g * kPyWin + s * kPySeg doubles, 65 and 520 doubles, so a half-wave's reads of one
// sample index fall on 64 distinct banks.
constexpr int kPySeg = kSegLen + 1;
constexpr int kPyWin = 8 * kPySeg;
typedef double py_f64x2_a8 __attribute__((ext_vector_type(2), aligned(8)));
typedef float py_f32x4_a4 __attribute__((ext_vector_type(4), aligned(4)));

// ep: (epoch, channel) rows of row_stride elements, the window at [skip, skip + 512) of each.
// The lane takes its 72 samples to registers, after which the window LDS is free and serves as
// the tile; the next pass's rows are in flight meanwhile.
// E = float (eegfx_extract_features_f32, the scratch epochs of eegfx_process_recording_fe): 16
// loads of four floats per lane, typed 4-byte aligned (the window starts on any 4-byte boundary),
// widened as they are written into the same window layout; the pyramid and the tile are unchanged.
template <int DMIN, typename E = double>
__global__ __launch_bounds__(64) void pyramid_from_epochs_kernel(const E* __restrict__ ep,
                                                                 int64_t n, int C, int skip, int nf,
                                                                 int row_stride,
                                                                 double* __restrict__ out) {
  constexpr bool F32 = std::is_same<E, float>::value;
  static_assert(kPyTileMax >= 8 * kPyWin, "the tile covers the windows it replaces");
  __shared__ __attribute__((aligned(16))) double lds[kPyTileMax];
  const int lane = threadIdx.x;
  const int g = lane >> 3, s = lane & 7;
  const int F = C * nf, ts = pyramid_tile_stride(nf);
  const int64_t e0 = (int64_t)blockIdx.x * 8;
  const int ne = (n - e0) < 8 ? (int)(n - e0) : 8;
  const int nsig = ne * C;
  const E* rows = ep + e0 * C * (int64_t)row_stride + skip;
  double* o = out + e0 * F;
  // quad q = 64 (j % 4) + lane of slot j / 4: doubles 2q, 2q + 1 of its window.  Slots past the
  // last signal read the last signal's window (the loads stay unconditional, the result unused).
  constexpr int NV = F32 ? 16 : 32;
  typename std::conditional<F32, py_f32x4_a4, py_f64x2_a8>::type v[NV];
  auto load = [&](int sig0) {
#pragma unroll
    for (int j = 0; j < NV; ++j) {
      if constexpr (F32) {  // quad q = 64 (j % 2) + lane of slot j / 2: floats 4q .. 4q + 3
        const int sg = min(sig0 + (j >> 1), nsig - 1);
        const int q = ((j & 1) << 6) | lane;
        v[j] = __builtin_nontemporal_load(
            (const py_f32x4_a4*)(rows + (int64_t)sg * row_stride + 4 * q));
      } else {
        const int sg = min(sig0 + (j >> 2), nsig - 1);
        const int q = ((j & 3) << 6) | lane;
        v[j] = __builtin_nontemporal_load(
            (const py_f64x2_a8*)(rows + (int64_t)sg * row_stride + 2 * q));
      }
    }
  };
  load(0);
  double acc = 0.0;
  for (int sig0 = 0; sig0 < nsig; sig0 += 8) {
    wave_sync();  // the previous pass's tile reads precede these writes
#pragma unroll
    for (int j = 0; j < NV; ++j) {
      if constexpr (F32) {
        const int q = ((j & 1) << 6) | lane;
        double* d = lds + (j >> 1) * kPyWin + (q >> 4) * kPySeg + 4 * (q & 15);
        d[0] = (double)v[j].x;
        d[1] = (double)v[j].y;
        d[2] = (double)v[j].z;
        d[3] = (double)v[j].w;
      } else {
        const int q = ((j & 3) << 6) | lane;
        double* d = lds + (j >> 2) * kPyWin + (q >> 5) * kPySeg + 2 * (q & 31);
        d[0] = v[j].x;
        d[1] = v[j].y;
      }
    }
    wave_sync();
    if (sig0 + 8 < nsig) load(sig0 + 8);
    const double* sig = lds + g * kPyWin;
    double x[kIn];
#pragma unroll
    for (int k = 0; k < kIn; ++k)
      x[k] = k < kSegLen ? sig[s * kPySeg + k] : sig[((s + 1) & 7) * kPySeg + k - kSegLen];
    wave_sync();  // every lane holds its samples: the windows give way to the tile
    double* mine = lds + g * ts;
    auto emit = [&](int idx, double val) {
      if (idx < nf) mine[py_slot(idx)] = val;
    };
    double a1[40], a6, d6;
    dwt8_pyramid_level1<DMIN, true>(x, nullptr, lane & ~7, s, a1, emit);
    dwt8_pyramid_levels2to6<DMIN, true>(a1, nullptr, lane & ~7, s, a6, d6, emit);
    emit(s, a6);
    emit(8 + s, d6);
    wave_sync();
    pyramid_flush(lds, ts, sig0, min(8, nsig - sig0), C, nf, ne, o, acc, lane);
  }
  pyramid_rescale(o, ne, F, sqrt(acc), lane);
}

}  // namespace dev

template <typename E>
static hipError_t pyramid_from_epochs_impl(hipStream_t st, const E* ep, int64_t n, int C, int skip,
                                           int nfeat, double* out, int row_stride) {
  if (n == 0) return hipSuccess;
  if (nfeat <= 16 || nfeat > dev::kPyMaxFeat || C < 1 || C > kMaxChannels)
    return hipErrorInvalidValue;
  const dim3 grid((unsigned)((n + 7) / 8)), block(64);
#define EEGFX_PYE(D)                                                                             \
  hipLaunchKernelGGL((dev::pyramid_from_epochs_kernel<D, E>), grid, block, 0, st, ep, n, C,     \
                     skip, nfeat, row_stride, out)
  switch (dev::pyramid_dmin(nfeat)) {
    case 1: EEGFX_PYE(1); break;
    case 2: EEGFX_PYE(2); break;
    case 3: EEGFX_PYE(3); break;
    case 4: EEGFX_PYE(4); break;
    default: EEGFX_PYE(5); break;
  }
#undef EEGFX_PYE
  return hipGetLastError();
}
hipError_t launch_pyramid_from_epochs(hipStream_t st, const double* ep, int64_t n, int C, int skip,
                                      int nfeat, double* out, int row_stride) {
  return pyramid_from_epochs_impl(st, ep, n, C, skip, nfeat, out, row_stride);
}
hipError_t launch_pyramid_from_epochs(hipStream_t st, const float* ep, int64_t n, int C, int skip,
                                      int nfeat, double* out, int row_stride) {
  return pyramid_from_epochs_impl(st, ep, n, C, skip, nfeat, out, row_stride);
}

}  // namespace eegfx
