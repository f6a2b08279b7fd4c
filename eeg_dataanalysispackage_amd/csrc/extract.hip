// extract.hip -- extractFeatures on materialised epochs (gfx950) and its launcher.
//   features_from_epochs_kernel  a11..a13: epochs -> L2-normalised dwt-8 features
//                                (WaveletTransform.java:107-141, SignalProcessing.java:38-52)
// The kernel takes the epochs' element type as a template parameter E: double (the reference's
// double[n][C][750]) or float (the fp32 values it widens, the *_f32 entries).
// Compiled with -ffp-contract=off: every fp32/fp64 expression is evaluated as written, one
// correctly rounded IEEE operation at a time, matching the Java (strictfp-equivalent) order.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <type_traits>

#include "dwt8.h"
#include "guard.h"
#include "launch.h"

namespace eegfx {
namespace dev {

// a11..a13 from materialised epochs.  One wave per workgroup owns 8 epochs and walks their
// channels; lane = 8*epoch + segment (dwt8.h).  For each channel the wave reads the 8 windows
// (512 doubles each, contiguous in the epoch rows) with 16-byte loads, 1 KB of one window per
// load instruction, and writes them to LDS in a bank-skewed layout: segment s of window g at
// g*kFeWin + s*kFeSeg doubles.  kFeSeg = 65 doubles (130 dwords, 2 mod 64) and kFeWin = 520
// (1,040 dwords, 16 mod 64), so the ds_read_b64 of lane (g, s) for any sample index falls on
// banks 16g + 2s (+1) plus a common offset: the 32 lanes of a half-wave use 64 distinct banks.
// (Each lane reading its own 512 contiguous bytes straight from memory touches 64 cache lines
// per load instruction; that pattern moved ~1.9 TB/s.)  The filter bank then runs from LDS: FMA
// the collapsed four-point filter of dwt8_collapsed_core on the doubles as they are, EXACT the
// level-by-level cascade with value halos.  Features collect in LDS, are normalised per epoch
// with the reference's sequential sum of squares and written coalesced.  33 KB of windows per
// workgroup: 4 workgroups per CU.
constexpr int kFeSeg = kSegLen + 1;
constexpr int kFeWin = 8 * kFeSeg;
constexpr size_t kFeWinBytes = sizeof(double) * 8 * kFeWin;
typedef double f64x2_a8 __attribute__((ext_vector_type(2), aligned(8)));

// Under fma numerics each lane also keeps the largest |x| of its samples, and the rows are
// checked against the conditioning guard (guard.h: sum over the channels of the measured X^2); a
// row that fails is recomputed under EXACT by the wave from the epochs in memory, the window LDS
// as scratch (rare).
// ROWS_OUT (wide rows, launcher): the 8 feature rows (8 F doubles: 32 KB at C = 32) do not stay in
// LDS, where they halved the resident workgroups.  After each channel the 8 x nfeat values pass
// through a 1 KB LDS tile, leave as whole 128-byte runs into `out`, and lanes 0-7 add their
// squares to the epoch's sum in index order (the reference's sequential sum,
// SignalProcessing.java:38-52); at the end the wave rescales its rows in place (L2-resident).
//
// Float32 epochs (E = float, eegfx_extract_features_f32 and the scratch epochs of
// eegfx_process_recording_fe): a window is 2 KB, read as 16 loads of four floats per lane (quad
// q = 64 (j % 2) + lane of window j / 2), again 1 KB of one window per load instruction.  The
// window starts at ep + 4 (row * row_stride + skip) bytes, on any 4-byte boundary, so the quads
// are typed 4-byte aligned, as the double pairs are typed 8-byte aligned (an odd skip): the
// 16-byte global load takes any dword address.  The samples are widened as they are written into
// the same LDS layout, and everything after that is the double kernel's: the rows are its rows.
typedef float f32x4_a4 __attribute__((ext_vector_type(4), aligned(4)));
template <bool FAST, bool ROWS_OUT, typename E = double>
__global__ __launch_bounds__(64) void features_from_epochs_kernel(const E* __restrict__ ep,
                                                                  int64_t n, int C, int skip,
                                                                  int nfeat, int row_stride,
                                                                  double* __restrict__ out,
                                                                  Guard guard) {
  constexpr bool F32 = std::is_same<E, float>::value;
  __shared__ __attribute__((aligned(16))) double win[8 * kFeWin];
  extern __shared__ __attribute__((aligned(16))) double fsmem[];
  const int lane = threadIdx.x;
  const int el = lane >> 3, s = lane & 7;
  const int F = C * nfeat;
  double* feat = fsmem;                             // [8][F], or the [8][16] tile (ROWS_OUT)
  double* norm = feat + (ROWS_OUT ? 8 * 16 : 8 * F);  // [8]
  const int64_t e0 = (int64_t)blockIdx.x * 8;
  const int64_t ne = (n - e0) < 8 ? (n - e0) : 8;
  double* o = out + e0 * F;
  // quad q = 64 (j % 4) + lane of window j / 4: doubles 2q, 2q + 1 of segment q / 32.  Epochs
  // past n read the last epoch's window (the loads stay unconditional; the result is dropped).
  // Channel c + 1's windows are in flight while channel c runs the filter bank.
  constexpr int NV = F32 ? 16 : 32;
  typename std::conditional<F32, f32x4_a4, f64x2_a8>::type v[NV];
  auto load = [&](int c) {
#pragma unroll
    for (int j = 0; j < NV; ++j) {
      if constexpr (F32) {
        const int g = j >> 1;
        const int64_t e = e0 + (g < ne ? g : ne - 1);
        const int q = ((j & 1) << 6) | lane;
        v[j] = __builtin_nontemporal_load(
            (const f32x4_a4*)(ep + (e * C + c) * row_stride + skip + 4 * q));
      } else {
        const int g = j >> 2;
        const int64_t e = e0 + (g < ne ? g : ne - 1);
        const int q = ((j & 3) << 6) | lane;
        v[j] = __builtin_nontemporal_load(
            (const f64x2_a8*)(ep + (e * C + c) * row_stride + skip + 2 * q));
      }
    }
  };
  load(0);
  double sx = 0.0;   // fma: sum over the channels of this lane's signal's X^2
  double acc = 0.0;  // ROWS_OUT, lanes < ne: epoch `lane`'s sum of squares so far
  for (int c = 0; c < C; ++c) {
    wave_sync();  // the previous channel's LDS reads precede these writes
#pragma unroll
    for (int j = 0; j < NV; ++j) {
      if constexpr (F32) {  // floats 4q .. 4q + 3 of segment q / 16, widened
        const int q = ((j & 1) << 6) | lane;
        double* d = win + (j >> 1) * kFeWin + (q >> 4) * kFeSeg + 4 * (q & 15);
        d[0] = (double)v[j].x;
        d[1] = (double)v[j].y;
        d[2] = (double)v[j].z;
        d[3] = (double)v[j].w;
      } else {
        const int q = ((j & 3) << 6) | lane;
        double* d = win + (j >> 2) * kFeWin + (q >> 5) * kFeSeg + 2 * (q & 31);
        d[0] = v[j].x;
        d[1] = v[j].y;
      }
    }
    wave_sync();
    if (c + 1 < C) load(c + 1);
    const double* own = win + el * kFeWin + s * kFeSeg;
    double a6, d6;
    if constexpr (FAST) {
      double xm = 0.0;
      dwt8_collapsed_core([&](int k) { return own[k]; },
                          [&](double v0, double v1, double& x0, double& x1) {
                            xm = fmax(xm, fmax(fabs(v0), fabs(v1)));
                            x0 = v0;
                            x1 = v1;
                          },
                          lane & ~7, s, a6, d6);
      xm = group8_max(xm);
      const double x2 = xm * xm;  // doubles below 2^-537 square to 0: keep X^2 != 0 (guard.h)
      sx += x2 == 0.0 && xm != 0.0 ? 0x1p-1022 : x2;
    } else {
      const double* sig = win + el * kFeWin;
      double x[kIn];
#pragma unroll
      for (int k = 0; k < kIn; ++k) x[k] = k < kSegLen ? own[k] : sig[((s + 1) & 7) * kFeSeg + k - kSegLen];
      dwt8_cascade<false, true>(x, nullptr, lane & ~7, s, a6, d6);
    }
    if constexpr (ROWS_OUT) {
      feat[el * 16 + s] = a6;  // the tile's previous reads finished before the window writes
      feat[el * 16 + 8 + s] = d6;
      wave_sync();
      for (int idx = lane; idx < ne * nfeat; idx += 64) {
        const int e = idx / nfeat, j = idx - e * nfeat;
        o[(int64_t)e * F + c * nfeat + j] = feat[e * 16 + j];
      }
      if (lane < ne)
        for (int j = 0; j < nfeat; ++j) {
          const double f = feat[lane * 16 + j];
          acc = acc + f * f;  // Math.pow(f, 2) summed in index order
        }
    } else if (el < ne) {
      if (s < nfeat) feat[el * F + c * nfeat + s] = a6;
      if (8 + s < nfeat) feat[el * F + c * nfeat + 8 + s] = d6;
    }
  }
  wave_sync();
  const double sx_row = __shfl(sx, (lane & 7) * 8, 64);  // epoch `lane`'s X^2 sum (lanes < 8)
  bool fails = false;
  if (lane < ne) {
    if constexpr (!ROWS_OUT) {
      for (int i = 0; i < F; ++i) {
        const double f = feat[lane * F + i];
        acc = acc + f * f;  // Math.pow(f, 2) summed in index order
      }
    }
    norm[lane] = sqrt(acc);
    // caller-supplied doubles: also the rows whose norm the squares cannot carry (guard.h)
    fails = FAST && guard.total && (guard_fails(acc, kGuardK2Collapsed, sx_row) ||
                                    guard_acc_out_of_range(acc, sx_row));
  }
  if constexpr (FAST) {  // the guard's rare path: flagged rows recomputed under EXACT in place
    uint64_t flagged = __ballot(fails);
    if (flagged) {
      wave_sync();
      if (lane == 0) {  // the only test is the measured one: its failures count as both
        guard_count_rechecked(guard, __popcll(flagged));
        guard_count_recomputed(guard, (unsigned long long)__popcll(flagged));
      }
      do {
        const int e = __ffsll((unsigned long long)flagged) - 1;
        const E* row = ep + (e0 + e) * C * (int64_t)row_stride + skip;
        static_assert(768 + kMaxChannels * 16 <= 8 * kFeWin, "the recomputed row fits the windows");
        double* dst = ROWS_OUT ? win + 768 : feat + e * F;  // past the 768-double scratch
        dwt8_exact_row_wave(
            [&](int c, int k) { return (double)row[(int64_t)c * row_stride + k]; }, C, nfeat, win,
            dst, lane);
        if constexpr (ROWS_OUT) {
          wave_sync();
          for (int i = lane; i < F; i += 64) o[(int64_t)e * F + i] = dst[i];
          wave_sync();
        }
        if (lane == 0) norm[e] = 1.0;  // the row is normalised
        flagged &= flagged - 1;
      } while (flagged);
    }
  }
  wave_sync();
  if constexpr (ROWS_OUT) {
    __threadfence_block();  // this wave's raw rows are complete before it reads them back
    for (int e = 0; e < ne; ++e) {  // eight loads in flight per batch (L2 round trips)
      double* r = o + (int64_t)e * F;
      const double nv = norm[e];
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
  } else {
    for (int idx = lane; idx < ne * F; idx += 64) o[idx] = feat[idx] / norm[idx / F];
  }
}

}  // namespace dev

template <typename E>
static hipError_t features_from_epochs_impl(hipStream_t st, const E* ep, int64_t n, int C, int skip,
                                            int nfeat, bool fast, double* out, int row_stride,
                                            const Guard& guard) {
  if (n == 0) return hipSuccess;
  // The rows stay in LDS while the workgroup (33 KB of windows + 8 rows) still fits three times
  // per CU (C <= 20 at 16 features); wider rows go through `out`, which keeps four per CU.
  // Measured (profiles/r04q/, fma / EXACT): C = 24 rows in LDS 2.86 / 3.52 ms, through `out`
  // 2.61 / 2.77 ms; C = 32 2.88 / 3.53 vs 2.82 / 2.96 ms; C = 16 2.40 / 2.54 vs 2.57 / 2.72 ms.
  const size_t lds_rows = dev::kFeWinBytes + sizeof(double) * (8 * (size_t)C * nfeat + 8);
  const bool rows_out = 3 * lds_rows > 160 * 1024;
  const size_t smem = sizeof(double) * (rows_out ? 8 * 16 + 8 : 8 * (size_t)C * nfeat + 8);
  dim3 grid((unsigned)((n + 7) / 8)), block(64);
  const Guard none{nullptr, nullptr, nullptr};
#define EEGFX_FFE(FA, RO)                                                                         \
  hipLaunchKernelGGL((dev::features_from_epochs_kernel<FA, RO, E>), grid, block, smem, st, ep, n, \
                     C, skip, nfeat, row_stride, out, FA ? guard : none)
  if (fast) { if (rows_out) EEGFX_FFE(true, true); else EEGFX_FFE(true, false); }
  else { if (rows_out) EEGFX_FFE(false, true); else EEGFX_FFE(false, false); }
#undef EEGFX_FFE
  return hipGetLastError();
}
hipError_t launch_features_from_epochs(hipStream_t st, const double* ep, int64_t n, int C, int skip,
                                       int nfeat, bool fast, double* out, int row_stride,
                                       const Guard& guard) {
  return features_from_epochs_impl(st, ep, n, C, skip, nfeat, fast, out, row_stride, guard);
}
hipError_t launch_features_from_epochs(hipStream_t st, const float* ep, int64_t n, int C, int skip,
                                       int nfeat, bool fast, double* out, int row_stride,
                                       const Guard& guard) {
  return features_from_epochs_impl(st, ep, n, C, skip, nfeat, fast, out, row_stride, guard);
}

}  // namespace eegfx
