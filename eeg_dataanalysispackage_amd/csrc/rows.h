// rows.h -- normalisation and store of the feature rows of an 8-epoch sub-tile, shared by the
// fused window kernel (fused.hip: its EXACT rows; its fma rows leave from registers) and the
// one-pass getData + features kernels (cut.hip: both numerics), and the second stage of the
// conditioning guard for the one-pass 3-channel kernel (recheck_c3; the guard's shared pieces are
// in guard.h).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "dwt8.h"
#include "guard.h"
#include "launch.h"

namespace eegfx {
namespace dev {

// SignalProcessing.normalize (SignalProcessing.java:38-52) for the <= 8 feature rows of a
// sub-tile, executed by one wave.  `fb` holds the rows in LDS; `norm` is an 8-double LDS scratch
// owned by the calling wave.
//   EXACT: lane e < ne folds Math.pow(f, 2) over row e in index order (the 8 dependent chains run
//          side by side), then the 64 lanes divide and store (16-byte stores).
//   FMA:   (1e-9 contract) the 8 lanes of an epoch each square-sum F/8 features, a 3-step
//          butterfly completes the row sum, and the row is scaled by 1/sqrt (rsqrt_nr: within an
//          ulp or two of x / s; an all-zero row still gives NaN = 0 * inf); the scaled rows go
//          back to LDS and leave as contiguous non-temporal 1 KB wave stores (storing each lane's
//          16-byte pieces 48 B apart cost 1,114 instead of 384 written bytes per row).  A row
//          whose sum of squares fails the conditioning guard (guard.h; gx = the C per-signal X^2)
//          goes to the second stage: recheck(flagged, acc), a wave-collective call on the mask of
//          flagged rows (bit 8e = row e) and this lane's row sum of squares, returns the mask of
//          rows that fail the test with their measured X too (per_row_recheck adapts a per-row
//          X^2 functor).  Only those rows are recomputed under EXACT by redo(e, row) into their
//          row slots before the store (rare: never on the bench workload), and counted in the
//          guard's running total.  Every recheck runs before the first redo, whose LDS scratch
//          may overwrite the staged windows that a recheck reads.
struct NoRedo {
  __device__ void operator()(int, double*) const {}
};
struct NoRecheck {  // no second stage: every flagged row is recomputed
  __device__ uint64_t operator()(uint64_t flagged, double) const { return flagged; }
};
// The second stage one row at a time: x2(e), a wave-collective call, returns row e's measured
// sum of X_c^2, bare (recheck_c3).
template <typename X2>
struct PerRowRecheck {
  X2 x2;
  __device__ __forceinline__ uint64_t operator()(uint64_t flagged, double acc) const {
    uint64_t left = 0;
    for (uint64_t f = flagged; f; f &= f - 1) {
      const int e1 = __ffsll((unsigned long long)f) - 1;
      const double acc_e = lane_value(acc, e1);  // e1 is wave-uniform
      // the verdict is wave-uniform: a scalar branch keeps `left` in SGPRs
      if (__builtin_amdgcn_readfirstlane(guard_fails_measured(acc_e, x2(e1 >> 3)) ? 1 : 0))
        left |= 1ull << e1;
    }
    return left;
  }
};
template <typename X2>
__device__ __forceinline__ PerRowRecheck<X2> per_row_recheck(X2 x2) {
  return PerRowRecheck<X2>{x2};
}
template <int F, bool FAST, int C = F / 16, typename Redo = NoRedo, typename Recheck = NoRecheck>
__device__ __forceinline__ void normalise_store(double* fb, double* norm, double* o, int ne,
                                                int lane, const double* gx = nullptr,
                                                Guard g = Guard{nullptr, nullptr, nullptr},
                                                Redo redo = Redo{}, Recheck recheck = Recheck{}) {
  typedef double f64x2 __attribute__((ext_vector_type(2)));
  if constexpr (FAST) {
    static_assert(F % 16 == 0, "8 lanes per row, pairs of features");
    constexpr int P = F / 8;
    const int e = lane >> 3, p = lane & 7;
    double v[P];
    double acc = 0.0;
#pragma unroll
    for (int i = 0; i < P; ++i) {
      v[i] = e < ne ? fb[e * F + p * P + i] : 0.0;
      acc = __builtin_fma(v[i], v[i], acc);
    }
    acc += __shfl_xor(acc, 1, 64);
    acc += __shfl_xor(acc, 2, 64);
    acc += __shfl_xor(acc, 4, 64);
    bool fails = false;
    if (EEGFX_GUARD && g.total && p == 0 && e < ne) {
      double sx = 0.0;
#pragma unroll
      for (int c = 0; c < C; ++c) sx += gx[e * C + c];
      fails = guard_fails(acc, kGuardK2Collapsed, sx);
    }
    const double inv = rsqrt_nr(acc);
    if (e < ne) {
#pragma unroll
      for (int i = 0; i < P; i += 2)
        *(double2*)(fb + e * F + p * P + i) = make_double2(v[i] * inv, v[i + 1] * inv);
    }
    wave_sync();
    uint64_t flagged = __ballot(fails);  // bit 8e: row e failed the a-priori test
    if (flagged) {                        // uniform, rare
      uint64_t left = recheck(flagged, acc);  // rows that fail the measured test too
      if (lane == 0) {
        guard_count_rechecked(g, __popcll(flagged));
        if (left) guard_count_recomputed(g, (unsigned long long)__popcll(left));
      }
      for (; left; left &= left - 1) {
        const int e1 = __ffsll((unsigned long long)left) - 1;
        redo(e1 >> 3, fb + (e1 >> 3) * F);
      }
    }
    for (int i = 2 * lane; i < ne * F; i += 128)
      __builtin_nontemporal_store(*(const f64x2*)(fb + i), (f64x2*)(o + i));
    wave_sync();
    (void)norm;
    return;
  }
  if (lane < ne) {
    double acc = 0.0;
#pragma unroll 16
    for (int i = 0; i < F; ++i) {
      const double f = fb[lane * F + i];
      acc = acc + f * f;
    }
    norm[lane] = sqrt(acc);
  }
  wave_sync();
  for (int i = 2 * lane; i < ne * F; i += 128) {
    const double v0 = fb[i] / norm[i / F];
    const double v1 = fb[i + 1] / norm[(i + 1) / F];
    *(double2*)(o + i) = make_double2(v0, v1);
  }
  wave_sync();
}

// The conditioning guard's second stage (guard.h) for one row of the one-pass 3-channel kernel,
// by one wave: lane l reads frames 64 (l >> 3) + 8 (l & 7) .. + 7 of the window at byte W of the
// recording, all three channels (zero past its end, the reference's padding), keeps each
// channel's min and max raw sample, decodes those six extremes exactly as the kernel decodes
// every sample (decode_f32: monotone in raw, so they bound the lane's |x|), and takes one wave
// maximum: X = max_c max |x_c|.  It returns 3 X^2 >= sum_c X_c^2, bare (guard_fails_measured),
// a rigorous bound at most 3x looser than the per-channel sum (which would cost three wave
// reductions: this pass is VALU-bound at the power cap, ~50 instead of ~100 VALU per row).
// One memory round trip for all 24 samples of a lane.
template <int FB>
__device__ __forceinline__ double recheck_c3(const uint8_t* __restrict__ raw, int64_t n_frames,
                                             const ChanSel& sel, int64_t W,
                                             const float* __restrict__ b, int lane) {
  const int f0 = 8 * lane;  // = 64 (lane >> 3) + 8 (lane & 7)
  int v[3][8];
  const int64_t B = W & ~(int64_t)1;
  const int64_t g0 = B / FB + f0;
  if (B / FB + kWin <= n_frames) {  // wave-uniform: the whole window inside, no per-load test
#pragma unroll
    for (int i = 0; i < 8; ++i)
#pragma unroll
      for (int c = 0; c < 3; ++c)
        v[c][i] = *(const int16_t*)(raw + B + (int64_t)(f0 + i) * FB + 2 * sel.col[c]);
  } else {
#pragma unroll
    for (int i = 0; i < 8; ++i)
#pragma unroll
      for (int c = 0; c < 3; ++c)
        v[c][i] = g0 + i < n_frames
                      ? *(const int16_t*)(raw + B + (int64_t)(f0 + i) * FB + 2 * sel.col[c])
                      : 0;
  }
  float xm = 0.0f;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    int mn = v[c][0], mx = v[c][0];
#pragma unroll
    for (int i = 1; i < 8; ++i) {
      mn = min(mn, v[c][i]);
      mx = max(mx, v[c][i]);
    }
    xm = fmaxf(xm, decode_f32(mn, mx, sel.res[c], b[c]));
  }
  const double X = (double)__uint_as_float(group_max_u32<64>(__float_as_uint(xm)));
  return 3.0 * (X * X);  // exact: X^2 has 48 significant bits
}

}  // namespace dev
}  // namespace eegfx
