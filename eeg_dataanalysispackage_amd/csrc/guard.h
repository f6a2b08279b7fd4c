// guard.h -- the conditioning guard of the fma numerics.
//
// Both numerics filter the SAME decoded doubles x (the fp32 decode and baseline are order-exact in
// both), so an fma row differs from the EXACT (reference-order) row only by fp64 rounding.
// tools/fma_bound.py propagates rigorous bounds through both filter banks, operation by operation
// in the kernels' order: |f_fma - f_exact| <= E * X per coefficient for a signal whose samples
// satisfy |x_i| <= X.  The normalised rows then differ by at most 2 |f_fma - f_exact| / |f_fma|
// (SignalProcessing.java:38-52 divides by the norm), so a row is certified within 0.5e-9 (half of
// the north_star's 1e-9; the normalisations' own rounding, ~1e-15, takes the rest) when
//     |f_fma|^2 >= K2 * sum_c X_c^2,     K2 = (2 / 0.5e-9)^2 * 8 (E_a6^2 + E_d6^2) * 1.25.
// A row that fails the test -- its features are close to rounding noise, or X_c is loose -- goes
// to a second stage: the wave that normalises it measures the row's own max |x| per channel
// (guard_measured_x2_wave) and tests again with that X -- in the 3-channel kernels the cheaper
// 3 max_c X_c^2 >= sum_c X_c^2 (rows.h recheck_c3: one wave reduction instead of three; the pass
// is VALU-bound at the power cap).  Only rows that still fail (e.g. a window
// in the filters' null space, an alternating +-A signal) are recomputed with the EXACT filter bank,
// value-identical to the reference, by the same wave inside the same kernel
// (dwt8_exact_row_wave): the 3-channel window kernel, the 32-channel kernel, the one-pass kernels,
// the batch extract and the per-epoch kernel.  Only the generic any-layout window kernel
// (window_wide_kernel) appends its failing rows to `list` for a follow-up launch
// (guard.hip exact_rows_kernel); `count` / `list` are unused elsewhere.
//
// X_c: for int16 recordings a bound known without touching the window,
//   |x| = |fl(fl(raw * r) - b)| <= (32768 |r| + |b|)(1 + 2^-23) for every int16 raw (zero padding
//   included), taken with a 2^-20 margin -- loose when the samples stay far below full scale (a
//   flat stretch decodes to ~1e-3 against X ~ 6e3), hence the second stage; for float32 recordings
//   and caller-supplied double epochs the measured max |x| of the window from the start (no
//   a-priori bound exists).
//
// The pieces of the verdict, one copy each, are here: the decode of a sample and of a pair of
// extremes (decode_f32), the reduction ladder over a lane group (ladder_reduce: group_max_u32,
// group_min_pk_i16), the two tests (guard_fails; guard_fails_measured, the only place the
// measured sum's 2^-20 margin is applied: every helper that measures returns the bare sum), the
// measured sum of a row by one wave (guard_measured_x2_wave), the whole verdict on a row by one
// wave (guard_row_fails_wave) and the samples of a recording for the rare paths (Recording).
// The kernels keep only how their lanes map to rows, channels and frames.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <type_traits>

namespace eegfx {

// tools/fma_bound.py (tests/test_taps.py checks these against it): the collapsed four-point filter
// of the window, batch and 32-channel kernels, and the level-by-level fma cascade of
// features_small_kernel.
constexpr double kGuardK2Collapsed = 7.02e-05;
constexpr double kGuardK2Cascade = 1.62e-04;

// Device state of a guarded launch: `count` flagged rows so far and their epoch indices in `list`
// (window_wide_kernel only: zeroed before the launch that fills it, capacity the launch's epochs),
// the running total of rows recomputed under EXACT since the context was created, and of rows that
// failed the a-priori test and went to the second stage (`rechecked`; may be null)
// (eegfx_ctx_guard_stats / eegfx_ctx_guard_detail).  total == nullptr disables the guard (EXACT).
// `total` and `rechecked` are running counters spread over kGuardSlots slots, one per 128-byte
// line, a workgroup adding into slot blockIdx % kGuardSlots: one shared word took every
// workgroup's atomic in turn, which at a 10 % flag rate cost as much as the kernel itself
// (profiles/r05h: 0.733 -> 1.398 ms).  The host sums the slots.
constexpr int kGuardSlots = 256;
constexpr int kGuardSlotWords = 16;  // 128 B
constexpr size_t kGuardSlotBytes = sizeof(unsigned long long) * kGuardSlots * kGuardSlotWords;
struct Guard {
  int* count;
  int64_t* list;
  unsigned long long* total;
  unsigned long long* rechecked = nullptr;
  // the 3-channel window kernel's guard strategy (fused.hip, EEGFX_TRACK_X): adapt[0] = 1 when
  // the previous launch sent more than 1/16 of its rows to the second stage (every lane then
  // tracks max |x| while decoding, so no row needs the scan), set by baseline_kernel from
  // adapt[1] (the rechecked total it last saw) and adapt[2] (that launch's rows); may be null
  unsigned long long* adapt = nullptr;
  // host-mapped word that baseline_kernel sets to the strategy it chose from adapt (the host picks
  // the window kernel's variant for its next launch from it); may be null
  unsigned int* track_out = nullptr;
};

// The guard's second stage in the fma 3-channel window kernel (fused.hip), two strategies:
//   scan   the a-priori int16 bound for every row, and a scan of the staged windows for the rows
//          it flags (channel_x2_rows): free while few rows are flagged;
//   track  every lane keeps the largest |x| of the samples it decodes (one v_max3_f32 per pair,
//          +3 % per step), so every row has its measured X_c and no flagged row needs the scan
//          (+0.8 % at a 32 % flag rate, where the scan costs +8 %).
// 1 (product) = adaptive: the host launches the tracking variant when the last launch's
// baseline_kernel found that the launch before sent more than 1/16 of its rows to the second
// stage; 0 = always scan, 2 = always track (A/B builds).
#ifndef EEGFX_TRACK_X
#define EEGFX_TRACK_X 1
#endif

namespace dev {

// X_c^2 for an int16 signal with resolution r and baseline b (see the header comment).
__device__ __forceinline__ double guard_x2_int16(float r, float b) {
  const double X = (32768.0 * fabs((double)r) + fabs((double)b)) * (1.0 + 0x1p-20);
  return X * X;
}

// Appends epoch e to the guard list (rare: rows whose features are rounding-level).
__device__ __forceinline__ void guard_flag(const Guard& g, int64_t e) {
  const int i = atomicAdd(g.count, 1);
  g.list[i] = e;
}

// sum of squares `acc` against the row's threshold; NaN fails (and is recomputed as EXACT).
__device__ __forceinline__ bool guard_fails(double acc, double k2, double sum_x2) {
  return !(acc >= k2 * sum_x2);
}

// The range of a row's sum of squares in which the conditioning test says anything about the
// normalised row.  The test bounds the features' differences; the norm is then taken from
// squares, and both numerics round those: outside this range the two norms can differ by more
// than the features do, so the row is recomputed under EXACT whatever the test says.
//   upper end: a certified row's fma and EXACT sums of squares differ by a relative 3e-9 at
//     most (the features by 0.5e-9 of the norm, <= 512 roundings of 2^-53), so while the fma
//     sum is <= 2^1023 = DBL_MAX / 2 (1 - 2^-53) the EXACT sum is finite as well.  Above it
//     (Inf included: Inf >= k2 * Inf certifies) one norm can be Inf, which turns every finite
//     feature into 0.0, and the other finite.
//   lower end: a square below DBL_MIN = 2^-1022 is rounded to a multiple of 2^-1074, an absolute
//     error of 2^-1075 that the relative bounds do not cover; over <= 512 squares and both
//     numerics that is 2^-1065.  With acc >= 2^-969 = DBL_MIN * 2^53 it is a relative 2^-96,
//     nothing beside the sum's own 2^-53 roundings.  Below, the EXACT row itself drifts with
//     the scale of its input (2^-530 * 50 N(0, 1): 5e-10 from the unscaled row), and only EXACT
//     reproduces that.
// acc = 0 with every X_c = 0 is the all-zero window: +-0 features and the reference's 0 / 0 = NaN
// row under both numerics, certified; the caller keeps sum_x2 != 0 when a sample is nonzero.
// Only caller-supplied doubles reach these ends (features_from_epochs_kernel).  The kernels
// that decode a recording filter fp32 values: |x| <= 2 FLT_MAX = 2^129 and a gain of at most
// (sum |h|)^6 = 2^6 over the six levels bound acc by 512 (2^6 * 2^129)^2 = 2^279, and a
// certified row has acc >= k2 * X^2 >= 7e-5 * 2^-298 (X >= 2^-149, the smallest fp32) or
// acc = sum_x2 = 0, so there the range test could never fail and is not made.
constexpr double kGuardAccMin = 0x1p-969;
constexpr double kGuardAccMax = 0x1p1023;
__device__ __forceinline__ bool guard_acc_out_of_range(double acc, double sum_x2) {
  return !((acc >= kGuardAccMin && acc <= kGuardAccMax) || (acc == 0.0 && sum_x2 == 0.0));
}

__device__ __forceinline__ void guard_slot_add(unsigned long long* slots, unsigned long long v) {
  atomicAdd(slots + (blockIdx.x & (kGuardSlots - 1)) * kGuardSlotWords, v);
}
// The window kernel's guard strategy for the launch that follows (Guard::adapt, EEGFX_TRACK_X),
// by the first wave of a baseline pass's block 0 (lane = tid < 64): track when the previous
// launch sent more than 1/16 of its rows to the second stage.  adapt[1] is the rechecked total
// seen last, as a signed offset (a host counter reset subtracts the total it clears, so the
// difference still counts the launches since); the choice also goes to the host-mapped word the
// host reads when it picks the window kernel's variant.
__device__ __forceinline__ void guard_adapt_update(const unsigned long long* rechecked,
                                                   unsigned long long* adapt,
                                                   unsigned int* track_out, int64_t n, int lane) {
  unsigned long long t = 0;
  for (int i = lane; i < kGuardSlots; i += 64) t += rechecked[i * kGuardSlotWords];
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) t += __shfl_xor(t, off, 64);
  if (lane == 0) {
    const long long delta = (long long)t - (long long)adapt[1];
    const unsigned long long nprev = adapt[2];
    unsigned long long mode = adapt[0];
    if (delta >= 0) mode = nprev > 0 && (unsigned long long)delta * 16 > nprev ? 1ull : 0ull;
    adapt[0] = mode;
    adapt[1] = t;
    adapt[2] = (unsigned long long)n;
    if (track_out)
      __hip_atomic_store(track_out, (unsigned int)mode, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  }
}

// rows recomputed with the EXACT cascade
__device__ __forceinline__ void guard_count_recomputed(const Guard& g, unsigned long long rows) {
  guard_slot_add(g.total, rows);
}
// rows that went to the second stage
__device__ __forceinline__ void guard_count_rechecked(const Guard& g, int rows) {
  if (g.rechecked && rows) guard_slot_add(g.rechecked, (unsigned long long)rows);
}

// lane j's v (j wave-uniform), as a wave-uniform value
__device__ __forceinline__ double lane_value(double v, int j) {
  const uint64_t b = __builtin_bit_cast(uint64_t, v);
  const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)b, j);
  const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(b >> 32), j);
  return __builtin_bit_cast(double, (uint64_t)hi << 32 | lo);
}

// The kernels' decode of a raw sample v (int16 or float32, as float) with resolution r and
// baseline b: x = fl(fl(v * r) - b), two correctly rounded fp32 operations
// (DataProviderUtils.java:49-59, Baseline.java:39-41; the file is compiled with
// -ffp-contract=off).  Every sample the guard measures or recomputes goes through here.
__device__ __forceinline__ float decode_f32(float v, float r, float b) {
  float y = v * r;
  y = y - b;
  return y;
}
// The decode is monotone in v, so the extremes (lo, hi) of a set of raw samples bound its |x|:
// max(|x(lo)|, |x(hi)|), the pair decoded with packed fp32 math (each half rounded as above).
__device__ __forceinline__ float decode_f32(int lo, int hi, float r, float b) {
  typedef float f32x2 __attribute__((ext_vector_type(2)));
  f32x2 x = f32x2{(float)lo, (float)hi} * f32x2{r, r};
  x = x + f32x2{-b, -b};
  return fmaxf(fabsf(x.x), fabsf(x.y));
}

// The reduction ladder over an aligned group of 2^lg lanes (lg = 3..6; every lane of the group
// gets the result), the one copy of its steps: step i combines lanes 2^i apart -- quad_perm
// xor 1 and xor 2, row_half_mirror and row_mirror as DPP moves (no LDS), then the two
// cross-row shuffles.  lg may be a runtime value (channel_x2_rows); a constant folds the tests.
template <int STEP>
__device__ __forceinline__ uint32_t ladder_peer(uint32_t v) {
  static_assert(STEP >= 0 && STEP < 6, "a wave has 64 lanes");
  constexpr int kCtrl[4] = {0xB1, 0x4E, 0x141, 0x140};
  if constexpr (STEP < 4)
    return (uint32_t)__builtin_amdgcn_mov_dpp((int)v, kCtrl[STEP], 0xF, 0xF, true);
  else
    return (uint32_t)__shfl_xor((int)v, 1 << STEP, 64);
}
template <typename Op>
__device__ __forceinline__ uint32_t ladder_reduce(uint32_t v, int lg, Op op) {
  v = op(v, ladder_peer<0>(v));
  v = op(v, ladder_peer<1>(v));
  v = op(v, ladder_peer<2>(v));
  if (lg >= 4) v = op(v, ladder_peer<3>(v));
  if (lg >= 5) v = op(v, ladder_peer<4>(v));
  if (lg >= 6) v = op(v, ladder_peer<5>(v));
  return v;
}
constexpr int ladder_log2(int lanes) {
  return lanes == 8 ? 3 : lanes == 16 ? 4 : lanes == 32 ? 5 : 6;
}
// Maximum of unsigned words over a group of LANES lanes.  A non-negative, non-NaN float orders
// like its bit pattern, so this is also the maximum of such floats (max |x|).
template <int LANES>
__device__ __forceinline__ uint32_t group_max_u32(uint32_t v) {
  static_assert(LANES == 8 || LANES == 16 || LANES == 32 || LANES == 64, "an aligned lane group");
  return ladder_reduce(v, ladder_log2(LANES), [](uint32_t a, uint32_t b) { return max(a, b); });
}
// Minimum of packed int16 pairs over a group of LANES lanes.
template <int LANES>
__device__ __forceinline__ uint32_t group_min_pk_i16(uint32_t v) {
  static_assert(LANES == 8 || LANES == 16 || LANES == 32 || LANES == 64, "an aligned lane group");
  typedef short s2 __attribute__((ext_vector_type(2)));
  return ladder_reduce(v, ladder_log2(LANES), [](uint32_t a, uint32_t b) {
    return __builtin_bit_cast(uint32_t, __builtin_elementwise_min(__builtin_bit_cast(s2, a),
                                                                  __builtin_bit_cast(s2, b)));
  });
}

// Packs a lane's (min, max) of int16 samples as (min, ~max) so that one packed minimum reduces
// both (min(~a, ~b) = ~max(a, b), no overflow); unpack with guard_unpack_min / _max.
__device__ __forceinline__ uint32_t guard_pack_minmax(int mn, int mx) {
  return ((uint32_t)mn & 0xFFFFu) | ((uint32_t)~mx << 16);
}
__device__ __forceinline__ int guard_unpack_min(uint32_t p) { return (int)(int16_t)(p & 0xFFFFu); }
__device__ __forceinline__ int guard_unpack_max(uint32_t p) { return ~(int)(int16_t)(p >> 16); }

// The second stage's test: `sum_x2` is a measured sum of X_c^2 (or a bound of it: 3 max_c X_c^2,
// rows.h recheck_c3) as its helper returns it, bare; the 2^-20 margin that covers the rounding
// of the decoded extremes' squares and of their sum is applied here and nowhere else.
__device__ __forceinline__ bool guard_fails_measured(double acc, double sum_x2) {
  return guard_fails(acc, kGuardK2Collapsed, sum_x2 * (1.0 + 0x1p-20));
}

// The second stage, by one wave (every lane calls it; the result is wave-uniform): sum over the
// row's C signals of X_c^2, X_c = max_k |x_c[k]| over the 512 window samples, measured.
// sample(c, k) returns the int16 raw value of sample k of channel c (0 for the zero padding past
// the recording's end); X_c is decode_f32 of the channel's extremes with res(c) and base(c).
// 16 lanes (one DPP row) per channel, four channels per pass; each lane's 32 reads are
// independent.  Returns the bare sum (guard_fails_measured).
template <typename Sample, typename Res, typename Base>
__device__ __forceinline__ double guard_measured_x2_wave(Sample sample, Res res, Base base, int C,
                                                         int lane) {
  const int grp = lane >> 4, l = lane & 15;
  double sx = 0.0;
#pragma unroll 1
  for (int c0 = 0; c0 < C; c0 += 4) {
    const int c = c0 + grp < C ? c0 + grp : C - 1;
    int lo = 32767, hi = -32768;
#pragma unroll 8
    for (int k = l; k < 512; k += 16) {
      const int v = sample(c, k);
      lo = min(lo, v);
      hi = max(hi, v);
    }
    // reduced over the DPP row = this channel's lanes
    const uint32_t p = group_min_pk_i16<16>(guard_pack_minmax(lo, hi));
    const double X = (double)decode_f32(guard_unpack_min(p), guard_unpack_max(p), res(c), base(c));
    double x2 = c0 + grp < C ? X * X : 0.0;
    x2 += __shfl_xor(x2, 16, 64);
    x2 += __shfl_xor(x2, 32, 64);
    sx += x2;
  }
  return sx;
}

// The verdict on one row by one wave (every lane calls it; the result is wave-uniform), for the
// kernels whose rows a single wave normalises (window_wide_kernel, the 32-channel kernel, the
// staged one-pass writers).  acc, sx: this lane's shares of the row's sum of squares and of the
// first stage's sum of X_c^2, summed over the wave here (acc returns the row's sum).  A row that
// fails the first stage is counted in `rechecked` and tested again with stage2(), a
// wave-collective call that returns the measured sum of X_c^2, bare: a scan
// (guard_measured_x2_wave) or the tracked per-channel values (guard_tracked_x2_wave).
// GuardMeasuredFirst instead: sx was the measured sum already (float32 recordings), the first
// test is the only one.  `on`: the caller's own enable condition.
struct GuardMeasuredFirst {};
template <typename Stage2>
__device__ __forceinline__ bool guard_row_fails_wave(double& acc, double sx, bool on,
                                                     Stage2 stage2, const Guard& g, int lane) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    acc += __shfl_xor(acc, off, 64);
    sx += __shfl_xor(sx, off, 64);
  }
  bool fails = on && guard_fails(acc, kGuardK2Collapsed, sx);
  if (fails) {  // wave-uniform, rare
    if (lane == 0) guard_count_rechecked(g, 1);
    if constexpr (!std::is_same<Stage2, GuardMeasuredFirst>::value)
      fails = guard_fails_measured(acc, stage2());
  }
  return fails;
}
// stage2 of guard_row_fails_wave from measured X_c^2 that the filter pass left in LDS (C <= 64).
__device__ __forceinline__ double guard_tracked_x2_wave(const double* x2, int C, int lane) {
  double sm = lane < C ? x2[lane] : 0.0;
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) sm += __shfl_xor(sm, off, 64);
  return sm;
}

// Samples of a multiplexed recording of T (int16_t or float) for the guard's rare paths, which
// read the recording itself: frame f, column col, zero past the recording's end
// (Arrays.copyOfRange's padding; toFloatArray -> 0.0f).  f >= 0 (a window follows its marker).
template <typename T>
struct Recording {
  const uint8_t* raw;
  int64_t n_frames;
  int ct;
  __device__ __forceinline__ float sample(int64_t f, int col) const {
    return f < n_frames ? (float)*(const T*)(raw + (f * ct + col) * (int64_t)sizeof(T)) : 0.0f;
  }
  // the decoded sample, as every kernel decodes it
  __device__ __forceinline__ double x(int64_t f, int col, float r, float b) const {
    return (double)decode_f32(sample(f, col), r, b);
  }
};

}  // namespace dev
}  // namespace eegfx
