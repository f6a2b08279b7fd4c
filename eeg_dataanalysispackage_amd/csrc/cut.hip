// cut.hip -- the epoch writers of getData() (gfx950) and their launchers.
//   cut_epochs_kernel            a3 + a5..a7: raw multiplexed samples -> baseline-corrected
//                                epochs double[n][C][750]  (OffLineDataProvider.java:216-233)
//   cut_write_*_kernel           the same write pass after the staged baseline kernels, by layout
//   cut_features_c3_kernel       the epochs and their dwt-8 rows in one pass (3-channel file)
//   narrow_epochs_kernel         resident double epochs -> float32 (eegfx_odp_get_data_f32)
// The epoch writers take the epochs' element type as a template parameter E: double (the
// reference's double[n][C][750]) or float (the fp32 values it widens, the *_f32 entries).
// Compiled with -ffp-contract=off: every fp32/fp64 expression is evaluated as written, one
// correctly rounded IEEE operation at a time, matching the Java (strictfp-equivalent) order.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <type_traits>

#include "dwt8.h"
#include "guard.h"
#include "launch.h"
#include "rows.h"

namespace eegfx {
namespace dev {

// Float32 epochs (eegfx_cut_epochs_f32 and the epochs of eegfx_process_recording_epochs_f32): the
// kernels below hold every epoch sample as the fp32 value v - base before they widen it, and the
// float instantiations (E = float) store that value as it is.  A lane's 16-byte store then covers
// four samples where the double store covers two, so the store loops are rebuilt around quads:
// the rows a workgroup writes form one run of `count` floats at `o` (row r's sample f at
// o[r * kPost + f]; value(r, f) gives it), and lane t stores samples [head + 4 t, head + 4 t + 4)
// of it as one float4, a wave's instruction covering 1 KB as the double2 stores do.  A float* is
// only 4-byte aligned and an epoch row is 3,000 bytes, so the run starts on any 4-byte boundary:
// `head` (0..3) floats up to the first 16-byte boundary and the 0..3 floats past the last whole
// quad are stored one by one, by the first lanes.  A quad may span two rows (750 = 2 mod 4, and
// an odd head splits even a pair).
template <int NT, typename V>
__device__ __forceinline__ void store_f32_run(float* __restrict__ o, int count, int t, V value) {
  const int head0 = (int)((0u - (uint32_t)((uintptr_t)o >> 2)) & 3u);
  const int head = head0 < count ? head0 : count;
  const int nq = (count - head) >> 2;
  for (int q = t; q < nq; q += NT) {
    const int i = head + 4 * q;
    int r = i / kPost, f = i - r * kPost;
    float v[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      v[j] = value(r, f);
      if (++f == kPost) { f = 0; ++r; }
    }
    *(float4*)(o + i) = make_float4(v[0], v[1], v[2], v[3]);
  }
  const int ntail = count - head - 4 * nq;
  if (t < head + ntail) {
    const int i = t < head ? t : 4 * nq + t;  // = head + 4 nq + (t - head)
    const int r = i / kPost;
    o[i] = value(r, i - r * kPost);
  }
}

// The rows of an LDS-staged chunk: frames [0, nf) of each of the C channel rows at `o`.  A whole
// epoch (nf = 750, the usual case) is one run; a partial chunk is one run of nf floats per row.
template <typename V>
__device__ __forceinline__ void store_f32_rows(float* __restrict__ o, int C, int nf, int t, V value) {
  if (nf == kPost) {
    store_f32_run<256>(o, C * kPost, t, value);
  } else {
    for (int c = 0; c < C; ++c)
      store_f32_run<256>(o + c * kPost, nf, t, [&](int, int f) { return value(c, f); });
  }
}

// The same rows as doubles: lane t stores pair q of channel row c, frames 2q and 2q + 1, as one
// 16-byte store (nf is even, so a pair never straddles two rows); (c, q) steps by 256 pairs.
template <typename V>
__device__ __forceinline__ void store_f64_rows(double* __restrict__ o, int C, int nf, int t, V value) {
  const int hp = nf / 2, npairs = C * hp, sc = 256 / hp, sq = 256 % hp;
  int c = t / hp, q = t - (t / hp) * hp;
  for (int idx = t; idx < npairs; idx += 256) {
    const int f = 2 * q;
    *(double2*)(o + (int64_t)c * kPost + f) = make_double2((double)value(c, f), (double)value(c, f + 1));
    c += sc;
    q += sq;
    if (q >= hp) { q -= hp; ++c; }
  }
}
template <typename E, typename V>
__device__ __forceinline__ void store_rows(E* __restrict__ o, int C, int nf, int t, V value) {
  if constexpr (std::is_same<E, float>::value) store_f32_rows(o, C, nf, t, value);
  else store_f64_rows(o, C, nf, t, value);
}

// OffLineDataProvider.java:220-225 (see fused.hip position_ok): an invalid position is cut as
// pos = 100.  The baseline kernels flag it (cut_epochs_kernel, which has none before it, itself).
__device__ __forceinline__ int64_t cut_position(int64_t p0, int64_t n_frames) {
  return p0 >= kPre && p0 - kPre <= n_frames ? p0 : kPre;
}

// The one decode: a sample inside the recording is the reference's (float)raw * res, and
// Arrays.copyOfRange zero-pads past the end (toFloatArray -> 0.0f; smp() is not evaluated there).
// The second form reads frame f, column col of the multiplexed recording.
template <typename Smp>
__device__ __forceinline__ float decode(bool inside, float res, Smp smp) {
  return inside ? (float)smp() * res : 0.0f;
}
template <typename T, typename I>
__device__ __forceinline__ float decode(const T* raw, I f, int64_t n_frames, int ct, int col,
                                        float res) {
  return decode(f >= 0 && f < n_frames, res, [&] { return raw[f * ct + col]; });
}

// Lanes 0..C-1 put the channel parameters and the epoch's C baselines into LDS (no barrier here).
__device__ __forceinline__ void stage_channels(const ChanSel& sel, const float* __restrict__ base, int C,
                                               int t, int* s_col, float* s_res, float* s_base) {
  if (t < C) {
    s_col[t] = sel.col[t];
    s_res[t] = sel.res[t];
    s_base[t] = base[t];
  }
}

// The bytes of packed int16 frames as they lie: dwords [a0, a0 + total) of the recording to
// `stage`, 8 loads in flight per thread.  The dword holding the recording's last two bytes
// (nbytes in all) is read as a half, so no load passes its end; dwords past it stage as 0.
__device__ __forceinline__ void stage_packed(uint32_t* stage, const int16_t* __restrict__ raw,
                                             int64_t a0, int total, int64_t nbytes, int t) {
  const uint32_t* src = (const uint32_t*)raw;
  for (int k0 = 0; k0 < total; k0 += 8 * 256) {
    uint32_t v[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int k = k0 + 256 * u + t;
      const int64_t a = (a0 + k) * 4;
      v[u] = 0u;
      if (k < total) {
        if (a + 4 <= nbytes) v[u] = src[a0 + k];
        else if (a + 2 <= nbytes) v[u] = (uint16_t)raw[(a >> 1)];
      }
    }
#pragma unroll
    for (int u = 0; u < 8; ++u)
      if (k0 + 256 * u + t < total) stage[k0 + 256 * u + t] = v[u];
  }
}

// a3 + a5..a7.  One workgroup per epoch.  Lanes 0..C-1 fold the 100 pre-stimulus samples of
// their channel sequentially in fp32 (Baseline.java:29-42 -- order-exact, so no tree reduction),
// then all lanes write the 750 post-stimulus samples, coalesced.
template <typename T, typename E = double>
__global__ __launch_bounds__(256) void cut_epochs_kernel(const T* __restrict__ raw, int64_t n_frames,
                                                         int ct, ChanSel sel, int C,
                                                         const int64_t* __restrict__ pos,
                                                         E* __restrict__ out,
                                                         int* __restrict__ err) {
  __shared__ float base[kMaxChannels];
  const int64_t e = blockIdx.x;
  const int64_t p0 = pos[e];
  const bool ok = p0 >= kPre && p0 - kPre <= n_frames;  // an invalid position is flagged here
  if (threadIdx.x == 0 && !ok && err)
    __hip_atomic_store(err, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  const int64_t p = cut_position(p0, n_frames);
  const int64_t lo = p - kPre;
  if ((int)threadIdx.x < C) {
    const int c = threadIdx.x;
    const int col = sel.col[c];
    const float r = sel.res[c];
    float b = 0.0f;
    for (int i = 0; i < kPre; ++i) b = b + decode(raw, lo + i, n_frames, ct, col, r);
    base[c] = b / (float)kPre;
  }
  __syncthreads();
  E* o = out + e * C * kPost;
  for (int idx = threadIdx.x; idx < C * kPost; idx += blockDim.x) {
    const int c = idx / kPost;
    const float v = decode(raw, p + (idx - c * kPost), n_frames, ct, sel.col[c], sel.res[c]);
    o[idx] = (E)(v - base[c]);  // this fallback stores single samples for both element types
  }
}

// a5..a7 write pass of the materialised epochs (getData()): the per-(epoch, channel) baselines
// come from the LDS-staged baseline kernels; the samples are read straight from the recording.
template <typename T, typename E = double>
__global__ __launch_bounds__(256) void cut_write_kernel(const T* __restrict__ raw, int64_t n_frames,
                                                        int ct, ChanSel sel, int C,
                                                        const int64_t* __restrict__ pos,
                                                        const float* __restrict__ base,
                                                        E* __restrict__ out) {
  const int64_t e = blockIdx.x;
  const int64_t p = cut_position(pos[e], n_frames);
  store_rows(out + e * C * kPost, C, kPost, (int)threadIdx.x, [&](int c, int f) {
    return decode(raw, p + f, n_frames, ct, sel.col[c], sel.res[c]) - base[e * C + c];
  });
}

// The same write pass for epochs of at most kCutPairs * 256 sample pairs (C <= 3): the channel
// parameters and the epoch's baselines go to LDS first, and each thread issues the raw reads of
// all its pairs before the first store, so a workgroup waits on memory twice instead of twice per
// loop trip (3 channels: 7.3-7.4 -> 6.0-6.7 ms per 1M epochs, profiles/r03as/, r03au/).  Since
// the LDS-staged passes below (4.6 ms there, profiles/r03az/) it serves only the layouts they skip:
// a few channels of a wide montage (ct > 8 C) or a raw buffer that is not dword aligned.
constexpr int kCutPairs = 5;
template <typename T, typename E = double>
__global__ __launch_bounds__(256) void cut_write_small_kernel(
    const T* __restrict__ raw, int64_t n_frames, int ct, ChanSel sel, int C,
    const int64_t* __restrict__ pos, const float* __restrict__ base, E* __restrict__ out) {
  __shared__ int s_col[kMaxChannels];
  __shared__ float s_res[kMaxChannels], s_base[kMaxChannels];
  const int t = threadIdx.x;
  const int64_t e = blockIdx.x;
  stage_channels(sel, base + e * C, C, t, s_col, s_res, s_base);
  const int64_t p = cut_position(pos[e], n_frames);
  __syncthreads();
  E* o = out + e * C * kPost;
  if constexpr (std::is_same<E, float>::value) {  // at most 640 quads: three trips
    store_f32_run<256>(o, C * kPost, t, [&](int c, int f) {
      return decode(raw, p + f, n_frames, ct, s_col[c], s_res[c]) - s_base[c];
    });
  } else {
    const int npairs = C * (kPost / 2);  // <= 256 * kCutPairs (launcher)
    float v0[kCutPairs], v1[kCutPairs];
#pragma unroll
    for (int u = 0; u < kCutPairs; ++u) {
      const int idx = 256 * u + t;
      v0[u] = v1[u] = 0.0f;
      if (idx < npairs) {
        const int c = idx / (kPost / 2);
        const int64_t f = p + 2 * (idx - c * (kPost / 2));
        const int col = s_col[c];
        const float r = s_res[c];
        v0[u] = decode(raw, f, n_frames, ct, col, r);
        v1[u] = decode(raw, f + 1, n_frames, ct, col, r);
      }
    }
#pragma unroll
    for (int u = 0; u < kCutPairs; ++u) {
      const int idx = 256 * u + t;
      if (idx < npairs) {
        const float b = s_base[idx / (kPost / 2)];
        *(double2*)(o + 2 * idx) = make_double2((double)(v0[u] - b), (double)(v1[u] - b));
      }
    }
  }
}

// The one-pass getData + extractFeatures of the staged write passes (FEAT: eegfx_process_recording_
// epochs, OffLineDataProvider.loadData then WaveletTransform.extractFeatures over its epochs,
// OffLineDataProvider.java:216-233 + WaveletTransform.java:107-141): after the workgroup has
// written the epoch's rows, the window frames [175, 687) are still staged in LDS, so the filter
// bank runs on them there -- lane = (channel, segment), 8 lanes per signal, 32 signals per pass
// of the 4 waves (C <= 64: at most two passes) -- instead of a second pass that re-reads the
// 12 KB of window rows from HBM.  smp(f, col): the staged raw sample of post-stimulus frame f;
// gsmp(f, col): the same sample from the recording (both zero past its end; guard.h Recording).
// The decode, filter banks, normalisation and the fma guard are those of the fused kernels (the
// shared pieces of guard.h and dwt8.h).  The feature row and the
// guard's rare-path scratch alias the staged frames once every wave is done with them (a barrier),
// so the LDS stays that of the plain write pass: configs[3]'s 51 KB, three workgroups per CU.
template <bool FAST, bool MEASURE, typename Smp, typename GSmp>
__device__ __forceinline__ void staged_features(Smp smp, GSmp gsmp, const int* s_col,
                                                const float* s_res, const float* s_base, int C,
                                                double* stage, double* gx, double* sh,
                                                double* __restrict__ fo, const Guard& guard,
                                                int tid) {
  const int lane = tid & 63, w = tid >> 6, s = lane & 7;
  double a6v[2] = {0.0, 0.0}, d6v[2] = {0.0, 0.0};
#pragma unroll
  for (int pass = 0; pass < 2; ++pass) {
    const int c0 = 32 * pass + 8 * w;
    if (c0 >= C) break;  // uniform per wave
    const int c = c0 + (lane >> 3);
    const bool valid = c < C;
    const int cc = valid ? c : 0;
    const int col = s_col[cc];
    const float r = s_res[cc], b = s_base[cc];
    float ym = 0.0f;
    signal_cascade<FAST, FAST && MEASURE>([&](int k) { return smp(175 + kSegLen * s + k, col); },
                                          r, b, lane & ~7, s, a6v[pass], d6v[pass], &ym);
    if constexpr (FAST) {
      const double x2 = signal_x2<MEASURE>(ym, r, b);
      if (valid && s == 0) gx[c] = x2;
    }
  }
  __syncthreads();  // every wave is done with the staged frames: the row may overwrite them
  double* feat = stage;
#pragma unroll
  for (int pass = 0; pass < 2; ++pass) {
    const int c = 32 * pass + 8 * w + (lane >> 3);
    if (c < C) {
      feat[c * 16 + s] = a6v[pass];
      feat[c * 16 + 8 + s] = d6v[pass];
    }
  }
  __syncthreads();
  const int F = 16 * C;
  if (w == 0) {  // SignalProcessing.normalize (SignalProcessing.java:38-52)
    if constexpr (FAST) {
      double acc = 0.0;
      for (int i = lane; i < F; i += 64) acc = __builtin_fma(feat[i], feat[i], acc);
      const double sx = lane < C ? gx[lane] : 0.0;  // C <= 64
      bool fails;  // wave-uniform (guard.h guard_row_fails_wave)
      if constexpr (!MEASURE) {  // int16: the second stage, the row's measured max |x|
        fails = guard_row_fails_wave(
            acc, sx, guard.total != nullptr,
            [&] {
              return guard_measured_x2_wave(
                  [&](int c, int k) { return (int)gsmp(175 + k, s_col[c]); },
                  [&](int c) { return s_res[c]; }, [&](int c) { return s_base[c]; }, C, lane);
            },
            guard, lane);
      } else {  // float32: the first test is the measured one
        fails = guard_row_fails_wave(acc, sx, guard.total != nullptr, GuardMeasuredFirst{}, guard,
                                     lane);
      }
      if (lane == 0) {
        sh[0] = rsqrt_nr(acc);
        sh[1] = fails ? 1.0 : 0.0;
      }
    } else if (lane == 0) {
      double acc = 0.0;
      for (int i = 0; i < F; ++i) acc = acc + feat[i] * feat[i];
      sh[0] = sqrt(acc);
    }
  }
  __syncthreads();
  if constexpr (FAST) {
    if (sh[1] != 0.0) {  // the guard's rare path: wave 0 recomputes the row under EXACT from the
                         // recording, the LDS past the row as scratch
      if (w == 0) {
        dwt8_exact_row_wave(
            [&](int c, int k) {
              return (double)decode_f32(gsmp(175 + k, s_col[c]), s_res[c], s_base[c]);
            },
            C, 16, feat + F, feat, lane);
        if (lane == 0) {
          sh[0] = 1.0;  // the row is normalised
          guard_count_recomputed(guard, 1ull);
        }
      }
      __syncthreads();
    }
  }
  const double nv = sh[0];
  for (int i = tid; i < F; i += 256) fo[i] = FAST ? feat[i] * nv : feat[i] / nv;
}

// LDS of the FEAT variants: the staged frames, or the feature row + the rare path's scratch that
// alias them if larger (16-byte aligned), then the guard's X^2 per channel and two shared words.
__host__ __device__ constexpr size_t staged_features_lds(size_t stage_bytes, int C) {
  return (((stage_bytes > (size_t)(16 * C + 768) * 8 ? stage_bytes : (size_t)(16 * C + 768) * 8)
           + 15) & ~(size_t)15) + 64 * 8 + 16;
}

// The one-pass getData + features for the reference's 3-channel file (6-byte int16 frames, the
// Fz/Cz/Pz selection; configs[0]-[2]): eight epochs per workgroup of four waves, so that the
// filter bank runs with full waves -- wave c = channel c, lane = (epoch, segment), the layout of
// the fused window kernel -- where the per-epoch staged kernel above leaves 232 of 256 lanes idle
// (measured: one pass 8.1 ms against 7.2 ms for the two passes, profiles/r04f).
//  1. stage: each epoch's 750 post-stimulus frames (1,127 dwords from the dword holding its first
//     byte) go to LDS with one skew dword per 96 (every 64 frames), so the 8 segment lanes of a
//     signal, 64 frames apart, read 8 distinct banks; epochs 1,160 dwords apart (8 mod 32).
//  2. rows: every thread decodes sample pairs (float)raw * res - b of (epoch, channel) rows and
//     stores them as 16-byte pairs, consecutive threads on consecutive pairs (the getData()
//     epochs, OffLineDataProvider.java:216-233).
//  3. features: waves 0-2 run the filter bank on the staged window frames [175, 687) (sample k of
//     segment s: half 3 (175 + 64 s + k) + col past the epoch's start half; its skew is
//     2 + s + [k >= 17], or [k >= 16] when the start half is odd and col = 2), then the rows are
//     normalised and stored as in the window kernel, fma rows through the conditioning guard.
constexpr int kCfEpochs = 8;
constexpr int kCfDwords = 1127;  // dwords staged per epoch: (2 + 750 * 6 + 3) / 4, rounded up
constexpr int kCfStride = 1160;  // LDS dwords per epoch: 1,127 + 12 skew dwords, = 8 (mod 32)
__device__ __forceinline__ int cf_lds_dword(int d) { return d + (int)(((uint32_t)d * 683u) >> 16); }
template <bool FAST, bool FEAT = true, typename E = double>
__global__ __launch_bounds__(256) void cut_features_c3_kernel(
    const int16_t* __restrict__ raw, int64_t n_frames, ChanSel sel,
    const int64_t* __restrict__ pos, const float* __restrict__ base, int64_t n,
    E* __restrict__ out, double* __restrict__ fout, Guard guard) {
  constexpr int CT = 3, C = 3, FB = 6, F = 48;
  static_assert(kCfEpochs * F * 8 + 768 * 8 <= kCfEpochs * kCfStride * 4, "rows + scratch alias");
  __shared__ __attribute__((aligned(16))) uint32_t stage[kCfEpochs * kCfStride];
  __shared__ double norm[kCfEpochs];
  __shared__ double gx[kCfEpochs * C];
  __shared__ int64_t sA[kCfEpochs];  // dword index of each epoch's first staged byte
  __shared__ int sH[kCfEpochs];      // 1 when the first frame starts at an odd half
  __shared__ int64_t sP[kCfEpochs];  // the (valid) marker position: frame of the first sample
  __shared__ int s_col[C];
  __shared__ float s_res[C], s_base[kCfEpochs * C];
  const int tid = threadIdx.x, lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int64_t e0 = (int64_t)blockIdx.x * kCfEpochs;
  const int ne = n - e0 < kCfEpochs ? (int)(n - e0) : kCfEpochs;
  const int64_t nbytes = n_frames * FB;
  if (tid < kCfEpochs) {
    const int64_t p = cut_position(tid < ne ? pos[e0 + tid] : kPre, n_frames);
    sA[tid] = (p * FB) >> 2;
    sH[tid] = (int)((p * FB) & 3) >> 1;
    sP[tid] = p;
  }
  if (tid < C) {
    s_col[tid] = sel.col[tid];
    s_res[tid] = sel.res[tid];
  }
  if (tid < kCfEpochs * C) s_base[tid] = tid < ne * C ? base[e0 * C + tid] : 0.0f;
  __syncthreads();
  {  // 1. stage: stage_packed's loop with this kernel's (epoch m, dword d) -> skewed LDS mapping
    const uint32_t* src = (const uint32_t*)raw;
    constexpr int TOTAL = kCfEpochs * kCfDwords;
    for (int k0 = 0; k0 < TOTAL; k0 += 8 * 256) {
      uint32_t v[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const int k = k0 + 256 * u + tid;
        const int m = k / kCfDwords, d = k - m * kCfDwords;
        v[u] = 0u;
        if (k < TOTAL && m < ne) {
          const int64_t a = (sA[m] + d) * 4;
          if (a + 4 <= nbytes) v[u] = src[sA[m] + d];
          else if (a + 2 <= nbytes) v[u] = (uint16_t)raw[a >> 1];
        }
      }
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const int k = k0 + 256 * u + tid;
        const int m = k / kCfDwords, d = k - m * kCfDwords;
        if (k < TOTAL) stage[m * kCfStride + cf_lds_dword(d)] = v[u];
      }
    }
  }
  __syncthreads();
  const int16_t* hs = (const int16_t*)stage;
  // staged half h of epoch m (h counted from the epoch's first staged byte)
  auto half = [&](int m, int h) { return hs[2 * m * kCfStride + h + 2 * (int)(((uint32_t)(h >> 1) * 683u) >> 16)]; };
  if constexpr (std::is_same<E, float>::value) {
    // 2. rows, float32: the workgroup's ne epochs are one run of ne * 3 * 750 floats
    store_f32_run<256>(out + e0 * C * kPost, ne * C * kPost, tid, [&](int rr, int f) {
      const int m = rr / C, c = rr - m * C;
      // Arrays.copyOfRange zero-pads past the end (toFloatArray -> 0.0f)
      const float v =
          sP[m] + f < n_frames ? (float)half(m, sH[m] + 3 * f + s_col[c]) * s_res[c] : 0.0f;
      return v - s_base[m * C + c];
    });
  } else {  // 2. rows: pair q of (epoch m, channel c) = frames 2q, 2q + 1
    constexpr int HP = kPost / 2, PER_E = C * HP;
    int idx = tid;
    int m = idx / PER_E, rem = idx - m * PER_E;
    int c = rem / HP, q = rem - c * HP;
    for (; idx < ne * PER_E; idx += 256) {
      const int h0 = sH[m] + 6 * q + s_col[c];
      const int64_t g = sP[m] + 2 * q;  // frame of the pair in the file
      const float r = s_res[c], b = s_base[m * C + c];
      // Arrays.copyOfRange zero-pads past the end (toFloatArray -> 0.0f)
      const float v0 = g < n_frames ? (float)half(m, h0) * r : 0.0f;
      const float v1 = g + 1 < n_frames ? (float)half(m, h0 + 3) * r : 0.0f;
      *(double2*)(out + ((e0 + m) * C + c) * kPost + 2 * q) =
          make_double2((double)(v0 - b), (double)(v1 - b));
      q += 256 % HP;
      c += 256 / HP;
      if (q >= HP) { q -= HP; ++c; }
      while (c >= C) { c -= C; ++m; }
    }
  }
  if constexpr (!FEAT) return;  // getData() alone (eegfx_cut_epochs_f64)
  // 3. features: wave c = channel c (waves 0-2), lane = (epoch el, segment s)
  const int el = lane >> 3, s = lane & 7;
  double a6 = 0.0, d6 = 0.0;
  if (w < C) {
    const int c = w, col = s_col[c];
    const int m = el < ne ? el : 0;
    const float r = s_res[c], b = s_base[m * C + c];
    const int hb = sH[m] + col + 3 * (175 + kSegLen * s);  // half of sample 0 of this segment
    const int16_t* own = hs + 2 * m * kCfStride + hb + 2 * (2 + s);
    const bool late16 = sH[m] + col == 3;                 // sample 16 already past the skew
    auto fetch = [&](int k) {
      return (float)own[3 * k + (k >= 17 ? 2 : (k == 16 && late16 ? 2 : 0))];
    };
    signal_cascade<FAST>(fetch, r, b, lane & ~7, s, a6, d6);
    if (FAST && s == 0) gx[el * C + c] = signal_x2<false>(0.0f, r, b);
  }
  double* fb = (double*)stage;
  __syncthreads();  // every wave is done with the staged frames: the rows may overwrite them
  if (w < C) {
    fb[el * F + w * 16 + s] = a6;
    fb[el * F + w * 16 + 8 + s] = d6;
  }
  __syncthreads();
  if (w == 0) {
    // the guard's rare path: the row recomputed under EXACT from the recording, the LDS past the
    // 8 rows as scratch (the other waves are done)
    const Recording<int16_t> rec{(const uint8_t*)raw, n_frames, CT};
    auto redo = [&](int e, double* row) {
      const int64_t f0 = sP[e] + 175;
      dwt8_exact_row_wave(
          [&](int cc, int k) {
            return rec.x(f0 + k, s_col[cc], s_res[cc], s_base[e * C + cc]);
          },
          C, 16, fb + kCfEpochs * F, row, lane);
    };
    // the guard's second stage: the row's measured max |x| per channel, from the recording
    auto recheck = [&](int e) {
      return recheck_c3<FB>((const uint8_t*)raw, n_frames, sel, (sP[e] + 175) * FB,
                            s_base + e * C, lane);
    };
    normalise_store<F, FAST, C>(fb, norm, fout + e0 * F, ne, lane, gx, guard, redo,
                                per_row_recheck(recheck));
  }
}

// The LDS-staged write pass for frames of a whole number of dwords (e.g. configs[3]'s 32-channel
// montage; used while the staged frames are at most twice the rows written, ct <= 8 C for int16).
// Reading one channel's samples straight from the multiplexed recording puts consecutive lanes a
// whole frame (64 B at 32 int16 channels) apart, so each wave load touches 64 cache lines for 128
// useful bytes (11.9 ms per 50k 32-channel epochs, 1.0 TB/s, profiles/r03at/).  Here workgroup
// (e, chunk) copies frames [f0, f0 + nf) of epoch e's post-stimulus span into LDS with coalesced
// dword loads, one padding dword per frame (frame stride FW + 1 dwords: odd when FW is even, so 64
// lanes reading 64 frames of one channel hit 64 distinct banks), then each lane decodes two
// consecutive samples of one channel row and stores them as one 16-byte pair: 2.3 ms
// (profiles/r03bc/; 16-byte staging loads measured the same as dword loads, profiles/r03az/).  Frames past the recording's end
// read as 0.0f (Arrays.copyOfRange zero padding).
// Chunk size: one chunk per epoch up to 64 KB of LDS (32 int16 channels: 51 KB, 3 workgroups per
// CU) -- each workgroup's rows are then one contiguous 192 KB run.  Chunks of 12 / 16 / 32 KB
// (more workgroups per CU, rows written in pieces) took 3.71 / 3.54 / 3.14 ms against 2.30-2.33 ms
// for 50k 32-channel epochs, C = 3 unchanged (profiles/r03bc/ab.log; -DEEGFX_CUT_LDS_MAX builds).
#ifndef EEGFX_CUT_LDS_MAX
#define EEGFX_CUT_LDS_MAX (64 * 1024)
#endif
constexpr int kCutLdsMax = EEGFX_CUT_LDS_MAX;
// The rows keep this kernel's own loops: written through store_rows and decode, its staging loop
// compiled to nested branches and the 32-channel cut took 2.326 ms against 2.301.
template <typename T, bool FEAT = false, bool FAST = false, typename E = double>
__global__ __launch_bounds__(256) void cut_write_lds_kernel(
    const T* __restrict__ raw, int64_t n_frames, int ct, ChanSel sel, int C,
    const int64_t* __restrict__ pos, const float* __restrict__ base, E* __restrict__ out,
    int nfc, double* __restrict__ fout = nullptr, Guard guard = Guard{nullptr, nullptr, nullptr}) {
  extern __shared__ __attribute__((aligned(16))) uint32_t stage[];
  __shared__ int s_col[kMaxChannels];
  __shared__ float s_res[kMaxChannels], s_base[kMaxChannels];
  const int t = threadIdx.x;
  const int64_t e = blockIdx.x;
  const int f0 = (int)blockIdx.y * nfc;
  const int nf = kPost - f0 < nfc ? kPost - f0 : nfc;  // even: nfc and kPost are
  if (t < C) {
    s_col[t] = sel.col[t];
    s_res[t] = sel.res[t];
    s_base[t] = base[e * C + t];
  }
  const int64_t p = cut_position(pos[e], n_frames);
  const int FW = ct * (int)sizeof(T) / 4, FS = FW + 1;
  const int64_t g0 = p + f0;  // first frame of this chunk
  const uint32_t* src = (const uint32_t*)raw;
  {  // dword k of the chunk is (frame k / FW, word k % FW); 8 loads in flight per thread
    const int total = nf * FW, sf = 256 / FW, sw = 256 % FW;
    int f = t / FW, w = t - (t / FW) * FW;
    for (int k0 = 0; k0 < total; k0 += 8 * 256) {
      uint32_t v[8];
      int fk[8], wk[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        fk[u] = f;
        wk[u] = w;
        const bool in = k0 + 256 * u + t < total && g0 + f < n_frames;
        v[u] = in ? src[(g0 + f) * FW + w] : 0u;
        f += sf;
        w += sw;
        if (w >= FW) { w -= FW; ++f; }
      }
#pragma unroll
      for (int u = 0; u < 8; ++u)
        if (k0 + 256 * u + t < total) stage[fk[u] * FS + wk[u]] = v[u];
    }
  }
  __syncthreads();
  if constexpr (std::is_same<E, float>::value) {
    float* o = out + e * C * kPost + f0;
    auto value = [&](int c, int f) {
      float s0;
      if constexpr (sizeof(T) == 2) s0 = (float)((const int16_t*)stage)[2 * f * FS + s_col[c]];
      else s0 = ((const float*)stage)[f * FS + s_col[c]];
      // Arrays.copyOfRange zero-pads past the end (toFloatArray -> 0.0f)
      const float v = g0 + f < n_frames ? s0 * s_res[c] : 0.0f;
      return v - s_base[c];
    };
    store_f32_rows(o, C, nf, t, value);
  } else {
    // rows: pair q of channel c covers frames f0 + 2q, f0 + 2q + 1
    const int hp = nf / 2, npairs = C * hp, sc = 256 / hp, sq = 256 % hp;
    int c = t / hp, q = t - (t / hp) * hp;
    double* o = out + e * C * kPost + f0;
    for (int idx = t; idx < npairs; idx += 256) {
      const int col = s_col[c];
      const float r = s_res[c], b = s_base[c];
      const int f = 2 * q;
      float s0, s1;
      if constexpr (sizeof(T) == 2) {
        const int16_t* h = (const int16_t*)stage;
        s0 = (float)h[2 * f * FS + col];
        s1 = (float)h[2 * (f + 1) * FS + col];
      } else {
        const float* h = (const float*)stage;
        s0 = h[f * FS + col];
        s1 = h[(f + 1) * FS + col];
      }
      // Arrays.copyOfRange zero-pads past the end (toFloatArray -> 0.0f)
      const float v0 = g0 + f < n_frames ? s0 * r : 0.0f;
      const float v1 = g0 + f + 1 < n_frames ? s1 * r : 0.0f;
      *(double2*)(o + (int64_t)c * kPost + f) = make_double2((double)(v0 - b), (double)(v1 - b));
      c += sc;
      q += sq;
      if (q >= hp) { q -= hp; ++c; }
    }
  }
  if constexpr (FEAT) {  // one chunk per epoch (launcher): the window frames are staged
    double* gx = (double*)((uint8_t*)stage + staged_features_lds((size_t)nf * FS * 4, C) - 64 * 8 - 16);
    const Recording<T> rec{(const uint8_t*)raw, n_frames, ct};
    staged_features<FAST, !std::is_same<T, int16_t>::value>(
        [&](int f, int col) {
          if constexpr (sizeof(T) == 2) return (float)((const int16_t*)stage)[2 * f * FS + col];
          else return ((const float*)stage)[f * FS + col];
        },
        [&](int f, int col) { return rec.sample(g0 + f, col); }, s_col, s_res, s_base, C,
        (double*)stage, gx, gx + 64, fout + e * 16 * C, guard, t);
  }
}

// The same LDS-staged write pass for int16 frames that are not a whole number of dwords (the
// 3-channel path of configs[0]-[2]: 6-byte frames): the chunk's bytes are staged as they lie, from
// the dword that holds its first frame, without per-frame padding; lanes reading the sample pairs
// of one channel are 2 frames apart (3 dwords at 3 channels: an odd stride, no bank conflicts).
template <bool FEAT = false, bool FAST = false, typename E = double>
__global__ __launch_bounds__(256) void cut_write_lds_packed_kernel(
    const int16_t* __restrict__ raw, int64_t n_frames, int ct, ChanSel sel, int C,
    const int64_t* __restrict__ pos, const float* __restrict__ base, E* __restrict__ out,
    int nfc, double* __restrict__ fout = nullptr, Guard guard = Guard{nullptr, nullptr, nullptr}) {
  extern __shared__ __attribute__((aligned(16))) uint32_t stage[];
  __shared__ int s_col[kMaxChannels];
  __shared__ float s_res[kMaxChannels], s_base[kMaxChannels];
  const int t = threadIdx.x;
  const int64_t e = blockIdx.x;
  const int f0 = (int)blockIdx.y * nfc;
  const int nf = kPost - f0 < nfc ? kPost - f0 : nfc;
  stage_channels(sel, base + e * C, C, t, s_col, s_res, s_base);
  const int64_t p = cut_position(pos[e], n_frames);
  const int64_t g0 = p + f0;
  const int FB = 2 * ct;
  const int64_t b0 = g0 * FB;                 // first byte of the chunk
  const int delta = (int)(b0 & 3);            // 0 or 2
  const int total = (delta + nf * FB + 3) >> 2;
  stage_packed(stage, raw, b0 >> 2, total, n_frames * FB, t);
  __syncthreads();
  const int16_t* h = (const int16_t*)((const uint8_t*)stage + delta);
  store_rows(out + e * C * kPost + f0, C, nf, t, [&](int c, int f) {
    return decode(g0 + f < n_frames, s_res[c], [&] { return h[f * ct + s_col[c]]; }) - s_base[c];
  });
  if constexpr (FEAT) {  // one chunk per epoch (launcher): the window frames are staged
    double* gx = (double*)((uint8_t*)stage + staged_features_lds((size_t)total * 4, C) - 64 * 8 - 16);
    const Recording<int16_t> rec{(const uint8_t*)raw, n_frames, ct};
    staged_features<FAST, false>(
        [&](int f, int col) { return (float)h[f * ct + col]; },
        [&](int f, int col) { return rec.sample(g0 + f, col); }, s_col, s_res, s_base, C,
        (double*)stage, gx, gx + 64, fout + e * 16 * C, guard, t);
  }
}

}  // namespace dev

// ---- launchers ---------------------------------------------------------------------------------
// Frames per LDS chunk of the staged getData passes: an even count, the 750 frames split into as
// few chunks as keep each chunk's LDS (frame_bytes per frame + slack) within kCutLdsMax.
static int cut_chunk_frames(int frame_bytes, int slack) {
  for (int nch = 1;; ++nch) {
    const int nfc = ((dev::kPost + nch - 1) / nch + 1) & ~1;
    if ((int64_t)nfc * frame_bytes + slack <= dev::kCutLdsMax || nfc <= 2) return nfc;
  }
}
// E: the epochs' element type (double: eegfx_cut_epochs_f64; float: eegfx_cut_epochs_f32, the
// same kernels storing the fp32 sample unwidened).
template <typename E>
static hipError_t cut_epochs_impl(hipStream_t st, const void* raw, int fmt, int64_t n_frames, int ct,
                                  const ChanSel& sel, int C, const int64_t* pos, int64_t n,
                                  E* out, void* scratch, int* err) {
  if (n == 0) return hipSuccess;
  dim3 grid((unsigned)n), block(256);
  // baselines by the staged kernels when a layout fits them, then the coalesced write pass
  hipError_t be = hipErrorNotSupported;
  // the write pass stores 16-byte pairs of doubles; its float stores align themselves
  const bool aligned = std::is_same<E, float>::value || ((uintptr_t)out & 15) == 0;
  if (!aligned) scratch = nullptr;
  if (scratch && fmt == 0 && ct == 3 && C == 3)
    be = launch_fused_baseline(st, raw, n_frames, ct, sel, C, pos, n, scratch, err, nullptr);
  else if (scratch && baseline_any_supported(fmt, ct, C))
    be = launch_baseline_any(st, raw, fmt, n_frames, ct, sel, C, pos, n, scratch, err, nullptr);
  if (be == hipSuccess && fmt == 0 && ct == 3 && C == 3 && ((uintptr_t)raw & 3) == 0) {
    // the reference's 3-channel file: the eight-epoch staged kernel without its feature phase
    // (4.8 -> 4.4 ms per 1M epochs against the per-epoch staged kernel, profiles/r04g)
    const dim3 g8((unsigned)((n + dev::kCfEpochs - 1) / dev::kCfEpochs));
    hipLaunchKernelGGL((dev::cut_features_c3_kernel<false, false, E>), g8, block, 0, st,
                       (const int16_t*)raw, n_frames, sel, pos, (const float*)scratch, n, out,
                       nullptr, Guard{nullptr, nullptr, nullptr});
    return hipGetLastError();
  }
  if (be == hipSuccess) {
    const bool small = C * (dev::kPost / 2) <= 256 * dev::kCutPairs;
    const int fbytes = ct * (fmt == 0 ? 2 : 4);
    // LDS staging reads every byte of the epoch's frames: used while they are at most twice the
    // rows written (ct <= 8 C int16), so a few channels of a wide montage keep the direct reads
    const bool stage = ((uintptr_t)raw & 3) == 0 && (int64_t)dev::kPost * fbytes <= 2 * 6000LL * C;
    if (stage && fbytes % 4 != 0 && fmt == 0) {
      const int nfc = cut_chunk_frames(fbytes, 8);
      const int nchunks = (dev::kPost + nfc - 1) / nfc;
      dim3 g2((unsigned)n, (unsigned)nchunks);
      hipLaunchKernelGGL((dev::cut_write_lds_packed_kernel<false, false, E>), g2, block,
                         (size_t)nfc * fbytes + 8, st, (const int16_t*)raw, n_frames, ct, sel, C,
                         pos, (const float*)scratch, out, nfc);
    } else if (stage && fbytes % 4 == 0) {
      // wide layouts: LDS-staged chunks of the epoch, an even number of frames each
      const int fs_bytes = (fbytes / 4 + 1) * 4;
      const int nfc = cut_chunk_frames(fs_bytes, 0);
      const int nchunks = (dev::kPost + nfc - 1) / nfc;
      dim3 g2((unsigned)n, (unsigned)nchunks);
      const size_t lds = (size_t)nfc * fs_bytes;
      if (fmt == 0)
        hipLaunchKernelGGL((dev::cut_write_lds_kernel<int16_t, false, false, E>), g2, block, lds,
                           st, (const int16_t*)raw, n_frames, ct, sel, C, pos,
                           (const float*)scratch, out, nfc);
      else
        hipLaunchKernelGGL((dev::cut_write_lds_kernel<float, false, false, E>), g2, block, lds,
                           st, (const float*)raw, n_frames, ct, sel, C, pos,
                           (const float*)scratch, out, nfc);
    } else if (fmt == 0 && small)
      hipLaunchKernelGGL((dev::cut_write_small_kernel<int16_t, E>), grid, block, 0, st,
                         (const int16_t*)raw, n_frames, ct, sel, C, pos, (const float*)scratch, out);
    else if (fmt == 0)
      hipLaunchKernelGGL((dev::cut_write_kernel<int16_t, E>), grid, block, 0, st,
                         (const int16_t*)raw, n_frames, ct, sel, C, pos, (const float*)scratch, out);
    else if (small)
      hipLaunchKernelGGL((dev::cut_write_small_kernel<float, E>), grid, block, 0, st,
                         (const float*)raw, n_frames, ct, sel, C, pos, (const float*)scratch, out);
    else
      hipLaunchKernelGGL((dev::cut_write_kernel<float, E>), grid, block, 0, st, (const float*)raw,
                         n_frames, ct, sel, C, pos, (const float*)scratch, out);
    return hipGetLastError();
  }
  if (fmt == 0)
    hipLaunchKernelGGL((dev::cut_epochs_kernel<int16_t, E>), grid, block, 0, st,
                       (const int16_t*)raw, n_frames, ct, sel, C, pos, out, err);
  else
    hipLaunchKernelGGL((dev::cut_epochs_kernel<float, E>), grid, block, 0, st, (const float*)raw,
                       n_frames, ct, sel, C, pos, out, err);
  return hipGetLastError();
}

hipError_t launch_cut_epochs(hipStream_t st, const void* raw, int fmt, int64_t n_frames, int ct,
                             const ChanSel& sel, int C, const int64_t* pos, int64_t n,
                             double* out, void* scratch, int* err) {
  return cut_epochs_impl(st, raw, fmt, n_frames, ct, sel, C, pos, n, out, scratch, err);
}
hipError_t launch_cut_epochs(hipStream_t st, const void* raw, int fmt, int64_t n_frames, int ct,
                             const ChanSel& sel, int C, const int64_t* pos, int64_t n,
                             float* out, void* scratch, int* err) {
  return cut_epochs_impl(st, raw, fmt, n_frames, ct, sel, C, pos, n, out, scratch, err);
}

template <typename E>
static hipError_t cut_features_impl(hipStream_t st, const void* raw, int fmt, int64_t n_frames,
                                    int ct, const ChanSel& sel, int C, const int64_t* pos,
                                    int64_t n, E* out, double* feat, bool fast, void* scratch,
                                    int* err, const Guard& guard) {
  if (!cut_features_supported(fmt, ct, C, raw, out, feat)) return hipErrorNotSupported;
  if (n == 0) return hipSuccess;
  hipError_t be = fmt == 0 && ct == 3 && C == 3
                      ? launch_fused_baseline(st, raw, n_frames, ct, sel, C, pos, n, scratch, err,
                                              nullptr)
                      : launch_baseline_any(st, raw, fmt, n_frames, ct, sel, C, pos, n, scratch, err,
                                            nullptr);
  if (be != hipSuccess) return be;
  const dim3 grid((unsigned)n), block(256);
  const int fbytes = ct * (fmt == 0 ? 2 : 4);
  const float* bs = (const float*)scratch;
  const Guard g = fast ? guard : Guard{nullptr, nullptr, nullptr};
  auto launch = [&](auto fa) {  // fa: `fast` as a type, the kernels' FAST
    constexpr bool FA = decltype(fa)::value;
    if (fmt == 0 && ct == 3 && C == 3) {  // the reference's file: eight epochs per workgroup
      const dim3 g8((unsigned)((n + dev::kCfEpochs - 1) / dev::kCfEpochs));
      hipLaunchKernelGGL((dev::cut_features_c3_kernel<FA, true, E>), g8, block, 0, st,
                         (const int16_t*)raw, n_frames, sel, pos, bs, n, out, feat, g);
    } else if (fbytes % 4 != 0) {  // int16, packed frames
      const size_t lds = dev::staged_features_lds((size_t)dev::kPost * fbytes + 8, C);
      hipLaunchKernelGGL((dev::cut_write_lds_packed_kernel<true, FA, E>), grid, block, lds, st,
                         (const int16_t*)raw, n_frames, ct, sel, C, pos, bs, out, dev::kPost, feat, g);
    } else {
      const int fs_bytes = (fbytes / 4 + 1) * 4;
      const size_t lds = dev::staged_features_lds((size_t)dev::kPost * fs_bytes, C);
      if (fmt == 0)
        hipLaunchKernelGGL((dev::cut_write_lds_kernel<int16_t, true, FA, E>), grid, block, lds, st,
                           (const int16_t*)raw, n_frames, ct, sel, C, pos, bs, out, dev::kPost, feat, g);
      else
        hipLaunchKernelGGL((dev::cut_write_lds_kernel<float, true, FA, E>), grid, block, lds, st,
                           (const float*)raw, n_frames, ct, sel, C, pos, bs, out, dev::kPost, feat, g);
    }
  };
  if (fast) launch(std::true_type{}); else launch(std::false_type{});
  return hipGetLastError();
}
hipError_t launch_cut_features(hipStream_t st, const void* raw, int fmt, int64_t n_frames, int ct,
                               const ChanSel& sel, int C, const int64_t* pos, int64_t n,
                               double* out, double* feat, bool fast, void* scratch, int* err,
                               const Guard& guard) {
  return cut_features_impl(st, raw, fmt, n_frames, ct, sel, C, pos, n, out, feat, fast, scratch, err,
                           guard);
}
hipError_t launch_cut_features(hipStream_t st, const void* raw, int fmt, int64_t n_frames, int ct,
                               const ChanSel& sel, int C, const int64_t* pos, int64_t n,
                               float* out, double* feat, bool fast, void* scratch, int* err,
                               const Guard& guard) {
  return cut_features_impl(st, raw, fmt, n_frames, ct, sel, C, pos, n, out, feat, fast, scratch, err,
                           guard);
}

// The one-pass kernels stage the whole post-stimulus span of an epoch (one chunk) plus the
// feature row and scratch in at most 64 KB of LDS: int16 files up to ~40 channels, float32 ~20.
// out_align: the alignment the epoch stores need (16: pairs of doubles; 4: the float stores align
// themselves, store_f32_run).
static bool cut_features_fit(int fmt, int ct, int C, const void* raw, const void* out,
                             uintptr_t out_align, const double* feat) {
  if (!(fmt == 0 || fmt == 1) || C < 1 || C > kMaxChannels || ct < 1) return false;
  if (((uintptr_t)raw & 3) || ((uintptr_t)out & (out_align - 1)) || !feat) return false;
  // the 3-channel kernel stores its rows as 16-byte pairs (normalise_store); the staged kernels
  // store doubles
  if (fmt == 0 && ct == 3 && C == 3 && ((uintptr_t)feat & 15)) return false;
  const int fbytes = ct * (fmt == 0 ? 2 : 4);
  const size_t stage = fbytes % 4 != 0 ? (size_t)dev::kPost * fbytes + 8
                                       : (size_t)dev::kPost * ((fbytes / 4 + 1) * 4);
  if (fbytes % 4 != 0 && fmt != 0) return false;
  if (!(fmt == 0 && ct == 3 && C == 3) && !baseline_any_supported(fmt, ct, C)) return false;
  return dev::staged_features_lds(stage, C) <= 64 * 1024;
}
bool cut_features_supported(int fmt, int ct, int C, const void* raw, const double* out,
                            const double* feat) {
  return cut_features_fit(fmt, ct, C, raw, out, 16, feat);
}
bool cut_features_supported(int fmt, int ct, int C, const void* raw, const float* out,
                            const double* feat) {
  return cut_features_fit(fmt, ct, C, raw, out, 4, feat);
}

// getData() as float32 (eegfx_odp_get_data_f32): the provider's resident double epochs are
// widened fp32 values, so the narrowing is exact.  Both buffers are device allocations (16-byte
// aligned): four doubles in, one 16-byte store out per lane; the last count % 4 by single lanes.
namespace dev {
__global__ __launch_bounds__(256) void narrow_epochs_kernel(const double* __restrict__ in,
                                                            float* __restrict__ out, int64_t count) {
  const int64_t nq = count >> 2;
  for (int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x; q < nq; q += (int64_t)gridDim.x * 256) {
    const double2 a = *(const double2*)(in + 4 * q), b = *(const double2*)(in + 4 * q + 2);
    *(float4*)(out + 4 * q) = make_float4((float)a.x, (float)a.y, (float)b.x, (float)b.y);
  }
  const int64_t t = 4 * nq + (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t < count) out[t] = (float)in[t];
}
}  // namespace dev
hipError_t launch_narrow_epochs(hipStream_t st, const double* in, float* out, int64_t count) {
  if (count == 0) return hipSuccess;
  if (((uintptr_t)in & 15) || ((uintptr_t)out & 15)) return hipErrorInvalidValue;
  int64_t blocks = ((count >> 2) + 255) / 256;
  blocks = blocks < 1 ? 1 : blocks > 65536 ? 65536 : blocks;
  hipLaunchKernelGGL(dev::narrow_epochs_kernel, dim3((unsigned)blocks), dim3(256), 0, st, in, out,
                     count);
  return hipGetLastError();
}

}  // namespace eegfx
