// fused.hip -- the benchmarked hot path: multiplexed int16 recording -> dwt-8 feature matrix.
//
// Replaces the reference's per-epoch chain
//   OffLineDataProvider.java:185-233  readBinaryData x3, copyOfRange, toFloatArray,
//                                      Baseline.correct, EpochHolder.setXZ
//   WaveletTransform.java:107-141      copy 512, eegdsp DWT, keep 16, normalize
// without materialising the 18 KB double[3][750] epoch: only the 612 frames that reach the
// features (100 baseline + 512 window) are read from HBM, and only the 384 B feature row is
// written back (4,064 algorithmic bytes per epoch).
//
// Two launches on one stream (DESIGN.md "Kernels"):
//
//  baseline_kernel  the 100 pre-stimulus frames of 64 epochs are staged in LDS by LDS-DMA (one
//                   16-byte-per-lane DMA per epoch, all issued before the one wait, no VGPR
//                   staging; runs against the end of the recording go through registers,
//                   zero-filled); lane e of wave c folds
//                   (epoch e, channel c) sequentially in fp32 -- Baseline.java:29-42 is
//                   order-exact, so this is deliberately not a tree reduction -- and writes
//                   b[n][C] (12 B per epoch) and each epoch's window word (byte offset of the
//                   window + an out-of-range bit) for window_kernel.  It also validates every
//                   marker position (OffLineDataProvider.java:220-225: pos-100 in [0, n_frames]).
//
//  window_kernel    workgroup = C waves (wave c = channel c), sub-tile = 8 epochs x 8 lanes per
//                   signal (dwt8.h).  The 512-frame windows arrive by LDS-DMA
//                   (global_load_lds_dwordx4: 16-byte aligned per-lane sources, no VGPRs) into a
//                   per-epoch LDS layout whose strides keep every half-wave of ds_read_u16 on
//                   distinct banks; each lane folds the window's sub-16-byte misalignment into
//                   its read base.  Lanes decode (float)raw*res - b two samples at a time just in
//                   time and run the filter bank (dwt8.h signal_cascade -- fma numerics: levels
//                   1-5 collapsed; EXACT: value halos in the reference's order).  fma:
//                   every channel wave normalises and stores its 16 features of each row from
//                   registers, the conditioning guard (guard.h) testing each row; EXACT: one wave
//                   normalises the 8 x 48 features (sequential sum of squares,
//                   SignalProcessing.java:38-52) and stores them as contiguous wave stores.
//
// The alternatives measured against this pair (persistent, work-queue, two-sub-tile and
// loader/consumer variants, the baselines folded into the window kernel, the collapsed operator
// on the FP64 matrix cores, the register-direct window, the six-point form with 4 lanes per
// signal, rows through LDS under fma) are kept as patches under tools/probes/history/ with their
// numbers in tools/probes/HISTORY.md and DESIGN.md §6; none of them ships.  A rejected variant
// goes there, not behind a compile-time switch: the switches left choose code only for the live
// ablation study (EEGFX_GUARD, EEGFX_COLLAPSED, EEGFX_TOOM) and the guard strategy (EEGFX_TRACK_X).
#include <hip/hip_runtime.h>

#include <cstdint>
#include <type_traits>

#include "dwt8.h"
#include "guard.h"
#include "launch.h"
#include "lds_dma.h"
#include "rows.h"

namespace eegfx {
namespace dev {

typedef uint32_t u32x4_a4 __attribute__((ext_vector_type(4), aligned(4)));
typedef uint32_t u32x4_a16 __attribute__((ext_vector_type(4), aligned(16)));

constexpr int kSub = 8;    // epochs per window sub-tile (8 epochs x 8 segments = 64 lanes)

constexpr int round_up_res(int v, int mod, int res) {  // smallest x >= v with x % mod == res
  return v + (((res - v % mod) % mod) + mod) % mod;
}

// LDS geometry for a CT-channel int16 recording.  Epoch e's window occupies EPQ contiguous quads
// from dword e*ESTR: quad i holds global quad floor16(B_e) + 384*(i/25) + 16*(i%25), i.e. segment
// s (64 frames, 384 B for CT = 3) is 25 quads = 100 dwords = 4 (mod 32) after segment s-1, the
// 25th quad covering the misalignment.  ESTR = 1 (mod 32), so the 32 lanes of a half-wave
// (4 epochs x 8 segments) read 32 distinct banks up to each epoch's misalignment shift.
template <int CT>
struct Geometry {
  static constexpr int FB = 2 * CT;
  static constexpr int SEGQ = kSegLen * FB / 16 + 1;     // 25
  static constexpr int EPQ = 8 * SEGQ;                    // 200 quads per epoch
  static constexpr int ESTR = round_up_res(EPQ * 4, 32, 1);  // 801 dwords
  static constexpr int BASEQ = (kPre * FB + 15) / 16 + 1;    // 39 quads (600 B + misalignment)
  static constexpr int BSTR = round_up_res(BASEQ * 4, 32, 29);  // odd, 29 (mod 32)
  // bytes a window DMA spans from floor16(B): 7 segments + the last segment's 25 quads
  static constexpr int64_t SPANB = (int64_t)kSegLen * FB * 7 + 16 * (SEGQ - 1) + 16;
};

// Window word of an epoch, written by baseline_kernel for window_kernel: the byte offset of its
// 512-frame window, B = (pos + 175) * FB (even), with bit 0 set when the DMA span from floor16(B)
// does not lie wholly inside the recording (the guarded path).  The window kernel then needs no
// 64-bit compares on its fast path (SALU has no 64-bit ordered compare on gfx950: every such
// test was a VALU instruction pair per epoch).

__device__ __forceinline__ void lds_store4(uint32_t* dst, const u32x4_a4& v) {
  dst[0] = v.x; dst[1] = v.y; dst[2] = v.z; dst[3] = v.w;
}

// One 16-byte quad at byte offset A (16-aligned; may lie outside the recording): the bytes of the
// recording it covers, zero elsewhere (Arrays.copyOfRange's zero padding).
__device__ __forceinline__ u32x4_a4 load16(const uint8_t* __restrict__ raw, int64_t nbytes,
                                           int64_t A) {
  if (A >= 0 && A + 16 <= nbytes) return *(const u32x4_a16*)(raw + A);
  u32x4_a4 v = {0u, 0u, 0u, 0u};
  if (A >= 0 && A < nbytes) {  // the recording ends inside this quad (even byte count)
    uint32_t t[4] = {0u, 0u, 0u, 0u};
    for (int i = 0; i < 4; ++i) {
      const int64_t a = A + 4 * i;
      if (a + 4 <= nbytes) t[i] = *(const uint32_t*)(raw + a);
      else if (a + 2 <= nbytes) t[i] = *(const uint16_t*)(raw + a);
    }
    v.x = t[0]; v.y = t[1]; v.z = t[2]; v.w = t[3];
  }
  return v;
}

// Marker positions the reference cuts (OffLineDataProvider.java:220-225): copyOfRange(ch, pos-100,
// pos+750) throws unless 0 <= pos-100 <= len.  Device-resident positions are checked here, where
// the kernels read them anyway; a violation raises the context's error word (vector store to
// host-mapped memory), reported as EEGFX_ERANGE by the next eegfx_ctx_synchronize.  The kernels
// stay memory-safe for any position: an invalid one is replaced by kPre (a valid cut) before any
// address is formed from it, so no offset arithmetic can overflow, and every read is still
// bounds-tested or zero-filled.
__device__ __forceinline__ bool position_ok(int64_t p, int64_t n_frames) {
  return p >= kPre && p - kPre <= n_frames;
}
__device__ __forceinline__ int64_t safe_position(int64_t p, int64_t n_frames) {
  return position_ok(p, n_frames) ? p : kPre;
}
__device__ __forceinline__ void flag_position(int* err) {
  if (err) __hip_atomic_store(err, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

// Pre-stimulus word of an epoch (LDS, baseline_kernel): the byte offset of its 100-frame run,
// (pos - 100) * FB (even), with bit 0 set when the BASEQ quads from floor16 of it do not lie wholly
// inside the recording (the guarded path).
//
// Staging is by LDS-DMA, as the windows' (dma_issue): wave w stages epochs w, w + NW, ... with one
// global_load_lds_dwordx4 each -- lane q < BASEQ moves quad q from the scalar base floor16(run)
// plus the per-lane constant 16 q to stage + e * BSTR + 4 q -- and every DMA of a wave leaves
// before its one wait.  No VGPR holds a sample or an address.  An epoch whose quads reach past the
// end of the recording (or a recording shorter than a quad) is filled through registers by load16
// instead, zero outside the recording, so no read leaves [raw, raw + nbytes).
// The fold reads (epoch e, frame i) with one ds_read_i16 per lane at dword e * BSTR + const:
// BSTR = 157 = 29 (mod 32) is odd, so the 32 lanes of a half-wave fall on 32 distinct banks (up to
// each epoch's sub-quad shift of at most 3 dwords, which can pair two lanes on a bank).
template <int CT, int C, int TILE, bool STREAM = false>
__global__ __launch_bounds__((TILE * C + 63) / 64 * 64) void baseline_kernel(
    const uint8_t* __restrict__ raw, int64_t n_frames, ChanSel sel, const int64_t* __restrict__ pos,
    int64_t n, float* __restrict__ bout, int64_t* __restrict__ wout, int* __restrict__ err,
    int* __restrict__ guard_count, const unsigned long long* __restrict__ rechecked,
    unsigned long long* __restrict__ adapt, unsigned int* __restrict__ track_out) {
  using G = Geometry<CT>;
  constexpr int NT = (TILE * C + 63) / 64 * 64;
  constexpr int NW = NT / 64;                  // waves
  constexpr int PER_W = (TILE + NW - 1) / NW;  // epochs a wave stages (22 of 64)
  static_assert(G::BASEQ <= 64 && PER_W <= 64, "one DMA per epoch, one lane per word");
  __shared__ __attribute__((aligned(16))) uint32_t stage[TILE * G::BSTR];
  __shared__ int64_t tB[TILE];
  const int tid = threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int64_t nbytes = n_frames * G::FB;
  const int64_t t0 = (int64_t)blockIdx.x * TILE;
  const int nt = (n - t0) < TILE ? (int)(n - t0) : TILE;
  // a window kernel that follows may append to the guard list (fma numerics)
  if (guard_count && blockIdx.x == 0 && tid == 0) *guard_count = 0;
  // the window kernel's guard strategy for this launch (guard.h guard_adapt_update)
  if (adapt && rechecked && blockIdx.x == 0 && tid < 64)
    guard_adapt_update(rechecked, adapt, track_out, n, tid);
  if (tid < TILE) {
    const int64_t p = tid < nt ? pos[t0 + tid] : kPre;
    if (!position_ok(p, n_frames)) flag_position(err);
    const int64_t sp = safe_position(p, n_frames);
    const int64_t R = (sp - kPre) * G::FB;  // >= 0
    tB[tid] = R | (((R & ~(int64_t)15) + 16 * G::BASEQ <= nbytes) ? 0 : 1);
    if (tid < nt) {
      const int64_t B = (sp + 175) * G::FB;
      const int64_t Bq = B & ~(int64_t)15;
      wout[t0 + tid] = B | ((Bq >= 0 && Bq + G::SPANB <= nbytes) ? 0 : 1);
    }
  }
  __syncthreads();
  // the words of this wave's epochs, lane t holding epoch w + NW t's: each becomes a scalar base
  // with two v_readlane
  const int el = w + NW * lane;
  const int64_t wl = tB[el < TILE ? el : TILE - 1];
  const int lo = (int)(uint32_t)wl, hi = (int)(uint32_t)((uint64_t)wl >> 32);
  const bool active = lane < G::BASEQ;
  // bit t: epoch w + NW t exists and is not guarded (a scalar mask: the loop's tests are uniform)
  const uint64_t dma = __ballot(el < nt && (lo & 1) == 0);
  const uint64_t fix = __ballot(el < nt && (lo & 1) != 0);
  if (active) {
#pragma unroll
    for (int t = 0; t < PER_W; ++t) {
      if ((dma >> t) & 1ull) {
        const uint32_t wlo = (uint32_t)__builtin_amdgcn_readlane(lo, t);
        const uint32_t whi = (uint32_t)__builtin_amdgcn_readlane(hi, t);
        const int64_t Rq = (int64_t)(((uint64_t)whi << 32) | (wlo & ~15u));
        dma16_s<STREAM>(raw + Rq, (uint32_t)(16 * lane), stage + (w + NW * t) * G::BSTR);
      }
    }
  }
  if (fix) {  // rare: a run against the end of the recording
    for (int e = w; e < nt; e += NW) {
      const int64_t W = tB[e];
      if ((W & 1) && active)
        lds_store4(stage + e * G::BSTR + 4 * lane,
                   load16(raw, nbytes, (W & ~(int64_t)15) + 16 * lane));
    }
  }
  dma_drain();
  __syncthreads();
  if (tid >= TILE * C) return;
  const int c = tid / TILE, e = tid - c * TILE;
  if (e >= nt) return;
  const float r = sel.res[c];
  const int16_t* src = (const int16_t*)((const uint8_t*)(stage + e * G::BSTR) + (tB[e] & 14)) +
                       sel.col[c];
  float b = 0.0f;
#pragma unroll 20
  for (int i = 0; i < kPre; ++i) b = b + (float)src[i * CT] * r;
  bout[(t0 + e) * C + c] = b / (float)kPre;
}


// DMA rows of an epoch window: each row (one global_load_lds_dwordx4, lanes < SPR * SEGQ active)
// carries SPR whole segments, so the lane's source offset is the same for every row:
// lane l lands in segment SPR j + l / SEGQ, quad l % SEGQ, i.e. from byte
// 64 FB (SPR j + l / SEGQ) + 16 (l % SEGQ) = (64 FB SPR) j + 16 l - (16 SEGQ - 64 FB) (l / SEGQ)
// of floor16(B): a scalar row base plus one per-lane constant.
template <int CT>
struct DmaRows {
  using G = Geometry<CT>;
  static constexpr int SPR = 64 / G::SEGQ;                 // segments per row (2 for CT = 3)
  static constexpr int PER_E = (8 + SPR - 1) / SPR;        // rows per epoch window (4)
  static constexpr int LANES = SPR * G::SEGQ;              // active lanes per row (50)
  static constexpr int ROWB = kSegLen * G::FB * SPR;       // source bytes per row (768)
  static constexpr int ROWDW = G::SEGQ * SPR * 4;          // LDS dwords per row (200)
  static_assert(SPR >= 1 && 8 % SPR == 0, "whole segments per row");
  uint32_t off;
  bool active;
  __device__ __forceinline__ explicit DmaRows(int lane) {
    const int sg = lane / G::SEGQ;
    off = (uint32_t)(16 * lane - (16 * G::SEGQ - kSegLen * G::FB) * sg);
    active = lane < LANES;
  }
};

// Issues the LDS-DMA of one sub-tile's windows: wave w stages epochs w, w+C, w+2C, ... (every
// DMA row of each).  The window words of those epochs are loaded (scalar: e0 and e are
// wave-uniform, so these are lgkmcnt loads and every vector-memory counter slot stays with the
// DMAs) before the first DMA, so the DMAs leave back to back; an epoch whose window lies wholly
// inside the recording (bit 0 of its word clear) takes the unguarded path.  Returns whether some
// quad of this lane could not be DMA'd (the window reaches past either end of the recording).
template <int CT, int C, bool NT>
__device__ __forceinline__ bool dma_issue(const uint8_t* __restrict__ raw, int64_t nbytes,
                                          const int64_t* __restrict__ wb, int64_t e0, int ne,
                                          uint32_t* win, int w, int lane, const DmaRows<CT>& rows) {
  using G = Geometry<CT>;
  constexpr int PER_E = DmaRows<CT>::PER_E;
  constexpr int NE = (kSub + C - 1) / C;
  int64_t W[NE];
#pragma unroll
  for (int t = 0; t < NE; ++t) {  // unconditional (clamped) loads: one scalar round trip
    const int e = w + t * C < kSub ? w + t * C : kSub - 1;
    W[t] = wb[e0 + (e < ne ? e : ne - 1)];
  }
  bool need_fix = false;
#pragma unroll
  for (int t = 0; t < NE; ++t) {
    const int e = w + t * C;
    if (e >= kSub || e >= ne) continue;  // uniform
    const int64_t Bq = W[t] & ~(int64_t)15;
    const uint8_t* sb = raw + Bq;
    uint32_t* dst = win + e * G::ESTR;
    if (((uint32_t)W[t] & 1u) == 0) {
      if (rows.active) {
#pragma unroll
        for (int j = 0; j < PER_E; ++j)
          dma16_s<NT>(sb + DmaRows<CT>::ROWB * j, rows.off, dst + DmaRows<CT>::ROWDW * j);
      }
    } else if (rows.active) {
#pragma unroll
      for (int j = 0; j < PER_E; ++j) {
        const int64_t A = Bq + DmaRows<CT>::ROWB * j + rows.off;
        if (A >= 0 && A + 16 <= nbytes)
          dma16_s<NT>(sb + DmaRows<CT>::ROWB * j, rows.off, dst + DmaRows<CT>::ROWDW * j);
        else need_fix = true;
      }
    }
  }
  return need_fix;
}

// Direct (non-DMA) fill of the quads dma_issue skipped (same wave -> epoch mapping): zero or
// partial quads at either end of the recording.
template <int CT, int C>
__device__ __forceinline__ void dma_fixup(const uint8_t* __restrict__ raw, int64_t nbytes,
                                          const int64_t* __restrict__ wb, int64_t e0, int ne,
                                          uint32_t* win, int w, int lane, const DmaRows<CT>& rows) {
  using G = Geometry<CT>;
  constexpr int PER_E = DmaRows<CT>::PER_E;
  for (int e = w; e < kSub; e += C) {
    if (e >= ne) break;
    const int64_t Bq = wb[e0 + e] & ~(int64_t)15;
#pragma unroll
    for (int j = 0; j < PER_E; ++j) {
      const int64_t A = Bq + DmaRows<CT>::ROWB * j + rows.off;
      if (rows.active && (A < 0 || A + 16 > nbytes))
        lds_store4(win + e * G::ESTR + DmaRows<CT>::ROWDW * j + 4 * lane, load16(raw, nbytes, A));
    }
  }
}

// The guard's second stage for channel `col` of the flagged rows of a sub-tile, by one channel
// wave: the flagged rows (bit 8 e of `flagged` = epoch e, 8 lanes per signal)
// share the wave, L = 64, 32, 16 or 8 lanes per row for 1, 2, 3-4 or 5-8 rows; each lane
// reads 512 / L consecutive frames of its row's window as staged in LDS (segment s at 16 SEGQ s
// bytes past the epoch's misalignment) and keeps the column's min and max raw sample; those two
// are decoded exactly as the kernel decodes every sample (decode_f32, guard.h: monotone in raw),
// and X_c = max |x| is reduced over the row's lanes (ladder_reduce).  Returns X_c^2 on the lane
// sub == 0 of
// each row's slot (0 elsewhere) and the epoch of the lane's slot in *row (-1 for lanes without
// one).  delta, b: the misalignment and baseline of the lane's epoch (lane / 8), shuffled to the
// slot's epoch.
template <int FB, int SEGQ, int EBYTES>
__device__ __forceinline__ double channel_x2_rows(uint64_t flagged, const uint8_t* win, int col,
                                                  float r, float b, int delta, int lane,
                                                  int* row) {
  static_assert(kSub * 8 == 64, "one wave per channel, 8 lanes per signal");
  uint64_t T = 0;
  int k = 0;
#pragma unroll
  for (int e = 0; e < kSub; ++e)
    if ((flagged >> (8 * e)) & 1ull) { T |= (uint64_t)e << (4 * k); ++k; }
  const int sh = k <= 1 ? 6 : k <= 2 ? 5 : k <= 4 ? 4 : 3;  // log2(L)
  const int j = lane >> sh, sub = lane & ((1 << sh) - 1);
  const bool valid = j < k;
  const int e = valid ? (int)((T >> (4 * j)) & 15u) : (int)(T & 15u);
  const int de = __shfl(delta, 8 * e, 64);
  const float be = __shfl(b, 8 * e, 64);
  const uint8_t* p0 = win + e * EBYTES + de + 2 * col;
  int mn = 32767, mx = -32768;
  // FPL = 512 / L frames per lane (a multiple of 8: runs never cross a segment), one fully unrolled
  // scan per row count so that every read of a lane is in flight before the first min / max
  auto scan = [&](auto fplc) {
    constexpr int FPL = decltype(fplc)::value;
    const int f0 = sub * FPL;
#pragma unroll
    for (int t = 0; t < FPL; t += 8) {
      const int f = f0 + t;
      const uint8_t* p = p0 + 16 * SEGQ * (f >> 6) + FB * (f & 63);
#pragma unroll
      for (int i = 0; i < 8; i += 2) {
        const int v0 = *(const int16_t*)(p + FB * i), v1 = *(const int16_t*)(p + FB * (i + 1));
        mn = min(mn, min(v0, v1));
        mx = max(mx, max(v0, v1));
      }
    }
  };
  switch (sh) {  // uniform
    case 6: scan(std::integral_constant<int, 8>()); break;
    case 5: scan(std::integral_constant<int, 16>()); break;
    case 4: scan(std::integral_constant<int, 32>()); break;
    default: scan(std::integral_constant<int, 64>()); break;
  }
  // maximum over the row's L lanes of |x| of the lane's extremes (decode_f32, guard.h)
  const uint32_t u = ladder_reduce(__float_as_uint(decode_f32(mn, mx, r, be)), sh,
                                   [](uint32_t a, uint32_t b) { return max(a, b); });
  const double X = (double)__uint_as_float(u);
  *row = valid && sub == 0 ? e : -1;
  return X * X;
}

// One sub-tile (8 epochs x C channels) per workgroup of C waves, wave w = channel w.  The windows
// land by LDS-DMA (NT: non-temporal, when neighbouring windows do not overlap); after the barrier
// that publishes them each lane decodes its 64 samples straight from LDS inside level 1 and the
// cascade runs in registers with cross-lane halos (ds_bpermute).  26 KB of LDS: 6 workgroups,
// 18 waves per CU.
//   fma:   every channel wave normalises and stores its own 16 features of each row from
//          registers (the row's sum of squares combined through LDS), and the guard's second
//          stage runs on all channel waves against the windows still staged -- scanning them
//          (channel_x2_rows) or, TRK, from the max |x| every lane tracked while decoding
//          (EEGFX_TRACK_X, guard.h).
//   EXACT: the a6/d6 rows overwrite the start of the window buffer once every wave has read its
//          samples, and wave 0 normalises and stores the 8 rows (rows.h normalise_store).
template <int CT, int C, bool FAST, bool NT, bool TRK = false>
__global__ __launch_bounds__(64 * C, 5) void window_kernel(
    const uint8_t* __restrict__ raw, int64_t n_frames, ChanSel sel, const int64_t* __restrict__ wb,
    const float* __restrict__ base, int64_t n, double* __restrict__ out, Guard guard) {
  using G = Geometry<CT>;
  constexpr int F = C * 16;
  static_assert(kSub * F * 8 <= kSub * G::ESTR * 4, "feature rows alias the window buffer");
  __shared__ __attribute__((aligned(16))) uint32_t win[kSub * G::ESTR];
  __shared__ double norm[kSub];                 // the rows' norms (EXACT)
  __shared__ double gx[FAST ? kSub * C : 1];    // the guard's X^2 per signal (fma)
  __shared__ double part[FAST ? kSub * C : 1];  // per-signal sums of squares (fma)
  __shared__ double xs[FAST ? kSub * C : 1];    // measured X_c^2 of flagged rows (fma)
  const int tid = threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);  // channel
  const int el = lane >> 3, s = lane & 7;
  const int64_t nbytes = n_frames * G::FB;
  const int col = sel.col[w];
  const float r = sel.res[w];
  const int64_t e0 = (int64_t)xcd_tile(blockIdx.x, gridDim.x) * kSub;
  const int64_t rest = n - e0;  // >= 1: the grid is ceil(n / kSub) tiles, xcd_tile a bijection
  const int ne = (rest >> 31) != 0 ? kSub : ((int)rest < kSub ? (int)rest : kSub);

  const bool mine = el < ne;
  // This lane's baseline and window word: loaded unconditionally (clamped to a valid epoch) and
  // used only once the window DMAs are in flight, so the prologue waits on one round trip (the
  // window words' scalar loads) before the DMAs leave instead of three.
  const int64_t ec = e0 + (mine ? el : ne - 1);
  const float b_ld = base[ec * C + w];
  const uint32_t w_ld = (uint32_t)wb[ec];
  const DmaRows<CT> rows(lane);
  if (dma_issue<CT, C, NT>(raw, nbytes, wb, e0, ne, win, w, lane, rows))
    dma_fixup<CT, C>(raw, nbytes, wb, e0, ne, win, w, lane, rows);
  const float b = mine ? b_ld : 0.0f;
  const int delta = mine ? (int)(w_ld & 14u) : 0;
  if (FAST && EEGFX_GUARD && (lane & 7) == 0) gx[el * C + w] = guard_x2_int16(r, b);  // read after the barriers
  dma_drain();
  __syncthreads();

  // this lane's 64 samples + 8 halo samples of signal (epoch el, channel w), decoded in level 1
  double a6 = 0.0, d6 = 0.0;
  // TRK: this launch tracks max |x| (EEGFX_TRACK_X, guard.h) -- a variant of its own, so the
  // scanning launches carry no second filter loop
  constexpr bool TRACKABLE = FAST && TRK && EEGFX_GUARD;
  constexpr bool track = TRACKABLE;  // (no flag is raised without guard.total either way)
  float ymax = 0.0f;
  const uint8_t* eb = (const uint8_t*)(win + el * G::ESTR) + delta + 2 * col;
  const int16_t* own = (const int16_t*)(eb + 16 * G::SEGQ * s);
  // a3 + a6 + a7 fused into the filter bank (dwt8.h signal_cascade), read straight from the
  // staged window: own[k * CT], k < 64
  signal_cascade<FAST, TRACKABLE>([&](int k) { return (float)own[k * CT]; }, r, b, lane & ~7, s,
                                  a6, d6, &ymax);

  if constexpr (FAST) {
    // Each channel wave keeps its 16 features of each row in registers: the row's sum of squares
    // is the three channels' shares, combined through LDS in channel order (the same value in
    // every wave), and every wave normalises and stores its own part -- 8 lines of 128 B, a6 then
    // d6 of its channel -- so the staged windows stay intact for the guard's second stage, which
    // then runs on all channel waves at once.
    const double q = group8_sum(__builtin_fma(a6, a6, d6 * d6));
    if constexpr (track) {
      // the signal's measured X_c^2, X_c = max |x| over its 8 lanes
      const double x2 = signal_x2<true>(ymax, r, b);
      if (s == 0) xs[el * C + w] = x2;
    }
    if (s == 0) part[el * C + w] = q;
    __syncthreads();
    double acc = part[el * C];
#pragma unroll
    for (int c = 1; c < C; ++c) acc += part[el * C + c];
    bool fails = false;
    if (EEGFX_GUARD && guard.total && s == 0 && mine) {
      double sx = gx[el * C];
#pragma unroll
      for (int c = 1; c < C; ++c) sx += gx[el * C + c];
      fails = guard_fails(acc, kGuardK2Collapsed, sx);
    }
    const uint64_t flagged = __ballot(fails);  // bit 8e; the same mask in every channel wave
    uint64_t left = 0;
    if (flagged) {  // uniform over the workgroup, rare
      if constexpr (!track) {  // scan: the flagged rows' measured X_c^2 go to LDS first (track:
                               // every row's is there already)
        int row;
        const double x2 = channel_x2_rows<G::FB, G::SEGQ, G::ESTR * 4>(
            flagged, (const uint8_t*)win, col, r, b, delta, lane, &row);
        if (row >= 0) xs[row * C + w] = x2;
        __syncthreads();
      }
      bool f2 = false;
      if (s == 0 && ((flagged >> (8 * el)) & 1ull)) {
        double sx = xs[el * C];
#pragma unroll
        for (int c = 1; c < C; ++c) sx += xs[el * C + c];
        f2 = guard_fails_measured(acc, sx);
      }
      left = __ballot(f2);
      if (w == 0 && lane == 0) {
        guard_count_rechecked(guard, __popcll(flagged));
        if (left) guard_count_recomputed(guard, (unsigned long long)__popcll(left));
      }
    }
    const double inv = rsqrt_nr1(acc);
    if (mine && !((left >> (8 * el)) & 1ull)) {
      double* o = out + (e0 + el) * F + w * 16 + s;
      __builtin_nontemporal_store(a6 * inv, o);
      __builtin_nontemporal_store(d6 * inv, o + 8);
    }
    if (left) {  // uniform
      // the guard's rarest path: each such row recomputed under EXACT from the recording, channel
      // w by wave w (the staged windows as scratch, 768 doubles per wave: every wave is done with
      // them, the barrier above), then normalised and stored by wave 0
      double* scratch = (double*)win + w * 768;
      double* rowbuf = (double*)win + C * 768;
      const Recording<int16_t> rec{raw, n_frames, CT};
      for (uint64_t f = left; f; f &= f - 1) {
        const int e = (__ffsll((unsigned long long)f) - 1) >> 3;
        const int64_t f0 = (wb[e0 + e] & ~(int64_t)1) / G::FB;  // first frame of the window
        dwt8_exact_row_block<C>(
            // C waves: the one channel wave w is asked for is its own, c = w
            [&](int, int k) { return rec.x(f0 + k, col, r, base[(e0 + e) * C + w]); },
            C, scratch, rowbuf, w, lane);
        if (w == 0)
          for (int i = lane; i < F; i += 64) out[(e0 + e) * F + i] = rowbuf[i];
        __syncthreads();
      }
    }
  } else {
    // EXACT: the rows go to LDS over the windows, and wave 0 normalises them in the reference's
    // order (sequential sum of squares, sqrt, divide) and stores them
    double* fb = (double*)win;
    __syncthreads();  // every wave has read its samples: the rows may overwrite the window
    // the row slot is recomputed here from an opaque copy of the lane id, so its address is not
    // kept live across the filter bank (it was the one spilled VGPR)
    int l2 = lane;
    asm volatile("" : "+v"(l2));
    const int slot = (l2 >> 3) * F + w * 16 + (l2 & 7);
    fb[slot] = a6;
    fb[slot + 8] = d6;
    __syncthreads();
    if (w == 0) normalise_store<F, false>(fb, norm, out + e0 * F, ne, lane);
  }
}

}  // namespace dev

// Non-temporal (streaming) reads when the average marker spacing n_frames / n leaves the regions
// a kernel reads (min_spacing frames per epoch) disjoint, so no other epoch would reuse the bytes
// through L2 (markers 1,000 frames apart: window_kernel 0.918 -> 0.910 ms; 100 frames apart, where
// each frame sits in ~6 windows: 0.777 -> 0.802 ms -- hence the test).
bool streaming_reads(int64_t n_frames, int64_t n, int64_t min_spacing) {
  return n > 0 && n_frames / n >= min_spacing;
}

bool fused_supported(int fmt, int ct, int C, const double* out) {
  return fmt == 0 && ct == 3 && C == 3 && ((uintptr_t)out & 15) == 0;
}

// Scratch of the fused path: [n][C] float baselines, then (16-byte aligned) the n int64 window
// words of baseline_kernel.
static size_t window_words_offset(int64_t n, int C) {
  return (sizeof(float) * (size_t)n * (size_t)C + 15) & ~(size_t)15;
}
size_t fused_scratch_bytes(int64_t n, int C) {
  return window_words_offset(n, C) + sizeof(int64_t) * (size_t)n;
}

int64_t fused_window_bytes_per_epoch(int ct, int C) {
  // window + 12 B of baselines + position + feature row
  return (int64_t)dev::kWin * ct * 2 + (int64_t)C * 4 + 8 + (int64_t)C * 16 * 8;
}

hipError_t launch_fused_baseline(hipStream_t st, const void* raw, int64_t n_frames, int ct,
                                 const ChanSel& sel, int C, const int64_t* pos, int64_t n,
                                 void* scratch, int* err, int* guard_count, const Guard* guard) {
  const unsigned long long* rechecked = guard ? guard->rechecked : nullptr;
  unsigned long long* adapt = guard && guard->total ? guard->adapt : nullptr;
  unsigned int* track_out = adapt ? guard->track_out : nullptr;
  if (ct != 3 || C != 3) return hipErrorNotSupported;
  if (n == 0) return hipSuccess;
  // 64 epochs per workgroup; 32 and 128 measured the same or slower.  Streaming
  // reads unless another epoch's window or baseline may share the pre-stimulus frames.
  constexpr int kTile = 64;
  const dim3 g((unsigned)((n + kTile - 1) / kTile)), blk((kTile * 3 + 63) / 64 * 64);
  int64_t* words = (int64_t*)((uint8_t*)scratch + window_words_offset(n, C));
  if (streaming_reads(n_frames, n, dev::kPre + 687))
    hipLaunchKernelGGL((dev::baseline_kernel<3, 3, kTile, true>), g, blk, 0, st,
                       (const uint8_t*)raw, n_frames, sel, pos, n, (float*)scratch, words, err,
                       guard_count, rechecked, adapt, track_out);
  else
    hipLaunchKernelGGL((dev::baseline_kernel<3, 3, kTile>), g, blk, 0, st, (const uint8_t*)raw,
                       n_frames, sel, pos, n, (float*)scratch, words, err, guard_count, rechecked,
                       adapt, track_out);
  return hipGetLastError();
}

hipError_t launch_fused_window(hipStream_t st, const void* raw, int64_t n_frames, int ct,
                               const ChanSel& sel, int C, const int64_t* pos, int64_t n, bool fast,
                               const void* scratch, double* out, const Guard& guard, bool track) {
  if (ct != 3 || C != 3) return hipErrorNotSupported;
  if (n == 0) return hipSuccess;
  const float* bs = (const float*)scratch;
  const int64_t* words = (const int64_t*)((const uint8_t*)scratch + window_words_offset(n, C));
  (void)pos;  // read by launch_fused_baseline, which wrote the window words
  const bool nt = streaming_reads(n_frames, n, dev::kWin + 8);
  const dim3 g((unsigned)((n + dev::kSub - 1) / dev::kSub));
#define EEGFX_WIN(FA, NTV, TK)                                                          \
  hipLaunchKernelGGL((dev::window_kernel<3, 3, FA, NTV, TK>), g, dim3(192), 0, st,      \
                     (const uint8_t*)raw, n_frames, sel, words, bs, n, out, guard)
  const bool trk = EEGFX_TRACK_X != 0 && (EEGFX_TRACK_X == 2 || track) && guard.total;
  if (fast && trk) { if (nt) EEGFX_WIN(true, true, true); else EEGFX_WIN(true, false, true); }
  else if (fast) { if (nt) EEGFX_WIN(true, true, false); else EEGFX_WIN(true, false, false); }
  else { if (nt) EEGFX_WIN(false, true, false); else EEGFX_WIN(false, false, false); }
#undef EEGFX_WIN
  return hipGetLastError();
}

}  // namespace eegfx
