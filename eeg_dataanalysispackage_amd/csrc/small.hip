// small.hip -- the per-epoch IFeatureExtraction drop-in (gfx950) and its launchers.
//   features_small_kernel        a11..a13 for small host batches: one workgroup per epoch
//   features_mailbox_kernel      the same, as one resident workgroup serving a host mailbox
// Compiled with -ffp-contract=off: every fp32/fp64 expression is evaluated as written, one
// correctly rounded IEEE operation at a time, matching the Java (strictfp-equivalent) order.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "dwt8.h"
#include "guard.h"
#include "launch.h"

namespace eegfx {
namespace dev {

// a11..a13 for small host batches (the per-epoch IFeatureExtraction drop-in): one workgroup per
// epoch reads the epoch's packed window rows (C x 512 doubles, pinned host memory mapped into the
// device) with 16-byte loads, all issued before the first wait -- one host-link round trip instead
// of the 72 dependent-free but scattered 8-byte loads per lane of features_from_epochs_kernel --
// stages them in LDS, runs each channel's six levels on a whole wave (dwt8_exact_signal_wave,
// channels dealt over the four waves), normalises, and writes the row back across the link.
// C <= kSmallMaxC.
//
// One epoch on one workgroup is a latency problem, not a throughput one, so this path computes
// EXACT numerics under both settings: the whole-wave levels keep each lane's dependent chain short
// (~190 operations) where the batch kernels' 8-lanes-per-signal fma cascade runs ~1,200 per lane,
// and an EXACT row needs no conditioning guard.  Under fma numerics the rows are therefore the
// EXACT ones (inside the 1e-9 contract by definition); the guard's counters do not count them.
constexpr int kSmallMaxC = 16;
#if defined(__HIP_DEVICE_COMPILE__) && !defined(__gfx950__)
#error "features_small_kernel stages 80 KB of LDS per workgroup: gfx950 (160 KB per CU) only"
#endif
struct SmallLds {
  double xs[kSmallMaxC * kWin];
  double scr[4][384];  // per-wave level scratch (dwt8_exact_signal_wave)
  double feat[kSmallMaxC * 16];
  double norm;
};
static_assert(sizeof(SmallLds) <= 160 * 1024, "features_small_kernel's LDS exceeds one gfx950 CU");

// One epoch (its C x 512 window doubles at `src`, 16-byte aligned) -> its row at `dst`, by a
// workgroup of 256 threads (uniform control flow; ends with a barrier).
__device__ __forceinline__ void small_epoch(const double* __restrict__ src_rows, int C, int nfeat,
                                            double* __restrict__ dst, SmallLds& sh) {
  typedef double f64x2 __attribute__((ext_vector_type(2)));
  const int tid = threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const f64x2* src = (const f64x2*)src_rows;
  const int npairs = C * kWin / 2;  // <= 4096: at most 16 per thread
  f64x2 v[16];
#pragma unroll
  for (int k = 0; k < 16; ++k) {
    const int i = tid + 256 * k;
    if (i < npairs) v[k] = src[i];
  }
#pragma unroll
  for (int k = 0; k < 16; ++k) {
    const int i = tid + 256 * k;
    if (i < npairs) *(f64x2*)(sh.xs + 2 * i) = v[k];
  }
  __syncthreads();
  const int F = C * nfeat;
  for (int c = w; c < C; c += 4) {  // uniform per wave
    const double f = dwt8_exact_signal_wave(sh.xs + c * kWin, sh.scr[w], lane);
    if (lane < nfeat) sh.feat[c * nfeat + lane] = f;
  }
  __syncthreads();
  // SignalProcessing.normalize: Math.pow(f, 2) summed in index order.  Wave 0 squares 64
  // features at a time, one per lane, and the running sum walks the lanes in order (readlane),
  // so the additions are the reference's, in its order, without a serial LDS round trip each.
  if (w == 0) {
    double acc = 0.0;
    for (int base = 0; base < F; base += 64) {
      const int i = base + lane;
      const double sq = i < F ? sh.feat[i] * sh.feat[i] : 0.0;
      const int m = F - base < 64 ? F - base : 64;
      for (int j = 0; j < m; ++j) acc = acc + lane_value(sq, j);
    }
    if (lane == 0) sh.norm = sqrt(acc);
  }
  __syncthreads();
  for (int i = tid; i < F; i += 256) dst[i] = sh.feat[i] / sh.norm;
  __syncthreads();  // sh is reused by the next epoch
}

__global__ __launch_bounds__(256) void features_small_kernel(const double* __restrict__ rows,
                                                             int C, int nfeat,
                                                             double* __restrict__ out) {
  __shared__ __attribute__((aligned(16))) SmallLds sh;
  const int64_t e = blockIdx.x;
  small_epoch(rows + e * C * kWin, C, nfeat, out + e * C * nfeat, sh);
}

// The opt-in resident form of the same path (eegfx_ctx_set_mailbox): one workgroup that stays on
// the device and serves the context's small host batches without a launch each.  Wave 0 polls
// the 64-bit request word of a host-mapped MailboxCmd (system-scope atomic loads, a short s_sleep
// between polls; the word carries the sequence number and the whole request); a new request's
// epochs are read from its pinned rows, computed by small_epoch exactly as
// features_small_kernel does, and written to its pinned output, then the completed sequence
// number is published (system-scope release after every wave's stores).  The kernel returns when
// the host sets `stop`, or after idle_ticks (s_memrealtime, 100 MHz) without a request -- every
// wave reaches that exit; the host relaunches it on the next request.  At entry it publishes its
// launch generation in `alive`: the host posts a request only to a server that has started (a
// kernel still queued behind other work is never handed a request the launch path might also
// serve).
__global__ __launch_bounds__(256) void features_mailbox_kernel(MailboxCmd* mb, uint64_t idle_ticks,
                                                               uint32_t gen) {
  __shared__ __attribute__((aligned(16))) SmallLds sh;
  __shared__ uint32_t cmd[2];  // request to serve, 0 = return
  const int tid = threadIdx.x;
  // Control flow stays wave-uniform throughout: wave 0 polls with all 64 lanes (one request per
  // poll, the loaded word made uniform with readfirstlane).  A lane-divergent `if (tid == 0)`
  // poll at the loop top let the compiler structurise the loop so that lanes other than 0 went
  // round the served request again instead of waiting at the barrier -- the server then never
  // answered.
  const bool wave0 = __builtin_amdgcn_readfirstlane(tid >> 6) == 0;
  uint32_t last = (uint32_t)__builtin_amdgcn_readfirstlane(
      (int)__hip_atomic_load(&mb->done, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_SYSTEM));
  const double* rows = mb->rows;
  double* out = mb->out;
  if (tid == 0) __hip_atomic_store(&mb->alive, gen, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
  for (;;) {
    if (wave0) {
      uint64_t go = 0;
      const uint64_t t0 = wall_clock64();
      for (;;) {
        // both words in one round trip across the link: relaxed loads issued back to back (an
        // acquire load would wait for its value before the second load); the acquire is the
        // system-scope fence every wave runs once a request is seen
        const uint64_t r = __hip_atomic_load(&mb->req, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        const uint32_t st = __hip_atomic_load(&mb->stop, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        const uint32_t lo = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)r);
        const uint32_t hi = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(r >> 32));
        if (hi != last) {
          go = (uint64_t)hi << 32 | lo;
          break;
        }
        if (__builtin_amdgcn_readfirstlane((int)st)) break;
        if (wall_clock64() - t0 > idle_ticks) break;
        __builtin_amdgcn_s_sleep(2);
      }
      if (tid == 0) {
        cmd[0] = (uint32_t)(go >> 32);
        cmd[1] = (uint32_t)go;
      }
    }
    __syncthreads();
    const uint32_t seq = (uint32_t)__builtin_amdgcn_readfirstlane((int)cmd[0]);
    if (seq == 0) break;  // stop or idle
    const uint32_t word = (uint32_t)__builtin_amdgcn_readfirstlane((int)cmd[1]);
    const int C = (int)((word >> 26) & 31) + 1, nfeat = (int)((word >> 21) & 31) + 1;
    const int64_t n = (int64_t)(word & ((1u << 21) - 1));
    // every wave: no stale line of the (reused) pinned rows from an earlier request
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "");
    for (int64_t e = 0; e < n; ++e)
      small_epoch(rows + e * C * kWin, C, nfeat, out + e * C * nfeat, sh);
    __threadfence_system();  // this thread's rows reach the host before the flag below
    __syncthreads();
    if (tid == 0) __hip_atomic_store(&mb->done, seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    last = seq;
  }
}

}  // namespace dev

bool features_small_supported(int C) { return C >= 1 && C <= dev::kSmallMaxC; }

hipError_t launch_features_mailbox(hipStream_t st, MailboxCmd* mb, uint64_t idle_ticks,
                                   uint32_t gen) {
  hipLaunchKernelGGL(dev::features_mailbox_kernel, dim3(1), dim3(256), 0, st, mb, idle_ticks, gen);
  return hipGetLastError();
}

hipError_t launch_features_small(hipStream_t st, const double* rows, int64_t n, int C, int nfeat,
                                 double* out) {
  if (n == 0) return hipSuccess;
  if (!features_small_supported(C)) return hipErrorNotSupported;
  hipLaunchKernelGGL(dev::features_small_kernel, dim3((unsigned)n), dim3(256), 0, st, rows, C,
                     nfeat, out);
  return hipGetLastError();
}

}  // namespace eegfx
