// api.cpp -- eegfx C ABI: device context and compute entry points.  The context's definition and
// the helpers shared with the OffLineDataProvider (odp.cpp) are declared in ctx.h.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <array>
#include <chrono>
#include <cmath>
#include <condition_variable>
#include <thread>
#include <type_traits>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <memory>
#include <mutex>
#include <sched.h>
#include <string>
#include <utility>
#include <vector>

#include "common.h"
#include "eegfx_ext.h"
#include "launch.h"
#include "spark_sample.h"

using namespace eegfx;

#include "ctx.h"


namespace eegfx {

PinnedPool& pinned_pool() {
  static PinnedPool* pool = new PinnedPool();  // never destroyed: buffers live to process exit
  return *pool;
}

ChanSel make_sel(const int32_t* cols, const float* res, int C, int ct) {
  if (C < 1 || C > kMaxChannels) fail(EEGFX_EINVAL, "C=%d outside [1, %d]", C, kMaxChannels);
  if (!cols || !res) fail(EEGFX_EINVAL, "cols/res must be host arrays");
  ChanSel s;
  memset(&s, 0, sizeof(s));
  for (int c = 0; c < C; ++c) {
    if (cols[c] < 0 || cols[c] >= ct)
      fail(EEGFX_EINVAL, "column %d of selected channel %d outside [0, %d)", cols[c], c, ct);
    s.col[c] = cols[c];
    s.res[c] = res[c];
  }
  return s;
}

void check_positions(const int64_t* pos, int64_t n, int64_t n_frames) {
  for (int64_t i = 0; i < n; ++i) {
    const int64_t lo = pos[i] - EEGFX_PRESTIMULUS;
    if (lo < 0 || lo > n_frames)
      fail(EEGFX_ERANGE, "epoch %lld: marker position %lld outside [100, %lld]", (long long)i,
           (long long)pos[i], (long long)n_frames + EEGFX_PRESTIMULUS);
  }
}

void check_fe_params(int C, int name, int epoch_size, int skip, int feature_size) {
  if (C < 1 || C > kMaxChannels) fail(EEGFX_EINVAL, "C=%d outside [1, %d]", C, kMaxChannels);
  if (skip < 0 || epoch_size <= 0 || skip + epoch_size > EEGFX_POSTSTIMULUS)
    fail(EEGFX_ERANGE, "window [%d, %d) outside the %d-sample epoch", skip, skip + epoch_size,
         EEGFX_POSTSTIMULUS);
  if (feature_size <= 0) fail(EEGFX_EINVAL, "feature size %d", feature_size);
  if (name != EEGFX_DWT8_NAME || epoch_size != EEGFX_DWT8_EPOCH_SIZE ||
      feature_size > EEGFX_DWT8_MAX_FEATURE_SIZE)
    fail(EEGFX_ENOTSUP,
         "no kernel for wavelet %d / epoch size %d / feature size %d (supported: dwt-8, 512, <=512)",
         name, epoch_size, feature_size);
}

// Feature sizes past a6 ++ d6 take the full-pyramid kernels (pyramid.hip): EXACT under both
// numerics settings, outside the fma guard and its counters, and never the per-epoch kernel or
// the resident server (mailbox_request packs nfeat - 1 into 5 bits).
bool wide_features(int feature_size) { return feature_size > EEGFX_DWT8_FEATURE_SIZE; }

}  // namespace eegfx

namespace {

// Resident-server slots per device (eegfx_ctx::mb_ready): the highest-priority hardware queues
// of the process (4 on the box: a fifth server shares a queue and waits behind another until it
// idles out).
constexpr int kMbSlotsPerDevice = 4;
constexpr int kMbMaxDevices = 64;
std::mutex g_mb_mu;
int g_mb_used[kMbMaxDevices] = {};
bool mb_acquire(int dev) {
  if (dev < 0 || dev >= kMbMaxDevices) return false;
  std::lock_guard<std::mutex> l(g_mb_mu);
  if (g_mb_used[dev] >= kMbSlotsPerDevice) return false;
  ++g_mb_used[dev];
  return true;
}
void mb_release(int dev) {
  std::lock_guard<std::mutex> l(g_mb_mu);
  if (dev >= 0 && dev < kMbMaxDevices && g_mb_used[dev] > 0) --g_mb_used[dev];
}

// Admission of small launched calls (one epoch per call from many threads, no server): at most
// kSmallCallers per device are inside the runtime at once, the others sleep and are admitted in
// arrival order.  Without it 28 threads launching and waiting on one device (Spark local[*] with
// 32 executor threads, 4 of them on servers) convoyed in the runtime: calls of 42-48 ms
// (profiles/r06/dropin_gate_ab.log; A/B builds vary the cap).  A leaving caller hands its place to
// the first waiter and wakes that thread alone (each waiter sleeps on its own condition variable):
// a shared one woke every waiter at every exit, ~24 wakeups per call at 32 threads.
#ifndef EEGFX_SMALL_CALLERS
#define EEGFX_SMALL_CALLERS 8
#endif
constexpr int kSmallCallers = EEGFX_SMALL_CALLERS;
struct SmallWaiter {
  std::condition_variable cv;
  bool admitted = false;
  SmallWaiter* next = nullptr;
};
std::mutex g_small_mu;
int g_small_inside[kMbMaxDevices] = {};
SmallWaiter* g_small_head[kMbMaxDevices] = {};  // FIFO of sleeping callers
SmallWaiter* g_small_tail[kMbMaxDevices] = {};
struct SmallCallGate {
  int dev;
  explicit SmallCallGate(int d) : dev(d >= 0 && d < kMbMaxDevices ? d : -1) {
    if (dev < 0 || kSmallCallers <= 0) return;
    std::unique_lock<std::mutex> l(g_small_mu);
    if (!g_small_head[dev] && g_small_inside[dev] < kSmallCallers) {
      ++g_small_inside[dev];
      return;
    }
    SmallWaiter me;
    (g_small_tail[dev] ? g_small_tail[dev]->next : g_small_head[dev]) = &me;
    g_small_tail[dev] = &me;
    me.cv.wait(l, [&] { return me.admitted; });  // the leaver unlinked us and kept our place
  }
  ~SmallCallGate() {
    if (dev < 0 || kSmallCallers <= 0) return;
    std::lock_guard<std::mutex> l(g_small_mu);
    SmallWaiter* w = g_small_head[dev];
    if (!w) {
      --g_small_inside[dev];
      return;
    }
    g_small_head[dev] = w->next;
    if (!g_small_head[dev]) g_small_tail[dev] = nullptr;
    w->admitted = true;
    w->cv.notify_one();  // under the lock: the waiter's frame outlives this call
  }
  SmallCallGate(const SmallCallGate&) = delete;
  SmallCallGate& operator=(const SmallCallGate&) = delete;
};

}  // namespace

bool eegfx_ctx::mb_ready() {
  if (!mailbox) return false;
  if (mb_stuck) {  // a server that never started: the launch path until it has run and returned
    if (!mb_returned()) return false;
    __atomic_store_n(&mb_host->stop, 0u, __ATOMIC_RELEASE);
    mb_stuck = false;
  }
  if (!mb_slot) {
    if (!mb_acquire(device)) return false;
    mb_slot = true;
  }
  if (!mb_stream) {
    try {
      // A stream of the highest priority: the runtime multiplexes a process's streams of one
      // priority over a few hardware queues, and a queue runs its packets in order, so a
      // normal-priority stream sharing the resident kernel's queue would wait behind it (up to
      // its 1 s idle exit).  The high-priority pool keeps the server on a queue of its own while
      // no more than kMbSlotsPerDevice servers exist.
      int least = 0, greatest = 0;
      HIP_CHECK(hipDeviceGetStreamPriorityRange(&least, &greatest));
      HIP_CHECK(hipStreamCreateWithPriority(&mb_stream, hipStreamNonBlocking, greatest));
      mb_host = (MailboxCmd*)pinned_pool().take(
          sizeof(MailboxCmd), hipHostMallocMapped | hipHostMallocCoherent, &mb_cap);
      memset(mb_host, 0, sizeof(MailboxCmd));
      HIP_CHECK(hipHostGetDevicePointer((void**)&mb_dev, mb_host, 0));
      mb_seq = 0;
    } catch (...) {
      release_mailbox();
      mailbox = true;  // still enabled: later calls retry
      throw;
    }
  }
  const auto now = std::chrono::steady_clock::now();
  // no request for 500 ms: the server may be close to its 1 s idle exit -- restart it, so no
  // request is ever posted to a kernel that is returning
  if (mb_live && now - mb_last > std::chrono::milliseconds(500)) {
    if (!mb_stop()) return false;
  }
  if (!mb_live) {
    mb_launch();
    mb_last = now;
  }
  if (!mb_started) {
    const auto t0 = std::chrono::steady_clock::now();
    while (__atomic_load_n(&mb_host->alive, __ATOMIC_ACQUIRE) != mb_gen) {
      if (std::chrono::steady_clock::now() - t0 > kMbStartWait) {
        // still queued: it returns at once when it runs (stop), the call takes the launch path
        __atomic_store_n(&mb_host->stop, 1u, __ATOMIC_RELEASE);
        mb_live = false;
        mb_stuck = true;
        return false;
      }
      __builtin_ia32_pause();
    }
    mb_started = true;
  }
  return true;
}

void eegfx_ctx::release_mailbox() {
  const bool stopped = mb_stop();
  if (mb_stream && stopped && !mb_stuck) (void)hipStreamDestroy(mb_stream);
  if (mb_host && stopped && !mb_stuck)
    pinned_pool().give(mb_host, mb_cap, hipHostMallocMapped | hipHostMallocCoherent);
  // a stuck server keeps its stream and command block (it still reads `stop` when it runs):
  // leaked rather than freed under a queued kernel
  mb_host = nullptr;
  mb_dev = nullptr;
  mb_stream = nullptr;
  mb_live = mb_started = mb_stuck = false;
  if (mb_slot) mb_release(device);
  mb_slot = false;
  mailbox = false;
}

namespace {

void* stage_in(eegfx_ctx* ctx, DevBuf& buf, const void* src, size_t bytes, int mem) {
  if (mem == EEGFX_MEM_DEVICE) return const_cast<void*>(src);
  void* d = buf.get(bytes);
  if (bytes) HIP_CHECK(hipMemcpyAsync(d, src, bytes, hipMemcpyHostToDevice, ctx->stream));
  return d;
}

// Host copy into pinned staging, split over up to 8 threads (one thread tops out near 6 GB/s,
// far below the ~57 GB/s host link it feeds).
void parallel_memcpy(void* dst, const void* src, size_t bytes) {
  const unsigned hw = std::max(1u, std::thread::hardware_concurrency());
  const size_t nt = std::min<size_t>({8, hw, std::max<size_t>(1, bytes >> 23)});
  if (nt <= 1) {
    memcpy(dst, src, bytes);
    return;
  }
  std::vector<std::thread> th;
  const size_t per = (bytes / nt + 63) & ~(size_t)63;
  for (size_t t = 0; t < nt; ++t) {
    const size_t a = t * per;
    if (a >= bytes) break;
    const size_t len = std::min(per, bytes - a);
    th.emplace_back([=] { memcpy((char*)dst + a, (const char*)src + a, len); });
  }
  for (auto& x : th) x.join();
}

// The processors this process may run on, as the JVM's Runtime.availableProcessors() counts them
// (Spark local[*]'s defaultParallelism, SparkInitializer.java:44): the affinity mask, capped by a
// cgroup CPU quota (cgroup v2 cpu.max or v1 cfs_quota_us / cfs_period_us), at least 1.
// std::thread::hardware_concurrency() counts every online CPU of the machine instead.
int available_processors() {
  int n = 0;
  cpu_set_t set;
  if (sched_getaffinity(0, sizeof(set), &set) == 0) n = CPU_COUNT(&set);
  if (n < 1) n = (int)std::max(1u, std::thread::hardware_concurrency());
  auto cap = [&](double quota, double period) {
    if (quota > 0 && period > 0) n = std::min(n, std::max(1, (int)std::ceil(quota / period)));
  };
  if (FILE* f = fopen("/sys/fs/cgroup/cpu.max", "r")) {
    char q[32] = {0};
    double period = 0;
    if (fscanf(f, "%31s %lf", q, &period) == 2 && strcmp(q, "max") != 0) cap(atof(q), period);
    fclose(f);
  } else if (FILE* fq = fopen("/sys/fs/cgroup/cpu/cpu.cfs_quota_us", "r")) {
    double quota = -1, period = 0;
    if (fscanf(fq, "%lf", &quota) != 1) quota = -1;
    fclose(fq);
    if (FILE* fp = fopen("/sys/fs/cgroup/cpu/cpu.cfs_period_us", "r")) {
      if (fscanf(fp, "%lf", &period) != 1) period = 0;
      fclose(fp);
    }
    cap(quota, period);
  }
  return n;
}


// Host batches up to this many window bytes go through the zero-copy path of
// eegfx_extract_features_f64 (about 64 epochs of 3 channels).
constexpr size_t kZeroCopyBytes = (size_t)768 << 10;
// the rows of the largest such batch: 192 window rows of 512 doubles, 16 features each
constexpr size_t kZeroCopyOutBytes =
    kZeroCopyBytes / (sizeof(double) * EEGFX_DWT8_EPOCH_SIZE) * EEGFX_DWT8_FEATURE_SIZE * sizeof(double);

void check_mem(int mem) {
  if (mem != EEGFX_MEM_HOST && mem != EEGFX_MEM_DEVICE) fail(EEGFX_EINVAL, "mem flag %d", mem);
}

// raw -> features on the context stream (device pointers).  Fused kernel when one covers the
// layout, otherwise cut + features through the context scratch buffer.
void run_features_from_raw(eegfx_ctx* ctx, const void* raw, int fmt, int64_t n_frames, int ct,
                           const ChanSel& sel, int C, const int64_t* pos, int64_t n,
                           double* out) {
  const bool fast = ctx->numerics != EEGFX_EXACT;
  // fma: rows that fail the conditioning guard (guard.h) are recomputed under EXACT -- inside the
  // kernel that flags them, or (the generic any-layout kernels) by a follow-up launch over the
  // guard list that launch_window_wide issues; baseline_any_kernel zeroes the list's count
  const Guard g = ctx->guard_for(n);
  if (fused_supported(fmt, ct, C, out)) {
    void* fscratch = ctx->fused.get(fused_scratch_bytes(n, C));
    HIP_CHECK(launch_fused_baseline(ctx->stream, raw, n_frames, ct, sel, C, pos, n, fscratch,
                                    ctx->err_dev, nullptr, fast ? &g : nullptr));
    ctx->tic();  // the dominant kernel (DESIGN.md "Measurement")
    HIP_CHECK(launch_fused_window(ctx->stream, raw, n_frames, ct, sel, C, pos, n, fast, fscratch,
                                  out, g, fast && ctx->guard_track()));
    ctx->toc(n * fused_window_bytes_per_epoch(ct, C));
    return;
  }
  if (wide_supported(fmt, ct, C)) {
    void* fscratch = ctx->fused.get(fused_scratch_bytes(n, C));
    HIP_CHECK(launch_baseline_any(ctx->stream, raw, fmt, n_frames, ct, sel, C, pos, n, fscratch,
                                  ctx->err_dev, g.count, fast ? &g : nullptr));
    ctx->tic();
    HIP_CHECK(launch_window_wide(ctx->stream, raw, fmt, n_frames, ct, sel, C, pos, n, fast,
                                 fscratch, out, g, fast && ctx->guard_track()));
    const int64_t elem = fmt == EEGFX_INT_16 ? 2 : 4;
    ctx->toc(n * (EEGFX_DWT8_EPOCH_SIZE * ct * elem + C * 4 + 8 + C * 16 * 8));
    return;
  }
  double* ep = (double*)ctx->scratch.get(sizeof(double) * (size_t)n * C * EEGFX_POSTSTIMULUS);
  ctx->tic();
  HIP_CHECK(launch_cut_epochs(ctx->stream, raw, fmt, n_frames, ct, sel, C, pos, n, ep,
                              ctx->fused.get(fused_scratch_bytes(n, C)), ctx->err_dev));
  HIP_CHECK(launch_features_from_epochs(ctx->stream, ep, n, C, EEGFX_DWT8_SKIP,
                                        EEGFX_DWT8_FEATURE_SIZE, fast, out, EEGFX_POSTSTIMULUS, g));
  ctx->toc(0);
}

}  // namespace

namespace eegfx {

// raw -> epochs + features (device pointers): the one-pass kernels when the layout fits them,
// else the cut pass followed by the batch extract over the rows it wrote.  E: double or float epochs
// (eegfx_process_recording_epochs / _f32): the same kernels, the same rows in `feat`.
template <typename E>
void run_epochs_and_features(eegfx_ctx* ctx, const void* raw, int fmt, int64_t n_frames, int ct,
                             const ChanSel& sel, int C, const int64_t* pos, int64_t n, E* ep,
                             double* feat) {
  const bool fast = ctx->numerics != EEGFX_EXACT;
  const Guard g = ctx->guard_for(n);
  void* fscratch = ctx->fused.get(fused_scratch_bytes(n, C));
  ctx->tic();
  if (cut_features_supported(fmt, ct, C, raw, ep, feat)) {
    HIP_CHECK(launch_cut_features(ctx->stream, raw, fmt, n_frames, ct, sel, C, pos, n, ep, feat,
                                  fast, fscratch, ctx->err_dev, g));
  } else {
    HIP_CHECK(launch_cut_epochs(ctx->stream, raw, fmt, n_frames, ct, sel, C, pos, n, ep, fscratch,
                                ctx->err_dev));
    HIP_CHECK(launch_features_from_epochs(ctx->stream, ep, n, C, EEGFX_DWT8_SKIP,
                                          EEGFX_DWT8_FEATURE_SIZE, fast, feat, EEGFX_POSTSTIMULUS,
                                          g));
  }
  ctx->toc(0);
}

template void run_epochs_and_features<double>(eegfx_ctx*, const void*, int, int64_t, int,
                                              const ChanSel&, int, const int64_t*, int64_t, double*,
                                              double*);

}  // namespace eegfx

namespace eegfx {
int ctx_device(const eegfx_ctx* ctx) { return ctx->device; }
void* ctx_stream(const eegfx_ctx* ctx) { return (void*)ctx->stream; }
}  // namespace eegfx

extern "C" {

const char* eegfx_version(void) { return "eegfx 0.1.0 (gfx950)"; }

int eegfx_device_count(int* count) {
  return guarded([&] {
    if (!count) fail(EEGFX_EINVAL, "null argument");
    HIP_CHECK(hipGetDeviceCount(count));
  });
}

int eegfx_ctx_create(int device, eegfx_ctx** out) {
  return guarded([&] {
    if (!out) fail(EEGFX_EINVAL, "null argument");
    std::unique_ptr<eegfx_ctx> c(new eegfx_ctx());
    c->device = device;
    c->activate();
    HIP_CHECK(hipStreamCreateWithFlags(&c->own, hipStreamNonBlocking));
    c->stream = c->own;
    c->bind_buffers();
    c->err_host = (int*)pinned_pool().take(16, hipHostMallocMapped, &c->err_cap);
    memset(c->err_host, 0, 16);  // the error word, then (+8) the guard strategy word
    HIP_CHECK(hipHostGetDevicePointer((void**)&c->err_dev, c->err_host, 0));
    // stream-ordered: no allocation or free of a context synchronises the device
    HIP_CHECK(hipMallocAsync((void**)&c->guard_dev, eegfx_ctx::kGuardDevBytes, c->own));
    HIP_CHECK(hipMemsetAsync(c->guard_dev, 0, eegfx_ctx::kGuardDevBytes, c->own));
    HIP_CHECK(hipStreamSynchronize(c->own));
    *out = c.release();
  });
}

int eegfx_ctx_set_stream(eegfx_ctx* ctx, void* hip_stream) {
  return guarded([&] {
    if (!ctx) fail(EEGFX_EINVAL, "null context");
    const hipStream_t next = hip_stream ? (hipStream_t)hip_stream : ctx->own;
    if (next == ctx->stream) return;
    // the context's buffers are ordered on its stream: drain the old one before switching
    ctx->activate();
    HIP_CHECK(hipStreamSynchronize(ctx->stream));
    ctx->stream = next;
  });
}

int eegfx_ctx_stream(eegfx_ctx* ctx, void** hip_stream) {
  return guarded([&] {
    if (!ctx || !hip_stream) fail(EEGFX_EINVAL, "null argument");
    *hip_stream = (void*)ctx->stream;
  });
}

int eegfx_ctx_set_numerics(eegfx_ctx* ctx, int numerics) {
  return guarded([&] {
    if (!ctx) fail(EEGFX_EINVAL, "null context");
    if (numerics != EEGFX_EXACT && numerics != EEGFX_FMA)
      fail(EEGFX_EINVAL, "numerics %d", numerics);
    ctx->numerics = numerics;
  });
}

int eegfx_ctx_set_timing(eegfx_ctx* ctx, int enable) {
  return guarded([&] {
    if (!ctx) fail(EEGFX_EINVAL, "null context");
    ctx->activate();
    HIP_CHECK(hipStreamSynchronize(ctx->stream));
    ctx->timing = enable != 0;
    ctx->n_timed = 0;  // events are reused
  });
}

int eegfx_ctx_set_mailbox(eegfx_ctx* ctx, int enable) {
  return guarded([&] {
    if (!ctx) fail(EEGFX_EINVAL, "null context");
    ctx->activate();
    if (!enable) {
      ctx->release_mailbox();
      return;
    }
    if (ctx->mailbox) return;
    // the small-call staging at its largest before any server is launched on it: a server reads
    // the buffers it was launched with, so growing them on a later call stopped and restarted it
    // (with a pinned allocation: the 3-4 ms first calls of tools/mailbox_threads at 16-32 threads)
    (void)ctx->pin_in.get(kZeroCopyBytes);
    (void)ctx->pin_out.get(kZeroCopyOutBytes);
    ctx->mailbox = true;  // the server starts on the first one-epoch call that gets a slot
    (void)ctx->mb_ready();
  });
}

int eegfx_ctx_get_mailbox(eegfx_ctx* ctx, int32_t* enabled, int32_t* resident) {
  return guarded([&] {
    if (!ctx) fail(EEGFX_EINVAL, "null context");
    if (enabled) *enabled = ctx->mailbox ? 1 : 0;
    if (resident) *resident = ctx->mailbox && ctx->mb_slot && ctx->mb_live && ctx->mb_started ? 1 : 0;
  });
}

int eegfx_ctx_synchronize(eegfx_ctx* ctx) {
  return guarded([&] {
    if (!ctx) fail(EEGFX_EINVAL, "null context");
    ctx->activate();
    ctx->drain();
  });
}

int eegfx_ctx_guard_detail(eegfx_ctx* ctx, int64_t* rows_checked, int64_t* rows_rechecked,
                           int64_t* rows_recomputed, int reset) {
  return guarded([&] {
    if (!ctx || !rows_checked || !rows_recomputed) fail(EEGFX_EINVAL, "null argument");
    ctx->activate();
    // the two slot arrays and, right behind them, Guard::adapt (strategy, rechecked offset, rows)
    std::vector<unsigned long long> slots(2 * kGuardSlots * kGuardSlotWords + 3);
    HIP_CHECK(hipMemcpyAsync(slots.data(), ctx->guard_recomputed_slots(),
                             2 * kGuardSlotBytes + 3 * sizeof(unsigned long long),
                             hipMemcpyDeviceToHost, ctx->stream));
    ctx->drain();
    unsigned long long tot[2] = {0, 0};  // recomputed, rechecked
    for (int k = 0; k < 2; ++k)
      for (int i = 0; i < kGuardSlots; ++i) tot[k] += slots[(size_t)(k * kGuardSlots + i) * kGuardSlotWords];
    *rows_checked = ctx->guard_checked;
    *rows_recomputed = (int64_t)tot[0];
    if (rows_rechecked) *rows_rechecked = (int64_t)tot[1];
    if (reset) {
      // the adaptive strategy's offset moves with the cleared total (fused.hip baseline_kernel)
      const unsigned long long off =
          (unsigned long long)((long long)slots[2 * kGuardSlots * kGuardSlotWords + 1] - (long long)tot[1]);
      HIP_CHECK(hipMemsetAsync(ctx->guard_recomputed_slots(), 0, 2 * kGuardSlotBytes, ctx->stream));
      HIP_CHECK(hipMemcpyAsync(ctx->guard_adapt() + 1, &off, sizeof off, hipMemcpyHostToDevice,
                               ctx->stream));
      ctx->drain();
      ctx->guard_checked = 0;
    }
  });
}

int eegfx_ctx_guard_stats(eegfx_ctx* ctx, int64_t* rows_checked, int64_t* rows_recomputed,
                          int reset) {
  return eegfx_ctx_guard_detail(ctx, rows_checked, nullptr, rows_recomputed, reset);
}

int eegfx_ctx_kernel_stats(eegfx_ctx* ctx, int64_t* launches, double* total_ms,
                           int64_t* total_bytes) {
  return guarded([&] {
    if (!ctx || !launches || !total_ms || !total_bytes) fail(EEGFX_EINVAL, "null argument");
    double ms = 0.0;
    int64_t bytes = 0;
    for (size_t i = 0; i < ctx->n_timed; ++i) {
      float t = 0.0f;
      HIP_CHECK(hipEventSynchronize(ctx->events[i].second));
      HIP_CHECK(hipEventElapsedTime(&t, ctx->events[i].first, ctx->events[i].second));
      ms += t;
      bytes += ctx->event_bytes[i];
    }
    *launches = (int64_t)ctx->n_timed;
    *total_ms = ms;
    *total_bytes = bytes;
  });
}

int eegfx_ctx_destroy(eegfx_ctx* ctx) {
  return guarded([&] {
    if (!ctx) return;
    (void)hipSetDevice(ctx->device);
    ctx->release_mailbox();  // before anything that synchronises the whole device
    (void)hipStreamSynchronize(ctx->stream);
    ctx->release_buffers();
    (void)hipStreamSynchronize(ctx->stream);
    (void)hipStreamSynchronize(ctx->own);
    pinned_pool().give(ctx->err_host, ctx->err_cap, hipHostMallocMapped);
    if (ctx->guard_dev) (void)hipFreeAsync(ctx->guard_dev, ctx->own);
    (void)hipStreamSynchronize(ctx->own);
    ctx->release_stream_resources();
    ctx->destroy_events();
    (void)hipStreamDestroy(ctx->own);
    delete ctx;
  });
}

int eegfx_read_raw(eegfx_ctx* ctx, const char* vhdr_path, const char* eeg_path, void* dst,
                   int64_t capacity_bytes, int mem) {
  return guarded([&] {
    if (!vhdr_path || !eeg_path || !dst) fail(EEGFX_EINVAL, "null argument");
    check_mem(mem);
    const Header h = read_header(vhdr_path);
    const int64_t n = recording_frames(h, eeg_path);
    const int64_t bytes = n * h.info.n_channels * sample_bytes(h.info.binary_format);
    if (bytes > capacity_bytes)
      fail(EEGFX_EINVAL, "capacity %lld < %lld bytes", (long long)capacity_bytes, (long long)bytes);
    if (mem == EEGFX_MEM_HOST) {
      read_recording(h, eeg_path, dst, n);
    } else {
      if (!ctx) fail(EEGFX_EINVAL, "device read needs a context");
      ctx->activate();
      std::vector<char> host((size_t)bytes);
      read_recording(h, eeg_path, host.data(), n);
      HIP_CHECK(hipMemcpyAsync(dst, host.data(), (size_t)bytes, hipMemcpyHostToDevice, ctx->stream));
      ctx->drain();
    }
  });
}

}  // extern "C"

// The entries that carry epochs exist for two element types (double[n][C][750], the reference's
// interface, and float[n][C][750], the fp32 values it widens): one implementation each, templated
// on the element type E, behind the extern "C" pairs that follow.
namespace {

// eegfx_cut_epochs_f64 / _f32: E is the element type of epochs_out.
template <typename E>
int cut_epochs_api(eegfx_ctx* ctx, const void* raw, int32_t fmt, int64_t n_frames, int32_t ct,
                   const int32_t* cols, const float* res, int32_t C, const int64_t* pos, int64_t n,
                   E* epochs_out, int mem) {
  return guarded([&] {
    if (!ctx) fail(EEGFX_EINVAL, "null context");
    check_mem(mem);
    if (fmt != EEGFX_INT_16 && fmt != EEGFX_IEEE_FLOAT_32) fail(EEGFX_EINVAL, "format %d", fmt);
    if (n_frames < 0 || n < 0 || ct < 1) fail(EEGFX_EINVAL, "negative size");
    if (n > 0 && (!raw || !pos || !epochs_out)) fail(EEGFX_EINVAL, "null buffer");
    const ChanSel sel = make_sel(cols, res, C, ct);
    if (mem == EEGFX_MEM_HOST) check_positions(pos, n, n_frames);
    if (n == 0) return;
    ctx->activate();
    const size_t raw_bytes = (size_t)n_frames * ct * (fmt == EEGFX_INT_16 ? 2 : 4);
    const size_t out_bytes = sizeof(E) * (size_t)n * C * EEGFX_POSTSTIMULUS;
    const void* d_raw = stage_in(ctx, ctx->raw, raw, raw_bytes, mem);
    const int64_t* d_pos = (const int64_t*)stage_in(ctx, ctx->pos, pos, sizeof(int64_t) * n, mem);
    E* d_out = mem == EEGFX_MEM_DEVICE ? epochs_out : (E*)ctx->out.get(out_bytes);
    ctx->tic();
    HIP_CHECK(launch_cut_epochs(ctx->stream, d_raw, fmt, n_frames, ct, sel, C, d_pos, n, d_out,
                                ctx->fused.get(fused_scratch_bytes(n, C)), ctx->err_dev));
    ctx->toc(0);
    if (mem == EEGFX_MEM_HOST) {
      HIP_CHECK(hipMemcpyAsync(epochs_out, d_out, out_bytes, hipMemcpyDeviceToHost, ctx->stream));
      ctx->drain();
    }
  });
}

// eegfx_extract_features_f64 / _f32: E is the element type of the epochs.  Float epochs take the
// same routes; the rows are those of the double call on the widened epochs, bit for bit.
template <typename E>
int extract_features_api(eegfx_ctx* ctx, const E* epochs, int64_t n, int32_t C, int32_t name,
                         int32_t epoch_size, int32_t skip, int32_t feature_size, double* out,
                         int mem) {
  return guarded([&] {
    if (!ctx) fail(EEGFX_EINVAL, "null context");
    check_mem(mem);
    check_fe_params(C, name, epoch_size, skip, feature_size);
    if (n < 0) fail(EEGFX_EINVAL, "negative count");
    if (n == 0) return;
    if (!epochs || !out) fail(EEGFX_EINVAL, "null buffer");
    ctx->activate();
    const size_t in_bytes = sizeof(E) * (size_t)n * C * EEGFX_POSTSTIMULUS;
    const size_t out_bytes = sizeof(double) * (size_t)n * C * feature_size;
    if (mem == EEGFX_MEM_HOST) {
      // Host epochs (the JNI drop-in, IFeatureExtraction.extractFeatures called once per epoch
      // from Spark map closures, LogisticRegressionClassifier.java:55-61, or serial loops,
      // NeuralNetworkClassifier.java:78-86).  Only the window columns [skip, skip+512) of each row
      // are needed (4,096 of 6,000 bytes; float epochs: 2,048 of 3,000).  row_w: the packed
      // window row of the small-batch staging, doubles for both element types (float windows
      // are widened while they are packed); row_c / row_p: the window and the epoch row as the
      // caller holds them.
      const size_t row_w = sizeof(double) * EEGFX_DWT8_EPOCH_SIZE;
      const size_t row_c = sizeof(E) * EEGFX_DWT8_EPOCH_SIZE;
      const size_t row_p = sizeof(E) * EEGFX_POSTSTIMULUS;
      const uint8_t* src = (const uint8_t*)epochs + sizeof(E) * (size_t)skip;
      if ((size_t)n * C * row_w <= kZeroCopyBytes && features_small_supported(C) &&
          !wide_features(feature_size)) {
        // Small batches (a single epoch above all): latency, not bandwidth.  The window rows are
        // packed into a pinned, device-mapped buffer by the calling thread and the kernel
        // (features_small_kernel) reads them -- and writes the rows -- across the host link
        // directly: one launch and one stream sync, no DMA transfers (each costs a copy-engine
        // round trip) and no allocation once the context's staging has grown.  The rows are EXACT
        // under both numerics (kernels.hip small_epoch), so the fma guard does not count them.
        // a resident server reads the staging it was launched with: stop it before a growth
        // (the next request restarts it on the new buffers)
        if (ctx->mb_live && ((size_t)n * C * row_w > ctx->pin_in.cap || out_bytes > ctx->pin_out.cap))
          ctx->mb_stop();
        double* hin = (double*)ctx->pin_in.get((size_t)n * C * row_w);
        double* hout = (double*)ctx->pin_out.get(out_bytes);
        for (int64_t r = 0; r < n * C; ++r) {
          if constexpr (std::is_same<E, float>::value) {
            const float* w = (const float*)(src + (size_t)r * row_p);
            double* d = hin + (size_t)r * EEGFX_DWT8_EPOCH_SIZE;
            for (int k = 0; k < EEGFX_DWT8_EPOCH_SIZE; ++k) d[k] = (double)w[k];
          } else {
            memcpy((uint8_t*)hin + (size_t)r * row_w, src + (size_t)r * row_p, row_w);
          }
        }
        // The resident server (no launch, no stream sync) takes single epochs: it serves a
        // request's epochs one after another (~7 us each), where a launch runs them on a
        // workgroup each (11 epochs: ~20 us launched against ~80 us served).
        if (n == 1 && ctx->mb_ready()) {
          ctx->mb_serve(n, C, feature_size);
          ctx->check_positions_flag();  // as every synchronising call (the launch path below)
          memcpy(out, hout, out_bytes);
          return;
        }
        SmallCallGate gate(ctx->device);
        ctx->tic();
        HIP_CHECK(launch_features_small(ctx->stream, (const double*)ctx->pin_in.device_ptr(), n, C,
                                        feature_size, (double*)ctx->pin_out.device_ptr()));
        ctx->toc(0);
        ctx->wait_small();
        ctx->check_positions_flag();
        memcpy(out, hout, out_bytes);
        return;
      }
      // Large batches: strided 2D copies of the window columns in chunks, each followed by its
      // kernels on the same stream (the kernels are ~3 % of a chunk's copy).  Measured with 100k
      // epochs: 4.2e6 epochs/s against 3.0e6 for copying the whole 18 KB epochs and a 4.6e6
      // host-link bound; packing the rows with host threads into pinned staging first was slower
      // (2.8e6).
      constexpr int64_t kChunk = 8192;  // epochs per chunk
      const size_t chunk_bytes = (size_t)std::min<int64_t>(n, kChunk) * C * row_c;
      uint8_t* dwin = (uint8_t*)ctx->scratch.get(chunk_bytes);
      double* d_out = (double*)ctx->out.get(out_bytes);
      const bool wide = wide_features(feature_size);
      const Guard g = wide ? Guard{nullptr, nullptr, nullptr} : ctx->guard_for(n);
      ctx->tic();
      for (int64_t e0 = 0; e0 < n; e0 += kChunk) {
        const int64_t m = std::min<int64_t>(kChunk, n - e0);
        HIP_CHECK(hipMemcpy2DAsync(dwin, row_c, src + (size_t)e0 * C * row_p, row_p, row_c,
                                   (size_t)(m * C), hipMemcpyHostToDevice, ctx->stream));
        double* rows = d_out + e0 * C * feature_size;
        if (wide)
          HIP_CHECK(launch_pyramid_from_epochs(ctx->stream, (const E*)dwin, m, C, 0,
                                               feature_size, rows, EEGFX_DWT8_EPOCH_SIZE));
        else
          HIP_CHECK(launch_features_from_epochs(ctx->stream, (const E*)dwin, m, C, 0,
                                                feature_size, ctx->numerics != EEGFX_EXACT, rows,
                                                EEGFX_DWT8_EPOCH_SIZE, g));
      }
      ctx->toc(0);
      HIP_CHECK(hipMemcpyAsync(out, d_out, out_bytes, hipMemcpyDeviceToHost, ctx->stream));
      ctx->drain();
      return;
    }
    const E* d_in = (const E*)stage_in(ctx, ctx->scratch, epochs, in_bytes, mem);
    double* d_out = mem == EEGFX_MEM_DEVICE ? out : (double*)ctx->out.get(out_bytes);
    if (wide_features(feature_size)) {
      ctx->tic();
      HIP_CHECK(launch_pyramid_from_epochs(ctx->stream, d_in, n, C, skip, feature_size, d_out,
                                           EEGFX_POSTSTIMULUS));
      ctx->toc(0);
    } else {
      const Guard g = ctx->guard_for(n);
      ctx->tic();
      HIP_CHECK(launch_features_from_epochs(ctx->stream, d_in, n, C, skip, feature_size,
                                            ctx->numerics != EEGFX_EXACT, d_out,
                                            EEGFX_POSTSTIMULUS, g));
      ctx->toc(0);
    }
    if (mem == EEGFX_MEM_HOST) {
      HIP_CHECK(hipMemcpyAsync(out, d_out, out_bytes, hipMemcpyDeviceToHost, ctx->stream));
      ctx->drain();
    }
  });
}

// eegfx_process_recording_epochs / _f32 with epochs_out != NULL.
template <typename E>
int process_recording_epochs_api(eegfx_ctx* ctx, const void* raw, int32_t fmt, int64_t n_frames,
                                 int32_t ct, const int32_t* cols, const float* res, int32_t C,
                                 const int64_t* pos, int64_t n, double* features, E* epochs_out,
                                 int mem) {
  return guarded([&] {
    if (!ctx) fail(EEGFX_EINVAL, "null context");
    check_mem(mem);
    if (fmt != EEGFX_INT_16 && fmt != EEGFX_IEEE_FLOAT_32) fail(EEGFX_EINVAL, "format %d", fmt);
    if (n_frames < 0 || n < 0 || ct < 1) fail(EEGFX_EINVAL, "negative size");
    if (n > 0 && (!raw || !pos || !features)) fail(EEGFX_EINVAL, "null buffer");
    const ChanSel sel = make_sel(cols, res, C, ct);
    if (mem == EEGFX_MEM_HOST) check_positions(pos, n, n_frames);
    if (n == 0) return;
    ctx->activate();
    const size_t raw_bytes = (size_t)n_frames * ct * (fmt == EEGFX_INT_16 ? 2 : 4);
    const size_t ep_bytes = sizeof(E) * (size_t)n * C * EEGFX_POSTSTIMULUS;
    const size_t f_bytes = sizeof(double) * (size_t)n * C * EEGFX_DWT8_FEATURE_SIZE;
    const void* d_raw = stage_in(ctx, ctx->raw, raw, raw_bytes, mem);
    const int64_t* d_pos = (const int64_t*)stage_in(ctx, ctx->pos, pos, sizeof(int64_t) * n, mem);
    E* d_ep = mem == EEGFX_MEM_DEVICE ? epochs_out : (E*)ctx->scratch.get(ep_bytes);
    double* d_f = mem == EEGFX_MEM_DEVICE ? features : (double*)ctx->out.get(f_bytes);
    run_epochs_and_features(ctx, d_raw, fmt, n_frames, ct, sel, C, d_pos, n, d_ep, d_f);
    if (mem == EEGFX_MEM_HOST) {
      HIP_CHECK(hipMemcpyAsync(epochs_out, d_ep, ep_bytes, hipMemcpyDeviceToHost, ctx->stream));
      HIP_CHECK(hipMemcpyAsync(features, d_f, f_bytes, hipMemcpyDeviceToHost, ctx->stream));
      ctx->drain();
    }
  });
}

}  // namespace

extern "C" {

int eegfx_cut_epochs_f64(eegfx_ctx* ctx, const void* raw, int32_t fmt, int64_t n_frames,
                         int32_t ct, const int32_t* cols, const float* res, int32_t C,
                         const int64_t* pos, int64_t n, double* epochs_out, int mem) {
  return cut_epochs_api(ctx, raw, fmt, n_frames, ct, cols, res, C, pos, n, epochs_out, mem);
}

int eegfx_cut_epochs_f32(eegfx_ctx* ctx, const void* raw, int32_t fmt, int64_t n_frames,
                         int32_t ct, const int32_t* cols, const float* res, int32_t C,
                         const int64_t* pos, int64_t n, float* epochs_out, int mem) {
  return cut_epochs_api(ctx, raw, fmt, n_frames, ct, cols, res, C, pos, n, epochs_out, mem);
}

int eegfx_extract_features_f64(eegfx_ctx* ctx, const double* epochs, int64_t n, int32_t C,
                               int32_t name, int32_t epoch_size, int32_t skip,
                               int32_t feature_size, double* out, int mem) {
  return extract_features_api(ctx, epochs, n, C, name, epoch_size, skip, feature_size, out, mem);
}

int eegfx_extract_features_f32(eegfx_ctx* ctx, const float* epochs, int64_t n, int32_t C,
                               int32_t name, int32_t epoch_size, int32_t skip,
                               int32_t feature_size, double* out, int mem) {
  return extract_features_api(ctx, epochs, n, C, name, epoch_size, skip, feature_size, out, mem);
}

int eegfx_process_recording(eegfx_ctx* ctx, const void* raw, int32_t fmt, int64_t n_frames,
                            int32_t ct, const int32_t* cols, const float* res, int32_t C,
                            const int64_t* pos, int64_t n, double* features, int mem) {
  return guarded([&] {
    if (!ctx) fail(EEGFX_EINVAL, "null context");
    check_mem(mem);
    if (fmt != EEGFX_INT_16 && fmt != EEGFX_IEEE_FLOAT_32) fail(EEGFX_EINVAL, "format %d", fmt);
    if (n_frames < 0 || n < 0 || ct < 1) fail(EEGFX_EINVAL, "negative size");
    if (n > 0 && (!raw || !pos || !features)) fail(EEGFX_EINVAL, "null buffer");
    const ChanSel sel = make_sel(cols, res, C, ct);
    if (mem == EEGFX_MEM_HOST) check_positions(pos, n, n_frames);
    if (n == 0) return;
    ctx->activate();
    const size_t raw_bytes = (size_t)n_frames * ct * (fmt == EEGFX_INT_16 ? 2 : 4);
    const size_t out_bytes = sizeof(double) * (size_t)n * C * EEGFX_DWT8_FEATURE_SIZE;
    const void* d_raw = stage_in(ctx, ctx->raw, raw, raw_bytes, mem);
    const int64_t* d_pos = (const int64_t*)stage_in(ctx, ctx->pos, pos, sizeof(int64_t) * n, mem);
    double* d_out = mem == EEGFX_MEM_DEVICE ? features : (double*)ctx->out.get(out_bytes);
    run_features_from_raw(ctx, d_raw, fmt, n_frames, ct, sel, C, d_pos, n, d_out);
    if (mem == EEGFX_MEM_HOST) {
      HIP_CHECK(hipMemcpyAsync(features, d_out, out_bytes, hipMemcpyDeviceToHost, ctx->stream));
      ctx->drain();
    }
  });
}

int eegfx_process_recording_fe(eegfx_ctx* ctx, const void* raw, int32_t fmt, int64_t n_frames,
                               int32_t ct, const int32_t* cols, const float* res, int32_t C,
                               const int64_t* pos, int64_t n, int32_t name, int32_t epoch_size,
                               int32_t skip, int32_t feature_size, double* features, int mem) {
  if (name == EEGFX_DWT8_NAME && epoch_size == EEGFX_DWT8_EPOCH_SIZE && skip == EEGFX_DWT8_SKIP &&
      feature_size == EEGFX_DWT8_FEATURE_SIZE)
    return eegfx_process_recording(ctx, raw, fmt, n_frames, ct, cols, res, C, pos, n, features,
                                   mem);
  return guarded([&] {
    if (!ctx) fail(EEGFX_EINVAL, "null context");
    check_mem(mem);
    if (fmt != EEGFX_INT_16 && fmt != EEGFX_IEEE_FLOAT_32) fail(EEGFX_EINVAL, "format %d", fmt);
    if (n_frames < 0 || n < 0 || ct < 1) fail(EEGFX_EINVAL, "negative size");
    if (n > 0 && (!raw || !pos || !features)) fail(EEGFX_EINVAL, "null buffer");
    const ChanSel sel = make_sel(cols, res, C, ct);
    check_fe_params(C, name, epoch_size, skip, feature_size);
    if (mem == EEGFX_MEM_HOST) check_positions(pos, n, n_frames);
    if (n == 0) return;
    ctx->activate();
    const size_t raw_bytes = (size_t)n_frames * ct * (fmt == EEGFX_INT_16 ? 2 : 4);
    const size_t out_bytes = sizeof(double) * (size_t)n * C * feature_size;
    const void* d_raw = stage_in(ctx, ctx->raw, raw, raw_bytes, mem);
    const int64_t* d_pos = (const int64_t*)stage_in(ctx, ctx->pos, pos, sizeof(int64_t) * n, mem);
    double* d_out = mem == EEGFX_MEM_DEVICE ? features : (double*)ctx->out.get(out_bytes);
    // The two passes: the epochs into scratch memory, then the rows from them.  (A fused raw ->
    // rows pyramid kernel measured slower than this at feature size 512: DESIGN.md 5.4.1.)
    // The scratch epochs are float32: the fp32 samples as the cut holds them (3,000 C bytes per
    // epoch), widened again by the kernels that read them -- the rows are those of double scratch.
    float* ep = (float*)ctx->scratch.get(sizeof(float) * (size_t)n * C * EEGFX_POSTSTIMULUS);
    ctx->tic();
    HIP_CHECK(launch_cut_epochs(ctx->stream, d_raw, fmt, n_frames, ct, sel, C, d_pos, n, ep,
                                ctx->fused.get(fused_scratch_bytes(n, C)), ctx->err_dev));
    if (wide_features(feature_size)) {
      HIP_CHECK(launch_pyramid_from_epochs(ctx->stream, ep, n, C, skip, feature_size, d_out,
                                           EEGFX_POSTSTIMULUS));
    } else {
      const Guard g = ctx->guard_for(n);
      HIP_CHECK(launch_features_from_epochs(ctx->stream, ep, n, C, skip, feature_size,
                                            ctx->numerics != EEGFX_EXACT, d_out,
                                            EEGFX_POSTSTIMULUS, g));
    }
    ctx->toc(0);
    if (mem == EEGFX_MEM_HOST) {
      HIP_CHECK(hipMemcpyAsync(features, d_out, out_bytes, hipMemcpyDeviceToHost, ctx->stream));
      ctx->drain();
    }
  });
}

int eegfx_process_recording_epochs(eegfx_ctx* ctx, const void* raw, int32_t fmt, int64_t n_frames,
                                   int32_t ct, const int32_t* cols, const float* res, int32_t C,
                                   const int64_t* pos, int64_t n, double* features,
                                   double* epochs_out, int mem) {
  if (!epochs_out)
    return eegfx_process_recording(ctx, raw, fmt, n_frames, ct, cols, res, C, pos, n, features,
                                   mem);
  return process_recording_epochs_api(ctx, raw, fmt, n_frames, ct, cols, res, C, pos, n, features,
                                      epochs_out, mem);
}

int eegfx_process_recording_epochs_f32(eegfx_ctx* ctx, const void* raw, int32_t fmt,
                                       int64_t n_frames, int32_t ct, const int32_t* cols,
                                       const float* res, int32_t C, const int64_t* pos, int64_t n,
                                       double* features, float* epochs_out, int mem) {
  if (!epochs_out)
    return eegfx_process_recording(ctx, raw, fmt, n_frames, ct, cols, res, C, pos, n, features,
                                   mem);
  return process_recording_epochs_api(ctx, raw, fmt, n_frames, ct, cols, res, C, pos, n, features,
                                      epochs_out, mem);
}

// Config 5 (BASELINE.json configs[4]): a long recording in host memory, streamed to the device in
// chunks of `chunk_frames` frames.  Epochs are taken in position order; a chunk starts at the
// first unprocessed epoch's baseline frame (pos - 100) and holds every following epoch whose
// frames [pos-100, pos+687) fit (or reach past the recording end, which the kernels zero-pad), so
// consecutive chunks overlap by at most one epoch span (787 frames) -- the halo.  A ring of four
// device chunk buffers and an upload stream let the H2D run up to three chunks ahead of the
// kernels, and each chunk's rows leave on a download stream as soon as its kernels finish (the
// host link runs both directions at once; with two buffers the event hops between streams
// stalled the uploads).  A pageable source is first copied into one of two pinned staging
// buffers by host threads (that copy overlaps the device work), a pinned source (hipHostMalloc /
// registered) is copied directly.
int eegfx_process_recording_streamed(eegfx_ctx* ctx, const void* raw, int32_t fmt,
                                     int64_t n_frames, int32_t ct, const int32_t* cols,
                                     const float* res, int32_t C, const int64_t* pos, int64_t n,
                                     double* features, int64_t chunk_frames) {
  return guarded([&] {
    if (!ctx) fail(EEGFX_EINVAL, "null context");
    if (fmt != EEGFX_INT_16 && fmt != EEGFX_IEEE_FLOAT_32) fail(EEGFX_EINVAL, "format %d", fmt);
    if (n_frames < 0 || n < 0 || ct < 1) fail(EEGFX_EINVAL, "negative size");
    if (n > 0 && (!raw || !pos || !features)) fail(EEGFX_EINVAL, "null buffer");
    constexpr int64_t kSpan = EEGFX_PRESTIMULUS + EEGFX_DWT8_SKIP + EEGFX_DWT8_EPOCH_SIZE;  // 787
    if (chunk_frames < kSpan)
      fail(EEGFX_EINVAL, "chunk_frames %lld < one epoch span (%lld)", (long long)chunk_frames,
           (long long)kSpan);
    const ChanSel sel = make_sel(cols, res, C, ct);
    check_positions(pos, n, n_frames);
    if (n == 0) return;
    ctx->activate();
    const int64_t FB = (int64_t)ct * (fmt == EEGFX_INT_16 ? 2 : 4);
    const int64_t F = (int64_t)C * EEGFX_DWT8_FEATURE_SIZE;
    // positions in order (the usual .vmrk case) are used as they are; otherwise the epochs are
    // processed in position order and the rows are put back at the end
    const bool in_order = std::is_sorted(pos, pos + n);
    std::vector<int64_t> order, sorted_pos;
    const int64_t* spos = pos;
    if (!in_order) {
      order.resize((size_t)n);
      for (int64_t i = 0; i < n; ++i) order[(size_t)i] = i;
      std::stable_sort(order.begin(), order.end(),
                       [&](int64_t a, int64_t b) { return pos[a] < pos[b]; });
      sorted_pos.resize((size_t)n);
      for (int64_t i = 0; i < n; ++i) sorted_pos[(size_t)i] = pos[order[(size_t)i]];
      spos = sorted_pos.data();
    }
    // The positions go up front on the context stream.  Measured slower (profiles/r06/): the
    // kernels writing the rows straight into a pinned caller buffer instead of a download per
    // chunk (8.84 against 7.2 ms per configs[4] step); a pageable position copy per chunk on the
    // upload stream (9.5 ms: each one blocks the host behind every earlier upload); one position
    // copy on the context stream behind the first chunk's frames (7.44-7.48 against 7.13-7.16);
    // each pinned chunk as two halves on two upload streams (7.75-7.81 against 7.14).
    int64_t* d_pos = (int64_t*)ctx->pos.get(sizeof(int64_t) * (size_t)n);
    HIP_CHECK(hipMemcpyAsync(d_pos, spos, sizeof(int64_t) * (size_t)n, hipMemcpyHostToDevice,
                             ctx->stream));
    double* d_out = (double*)ctx->out.get(sizeof(double) * (size_t)(n * F));
    (void)ctx->fused.get(fused_scratch_bytes(n, C));  // every chunk's baselines fit: no realloc
    // chunk buffers: 64 B front pad (the kernels round the first quad down by < 16 B) + data
    // (rounded to 256 B so the second buffer is as aligned as the first: the kernels read
    // 16-byte quads relative to `raw`)
    const size_t cbytes = ((size_t)(chunk_frames * FB) + 128 + 255) & ~(size_t)255;
    // Chunk sizes ramp up (c/4, c/2, then c) and down (about half of what remains, not below
    // c/4) so that the first upload and the last download -- the parts of a call that nothing
    // overlaps -- stay short.
    const int64_t last = spos[n - 1] - EEGFX_PRESTIMULUS + kSpan;
    auto chunk_at = [&](int64_t k, int64_t lo) {
      int64_t c = k < 2 ? chunk_frames >> (2 - k) : chunk_frames;
      const int64_t rest = last - lo;
      if (rest < 2 * chunk_frames) c = std::min(c, (rest + 1) / 2);
      return std::min(chunk_frames, std::max(c, std::max(chunk_frames / 4, 2 * kSpan)));
    };
    struct Chunk {
      int64_t i, j, lo, hi;  // epochs [i, j), frames [lo, hi)
    };
    std::vector<Chunk> plan;
    for (int64_t i = 0; i < n;) {
      const int64_t lo = spos[i] - EEGFX_PRESTIMULUS;
      const int64_t hi = std::min(lo + chunk_at((int64_t)plan.size(), lo), n_frames);
      // the epochs whose span [pos-100, pos+687) ends by hi (all of them at the recording end):
      // a prefix of the sorted positions, found by bisection (a linear scan of configs[4]'s 576k
      // positions delayed the first upload by ~150 us)
      const int64_t j =
          hi == n_frames ? n
                         : std::upper_bound(spos + i, spos + n, hi + EEGFX_PRESTIMULUS - kSpan) - spos;
      plan.push_back({i, j, lo, hi});
      i = j;
    }
    // A ring of 4 device chunk buffers (fewer for fewer chunks).  One buffer per chunk (the whole
    // 346 MB recording in HBM, no upload ever waiting for an earlier chunk's kernels) measured the
    // same: 7.16-7.18 against 7.13-7.18 ms (profiles/r06/stream_ring_ab.log).
    const size_t R = std::min<size_t>(plan.size(), 4);
    uint8_t* dbuf = (uint8_t*)ctx->raw.get(R * cbytes);
    hipPointerAttribute_t attr;
    const bool pinned = hipPointerGetAttributes(&attr, raw) == hipSuccess &&
                        attr.type == hipMemoryTypeHost;
    (void)hipGetLastError();  // a pageable pointer can leave an error behind
    void* pin[2] = {nullptr, nullptr};
    ctx->stream_resources(std::max<size_t>(R, 2));
    hipStream_t cs = ctx->up, os = ctx->down;  // upload (H2D) and download (D2H) streams
    hipEvent_t* copied = ctx->copied.data();
    hipEvent_t* done = ctx->done.data();
    try {
      if (!pinned) {  // the context's grow-only staging (pinned_pool: growing it syncs nothing)
        for (int b = 0; b < 2; ++b) pin[b] = ctx->pin_chunk[b].get(cbytes);
      }
      ctx->drain();  // d_pos uploaded; buffers idle
      for (size_t k = 0; k < plan.size(); ++k) {
        const size_t b = k % R;
        const int64_t i = plan[k].i, j = plan[k].j, lo = plan[k].lo, hi = plan[k].hi;
        const int64_t Lb = (lo * FB) & ~(int64_t)15, Hb = hi * FB;
        const size_t bytes = Hb > Lb ? (size_t)(Hb - Lb) : 0;
        uint8_t* dst = dbuf + (size_t)b * cbytes + 64;
        if (k >= R) HIP_CHECK(hipStreamWaitEvent(cs, done[b], 0));  // kernels of chunk k-R done
        const uint8_t* src = (const uint8_t*)raw + Lb;
        if (!pinned) {  // two pinned staging buffers: staging k&1 is free once chunk k-2 uploaded
          if (k >= 2) HIP_CHECK(hipEventSynchronize(copied[(k - 2) % R]));
          if (bytes) parallel_memcpy(pin[k & 1], src, bytes);
          src = (const uint8_t*)pin[k & 1];
        }
        if (bytes) HIP_CHECK(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, cs));
        HIP_CHECK(hipEventRecord(copied[b], cs));
        HIP_CHECK(hipStreamWaitEvent(ctx->stream, copied[b], 0));
        // frame f of the recording lives at raw_dev + f*FB for lo <= f < hi (pointer arithmetic
        // only: nothing below dst is ever read)
        const uint8_t* raw_dev = dst - Lb;
        run_features_from_raw(ctx, raw_dev, fmt, hi, ct, sel, C, d_pos + i, j - i,
                              d_out + i * F);
        HIP_CHECK(hipEventRecord(done[b], ctx->stream));
        if (in_order) {  // rows of this chunk go straight to the caller on the download stream
          HIP_CHECK(hipStreamWaitEvent(os, done[b], 0));
          HIP_CHECK(hipMemcpyAsync(features + i * F, d_out + i * F,
                                   sizeof(double) * (size_t)((j - i) * F), hipMemcpyDeviceToHost,
                                   os));
        }
      }
      if (in_order) {
        HIP_CHECK(hipStreamSynchronize(os));
      } else {
        std::vector<double> sorted((size_t)(n * F));
        HIP_CHECK(hipMemcpyAsync(sorted.data(), d_out, sizeof(double) * sorted.size(),
                                 hipMemcpyDeviceToHost, ctx->stream));
        ctx->drain();
        for (int64_t r = 0; r < n; ++r)
          memcpy(features + order[(size_t)r] * F, sorted.data() + r * F,
                 sizeof(double) * (size_t)F);
      }
      HIP_CHECK(hipStreamSynchronize(cs));
      ctx->drain();
    } catch (...) {
      (void)hipStreamSynchronize(ctx->stream);
      if (cs) (void)hipStreamSynchronize(cs);
      if (os) (void)hipStreamSynchronize(os);
      throw;
    }
  });
}

// the classifier of LogisticRegressionClassifier.java:85-114 on the GPU
// (csrc/logreg.hip): MLlib 1.6.2 LogisticRegressionWithSGD.  miniBatchFraction < 1: iteration i
// trains on data.sample(false, f, 42 + i) of the rows in `num_partitions` ParallelCollectionRDD
// slices (spark_sample.h), drawn on the host (threads over iterations) as one bit mask per
// iteration and uploaded before the iterations that read them.  The hinge loop of
// eegfx_ext.h (SVMWithSGD) stays full-batch (outside the contract, not extended).
static int glm_sgd_train(int grad, eegfx_ctx* ctx, const double* X, const double* y, int64_t n,
                         int32_t d, int32_t num_iterations, double step_size, double reg_param,
                         double mini_batch_fraction, double convergence_tol,
                         int32_t num_partitions, double* weights, int32_t* iterations_run,
                         int mem) {
  return guarded([&] {
    if (!ctx || !weights) fail(EEGFX_EINVAL, "null argument");
    check_mem(mem);
    if (n < 1) fail(EEGFX_EINVAL, "empty training set");  // GeneralizedLinearAlgorithm: first()
    if (!X || !y) fail(EEGFX_EINVAL, "null X / y");
    if (d < 1 || d > kLrMaxFeatures) fail(EEGFX_EINVAL, "d=%d outside [1, %d]", d, kLrMaxFeatures);
    if (num_iterations < 0) fail(EEGFX_EINVAL, "num_iterations %d", num_iterations);
    // RDD.sample's require(fraction >= 0.0), then BernoulliSampler's upper bound 1 up to
    // RandomSampler.roundingEpsilon
    if (!(mini_batch_fraction >= 0.0))
      fail(EEGFX_EINVAL, "Negative fraction value: %g", mini_batch_fraction);
    if (!(mini_batch_fraction <= 1.0 + 1e-6))
      fail(EEGFX_EINVAL, "Sampling fraction (%g) must be on interval [0, 1]", mini_batch_fraction);
    const bool sampled = mini_batch_fraction < 1.0;
    if (sampled && grad != kGradLogistic)
      fail(EEGFX_ENOTSUP, "miniBatchFraction %g: the SVM loop is full-batch only",
           mini_batch_fraction);
    if (sampled && num_partitions < 1) fail(EEGFX_EINVAL, "num_partitions %d", num_partitions);
    ctx->activate();
    const double* dX = X;
    const double* dy = y;
    if (mem == EEGFX_MEM_HOST) {
      double* bx = (double*)ctx->lr_x.get(sizeof(double) * (size_t)(n * d));
      double* by = (double*)ctx->lr_y.get(sizeof(double) * (size_t)n);
      HIP_CHECK(hipMemcpyAsync(bx, X, sizeof(double) * (size_t)(n * d), hipMemcpyHostToDevice,
                               ctx->stream));
      HIP_CHECK(hipMemcpyAsync(by, y, sizeof(double) * (size_t)n, hipMemcpyHostToDevice,
                               ctx->stream));
      dX = bx;
      dy = by;
    }
    const size_t sbytes = sizeof(LrState) + sizeof(double) * (size_t)d;
    std::vector<uint8_t> hs(sbytes, 0);
    LrState* h = (LrState*)hs.data();
    h->converged = num_iterations == 0 ? 1 : 0;
    memcpy(h->w, weights, sizeof(double) * (size_t)d);  // initial weights (zeros in MLlib)
    LrState* st = (LrState*)ctx->lr_state.get(sbytes);
    HIP_CHECK(hipMemcpyAsync(st, hs.data(), sbytes, hipMemcpyHostToDevice, ctx->stream));
    HIP_CHECK(launch_lr_validate(ctx->stream, dy, n, st));
    const int G = lr_grid(n);
    double* part = (double*)ctx->lr_part.get(sizeof(double) * (size_t)G * d);
    if (!sampled) {
      for (int i = 0; i < num_iterations; ++i)
        HIP_CHECK(launch_lr_iteration(ctx->stream, grad, dX, dy, n, d, nullptr, n, st, part, G,
                                      step_size, reg_param, convergence_tol, num_iterations));
    } else {
      // the masks of up to ~256 MB of iterations at a time, drawn by threads over iterations
      const int64_t words = (n + 31) / 32;
      const int chunk = (int)std::max<int64_t>(
          1, std::min<int64_t>(num_iterations, ((int64_t)64 << 20) / words));
      std::vector<uint32_t> masks((size_t)(chunk * words));
      std::vector<int64_t> counts((size_t)chunk);
      uint32_t* dmask = (uint32_t*)ctx->lr_mask.get(sizeof(uint32_t) * masks.size());
      const int T_max = std::min(64, available_processors());
      for (int i0 = 0; i0 < num_iterations; i0 += chunk) {
        const int k = std::min(chunk, num_iterations - i0);
        ctx->drain();  // the previous chunk's upload and iterations are done with both buffers
        if (i0 > 0) {  // converged (or stopped): the remaining iterations would be skipped
          int32_t conv = 0;
          HIP_CHECK(hipMemcpyAsync(&conv, &st->converged, sizeof(conv), hipMemcpyDeviceToHost,
                                   ctx->stream));
          HIP_CHECK(hipStreamSynchronize(ctx->stream));
          if (conv != 0) break;
        }
        const int T = std::max(1, std::min(k, T_max));
        {
          Joiner pool;
          for (int t = 0; t < T; ++t)
            pool.th.emplace_back([&, t] {
              for (int j = t; j < k; j += T)  // GradientDescent's i = i0 + j + 1, seed 42 + i
                counts[j] = spark::sample_mask(n, mini_batch_fraction, num_partitions,
                                               42 + (int64_t)(i0 + j + 1),
                                               &masks[(size_t)j * words]);
            });
        }
        HIP_CHECK(hipMemcpyAsync(dmask, masks.data(), sizeof(uint32_t) * (size_t)(k * words),
                                 hipMemcpyHostToDevice, ctx->stream));
        for (int j = 0; j < k; ++j)
          HIP_CHECK(launch_lr_iteration(ctx->stream, grad, dX, dy, n, d, dmask + (size_t)j * words,
                                        counts[j], st, part, G, step_size, reg_param,
                                        convergence_tol, num_iterations));
      }
    }
    HIP_CHECK(hipMemcpyAsync(hs.data(), st, sbytes, hipMemcpyDeviceToHost, ctx->stream));
    ctx->drain();
    if (h->converged == 2) fail(EEGFX_EINVAL, "Input validation failed: labels must be 0.0 or 1.0");
    memcpy(weights, h->w, sizeof(double) * (size_t)d);
    if (iterations_run) *iterations_run = h->iter;
  });
}

static int glm_predict(int grad, eegfx_ctx* ctx, const double* X, int64_t n, int32_t d,
                       const double* weights, double intercept, double threshold, double* out,
                       int mem) {
  return guarded([&] {
    if (!ctx || !weights) fail(EEGFX_EINVAL, "null argument");
    check_mem(mem);
    if (n < 0 || d < 1 || d > kLrMaxFeatures) fail(EEGFX_EINVAL, "n=%lld d=%d", (long long)n, d);
    if (n == 0) return;
    if (!X || !out) fail(EEGFX_EINVAL, "null X / out");
    ctx->activate();
    const double* dX = X;
    double* dout = out;
    if (mem == EEGFX_MEM_HOST) {
      double* bx = (double*)ctx->lr_x.get(sizeof(double) * (size_t)(n * d));
      HIP_CHECK(hipMemcpyAsync(bx, X, sizeof(double) * (size_t)(n * d), hipMemcpyHostToDevice,
                               ctx->stream));
      dX = bx;
      dout = (double*)ctx->lr_y.get(sizeof(double) * (size_t)n);
    }
    const size_t sbytes = sizeof(LrState) + sizeof(double) * (size_t)d;
    LrState* st = (LrState*)ctx->lr_state.get(sbytes);
    HIP_CHECK(hipMemcpyAsync(st->w, weights, sizeof(double) * (size_t)d, hipMemcpyHostToDevice,
                             ctx->stream));
    const bool use_t = !std::isnan(threshold);  // clearThreshold -> scores / margins
    HIP_CHECK(launch_lr_predict(ctx->stream, grad, dX, n, d, st->w, intercept, threshold,
                                use_t ? 1 : 0, dout));
    if (mem == EEGFX_MEM_HOST)
      HIP_CHECK(hipMemcpyAsync(out, dout, sizeof(double) * (size_t)n, hipMemcpyDeviceToHost,
                               ctx->stream));
    ctx->drain();
  });
}

int eegfx_logreg_sgd_train_partitioned(eegfx_ctx* ctx, const double* X, const double* y,
                                       int64_t n, int32_t d, int32_t num_iterations,
                                       double step_size, double reg_param,
                                       double mini_batch_fraction, double convergence_tol,
                                       int32_t num_partitions, double* weights,
                                       int32_t* iterations_run, int mem) {
  return glm_sgd_train(kGradLogistic, ctx, X, y, n, d, num_iterations, step_size, reg_param,
                       mini_batch_fraction, convergence_tol, num_partitions, weights,
                       iterations_run, mem);
}

int eegfx_logreg_sgd_train(eegfx_ctx* ctx, const double* X, const double* y, int64_t n, int32_t d,
                           int32_t num_iterations, double step_size, double reg_param,
                           double mini_batch_fraction, double convergence_tol, double* weights,
                           int32_t* iterations_run, int mem) {
  // Spark local[*] (SparkInitializer.java:44): defaultParallelism = the processors available
  // to the process (Runtime.availableProcessors(): affinity and cgroup quota honoured)
  const int32_t parts = (int32_t)available_processors();
  return glm_sgd_train(kGradLogistic, ctx, X, y, n, d, num_iterations, step_size, reg_param,
                       mini_batch_fraction, convergence_tol, parts, weights, iterations_run, mem);
}

int eegfx_spark_sample(int64_t n, double fraction, int32_t num_partitions, int64_t seed,
                       uint32_t* mask, int64_t* kept) {
  return guarded([&] {
    if (n < 0 || num_partitions < 1 || !mask || !kept) fail(EEGFX_EINVAL, "bad argument");
    if (!(fraction >= -1e-6 && fraction <= 1.0 + 1e-6))
      fail(EEGFX_EINVAL, "Sampling fraction (%g) must be on interval [0, 1]", fraction);
    *kept = spark::sample_mask(n, fraction, num_partitions, seed, mask);
  });
}

int eegfx_logreg_predict(eegfx_ctx* ctx, const double* X, int64_t n, int32_t d,
                         const double* weights, double intercept, double threshold, double* out,
                         int mem) {
  return glm_predict(kGradLogistic, ctx, X, n, d, weights, intercept, threshold, out, mem);
}

// The classifier of SVMClassifier.java:83-111 (MLlib 1.6.2 SVMWithSGD: HingeGradient, the same
// SquaredL2Updater / GradientDescent loop) and SVMModel.predict (:71, :114-137).
int eegfx_svm_sgd_train(eegfx_ctx* ctx, const double* X, const double* y, int64_t n, int32_t d,
                        int32_t num_iterations, double step_size, double reg_param,
                        double mini_batch_fraction, double convergence_tol, double* weights,
                        int32_t* iterations_run, int mem) {
  return glm_sgd_train(kGradHinge, ctx, X, y, n, d, num_iterations, step_size, reg_param,
                       mini_batch_fraction, convergence_tol, 1, weights, iterations_run, mem);
}

int eegfx_svm_predict(eegfx_ctx* ctx, const double* X, int64_t n, int32_t d, const double* weights,
                      double intercept, double threshold, double* out, int mem) {
  return glm_predict(kGradHinge, ctx, X, n, d, weights, intercept, threshold, out, mem);
}

int eegfx_plan_markers_device(eegfx_ctx* ctx, const int64_t* positions,
                              const int32_t* stimulus_index, int64_t n_markers, int64_t n_frames,
                              int32_t guessed, int64_t* balance, int64_t* pos_out,
                              double* label_out, int64_t* n_selected, int mem) {
  return guarded([&] {
    if (!ctx || !balance || !n_selected) fail(EEGFX_EINVAL, "null argument");
    check_mem(mem);
    if (n_markers < 0) fail(EEGFX_EINVAL, "negative marker count");
    if (*balance < -1 || *balance > 1)
      fail(EEGFX_EINVAL, "balance %lld outside {-1, 0, 1}", (long long)*balance);
    *n_selected = 0;
    if (n_markers == 0) return;
    if (!positions || !stimulus_index) fail(EEGFX_EINVAL, "null markers");
    ctx->activate();
    const int64_t n = n_markers;
    const int64_t* d_pos = (const int64_t*)stage_in(ctx, ctx->pos, positions, sizeof(int64_t) * n,
                                                    mem);
    const int32_t* d_stim = (const int32_t*)stage_in(ctx, ctx->lr_y, stimulus_index,
                                                     sizeof(int32_t) * n, mem);
    int64_t* d_pos_out = pos_out;
    double* d_label = label_out;
    if (mem == EEGFX_MEM_HOST) {
      uint8_t* o = (uint8_t*)ctx->out.get((sizeof(int64_t) + sizeof(double)) * (size_t)n);
      d_pos_out = pos_out ? (int64_t*)o : nullptr;
      d_label = label_out ? (double*)(o + sizeof(int64_t) * (size_t)n) : nullptr;
    }
    void* scratch = ctx->scratch.get(plan_scratch_bytes(n));
    PlanResult r;
    HIP_CHECK(launch_plan_markers(ctx->stream, d_pos, d_stim, n, n_frames, guessed,
                                  (int)*balance, scratch, d_pos_out, d_label, &r));
    if (mem == EEGFX_MEM_HOST && r.selected > 0) {
      if (pos_out)
        HIP_CHECK(hipMemcpyAsync(pos_out, d_pos_out, sizeof(int64_t) * (size_t)r.selected,
                                 hipMemcpyDeviceToHost, ctx->stream));
      if (label_out)
        HIP_CHECK(hipMemcpyAsync(label_out, d_label, sizeof(double) * (size_t)r.selected,
                                 hipMemcpyDeviceToHost, ctx->stream));
    }
    ctx->drain();
    *balance = r.balance;
    *n_selected = r.selected;
    if (r.first_unparsable >= 0)  // Integer.parseInt's NumberFormatException ends the reference loop
      fail(EEGFX_EFORMAT, "marker %lld: unparsable stimulus description",
           (long long)r.first_unparsable);
  });
}

int eegfx_synth_recording(eegfx_ctx* ctx, int16_t* dst, int64_t n_frames, int32_t n_channels,
                          uint64_t seed) {
  return guarded([&] {
    if (!ctx || !dst) fail(EEGFX_EINVAL, "null argument");
    if (n_frames < 0 || n_channels < 1) fail(EEGFX_EINVAL, "bad size");
    ctx->activate();
    HIP_CHECK(launch_synth(ctx->stream, dst, n_frames, n_channels, seed));
  });
}

}  // extern "C"
