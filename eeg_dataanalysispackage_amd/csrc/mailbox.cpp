// mailbox.cpp -- the host state machine of a context's resident small-batch server (mailbox.h).
#include <cstring>
#include <thread>

#include "ctx.h"
#include "small_gate.h"

namespace eegfx {

void Mailbox::launch() {
  // the staging a server reads is fixed for its lifetime (growing it stops the server first)
  host->rows = ctx->pin_in.p ? (const double*)ctx->pin_in.device_ptr() : nullptr;
  host->out = ctx->pin_out.p ? (double*)ctx->pin_out.device_ptr() : nullptr;
  if (++gen == 0) gen = 1;
  HIP_CHECK(launch_features_mailbox(stream, dev, kIdleTicks, gen));
  live = true;
  started = false;
}

bool Mailbox::stop() {
  if (!host || !live) return true;
  __atomic_store_n(&host->stop, 1u, __ATOMIC_RELEASE);
  const auto t0 = std::chrono::steady_clock::now();
  hipError_t q;
  while ((q = hipStreamQuery(stream)) == hipErrorNotReady) {
    if (std::chrono::steady_clock::now() - t0 >
        (started ? std::chrono::milliseconds(10000) : std::chrono::milliseconds(100))) {
      live = false;
      stuck = true;
      return false;
    }
    std::this_thread::yield();
  }
  __atomic_store_n(&host->stop, 0u, __ATOMIC_RELEASE);
  live = false;
  HIP_CHECK(q);
  return true;
}

void Mailbox::stop_before_growth(size_t in_bytes, size_t out_bytes) {
  if (live && (in_bytes > ctx->pin_in.cap || out_bytes > ctx->pin_out.cap)) stop();
}

bool Mailbox::returned() {
  const hipError_t q = hipStreamQuery(stream);
  if (q == hipErrorNotReady) return false;
  HIP_CHECK(q);
  return true;
}

bool Mailbox::ready() {
  if (!on) return false;
  if (stuck) {  // a server that never started: the launch path until it has run and returned
    if (!returned()) return false;
    __atomic_store_n(&host->stop, 0u, __ATOMIC_RELEASE);
    stuck = false;
  }
  if (!slot) {
    if (!mb_acquire(ctx->device)) return false;
    slot = true;
  }
  if (!stream) {
    try {
      // A stream of the highest priority: the runtime multiplexes a process's streams of one
      // priority over a few hardware queues, and a queue runs its packets in order, so a
      // normal-priority stream sharing the resident kernel's queue would wait behind it (up to
      // its 1 s idle exit).  The high-priority pool keeps the server on a queue of its own while
      // no more than kMbSlotsPerDevice servers exist.
      int least = 0, greatest = 0;
      HIP_CHECK(hipDeviceGetStreamPriorityRange(&least, &greatest));
      HIP_CHECK(hipStreamCreateWithPriority(&stream, hipStreamNonBlocking, greatest));
      host = (MailboxCmd*)pinned_pool().take(sizeof(MailboxCmd),
                                             hipHostMallocMapped | hipHostMallocCoherent, &cap);
      memset(host, 0, sizeof(MailboxCmd));
      HIP_CHECK(hipHostGetDevicePointer((void**)&dev, host, 0));
      seq = 0;
    } catch (...) {
      release();
      on = true;  // still enabled: later calls retry
      throw;
    }
  }
  const auto now = std::chrono::steady_clock::now();
  // no request for 500 ms: the server may be close to its 1 s idle exit -- restart it, so no
  // request is ever posted to a kernel that is returning
  if (live && now - last > std::chrono::milliseconds(500) && !stop()) return false;
  if (!live) {
    launch();
    last = now;
  }
  if (!started) {
    const auto t0 = std::chrono::steady_clock::now();
    while (__atomic_load_n(&host->alive, __ATOMIC_ACQUIRE) != gen) {
      if (std::chrono::steady_clock::now() - t0 > kStartWait) {
        // still queued: it returns at once when it runs (stop), the call takes the launch path
        __atomic_store_n(&host->stop, 1u, __ATOMIC_RELEASE);
        live = false;
        stuck = true;
        return false;
      }
      __builtin_ia32_pause();
    }
    started = true;
  }
  return true;
}

void Mailbox::serve(int64_t n, int C, int nfeat) {
  MailboxCmd* m = host;
  if (++seq == 0) seq = 1;  // 0 means "no request" to the kernel
  const auto now = std::chrono::steady_clock::now();
  __atomic_store_n(&m->req, mailbox_request(seq, C, nfeat, n), __ATOMIC_RELEASE);
  for (uint64_t spin = 1;; ++spin) {
    if (__atomic_load_n(&m->done, __ATOMIC_ACQUIRE) == seq) break;
    // as wait_small: a waiter past kSmallSpin sleeps between polls instead of staying runnable
    if ((spin & 63) == 0 && std::chrono::steady_clock::now() - now > eegfx_ctx::kSmallSpin)
      std::this_thread::sleep_for(std::chrono::microseconds(10));
    if ((spin & 4095) == 0) {
      // a server that returned with the request pending (an error, or a stop from another
      // path): serve it again on the same stream, after that kernel
      if (returned() && __atomic_load_n(&m->done, __ATOMIC_ACQUIRE) != seq) launch();
      if (std::chrono::steady_clock::now() - now > std::chrono::seconds(30))
        fail(EEGFX_EHIP, "mailbox request %u not served within 30 s", seq);
    }
    __builtin_ia32_pause();
  }
  last = std::chrono::steady_clock::now();
}

void Mailbox::release() {
  const bool stopped = stop();
  if (stream && stopped && !stuck) (void)hipStreamDestroy(stream);
  if (host && stopped && !stuck)
    pinned_pool().give(host, cap, hipHostMallocMapped | hipHostMallocCoherent);
  // a stuck server keeps its stream and command block (it still reads `stop` when it runs):
  // leaked rather than freed under a queued kernel
  host = nullptr;
  dev = nullptr;
  stream = nullptr;
  live = started = stuck = false;
  if (slot) mb_release(ctx->device);
  slot = false;
  on = false;
}

}  // namespace eegfx
