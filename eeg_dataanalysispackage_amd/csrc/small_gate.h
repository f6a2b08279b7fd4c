// small_gate.h -- the two process-wide, per-device admission structures of the small-call paths:
// the resident-server slot registry and the gate of small launched calls.  Host concurrency code
// only (no HIP): tests/c_abi/small_gate_check.cpp runs it on the CPU under the sanitizers.
#pragma once

#include <condition_variable>
#include <mutex>

namespace eegfx {

// Resident-server slots per device (Mailbox::ready): the highest-priority hardware queues
// of the process (4 on the box: a fifth server shares a queue and waits behind another until it
// idles out).
constexpr int kMbSlotsPerDevice = 4;
constexpr int kMbMaxDevices = 64;
inline std::mutex g_mb_mu;
inline int g_mb_used[kMbMaxDevices] = {};
inline bool mb_acquire(int dev) {
  if (dev < 0 || dev >= kMbMaxDevices) return false;
  std::lock_guard<std::mutex> l(g_mb_mu);
  if (g_mb_used[dev] >= kMbSlotsPerDevice) return false;
  ++g_mb_used[dev];
  return true;
}
inline void mb_release(int dev) {
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
inline std::mutex g_small_mu;
inline int g_small_inside[kMbMaxDevices] = {};
inline SmallWaiter* g_small_head[kMbMaxDevices] = {};  // FIFO of sleeping callers
inline SmallWaiter* g_small_tail[kMbMaxDevices] = {};
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

}  // namespace eegfx
