// mailbox.h -- the opt-in resident small-batch server of a context (eegfx_ctx_set_mailbox,
// features_mailbox_kernel): its state and its host state machine.  Internal: not installed.
#pragma once

#include <hip/hip_runtime.h>

#include <chrono>

#include "launch.h"

struct eegfx_ctx;

namespace eegfx {

// A host-mapped command block, the kernel's own stream (never the context stream: the kernel
// stays resident), the request sequence and the time of the last request.  A server needs a
// hardware queue of its own (a queue runs its packets in order: a second kernel behind a
// resident one waits for it to idle out), and the highest-priority pool has kMbSlotsPerDevice of
// them, so at most that many contexts of the process hold a server slot on a device
// (mb_acquire, small_gate.h); the others serve their calls on the launch path, and take a slot
// when one frees.  The server reads the owning context's small-call staging (pin_in, pin_out).
struct Mailbox {
  eegfx_ctx* ctx;        // the owner: its device and its small-call staging
  bool on = false;       // enabled by the caller
  bool slot = false;     // holds one of the device's server slots
  hipStream_t stream = nullptr;
  MailboxCmd* host = nullptr;
  MailboxCmd* dev = nullptr;
  size_t cap = 0;  // pinned_pool capacity of host
  uint32_t seq = 0;
  uint32_t gen = 0;      // launch generation (MailboxCmd::alive)
  bool live = false;     // launched and not stopped by the host (it may still have idled out)
  bool started = false;  // the live server has published its generation
  bool stuck = false;    // a server that did not start in time: stopped, not yet returned
  std::chrono::steady_clock::time_point last{};
  static constexpr uint64_t kIdleTicks = 100000000;  // 1 s of s_memrealtime (100 MHz)
  static constexpr auto kStartWait = std::chrono::milliseconds(20);

  bool enabled() const { return on; }
  bool resident() const { return on && slot && live && started; }
  void launch();
  // Stops a live server: `stop` is seen within one poll.  A server that has not returned after
  // 10 s (100 ms if it has not been seen to start: its queue is held by another resident kernel)
  // keeps `stop` set, so it returns as soon as it runs, and is marked stuck; ready() clears
  // `stop` once it has returned.
  // Returns whether the kernel has returned.
  bool stop();
  // A resident server reads the staging it was launched with: stops it before a growth past the
  // staging's capacity (the next request restarts it on the new buffers).
  void stop_before_growth(size_t in_bytes, size_t out_bytes);
  // hipSuccess: the server kernel has returned; hipErrorNotReady: it is running; anything else
  // is an error of the stream and is raised
  bool returned();
  // Whether the resident server takes this call (false: the launch path).  Takes a device slot
  // and sets the server up on first use; restarts a server that may be near its 1 s idle exit
  // (no request for 500 ms) so a request never races that exit; posts nothing until the server
  // has published its generation, and falls back to the launch path (marking the server stuck)
  // if it has not started within kStartWait.
  bool ready();
  // One request: n epochs of packed window rows in pin_in -> rows in pin_out (after ready()).
  void serve(int64_t n, int C, int nfeat);
  // Stops the server, gives back its slot and disables it.
  void release();
};

}  // namespace eegfx
