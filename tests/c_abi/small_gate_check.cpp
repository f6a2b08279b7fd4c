// small_gate_check.cpp -- the small-call gate and the server slot registry (csrc/small_gate.h) on
// the CPU, as a stand-alone program: built with -fsanitize=thread and with
// -fsanitize=address,undefined by tests/test_small_gate.py and run directly.  No HIP call.
//
//   1. 32 threads x PASSES passes through SmallCallGate on device 0, 4 threads on device 5: never
//      more than kSmallCallers inside per device (a high-water mark), every pass completes.
//   2. Admission order equals arrival order: with the gate full, waiters arrive one at a time
//      (arrival = the waiter is linked into the gate's queue, read under the gate's own lock) and
//      every exit admits exactly the one at the head.  Holds for any cap >= 1; the test also
//      builds the program with -DEEGFX_SMALL_CALLERS=1.
//   3. Out-of-range devices pass straight through; the slot registry refuses a fifth server on a
//      device, takes one again after a release, and refuses out-of-range devices.
#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <thread>
#include <vector>

#include "small_gate.h"

using namespace eegfx;

#define CHECK(cond)                                                        \
  do {                                                                     \
    if (!(cond)) {                                                         \
      fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); \
      exit(1);                                                             \
    }                                                                      \
  } while (0)

static int queued(int dev) {  // waiters linked into the device's FIFO
  std::lock_guard<std::mutex> l(g_small_mu);
  int k = 0;
  for (SmallWaiter* w = g_small_head[dev]; w; w = w->next) ++k;
  return k;
}

static int inside(int dev) {
  std::lock_guard<std::mutex> l(g_small_mu);
  return g_small_inside[dev];
}

static void stress(int passes) {
  struct Dev {
    int dev, threads;
    std::atomic<int> in{0}, high{0};
    std::atomic<long> done{0};
  };
  Dev devs[2];
  devs[0].dev = 0, devs[0].threads = 32;
  devs[1].dev = 5, devs[1].threads = 4;
  std::vector<std::thread> th;
  for (Dev& d : devs)
    for (int t = 0; t < d.threads; ++t)
      th.emplace_back([&d, passes] {
        for (int p = 0; p < passes; ++p) {
          SmallCallGate gate(d.dev);
          const int now = d.in.fetch_add(1) + 1;
          int h = d.high.load();
          while (now > h && !d.high.compare_exchange_weak(h, now)) {
          }
          if ((p & 15) == 0) std::this_thread::yield();  // let the queue build up
          d.in.fetch_sub(1);
          d.done.fetch_add(1);
        }
      });
  for (auto& t : th) t.join();
  for (Dev& d : devs) {
    CHECK(d.done.load() == (long)d.threads * passes);
    CHECK(d.high.load() >= 1 && d.high.load() <= kSmallCallers);
    CHECK(inside(d.dev) == 0 && queued(d.dev) == 0);
    printf("device %d: %d threads x %d passes, at most %d inside (cap %d)\n", d.dev, d.threads,
           passes, d.high.load(), kSmallCallers);
  }
}

static void fifo() {
  const int dev = 2, W = 12;
  std::vector<std::unique_ptr<SmallCallGate>> holders;  // fill the gate: none of these waits
  for (int i = 0; i < kSmallCallers; ++i) holders.emplace_back(new SmallCallGate(dev));
  CHECK(inside(dev) == kSmallCallers && queued(dev) == 0);
  std::atomic<int> admitted{0};
  std::vector<int> order(W, -1);  // order[ticket] = the waiter admitted as the ticket-th
  std::vector<std::atomic<bool>> leave(W);
  for (auto& f : leave) f.store(false);
  std::vector<std::thread> th;
  for (int i = 0; i < W; ++i) {
    th.emplace_back([&, i] {
      SmallCallGate gate(dev);
      order[admitted.load()] = i;  // one admission at a time: the main thread paces the exits
      admitted.fetch_add(1);
      while (!leave[i].load()) std::this_thread::yield();
    });
    while (queued(dev) != i + 1) std::this_thread::yield();  // waiter i has arrived
  }
  for (int k = 0; k < W; ++k) {  // one exit, one admission: the head of the queue
    if (k < kSmallCallers)
      holders[k].reset();
    else
      leave[order[k - kSmallCallers]].store(true);
    while (admitted.load() != k + 1) std::this_thread::yield();
    CHECK(order[k] == k);
    CHECK(queued(dev) == W - k - 1 && inside(dev) == kSmallCallers);
  }
  holders.clear();
  for (auto& f : leave) f.store(true);
  for (auto& t : th) t.join();
  CHECK(inside(dev) == 0 && queued(dev) == 0);
  printf("fifo: %d waiters admitted in arrival order (cap %d)\n", W, kSmallCallers);
}

static void disabled_and_slots() {
  for (int dev : {-1, kMbMaxDevices, kMbMaxDevices + 7}) {  // no gate: more than the cap pass
    std::vector<std::unique_ptr<SmallCallGate>> g;
    for (int i = 0; i < kSmallCallers + 3; ++i) g.emplace_back(new SmallCallGate(dev));
    CHECK(g.back()->dev == -1);
  }
  for (int i = 0; i < kMbSlotsPerDevice; ++i) CHECK(mb_acquire(3));
  CHECK(!mb_acquire(3));  // a fifth server on the device
  CHECK(mb_acquire(4));   // another device has its own slots
  mb_release(3);
  CHECK(mb_acquire(3));
  CHECK(!mb_acquire(3));
  CHECK(!mb_acquire(-1) && !mb_acquire(kMbMaxDevices));
  mb_release(-1);  // ignored
  mb_release(kMbMaxDevices);
  for (int i = 0; i < kMbSlotsPerDevice; ++i) mb_release(3);
  mb_release(3);  // one release too many is ignored
  mb_release(4);
  for (int i = 0; i < kMbSlotsPerDevice; ++i) CHECK(mb_acquire(3));
  CHECK(!mb_acquire(3));
  printf("slots: %d per device\n", kMbSlotsPerDevice);
}

int main(int argc, char** argv) {
  static_assert(kSmallCallers >= 1, "the check needs an enabled gate");
  const int passes = argc > 1 ? atoi(argv[1]) : 3000;
  stress(passes);
  fifo();
  disabled_and_slots();
  printf("small_gate_check ok\n");
  return 0;
}
