// ctx.h -- the device context (struct eegfx_ctx) and the helpers that the host sources share:
// the staging of host-memory arguments (stage_in, dev_out, copy_out and what is built on them),
// the argument checks (defined in api.cpp) and the device-pointer pipelines (routes.cpp), used by
// api.cpp, routes.cpp, streamed.cpp, classify.cpp, sharded.cpp, nn.cpp, tree_driver.cpp,
// mailbox.cpp, flow.cpp and odp.cpp (the OffLineDataProvider).
// Internal: not installed.
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <array>
#include <chrono>
#include <cstdint>
#include <map>
#include <mutex>
#include <thread>
#include <utility>
#include <vector>

#include "common.h"
#include "eegfx_ext.h"
#include "joiner.h"
#include "launch.h"
#include "mailbox.h"

#define HIP_CHECK(expr)                                                                 \
  do {                                                                                  \
    hipError_t _e = (expr);                                                             \
    if (_e != hipSuccess) fail(EEGFX_EHIP, "%s: %s", #expr, hipGetErrorString(_e));     \
  } while (0)

// Microseconds a small call's waiter spins before it sleeps (A/B builds vary it).
#ifndef EEGFX_SMALL_SPIN_US
#define EEGFX_SMALL_SPIN_US 30
#endif

namespace eegfx {

// Grow-only device allocation owned by a context, stream-ordered on the context's stream (`*sp`):
// every use of the buffer is enqueued there (the streamed path's side streams are drained before
// its call returns), so the old allocation is released behind the work already queued and the new
// one is ready for the work that follows.  Growing never waits for the device -- other contexts
// keep running (a hipDeviceSynchronize + hipFree here stalled every context on the device).
struct DevBuf {
  void* p = nullptr;
  size_t cap = 0;
  const hipStream_t* sp = nullptr;
  void* get(size_t bytes) {
    if (bytes > cap) {
      if (p) (void)hipFreeAsync(p, *sp);
      p = nullptr;
      cap = 0;
      if (hipMallocAsync(&p, bytes ? bytes : 1, *sp) != hipSuccess) {
        (void)hipGetLastError();
        p = nullptr;
        fail(EEGFX_ENOMEM, "hipMallocAsync(%zu) failed", bytes);
      }
      cap = bytes;
    }
    return p;
  }
  void release() {
    if (p) (void)hipFreeAsync(p, *sp);
    p = nullptr;
    cap = 0;
  }
};

// Pinned host memory is never returned to the runtime while the process runs: hipHostFree (like
// hipFree) synchronises the whole device, which waits for every resident per-epoch server of
// every context (up to its 1 s idle exit) -- a context destroyed or a staging buffer grown on one
// executor thread stalled every other thread's calls for a second (profiles/r06/dropin_threads).
// Buffers go back to this process-wide pool instead and are reused by the next request of at
// least their size with the same flags; the pool holds at most the peak of what was in use.
struct PinnedPool {
  std::mutex mu;
  std::multimap<std::pair<unsigned, size_t>, void*> free;  // (flags, capacity) -> buffer
  void* take(size_t bytes, unsigned flags, size_t* cap) {
    bytes = std::max<size_t>(bytes, 64);
    {
      std::lock_guard<std::mutex> l(mu);
      auto it = free.lower_bound({flags, bytes});
      if (it != free.end() && it->first.first == flags && it->first.second <= 2 * bytes + 65536) {
        void* p = it->second;
        *cap = it->first.second;
        free.erase(it);
        return p;
      }
    }
    void* p = nullptr;
    if (hipHostMalloc(&p, bytes, flags) != hipSuccess) {
      (void)hipGetLastError();
      fail(EEGFX_ENOMEM, "hipHostMalloc(%zu) failed", bytes);
    }
    *cap = bytes;
    return p;
  }
  void give(void* p, size_t cap, unsigned flags) {
    if (!p) return;
    std::lock_guard<std::mutex> l(mu);
    free.emplace(std::make_pair(flags, cap), p);
  }
};
PinnedPool& pinned_pool();

// Grow-only pinned host buffer (hipHostMalloc: mapped into the device address space, from
// pinned_pool), for the small-batch IFeatureExtraction path and the streamed path's host staging.
// Only touched by the owning context's calls, which synchronise before they return.
struct PinBuf {
  void* p = nullptr;
  size_t cap = 0;
  void* get(size_t bytes) {
    if (bytes > cap) {
      pinned_pool().give(p, cap, hipHostMallocMapped);
      p = nullptr;
      cap = 0;
      p = pinned_pool().take(bytes, hipHostMallocMapped, &cap);
    }
    return p;
  }
  void* device_ptr() const {
    void* d = nullptr;
    if (hipHostGetDevicePointer(&d, p, 0) != hipSuccess)
      fail(EEGFX_EHIP, "hipHostGetDevicePointer failed");
    return d;
  }
  void release() {
    pinned_pool().give(p, cap, hipHostMallocMapped);
    p = nullptr;
    cap = 0;
  }
};

ChanSel make_sel(const int32_t* cols, const float* res, int C, int ct);
void check_positions(const int64_t* pos, int64_t n, int64_t n_frames);
void check_fe_params(int C, int name, int epoch_size, int skip, int feature_size);
bool wide_features(int feature_size);

}  // namespace eegfx

// the C ABI's opaque type lives in the global namespace; both sources that see its definition
// use namespace eegfx throughout
using namespace eegfx;

struct eegfx_ctx {
  int device = 0;
  hipStream_t own = nullptr;
  hipStream_t stream = nullptr;
  int numerics = EEGFX_EXACT;
  // Error word of the device-side position checks (fused.hip position_ok): host-mapped pinned
  // memory the kernels store 1 into; eegfx_ctx_synchronize reports and clears it.
  int* err_host = nullptr;
  int* err_dev = nullptr;
  size_t err_cap = 0;  // pinned_pool capacity of err_host
  // the fma window kernel's guard strategy (guard.h EEGFX_TRACK_X), set by baseline_kernel in the
  // same host-mapped block, 8 bytes past the error word
  unsigned int* track_host() const { return (unsigned int*)((char*)err_host + 8); }
  unsigned int* track_dev() const { return (unsigned int*)((char*)err_dev + 8); }
  bool guard_track() const {
    return EEGFX_TRACK_X == 2 ||
           (EEGFX_TRACK_X == 1 && __atomic_load_n(track_host(), __ATOMIC_RELAXED) != 0);
  }
  bool timing = false;
  // HIP event pairs bracketing each timed (dominant) kernel launch on the context stream, plus
  // the algorithmic bytes each launch moved; summed by eegfx_ctx_kernel_stats.
  std::vector<std::pair<hipEvent_t, hipEvent_t>> events;
  std::vector<int64_t> event_bytes;
  size_t n_timed = 0;
  // The grow-only device buffers.  A call drains the stream before it returns, so entries share
  // them freely from call to call; two buffers that one call uses at once stay apart.  Each is
  // also named in buffers() below -- the one other place a new buffer is added.
  // The raw entries (api.cpp, streamed.cpp, odp.cpp) and eegfx_plan_markers_device: a host
  // caller's recording and positions, the results on their way back (plan: pos_out ++ label_out),
  // the intermediate epochs / window chunks / plan scratch, the fused kernels' scratch.
  DevBuf raw, pos, out, scratch, fused;
  // Host callers' rows, shared by eegfx_logreg_* / eegfx_svm_* / eegfx_dtree_* / eegfx_rforest_*
  // train and predict (stage_xy, predict_frame): X [n][d] in; one value per row -- the labels in
  // (train) or the predictions out (predict), and the int32 stimulus index per marker of
  // eegfx_plan_markers_device.
  DevBuf rows_x, row_vals;
  // eegfx_logreg_* / eegfx_svm_* / eegfx_glm_*: LrState (train: state, weights and the label
  // verdict behind them; predict: the weights), the gradient partials, a chunk of mini-batch masks
  DevBuf lr_state, lr_part, lr_mask;
  // more than one shard: the root's [shards][d] slots / another shard's folded d-vector; the
  // positions of a shard given without them
  DevBuf lr_fold, lr_pos;
  // eegfx_dtree_train / eegfx_rforest_train (dt_bin_rows, grow_trees): threshold table, bins, slot
  // + label per row, one group's histograms (and the gathered split sample).  dt_nodes: records
  // per node from the host -- a group's DtDecisions (train), the model's DtNodes
  // (eegfx_dtree_predict / eegfx_rforest_predict).
  DevBuf dt_tab, dt_bins, dt_rows, dt_hist, dt_nodes;
  // the bagged or subsampled forest on top of them: weight per tree and row, slot per tree and
  // row.  rf_tab: int32 tables from the host -- a group's feature subsets and launch tree lists
  // (eegfx_rforest_train), the tree offsets (eegfx_rforest_predict).
  DevBuf rf_weight, rf_slot, rf_tab;
  // the train/test flow: rows to gather from (eegfx_gather_rows, eegfx_odp_split) / predictions
  // (eegfx_confusion_counts); the indices, the gathered rows (gather, split); labels in (split,
  // confusion); labels out (split); the kernels' flag / counter block (all three).
  DevBuf fl_src, fl_idx, fl_dst, fl_lab, fl_y, fl_flag;
  // eegfx_nn_*: NnState with the parameters and the updater's state (train; predict: the
  // parameters), the gradient partials, the loss per iteration; eegfx_nn_statistics: a host
  // caller's scores (its labels go to row_vals), the counters followed by the partial sums.
  DevBuf nn_state, nn_part, nn_scores, nn_in, nn_stat;
  // eegfx_nn_train_opt: NnOpt with the optimiser's vectors, one NnSearchRec per iteration
  DevBuf nn_opt, nn_search;
  PinBuf pin_in, pin_out;                // small-batch extract_features staging (zero-copy)
  PinBuf pin_chunk[2];                   // streamed path: host staging of pageable recordings;
                                         // a sharded provider's worker: the file spans it reads
  // The fma numerics' conditioning guard (guard.h): device memory holding the flagged-row count
  // of the current window_wide_kernel launch (first 128 B), then the running totals of recomputed
  // rows and of rows that went to the second stage, each spread over kGuardSlots lines; the
  // flagged-row list; guard_checked counts the rows that went through a guarded launch.
  static constexpr size_t kGuardDevBytes = 128 + 2 * kGuardSlotBytes + 128;  // + Guard::adapt
  int* guard_dev = nullptr;
  DevBuf guard_list;
  int64_t guard_checked = 0;
  unsigned long long* guard_recomputed_slots() const {
    return (unsigned long long*)((char*)guard_dev + 128);
  }
  unsigned long long* guard_rechecked_slots() const {
    return (unsigned long long*)((char*)guard_dev + 128 + kGuardSlotBytes);
  }
  unsigned long long* guard_adapt() const {
    return (unsigned long long*)((char*)guard_dev + 128 + 2 * kGuardSlotBytes);
  }
  Guard guard_for(int64_t n) {
    if (numerics == EEGFX_EXACT) return Guard{nullptr, nullptr, nullptr};
    guard_checked += n;
    return Guard{guard_dev, (int64_t*)guard_list.get(sizeof(int64_t) * (size_t)std::max<int64_t>(n, 1)),
                 guard_recomputed_slots(), guard_rechecked_slots(), guard_adapt(), track_dev()};
  }
  // every DevBuf of the context: bound to the stream at creation, released at destruction
  auto buffers() {
    return std::array{&raw, &pos, &out, &scratch, &fused, &rows_x, &row_vals, &lr_state, &lr_part,
                      &lr_mask, &lr_fold, &lr_pos, &guard_list, &dt_tab, &dt_bins, &dt_rows,
                      &dt_hist, &dt_nodes,
                      &rf_weight, &rf_slot, &rf_tab, &fl_src, &fl_idx, &fl_dst, &fl_lab, &fl_y,
                      &fl_flag, &nn_state, &nn_part, &nn_scores, &nn_in, &nn_stat,
                      &nn_opt, &nn_search};
  }
  void bind_buffers() {
    for (DevBuf* b : buffers()) b->sp = &stream;
  }
  void release_buffers() {
    for (DevBuf* b : buffers()) b->release();
    pin_in.release();
    pin_out.release();
    pin_chunk[0].release();
    pin_chunk[1].release();
  }
  // streamed path (eegfx_process_recording_streamed): upload / download streams and the chunk
  // events, created on first use and kept for the context's lifetime
  hipStream_t up = nullptr, down = nullptr;
  std::vector<hipEvent_t> copied, done;  // per device chunk buffer: uploaded / kernels done
  // a provider's worker: the last upload out of each pin_chunk buffer, created on first use too
  hipEvent_t staged[2] = {nullptr, nullptr};
  void stream_resources(size_t ring) {
    if (!up) {
      HIP_CHECK(hipStreamCreateWithFlags(&up, hipStreamNonBlocking));
      HIP_CHECK(hipStreamCreateWithFlags(&down, hipStreamNonBlocking));
    }
    while (copied.size() < ring) {
      hipEvent_t a = nullptr, b = nullptr;
      HIP_CHECK(hipEventCreateWithFlags(&a, hipEventDisableTiming));
      if (hipEventCreateWithFlags(&b, hipEventDisableTiming) != hipSuccess) {
        (void)hipEventDestroy(a);
        fail(EEGFX_EHIP, "hipEventCreateWithFlags");
      }
      copied.push_back(a);
      done.push_back(b);
    }
  }
  // Completion of a small (latency-bound) call: spinning on an event query returns ~0.5 us sooner
  // than hipStreamSynchronize (the drop-in bench's launch floor: 11.6 vs 12.2 us).  Past kSmallSpin
  // the thread sleeps until the event completes (a blocking-sync event: interrupt-driven), so a
  // waiter is not runnable: with more calling threads than cores (Spark local[*] on a CPU quota),
  // runnable waiters kept threads whose work had completed off the cores for scheduler slices
  // (profiles/r06/dropin_gate_ab.log).
  static constexpr auto kSmallSpin = std::chrono::microseconds(EEGFX_SMALL_SPIN_US);
  hipEvent_t small_done = nullptr;
  void wait_small() {
    if (!small_done)
      HIP_CHECK(hipEventCreateWithFlags(&small_done, hipEventDisableTiming | hipEventBlockingSync));
    HIP_CHECK(hipEventRecord(small_done, stream));
    const auto t0 = std::chrono::steady_clock::now();
    hipError_t e;
    while ((e = hipEventQuery(small_done)) == hipErrorNotReady) {
      if (std::chrono::steady_clock::now() - t0 > kSmallSpin) {
        HIP_CHECK(hipEventSynchronize(small_done));
        return;
      }
    }
    HIP_CHECK(e);
  }
  // The opt-in resident small-batch server (eegfx_ctx_set_mailbox): mailbox.h.
  Mailbox mb{this};
  void release_stream_resources() {
    mb.release();
    if (small_done) (void)hipEventDestroy(small_done);
    small_done = nullptr;
    for (hipEvent_t e : copied) (void)hipEventDestroy(e);
    for (hipEvent_t e : done) (void)hipEventDestroy(e);
    copied.clear();
    done.clear();
    for (hipEvent_t& e : staged) {
      if (e) (void)hipEventDestroy(e);
      e = nullptr;
    }
    if (up) (void)hipStreamDestroy(up);
    if (down) (void)hipStreamDestroy(down);
    up = down = nullptr;
  }

  void activate() const { HIP_CHECK(hipSetDevice(device)); }
  // Waits for the stream, then reports (and clears) a device-resident marker position that a
  // kernel enqueued on this context since the last check refused: every API call that
  // synchronises does this, so an invalid position surfaces at the first synchronising call
  // after it (at the latest eegfx_ctx_synchronize), never silently.
  void check_positions_flag() {
    if (__atomic_exchange_n(err_host, 0, __ATOMIC_ACQ_REL) != 0)
      fail(EEGFX_ERANGE,
           "a device-resident marker position lies outside [100, n_frames + 100] "
           "(OffLineDataProvider.java:220-225: ArrayIndexOutOfBoundsException); the rows of such "
           "epochs are unspecified");
  }
  void drain() {
    HIP_CHECK(hipStreamSynchronize(stream));
    check_positions_flag();
  }
  void tic() {
    if (!timing) return;
    if (n_timed == events.size()) {
      // timing only (read after the stream drains): no system-scope fence at each record, so
      // the bracketed kernel's neighbours pay no cache writeback / invalidate for the timing
      hipEvent_t a, b;
      HIP_CHECK(hipEventCreateWithFlags(&a, hipEventDisableSystemFence));
      HIP_CHECK(hipEventCreateWithFlags(&b, hipEventDisableSystemFence));
      events.emplace_back(a, b);
      event_bytes.push_back(0);
    }
    HIP_CHECK(hipEventRecord(events[n_timed].first, stream));
  }
  void toc(int64_t bytes) {
    if (!timing) return;
    HIP_CHECK(hipEventRecord(events[n_timed].second, stream));
    event_bytes[n_timed] = bytes;
    ++n_timed;
  }
  void destroy_events() {
    for (auto& e : events) {
      (void)hipEventDestroy(e.first);
      (void)hipEventDestroy(e.second);
    }
    events.clear();
    event_bytes.clear();
    n_timed = 0;
  }
};

namespace eegfx {

void check_mem(int mem);

// ---- a `mem` argument becomes device pointers.  Everything is queued on the context stream.
// An argument as the kernels read it: the caller's device pointer, or a copy of the host array in
// `buf` (T const for an input; not for an output whose first contents count).
template <typename T>
T* stage_in(eegfx_ctx* ctx, DevBuf& buf, T* src, size_t bytes, int mem) {
  if (mem == EEGFX_MEM_DEVICE) return src;
  void* d = buf.get(bytes);
  if (bytes) HIP_CHECK(hipMemcpyAsync(d, src, bytes, hipMemcpyHostToDevice, ctx->stream));
  return (T*)d;
}
// Where a call's results are written on the device: the caller's buffer, or the context's.
template <typename T>
T* dev_out(DevBuf& buf, T* caller, size_t bytes, int mem) {
  return mem == EEGFX_MEM_DEVICE ? caller : (T*)buf.get(bytes);
}
// A call's results queued back to a host caller; nothing for a device caller or for no bytes.
// No drain: the classifier, tree, gather and confusion entries drain for both memory kinds.
inline void copy_back(eegfx_ctx* ctx, void* host_dst, const void* dev_src, size_t bytes, int mem) {
  if (mem == EEGFX_MEM_HOST && bytes)
    HIP_CHECK(hipMemcpyAsync(host_dst, dev_src, bytes, hipMemcpyDeviceToHost, ctx->stream));
}
// ... and the stream drained for that host caller (the raw entries: a device caller's results
// stay stream-ordered).
inline void copy_out(eegfx_ctx* ctx, void* host_dst, const void* dev_src, size_t bytes, int mem) {
  copy_back(ctx, host_dst, dev_src, bytes, mem);
  if (mem == EEGFX_MEM_HOST) ctx->drain();
}

// ---- the classifier entries' front door and frames
constexpr const char* kBadLabels = "Input validation failed: labels must be 0.0 or 1.0";
inline void check_train_d(int32_t d) {
  if (d < 1 || d > kLrMaxFeatures) fail(EEGFX_EINVAL, "d=%d outside [1, %d]", d, kLrMaxFeatures);
}
inline void check_predict_dims(int64_t n, int32_t d) {
  if (n < 0 || d < 1 || d > kLrMaxFeatures) fail(EEGFX_EINVAL, "n=%lld d=%d", (long long)n, d);
}
// The training pair of glm_sgd_train_shards and dt_bin_rows as the kernels read it.
struct TrainXY {
  const double* X;
  const double* y;
};
inline TrainXY stage_xy(eegfx_ctx* ctx, const double* X, const double* y, int64_t n, int32_t d,
                        int mem) {
  const double* dX = stage_in(ctx, ctx->rows_x, X, sizeof(double) * (size_t)(n * d), mem);
  return {dX, stage_in(ctx, ctx->row_vals, y, sizeof(double) * (size_t)n, mem)};
}
// The frame of a predict call (glm_predict, predict_rows; n > 0): X staged, launch(dX, dout)
// uploads the model and runs the kernel, the predictions go back to a host caller, and the stream
// drains for both memory kinds -- the model is read out of the caller's arrays until then.
template <typename Launch>
void predict_frame(eegfx_ctx* ctx, const double* X, int64_t n, int32_t d, double* out, int mem,
                   Launch&& launch) {
  ctx->activate();
  const double* dX = stage_in(ctx, ctx->rows_x, X, sizeof(double) * (size_t)(n * d), mem);
  double* dout = dev_out(ctx->row_vals, out, sizeof(double) * (size_t)n, mem);
  launch(dX, dout);
  copy_back(ctx, out, dout, sizeof(double) * (size_t)n, mem);
  ctx->drain();
}

// The processors this process may run on (classify.cpp): Spark local[*]'s defaultParallelism.
int available_processors();
// sharded.cpp: the one GradientDescent driver, behind eegfx_glm_sgd_train_sharded and, with the
// context as its one shard, behind the one-context entries (classify.cpp).  The caller has
// checked the shards (contexts distinct, X / y there where n > 0); `weights` in and, on success
// only, out.  mem: where every shard's X and y lie (pos: the device); host rows are staged on the
// shard's context once the arguments have passed.  A guarded call of its own: returns the status.
int glm_sgd_train_shards(int grad, const eegfx_glm_shard* shards, int32_t n_shards, int32_t d,
                         int32_t num_iterations, double step_size, double reg_param,
                         double mini_batch_fraction, double convergence_tol,
                         int32_t num_partitions, double* weights, int32_t* iterations_run,
                         int mem);
// classify.cpp, the driver's: the argument ladder past the null and row-count checks (returns
// whether the run is sampled); the iterations whose masks are drawn and uploaded at a time; and
// the masks of iterations i0 + 1 .. i0 + k over n rows ((n + 31) / 32 words each) with their row
// counts, drawn by threads.
bool check_sgd_args(int grad, int32_t d, int32_t num_iterations, double mini_batch_fraction,
                    int32_t num_partitions);
int sgd_mask_chunk(int64_t n, int num_iterations);
void draw_sgd_masks(int64_t n, double fraction, int num_partitions, int i0, int k, uint32_t* masks,
                    int64_t* counts);
// `bytes` from src on context `from` to dst on context `to`, on `st`: a device-to-device copy
// where the two share a device, a peer copy otherwise.
inline void copy_between(void* dst, const eegfx_ctx* to, const void* src, const eegfx_ctx* from,
                         size_t bytes, hipStream_t st) {
  if (to->device == from->device)
    HIP_CHECK(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, st));
  else
    HIP_CHECK(hipMemcpyPeerAsync(dst, to->device, src, from->device, bytes, st));
}
// flow.cpp: eegfx_confusion_counts' verdict on a device count (bad label, then fewer than two
// actual classes), and its cells as counts.
void confusion_verdict(const ConfusionOut& h, int64_t counts[4]);
// tree_driver.cpp: the binned rows of a tree or forest call.  Host: the threshold table `tab`
// (int32 flags[4], nthr[d], double thr[d][T]); device: the same table, bins uint8 [n][d], slot
// int32 [n] = 0, label uint8 [n], and the scratch allocation for the histograms.
struct DtBinned {
  int B = 0, T = 0;  // numBins, numSplits
  std::vector<uint8_t> tab;
  int32_t* nthr = nullptr;
  double* thr = nullptr;
  uint8_t* dtab = nullptr;
  uint8_t* bins = nullptr;
  int32_t* slot = nullptr;
  uint8_t* label = nullptr;
  void* scratch = nullptr;
};
void dt_bin_rows(eegfx_ctx* ctx, const double* X, const double* y, int64_t n, int32_t d,
                 int32_t max_bins, int64_t split_seed, int mem, size_t hist_bytes, DtBinned* out);
// flow.cpp: Collections.shuffle(list, new Random(seed)) of n items as the original index of every
// position, and the row gather on the context stream (device pointers, m > 0, timed): `slot`
// (0 or 1) picks the word of ctx->fl_flag that gather_check reads after the stream has drained.
std::vector<int64_t> java_shuffle(int64_t n, int64_t seed);
void run_gather_rows(eegfx_ctx* ctx, const double* src, int64_t n_src, int d, const int64_t* idx,
                     int64_t m, double* dst, int slot);
void gather_check(eegfx_ctx* ctx, int slots, int64_t n_src);
// The raw entries' argument ladder up to the null-buffer check (api.cpp check_raw_args goes on
// from it).  `mem`: EEGFX_MEM_HOST from an entry without a mem flag.
void check_raw_head(const eegfx_ctx* ctx, int mem, const void* raw, int fmt, int64_t n_frames,
                    int ct, const int64_t* pos, int64_t n, const void* out);

// raw -> features on the context stream (device pointers).  Fused kernel when one covers the
// layout, otherwise cut + features through the context scratch buffer.
void run_features_from_raw(eegfx_ctx* ctx, const void* raw, int fmt, int64_t n_frames, int ct,
                           const ChanSel& sel, int C, const int64_t* pos, int64_t n, double* out);

// raw -> epochs + features (device pointers): the one-pass kernels when the layout fits them,
// else the cut pass followed by the batch extract over the rows it wrote.  E: double or float epochs
// (eegfx_process_recording_epochs / _f32): the same kernels, the same rows in `feat`.
template <typename E>
void run_epochs_and_features(eegfx_ctx* ctx, const void* raw, int fmt, int64_t n_frames, int ct,
                             const ChanSel& sel, int C, const int64_t* pos, int64_t n, E* ep,
                             double* feat);

// Epoch rows (device pointers, `row_stride` elements apart, double or float) -> features: the
// library's one choice between the full-pyramid kernels (feature sizes past a6 ++ d6: no guard)
// and the filter bank under the fma guard.  The guard is taken for these n rows
// (eegfx_ctx::guard_for, once per launch) unless the caller took one for a whole call that it
// launches in chunks (`call_guard`).  No tic / toc: the callers bracket what they time.
template <typename E>
void run_features_from_epochs(eegfx_ctx* ctx, const E* ep, int64_t n, int C, int skip,
                              int feature_size, double* out, int row_stride,
                              const Guard* call_guard = nullptr);

}  // namespace eegfx
