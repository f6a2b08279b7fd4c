// api.cpp -- eegfx C ABI: the context's lifecycle and statistics, and the compute entry points over
// raw recordings and epochs: each validates, stages, runs a pipeline of routes.cpp and copies back.
// The argument checks that ctx.h declares are defined here.  The other entry points:
// streamed.cpp (the streamed raw entry), classify.cpp (the MLlib classifiers), odp.cpp (the
// OffLineDataProvider); mailbox.cpp holds the resident server.
#include <algorithm>
#include <cstring>
#include <memory>
#include <type_traits>
#include <vector>

#include "ctx.h"
#include "small_gate.h"

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

void check_mem(int mem) {
  if (mem != EEGFX_MEM_HOST && mem != EEGFX_MEM_DEVICE) fail(EEGFX_EINVAL, "mem flag %d", mem);
}

void check_raw_head(const eegfx_ctx* ctx, int mem, const void* raw, int fmt, int64_t n_frames,
                    int ct, const int64_t* pos, int64_t n, const void* out) {
  if (!ctx) fail(EEGFX_EINVAL, "null context");
  check_mem(mem);
  if (fmt != EEGFX_INT_16 && fmt != EEGFX_IEEE_FLOAT_32) fail(EEGFX_EINVAL, "format %d", fmt);
  if (n_frames < 0 || n < 0 || ct < 1) fail(EEGFX_EINVAL, "negative size");
  if (n > 0 && (!raw || !pos || !out)) fail(EEGFX_EINVAL, "null buffer");
}

int ctx_device(const eegfx_ctx* ctx) { return ctx->device; }
void* ctx_stream(const eegfx_ctx* ctx) { return (void*)ctx->stream; }
}  // namespace eegfx

// The entries that carry epochs exist for two element types (double[n][C][750], the reference's
// interface, and float[n][C][750], the fp32 values it widens): one implementation each, templated
// on the element type E, behind the extern "C" pairs that follow.
namespace {

// Host batches up to this many window bytes go through the zero-copy path of
// eegfx_extract_features_f64 (about 64 epochs of 3 channels).
constexpr size_t kZeroCopyBytes = (size_t)768 << 10;
// the rows of the largest such batch: 192 window rows of 512 doubles, 16 features each
constexpr size_t kZeroCopyOutBytes =
    kZeroCopyBytes / (sizeof(double) * EEGFX_DWT8_EPOCH_SIZE) * EEGFX_DWT8_FEATURE_SIZE * sizeof(double);

// The front door of the raw-recording entries.  The order of the checks is part of the interface
// (tests/test_gpu_api_errors.py): null context, mem flag, format, sizes, null buffers
// (check_raw_head), then the channel selection: C, null cols / res, each column.  `out`: the
// buffer the entry requires when n > 0.
ChanSel check_raw_args(const eegfx_ctx* ctx, int mem, const void* raw, int fmt, int64_t n_frames,
                       int ct, const int32_t* cols, const float* res, int C, const int64_t* pos,
                       int64_t n, const void* out) {
  check_raw_head(ctx, mem, raw, fmt, n_frames, ct, pos, n, out);
  return make_sel(cols, res, C, ct);
}

// ... and its second half, after any check of the entry's own: host positions are checked (device
// ones by the kernels, ctx.h check_positions_flag), no epochs is no work (false), then the
// recording and the positions as the kernels read them.
struct RawIn {
  const void* raw;
  const int64_t* pos;
};
bool stage_raw(eegfx_ctx* ctx, const void* raw, const int64_t* pos, int64_t n, int64_t n_frames,
               int ct, int fmt, int mem, RawIn* in) {
  if (mem == EEGFX_MEM_HOST) check_positions(pos, n, n_frames);
  if (n == 0) return false;
  ctx->activate();
  const size_t raw_bytes = (size_t)n_frames * ct * (fmt == EEGFX_INT_16 ? 2 : 4);
  in->raw = stage_in(ctx, ctx->raw, raw, raw_bytes, mem);
  in->pos = stage_in(ctx, ctx->pos, pos, sizeof(int64_t) * n, mem);
  return true;
}

// eegfx_cut_epochs_f64 / _f32: E is the element type of epochs_out.
template <typename E>
int cut_epochs_api(eegfx_ctx* ctx, const void* raw, int32_t fmt, int64_t n_frames, int32_t ct,
                   const int32_t* cols, const float* res, int32_t C, const int64_t* pos, int64_t n,
                   E* epochs_out, int mem) {
  return guarded([&] {
    const ChanSel sel = check_raw_args(ctx, mem, raw, fmt, n_frames, ct, cols, res, C, pos, n,
                                       epochs_out);
    RawIn in;
    if (!stage_raw(ctx, raw, pos, n, n_frames, ct, fmt, mem, &in)) return;
    const size_t out_bytes = sizeof(E) * (size_t)n * C * EEGFX_POSTSTIMULUS;
    E* d_out = dev_out(ctx->out, epochs_out, out_bytes, mem);
    ctx->tic();
    HIP_CHECK(launch_cut_epochs(ctx->stream, in.raw, fmt, n_frames, ct, sel, C, in.pos, n, d_out,
                                ctx->fused.get(fused_scratch_bytes(n, C)), ctx->err_dev));
    ctx->toc(0);
    copy_out(ctx, epochs_out, d_out, out_bytes, mem);
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
        // under both numerics (small.hip small_epoch), so the fma guard does not count them.
        ctx->mb.stop_before_growth((size_t)n * C * row_w, out_bytes);
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
        if (n == 1 && ctx->mb.ready()) {
          ctx->mb.serve(n, C, feature_size);
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
      // one guard for the whole call, not one per chunk
      const Guard g =
          wide_features(feature_size) ? Guard{nullptr, nullptr, nullptr} : ctx->guard_for(n);
      ctx->tic();
      for (int64_t e0 = 0; e0 < n; e0 += kChunk) {
        const int64_t m = std::min<int64_t>(kChunk, n - e0);
        HIP_CHECK(hipMemcpy2DAsync(dwin, row_c, src + (size_t)e0 * C * row_p, row_p, row_c,
                                   (size_t)(m * C), hipMemcpyHostToDevice, ctx->stream));
        run_features_from_epochs(ctx, (const E*)dwin, m, C, 0, feature_size,
                                 d_out + e0 * C * feature_size, EEGFX_DWT8_EPOCH_SIZE, &g);
      }
      ctx->toc(0);
      copy_out(ctx, out, d_out, out_bytes, EEGFX_MEM_HOST);
      return;
    }
    ctx->tic();  // device epochs, device rows
    run_features_from_epochs(ctx, epochs, n, C, skip, feature_size, out, EEGFX_POSTSTIMULUS);
    ctx->toc(0);
  });
}

// eegfx_process_recording_epochs / _f32; without epochs_out they are eegfx_process_recording.
template <typename E>
int process_recording_epochs_api(eegfx_ctx* ctx, const void* raw, int32_t fmt, int64_t n_frames,
                                 int32_t ct, const int32_t* cols, const float* res, int32_t C,
                                 const int64_t* pos, int64_t n, double* features, E* epochs_out,
                                 int mem) {
  if (!epochs_out)
    return eegfx_process_recording(ctx, raw, fmt, n_frames, ct, cols, res, C, pos, n, features,
                                   mem);
  return guarded([&] {
    const ChanSel sel = check_raw_args(ctx, mem, raw, fmt, n_frames, ct, cols, res, C, pos, n,
                                       features);
    RawIn in;
    if (!stage_raw(ctx, raw, pos, n, n_frames, ct, fmt, mem, &in)) return;
    const size_t ep_bytes = sizeof(E) * (size_t)n * C * EEGFX_POSTSTIMULUS;
    const size_t f_bytes = sizeof(double) * (size_t)n * C * EEGFX_DWT8_FEATURE_SIZE;
    E* d_ep = dev_out(ctx->scratch, epochs_out, ep_bytes, mem);
    double* d_f = dev_out(ctx->out, features, f_bytes, mem);
    run_epochs_and_features(ctx, in.raw, fmt, n_frames, ct, sel, C, in.pos, n, d_ep, d_f);
    copy_back(ctx, epochs_out, d_ep, ep_bytes, mem);  // both copies ahead of copy_out's one drain
    copy_out(ctx, features, d_f, f_bytes, mem);
  });
}

}  // namespace

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
    if (!enable) return ctx->mb.release();
    if (ctx->mb.enabled()) return;
    // the small-call staging at its largest before any server is launched on it: a server reads
    // the buffers it was launched with, so growing them on a later call stopped and restarted it
    // (with a pinned allocation: the 3-4 ms first calls of tools/mailbox_threads at 16-32 threads)
    (void)ctx->pin_in.get(kZeroCopyBytes);
    (void)ctx->pin_out.get(kZeroCopyOutBytes);
    ctx->mb.on = true;  // the server starts on the first one-epoch call that gets a slot
    (void)ctx->mb.ready();
  });
}

int eegfx_ctx_get_mailbox(eegfx_ctx* ctx, int32_t* enabled, int32_t* resident) {
  return guarded([&] {
    if (!ctx) fail(EEGFX_EINVAL, "null context");
    if (enabled) *enabled = ctx->mb.enabled() ? 1 : 0;
    if (resident) *resident = ctx->mb.resident() ? 1 : 0;
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
    ctx->mb.release();  // before anything that synchronises the whole device
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
    const ChanSel sel = check_raw_args(ctx, mem, raw, fmt, n_frames, ct, cols, res, C, pos, n,
                                       features);
    RawIn in;
    if (!stage_raw(ctx, raw, pos, n, n_frames, ct, fmt, mem, &in)) return;
    const size_t out_bytes = sizeof(double) * (size_t)n * C * EEGFX_DWT8_FEATURE_SIZE;
    double* d_out = dev_out(ctx->out, features, out_bytes, mem);
    run_features_from_raw(ctx, in.raw, fmt, n_frames, ct, sel, C, in.pos, n, d_out);
    copy_out(ctx, features, d_out, out_bytes, mem);
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
    const ChanSel sel = check_raw_args(ctx, mem, raw, fmt, n_frames, ct, cols, res, C, pos, n,
                                       features);
    check_fe_params(C, name, epoch_size, skip, feature_size);
    RawIn in;
    if (!stage_raw(ctx, raw, pos, n, n_frames, ct, fmt, mem, &in)) return;
    const size_t out_bytes = sizeof(double) * (size_t)n * C * feature_size;
    double* d_out = dev_out(ctx->out, features, out_bytes, mem);
    // The two passes: the epochs into scratch memory, then the rows from them.  (A fused raw ->
    // rows pyramid kernel measured slower than this at feature size 512: DESIGN.md 5.4.1.)
    // The scratch epochs are float32: the fp32 samples as the cut holds them (3,000 C bytes per
    // epoch), widened again by the kernels that read them -- the rows are those of double scratch.
    float* ep = (float*)ctx->scratch.get(sizeof(float) * (size_t)n * C * EEGFX_POSTSTIMULUS);
    ctx->tic();
    HIP_CHECK(launch_cut_epochs(ctx->stream, in.raw, fmt, n_frames, ct, sel, C, in.pos, n, ep,
                                ctx->fused.get(fused_scratch_bytes(n, C)), ctx->err_dev));
    run_features_from_epochs(ctx, ep, n, C, skip, feature_size, d_out, EEGFX_POSTSTIMULUS);
    ctx->toc(0);
    copy_out(ctx, features, d_out, out_bytes, mem);
  });
}

int eegfx_process_recording_epochs(eegfx_ctx* ctx, const void* raw, int32_t fmt, int64_t n_frames,
                                   int32_t ct, const int32_t* cols, const float* res, int32_t C,
                                   const int64_t* pos, int64_t n, double* features,
                                   double* epochs_out, int mem) {
  return process_recording_epochs_api(ctx, raw, fmt, n_frames, ct, cols, res, C, pos, n, features,
                                      epochs_out, mem);
}

int eegfx_process_recording_epochs_f32(eegfx_ctx* ctx, const void* raw, int32_t fmt,
                                       int64_t n_frames, int32_t ct, const int32_t* cols,
                                       const float* res, int32_t C, const int64_t* pos, int64_t n,
                                       double* features, float* epochs_out, int mem) {
  return process_recording_epochs_api(ctx, raw, fmt, n_frames, ct, cols, res, C, pos, n, features,
                                      epochs_out, mem);
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
    const int64_t* d_pos = stage_in(ctx, ctx->pos, positions, sizeof(int64_t) * n, mem);
    const int32_t* d_stim = stage_in(ctx, ctx->row_vals, stimulus_index, sizeof(int32_t) * n, mem);
    // a host caller's two outputs share one allocation, pos_out[n] then label_out[n]; null for a
    // device caller, whose buffers are written in place
    uint8_t* o = dev_out<uint8_t>(ctx->out, nullptr, (sizeof(int64_t) + sizeof(double)) * (size_t)n,
                                  mem);
    int64_t* d_pos_out = o && pos_out ? (int64_t*)o : pos_out;
    double* d_label = o && label_out ? (double*)(o + sizeof(int64_t) * (size_t)n) : label_out;
    void* scratch = ctx->scratch.get(plan_scratch_bytes(n));
    PlanResult r;
    HIP_CHECK(launch_plan_markers(ctx->stream, d_pos, d_stim, n, n_frames, guessed,
                                  (int)*balance, scratch, d_pos_out, d_label, &r));
    if (pos_out) copy_back(ctx, pos_out, d_pos_out, sizeof(int64_t) * (size_t)r.selected, mem);
    if (label_out) copy_back(ctx, label_out, d_label, sizeof(double) * (size_t)r.selected, mem);
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
