// streamed.cpp -- eegfx_process_recording_streamed: a long host recording through a ring of device
// chunk buffers (BASELINE.json configs[4]).
#include <algorithm>
#include <cstring>
#include <vector>

#include "ctx.h"
#include "stream_plan.h"

extern "C" {

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
    // the raw entries' ladder (api.cpp), with the chunk size checked ahead of the selection
    check_raw_head(ctx, EEGFX_MEM_HOST, raw, fmt, n_frames, ct, pos, n, features);
    constexpr int64_t kSpan = kStreamSpan;  // 787
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
    // the chunks, and one buffer size for all of them (stream_plan.h; a chunk_frames beyond what
    // the recording can use gives one chunk, sized by the recording)
    const std::vector<StreamChunk> plan = stream_plan(spos, n, n_frames, chunk_frames);
    const size_t cbytes = stream_buffer_bytes(plan, FB);
    // A ring of 4 device chunk buffers (fewer for fewer chunks).  One buffer per chunk (the whole
    // 346 MB recording in HBM, no upload ever waiting for an earlier chunk's kernels) measured the
    // same: 7.16-7.18 against 7.13-7.18 ms (profiles/r06/stream_ring_ab.log).
    const size_t R = stream_ring(plan.size());
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
        const size_t b = stream_slot(k, R), st = stream_staging(k);
        const int64_t i = plan[k].i, j = plan[k].j, hi = plan[k].hi;
        const StreamBytes cb = stream_chunk_bytes(plan[k], FB);
        const int64_t Lb = cb.Lb;
        const size_t bytes = cb.bytes;
        uint8_t* dst = dbuf + (size_t)b * cbytes + 64;
        if (k >= R) HIP_CHECK(hipStreamWaitEvent(cs, done[b], 0));  // kernels of chunk k-R done
        const uint8_t* src = (const uint8_t*)raw + Lb;
        if (!pinned) {  // two pinned staging buffers: staging k % 2 is free once chunk k-2 uploaded
          if (k >= 2) HIP_CHECK(hipEventSynchronize(copied[(k - 2) % R]));
          if (bytes) parallel_memcpy(pin[st], src, bytes);
          src = (const uint8_t*)pin[st];
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

}  // extern "C"
