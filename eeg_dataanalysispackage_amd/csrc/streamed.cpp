// streamed.cpp -- eegfx_process_recording_streamed: a long host recording through a ring of device
// chunk buffers (BASELINE.json configs[4]).
#include <algorithm>
#include <cstring>
#include <thread>
#include <vector>

#include "ctx.h"

// Host copy into pinned staging, split over up to 8 threads (one thread tops out near 6 GB/s,
// far below the ~57 GB/s host link it feeds).
static void parallel_memcpy(void* dst, const void* src, size_t bytes) {
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

}  // extern "C"
