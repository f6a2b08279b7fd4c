// stream_plan.h -- the host arithmetic of eegfx_process_recording_streamed (streamed.cpp): which
// epochs and frames each chunk holds, the bytes it uploads, the size of a chunk buffer, the ring
// slot and the pinned staging of chunk k, and the split of the threaded host copy.  Host code only
// (no HIP): tests/c_abi/stream_plan_check.cpp runs it on the CPU under the sanitizers and
// tests/stream_cases.py restates it.
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <thread>
#include <vector>

#include "eegfx.h"

namespace eegfx {

// frames of one epoch in the recording: [pos - 100, pos + 687)
constexpr int64_t kStreamSpan = EEGFX_PRESTIMULUS + EEGFX_DWT8_SKIP + EEGFX_DWT8_EPOCH_SIZE;
constexpr size_t kStreamRing = 4;     // device chunk buffers
constexpr size_t kStreamStagings = 2; // pinned staging buffers of a pageable source

struct StreamChunk {
  int64_t i, j, lo, hi;  // epochs [i, j), frames [lo, hi)
};

// The chunk size the plan works with.  From 4 * n_frames up the first chunk (c/4) already reaches
// the recording's end, so every such value gives the same one-chunk plan: the caller's value is
// cut there, and no product below can wrap (n_frames frames are in memory, so 4 * n_frames * FB
// is far inside 64 bits).
inline int64_t stream_chunk_frames(int64_t chunk_frames, int64_t n_frames) {
  const int64_t cap = n_frames <= INT64_MAX / 4 ? std::max(4 * n_frames, kStreamSpan) : INT64_MAX;
  return std::min(chunk_frames, cap);
}

// Chunk sizes ramp up (c/4, c/2, then c) and down (about half of what remains, not below c/4) so
// that the first upload and the last download -- the parts of a call that nothing overlaps -- stay
// short.  `last`: the frame after the last epoch's span.
inline int64_t stream_chunk_at(int64_t k, int64_t lo, int64_t last, int64_t chunk_frames) {
  int64_t c = k < 2 ? chunk_frames >> (2 - k) : chunk_frames;
  const int64_t rest = last - lo;
  if (rest < 2 * chunk_frames) c = std::min(c, (rest + 1) / 2);
  return std::min(chunk_frames, std::max(c, std::max(chunk_frames / 4, 2 * kStreamSpan)));
}

// The chunks of n >= 1 sorted positions, each in [100, n_frames + 100].  A chunk starts at the
// first unprocessed epoch's baseline frame and takes the epochs whose span ends by its `hi` (all
// of them at the recording's end, where the kernels zero-pad).
inline std::vector<StreamChunk> stream_plan(const int64_t* spos, int64_t n, int64_t n_frames,
                                            int64_t chunk_frames) {
  chunk_frames = stream_chunk_frames(chunk_frames, n_frames);
  const int64_t last = spos[n - 1] - EEGFX_PRESTIMULUS + kStreamSpan;
  std::vector<StreamChunk> plan;
  for (int64_t i = 0; i < n;) {
    const int64_t lo = spos[i] - EEGFX_PRESTIMULUS;
    const int64_t hi =
        std::min(lo + stream_chunk_at((int64_t)plan.size(), lo, last, chunk_frames), n_frames);
    // a prefix of the sorted positions, found by bisection (a linear scan of configs[4]'s 576k
    // positions delayed the first upload by ~150 us)
    const int64_t j =
        hi == n_frames
            ? n
            : std::upper_bound(spos + i, spos + n, hi + EEGFX_PRESTIMULUS - kStreamSpan) - spos;
    plan.push_back({i, j, lo, hi});
    i = j;
  }
  return plan;
}

// The bytes [Lb, Hb) of the recording a chunk uploads: from the 16-byte floor of its first frame
// (the kernels read 16-byte quads) to the end of its last.
struct StreamBytes {
  int64_t Lb, Hb;
  size_t bytes;
};
inline StreamBytes stream_chunk_bytes(const StreamChunk& c, int64_t FB) {
  const int64_t Lb = (c.lo * FB) & ~(int64_t)15, Hb = c.hi * FB;
  return {Lb, Hb, Hb > Lb ? (size_t)(Hb - Lb) : 0};
}

// One chunk buffer: 64 B front pad (the kernels round the first quad down by < 16 B) + the
// plan's largest upload + 64 B, rounded to 256 B so that every buffer of the ring is as aligned as
// the first (the kernels read 16-byte quads relative to `raw`).
inline size_t stream_buffer_bytes(const std::vector<StreamChunk>& plan, int64_t FB) {
  size_t most = 0;
  for (const StreamChunk& c : plan) most = std::max(most, stream_chunk_bytes(c, FB).bytes);
  return (most + 128 + 255) & ~(size_t)255;
}

// A ring of 4 device chunk buffers (fewer for fewer chunks): chunk k uploads into slot k % R once
// the kernels of chunk k - R are done; a pageable source goes through staging k & 1, free once
// chunk k - 2 has been uploaded.
inline size_t stream_ring(size_t chunks) { return std::min(chunks, kStreamRing); }
inline size_t stream_slot(size_t k, size_t R) { return k % R; }
inline size_t stream_staging(size_t k) { return k % kStreamStagings; }

// Host copy into pinned staging, split over up to 8 threads (one thread tops out near 6 GB/s,
// far below the ~57 GB/s host link it feeds): a thread per whole 8 MB, pieces of `per` bytes
// (a multiple of 64), the last one shorter.  `per` comes from the quotient rounded up: rounded
// down, a byte count such as 16 MB + 1 over two threads lost its last byte (nt * per < bytes).
struct CopySplit {
  size_t nt, per;
};
inline CopySplit copy_split(size_t bytes, unsigned hw) {
  const size_t nt = std::min<size_t>({8, std::max(1u, hw), std::max<size_t>(1, bytes >> 23)});
  return {nt, nt <= 1 ? bytes : ((bytes + nt - 1) / nt + 63) & ~(size_t)63};
}
// piece t of the split: [a, a + len), len == 0 past the end
inline void copy_piece(CopySplit s, size_t bytes, size_t t, size_t* a, size_t* len) {
  *a = std::min(t * s.per, bytes);
  *len = std::min(s.per, bytes - *a);
}
inline void parallel_memcpy(void* dst, const void* src, size_t bytes,
                            unsigned hw = std::thread::hardware_concurrency()) {
  const CopySplit s = copy_split(bytes, hw);
  if (s.nt <= 1) {
    memcpy(dst, src, bytes);
    return;
  }
  std::vector<std::thread> th;
  for (size_t t = 0; t < s.nt; ++t) {
    size_t a, len;
    copy_piece(s, bytes, t, &a, &len);
    if (len == 0) break;
    th.emplace_back([=] { memcpy((char*)dst + a, (const char*)src + a, len); });
  }
  for (auto& x : th) x.join();
}

}  // namespace eegfx
