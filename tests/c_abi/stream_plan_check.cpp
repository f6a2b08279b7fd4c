// The streamed entry's host arithmetic (csrc/stream_plan.h) on its own, for a sanitizer build
// (tests/test_stream_cases.py builds this with -fsanitize=address,undefined, runs it directly and
// compares its output with the Python restatement, tests/stream_cases.py).  Commands, one a line
// on stdin, every number decimal:
//   plan N_FRAMES FB CHUNK_FRAMES N P0 .. P(N-1)   sorted positions.  Prints
//       "plan chunks=K c=<chunk size used> cbytes=<buffer bytes> R=<ring>", then for each chunk
//       "chunk k i j lo hi Lb Hb bytes slot staging".
//   split BYTES HW      prints "split nt per", then "piece t a len" for every t < nt.
//   copy BYTES HW       runs parallel_memcpy between host buffers with 4,096 sentinel bytes on
//                       both sides of each and prints "copy ok" or what differs.
// The last line is "stream_plan_check ok".
#include <cinttypes>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "stream_plan.h"

using namespace eegfx;

static int64_t next_int(bool* ok) {
  long long v = 0;
  *ok = scanf("%lld", &v) == 1;
  return (int64_t)v;
}

static int64_t need_int() {
  bool ok;
  const int64_t v = next_int(&ok);
  if (!ok) {
    fprintf(stderr, "short input\n");
    exit(2);
  }
  return v;
}

static void run_plan() {
  const int64_t n_frames = need_int(), FB = need_int(), chunk_frames = need_int(), n = need_int();
  std::vector<int64_t> pos((size_t)n);
  for (auto& p : pos) p = need_int();
  const std::vector<StreamChunk> plan = stream_plan(pos.data(), n, n_frames, chunk_frames);
  const size_t cbytes = stream_buffer_bytes(plan, FB), R = stream_ring(plan.size());
  printf("plan chunks=%zu c=%" PRId64 " cbytes=%zu R=%zu\n", plan.size(),
         stream_chunk_frames(chunk_frames, n_frames), cbytes, R);
  for (size_t k = 0; k < plan.size(); ++k) {
    const StreamBytes b = stream_chunk_bytes(plan[k], FB);
    printf("chunk %zu %" PRId64 " %" PRId64 " %" PRId64 " %" PRId64 " %" PRId64 " %" PRId64
           " %zu %zu %zu\n",
           k, plan[k].i, plan[k].j, plan[k].lo, plan[k].hi, b.Lb, b.Hb, b.bytes,
           stream_slot(k, R), stream_staging(k));
  }
}

static void run_split() {
  const size_t bytes = (size_t)need_int();
  const unsigned hw = (unsigned)need_int();
  const CopySplit s = copy_split(bytes, hw);
  printf("split %zu %zu\n", s.nt, s.per);
  for (size_t t = 0; t < s.nt; ++t) {
    size_t a, len;
    copy_piece(s, bytes, t, &a, &len);
    printf("piece %zu %zu %zu\n", t, a, len);
  }
}

static void run_copy() {
  constexpr size_t kGuard = 4096;
  const size_t bytes = (size_t)need_int();
  const unsigned hw = (unsigned)need_int();
  std::vector<uint8_t> src(bytes + 2 * kGuard), dst(bytes + 2 * kGuard, 0xA5), want;
  uint64_t x = 0x9E3779B97F4A7C15ull ^ bytes;
  for (auto& b : src) {  // xorshift64: no byte pattern of a period the pieces could hide behind
    x ^= x << 13, x ^= x >> 7, x ^= x << 17;
    b = (uint8_t)(x >> 32);
  }
  want = dst;
  memcpy(want.data() + kGuard, src.data() + kGuard, bytes);
  const std::vector<uint8_t> src0 = src;
  parallel_memcpy(dst.data() + kGuard, src.data() + kGuard, bytes, hw);
  if (src != src0) {
    printf("copy %zu: the source changed\n", bytes);
    return;
  }
  for (size_t i = 0; i < dst.size(); ++i)
    if (dst[i] != want[i]) {
      printf("copy %zu: byte %lld differs (%s)\n", bytes, (long long)i - (long long)kGuard,
             i < kGuard || i >= kGuard + bytes ? "sentinel" : "payload");
      return;
    }
  printf("copy ok\n");
}

int main() {
  char cmd[16];
  while (scanf("%15s", cmd) == 1) {
    if (!strcmp(cmd, "plan")) {
      run_plan();
    } else if (!strcmp(cmd, "split")) {
      run_split();
    } else if (!strcmp(cmd, "copy")) {
      run_copy();
    } else {
      fprintf(stderr, "unknown command %s\n", cmd);
      return 2;
    }
  }
  printf("stream_plan_check ok\n");
  return 0;
}
