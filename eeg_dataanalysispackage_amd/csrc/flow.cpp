// flow.cpp -- the train/test flow's glue of the eegfx C ABI (eegfx_java_shuffle,
// eegfx_split_shard_plan, eegfx_gather_rows, eegfx_confusion_counts) over the kernels of flow.hip;
// eegfx_odp_split and eegfx_odp_split_sharded (odp.cpp) are built from the same pieces.  PipelineBuilder.java:170-223: shuffle both lists with
// Random(1), split 70/30, train, test, report four counters.
#include <cstring>
#include <vector>

#include "ctx.h"
#include "split_plan.h"

namespace eegfx {

namespace {

// java.util.Random: the 48-bit linear congruential generator of the JDK
struct JavaRandom {
  static constexpr uint64_t kMult = 0x5DEECE66DULL, kMask = (1ULL << 48) - 1;
  uint64_t seed;
  explicit JavaRandom(int64_t s) : seed(((uint64_t)s ^ kMult) & kMask) {}
  int32_t next31() {
    seed = (seed * kMult + 0xB) & kMask;
    return (int32_t)(seed >> 17);
  }
  int32_t next_int(int32_t bound) {  // bound > 0
    if ((bound & (bound - 1)) == 0) return (int32_t)(((int64_t)bound * next31()) >> 31);
    for (;;) {
      const int32_t bits = next31(), val = bits % bound;
      if ((int64_t)bits - val + (bound - 1) < ((int64_t)1 << 31)) return val;  // no int overflow
    }
  }
};

constexpr size_t kFlagBytes = 2 * sizeof(unsigned long long) + sizeof(ConfusionOut);

}  // namespace

std::vector<int64_t> java_shuffle(int64_t n, int64_t seed) {
  if (n < 0 || n >= ((int64_t)1 << 31))
    fail(EEGFX_EINVAL, "a list of %lld items (a Java list holds [0, 2^31))", (long long)n);
  std::vector<int64_t> perm((size_t)n);
  for (int64_t i = 0; i < n; ++i) perm[(size_t)i] = i;
  JavaRandom rnd(seed);
  for (int64_t i = n; i > 1; --i)  // Collections.shuffle: swap(list, i - 1, rnd.nextInt(i))
    std::swap(perm[(size_t)(i - 1)], perm[(size_t)rnd.next_int((int32_t)i)]);
  return perm;
}

void run_gather_rows(eegfx_ctx* ctx, const double* src, int64_t n_src, int d, const int64_t* idx,
                     int64_t m, double* dst, int slot) {
  unsigned long long* bad = (unsigned long long*)ctx->fl_flag.get(kFlagBytes) + slot;
  HIP_CHECK(hipMemsetAsync(bad, 0xFF, sizeof(*bad), ctx->stream));
  ctx->tic();
  HIP_CHECK(launch_gather_rows(ctx->stream, src, n_src, d, idx, m, dst, bad));
  ctx->toc(m * (2 * (int64_t)sizeof(double) * d + (int64_t)sizeof(int64_t)));
}

void gather_check(eegfx_ctx* ctx, int slots, int64_t n_src) {
  unsigned long long bad[2] = {~0ULL, ~0ULL};
  HIP_CHECK(hipMemcpyAsync(bad, ctx->fl_flag.get(kFlagBytes), sizeof(bad[0]) * (size_t)slots,
                           hipMemcpyDeviceToHost, ctx->stream));
  ctx->drain();
  for (int s = 0; s < slots; ++s)
    if (bad[s] != ~0ULL)
      fail(EEGFX_ERANGE, "idx[%llu] lies outside [0, %lld): that row was not copied", bad[s],
           (long long)n_src);
}

void confusion_verdict(const ConfusionOut& h, int64_t counts[4]) {
  if (h.seen & kSeenOther) fail(EEGFX_EINVAL, "%s", kBadLabels);
  // MulticlassMetrics' matrix has one row per actual class: with fewer than two the
  // reference's cm[1] throws (LogisticRegressionClassifier.java:131)
  if (h.seen != (kSeenZero | kSeenOne))
    fail(EEGFX_ERANGE, "Index 1 out of bounds for length %d: the labels hold %s",
         h.seen ? 1 : 0, h.seen ? "one class" : "no class");
  for (int k = 0; k < 4; ++k) counts[k] = (int64_t)h.cell[k];
}

}  // namespace eegfx

extern "C" {

int eegfx_java_shuffle(int64_t n, int64_t seed, int64_t* perm) {
  return guarded([&] {
    const std::vector<int64_t> p = java_shuffle(n, seed);
    if (n > 0 && !perm) fail(EEGFX_EINVAL, "null argument");
    if (n > 0) memcpy(perm, p.data(), sizeof(int64_t) * (size_t)n);
  });
}

int eegfx_split_shard_plan(int64_t n, int64_t first, int64_t count, int64_t seed,
                           double train_fraction, int64_t* idx, int64_t* pos, int64_t* n_train,
                           int64_t* n_test) {
  return guarded([&] {
    const std::vector<int64_t> perm = java_shuffle(n, seed);
    if (!n_train || !n_test) fail(EEGFX_EINVAL, "null argument");
    if (!(train_fraction >= 0.0 && train_fraction <= 1.0))
      fail(EEGFX_EINVAL, "train_fraction %g outside [0, 1]", train_fraction);
    if (first < 0 || count < 0 || first > n || count > n - first)
      fail(EEGFX_EINVAL, "rows [%lld, %lld + %lld) outside [0, %lld]", (long long)first,
           (long long)first, (long long)count, (long long)n);
    if (count > 0 && (!idx || !pos)) fail(EEGFX_EINVAL, "null idx / pos");
    const SplitShardPlan s = split_shard_plan(perm.data(), n, (int64_t)((double)n * train_fraction),
                                              first, count);
    *n_train = s.n_train;
    *n_test = s.n_test;
    if (count > 0) {
      memcpy(idx, s.idx.data(), sizeof(int64_t) * (size_t)count);
      memcpy(pos, s.pos.data(), sizeof(int64_t) * (size_t)count);
    }
  });
}

int eegfx_gather_rows(eegfx_ctx* ctx, const double* src, int64_t n_src, int32_t d,
                      const int64_t* idx, int64_t m, double* dst, int mem) {
  return guarded([&] {
    if (!ctx) fail(EEGFX_EINVAL, "null argument");
    check_mem(mem);
    if (d < 1 || d > kGatherMaxD) fail(EEGFX_EINVAL, "d=%d outside [1, %d]", d, kGatherMaxD);
    if (n_src < 0 || m < 0)
      fail(EEGFX_EINVAL, "n_src=%lld m=%lld", (long long)n_src, (long long)m);
    if (m == 0) return;
    if (!idx || !dst || (n_src > 0 && !src)) fail(EEGFX_EINVAL, "null src / idx / dst");
    ctx->activate();
    const size_t row = sizeof(double) * (size_t)d;
    const double* d_src = stage_in(ctx, ctx->fl_src, src, row * (size_t)n_src, mem);
    const int64_t* d_idx = stage_in(ctx, ctx->fl_idx, idx, sizeof(int64_t) * (size_t)m, mem);
    // dst goes up too: the rows of bad indices keep what the caller's buffer holds
    double* d_dst = stage_in(ctx, ctx->fl_dst, dst, row * (size_t)m, mem);
    run_gather_rows(ctx, d_src, n_src, d, d_idx, m, d_dst, 0);
    copy_back(ctx, dst, d_dst, row * (size_t)m, mem);
    gather_check(ctx, 1, n_src);  // drains for both memory kinds
  });
}

int eegfx_confusion_counts(eegfx_ctx* ctx, const double* pred, const double* labels, int64_t n,
                           int64_t counts[4], int mem) {
  return guarded([&] {
    if (!ctx || !counts) fail(EEGFX_EINVAL, "null argument");
    check_mem(mem);
    if (n < 0) fail(EEGFX_EINVAL, "n=%lld", (long long)n);
    if (n > 0 && (!pred || !labels)) fail(EEGFX_EINVAL, "null pred / labels");
    ConfusionOut h;
    memset(&h, 0, sizeof(h));
    if (n > 0) {
      ctx->activate();
      const size_t bytes = sizeof(double) * (size_t)n;
      const double* d_pred = stage_in(ctx, ctx->fl_src, pred, bytes, mem);
      const double* d_lab = stage_in(ctx, ctx->fl_lab, labels, bytes, mem);
      ConfusionOut* out =
          (ConfusionOut*)((unsigned long long*)ctx->fl_flag.get(kFlagBytes) + 2);
      HIP_CHECK(hipMemsetAsync(out, 0, sizeof(*out), ctx->stream));
      HIP_CHECK(launch_confusion(ctx->stream, d_pred, d_lab, n, out));
      HIP_CHECK(hipMemcpyAsync(&h, out, sizeof(h), hipMemcpyDeviceToHost, ctx->stream));
      ctx->drain();
    }
    confusion_verdict(h, counts);
  });
}

}  // extern "C"
