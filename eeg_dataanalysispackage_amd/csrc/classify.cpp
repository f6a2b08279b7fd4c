// classify.cpp -- the one-context MLlib classifier entries of the eegfx C ABI (eegfx_logreg_*,
// eegfx_svm_*, eegfx_spark_sample): the trainers' front door to the one SGD driver
// (sharded.cpp glm_sgd_train_shards), whose argument checks and mini-batch masks live here, and the
// predict driver over the kernels of logreg.hip.
#include <sched.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <thread>
#include <vector>

#include "ctx.h"
#include "spark_sample.h"

// The processors this process may run on, as the JVM's Runtime.availableProcessors() counts them
// (Spark local[*]'s defaultParallelism, SparkInitializer.java:44): the affinity mask, capped by a
// cgroup CPU quota (cgroup v2 cpu.max or v1 cfs_quota_us / cfs_period_us), at least 1.
// std::thread::hardware_concurrency() counts every online CPU of the machine instead.
int eegfx::available_processors() {
  int n = 0;
  cpu_set_t set;
  if (sched_getaffinity(0, sizeof(set), &set) == 0) n = CPU_COUNT(&set);
  if (n < 1) n = (int)std::max(1u, std::thread::hardware_concurrency());
  auto cap = [&](double quota, double period) {
    if (quota > 0 && period > 0) n = std::min(n, std::max(1, (int)std::ceil(quota / period)));
  };
  if (FILE* f = fopen("/sys/fs/cgroup/cpu.max", "r")) {
    char q[32] = {0};
    double period = 0;
    if (fscanf(f, "%31s %lf", q, &period) == 2 && strcmp(q, "max") != 0) cap(atof(q), period);
    fclose(f);
  } else if (FILE* fq = fopen("/sys/fs/cgroup/cpu/cpu.cfs_quota_us", "r")) {
    double quota = -1, period = 0;
    if (fscanf(fq, "%lf", &quota) != 1) quota = -1;
    fclose(fq);
    if (FILE* fp = fopen("/sys/fs/cgroup/cpu/cpu.cfs_period_us", "r")) {
      if (fscanf(fp, "%lf", &period) != 1) period = 0;
      fclose(fp);
    }
    cap(quota, period);
  }
  return n;
}

bool eegfx::check_sgd_args(int grad, int32_t d, int32_t num_iterations, double mini_batch_fraction,
                           int32_t num_partitions) {
  check_train_d(d);
  if (num_iterations < 0) fail(EEGFX_EINVAL, "num_iterations %d", num_iterations);
  // RDD.sample's require(fraction >= 0.0), then BernoulliSampler's upper bound 1 up to
  // RandomSampler.roundingEpsilon
  if (!(mini_batch_fraction >= 0.0))
    fail(EEGFX_EINVAL, "Negative fraction value: %g", mini_batch_fraction);
  if (!(mini_batch_fraction <= 1.0 + 1e-6))
    fail(EEGFX_EINVAL, "Sampling fraction (%g) must be on interval [0, 1]", mini_batch_fraction);
  const bool sampled = mini_batch_fraction < 1.0;
  if (sampled && grad != kGradLogistic)
    fail(EEGFX_ENOTSUP, "miniBatchFraction %g: the SVM loop is full-batch only",
         mini_batch_fraction);
  if (sampled && num_partitions < 1) fail(EEGFX_EINVAL, "num_partitions %d", num_partitions);
  return sampled;
}

// the masks of up to ~256 MB of iterations at a time
int eegfx::sgd_mask_chunk(int64_t n, int num_iterations) {
  const int64_t words = (n + 31) / 32;
  return (int)std::max<int64_t>(1, std::min<int64_t>(num_iterations, ((int64_t)64 << 20) / words));
}

// drawn by threads over iterations
void eegfx::draw_sgd_masks(int64_t n, double fraction, int num_partitions, int i0, int k,
                           uint32_t* masks, int64_t* counts) {
  const int64_t words = (n + 31) / 32;
  const int T = std::max(1, std::min({k, 64, available_processors()}));
  Joiner pool;
  for (int t = 0; t < T; ++t)
    pool.th.emplace_back([=] {
      for (int j = t; j < k; j += T)  // GradientDescent's i = i0 + j + 1, seed 42 + i
        counts[j] = spark::sample_mask(n, fraction, num_partitions, 42 + (int64_t)(i0 + j + 1),
                                       &masks[(size_t)j * words]);
    });
}

// the classifier of LogisticRegressionClassifier.java:85-114 on the GPU
// (csrc/logreg.hip): MLlib 1.6.2 LogisticRegressionWithSGD.  miniBatchFraction < 1: iteration i
// trains on data.sample(false, f, 42 + i) of the rows in `num_partitions` ParallelCollectionRDD
// slices (spark_sample.h), drawn on the host (threads over iterations) as one bit mask per
// iteration and uploaded before the iterations that read them.  The hinge loop of
// eegfx_ext.h (SVMWithSGD) stays full-batch (outside the contract, not extended).
// The entry's own refusals, then the driver of sharded.cpp with the context as its one shard.
static int glm_sgd_train(int grad, eegfx_ctx* ctx, const double* X, const double* y, int64_t n,
                         int32_t d, int32_t num_iterations, double step_size, double reg_param,
                         double mini_batch_fraction, double convergence_tol,
                         int32_t num_partitions, double* weights, int32_t* iterations_run,
                         int mem) {
  const int refused = guarded([&] {
    if (!ctx || !weights) fail(EEGFX_EINVAL, "null argument");
    check_mem(mem);
    if (n < 1) fail(EEGFX_EINVAL, "empty training set");  // GeneralizedLinearAlgorithm: first()
    if (!X || !y) fail(EEGFX_EINVAL, "null X / y");
  });
  if (refused != EEGFX_OK) return refused;
  // the driver goes on with the ladder (check_sgd_args) and stages a host caller's rows behind it
  const eegfx_glm_shard one = {ctx, X, y, nullptr, n};
  return glm_sgd_train_shards(grad, &one, 1, d, num_iterations, step_size, reg_param,
                              mini_batch_fraction, convergence_tol, num_partitions, weights,
                              iterations_run, mem);
}

static int glm_predict(int grad, eegfx_ctx* ctx, const double* X, int64_t n, int32_t d,
                       const double* weights, double intercept, double threshold, double* out,
                       int mem) {
  return guarded([&] {
    if (!ctx || !weights) fail(EEGFX_EINVAL, "null argument");
    check_mem(mem);
    check_predict_dims(n, d);
    if (n == 0) return;
    if (!X || !out) fail(EEGFX_EINVAL, "null X / out");
    predict_frame(ctx, X, n, d, out, mem, [&](const double* dX, double* dout) {
      const size_t sbytes = sizeof(LrState) + sizeof(double) * (size_t)d;
      LrState* st = (LrState*)ctx->lr_state.get(sbytes);
      HIP_CHECK(hipMemcpyAsync(st->w, weights, sizeof(double) * (size_t)d, hipMemcpyHostToDevice,
                               ctx->stream));
      const bool use_t = !std::isnan(threshold);  // clearThreshold -> scores / margins
      HIP_CHECK(launch_lr_predict(ctx->stream, grad, dX, n, d, st->w, intercept, threshold,
                                  use_t ? 1 : 0, dout));
    });
  });
}

extern "C" {

int eegfx_logreg_sgd_train_partitioned(eegfx_ctx* ctx, const double* X, const double* y,
                                       int64_t n, int32_t d, int32_t num_iterations,
                                       double step_size, double reg_param,
                                       double mini_batch_fraction, double convergence_tol,
                                       int32_t num_partitions, double* weights,
                                       int32_t* iterations_run, int mem) {
  return glm_sgd_train(kGradLogistic, ctx, X, y, n, d, num_iterations, step_size, reg_param,
                       mini_batch_fraction, convergence_tol, num_partitions, weights,
                       iterations_run, mem);
}

int eegfx_logreg_sgd_train(eegfx_ctx* ctx, const double* X, const double* y, int64_t n, int32_t d,
                           int32_t num_iterations, double step_size, double reg_param,
                           double mini_batch_fraction, double convergence_tol, double* weights,
                           int32_t* iterations_run, int mem) {
  // Spark local[*] (SparkInitializer.java:44): defaultParallelism = the processors available
  // to the process (Runtime.availableProcessors(): affinity and cgroup quota honoured)
  return glm_sgd_train(kGradLogistic, ctx, X, y, n, d, num_iterations, step_size, reg_param,
                       mini_batch_fraction, convergence_tol, (int32_t)available_processors(),
                       weights, iterations_run, mem);
}

int eegfx_available_processors(void) { return available_processors(); }

int eegfx_spark_sample(int64_t n, double fraction, int32_t num_partitions, int64_t seed,
                       uint32_t* mask, int64_t* kept) {
  return guarded([&] {
    if (n < 0 || num_partitions < 1 || !mask || !kept) fail(EEGFX_EINVAL, "bad argument");
    if (!(fraction >= -1e-6 && fraction <= 1.0 + 1e-6))
      fail(EEGFX_EINVAL, "Sampling fraction (%g) must be on interval [0, 1]", fraction);
    *kept = spark::sample_mask(n, fraction, num_partitions, seed, mask);
  });
}

int eegfx_logreg_predict(eegfx_ctx* ctx, const double* X, int64_t n, int32_t d,
                         const double* weights, double intercept, double threshold, double* out,
                         int mem) {
  return glm_predict(kGradLogistic, ctx, X, n, d, weights, intercept, threshold, out, mem);
}

// The classifier of SVMClassifier.java:83-111 (MLlib 1.6.2 SVMWithSGD: HingeGradient, the same
// SquaredL2Updater / GradientDescent loop) and SVMModel.predict (:71, :114-137).
int eegfx_svm_sgd_train(eegfx_ctx* ctx, const double* X, const double* y, int64_t n, int32_t d,
                        int32_t num_iterations, double step_size, double reg_param,
                        double mini_batch_fraction, double convergence_tol, double* weights,
                        int32_t* iterations_run, int mem) {
  return glm_sgd_train(kGradHinge, ctx, X, y, n, d, num_iterations, step_size, reg_param,
                       mini_batch_fraction, convergence_tol, 1, weights, iterations_run, mem);
}

int eegfx_svm_predict(eegfx_ctx* ctx, const double* X, int64_t n, int32_t d, const double* weights,
                      double intercept, double threshold, double* out, int mem) {
  return glm_predict(kGradHinge, ctx, X, n, d, weights, intercept, threshold, out, mem);
}

}  // extern "C"
