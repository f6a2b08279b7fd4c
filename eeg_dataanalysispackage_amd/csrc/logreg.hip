// logreg.hip -- the classifier the reference trains on the feature matrix, on the GPU
// (SURVEY.md 8f rank 4): Spark MLlib 1.6.2 LogisticRegressionWithSGD as called by
// Classification/LogisticRegressionClassifier.java:85-114, i.e. gradient descent with
// LogisticGradient, SquaredL2Updater and GradientDescent's convergence test, no intercept, over
// the whole batch or (miniBatchFraction < 1) over the rows of iteration i's sample, a bit mask
// the host draws with Spark's own sampler (api.cpp spark_sample_mask); and
// LogisticRegressionModel.predict for :117-141.
//
// One iteration = two launches on the context stream, no host round trip:
//   lr_grad_kernel    G workgroups x 4 waves.  Row r goes to wave r mod (4G); a wave's 64 lanes
//                     split the d features (lane k: features k, k+64, ...), so a row is one
//                     coalesced load; margin by a wave butterfly, multiplier = 1/(1+exp(-w.x)) - y,
//                     per-lane gradient accumulators.  The 4 waves of a workgroup are summed in LDS
//                     in wave order and the workgroup's partial gradient stored.
//   lr_update_kernel  one workgroup: partials summed in workgroup order (deterministic), / n, the
//                     SquaredL2Updater step with step/sqrt(i), ||w_prev - w|| < tol*max(||w||, 1)
//                     sets the converged flag (from the second iteration, as GradientDescent).
// Every kernel first reads the flag, so the remaining iterations of a converged run are empty
// launches.  Weights and the iteration state stay in device memory for the whole run.
//
// Over several shards (sharded.cpp) each shard runs the gradient kernel
// on its rows and lr_fold_kernel sums its partials into one d-vector -- the loop lr_update_kernel
// sums with, lr_fold_partials -- which the root's lr_update_kernel reads as one partial per shard.
// lr_count_kernel is the test half: lr_predict_kernel's score met with the label in the cells of
// flow.hip's confusion_kernel, no prediction stored.
//
// The same loop with HingeGradient is MLlib 1.6.2 SVMWithSGD (Classification/SVMClassifier.java:
// 83-111: same updater, convergence test and defaults), scored by SVMModel.predict (:71, :114-137):
// the gradient kernels take the gradient as a template parameter (grad_mult).
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdlib>

#include "launch.h"

namespace eegfx {
namespace dev {

constexpr int kLrWaves = 4;
#ifndef EEGFX_LR_UNROLL
#define EEGFX_LR_UNROLL 4
#endif

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

// Gradient multiplier of one row (the gradient is mult * x).  GRAD 0 = LogisticGradient (binary):
// 1/(1+exp(-w.x)) - y.  GRAD 1 = HingeGradient (SVMWithSGD): with s = 2y - 1, -s when 1 > s * w.x,
// else 0 (the row adds nothing, as MLlib's axpy is skipped).
template <int GRAD>
__device__ __forceinline__ double grad_mult(double margin, double y) {
  if constexpr (GRAD == 0) {
    return 1.0 / (1.0 + exp(-margin)) - y;
  } else {
    const double s = 2.0 * y - 1.0;
    return 1.0 > s * margin ? -s : 0.0;
  }
}

// acc + mult * x, one row's term of the gradient.  HingeGradient runs its axpy only for a row
// inside the hinge: any other row -- one whose margin is NaN included, since 1 > NaN is false --
// has multiplier 0 and leaves the sum as it is, whatever the row holds (0 * NaN would be NaN).
// LogisticGradient multiplies every row; its multiplier is never an exact 0 for a non-finite
// margin, and it keeps the plain fma.
template <int GRAD>
__device__ __forceinline__ double axpy_row(double mult, double x, double acc) {
  if constexpr (GRAD == 0) {
    return __builtin_fma(mult, x, acc);
  } else {
    return mult != 0.0 ? __builtin_fma(mult, x, acc) : acc;
  }
}

// Row r of iteration's sample (mask == nullptr: every row).  POS: the rows are a shard of a longer
// list (eegfx_glm_sgd_train_sharded) and the row's bit is pos[r], not r: a flag of the kernel, so
// that the instances the one-context entries launch are the code they were without it.
template <bool POS>
__device__ __forceinline__ bool sampled(const uint32_t* __restrict__ mask,
                                        const int64_t* __restrict__ pos, int64_t r) {
  if constexpr (POS) {
    const int64_t b = pos[r];
    return (mask[b >> 5] >> (b & 31)) & 1u;
  } else {
    return !mask || ((mask[r >> 5] >> (r & 31)) & 1u);
  }
}

template <int KD, int GRAD, bool POS>  // features per lane: d <= 64 * KD
__global__ __launch_bounds__(64 * kLrWaves) void lr_grad_kernel(
    const double* __restrict__ X, const double* __restrict__ y, int64_t n, int d,
    const uint32_t* __restrict__ mask, const int64_t* __restrict__ pos,
    const LrState* __restrict__ st, double* __restrict__ partial) {
  if (st->converged) return;
  __shared__ double acc_s[kLrWaves][64 * KD];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const double* wt = st->w;
  double wv[KD], acc[KD];
#pragma unroll
  for (int k = 0; k < KD; ++k) {
    const int f = lane + 64 * k;
    wv[k] = f < d ? wt[f] : 0.0;
    acc[k] = 0.0;
  }
  const int64_t stride = (int64_t)gridDim.x * kLrWaves;
  for (int64_t r = (int64_t)blockIdx.x * kLrWaves + w; r < n; r += stride) {
    if (!sampled<POS>(mask, pos, r)) continue;  // wave-uniform: one row per wave
    const double* row = X + r * d;
    double x[KD];
    double dot = 0.0;
#pragma unroll
    for (int k = 0; k < KD; ++k) {
      const int f = lane + 64 * k;
      x[k] = f < d ? row[f] : 0.0;
      dot = __builtin_fma(x[k], wv[k], dot);
    }
    dot = wave_sum(dot);
    const double mult = grad_mult<GRAD>(dot, y[r]);
#pragma unroll
    for (int k = 0; k < KD; ++k) acc[k] = axpy_row<GRAD>(mult, x[k], acc[k]);
  }
#pragma unroll
  for (int k = 0; k < KD; ++k) acc_s[w][lane + 64 * k] = acc[k];
  __syncthreads();
  for (int f = threadIdx.x; f < d; f += blockDim.x) {
    double s = acc_s[0][f];
#pragma unroll
    for (int v = 1; v < kLrWaves; ++v) s += acc_s[v][f];
    partial[(int64_t)blockIdx.x * d + f] = s;
  }
}

// Cross-lane move of a double by DPP (two 32-bit halves); all 64 lanes active.
template <int CTRL>
__device__ __forceinline__ double dpp_d(double v) {
  const uint64_t u = __builtin_bit_cast(uint64_t, v);
  const int lo = __builtin_amdgcn_update_dpp(0, (int)(uint32_t)u, CTRL, 0xF, 0xF, false);
  const int hi = __builtin_amdgcn_update_dpp(0, (int)(uint32_t)(u >> 32), CTRL, 0xF, 0xF, false);
  return __builtin_bit_cast(double, ((uint64_t)(uint32_t)hi << 32) | (uint32_t)lo);
}
// Sum over the 16 lanes of a DPP row, result in every lane of the row: quad_perm xor 1, xor 2,
// then row_half_mirror and row_mirror pair the quads and the halves (4 VALU steps, no LDS).
__device__ __forceinline__ double row16_sum(double v) {
  v += dpp_d<0xB1>(v);
  v += dpp_d<0x4E>(v);
  v += dpp_d<0x141>(v);
  v += dpp_d<0x140>(v);
  return v;
}

// d <= 16*FPL: a row is owned by the 16 lanes of one DPP row (lane j: features j, j+16, ...), so
// a wave works on 4 rows at once, two such groups in flight.
template <int FPL, int GRAD, bool POS>
__global__ __launch_bounds__(64 * kLrWaves) void lr_grad16_kernel(
    const double* __restrict__ X, const double* __restrict__ y, int64_t n, int d,
    const uint32_t* __restrict__ mask, const int64_t* __restrict__ pos,
    const LrState* __restrict__ st, double* __restrict__ partial) {
  if (st->converged) return;
  __shared__ double acc_s[kLrWaves * 4][16 * FPL];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int q = lane >> 4, j = lane & 15;
  double wv[FPL], acc[FPL];
#pragma unroll
  for (int k = 0; k < FPL; ++k) {
    const int f = j + 16 * k;
    wv[k] = f < d ? st->w[f] : 0.0;
    acc[k] = 0.0;
  }
  constexpr int U = EEGFX_LR_UNROLL;  // groups of 4 rows in flight per wave
  const int64_t stride = (int64_t)gridDim.x * kLrWaves * 4 * U;
  for (int64_t r0 = ((int64_t)blockIdx.x * kLrWaves + w) * 4 * U; r0 < n; r0 += stride) {
    double x[U][FPL], dot[U], yy[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      // unconditional loads from clamped addresses (no exec-mask branch around a load, so all
      // U x FPL loads of the group issue before the first wait).  A row past n re-reads row
      // n-1 and gets multiplier 0; a feature slot past d re-reads feature d-1, meets weight 0
      // and is never stored.  With finite data both add exact zeros.  A re-read NaN or Inf
      // would not (0 * NaN = NaN): it makes the margin of its row non-finite, and a wave that
      // sees such a margin redoes its group the careful way below.
      // (Measured per gradient: hinge 0.114 -> 0.082 ms per iteration on 1M x 48; logistic,
      // whose exp the compiler already schedules the guarded loads around, keeps the guarded
      // form: 0.087 vs 0.090 ms.  Taking the U margins before the first fma of the group, as
      // the test below needs: hinge 0.085 -> 0.081 ms, profiles/logreg_shapes/.)
      const int64_t r = r0 + 4 * u + q;
      dot[u] = 0.0;
      if constexpr (GRAD == 0) {
        const bool ok = r < n && sampled<POS>(mask, pos, r);
        const double* row = X + (ok ? r : 0) * d;
#pragma unroll
        for (int k = 0; k < FPL; ++k) {
          const int f = j + 16 * k;
          x[u][k] = (ok && f < d) ? row[f] : 0.0;
          dot[u] = __builtin_fma(x[u][k], wv[k], dot[u]);
        }
        yy[u] = ok ? y[r] : 0.0;
      } else {
        const double* row = X + (r < n ? r : n - 1) * d;
#pragma unroll
        for (int k = 0; k < FPL; ++k) {
          const int f = j + 16 * k;
          x[u][k] = row[f < d ? f : d - 1];
          dot[u] = __builtin_fma(x[u][k], wv[k], dot[u]);
        }
        yy[u] = y[r < n ? r : n - 1];
      }
    }
    double mult[U], msum = 0.0;
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const double m = row16_sum(dot[u]);
      const bool ok = r0 + 4 * u + q < n && sampled<POS>(mask, pos, r0 + 4 * u + q);
      mult[u] = ok ? grad_mult<GRAD>(m, yy[u]) : 0.0;
      msum += m;  // non-finite as soon as one margin is
    }
    if constexpr (GRAD == 1) {
      // A finite margin means every value loaded for the row is finite -- the re-read ones
      // too, which met weight 0 -- and then fma(0, x, acc) == acc: the plain sums below are
      // MLlib's.  A wave holding a non-finite margin (wave-uniform, so row16_sum's DPP still
      // has all lanes) zeroes the slots past d, takes the margins again -- an Inf re-read for
      // a slot past d made Inf * 0 = NaN of a margin that may be +-Inf -- and skips the rows
      // with multiplier 0 as HingeGradient skips its axpy.
      if (__builtin_amdgcn_ballot_w64(!(__builtin_fabs(msum) <= __DBL_MAX__)) != 0) {
#pragma unroll
        for (int u = 0; u < U; ++u) {
          double dt = 0.0;
#pragma unroll
          for (int k = 0; k < FPL; ++k) {
            if (j + 16 * k >= d) x[u][k] = 0.0;
            dt = __builtin_fma(x[u][k], wv[k], dt);
          }
          const double m = row16_sum(dt);
          const bool ok = r0 + 4 * u + q < n && sampled<POS>(mask, pos, r0 + 4 * u + q);
          const double mu = ok ? grad_mult<GRAD>(m, yy[u]) : 0.0;
#pragma unroll
          for (int k = 0; k < FPL; ++k) acc[k] = axpy_row<GRAD>(mu, x[u][k], acc[k]);
        }
        continue;
      }
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
#pragma unroll
      for (int k = 0; k < FPL; ++k) acc[k] = __builtin_fma(mult[u], x[u][k], acc[k]);
    }
  }
#pragma unroll
  for (int k = 0; k < FPL; ++k) acc_s[w * 4 + q][j + 16 * k] = acc[k];
  __syncthreads();
  for (int f = threadIdx.x; f < d; f += blockDim.x) {
    double s = acc_s[0][f];
#pragma unroll
    for (int v = 1; v < kLrWaves * 4; ++v) s += acc_s[v][f];
    partial[(int64_t)blockIdx.x * d + f] = s;
  }
}

// The sum of G partial gradients [G][d], feature by feature, by one workgroup of 256 threads:
// thread (j, f) adds partials b = j, j+K, ... (K groups of d threads), then the K group sums are
// added in group order -- a fixed order, so runs are bit-reproducible.  each(f, g) receives the sum
// of feature f on the thread that owns it.  gs: 256 doubles of LDS.
template <typename Each>
__device__ __forceinline__ void lr_fold_partials(const double* __restrict__ partial, int G, int d,
                                                 double* gs, Each&& each) {
  const int K = d <= 128 ? (int)blockDim.x / d : 1;
  if (K > 1) {
    const int t = threadIdx.x, jj = t / d, f = t - jj * d;
    if (jj < K) {
      double a0 = 0.0, a1 = 0.0;
      int b = jj;
      for (; b + K < G; b += 2 * K) {
        a0 += partial[(int64_t)b * d + f];
        a1 += partial[(int64_t)(b + K) * d + f];
      }
      if (b < G) a0 += partial[(int64_t)b * d + f];
      gs[t] = a0 + a1;
    }
    __syncthreads();
  }
  for (int f = threadIdx.x; f < d; f += blockDim.x) {
    double g = 0.0;
    if (K > 1) {
      for (int jj = 0; jj < K; ++jj) g += gs[jj * d + f];
    } else {
      for (int b = 0; b < G; ++b) g += partial[(int64_t)b * d + f];
    }
    each(f, g);
  }
}

// A shard's G workgroup partials as one d-vector (eegfx_glm_sgd_train_sharded): the vector the
// root's lr_update_kernel then reads as one partial of its own.
__global__ __launch_bounds__(256) void lr_fold_kernel(const double* __restrict__ partial, int G,
                                                      int d, const LrState* __restrict__ st,
                                                      double* __restrict__ out) {
  if (st->converged) return;
  __shared__ double gs[256];
  lr_fold_partials(partial, G, d, gs, [&](int f, double g) { out[f] = g; });
}

__global__ __launch_bounds__(256) void lr_update_kernel(const double* __restrict__ partial, int G,
                                                        int64_t n, int d, double step_size,
                                                        double reg, double tol, int max_iter,
                                                        LrState* __restrict__ st) {
  if (st->converged) return;
  __shared__ double red[2][256];
  __shared__ double gs[256];
  const int it = st->iter + 1;
  const double step = step_size / sqrt((double)it);
  double diff2 = 0.0, norm2 = 0.0;
  lr_fold_partials(partial, G, d, gs, [&](int f, double g) {
    g = g / (double)n;
    const double old = st->w[f];
    double nw = old * (1.0 - step * reg);
    nw = nw + (-step) * g;
    st->w[f] = nw;
    diff2 += (old - nw) * (old - nw);
    norm2 += nw * nw;
  });
  red[0][threadIdx.x] = diff2;
  red[1][threadIdx.x] = norm2;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) {
      red[0][threadIdx.x] += red[0][threadIdx.x + s];
      red[1][threadIdx.x] += red[1][threadIdx.x + s];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    st->iter = it;
    const int up = st->updates + 1;
    st->updates = up;
    // GradientDescent.isConverged, checked once two updated iterates exist (with a full batch:
    // from iteration 2; an empty mini-batch updates nothing and tests nothing)
    const double diff = sqrt(red[0][0]), nrm = sqrt(red[1][0]);
    if ((up >= 2 && diff < tol * (nrm > 1.0 ? nrm : 1.0)) || it >= max_iter) st->converged = 1;
  }
}

// An iteration whose mini-batch sample is empty (GradientDescent: "The size of sampled batch is
// zero"): i advances, the weights and the convergence state do not.
__global__ void lr_skip_kernel(int max_iter, LrState* __restrict__ st) {
  if (st->converged || threadIdx.x != 0) return;
  st->iter += 1;
  if (st->iter >= max_iter) st->converged = 1;
}

// KIND 0: LogisticRegressionModel.predictPoint (score = sigmoid(w.x + b)); KIND 1:
// SVMModel.predictPoint (score = the margin w.x + b).  The score of row r, in every lane of the
// wave that computes it.
template <int KD, int KIND>
__device__ __forceinline__ double lr_score(const double* __restrict__ X, int64_t r, int d,
                                           const double* __restrict__ wt, double intercept,
                                           int lane) {
  double dot = 0.0;
#pragma unroll
  for (int k = 0; k < KD; ++k) {
    const int f = lane + 64 * k;
    if (f < d) dot = __builtin_fma(X[r * d + f], wt[f], dot);
  }
  dot = wave_sum(dot);
  const double margin = dot + intercept;
  return KIND == 0 ? 1.0 / (1.0 + exp(-margin)) : margin;
}
// What the model predicts from a score: score > threshold ? 1 : 0, or the score itself.
__device__ __forceinline__ double lr_decide(double score, double threshold, int use_threshold) {
  return use_threshold ? (score > threshold ? 1.0 : 0.0) : score;
}

template <int KD, int KIND>
__global__ __launch_bounds__(256) void lr_predict_kernel(const double* __restrict__ X, int64_t n,
                                                         int d, const double* __restrict__ wt,
                                                         double intercept, double threshold,
                                                         int use_threshold,
                                                         double* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= n) return;
  const double score = lr_score<KD, KIND>(X, r, d, wt, intercept, lane);
  if (lane == 0) out[r] = lr_decide(score, threshold, use_threshold);
}

// Score and count in one pass (eegfx_glm_count_sharded): row r of a trip goes to wave r mod (4 G),
// which scores it as lr_predict_kernel does; the prediction meets the row's label in the cells of
// confusion_kernel (flow.hip: tp, tn, "fp" = actual 1 / predicted 0, "fn"; a prediction that is
// neither 0.0 nor 1.0 is counted nowhere).  Every lane of a wave holds the wave's counts; the four
// waves are added in LDS and the workgroup adds its non-zero sums to out with one atomic each.
template <int KD, int KIND>
__global__ __launch_bounds__(256) void lr_count_kernel(const double* __restrict__ X,
                                                       const double* __restrict__ y, int64_t n,
                                                       int d, const double* __restrict__ wt,
                                                       double intercept, double threshold,
                                                       int use_threshold,
                                                       ConfusionOut* __restrict__ out) {
  __shared__ unsigned long long cell_s[4][4];
  __shared__ unsigned seen_s[4];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  unsigned long long cell[4] = {0, 0, 0, 0};
  unsigned seen = 0;
  const int64_t stride = (int64_t)gridDim.x * 4;
  for (int64_t r = (int64_t)blockIdx.x * 4 + w; r < n; r += stride) {
    const double p =
        lr_decide(lr_score<KD, KIND>(X, r, d, wt, intercept, lane), threshold, use_threshold);
    const double a = y[r];
    const bool a1 = a == 1.0, a0 = a == 0.0;
    seen |= a1 ? kSeenOne : a0 ? kSeenZero : kSeenOther;
    const bool p1 = p == 1.0, p0 = p == 0.0;
    cell[0] += a1 && p1;
    cell[1] += a0 && p0;
    cell[2] += a1 && p0;
    cell[3] += a0 && p1;
  }
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < 4; ++k) cell_s[w][k] = cell[k];
    seen_s[w] = seen;
  }
  __syncthreads();
  if (threadIdx.x < 4) {
    const int k = threadIdx.x;
    const unsigned long long s = cell_s[0][k] + cell_s[1][k] + cell_s[2][k] + cell_s[3][k];
    if (s) atomicAdd(&out->cell[k], s);
  } else if (threadIdx.x == 4) {
    const unsigned s = seen_s[0] | seen_s[1] | seen_s[2] | seen_s[3];
    if (s) atomicOr(&out->seen, s);
  }
}

// DataValidators.binaryLabelValidator: every label 0.0 or 1.0, else the run fails (flag 2).
__global__ __launch_bounds__(256) void lr_validate_kernel(const double* __restrict__ y, int64_t n,
                                                          LrState* __restrict__ st) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x)
    if (!(y[i] == 0.0 || y[i] == 1.0)) st->converged = 2;
}

}  // namespace dev

hipError_t launch_lr_validate(hipStream_t st, const double* y, int64_t n, LrState* state) {
  const int64_t g = (n + 255) / 256;
  hipLaunchKernelGGL(dev::lr_validate_kernel, dim3((unsigned)(g < 1 ? 1 : (g > 4096 ? 4096 : g))),
                     dim3(256), 0, st, y, n, state);
  return hipGetLastError();
}

int lr_grid(int64_t n) {
  constexpr int64_t cap = 512;  // 2 workgroups per CU
  const int64_t g = (n + 16 * dev::kLrWaves - 1) / (16 * dev::kLrWaves);  // >= 16 rows per wave
  return (int)(g < 1 ? 1 : (g > cap ? cap : g));
}

#define EEGFX_LR_KD(KD, CALL) \
  case KD:                    \
    CALL;                     \
    break;

template <int GRAD, bool POS>
static hipError_t lr_gradient(hipStream_t st, const double* X, const double* y, int64_t n, int d,
                              const uint32_t* mask, const int64_t* pos, const LrState* state,
                              double* partial, int G) {
#define EEGFX_LR_GRAD(KERNEL, KD)                                                                \
  EEGFX_LR_KD(KD, hipLaunchKernelGGL((dev::KERNEL<KD, GRAD, POS>), dim3(G), dim3(256), 0, st, X, \
                                     y, n, d, mask, pos, state, partial))
  if (d <= 128) {
    const int fpl = (d + 15) / 16;
    switch (fpl <= 1 ? 1 : fpl <= 2 ? 2 : fpl <= 3 ? 3 : fpl <= 4 ? 4 : 8) {
      EEGFX_LR_GRAD(lr_grad16_kernel, 1)
      EEGFX_LR_GRAD(lr_grad16_kernel, 2)
      EEGFX_LR_GRAD(lr_grad16_kernel, 3)
      EEGFX_LR_GRAD(lr_grad16_kernel, 4)
      EEGFX_LR_GRAD(lr_grad16_kernel, 8)
    }
  } else {
    const int kd = (d + 63) / 64;
    switch (kd <= 1 ? 1 : kd <= 2 ? 2 : kd <= 4 ? 4 : kd <= 8 ? 8 : 16) {
      EEGFX_LR_GRAD(lr_grad_kernel, 1)
      EEGFX_LR_GRAD(lr_grad_kernel, 2)
      EEGFX_LR_GRAD(lr_grad_kernel, 4)
      EEGFX_LR_GRAD(lr_grad_kernel, 8)
      EEGFX_LR_GRAD(lr_grad_kernel, 16)
    }
  }
#undef EEGFX_LR_GRAD
  return hipGetLastError();
}

hipError_t launch_lr_gradient(hipStream_t st, int grad, const double* X, const double* y,
                              int64_t n, int d, const uint32_t* mask, const int64_t* pos,
                              const LrState* state, double* partial, int G) {
  // the hinge loop is full-batch: no mask, so no positions to look up
  if (grad == kGradHinge) return lr_gradient<1, false>(st, X, y, n, d, nullptr, nullptr, state,
                                                       partial, G);
  return mask && pos ? lr_gradient<0, true>(st, X, y, n, d, mask, pos, state, partial, G)
                     : lr_gradient<0, false>(st, X, y, n, d, mask, nullptr, state, partial, G);
}

hipError_t launch_lr_fold(hipStream_t st, const double* partial, int G, int d,
                          const LrState* state, double* out) {
  hipLaunchKernelGGL(dev::lr_fold_kernel, dim3(1), dim3(256), 0, st, partial, G, d, state, out);
  return hipGetLastError();
}

hipError_t launch_lr_update(hipStream_t st, const double* partial, int G, int64_t count, int d,
                            LrState* state, double step_size, double reg, double tol,
                            int max_iter) {
  hipLaunchKernelGGL(dev::lr_update_kernel, dim3(1), dim3(256), 0, st, partial, G, count, d,
                     step_size, reg, tol, max_iter, state);
  return hipGetLastError();
}

hipError_t launch_lr_skip(hipStream_t st, LrState* state, int max_iter) {
  hipLaunchKernelGGL(dev::lr_skip_kernel, dim3(1), dim3(64), 0, st, max_iter, state);
  return hipGetLastError();
}

template <int KIND>
static hipError_t lr_predict(hipStream_t st, const double* X, int64_t n, int d, const double* w,
                             double intercept, double threshold, int use_threshold, double* out) {
  const dim3 grid((unsigned)((n + 3) / 4));
  const int kd = (d + 63) / 64;
  switch (kd <= 1 ? 1 : kd <= 2 ? 2 : kd <= 4 ? 4 : kd <= 8 ? 8 : 16) {
    EEGFX_LR_KD(1, hipLaunchKernelGGL((dev::lr_predict_kernel<1, KIND>), grid, dim3(256), 0, st, X,
                                      n, d, w, intercept, threshold, use_threshold, out))
    EEGFX_LR_KD(2, hipLaunchKernelGGL((dev::lr_predict_kernel<2, KIND>), grid, dim3(256), 0, st, X,
                                      n, d, w, intercept, threshold, use_threshold, out))
    EEGFX_LR_KD(4, hipLaunchKernelGGL((dev::lr_predict_kernel<4, KIND>), grid, dim3(256), 0, st, X,
                                      n, d, w, intercept, threshold, use_threshold, out))
    EEGFX_LR_KD(8, hipLaunchKernelGGL((dev::lr_predict_kernel<8, KIND>), grid, dim3(256), 0, st, X,
                                      n, d, w, intercept, threshold, use_threshold, out))
    EEGFX_LR_KD(16, hipLaunchKernelGGL((dev::lr_predict_kernel<16, KIND>), grid, dim3(256), 0, st,
                                       X, n, d, w, intercept, threshold, use_threshold, out))
  }
  return hipGetLastError();
}

hipError_t launch_lr_predict(hipStream_t st, int grad, const double* X, int64_t n, int d,
                             const double* w, double intercept, double threshold,
                             int use_threshold, double* out) {
  if (n == 0) return hipSuccess;
  return grad == kGradHinge
             ? lr_predict<1>(st, X, n, d, w, intercept, threshold, use_threshold, out)
             : lr_predict<0>(st, X, n, d, w, intercept, threshold, use_threshold, out);
}

template <int KIND>
static hipError_t lr_count(hipStream_t st, const double* X, const double* y, int64_t n, int d,
                           const double* w, double intercept, double threshold, int use_threshold,
                           ConfusionOut* out) {
  const dim3 grid(grid_for(n, 4, kLrCountMaxBlocks));
  const int kd = (d + 63) / 64;
  switch (kd <= 1 ? 1 : kd <= 2 ? 2 : kd <= 4 ? 4 : kd <= 8 ? 8 : 16) {
    EEGFX_LR_KD(1, hipLaunchKernelGGL((dev::lr_count_kernel<1, KIND>), grid, dim3(256), 0, st, X, y,
                                      n, d, w, intercept, threshold, use_threshold, out))
    EEGFX_LR_KD(2, hipLaunchKernelGGL((dev::lr_count_kernel<2, KIND>), grid, dim3(256), 0, st, X, y,
                                      n, d, w, intercept, threshold, use_threshold, out))
    EEGFX_LR_KD(4, hipLaunchKernelGGL((dev::lr_count_kernel<4, KIND>), grid, dim3(256), 0, st, X, y,
                                      n, d, w, intercept, threshold, use_threshold, out))
    EEGFX_LR_KD(8, hipLaunchKernelGGL((dev::lr_count_kernel<8, KIND>), grid, dim3(256), 0, st, X, y,
                                      n, d, w, intercept, threshold, use_threshold, out))
    EEGFX_LR_KD(16, hipLaunchKernelGGL((dev::lr_count_kernel<16, KIND>), grid, dim3(256), 0, st,
                                       X, y, n, d, w, intercept, threshold, use_threshold, out))
  }
  return hipGetLastError();
}

hipError_t launch_lr_count(hipStream_t st, int grad, const double* X, const double* y, int64_t n,
                           int d, const double* w, double intercept, double threshold,
                           int use_threshold, ConfusionOut* out) {
  if (n == 0) return hipSuccess;
  return grad == kGradHinge
             ? lr_count<1>(st, X, y, n, d, w, intercept, threshold, use_threshold, out)
             : lr_count<0>(st, X, y, n, d, w, intercept, threshold, use_threshold, out);
}
#undef EEGFX_LR_KD

}  // namespace eegfx
