// nn.hip -- the dense network of train_clf=nn on the GPU: the model the
// reference builds from its config_layer<i>_* keys (Classification/NeuralNetworkClassifier.java:
// 102-137, 258-320), trained by full-batch gradient descent with one of five updaters, in float64.
//
// One iteration = two launches on the context stream, no host round trip:
//   nn_grad_kernel    G workgroups x 256 threads.  A workgroup stages the weights in LDS once
//                     (layer 1's only where they fit: a wide first layer is read through L2), then
//                     takes tiles of tl.rows feature rows a grid stride apart.  A tile's rows are
//                     loaded once, coalesced, into LDS; forward, loss, backward and the weight
//                     gradients of those rows are computed out of LDS, so a row's activations never
//                     reach HBM.  Forward and backward: thread e takes element (row e / n_out,
//                     unit e % n_out) of the layer, so a wavefront reads consecutive weights and
//                     broadcasts the activation.  Gradient: thread t owns parameters t, t + 256,
//                     ... and adds the tile's rows to them in row order -- the first kNnAccRegs in
//                     registers, the rest in the workgroup's own slab of `partial` (same thread
//                     every time: no atomics).  At the end the slab holds the workgroup's sums and
//                     its loss sum.
//   nn_update_kernel<false>  one thread per parameter: the partials summed in workgroup order
//                     (nn_partial_mean), / n, the updater's elementwise step; workgroup 0 also sums
//                     the losses into scores[iteration].  The last workgroup to finish
//                     (nn_last_workgroup) advances the iteration.
// The order of every sum is a function of (n, d, the widths) alone: two runs give the same bits.
// Under a line-search optimiser (eegfx_nn_train_opt) an iteration is the
// fixed sequence maxLs x (nn_score_kernel, nn_search_kernel), nn_grad_kernel,
// nn_update_kernel<true>, nn_direction_kernel, still without a host round trip:
//   nn_score_kernel   nn_grad_kernel's forward pass and row loss over a candidate vector, in the
//                     same tiles, grid and loss slots: the bits the gradient pass would report.
//   nn_search_kernel  one thread per parameter: every workgroup takes the same decision of the
//                     backtracking line search from the state in device memory and writes its slice
//                     of the next candidate or of the accepted parameters; the last one commits.
//   nn_update_kernel<true>  the same kernel body, but the updater's output is stored as the
//                     gradient the optimisers see.
//   nn_direction_kernel  one workgroup: the dot products, the CG / LBFGS direction, both
//                     termination tests and the set-up of the next search, in an order fixed by P
//                     alone.
//   nn_predict_kernel the forward pass of nn_grad_kernel, output 0 of the last layer per row.
//   nn_stats_kernel   ClassificationStatistics.add over (score, label) pairs: four integer
//                     counters (atomics on integers), three sums as per-workgroup partials.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "eegfx.h"
#include "launch.h"

namespace eegfx {

constexpr int kNnThreads = 256;
constexpr int kNnMaxTileRows = 64;     // rows of a tile: at most one per lane of the loss step
constexpr int kNnMinStagedRows = 8;    // layer 1's weights go to LDS if this many rows still fit
constexpr int kNnLdsBytes = 147456;    // 144 KB of a gfx950 CU's 160 KB
constexpr int kNnGridCap = 768;        // 3 workgroups for each of the 256 CUs
constexpr int kNnAccRegs = 4;          // gradient sums a thread keeps in registers
constexpr int kNnPartialDoubles = 8388608;  // cap of G * (P + 1): 64 MB of partials
constexpr int kNnValidateThreads = 256;
constexpr int kNnValidateMaxBlocks = 4096;
constexpr int kNnStatThreads = 256;
constexpr int kNnStatUnroll = 4;       // rows a thread takes per trip of nn_stats_kernel's loop
constexpr int kNnStatMaxBlocks = 2048;
constexpr int kNnDirThreads = 1024;   // the one workgroup of nn_direction_kernel

namespace dev {

__device__ __forceinline__ double nn_act(int act, double z) {
  switch (act) {
    case EEGFX_NN_ACT_TANH: return tanh(z);
    case EEGFX_NN_ACT_RELU: return z > 0.0 ? z : (z == z ? 0.0 : z);  // a NaN stays a NaN
    case EEGFX_NN_ACT_IDENTITY: return z;
    case EEGFX_NN_ACT_SOFTPLUS: return (z > 0.0 ? z : 0.0) + log1p(exp(-fabs(z)));
    case EEGFX_NN_ACT_ELU: return z > 0.0 ? z : expm1(z);
    default: return 1.0 / (1.0 + exp(-z));
  }
}

// f'(z), with a = f(z) at hand (not for softmax)
__device__ __forceinline__ double nn_dact(int act, double z, double a) {
  switch (act) {
    case EEGFX_NN_ACT_TANH: return 1.0 - a * a;
    case EEGFX_NN_ACT_RELU: return z > 0.0 ? 1.0 : 0.0;
    case EEGFX_NN_ACT_IDENTITY: return 1.0;
    case EEGFX_NN_ACT_SOFTPLUS: return 1.0 / (1.0 + exp(-z));
    case EEGFX_NN_ACT_ELU: return z > 0.0 ? 1.0 : exp(z);
    default: return a * (1.0 - a);
  }
}

// z + sum_i a[i] * w[i * ws], in index order
__device__ __forceinline__ double nn_dot(const double* a, const double* w, int ws, int n,
                                         double z) {
  for (int i = 0; i < n; ++i) z = __builtin_fma(a[i], w[(int64_t)i * ws], z);
  return z;
}

// The weights (padded to their LDS stride) and biases of every layer, once per workgroup.
__device__ __forceinline__ void nn_stage_weights(const NnNet& net, const NnTile& tl, double* lds,
                                                 const double* __restrict__ params) {
  const int t = threadIdx.x;
  for (int l = 0; l < net.L; ++l) {
    const int no = net.n_out[l], nw = net.n_in[l] * no;
    const double* src = params + net.w_off[l];
    if (l > 0 || tl.w1_lds) {
      int i = t / no, j = t - i * no;
      const int di = kNnThreads / no, dj = kNnThreads - di * no;
      for (int e = t; e < nw; e += kNnThreads) {
        lds[tl.w_lds[l] + i * tl.w_stride[l] + j] = src[e];
        i += di;
        j += dj;
        if (j >= no) {
          j -= no;
          ++i;
        }
      }
    }
    for (int j = t; j < no; j += kNnThreads) lds[tl.b_lds[l] + j] = src[nw + j];
  }
}

// Rows [row0, row0 + rows) of X into the tile, and (y != null) their labels.
__device__ __forceinline__ void nn_load_rows(const NnNet& net, const NnTile& tl, double* lds,
                                             const double* __restrict__ X,
                                             const double* __restrict__ y, int64_t row0,
                                             int rows) {
  const int t = threadIdx.x, d = net.d;
  const double* src = X + row0 * d;
  int r = t / d, c = t - r * d;
  const int dr = kNnThreads / d, dc = kNnThreads - dr * d;
  for (int e = t; e < rows * d; e += kNnThreads) {
    lds[tl.x_off + r * tl.x_stride + c] = src[e];
    r += dr;
    c += dc;
    if (c >= d) {
      c -= d;
      ++r;
    }
  }
  if (y && t < rows) lds[tl.y_off + t] = y[row0 + t];
}

// a_l = f(a_{l-1} W_l + b_l) for the tile's rows, layer after layer; z_l is kept for the backward
// pass.  Ends behind a barrier.
__device__ __forceinline__ void nn_forward(const NnNet& net, const NnTile& tl, double* lds,
                                           const double* __restrict__ params, int rows) {
  const int t = threadIdx.x;
  for (int l = 0; l < net.L; ++l) {
    const int no = net.n_out[l], ni = net.n_in[l], act = net.act[l];
    const int in_off = l == 0 ? tl.x_off : tl.a_off[l - 1];
    const int in_stride = l == 0 ? tl.x_stride : tl.a_stride[l - 1];
    const int os = tl.a_stride[l];
    int r = t / no, j = t - r * no;
    const int dr = kNnThreads / no, dj = kNnThreads - dr * no;
    for (int e = t; e < rows * no; e += kNnThreads) {
      const double* a = lds + in_off + r * in_stride;
      double z = lds[tl.b_lds[l] + j];
      if (l == 0 && !tl.w1_lds)
        z = nn_dot(a, params + net.w_off[0] + j, no, ni, z);
      else
        z = nn_dot(a, lds + tl.w_lds[l] + j, tl.w_stride[l], ni, z);
      lds[tl.z_off[l] + r * os + j] = z;
      if (act != EEGFX_NN_ACT_SOFTMAX) lds[tl.a_off[l] + r * os + j] = nn_act(act, z);
      r += dr;
      j += dj;
      if (j >= no) {
        j -= no;
        ++r;
      }
    }
    __syncthreads();
    if (act == EEGFX_NN_ACT_SOFTMAX) {  // over the layer's outputs, max-subtracted
      if (t < rows) {
        const double* z = lds + tl.z_off[l] + t * os;
        double* a = lds + tl.a_off[l] + t * os;
        double m = z[0];
        for (int j2 = 1; j2 < no; ++j2) m = fmax(m, z[j2]);
        double s = 0.0;
        for (int j2 = 0; j2 < no; ++j2) {
          const double ez = exp(z[j2] - m);
          a[j2] = ez;
          s += ez;
        }
        for (int j2 = 0; j2 < no; ++j2) a[j2] = a[j2] / s;
      }
      __syncthreads();
    }
  }
}

// Where parameter p's gradient terms lie in the tile: sum over rows r of
// lds[a_off + r * a_stride] * lds[d_off + r * d_stride]; a_off < 0: a bias (the factor is 1).
struct NnTerm {
  int a_off, a_stride, d_off, d_stride;
};
__device__ __forceinline__ NnTerm nn_term(const NnNet& net, const NnTile& tl, int p) {
  int l = 0;
  for (int k = 1; k < net.L; ++k)
    if (p >= net.w_off[k]) l = k;
  const int q = p - net.w_off[l], no = net.n_out[l], nw = net.n_in[l] * no;
  NnTerm tm;
  tm.d_stride = tl.a_stride[l];
  if (q < nw) {
    const int i = q / no;
    tm.d_off = tl.z_off[l] + (q - i * no);
    tm.a_off = (l == 0 ? tl.x_off : tl.a_off[l - 1]) + i;
    tm.a_stride = l == 0 ? tl.x_stride : tl.a_stride[l - 1];
  } else {
    tm.d_off = tl.z_off[l] + (q - nw);
    tm.a_off = -1;
    tm.a_stride = 0;
  }
  return tm;
}
__device__ __forceinline__ double nn_term_sum(const double* lds, const NnTerm& tm, int rows,
                                              double acc) {
  if (tm.a_off >= 0) {
    for (int r = 0; r < rows; ++r)
      acc = __builtin_fma(lds[tm.a_off + r * tm.a_stride], lds[tm.d_off + r * tm.d_stride], acc);
  } else {
    for (int r = 0; r < rows; ++r) acc += lds[tm.d_off + r * tm.d_stride];
  }
  return acc;
}

// The loss of one row over the two outputs against {y0, y1}, and dL/dp of each: the one place
// the gradient pass and the score pass (nn_score_kernel) take a row's loss from.
__device__ __forceinline__ double nn_row_loss(int kind, double p0, double p1, double y0, double y1,
                                              double* g0, double* g1) {
  switch (kind) {
    case EEGFX_NN_LOSS_XENT:
      *g0 = -y0 / p0 + (1.0 - y0) / (1.0 - p0);
      *g1 = -y1 / p1 + (1.0 - y1) / (1.0 - p1);
      return -((y0 * log(p0) + (1.0 - y0) * log(1.0 - p0)) +
               (y1 * log(p1) + (1.0 - y1) * log(1.0 - p1)));
    case EEGFX_NN_LOSS_NLL:
      *g0 = -y0 / p0;
      *g1 = -y1 / p1;
      return -(y0 * log(p0) + y1 * log(p1));
    case EEGFX_NN_LOSS_SQUARED:
      *g0 = 2.0 * (p0 - y0);
      *g1 = 2.0 * (p1 - y1);
      return (p0 - y0) * (p0 - y0) + (p1 - y1) * (p1 - y1);
    default:
      *g0 = p0 - y0;
      *g1 = p1 - y1;
      return ((p0 - y0) * (p0 - y0) + (p1 - y1) * (p1 - y1)) / 2.0;
  }
}

// The workgroup's loss sum (row t of every tile in my_loss), in row order, into *out.
__device__ __forceinline__ void nn_store_loss(const NnTile& tl, double* lds, double my_loss,
                                              double* out) {
  const int t = threadIdx.x;
  __syncthreads();
  if (t < kNnMaxTileRows) lds[tl.loss_off + t] = my_loss;
  __syncthreads();
  if (t == 0) {
    double s = 0.0;
    for (int r = 0; r < kNnMaxTileRows; ++r) s += lds[tl.loss_off + r];
    *out = s;
  }
}

__global__ __launch_bounds__(kNnThreads) void nn_grad_kernel(
    const double* __restrict__ X, const double* __restrict__ y, int64_t n, const NnNet net,
    const NnTile tl, const NnState* __restrict__ st, double* __restrict__ partial) {
  if (st->flag) return;
  extern __shared__ __attribute__((aligned(16))) double nn_lds[];
  double* lds = nn_lds;
  const double* params = (const double*)(st + 1);
  const int t = threadIdx.x, P = net.P, L = net.L;
  double* slab = partial + (int64_t)blockIdx.x * (P + 1);
  nn_stage_weights(net, tl, lds, params);
  NnTerm term[kNnAccRegs];
  double acc[kNnAccRegs];
#pragma unroll
  for (int k = 0; k < kNnAccRegs; ++k) {
    acc[k] = 0.0;
    const int p = t + k * kNnThreads;
    term[k] = nn_term(net, tl, p < P ? p : 0);
  }
  for (int p = t + kNnAccRegs * kNnThreads; p < P; p += kNnThreads) slab[p] = 0.0;
  double my_loss = 0.0;  // of row t of every tile
  const int last = L - 1, out_act = net.act[last];
  for (int64_t row0 = (int64_t)blockIdx.x * tl.rows; row0 < n;
       row0 += (int64_t)gridDim.x * tl.rows) {
    const int rows = (int)(n - row0 < tl.rows ? n - row0 : tl.rows);
    __syncthreads();  // the previous tile's gradient step has read the tile; the weights stand
    nn_load_rows(net, tl, lds, X, y, row0, rows);
    __syncthreads();
    nn_forward(net, tl, lds, params, rows);
    // the loss of row t and its gradient at the two pre-activations of the output layer
    if (t < rows) {
      const int os = tl.a_stride[last];
      double* z = lds + tl.z_off[last] + t * os;
      const double p0 = lds[tl.a_off[last] + t * os], p1 = lds[tl.a_off[last] + t * os + 1];
      const double y0 = lds[tl.y_off + t], y1 = fabs(1.0 - y0);  // labels[i] = {t, |1 - t|}
      double g0, g1;
      const double loss = nn_row_loss(net.loss, p0, p1, y0, y1, &g0, &g1);
      my_loss += loss;
      double d0, d1;
      if ((net.loss == EEGFX_NN_LOSS_XENT && out_act == EEGFX_NN_ACT_SIGMOID) ||
          (net.loss == EEGFX_NN_LOSS_NLL && out_act == EEGFX_NN_ACT_SOFTMAX)) {
        d0 = p0 - y0;
        d1 = p1 - y1;
      } else if (out_act == EEGFX_NN_ACT_SOFTMAX) {  // the 2 x 2 Jacobian
        const double gp = g0 * p0 + g1 * p1;
        d0 = p0 * (g0 - gp);
        d1 = p1 * (g1 - gp);
      } else {
        d0 = g0 * nn_dact(out_act, z[0], p0);
        d1 = g1 * nn_dact(out_act, z[1], p1);
      }
      z[0] = d0;
      z[1] = d1;
    }
    __syncthreads();
    // delta_{l-1} = (delta_l W_l^T) * f'(z_{l-1}), written over z_{l-1}
    for (int l = last; l >= 1; --l) {
      const int ni = net.n_in[l], no = net.n_out[l], act = net.act[l - 1];
      const int ps = tl.a_stride[l - 1];
      int r = t / ni, i = t - r * ni;
      const int dr = kNnThreads / ni, di = kNnThreads - dr * ni;
      for (int e = t; e < rows * ni; e += kNnThreads) {
        const double s = nn_dot(lds + tl.z_off[l] + r * tl.a_stride[l],
                                lds + tl.w_lds[l] + i * tl.w_stride[l], 1, no, 0.0);
        double* zp = lds + tl.z_off[l - 1] + r * ps + i;
        *zp = act == EEGFX_NN_ACT_SOFTMAX
                  ? s
                  : s * nn_dact(act, *zp, lds[tl.a_off[l - 1] + r * ps + i]);
        r += dr;
        i += di;
        if (i >= ni) {
          i -= ni;
          ++r;
        }
      }
      __syncthreads();
      if (act == EEGFX_NN_ACT_SOFTMAX) {  // a hidden softmax: delta_i = a_i (s_i - sum_m s_m a_m)
        if (t < rows) {
          double* s = lds + tl.z_off[l - 1] + t * ps;
          const double* a = lds + tl.a_off[l - 1] + t * ps;
          double sa = 0.0;
          for (int m = 0; m < ni; ++m) sa = __builtin_fma(s[m], a[m], sa);
          for (int m = 0; m < ni; ++m) s[m] = a[m] * (s[m] - sa);
        }
        __syncthreads();
      }
    }
    // the rows' terms of every parameter's gradient, in row order
#pragma unroll
    for (int k = 0; k < kNnAccRegs; ++k)
      if (t + k * kNnThreads < P) acc[k] = nn_term_sum(lds, term[k], rows, acc[k]);
    for (int p = t + kNnAccRegs * kNnThreads; p < P; p += kNnThreads)
      slab[p] = nn_term_sum(lds, nn_term(net, tl, p), rows, slab[p]);
  }
#pragma unroll
  for (int k = 0; k < kNnAccRegs; ++k)
    if (t + k * kNnThreads < P) slab[t + k * kNnThreads] = acc[k];
  nn_store_loss(tl, lds, my_loss, slab + P);
}

// The updater's u for the mean gradient g of one parameter (p <- p - u), iteration `it` (0-based),
// its state advanced in place.
__device__ __forceinline__ double nn_updater(int updater, double lr, double mu, int it, double g,
                                             double* s1, double* s2) {
  switch (updater) {
    case EEGFX_NN_UPD_SGD:
      return lr * g;
    case EEGFX_NN_UPD_ADAM: {
      const double b1 = 0.9, b2 = 0.999, t = (double)(it + 1);
      const double m = b1 * *s1 + (1.0 - b1) * g;
      const double v = b2 * *s2 + (1.0 - b2) * (g * g);
      *s1 = m;
      *s2 = v;
      return lr * sqrt(1.0 - pow(b2, t)) / (1.0 - pow(b1, t)) * (m / (sqrt(v) + 1e-8));
    }
    case EEGFX_NN_UPD_ADAGRAD: {
      const double h = *s1 + g * g;
      *s1 = h;
      return lr * g / (sqrt(h) + 1e-6);
    }
    case EEGFX_NN_UPD_RMSPROP: {
      const double r = 0.95 * *s1 + 0.05 * (g * g);
      *s1 = r;
      return lr * g / sqrt(r + 1e-8);
    }
    default: {  // nesterovs
      const double v = *s1, vn = mu * v - lr * g;
      *s1 = vn;
      return mu * v - (1.0 + mu) * vn;
    }
  }
}

// The vectors behind NnOpt (the line-search optimisers, below).
enum { kVecG = 0, kVecGNew = 1, kVecDir = 2, kVecCand = 3, kVecPOld = 4, kVecGOld = 5,
       kVecS = 6, kVecY = kVecS + kNnLbfgsM };
__device__ __forceinline__ double* nn_opt_vec(const NnOpt* opt, int k, int P) {
  return (double*)(opt + 1) + (int64_t)k * P;
}

// Column p of the G workgroups' partials, summed in workgroup order, / n: the mean gradient of
// parameter p, or (p == P) the loss.
__device__ __forceinline__ double nn_partial_mean(const double* __restrict__ partial, int G,
                                                  int64_t n, int P, int p) {
  const int64_t stride = P + 1;
  double s = 0.0;
  for (int b = 0; b < G; ++b) s += partial[b * stride + p];
  return s / (double)n;
}

// True in thread 0 of the last workgroup of the grid to get here, with the ticket reset: every
// workgroup has then read the state that this thread goes on to commit.
__device__ __forceinline__ bool nn_last_workgroup(uint32_t* ticket) {
  __syncthreads();
  if (threadIdx.x != 0) return false;
  __threadfence();
  if (atomicAdd(ticket, 1u) != gridDim.x - 1) return false;
  *ticket = 0;
  return true;
}

// One thread per parameter: the updater's u for the mean gradient.  OPT == false (an SGD step):
// p <- p - u, and the loss goes to scores[it] where scores is set.  OPT == true (the gradient
// pass of the optimisers): the same sums, the same updater on the same state, but u goes to g_new,
// the loss to NnOpt::score_new and the parameters stay; st->iter then counts the gradient passes.
template <bool OPT>
__global__ __launch_bounds__(kNnThreads) void nn_update_kernel(
    const double* __restrict__ partial, int G, int64_t n, int P, int updater, double lr,
    double mu, NnState* __restrict__ st, NnOpt* __restrict__ opt, double* __restrict__ scores) {
  if (st->flag) return;
  const int it = st->iter;  // every thread reads it before its workgroup takes a ticket
  const int p = blockIdx.x * kNnThreads + threadIdx.x;
  if (p < P) {
    const double g = nn_partial_mean(partial, G, n, P, p);
    double* w = (double*)(st + 1) + p;
    double* s1 = w + P;
    double* s2 = s1 + P;
    const double u = nn_updater(updater, lr, mu, it, g, s1, s2);
    if constexpr (OPT)
      nn_opt_vec(opt, kVecGNew, P)[p] = u;
    else
      *w = *w - u;
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    if constexpr (OPT)
      opt->score_new = nn_partial_mean(partial, G, n, P, P);
    else if (scores)
      scores[it] = nn_partial_mean(partial, G, n, P, P);
  }
  if (nn_last_workgroup(&st->ticket)) st->iter = it + 1;
}

// ---- the line-search optimisers (eegfx_nn_train_opt) --------------------
// p - step * dir: the one expression a candidate and the accepted parameters are made with, so
// the parameters a search accepts are the bits of the candidate it scored.
__device__ __forceinline__ double nn_move(double p, double step, double d) { return p - step * d; }
__device__ __forceinline__ bool nn_finite(double v) { return fabs(v) <= 1.7976931348623157e308; }

// nn_grad_kernel's forward pass and row loss over NnOpt's candidate vector: the same tiles, grid
// and loss slot of `partial`, so the score of a vector is what the gradient pass reports for it.
__global__ __launch_bounds__(kNnThreads) void nn_score_kernel(
    const double* __restrict__ X, const double* __restrict__ y, int64_t n, const NnNet net,
    const NnTile tl, const NnState* __restrict__ st, const NnOpt* __restrict__ opt,
    double* __restrict__ partial) {
  if (st->flag || opt->line.done) return;
  extern __shared__ __attribute__((aligned(16))) double nn_lds[];
  double* lds = nn_lds;
  const double* params = nn_opt_vec(opt, kVecCand, net.P);
  const int t = threadIdx.x, last = net.L - 1;
  nn_stage_weights(net, tl, lds, params);
  double my_loss = 0.0;  // of row t of every tile
  for (int64_t row0 = (int64_t)blockIdx.x * tl.rows; row0 < n;
       row0 += (int64_t)gridDim.x * tl.rows) {
    const int rows = (int)(n - row0 < tl.rows ? n - row0 : tl.rows);
    __syncthreads();  // the previous tile's loss step has read the tile
    nn_load_rows(net, tl, lds, X, y, row0, rows);
    __syncthreads();
    nn_forward(net, tl, lds, params, rows);
    if (t < rows) {
      const int os = tl.a_stride[last];
      const double p0 = lds[tl.a_off[last] + t * os], p1 = lds[tl.a_off[last] + t * os + 1];
      const double y0 = lds[tl.y_off + t], y1 = fabs(1.0 - y0);
      double g0, g1;
      my_loss += nn_row_loss(net.loss, p0, p1, y0, y1, &g0, &g1);
    }
  }
  nn_store_loss(tl, lds, my_loss, partial + (int64_t)blockIdx.x * (net.P + 1) + net.P);
}

// One trial of BackTrackLineSearch with the trial's score `sc` at hand.  Returns what the
// parameter threads do: 0 write the next candidate p - *move * dir, 1 the search has ended and
// p <- p - *move * dir, 2 it has ended with step 0.  rec: the iteration's record once it ends.
__device__ __forceinline__ int nn_line_step(NnLine& ln, double sc, int max_ls, double* move,
                                            NnSearchRec* rec) {
  const double s0 = ln.s0, slope = ln.slope, step = ln.step, prev = ln.sc;
  ln.sc = sc;
  ln.trials += 1;
  rec->trials = ln.trials;
  rec->pad = 0;
  if (sc < ln.best) {
    ln.best = sc;
    ln.best_step = step;
  }
  if (sc <= s0 + 1e-4 * step * slope) {  // Armijo (false for a NaN score)
    ln.done = 1;
    rec->step = *move = step;
    rec->score = sc;
    return 1;
  }
  double tmp;
  if (!nn_finite(sc) || !nn_finite(prev)) {
    tmp = 0.2 * step;
  } else if (step == 1.0) {
    tmp = -slope / (2.0 * (sc - s0 - slope));
  } else {
    const double step2 = ln.step2;
    const double r1 = sc - s0 - step * slope, r2 = ln.sc2 - s0 - step2 * slope;
    const double q1 = r1 / (step * step), q2 = r2 / (step2 * step2);
    const double a = (q1 - q2) / (step - step2);
    const double b = (-step2 * q1 + step * q2) / (step - step2);
    if (a == 0.0) {
      tmp = -slope / (2.0 * b);
    } else {
      const double disc = b * b - 3.0 * a * slope;
      if (disc < 0.0)
        tmp = 0.5 * step;
      else if (b <= 0.0)
        tmp = (-b + sqrt(disc)) / (3.0 * a);
      else
        tmp = -slope / (b + sqrt(disc));
    }
    if (!(tmp < 0.5 * step)) tmp = 0.5 * step;
  }
  ln.step2 = step;
  ln.sc2 = sc;
  ln.step = tmp > 0.1 * step ? tmp : 0.1 * step;
  if (ln.trials < max_ls && !(ln.step < ln.step_min)) {
    *move = ln.step;
    return 0;
  }
  ln.done = 1;
  if (ln.trials == max_ls && ln.best < s0) {
    rec->step = *move = ln.best_step;
    rec->score = ln.best;
    return 1;
  }
  rec->step = *move = 0.0;
  rec->score = s0;
  return 2;
}

// One thread per parameter.  Thread 0 of every workgroup sums the G loss partials in workgroup
// order and takes the search's decision from the state in device memory (the same in every
// workgroup); the workgroup then writes its slice of the next candidate or of the accepted p.  The
// last workgroup to take a ticket commits the state: by then every workgroup has read it.
__global__ __launch_bounds__(kNnThreads) void nn_search_kernel(
    const double* __restrict__ partial, int G, int64_t n, int P, int max_ls,
    NnState* __restrict__ st, NnOpt* __restrict__ opt, NnSearchRec* __restrict__ search) {
  if (st->flag || opt->line.done) return;
  __shared__ double sh_move;
  __shared__ int sh_mode;
  NnLine ln;
  NnSearchRec rec;
  int it = 0;
  if (threadIdx.x == 0) {
    ln = opt->line;
    it = opt->it;
    double move;
    sh_mode = nn_line_step(ln, nn_partial_mean(partial, G, n, P, P), max_ls, &move, &rec);
    sh_move = move;
  }
  __syncthreads();
  const int mode = sh_mode, k = blockIdx.x * kNnThreads + threadIdx.x;
  if (k < P && mode != 2) {
    double* p = (double*)(st + 1);
    const double v = nn_move(p[k], sh_move, nn_opt_vec(opt, kVecDir, P)[k]);
    if (mode == 1)
      p[k] = v;
    else
      nn_opt_vec(opt, kVecCand, P)[k] = v;
  }
  if (nn_last_workgroup(&opt->ticket)) {
    opt->line = ln;
    if (ln.done) search[it] = rec;
  }
}

// v[k] <- the workgroup's sum of v[k] over its kNnDirThreads threads, in a tree whose shape is
// fixed; red: N * kNnDirThreads doubles of LDS.  Ends behind a barrier.
template <int N>
__device__ __forceinline__ void nn_block_sum(double (&v)[N], double* red) {
  const int t = threadIdx.x;
#pragma unroll
  for (int k = 0; k < N; ++k) red[k * kNnDirThreads + t] = v[k];
  __syncthreads();
  for (int h = kNnDirThreads / 2; h > 0; h >>= 1) {
    if (t < h) {
#pragma unroll
      for (int k = 0; k < N; ++k) red[k * kNnDirThreads + t] += red[k * kNnDirThreads + t + h];
    }
    __syncthreads();
  }
#pragma unroll
  for (int k = 0; k < N; ++k) v[k] = red[k * kNnDirThreads];
  __syncthreads();
}
// ... and the largest v; a NaN among them makes it a NaN, wherever it stands
__device__ __forceinline__ double nn_block_max(double v, double* red) {
  const int t = threadIdx.x;
  red[t] = v;
  __syncthreads();
  for (int h = kNnDirThreads / 2; h > 0; h >>= 1) {
    if (t < h && (red[t + h] > red[t] || red[t + h] != red[t + h])) red[t] = red[t + h];
    __syncthreads();
  }
  v = red[0];
  __syncthreads();
  return v;
}

// One workgroup.  Thread t owns elements t, t + kNnDirThreads, ... of every vector (so no element
// passes between threads but through the reductions), and sums them in that order: every sum's
// order is a function of P alone.  After a gradient pass: the algorithm's next direction, g <-
// g_new, ZeroDirection and EpsTermination (NnState::flag = 1), scores[it + 1], and the next
// search's constants with its first candidate (or its return of 0 where 1 < stepMin).
__global__ __launch_bounds__(kNnDirThreads) void nn_direction_kernel(
    int P, int algo, int iters, int first, NnState* __restrict__ st, NnOpt* __restrict__ opt,
    double* __restrict__ scores, NnSearchRec* __restrict__ search) {
  if (st->flag) return;
  __shared__ double red[3 * kNnDirThreads];
  constexpr int D = kNnDirThreads, M = kNnLbfgsM;
  const int t = threadIdx.x;
  const double* p = (const double*)(st + 1);
  double* g = nn_opt_vec(opt, kVecG, P);
  const double* gn = nn_opt_vec(opt, kVecGNew, P);
  double* dir = nn_opt_vec(opt, kVecDir, P);
  double* p_old = nn_opt_vec(opt, kVecPOld, P);
  double* g_old = nn_opt_vec(opt, kVecGOld, P);
  // the scalars of the state, read by every thread before thread 0 writes any (at the end,
  // behind the barriers of the reductions)
  const int it = first ? -1 : opt->it;
  const double old = opt->score, score = opt->score_new;
  int hist = opt->hist, head = opt->head;
  double rho_new = 0.0;
  bool stop = false;
  const bool lbfgs = algo == EEGFX_NN_OPT_LBFGS;
  if (first) {
    for (int k = t; k < P; k += D) {
      const double v = gn[k];
      g[k] = v;
      dir[k] = v;
      if (lbfgs) {
        p_old[k] = p[k];
        g_old[k] = v;
      }
    }
  } else {
    if (algo == EEGFX_NN_OPT_CG) {
      double v[2] = {0.0, 0.0};  // dgg, gg
      for (int k = t; k < P; k += D) {
        v[0] += (gn[k] - g[k]) * gn[k];
        v[1] += g[k] * g[k];
      }
      nn_block_sum(v, red);
      const double q = v[0] / v[1], gamma = q < 0.0 ? 0.0 : q;
      for (int k = t; k < P; k += D) dir[k] = gamma * dir[k] + gn[k];
    } else if (lbfgs) {
      head = hist == 0 ? 0 : (head + 1) % M;
      hist = hist < M ? hist + 1 : M;
      double* s_new = nn_opt_vec(opt, kVecS + head, P);
      double* y_new = nn_opt_vec(opt, kVecY + head, P);
      double v[2] = {0.0, 0.0};  // dot(s, y), dot(y, y)
      for (int k = t; k < P; k += D) {
        const double s = p[k] - p_old[k], yv = gn[k] - g_old[k];
        s_new[k] = s;
        y_new[k] = yv;
        v[0] += s * yv;
        v[1] += yv * yv;
        dir[k] = gn[k];
        p_old[k] = p[k];
        g_old[k] = gn[k];
      }
      nn_block_sum(v, red);
      const double sy = v[0] + 1e-5, yy = v[1] + 1e-5;
      rho_new = 1.0 / sy;
      double a[M];
#pragma unroll
      for (int j = 0; j < M; ++j) {  // newest -> oldest
        a[j] = 0.0;
        if (j < hist) {
          const int slot = (head - j + M) % M;
          const double* sv = nn_opt_vec(opt, kVecS + slot, P);
          const double* yv = nn_opt_vec(opt, kVecY + slot, P);
          double d[1] = {0.0};
          for (int k = t; k < P; k += D) d[0] += sv[k] * dir[k];
          nn_block_sum(d, red);
          a[j] = (j == 0 ? rho_new : opt->rho[slot]) * d[0];
          for (int k = t; k < P; k += D) dir[k] -= a[j] * yv[k];
        }
      }
      const double scale = sy / yy;
      for (int k = t; k < P; k += D) dir[k] *= scale;
#pragma unroll
      for (int j = M - 1; j >= 0; --j) {  // oldest -> newest
        if (j < hist) {
          const int slot = (head - j + M) % M;
          const double* sv = nn_opt_vec(opt, kVecS + slot, P);
          const double* yv = nn_opt_vec(opt, kVecY + slot, P);
          double d[1] = {0.0};
          for (int k = t; k < P; k += D) d[0] += yv[k] * dir[k];
          nn_block_sum(d, red);
          const double b = (j == 0 ? rho_new : opt->rho[slot]) * d[0];
          for (int k = t; k < P; k += D) dir[k] += (a[j] - b) * sv[k];
        }
      }
    } else {
      for (int k = t; k < P; k += D) dir[k] = gn[k];
    }
    double asum[1] = {0.0};
    for (int k = t; k < P; k += D) {
      const double v = gn[k];
      g[k] = v;
      asum[0] += fabs(v);
    }
    nn_block_sum(asum, red);
    stop = asum[0] == 0.0;  // ZeroDirection
    if (!(score == 0.0 && old == 0.0) &&
        2.0 * fabs(old - score) <= 1e-5 * (fabs(old) + fabs(score) + 1e-4))
      stop = true;          // EpsTermination
  }
  const int next = it + 1;
  const bool search_next = !stop && next < iters;
  NnLine ln{};
  if (search_next) {
    double v[2] = {0.0, 0.0};  // dot(dir, dir), dot(dir, g)
    double test = 0.0;
    for (int k = t; k < P; k += D) {
      v[0] += dir[k] * dir[k];
      v[1] += dir[k] * g[k];
      const double ap = fabs(p[k]), q = fabs(g[k]) / (ap > 1.0 ? ap : 1.0);
      if (q > test || q != q) test = q;
    }
    nn_block_sum(v, red);
    test = nn_block_max(test, red);
    const double norm = sqrt(v[0]);
    if (norm > 100.0) {  // stepMax; the slope stays what it was
      const double f = 100.0 / norm;
      for (int k = t; k < P; k += D) dir[k] *= f;
    }
    ln.s0 = ln.sc = ln.sc2 = ln.best = score;
    ln.slope = -v[1];
    ln.step_min = 1e-7 / test;
    ln.step = ln.best_step = 1.0;
    ln.step2 = 0.0;
    ln.done = ln.step < ln.step_min ? 1 : 0;
    if (!ln.done) {
      double* cand = nn_opt_vec(opt, kVecCand, P);
      for (int k = t; k < P; k += D) cand[k] = nn_move(p[k], 1.0, dir[k]);
    }
  }
  __syncthreads();
  if (t == 0) {
    opt->score = score;
    if (!first) {
      opt->iterations_run = next;
      if (lbfgs) {
        opt->hist = hist;
        opt->head = head;
        opt->rho[head] = rho_new;
      }
    }
    if (stop) st->flag = 1;
    if (search_next) {
      opt->it = next;
      opt->line = ln;
      if (scores) scores[next] = score;
      if (ln.done) search[next] = NnSearchRec{0.0, score, 0, 0};
    }
  }
}

__global__ __launch_bounds__(kNnThreads) void nn_predict_kernel(
    const double* __restrict__ X, int64_t n, const NnNet net, const NnTile tl,
    const double* __restrict__ params, double* __restrict__ out) {
  extern __shared__ __attribute__((aligned(16))) double nn_lds[];
  double* lds = nn_lds;
  const int t = threadIdx.x, last = net.L - 1;
  nn_stage_weights(net, tl, lds, params);
  for (int64_t row0 = (int64_t)blockIdx.x * tl.rows; row0 < n;
       row0 += (int64_t)gridDim.x * tl.rows) {
    const int rows = (int)(n - row0 < tl.rows ? n - row0 : tl.rows);
    __syncthreads();
    nn_load_rows(net, tl, lds, X, nullptr, row0, rows);
    __syncthreads();
    nn_forward(net, tl, lds, params, rows);
    if (t < rows) out[row0 + t] = lds[tl.a_off[last] + t * tl.a_stride[last]];
  }
}

// DataValidators-style check of the other trainers: every label 0.0 or 1.0 (-0.0 is 0.0).
__global__ __launch_bounds__(kNnValidateThreads) void nn_validate_kernel(
    const double* __restrict__ y, int64_t n, NnState* __restrict__ st) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x)
    if (!(y[i] == 0.0 || y[i] == 1.0)) st->flag = 2;
}

// Java 7+ Math.round(double): floor(x + 1/2) without the rounding error of the addition (x -
// floor(x) is exact), NaN -> 0, saturating at the ends of long.
__device__ __forceinline__ long long java_round(double x) {
  if (x != x) return 0;
  if (x >= 9223372036854775807.0) return 0x7FFFFFFFFFFFFFFFLL;
  if (x <= -9223372036854775808.0) return -0x7FFFFFFFFFFFFFFFLL - 1;
  const double f = floor(x);
  return (long long)f + (x - f >= 0.5 ? 1 : 0);
}

__device__ __forceinline__ unsigned long long nn_wave_sum(unsigned long long v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
  return v;  // lane 0 holds the wave's sum
}

__global__ __launch_bounds__(kNnStatThreads) void nn_stats_kernel(
    const double* __restrict__ scores, const double* __restrict__ labels, int64_t n,
    NnStatsOut* __restrict__ out, double* __restrict__ sums) {
  constexpr int U = kNnStatUnroll;
  __shared__ double red[3][kNnStatThreads];
  unsigned long long cell[4] = {0, 0, 0, 0};  // tp, tn, fp, fn
  double acc[3] = {0.0, 0.0, 0.0};            // MSE, class1sum, class2sum
  const int64_t step = (int64_t)gridDim.x * blockDim.x;
  for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r < n; r += step * U) {
    double a[U], s[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const bool live = r + u * step < n;
      a[u] = live ? labels[r + u * step] : 0.0;
      s[u] = live ? scores[r + u * step] : 0.0;
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      if (r + u * step >= n) continue;
      acc[0] += (a[u] - s[u]) * (a[u] - s[u]);
      const long long want = java_round(a[u]), got = java_round(s[u]);
      if (want == 0) {
        cell[got == 0 ? 1 : 2] += 1;
        acc[1] += s[u];
      } else if (want == 1) {
        cell[got == 1 ? 0 : 3] += 1;
        acc[2] += s[u];
      }
    }
  }
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const unsigned long long s = nn_wave_sum(cell[k]);
    if ((threadIdx.x & 63) == 0 && s) atomicAdd(&out->cell[k], s);
  }
#pragma unroll
  for (int k = 0; k < 3; ++k) red[k][threadIdx.x] = acc[k];
  __syncthreads();
  for (int h = kNnStatThreads / 2; h > 0; h >>= 1) {
    if ((int)threadIdx.x < h) {
#pragma unroll
      for (int k = 0; k < 3; ++k) red[k][threadIdx.x] += red[k][threadIdx.x + h];
    }
    __syncthreads();
  }
  if (threadIdx.x < 3) sums[blockIdx.x * 3 + threadIdx.x] = red[threadIdx.x][0];
}

}  // namespace dev

NnTile nn_plan_tile(const NnNet& net) {
  auto odd = [](int v) { return v | 1; };
  NnTile t{};
  t.x_stride = odd(net.d);
  int per_row = t.x_stride + 2;  // features, label, (loss_off holds kNnMaxTileRows always)
  int fixed = kNnMaxTileRows;
  for (int l = 0; l < net.L; ++l) {
    t.w_stride[l] = odd(net.n_out[l]);
    t.a_stride[l] = odd(net.n_out[l]);
    per_row += 2 * t.a_stride[l];
    fixed += net.n_out[l];
    if (l > 0) fixed += net.n_in[l] * t.w_stride[l];
  }
  const int budget = kNnLdsBytes / (int)sizeof(double);
  const int w1 = net.n_in[0] * t.w_stride[0];
  const int with_w1 = (budget - fixed - w1) / per_row;  // negative: does not fit at all
  t.w1_lds = with_w1 >= kNnMinStagedRows ? 1 : 0;
  if (t.w1_lds) fixed += w1;
  t.rows = std::min(kNnMaxTileRows, (budget - fixed) / per_row);
  int off = 0;
  auto take = [&](int doubles) {
    const int at = off;
    off += doubles;
    return at;
  };
  t.loss_off = take(kNnMaxTileRows);
  for (int l = 0; l < net.L; ++l) {
    t.w_lds[l] = (l > 0 || t.w1_lds) ? take(net.n_in[l] * t.w_stride[l]) : 0;
    t.b_lds[l] = take(net.n_out[l]);
  }
  t.y_off = take(t.rows);
  t.x_off = take(t.rows * t.x_stride);
  for (int l = 0; l < net.L; ++l) {
    t.a_off[l] = take(t.rows * t.a_stride[l]);
    t.z_off[l] = take(t.rows * t.a_stride[l]);
  }
  t.doubles = off;
  return t;
}

int nn_grid(int64_t n, const NnNet& net, const NnTile& tl) {
  const int64_t tiles = (n + tl.rows - 1) / tl.rows;
  const int64_t cap = std::min<int64_t>(kNnGridCap, std::max(1, kNnPartialDoubles / (net.P + 1)));
  return (int)std::max<int64_t>(1, std::min(tiles, cap));
}

// A workgroup of these kernels asks for more LDS than the 64 KB a launch gets unasked.
template <typename K>
static hipError_t nn_allow_lds(K kernel) {
  return hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                             kNnLdsBytes);
}

hipError_t launch_nn_validate(hipStream_t st, const double* y, int64_t n, NnState* state) {
  hipLaunchKernelGGL(dev::nn_validate_kernel,
                     dim3(grid_for(n, kNnValidateThreads, kNnValidateMaxBlocks)),
                     dim3(kNnValidateThreads), 0, st, y, n, state);
  return hipGetLastError();
}

static dim3 nn_param_grid(int P) { return dim3((P + kNnThreads - 1) / kNnThreads); }

hipError_t launch_nn_gradient(hipStream_t st, const double* X, const double* y, int64_t n,
                              const NnNet& net, const NnTile& tl, int G, NnState* state,
                              double* partial, double lr, double momentum, NnOpt* opt,
                              double* scores) {
  hipError_t e = nn_allow_lds(dev::nn_grad_kernel);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(dev::nn_grad_kernel, dim3(G), dim3(kNnThreads),
                     sizeof(double) * (size_t)tl.doubles, st, X, y, n, net, tl, state, partial);
  e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(opt ? dev::nn_update_kernel<true> : dev::nn_update_kernel<false>,
                     nn_param_grid(net.P), dim3(kNnThreads), 0, st, partial, G, n, net.P,
                     net.updater, lr, momentum, state, opt, scores);
  return hipGetLastError();
}

hipError_t launch_nn_trial(hipStream_t st, const double* X, const double* y, int64_t n,
                           const NnNet& net, const NnTile& tl, int G, NnState* state, NnOpt* opt,
                           double* partial, int max_ls, NnSearchRec* search) {
  hipError_t e = nn_allow_lds(dev::nn_score_kernel);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(dev::nn_score_kernel, dim3(G), dim3(kNnThreads),
                     sizeof(double) * (size_t)tl.doubles, st, X, y, n, net, tl, state, opt,
                     partial);
  e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(dev::nn_search_kernel, nn_param_grid(net.P), dim3(kNnThreads), 0, st,
                     partial, G, n, net.P, max_ls, state, opt, search);
  return hipGetLastError();
}

hipError_t launch_nn_direction(hipStream_t st, const NnNet& net, int algorithm, int iterations,
                               bool first, NnState* state, NnOpt* opt, double* scores,
                               NnSearchRec* search) {
  hipLaunchKernelGGL(dev::nn_direction_kernel, dim3(1), dim3(kNnDirThreads), 0, st, net.P,
                     algorithm, iterations, first ? 1 : 0, state, opt, scores, search);
  return hipGetLastError();
}

hipError_t launch_nn_predict(hipStream_t st, const double* X, int64_t n, const NnNet& net,
                             const NnTile& tl, const double* params, double* out) {
  if (n == 0) return hipSuccess;
  hipError_t e = nn_allow_lds(dev::nn_predict_kernel);
  if (e != hipSuccess) return e;
  const int64_t tiles = (n + tl.rows - 1) / tl.rows;
  hipLaunchKernelGGL(dev::nn_predict_kernel, dim3((unsigned)std::min<int64_t>(tiles, kNnGridCap)),
                     dim3(kNnThreads), sizeof(double) * (size_t)tl.doubles, st, X, n, net, tl,
                     params, out);
  return hipGetLastError();
}

int nn_stats_grid(int64_t n) {
  return (int)grid_for(n, kNnStatThreads * kNnStatUnroll, kNnStatMaxBlocks);
}

hipError_t launch_nn_stats(hipStream_t st, const double* scores, const double* labels, int64_t n,
                           NnStatsOut* out, double* sums) {
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(dev::nn_stats_kernel, dim3(nn_stats_grid(n)), dim3(kNnStatThreads), 0, st,
                     scores, labels, n, out, sums);
  return hipGetLastError();
}

}  // namespace eegfx
