// nn.cpp -- the train_clf=nn drivers of the eegfx C ABI (eegfx_nn_param_count, eegfx_nn_train,
// eegfx_nn_train_opt, eegfx_nn_predict, eegfx_nn_statistics) over the kernels of nn.hip (DESIGN.md
// sections 10.7 and 10.8).
#include <cstring>
#include <vector>

#include "ctx.h"

namespace {

// The model of a config, checked: what is refused names the reference's config key and the value.
NnNet nn_check_model(int32_t d, const eegfx_nn_config* cfg) {
  if (!cfg) fail(EEGFX_EINVAL, "null argument");
  check_train_d(d);
  const int L = cfg->n_layers;
  if (L < 1 || L > kNnMaxLayers)
    fail(EEGFX_EINVAL, "%d layers (the config_layer* keys / 4): 1 to %d are supported", L,
         kNnMaxLayers);
  NnNet net{};
  net.L = L;
  net.d = d;
  int off = 0;
  for (int l = 0; l < L; ++l) {
    const int no = cfg->n_out[l], act = cfg->activation[l];
    if (l < L - 1 && (no < 1 || no > kNnMaxWidth))
      fail(EEGFX_EINVAL, "config_layer%d_n_out=%d: a dense layer's width lies in [1, %d]", l + 1,
           no, kNnMaxWidth);
    if (l == L - 1 && no != 2)
      fail(EEGFX_EINVAL,
           "config_layer%d_n_out=%d: the output layer's n_out must be 2 (the labels are "
           "{t, |1 - t|})", l + 1, no);
    if (act < EEGFX_NN_ACT_SIGMOID || act > EEGFX_NN_ACT_SOFTMAX)
      fail(EEGFX_EINVAL, "config_layer%d_activation_function: code %d is no EEGFX_NN_ACT_*", l + 1,
           act);
    net.n_in[l] = l == 0 ? d : cfg->n_out[l - 1];
    net.n_out[l] = no;
    net.act[l] = act;
    net.w_off[l] = off;
    off += net.n_in[l] * no + no;
  }
  net.P = off;
  if (cfg->loss < EEGFX_NN_LOSS_MSE || cfg->loss > EEGFX_NN_LOSS_SQUARED)
    fail(EEGFX_EINVAL, "config_loss_function: code %d is no EEGFX_NN_LOSS_*", cfg->loss);
  if (cfg->updater < EEGFX_NN_UPD_NESTEROVS || cfg->updater > EEGFX_NN_UPD_RMSPROP)
    fail(EEGFX_EINVAL, "config_updater: code %d is no EEGFX_NN_UPD_*", cfg->updater);
  net.loss = cfg->loss;
  net.updater = cfg->updater;
  return net;
}

// The one training driver, inside the caller's `guarded`.  opt null or algorithm SGD: the
// reference's plain loop of updater steps (search_out is never written, every iteration runs).
// Otherwise one of the line-search optimisers; opt's own fields have been checked by the caller.
void nn_train_impl(eegfx_ctx* ctx, const double* X, const double* y, int64_t n, int32_t d,
                   const eegfx_nn_config* cfg, const eegfx_nn_optimizer* opt,
                   const double* params0, double* params_out, double* scores_out,
                   eegfx_nn_search* search_out, int32_t* iterations_run, int mem) {
  static_assert(sizeof(NnSearchRec) == sizeof(eegfx_nn_search), "eegfx_nn_search's layout");
  if (!ctx || !cfg || !params0 || !params_out) fail(EEGFX_EINVAL, "null argument");
  check_mem(mem);
  if (n < 1) fail(EEGFX_EINVAL, "empty training set");
  if (!X || !y) fail(EEGFX_EINVAL, "null X / y");
  const NnNet net = nn_check_model(d, cfg);
  const int iters = cfg->num_iterations;
  if (iters < 0) fail(EEGFX_EINVAL, "config_num_iterations=%d", iters);
  const bool sgd = !opt || opt->algorithm == EEGFX_NN_OPT_SGD;
  const size_t P = (size_t)net.P;
  if (!sgd && iters == 0) {  // no device work: the labels are not validated (the SGD loop does)
    memmove(params_out, params0, sizeof(double) * P);
    if (iterations_run) *iterations_run = 0;
    return;
  }
  ctx->activate();
  const TrainXY rows = stage_xy(ctx, X, y, n, d, mem);
  const size_t head = sizeof(NnState) + sizeof(double) * P;  // the state and the parameters
  const size_t sbytes = head + 2 * sizeof(double) * P;       // ... and the updater's state
  std::vector<uint8_t> hs(sbytes, 0);
  NnState* h = (NnState*)hs.data();
  memcpy(nn_params(h), params0, sizeof(double) * P);
  NnState* st = (NnState*)ctx->nn_state.get(sbytes);
  HIP_CHECK(hipMemcpyAsync(st, hs.data(), sbytes, hipMemcpyHostToDevice, ctx->stream));
  HIP_CHECK(launch_nn_validate(ctx->stream, rows.y, n, st));
  const NnTile tl = nn_plan_tile(net);
  const int G = nn_grid(n, net, tl);
  double *part = nullptr, *dscores = nullptr;
  if (iters > 0) {
    part = (double*)ctx->nn_part.get(sizeof(double) * (size_t)G * (P + 1));
    if (!sgd || scores_out) dscores = (double*)ctx->nn_scores.get(sizeof(double) * (size_t)iters);
  }
  const int64_t pass_bytes = n * (int64_t)sizeof(double) * (d + 1);
  NnOpt* dopt = nullptr;
  NnSearchRec* dsearch = nullptr;
  if (sgd) {
    for (int i = 0; i < iters; ++i) {
      ctx->tic();
      HIP_CHECK(launch_nn_gradient(ctx->stream, rows.X, rows.y, n, net, tl, G, st, part,
                                   cfg->learning_rate, cfg->momentum, nullptr, dscores));
      ctx->toc(pass_bytes);
    }
  } else {
    const int max_ls = opt->max_line_search_iterations;
    const int vectors = opt->algorithm == EEGFX_NN_OPT_LBFGS ? kNnOptVectorsLbfgs : kNnOptVectors;
    dopt = (NnOpt*)ctx->nn_opt.get(sizeof(NnOpt) + sizeof(double) * P * (size_t)vectors);
    HIP_CHECK(hipMemsetAsync(dopt, 0, sizeof(NnOpt), ctx->stream));
    dsearch = (NnSearchRec*)ctx->nn_search.get(sizeof(NnSearchRec) * (size_t)iters);
    // The fixed worst-case sequence: the kernels of a search that has ended, or of a training
    // that has terminated, return at once, so nothing is read back before the end.
    auto gradient_and_direction = [&](bool first) {
      HIP_CHECK(launch_nn_gradient(ctx->stream, rows.X, rows.y, n, net, tl, G, st, part,
                                   cfg->learning_rate, cfg->momentum, dopt, nullptr));
      HIP_CHECK(launch_nn_direction(ctx->stream, net, opt->algorithm, iters, first, st, dopt,
                                    dscores, dsearch));
    };
    gradient_and_direction(true);
    for (int i = 0; i < iters; ++i) {
      ctx->tic();
      for (int k = 0; k < max_ls; ++k)
        HIP_CHECK(launch_nn_trial(ctx->stream, rows.X, rows.y, n, net, tl, G, st, dopt, part,
                                  max_ls, dsearch));
      gradient_and_direction(false);
      ctx->toc(pass_bytes);
    }
  }
  NnOpt hopt{};
  std::vector<double> scores((size_t)(dscores ? iters : 0));
  std::vector<NnSearchRec> search((size_t)(dsearch ? iters : 0));
  HIP_CHECK(hipMemcpyAsync(hs.data(), st, head, hipMemcpyDeviceToHost, ctx->stream));
  if (dopt)
    HIP_CHECK(hipMemcpyAsync(&hopt, dopt, sizeof(hopt), hipMemcpyDeviceToHost, ctx->stream));
  if (dscores)
    HIP_CHECK(hipMemcpyAsync(scores.data(), dscores, sizeof(double) * scores.size(),
                             hipMemcpyDeviceToHost, ctx->stream));
  if (dsearch)
    HIP_CHECK(hipMemcpyAsync(search.data(), dsearch, sizeof(NnSearchRec) * search.size(),
                             hipMemcpyDeviceToHost, ctx->stream));
  ctx->drain();
  if (h->flag == 2) fail(EEGFX_EINVAL, "%s", kBadLabels);
  const size_t run = sgd ? (size_t)iters : (size_t)hopt.iterations_run;
  memcpy(params_out, nn_params(h), sizeof(double) * P);
  if (scores_out && dscores) memcpy(scores_out, scores.data(), sizeof(double) * run);
  if (search_out && dsearch) memcpy(search_out, search.data(), sizeof(NnSearchRec) * run);
  if (iterations_run) *iterations_run = (int32_t)run;
}

}  // namespace

extern "C" {

int64_t eegfx_nn_param_count(int32_t d, const eegfx_nn_config* cfg) {
  int64_t count = 0;
  const int rc = guarded([&] { count = nn_check_model(d, cfg).P; });
  return rc == EEGFX_OK ? count : rc;
}

int eegfx_nn_train(eegfx_ctx* ctx, const double* X, const double* y, int64_t n, int32_t d,
                   const eegfx_nn_config* cfg, const double* params0, double* params_out,
                   double* scores_out, int mem) {
  return guarded([&] {
    nn_train_impl(ctx, X, y, n, d, cfg, nullptr, params0, params_out, scores_out, nullptr, nullptr,
                  mem);
  });
}

int eegfx_nn_train_opt(eegfx_ctx* ctx, const double* X, const double* y, int64_t n, int32_t d,
                       const eegfx_nn_config* cfg, const eegfx_nn_optimizer* opt,
                       const double* params0, double* params_out, double* scores_out,
                       eegfx_nn_search* search_out, int32_t* iterations_run, int mem) {
  return guarded([&] {
    if (!opt) fail(EEGFX_EINVAL, "null argument");
    if (opt->algorithm < EEGFX_NN_OPT_SGD || opt->algorithm > EEGFX_NN_OPT_LBFGS)
      fail(EEGFX_EINVAL, "algorithm=%d is no EEGFX_NN_OPT_*", opt->algorithm);
    if (opt->max_line_search_iterations < 1 || opt->max_line_search_iterations > 32)
      fail(EEGFX_EINVAL, "max_line_search_iterations=%d outside [1, 32]",
           opt->max_line_search_iterations);
    nn_train_impl(ctx, X, y, n, d, cfg, opt, params0, params_out, scores_out, search_out,
                  iterations_run, mem);
  });
}

int eegfx_nn_predict(eegfx_ctx* ctx, const double* X, int64_t n, int32_t d,
                     const eegfx_nn_config* cfg, const double* params, double* out, int mem) {
  return guarded([&] {
    if (!ctx || !cfg || !params) fail(EEGFX_EINVAL, "null argument");
    check_mem(mem);
    check_predict_dims(n, d);
    const NnNet net = nn_check_model(d, cfg);
    if (n == 0) return;
    if (!X || !out) fail(EEGFX_EINVAL, "null X / out");
    predict_frame(ctx, X, n, d, out, mem, [&](const double* dX, double* dout) {
      const size_t bytes = sizeof(double) * (size_t)net.P;
      double* dp = (double*)ctx->nn_state.get(bytes);
      HIP_CHECK(hipMemcpyAsync(dp, params, bytes, hipMemcpyHostToDevice, ctx->stream));
      HIP_CHECK(launch_nn_predict(ctx->stream, dX, n, net, nn_plan_tile(net), dp, dout));
    });
  });
}

int eegfx_nn_statistics(eegfx_ctx* ctx, const double* scores, const double* labels, int64_t n,
                        int64_t counts[4], double sums[3], int mem) {
  return guarded([&] {
    if (!ctx || !counts || !sums) fail(EEGFX_EINVAL, "null argument");
    check_mem(mem);
    if (n < 0) fail(EEGFX_EINVAL, "n=%lld", (long long)n);
    if (n > 0 && (!scores || !labels)) fail(EEGFX_EINVAL, "null scores / labels");
    NnStatsOut h;
    memset(&h, 0, sizeof(h));
    double total[3] = {0.0, 0.0, 0.0};
    if (n > 0) {
      ctx->activate();
      const size_t bytes = sizeof(double) * (size_t)n;
      const double* d_scores = stage_in(ctx, ctx->nn_in, scores, bytes, mem);
      const double* d_labels = stage_in(ctx, ctx->row_vals, labels, bytes, mem);
      const int G = nn_stats_grid(n);
      std::vector<double> part((size_t)G * 3);
      const size_t pbytes = sizeof(double) * part.size();
      NnStatsOut* out = (NnStatsOut*)ctx->nn_stat.get(sizeof(NnStatsOut) + pbytes);
      double* d_part = (double*)(out + 1);
      HIP_CHECK(hipMemsetAsync(out, 0, sizeof(*out), ctx->stream));
      HIP_CHECK(launch_nn_stats(ctx->stream, d_scores, d_labels, n, out, d_part));
      HIP_CHECK(hipMemcpyAsync(&h, out, sizeof(h), hipMemcpyDeviceToHost, ctx->stream));
      HIP_CHECK(hipMemcpyAsync(part.data(), d_part, pbytes, hipMemcpyDeviceToHost, ctx->stream));
      ctx->drain();
      for (int b = 0; b < G; ++b)  // the workgroups' sums, in workgroup order
        for (int k = 0; k < 3; ++k) total[k] += part[(size_t)b * 3 + k];
    }
    for (int k = 0; k < 4; ++k) counts[k] = (int64_t)h.cell[k];
    for (int k = 0; k < 3; ++k) sums[k] = total[k];
  });
}

}  // extern "C"
