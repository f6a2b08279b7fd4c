// launch.h -- host-side launchers of the gfx950 kernels (cut.hip, extract.hip, small.hip,
// synth.hip, fused.hip, wide.hip, pyramid.hip).
#pragma once

#include <hip/hip_runtime_api.h>

#include <cstdint>

#include "guard.h"

namespace eegfx {

constexpr int kMaxChannels = 64;

// Selected channels, passed by value as a kernel argument: 0-based column in the multiplexed
// frame and the .vhdr resolution (narrowed to float, as the reference multiplies in fp32).
struct ChanSel {
  int32_t col[kMaxChannels];
  float res[kMaxChannels];
};

// err: device-visible int (the context's host-mapped error word) set to 1 when a kernel reads a
// marker position the reference would not cut (pos - 100 outside [0, n_frames]); may be null.
// scratch: fused_scratch_bytes(n, C) bytes for the baselines (nullptr: single-kernel fallback)
hipError_t launch_cut_epochs(hipStream_t st, const void* raw, int fmt, int64_t n_frames, int ct,
                             const ChanSel& sel, int C, const int64_t* pos, int64_t n,
                             double* out, void* scratch, int* err);
// The same epochs as float[n][C][750] (eegfx_cut_epochs_f32): the fp32 value the double form
// widens, stored as it is; `out` may sit on any 4-byte boundary.
hipError_t launch_cut_epochs(hipStream_t st, const void* raw, int fmt, int64_t n_frames, int ct,
                             const ChanSel& sel, int C, const int64_t* pos, int64_t n,
                             float* out, void* scratch, int* err);
// The one-pass getData + features (cut.hip staged_features): baselines, then one workgroup
// per epoch writes the epoch's rows to `out` (double[n][C][750]) and its normalised dwt-8 row to
// `feat` (double[n][16 C]) from the same LDS-staged frames.  hipErrorNotSupported when the layout
// does not fit (cut_features_supported): the caller cuts, then extracts from the rows.
bool cut_features_supported(int fmt, int ct, int C, const void* raw, const double* out,
                            const double* feat);
hipError_t launch_cut_features(hipStream_t st, const void* raw, int fmt, int64_t n_frames, int ct,
                               const ChanSel& sel, int C, const int64_t* pos, int64_t n,
                               double* out, double* feat, bool fast, void* scratch, int* err,
                               const Guard& guard);
// float epochs (eegfx_process_recording_epochs_f32): the same kernels, the same rows in `feat`
bool cut_features_supported(int fmt, int ct, int C, const void* raw, const float* out,
                            const double* feat);
hipError_t launch_cut_features(hipStream_t st, const void* raw, int fmt, int64_t n_frames, int ct,
                               const ChanSel& sel, int C, const int64_t* pos, int64_t n,
                               float* out, double* feat, bool fast, void* scratch, int* err,
                               const Guard& guard);
// row_stride: elements between consecutive (epoch, channel) rows of `ep` (750 for materialised
// epochs, 512 for the window-only rows the host path stages)
// guard (fma numerics): the conditioning guard (guard.h); flagged rows are recomputed under EXACT
// inside the kernel and counted in guard.total.
hipError_t launch_features_from_epochs(hipStream_t st, const double* ep, int64_t n, int C, int skip,
                                       int nfeat, bool fast, double* out, int row_stride,
                                       const Guard& guard);
// float epochs (eegfx_extract_features_f32; any 4-byte-aligned `ep`): widened as the windows are
// staged, the rows are those of the double form on the widened epochs
hipError_t launch_features_from_epochs(hipStream_t st, const float* ep, int64_t n, int C, int skip,
                                       int nfeat, bool fast, double* out, int row_stride,
                                       const Guard& guard);
// double[count] -> float[count] on the device (eegfx_odp_get_data_f32); 16-byte-aligned buffers
hipError_t launch_narrow_epochs(hipStream_t st, const double* in, float* out, int64_t count);
// Small host batches (small.hip features_small_kernel): rows = n x C x 512 packed window rows,
// one workgroup per epoch, C <= 16; rows / out may be device pointers of mapped pinned memory.
bool features_small_supported(int C);
// guard.total counts the rows the kernel recomputed under EXACT (guard.h); count/list unused.
// The resident small-batch server (eegfx_ctx_set_mailbox): a host-mapped command block, written
// by the host except `done` (the device's last completed request).
struct MailboxCmd {
  // The request word, written last by the host (release): sequence number << 32 | (C - 1) << 26 |
  // (nfeat - 1) << 21 | n -- the whole request in one aligned 64-bit load, so the kernel needs no
  // second round trip across the host link for its fields (bit 31 unused: the per-epoch path
  // computes EXACT rows under both numerics).
  uint64_t req;
  uint32_t done;  // the last sequence number whose rows are in `out` (device)
  uint32_t stop;  // 1: the kernel returns
  uint32_t alive;  // the launch generation of the kernel that has started (device, at entry)
  uint32_t pad_;
  // staging, fixed while a server runs (growing it stops the server first); read at kernel start
  const double* rows;  // device-mapped pinned [n][C][512] window doubles
  double* out;         // device-mapped pinned [n][C * nfeat] rows
};
inline uint64_t mailbox_request(uint32_t seq, int C, int nfeat, int64_t n) {
  return (uint64_t)seq << 32 | (uint64_t)(C - 1) << 26 | (uint64_t)(nfeat - 1) << 21 |
         (uint64_t)n;
}
hipError_t launch_features_mailbox(hipStream_t st, MailboxCmd* mb, uint64_t idle_ticks,
                                   uint32_t gen);
hipError_t launch_features_small(hipStream_t st, const double* rows, int64_t n, int C, int nfeat,
                                 double* out);
hipError_t launch_synth(hipStream_t st, int16_t* dst, int64_t n_frames, int ct, uint64_t seed);

// Non-temporal reads pay when the regions neighbouring epochs read do not overlap: the average
// marker spacing n_frames / n is at least min_spacing frames (fused.hip).
bool streaming_reads(int64_t n_frames, int64_t n, int64_t min_spacing);

// Fused raw -> features (fused.hip): baseline_kernel then window_kernel.  `scratch` holds
// fused_scratch_bytes(n, C) bytes of device memory (the per-epoch baselines).  fused_supported
// says whether the 3-channel kernels cover (fmt, ct, C); the any-layout kernels of wide.hip take
// the rest.
bool fused_supported(int fmt, int ct, int C, const double* out);
size_t fused_scratch_bytes(int64_t n, int C);
// guard_count: zeroed by the baseline kernel when not null (the 3-channel window kernel recomputes
// the rows that fail the fma conditioning guard itself and uses guard.total only).
hipError_t launch_fused_baseline(hipStream_t st, const void* raw, int64_t n_frames, int ct,
                                 const ChanSel& sel, int C, const int64_t* pos, int64_t n,
                                 void* scratch, int* err, int* guard_count,
                                 const Guard* guard = nullptr);
hipError_t launch_fused_window(hipStream_t st, const void* raw, int64_t n_frames, int ct,
                               const ChanSel& sel, int C, const int64_t* pos, int64_t n, bool fast,
                               const void* scratch, double* out, const Guard& guard,
                               bool track = false);
// Algorithmic HBM bytes per epoch of window_kernel (the dominant kernel): window frames, the
// baseline and marker position it reads, the feature row it writes.
int64_t fused_window_bytes_per_epoch(int ct, int C);

// Any-layout fused path (wide.hip): baseline_any_kernel then window_wide_kernel, same scratch
// contract as the 3-channel kernels.  wide_supported: int16/float32, C <= 64, one epoch's staged
// window + features within 64 KB of LDS (int16: about 60 channels in the file).
bool wide_supported(int fmt, int ct, int C);
bool baseline_any_supported(int fmt, int ct, int C);
hipError_t launch_baseline_any(hipStream_t st, const void* raw, int fmt, int64_t n_frames, int ct,
                               const ChanSel& sel, int C, const int64_t* pos, int64_t n,
                               void* scratch, int* err, int* guard_count,
                               const Guard* guard = nullptr);
hipError_t launch_window_wide(hipStream_t st, const void* raw, int fmt, int64_t n_frames, int ct,
                              const ChanSel& sel, int C, const int64_t* pos, int64_t n, bool fast,
                              const void* scratch, double* out, const Guard& guard,
                              bool track = false);

// The full pyramid (pyramid.hip): feature sizes 17..512, EXACT under both numerics settings, no
// guard.  ep / row_stride / skip as launch_features_from_epochs; out = double[n][C * nfeat].
hipError_t launch_pyramid_from_epochs(hipStream_t st, const double* ep, int64_t n, int C, int skip,
                                      int nfeat, double* out, int row_stride);
hipError_t launch_pyramid_from_epochs(hipStream_t st, const float* ep, int64_t n, int C, int skip,
                                      int nfeat, double* out, int row_stride);

// guard.hip: the EXACT recomputation of the rows the generic any-layout kernels flagged (no-op
// when g.count is null; launch_window_wide issues it).  raw: the same recording / positions /
// baselines (scratch) as the fused launch.
hipError_t launch_guard_fixup_raw(hipStream_t st, const void* raw, int fmt, int64_t n_frames,
                                  int ct, const ChanSel& sel, int C, const int64_t* pos,
                                  const void* scratch, const Guard& g, double* out);

// logreg.hip: MLlib LogisticRegressionWithSGD (full batch) on device.  State block: iteration
// count, flag (0 running, 1 converged / done), then the d weights.  lr_validate_kernel's verdict
// goes to a header of its own behind them (sharded.cpp validity_word).
struct LrState {
  int32_t iter;       // iterations done (GradientDescent's i - 1)
  int32_t converged;  // 1: converged or done; in the validity word, 2: label validation failed
  int32_t updates;    // iterations that updated the weights (a non-empty mini-batch)
  int32_t pad;
  double w[];
};
constexpr int kLrMaxFeatures = 1024;

// plan.hip: marker planning (a4 + a8) as a scan over 3-state balance maps.
struct PlanResult {
  int64_t selected;          // accepted markers
  int64_t balance;           // final class balance
  int64_t first_unparsable;  // index of the first INT32_MIN stimulus index, -1 if none
};
size_t plan_scratch_bytes(int64_t n);
hipError_t launch_plan_markers(hipStream_t st, const int64_t* pos, const int32_t* stim, int64_t n,
                               int64_t n_frames, int32_t guessed, int d0, void* scratch,
                               int64_t* pos_out, double* label_out, PlanResult* result);
int lr_grid(int64_t n);
hipError_t launch_lr_validate(hipStream_t st, const double* y, int64_t n, LrState* state);
// grad: kGradLogistic (LogisticRegressionWithSGD) or kGradHinge (SVMWithSGD); the predict
// kernel scores with the matching model (sigmoid of the margin / the margin itself).
constexpr int kGradLogistic = 0;
constexpr int kGradHinge = 1;
hipError_t launch_lr_predict(hipStream_t st, int grad, const double* X, int64_t n, int d,
                             const double* w, double intercept, double threshold,
                             int use_threshold, double* out);
// The pieces of an iteration, put together by the one driver (sharded.cpp): the gradient partials
// [G][d] of the rows X[n] (mask: the iteration's mini-batch sample, bit p of word p / 32 = row p
// of the whole list, nullptr = the whole batch; pos: row r is row pos[r] of the list, nullptr: r);
// with more than one shard, those partials as one d-vector `out`, in lr_update_kernel's order of
// summation; the update from G partials with `count` > 0 rows, the sample's, as the divisor; the
// step of an empty sample (count 0: no gradient, no update).
hipError_t launch_lr_gradient(hipStream_t st, int grad, const double* X, const double* y,
                              int64_t n, int d, const uint32_t* mask, const int64_t* pos,
                              const LrState* state, double* partial, int G);
hipError_t launch_lr_fold(hipStream_t st, const double* partial, int G, int d,
                          const LrState* state, double* out);
hipError_t launch_lr_update(hipStream_t st, const double* partial, int G, int64_t count, int d,
                            LrState* state, double step_size, double reg, double tol,
                            int max_iter);
hipError_t launch_lr_skip(hipStream_t st, LrState* state, int max_iter);


// blocks for `items` at `per_block` a block: at least 1, at most `cap` (grid-stride kernels)
inline unsigned grid_for(int64_t items, int per_block, int64_t cap) {
  const int64_t g = (items + per_block - 1) / per_block;
  return (unsigned)(g < 1 ? 1 : (g > cap ? cap : g));
}

// dtree.hip: the O(n d) passes of the decision tree (eegfx_dtree_*; the host half is dtree_host.h,
// the driver tree_driver.cpp).
struct DtDecision {   // one queued node's outcome, read by rf_route_kernel
  int32_t feature;    // -1: the node became a leaf
  int32_t split;      // bins 0..split go left
  int32_t left, right;  // the children's queue tickets, -1: leaf
};
struct DtNode {       // one node as dt_predict_kernel walks it
  int32_t feature, left, right, pad;
  double threshold, predict;
};
constexpr int kDtMaxBins = 256;
// counters (uint32) of the histogram kernel's LDS: 128 KB of a gfx950 CU's 160 KB
constexpr int kDtLdsCounters = 32768;
// X -> bins uint8 [n][d] (the thresholds below the value, of feature f's nthr[f] ascending ones at
// thr[f * T]), label uint8 [n], slot int32 [n] = 0.  flags[0] = 1: a non-finite feature;
// flags[1] = 1: a label other than 0.0 / 1.0 (both zeroed by the caller).
hipError_t launch_dt_bin(hipStream_t st, const double* X, const double* y, int64_t n, int d,
                         int T, const int32_t* nthr, const double* thr, int32_t* flags,
                         uint8_t* bins, uint8_t* label, int32_t* slot);
// hist uint32 [g][d][B][2] (zeroed by the caller) += the rows whose slot lies in [g0, g0 + g);
// privatised in LDS when g * d * B * 2 <= kDtLdsCounters, else global atomics
hipError_t launch_dt_hist(hipStream_t st, const uint8_t* bins, const uint8_t* label,
                          const int32_t* slot, int64_t n, int d, int B, int g0, int g,
                          uint32_t* hist);
// rows idx[0..m) of X, packed
hipError_t launch_dt_gather(hipStream_t st, const double* X, int d, const int64_t* idx, int64_t m,
                            double* out);
hipError_t launch_dt_predict(hipStream_t st, const double* X, int64_t n, int d,
                             const DtNode* nodes, int n_nodes, double* out);

// rforest.hip: the passes of the random forest over every tree's rows (eegfx_rforest_*; the host
// half is rforest_host.h).  weight uint8 [tree][row], slot int32 [tree][row]: the queue ticket of
// the row's node in that tree, -1: a leaf or weight 0.
hipError_t launch_rf_init(hipStream_t st, const uint8_t* weight, int64_t n, int num_trees,
                          int32_t* slot);
// hist uint32 [g][k][B][2] (zeroed by the caller) += the weights of the rows whose slot lies in
// [s0, s0 + g), over trees[nt] (the distinct trees of those nodes); sub int32 [g][k]: the features
// of each node, nullptr: features 0..k-1 (k == d).  Privatised in LDS when g * k * B * 2 <=
// kDtLdsCounters, else global atomics.
hipError_t launch_rf_hist(hipStream_t st, const uint8_t* bins, const uint8_t* label,
                          const uint8_t* weight, const int32_t* slot, int64_t n, int d, int B,
                          int k, int s0, int g, const int32_t* trees, int nt, const int32_t* sub,
                          uint32_t* hist);
// dec[g]: the outcome of tickets [s0, s0 + g), left / right = the children's tickets; rows of other
// tickets (nodes still queued) keep theirs.  The single unweighted tree: trees -> {0}, nt = 1 and
// dt_bin_kernel's slot column.
hipError_t launch_rf_route(hipStream_t st, const uint8_t* bins, int64_t n, int d,
                           const int32_t* trees, int nt, int s0, int g, const DtDecision* dec,
                           int32_t* slot);
// nodes: the trees concatenated, children relative to their tree's first node; offsets[trees + 1]
hipError_t launch_rf_predict(hipStream_t st, const double* X, int64_t n, int d,
                             const DtNode* nodes, const int32_t* offsets, int num_trees,
                             double* out);

// flow.hip: the train/test flow's row gather and confusion counts (eegfx_gather_rows,
// eegfx_confusion_counts, eegfx_odp_split).
constexpr int kGatherMaxD = 1536;      // 3 channels x the extractor's largest feature size
constexpr int kGatherThreads = 256;
constexpr int kGatherUnroll = 4;       // pieces a thread moves per trip of its grid-stride loop
constexpr int kGatherMaxBlocks = 2048;  // 8 workgroups for each of the 256 CUs
// dst[i][0:d] = src[idx[i]][0:d] for i < m, bits copied; 16-byte pieces when d is even and src
// and dst lie on 16-byte boundaries, else 8-byte pieces.  An idx[i] outside [0, n_src) copies
// nothing for row i and lowers *bad (set to ~0 by the caller) to the smallest such i.
hipError_t launch_gather_rows(hipStream_t st, const double* src, int64_t n_src, int d,
                              const int64_t* idx, int64_t m, double* dst, unsigned long long* bad);
constexpr int kConfusionThreads = 256;
constexpr unsigned kSeenZero = 1, kSeenOne = 2, kSeenOther = 4;
struct ConfusionOut {          // zeroed by the caller
  unsigned long long cell[4];  // tp, tn, fp, fn as classification.reference_statistics reads them
  unsigned seen;               // kSeen* of the labels: 0.0, 1.0, anything else
  unsigned pad;
};
hipError_t launch_confusion(hipStream_t st, const double* pred, const double* labels, int64_t n,
                            ConfusionOut* out);
// logreg.hip lr_count_kernel: the rows X[n] scored as launch_lr_predict scores them and counted
// against y[n] as launch_confusion counts, without the predictions in memory; `out` accumulates.
constexpr int kLrCountMaxBlocks = 2048;  // 4 rows per workgroup and trip
hipError_t launch_lr_count(hipStream_t st, int grad, const double* X, const double* y, int64_t n,
                           int d, const double* w, double intercept, double threshold,
                           int use_threshold, ConfusionOut* out);

// nn.hip: the dense network of train_clf=nn (eegfx_nn_*).  The codes are
// those of eegfx.h (EEGFX_NN_ACT_*, EEGFX_NN_LOSS_*, EEGFX_NN_UPD_*).
constexpr int kNnMaxLayers = 4;
constexpr int kNnMaxWidth = 64;
struct NnNet {               // the checked model
  int32_t L, d, P;           // layers, features, parameters
  int32_t loss, updater;
  int32_t n_in[kNnMaxLayers], n_out[kNnMaxLayers], act[kNnMaxLayers];
  int32_t w_off[kNnMaxLayers];  // layer l in the flat vector: W [n_in][n_out], then b [n_out]
};
// How a workgroup lays one tile of `rows` feature rows out in LDS (offsets and strides in
// doubles; every stride is odd, so lanes that differ in the row meet different banks).  A
// function of the model alone (nn_plan_tile).
struct NnTile {
  int32_t rows;      // feature rows per tile
  int32_t w1_lds;    // 1: layer 1's weights are staged in LDS; 0: read through L2 (wide d)
  int32_t doubles;   // LDS of the workgroup
  int32_t x_off, x_stride;   // the rows' features [rows][x_stride]
  int32_t y_off, loss_off;   // label / loss of each row
  int32_t w_lds[kNnMaxLayers], w_stride[kNnMaxLayers], b_lds[kNnMaxLayers];
  int32_t a_off[kNnMaxLayers], z_off[kNnMaxLayers], a_stride[kNnMaxLayers];
};
struct NnState {     // followed by double params[P], s1[P], s2[P] (the updater's state)
  int32_t iter;      // iterations done
  int32_t flag;      // 2: label validation failed (every kernel then returns at once)
  uint32_t ticket;   // nn_last_workgroup's count for the running nn_update_kernel
  int32_t pad;
};
inline double* nn_params(NnState* st) { return (double*)(st + 1); }
NnTile nn_plan_tile(const NnNet& net);
int nn_grid(int64_t n, const NnNet& net, const NnTile& tl);
hipError_t launch_nn_validate(hipStream_t st, const double* y, int64_t n, NnState* state);
hipError_t launch_nn_predict(hipStream_t st, const double* X, int64_t n, const NnNet& net,
                             const NnTile& tl, const double* params, double* out);
// The line-search optimisers of eegfx_nn_train_opt.  NnState::flag 1:
// training has terminated (ZeroDirection / EpsTermination); every kernel then returns at once.
constexpr int kNnLbfgsM = 4;       // LBFGS history
constexpr int kNnOptVectors = 6;   // g, g_new, dir, cand, p_old, g_old ...
constexpr int kNnOptVectorsLbfgs = kNnOptVectors + 2 * kNnLbfgsM;  // ... s[m], y[m]
struct NnLine {                    // BackTrackLineSearch's state between two trials
  double s0, slope, step_min;      // the score at p, -dot(dir, g), relTolx / test
  double step, step2, sc, sc2;     // this trial's step and the one before, with their scores
  double best, best_step;
  int32_t trials;                  // trials evaluated in this search
  int32_t done;                    // 1: the search of iteration `it` has ended
};
struct NnSearchRec {               // eegfx_nn_search
  double step, score;
  int32_t trials, pad;
};
struct NnOpt {       // followed by double [kNnOptVectors or kNnOptVectorsLbfgs][P]
  NnLine line;
  double score, score_new;         // the loss at p; what the last gradient pass reported
  double rho[kNnLbfgsM];           // LBFGS ring: 1 / (dot(s, y) + EPS) per slot
  int32_t it;                      // the iteration the search state belongs to
  int32_t iterations_run;
  int32_t hist, head;              // LBFGS: pairs held, slot of the newest
  uint32_t ticket;                 // nn_last_workgroup's count for the running nn_search_kernel
  int32_t pad;
};
// nn_grad_kernel, then nn_update_kernel.  partial: double [G][P + 1] (the workgroup's gradient
// sums, then its loss sum).  opt null: an SGD step (nn_update_kernel<false>; scores: null or one
// loss per iteration).  opt set: the gradient pass of the optimisers (nn_update_kernel<true>: the
// updater's output stored as g_new, the loss as NnOpt::score_new; NnState::iter counts the passes).
hipError_t launch_nn_gradient(hipStream_t st, const double* X, const double* y, int64_t n,
                              const NnNet& net, const NnTile& tl, int G, NnState* state,
                              double* partial, double lr, double momentum, NnOpt* opt,
                              double* scores);
// One trial: nn_score_kernel (the loss of NnOpt's candidate, in the gradient launch's tiles, grid
// and partial slots), then nn_search_kernel (the search's decision; search: one record per
// iteration).  Both return at once when the iteration's search has ended.
hipError_t launch_nn_trial(hipStream_t st, const double* X, const double* y, int64_t n,
                           const NnNet& net, const NnTile& tl, int G, NnState* state, NnOpt* opt,
                           double* partial, int max_ls, NnSearchRec* search);
// nn_direction_kernel: the next direction (algorithm: EEGFX_NN_OPT_*), both termination tests,
// scores[it + 1] and the set-up of the next search.  first: behind the gradient pass at params0.
hipError_t launch_nn_direction(hipStream_t st, const NnNet& net, int algorithm, int iterations,
                               bool first, NnState* state, NnOpt* opt, double* scores,
                               NnSearchRec* search);
struct NnStatsOut {                   // zeroed by the caller
  unsigned long long cell[4];         // tp, tn, fp, fn of ClassificationStatistics.add
};
int nn_stats_grid(int64_t n);
// sums: double [grid][3] = each workgroup's (label - score)^2, class-1 and class-2 score sums
hipError_t launch_nn_stats(hipStream_t st, const double* scores, const double* labels, int64_t n,
                           NnStatsOut* out, double* sums);

}  // namespace eegfx
