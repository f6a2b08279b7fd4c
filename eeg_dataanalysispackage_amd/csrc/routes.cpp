// routes.cpp -- which kernels a batch takes: the device-pointer pipelines behind the entry points
// of api.cpp, streamed.cpp and odp.cpp (declared in ctx.h).  Everything here runs on the context
// stream, on device pointers, after the arguments were checked.
#include "ctx.h"

namespace eegfx {

// Feature sizes past a6 ++ d6 take the full-pyramid kernels (pyramid.hip): EXACT under both
// numerics settings, outside the fma guard and its counters, and never the per-epoch kernel or
// the resident server (mailbox_request packs nfeat - 1 into 5 bits).
bool wide_features(int feature_size) { return feature_size > EEGFX_DWT8_FEATURE_SIZE; }

void run_features_from_raw(eegfx_ctx* ctx, const void* raw, int fmt, int64_t n_frames, int ct,
                           const ChanSel& sel, int C, const int64_t* pos, int64_t n, double* out) {
  const bool fast = ctx->numerics != EEGFX_EXACT;
  // fma: rows that fail the conditioning guard (guard.h) are recomputed under EXACT -- inside the
  // kernel that flags them, or (the generic any-layout kernels) by a follow-up launch over the
  // guard list that launch_window_wide issues; baseline_any_kernel zeroes the list's count
  const Guard g = ctx->guard_for(n);
  if (fused_supported(fmt, ct, C, out)) {
    void* fscratch = ctx->fused.get(fused_scratch_bytes(n, C));
    HIP_CHECK(launch_fused_baseline(ctx->stream, raw, n_frames, ct, sel, C, pos, n, fscratch,
                                    ctx->err_dev, nullptr, fast ? &g : nullptr));
    ctx->tic();  // the dominant kernel (DESIGN.md "Measurement")
    HIP_CHECK(launch_fused_window(ctx->stream, raw, n_frames, ct, sel, C, pos, n, fast, fscratch,
                                  out, g, fast && ctx->guard_track()));
    ctx->toc(n * fused_window_bytes_per_epoch(ct, C));
    return;
  }
  if (wide_supported(fmt, ct, C)) {
    void* fscratch = ctx->fused.get(fused_scratch_bytes(n, C));
    HIP_CHECK(launch_baseline_any(ctx->stream, raw, fmt, n_frames, ct, sel, C, pos, n, fscratch,
                                  ctx->err_dev, g.count, fast ? &g : nullptr));
    ctx->tic();
    HIP_CHECK(launch_window_wide(ctx->stream, raw, fmt, n_frames, ct, sel, C, pos, n, fast,
                                 fscratch, out, g, fast && ctx->guard_track()));
    const int64_t elem = fmt == EEGFX_INT_16 ? 2 : 4;
    ctx->toc(n * (EEGFX_DWT8_EPOCH_SIZE * ct * elem + C * 4 + 8 + C * 16 * 8));
    return;
  }
  double* ep = (double*)ctx->scratch.get(sizeof(double) * (size_t)n * C * EEGFX_POSTSTIMULUS);
  ctx->tic();
  HIP_CHECK(launch_cut_epochs(ctx->stream, raw, fmt, n_frames, ct, sel, C, pos, n, ep,
                              ctx->fused.get(fused_scratch_bytes(n, C)), ctx->err_dev));
  run_features_from_epochs(ctx, ep, n, C, EEGFX_DWT8_SKIP, EEGFX_DWT8_FEATURE_SIZE, out,
                           EEGFX_POSTSTIMULUS, &g);
  ctx->toc(0);
}

template <typename E>
void run_epochs_and_features(eegfx_ctx* ctx, const void* raw, int fmt, int64_t n_frames, int ct,
                             const ChanSel& sel, int C, const int64_t* pos, int64_t n, E* ep,
                             double* feat) {
  const bool fast = ctx->numerics != EEGFX_EXACT;
  const Guard g = ctx->guard_for(n);
  void* fscratch = ctx->fused.get(fused_scratch_bytes(n, C));
  ctx->tic();
  if (cut_features_supported(fmt, ct, C, raw, ep, feat)) {
    HIP_CHECK(launch_cut_features(ctx->stream, raw, fmt, n_frames, ct, sel, C, pos, n, ep, feat,
                                  fast, fscratch, ctx->err_dev, g));
  } else {
    HIP_CHECK(launch_cut_epochs(ctx->stream, raw, fmt, n_frames, ct, sel, C, pos, n, ep, fscratch,
                                ctx->err_dev));
    run_features_from_epochs(ctx, (const E*)ep, n, C, EEGFX_DWT8_SKIP, EEGFX_DWT8_FEATURE_SIZE,
                             feat, EEGFX_POSTSTIMULUS, &g);
  }
  ctx->toc(0);
}

template void run_epochs_and_features<double>(eegfx_ctx*, const void*, int, int64_t, int,
                                              const ChanSel&, int, const int64_t*, int64_t, double*,
                                              double*);
template void run_epochs_and_features<float>(eegfx_ctx*, const void*, int, int64_t, int,
                                             const ChanSel&, int, const int64_t*, int64_t, float*,
                                             double*);

template <typename E>
void run_features_from_epochs(eegfx_ctx* ctx, const E* ep, int64_t n, int C, int skip,
                              int feature_size, double* out, int row_stride,
                              const Guard* call_guard) {
  if (wide_features(feature_size)) {
    HIP_CHECK(launch_pyramid_from_epochs(ctx->stream, ep, n, C, skip, feature_size, out,
                                         row_stride));
    return;
  }
  const Guard g = call_guard ? *call_guard : ctx->guard_for(n);
  HIP_CHECK(launch_features_from_epochs(ctx->stream, ep, n, C, skip, feature_size,
                                        ctx->numerics != EEGFX_EXACT, out, row_stride, g));
}

template void run_features_from_epochs<double>(eegfx_ctx*, const double*, int64_t, int, int, int,
                                               double*, int, const Guard*);
template void run_features_from_epochs<float>(eegfx_ctx*, const float*, int64_t, int, int, int,
                                              double*, int, const Guard*);

}  // namespace eegfx
