// sharded.cpp -- the MLlib SGD classifiers' one GradientDescent driver (glm_sgd_train_shards), over
// the kernels of logreg.hip, and the entries over rows that stay on several contexts
// (eegfx_glm_sgd_train_sharded, eegfx_glm_shard_state, eegfx_glm_count_sharded; DESIGN.md section
// 10.11).  The one-context entries of classify.cpp hand the driver their context as its one shard.
//
// GradientDescent's iteration is a sum over rows followed by a d-vector update, so it shards
// exactly: every shard sums the gradient of its own rows (the gradient kernel, then lr_fold_kernel:
// its G workgroup partials as one d-vector), the vectors meet in a [shards][d] slot buffer on the
// root -- the first shard with rows -- whose lr_update_kernel reads them as G = shards partials,
// and the root's LrState (flag, counters, weights) goes back to every shard's copy.  One host
// thread enqueues all of it in iteration order; nothing waits on the host and no kernel waits on
// another device's memory: the ordering is stream events alone.
//   shard s, iteration i   [wait back(i-1)]  gradient  fold  copy to slot s  record sent_s(i)
//   root,    iteration i   gradient  fold into slot 0  wait sent_s(i), all s  update
//                          copy the state to every s  record back(i)
// A lone shard needs none of that: its iteration is the gradient kernel and lr_update_kernel on its
// own G partials -- the sum the fold would have taken, in lr_fold_partials' order either way -- with
// no fold, slot buffer, event or copy.
// Hazards.  Slot s is rewritten by shard s's copy of iteration i+1, which its stream runs after
// back(i), recorded after the update of iteration i read the slot.  Shard s's state copy is
// overwritten by the root after the root's stream waited on sent_s(i), recorded after shard s's
// gradient and fold of iteration i read it.  So one slot buffer and one state copy per shard do.
// Every wait on an event is enqueued before the event is recorded again; the events still come in
// rings of two, so that a wait never depends on which record a runtime takes it to mean.
#include <cmath>
#include <cstring>
#include <vector>

#include "ctx.h"

namespace eegfx {
namespace {

constexpr int kEventRing = 2;

// The training state as a shard holds it: LrState with the d weights -- what the root sends
// round -- and behind it the word lr_validate_kernel reports this shard's labels in, which stays
// the shard's own.
size_t state_bytes(int d) { return sizeof(LrState) + sizeof(double) * (size_t)d; }
LrState* validity_word(LrState* st, int d) { return (LrState*)((char*)st + state_bytes(d)); }

struct Active {  // a shard with rows
  eegfx_ctx* ctx;
  const double* X;
  const double* y;
  const int64_t* pos;  // device; nullptr: the row's own index (only the shard at offset 0)
  int64_t n;
  int G;
  LrState* st;
  double* part;
  double* fold;        // root: the slots [active][d]; else this shard's d-vector; lone: none
  uint32_t* mask;
  hipEvent_t sent[kEventRing];
};

struct Events {  // created on their stream's device, destroyed with the call
  std::vector<hipEvent_t> all;
  hipEvent_t make(const eegfx_ctx* c) {
    c->activate();
    hipEvent_t e = nullptr;
    HIP_CHECK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    all.push_back(e);
    return e;
  }
  ~Events() {
    for (hipEvent_t e : all) (void)hipEventDestroy(e);
  }
};

void check_shards(const eegfx_glm_shard* shards, int32_t n_shards) {
  if (n_shards < 0 || (n_shards > 0 && !shards)) fail(EEGFX_EINVAL, "null argument");
  for (int32_t s = 0; s < n_shards; ++s) {
    if (!shards[s].ctx) fail(EEGFX_EINVAL, "shard %d: null context", s);
    if (shards[s].n < 0) fail(EEGFX_EINVAL, "shard %d: n=%lld", s, (long long)shards[s].n);
    if (shards[s].n > 0 && (!shards[s].X || !shards[s].y)) fail(EEGFX_EINVAL, "null X / y");
    for (int32_t t = 0; t < s; ++t)
      if (shards[t].ctx == shards[s].ctx)
        fail(EEGFX_EINVAL, "shard %d repeats the context of shard %d: the two would share its "
             "buffers", s, t);
  }
}

// Nothing of a failed call stays in flight: it reads the caller's rows and host vectors of ours.
template <typename F>
void drained_on_failure(const std::vector<Active>& act, F&& body) {
  try {
    body();
  } catch (...) {
    for (const Active& a : act) {
      (void)hipSetDevice(a.ctx->device);
      (void)hipStreamSynchronize(a.ctx->stream);
    }
    throw;
  }
}

}  // namespace

int glm_sgd_train_shards(int grad, const eegfx_glm_shard* shards, int32_t n_shards, int32_t d,
                         int32_t num_iterations, double step_size, double reg_param,
                         double mini_batch_fraction, double convergence_tol,
                         int32_t num_partitions, double* weights, int32_t* iterations_run,
                         int mem) {
  return guarded([&] {
    int64_t n_total = 0;
    for (int32_t s = 0; s < n_shards; ++s) n_total += shards[s].n;
    if (n_total < 1) fail(EEGFX_EINVAL, "empty training set");
    const bool sampled =
        check_sgd_args(grad, d, num_iterations, mini_batch_fraction, num_partitions);

    const size_t sbytes = state_bytes(d), vbytes = sizeof(LrState);
    std::vector<uint8_t> hs(sbytes + vbytes, 0);
    LrState* h = (LrState*)hs.data();
    h->converged = num_iterations == 0 ? 1 : 0;
    memcpy(h->w, weights, sizeof(double) * (size_t)d);  // initial weights (zeros in MLlib)

    std::vector<Active> act;
    std::vector<std::vector<int64_t>> own_pos;  // uploads in flight until the first drain
    Events events;
    const int64_t words = (n_total + 31) / 32;
    const int chunk = sampled ? sgd_mask_chunk(n_total, num_iterations) : 0;
    std::vector<std::vector<uint8_t>> finals;
    drained_on_failure(act, [&] {
      int64_t offset = 0;
      int32_t n_active = 0;
      for (int32_t s = 0; s < n_shards; ++s) n_active += shards[s].n > 0;
      for (int32_t s = 0; s < n_shards; offset += shards[s++].n) {
        const eegfx_glm_shard& in = shards[s];
        if (in.n == 0) continue;
        const bool root = act.empty();
        act.push_back({in.ctx, in.X, in.y, in.pos, in.n, lr_grid(in.n)});  // drained from here on
        Active& a = act.back();
        eegfx_ctx* c = a.ctx;
        c->activate();
        const TrainXY xy = stage_xy(c, in.X, in.y, in.n, d, mem);
        a.X = xy.X;
        a.y = xy.y;
        a.st = (LrState*)c->lr_state.get(sbytes + vbytes);
        a.part = (double*)c->lr_part.get(sizeof(double) * (size_t)a.G * d);
        if (n_active > 1)
          a.fold = (double*)c->lr_fold.get(sizeof(double) * (size_t)d * (root ? n_active : 1));
        a.mask = sampled ? (uint32_t*)c->lr_mask.get(sizeof(uint32_t) * (size_t)(chunk * words))
                         : nullptr;
        if (sampled && !a.pos && offset > 0) {
          own_pos.emplace_back((size_t)a.n);
          for (int64_t r = 0; r < a.n; ++r) own_pos.back()[(size_t)r] = offset + r;
          int64_t* p = (int64_t*)c->lr_pos.get(sizeof(int64_t) * (size_t)a.n);
          HIP_CHECK(hipMemcpyAsync(p, own_pos.back().data(), sizeof(int64_t) * (size_t)a.n,
                                   hipMemcpyHostToDevice, c->stream));
          a.pos = p;
        }
        HIP_CHECK(hipMemcpyAsync(a.st, hs.data(), sbytes + vbytes, hipMemcpyHostToDevice,
                                 c->stream));
        HIP_CHECK(launch_lr_validate(c->stream, a.y, a.n, validity_word(a.st, d)));
        for (hipEvent_t& e : a.sent) e = root ? nullptr : events.make(c);
      }
      const Active& root = act[0];
      const size_t k_act = act.size();
      hipEvent_t back[kEventRing] = {nullptr, nullptr};
      if (k_act > 1) {
        for (hipEvent_t& e : back) e = events.make(root.ctx);
        // every buffer exists before another context's stream writes to it
        for (const Active& a : act) {
          a.ctx->activate();
          a.ctx->drain();
        }
      }
      int device = -1;
      auto on = [&](const Active& a) {
        if (a.ctx->device != device) a.ctx->activate();
        device = a.ctx->device;
        return a.ctx->stream;
      };
      // iteration `it` (0-based) on this chunk's mask j, `count` rows in its sample
      auto iteration = [&](int it, int j, int64_t count) {
        const int ring = it % kEventRing;
        if (count > 0) {
          for (size_t s = k_act; s-- > 0;) {  // the root last: the others are at work by then
            const Active& a = act[s];
            const hipStream_t st = on(a);
            const uint32_t* mask = sampled ? a.mask + (size_t)j * words : nullptr;
            HIP_CHECK(launch_lr_gradient(st, grad, a.X, a.y, a.n, d, mask, a.pos, a.st, a.part,
                                         a.G));
            if (k_act == 1) break;  // a lone shard: the update reads a.part as it is
            HIP_CHECK(launch_lr_fold(st, a.part, a.G, d, a.st, s == 0 ? root.fold : a.fold));
            if (s == 0) continue;
            copy_between(root.fold + s * (size_t)d, root.ctx, a.fold, a.ctx,
                         sizeof(double) * (size_t)d, st);
            HIP_CHECK(hipEventRecord(a.sent[ring], st));
          }
          const hipStream_t st = on(root);
          for (size_t s = 1; s < k_act; ++s) HIP_CHECK(hipStreamWaitEvent(st, act[s].sent[ring], 0));
          const bool lone = k_act == 1;  // its own partials: the same sum without the fold
          HIP_CHECK(launch_lr_update(st, lone ? root.part : root.fold, lone ? root.G : (int)k_act,
                                     count, d, root.st, step_size, reg_param, convergence_tol,
                                     num_iterations));
        } else {  // an empty sample: the iteration counts, nothing else moves
          HIP_CHECK(launch_lr_skip(on(root), root.st, num_iterations));
        }
        if (k_act == 1) return;
        const hipStream_t st = on(root);
        for (size_t s = 1; s < k_act; ++s)
          copy_between(act[s].st, act[s].ctx, root.st, root.ctx, sbytes, st);
        HIP_CHECK(hipEventRecord(back[ring], st));
        for (size_t s = 1; s < k_act; ++s) HIP_CHECK(hipStreamWaitEvent(on(act[s]), back[ring], 0));
      };
      auto drain_all = [&] {
        for (const Active& a : act) {
          on(a);
          a.ctx->drain();
        }
      };
      if (!sampled) {
        for (int i = 0; i < num_iterations; ++i) iteration(i, 0, n_total);
      } else {
        std::vector<uint32_t> masks((size_t)(chunk * words));
        std::vector<int64_t> counts((size_t)chunk);
        for (int i0 = 0; i0 < num_iterations; i0 += chunk) {
          const int k = std::min(chunk, num_iterations - i0);
          drain_all();  // the previous chunk's uploads and iterations are done with the buffers
          if (i0 > 0) {  // converged (or stopped): the remaining iterations would be skipped
            int32_t conv = 0;
            HIP_CHECK(hipMemcpyAsync(&conv, &root.st->converged, sizeof(conv),
                                     hipMemcpyDeviceToHost, on(root)));
            HIP_CHECK(hipStreamSynchronize(root.ctx->stream));
            if (conv != 0) break;
          }
          draw_sgd_masks(n_total, mini_batch_fraction, num_partitions, i0, k, masks.data(),
                         counts.data());
          for (const Active& a : act)
            HIP_CHECK(hipMemcpyAsync(a.mask, masks.data(), sizeof(uint32_t) * (size_t)(k * words),
                                     hipMemcpyHostToDevice, on(a)));
          for (int j = 0; j < k; ++j) iteration(i0 + j, j, counts[(size_t)j]);
        }
        drain_all();  // the masks leave scope
      }
      finals.assign(k_act, std::vector<uint8_t>(sbytes + vbytes));
      for (size_t s = 0; s < k_act; ++s)
        HIP_CHECK(hipMemcpyAsync(finals[s].data(), act[s].st, sbytes + vbytes,
                                 hipMemcpyDeviceToHost, on(act[s])));
      drain_all();
    });
    for (const std::vector<uint8_t>& f : finals)
      if (validity_word((LrState*)f.data(), d)->converged == 2)
        fail(EEGFX_EINVAL, "%s", kBadLabels);
    for (const std::vector<uint8_t>& f : finals)  // the last broadcast reached every shard
      if (memcmp(f.data(), finals[0].data(), sbytes) != 0)
        fail(EEGFX_EHIP, "a shard's final state differs from the root's");
    const LrState* r = (const LrState*)finals[0].data();
    memcpy(weights, r->w, sizeof(double) * (size_t)d);
    if (iterations_run) *iterations_run = r->iter;
  });
}

}  // namespace eegfx

extern "C" {

int eegfx_glm_sgd_train_sharded(int grad, const eegfx_glm_shard* shards, int32_t n_shards,
                                int32_t d, int32_t num_iterations, double step_size,
                                double reg_param, double mini_batch_fraction,
                                double convergence_tol, int32_t num_partitions, double* weights,
                                int32_t* iterations_run) {
  const int refused = guarded([&] {
    if (!weights) fail(EEGFX_EINVAL, "null argument");
    check_shards(shards, n_shards);
  });
  if (refused != EEGFX_OK) return refused;
  return glm_sgd_train_shards(grad, shards, n_shards, d, num_iterations, step_size, reg_param,
                              mini_batch_fraction, convergence_tol, num_partitions, weights,
                              iterations_run, EEGFX_MEM_DEVICE);
}

int eegfx_glm_shard_state(eegfx_ctx* ctx, int32_t d, int32_t head[4], double* weights) {
  return guarded([&] {
    if (!ctx || !head || !weights) fail(EEGFX_EINVAL, "null argument");
    check_train_d(d);
    if (ctx->lr_state.cap < state_bytes(d)) fail(EEGFX_EINVAL, "the context holds no such state");
    std::vector<uint8_t> hs(state_bytes(d));
    ctx->activate();
    HIP_CHECK(hipMemcpyAsync(hs.data(), ctx->lr_state.p, hs.size(), hipMemcpyDeviceToHost,
                             ctx->stream));
    ctx->drain();
    const LrState* h = (const LrState*)hs.data();
    const int32_t v[4] = {h->iter, h->converged, h->updates, h->pad};
    memcpy(head, v, sizeof(v));
    memcpy(weights, h->w, sizeof(double) * (size_t)d);
  });
}

int eegfx_glm_count_sharded(int grad, const eegfx_glm_shard* shards, int32_t n_shards, int32_t d,
                            const double* weights, double intercept, double threshold,
                            int64_t counts[4]) {
  return guarded([&] {
    if (!weights || !counts) fail(EEGFX_EINVAL, "null argument");
    check_shards(shards, n_shards);
    check_predict_dims(0, d);
    if (grad != kGradLogistic && grad != kGradHinge) fail(EEGFX_EINVAL, "grad=%d", grad);
    std::vector<Active> act;
    for (int32_t s = 0; s < n_shards; ++s)
      if (shards[s].n > 0)
        act.push_back(Active{shards[s].ctx, shards[s].X, shards[s].y, nullptr, shards[s].n});
    std::vector<ConfusionOut> part(act.size());
    const bool use_t = !std::isnan(threshold);  // clearThreshold -> scores / margins
    drained_on_failure(act, [&] {
      for (size_t s = 0; s < act.size(); ++s) {
        eegfx_ctx* c = act[s].ctx;
        c->activate();
        LrState* st = (LrState*)c->lr_state.get(state_bytes(d));
        ConfusionOut* out = (ConfusionOut*)c->lr_part.get(sizeof(ConfusionOut));
        HIP_CHECK(hipMemcpyAsync(st->w, weights, sizeof(double) * (size_t)d,
                                 hipMemcpyHostToDevice, c->stream));
        HIP_CHECK(hipMemsetAsync(out, 0, sizeof(*out), c->stream));
        HIP_CHECK(launch_lr_count(c->stream, grad, act[s].X, act[s].y, act[s].n, d, st->w,
                                  intercept, threshold, use_t ? 1 : 0, out));
        HIP_CHECK(hipMemcpyAsync(&part[s], out, sizeof(*out), hipMemcpyDeviceToHost, c->stream));
      }
      for (const Active& a : act) {
        a.ctx->activate();
        a.ctx->drain();
      }
    });
    ConfusionOut sum;
    memset(&sum, 0, sizeof(sum));
    for (const ConfusionOut& p : part) {
      for (int k = 0; k < 4; ++k) sum.cell[k] += p.cell[k];
      sum.seen |= p.seen;
    }
    confusion_verdict(sum, counts);
  });
}

}  // extern "C"
