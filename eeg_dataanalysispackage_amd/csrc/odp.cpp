// odp.cpp -- the OffLineDataProvider of the eegfx C ABI (eegfx_odp_*, eegfx_shard_span).
//
// Mirrors DataTransformation/OffLineDataProvider.java (constructor :78, loadData :88-98,
// handleInput :111-141, processEEGFiles :147-268, loadFilesFromInfoTxt :283-319, setFileNames
// :327-365, getData :370, getDataLabels :377) with local files in place of HDFS.  Epochs are cut
// and baseline-corrected on the GPU and stay resident in HBM; getData() copies them back on demand.
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <memory>
#include <string>
#include <thread>
#include <utility>
#include <vector>

#include "ctx.h"
#include "split_plan.h"

using namespace eegfx;

// ================================================================================================
// OffLineDataProvider
// ================================================================================================
struct eegfx_odp {
  std::vector<std::string> args;
  std::string error;
  // Map<String, Integer> files = new LinkedHashMap<>() (:54): insertion order, put() on an
  // existing key keeps the position and replaces the value.
  std::vector<std::pair<std::string, int32_t>> files;
  std::string file_prefix;
  std::string vhdr_file, vmrk_file, eeg_file;
  int32_t fz_index = 0, cz_index = 0, pz_index = 0;  // fields: persist across files (:49-51)
  int64_t balance = 0;                                // numberOfTargets - numberOfNonTargets
  int64_t epochs_counter = 0;
  std::vector<double> labels;
  std::vector<int64_t> positions;
  std::vector<int32_t> file_of_epoch;
  int64_t n_epochs = 0;

  // loadData plans on the host, in file order (process_eeg_files: selection, labels, and per file
  // what a shard needs to cut from it); the epochs then live in `shards`, one per context.
  // eegfx_odp_create's provider is one shard on its context and keeps the reference's sequential
  // semantics: a repeated loadData appends to what the provider holds (the reference's fields
  // persist, :53-60), and every listed payload is opened where the reference reads it.
  bool sequential = false;
  std::vector<eegfx_ctx*> ctxs;  // empty: planning-only
  int32_t n_shards = 1;
  struct FilePlan {
    int32_t file_idx;
    std::string eeg;
    Header h;
    int64_t n_frames;
    int32_t idx[3];  // Fz, Cz, Pz as they stood at this file
  };
  std::vector<FilePlan> plans;
  struct Shard {
    int64_t first = 0, count = 0;
    void* d_epochs = nullptr;    // double[count][3][750] on the shard's context, exact size
    // dwt-8 rows of the epochs, double[count][48], computed in the same pass as the epochs under
    // the numerics of the load; getFeatures() with the reference's parameters (8, 512, 175, 16)
    // under the same numerics is then a copy
    void* d_features = nullptr;
    int numerics = -1;  // numerics of d_features' rows; -1: loads under different numerics
  };
  std::vector<Shard> shards;
  // eegfx_odp_split_sharded's buffers, one allocation per shard on its context: X [count][d] and
  // y [count] (the training rows, then the test rows), then their positions int64 [count]
  std::vector<void*> split_bufs;

  void put_file(const std::string& k, int32_t v) {
    for (auto& kv : files)
      if (kv.first == k) {
        kv.second = v;
        return;
      }
    files.emplace_back(k, v);
  }

  static bool ends_with_4(const std::string& s, const char* suf) {
    // fileLocation.substring(fileLocation.length() - 4): StringIndexOutOfBounds below 4 chars.
    if (s.size() < 4) fail(EEGFX_EINVAL, "String index out of range: %d", (int)s.size() - 4);
    return s.compare(s.size() - 4, 4, suf) == 0;
  }

  void handle_input() {  // :111-141
    if (args.empty() || args.size() > 6)
      fail(EEGFX_EINVAL,
           "Please enter the input in one of these formats: 1. <location of info.txt file> "
           "2. <location of a .eeg file> <guessed number>  *<optional values>");
    const std::string& loc = args[0];
    if (ends_with_4(loc, ".eeg")) {
      file_prefix = "";
      if (args.size() < 2) fail(EEGFX_EINVAL, "Index 1 out of bounds for length 1");
      int32_t g;
      if (!java_parse_int(args[1], &g))
        fail(EEGFX_EFORMAT, "For input string: \"%s\"", args[1].c_str());
      put_file(loc, g);
    } else if (ends_with_4(loc, ".txt")) {
      const size_t slash = loc.rfind('/');
      if (slash == std::string::npos) fail(EEGFX_EINVAL, "String index out of range: -1");
      file_prefix = loc.substr(0, slash) + "/";
      load_files_from_info_txt(loc);
    } else {
      fail(EEGFX_EINVAL,
           "Please enter the input in one of these formats: 1. <location of info.txt file> "
           "2. <location of a .eeg file> <target number>  *<optional values>");
    }
  }

  void load_files_from_info_txt(const std::string& loc) {  // :283-319
    FILE* f = fopen(loc.c_str(), "rb");
    if (!f) fail(EEGFX_EIO, "File %s does not exist", loc.c_str());
    std::string text;
    char buf[4096];
    size_t r;
    while ((r = fread(buf, 1, sizeof(buf), f)) > 0) text.append(buf, r);
    fclose(f);
    std::vector<std::string> lines;
    std::string cur;
    for (size_t i = 0; i < text.size(); ++i) {  // BufferedReader.readLine
      const char ch = text[i];
      if (ch == '\n' || ch == '\r') {
        lines.push_back(cur);
        cur.clear();
        if (ch == '\r' && i + 1 < text.size() && text[i + 1] == '\n') ++i;
      } else {
        cur.push_back(ch);
      }
    }
    if (!cur.empty()) lines.push_back(cur);
    for (const std::string& line : lines) {
      if (line.empty() || line[0] == '#') continue;
      std::vector<std::string> parts = java_split_space(line);
      if (parts.size() > 1) {
        int32_t num;
        if (!java_parse_int(parts[1], &num))
          fail(EEGFX_EFORMAT, "Line %s contains an improper number format", line.c_str());
        put_file(parts[0], num);
      }
    }
  }

  // setFileNames (:327-365): false = the reference's caught IllegalArgumentException (skip file).
  bool set_file_names(const std::string& loc, std::string* why) {
    if (loc.size() <= 4) {
      *why = "Incorrect file name, must be at least longer than 4 characters ";
      return false;
    }
    if (loc.compare(loc.size() - 4, 4, ".eeg") != 0) {
      *why = "Invalid .eeg file";
      return false;
    }
    const std::string base = loc.substr(0, loc.rfind('.'));
    const std::string vhdr = base + ".vhdr", vmrk = base + ".vmrk";
    if (!file_exists(vhdr)) {
      *why = "No related .vhdr file found for the original .eeg file " + vhdr;
      return false;
    }
    if (!file_exists(vmrk)) {
      *why = "No related .vmrk file found for the original .eeg file " + vmrk;
      return false;
    }
    if (!file_exists(loc)) {
      *why = "No related .eeg file found for the original .eeg file " + loc;
      return false;
    }
    vhdr_file = vhdr;
    vmrk_file = vmrk;
    eeg_file = loc;
    return true;
  }

  // columns and resolutions of Fz, Cz, Pz (1-based channel numbers) in a recording
  static ChanSel file_sel(const Header& h, const int32_t idx[3]) {
    int32_t cols[3];
    float res[3];
    for (int c = 0; c < 3; ++c) {
      cols[c] = idx[c] - 1;
      res[c] = 1.0f;
      for (const auto& ci : h.channels)
        if (ci.number == idx[c]) res[c] = (float)ci.resolution;
    }
    return make_sel(cols, res, 3, h.info.n_channels);
  }

  void process_eeg_files() {  // :147-268
    int32_t file_idx = -1;
    for (const auto& entry : files) {
      ++file_idx;
      std::string why;
      if (!set_file_names(file_prefix + entry.first, &why)) continue;  // logged + skipped (:157-161)
      const Header h = read_header(vhdr_file);
      for (const auto& ch : h.channels) {  // :172-183
        std::string name = ch.name;
        for (auto& c : name) c = (char)tolower((unsigned char)c);
        if (name == "fz") fz_index = ch.number;
        else if (name == "cz") cz_index = ch.number;
        if (name == "pz") pz_index = ch.number;
      }
      const int32_t sel[3] = {fz_index, cz_index, pz_index};
      for (int c = 0; c < 3; ++c)
        if (sel[c] < 1 || sel[c] > h.info.n_channels)
          fail(EEGFX_EINVAL, "%s: channel %s not found (index %d)", vhdr_file.c_str(),
               c == 0 ? "Fz" : c == 1 ? "Cz" : "Pz", sel[c]);
      const int64_t n_frames = recording_frames(h, eeg_file);
      // the reference reads the payload here (:185-188): a payload that cannot be opened stops
      // the load at this file, ahead of its markers, whether or not it selects an epoch
      // (planning-only providers never touch the recording payload)
      if (sequential && !ctxs.empty()) read_file_bytes(eeg_file, nullptr, 0);
      plans.push_back(FilePlan{file_idx, eeg_file, h, n_frames, {sel[0], sel[1], sel[2]}});

      const std::vector<eegfx_marker> markers = read_markers(vmrk_file);
      std::vector<int64_t> pos(markers.size());
      std::vector<double> lab(markers.size());
      int64_t k = 0;
      const int rc = eegfx_plan_markers(markers.data(), (int64_t)markers.size(), n_frames,
                                        entry.second, &balance, pos.data(), lab.data(), &k);
      pos.resize((size_t)k);
      lab.resize((size_t)k);
      epochs_counter += k;
      n_epochs += k;  // epochs accepted before an error stay
      positions.insert(positions.end(), pos.begin(), pos.end());
      labels.insert(labels.end(), lab.begin(), lab.end());
      file_of_epoch.insert(file_of_epoch.end(), (size_t)k, file_idx);
      if (rc != EEGFX_OK) fail(rc, "%s", last_error().c_str());
    }
  }

  // ---- the device pass: one worker per context -------------------------------------------------
  void release_split() {
    for (size_t r = 0; r < split_bufs.size() && r < ctxs.size(); ++r) {
      if (!split_bufs[r]) continue;
      (void)hipSetDevice(ctxs[r]->device);
      (void)hipFreeAsync(split_bufs[r], ctxs[r]->stream);
      (void)hipStreamSynchronize(ctxs[r]->stream);
    }
    split_bufs.clear();
  }

  void release_shards() {
    release_split();
    for (size_t r = 0; r < shards.size() && r < ctxs.size(); ++r) {
      Shard& s = shards[r];
      if (!s.d_epochs && !s.d_features) continue;
      (void)hipSetDevice(ctxs[r]->device);
      if (s.d_epochs) (void)hipFreeAsync(s.d_epochs, ctxs[r]->stream);
      if (s.d_features) (void)hipFreeAsync(s.d_features, ctxs[r]->stream);
      (void)hipStreamSynchronize(ctxs[r]->stream);
      s.d_epochs = s.d_features = nullptr;
    }
  }

  // Shard r: eegfx_shard_range(planned, r, n_shards) clipped to the first `kept` epochs.
  void set_ranges(int64_t planned, int64_t kept) {
    for (int32_t r = 0; r < n_shards; ++r) {
      int64_t a = 0, b = 0;
      if (eegfx_shard_range(planned, r, n_shards, &a, &b) != EEGFX_OK)
        fail(EEGFX_EINVAL, "%s", last_error().c_str());
      shards[(size_t)r].first = std::min(a, kept);
      shards[(size_t)r].count = std::min(b, kept) - std::min(a, kept);
    }
  }

  struct WorkerError {
    int code = EEGFX_OK;
    int32_t file = -1;  // index (in `files`) of the file the worker was on
    std::string text;
  };

  // The worker of context r: the files its range intersects, in order; of each, the frames
  // eegfx_shard_span names, through two pinned staging buffers (the read of one file overlaps the
  // upload and the kernels of the one before), into the epochs' slots of the shard's buffers.
  // The epochs before `base` are those of earlier loads (a sequential provider's): their rows are
  // copied into the buffers of the new size and only the epochs from `base` on are computed.
  void run_shard(size_t r, int64_t base, const std::vector<int32_t>& plan_of_file,
                 WorkerError* we) {
    eegfx_ctx* c = ctxs[r];
    Shard& s = shards[r];
    const int64_t begin = std::max(s.first, base), held = begin - s.first;
    int32_t cur_file = file_of_epoch[(size_t)begin];
    bool used[2] = {false, false};
    try {
      c->activate();
      const size_t per = sizeof(double) * 3 * EEGFX_POSTSTIMULUS;
      const size_t fper = sizeof(double) * 3 * EEGFX_DWT8_FEATURE_SIZE;
      // each buffer once per load at its exact size; rows held from earlier loads move over on
      // the context stream (the feature rows only while they are of one numerics)
      auto resize = [&](void*& buf, size_t row, bool keep) {
        void* p = nullptr;
        HIP_CHECK(hipMallocAsync(&p, row * (size_t)s.count, c->stream));
        const hipError_t e = held && keep ? hipMemcpyAsync(p, buf, row * (size_t)held,
                                                            hipMemcpyDeviceToDevice, c->stream)
                                          : hipSuccess;
        if (buf) (void)hipFreeAsync(buf, c->stream);
        buf = p;
        HIP_CHECK(e);
      };
      resize(s.d_epochs, per, true);
      resize(s.d_features, fper, s.numerics >= 0);
      s.numerics = held == 0 || s.numerics == c->numerics ? c->numerics : -1;
      for (hipEvent_t& x : c->staged)
        if (!x) HIP_CHECK(hipEventCreateWithFlags(&x, hipEventDisableTiming));
      const int64_t end = s.first + s.count;
      int b = 0;
      for (int64_t i = begin; i < end; b ^= 1) {
        const int32_t f = file_of_epoch[(size_t)i];
        cur_file = f;
        int64_t j = i;
        while (j < end && file_of_epoch[(size_t)j] == f) ++j;
        const int64_t k = j - i;
        const FilePlan& fp = plans[(size_t)plan_of_file[(size_t)f]];
        int64_t first = 0, frames = 0;
        if (eegfx_shard_span(&positions[(size_t)i], k, fp.n_frames, &first, &frames) != EEGFX_OK)
          fail(EEGFX_EINVAL, "%s", last_error().c_str());
        // pos - 100 == n_frames for every epoch of the span: one frame earlier, so that no kernel
        // is launched on an empty recording (a recording of no frames at all stays empty, as it
        // is for the one-context provider)
        if (frames == 0 && first > 0) {
          --first;
          frames = 1;
        }
        const int ct = fp.h.info.n_channels;
        const size_t raw_bytes = (size_t)frames * ct * sample_bytes(fp.h.info.binary_format);
        const size_t pos_off = (raw_bytes + 7) & ~(size_t)7;
        if (used[b]) HIP_CHECK(hipEventSynchronize(c->staged[b]));  // its last upload has left it
        char* host = (char*)c->pin_chunk[b].get(pos_off + sizeof(int64_t) * (size_t)k);
        read_recording_span(fp.h, fp.eeg, host, fp.n_frames, first, frames);
        int64_t* h_pos = (int64_t*)(host + pos_off);
        for (int64_t t = 0; t < k; ++t) h_pos[t] = positions[(size_t)(i + t)] - first;
        void* d_raw = c->raw.get(raw_bytes);
        if (raw_bytes)
          HIP_CHECK(hipMemcpyAsync(d_raw, host, raw_bytes, hipMemcpyHostToDevice, c->stream));
        int64_t* d_pos = (int64_t*)c->pos.get(sizeof(int64_t) * (size_t)k);
        HIP_CHECK(hipMemcpyAsync(d_pos, h_pos, sizeof(int64_t) * (size_t)k, hipMemcpyHostToDevice,
                                 c->stream));
        if (j < end) {  // a later span may take this buffer
          HIP_CHECK(hipEventRecord(c->staged[b], c->stream));
          used[b] = true;
        }
        run_epochs_and_features(c, d_raw, fp.h.info.binary_format, frames, ct,
                                file_sel(fp.h, fp.idx), 3, d_pos, k,
                                (double*)((char*)s.d_epochs + per * (size_t)(i - s.first)),
                                (double*)((char*)s.d_features + fper * (size_t)(i - s.first)));
        i = j;
      }
      c->drain();
    } catch (const Error& e) {
      *we = WorkerError{e.code, cur_file, e.what()};
    } catch (const std::bad_alloc&) {
      *we = WorkerError{EEGFX_ENOMEM, cur_file, "out of host memory"};
    } catch (const std::exception& e) {
      *we = WorkerError{EEGFX_EINVAL, cur_file, e.what()};
    }
    // after a failure copies may still read the staging buffers: nothing is left in flight
    if (we->code != EEGFX_OK) (void)hipStreamSynchronize(c->stream);
  }

  // Runs the workers and joins them; the failure in the earliest file, if any.  A single shard
  // with epochs to compute runs on the calling thread.
  WorkerError compute(int64_t base) {
    std::vector<int32_t> plan_of_file(files.size(), -1);
    for (size_t p = 0; p < plans.size(); ++p) plan_of_file[(size_t)plans[p].file_idx] = (int32_t)p;
    std::vector<WorkerError> errs(shards.size());
    std::vector<size_t> busy;
    for (size_t r = 0; r < shards.size(); ++r)
      if (shards[r].first + shards[r].count > base) busy.push_back(r);
    if (busy.size() == 1) {
      run_shard(busy[0], base, plan_of_file, &errs[busy[0]]);
    } else {
      Joiner workers;
      for (size_t r : busy)
        workers.th.emplace_back([this, r, base, &plan_of_file, &errs] {
          run_shard(r, base, plan_of_file, &errs[r]);
        });
    }
    WorkerError worst;
    for (const WorkerError& e : errs)
      if (e.code != EEGFX_OK && (worst.code == EEGFX_OK || e.file < worst.file)) worst = e;
    return worst;
  }

  // What an earlier load left is released: loadData starts over.
  void reset() {
    release_shards();
    shards.assign((size_t)n_shards, Shard());
    files.clear();
    labels.clear();
    positions.clear();
    file_of_epoch.clear();
    file_prefix.clear();
    n_epochs = epochs_counter = balance = 0;
    fz_index = cz_index = pz_index = 0;
  }

  // loadData (:88-98): every exception is logged as fatal and swallowed; what was loaded stays.
  int load() {
    int64_t base = 0;  // the epochs held from earlier loads
    release_split();
    int rc = guarded([&] {
      if (!sequential) reset();
      base = n_epochs;
      plans.clear();
      for (size_t r = 1; r < ctxs.size(); ++r)
        if (ctxs[r]->numerics != ctxs[0]->numerics)
          fail(EEGFX_EINVAL,
               "the contexts of a provider must hold the same numerics at loadData (context %d "
               "holds %d, context 0 holds %d)", (int)r, ctxs[r]->numerics, ctxs[0]->numerics);
      handle_input();
      process_eeg_files();
    });
    std::string text = rc == EEGFX_OK ? "" : last_error();
    const int64_t planned = n_epochs;
    const int rc2 = guarded([&] {
      set_ranges(planned, planned);
      if (ctxs.empty() || planned == base) return;
      WorkerError w;
      try {
        w = compute(base);
      } catch (const std::exception& e) {  // no worker ran to its end: nothing of this load is kept
        w = WorkerError{EEGFX_EINVAL, 0, e.what()};
      }
      if (w.code == EEGFX_OK) return;
      // the load stops in that file: the files before it stay (file indices ascend within a load)
      const int64_t kept =
          std::lower_bound(file_of_epoch.begin() + base, file_of_epoch.end(), w.file) -
          file_of_epoch.begin();
      positions.resize((size_t)kept);
      labels.resize((size_t)kept);
      file_of_epoch.resize((size_t)kept);
      n_epochs = kept;
      set_ranges(planned, kept);
      fail(w.code, "%s", w.text.c_str());
    });
    if (rc2 != EEGFX_OK) {
      rc = rc2;
      text = last_error();
    }
    error = text;
    set_last_error(text);
    return rc;
  }

  // An accessor's work on every shard that holds epochs: `enqueue(ctx, shard)` on each context's
  // stream first, then every context is drained, so the devices work at the same time.  Whatever
  // was enqueued is drained even when a later step fails (it writes into the caller's buffer).
  template <typename F>
  void on_shards(F&& enqueue) const {
    if (ctxs.empty()) fail(EEGFX_EINVAL, "planning-only provider (no device context) holds no epochs");
    size_t started = 0;
    std::unique_ptr<Error> first;
    try {
      for (; started < shards.size(); ++started) {
        if (shards[started].count == 0) continue;
        ctxs[started]->activate();
        enqueue(ctxs[started], shards[started]);
      }
    } catch (const Error& e) {
      first.reset(new Error(e));
      started = std::min(started + 1, shards.size());
    }
    for (size_t r = 0; r < started; ++r) {
      if (shards[r].count == 0) continue;
      try {
        ctxs[r]->activate();
        ctxs[r]->drain();
      } catch (const Error& e) {
        if (!first) first.reset(new Error(e));
      }
    }
    if (first) throw *first;
  }

  // getFeatures on every shard: the rows computed with the epochs at loadData when they are the
  // ones asked for (the one-pass kernels), else the batch extract over the resident epochs;
  // `land(ctx, shard, rows, bytes)` enqueues their copy to where the caller wants them.
  template <typename F>
  void feature_rows(int32_t skip, int32_t feature_size, F&& land) const {
    const size_t row = sizeof(double) * 3 * (size_t)feature_size;
    on_shards([&](eegfx_ctx* ctx, const Shard& s) {
      const size_t bytes = row * (size_t)s.count;
      if (skip == EEGFX_DWT8_SKIP && feature_size == EEGFX_DWT8_FEATURE_SIZE &&
          s.numerics == ctx->numerics && s.d_features) {
        land(ctx, s, (const double*)s.d_features, bytes);
        return;
      }
      double* d_out = (double*)ctx->out.get(bytes);
      run_features_from_epochs(ctx, (const double*)s.d_epochs, s.count, 3, skip, feature_size,
                               d_out, EEGFX_POSTSTIMULUS);
      land(ctx, s, d_out, bytes);
    });
  }
};

extern "C" {

// ---- OffLineDataProvider ----------------------------------------------------------------------
int eegfx_odp_create(eegfx_ctx* ctx, const char* const* args, int32_t n_args, eegfx_odp** out) {
  return guarded([&] {
    if (!out || (n_args > 0 && !args) || n_args < 0) fail(EEGFX_EINVAL, "null argument");
    std::unique_ptr<eegfx_odp> o(new eegfx_odp());
    o->sequential = true;
    if (ctx) o->ctxs.push_back(ctx);
    o->shards.assign(1, eegfx_odp::Shard());
    for (int i = 0; i < n_args; ++i) o->args.emplace_back(args[i] ? args[i] : "");
    *out = o.release();
  });
}

int eegfx_odp_load_data(eegfx_odp* odp) {
  if (!odp) {
    set_last_error("null provider");
    return EEGFX_EINVAL;
  }
  return odp->load();
}

const char* eegfx_odp_error(const eegfx_odp* odp) { return odp ? odp->error.c_str() : "null provider"; }

int64_t eegfx_odp_num_epochs(const eegfx_odp* odp) { return odp ? odp->n_epochs : 0; }

int eegfx_odp_get_data(const eegfx_odp* odp, double* out) {
  return guarded([&] {
    if (!odp || !out) fail(EEGFX_EINVAL, "null argument");
    if (!odp->n_epochs) return;
    const size_t per = sizeof(double) * 3 * EEGFX_POSTSTIMULUS;
    odp->on_shards([&](eegfx_ctx* ctx, const eegfx_odp::Shard& s) {
      HIP_CHECK(hipMemcpyAsync((char*)out + per * (size_t)s.first, s.d_epochs,
                               per * (size_t)s.count, hipMemcpyDeviceToHost, ctx->stream));
    });
  });
}

int eegfx_odp_get_data_f32(const eegfx_odp* odp, float* out) {
  return guarded([&] {
    if (!odp || !out) fail(EEGFX_EINVAL, "null argument");
    if (!odp->n_epochs) return;
    // the resident epochs stay double; a narrowing kernel feeds the copy (exact: every value is a
    // widened fp32), so half the bytes cross the host link
    odp->on_shards([&](eegfx_ctx* ctx, const eegfx_odp::Shard& s) {
      const int64_t count = 3 * EEGFX_POSTSTIMULUS * s.count;
      float* d_f32 = (float*)ctx->scratch.get(sizeof(float) * (size_t)count);
      HIP_CHECK(launch_narrow_epochs(ctx->stream, (const double*)s.d_epochs, d_f32, count));
      HIP_CHECK(hipMemcpyAsync(out + 3 * EEGFX_POSTSTIMULUS * s.first, d_f32,
                               sizeof(float) * (size_t)count, hipMemcpyDeviceToHost,
                               ctx->stream));
    });
  });
}

int eegfx_odp_get_labels(const eegfx_odp* odp, double* out) {
  return guarded([&] {
    if (!odp || !out) fail(EEGFX_EINVAL, "null argument");
    std::copy(odp->labels.begin(), odp->labels.end(), out);
  });
}

int eegfx_odp_get_positions(const eegfx_odp* odp, int64_t* pos_out, int32_t* file_out) {
  return guarded([&] {
    if (!odp) fail(EEGFX_EINVAL, "null argument");
    if (pos_out) std::copy(odp->positions.begin(), odp->positions.end(), pos_out);
    if (file_out) std::copy(odp->file_of_epoch.begin(), odp->file_of_epoch.end(), file_out);
  });
}

int eegfx_odp_get_features(eegfx_odp* odp, int32_t name, int32_t epoch_size, int32_t skip,
                           int32_t feature_size, double* out) {
  return guarded([&] {
    if (!odp || !out) fail(EEGFX_EINVAL, "null argument");
    check_fe_params(3, name, epoch_size, skip, feature_size);
    if (!odp->n_epochs) return;
    const size_t row = sizeof(double) * 3 * (size_t)feature_size;
    odp->feature_rows(skip, feature_size, [&](eegfx_ctx* ctx, const eegfx_odp::Shard& s,
                                              const double* rows, size_t bytes) {
      HIP_CHECK(hipMemcpyAsync((char*)out + row * (size_t)s.first, rows, bytes,
                               hipMemcpyDeviceToHost, ctx->stream));
    });
  });
}

int eegfx_odp_split(eegfx_odp* odp, eegfx_ctx* ctx, int64_t seed, double train_fraction,
                    int32_t name, int32_t epoch_size, int32_t skip, int32_t feature_size,
                    double* X, double* y, int64_t* n_train, int mem) {
  return guarded([&] {
    if (!odp || !n_train) fail(EEGFX_EINVAL, "null argument");
    check_mem(mem);
    if (!(train_fraction >= 0.0 && train_fraction <= 1.0))
      fail(EEGFX_EINVAL, "train_fraction %g outside [0, 1]", train_fraction);
    check_fe_params(3, name, epoch_size, skip, feature_size);
    if (odp->ctxs.empty())
      fail(EEGFX_EINVAL, "planning-only provider (no device context) holds no epochs");
    if (!ctx) ctx = odp->ctxs[0];
    const int64_t n = odp->n_epochs;
    *n_train = (int64_t)((double)n * train_fraction);  // (int)(data.size()*0.7)
    if (n == 0) return;
    if (!X || !y) fail(EEGFX_EINVAL, "null X / y");
    const std::vector<int64_t> perm = java_shuffle(n, seed);
    const int d = 3 * feature_size;
    const size_t row = sizeof(double) * (size_t)d;
    // every row in list order in one buffer on ctx; the allocations are complete before another
    // context's stream writes there
    ctx->activate();
    char* rows = (char*)ctx->fl_src.get(row * (size_t)n);
    int64_t* d_perm = (int64_t*)ctx->fl_idx.get(sizeof(int64_t) * (size_t)n);
    double* d_lab = (double*)ctx->fl_lab.get(sizeof(double) * (size_t)n);
    double* d_X = dev_out(ctx->fl_dst, X, row * (size_t)n, mem);
    double* d_y = dev_out(ctx->fl_y, y, sizeof(double) * (size_t)n, mem);
    ctx->drain();
    odp->feature_rows(skip, feature_size, [&](eegfx_ctx* c, const eegfx_odp::Shard& s,
                                              const double* from, size_t bytes) {
      copy_between(rows + row * (size_t)s.first, ctx, from, c, bytes, c->stream);
    });
    ctx->activate();
    HIP_CHECK(hipMemcpyAsync(d_lab, odp->labels.data(), sizeof(double) * (size_t)n,
                             hipMemcpyHostToDevice, ctx->stream));
    HIP_CHECK(hipMemcpyAsync(d_perm, perm.data(), sizeof(int64_t) * (size_t)n,
                             hipMemcpyHostToDevice, ctx->stream));
    run_gather_rows(ctx, (const double*)rows, n, d, d_perm, n, d_X, 0);
    run_gather_rows(ctx, d_lab, n, 1, d_perm, n, d_y, 1);
    copy_back(ctx, X, d_X, row * (size_t)n, mem);
    copy_back(ctx, y, d_y, sizeof(double) * (size_t)n, mem);
    gather_check(ctx, 2, n);  // drains for both memory kinds
  });
}

int eegfx_odp_split_sharded(eegfx_odp* odp, int64_t seed, double train_fraction, int32_t name,
                            int32_t epoch_size, int32_t skip, int32_t feature_size,
                            eegfx_split_shard* out) {
  return guarded([&] {
    if (!odp || !out) fail(EEGFX_EINVAL, "null argument");
    if (!(train_fraction >= 0.0 && train_fraction <= 1.0))
      fail(EEGFX_EINVAL, "train_fraction %g outside [0, 1]", train_fraction);
    check_fe_params(3, name, epoch_size, skip, feature_size);
    if (odp->ctxs.empty())
      fail(EEGFX_EINVAL, "planning-only provider (no device context) holds no epochs");
    odp->release_split();
    const size_t k = odp->shards.size();
    for (size_t r = 0; r < k; ++r) out[r] = eegfx_split_shard{(int32_t)r};
    const int64_t n = odp->n_epochs;
    if (n == 0) return;
    const std::vector<int64_t> perm = java_shuffle(n, seed);
    const int64_t cut = (int64_t)((double)n * train_fraction);  // (int)(data.size()*0.7)
    const int d = 3 * feature_size;
    std::vector<SplitShardPlan> plans(k);  // read by the uploads until the contexts are drained
    odp->split_bufs.assign(k, nullptr);
    odp->feature_rows(skip, feature_size, [&](eegfx_ctx* c, const eegfx_odp::Shard& s,
                                              const double* rows, size_t) {
      const size_t r = (size_t)(&s - odp->shards.data()), m = (size_t)s.count;
      SplitShardPlan& pl = plans[r];
      pl = split_shard_plan(perm.data(), n, cut, s.first, s.count);
      HIP_CHECK(hipMallocAsync(&odp->split_bufs[r], sizeof(double) * m * (size_t)(d + 2),
                               c->stream));
      double* X = (double*)odp->split_bufs[r];
      double* y = X + m * (size_t)d;
      int64_t* pos = (int64_t*)(y + m);
      int64_t* idx = (int64_t*)c->fl_idx.get(sizeof(int64_t) * m);
      double* lab = (double*)c->fl_lab.get(sizeof(double) * m);
      HIP_CHECK(hipMemcpyAsync(idx, pl.idx.data(), sizeof(int64_t) * m, hipMemcpyHostToDevice,
                               c->stream));
      HIP_CHECK(hipMemcpyAsync(pos, pl.pos.data(), sizeof(int64_t) * m, hipMemcpyHostToDevice,
                               c->stream));
      HIP_CHECK(hipMemcpyAsync(lab, &odp->labels[(size_t)s.first], sizeof(double) * m,
                               hipMemcpyHostToDevice, c->stream));
      run_gather_rows(c, rows, s.count, d, idx, s.count, X, 0);
      run_gather_rows(c, lab, s.count, 1, idx, s.count, y, 1);
      const int64_t a = pl.n_train, b = pl.n_test;
      out[r].n_train = a;
      out[r].n_test = b;
      out[r].X_train = a ? X : nullptr;
      out[r].y_train = a ? y : nullptr;
      out[r].pos_train = a ? pos : nullptr;
      out[r].X_test = b ? X + (size_t)a * d : nullptr;
      out[r].y_test = b ? y + a : nullptr;
      out[r].pos_test = b ? pos + a : nullptr;
    });
    for (size_t r = 0; r < k; ++r) {
      if (odp->shards[r].count == 0) continue;
      odp->ctxs[r]->activate();
      gather_check(odp->ctxs[r], 2, odp->shards[r].count);
    }
  });
}

int eegfx_odp_create_multi(eegfx_ctx* const* ctxs, int32_t n_ctx, const char* const* args,
                           int32_t n_args, eegfx_odp** out) {
  return guarded([&] {
    if (!out || (n_args > 0 && !args) || n_args < 0) fail(EEGFX_EINVAL, "null argument");
    if (n_ctx < 1 || n_ctx > EEGFX_ODP_MAX_SHARDS)
      fail(EEGFX_EINVAL, "%d contexts outside [1, %d]", n_ctx, EEGFX_ODP_MAX_SHARDS);
    std::unique_ptr<eegfx_odp> o(new eegfx_odp());
    o->n_shards = n_ctx;
    for (int i = 0; ctxs && i < n_ctx; ++i) {
      if (!ctxs[i]) fail(EEGFX_EINVAL, "context %d is null", i);
      for (int j = 0; j < i; ++j)
        if (ctxs[j] == ctxs[i])
          fail(EEGFX_EINVAL, "context %d repeats context %d: two shards would share its buffers", i,
               j);
      o->ctxs.push_back(ctxs[i]);
    }
    o->shards.assign((size_t)n_ctx, eegfx_odp::Shard());
    for (int i = 0; i < n_args; ++i) o->args.emplace_back(args[i] ? args[i] : "");
    *out = o.release();
  });
}

int eegfx_odp_num_shards(const eegfx_odp* odp) { return odp ? odp->n_shards : 0; }

int eegfx_odp_get_shard(const eegfx_odp* odp, int32_t i, eegfx_odp_shard* out) {
  return guarded([&] {
    if (!odp || !out) fail(EEGFX_EINVAL, "null argument");
    if (i < 0 || i >= odp->n_shards)
      fail(EEGFX_EINVAL, "shard %d outside [0, %d)", i, odp->n_shards);
    const eegfx_odp::Shard& s = odp->shards[(size_t)i];
    eegfx_odp_shard v = {i, -1, s.first, s.count, nullptr, nullptr, -1};
    if (!odp->ctxs.empty()) {
      v.device = odp->ctxs[(size_t)i]->device;
      if (s.count > 0) {
        v.epochs = (const double*)s.d_epochs;
        if (s.d_features && s.numerics >= 0) {
          v.features = (const double*)s.d_features;
          v.features_numerics = s.numerics;
        }
      }
    }
    *out = v;
  });
}

int eegfx_shard_span(const int64_t* pos, int64_t n, int64_t n_frames, int64_t* first_frame,
                     int64_t* frames) {
  return guarded([&] {
    if (n < 0 || n_frames < 0 || (n > 0 && !pos) || !first_frame || !frames)
      fail(EEGFX_EINVAL, "shard_span(n=%lld, n_frames=%lld)", (long long)n, (long long)n_frames);
    *first_frame = *frames = 0;
    if (n == 0) return;
    const auto mm = std::minmax_element(pos, pos + n);
    check_positions(mm.first, 1, n_frames);
    check_positions(mm.second, 1, n_frames);
    *first_frame = *mm.first - EEGFX_PRESTIMULUS;
    *frames = std::min(n_frames, *mm.second + EEGFX_POSTSTIMULUS) - *first_frame;
  });
}

void eegfx_odp_destroy(eegfx_odp* odp) {
  if (!odp) return;
  odp->release_shards();
  delete odp;
}

}  // extern "C"
