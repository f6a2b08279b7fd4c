/*
 * eegfx.h -- C ABI of the MI355X-native epoch-to-feature path.
 *
 * This is the drop-in boundary for the reference's hot path
 * (NEUROINFORMATICS-GROUP-FAV-KIV-ZCU/EEG_DataAnalysisPackage, paths relative to its checkout):
 *
 *   src/main/java/cz/zcu/kiv/DataTransformation/OffLineDataProvider.java   (processEEGFiles)
 *   src/main/java/cz/zcu/kiv/FeatureExtraction/IFeatureExtraction.java     (extractFeatures)
 *   src/main/java/cz/zcu/kiv/FeatureExtraction/WaveletTransform.java       (fe=dwt-8)
 *
 * Every entry point below names the reference interface it replaces.  The ABI is plain C:
 * no C++ or torch types, caller-owned buffers, int status returns (0 = ok, < 0 = error),
 * error text from eegfx_last_error() (thread-local).  Java binds it through JNI
 * (INTEGRATION.md); Python binds it through ctypes (eeg_dataanalysispackage_amd/_lib.py).
 *
 * Threading: every function is reentrant.  Calls that take an eegfx_ctx serialise on that
 * context's HIP stream; use one context per calling thread (e.g. per Spark executor thread,
 * LogisticRegressionClassifier.java:50,90) for concurrency.
 *
 * Memory: pointer arguments of compute calls are host or device pointers as selected by the
 * `mem` argument (EEGFX_MEM_HOST: the library stages through its own device buffers and
 * returns after the results are back in host memory; EEGFX_MEM_DEVICE: pointers are HIP
 * device pointers, the work is enqueued on the context stream and the call returns without
 * synchronising -- call eegfx_ctx_synchronize()).  Device-resident marker positions are
 * validated by the kernels that read them (OffLineDataProvider.java:220-225: pos-100 must lie
 * in [0, n_frames]); a violation is reported as EEGFX_ERANGE by the next call on that context
 * that synchronises it, which also clears it.  The calls that synchronise are
 * eegfx_ctx_synchronize, eegfx_ctx_guard_stats / _detail, every EEGFX_MEM_HOST compute call,
 * eegfx_read_raw with EEGFX_MEM_DEVICE, eegfx_logreg_sgd_train / eegfx_svm_sgd_train /
 * eegfx_dtree_train / eegfx_rforest_train, and eegfx_logreg_predict / eegfx_svm_predict /
 * eegfx_dtree_predict / eegfx_rforest_predict with EEGFX_MEM_DEVICE.  When such a call returns
 * EEGFX_ERANGE for an earlier call's position, its own work has completed and its outputs are
 * valid; the rows of the epochs with the refused positions are unspecified.  Results of
 * EEGFX_MEM_DEVICE calls are unspecified until a synchronising call has returned EEGFX_OK.  Host
 * positions are checked before any work is enqueued and fail the call itself.
 *
 * Numerics: EEGFX_EXACT reproduces the reference's fp64 operation order value for value;
 * EEGFX_FMA runs the fused-multiply-add filter bank and is within 1e-9 of it on every row: a
 * conditioning guard bounds each row's rounding difference from the EXACT row,
 * and the rows it cannot certify (features at rounding level, e.g. a window in the filters' null
 * space) are recomputed under EXACT on the device before the call's results are complete.
 * Samples may hold any bit pattern and resolutions any float: NaN, +-Inf, -0.0, subnormal and
 * overflowing fp32 products are carried through the decode as IEEE arithmetic carries them, and
 * a row comes out as the reference computes it (a NaN or Inf in the window or the baseline gives
 * an all-NaN row, an overflowing sum of squares 0.0 for every finite feature) under both
 * numerics; the rows of the other epochs are unaffected.
 * Epochs: double[n][C][750] is the reference's interface; every epoch sample is an fp32 value
 * widened (EpochHolder.java:75-91), and the *_f32 entries carry the same values as float[n][C][750]
 * at half the bytes (each names the f64 entry it mirrors).
 * Small host batches of eegfx_extract_features_f64 (the per-epoch drop-in) are computed under
 * EXACT in both settings (latency-bound; the guard's counters do not count them), and so are
 * feature sizes above 16 on every path (the full pyramid; see eegfx_extract_features_f64).
 */
#ifndef EEGFX_H_
#define EEGFX_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define EEGFX_ABI_VERSION 1

/* ---- status codes ---------------------------------------------------------------------- */
#define EEGFX_OK 0
#define EEGFX_EINVAL -1    /* bad argument: IllegalArgumentException in the reference      */
#define EEGFX_EIO -2       /* file missing / unreadable: IOException                       */
#define EEGFX_EFORMAT -3   /* malformed .vhdr/.vmrk/info.txt: NumberFormatException & co.  */
#define EEGFX_EHIP -4      /* HIP runtime error                                            */
#define EEGFX_ENOMEM -5    /* allocation failure                                           */
#define EEGFX_ERANGE -6    /* epoch out of range: ArrayIndexOutOfBoundsException           */
#define EEGFX_ENOTSUP -7   /* parameter combination without a kernel                       */

/* ---- constants of the reference (Utils/Const.java:61-71, WaveletTransform.java:47-87) ---- */
#define EEGFX_PRESTIMULUS 100   /* Const.PREESTIMULUS_VALUES  */
#define EEGFX_POSTSTIMULUS 750  /* Const.POSTSTIMULUS_VALUES  */
#define EEGFX_USED_CHANNELS 3   /* Const.USED_CHANNELS        */
#define EEGFX_DWT8_NAME 8       /* fe=dwt-8: WaveletTransform(8, 512, 175, 16), PipelineBuilder.java:131 */
#define EEGFX_DWT8_EPOCH_SIZE 512
#define EEGFX_DWT8_SKIP 175
#define EEGFX_DWT8_FEATURE_SIZE 16
#define EEGFX_DWT8_MAX_FEATURE_SIZE 512 /* the whole pyramid of a 512-sample window */

/* sample formats of BrainVision BinaryFormat= */
#define EEGFX_INT_16 0
#define EEGFX_IEEE_FLOAT_32 1

#define EEGFX_MEM_HOST 0
#define EEGFX_MEM_DEVICE 1

/* numerics of the DWT filter bank */
#define EEGFX_EXACT 0   /* separate fp64 mul + add in the reference order: bit-exact to Java */
#define EEGFX_FMA 1     /* fp64 fused multiply-add: within 1e-9 relative, fewer instructions;
                           rows the conditioning guard cannot certify are recomputed EXACT */

typedef struct eegfx_ctx eegfx_ctx;
typedef struct eegfx_odp eegfx_odp;

/* ---- library / context ------------------------------------------------------------------ */
const char* eegfx_version(void);
const char* eegfx_last_error(void);
int eegfx_device_count(int* count);
/* Creates a context on HIP device `device` with its own non-blocking stream. */
int eegfx_ctx_create(int device, eegfx_ctx** out);
/* Makes the context enqueue on `hip_stream` (hipStream_t, e.g. torch's current stream);
 * NULL restores the context's own stream.  The previous stream is drained first (the context's
 * device buffers are allocated and released in its stream's order).  The context keeps using an
 * external stream until told otherwise -- eegfx_ctx_destroy drains and frees on it too -- so call
 * eegfx_ctx_set_stream(ctx, NULL) before the caller destroys that stream. */
int eegfx_ctx_set_stream(eegfx_ctx* ctx, void* hip_stream);
/* The stream the context currently enqueues on (hipStream_t). */
int eegfx_ctx_stream(eegfx_ctx* ctx, void** hip_stream);
int eegfx_ctx_set_numerics(eegfx_ctx* ctx, int numerics); /* EEGFX_EXACT (default) | EEGFX_FMA */
/* Waits for the context's stream; EEGFX_ERANGE if a kernel enqueued since the last call met a
 * device-resident marker position the reference would not cut (the flag is cleared). */
int eegfx_ctx_synchronize(eegfx_ctx* ctx);
/* Kernel timing for the roofline leg of bench.py.  While enabled, every compute call brackets its
 * dominant kernel (window_kernel for the fused path) with a pair of HIP events on the context
 * stream; eegfx_ctx_kernel_stats returns the number of timed launches, their summed duration
 * (ms) and the algorithmic HBM bytes they moved.  Enabling (again) resets the counters. */
int eegfx_ctx_set_timing(eegfx_ctx* ctx, int enable);
int eegfx_ctx_kernel_stats(eegfx_ctx* ctx, int64_t* launches, double* total_ms,
                           int64_t* total_bytes);
/* The fma numerics' conditioning guard: rows that went through a guarded (EEGFX_FMA) feature
 * launch on this context, and rows the guard recomputed under EEGFX_EXACT, since the context was
 * created or last reset (reset != 0 clears both after reading).  Synchronises the context.
 * Guarded launches include the feature rows eegfx_odp_load_data computes for the provider's
 * resident feature matrix (eegfx_odp_get_features copies them), on the context it was given. */
int eegfx_ctx_guard_stats(eegfx_ctx* ctx, int64_t* rows_checked, int64_t* rows_recomputed,
                          int reset);
/* The same counters, with the rows that failed the guard's a-priori test and went to its second
 * stage (the row's measured max |x|): rows_rechecked >= rows_recomputed, and
 * rows_rechecked - rows_recomputed rows were certified by the second stage.  For float32
 * recordings and double epochs the only test is the measured one: a row that fails it counts in
 * both.  rows_rechecked may be NULL. */
int eegfx_ctx_guard_detail(eegfx_ctx* ctx, int64_t* rows_checked, int64_t* rows_rechecked,
                           int64_t* rows_recomputed, int reset);
/* Opt-in resident server for the per-epoch drop-in (IFeatureExtraction.extractFeatures called
 * once per epoch, LogisticRegressionClassifier.java:55-61): enable != 0 starts one resident
 * workgroup on its own stream that polls a host-mapped command word, so single-epoch
 * EEGFX_MEM_HOST eegfx_extract_features_f64 calls on this context (C <= 16) are served without a
 * kernel launch or a stream synchronisation -- the same device code, the same rows (small
 * batches of more epochs stay on the launch path, which runs them in parallel).  It returns by itself after 1 s without a request (and is restarted by the next one), or
 * when disabled / the context is destroyed.  While it runs, a device-wide synchronisation
 * (hipDeviceSynchronize, hipFree, hipHostFree) waits for it: disable it before such calls (the
 * library makes none: its pinned buffers are pooled for the process, its device buffers are
 * allocated and freed stream-ordered, so creating and destroying contexts never waits).  Its
 * stream has the highest priority, which keeps it on a hardware queue of its own (streams of one
 * priority share a few queues in order).  That pool has 4 queues, so at most 4
 * contexts of a process hold a server on one device at a time: a context enabled beyond that
 * serves its calls on the launch path (same rows) and takes a server once a slot frees.  A
 * server that has not started within 20 ms of its launch (its queue held by other work) is
 * stopped and the call takes the launch path; no request is ever posted to a server that has not
 * started.  Off by default. */
int eegfx_ctx_set_mailbox(eegfx_ctx* ctx, int enable);
/* Whether the resident server is enabled on ctx and whether it currently holds a slot with a
 * started server (either pointer may be NULL). */
int eegfx_ctx_get_mailbox(eegfx_ctx* ctx, int32_t* enabled, int32_t* resident);
int eegfx_ctx_destroy(eegfx_ctx* ctx);

/* ---- BrainVision reader (replaces eegloader-hdfs 2.4 cz.zcu.kiv.signal.*, pom.xml:84-88) - */
typedef struct {
  int32_t number;        /* 1-based channel number (Ch<n>=)            ChannelInfo.getNumber() */
  char name[64];         /* first field, "\1" decoded to ','           ChannelInfo.getName()   */
  char reference[64];
  double resolution;     /* third field; 1.0 when empty                                        */
  char unit[32];         /*                                            ChannelInfo.getUnits()  */
} eegfx_channel_info;

typedef struct {
  int32_t n_channels;          /* NumberOfChannels=                                           */
  int32_t binary_format;       /* EEGFX_INT_16 | EEGFX_IEEE_FLOAT_32                           */
  int32_t multiplexed;         /* DataOrientation=MULTIPLEXED -> 1, VECTORIZED -> 0           */
  double sampling_interval_us; /* SamplingInterval=                                           */
  char data_file[512];
  char marker_file[512];
} eegfx_header_info;

typedef struct {
  int32_t number;         /* Mk<n>                                                           */
  char type[64];          /* e.g. "Stimulus", "New Segment"                                  */
  char description[64];   /* e.g. "S  2"                       EEGMarker.getStimulus()       */
  int64_t position;       /* data point, used verbatim as a 0-based index                    */
  int64_t size;
  int32_t channel;
  int32_t stimulus_index; /* int(digits(description)) - 1, or -1 (OffLineDataProvider.java:207-214) */
} eegfx_marker;

/* DataTransformer.getChannelInfo(vhdr) (OffLineDataProvider.java:167-168). `channels` may be
 * NULL to query; at most max_channels entries are written. */
int eegfx_read_header(const char* vhdr_path, eegfx_header_info* info,
                      eegfx_channel_info* channels, int32_t max_channels);
/* DataTransformer.readMarkerList(vmrk) (OffLineDataProvider.java:196). `markers` may be NULL
 * to query the count. */
int eegfx_read_markers(const char* vmrk_path, eegfx_marker* markers, int64_t max_markers,
                       int64_t* n_markers);
/* Number of frames of a .eeg file given its header (file size / (channels * sample size)). */
int eegfx_recording_frames(const char* vhdr_path, const char* eeg_path, int64_t* n_frames);
/* Reads the raw multiplexed samples of a .eeg file into `dst` (n_frames * n_channels samples of
 * the header's binary format; host or device memory per `mem`).  A DataOrientation=VECTORIZED
 * file (channel after channel) is interleaved into the same multiplexed layout while it is read.
 * The decode itself (a3) is done by the kernels, fused with the epoch cut. */
int eegfx_read_raw(eegfx_ctx* ctx, const char* vhdr_path, const char* eeg_path, void* dst,
                   int64_t capacity_bytes, int mem);

/* ---- marker planning: OffLineDataProvider.java:200-265 (a4 + a8) ----------------------------
 * For each marker in order: skip it (no state change) iff position-100 < 0 or
 * position-100 > n_frames (the AIOOBE of Arrays.copyOfRange, :220-225, caught at :262-264);
 * target iff stimulus_index+1 == guessed (:238-240); class balance (:248-260) with
 * *balance = numberOfTargets - numberOfNonTargets carried across files: accept a target iff
 * *balance <= 0, a non-target iff *balance >= 0.  Writes the accepted positions and labels
 * (1.0 / 0.0) in order.  pos_out/label_out may be NULL to count. */
int eegfx_plan_markers(const eegfx_marker* markers, int64_t n_markers, int64_t n_frames,
                       int32_t guessed, int64_t* balance, int64_t* pos_out, double* label_out,
                       int64_t* n_selected);

/* The same planning on the device, for marker lists of configs[2] size (64M markers): each marker
 * is a map of the balance state {-1, 0, 1} (target: D <= 0 -> D + 1; non-target: D >= 0 -> D - 1;
 * out of range: identity), so the sequential walk is a prefix composition, scanned
 * in parallel, followed by a stream compaction of the accepted markers.  positions /
 * stimulus_index (INT32_MIN = unparsable description: planning stops there with EEGFX_EFORMAT,
 * the accepted prefix kept) and pos_out / label_out per `mem`; *balance must be -1, 0 or 1 (the
 * reference's balance starts at 0 and never leaves that set). */
int eegfx_plan_markers_device(eegfx_ctx* ctx, const int64_t* positions,
                              const int32_t* stimulus_index, int64_t n_markers, int64_t n_frames,
                              int32_t guessed, int64_t* balance, int64_t* pos_out,
                              double* label_out, int64_t* n_selected, int mem);

/* ---- compute ------------------------------------------------------------------------------ */
/* a3 + a5..a7: raw multiplexed recording -> baseline-corrected epochs double[n][C][750]
 * (OffLineDataProvider.java:216-233 + EpochHolder.setFZ/CZ/PZ, the List<double[][]> that
 * getData() returns).  cols[c] = 0-based column of selected channel c, res[c] its resolution
 * (host arrays, C <= 64).  raw/pos/epochs_out per `mem`. */
int eegfx_cut_epochs_f64(eegfx_ctx* ctx, const void* raw, int32_t fmt, int64_t n_frames,
                         int32_t n_channels_total, const int32_t* cols, const float* res,
                         int32_t C, const int64_t* pos, int64_t n_epochs, double* epochs_out,
                         int mem);
/* eegfx_cut_epochs_f64 with float32 epochs, float[n][C][750]: element for element the fp32 value
 * (EpochHolder.setFZ/CZ/PZ stores (double) e[i+100] of a float array) that the f64 entry widens,
 * stored as it is -- widening this buffer gives the f64 entry's buffer bit for bit (-0.0,
 * subnormals, +-Inf, NaN included) at half the bytes.  Same layouts, position checks and status
 * codes.  epochs_out may sit on any 4-byte boundary. */
int eegfx_cut_epochs_f32(eegfx_ctx* ctx, const void* raw, int32_t fmt, int64_t n_frames,
                         int32_t n_channels_total, const int32_t* cols, const float* res,
                         int32_t C, const int64_t* pos, int64_t n_epochs, float* epochs_out,
                         int mem);

/* IFeatureExtraction.extractFeatures (IFeatureExtraction.java:27-35), batched over n epochs:
 * WaveletTransform(name, epoch_size, skip, feature_size).extractFeatures for each
 * epochs[i] = double[C][750] (WaveletTransform.java:107-141).  out = double[n][C*feature_size],
 * each row L2-normalised (SignalProcessing.java:38-52).  Supported: name 8 with epoch_size 512,
 * skip + 512 <= 750, feature_size <= 512 (EEGFX_DWT8_MAX_FEATURE_SIZE) and C <= 64.  A channel's
 * features are the first feature_size coefficients of the in-place pyramid of its 512-sample
 * window (WaveletTransform.java:126-137, :205-212),
 *     [a6(8) d6(8) d5(16) d4(32) d3(64) d2(128) d1(256)]
 * so feature_size <= 16 takes a6 ++ d6 and every larger size adds detail bands, coarsest first.
 * feature_size > 16 is computed under EEGFX_EXACT in both numerics settings (the fma guard has
 * no bound for the detail bands; its counters do not count these rows) and always by a launch:
 * such calls leave a resident server (eegfx_ctx_set_mailbox) and its staging alone.
 * feature_size > 512 and any other name or epoch_size return EEGFX_ENOTSUP. */
int eegfx_extract_features_f64(eegfx_ctx* ctx, const double* epochs, int64_t n, int32_t C,
                               int32_t name, int32_t epoch_size, int32_t skip,
                               int32_t feature_size, double* out, int mem);
/* eegfx_extract_features_f64 on float32 epochs, float[n][C][750] (any 4-byte-aligned pointer):
 * the rows are those of the f64 entry on the same epochs widened to double, bit for bit, under
 * both numerics and for every feature size, skip and C it supports; the same argument checks,
 * status codes, routes (device; small and large host batches, the large ones moving 2,048 bytes
 * per window row over the host link) and guard counters. */
int eegfx_extract_features_f32(eegfx_ctx* ctx, const float* epochs, int64_t n, int32_t C,
                               int32_t name, int32_t epoch_size, int32_t skip,
                               int32_t feature_size, double* out, int mem);

/* The fused hot path: raw multiplexed recording -> dwt-8 feature matrix, without materialising
 * the epochs.  Equals eegfx_cut_epochs_f64 followed by eegfx_extract_features_f64 with
 * (8, 512, 175, 16), bit for bit under EEGFX_EXACT. */
int eegfx_process_recording(eegfx_ctx* ctx, const void* raw, int32_t fmt, int64_t n_frames,
                            int32_t n_channels_total, const int32_t* cols, const float* res,
                            int32_t C, const int64_t* pos, int64_t n_epochs, double* features,
                            int mem);

/* eegfx_process_recording for any WaveletTransform(name, epoch_size, skip, feature_size) that
 * eegfx_extract_features_f64 supports: features = double[n][C * feature_size], equal to
 * eegfx_cut_epochs_f64 followed by eegfx_extract_features_f64 with the same parameters (bit for
 * bit under EEGFX_EXACT; feature_size > 16 is EXACT in both settings, see there).  With
 * (8, 512, 175, 16) it is eegfx_process_recording itself, the fused kernels.  Every other
 * combination cuts the epochs into the context's scratch memory (float32: 3,000 C bytes per epoch) and
 * extracts from them on the device, for every layout eegfx_cut_epochs_f64 accepts: a fused
 * kernel for wide rows measured slower than the two passes at feature_size 512 (DESIGN.md
 * 5.4.1).  Positions are validated as in
 * eegfx_process_recording: host positions fail the call with EEGFX_ERANGE, device positions are
 * reported by the next synchronising call.  skip + 512 > 750 is EEGFX_ERANGE, feature_size > 512
 * or another name / epoch_size EEGFX_ENOTSUP. */
int eegfx_process_recording_fe(eegfx_ctx* ctx, const void* raw, int32_t fmt, int64_t n_frames,
                               int32_t n_channels_total, const int32_t* cols, const float* res,
                               int32_t C, const int64_t* pos, int64_t n_epochs, int32_t name,
                               int32_t epoch_size, int32_t skip, int32_t feature_size,
                               double* features, int mem);

/* getData() and extractFeatures in one pass (OffLineDataProvider.java:216-233 materialises the
 * epochs, LogisticRegressionClassifier.java:87-90 then maps WaveletTransform.extractFeatures over
 * them): the baseline-corrected epochs double[n][C][750] (epochs_out) and their dwt-8 rows
 * double[n][16 C] (features) from one read of each epoch's frames, the filter bank running on
 * the frames the epoch write staged.  Each output equals its own call (eegfx_cut_epochs_f64 /
 * eegfx_process_recording), bit for bit under EEGFX_EXACT.  epochs_out == NULL: the same as
 * eegfx_process_recording.  Layouts whose epoch span does not fit one workgroup's LDS (more than
 * ~40 int16 / ~20 float32 channels in the file) run the two passes instead. */
int eegfx_process_recording_epochs(eegfx_ctx* ctx, const void* raw, int32_t fmt, int64_t n_frames,
                                   int32_t n_channels_total, const int32_t* cols,
                                   const float* res, int32_t C, const int64_t* pos,
                                   int64_t n_epochs, double* features, double* epochs_out,
                                   int mem);
/* eegfx_process_recording_epochs with float32 epochs, float[n][C][750] (as eegfx_cut_epochs_f32:
 * the fp32 values the f64 entry widens, any 4-byte-aligned pointer); `features` are the f64
 * entry's rows, bit for bit.  The same layouts take the one pass and the two passes. */
int eegfx_process_recording_epochs_f32(eegfx_ctx* ctx, const void* raw, int32_t fmt,
                                       int64_t n_frames, int32_t n_channels_total,
                                       const int32_t* cols, const float* res, int32_t C,
                                       const int64_t* pos, int64_t n_epochs, double* features,
                                       float* epochs_out, int mem);

/* configs[4] -- long recordings streamed from host memory: raw (host, n_frames x
 * n_channels_total samples), pos and features are HOST arrays; the recording is moved to the device
 * in chunks of at most chunk_frames frames (>= 787, the frames one epoch spans) on an upload
 * stream that runs up to three chunks ahead of the kernels (a ring of four device chunk buffers;
 * pageable sources go through two pinned staging buffers that the context keeps for later calls
 * and frees when it is destroyed, pinned sources are copied directly),
 * and the rows of each chunk return on a download stream.  Positions may come in any
 * order; features[i] belongs to pos[i].  Results equal eegfx_process_recording on the whole
 * recording (bit for bit under EEGFX_EXACT).  Replaces the whole-file readBinaryData decode of
 * OffLineDataProvider.java:186-188 for recordings that are not kept resident. */
int eegfx_process_recording_streamed(eegfx_ctx* ctx, const void* raw, int32_t fmt,
                                     int64_t n_frames, int32_t n_channels_total,
                                     const int32_t* cols, const float* res, int32_t C,
                                     const int64_t* pos, int64_t n_epochs, double* features,
                                     int64_t chunk_frames);

/* ---- the downstream classifier ----------------------------------------
 * LogisticRegressionClassifier.java:85-114 trains Spark MLlib 1.6.2 LogisticRegressionWithSGD on
 * the feature rows: the default constructor (step 1.0, 100 iterations, regParam 0.01, fraction
 * 1.0) or, with the config_* keys, the static train(...) with regParam 0.0.  This runs that
 * full-batch gradient descent on the device: LogisticGradient, SquaredL2Updater with
 * step/sqrt(i), GradientDescent's convergence test (||w_prev - w|| < tol * max(||w||, 1), MLlib's
 * tol = 0.001), no intercept.  X is n x d row-major (the feature matrix as produced), y the 0/1
 * labels; `weights` holds the initial weights (zeros in MLlib) on entry and the trained ones on
 * return (host array).  mini_batch_fraction < 1 samples each iteration's mini-batch as MLlib does
 * (eegfx_logreg_sgd_train_partitioned below); labels other than 0/1 give EEGFX_EINVAL ("Input
 * validation failed").  eegfx_logreg_predict: LogisticRegressionModel.predict -- score = 1/(1+exp(-(w.x+b))),
 * out = score > threshold ? 1 : 0, or the score itself when threshold is NaN (clearThreshold). */
int eegfx_logreg_sgd_train(eegfx_ctx* ctx, const double* X, const double* y, int64_t n, int32_t d,
                           int32_t num_iterations, double step_size, double reg_param,
                           double mini_batch_fraction, double convergence_tol, double* weights,
                           int32_t* iterations_run, int mem);
int eegfx_logreg_predict(eegfx_ctx* ctx, const double* X, int64_t n, int32_t d,
                         const double* weights, double intercept, double threshold, double* out,
                         int mem);
/* The same training with the Spark partition count stated.  mini_batch_fraction f in [0, 1)
 * (config_mini_batch_fraction, LogisticRegressionClassifier.java:98-108, README.md:136): iteration
 * i (1-based) trains on MLlib's data.sample(false, f, 42 + i) of the n rows split into
 * num_partitions ParallelCollectionRDD slices (partition p: rows [p n / N, (p + 1) n / N)), the
 * sample drawn on the host with Spark 1.6.2's own sampler (PartitionwiseSampledRDD seeds from
 * java.util.Random, BernoulliSampler / GapSamplingIterator on XORShiftRandom; eegfx_spark_sample)
 * and the gradient divided by the sample size; an empty sample skips the update.  f >= 1: the
 * full batch.  eegfx_logreg_sgd_train is this function with num_partitions = the host's hardware
 * threads (Spark local[*]'s defaultParallelism, SparkInitializer.java:44). */
int eegfx_logreg_sgd_train_partitioned(eegfx_ctx* ctx, const double* X, const double* y,
                                       int64_t n, int32_t d, int32_t num_iterations,
                                       double step_size, double reg_param,
                                       double mini_batch_fraction, double convergence_tol,
                                       int32_t num_partitions, double* weights,
                                       int32_t* iterations_run, int mem);
/* RDD.sample(false, fraction, seed) of n rows in num_partitions slices (pure host function):
 * mask = bit r of word r / 32 set for every kept row ((n + 31) / 32 words), *kept = their count. */
int eegfx_spark_sample(int64_t n, double fraction, int32_t num_partitions, int64_t seed,
                       uint32_t* mask, int64_t* kept);

/* ---- train_clf=dt: the decision tree (DecisionTreeClassifier.java:99-127) --------------------
 * MLlib 1.6.2 DecisionTree over continuous features and two classes, as DESIGN.md section 10
 * states it: per-feature thresholds from min(n, max(max_bins^2, 10000)) sampled rows (all rows, or
 * RDD.sample(false, required / n, split_seed) in one partition), rows binned on the device, one
 * integer class histogram per node and level, the best split chosen on the host, rows routed to
 * their children on the device.  The statistics are integer counts and every gain is plain fp64,
 * so the tree is defined bit for bit.  eegfx_dtree_train writes the nodes ascending by `id` into
 * the host array `nodes`; when `capacity` is too small it returns EEGFX_EINVAL with the count
 * needed in *n_nodes.  Limits: 1 <= d <= 1024, 2 <= max_bins <= 256 (above: EEGFX_ENOTSUP),
 * 0 <= max_depth <= 30, min_instances_per_node >= 1, 2 <= n < 2^31.  A non-finite feature or a
 * label other than 0.0 / 1.0 is EEGFX_EINVAL.  eegfx_dtree_predict walks the tree per row (left
 * iff x[feature] <= threshold, so a NaN goes right) and writes the leaf's `predict`; a node array
 * whose children do not lie inside the array and after their parent, or with a feature >= d, is
 * EEGFX_EINVAL.  `mem` covers X, y and out; both calls synchronise. */
#define EEGFX_GINI 0
#define EEGFX_ENTROPY 1
typedef struct {
  int32_t id;            /* Spark node index: root 1, children 2i and 2i + 1 */
  int32_t feature;       /* -1: leaf */
  int32_t left, right;   /* array positions of the children, -1: leaf */
  double threshold, predict, impurity, gain;
} eegfx_tree_node;
int eegfx_dtree_train(eegfx_ctx* ctx, const double* X, const double* y, int64_t n, int32_t d,
                      int32_t impurity, int32_t max_depth, int32_t max_bins,
                      int32_t min_instances_per_node, int64_t split_seed,
                      eegfx_tree_node* nodes /* host */, int32_t capacity, int32_t* n_nodes,
                      int mem);
int eegfx_dtree_predict(eegfx_ctx* ctx, const double* X, int64_t n, int32_t d,
                        const eegfx_tree_node* nodes /* host */, int32_t n_nodes, double* out,
                        int mem);

/* ---- train_clf=rf: the random forest (RandomForestClassifier.java:101-136) --------------------
 * MLlib 1.6.2 RandomForest over continuous features and two classes, as DESIGN.md section 10.2
 * states it: the decision tree's thresholds and bins (one table for all trees); every tree's row
 * weights from commons-math's PoissonDistribution(1.0) on a Well19937c, one sampler per
 * ParallelCollectionRDD slice seeded with seed + slice + 1 (num_trees == 1: every weight 1);
 * feature_subset features per node (AUTO: ALL for one tree, else SQRT), drawn per node by reservoir
 * sampling seeded from java.util.Random(seed); nodes split in queue order, in groups of at most
 * 256 MB of aggregates; prediction is the majority of the trees' votes, 0.0 on a tie.  The
 * weights and the weighted histograms are integers and the gains the decision tree's fp64, so
 * the forest is defined bit for bit.  eegfx_rforest_train writes the trees one after another into
 * the host array `nodes` (each ascending by `id`, `left` / `right` relative to the tree's first
 * node) and tree t's range into tree_offsets[t], tree_offsets[t + 1]; when `capacity` is too
 * small it returns EEGFX_EINVAL with the count needed in *n_nodes.  num_trees = 1 with AUTO or ALL
 * is eegfx_dtree_train's tree.  num_partitions 0: the processors available to the process, as
 * eegfx_logreg_sgd_train takes them.  Limits: eegfx_dtree_train's, num_trees >= 1,
 * num_partitions >= 0; a Poisson draw above 255 or a tree whose weights sum above 2^32 - 1 is
 * EEGFX_ENOTSUP.  eegfx_rforest_predict refuses (EEGFX_EINVAL) offsets that do not ascend from 0
 * and a tree that eegfx_dtree_predict would refuse.  eegfx_poisson_bag (pure host function) writes
 * the weights uint8 [num_trees][n] the training draws. */
#define EEGFX_SUBSET_AUTO 0
#define EEGFX_SUBSET_ALL 1
#define EEGFX_SUBSET_SQRT 2
#define EEGFX_SUBSET_LOG2 3
#define EEGFX_SUBSET_ONETHIRD 4
int eegfx_rforest_train(eegfx_ctx* ctx, const double* X, const double* y, int64_t n, int32_t d,
                        int32_t impurity, int32_t max_depth, int32_t max_bins,
                        int32_t min_instances_per_node, int32_t num_trees, int32_t feature_subset,
                        int64_t seed /* the reference: 12345 */, int32_t num_partitions,
                        int64_t split_seed, eegfx_tree_node* nodes /* host */, int32_t capacity,
                        int32_t* tree_offsets /* host, [num_trees + 1] */, int32_t* n_nodes,
                        int mem);
int eegfx_rforest_predict(eegfx_ctx* ctx, const double* X, int64_t n, int32_t d,
                          const eegfx_tree_node* nodes /* host */,
                          const int32_t* tree_offsets /* host */, int32_t num_trees, double* out,
                          int mem);
int eegfx_poisson_bag(int64_t n, int32_t num_trees, int32_t num_partitions, int64_t seed,
                      uint8_t* weights);

/* eegfx_svm_* (MLlib SVMWithSGD on the same device loop) is declared in eegfx_ext.h: SURVEY.md
 * section 2 marks the SVM classifier out of the hot-path scope, so it is not part of this contract. */

/* ---- multi-GPU ------------------------------------------------------------
 * Epochs shard by contiguous ranges of the selected-epoch list (eegfx_shard_range: balanced, the
 * first n % world ranks take one more); each rank runs the fused path on its range with no
 * collective; eegfx_gather then assembles the [n_total][cols] feature matrix in rank order (the
 * reference's getData() order, OffLineDataProvider.java:370) on every rank, by one RCCL broadcast
 * per rank inside a group (ragged shards land directly in their rows).  `local` and `out` are
 * device pointers on the communicator's context device; the collective runs on that context's
 * stream.  One communicator per (process, device): rank 0 creates the unique id and ships it to
 * the other ranks out of band (e.g. a Spark broadcast variable); a single process that drives
 * several devices (Spark local[*]) uses eegfx_comm_init_all and brackets its per-device gathers
 * with eegfx_group_start / eegfx_group_end. */
#define EEGFX_COMM_ID_BYTES 128
typedef struct eegfx_comm eegfx_comm;
int eegfx_shard_range(int64_t n, int32_t rank, int32_t world, int64_t* start, int64_t* end);
/* The schedule eegfx_gather runs: for every root r < world, the first row offsets[r] and the row
 * count counts[r] of the broadcast rooted at r (= eegfx_shard_range of r; a root with no rows
 * issues no broadcast).  Pure host function. */
int eegfx_gather_schedule(int64_t n_total, int32_t world, int64_t* offsets, int64_t* counts);
int eegfx_comm_unique_id(void* id /* EEGFX_COMM_ID_BYTES */);
int eegfx_comm_create(eegfx_ctx* ctx, int32_t world, int32_t rank, const void* id,
                      eegfx_comm** out);
int eegfx_comm_init_all(eegfx_ctx* const* ctxs, int32_t n, eegfx_comm** out /* n */);
int eegfx_comm_rank(const eegfx_comm* comm, int32_t* rank, int32_t* world);
int eegfx_gather(eegfx_comm* comm, const double* local, int64_t n_total, int64_t cols,
                 double* out);
/* Rooted gather ("grouped ncclSend/ncclRecv to rank 0"): the [n_total][cols]
 * matrix is assembled on `root` only -- the reference's consumer is one JVM holding one list
 * (OffLineDataProvider.java:370-379 getData(), parallelize on the driver in
 * LogisticRegressionClassifier.java:87-94).  Every other rank sends its shard once, the root
 * receives each ragged shard straight into its rows of `out` (its own shard: a device copy, or
 * nothing when `local` already is those rows), all inside one RCCL group, on the context
 * stream.  `out` is read on the root only (may be NULL elsewhere).  Root inbound traffic is
 * (world-1)/world of the matrix over its world-1 xGMI links, where eegfx_gather moves the whole
 * matrix to every rank. */
int eegfx_gather_root(eegfx_comm* comm, const double* local, int64_t n_total, int64_t cols,
                      int32_t root, double* out);
/* The point-to-point plan eegfx_gather_root issues on `rank` (pure host function): up to `world`
 * operations {kind, peer, first row, rows}; the root receives from every other rank with rows
 * (in rank order) and copies its own shard, every other rank with rows sends once to the root. */
#define EEGFX_GATHER_SEND 0
#define EEGFX_GATHER_RECV 1
#define EEGFX_GATHER_COPY 2
typedef struct {
  int32_t kind;  /* EEGFX_GATHER_SEND | _RECV | _COPY                          */
  int32_t peer;  /* the other rank (the root for a send; the rank itself for a copy) */
  int64_t row;   /* first row of the shard in the [n_total][cols] matrix             */
  int64_t rows;  /* rows moved                                                        */
} eegfx_gather_op;
int eegfx_gather_root_plan(int64_t n_total, int32_t world, int32_t rank, int32_t root,
                           eegfx_gather_op* ops /* world entries */, int32_t* n_ops);
int eegfx_group_start(void);
int eegfx_group_end(void);
int eegfx_comm_destroy(eegfx_comm* comm);

/* Deterministic synthetic multiplexed int16 recording, generated on device:
 * DC -25000 counts + bounded random walk + 10 Hz sinusoid, clipped to int16.  dst is a device
 * pointer of n_frames * n_channels int16. */
int eegfx_synth_recording(eegfx_ctx* ctx, int16_t* dst, int64_t n_frames, int32_t n_channels,
                          uint64_t seed);

/* ---- OffLineDataProvider (OffLineDataProvider.java:42-380) ----------------------------------
 * Same argument conventions as the Java constructor: args = { "<info.txt>" } or
 * { "<file.eeg>", "<guessed>", optional... } (1..6 entries).  Paths are local files (the HDFS
 * client of the reference is out of scope).  load_data never fails: like the reference
 * (:88-98) it stops at the first fatal error and keeps what was loaded; the message is
 * available from eegfx_odp_error(). */
/* The provider with one shard, on `ctx`: eegfx_odp_create_multi's provider over that one context
 * (same planning pass, same worker, run on the calling thread), with the reference's sequential
 * semantics in two places.  A repeated load_data appends: files, the Fz/Cz/Pz indices, the
 * balance, the counters and the epochs of earlier loads persist as the reference's fields do
 * (:53-60); the shard is reallocated once per load at its exact size and the rows it held are
 * copied on the context stream (its `features` are dropped, and recomputed by get_features,
 * once two loads ran under different numerics).  And the payload of every listed recording is
 * opened where the reference reads it, in file order and ahead of the file's markers, so one
 * that cannot be opened stops the load there (EEGFX_EIO) even if no epoch is selected from it;
 * eegfx_odp_create_multi's workers open only the files their epochs come from.
 * ctx may be NULL: a planning-only provider parses, selects and labels (positions, labels,
 * file indices) without reading the sample payload or touching a GPU. */
int eegfx_odp_create(eegfx_ctx* ctx, const char* const* args, int32_t n_args, eegfx_odp** out);
int eegfx_odp_load_data(eegfx_odp* odp);
const char* eegfx_odp_error(const eegfx_odp* odp);       /* "" when loading succeeded */
int64_t eegfx_odp_num_epochs(const eegfx_odp* odp);
/* getData(): double[n][3][750] host copy */
int eegfx_odp_get_data(const eegfx_odp* odp, double* out);
/* eegfx_odp_get_data as float[n][3][750]: the resident double epochs narrowed on the device
 * (exact: every value is a widened fp32), so half the bytes cross the host link. */
int eegfx_odp_get_data_f32(const eegfx_odp* odp, float* out);
/* getDataLabels(): double[n] */
int eegfx_odp_get_labels(const eegfx_odp* odp, double* out);
/* Selected marker positions (int64[n]) and source file index (int32[n]) of every epoch. */
int eegfx_odp_get_positions(const eegfx_odp* odp, int64_t* pos_out, int32_t* file_out);
/* fe=dwt-8 features of every loaded epoch, computed on the device from the resident epochs. */
int eegfx_odp_get_features(eegfx_odp* odp, int32_t name, int32_t epoch_size, int32_t skip,
                           int32_t feature_size, double* out);
void eegfx_odp_destroy(eegfx_odp* odp);

/* ---- OffLineDataProvider over several contexts ----------------------------------------------
 * A provider over n_ctx contexts (1..EEGFX_ODP_MAX_SHARDS), any mix of devices, each context at
 * most once (a repeated context: EEGFX_EINVAL, as two shards would share its scratch buffers).
 * ctxs == NULL with n_ctx >= 1: a planning-only provider that reports the same shard ranges and
 * touches no GPU and no sample payload.
 *
 * eegfx_odp_load_data on such a provider works in two phases.  It first plans on the host, once
 * and in file order, exactly as the planning-only provider does (headers, the Fz/Cz/Pz indices
 * and the target / non-target balance carried across files, markers): the whole selected-epoch
 * list.  Context r then owns the epochs eegfx_shard_range(n, r, n_ctx) of that list -- the
 * partition eegfx_gather_root expects of rank r, so a shard's `features` is a valid `local`
 * argument for it.  One worker thread per context that has epochs walks the files its range
 * intersects (a single such context: the calling thread), reads only the frames eegfx_shard_span
 * names for its positions in each file,
 * uploads them and runs the one-pass kernels on its context's stream, into resident buffers
 * allocated once at their exact size.  Every context has been drained when load_data returns.
 *
 * All contexts must hold the same numerics at load_data (else EEGFX_EINVAL, nothing is loaded).
 * The call starts over: what an earlier load_data of the provider left is released first
 * (eegfx_odp_create's provider appends instead).
 * After the call num_epochs, positions, labels, file indices, the return code and the
 * eegfx_odp_error text equal those of eegfx_odp_create's provider on the same arguments (bit for
 * bit under EEGFX_EXACT; within the fma contract under EEGFX_FMA, whose guard strategy is
 * per-context state), but for a payload that cannot be opened in a file no epoch comes from.  A failure a worker meets in file j (a payload read, a HIP error)
 * overrides an error planning found in file j or later and keeps only the epochs of the files
 * before j; the shard ranges are then the planned ranges clipped to what is kept -- the one
 * exception to the balanced partition.
 *
 * eegfx_odp_get_data / _get_data_f32 / _get_labels / _get_positions / _get_features return rows
 * in list order: each shard does the one-context work on its own context, straight into rows
 * [first, first + count) of the caller's buffer, enqueued on every context before any is
 * drained.  eegfx_odp_destroy frees every shard on its own device.  The threading rule of a
 * context extends to the provider: no other call may use one of its contexts during a call on
 * the provider. */
#define EEGFX_ODP_MAX_SHARDS 64
int eegfx_odp_create_multi(eegfx_ctx* const* ctxs, int32_t n_ctx, const char* const* args,
                           int32_t n_args, eegfx_odp** out);

/* The device view of one shard.  The pointers stay valid until the next eegfx_odp_load_data or
 * eegfx_odp_destroy of the provider and are complete when eegfx_odp_load_data returns.
 * eegfx_odp_create's provider has one shard, over everything it holds. */
typedef struct {
  int32_t ctx_index;         /* index into ctxs                                                 */
  int32_t device;            /* HIP device of that context; -1 for a planning-only provider      */
  int64_t first, count;      /* the shard's epochs in getData() order                            */
  const double* epochs;      /* device, double[count][3][750]; NULL if count == 0 / planning     */
  const double* features;    /* device, double[count][48], rows of (8,512,175,16) computed at
                                loadData; NULL if count == 0 / planning / not resident           */
  int32_t features_numerics; /* EEGFX_EXACT | EEGFX_FMA of those rows, -1 if features == NULL    */
} eegfx_odp_shard;
int eegfx_odp_num_shards(const eegfx_odp* odp);   /* 1 for eegfx_odp_create's provider */
int eegfx_odp_get_shard(const eegfx_odp* odp, int32_t i, eegfx_odp_shard* out);

/* Pure host function: the frames a shard's epochs of one recording touch.
 * first_frame = min(pos) - 100, frames = min(n_frames, max(pos) + 750) - first_frame
 * (positions in any order, each with pos - 100 in [0, n_frames]; n == 0 gives 0, 0).  An epoch
 * cut from the span with positions rebased by first_frame and n_frames = frames equals the one
 * cut from the whole recording: the span keeps the recording's end, so the zero padding past it
 * is the same. */
int eegfx_shard_span(const int64_t* pos, int64_t n, int64_t n_frames, int64_t* first_frame,
                     int64_t* frames);

/* ---- the train/test flow (PipelineBuilder.java:170-223) on the device ------------------------
 * The train_clf branch shuffles the epochs and the labels with Random(1), splits 70/30, trains,
 * tests and reports four counters.  These entries keep the feature rows on the device from the
 * provider's shards to the classifiers.
 *
 * eegfx_java_shuffle (pure host function): perm[i] is the original index of the element at
 * position i after Collections.shuffle(list, new Random(seed)) of a list of n items.  n outside
 * [0, 2^31) is EEGFX_EINVAL.
 *
 * eegfx_gather_rows: dst[i][0:d] = src[idx[i]][0:d] for i < m, rows of 1 <= d <= 1536 doubles
 * copied as bits (NaN payloads and -0.0 survive), idx may repeat; src [n_src][d], idx and dst
 * [m][d] all live on the side `mem` names and need only 8-byte alignment.  An idx[i] outside
 * [0, n_src) copies nothing for row i; the call then returns EEGFX_ERANGE and names the smallest
 * such i (host memory: that row keeps what dst held).  m == 0 is EEGFX_OK without a launch.
 * The call synchronises.
 *
 * eegfx_confusion_counts: counts = {tp, tn, fp, fn} of pred[n] against labels[n] in the
 * reference's reading of MulticlassMetrics' column-major matrix (LogisticRegressionClassifier
 * .java:129-137): tp = actual 1 / predicted 1, tn = actual 0 / predicted 0, "fp" = actual 1 /
 * predicted 0, "fn" = actual 0 / predicted 1.  A prediction that is neither 0.0 nor 1.0 (NaN, a
 * raw score) is counted nowhere.  A label that is neither 0.0 nor 1.0 is EEGFX_EINVAL (checked
 * first); labels of one class only, or n == 0, are EEGFX_ERANGE: the reference's cm[1] throws.
 * `counts` is host memory; `mem` names the side of pred and labels.  The call synchronises.
 *
 * eegfx_odp_split: X[n][3 * feature_size] = the provider's feature rows (eegfx_odp_get_features
 * with the same parameters, bit for bit) and y[n] = its labels, both in the order
 * eegfx_java_shuffle(n, seed) gives; rows [0, *n_train) are the training part, *n_train =
 * (int64_t)(n * train_fraction) as (int)(data.size()*0.7) truncates.  `mem` names the side of X
 * and y; device buffers live on ctx's device (ctx == NULL: the provider's first context).  Every
 * shard lands its rows in a buffer of ctx by a device-to-device copy on its own stream; the
 * gathers for X and y then run on ctx's stream, so no row passes through host memory.
 * train_fraction outside [0, 1] and a planning-only provider are EEGFX_EINVAL; n == 0 is
 * EEGFX_OK with *n_train = 0.  The call synchronises. */
int eegfx_java_shuffle(int64_t n, int64_t seed, int64_t* perm);
int eegfx_gather_rows(eegfx_ctx* ctx, const double* src, int64_t n_src, int32_t d,
                      const int64_t* idx, int64_t m, double* dst, int mem);
int eegfx_confusion_counts(eegfx_ctx* ctx, const double* pred, const double* labels, int64_t n,
                           int64_t counts[4], int mem);
int eegfx_odp_split(eegfx_odp* odp, eegfx_ctx* ctx, int64_t seed, double train_fraction,
                    int32_t name, int32_t epoch_size, int32_t skip, int32_t feature_size,
                    double* X, double* y, int64_t* n_train, int mem);

/* ---- the flow over the provider's shards: data-parallel SGD, rows in place --------------------
 * eegfx_odp_split gathers every shard's rows on one context.  These entries leave them where they
 * are: the split is kept per shard, LogisticRegressionWithSGD /
 * SVMWithSGD sum their gradient where the rows live and move d doubles per shard and iteration,
 * and the four counters are integers that add.
 *
 * eegfx_split_shard_plan (pure host function): the rows [first, first + count) of a list of n
 * rows, within [0, n], as the split of eegfx_odp_split(seed, train_fraction) sees them.  With
 * perm = eegfx_java_shuffle(n, seed) and cut = (int64_t)(n * train_fraction), the row
 * first + idx[j] stands at position p of perm: j < *n_train lists the training rows (p < cut,
 * pos[j] = p), j >= *n_train the *n_test test rows (pos[j] = p - cut), each part in increasing p.
 * idx and pos hold `count` entries.
 *
 * eegfx_odp_split_sharded: out[s], s < eegfx_odp_num_shards, is shard s's part of that split, on
 * its own context: the feature rows eegfx_odp_split takes for the same parameters (the resident
 * `features` where they match, else the rows eegfx_odp_get_features computes) and the labels,
 * gathered on the shard's stream, with the position of every row in its part.  No feature row
 * crosses a device boundary or reaches host memory.  A pointer is NULL where its count is 0.  The
 * provider owns the buffers: they stay valid until the next eegfx_odp_split_sharded,
 * eegfx_odp_load_data or eegfx_odp_destroy.  Errors are those of eegfx_odp_split; n == 0 is
 * EEGFX_OK with every count 0.  Every context has been drained when the call returns. */
typedef struct {
  int32_t ctx_index;         /* index into the provider's contexts                               */
  int32_t pad;
  int64_t n_train, n_test;
  const double* X_train;     /* device, double[n_train][3 * feature_size]                        */
  const double* y_train;     /* device, double[n_train]                                          */
  const int64_t* pos_train;  /* device, position of each row in the training part, increasing    */
  const double* X_test;      /* device, double[n_test][3 * feature_size]                         */
  const double* y_test;
  const int64_t* pos_test;   /* device, position of each row in the test part, increasing        */
} eegfx_split_shard;
int eegfx_split_shard_plan(int64_t n, int64_t first, int64_t count, int64_t seed,
                           double train_fraction, int64_t* idx, int64_t* pos, int64_t* n_train,
                           int64_t* n_test);
int eegfx_odp_split_sharded(eegfx_odp* odp, int64_t seed, double train_fraction, int32_t name,
                            int32_t epoch_size, int32_t skip, int32_t feature_size,
                            eegfx_split_shard* out /* eegfx_odp_num_shards */);

/* eegfx_glm_sgd_train_sharded: eegfx_logreg_sgd_train_partitioned (grad 0, LogisticGradient) or
 * the hinge loop of eegfx_ext.h (grad 1, HingeGradient: full batch only) over rows that lie in
 * n_shards pieces, each on its own context (any mix of devices; each context at most once, else
 * EEGFX_EINVAL).  X [n][d], y [n] and pos [n] are device pointers on that context's device.  pos
 * names the position of each row in the whole training list (distinct, within [0, sum of n));
 * pos == NULL: the shard's rows follow those of the shards before it.  The positions only matter
 * to mini_batch_fraction < 1, whose iteration i takes the rows of data.sample(false, f, 42 + i)
 * over the whole list in num_partitions slices.  Shards with n == 0 take no part; the first shard
 * with rows is the root.  Per iteration every shard sums the gradient of its rows on its own
 * stream and sends d doubles to the root, the root updates and sends the state back: no host
 * synchronisation, the ordering is stream events.  The sum over shards is taken in shard order,
 * so runs are bit-reproducible; one shard gives the bits of the one-context entry.
 * `weights` holds the initial weights on entry and the result on return (untouched by a failing
 * call); arguments, bounds and errors are those of the one-context entry.  Every context has been
 * drained when the call returns.
 *
 * eegfx_glm_shard_state: the training state the last eegfx_glm_sgd_train_sharded, or the last
 * one-context train entry (one shard of its own), left on ctx -- head = {iterations, flag (1:
 * done), updates, 0} and the d weights: on every shard that took part it equals the root's, bit
 * for bit.
 *
 * eegfx_glm_count_sharded: counts = {tp, tn, fp, fn} in eegfx_confusion_counts' reading, of the
 * model's predictions (grad 0: LogisticRegressionModel, grad 1: SVMModel; threshold NaN: the raw
 * score, as clearThreshold) against y over every shard's rows: what eegfx_logreg_predict followed
 * by eegfx_confusion_counts gives on the rows together, without a prediction in memory.  pos is
 * not read.  A label that is neither 0.0 nor 1.0 on any shard is EEGFX_EINVAL (checked first);
 * labels of one class only over all shards, or no rows, are EEGFX_ERANGE.  Synchronises. */
typedef struct {
  eegfx_ctx* ctx;
  const double* X;
  const double* y;
  const int64_t* pos;
  int64_t n;
} eegfx_glm_shard;
int eegfx_glm_sgd_train_sharded(int grad, const eegfx_glm_shard* shards, int32_t n_shards,
                                int32_t d, int32_t num_iterations, double step_size,
                                double reg_param, double mini_batch_fraction,
                                double convergence_tol, int32_t num_partitions, double* weights,
                                int32_t* iterations_run);
int eegfx_available_processors(void);  /* eegfx_logreg_sgd_train's num_partitions: local[*] */
int eegfx_glm_shard_state(eegfx_ctx* ctx, int32_t d, int32_t head[4], double* weights);
int eegfx_glm_count_sharded(int grad, const eegfx_glm_shard* shards, int32_t n_shards, int32_t d,
                            const double* weights, double intercept, double threshold,
                            int64_t counts[4]);

/* ---- train_clf=nn: the dense network of NeuralNetworkClassifier.java on the device ------------
 * DESIGN.md section 10.7 holds the definition; DL4J itself is not reproduced bit for bit (it
 * computes in float32 and draws its initial weights from ND4J's stream).  Everything is float64.
 *
 * The model: n_layers (1..4) layers; layer l maps n_in (d for the first, the previous layer's
 * n_out otherwise) to n_out[l] units, a = f(x W + b) with f = activation[l].  Hidden widths lie in
 * [1, 64]; the last layer's n_out must be 2 (the reference fits labels {t, |1 - t|}).  The
 * parameters are one flat double vector, layer after layer, each W[n_in][n_out] row-major followed
 * by b[n_out]; the count of it is what the param_count entry returns (a pure host function;
 * a negative status for a model that is refused, the text in eegfx_last_error()).
 *
 * eegfx_nn_train: num_iterations full-batch iterations from params0 (host memory, as params_out
 * and scores_out are): the gradient of `loss` over the two outputs against {y, |1 - y|}, summed
 * over the rows and divided by n, then p <- p - u with the updater's u (lr = learning_rate,
 * mu = momentum):
 *   SGD        u = lr g
 *   NESTEROVS  v' = mu v - lr g; u = mu v - (1 + mu) v'
 *   ADAM       (0.9, 0.999, 1e-8) u = lr sqrt(1 - b2^t) / (1 - b1^t) m / (sqrt(v) + eps)
 *   ADAGRAD    (1e-6) h += g^2; u = lr g / (sqrt(h) + eps)
 *   RMSPROP    (0.95, 1e-8) r = 0.95 r + 0.05 g^2; u = lr g / sqrt(r + eps)
 * scores_out (may be NULL): the loss before each iteration's step, num_iterations doubles.
 * num_iterations == 0 returns params0.  A label other than 0.0 / 1.0 is EEGFX_EINVAL and leaves
 * params_out and scores_out alone; non-finite features are trained on (they make the parameters
 * they reach non-finite).  The sums run in an order fixed by (n, d, the widths): two calls give the
 * same bits, from host or device rows.  X [n][d] and y [n] live on the side `mem` names, 1 <= d <=
 * 1024, n >= 1.  The call synchronises.
 *
 * eegfx_nn_predict: out[r] = output 0 of the last layer for row r (the reference's
 * model.output(features).getDouble(0)); X and out on the side `mem` names, params host memory.
 *
 * eegfx_nn_statistics: Utils/ClassificationStatistics.add(score, label) over n pairs, with
 * round = Java's Math.round: a label that rounds to 0 counts a true negative if the score rounds
 * to 0, else a false positive, and adds the score to sums[1]; a label that rounds to 1 counts a
 * true positive if the score rounds to 1, else a false negative, and adds the score to sums[2];
 * any other label counts nowhere.  sums[0] = the sum of (label - score)^2 over all pairs.
 * counts = {tp, tn, fp, fn}; counts and sums are host memory, scores and labels on the side `mem`
 * names.  n == 0 gives zeros.  The call synchronises. */
#define EEGFX_NN_MAX_LAYERS 4
#define EEGFX_NN_MAX_WIDTH 64
enum {
  EEGFX_NN_ACT_SIGMOID = 0, EEGFX_NN_ACT_TANH = 1, EEGFX_NN_ACT_RELU = 2,
  EEGFX_NN_ACT_IDENTITY = 3, EEGFX_NN_ACT_SOFTPLUS = 4, EEGFX_NN_ACT_ELU = 5,
  EEGFX_NN_ACT_SOFTMAX = 6
};
enum { EEGFX_NN_LOSS_MSE = 0, EEGFX_NN_LOSS_XENT = 1, EEGFX_NN_LOSS_NLL = 2,
       EEGFX_NN_LOSS_SQUARED = 3 };
enum { EEGFX_NN_UPD_NESTEROVS = 0, EEGFX_NN_UPD_SGD = 1, EEGFX_NN_UPD_ADAM = 2,
       EEGFX_NN_UPD_ADAGRAD = 3, EEGFX_NN_UPD_RMSPROP = 4 };
typedef struct {
  int32_t n_layers;
  int32_t n_out[EEGFX_NN_MAX_LAYERS];
  int32_t activation[EEGFX_NN_MAX_LAYERS]; /* EEGFX_NN_ACT_* */
  int32_t loss;                            /* EEGFX_NN_LOSS_* */
  int32_t updater;                         /* EEGFX_NN_UPD_* */
  int32_t num_iterations;
  double learning_rate;
  double momentum;
} eegfx_nn_config;
int64_t eegfx_nn_param_count(int32_t d, const eegfx_nn_config* cfg);
int eegfx_nn_train(eegfx_ctx* ctx, const double* X, const double* y, int64_t n, int32_t d,
                   const eegfx_nn_config* cfg, const double* params0, double* params_out,
                   double* scores_out, int mem);
/* eegfx_nn_train under one of DL4J 0.8's line-search optimisers (config_optimization_algo =
 * line_gradient_descent, conjugate_gradient -- the reference's default -- or lbfgs), as DESIGN.md
 * section 10.8 defines them: every iteration a BackTrackLineSearch of at most
 * max_line_search_iterations trials (1..32; DL4J's default is 5) along the direction the
 * algorithm builds from the updater's output for the mean gradient, then a gradient pass at the
 * new parameters; training stops early at ZeroDirection or EpsTermination.  params_out: the
 * parameters after the last iteration run.  scores_out (may be NULL): the loss at the start of
 * each iteration run; search_out (may be NULL): per iteration run the step the search returned,
 * the score it holds for that step and the trials it evaluated; entries at or past
 * *iterations_run (may be NULL) are left as they were.  algorithm == EEGFX_NN_OPT_SGD is
 * eegfx_nn_train bit for bit (iterations_run = num_iterations, search_out untouched).  Labels,
 * non-finite features, the order of the sums and `mem` as for eegfx_nn_train; num_iterations == 0
 * returns params0 without a launch.  The call synchronises once, at its end. */
enum { EEGFX_NN_OPT_SGD = 0, EEGFX_NN_OPT_LINE_GD = 1, EEGFX_NN_OPT_CG = 2, EEGFX_NN_OPT_LBFGS = 3 };
typedef struct { int32_t algorithm; int32_t max_line_search_iterations; } eegfx_nn_optimizer;
typedef struct { double step; double score; int32_t trials; int32_t pad; } eegfx_nn_search;
int eegfx_nn_train_opt(eegfx_ctx* ctx, const double* X, const double* y, int64_t n, int32_t d,
                       const eegfx_nn_config* cfg, const eegfx_nn_optimizer* opt,
                       const double* params0, double* params_out, double* scores_out,
                       eegfx_nn_search* search_out, int32_t* iterations_run, int mem);
int eegfx_nn_predict(eegfx_ctx* ctx, const double* X, int64_t n, int32_t d,
                     const eegfx_nn_config* cfg, const double* params, double* out, int mem);
int eegfx_nn_statistics(eegfx_ctx* ctx, const double* scores, const double* labels, int64_t n,
                        int64_t counts[4], double sums[3], int mem);

#ifdef __cplusplus
}
#endif
#endif /* EEGFX_H_ */
