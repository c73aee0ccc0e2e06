/*
 * wsa.h — C ABI of libwsa: the MI355X (gfx950) implementation of the formantanalyzer hot path
 *         PCM -> Hann -> FFT -> mel -> u32 frame -> peak scan -> voiced state machine / noise gate
 *         -> formant tracking -> segment finalize -> (syllables) -> 53-feature vectors.
 *
 * This is the drop-in boundary.  Every entry point names the reference interface
 * it stands in for; "ref" = /root/reference/dist/main.js (line 2, byte offset "@B<n>") which
 * bundles formantanalyzer@1.1.6, and /root/reference/src/index.js (its caller).
 * INTEGRATION.md shows the N-API / ctypes bindings over this header.
 *
 * Conventions: plain C types only; every function returns a wsa_status (0 = OK); the library
 * never falls back to a CPU path — if no gfx950 device / code object is available, wsa_create
 * fails with WSA_ERR_NO_DEVICE.  A context is not thread-safe; distinct contexts are.
 */
#ifndef WSA_H
#define WSA_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define WSA_ABI_VERSION 5       /* 5: wsa_queue_create / wsa_queue_destroy (a HIP stream for hosts without a HIP binding: batches of one device overlap instead of queueing on the null stream); 4: wsa_host_alloc / wsa_host_free (page-locked clip memory), wsa_gather_rows runs every rank on its own device and stream; 3: wsa_gather_* (multi-GPU collection over RCCL); 2: wsa_stream_rows gained stream_cuts, formants, utt_*, track_*, WSA_FLAG_STREAM_CUT, d_spectra always set, default output_level 4 */
#define WSA_NFEAT 53            /* ref src/localstore.js:7 process_exp_features_len[5] == [13] == 53 */
#define WSA_NUTT 264            /* utterance features of output_level 11 (ref @B107902: 15 histograms) */

typedef enum {
    WSA_OK = 0,
    WSA_ERR_INVALID = 1,        /* bad argument / unsupported configuration */
    WSA_ERR_NO_DEVICE = 2,      /* no gfx950 GPU or HIP runtime failure at create */
    WSA_ERR_HIP = 3,            /* HIP runtime error (see wsa_last_error) */
    WSA_ERR_CAPACITY = 4,       /* a device-side arena overflowed (reported, never silently wrong) */
    WSA_ERR_BUSY = 5            /* "Error: Already playing" (ref @B4554) */
} wsa_status;

/*
 * Configuration = the reference's settings object: defaults ref @B2965, merged by
 * configure(cfg) ref @B3292, forwarded to the worklet ref @B6726 and to reset_segmentation
 * ref @B24629.  Units as in the reference (Hz, ms, dB).  wsa_config_default() fills the
 * reference defaults.
 */
typedef struct {
    int32_t spec_type;          /* 1 mel bands (hot path), 2 power bins, 3 magnitude bins */
    int32_t output_level;       /* 5 = segment features, 13 = syllable features; 4 / 10 = segment / syllable formant
                                   frames (rows carry the indices, d_formants the [len][9] frames); 11 = level 10 plus the
                                   264 utterance features after every result (d_utt_*); 12 = one row per syllable whose
                                   first 23 feature slots hold the polynomial coefficients (slot 23 = 1 marks a syllable on
                                   which numeric.uncmin threw in the reference: its make_coeffs then returns only the rows
                                   before it, so a host reports the segment's features up to that row, the times in full); 3: indices only;
                                   1,2: u32 spectrum frames only — the back end is not run, any band count) */
    double  f_min, f_max;       /* Hz */
    int32_t N_fft_bins, N_mel_bins;
    double  window_width, window_step;     /* ms */
    double  pause_length, min_seg_length;  /* ms */
    int32_t auto_noise_gate;
    double  voiced_max_dB, voiced_min_dB;
    double  pre_norm_gain, high_f_emph;
} wsa_config;

typedef struct wsa_ctx wsa_ctx;         /* one per (config, device) — the module-level state of ref inner module 1 */
typedef struct wsa_batch wsa_batch;     /* a planned batch shape: n_clips x n_samples[] at one sample rate */

void wsa_config_default(wsa_config *cfg);                                 /* ref @B2965 */
int  wsa_abi_version(void);

/* ref: module load + configure() (@B3292).  device = HIP device ordinal. */
wsa_status wsa_create(const wsa_config *cfg, int32_t device, wsa_ctx **out);
void       wsa_destroy(wsa_ctx *ctx);
const char *wsa_last_error(const wsa_ctx *ctx);   /* ctx may be NULL: last create error */

/* Geometry the front end derives from (config, fs): what ref reset_nodes (@B6992) hands the worklet. */
typedef struct {
    int32_t nfft, win, hop, bands, kmax;
} wsa_geometry;
wsa_status wsa_geometry_for(const wsa_ctx *ctx, double fs, wsa_geometry *out);
/* centre frequency of each output band — the `{bins_Hz: [...]}` message of the worklet (ref @B8380) */
wsa_status wsa_bins_hz(const wsa_ctx *ctx, double fs, double *out, int32_t n);

/*
 * Plan a batch: n_clips independent clips ("launches" in the reference's terms: each clip is one
 * LaunchAudioNodes(1, buffer, cb, labels, offline=true, test_play=false) run, ref @B4469), clip i
 * having n_samples[i] mono float32 samples at `fs`.  Allocates all device work space; nothing is
 * allocated in wsa_batch_run.
 */
wsa_status wsa_batch_create(wsa_ctx *ctx, uint32_t n_clips, const uint32_t *n_samples, double fs, wsa_batch **out);
/*
 * The same with a sample-rate conversion in front: the clips the caller hands to wsa_batch_run / wsa_batch_run_host
 * are at fs_in (n_samples_in[i] samples), the analysis runs on their conversion to fs_out (wsa_resample_length
 * samples each) — what the browser's decodeAudioData does to a file before the reference sees it (its offline path
 * decodes into `new OfflineAudioContext(1, 48e6, 48e3)`, ref dist/main.js:2 @B18769: always 48 kHz).  The converter is
 * specified here, not by the reference (RS-1, DESIGN.md: 32-tap windowed sinc, 32 sub-sample offsets, parity unpinned).
 * The converted PCM lives in the batch; wsa_batch_copy_pcm hands it out.
 */
wsa_status wsa_batch_create_resampled(wsa_ctx *ctx, uint32_t n_clips, const uint32_t *n_samples_in, double fs_in, double fs_out, wsa_batch **out);
uint64_t   wsa_resample_length(uint64_t n_in, double fs_in, double fs_out);      /* trunc(n_in * fs_out / fs_in) */
/*
 * The same for clips of different rates (an addition within version 5: probe for wsa_batch_create_mixed): clip i arrives at
 * fs_in[i] (n_samples_in[i] samples) and is analysed at fs_out.  Stands in for the application's folder loop: every file of a
 * folder, one after the other (ref src/index.js:277-296), goes to the browser's decodeAudioData inside
 * `new OfflineAudioContext(1, 48e6, 48e3)` (ref dist/main.js:2 @B18769), which converts whatever rate the file has - here as ONE launch.
 *   - fs_in[i] != fs_out: clip i is converted by RS-1 with its own ratio = fs_in[i] / fs_out (in double, exactly like that) and
 *     its own offset-kernel table; wsa_resample_length(n_samples_in[i], fs_in[i], fs_out) samples.
 *   - fs_in[i] == fs_out: clip i is NOT filtered; its samples reach the front end bit for bit, length unchanged (what the browser
 *     does with a file at the context's rate).  RS-1 at ratio 1 is a 0.9-Nyquist low-pass, not an identity:
 *     wsa_batch_create_resampled with equal rates keeps filtering, this entry point copies.
 *   - Every rate positive and within a factor 16 of fs_out, converted lengths below 2^32 - 16: else WSA_ERR_INVALID with a message
 *     that names the clip.  Any number of distinct rates (one 8.4 KB table per rate).
 *   - Everything that works on a resampling batch works on this one, unchanged in shape: wsa_batch_run (clip i at
 *     d_pcm + i * clip_stride, clip_stride >= the longest INPUT clip), wsa_batch_run_host, wsa_batch_run_host_i16,
 *     wsa_batch_copy_pcm, wsa_batch_get_info, results, stage times, wsa_batch_classify.  wsa_batch_run allocates nothing and
 *     stays capturable into a hipGraph.
 */
wsa_status wsa_batch_create_mixed(wsa_ctx *ctx, uint32_t n_clips, const uint32_t *n_samples_in, const double *fs_in, double fs_out, wsa_batch **out);
/* converted PCM of a resampling batch after a run: pcm [n_clips][stride] floats, stride >= the longest converted clip */
wsa_status wsa_batch_copy_pcm(wsa_batch *b, void *stream, float *pcm, uint64_t stride);
void       wsa_batch_destroy(wsa_batch *b);

/*
 * Run the whole hot path on device-resident PCM.  d_pcm is a device pointer; clip i starts at
 * d_pcm + i * clip_stride (floats).  `stream` is a hipStream_t (NULL = default stream).  Fully
 * asynchronous: only kernel launches / async copies are enqueued, so the call can be captured in
 * a hipGraph and timed with events on `stream`.
 * Stands in for: worklet process() (not in ref tree) -> port.onmessage -> spectrum_push (@B8752,
 * @B30392) -> D() (@B25717) -> O() (@B27088) for every frame of every clip.
 */
wsa_status wsa_batch_run(wsa_batch *b, const float *d_pcm, uint64_t clip_stride, void *stream);

/* Same, PCM in host memory (clip i at pcm[i]); copies H2D on `stream` first (PCIe-inclusive path). */
wsa_status wsa_batch_run_host(wsa_batch *b, const float *const *pcm, void *stream);
/* Same with 16-bit PCM as a WAV file holds it (ref: the file's ArrayBuffer goes in as it is, src/index.js:291): clip i = its samples
 * interleaved over `channels[i]` channels (NULL: all mono), channel 0 is analysed; n_samples[i] of the plan counts frames of one
 * channel.  Half the PCIe bytes of the float path; the conversion x / 32768 runs on the device and is exact in fp32, so the rows equal
 * those of wsa_batch_run_host on the converted floats bit for bit.  Uploads are issued clip by clip on `stream` in front of the kernels. */
wsa_status wsa_batch_run_host_i16(wsa_batch *b, const int16_t *const *pcm, const uint32_t *channels, void *stream);
/* Page-locked host memory for the clips of the two entry points above (no counterpart in the reference: the app hands the browser the file's
 * ArrayBuffer, src/index.js:291).  A copy out of ordinary (pageable) memory is staged by the runtime through its own pinned buffers on the calling
 * thread; a clip that already lies in memory from wsa_host_alloc goes to the device by DMA at the link's rate.  Hosts that read many files
 * allocate their clip buffers here (the Node host: allocPinned).  Any clip pointer is accepted by the run functions either way.
 * wsa_host_free(NULL) is a no-op.  The copy out of page-locked memory is a true asynchronous DMA: until the run's stream has completed, clip buffers
 * must stay allocated AND unmodified (a host that refills a slab for the next batch waits for wsa_batch_result of the one in flight first, or
 * alternates between two slabs).  Clips that lie back to back inside ONE wsa_host_alloc allocation (and keep the device layout's alignment) travel as
 * one copy; copies are never merged across two allocations, however close they lie. */
wsa_status wsa_host_alloc(wsa_ctx *ctx, uint64_t bytes, void **out);
void       wsa_host_free(void *p);
/* A stream of the library's own on the context's device (a non-blocking hipStream_t), for hosts that have no HIP binding to make one (the Node addon):
 * what every `stream` argument of this header accepts.  Runs handed different queues overlap on the device — the upload of one batch under the kernels
 * of another (the reference's app loops over files one launch at a time, src/index.js:277-296; a host that does the same over batches keeps the PCIe
 * link busy that way) — where runs on NULL, the device's null stream, queue up behind each other.  Destroy a queue only when nothing runs on it. */
wsa_status wsa_queue_create(wsa_ctx *ctx, void **stream);
void       wsa_queue_destroy(wsa_ctx *ctx, void *stream);
/* Waits for everything enqueued on `stream` (NULL: the device's null stream) — for hosts without a HIP binding that call an entry which
 * only enqueues and hands out no copy of its own, such as wsa_regress_rows on page-locked rows (probe for it: an addition within version 5). */
wsa_status wsa_queue_synchronize(wsa_ctx *ctx, void *stream);

/*
 * Results of the last run (device resident, compacted in (clip, si[, syllable]) order — the order
 * in which the reference would have invoked callback(si, label, seg_time, features), ref @B28869).
 *
 * rows:     one per callback feature vector: level 5 one per reported segment, level 13 one per
 *           syllable.  meta columns (int32):
 *             [0] clip  [1] si (callback index within the clip, ref `callbacks_processed-1`)
 *             [2] t_start frame  [3] t_len frames   -> seg_time as the reference computes it
 *                 level 5:  [t_start*step_s, (t_len+1)*step_s]                       (ref @B31504)
 *                 level 13: [((t_start)*step_s).toFixed(3), ((t_len+1)*step_s).toFixed(3)]
 *                           with t_start = segments_ci[si][0] + syl_start            (ref @B31114)
 *             [4] own segment index in segments_ci  [5] syllable index in its segment (level 13, else 0)
 *             [6] own start frame (segment, or segment start + syllable start)  [7] own length
 *           features: double[53] per row (ref @B33436 order).
 * segments: every [start,len] the reference pushes to segments_ci (ref @B27190), including the
 *           ones whose straighten step throws (flag -1): int32 [n_segments][4] =
 *           {clip, start, len, flag} with flag 1 = reported, 0 = no feature rows, -1 = dropped.
 */
typedef struct {
    uint32_t n_clips, n_rows, n_segments, n_frames_total;
    uint32_t status_flags;                /* WSA_FLAG_* */
    const int32_t  *d_row_meta;           /* device [n_rows][8] */
    const double   *d_row_feat;           /* device [n_rows][53] */
    const int32_t  *d_segments;           /* device [n_segments][4] */
    const uint32_t *d_clip_row_off;       /* device [n_clips+1] */
    const uint32_t *d_clip_seg_off;       /* device [n_clips+1] */
    const uint32_t *d_spectra;            /* device [n_frames_total][bands] u32 frames (the worklet's output) */
    const uint32_t *d_clip_frame_off;     /* device [n_clips+1] */
    const float    *d_formants;           /* levels 4 / 10 (else NULL): device [n_frames_total][9] f32 — the straightened
                                             frames (3 x bin, band energy, width; ref @B35074) of every reported segment,
                                             frame d of the segment of a row at d_clip_frame_off[clip] + meta[6] + d
                                             (level 4: the row's segment; level 10: the row's syllable, meta[7] frames) */
    /* level 11 (else 0 / NULL): one entry per callback `callback(0, label, Y(), get_utterance_features(...))` of the
     * reference's dispatcher (ref @B28869, @B107902), i.e. one per result, each over everything the clip produced so far */
    uint32_t        n_utterance_rows;
    const int32_t  *d_utt_meta;           /* device [n][4] = {clip, result index, t_start frame, t_sum frames}:
                                             seg_time = [t_start*step_s, (t_sum+1)*step_s]  (ref Y() @B31330) */
    const double   *d_utt_feat;           /* device [n][264] */
    const uint32_t *d_clip_utt_off;       /* device [n_clips+1] */
} wsa_device_result;

/* Synchronises `stream`, reads the counters back and fills `out` (pointers stay valid until the
 * next run on this batch or wsa_batch_destroy). */
wsa_status wsa_batch_result(wsa_batch *b, void *stream, wsa_device_result *out);

/* Copy results to caller-provided host buffers (any pointer may be NULL to skip it).
 * Capacities in elements of the respective row type; fails with WSA_ERR_INVALID if too small. */
wsa_status wsa_batch_copy_rows(wsa_batch *b, void *stream, int32_t *row_meta, double *row_feat, uint32_t rows_cap,
                               int32_t *segments, uint32_t seg_cap, uint32_t *clip_row_off, uint32_t *clip_seg_off);
wsa_status wsa_batch_copy_spectra(wsa_batch *b, void *stream, uint32_t *spectra, uint64_t cap_words, uint32_t *clip_frame_off);
/* The u32 frames (the worklet's messages, ref @B8568) are handed from the front end to the peak scan through an array in HBM, so
 * they are always available after a run (wsa_batch_copy_spectra, d_spectra); this call is kept for hosts written against ABI
 * version 1, where a fused front end could keep them on the chip, and has no effect. */
wsa_status wsa_batch_keep_spectra(wsa_batch *b, int32_t on);
/* Number of times results were fetched only after a second pass of the back end with the full-size tracker table (the
 * default tracker variant keeps its active-track table in LDS and reports an overflow; see wsa_batch_result).  A hipGraph
 * captured from wsa_batch_run keeps replaying the variant it was captured with: re-capture after this number changed. */
wsa_status wsa_batch_backend_reruns(const wsa_batch *b, uint32_t *out);
/* levels 4 / 10: the whole d_formants table ([n_frames_total][9] floats; rows of frames outside reported segments are unspecified) */
wsa_status wsa_batch_copy_formants(wsa_batch *b, void *stream, float *formants, uint64_t cap_frames);
/* level 3: the ranked raw formant tracks of every segment — what the reference's callback receives as its third
 * argument (`s.push(get_ranked_formants())`, ref dist/main.js:2 @B28273; dispatched by `b(e, label, s[e])` @B30132).
 * Segments in the order of d_segments.  seg_off [n_segments + 1][2] = offsets of a segment's points / ranked ids;
 * points [n_points][8] in arrival order = {track id, bin | width << 8, band energy (f64: lo, hi word), start bin,
 * amplitude (u32), filing index (the reference's frame list entry), end bin} — the per-point entries of the 18-field
 * track record (@B35952: [7] frames, [8] starts, [9] ends, [10] bins, [11] amps, [12] energies; every other field is a
 * function of them); ranked [n_ranked] = ids of the tracks with count >= 2 and mean bin >= 7, ascending by mean bin (@B35670). */
typedef struct { uint32_t n_segments; uint64_t n_points, n_ranked; } wsa_tracks_info;
wsa_status wsa_batch_tracks_info(wsa_batch *b, void *stream, wsa_tracks_info *out);
wsa_status wsa_batch_copy_tracks(wsa_batch *b, void *stream, uint64_t *seg_off, int32_t *points, uint64_t cap_points, int32_t *ranked, uint64_t cap_ranked);
/* level 11: the utterance-feature entries (any pointer may be NULL); cap_rows in entries */
wsa_status wsa_batch_copy_utterance(wsa_batch *b, void *stream, int32_t *utt_meta, double *utt_feat, uint32_t cap_rows, uint32_t *clip_utt_off);

/* Capacity bounds of a planned batch (so callers can size buffers before running). */
typedef struct {
    uint32_t n_clips, n_frames_total, max_frames_per_clip, bands;
    uint32_t rows_cap, segments_cap;      /* worst-case totals */
    uint64_t workspace_bytes;             /* device memory held by the batch */
} wsa_batch_info;
wsa_status wsa_batch_get_info(const wsa_batch *b, wsa_batch_info *out);

/* Per-stage device time of the last run in ms, measured with HIP events on the run's stream
 * (valid after wsa_batch_result): [0] front end (PCM->u32), [1] peak candidates + gate + span order,
 * [2] tracker (formant tracking + finalize), [3] compaction. */
wsa_status wsa_batch_stage_ms(wsa_batch *b, float out[4]);

/* Stage events are recorded on the run's stream by default; switch them off before capturing a run
 * into a hipGraph. */
wsa_status wsa_batch_enable_timing(wsa_batch *b, int32_t on);

/* Per-frame state trace of the sequential stage (tests / debugging): 12 doubles per frame =
 * c_ci, c_started, no_fm_segs, ctx_max, noise_floor, n_peaks, argmax bin, h, d, g (the values the
 * reference's frame loop holds just before `c_ci++`, ref @B26985) and the tracker's non-formant /
 * formant energy accumulators (ref @B35952 `s`, `c`). */
wsa_status wsa_batch_enable_trace(wsa_batch *b, int32_t on);
wsa_status wsa_batch_copy_trace(wsa_batch *b, void *stream, double *out, uint64_t cap_rows);

/* Run only the front end (PCM -> u32 frames), for front-end parity tests and profiling. */
wsa_status wsa_batch_run_frontend(wsa_batch *b, const float *d_pcm, uint64_t clip_stride, void *stream);
/* Run only the back end on caller-supplied u32 frames laid out like d_spectra (device pointer). */
wsa_status wsa_batch_run_backend(wsa_batch *b, const uint32_t *d_spectra, void *stream);

/*
 * ---- Collection of the feature rows of several GPUs (BASELINE config 4: clips sharded per GPU, "a single RCCL gather over xGMI").
 * No counterpart in the reference: it runs one launch per file on one device (ref src/index.js:291) and all state is per launch
 * (reset_segmentation, ref dist/main.js:2 @B24629), so clips shard over GPUs with nothing exchanged on the data path; collecting the row
 * tables is the only communication.  One PROCESS drives the GPUs here (the Node host: configure({devices: [...]})): one context per
 * GPU = one rank, one planned batch per context holding that rank's clips.  After wsa_batch_run on every batch, wsa_gather_rows reads the
 * ranks' row counts (every run publishes them) and moves exactly each rank's rows — [rows][8] int32 metadata and [rows][53] double
 * features, in their own types — into the root context's device memory with ONE grouped RCCL exchange (ncclSend / ncclRecv over the
 * direct xGMI links; the root's own rows as a send to itself in the same group): rows of rank 0, rank 1, ... back to back, each rank's
 * rows in its own (clip, callback) order with meta[0] = the clip's index inside its rank.  Then one copy from the root device
 * (wsa_gather_copy_rows) instead of one per GPU.  librccl is loaded on first use; WSA_ERR_NO_DEVICE if it is not there.
 * With one process per GPU (bench.py under torch.distributed) the same protocol runs as webspeechanalyzer_amd/gather.py.
 */
typedef struct wsa_gather wsa_gather;
typedef struct {
    uint32_t n_ranks, n_rows;             /* n_rows = sum of rows_per_rank */
    const uint32_t *rows_per_rank;        /* host [n_ranks], valid until the next gather */
    const int32_t  *d_row_meta;           /* root device [n_rows][8] */
    const double   *d_row_feat;           /* root device [n_rows][53] */
} wsa_gather_result;
/* ctxs[i] = rank i (distinct devices); root = index of the context whose device collects */
wsa_status wsa_gather_create(wsa_ctx *const *ctxs, int32_t n_ranks, int32_t root, wsa_gather **out);
void       wsa_gather_destroy(wsa_gather *g);
/* batches[i] = rank i's batch, planned on ctxs[i] (checked) and run on streams[i].  Waits for every rank's run, then enqueues the
 * exchange, every rank's calls with that rank's device current: on streams[i], or — where streams or streams[i] is NULL — on a stream
 * of the gather's own on rank i's device (never "the null stream of whatever device is current").  The tables are complete when the
 * root's stream is (wsa_gather_copy_rows waits for it).  d_row_meta / d_row_feat / rows_per_rank belong to the wsa_gather and are
 * valid until the NEXT wsa_gather_rows on it (which may free and re-allocate the tables) or wsa_gather_destroy.  If a call inside the
 * RCCL group fails, the group is still closed, the first error is returned (wsa_last_error of the root context) and the wsa_gather
 * refuses further use: destroy it and create a new one.  A wsa_gather is not thread-safe (one gather at a time per object). */
wsa_status wsa_gather_rows(wsa_gather *g, wsa_batch *const *batches, void *const *streams, wsa_gather_result *out);
/* Waits for the last gather and copies its tables to the host (either pointer may be NULL); rows_cap in rows. */
wsa_status wsa_gather_copy_rows(wsa_gather *g, int32_t *row_meta, double *row_feat, uint32_t rows_cap);

/*
 * ---- Streams: n_streams concurrent launches advancing in lock step (BASELINE config "streaming").
 * Stands in for the reference's online path: the worklet's process() per frame -> port message ->
 * spectrum_push (ref @B8752, @B30392) with the module-level segmenter / tracker state carried from
 * frame to frame, the callback fired when a segment closes (ref @B28869), and StopAudioNodes ->
 * segment_truncate (ref @B5699, @B30757) at the end of a stream.  Every step hands each stream
 * frames_per_step * hop new samples; results are identical to running the whole signal as one clip.
 * A step only enqueues work (H2D of the control words, kernels, D2H of the step's rows) and is captured
 * into a hipGraph after the first call (wsa_stream_enable_graph), so a step is one graph launch.
 */
typedef struct wsa_stream wsa_stream;

/* status_flags of wsa_device_result / wsa_stream_rows */
#define WSA_FLAG_CAPACITY   1u   /* a device-side arena overflowed: results invalid (the call also returns WSA_ERR_CAPACITY) */
#define WSA_FLAG_STREAM_CUT 8u   /* streams: some stream's voiced span reached max_span_frames in this step and was cut (stream_cuts tells which);
                                    that stream's rows deviate from one uninterrupted run until its next pause — not an error */

#define WSA_STREAM_ACTIVE 1u    /* the stream has samples in this step */
#define WSA_STREAM_START  2u    /* fresh launch state before this step's frames (ref reset_segmentation @B24629) */
#define WSA_STREAM_STOP   4u    /* segment_truncate after this step's frames (ref @B30757): flushes the open segment */

/* max_span_frames: longest voiced span (frames between two segmenter resets) a stream may hold, rounded
 * up to a power of two.  A source that does not pause for that long is cut there as if it had been stopped and started again
 * (segment_truncate, ref @B30757): the segment so far is reported, tracking starts afresh — for THAT stream only, and
 * counted in wsa_stream_rows.stream_cuts; its results deviate from one uninterrupted run until its next pause. */
wsa_status wsa_stream_create(wsa_ctx *ctx, uint32_t n_streams, double fs, uint32_t frames_per_step,
                             uint32_t max_span_frames, wsa_stream **out);
void       wsa_stream_destroy(wsa_stream *st);
uint32_t   wsa_stream_samples_per_step(const wsa_stream *st);        /* frames_per_step * hop */

/* One step on device-resident PCM: stream i's new samples at d_pcm + i * stream_stride.  ctl = host array
 * of n_streams control bytes (WSA_STREAM_*), or NULL: START|ACTIVE on the first step, ACTIVE afterwards.
 * A launch's signal is the concatenation of the samples the stream was handed in its ACTIVE steps since its START.  A step without
 * WSA_STREAM_ACTIVE is a step in which no time passes for that stream: its row is not read (it may hold anything), its carried samples and
 * its analysis state stay as they are, and the next ACTIVE step continues the signal where the last one ended, however many steps lie
 * between.  WSA_STREAM_START needs no WSA_STREAM_STOP before it: a START while a launch is live, even one whose first frames have not yet
 * been delivered, drops that launch where it stands (its open segment is not reported) and begins a new one whose frames see none of the
 * earlier samples.  With overlapping windows (q = ceil(win / hop) > 1) frame k of a launch, samples [k hop, k hop + win), is analysed in the
 * step that brings the launch to (k + q) hop samples, so the first q - 1 frame slots after a START stay empty. */
wsa_status wsa_stream_step(wsa_stream *st, const float *d_pcm, uint64_t stream_stride, const uint8_t *ctl, void *stream);
/* Same with the samples in the stream object's own pinned host buffer ([n_streams][samples_per_step]
 * floats): fill it, call this; the H2D copy is part of the step (and of its graph).  The device reads the buffer while the
 * step runs: refill it only after wsa_stream_collect has returned for that step. */
float     *wsa_stream_host_input(wsa_stream *st);
wsa_status wsa_stream_step_host(wsa_stream *st, const uint8_t *ctl, void *stream);

/* Rows of the last step, in (stream, callback) order; meta / feature layout as wsa_device_result with
 * [0] = stream index and [1] = callback index since the stream's START.  Host memory owned by the stream
 * object, valid until the next step. */
typedef struct {
    uint32_t n_rows, n_segments, status_flags;
    const int32_t *row_meta;       /* [n_rows][8] */
    const double  *row_feat;       /* [n_rows][53] */
    const int32_t *segments;       /* [n_segments][4] = {stream, start, len, flag} */
    const uint32_t *stream_cuts;   /* [n_streams] spans cut at max_span_frames since the stream's START */
    /* levels 4 / 10 (else NULL): the straightened frames (3 x bin, band energy, width; ref @B35074) of row r's segment (level 4) or
     * syllable (level 10): meta[7] frames of 9 floats starting at formants + 9 * row_formant_off[r] ([n_rows + 1] offsets) */
    const float    *formants;
    const uint32_t *row_formant_off;
    /* level 11 (else 0 / NULL): one entry per result of this step, as wsa_device_result's utterance tables — utt_meta [n][4] =
     * {stream, result index since START, first segment's start, sum of the segment lengths so far}, utt_feat [n][264]: the histograms over
     * everything the stream has produced since its START (ref @B107902), carried on the device from step to step */
    uint32_t        n_utterance_rows;
    const int32_t  *utt_meta;
    const double   *utt_feat;
    /* level 3 (else 0 / NULL): the ranked raw tracks of this step's segments, laid out as wsa_batch_copy_tracks lays them out — track_off
     * [n_segments + 1][2] = first point / first ranked id of segment k, track_points [n_track_points][8], track_ranked [n_track_ranked] */
    uint64_t        n_track_points, n_track_ranked;
    const uint64_t *track_off;
    const int32_t  *track_points;
    const int32_t  *track_ranked;
} wsa_stream_rows;
wsa_status wsa_stream_collect(wsa_stream *st, void *stream, wsa_stream_rows *out);   /* synchronises `stream` */
wsa_status wsa_stream_enable_graph(wsa_stream *st, int32_t on);
/* n_steps timed steps (measurement helper): step k copies feed[k mod feed_steps] ([n_streams][samples_per_step] floats; NULL: the
 * input buffer stays as it is) into the pinned input buffer, then wsa_stream_step_host + wsa_stream_collect are timed with the
 * host's monotonic clock; out_us[k] = microseconds of step k, *rows_total = feature rows produced (may be NULL). */
wsa_status wsa_stream_time_steps(wsa_stream *st, uint32_t n_steps, const float *feed, uint32_t feed_steps, void *stream, double *out_us, uint64_t *rows_total);

/*
 * ---- Syllable classification (additions within version 5: probe for wsa_model_create).
 * Stands in for what the reference APPLICATION does with the level-13 rows when `predict_en` is set (ref src/index.js:56,
 * src/prediction.js:47-169): ml5 `classifyMultiple` with a trained dense network (dist/nnmodel/<db>/cats_<label>/) over a
 * callback's syllables, the fold of the per-syllable confidences into one [label, confidence] per callback, and the per-launch
 * accumulator behind the app's meters (Label_conf_all).  K6 runs the network (f32 MFMA; tolerance against tfjs, DESIGN.md
 * "K6"), K6b the fold (exact double arithmetic).  Everything is enqueued on the caller's stream; after the first
 * wsa_batch_classify on a batch nothing is allocated, so wsa_batch_run + wsa_batch_classify can be captured into a hipGraph.
 * A model belongs to the context it was created on; destroy it before that context.
 */
typedef struct wsa_model wsa_model;
enum { WSA_ACT_LINEAR = 0, WSA_ACT_RELU = 1, WSA_ACT_SIGMOID = 2, WSA_ACT_TANH = 3, WSA_ACT_SOFTMAX = 4 };
#define WSA_MODEL_MAX_LAYERS 8
#define WSA_MODEL_MAX_WIDTH 1024
#define WSA_MODEL_MAX_CLASSES 64
typedef struct {
    int32_t n_layers;                     /* Dense layers, 1 .. WSA_MODEL_MAX_LAYERS */
    const int32_t *units;                 /* [n_layers + 1]; units[0] must be the row width of an ML level (wsa_level_feature_count:
                                             53, 264 or 23), widths <= WSA_MODEL_MAX_WIDTH, units[n_layers] <= WSA_MODEL_MAX_CLASSES */
    const int32_t *activation;            /* [n_layers] WSA_ACT_*; softmax only on the last layer */
    const float *const *kernel;           /* [n_layers] -> [units[i]][units[i+1]] row-major (the tfjs Dense kernel) */
    const float *const *bias;             /* [n_layers] -> [units[i+1]] */
    const double *in_min, *in_max;        /* [units[0]] model_meta.json inputs["0" .. "units[0] - 1"].min / max */
    const char *const *labels;            /* [units[n_layers]] the legend keys in legend order, or NULL.  Only used for the order in which the
                                             fold scans labels: keys that are array indices ("0", "17") come first, ascending, as in
                                             Object.keys (ref prediction.js:134) */
} wsa_model_desc;
/* The feature count of one stored row at an output level whose ML panel the reference application enables (ref src/index.js:723,
 * src/localstore.js:7 process_exp_features_len): 53 at levels 5 and 13, 264 at level 11, 23 at level 12; 0 at every other level.  A
 * model's input count must be one of the three (anything else, the 63 of the shipped ords_V among it, is refused).  A pure function;
 * hosts probe for this symbol to learn that models of 264 and 23 inputs are taken (an addition within version 5). */
int32_t    wsa_level_feature_count(int32_t output_level);
wsa_status wsa_model_create(wsa_ctx *ctx, const wsa_model_desc *d, wsa_model **out);    /* copies the weights to the context's device */
void       wsa_model_destroy(wsa_model *m);
/* prob[r][c] (f32, [n_rows][units[n_layers]]) of dense device rows feat[r][units[0]] (double): normalised as ml5's normalizeValue
 * ((x - min) / (max - min) in double, no clamping), rounded to f32, then the network.  Device pointers; asynchronous on `stream`. */
wsa_status wsa_classify_rows(const wsa_model *m, const double *d_feat, uint32_t n_rows, float *d_prob, void *stream);
/* After a run at output_level 5 or 13: the probabilities of every row of the batch and, at level 13 (softmax models only), the
 * fold per callback and per clip.  WSA_ERR_INVALID at any other level, for a model of another context, and for a fold requested
 * from a model without a softmax output.
 * ML at levels 11 and 12 (per-row outputs only, no fold and no per-clip sums, as at level 5):
 *   level 11 with a 264-input model: the rows are the utterance table (wsa_device_result d_utt_feat, n_utterance_rows rows in its
 *            order); wsa_class_result.n_rows is that count.  The app stores a file's LAST utterance row (ref src/index.js:42 stores
 *            under part 0, every callback overwriting the one before): row d_clip_utt_off[clip + 1] - 1 of a clip that has any.
 *   level 12 with a 23-input model: the rows are the row table, read at its stride of WSA_NFEAT, slots 0 .. 22.  A row whose slot 23
 *            marks a thrown uncmin gets NaN in every output (written by the epilogue: deterministic, and unusable).
 * Every other pairing of the batch's level and the model's input count is refused with a message that names both.  Ensembles and
 * streams take 53-input models only. */
wsa_status wsa_batch_classify(wsa_batch *b, const wsa_model *m, void *stream);
/* Synchronises `stream` and hands out the last classification (device pointers valid until the next wsa_batch_classify with a
 * model of more classes or wsa_batch_destroy):
 *   d_prob      [n_rows][n_classes] f32, rows in the order of wsa_device_result's tables
 *   d_cb        [n_callbacks][4] = {clip, si, first row, rows} — one entry per level-13 callback (a run of rows with the same clip, si)
 *   d_cb_label  [n_callbacks] class index of the callback's label; -1 = the reference's `null` (no sum above 0); -2 = no prediction
 *               at all (the callback's durations sum to 0: the reference skips the model and callback_after_pred)
 *   d_cb_conf   [n_callbacks] f64 confidence: max label sum / sum of the durations (ref prediction.js:168)
 *   d_clip_conf [n_clips][n_classes] f64: Label_conf_all of each clip (reset per launch, ref src/index.js:395), 0 for labels never added
 * Level 5: n_callbacks = 0 and no clip sums (d_cb* / d_clip_conf NULL). */
typedef struct {
    uint32_t n_rows, n_classes, n_callbacks, n_clips;
    const float *d_prob; const int32_t *d_cb; const int32_t *d_cb_label;
    const double *d_cb_conf; const double *d_clip_conf;
} wsa_class_result;
wsa_status wsa_batch_class_result(wsa_batch *b, void *stream, wsa_class_result *out);
/* The same tables copied to host buffers (any pointer may be NULL to skip it), for hosts without a HIP binding: prob [rows_cap][n_classes],
 * cb [cb_cap][4], cb_label / cb_conf [cb_cap], clip_conf [n_clips][n_classes] (level 13 only).  WSA_ERR_INVALID if a capacity is too small. */
wsa_status wsa_batch_copy_classes(wsa_batch *b, void *stream, float *prob, uint32_t rows_cap, int32_t *cb, int32_t *cb_label, double *cb_conf,
                                  uint32_t cb_cap, double *clip_conf);

/*
 * ---- Ensembles: every model DB of the application in one pass (additions within version 5: probe for wsa_ensemble_create).
 * The reference application does not predict with one model: predict_by_multiple_syllables runs the model of every DB in
 * `available_DBs` over a callback's syllables (ref src/prediction.js:12, 60-63) and folds each DB's confidences separately
 * (Label_conf_all[db], Label_conf_seg[db]).  seg_confidence_sort (ref prediction.js:127-169) then reports the label of the DB with
 * the largest segment sum and keeps `min_entropy_db`, the DB whose launch-long accumulator is the most decided; that DB's meters
 * and "Entropy" readout are what the user sees (plot_prediction_meters, ref prediction.js:172-215).  An ensemble is that list of
 * DBs.  K6e classifies with all members in one launch over (member, tile) pairs — a member's probabilities are bit for bit those of
 * wsa_classify_rows with that model — K6b-e folds with one wave per (clip, member) and decides in the same kernel, and one compaction
 * writes every table, so an ensemble costs three launches whatever its size (DESIGN.md "K6e").
 *
 * One difference from the reference, on purpose: it never resets `min_entropy_db` itself — reset_predictions(true) resets only
 * max_inv_entropy (ref prediction.js:35) — so a launch in which no accumulator exceeds 0 keeps showing the previous launch's DB.
 * The device knows one launch at a time and reports -1 for such a clip or stream; a host that wants the reference's behaviour
 * carries the last non-negative value across launches, in the order it dispatched them (the N-API layer's job).
 */
#define WSA_ENSEMBLE_MAX 8
typedef struct wsa_ensemble wsa_ensemble;
/* Members in the order of `available_DBs`: every tie between DBs goes to the earlier member (the strict > of ref prediction.js:156,
 * 161).  n = 1 .. WSA_ENSEMBLE_MAX; the same model may be two members.  WSA_ERR_INVALID: n out of range, a NULL member, a member of
 * another context.  The models must outlive the ensemble; destroy it before its context. */
wsa_status wsa_ensemble_create(wsa_ctx *ctx, const wsa_model *const *models, uint32_t n, wsa_ensemble **out);
void       wsa_ensemble_destroy(wsa_ensemble *e);
/* As wsa_batch_classify, with every member: level 13 gives probabilities, per-member folds and the decision (every member must
 * end in softmax, else WSA_ERR_INVALID), level 5 per-member probabilities only, any other level WSA_ERR_INVALID.  Enqueued on
 * `stream`; after the first call with an ensemble on a batch nothing is allocated, so wsa_batch_run + wsa_batch_classify_ensemble
 * can be captured into a hipGraph.  The ensemble must outlive the batch's use of its tables. */
wsa_status wsa_batch_classify_ensemble(wsa_batch *b, const wsa_ensemble *e, void *stream);
/* Synchronises `stream` and hands out the last ensemble classification (device pointers, valid until the next
 * wsa_batch_classify_ensemble with another ensemble or wsa_batch_destroy).  Per member d < n_members:
 *   d_prob[d]       [n_rows][n_classes[d]] f32
 *   d_cb_label[d], d_cb_conf[d] [n_callbacks]: what wsa_class_result gives for that model alone (-1 / -2 alike)
 *   d_cb_all_max[d] [n_callbacks] f64: DB_entropies_all[d] after that callback, the largest entry of the member's Label_conf_all (0 if none
 *                   exceeds 0; ref prediction.js:136-153)
 *   d_clip_conf[d]  [n_clips][n_classes[d]] f64: the member's Label_conf_all per clip
 * Across members:
 *   d_cb           [n_callbacks][4] = {clip, si, first row, rows}
 *   d_cb_db        [n_callbacks] the member whose label won the callback (the first whose segment maximum exceeds the running one, from 0);
 *                  -1 = no member has a segment sum above 0 (the reference's label `null`, confidence 0); -2 = skipped, as d_cb_label
 *   d_cb_top_label [n_callbacks] class index within that member's legend (-1 where d_cb_db < 0)
 *   d_cb_top_conf  [n_callbacks] f64 max_conf_db_seg / seg_weight (ref prediction.js:168)
 *   d_cb_min_db    [n_callbacks] min_entropy_db after that callback: updated only where a member's DB_entropies_all exceeds
 *                  max_inv_entropy, which runs across the clip's callbacks (ref prediction.js:161-165); -1 while none has exceeded 0.
 *                  Skipped callbacks leave it as it was.
 *   d_cb_entropy   [n_callbacks] f64 1 - DB_entropies_all[min_db] / all_class_sum, the sum over Label_conf_all[min_db] in Object.keys
 *                  order (ref prediction.js:182-184, 207); NaN while d_cb_min_db is -1
 *   d_clip_min_db  [n_clips] the clip's last callback's d_cb_min_db (-1 for a clip without one)
 * Level 5: n_callbacks = 0 and only d_prob is set.  Single-model and ensemble results of one batch are separate:
 * wsa_batch_class_result after an ensemble call returns WSA_ERR_INVALID, and the other way round. */
typedef struct {
    uint32_t n_rows, n_members, n_callbacks, n_clips;
    uint32_t n_classes[WSA_ENSEMBLE_MAX];
    const float   *d_prob[WSA_ENSEMBLE_MAX];
    const int32_t *d_cb_label[WSA_ENSEMBLE_MAX];
    const double  *d_cb_conf[WSA_ENSEMBLE_MAX];
    const double  *d_cb_all_max[WSA_ENSEMBLE_MAX];
    const double  *d_clip_conf[WSA_ENSEMBLE_MAX];
    const int32_t *d_cb; const int32_t *d_cb_db; const int32_t *d_cb_top_label; const double *d_cb_top_conf;
    const int32_t *d_cb_min_db; const double *d_cb_entropy; const int32_t *d_clip_min_db;
} wsa_ensemble_result;
wsa_status wsa_batch_ensemble_result(wsa_batch *b, void *stream, wsa_ensemble_result *out);
/* The same tables copied to host buffers (any pointer may be NULL to skip it): prob[d] [rows_cap][n_classes[d]], the per-callback
 * tables [cb_cap] (cb [cb_cap][4]), clip_conf[d] [n_clips][n_classes[d]], clip_min_db [n_clips].  WSA_ERR_INVALID if a capacity
 * is too small. */
typedef struct {
    uint32_t rows_cap, cb_cap;
    float   *prob[WSA_ENSEMBLE_MAX];
    int32_t *cb_label[WSA_ENSEMBLE_MAX];
    double  *cb_conf[WSA_ENSEMBLE_MAX];
    double  *cb_all_max[WSA_ENSEMBLE_MAX];
    double  *clip_conf[WSA_ENSEMBLE_MAX];
    int32_t *cb; int32_t *cb_db; int32_t *cb_top_label; double *cb_top_conf;
    int32_t *cb_min_db; double *cb_entropy; int32_t *clip_min_db;
} wsa_ensemble_host;
wsa_status wsa_batch_copy_ensemble(wsa_batch *b, void *stream, const wsa_ensemble_host *dst);

/*
 * ---- Classification inside the stream step (additions within version 5: probe for wsa_stream_set_model).
 * The app's live path (ref src/prediction.js:47: predict_by_multiple_syllables after every level-13 callback of a live source, the
 * per-launch Label_conf_all behind the meters) for every stream of a wsa_stream: K6 on each step's rows and, at level 13, the fold with
 * one accumulator per stream carried on the device from step to step.  Both are kernels of the step, so a step stays one graph launch
 * and its results arrive through the step's mapped pinned buffers.
 *   - One accumulator per stream (Label_conf_all and the order its labels were added in), reset by START — a START step's rows
 *     already belong to the new launch — untouched on idle steps, kept after STOP until the stream's next START.
 *   - STOP-flush rows and the rows of cut spans (WSA_FLAG_STREAM_CUT) are classified like any others.
 *   - wsa_stream_time_steps times the step with the classifier in it when one is attached.
 */
/* Attach (m != NULL) or detach (NULL) a classifier.  Levels 5 / 13 only; level 13 needs a softmax model; same context.
 * Synchronises the last step, (re)allocates the class tables, zeroes every stream's accumulator and drops the captured graph
 * (the next step recaptures with the classifier in it).  The model must outlive its attachment. */
wsa_status wsa_stream_set_model(wsa_stream *st, const wsa_model *m);
typedef struct {
    uint32_t n_rows, n_classes, n_callbacks, n_streams;
    const float   *prob;         /* [n_rows][n_classes], rows in wsa_stream_rows order */
    const int32_t *cb;           /* [n_callbacks][4] = {stream, si, first row, rows} (level 13; else 0 / NULL) */
    const int32_t *cb_label;     /* as wsa_class_result: -1 = null, -2 = no prediction */
    const double  *cb_conf;
    const double  *stream_conf;  /* [n_streams][n_classes] Label_conf_all since each stream's START (level 13), 0 for labels never added */
} wsa_stream_class_result;
/* After wsa_stream_collect of the same step: host memory owned by the stream object, valid until the next step.
 * WSA_ERR_INVALID without an attached model. */
wsa_status wsa_stream_classes(wsa_stream *st, wsa_stream_class_result *out);
/* The same with an ensemble (additions within version 5: probe for wsa_ensemble_create): K6e on each step's rows and, at level 13, one
 * accumulator per stream and member plus one running max_inv_entropy / min_entropy_db per stream (ref prediction.js:16-17), all carried
 * on the device, reset by START, untouched on idle steps and kept after STOP.  Three kernels of the step; the step stays one graph
 * launch.  Attach (e != NULL) or detach (NULL) as wsa_stream_set_model does; setting a model detaches an ensemble and vice versa. */
wsa_status wsa_stream_set_ensemble(wsa_stream *st, const wsa_ensemble *e);
typedef struct {
    uint32_t n_rows, n_members, n_callbacks, n_streams;
    uint32_t n_classes[WSA_ENSEMBLE_MAX];
    const float   *prob[WSA_ENSEMBLE_MAX];         /* [n_rows][n_classes[d]] */
    const int32_t *cb_label[WSA_ENSEMBLE_MAX];     /* the tables of wsa_ensemble_result for the step's callbacks (level 13; else NULL) */
    const double  *cb_conf[WSA_ENSEMBLE_MAX];
    const double  *cb_all_max[WSA_ENSEMBLE_MAX];
    const double  *stream_conf[WSA_ENSEMBLE_MAX];  /* [n_streams][n_classes[d]] the member's Label_conf_all since each stream's START */
    const int32_t *cb;                             /* [n_callbacks][4] = {stream, si, first row, rows} */
    const int32_t *cb_db; const int32_t *cb_top_label; const double *cb_top_conf;
    const int32_t *cb_min_db; const double *cb_entropy;
    const int32_t *stream_min_db;                  /* [n_streams] min_entropy_db since each stream's START (-1: none yet) */
} wsa_stream_ensemble_result;
/* After wsa_stream_collect of the same step: host memory owned by the stream object, valid until the next step.
 * WSA_ERR_INVALID without an attached ensemble. */
wsa_status wsa_stream_ensemble_classes(wsa_stream *st, wsa_stream_ensemble_result *out);

/*
 * ---- Streams of different rates, converted inside the step (additions within version 5: probe for wsa_stream_create_mixed).
 * Stream i arrives at fs_in[i] and is analysed at fs_out: the conversion RS-1 (wsa_batch_create_resampled above) runs as a
 * kernel of the step (K0s) with per-stream state carried on the device, so that a stream fed a signal in pieces gives exactly the rows
 * wsa_batch_create_mixed gives for the whole signal.  This has no counterpart in the reference: its live path (ref dist/main.js:2 @B8752)
 * runs at whatever rate the audio hardware has and converts nothing; only its offline path sees converted samples, because the browser
 * decodes every file into the 48 kHz context (@B18769).  Like `resample_to` for batches it is ours: it lets a live 44.1 kHz or 16 kHz
 * source be analysed with the geometry — and the classifier of wsa_stream_set_model be fed the features — of the 48 kHz files the shipped
 * models were trained on, and lets sources of different rates share one lock-step set.
 *
 * Per stream, counted since its last START: N input samples received, Y converted samples handed to the front end, K frames analysed;
 * ratio = fs_in[i] / fs_out in double, exactly as K0 forms it.
 *   - Output n is READY when every tap RS-1 reads for it has arrived: floor((double)n * ratio) + 16 <= N (taps before sample 0 are RS-1's
 *     zeros).  Its value is the one the batch computes (position from the absolute index n, same table, same order of operations), so
 *     nothing is ever revised.  A step hands on all ready outputs, never more than wsa_resample_length(N, ...): wsa_resample_ready.
 *   - STOP, after the step's samples are counted: the outputs up to wsa_resample_length(N, ...) are produced with zeros for the taps at or
 *     beyond N (as a batch pads a clip's end), the frames they complete are analysed, then segment_truncate as for any stream.
 *   - fs_in[i] == fs_out: the stream is copied, not filtered, and has no look-ahead (the rule of wsa_batch_create_mixed).  A set whose
 *     streams all sit at fs_out, fed frames_per_step * hop samples per step, gives the rows of a wsa_stream_create set in the same steps.
 *   - Frame k is y[k * hop, k * hop + win) of the converted signal and is analysed in the step in which Y reaches k * hop + win — the
 *     batch's frames.  A step analyses ALL frames that became complete; there is no backlog.
 *   - A step accepts n_in[i] <= wsa_stream_input_capacity(st, i) = ceil(frames_per_step * hop * ratio) samples of stream i (more:
 *     WSA_ERR_INVALID naming the stream); 0 on an active stream is legal.  A host that sends the capacity every step completes
 *     frames_per_step + 1 frames in a step now and then, and a STOP step adds the tail (about 16 / ratio outputs); the step's internal
 *     frame capacity is derived from that (wsa_stream_frames_bound), not from frames_per_step.
 *   - n_in == NULL: PACED input, every active stream delivers what keeps it on real time, floor((s + 1) * F * hop * ratio) -
 *     floor(s * F * hop * ratio) samples in its s-th active step since START (1102 / 1103 alternating at 44.1 -> 48 kHz, 25 ms steps);
 *     wsa_stream_paced_input tells the next count.  Paced streams never exceed frames_per_step frames per step.
 *   - START resets N, Y, K, the input history and the carried converted samples; idle streams keep everything; after STOP a stream needs
 *     START.  Control bytes, cuts (WSA_FLAG_STREAM_CUT), rows and wsa_stream_collect are those of any stream set.
 *   - Rates: each positive and within a factor 16 of fs_out, else WSA_ERR_INVALID naming the stream; any number of distinct rates.
 * The host decides every count (N, Y, K, the step's outputs, the carried samples, the frames): integer bookkeeping and the one predicate
 * above, written into the step's mapped control words.  The device never decides how many outputs exist, and the captured graph is
 * replayed unchanged whatever the counts are.  wsa_stream_step / wsa_stream_step_host on a mixed set are the _n forms with n_in == NULL;
 * the _n forms on a plain set accept NULL or exactly samples_per_step for every active stream.  wsa_stream_samples_per_step is
 * frames_per_step * hop (samples at fs_out); wsa_stream_host_input is [n_streams][wsa_stream_input_stride] floats, stream i's samples of
 * the step at the start of its row; wsa_stream_time_steps takes feed blocks of that shape and steps paced.  wsa_stream_set_model and every
 * output level streams serve work unchanged.
 */
wsa_status wsa_stream_create_mixed(wsa_ctx *ctx, uint32_t n_streams, const double *fs_in, double fs_out, uint32_t frames_per_step,
                                   uint32_t max_span_frames, wsa_stream **out);
uint32_t   wsa_stream_input_capacity(const wsa_stream *st, uint32_t stream);   /* samples one step accepts (a plain set: samples_per_step) */
uint32_t   wsa_stream_input_stride(const wsa_stream *st);                      /* floats per stream in the pinned input buffer */
uint32_t   wsa_stream_paced_input(const wsa_stream *st, uint32_t stream);      /* what n_in == NULL takes in the next step (without a START in it) */
uint32_t   wsa_stream_step_frame_capacity(const wsa_stream *st);               /* frames per stream the step is sized for (a plain set: frames_per_step) */
/* stream i's n_in[i] samples at d_pcm + i * stream_stride (stream_stride >= the largest count of the step) */
wsa_status wsa_stream_step_n(wsa_stream *st, const float *d_pcm, uint64_t stream_stride, const uint32_t *n_in, const uint8_t *ctl, void *stream);
wsa_status wsa_stream_step_host_n(wsa_stream *st, const uint32_t *n_in, const uint8_t *ctl, void *stream);
/* pure: the outputs of the first n_in samples that are ready (the rule above, clamp included; n_in at equal rates) */
uint64_t   wsa_resample_ready(uint64_t n_in, double fs_in, double fs_out);
/* pure: the frames one step can complete at most, for frames_per_step, the hop in samples at fs_out and the smallest fs_in / fs_out of the
 * set's converted streams (0: every stream at fs_out): ceil((frames_per_step * hop + ceil(16 / min_ratio) + 3) / hop) */
uint32_t   wsa_stream_frames_bound(uint32_t frames_per_step, uint32_t hop, double min_ratio);
/* after wsa_stream_collect: the converted samples the last step produced (the copied ones of a stream at fs_out), out [n_streams][cap]
 * floats, counts [n_streams]; either may be NULL.  WSA_ERR_INVALID if a stream produced more than cap. */
wsa_status wsa_stream_copy_converted(wsa_stream *st, float *out, uint32_t cap, uint32_t *counts);

/*
 * ---- Training (additions within version 5: probe for wsa_trainer_create).
 * Stands in for the other half of the reference APPLICATION's "ML" panel: src/neuralmodel.js:163-403 (train_nn) hands the stored
 * level-13 rows to ml5.neuralNetwork(...).train({epochs, batchSize}).  In dist/ml5.min.js (ml5 0.6.0 on tfjs 1.7.2, byte offsets):
 * `compile` @2770937 (task classification: categoricalCrossentropy, tf.train.sgd(learningRate), metrics ["accuracy"]),
 * `trainInternal` @2768349 ({epochs: 10, batchSize: 32, validationSplit: .1}; model.fit @2755107 shuffles per epoch),
 * `normalizeValue` @2469274, `createOneHotEncodings` @2745375.  One run is the deterministic function TR-1 of DESIGN.md: the SGD
 * arithmetic is pinned to tfjs by tests/golden/train_expected.json; the initial weights and the order of the training rows in every
 * epoch are the caller's (the reference draws both from Math.random).  K7 (csrc/train.hip, csrc/train_stages.hpp) is reproducible bit for bit.
 * Classification only: the regression models (ords_*: mean squared error, Adam) are not trained.
 * A trainer belongs to the context it was created on; destroy it before that context.
 */
typedef struct wsa_trainer wsa_trainer;
typedef struct { uint32_t epochs_done; double loss, acc, val_loss, val_acc; } wsa_train_stats;   /* of the last finished epoch; val_* are 0 when n_val is 0 */
/* init: the stack with its INITIAL kernels / biases, in_min / in_max the ranges to normalise with, labels the legend (or NULL).
 * feat: host [n_rows][units[0]] double (dense rows of the model's input count: 53, 264 or 23); label: host [n_rows] class index; the last n_val rows are validation and never trained on.
 * A batch_size above the number of training rows is one step over all of them.  WSA_ERR_INVALID with a message: a last layer that
 * is not softmax, a label outside 0 .. classes - 1, n_val >= n_rows, batch_size 0, a learning rate that is not finite as an f32, and a
 * feature with in_max == in_min (ml5 would train on NaN inputs; refused instead, naming the feature). */
wsa_status wsa_trainer_create(wsa_ctx *ctx, const wsa_model_desc *init, const double *feat, const int32_t *label, uint32_t n_rows,
                              uint32_t n_val, uint32_t batch_size, double learning_rate, wsa_trainer **out);
/* One epoch: ceil(n_train / batch_size) SGD steps over the training rows taken in `order` (host [n_rows - n_val], every entry in
 * 0 .. n_train - 1, checked before anything is enqueued; NULL = 0, 1, 2, ...), then one forward pass over the validation rows.
 * Only enqueues on `stream`; allocates nothing.  A trainer has one set of buffers: every call on it (epoch, stats, copy_weights,
 * model) must pass the SAME stream, whose order is what serialises the epochs. */
wsa_status wsa_trainer_epoch(wsa_trainer *t, const uint32_t *order, void *stream);
wsa_status wsa_trainer_stats(wsa_trainer *t, void *stream, wsa_train_stats *out);                            /* synchronises `stream` */
/* the current weights, unpadded, in the tfjs layout of wsa_model_desc (kernel[l] [units[l]][units[l+1]], bias[l] [units[l+1]]); synchronises */
wsa_status wsa_trainer_copy_weights(wsa_trainer *t, void *stream, float *const *kernel, float *const *bias);
/* a snapshot of the current weights as a model every wsa_*classify* entry point takes (the caller destroys it); synchronises */
wsa_status wsa_trainer_model(wsa_trainer *t, void *stream, wsa_model **out);
void       wsa_trainer_destroy(wsa_trainer *t);

/*
 * ---- Regression models (additions within version 5: probe for wsa_regress_trainer_create).
 * The app's other kind of model, dist/nnmodel/<db>/ords_<label>/ for the ordinal labels V, A and D: ref src/neuralmodel.js:268-333
 * (train_nn, ordinal branch) with nn_default_options_ords (src/neuralmodel_aux.js:127-150: task "regression", 64 sigmoid / 16 sigmoid /
 * 1 sigmoid, learningRate 0.2).  In dist/ml5.min.js `compile` @2770937 gives a regression task meanSquaredError,
 * tf.train.adam(learningRate) (tfjs 1.7.2 AdamOptimizer.applyGradients @548581) and ["accuracy"], which tfjs resolves to binaryAccuracy
 * for a one-unit output; ml5 normalises the output `y` to (y - min) / (max - min) (normalizeData) and un-normalises every prediction,
 * t * (max - min) + min (unnormalizeValue @2469277), with model_meta.json's outputs.y.{min,max}.  One run is the deterministic function
 * TR-2 of DESIGN.md, pinned to tfjs by tests/golden/regress_expected.json.
 * A regression model is an ordinary wsa_model whose last layer has ONE unit and is linear, relu, sigmoid or tanh; wsa_model_desc is
 * unchanged and the output range travels as arguments.  Every entry refuses (WSA_ERR_INVALID with a message) more than one output
 * unit, a softmax last layer, non-finite out_min / out_max and out_max == out_min.
 * One value per callback and a running value per clip or stream, and regression models on streams: specification RG-1 of DESIGN.md,
 * "Regression groups" below (wsa_regress_group_create).
 */
/* K6 with the un-normalising epilogue on device rows (ref src/neuralmodel.js:540-585 predict_single -> predictMultiple; :410-535
 * predict_db_nn -> result_out[0].value): dense d_feat [n_rows][units[0]] f64 -> d_value [n_rows] f64 = (double)p * (out_max - out_min) +
 * out_min, p the f32 output of the one unit, the product and the sum rounded separately.  Asynchronous on `stream`; allocates nothing. */
wsa_status wsa_regress_rows(const wsa_model *m, double out_min, double out_max,
                            const double *d_feat, uint32_t n_rows, double *d_value, void *stream);
/* The same on the rows of the batch's last run: levels 5 and 13 (and 11 with a 264-input model, 12 with a 23-input model: the rows
 * and the NaN rule of wsa_batch_classify); one value per row in the order of wsa_device_result's tables, equal bit
 * for bit to wsa_regress_rows over d_feat.  Only enqueues; after the first call on a batch nothing is allocated.  Also refuses a model
 * of another context.  A batch keeps ONE last model call: after this one wsa_batch_class_result is refused, and the other way round. */
wsa_status wsa_batch_regress(wsa_batch *b, const wsa_model *m, double out_min, double out_max, void *stream);
/* Synchronises `stream`; *n_rows (may be NULL) = the rows of the last run, value (may be NULL) [rows_cap] their values.
 * WSA_ERR_INVALID if rows_cap is too small or the batch's last model call was not wsa_batch_regress. */
wsa_status wsa_batch_copy_values(wsa_batch *b, void *stream, double *value, uint32_t rows_cap, uint32_t *n_rows);
/* wsa_trainer_create for a regression model (ref src/neuralmodel.js:268-333 -> ml5 neuralNetwork.train, task "regression"):
 * target: host [n_rows] double, the label's values; out_min / out_max the range they are normalised with.  Returns the same
 * wsa_trainer: wsa_trainer_epoch, _stats (loss = mean squared error of the normalised output; acc = tfjs's binaryAccuracy, the app
 * prints both), _copy_weights, _model (a model for wsa_regress_rows / wsa_batch_regress) and _destroy work on it unchanged.  Adam's
 * two moments and accumulated betas live on the device for the life of the trainer and are carried from epoch to epoch; an epoch is
 * still only enqueued.  Refuses, beside the above and everything wsa_trainer_create refuses but the softmax rule and the labels: a
 * target that is not finite, or whose normalised value is not finite as an f32. */
wsa_status wsa_regress_trainer_create(wsa_ctx *ctx, const wsa_model_desc *init, const double *feat,
                                      const double *target, uint32_t n_rows, uint32_t n_val, uint32_t batch_size,
                                      double learning_rate, double out_min, double out_max, wsa_trainer **out);

/*
 * ---- Training groups (additions within version 5: probe for wsa_train_group_create).
 * At the app's settings (ml5's batch of 32) an epoch of one trainer is bound by its launches, not by arithmetic, and the app needs one
 * model per DB and head (setPredictionModels / setPredictionValues: available_DBs x {cats_emotion, ords_V, ords_A, ords_D}).  A group
 * steps up to WSA_TRAIN_GROUP_MAX trainers in lock step: every launch covers the same stage of every member that has that stage in this
 * step (K7g, csrc/train_group.hip), so N models train in about the wall time of the longest one.  Specification TG-1 of DESIGN.md: a group
 * epoch IS wsa_trainer_epoch on every member, in any order, bit for bit (weights, Adam's moments, wsa_train_stats).
 * The group adopts existing trainers, classification and regression alike, of any stack, width (53 / 264 / 23), row count, batch size,
 * n_val and learning rate; it owns only a descriptor table.  wsa_trainer_stats / _copy_weights / _model keep working on a member, and
 * wsa_trainer_epoch on a member between group epochs is legal on the same stream (it is that member's next solo epoch).  Every call on
 * a group and on its members passes the SAME stream.  Destroy a group BEFORE any of its members; wsa_train_group_destroy releases
 * the members, which live on as solo trainers and may join another group.  (A member destroyed first empties the group: the other members are
 * released and wsa_train_group_epoch refuses from then on; the group itself is still to be destroyed.)
 */
#define WSA_TRAIN_GROUP_MAX 32
typedef struct wsa_train_group wsa_train_group;
/* WSA_ERR_INVALID with a message that names the member index: n of 0 or above WSA_TRAIN_GROUP_MAX, a NULL member, a member of another
 * context, the same trainer given twice, a trainer already in a living group. */
wsa_status wsa_train_group_create(wsa_ctx *ctx, wsa_trainer *const *members, uint32_t n, wsa_train_group **out);
void       wsa_train_group_destroy(wsa_train_group *g);             /* releases the members; they live on as solo trainers */
/* One epoch of every member: orders[m] as wsa_trainer_epoch's `order` of member m (host [n_train of m], or NULL = 0, 1, 2, ...);
 * orders itself may be NULL.  Every member's order is checked before anything is enqueued (the message names member and index) and is
 * staged through that member's own pinned buffers.  A member whose epoch has fewer steps drops out of the later launches; after the
 * longest member's last step comes one validation pass for the members with n_val > 0, then one finish.  Only enqueues; allocates nothing. */
wsa_status wsa_train_group_epoch(wsa_train_group *g, const uint32_t *const *orders, void *stream);
wsa_status wsa_train_group_stats(wsa_train_group *g, void *stream, wsa_train_stats *out /* [n] */);  /* one synchronisation for all members */
/* host arithmetic only: the kernel launches of one group epoch, TG-1's formula over the members' (nl, n_train, batch, n_val) */
wsa_status wsa_train_group_launches(const wsa_train_group *g, uint32_t *per_epoch);
/* pure, needs no device: the same formula over n (1 .. WSA_TRAIN_GROUP_MAX) shapes given as arrays; nl 1 .. 8, n_train and batch >= 1
 * (a batch above n_train is one step), else WSA_ERR_INVALID */
wsa_status wsa_train_group_launch_count(const uint32_t *nl, const uint32_t *n_train, const uint32_t *batch, const uint32_t *n_val,
                                        uint32_t n, uint64_t *per_epoch);

/*
 * ---- Predicting a labelled feature DB and the app's results table (additions within version 5: probe for wsa_dbstats_create).
 * Stands in for the reference APPLICATION's "Predict" button and the panel it fills: src/neuralmodel.js:410-535 (start_nn_prediction ->
 * predict_db_nn -> nn_db_results_handler) runs a model over EVERY stored row of a DB, update_pred_label (src/localstore.js:723-769)
 * writes each row's prediction into the row's `pred` pair, and shows_stats_table (src/localstore.js:498-627) counts, per categorical
 * head, correct / wrong / blank rows and per class count, duration, correct and wrong, and per ordinal head the range, the samples, the
 * predicted rows and the squared error.  Specification DS-1 and kernels K8 of DESIGN.md (csrc/dbstats.hip).
 * A wsa_dbstats object holds one DB on the context's device: its feature rows, one duration per row (parseFloat(time[1]),
 * localstore.js:534) and, per head, a true column and a predicted column.  The HOST resolves everything that is a string: it builds each
 * categorical head's vocabulary (the head's counted true labels and the model's legend labels) and applies the class-list / '*' rule of
 * localstore.js:523; the device sees indices.  The DEVICE applies the numeric rules: the decision over a row's probabilities
 * (neuralmodel.js nn_db_results_handler: the first entry of ml5's stably sorted result whose confidence is > a maximum that starts at 0)
 * and "truthy and not NaN" for ordinal values (v == v && v != 0; localstore.js:587, 593), so that a predicted 0 is dropped where it is made.
 * Every f64 sum of the table is "rows of a chunk of WSA_DBSTATS_CHUNK_ROWS consecutive rows in row order, then chunks in chunk order",
 * whatever the grid: a run is reproducible bit for bit and a CPU restatement gives the same bits.  No floating-point atomics.
 * A DB object belongs to the context it was created on; destroy it before that context.  One set of buffers: pass the SAME stream to
 * every call on it.
 */
#define WSA_DBSTATS_MAX_CLASSES 256   /* vocabulary entries of one categorical head */
#define WSA_DBSTATS_MAX_HEADS   8     /* heads of each kind */
#define WSA_DBSTATS_CHUNK_ROWS  256   /* R of DS-1 */
typedef struct wsa_dbstats wsa_dbstats;
/* predicted_states of one categorical head (ref localstore.js:517, 541-552) */
typedef struct { uint64_t correct, wrong, blank; } wsa_dbstats_cat;
/* one vocabulary entry (ref localstore.js:525-548: label_class_samples / _duration / _correct / _wrong); first_row = the smallest counted
 * row with this true class, UINT32_MAX if none: label_unique_value lists the classes in ascending first_row */
typedef struct { uint64_t count, correct, wrong; double duration; uint32_t first_row, reserved; } wsa_dbstats_class;
/* one ordinal head (ref localstore.js:584-598): min starts at +Infinity, max at 0, sq_sum = sum of (pred - true)^2, d * d in double */
typedef struct { uint64_t true_n, pred_n; double min, max, sq_sum; } wsa_dbstats_ord;
/* feat: host [n_rows][n_feat] double (NULL: a DB that is only counted, never predicted); duration: host [n_rows] double;
 * vocab: host [n_cat] vocabulary sizes.  Every true column starts as "does not count" and every predicted column as blank / missing.
 * WSA_ERR_INVALID with a message: n_rows 0, more than WSA_DBSTATS_MAX_HEADS heads of a kind, no head at all, a vocabulary of 0 or of more
 * than WSA_DBSTATS_MAX_CLASSES entries (naming the head). */
wsa_status wsa_dbstats_create(wsa_ctx *ctx, const double *feat, const double *duration, uint32_t n_rows,
                              uint32_t n_cat, const uint32_t *vocab, uint32_t n_ord, wsa_dbstats **out);          /* n_feat = WSA_NFEAT */
/* The same for a DB of rows of n_feat features: 53 (levels 5 and 13), 264 (level 11) or 23 (level 12), any other width is refused.
 * wsa_dbstats_predict_classes / _predict_values refuse a model whose input count is not the DB's width (an addition within
 * version 5: probe for wsa_level_feature_count). */
wsa_status wsa_wide_dbstats_create(wsa_ctx *ctx, const double *feat, uint32_t n_feat, const double *duration, uint32_t n_rows,
                                   uint32_t n_cat, const uint32_t *vocab, uint32_t n_ord, wsa_dbstats **out);
void       wsa_dbstats_destroy(wsa_dbstats *db);
/* host [n_rows] columns of categorical head `head`: true_idx -1 = the row does not count (no true pair, a falsy label, a label outside
 * the class list: localstore.js:523), pred_idx (NULL: all blank) -1 = blank (localstore.js:537).  An index outside -1 .. V - 1 is refused
 * naming the row.  Synchronous. */
wsa_status wsa_dbstats_set_classes(wsa_dbstats *db, uint32_t head, const int32_t *true_idx, const int32_t *pred_idx);
/* host [n_rows] columns of ordinal head `head`; NaN = missing; pred_value may be NULL (all missing).  The device drops 0 and NaN. */
wsa_status wsa_dbstats_set_values(wsa_dbstats *db, uint32_t head, const double *true_value, const double *pred_value);
/* predict_db_nn with a cats model (ref neuralmodel.js:410-535): wsa_classify_rows over all rows, then K8's decision per row into the
 * head's predicted column: legend_to_vocab[c] (host [classes of m], each -1 .. V - 1) of the first class c in legend order with the
 * largest probability, -1 (the reference's null) when no probability is > 0.  A NaN probability never wins (not pinned against the
 * reference).  Only enqueues; after the first call nothing is allocated.  WSA_ERR_INVALID: a regression model (one unit without
 * softmax), a model of another context, a DB without feature rows, a model whose input count is not the DB's width. */
wsa_status wsa_dbstats_predict_classes(wsa_dbstats *db, uint32_t head, const wsa_model *m, const int32_t *legend_to_vocab, void *stream);
/* the decision alone, on the caller's device table d_prob [n_rows][n_classes] f32, n_classes 1 .. 64 */
wsa_status wsa_dbstats_decide_rows(wsa_dbstats *db, uint32_t head, const float *d_prob, uint32_t n_classes, const int32_t *legend_to_vocab, void *stream);
/* predict_db_nn with an ords model (result_out[0].value): wsa_regress_rows into the head's predicted column.  Only enqueues; allocates
 * nothing.  WSA_ERR_INVALID: everything wsa_regress_rows refuses (a classifier among it), a model of another context, no feature rows. */
wsa_status wsa_dbstats_predict_values(wsa_dbstats *db, uint32_t head, const wsa_model *m, double out_min, double out_max, void *stream);
/* shows_stats_table's numbers: enqueues the two passes over all heads at once, synchronises `stream` and copies out cat [n_cat],
 * cls [sum of the vocabulary sizes] (head 0's entries first) and ord [n_ord]; a pointer may be NULL to skip it. */
wsa_status wsa_dbstats_table(wsa_dbstats *db, void *stream, wsa_dbstats_cat *cat, wsa_dbstats_class *cls, wsa_dbstats_ord *ord);
/* a head's predicted column, for the host to write the `pred` pairs back (update_pred_label); synchronises `stream` */
wsa_status wsa_dbstats_copy_classes(wsa_dbstats *db, uint32_t head, void *stream, int32_t *pred_idx);
wsa_status wsa_dbstats_copy_values(wsa_dbstats *db, uint32_t head, void *stream, double *pred_value);
/* the probabilities the last wsa_dbstats_predict_classes decided on, prob [n_rows][n_classes] f32 (n_classes must be that model's);
 * synchronises `stream`.  WSA_ERR_INVALID before the first prediction. */
wsa_status wsa_dbstats_copy_probs(wsa_dbstats *db, void *stream, float *prob, uint32_t n_classes);

/*
 * ---- KNN classifier (additions within version 5: probe for wsa_knn_create).
 * Stands in for the application's third learner, ref src/neuralmodel.js:729-837 (train_knn; its button handler is exported at
 * src/index.js:165-168): ml5.KNNClassifier() over a labelled feature DB — addExample(features, label) for the first 80 % of the rows,
 * classify(features, 10, ...) for the next 100.  In dist/ml5.min.js that is the tfjs knn-classifier (addExample, similarities,
 * predictClass, calculateTopClass, normalizeVectorToUnitLength): specification KN-1 of DESIGN.md §3, kernels K9 (csrc/knn.hip).
 * The classifier is deterministic, so every output is pinned: tests/golden/knn_expected.json holds what ml5 itself computes.
 * A store belongs to the context it was created on; destroy it before that context.  One set of buffers: pass the SAME stream to every
 * call on it (adds and classifications are ordered by that stream).
 * The device never sees label strings.  Class indices are in ml5's class-id order, which the HOST works out (webspeechanalyzer_amd/knn.py
 * label_order, js/knn.js labelOrder): ml5 gives a string label the index of its first appearance, and a number label is its own class id.
 */
#define WSA_KNN_MAX_K 64        /* one query's neighbour list fits the lanes of one wave */
typedef struct wsa_knn wsa_knn;
/* ref ml5.KNNClassifier() (neuralmodel.js:764).  width: the row width of an ML level (wsa_level_feature_count: 53, 264 or 23, anything
 * else is refused); n_classes 1 .. WSA_MODEL_MAX_CLASSES; capacity: the most rows the store will ever hold (allocated here). */
wsa_status wsa_knn_create(wsa_ctx *ctx, int32_t width, int32_t n_classes, uint32_t capacity, wsa_knn **out);
void       wsa_knn_destroy(wsa_knn *knn);
/* ref knnClassifier.addExample(features, label) (neuralmodel.js:777), n rows at once: d_feat device [n][width] f64 (dense), d_class device
 * [n] i32 class indices.  Each row is rounded to f32 and divided by its Euclidean norm in f32; rows are kept in insertion order and never
 * move; every row's grouped rank (rows of earlier classes + index within its own class) is recomputed.  Only enqueues; allocates nothing.
 * Adding after classifying is legal, as in ml5.  WSA_ERR_CAPACITY when the rows do not fit.  A class index outside 0 .. n_classes - 1 is
 * stored as class 0 and reported by the next wsa_knn_count. */
wsa_status wsa_knn_add(wsa_knn *knn, const double *d_feat, const int32_t *d_class, uint32_t n, void *stream);
/* ref knnClassifier.getCountByLabel(): synchronises `stream`; *n_rows = rows stored, class_rows [n_classes] = rows per class (either may be
 * NULL).  WSA_ERR_INVALID naming the row if an add carried a class index out of range. */
wsa_status wsa_knn_count(wsa_knn *knn, void *stream, uint32_t *n_rows, uint32_t *class_rows);
/* ref knnClassifier.classify(features, k, cb) (neuralmodel.js:811) for n_rows dense device rows d_feat [n_rows][width] f64; k 1 ..
 * WSA_KNN_MAX_K, k_eff = min(k, rows stored).  Any output may be NULL:
 *   d_label [n_rows] i32      the first class, in index order, with the most votes (ml5 calculateTopClass)
 *   d_conf  [n_rows][n_classes] f64   votes / k_eff
 *   d_nbr   [n_rows][k] i32   insertion indices of the k_eff neighbours in selection order (similarity descending, then grouped rank
 *                             ascending: ml5's stable top-k over its grouped train matrix); entries k_eff .. k - 1 are -1
 *   d_sim   [n_rows][k] f32   their similarities; entries k_eff .. k - 1 are NaN
 * Similarities are f32 with the device's own fixed summation order (a tolerance against tfjs, DESIGN.md "K9"); given them, everything
 * else is exact.  A NaN similarity (a zero or non-finite row: not pinned against ml5) is lower than every number, ranks decide among
 * NaNs, and it is written as NaN.  Only enqueues; allocates nothing.  WSA_ERR_INVALID: k out of range, an empty store. */
wsa_status wsa_knn_classify_rows(const wsa_knn *knn, const double *d_feat, uint32_t n_rows, uint32_t k, int32_t *d_label, double *d_conf,
                                 int32_t *d_nbr, float *d_sim, void *stream);
/* rows per tile of K9 (tests place their edge cases by these): the store is streamed train_rows rows at a time, a workgroup keeps
 * query_rows query rows resident */
wsa_status wsa_knn_tile_info(int32_t *train_rows, int32_t *query_rows);
/* The same over the rows of the batch's last run, the row count read on the device: levels 5 and 13 with a 53-wide store (the row table),
 * level 11 with a 264-wide store (the utterance table, in its order), level 12 with a 23-wide store (slots 0 .. 22 of the row table; a
 * row whose slot 23 marks a thrown uncmin gets label -1, NaN confidences and similarities and neighbours -1, as wsa_batch_classify gives it
 * NaN).  Every other pairing is refused with a message that names both.  Equal bit for bit to wsa_knn_classify_rows over the same rows.
 * After the first call on a batch (or the first with more classes or a larger k) nothing is allocated, so wsa_batch_run + wsa_batch_knn can
 * be captured into a hipGraph; a captured graph keeps the store's row count of the capture.  The KNN tables of a batch are separate from
 * its model calls' (wsa_batch_classify, _ensemble, _regress). */
wsa_status wsa_batch_knn(wsa_batch *b, const wsa_knn *knn, uint32_t k, void *stream);
/* device tables of the last wsa_batch_knn, laid out as wsa_knn_classify_rows' outputs; valid until the next wsa_batch_knn that allocates
 * or wsa_batch_destroy */
typedef struct {
    uint32_t n_rows, n_classes, k, k_eff;
    const int32_t *d_label; const double *d_conf; const int32_t *d_nbr; const float *d_sim;
} wsa_knn_result;
wsa_status wsa_batch_knn_result(wsa_batch *b, void *stream, wsa_knn_result *out);          /* synchronises `stream` */
/* the same tables copied to host buffers of rows_cap rows (any pointer may be NULL to skip it); WSA_ERR_INVALID if rows_cap is too small */
wsa_status wsa_batch_copy_knn(wsa_batch *b, void *stream, int32_t *label, double *conf, int32_t *nbr, float *sim, uint32_t rows_cap);

/*
 * ---- KNN on live streams and the per-callback fold of KNN results (additions within version 5: probe for wsa_stream_set_knn).
 * Kernels K9s (csrc/knn.hip) and the fold of specification KN-2 (csrc/knn_fold.hip).
 * K9s is K9 for few query rows: the store is cut into S slices of whole tiles, one workgroup per (query tile, slice) selects within its
 * slice and leaves a partial list in a scratch table, and one wave per query merges its S lists and runs K9's epilogue.  A similarity is
 * the same bits as K9's and the order (similarity descending, grouped rank ascending) is total, so the four tables equal
 * wsa_knn_classify_rows' bit for bit whatever S is.
 *   S, chosen when a store is attached, for a window of W query rows (a stream set's D2H window of at most 1024 rows) against a store of
 *   T tiles of 64 rows on a device of n_cu compute units: S = ceil(2 n_cu / ceil(W / 64)), so that (query tiles x S) gives every CU two
 *   workgroups; at most ceil(T / 4), so that no slice is shorter than four tiles; at most WSA_KNN_SPLIT_MAX_SLICES; and at most what
 *   keeps the scratch table, W x S x (12 k + 4) bytes, within WSA_KNN_SPLIT_SCRATCH_BYTES.  At least 1.
 * KN-2 is K6b's fold (wsa_class_result, ref src/prediction.js:86-123) fed, per row, the n_classes pairs (class index, votes / k_eff as the
 * f64 of d_conf) in classifyMultiple's order — confidence descending, ties in class-index order — with the class indices as the legend.
 * The reference application has no KNN path there: the definition is this project's.
 */
#define WSA_KNN_SPLIT_MAX_SLICES 256
#define WSA_KNN_SPLIT_SCRATCH_BYTES (64u << 20)
/* KN-2 over the tables of the batch's last wsa_batch_knn (output_level 13 only: WSA_ERR_INVALID otherwise, or before a wsa_batch_knn),
 * one accumulator per clip.  Only enqueues; after the first call on a batch nothing is allocated, so it can be captured behind
 * wsa_batch_run + wsa_batch_knn. */
wsa_status wsa_batch_knn_fold(wsa_batch *b, void *stream);
/* as wsa_class_result's callback tables: d_cb [n_callbacks][4] = {clip, si, first row, rows}, d_cb_label (-1 = null, -2 = no prediction),
 * d_cb_conf, d_clip_conf [n_clips][n_classes]; valid until the next wsa_batch_knn / wsa_batch_knn_fold that allocates */
typedef struct {
    uint32_t n_callbacks, n_classes, n_clips;
    const int32_t *d_cb; const int32_t *d_cb_label; const double *d_cb_conf; const double *d_clip_conf;
} wsa_knn_fold_result;
wsa_status wsa_batch_knn_fold_result(wsa_batch *b, void *stream, wsa_knn_fold_result *out);      /* synchronises `stream` */
/* the same tables copied to host buffers (any pointer may be NULL): cb [cb_cap][4], cb_label / cb_conf [cb_cap], clip_conf [n_clips][n_classes] */
wsa_status wsa_batch_copy_knn_fold(wsa_batch *b, void *stream, int32_t *cb, int32_t *cb_label, double *cb_conf, uint32_t cb_cap, double *clip_conf);
/* Attach (knn != NULL) or detach (NULL) a KNN store: K9s on every step's rows (partial + merge) and, at output_level 13, KN-2 with one
 * accumulator per stream carried on the device — reset by START, untouched on idle steps, kept after STOP — as kernels of the step, on
 * the step's own stream behind its other kernels; the step stays one graph launch.  Levels 5 and 13 with a 53-wide store only; refused
 * with a message: any other level or width (naming both), a store of another context, k outside 1 .. WSA_KNN_MAX_K, an empty store.
 * Synchronises the last step, allocates everything (tables, the K9s scratch, the accumulators, zeroed) and drops the captured graph.
 * The store's row count is the one at attach (a captured graph keeps it); attaching again picks up added rows.  The KNN tables are
 * separate from a model's or an ensemble's: attaching a store neither detaches nor is detached by wsa_stream_set_model /
 * wsa_stream_set_ensemble.  The store must outlive its attachment.  wsa_stream_time_steps times the step with these kernels in it. */
wsa_status wsa_stream_set_knn(wsa_stream *st, const wsa_knn *knn, uint32_t k);
typedef struct {
    uint32_t n_rows, n_classes, k, k_eff, n_callbacks, n_streams, slices;      /* slices: the S chosen at attach */
    const int32_t *label;        /* [n_rows], rows in wsa_stream_rows order; the four row tables as wsa_knn_classify_rows' outputs */
    const double  *conf;         /* [n_rows][n_classes] */
    const int32_t *nbr;          /* [n_rows][k] */
    const float   *sim;          /* [n_rows][k] */
    const int32_t *cb;           /* [n_callbacks][4] = {stream, si, first row, rows} (level 13; else 0 / NULL) */
    const int32_t *cb_label;     /* -1 = null, -2 = no prediction */
    const double  *cb_conf;
    const double  *stream_conf;  /* [n_streams][n_classes] KN-2's Label_conf_all since each stream's START (level 13) */
} wsa_stream_knn_result;
/* After wsa_stream_collect of the same step: host memory owned by the stream object, valid until the next step.
 * WSA_ERR_INVALID without an attached store. */
wsa_status wsa_stream_knn_classes(wsa_stream *st, wsa_stream_knn_result *out);

/*
 * ---- Regression groups: V, A and D per callback, in batches and streams (additions within version 5: probe for wsa_regress_group_create).
 * Specification RG-1 (csrc/regress_fold.hpp, regress_fold.hip).  The reference application wires this path up and breaks
 * it: `?type=ords&label=V` sets predict_type = "ords" (ref src/index.js:892-893), every level-13 callback then goes through
 * predict_by_multiple_syllables -> predictMultiple (ref src/prediction.js:47-123, src/neuralmodel.js:564-565), and the fold reads
 * result_out[ph].confidence, which a regression result does not have: every sum is NaN.  The definition is therefore this project's:
 * per head h, the rows' values v_h weighted as the app weights every per-syllable result, by w = sqrt(d), d = parseFloat(((len + 1) *
 * step_s).toFixed(3)) (ref src/prediction.js:93):  cb_value[h] = (sum v w) / (sum w) over the callback's rows whose v_h is finite, in
 * row order, each product and each sum rounded on its own; a callback whose durations sum to 0 is skipped (value NaN, weight 0); the
 * same terms in the same order, continued from callback to callback (skipped ones left out), are the running sums of the clip or the
 * stream.  A signal dealt over stream steps gives the bits of the whole signal in one batch.
 * A group is 1 .. WSA_REGRESS_GROUP_MAX heads: regression models (what wsa_regress_rows accepts) of 53 inputs on one context, each with
 * its output range; the same model may appear twice.  All heads run in ONE grouped K6 launch (the ensemble's kernel with the regression
 * epilogue); head h's values equal wsa_regress_rows with that model and range bit for bit.  The models must outlive the group.
 */
#define WSA_REGRESS_GROUP_MAX 8
typedef struct wsa_regress_group wsa_regress_group;
/* WSA_ERR_INVALID with a message: n outside 1 .. 8, a NULL member, a member of another context, a member that does not take 53 inputs,
 * and per member everything wsa_regress_rows refuses (a classifier, several output units, a bad range). */
wsa_status wsa_regress_group_create(wsa_ctx *ctx, const wsa_model *const *models, const double *out_min, const double *out_max,
                                    uint32_t n, wsa_regress_group **out);
void       wsa_regress_group_destroy(wsa_regress_group *g);
/* dense d_feat [n_rows][53] f64 -> d_value[h] [n_rows] f64 for every head h (d_value: a HOST array of n device pointers), one grouped
 * launch on `stream`.  The group keeps one launch table: a call waits (on the host) for the group's previous call to finish. */
wsa_status wsa_regress_group_rows(wsa_regress_group *g, const double *d_feat, uint32_t n_rows, double *const *d_value, void *stream);
/* The group over the rows of the batch's last run, and at output_level 13 the RG-1 fold behind it, one accumulator set per clip.
 * Output_level 5 and 13 only: every other level is refused by name.  Only enqueues; after the first call on a batch with a group
 * nothing is allocated, so it can be captured behind wsa_batch_run.  It is the batch's ONE last model call (beside wsa_batch_classify,
 * _classify_ensemble and _regress): their result functions are refused after it, and these after them. */
wsa_status wsa_batch_regress_group(wsa_batch *b, const wsa_regress_group *g, void *stream);
/* device tables of the last wsa_batch_regress_group, valid until the next one that allocates or wsa_batch_destroy.  Level 5: d_value
 * only, n_callbacks 0 and every other pointer NULL. */
typedef struct {
    uint32_t n_rows, n_heads, n_callbacks, n_clips;
    const double  *d_value[WSA_REGRESS_GROUP_MAX];        /* [n_rows] v_h, rows in wsa_device_result's order */
    const double  *d_cb_value[WSA_REGRESS_GROUP_MAX];     /* [n_callbacks] S_h / W_h; NaN: skipped callback, or no usable row */
    const double  *d_cb_weight[WSA_REGRESS_GROUP_MAX];    /* [n_callbacks] W_h */
    const double  *d_clip_sum[WSA_REGRESS_GROUP_MAX];     /* [n_clips] A_h */
    const double  *d_clip_weight[WSA_REGRESS_GROUP_MAX];  /* [n_clips] B_h */
    const double  *d_clip_value[WSA_REGRESS_GROUP_MAX];   /* [n_clips] A_h / B_h, NaN when B_h == 0 */
    const int32_t *d_cb;                                  /* [n_callbacks][4] = {clip, si, first row, rows}, as wsa_class_result's */
} wsa_value_result;
wsa_status wsa_batch_value_result(wsa_batch *b, void *stream, wsa_value_result *out);            /* synchronises `stream` */
/* the same tables copied to host buffers; any pointer may be NULL to skip it.  value: [rows_cap] each; cb [cb_cap][4], cb_value and
 * cb_weight [cb_cap] each; clip_* [n_clips] each.  WSA_ERR_INVALID if a capacity is too small for a table that is asked for. */
typedef struct {
    uint32_t rows_cap, cb_cap;
    double  *value[WSA_REGRESS_GROUP_MAX], *cb_value[WSA_REGRESS_GROUP_MAX], *cb_weight[WSA_REGRESS_GROUP_MAX];
    double  *clip_sum[WSA_REGRESS_GROUP_MAX], *clip_weight[WSA_REGRESS_GROUP_MAX], *clip_value[WSA_REGRESS_GROUP_MAX];
    int32_t *cb;
} wsa_value_host;
wsa_status wsa_batch_copy_value_fold(wsa_batch *b, void *stream, const wsa_value_host *dst);
/* Attach (g != NULL) or detach (NULL) a regression group: the grouped K6 on every step's rows and, at output_level 13, RG-1 with the
 * running sums of every (stream, head) carried on the device — reset by START (a START step's rows belong to the new launch), untouched
 * on idle steps, kept after STOP; STOP-flush rows and the rows of cut spans fold like any others — as kernels of the step, on the step's
 * own stream behind its other kernels; the step stays one graph launch.  Levels 5 and 13 only (refused by name otherwise), a group of
 * the streams' context.  Synchronises the last step, allocates everything (tables, the carried sums, zeroed) and drops the captured graph.
 * These tables are separate from a model's, an ensemble's and a KNN store's: attaching a group neither detaches any of those nor is
 * detached by them, and classes and V, A, D come out of the same step.  The group must outlive its attachment.
 * wsa_stream_time_steps times the step with these kernels in it. */
wsa_status wsa_stream_set_regress(wsa_stream *st, const wsa_regress_group *g);
typedef struct {
    uint32_t n_rows, n_heads, n_callbacks, n_streams;
    const double  *value[WSA_REGRESS_GROUP_MAX];          /* [n_rows], rows in wsa_stream_rows order */
    const int32_t *cb;                                    /* [n_callbacks][4] = {stream, si, first row, rows} (level 13; else 0 / NULL) */
    const double  *cb_value[WSA_REGRESS_GROUP_MAX];       /* [n_callbacks] */
    const double  *cb_weight[WSA_REGRESS_GROUP_MAX];      /* [n_callbacks] */
    const double  *stream_sum[WSA_REGRESS_GROUP_MAX];     /* [n_streams] A_h since each stream's START */
    const double  *stream_weight[WSA_REGRESS_GROUP_MAX];  /* [n_streams] B_h */
    const double  *stream_value[WSA_REGRESS_GROUP_MAX];   /* [n_streams] A_h / B_h, NaN when B_h == 0 */
} wsa_stream_value_result;
/* After wsa_stream_collect of the same step: host memory owned by the stream object, valid until the next step.
 * WSA_ERR_INVALID without an attached group. */
wsa_status wsa_stream_values(wsa_stream *st, wsa_stream_value_result *out);

/*
 * ---- Packed PCM into streams, unpacked on the GPU inside the step (additions within version 5: probe for wsa_stream_set_input_format).
 *
 * The stream counterpart of wsa_batch_run_host_i16: a live source hands over 16-bit PCM (often interleaved stereo) or 8-bit G.711, and
 * the host puts exactly those bytes into the stream set's pinned buffer — half or a quarter of the PCIe bytes of floats, no widening loop
 * on the CPU.  Spec PK-1: a packed sample becomes the float the float entry points would have been given, and nothing
 * else changes — a set fed packed input gives, step for step and byte for byte, what the same set gives when fed wsa_pcm_decode(packed)
 * through wsa_stream_step_host / wsa_stream_step (rows, segments, cuts, formants, utterance rows, raw tracks, wsa_stream_copy_converted,
 * every attached model's tables), eager or graph.
 *   - WSA_PCM_I16: (float)x / 32768, exact in fp32, as wsa_batch_run_host_i16 converts.  WSA_PCM_MULAW / WSA_PCM_ALAW: the 16-bit linear
 *     value of ITU-T G.711 (mu-law +-32124, A-law +-32256) / 32768, exact as well.
 *   - Stream i delivers frames interleaved over channels[i] channels (1 .. 64, as for batches); channel 0 is analysed: sample j is element
 *     j * channels[i] of the stream's row.  Counts (n_in, wsa_stream_input_capacity, wsa_stream_paced_input) stay frames of one channel.
 *   - Bytes of a row behind the step's count for that stream, the other channels and the rows of streams not active in the step are
 *     never read into a result.
 * wsa_stream_set_input_format is legal before the first step and between a wsa_stream_collect and the next step; it (re)allocates the
 * pinned packed buffer — [n_streams][wsa_stream_input_stride_bytes] bytes, a row = wsa_stream_input_stride * max channels * sample size
 * rounded up to 16, zeroed — and drops a captured graph.  WSA_PCM_F32 returns to the float buffers (channels NULL or all 1).  While a
 * packed format is set, wsa_stream_step_host / _host_n read the packed buffer, wsa_stream_step_packed takes device-resident packed rows
 * (d_pcm aligned to 16 bytes, stream i's row at d_pcm + i * stream_stride_bytes, n_streams * stream_stride_bytes bytes readable; n_in
 * NULL: samples_per_step / the paced counts), and the float device entry points are refused.  WSA_ERR_INVALID with a message naming the
 * fault: an unknown format; a channel count outside 1 .. 64; channels above 1 with WSA_PCM_F32; wsa_stream_step_packed on an F32 set;
 * wsa_stream_step / wsa_stream_step_n on a packed set; wsa_stream_time_steps with a float feed on a packed set and
 * wsa_stream_time_steps_packed with a feed on an F32 set; a stream_stride_bytes that is no multiple of 16 or too small for the largest
 * count of the step.
 */
#define WSA_PCM_F32   0   /* floats, mono: the entry points above as they are */
#define WSA_PCM_I16   1   /* signed 16-bit, native byte order */
#define WSA_PCM_MULAW 2   /* G.711 mu-law, one byte per sample */
#define WSA_PCM_ALAW  3   /* G.711 A-law, one byte per sample */
wsa_status wsa_stream_set_input_format(wsa_stream *st, int32_t format, const uint32_t *channels /* [n_streams], NULL = mono */);
void      *wsa_stream_host_input_packed(wsa_stream *st);        /* NULL while the format is F32 */
uint32_t   wsa_stream_input_stride_bytes(const wsa_stream *st); /* bytes per stream row of that buffer, a multiple of 16 (F32: of the float buffer) */
wsa_status wsa_stream_step_packed(wsa_stream *st, const void *d_pcm, uint64_t stream_stride_bytes,
                                  const uint32_t *n_in, const uint8_t *ctl, void *stream);   /* device-resident packed input */
/* wsa_stream_time_steps with feed blocks of [n_streams][wsa_stream_input_stride_bytes] packed bytes */
wsa_status wsa_stream_time_steps_packed(wsa_stream *st, uint32_t n_steps, const void *feed, uint32_t feed_steps,
                                        void *stream, double *out_us, uint64_t *rows_total);
/* PK-1 on the host, no device: channel 0 of n_frames interleaved frames -> out[n_frames].  WSA_ERR_INVALID (no context, no message):
 * an unknown format, channels outside 1 .. 64, a NULL buffer with n_frames > 0. */
wsa_status wsa_pcm_decode(int32_t format, const void *in, uint64_t n_frames, uint32_t channels, float *out);

/*
 * ---- Every PCM encoding a WAV holds into batches, unpacked on the GPU (additions within version 5: probe for wsa_batch_run_host_packed).
 *
 * The batch counterpart of the packed stream input, spec PK-2: a batch's clips go to the device as the bytes the file
 * holds, every clip in its own format and with its own channel count, and ONE kernel (batch_unpack_kernel) turns channel 0 of each clip
 * into the floats the float path would have been given.  A run on packed clips gives byte for byte what the same batch gives through
 * wsa_batch_run_host on wsa_pcm_decode(packed): every result table, wsa_batch_copy_pcm on resampling batches, every attached model's
 * output — at every output level, on plain, resampled and mixed-rate batches.
 *   - The formats of PK-1 (WSA_PCM_F32 .. WSA_PCM_ALAW above) and the linear encodings below, little-endian as a WAV holds them.
 *     Numbers 4 .. 7 are unassigned (kept for further 8-bit companded codes) and refused everywhere.
 *       WSA_PCM_U8   1 byte            (x - 128) / 128                                   exact
 *       WSA_PCM_I24  3 bytes, packed   the sign-extended value / 2^23                    exact in fp32
 *       WSA_PCM_I32  4 bytes           (float)x / 2^31, converted to nearest even        2^31 - 1 gives 1.0f
 *       WSA_PCM_F64  8 bytes           the double rounded to fp32, nearest even          overflow gives +-Inf, -0 is kept, results below 2^-126
 *                                                                                        are fp32 denormals and are kept, NaN stays NaN
 *     WSA_PCM_F32 with more than one channel is legal for batches (interleaved floats, channel 0 copied bit for bit); streams keep
 *     refusing it, and wsa_stream_set_input_format keeps refusing 8 .. 11: these are file encodings.
 *   - Clip i is n_samples(_in)[i] frames interleaved over channels[i] channels (1 .. 64; NULL: all mono): sample j is element
 *     j * channels[i] of the clip's bytes.  Bytes behind a clip's last frame and the other channels never influence a result; floats
 *     behind a clip's count in its staging row are not written.
 * wsa_batch_run_host_packed: clips in host memory (clip i at pcm[i], any alignment); one upload per clip (clips that lie back to back
 * in one wsa_host_alloc slab travel merged where the device layout allows it), then the unpack kernel, then the run.
 * wsa_batch_set_input_format plans the device-resident layout once — the descriptor table is uploaded and the float staging
 * allocated — and is legal before a run and between a result and the next run.  wsa_batch_packed_offset(b, i) is then the byte
 * offset of clip i (a multiple of 16), and with i == n_clips the number of bytes to provide.  wsa_batch_run_packed reads
 * device-resident packed clips at d_packed + offset(i) (d_packed aligned to 16 bytes): kernel launches only, nothing is allocated, the
 * call can be captured into a hipGraph like wsa_batch_run.
 * WSA_ERR_INVALID with a message that names the clip: an unknown format (4 .. 7 included), channels outside 1 .. 64;
 * wsa_batch_run_packed before wsa_batch_set_input_format, or with a NULL or misaligned d_packed.
 * wsa_pcm_decode knows the same formats, any channel count 1 .. 64 for each.
 */
#define WSA_PCM_U8    8   /* unsigned 8-bit, as an 8-bit WAV holds it */
#define WSA_PCM_I24   9   /* signed 24-bit, 3 bytes per sample, little-endian */
#define WSA_PCM_I32  10   /* signed 32-bit, little-endian */
#define WSA_PCM_F64  11   /* IEEE double, little-endian */
wsa_status wsa_batch_run_host_packed(wsa_batch *b, const void *const *pcm, const int32_t *formats /* [n_clips] */,
                                     const uint32_t *channels /* [n_clips], NULL = mono */, void *stream);
wsa_status wsa_batch_set_input_format(wsa_batch *b, const int32_t *formats, const uint32_t *channels);
uint64_t   wsa_batch_packed_offset(const wsa_batch *b, uint32_t clip);   /* 0 before wsa_batch_set_input_format and for clip > n_clips */
wsa_status wsa_batch_run_packed(wsa_batch *b, const void *d_packed, void *stream);

/*
 * ---- Multichannel PCM: any channel, every channel or the mono mix (additions within version 5: probe for wsa_batch_set_input_channels).
 *
 * The entries above analyse channel 0 of an interleaved clip or stream.  Spec PK-3: each clip (each stream) names what it
 * takes from an interleaved source of `channels` channels through a `select` word and a `source` word.
 *   - select: a channel index 0 .. channels - 1 — sample j is element j * channels + select, decoded as PK-1 / PK-2 decode channel 0 — or
 *     WSA_CHANNEL_MIX: m_j = (((x_j,0 + x_j,1) + x_j,2) + ...) * fl32(1 / channels), every term a PK-2 decoded fp32 value, fp32 additions in
 *     ascending channel order, then one fp32 multiply (two channels: Web Audio's 0.5 * (L + R)).  NaN and Inf propagate as fp32 arithmetic
 *     gives them; one channel with MIX is the plain decode.  NULL: every clip takes channel 0.
 *   - source: NULL (every clip reads its own bytes), or source[i] = the clip whose bytes clip i reads.  A source names itself
 *     (source[source[i]] == source[i]); a consumer takes its source's format and channel count (its own formats / channels entries are
 *     not read) and has no more frames than its source.  The bytes of a C-channel file travel once and feed up to C + 1 clips.  Consumers
 *     have no bytes of their own: wsa_batch_packed_offset of a consumer is its source's offset.
 *   - Nothing behind a source's last frame is read, nothing behind a clip's own frame count is written.
 * A clip that selects c, or the mix, gives byte for byte what the same batch gives through wsa_batch_run_host on a mono float clip holding
 * wsa_pcm_decode_select of those bytes: every result table at every output level, on plain, resampled and mixed-rate batches, every
 * attached model's output; streams the same, step for step, against wsa_stream_step_host.
 * wsa_batch_set_input_channels has the role of wsa_batch_set_input_format (plans the layout, uploads the descriptors, allocates the
 * staging); wsa_batch_run_packed then runs it, launches only (batch_deinterleave_kernel: each source's bytes once through LDS, one float
 * row per clip that reads them).  wsa_batch_run_host_channels takes host clips; pcm[i] of a consumer is ignored.
 * wsa_stream_set_input_channels: stream i reads the packed row of stream source[i] (formats as wsa_stream_set_input_format takes them);
 * counts and control bytes stay per stream, the host fills one row per source.  WSA_PCM_F32 returns to the float buffers (channels all 1,
 * select 0 or the mix, every stream its own source).
 * WSA_ERR_INVALID with a message that names the clip or stream: a select that is neither an index below `channels` nor
 * WSA_CHANNEL_MIX; a source out of range, or one that is not its own source; a consumer with more frames than its source; what the
 * format entries refuse.  wsa_pcm_decode_select (no context, no message) refuses what wsa_pcm_decode refuses, and such a select.
 * wsa_pcm_channels_tile_frames: the frames of one source a workgroup of batch_deinterleave_kernel takes at a time (a multiple of 16; 0 for
 * an unknown format or channels outside 1 .. 64).
 */
#define WSA_CHANNEL_MIX 0xFFFFFFFFu
/* PK-3 on the host, no device.  select = c reads nothing behind channel c of the last frame; the mix reads whole frames */
wsa_status wsa_pcm_decode_select(int32_t format, const void *in, uint64_t n_frames, uint32_t channels, uint32_t select, float *out);
wsa_status wsa_batch_set_input_channels(wsa_batch *b, const int32_t *formats, const uint32_t *channels, const uint32_t *select,
                                        const uint32_t *source);
wsa_status wsa_batch_run_host_channels(wsa_batch *b, const void *const *pcm, const int32_t *formats, const uint32_t *channels,
                                       const uint32_t *select, const uint32_t *source, void *stream);
wsa_status wsa_stream_set_input_channels(wsa_stream *st, int32_t format, const uint32_t *channels, const uint32_t *select,
                                         const uint32_t *source);
uint32_t   wsa_pcm_channels_tile_frames(int32_t format, uint32_t channels);

/*
 * ---- A feature DB that stays on the device (additions within version 5: probe for wsa_featdb_create).
 * Stands in for what the reference APPLICATION keeps between its steps: every callback's rows go into a feature DB (ref src/index.js:35-100
 * call_backed -> StoreFeatures, js/featuredb.js), and training (src/neuralmodel.js:163-403), prediction (:410-535), the results table
 * (src/localstore.js:498-627) and the KNN learner (src/neuralmodel.js:731-837) all read that DB.  Specification FD-1 of DESIGN.md §3,
 * kernels K10 (csrc/featdb.hip).  A wsa_featdb holds the FEATURE columns of such a DB on the context's device, ONE allocation of
 * capacity_rows x width doubles made at create; rows are appended behind the ones it holds and never move.  Strings (file names, part
 * tags, times, labels) stay on the host, which learns from `kept` which source row each stored row came from.
 * One set of buffers: pass the SAME stream to every call on it.  A DB belongs to the context it was created on; destroy it before that
 * context.  Trainers, DB statistics and KNN stores made from a DB hold no reference to it.
 */
typedef struct wsa_featdb wsa_featdb;
/* width: 53, 264 or 23 (wsa_level_feature_count), anything else is refused; capacity_rows at least 1 */
wsa_status wsa_featdb_create(wsa_ctx *ctx, int32_t width, uint32_t capacity_rows, wsa_featdb **out);
void       wsa_featdb_destroy(wsa_featdb *db);
wsa_status wsa_featdb_clear(wsa_featdb *db);                       /* the count returns to 0; nothing is freed */
wsa_status wsa_featdb_count(const wsa_featdb *db, uint32_t *n_rows);
/* The rows of the batch's last run that the app's storing keeps, appended in source order, columns copied bit for bit:
 *   levels 5 and 13 (width 53): every row;
 *   level 12 (width 23): row r of the row table unless a row r' <= r of the same callback (meta[0], meta[1]) has a slot 23 that is not
 *            equal to 0 (NaN counts as marked): a syllable on which uncmin threw ends its callback's list; columns 0 .. 22 are stored;
 *   level 11 (width 264): of the utterance rows the last one of every clip that has any, row d_clip_utt_off[c + 1] - 1.
 * *first_row = the DB row of the first appended one, *n_added their number (either may be NULL); kept (host int32 [kept_cap], or NULL)
 * receives, per appended row, its source row (level 11: utterance row) index.  SYNCHRONISES `stream` for the run's counters (as
 * wsa_batch_result does, with its rerun rule) and, at levels 11 and 12, once more for the number of kept rows; at levels 5 and 13 the copy
 * is only enqueued behind that.
 * WSA_ERR_INVALID with a message: a level that does not go with the width (naming both), a batch of another context, a batch without
 * a run, kept_cap below the rows to add.  A run with WSA_FLAG_CAPACITY set is refused with WSA_ERR_CAPACITY and the message of
 * wsa_batch_result.  WSA_ERR_CAPACITY naming the DB's count, the rows to add and the capacity when they do not fit.  A refused call
 * leaves the DB unchanged in every byte. */
wsa_status wsa_featdb_append_batch(wsa_featdb *db, wsa_batch *batch, void *stream, uint32_t *first_row, uint32_t *n_added,
                                   int32_t *kept, uint32_t kept_cap);
/* n dense host rows [n][width] (an imported data_<db>.json); WSA_ERR_CAPACITY as above.  Returns when the rows are on the device. */
wsa_status wsa_featdb_append_host(wsa_featdb *db, const double *feat, uint32_t n, void *stream);
/* the DB's rows on the device, dense [count][width] f64; the pointer is valid until wsa_featdb_destroy */
wsa_status wsa_featdb_device_rows(const wsa_featdb *db, const double **d_feat);
/* rows first .. first + n - 1 to host memory out [n][width]; synchronises `stream` */
wsa_status wsa_featdb_copy_rows(wsa_featdb *db, void *stream, uint32_t first, uint32_t n, double *out);
/* d_out [n][width] (device) = DB rows rows[0 .. n-1] (host uint32, duplicates allowed).  Every index is checked against the count before
 * anything is enqueued (the message names the entry); the list is staged through pinned memory.  Only enqueues. */
wsa_status wsa_featdb_gather(wsa_featdb *db, const uint32_t *rows, uint32_t n, double *d_out, void *stream);
/* Per column the minimum and the maximum over the selected rows (rows == NULL: rows 0 .. n - 1; duplicates allowed; n at least 1) into
 * host in_min / in_max [width].  A column that holds a NaN among the selected rows gives NaN for both; otherwise the exact minimum and
 * maximum with -0 below +0.  Both are exact selections on the bit patterns, so the result does not depend on the grid; there are no
 * floating-point atomics.  Synchronises `stream`. */
wsa_status wsa_featdb_ranges(wsa_featdb *db, const uint32_t *rows, uint32_t n, void *stream, double *in_min, double *in_max);
/* sizes of K10 in rows (tests place their edge cases by these): the keep / scan kernel ballots rows_per_wave_tile source rows per wave and
 * walks the source rows_per_workgroup at a time; the copy kernel takes rows_per_pass appended rows per pass of its grid */
wsa_status wsa_featdb_tile_info(int32_t *rows_per_wave_tile, int32_t *rows_per_workgroup, int32_t *rows_per_pass);
/* wsa_trainer_create / wsa_regress_trainer_create with feat = DB rows rows[0 .. n_rows - 1] in that order (host uint32 [n_rows],
 * duplicates allowed): the trainer is in every bit the one the host entry makes from the host copy of those rows (one kernel normalises
 * row rows[i] into the trainer's x[i] with the same expression).  Refuses what those refuse, and a DB of another context, a DB whose
 * width is not units[0], a row index outside the DB (naming the entry).  Waits for the device before it reads the DB; the trainer keeps
 * no reference to the DB. */
wsa_status wsa_trainer_create_db(wsa_ctx *ctx, const wsa_model_desc *init, const wsa_featdb *db, const uint32_t *rows, const int32_t *label,
                                 uint32_t n_rows, uint32_t n_val, uint32_t batch_size, double learning_rate, wsa_trainer **out);
wsa_status wsa_regress_trainer_create_db(wsa_ctx *ctx, const wsa_model_desc *init, const wsa_featdb *db, const uint32_t *rows,
                                         const double *target, uint32_t n_rows, uint32_t n_val, uint32_t batch_size,
                                         double learning_rate, double out_min, double out_max, wsa_trainer **out);
/* wsa_wide_dbstats_create over DB rows first_row .. first_row + n_rows - 1, copied device to device (n_feat = the DB's width);
 * waits for the device before it reads the DB */
wsa_status wsa_featdb_dbstats_create(wsa_ctx *ctx, const wsa_featdb *db, uint32_t first_row, uint32_t n_rows, const double *duration,
                                 uint32_t n_cat, const uint32_t *vocab, uint32_t n_ord, wsa_dbstats **out);

/*
 * ---- Live streams collect into the device DB (additions within version 5: probe for wsa_stream_set_featdb).
 * The other half of the app's collecting: call_backed -> StoreFeatures files every callback, from a file or from the microphone
 * (ref src/index.js:35-100, src/localstore.js:39-65).  Specification FD-2 of DESIGN.md §3, kernels in csrc/stream_featdb.hip.
 * Attach (db != NULL) or detach (NULL) a feature DB: while attached, every step appends that step's rows to the DB as two kernels of the
 * step — a plan kernel (keep rule, scan, capacity decision) and a copy kernel — on the step's own stream, behind the level's own
 * kernels and before the epilogue; the step stays one graph launch.  What a step stores:
 *   levels 5 and 13 (width 53): every row of the step;
 *   level 12 (width 23): FD-1's rule on the step's row table (a callback's rows all arrive in one step), columns 0 .. 22;
 *   level 11 (width 264): every stream owns ONE DB row per launch (the app files every utterance result under part 0, so each replaces
 *            the one before): a stream's START forgets its row; a stream with results in the step takes the next new DB row if it has
 *            none (new rows in stream order) and the LAST of its results of the step is written there.  Rows never move.
 * Every column is the source's 64 bits.  Each step is decided alone before anything is written: a step whose flags carry
 * WSA_FLAG_CAPACITY stores nothing; a step whose new rows do not fit the DB's capacity stores nothing at all (level 11: no replacement
 * and no row handed out either; START still forgets), reports their number in not_fitted and sets WSA_FLAG_DB_FULL in the step's
 * status_flags (not fatal).  A later step that fits is stored.
 * The host owns the count: it hands wsa_featdb_count to every step before the launch and advances it when it reads the step's outcome,
 * in wsa_stream_collect or at the start of the next step.  Between a collect and the next step every wsa_featdb_* entry, the DB
 * trainers and wsa_featdb_dbstats_create work on an attached DB as on any; between a step and its collect they are refused with a
 * message (wsa_featdb_count then tells the count before the step).  wsa_featdb_clear on an attached DB is always refused: detach, clear,
 * attach.
 * Synchronises the last step, allocates everything and drops the captured graph.  Refused with a message that names the values: a DB of
 * another context; a width that does not go with the set's output_level (53: levels 5 / 13, 23: level 12, 264: level 11; levels 3, 4
 * and 10 store nothing); a DB that is attached to another stream set.  Separate from the model, ensemble, KNN and regression
 * attachments.  The DB must outlive its attachment (detach, or destroy the stream set, first).
 */
#define WSA_FLAG_DB_FULL 16u     /* streams: this step's new rows did not fit the attached feature DB; the step stored nothing (wsa_stream_db_rows) */
wsa_status wsa_stream_set_featdb(wsa_stream *st, wsa_featdb *db);
typedef struct {
    uint32_t first_row;          /* the DB row of the step's first new row (the count before the step) */
    uint32_t n_added;            /* new DB rows: first_row .. first_row + n_added - 1 */
    uint32_t n_replaced;         /* level 11: DB rows rewritten in place */
    uint32_t not_fitted;         /* the new rows of a step that stored nothing because they did not fit; else 0 */
    const int32_t *kept;         /* [n_added]: the row of wsa_stream_rows (level 11: the utterance row) that became DB row first_row + i */
    const int32_t *replaced;     /* [n_replaced][2] = {utterance row, DB row} (level 11; else NULL) */
} wsa_stream_db_result;
/* After wsa_stream_collect of the same step: host memory owned by the stream object, valid until the next step.
 * WSA_ERR_INVALID without an attached DB. */
wsa_status wsa_stream_db_rows(wsa_stream *st, wsa_stream_db_result *out);
/* sizes of the step's DB kernels in rows: the plan kernel ballots rows_per_wave_tile rows per wave and walks the step's table
 * rows_per_workgroup at a time; the copy kernel moves tiles of copy_tile_rows stored rows with a grid of at most copy_grid workgroups,
 * fixed at attach (min(copy_grid, tiles of the step's row capacity)) */
wsa_status wsa_stream_featdb_tile_info(int32_t *rows_per_wave_tile, int32_t *rows_per_workgroup, int32_t *copy_tile_rows, int32_t *copy_grid);

#ifdef __cplusplus
}
#endif
#endif
