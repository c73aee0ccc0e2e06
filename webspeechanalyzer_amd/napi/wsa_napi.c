/*
 * wsa_napi.c — thin N-API binding of the C ABI (include/wsa.h) for the JavaScript host
 * (webspeechanalyzer_amd/js/formantanalyzer.js).  Raw node_api.h, N-API >= 4 (async work).
 *
 * Exposes exactly what the host needs:
 *   abiVersion() -> number
 *   defaults() -> config object                                  (wsa_config_default, ref @B2965)
 *   create(config, device) -> external ctx                        (wsa_create)
 *   destroy(ctx)
 *   geometry(ctx, fs) -> {nfft, win, hop, bands, kmax}            (wsa_geometry_for)
 *   binsHz(ctx, fs) -> Float64Array                               (wsa_bins_hz, ref @B8380)
 *   processBatch(ctx, clips: Float32Array[], fs[, output_level[, analysis_rate]]) -> Promise<{meta, feat, segments, rowOff, segOff, stageMs[, formants, frameOff][, trackOff, trackPoints, trackRanked]}>
 *       runs wsa_batch_create / wsa_batch_run_host / wsa_batch_copy_rows on a worker thread
 *       (napi_async_work) so the JS thread stays free; the promise settles on the JS main thread.
 *   streamOpen(ctx, nStreams, fs, framesPerStep, maxSpanFrames) -> external stream      (wsa_stream_create)
 *   streamOpenMixed(ctx, nStreams, rates: Float64Array, fsOut, framesPerStep, maxSpanFrames) -> external stream   (wsa_stream_create_mixed:
 *       stream i arrives at rates[i] and is converted to fsOut inside the step)
 *   streamInfo(stream) -> {capacity: Uint32Array, inputStride, samplesPerStep}   (wsa_stream_input_capacity / _input_stride / _samples_per_step)
 *   streamPaced(stream) -> Uint32Array: the samples a paced step takes from every stream next   (wsa_stream_paced_input)
 *   streamInput(stream) -> Float32Array over the pinned [nStreams][inputStride] input buffer (no copy; inputStride = samplesPerStep on a plain set)
 *   streamSetInput(stream, format, channels) before the first streamInput: wsa_stream_set_input_format; streamInput then gives an Int16Array / Uint8Array
 *     over the packed pinned buffer, [nStreams][streamInfo().inputStrideBytes / element size]
 *   streamSetInput(stream, format, channels, select, source): wsa_stream_set_input_channels (spec PK-3: stream i takes channel select[i], 0xFFFFFFFF the mix,
 *     of the packed row of stream source[i])
 *   decodePcm(format, typedArray, channels[, select]) -> Float32Array   (wsa_pcm_decode_select: channel `select` of interleaved frames or their mix, specs PK-1 / PK-3)
 *   streamStep(stream, ctl: Uint8Array | null[, counts: Uint32Array | null]) -> {meta, feat, segments}   (wsa_stream_step_host[_n] + wsa_stream_collect;
 *       one hipGraph launch, well under a millisecond, so it runs on the calling thread; counts: samples per stream in this step, else paced)
 *   processBatch(..., model, formats)           (9th argument an Int32Array of WSA_PCM_* numbers: the clips are Uint8Arrays over the bytes a file holds, any
 *                                               mix of encodings, clip i interleaved over channels[i] channels: wsa_batch_run_host_packed, spec PK-2)
 *   processBatch(..., model, formats, select, source)   (10th / 11th argument Uint32Arrays: clip i takes channel select[i] or the mix of the bytes of clip
 *                                               source[i], which travel once: wsa_batch_run_host_channels, spec PK-3)
 *   processBatch(..., [models])                 (8th argument an array of models: wsa_batch_classify_ensemble; the result gains `ens`)
 *   streamSetEnsemble(stream, [models] | null)  (wsa_stream_set_ensemble: streamStep results gain `ens`)
 *   streamSetRegress(stream, [models] | null, outMin: Float64Array, outMax: Float64Array)   (wsa_stream_set_regress: streamStep results gain regValue [H][rows], regCb, regCbValue / regCbWeight
 *                                               [H][callbacks], regSum / regWeight / regRunValue [H][streams], regNHeads; the stream object owns the group it makes of the models)
 *   batchRegressGroup(ctx, [models], outMin, outMax) -> the same tables (value, cb, cbValue, cbWeight, clipSum, clipWeight, clipValue, nHeads) over the rows of the context's last
 *                                               processBatch (wsa_batch_regress_group on its kept plan; specification RG-1)
 *   streamSetKnn(stream, knn | null, k)         (wsa_stream_set_knn: streamStep results gain knnLabel, knnConf, knnCb, knnCbLabel, knnCbConf, knnStreamConf, knnNClasses;
 *                                                beside a model or an ensemble, not in place of one)
 *   streamSetModel(stream, model | null)        (wsa_stream_set_model: streamStep results gain prob, cb, cbLabel, cbConf, streamConf, nClasses)
 *   streamSetFeatdb(stream, db | null)          (wsa_stream_set_featdb, specification FD-2: every streamStep appends its rows to the device DB; flags gain WSA_FLAG_DB_FULL)
 *   streamDbRows(stream) -> {first, added, replaced, notFitted, kept, replacedRows}      (wsa_stream_db_rows of the last streamStep)
 *   streamClose(stream)
 * Rejections carry the library's error string.  No compute happens in this file.
 */
#include <node_api.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <pthread.h>
#include "../../include/wsa.h"
#include "../../include/wsa_eval.h"

#define NAPI_OK(env, call) do { if ((call) != napi_ok) { napi_throw_error((env), NULL, "N-API call failed: " #call); return NULL; } } while (0)

static const char *CFG_INT[] = {"spec_type", "output_level", "N_fft_bins", "N_mel_bins", "auto_noise_gate"};
static const char *CFG_DBL[] = {"f_min", "f_max", "window_width", "window_step", "pause_length", "min_seg_length",
                                "voiced_max_dB", "voiced_min_dB", "pre_norm_gain", "high_f_emph"};

static int32_t *cfg_int(wsa_config *c, int i) {
    switch (i) { case 0: return &c->spec_type; case 1: return &c->output_level; case 2: return &c->N_fft_bins;
                 case 3: return &c->N_mel_bins; default: return &c->auto_noise_gate; }
}
static double *cfg_dbl(wsa_config *c, int i) {
    switch (i) { case 0: return &c->f_min; case 1: return &c->f_max; case 2: return &c->window_width; case 3: return &c->window_step;
                 case 4: return &c->pause_length; case 5: return &c->min_seg_length; case 6: return &c->voiced_max_dB;
                 case 7: return &c->voiced_min_dB; case 8: return &c->pre_norm_gain; default: return &c->high_f_emph; }
}

static napi_value config_to_js(napi_env env, const wsa_config *c) {
    napi_value o, v;
    NAPI_OK(env, napi_create_object(env, &o));
    for (int i = 0; i < 5; i++) {
        if (i == 4) { NAPI_OK(env, napi_get_boolean(env, *cfg_int((wsa_config *)c, i) != 0, &v)); }
        else NAPI_OK(env, napi_create_int32(env, *cfg_int((wsa_config *)c, i), &v));
        NAPI_OK(env, napi_set_named_property(env, o, CFG_INT[i], v));
    }
    for (int i = 0; i < 10; i++) {
        NAPI_OK(env, napi_create_double(env, *cfg_dbl((wsa_config *)c, i), &v));
        NAPI_OK(env, napi_set_named_property(env, o, CFG_DBL[i], v));
    }
    return o;
}

static int js_to_config(napi_env env, napi_value o, wsa_config *c) {
    wsa_config_default(c);
    for (int i = 0; i < 5; i++) {
        bool has; napi_value v; napi_valuetype t;
        if (napi_has_named_property(env, o, CFG_INT[i], &has) != napi_ok || !has) continue;
        if (napi_get_named_property(env, o, CFG_INT[i], &v) != napi_ok || napi_typeof(env, v, &t) != napi_ok) return 0;
        if (t == napi_boolean) { bool b; napi_get_value_bool(env, v, &b); *cfg_int(c, i) = b ? 1 : 0; }
        else if (t == napi_number) { double d; napi_get_value_double(env, v, &d); *cfg_int(c, i) = (int32_t)d; }
    }
    for (int i = 0; i < 10; i++) {
        bool has; napi_value v; napi_valuetype t;
        if (napi_has_named_property(env, o, CFG_DBL[i], &has) != napi_ok || !has) continue;
        if (napi_get_named_property(env, o, CFG_DBL[i], &v) != napi_ok || napi_typeof(env, v, &t) != napi_ok) return 0;
        if (t == napi_number) napi_get_value_double(env, v, cfg_dbl(c, i));
    }
    return 1;
}

static napi_value fn_abi_version(napi_env env, napi_callback_info info) {
    napi_value v; NAPI_OK(env, napi_create_int32(env, wsa_abi_version(), &v)); return v;
}
static napi_value fn_defaults(napi_env env, napi_callback_info info) {
    wsa_config c; wsa_config_default(&c); return config_to_js(env, &c);
}

/* What JS holds for a context: a box that outlives wsa_destroy, so that a handle used after destroy() (or destroyed twice) finds NULL
 * instead of freed memory, and that counts the batches in flight and the open streams created from the context — destroy() refuses
 * while any of them is alive (their wsa_batch / wsa_stream objects point into the context). */
typedef struct {
    wsa_ctx *ctx; uint32_t children;
    /* the planned batch of the last processBatch call: a call with the same clip lengths and rates reuses it (planning a 1024-clip
     * batch allocates GBs of work space: ~3 ms and more); taken out of the box while a job uses it, dropped by destroy() */
    wsa_batch *plan; uint32_t plan_n; uint32_t *plan_ns; double plan_fs, plan_fs_out; double *plan_fs_each;   /* plan_fs_each: one rate per clip (wsa_batch_create_mixed), else NULL */
    /* the context's own HIP stream (wsa_queue_create, made by the first processBatch): every job of the context runs on it, so that the jobs of TWO
     * contexts on one device overlap — the upload of one batch under the kernels of the other — instead of queueing on the device's null stream */
    void *queue;
    struct model_box *models;     /* the classifier models created on this context (modelCreate): destroy() destroys them with it */
    /* the ensemble of the last processBatch call that had one (wsa_ensemble_create over ens_models): a call with the same list reuses it, so the
     * kept plan keeps its ensemble tables too; made and replaced by the job (one job at a time uses a context), dropped by destroy() */
    wsa_ensemble *ens; struct model_box *ens_models[WSA_ENSEMBLE_MAX]; uint32_t ens_n;
    struct knn_box *knns;         /* the KNN stores created on this context (knnCreate): destroy() destroys them with it */
    struct fdb_box *fdbs;         /* the device feature DBs created on this context (featdbCreate): destroy() destroys them with it */
    /* the regression group of the last batchRegressGroup call (wsa_regress_group_create over reg_models and their ranges): a call with the same models
     * and ranges reuses it, so the kept plan keeps its group tables and allocates nothing; replaced by the next other list, dropped by destroy() */
    wsa_regress_group *reg; struct model_box *reg_models[WSA_REGRESS_GROUP_MAX]; double reg_lo[WSA_REGRESS_GROUP_MAX], reg_hi[WSA_REGRESS_GROUP_MAX]; uint32_t reg_n;
} ctx_box;
/* What JS holds for a model (wsa_model): like the context's box it outlives the model, so that a handle used after modelDestroy() or after its
 * context's destroy() finds NULL; `busy` counts the jobs that classify with it (modelDestroy() refuses meanwhile) */
typedef struct model_box { wsa_model *m; ctx_box *owner; uint32_t busy, n_classes, n_inputs; struct model_box *next; } model_box;   /* n_inputs: units[0], the width of the rows the model takes (53, 264 or 23) */
static void model_unlink(model_box *mb) {
    if (mb->owner) for (model_box **q = &mb->owner->models; *q; q = &(*q)->next) if (*q == mb) { *q = mb->next; break; }
    mb->owner = NULL; mb->next = NULL;
}
/* What JS holds for a KNN store (wsa_knn): a box like a model's; every call on a store is synchronous, so it is never busy */
typedef struct knn_box { wsa_knn *k; ctx_box *owner; uint32_t width, n_classes; struct knn_box *next; } knn_box;
static void knn_unlink(knn_box *kb) {
    if (kb->owner) for (knn_box **q = &kb->owner->knns; *q; q = &(*q)->next) if (*q == kb) { *q = kb->next; break; }
    kb->owner = NULL; kb->next = NULL;
}
/* What JS holds for a device feature DB (wsa_featdb): a box like a KNN store's; every call on a DB is synchronous but train, which counts as a child of the context */
typedef struct fdb_box { wsa_featdb *db; ctx_box *owner; uint32_t width; struct fdb_box *next; } fdb_box;
static void fdb_unlink(fdb_box *fb) {
    if (fb->owner) for (fdb_box **q = &fb->owner->fdbs; *q; q = &(*q)->next) if (*q == fb) { *q = fb->next; break; }
    fb->owner = NULL; fb->next = NULL;
}
static void box_drop_ensemble(ctx_box *b) {
    if (b->ens) wsa_ensemble_destroy(b->ens);
    b->ens = NULL; b->ens_n = 0;
}
static void box_drop_regress(ctx_box *b) {
    if (b->reg) wsa_regress_group_destroy(b->reg);
    b->reg = NULL; b->reg_n = 0;
}
static void box_drop_plan(ctx_box *b) {
    if (b->plan) wsa_batch_destroy(b->plan);
    free(b->plan_ns); free(b->plan_fs_each); b->plan = NULL; b->plan_ns = NULL; b->plan_fs_each = NULL; b->plan_n = 0;
}
/* the communicator of gatherRows (one at a time; rebuilt when the set of contexts changes, dropped before any of its contexts is destroyed) */
static wsa_gather *g_gather = NULL; static wsa_ctx **g_gather_ctxs = NULL; static uint32_t g_gather_n = 0;
/* gatherRows jobs run on libuv worker threads, destroy() on the JS thread: every access to the three words above holds this lock
 * (a wsa_gather is not thread-safe either: one exchange at a time) */
static pthread_mutex_t g_gather_lock = PTHREAD_MUTEX_INITIALIZER;
static void gather_drop(void) {          /* caller holds g_gather_lock */
    if (g_gather) wsa_gather_destroy(g_gather);
    free(g_gather_ctxs); g_gather = NULL; g_gather_ctxs = NULL; g_gather_n = 0;
}
static void ctx_finalize(napi_env env, void *data, void *hint) {          /* the JS handle is gone */
    ctx_box *b = (ctx_box *)data;
    if (!b->ctx && b->children == 0) free(b);        /* a context nobody destroyed stays (explicit destroy() only: the finalizer may run at process exit, after the HIP runtime) */
}

static napi_value fn_create(napi_env env, napi_callback_info info) {
    size_t argc = 2; napi_value argv[2];
    NAPI_OK(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
    wsa_config c; int32_t device = 0;
    if (argc < 1 || !js_to_config(env, argv[0], &c)) { napi_throw_type_error(env, NULL, "create(config, device)"); return NULL; }
    if (argc > 1) napi_get_value_int32(env, argv[1], &device);
    wsa_ctx *ctx = NULL;
    const wsa_status st = wsa_create(&c, device, &ctx);
    if (st != WSA_OK) { napi_throw_error(env, NULL, wsa_last_error(NULL)); return NULL; }
    ctx_box *box = calloc(1, sizeof *box);
    box->ctx = ctx;
    napi_value ext; NAPI_OK(env, napi_create_external(env, box, ctx_finalize, NULL, &ext));
    return ext;
}
static ctx_box *get_box(napi_env env, napi_value v) {
    void *p = NULL; if (napi_get_value_external(env, v, &p) != napi_ok) return NULL; return (ctx_box *)p;
}
static wsa_ctx *get_ctx(napi_env env, napi_value v) {                      /* NULL once destroy() has run */
    ctx_box *b = get_box(env, v); return b ? b->ctx : NULL;
}
static napi_value fn_destroy(napi_env env, napi_callback_info info) {
    size_t argc = 1; napi_value argv[1];
    NAPI_OK(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
    ctx_box *b = argc ? get_box(env, argv[0]) : NULL;
    if (b && b->ctx) {
        if (b->children) { napi_throw_error(env, NULL, "context still has batches in flight or open streams"); return NULL; }
        pthread_mutex_lock(&g_gather_lock);
        for (uint32_t i = 0; i < g_gather_n; i++) if (g_gather_ctxs[i] == b->ctx) { gather_drop(); break; }      /* the communicator goes before its contexts */
        pthread_mutex_unlock(&g_gather_lock);
        box_drop_plan(b);
        box_drop_ensemble(b);                /* (before its models) */
        box_drop_regress(b);
        while (b->models) { model_box *mb = b->models; wsa_model_destroy(mb->m); mb->m = NULL; model_unlink(mb); }     /* models go before their context */
        while (b->knns) { knn_box *kb = b->knns; wsa_knn_destroy(kb->k); kb->k = NULL; knn_unlink(kb); }               /* and so do KNN stores */
        while (b->fdbs) { fdb_box *fb = b->fdbs; wsa_featdb_destroy(fb->db); fb->db = NULL; fdb_unlink(fb); }           /* and device feature DBs */
        if (b->queue) { wsa_queue_destroy(b->ctx, b->queue); b->queue = NULL; }
        wsa_destroy(b->ctx); b->ctx = NULL;
    }
    return NULL;
}
/* allocPinned(ctx, bytes) -> ArrayBuffer over page-locked host memory (wsa_host_alloc): clips read into views of it reach the device by DMA at the
 * link's rate instead of through the runtime's staging copies.  The memory is released when the ArrayBuffer is collected. */
/* every page-locked buffer handed to JS has a record: freePinned(ab) releases the memory at a moment of the caller's choosing (hipHostFree synchronises the device:
 * inside the garbage collector's finalizer that stall hits the event loop whenever V8 decides) and detaches the ArrayBuffer; the finalizer then finds nothing left to do */
typedef struct pinned_rec { void *p; uint64_t bytes; int freed; struct pinned_rec *next; } pinned_rec;
static pinned_rec *g_pinned = NULL;                 /* JS thread only */
static void pinned_release(napi_env env, pinned_rec *r) {
    if (r->freed) return;
    int64_t now = 0;
    napi_adjust_external_memory(env, -(int64_t)r->bytes, &now);      /* V8 was told about the bytes at allocation: page-locked slabs do create GC pressure */
    wsa_host_free(r->p);
    r->freed = 1;
}
static void pinned_finalize(napi_env env, void *data, void *hint) {
    pinned_rec *r = (pinned_rec *)hint;
    pinned_release(env, r);
    for (pinned_rec **q = &g_pinned; *q; q = &(*q)->next) if (*q == r) { *q = r->next; break; }
    free(r);
}
static napi_value fn_alloc_pinned(napi_env env, napi_callback_info info) {
    size_t argc = 2; napi_value argv[2]; double bytes = 0;
    NAPI_OK(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
    wsa_ctx *ctx = argc ? get_ctx(env, argv[0]) : NULL;
    if (!ctx || argc < 2 || napi_get_value_double(env, argv[1], &bytes) != napi_ok || bytes < 0 || bytes > 68719476736.0) { napi_throw_type_error(env, NULL, "allocPinned(ctx, bytes)"); return NULL; }
    void *p = NULL;
    if (wsa_host_alloc(ctx, (uint64_t)bytes, &p) != WSA_OK) { napi_throw_error(env, NULL, wsa_last_error(ctx)); return NULL; }
    pinned_rec *r = calloc(1, sizeof *r);
    if (!r) { wsa_host_free(p); napi_throw_error(env, NULL, "out of memory"); return NULL; }
    r->p = p; r->bytes = (uint64_t)bytes;
    napi_value ab;
    if (napi_create_external_arraybuffer(env, p, (size_t)bytes, pinned_finalize, r, &ab) != napi_ok) { wsa_host_free(p); free(r); napi_throw_error(env, NULL, "napi_create_external_arraybuffer failed"); return NULL; }
    r->next = g_pinned; g_pinned = r;
    { int64_t now = 0; napi_adjust_external_memory(env, (int64_t)bytes, &now); }
    return ab;
}
/* freePinned(ab): the page-locked memory behind an ArrayBuffer of allocPinned goes back NOW (no run may still be reading it) and the ArrayBuffer is detached:
 * views on it have length 0 from here on.  Returns true when it was such a buffer and still allocated. */
static napi_value fn_free_pinned(napi_env env, napi_callback_info info) {
    size_t argc = 1; napi_value argv[1]; void *data = NULL; size_t len = 0; bool is_ab = false;
    NAPI_OK(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
    if (argc < 1 || napi_is_arraybuffer(env, argv[0], &is_ab) != napi_ok || !is_ab || napi_get_arraybuffer_info(env, argv[0], &data, &len) != napi_ok) { napi_throw_type_error(env, NULL, "freePinned(arrayBuffer)"); return NULL; }
    bool done = false;
    for (pinned_rec *r = g_pinned; r; r = r->next) if (r->p == data && !r->freed) { pinned_release(env, r); done = true; break; }
    if (done) (void)napi_detach_arraybuffer(env, argv[0]);
    napi_value v; NAPI_OK(env, napi_get_boolean(env, done, &v)); return v;
}
static napi_value fn_geometry(napi_env env, napi_callback_info info) {
    size_t argc = 2; napi_value argv[2]; double fs = 0;
    NAPI_OK(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
    wsa_ctx *ctx = argc ? get_ctx(env, argv[0]) : NULL;
    if (!ctx || argc < 2 || napi_get_value_double(env, argv[1], &fs) != napi_ok) { napi_throw_type_error(env, NULL, "geometry(ctx, fs)"); return NULL; }
    wsa_geometry g;
    if (wsa_geometry_for(ctx, fs, &g) != WSA_OK) { napi_throw_error(env, NULL, wsa_last_error(ctx)); return NULL; }
    napi_value o, v; NAPI_OK(env, napi_create_object(env, &o));
    const char *names[5] = {"nfft", "win", "hop", "bands", "kmax"}; const int32_t vals[5] = {g.nfft, g.win, g.hop, g.bands, g.kmax};
    for (int i = 0; i < 5; i++) { NAPI_OK(env, napi_create_int32(env, vals[i], &v)); NAPI_OK(env, napi_set_named_property(env, o, names[i], v)); }
    return o;
}
static napi_value fn_bins_hz(napi_env env, napi_callback_info info) {
    size_t argc = 2; napi_value argv[2]; double fs = 0;
    NAPI_OK(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
    wsa_ctx *ctx = argc ? get_ctx(env, argv[0]) : NULL;
    if (!ctx || argc < 2 || napi_get_value_double(env, argv[1], &fs) != napi_ok) { napi_throw_type_error(env, NULL, "binsHz(ctx, fs)"); return NULL; }
    wsa_geometry g;
    if (wsa_geometry_for(ctx, fs, &g) != WSA_OK) { napi_throw_error(env, NULL, wsa_last_error(ctx)); return NULL; }
    napi_value ab, ta; void *data = NULL;
    NAPI_OK(env, napi_create_arraybuffer(env, sizeof(double) * (size_t)g.bands, &data, &ab));
    if (wsa_bins_hz(ctx, fs, (double *)data, g.bands) != WSA_OK) { napi_throw_error(env, NULL, wsa_last_error(ctx)); return NULL; }
    NAPI_OK(env, napi_create_typedarray(env, napi_float64_array, (size_t)g.bands, ab, 0, &ta));
    return ta;
}

/* ---- processBatch: async work ---- */
typedef struct {
    napi_async_work work; napi_deferred deferred;
    wsa_ctx *ctx; double fs; double fs_out;      /* fs_out != fs: convert in front (wsa_batch_create_resampled) */
    double *fs_each;                             /* one rate per clip (a Float64Array in place of fs): wsa_batch_create_mixed, fs is 0 */
    uint32_t n_clips; uint32_t *n_samples; const float **pcm; napi_ref *clip_refs;
    int is_i16; uint32_t *channels;   /* Int16Array clips (pcm[] then holds int16 pointers): wsa_batch_run_host_i16 */
    uint32_t *select, *source;        /* 10th / 11th argument (with formats): clip i takes channel select[i] (0xFFFFFFFF: the mix) of the bytes of clip source[i]: wsa_batch_run_host_channels, spec PK-3 */
    int32_t *formats;                 /* 9th argument: one WSA_PCM_* number per clip, the clips Uint8Arrays of the files' bytes (pcm[] holds byte pointers): wsa_batch_run_host_packed */
    wsa_batch *plan; int plan_reused; /* taken from / returned to the box on the JS thread */
    /* results */
    wsa_status st; char err[512];
    uint32_t n_rows, n_segs; int32_t *meta; double *feat; int32_t *segs; uint32_t *row_off, *seg_off; float stage_ms[4];
    uint32_t n_frames; float *formants; uint32_t *frame_off;      /* levels 4 / 10 */
    uint32_t n_utt; int32_t *utt_meta; double *utt_feat; uint32_t *utt_off;   /* level 11 */
    int defer_rows;               /* the rows stay on the device (gatherRows collects them from all shards with one RCCL exchange) */
    int level; uint32_t trk_segs; uint64_t trk_np, trk_nr; uint64_t *trk_off; int32_t *trk_pts, *trk_rank;   /* level 3 */
    ctx_box *box;                 /* the JS handle's box: one child while the job runs */
    void *queue;                  /* the context's stream (ctx_box.queue) */
    model_box *model;             /* classify the rows with it (levels 5 / 13), or NULL */
    uint32_t n_classes, n_cb; float *prob; int32_t *cb, *cb_label; double *cb_conf, *clip_conf;
    /* ... or with an ensemble of n_ens models (wsa_batch_classify_ensemble): the tables of wsa_batch_copy_ensemble */
    model_box *ens_models[WSA_ENSEMBLE_MAX]; uint32_t n_ens; int ens_done; uint32_t ens_classes[WSA_ENSEMBLE_MAX]; wsa_ensemble_host eh;
} job_t;

/* the ensemble tables as a JS object: {nMembers, nClasses, prob[], cbLabel[], cbConf[], cbAllMax[], conf[] (Label_conf_all per clip / stream),
 * cb, cbDb, cbTopLabel, cbTopConf, cbMinDb, cbEntropy, minDb (per clip / stream)}; fold = 0 (level 5): nMembers, nClasses and prob only */
typedef struct {
    uint32_t n, n_rows, n_cb, n_units; const uint32_t *n_classes; int fold;
    const float *const *prob; const int32_t *const *cb_label; const double *const *cb_conf; const double *const *cb_all_max; const double *const *conf;
    const int32_t *cb, *cb_db, *cb_top_label, *cb_min_db, *min_db; const double *cb_top_conf, *cb_entropy;
} ens_view;
static napi_value make_typed(napi_env env, napi_typedarray_type type, const void *src, size_t count, size_t elt);
static napi_value ens_object(napi_env env, const ens_view *v) {
    napi_value o, nm, a_prob, a_lab, a_conf, a_max, a_acc;
    napi_create_object(env, &o);
    napi_create_uint32(env, v->n, &nm); napi_set_named_property(env, o, "nMembers", nm);
    napi_set_named_property(env, o, "nClasses", make_typed(env, napi_uint32_array, v->n_classes, v->n, 4));
    napi_create_array_with_length(env, v->n, &a_prob); napi_create_array_with_length(env, v->n, &a_lab); napi_create_array_with_length(env, v->n, &a_conf);
    napi_create_array_with_length(env, v->n, &a_max); napi_create_array_with_length(env, v->n, &a_acc);
    for (uint32_t d = 0; d < v->n; d++) {
        napi_set_element(env, a_prob, d, make_typed(env, napi_float32_array, v->prob[d], (size_t)v->n_rows * v->n_classes[d], 4));
        if (!v->fold) continue;
        napi_set_element(env, a_lab, d, make_typed(env, napi_int32_array, v->cb_label[d], v->n_cb, 4));
        napi_set_element(env, a_conf, d, make_typed(env, napi_float64_array, v->cb_conf[d], v->n_cb, 8));
        napi_set_element(env, a_max, d, make_typed(env, napi_float64_array, v->cb_all_max[d], v->n_cb, 8));
        napi_set_element(env, a_acc, d, make_typed(env, napi_float64_array, v->conf[d], (size_t)v->n_units * v->n_classes[d], 8));
    }
    napi_set_named_property(env, o, "prob", a_prob);
    if (!v->fold) return o;
    napi_set_named_property(env, o, "cbLabel", a_lab); napi_set_named_property(env, o, "cbConf", a_conf);
    napi_set_named_property(env, o, "cbAllMax", a_max); napi_set_named_property(env, o, "conf", a_acc);
    napi_set_named_property(env, o, "cb", make_typed(env, napi_int32_array, v->cb, (size_t)v->n_cb * 4, 4));
    napi_set_named_property(env, o, "cbDb", make_typed(env, napi_int32_array, v->cb_db, v->n_cb, 4));
    napi_set_named_property(env, o, "cbTopLabel", make_typed(env, napi_int32_array, v->cb_top_label, v->n_cb, 4));
    napi_set_named_property(env, o, "cbTopConf", make_typed(env, napi_float64_array, v->cb_top_conf, v->n_cb, 8));
    napi_set_named_property(env, o, "cbMinDb", make_typed(env, napi_int32_array, v->cb_min_db, v->n_cb, 4));
    napi_set_named_property(env, o, "cbEntropy", make_typed(env, napi_float64_array, v->cb_entropy, v->n_cb, 8));
    napi_set_named_property(env, o, "minDb", make_typed(env, napi_int32_array, v->min_db, v->n_units, 4));
    return o;
}
static void ens_host_free(wsa_ensemble_host *h) {
    for (int d = 0; d < WSA_ENSEMBLE_MAX; d++) { free(h->prob[d]); free(h->cb_label[d]); free(h->cb_conf[d]); free(h->cb_all_max[d]); free(h->clip_conf[d]); }
    free(h->cb); free(h->cb_db); free(h->cb_top_label); free(h->cb_top_conf); free(h->cb_min_db); free(h->cb_entropy); free(h->clip_min_db);
    memset(h, 0, sizeof *h);
}

static void job_execute(napi_env env, void *data) {
    job_t *j = (job_t *)data;
    wsa_batch *b = j->plan;
    if (!j->box->queue) {           /* (one job at a time uses a context, so nobody else looks at the box's stream now) */
        j->st = wsa_queue_create(j->ctx, &j->box->queue);
        if (j->st != WSA_OK) { snprintf(j->err, sizeof j->err, "%s", wsa_last_error(j->ctx)); return; }
    }
    j->queue = j->box->queue;
    if (!b) {
        j->st = j->fs_each ? wsa_batch_create_mixed(j->ctx, j->n_clips, j->n_samples, j->fs_each, j->fs_out, &b)
              : (j->fs_out > 0 && j->fs_out != j->fs) ? wsa_batch_create_resampled(j->ctx, j->n_clips, j->n_samples, j->fs, j->fs_out, &b)
                                                      : wsa_batch_create(j->ctx, j->n_clips, j->n_samples, j->fs, &b);
        if (j->st != WSA_OK) { snprintf(j->err, sizeof j->err, "%s", wsa_last_error(j->ctx)); return; }
        j->plan = b;
    }
    do {
        j->st = j->select ? wsa_batch_run_host_channels(b, (const void *const *)j->pcm, j->formats, j->channels, j->select, j->source, j->queue)
              : j->formats ? wsa_batch_run_host_packed(b, (const void *const *)j->pcm, j->formats, j->channels, j->queue)
              : j->is_i16 ? wsa_batch_run_host_i16(b, (const int16_t *const *)j->pcm, j->channels, j->queue) : wsa_batch_run_host(b, j->pcm, j->queue);
        if (j->st != WSA_OK) break;
        wsa_device_result r;
        j->st = wsa_batch_result(b, j->queue, &r);
        if (j->st != WSA_OK) break;
        j->n_rows = r.n_rows; j->n_segs = r.n_segments;
        j->meta = malloc(sizeof(int32_t) * 8 * (size_t)(r.n_rows ? r.n_rows : 1));
        j->feat = malloc(sizeof(double) * WSA_NFEAT * (size_t)(r.n_rows ? r.n_rows : 1));
        j->segs = malloc(sizeof(int32_t) * 4 * (size_t)(r.n_segments ? r.n_segments : 1));
        j->row_off = malloc(sizeof(uint32_t) * ((size_t)j->n_clips + 1));
        j->seg_off = malloc(sizeof(uint32_t) * ((size_t)j->n_clips + 1));
        if (!j->meta || !j->feat || !j->segs || !j->row_off || !j->seg_off) { j->st = WSA_ERR_INVALID; snprintf(j->err, sizeof j->err, "out of memory"); return; }
        j->st = wsa_batch_copy_rows(b, j->queue, j->defer_rows ? NULL : j->meta, j->defer_rows ? NULL : j->feat, r.n_rows ? r.n_rows : 1, j->segs, r.n_segments ? r.n_segments : 1, j->row_off, j->seg_off);
        if (j->st != WSA_OK) break;
        if (r.d_formants) {                                   /* levels 4 / 10: the straightened frames */
            j->n_frames = r.n_frames_total;
            j->formants = malloc(sizeof(float) * 9 * (size_t)(r.n_frames_total ? r.n_frames_total : 1));
            j->frame_off = malloc(sizeof(uint32_t) * ((size_t)j->n_clips + 1));
            if (!j->formants || !j->frame_off) { j->st = WSA_ERR_INVALID; snprintf(j->err, sizeof j->err, "out of memory"); return; }
            j->st = wsa_batch_copy_formants(b, j->queue, j->formants, r.n_frames_total ? r.n_frames_total : 1);
            if (j->st != WSA_OK) break;
            j->st = wsa_batch_copy_spectra(b, j->queue, NULL, 0, j->frame_off);
            if (j->st != WSA_OK) break;
        }
        if (r.d_utt_feat) {                                   /* level 11: utterance features after every result */
            j->n_utt = r.n_utterance_rows;
            j->utt_meta = malloc(sizeof(int32_t) * 4 * (size_t)(j->n_utt ? j->n_utt : 1));
            j->utt_feat = malloc(sizeof(double) * WSA_NUTT * (size_t)(j->n_utt ? j->n_utt : 1));
            j->utt_off = malloc(sizeof(uint32_t) * ((size_t)j->n_clips + 1));
            if (!j->utt_meta || !j->utt_feat || !j->utt_off) { j->st = WSA_ERR_INVALID; snprintf(j->err, sizeof j->err, "out of memory"); return; }
            j->st = wsa_batch_copy_utterance(b, j->queue, j->utt_meta, j->utt_feat, j->n_utt ? j->n_utt : 1, j->utt_off);
            if (j->st != WSA_OK) break;
        }
        if (j->level == 3) {                                  /* level 3: the ranked raw tracks (points + ranked ids per segment) */
            wsa_tracks_info ti;
            j->st = wsa_batch_tracks_info(b, j->queue, &ti);
            if (j->st != WSA_OK) break;
            j->trk_segs = ti.n_segments; j->trk_np = ti.n_points; j->trk_nr = ti.n_ranked;
            j->trk_off = malloc(sizeof(uint64_t) * 2 * ((size_t)ti.n_segments + 1));
            j->trk_pts = malloc(sizeof(int32_t) * 8 * (size_t)(ti.n_points ? ti.n_points : 1));
            j->trk_rank = malloc(sizeof(int32_t) * (size_t)(ti.n_ranked ? ti.n_ranked : 1));
            if (!j->trk_off || !j->trk_pts || !j->trk_rank) { j->st = WSA_ERR_INVALID; snprintf(j->err, sizeof j->err, "out of memory"); return; }
            j->st = wsa_batch_copy_tracks(b, j->queue, j->trk_off, j->trk_pts, ti.n_points, j->trk_rank, ti.n_ranked);
            if (j->st != WSA_OK) break;
        }
        if (j->model) {                                       /* K6 (+ K6b at level 13) on the batch's rows: the app's classifier */
            j->st = wsa_batch_classify(b, j->model->m, j->queue);
            if (j->st != WSA_OK) break;
            wsa_class_result cr;
            j->st = wsa_batch_class_result(b, j->queue, &cr);
            if (j->st != WSA_OK) break;
            j->n_classes = cr.n_classes; j->n_cb = cr.n_callbacks;
            j->prob = malloc(sizeof(float) * (size_t)cr.n_classes * (cr.n_rows ? cr.n_rows : 1));
            j->cb = malloc(sizeof(int32_t) * 4 * (size_t)(cr.n_callbacks ? cr.n_callbacks : 1));
            j->cb_label = malloc(sizeof(int32_t) * (size_t)(cr.n_callbacks ? cr.n_callbacks : 1));
            j->cb_conf = malloc(sizeof(double) * (size_t)(cr.n_callbacks ? cr.n_callbacks : 1));
            j->clip_conf = malloc(sizeof(double) * (size_t)cr.n_classes * (j->n_clips ? j->n_clips : 1));
            if (!j->prob || !j->cb || !j->cb_label || !j->cb_conf || !j->clip_conf) { j->st = WSA_ERR_INVALID; snprintf(j->err, sizeof j->err, "out of memory"); return; }
            memset(j->clip_conf, 0, sizeof(double) * (size_t)cr.n_classes * j->n_clips);
            j->st = wsa_batch_copy_classes(b, j->queue, j->prob, cr.n_rows ? cr.n_rows : 1, j->cb, j->cb_label, j->cb_conf, cr.n_callbacks ? cr.n_callbacks : 1, j->clip_conf);
            if (j->st != WSA_OK) break;
        }
        if (j->n_ens) {                                       /* K6e (+ K6b-e and the decision at level 13): every model DB of the app at once */
            ctx_box *bx = j->box;
            int same = bx->ens && bx->ens_n == j->n_ens;
            for (uint32_t d = 0; same && d < j->n_ens; d++) same = bx->ens_models[d] == j->ens_models[d];
            if (!same) {
                const wsa_model *ms[WSA_ENSEMBLE_MAX];
                for (uint32_t d = 0; d < j->n_ens; d++) ms[d] = j->ens_models[d]->m;
                box_drop_ensemble(bx);
                j->st = wsa_ensemble_create(j->ctx, ms, j->n_ens, &bx->ens);
                if (j->st != WSA_OK) break;
                bx->ens_n = j->n_ens; memcpy(bx->ens_models, j->ens_models, sizeof bx->ens_models);
            }
            j->st = wsa_batch_classify_ensemble(b, bx->ens, j->queue);
            if (j->st != WSA_OK) break;
            wsa_ensemble_result er;
            j->st = wsa_batch_ensemble_result(b, j->queue, &er);
            if (j->st != WSA_OK) break;
            const size_t R = er.n_rows ? er.n_rows : 1, K = er.n_callbacks ? er.n_callbacks : 1, NC = j->n_clips ? j->n_clips : 1;
            const int fold = er.d_cb != NULL;
            wsa_ensemble_host *h = &j->eh;
            int ok = 1;
            h->rows_cap = (uint32_t)R; h->cb_cap = (uint32_t)K; j->n_cb = er.n_callbacks;
            for (uint32_t d = 0; d < j->n_ens; d++) {
                j->ens_classes[d] = er.n_classes[d];
                ok = ok && (h->prob[d] = malloc(sizeof(float) * R * er.n_classes[d]));
                if (fold) ok = ok && (h->cb_label[d] = malloc(sizeof(int32_t) * K)) && (h->cb_conf[d] = malloc(sizeof(double) * K))
                               && (h->cb_all_max[d] = malloc(sizeof(double) * K)) && (h->clip_conf[d] = calloc(NC * er.n_classes[d], sizeof(double)));
            }
            if (fold) ok = ok && (h->cb = malloc(sizeof(int32_t) * 4 * K)) && (h->cb_db = malloc(sizeof(int32_t) * K)) && (h->cb_top_label = malloc(sizeof(int32_t) * K))
                           && (h->cb_top_conf = malloc(sizeof(double) * K)) && (h->cb_min_db = malloc(sizeof(int32_t) * K)) && (h->cb_entropy = malloc(sizeof(double) * K))
                           && (h->clip_min_db = malloc(sizeof(int32_t) * NC));
            if (!ok) { j->st = WSA_ERR_INVALID; snprintf(j->err, sizeof j->err, "out of memory"); return; }
            j->st = wsa_batch_copy_ensemble(b, j->queue, h);
            if (j->st != WSA_OK) break;
            j->ens_done = fold ? 2 : 1;
        }
        wsa_batch_stage_ms(b, j->stage_ms);
    } while (0);
    if (j->st != WSA_OK) snprintf(j->err, sizeof j->err, "%s", wsa_last_error(j->ctx));
    /* the plan goes back to the box in job_complete (JS thread) */
}

static napi_value make_typed(napi_env env, napi_typedarray_type type, const void *src, size_t count, size_t elt) {
    napi_value ab, ta; void *data = NULL;
    if (napi_create_arraybuffer(env, count * elt, &data, &ab) != napi_ok) return NULL;
    if (count) memcpy(data, src, count * elt);
    if (napi_create_typedarray(env, type, count, ab, 0, &ta) != napi_ok) return NULL;
    return ta;
}

/* H tables of `count` doubles each as one Float64Array [H][count] */
static napi_value make_heads(napi_env env, const double *const *src, uint32_t H, size_t count) {
    napi_value ab, ta; void *data = NULL;
    if (napi_create_arraybuffer(env, (size_t)H * count * 8, &data, &ab) != napi_ok) return NULL;
    for (uint32_t h = 0; count && h < H; h++) memcpy((double *)data + (size_t)h * count, src[h], count * 8);
    if (napi_create_typedarray(env, napi_float64_array, (size_t)H * count, ab, 0, &ta) != napi_ok) return NULL;
    return ta;
}

static void job_complete(napi_env env, napi_status status, void *data) {
    job_t *j = (job_t *)data;
    if (j->box && j->box->children) j->box->children--;
    if (j->model && j->model->busy) j->model->busy--;
    for (uint32_t d = 0; d < j->n_ens; d++) if (j->ens_models[d]->busy) j->ens_models[d]->busy--;
    if (j->plan) {                       /* keep the plan for the next call of the same shape (one entry; a failed run drops it) */
        if (j->box && j->box->ctx && j->st == WSA_OK && !j->box->plan) {
            j->box->plan = j->plan; j->box->plan_n = j->n_clips; j->box->plan_fs = j->fs; j->box->plan_fs_out = j->fs_out;
            j->box->plan_ns = j->n_samples; j->n_samples = NULL; j->box->plan_fs_each = j->fs_each; j->fs_each = NULL;
        } else wsa_batch_destroy(j->plan);
        j->plan = NULL;
    }
    for (uint32_t i = 0; i < j->n_clips; i++) napi_delete_reference(env, j->clip_refs[i]);
    if (status != napi_ok || j->st != WSA_OK) {
        napi_value msg;
        napi_create_string_utf8(env, j->st != WSA_OK ? j->err : "async work cancelled", NAPI_AUTO_LENGTH, &msg);
        napi_reject_deferred(env, j->deferred, msg);          /* the reference rejects with strings (ref @B4554) */
    } else {
        napi_value o;
        napi_create_object(env, &o);
        if (!j->defer_rows) {
            napi_set_named_property(env, o, "meta", make_typed(env, napi_int32_array, j->meta, (size_t)j->n_rows * 8, 4));
            napi_set_named_property(env, o, "feat", make_typed(env, napi_float64_array, j->feat, (size_t)j->n_rows * WSA_NFEAT, 8));
        }
        napi_set_named_property(env, o, "segments", make_typed(env, napi_int32_array, j->segs, (size_t)j->n_segs * 4, 4));
        napi_set_named_property(env, o, "rowOff", make_typed(env, napi_uint32_array, j->row_off, (size_t)j->n_clips + 1, 4));
        napi_set_named_property(env, o, "segOff", make_typed(env, napi_uint32_array, j->seg_off, (size_t)j->n_clips + 1, 4));
        napi_set_named_property(env, o, "stageMs", make_typed(env, napi_float32_array, j->stage_ms, 4, 4));
        if (j->utt_feat) {
            napi_set_named_property(env, o, "uttMeta", make_typed(env, napi_int32_array, j->utt_meta, (size_t)j->n_utt * 4, 4));
            napi_set_named_property(env, o, "uttFeat", make_typed(env, napi_float64_array, j->utt_feat, (size_t)j->n_utt * WSA_NUTT, 8));
            napi_set_named_property(env, o, "uttOff", make_typed(env, napi_uint32_array, j->utt_off, (size_t)j->n_clips + 1, 4));
        }
        if (j->trk_off) {
            /* offsets as doubles (exact below 2^53): [n_segments + 1][2] = first point / first ranked id of a segment */
            const size_t n = 2 * ((size_t)j->trk_segs + 1);
            double *od = malloc(sizeof(double) * n);
            for (size_t i = 0; i < n; i++) od[i] = (double)j->trk_off[i];
            napi_set_named_property(env, o, "trackOff", make_typed(env, napi_float64_array, od, n, 8));
            free(od);
            napi_set_named_property(env, o, "trackPoints", make_typed(env, napi_int32_array, j->trk_pts, (size_t)j->trk_np * 8, 4));
            napi_set_named_property(env, o, "trackRanked", make_typed(env, napi_int32_array, j->trk_rank, (size_t)j->trk_nr, 4));
        }
        if (j->formants) {
            napi_set_named_property(env, o, "formants", make_typed(env, napi_float32_array, j->formants, (size_t)j->n_frames * 9, 4));
            napi_set_named_property(env, o, "frameOff", make_typed(env, napi_uint32_array, j->frame_off, (size_t)j->n_clips + 1, 4));
        }
        if (j->prob) {                    /* the classifier's tables (include/wsa.h wsa_batch_copy_classes) */
            napi_value nc; napi_create_uint32(env, j->n_classes, &nc); napi_set_named_property(env, o, "nClasses", nc);
            napi_set_named_property(env, o, "prob", make_typed(env, napi_float32_array, j->prob, (size_t)j->n_rows * j->n_classes, 4));
            napi_set_named_property(env, o, "cb", make_typed(env, napi_int32_array, j->cb, (size_t)j->n_cb * 4, 4));
            napi_set_named_property(env, o, "cbLabel", make_typed(env, napi_int32_array, j->cb_label, (size_t)j->n_cb, 4));
            napi_set_named_property(env, o, "cbConf", make_typed(env, napi_float64_array, j->cb_conf, (size_t)j->n_cb, 8));
            napi_set_named_property(env, o, "clipConf", make_typed(env, napi_float64_array, j->clip_conf, (size_t)j->n_clips * j->n_classes, 8));
        }
        if (j->ens_done) {                /* the ensemble's tables (include/wsa.h wsa_batch_copy_ensemble) */
            const wsa_ensemble_host *h = &j->eh;
            const ens_view v = {j->n_ens, j->n_rows, j->n_cb, j->n_clips, j->ens_classes, j->ens_done == 2,
                                (const float *const *)h->prob, (const int32_t *const *)h->cb_label, (const double *const *)h->cb_conf, (const double *const *)h->cb_all_max,
                                (const double *const *)h->clip_conf, h->cb, h->cb_db, h->cb_top_label, h->cb_min_db, h->clip_min_db, h->cb_top_conf, h->cb_entropy};
            napi_set_named_property(env, o, "ens", ens_object(env, &v));
        }
        napi_resolve_deferred(env, j->deferred, o);
    }
    napi_delete_async_work(env, j->work);
    ens_host_free(&j->eh);
    free(j->prob); free(j->cb); free(j->cb_label); free(j->cb_conf); free(j->clip_conf);
    free(j->meta); free(j->feat); free(j->segs); free(j->row_off); free(j->seg_off); free(j->formants); free(j->frame_off); free(j->utt_meta); free(j->utt_feat); free(j->utt_off); free(j->trk_off); free(j->trk_pts); free(j->trk_rank);
    free(j->n_samples); free(j->fs_each); free((void *)j->pcm); free(j->clip_refs); free(j->channels); free(j->formats); free(j->select); free(j);
}

static napi_value fn_process_batch(napi_env env, napi_callback_info info) {
    size_t argc = 11; napi_value argv[11];
    NAPI_OK(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
    wsa_ctx *ctx = argc ? get_ctx(env, argv[0]) : NULL;
    bool is_arr = false; double fs = 0; uint32_t n = 0;
    model_box *mb = NULL;                                        /* 8th argument: a model of modelCreate on this context (classify the rows), an array of 1 .. 8 of them (an ensemble), or undefined / null */
    model_box *ens_models[WSA_ENSEMBLE_MAX] = {0}; uint32_t n_ens = 0;
    bool ens_arr = false;
    if (argc >= 8 && napi_is_array(env, argv[7], &ens_arr) == napi_ok && ens_arr) {
        uint32_t len = 0;
        napi_get_array_length(env, argv[7], &len);
        if (len < 1 || len > WSA_ENSEMBLE_MAX) { napi_throw_error(env, NULL, "processBatch: an ensemble has 1 .. 8 models"); return NULL; }
        for (uint32_t d = 0; d < len; d++) {
            napi_value el; napi_valuetype t = napi_undefined; void *p = NULL;
            if (napi_get_element(env, argv[7], d, &el) != napi_ok || napi_typeof(env, el, &t) != napi_ok || t != napi_external || napi_get_value_external(env, el, &p) != napi_ok || !p || !((model_box *)p)->m) {
                napi_throw_error(env, NULL, "processBatch: a model handle of the ensemble was destroyed (or is not a model)"); return NULL;
            }
            if (!ctx || ((model_box *)p)->owner != get_box(env, argv[0])) { napi_throw_error(env, NULL, "processBatch: a model of the ensemble belongs to another context"); return NULL; }
            ens_models[d] = (model_box *)p;
        }
        n_ens = len;
    } else if (argc >= 8) {
        napi_valuetype t; napi_typeof(env, argv[7], &t);
        if (t != napi_undefined && t != napi_null) {
            void *p = NULL;
            if (t != napi_external || napi_get_value_external(env, argv[7], &p) != napi_ok || !((model_box *)p)->m) { napi_throw_error(env, NULL, "processBatch: the model handle was destroyed (or is not a model)"); return NULL; }
            mb = (model_box *)p;
            if (!ctx || mb->owner != get_box(env, argv[0])) { napi_throw_error(env, NULL, "processBatch: the model belongs to another context"); return NULL; }
        }
    }
    /* fs: a number, or a Float64Array with one rate per clip (the clips are then converted to analysisRate, each from its own rate) */
    double *fs_each = NULL; size_t fs_each_n = 0; bool fs_ok = false;
    if (argc >= 3) {
        bool ta = false; napi_typedarray_type ft; void *fd = NULL;
        if (napi_get_value_double(env, argv[2], &fs) == napi_ok) fs_ok = true;
        else if (napi_is_typedarray(env, argv[2], &ta) == napi_ok && ta && napi_get_typedarray_info(env, argv[2], &ft, &fs_each_n, &fd, NULL, NULL) == napi_ok && ft == napi_float64_array) { fs_each = (double *)fd; fs_ok = true; fs = 0; }
    }
    if (!ctx || argc < 3 || napi_is_array(env, argv[1], &is_arr) != napi_ok || !is_arr ||
        !fs_ok || napi_get_array_length(env, argv[1], &n) != napi_ok || (fs_each && fs_each_n != n)) {
        napi_throw_type_error(env, NULL, "processBatch(ctx, Float32Array[] | Int16Array[], fs[, level[, analysisRate[, channels[, deferRows]]]])"); return NULL;
    }
    job_t *j = calloc(1, sizeof *j);
    if (!j) { napi_throw_error(env, NULL, "out of memory"); return NULL; }
    if (argc >= 7) { bool d = false; if (napi_get_value_bool(env, argv[6], &d) == napi_ok) j->defer_rows = d ? 1 : 0; }
    j->ctx = ctx; j->fs = fs; j->n_clips = n; j->box = get_box(env, argv[0]); j->model = mb;
    j->n_ens = n_ens; memcpy(j->ens_models, ens_models, sizeof j->ens_models);
    if (fs_each) { j->fs_each = malloc(sizeof(double) * (n ? n : 1)); if (!j->fs_each) { free(j); napi_throw_error(env, NULL, "out of memory"); return NULL; } memcpy(j->fs_each, fs_each, sizeof(double) * n); }
    if (argc >= 4) { int32_t lv = 0; if (napi_get_value_int32(env, argv[3], &lv) == napi_ok) j->level = lv; }
    if (argc >= 5) { double fo = 0; if (napi_get_value_double(env, argv[4], &fo) == napi_ok) j->fs_out = fo; }           /* analysis rate */   /* the ctx's output_level: 3 adds the raw tracks */
    j->n_samples = calloc(n ? n : 1, sizeof(uint32_t)); j->pcm = calloc(n ? n : 1, sizeof(float *)); j->clip_refs = calloc(n ? n : 1, sizeof(napi_ref));
    if (!j->n_samples || !j->pcm || !j->clip_refs) { free(j->n_samples); free(j->fs_each); free((void *)j->pcm); free(j->clip_refs); free(j); napi_throw_error(env, NULL, "out of memory"); return NULL; }
    /* clips: all Float32Array (mono floats) or all Int16Array (16-bit PCM as a WAV file holds it, interleaved over channels[i] channels
     * given by the optional 6th argument, a Uint32Array; channel 0 is analysed and the conversion runs on the device) */
    uint32_t *chan = NULL; size_t chan_len = 0;
    if (argc >= 6) {
        napi_typedarray_type ct; void *cd = NULL; bool cta = false;
        if (napi_is_typedarray(env, argv[5], &cta) == napi_ok && cta && napi_get_typedarray_info(env, argv[5], &ct, &chan_len, &cd, NULL, NULL) == napi_ok && ct == napi_uint32_array) chan = (uint32_t *)cd;
    }
    /* ... or, with a 9th argument (an Int32Array of WSA_PCM_* numbers, one per clip): every clip a Uint8Array over the bytes a file holds, clip i in
     * formats[i] and interleaved over channels[i] channels — any mix of encodings in one batch, unpacked on the device (spec PK-2) */
    if (argc >= 9) {
        napi_typedarray_type ft; void *fd = NULL; bool fta = false; size_t fl = 0; napi_valuetype vt = napi_undefined;
        napi_typeof(env, argv[8], &vt);
        if (vt != napi_undefined && vt != napi_null) {
            if (napi_is_typedarray(env, argv[8], &fta) != napi_ok || !fta || napi_get_typedarray_info(env, argv[8], &ft, &fl, &fd, NULL, NULL) != napi_ok || ft != napi_int32_array || fl != n) {
                free(j->n_samples); free(j->fs_each); free((void *)j->pcm); free(j->clip_refs); free(j);
                napi_throw_type_error(env, NULL, "processBatch: formats is an Int32Array with one WSA_PCM_* number per clip"); return NULL;
            }
            j->formats = malloc(sizeof(int32_t) * (n ? n : 1)); j->channels = calloc(n ? n : 1, sizeof(uint32_t));
            if (!j->formats || !j->channels) { free(j->n_samples); free(j->fs_each); free((void *)j->pcm); free(j->clip_refs); free(j->channels); free(j->formats); free(j); napi_throw_error(env, NULL, "out of memory"); return NULL; }
            memcpy(j->formats, fd, sizeof(int32_t) * n);
        }
    }
    /* ... and with a 10th and an 11th (Uint32Arrays, one word per clip): what each clip takes of which clip's bytes (spec PK-3).  A consumer's entry of
     * the clip array is its source's Uint8Array (its length gives the frames; the library does not read a consumer's pointer) */
    if (argc >= 11 && j->formats) {
        napi_typedarray_type st, ut; void *sd = NULL, *ud = NULL; bool sta = false, uta = false; size_t sl = 0, ul = 0; napi_valuetype vt = napi_undefined;
        napi_typeof(env, argv[9], &vt);
        if (vt != napi_undefined && vt != napi_null) {
            if (napi_is_typedarray(env, argv[9], &sta) != napi_ok || !sta || napi_get_typedarray_info(env, argv[9], &st, &sl, &sd, NULL, NULL) != napi_ok || st != napi_uint32_array || sl != n
                || napi_is_typedarray(env, argv[10], &uta) != napi_ok || !uta || napi_get_typedarray_info(env, argv[10], &ut, &ul, &ud, NULL, NULL) != napi_ok || ut != napi_uint32_array || ul != n) {
                free(j->n_samples); free(j->fs_each); free((void *)j->pcm); free(j->clip_refs); free(j->channels); free(j->formats); free(j);
                napi_throw_type_error(env, NULL, "processBatch: select and source are Uint32Arrays with one word per clip"); return NULL;
            }
            j->select = malloc(sizeof(uint32_t) * 2 * (n ? n : 1));
            if (!j->select) { free(j->n_samples); free(j->fs_each); free((void *)j->pcm); free(j->clip_refs); free(j->channels); free(j->formats); free(j); napi_throw_error(env, NULL, "out of memory"); return NULL; }
            j->source = j->select + (n ? n : 1);
            memcpy(j->select, sd, sizeof(uint32_t) * n); memcpy(j->source, ud, sizeof(uint32_t) * n);
        }
    }
    for (uint32_t i = 0; i < n; i++) {
        napi_value el; napi_typedarray_type tt; size_t len; void *data; bool is_ta = false;
        const char *bad = NULL;
        if (j->formats) {
            const int32_t f = j->formats[i];
            const uint32_t sb = (f == WSA_PCM_F32 || f == WSA_PCM_I32) ? 4u : f == WSA_PCM_I16 ? 2u : f == WSA_PCM_I24 ? 3u : f == WSA_PCM_F64 ? 8u
                              : (f == WSA_PCM_MULAW || f == WSA_PCM_ALAW || f == WSA_PCM_U8) ? 1u : 0u;
            const uint32_t ch = (chan && i < chan_len) ? chan[i] : 1;
            if (napi_get_element(env, argv[1], i, &el) != napi_ok || napi_is_typedarray(env, el, &is_ta) != napi_ok || !is_ta ||
                napi_get_typedarray_info(env, el, &tt, &len, &data, NULL, NULL) != napi_ok || tt != napi_uint8_array) bad = "with formats every clip must be a Uint8Array over the file's bytes";
            else if (!sb) bad = "processBatch: unknown input format";
            else if (ch < 1 || ch > 64) bad = "processBatch: channels must be 1 .. 64";
            if (!bad) {
                j->channels[i] = ch; j->n_samples[i] = (uint32_t)(len / ((size_t)sb * ch)); j->pcm[i] = (const float *)data;
                napi_create_reference(env, el, 1, &j->clip_refs[i]);
                continue;
            }
        }
        else if (napi_get_element(env, argv[1], i, &el) != napi_ok || napi_is_typedarray(env, el, &is_ta) != napi_ok || !is_ta ||
            napi_get_typedarray_info(env, el, &tt, &len, &data, NULL, NULL) != napi_ok || (tt != napi_float32_array && tt != napi_int16_array)) bad = "every clip must be a Float32Array or an Int16Array";
        else if (i > 0 && (tt == napi_int16_array) != (j->is_i16 != 0)) bad = "the clips of one batch must be of one kind";
        if (bad) {
            for (uint32_t k = 0; k < i; k++) napi_delete_reference(env, j->clip_refs[k]);
            free(j->n_samples); free(j->fs_each); free((void *)j->pcm); free(j->clip_refs); free(j->channels); free(j->formats); free(j->select); free(j);
            napi_throw_type_error(env, NULL, bad); return NULL;
        }
        if (i == 0) { j->is_i16 = tt == napi_int16_array; if (j->is_i16) j->channels = calloc(n, sizeof(uint32_t)); }
        uint32_t ch = 1;
        if (j->is_i16) { ch = (chan && i < chan_len && chan[i] >= 1) ? chan[i] : 1; j->channels[i] = ch; }
        j->n_samples[i] = (uint32_t)(len / ch); j->pcm[i] = (const float *)data;
        napi_create_reference(env, el, 1, &j->clip_refs[i]);      /* keep the PCM alive while the worker reads it */
    }
    /* a plan of exactly this shape waiting in the box?  (one job at a time uses a context: the plan leaves the box while it runs) */
    if (j->box->plan) {
        int same = j->box->plan_n == n && j->box->plan_fs == j->fs && j->box->plan_fs_out == j->fs_out && (j->box->plan_fs_each != NULL) == (j->fs_each != NULL);
        for (uint32_t i = 0; same && i < n; i++) same = j->box->plan_ns[i] == j->n_samples[i] && (!j->fs_each || j->box->plan_fs_each[i] == j->fs_each[i]);
        if (same) { j->plan = j->box->plan; j->plan_reused = 1; j->box->plan = NULL; free(j->box->plan_ns); free(j->box->plan_fs_each); j->box->plan_ns = NULL; j->box->plan_fs_each = NULL; j->box->plan_n = 0; }
        else box_drop_plan(j->box);
    }
    napi_value promise, name;
    NAPI_OK(env, napi_create_promise(env, &j->deferred, &promise));
    NAPI_OK(env, napi_create_string_utf8(env, "wsa.processBatch", NAPI_AUTO_LENGTH, &name));
    NAPI_OK(env, napi_create_async_work(env, NULL, name, job_execute, job_complete, j, &j->work));
    NAPI_OK(env, napi_queue_async_work(env, j->work));
    j->box->children++;                                          /* until job_complete */
    if (mb) mb->busy++;
    for (uint32_t d = 0; d < n_ens; d++) ens_models[d]->busy++;
    return promise;
}

/* ---- gatherRows: the rows of the contexts' last batches (processBatch(..., deferRows = true)) collected on the first context's device by one
 * RCCL exchange (wsa_gather_rows) and copied to the host once; resolves {meta, feat, rowsPerRank} ---- */
typedef struct {
    napi_async_work work; napi_deferred deferred;
    uint32_t n; ctx_box **boxes; wsa_ctx **ctxs; wsa_batch **plans;
    wsa_status st; char err[512];
    uint32_t n_rows; uint32_t *per; int32_t *meta; double *feat;
} gjob_t;
static void gjob_execute_locked(gjob_t *j);
static void gjob_execute(napi_env env, void *data) {
    pthread_mutex_lock(&g_gather_lock);
    gjob_execute_locked((gjob_t *)data);
    pthread_mutex_unlock(&g_gather_lock);
}
static void gjob_execute_locked(gjob_t *j) {
    int same = g_gather && g_gather_n == j->n;
    for (uint32_t i = 0; same && i < j->n; i++) same = g_gather_ctxs[i] == j->ctxs[i];
    if (!same) {
        gather_drop();
        j->st = wsa_gather_create(j->ctxs, (int32_t)j->n, 0, &g_gather);
        if (j->st != WSA_OK) { snprintf(j->err, sizeof j->err, "%s", wsa_last_error(j->ctxs[0])); g_gather = NULL; return; }
        g_gather_ctxs = malloc(sizeof(wsa_ctx *) * j->n); g_gather_n = j->n;
        if (!g_gather_ctxs) { gather_drop(); j->st = WSA_ERR_INVALID; snprintf(j->err, sizeof j->err, "out of memory"); return; }
        memcpy(g_gather_ctxs, j->ctxs, sizeof(wsa_ctx *) * j->n);
    }
    wsa_gather_result r;
    j->st = wsa_gather_rows(g_gather, j->plans, NULL, &r);
    if (j->st == WSA_OK) {
        j->n_rows = r.n_rows;
        j->per = malloc(sizeof(uint32_t) * j->n);
        j->meta = malloc(sizeof(int32_t) * 8 * (size_t)(r.n_rows ? r.n_rows : 1));
        j->feat = malloc(sizeof(double) * WSA_NFEAT * (size_t)(r.n_rows ? r.n_rows : 1));
        if (!j->per || !j->meta || !j->feat) { j->st = WSA_ERR_INVALID; snprintf(j->err, sizeof j->err, "out of memory"); return; }
        memcpy(j->per, r.rows_per_rank, sizeof(uint32_t) * j->n);
        j->st = wsa_gather_copy_rows(g_gather, j->meta, j->feat, r.n_rows ? r.n_rows : 1);
    }
    if (j->st != WSA_OK) { snprintf(j->err, sizeof j->err, "%s", wsa_last_error(j->ctxs[0])); gather_drop(); }      /* a failed exchange leaves the communicators unusable: the next job builds new ones */
}
static void gjob_complete(napi_env env, napi_status status, void *data) {
    gjob_t *j = (gjob_t *)data;
    for (uint32_t i = 0; i < j->n; i++) if (j->boxes[i]->children) j->boxes[i]->children--;
    if (status != napi_ok || j->st != WSA_OK) {
        napi_value msg;
        napi_create_string_utf8(env, j->st != WSA_OK ? j->err : "async work cancelled", NAPI_AUTO_LENGTH, &msg);
        napi_reject_deferred(env, j->deferred, msg);
    } else {
        napi_value o; napi_create_object(env, &o);
        napi_set_named_property(env, o, "meta", make_typed(env, napi_int32_array, j->meta, (size_t)j->n_rows * 8, 4));
        napi_set_named_property(env, o, "feat", make_typed(env, napi_float64_array, j->feat, (size_t)j->n_rows * WSA_NFEAT, 8));
        napi_set_named_property(env, o, "rowsPerRank", make_typed(env, napi_uint32_array, j->per, j->n, 4));
        napi_resolve_deferred(env, j->deferred, o);
    }
    napi_delete_async_work(env, j->work);
    free(j->per); free(j->meta); free(j->feat); free(j->boxes); free(j->ctxs); free(j->plans); free(j);
}
static napi_value fn_gather_rows(napi_env env, napi_callback_info info) {
    size_t argc = 1; napi_value argv[1];
    NAPI_OK(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
    bool is_arr = false; uint32_t n = 0;
    if (argc < 1 || napi_is_array(env, argv[0], &is_arr) != napi_ok || !is_arr || napi_get_array_length(env, argv[0], &n) != napi_ok || n < 1) {
        napi_throw_type_error(env, NULL, "gatherRows(ctx[])"); return NULL;
    }
    gjob_t *j = calloc(1, sizeof *j);
    if (j) { j->n = n; j->boxes = calloc(n, sizeof(ctx_box *)); j->ctxs = calloc(n, sizeof(wsa_ctx *)); j->plans = calloc(n, sizeof(wsa_batch *)); }
    if (!j || !j->boxes || !j->ctxs || !j->plans) { if (j) { free(j->boxes); free(j->ctxs); free(j->plans); free(j); } napi_throw_error(env, NULL, "out of memory"); return NULL; }
    for (uint32_t i = 0; i < n; i++) {
        napi_value el;
        ctx_box *b = napi_get_element(env, argv[0], i, &el) == napi_ok ? get_box(env, el) : NULL;
        if (!b || !b->ctx || !b->plan) {       /* the rows to collect are those of the plan the context's last processBatch left in its box */
            free(j->boxes); free(j->ctxs); free(j->plans); free(j);
            napi_throw_error(env, NULL, "gatherRows: every context needs a finished processBatch(..., deferRows = true)"); return NULL;
        }
        j->boxes[i] = b; j->ctxs[i] = b->ctx; j->plans[i] = b->plan;
    }
    napi_value promise, name;
    NAPI_OK(env, napi_create_promise(env, &j->deferred, &promise));
    NAPI_OK(env, napi_create_string_utf8(env, "wsa.gatherRows", NAPI_AUTO_LENGTH, &name));
    NAPI_OK(env, napi_create_async_work(env, NULL, name, gjob_execute, gjob_complete, j, &j->work));
    NAPI_OK(env, napi_queue_async_work(env, j->work));
    for (uint32_t i = 0; i < n; i++) j->boxes[i]->children++;      /* the contexts (and their plans) stay until gjob_complete */
    return promise;
}

/* ---- streams ---- */
typedef struct { wsa_stream *st; wsa_ctx *ctx; ctx_box *box; uint32_t n, sps; int32_t fmt; napi_ref input_ref; model_box *model; wsa_ensemble *ens; model_box *ens_models[WSA_ENSEMBLE_MAX]; uint32_t n_ens; struct knn_box *knn; wsa_regress_group *reg; model_box *reg_models[WSA_REGRESS_GROUP_MAX]; uint32_t n_reg; } stream_t;   /* input_ref: the ArrayBuffer over the pinned input, detached at close; model: attached classifier (holds its busy count) */
static void stream_finalize(napi_env env, void *data, void *hint) { /* explicit streamClose() only */ }
static stream_t *get_stream(napi_env env, napi_value v) {
    void *p = NULL; if (napi_get_value_external(env, v, &p) != napi_ok) return NULL; return (stream_t *)p;
}
static napi_value fn_stream_open(napi_env env, napi_callback_info info) {
    size_t argc = 5; napi_value argv[5]; double fs = 0; uint32_t n = 0, fps = 1, span = 1024;
    NAPI_OK(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
    wsa_ctx *ctx = argc ? get_ctx(env, argv[0]) : NULL;
    if (!ctx || argc < 3 || napi_get_value_uint32(env, argv[1], &n) != napi_ok || napi_get_value_double(env, argv[2], &fs) != napi_ok) {
        napi_throw_type_error(env, NULL, "streamOpen(ctx, nStreams, fs, framesPerStep, maxSpanFrames)"); return NULL;
    }
    if (argc > 3) napi_get_value_uint32(env, argv[3], &fps);
    if (argc > 4) napi_get_value_uint32(env, argv[4], &span);
    stream_t *h = calloc(1, sizeof *h);
    h->ctx = ctx; h->n = n; h->box = get_box(env, argv[0]);
    if (wsa_stream_create(ctx, n, fs, fps, span, &h->st) != WSA_OK) { free(h); napi_throw_error(env, NULL, wsa_last_error(ctx)); return NULL; }
    h->box->children++;                                          /* until streamClose */
    wsa_stream_enable_graph(h->st, 1);
    h->sps = wsa_stream_input_stride(h->st);                     /* (a plain set: samples_per_step) */
    napi_value ext; NAPI_OK(env, napi_create_external(env, h, stream_finalize, NULL, &ext));
    return ext;
}
static napi_value fn_stream_open_mixed(napi_env env, napi_callback_info info) {
    size_t argc = 6; napi_value argv[6]; double fs_out = 0; uint32_t n = 0, fps = 1, span = 1024;
    NAPI_OK(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
    wsa_ctx *ctx = argc ? get_ctx(env, argv[0]) : NULL;
    bool is_ta = false; napi_typedarray_type tt = napi_int8_array; size_t len = 0; void *data = NULL;
    if (!ctx || argc < 4 || napi_get_value_uint32(env, argv[1], &n) != napi_ok || napi_is_typedarray(env, argv[2], &is_ta) != napi_ok || !is_ta
        || napi_get_typedarray_info(env, argv[2], &tt, &len, &data, NULL, NULL) != napi_ok || tt != napi_float64_array || len != n
        || napi_get_value_double(env, argv[3], &fs_out) != napi_ok) {
        napi_throw_type_error(env, NULL, "streamOpenMixed(ctx, nStreams, rates: Float64Array(nStreams), fsOut, framesPerStep, maxSpanFrames)"); return NULL;
    }
    if (argc > 4) napi_get_value_uint32(env, argv[4], &fps);
    if (argc > 5) napi_get_value_uint32(env, argv[5], &span);
    stream_t *h = calloc(1, sizeof *h);
    h->ctx = ctx; h->n = n; h->box = get_box(env, argv[0]);
    if (wsa_stream_create_mixed(ctx, n, (const double *)data, fs_out, fps, span, &h->st) != WSA_OK) { free(h); napi_throw_error(env, NULL, wsa_last_error(ctx)); return NULL; }
    h->box->children++;
    wsa_stream_enable_graph(h->st, 1);
    h->sps = wsa_stream_input_stride(h->st);
    napi_value ext; NAPI_OK(env, napi_create_external(env, h, stream_finalize, NULL, &ext));
    return ext;
}
static napi_value fn_stream_info(napi_env env, napi_callback_info info) {
    size_t argc = 1; napi_value argv[1];
    NAPI_OK(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
    stream_t *h = argc ? get_stream(env, argv[0]) : NULL;
    if (!h || !h->st) { napi_throw_type_error(env, NULL, "streamInfo(stream)"); return NULL; }
    uint32_t *cap = malloc(sizeof(uint32_t) * (h->n ? h->n : 1));
    for (uint32_t i = 0; i < h->n; i++) cap[i] = wsa_stream_input_capacity(h->st, i);
    napi_value o, v;
    napi_create_object(env, &o);
    napi_set_named_property(env, o, "capacity", make_typed(env, napi_uint32_array, cap, (size_t)h->n, 4));
    free(cap);
    napi_create_uint32(env, wsa_stream_input_stride(h->st), &v); napi_set_named_property(env, o, "inputStride", v);
    napi_create_uint32(env, wsa_stream_samples_per_step(h->st), &v); napi_set_named_property(env, o, "samplesPerStep", v);
    napi_create_uint32(env, wsa_stream_input_stride_bytes(h->st), &v); napi_set_named_property(env, o, "inputStrideBytes", v);
    return o;
}
/* streamSetInput(stream, format 0 .. 3, channels: Uint32Array(nStreams) | null[, select, source: Uint32Array(nStreams) | null]): wsa_stream_set_input_format, or with
 * a select or a source wsa_stream_set_input_channels (spec PK-3); before the first streamInput */
static napi_value fn_stream_set_input(napi_env env, napi_callback_info info) {
    size_t argc = 5; napi_value argv[5]; int32_t fmt = 0;
    NAPI_OK(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
    stream_t *h = argc ? get_stream(env, argv[0]) : NULL;
    if (!h || !h->st || argc < 2 || napi_get_value_int32(env, argv[1], &fmt) != napi_ok) { napi_throw_type_error(env, NULL, "streamSetInput(stream, format, channels)"); return NULL; }
    if (h->input_ref) { napi_throw_error(env, NULL, "streamSetInput: the input buffer of this stream object has been handed out already"); return NULL; }
    const uint32_t *chan = NULL;
    if (argc > 2) {
        bool is_ta = false; napi_typedarray_type tt; size_t len; void *data;
        if (napi_is_typedarray(env, argv[2], &is_ta) == napi_ok && is_ta) {
            if (napi_get_typedarray_info(env, argv[2], &tt, &len, &data, NULL, NULL) != napi_ok || tt != napi_uint32_array || len != h->n) {
                napi_throw_type_error(env, NULL, "channels must be a Uint32Array with one count per stream"); return NULL;
            }
            chan = (const uint32_t *)data;
        }
    }
    const uint32_t *ss[2] = {NULL, NULL};
    for (size_t a = 3; a < argc && a < 5; a++) {
        bool is_ta = false; napi_typedarray_type tt; size_t len; void *data;
        if (napi_is_typedarray(env, argv[a], &is_ta) == napi_ok && is_ta) {
            if (napi_get_typedarray_info(env, argv[a], &tt, &len, &data, NULL, NULL) != napi_ok || tt != napi_uint32_array || len != h->n) {
                napi_throw_type_error(env, NULL, "select and source must be Uint32Arrays with one word per stream"); return NULL;
            }
            ss[a - 3] = (const uint32_t *)data;
        }
    }
    const wsa_status sst = (ss[0] || ss[1]) ? wsa_stream_set_input_channels(h->st, fmt, chan, ss[0], ss[1]) : wsa_stream_set_input_format(h->st, fmt, chan);
    if (sst != WSA_OK) { napi_throw_error(env, NULL, wsa_last_error(h->ctx)); return NULL; }
    h->fmt = fmt;
    return NULL;
}
/* decodePcm(format, typedArray, channels[, select]) -> Float32Array: wsa_pcm_decode_select, channel `select` (0; 0xFFFFFFFF: the mix) of the interleaved frames
 * (specs PK-1 / PK-3, no device) */
static napi_value fn_decode_pcm(napi_env env, napi_callback_info info) {
    size_t argc = 4; napi_value argv[4]; int32_t fmt = 0; uint32_t ch = 1, sel = 0;
    NAPI_OK(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
    bool is_ta = false; napi_typedarray_type tt = napi_int8_array; size_t len = 0; void *data = NULL;
    if (argc < 2 || napi_get_value_int32(env, argv[0], &fmt) != napi_ok || napi_is_typedarray(env, argv[1], &is_ta) != napi_ok || !is_ta
        || napi_get_typedarray_info(env, argv[1], &tt, &len, &data, NULL, NULL) != napi_ok) {
        napi_throw_type_error(env, NULL, "decodePcm(format, typedArray, channels)"); return NULL;
    }
    if (argc > 2) napi_get_value_uint32(env, argv[2], &ch);
    const napi_typedarray_type want = fmt == WSA_PCM_F32 ? napi_float32_array : fmt == WSA_PCM_I16 ? napi_int16_array : napi_uint8_array;
    if (fmt < WSA_PCM_F32 || fmt > WSA_PCM_ALAW) { napi_throw_error(env, NULL, "decodePcm: unknown input format"); return NULL; }
    if (tt != want) { napi_throw_type_error(env, NULL, "decodePcm: f32 takes a Float32Array, i16 an Int16Array, mulaw / alaw a Uint8Array"); return NULL; }
    if (ch < 1 || ch > 64) { napi_throw_error(env, NULL, "decodePcm: channel count outside 1 .. 64"); return NULL; }
    if (argc > 3) napi_get_value_uint32(env, argv[3], &sel);
    if (sel >= ch && sel != WSA_CHANNEL_MIX) { napi_throw_error(env, NULL, "decodePcm: select is neither a channel below the channel count nor the mix"); return NULL; }
    const size_t last = sel == WSA_CHANNEL_MIX ? ch - 1u : sel;           /* the last channel of a frame that is read */
    const size_t frames = len > last ? (len - 1 - last) / ch + 1 : 0;
    napi_value ab, ta; void *out = NULL;
    NAPI_OK(env, napi_create_arraybuffer(env, frames * sizeof(float), &out, &ab));
    if (wsa_pcm_decode_select(fmt, data, frames, ch, sel, (float *)out) != WSA_OK) { napi_throw_error(env, NULL, "decodePcm: refused"); return NULL; }
    NAPI_OK(env, napi_create_typedarray(env, napi_float32_array, frames, ab, 0, &ta));
    return ta;
}
static napi_value fn_stream_paced(napi_env env, napi_callback_info info) {
    size_t argc = 1; napi_value argv[1];
    NAPI_OK(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
    stream_t *h = argc ? get_stream(env, argv[0]) : NULL;
    if (!h || !h->st) { napi_throw_type_error(env, NULL, "streamPaced(stream)"); return NULL; }
    uint32_t *cnt = malloc(sizeof(uint32_t) * (h->n ? h->n : 1));
    for (uint32_t i = 0; i < h->n; i++) cnt[i] = wsa_stream_paced_input(h->st, i);
    napi_value ta = make_typed(env, napi_uint32_array, cnt, (size_t)h->n, 4);
    free(cnt);
    return ta;
}
static napi_value fn_stream_input(napi_env env, napi_callback_info info) {
    size_t argc = 1; napi_value argv[1];
    NAPI_OK(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
    stream_t *h = argc ? get_stream(env, argv[0]) : NULL;
    if (!h || !h->st) { napi_throw_type_error(env, NULL, "streamInput(stream)"); return NULL; }
    /* a packed format (streamSetInput): the Int16Array / Uint8Array over the pinned packed buffer, [nStreams][inputStrideBytes / element size] */
    void *packed = wsa_stream_host_input_packed(h->st);
    const size_t elt = !packed ? sizeof(float) : h->fmt == WSA_PCM_I16 ? 2 : 1;
    const size_t count = packed ? (size_t)h->n * wsa_stream_input_stride_bytes(h->st) / elt : (size_t)h->n * h->sps;
    napi_value ab, ta;
    if (h->input_ref) {                      /* one ArrayBuffer per stream object: hand the same one out again */
        NAPI_OK(env, napi_get_reference_value(env, h->input_ref, &ab));
    } else {
        NAPI_OK(env, napi_create_external_arraybuffer(env, packed ? packed : (void *)wsa_stream_host_input(h->st), count * elt, NULL, NULL, &ab));
        NAPI_OK(env, napi_create_reference(env, ab, 1, &h->input_ref));
    }
    NAPI_OK(env, napi_create_typedarray(env, !packed ? napi_float32_array : h->fmt == WSA_PCM_I16 ? napi_int16_array : napi_uint8_array, count, ab, 0, &ta));
    return ta;
}
static napi_value fn_stream_step(napi_env env, napi_callback_info info) {
    size_t argc = 3; napi_value argv[3];
    NAPI_OK(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
    stream_t *h = argc ? get_stream(env, argv[0]) : NULL;
    if (!h || !h->st) { napi_throw_type_error(env, NULL, "streamStep(stream, ctl[, counts])"); return NULL; }
    const uint8_t *ctl = NULL;
    const uint32_t *counts = NULL;
    if (argc > 2) {
        bool is_ta = false; napi_typedarray_type tt; size_t len; void *data;
        if (napi_is_typedarray(env, argv[2], &is_ta) == napi_ok && is_ta) {
            if (napi_get_typedarray_info(env, argv[2], &tt, &len, &data, NULL, NULL) != napi_ok || tt != napi_uint32_array || len != h->n) {
                napi_throw_type_error(env, NULL, "counts must be a Uint32Array with one count per stream"); return NULL;
            }
            counts = (const uint32_t *)data;
        }
    }
    if (argc > 1) {
        bool is_ta = false; napi_typedarray_type tt; size_t len; void *data;
        if (napi_is_typedarray(env, argv[1], &is_ta) == napi_ok && is_ta) {
            if (napi_get_typedarray_info(env, argv[1], &tt, &len, &data, NULL, NULL) != napi_ok || tt != napi_uint8_array || len != h->n) {
                napi_throw_type_error(env, NULL, "ctl must be a Uint8Array with one byte per stream"); return NULL;
            }
            ctl = (const uint8_t *)data;
        }
    }
    wsa_stream_rows r;
    if ((counts ? wsa_stream_step_host_n(h->st, counts, ctl, NULL) : wsa_stream_step_host(h->st, ctl, NULL)) != WSA_OK || wsa_stream_collect(h->st, NULL, &r) != WSA_OK) {
        napi_throw_error(env, NULL, wsa_last_error(h->ctx)); return NULL;
    }
    napi_value o;
    napi_create_object(env, &o);
    napi_set_named_property(env, o, "meta", make_typed(env, napi_int32_array, r.row_meta, (size_t)r.n_rows * 8, 4));
    napi_set_named_property(env, o, "feat", make_typed(env, napi_float64_array, r.row_feat, (size_t)r.n_rows * WSA_NFEAT, 8));
    napi_set_named_property(env, o, "segments", make_typed(env, napi_int32_array, r.segments, (size_t)r.n_segments * 4, 4));
    napi_set_named_property(env, o, "cuts", make_typed(env, napi_uint32_array, r.stream_cuts, (size_t)h->n, 4));
    if (r.utt_feat) {                               /* level 11: one 264-vector per result of the step */
        napi_set_named_property(env, o, "uttMeta", make_typed(env, napi_int32_array, r.utt_meta, (size_t)r.n_utterance_rows * 4, 4));
        napi_set_named_property(env, o, "uttFeat", make_typed(env, napi_float64_array, r.utt_feat, (size_t)r.n_utterance_rows * WSA_NUTT, 8));
    }
    if (r.formants && r.row_formant_off) {          /* levels 4 / 10: the straightened frames of the rows */
        napi_set_named_property(env, o, "formantOff", make_typed(env, napi_uint32_array, r.row_formant_off, (size_t)r.n_rows + 1, 4));
        napi_set_named_property(env, o, "formants", make_typed(env, napi_float32_array, r.formants, (size_t)r.row_formant_off[r.n_rows] * 9, 4));
    }
    if (r.track_off) {                              /* level 3: ranked raw tracks of the step's segments, as LaunchBatch's trackOff / trackPoints / trackRanked */
        const size_t n = 2 * ((size_t)r.n_segments + 1);
        double *od = malloc(sizeof(double) * n);
        for (size_t i = 0; i < n; i++) od[i] = (double)r.track_off[i];
        napi_set_named_property(env, o, "trackOff", make_typed(env, napi_float64_array, od, n, 8));
        free(od);
        napi_set_named_property(env, o, "trackPoints", make_typed(env, napi_int32_array, r.track_points, (size_t)r.n_track_points * 8, 4));
        napi_set_named_property(env, o, "trackRanked", make_typed(env, napi_int32_array, r.track_ranked, (size_t)r.n_track_ranked, 4));
    }
    { napi_value fl; napi_create_uint32(env, r.status_flags, &fl); napi_set_named_property(env, o, "flags", fl); }   /* WSA_FLAG_* (8: a span was cut in this step) */
    if (h->model) {                                 /* the attached classifier's tables of this step, named as processBatch's (streamConf: per stream, carried) */
        wsa_stream_class_result c;
        if (wsa_stream_classes(h->st, &c) != WSA_OK) { napi_throw_error(env, NULL, wsa_last_error(h->ctx)); return NULL; }
        napi_set_named_property(env, o, "prob", make_typed(env, napi_float32_array, c.prob, (size_t)c.n_rows * c.n_classes, 4));
        if (c.cb) {
            napi_set_named_property(env, o, "cb", make_typed(env, napi_int32_array, c.cb, (size_t)c.n_callbacks * 4, 4));
            napi_set_named_property(env, o, "cbLabel", make_typed(env, napi_int32_array, c.cb_label, (size_t)c.n_callbacks, 4));
            napi_set_named_property(env, o, "cbConf", make_typed(env, napi_float64_array, c.cb_conf, (size_t)c.n_callbacks, 8));
            napi_set_named_property(env, o, "streamConf", make_typed(env, napi_float64_array, c.stream_conf, (size_t)c.n_streams * c.n_classes, 8));
        }
        napi_value nc; napi_create_uint32(env, c.n_classes, &nc); napi_set_named_property(env, o, "nClasses", nc);
    }
    if (h->knn) {                                   /* the attached KNN store's tables of this step (K9s; level 13: the fold KN-2, knnStreamConf per stream, carried) */
        wsa_stream_knn_result c;
        if (wsa_stream_knn_classes(h->st, &c) != WSA_OK) { napi_throw_error(env, NULL, wsa_last_error(h->ctx)); return NULL; }
        napi_set_named_property(env, o, "knnLabel", make_typed(env, napi_int32_array, c.label, (size_t)c.n_rows, 4));
        napi_set_named_property(env, o, "knnConf", make_typed(env, napi_float64_array, c.conf, (size_t)c.n_rows * c.n_classes, 8));
        if (c.cb) {
            napi_set_named_property(env, o, "knnCb", make_typed(env, napi_int32_array, c.cb, (size_t)c.n_callbacks * 4, 4));
            napi_set_named_property(env, o, "knnCbLabel", make_typed(env, napi_int32_array, c.cb_label, (size_t)c.n_callbacks, 4));
            napi_set_named_property(env, o, "knnCbConf", make_typed(env, napi_float64_array, c.cb_conf, (size_t)c.n_callbacks, 8));
            napi_set_named_property(env, o, "knnStreamConf", make_typed(env, napi_float64_array, c.stream_conf, (size_t)c.n_streams * c.n_classes, 8));
        }
        napi_value nc; napi_create_uint32(env, c.n_classes, &nc); napi_set_named_property(env, o, "knnNClasses", nc);
    }
    if (h->ens) {                                   /* the attached ensemble's tables of this step (conf / minDb: per stream, carried) */
        wsa_stream_ensemble_result c;
        if (wsa_stream_ensemble_classes(h->st, &c) != WSA_OK) { napi_throw_error(env, NULL, wsa_last_error(h->ctx)); return NULL; }
        const ens_view v = {c.n_members, c.n_rows, c.n_callbacks, c.n_streams, c.n_classes, c.cb != NULL, c.prob, c.cb_label, c.cb_conf, c.cb_all_max, c.stream_conf,
                            c.cb, c.cb_db, c.cb_top_label, c.cb_min_db, c.stream_min_db, c.cb_top_conf, c.cb_entropy};
        napi_set_named_property(env, o, "ens", ens_object(env, &v));
    }
    if (h->reg) {                                   /* the attached regression group's tables of this step (level 13: the fold RG-1; regSum / regWeight / regRunValue per stream, carried) */
        wsa_stream_value_result c;
        if (wsa_stream_values(h->st, &c) != WSA_OK) { napi_throw_error(env, NULL, wsa_last_error(h->ctx)); return NULL; }
        napi_set_named_property(env, o, "regValue", make_heads(env, c.value, c.n_heads, c.n_rows));
        if (c.cb) {
            napi_set_named_property(env, o, "regCb", make_typed(env, napi_int32_array, c.cb, (size_t)c.n_callbacks * 4, 4));
            napi_set_named_property(env, o, "regCbValue", make_heads(env, c.cb_value, c.n_heads, c.n_callbacks));
            napi_set_named_property(env, o, "regCbWeight", make_heads(env, c.cb_weight, c.n_heads, c.n_callbacks));
            napi_set_named_property(env, o, "regSum", make_heads(env, c.stream_sum, c.n_heads, c.n_streams));
            napi_set_named_property(env, o, "regWeight", make_heads(env, c.stream_weight, c.n_heads, c.n_streams));
            napi_set_named_property(env, o, "regRunValue", make_heads(env, c.stream_value, c.n_heads, c.n_streams));
        }
        napi_value nh; napi_create_uint32(env, c.n_heads, &nh); napi_set_named_property(env, o, "regNHeads", nh);
    }
    return o;
}
static void stream_drop_ensemble(stream_t *h) {     /* after the stream object stopped using it */
    if (h->ens) wsa_ensemble_destroy(h->ens);
    for (uint32_t d = 0; d < h->n_ens; d++) if (h->ens_models[d]->busy) h->ens_models[d]->busy--;
    h->ens = NULL; h->n_ens = 0;
}
static void stream_drop_regress(stream_t *h) {      /* after the stream object stopped using it */
    if (h->reg) wsa_regress_group_destroy(h->reg);
    for (uint32_t d = 0; d < h->n_reg; d++) if (h->reg_models[d]->busy) h->reg_models[d]->busy--;
    h->reg = NULL; h->n_reg = 0;
}
static napi_value fn_stream_close(napi_env env, napi_callback_info info) {
    size_t argc = 1; napi_value argv[1];
    NAPI_OK(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
    stream_t *h = argc ? get_stream(env, argv[0]) : NULL;
    if (h && h->st) {
        if (h->input_ref) {                  /* the pinned buffer goes away with the stream object: views on it must not outlive it */
            napi_value ab;
            if (napi_get_reference_value(env, h->input_ref, &ab) == napi_ok && ab) napi_detach_arraybuffer(env, ab);
            napi_delete_reference(env, h->input_ref); h->input_ref = NULL;
        }
        wsa_stream_destroy(h->st); h->st = NULL;
        h->knn = NULL;
        stream_drop_regress(h);
        if (h->model) { if (h->model->busy) h->model->busy--; h->model = NULL; }
        stream_drop_ensemble(h);
        if (h->box && h->box->children) h->box->children--;
    }
    return NULL;
}
static napi_value fn_stream_set_model(napi_env env, napi_callback_info info) {
    size_t argc = 2; napi_value argv[2];
    NAPI_OK(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
    stream_t *h = argc ? get_stream(env, argv[0]) : NULL;
    if (!h || !h->st || argc < 2) { napi_throw_type_error(env, NULL, "streamSetModel(stream, model | null)"); return NULL; }
    model_box *mb = NULL;
    napi_valuetype t;
    NAPI_OK(env, napi_typeof(env, argv[1], &t));
    if (t != napi_null && t != napi_undefined) {
        void *p = NULL;
        if (t != napi_external || napi_get_value_external(env, argv[1], &p) != napi_ok || !p || !((model_box *)p)->m) { napi_throw_error(env, NULL, "streamSetModel: the model handle was destroyed (or is not a model)"); return NULL; }
        mb = (model_box *)p;
        if (mb->owner != h->box) { napi_throw_error(env, NULL, "streamSetModel: the model belongs to another context"); return NULL; }
    }
    if (wsa_stream_set_model(h->st, mb ? mb->m : NULL) != WSA_OK) { napi_throw_error(env, NULL, wsa_last_error(h->ctx)); return NULL; }
    if (h->model && h->model->busy) h->model->busy--;          /* modelDestroy() refuses while a stream holds the model */
    h->model = mb;
    if (mb) { mb->busy++; stream_drop_ensemble(h); }            /* (the library detached the ensemble) */
    return NULL;
}
/* streamSetKnn(stream, knn | null, k): the store stays the caller's; knnDestroy() refuses while its context has open streams */
static napi_value fn_stream_set_knn(napi_env env, napi_callback_info info) {
    size_t argc = 3; napi_value argv[3];
    NAPI_OK(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
    stream_t *h = argc ? get_stream(env, argv[0]) : NULL;
    if (!h || !h->st || argc < 2) { napi_throw_type_error(env, NULL, "streamSetKnn(stream, knn | null, k)"); return NULL; }
    struct knn_box *kb = NULL;
    uint32_t k = 0;
    napi_valuetype t;
    NAPI_OK(env, napi_typeof(env, argv[1], &t));
    if (t != napi_null && t != napi_undefined) {
        void *p = NULL;
        if (t != napi_external || napi_get_value_external(env, argv[1], &p) != napi_ok || !p || !((struct knn_box *)p)->k) { napi_throw_error(env, NULL, "streamSetKnn: the KNN store was destroyed (or is not a store)"); return NULL; }
        kb = (struct knn_box *)p;
        if (kb->owner != h->box) { napi_throw_error(env, NULL, "streamSetKnn: the KNN store belongs to another context"); return NULL; }
        if (argc < 3 || napi_get_value_uint32(env, argv[2], &k) != napi_ok) { napi_throw_type_error(env, NULL, "streamSetKnn(stream, knn | null, k)"); return NULL; }
    }
    if (wsa_stream_set_knn(h->st, kb ? kb->k : NULL, k) != WSA_OK) { napi_throw_error(env, NULL, wsa_last_error(h->ctx)); return NULL; }
    h->knn = kb;
    return NULL;
}
/* streamSetEnsemble(stream, [models] | null): the stream object owns the wsa_ensemble it makes of them, until it is replaced, detached or closed */
static napi_value fn_stream_set_ensemble(napi_env env, napi_callback_info info) {
    size_t argc = 2; napi_value argv[2];
    NAPI_OK(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
    stream_t *h = argc ? get_stream(env, argv[0]) : NULL;
    if (!h || !h->st || argc < 2) { napi_throw_type_error(env, NULL, "streamSetEnsemble(stream, [models] | null)"); return NULL; }
    model_box *mbs[WSA_ENSEMBLE_MAX] = {0}; const wsa_model *ms[WSA_ENSEMBLE_MAX]; uint32_t n = 0;
    bool arr = false;
    napi_valuetype t;
    NAPI_OK(env, napi_typeof(env, argv[1], &t));
    if (t != napi_null && t != napi_undefined) {
        if (napi_is_array(env, argv[1], &arr) != napi_ok || !arr || napi_get_array_length(env, argv[1], &n) != napi_ok || n < 1 || n > WSA_ENSEMBLE_MAX) {
            napi_throw_error(env, NULL, "streamSetEnsemble: an ensemble has 1 .. 8 models"); return NULL;
        }
        for (uint32_t d = 0; d < n; d++) {
            napi_value el; napi_valuetype et = napi_undefined; void *p = NULL;
            if (napi_get_element(env, argv[1], d, &el) != napi_ok || napi_typeof(env, el, &et) != napi_ok || et != napi_external || napi_get_value_external(env, el, &p) != napi_ok || !p || !((model_box *)p)->m) {
                napi_throw_error(env, NULL, "streamSetEnsemble: a model handle was destroyed (or is not a model)"); return NULL;
            }
            mbs[d] = (model_box *)p; ms[d] = mbs[d]->m;
            if (mbs[d]->owner != h->box) { napi_throw_error(env, NULL, "streamSetEnsemble: a model belongs to another context"); return NULL; }
        }
    }
    wsa_ensemble *e = NULL;
    if (n && wsa_ensemble_create(h->ctx, ms, n, &e) != WSA_OK) { napi_throw_error(env, NULL, wsa_last_error(h->ctx)); return NULL; }
    if (wsa_stream_set_ensemble(h->st, e) != WSA_OK) { if (e) wsa_ensemble_destroy(e); napi_throw_error(env, NULL, wsa_last_error(h->ctx)); return NULL; }
    stream_drop_ensemble(h);
    if (e) {
        h->ens = e; h->n_ens = n; memcpy(h->ens_models, mbs, sizeof h->ens_models);
        for (uint32_t d = 0; d < n; d++) mbs[d]->busy++;
        if (h->model) { if (h->model->busy) h->model->busy--; h->model = NULL; }     /* (the library detached the model) */
    }
    return NULL;
}

/* ---- the app's classifier: modelCreate(ctx, {units, activation, kernels, biases, inMin, inMax, labels}) -> handle (wsa_model_create);
 * modelDestroy(handle).  The handle is a box: after modelDestroy() or its context's destroy() any use throws instead of touching freed memory. */
static void model_finalize(napi_env env, void *data, void *hint) {
    model_box *mb = (model_box *)data;
    if (!mb->m && !mb->owner) free(mb);              /* a live model stays (explicit destroy only, as contexts) */
}
static int typed_of(napi_env env, napi_value o, const char *name, napi_typedarray_type want, void **data, size_t *len) {
    napi_value v; bool ta = false; napi_typedarray_type t;
    if (napi_get_named_property(env, o, name, &v) != napi_ok || napi_is_typedarray(env, v, &ta) != napi_ok || !ta) return 0;
    if (napi_get_typedarray_info(env, v, &t, len, data, NULL, NULL) != napi_ok || t != want) return 0;
    return 1;
}
static napi_value fn_model_create(napi_env env, napi_callback_info info) {
    size_t argc = 2; napi_value argv[2];
    NAPI_OK(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
    ctx_box *box = argc ? get_box(env, argv[0]) : NULL;
    const char *usage = "modelCreate(ctx, {units: Int32Array, activation: Int32Array, kernels: Float32Array[], biases: Float32Array[], inMin: Float64Array, inMax: Float64Array, labels: string[]})";
    if (!box || !box->ctx || argc < 2) { napi_throw_type_error(env, NULL, usage); return NULL; }
    int32_t *units = NULL, *act = NULL; double *mn = NULL, *mx = NULL; size_t nu = 0, na = 0, nmn = 0, nmx = 0;
    if (!typed_of(env, argv[1], "units", napi_int32_array, (void **)&units, &nu) || !typed_of(env, argv[1], "activation", napi_int32_array, (void **)&act, &na) ||
        !typed_of(env, argv[1], "inMin", napi_float64_array, (void **)&mn, &nmn) || !typed_of(env, argv[1], "inMax", napi_float64_array, (void **)&mx, &nmx) ||
        nu < 2 || na != nu - 1 || na > WSA_MODEL_MAX_LAYERS || units[0] < 1 || nmn != (size_t)units[0] || nmx != (size_t)units[0]) { napi_throw_type_error(env, NULL, usage); return NULL; }
    napi_value ka, ba; bool ia = false, ib = false; uint32_t nk = 0, nb = 0;
    if (napi_get_named_property(env, argv[1], "kernels", &ka) != napi_ok || napi_is_array(env, ka, &ia) != napi_ok || !ia || napi_get_array_length(env, ka, &nk) != napi_ok ||
        napi_get_named_property(env, argv[1], "biases", &ba) != napi_ok || napi_is_array(env, ba, &ib) != napi_ok || !ib || napi_get_array_length(env, ba, &nb) != napi_ok ||
        nk != na || nb != na) { napi_throw_type_error(env, NULL, usage); return NULL; }
    const float *kp[WSA_MODEL_MAX_LAYERS], *bp[WSA_MODEL_MAX_LAYERS];
    for (uint32_t l = 0; l < na; l++) {
        napi_value kv, bv; bool t1 = false, t2 = false; napi_typedarray_type tk, tb; size_t lk = 0, lb = 0; void *dk = NULL, *db = NULL;
        if (napi_get_element(env, ka, l, &kv) != napi_ok || napi_is_typedarray(env, kv, &t1) != napi_ok || !t1 || napi_get_typedarray_info(env, kv, &tk, &lk, &dk, NULL, NULL) != napi_ok ||
            napi_get_element(env, ba, l, &bv) != napi_ok || napi_is_typedarray(env, bv, &t2) != napi_ok || !t2 || napi_get_typedarray_info(env, bv, &tb, &lb, &db, NULL, NULL) != napi_ok ||
            tk != napi_float32_array || tb != napi_float32_array || lk != (size_t)units[l] * (size_t)units[l + 1] || lb != (size_t)units[l + 1]) {
            napi_throw_type_error(env, NULL, "modelCreate: kernels[i] must be a Float32Array of units[i] x units[i+1], biases[i] one of units[i+1]"); return NULL;
        }
        kp[l] = (const float *)dk; bp[l] = (const float *)db;
    }
    /* labels (optional): strings, legend order */
    char **labels = NULL; uint32_t nl = 0;
    { napi_value la; bool il = false;
      if (napi_get_named_property(env, argv[1], "labels", &la) == napi_ok && napi_is_array(env, la, &il) == napi_ok && il && napi_get_array_length(env, la, &nl) == napi_ok && nl == (uint32_t)units[na]) {
          labels = calloc(nl, sizeof(char *));
          for (uint32_t i = 0; labels && i < nl; i++) {
              napi_value e; size_t len = 0;
              if (napi_get_element(env, la, i, &e) != napi_ok || napi_get_value_string_utf8(env, e, NULL, 0, &len) != napi_ok) { len = 0; labels[i] = calloc(1, 1); continue; }
              labels[i] = calloc(len + 1, 1);
              if (labels[i]) napi_get_value_string_utf8(env, e, labels[i], len + 1, &len);
          }
      } else nl = 0; }
    wsa_model_desc d = {(int32_t)na, units, act, kp, bp, mn, mx, (const char *const *)labels};
    wsa_model *m = NULL;
    const wsa_status st = wsa_model_create(box->ctx, &d, &m);
    for (uint32_t i = 0; labels && i < nl; i++) free(labels[i]);
    free(labels);
    if (st != WSA_OK) { napi_throw_error(env, NULL, wsa_last_error(box->ctx)); return NULL; }
    model_box *mb = calloc(1, sizeof *mb);
    if (!mb) { wsa_model_destroy(m); napi_throw_error(env, NULL, "out of memory"); return NULL; }
    mb->m = m; mb->owner = box; mb->n_classes = (uint32_t)units[na]; mb->n_inputs = (uint32_t)units[0]; mb->next = box->models; box->models = mb;
    napi_value ext; NAPI_OK(env, napi_create_external(env, mb, model_finalize, NULL, &ext));
    return ext;
}
static napi_value fn_model_destroy(napi_env env, napi_callback_info info) {
    size_t argc = 1; napi_value argv[1]; void *p = NULL;
    NAPI_OK(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
    if (argc < 1 || napi_get_value_external(env, argv[0], &p) != napi_ok || !p) { napi_throw_type_error(env, NULL, "modelDestroy(model)"); return NULL; }
    model_box *mb = (model_box *)p;
    if (mb->busy) { napi_throw_error(env, NULL, "the model is in use by a batch in flight or an open stream"); return NULL; }
    if (mb->owner && mb->owner->ens) {          /* the context's kept ensemble may hold it: no job is in flight with it (busy is 0), so it goes first */
        for (uint32_t d = 0; d < mb->owner->ens_n; d++) if (mb->owner->ens_models[d] == mb) {
            if (mb->owner->children) { napi_throw_error(env, NULL, "the model is part of the context's ensemble while a batch is in flight"); return NULL; }
            box_drop_ensemble(mb->owner); break;
        }
    }
    if (mb->owner && mb->owner->reg)            /* ... and so may its kept regression group (batchRegressGroup is synchronous: nothing is in flight with it) */
        for (uint32_t d = 0; d < mb->owner->reg_n; d++) if (mb->owner->reg_models[d] == mb) { box_drop_regress(mb->owner); break; }
    if (mb->m) { wsa_model_destroy(mb->m); mb->m = NULL; }
    model_unlink(mb);
    return NULL;
}

/* ---- training (wsa_trainer_*, K7): train(ctx, spec, {features: Float64Array [n][units[0]] (53, 264 or 23 wide), y: Int32Array [n], nVal, batchSize, learningRate, epochs,
 * orders: Uint32Array [epochs][n - nVal] | undefined}, onEpoch | undefined) -> Promise of {kernels: Float32Array[], biases: Float32Array[],
 * history: Float64Array [epochs][4] = loss, acc, val_loss, val_acc}.  `spec` is modelCreate's object and holds the INITIAL weights.  The epochs run
 * on a thread of their own (the inputs are copied first); after every epoch onEpoch(epoch, {loss, acc, val_loss, val_acc}) is queued to the JS
 * thread (ml5's whileTraining), and the Promise settles after the last of them was delivered: both go through one first-in first-out queue. */
typedef struct {
    ctx_box *box; napi_deferred deferred; napi_threadsafe_function tsfn; pthread_t thread; napi_ref on_epoch;
    int32_t nl, units[WSA_MODEL_MAX_LAYERS + 1], act[WSA_MODEL_MAX_LAYERS];
    float *kernel[WSA_MODEL_MAX_LAYERS], *bias[WSA_MODEL_MAX_LAYERS];
    double mn[WSA_NUTT], mx[WSA_NUTT];                     /* units[0] entries: the widest row of an ML level has WSA_NUTT */
    double *feat; int32_t *y; uint32_t *orders; uint32_t n, n_val, batch, epochs; double lr;
    const wsa_featdb *db; uint32_t *rows;                 /* db != NULL: the rows are DB rows rows[0 .. n-1] (wsa_trainer_create_db), feat is NULL */
    double *values, out_min, out_max;                     /* values != NULL: a regression model (wsa_regress_trainer_create) instead of y */
    double *history; wsa_status st; char err[512];
} train_job;
typedef struct { train_job *j; int32_t epoch; wsa_train_stats s; } train_msg;          /* epoch < 0: the run is over */

static void train_job_free(train_job *j) {
    for (int l = 0; l < WSA_MODEL_MAX_LAYERS; l++) { free(j->kernel[l]); free(j->bias[l]); }
    free(j->feat); free(j->y); free(j->values); free(j->orders); free(j->history); free(j->rows); free(j);
}
/* the trainer of a job: from host rows, or from the rows of a device feature DB */
static wsa_status train_job_trainer(wsa_ctx *ctx, const train_job *j, const wsa_model_desc *d, wsa_trainer **t) {
    if (j->db) return j->values ? wsa_regress_trainer_create_db(ctx, d, j->db, j->rows, j->values, j->n, j->n_val, j->batch, j->lr, j->out_min, j->out_max, t)
                                : wsa_trainer_create_db(ctx, d, j->db, j->rows, j->y, j->n, j->n_val, j->batch, j->lr, t);
    return j->values ? wsa_regress_trainer_create(ctx, d, j->feat, j->values, j->n, j->n_val, j->batch, j->lr, j->out_min, j->out_max, t)
                     : wsa_trainer_create(ctx, d, j->feat, j->y, j->n, j->n_val, j->batch, j->lr, t);
}
static void *train_thread(void *arg) {
    train_job *j = (train_job *)arg;
    wsa_ctx *ctx = j->box->ctx;
    wsa_trainer *t = NULL;
    wsa_model_desc d = {j->nl, j->units, j->act, (const float *const *)j->kernel, (const float *const *)j->bias, j->mn, j->mx, NULL};
    j->st = train_job_trainer(ctx, j, &d, &t);
    for (uint32_t e = 0; j->st == WSA_OK && e < j->epochs; e++) {
        j->st = wsa_trainer_epoch(t, j->orders ? j->orders + (size_t)e * (j->n - j->n_val) : NULL, j->box->queue);
        wsa_train_stats s;
        if (j->st == WSA_OK) j->st = wsa_trainer_stats(t, j->box->queue, &s);
        if (j->st != WSA_OK) break;
        j->history[4 * e] = s.loss; j->history[4 * e + 1] = s.acc; j->history[4 * e + 2] = s.val_loss; j->history[4 * e + 3] = s.val_acc;
        train_msg *m = malloc(sizeof *m);
        if (m) { m->j = j; m->epoch = (int32_t)e; m->s = s; if (napi_call_threadsafe_function(j->tsfn, m, napi_tsfn_blocking) != napi_ok) free(m); }
    }
    if (j->st == WSA_OK) j->st = wsa_trainer_copy_weights(t, j->box->queue, j->kernel, j->bias);
    if (j->st != WSA_OK) snprintf(j->err, sizeof j->err, "%s", wsa_last_error(ctx));
    if (t) wsa_trainer_destroy(t);
    train_msg *m = malloc(sizeof *m);                       /* (a few bytes: if even this fails the Promise stays pending) */
    if (m) { m->j = j; m->epoch = -1; napi_call_threadsafe_function(j->tsfn, m, napi_tsfn_blocking); }
    return NULL;
}
/* {kernels, biases, history} of a finished job */
static napi_value train_result(napi_env env, train_job *j) {
    napi_value o, ka, ba; napi_create_object(env, &o); napi_create_array_with_length(env, (size_t)j->nl, &ka); napi_create_array_with_length(env, (size_t)j->nl, &ba);
    for (int l = 0; l < j->nl; l++) {
        napi_set_element(env, ka, (uint32_t)l, make_typed(env, napi_float32_array, j->kernel[l], (size_t)j->units[l] * (size_t)j->units[l + 1], sizeof(float)));
        napi_set_element(env, ba, (uint32_t)l, make_typed(env, napi_float32_array, j->bias[l], (size_t)j->units[l + 1], sizeof(float)));
    }
    napi_set_named_property(env, o, "kernels", ka); napi_set_named_property(env, o, "biases", ba);
    napi_set_named_property(env, o, "history", make_typed(env, napi_float64_array, j->history, (size_t)j->epochs * 4, sizeof(double)));
    return o;
}
/* the job's onEpoch(epoch, {loss, acc, val_loss, val_acc}), if it has one */
static void train_on_epoch(napi_env env, train_job *j, int32_t epoch, const wsa_train_stats *s) {
    napi_value fn, undef, argv[2], v;
    if (j->on_epoch && napi_get_reference_value(env, j->on_epoch, &fn) == napi_ok && napi_get_undefined(env, &undef) == napi_ok &&
        napi_create_int32(env, epoch, &argv[0]) == napi_ok && napi_create_object(env, &argv[1]) == napi_ok) {
        const char *names[4] = {"loss", "acc", "val_loss", "val_acc"}; const double vals[4] = {s->loss, s->acc, s->val_loss, s->val_acc};
        for (int i = 0; i < 4; i++) if (napi_create_double(env, vals[i], &v) == napi_ok) napi_set_named_property(env, argv[1], names[i], v);
        napi_call_function(env, undef, fn, 2, argv, NULL);
    }
}
static void train_call_js(napi_env env, napi_value js_cb, void *context, void *data) {
    train_msg *m = (train_msg *)data;
    train_job *j = m->j;
    if (!env) { free(m); return; }
    if (m->epoch >= 0) {
        train_on_epoch(env, j, m->epoch, &m->s);
        free(m);
        return;
    }
    free(m);
    pthread_join(j->thread, NULL);
    if (j->box->children) j->box->children--;
    if (j->st != WSA_OK) {
        napi_value msg; napi_create_string_utf8(env, j->err, NAPI_AUTO_LENGTH, &msg);
        napi_reject_deferred(env, j->deferred, msg);
    } else napi_resolve_deferred(env, j->deferred, train_result(env, j));
    if (j->on_epoch) napi_delete_reference(env, j->on_epoch);
    napi_release_threadsafe_function(j->tsfn, napi_tsfn_release);
    train_job_free(j);
}
static int num_of(napi_env env, napi_value o, const char *name, double *out) {
    napi_value v; napi_valuetype t;
    return napi_get_named_property(env, o, name, &v) == napi_ok && napi_typeof(env, v, &t) == napi_ok && t == napi_number && napi_get_value_double(env, v, out) == napi_ok;
}
static void *dup_bytes(const void *p, size_t bytes) { void *q = malloc(bytes ? bytes : 1); if (q && bytes) memcpy(q, p, bytes); return q; }
static const char *TRAIN_USAGE = "train(ctx, {units, activation, kernels, biases, inMin, inMax}, {features: Float64Array | db + rows: Uint32Array, y: Int32Array | values: Float64Array + outMin + outMax, nVal, batchSize, learningRate, epochs, orders?: Uint32Array}, onEpoch?)";
/* a job from train's arguments (argv[0] unused, argv[1] the spec, argv[2] the run, argv[3] onEpoch when argc > 3), the inputs copied; NULL with an
 * exception pending */
static train_job *train_job_from(napi_env env, ctx_box *box, size_t argc, const napi_value *argv) {
    const char *usage = TRAIN_USAGE;
    int32_t *units = NULL, *act = NULL, *y = NULL; double *mn = NULL, *mx = NULL, *feat = NULL, *values = NULL; uint32_t *orders = NULL;
    size_t nu = 0, na = 0, nmn = 0, nmx = 0, nf = 0, ny = 0, no = 0;
    double n_val = 0, batch = 0, lr = 0, epochs = 0, out_min = 0, out_max = 0;
    /* a regression run (specification TR-2): `values` (the label's real values) with `outMin` / `outMax` in place of `y` */
    const int regress = typed_of(env, argv[2], "values", napi_float64_array, (void **)&values, &ny);
    /* `db` (a featdbCreate handle of this context) with `rows` (its row indices) in place of `features`: the rows stay on the device */
    fdb_box *fb = NULL; uint32_t *rows = NULL; size_t nr = 0;
    { napi_value dv; napi_valuetype dt = napi_undefined; void *pp = NULL;
      if (napi_get_named_property(env, argv[2], "db", &dv) == napi_ok && napi_typeof(env, dv, &dt) == napi_ok && dt == napi_external && napi_get_value_external(env, dv, &pp) == napi_ok) fb = (fdb_box *)pp; }
    if (fb && (!fb->db || fb->owner != box)) { napi_throw_error(env, NULL, "train: the device DB was destroyed or belongs to another context"); return NULL; }
    if (fb && !typed_of(env, argv[2], "rows", napi_uint32_array, (void **)&rows, &nr)) { napi_throw_type_error(env, NULL, usage); return NULL; }
    if (regress && (!num_of(env, argv[2], "outMin", &out_min) || !num_of(env, argv[2], "outMax", &out_max))) { napi_throw_type_error(env, NULL, usage); return NULL; }
    if (!typed_of(env, argv[1], "units", napi_int32_array, (void **)&units, &nu) || !typed_of(env, argv[1], "activation", napi_int32_array, (void **)&act, &na) ||
        !typed_of(env, argv[1], "inMin", napi_float64_array, (void **)&mn, &nmn) || !typed_of(env, argv[1], "inMax", napi_float64_array, (void **)&mx, &nmx) ||
        nu < 2 || na != nu - 1 || na > WSA_MODEL_MAX_LAYERS || units[0] < 1 || units[0] > WSA_NUTT || nmn != (size_t)units[0] || nmx != (size_t)units[0] ||
        (!fb && !typed_of(env, argv[2], "features", napi_float64_array, (void **)&feat, &nf)) || (!regress && !typed_of(env, argv[2], "y", napi_int32_array, (void **)&y, &ny)) ||
        ny < 1 || (fb ? nr != ny : nf != ny * (size_t)units[0]) || ny > 0xffffffffu ||
        !num_of(env, argv[2], "nVal", &n_val) || !num_of(env, argv[2], "batchSize", &batch) || !num_of(env, argv[2], "learningRate", &lr) || !num_of(env, argv[2], "epochs", &epochs) ||
        n_val < 0 || n_val >= (double)ny || batch < 0 || batch > 4294967295.0 || epochs < 1 || epochs > 1e6) { napi_throw_type_error(env, NULL, usage); return NULL; }
    const uint32_t n_train = (uint32_t)ny - (uint32_t)n_val;
    if (typed_of(env, argv[2], "orders", napi_uint32_array, (void **)&orders, &no) && no != (size_t)epochs * n_train) { napi_throw_type_error(env, NULL, "train: orders must hold epochs x (rows - nVal) indices"); return NULL; }
    napi_value ka, ba; bool ia = false, ib = false; uint32_t nk = 0, nb = 0;
    if (napi_get_named_property(env, argv[1], "kernels", &ka) != napi_ok || napi_is_array(env, ka, &ia) != napi_ok || !ia || napi_get_array_length(env, ka, &nk) != napi_ok ||
        napi_get_named_property(env, argv[1], "biases", &ba) != napi_ok || napi_is_array(env, ba, &ib) != napi_ok || !ib || napi_get_array_length(env, ba, &nb) != napi_ok ||
        nk != na || nb != na) { napi_throw_type_error(env, NULL, usage); return NULL; }
    for (size_t l = 0; l <= na; l++) if (units[l] < 1 || units[l] > WSA_MODEL_MAX_WIDTH) { napi_throw_type_error(env, NULL, "train: layer widths are 1 .. 1024"); return NULL; }
    train_job *j = calloc(1, sizeof *j);
    if (!j) { napi_throw_error(env, NULL, "out of memory"); return NULL; }
    j->box = box; j->nl = (int32_t)na; j->n = (uint32_t)ny; j->n_val = (uint32_t)n_val; j->batch = (uint32_t)batch; j->epochs = (uint32_t)epochs; j->lr = lr;
    memcpy(j->units, units, nu * sizeof(int32_t)); memcpy(j->act, act, na * sizeof(int32_t)); memcpy(j->mn, mn, nmn * sizeof(double)); memcpy(j->mx, mx, nmx * sizeof(double));
    bool ok = true;
    for (uint32_t l = 0; l < na && ok; l++) {
        napi_value kv, bv; bool t1 = false, t2 = false; napi_typedarray_type tk, tb; size_t lk = 0, lb = 0; void *dk = NULL, *db = NULL;
        ok = napi_get_element(env, ka, l, &kv) == napi_ok && napi_is_typedarray(env, kv, &t1) == napi_ok && t1 && napi_get_typedarray_info(env, kv, &tk, &lk, &dk, NULL, NULL) == napi_ok &&
             napi_get_element(env, ba, l, &bv) == napi_ok && napi_is_typedarray(env, bv, &t2) == napi_ok && t2 && napi_get_typedarray_info(env, bv, &tb, &lb, &db, NULL, NULL) == napi_ok &&
             tk == napi_float32_array && tb == napi_float32_array && lk == (size_t)units[l] * (size_t)units[l + 1] && lb == (size_t)units[l + 1];
        if (ok) { j->kernel[l] = dup_bytes(dk, lk * sizeof(float)); j->bias[l] = dup_bytes(db, lb * sizeof(float)); ok = j->kernel[l] && j->bias[l]; }
    }
    if (!ok) { train_job_free(j); napi_throw_type_error(env, NULL, "train: kernels[i] must be a Float32Array of units[i] x units[i+1], biases[i] one of units[i+1]"); return NULL; }
    if (fb) { j->db = fb->db; j->rows = dup_bytes(rows, nr * sizeof(uint32_t)); }
    else j->feat = dup_bytes(feat, nf * sizeof(double));
    j->history = calloc((size_t)j->epochs * 4, sizeof(double));
    if (regress) { j->values = dup_bytes(values, ny * sizeof(double)); j->out_min = out_min; j->out_max = out_max; }
    else j->y = dup_bytes(y, ny * sizeof(int32_t));
    if (orders) j->orders = dup_bytes(orders, no * sizeof(uint32_t));
    if ((fb ? !j->rows : !j->feat) || (regress ? !j->values : !j->y) || !j->history || (orders && !j->orders)) { train_job_free(j); napi_throw_error(env, NULL, "out of memory"); return NULL; }
    napi_valuetype ft = napi_undefined;
    if (argc > 3 && napi_typeof(env, argv[3], &ft) == napi_ok && ft == napi_function && napi_create_reference(env, argv[3], 1, &j->on_epoch) != napi_ok) j->on_epoch = NULL;
    return j;
}
static napi_value fn_train(napi_env env, napi_callback_info info) {
    size_t argc = 4; napi_value argv[4];
    NAPI_OK(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
    ctx_box *box = argc ? get_box(env, argv[0]) : NULL;
    if (!box || !box->ctx || argc < 3) { napi_throw_type_error(env, NULL, TRAIN_USAGE); return NULL; }
    train_job *j = train_job_from(env, box, argc, argv);
    if (!j) return NULL;
    napi_value promise, name;
    if (napi_create_promise(env, &j->deferred, &promise) != napi_ok || napi_create_string_utf8(env, "wsa_train", NAPI_AUTO_LENGTH, &name) != napi_ok ||
        napi_create_threadsafe_function(env, NULL, NULL, name, 0, 1, NULL, NULL, NULL, train_call_js, &j->tsfn) != napi_ok) {
        if (j->on_epoch) napi_delete_reference(env, j->on_epoch);
        train_job_free(j); napi_throw_error(env, NULL, "train: could not set up the job"); return NULL;
    }
    box->children++;                                             /* until the run's last message: destroy() refuses meanwhile */
    if (pthread_create(&j->thread, NULL, train_thread, j) != 0) {
        box->children--; napi_release_threadsafe_function(j->tsfn, napi_tsfn_release);
        if (j->on_epoch) napi_delete_reference(env, j->on_epoch);
        napi_value msg; napi_create_string_utf8(env, "train: could not start a thread", NAPI_AUTO_LENGTH, &msg); napi_reject_deferred(env, j->deferred, msg);
        train_job_free(j);
    }
    return promise;
}

/* ---- training groups (wsa_train_group_*, K7g, specification TG-1): trainGroup(ctx, [[spec, run, onEpoch | undefined], ...]) -> Promise of an array with,
 * per job and in job order, what train resolves to.  1 .. WSA_TRAIN_GROUP_MAX jobs, each with train's own arguments; classifiers and regression
 * models mix.  All jobs' trainers step in lock step on one thread, one launch per stage for all of them; a job with fewer epochs leaves and the group
 * is formed again from the rest, so every job's result equals its own train call bit for bit.  A job's onEpoch fires after each of ITS epochs. */
typedef struct {
    ctx_box *box; napi_deferred deferred; napi_threadsafe_function tsfn; pthread_t thread;
    uint32_t n; train_job *job[WSA_TRAIN_GROUP_MAX];
    wsa_status st; char err[512];
} train_group_job;
typedef struct { train_group_job *g; uint32_t member; int32_t epoch; wsa_train_stats s; } train_group_msg;          /* epoch < 0: the run is over */

static void train_group_free(napi_env env, train_group_job *g) {
    for (uint32_t i = 0; i < g->n; i++) {
        if (env && g->job[i]->on_epoch) napi_delete_reference(env, g->job[i]->on_epoch);
        train_job_free(g->job[i]);
    }
    free(g);
}
static void *train_group_thread(void *arg) {
    train_group_job *g = (train_group_job *)arg;
    wsa_ctx *ctx = g->box->ctx;
    wsa_trainer *t[WSA_TRAIN_GROUP_MAX] = {0};
    uint32_t longest = 0;
    g->st = WSA_OK;
    for (uint32_t i = 0; i < g->n && g->st == WSA_OK; i++) {
        train_job *j = g->job[i];
        wsa_model_desc d = {j->nl, j->units, j->act, (const float *const *)j->kernel, (const float *const *)j->bias, j->mn, j->mx, NULL};
        g->st = train_job_trainer(ctx, j, &d, &t[i]);
        if (j->epochs > longest) longest = j->epochs;
    }
    wsa_train_group *grp = NULL;
    uint32_t live[WSA_TRAIN_GROUP_MAX], n_live = 0;                      /* the members of grp, as job indices */
    for (uint32_t e = 0; g->st == WSA_OK && e < longest; e++) {
        uint32_t now[WSA_TRAIN_GROUP_MAX], n_now = 0;
        for (uint32_t i = 0; i < g->n; i++) if (g->job[i]->epochs > e) now[n_now++] = i;
        if (!grp || n_now != n_live) {                                   /* jobs only ever leave: the same count is the same set */
            wsa_trainer *members[WSA_TRAIN_GROUP_MAX];
            if (grp) { wsa_train_group_destroy(grp); grp = NULL; }
            for (uint32_t k = 0; k < n_now; k++) { live[k] = now[k]; members[k] = t[now[k]]; }
            n_live = n_now;
            g->st = wsa_train_group_create(ctx, members, n_live, &grp);
            if (g->st != WSA_OK) break;
        }
        const uint32_t *orders[WSA_TRAIN_GROUP_MAX];
        wsa_train_stats s[WSA_TRAIN_GROUP_MAX];
        for (uint32_t k = 0; k < n_live; k++) {
            const train_job *j = g->job[live[k]];
            orders[k] = j->orders ? j->orders + (size_t)e * (j->n - j->n_val) : NULL;
        }
        g->st = wsa_train_group_epoch(grp, orders, g->box->queue);
        if (g->st == WSA_OK) g->st = wsa_train_group_stats(grp, g->box->queue, s);
        if (g->st != WSA_OK) break;
        for (uint32_t k = 0; k < n_live; k++) {
            train_job *j = g->job[live[k]];
            j->history[4 * e] = s[k].loss; j->history[4 * e + 1] = s[k].acc; j->history[4 * e + 2] = s[k].val_loss; j->history[4 * e + 3] = s[k].val_acc;
            train_group_msg *m = malloc(sizeof *m);
            if (m) { m->g = g; m->member = live[k]; m->epoch = (int32_t)e; m->s = s[k]; if (napi_call_threadsafe_function(g->tsfn, m, napi_tsfn_blocking) != napi_ok) free(m); }
        }
    }
    if (g->st != WSA_OK) snprintf(g->err, sizeof g->err, "%s", wsa_last_error(ctx));
    if (grp) wsa_train_group_destroy(grp);                               /* before its members */
    for (uint32_t i = 0; i < g->n; i++) {
        if (g->st == WSA_OK && t[i]) {
            g->st = wsa_trainer_copy_weights(t[i], g->box->queue, g->job[i]->kernel, g->job[i]->bias);
            if (g->st != WSA_OK) snprintf(g->err, sizeof g->err, "%s", wsa_last_error(ctx));
        }
        if (t[i]) wsa_trainer_destroy(t[i]);
    }
    train_group_msg *m = malloc(sizeof *m);                              /* (a few bytes: if even this fails the Promise stays pending) */
    if (m) { m->g = g; m->member = 0; m->epoch = -1; napi_call_threadsafe_function(g->tsfn, m, napi_tsfn_blocking); }
    return NULL;
}
static void train_group_call_js(napi_env env, napi_value js_cb, void *context, void *data) {
    train_group_msg *m = (train_group_msg *)data;
    train_group_job *g = m->g;
    if (!env) { free(m); return; }
    if (m->epoch >= 0) {
        train_on_epoch(env, g->job[m->member], m->epoch, &m->s);
        free(m);
        return;
    }
    free(m);
    pthread_join(g->thread, NULL);
    if (g->box->children) g->box->children--;
    if (g->st != WSA_OK) {
        napi_value msg; napi_create_string_utf8(env, g->err, NAPI_AUTO_LENGTH, &msg);
        napi_reject_deferred(env, g->deferred, msg);
    } else {
        napi_value out; napi_create_array_with_length(env, (size_t)g->n, &out);
        for (uint32_t i = 0; i < g->n; i++) napi_set_element(env, out, i, train_result(env, g->job[i]));
        napi_resolve_deferred(env, g->deferred, out);
    }
    napi_release_threadsafe_function(g->tsfn, napi_tsfn_release);
    train_group_free(env, g);
}
static napi_value fn_train_group(napi_env env, napi_callback_info info) {
    size_t argc = 2; napi_value argv[2];
    NAPI_OK(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
    ctx_box *box = argc ? get_box(env, argv[0]) : NULL;
    const char *usage = "trainGroup(ctx, [[spec, run, onEpoch?], ...]): 1 .. 32 jobs, each with train's arguments";
    bool is_array = false; uint32_t n = 0;
    if (!box || !box->ctx || argc < 2 || napi_is_array(env, argv[1], &is_array) != napi_ok || !is_array || napi_get_array_length(env, argv[1], &n) != napi_ok ||
        n < 1 || n > WSA_TRAIN_GROUP_MAX) { napi_throw_type_error(env, NULL, usage); return NULL; }
    train_group_job *g = calloc(1, sizeof *g);
    if (!g) { napi_throw_error(env, NULL, "out of memory"); return NULL; }
    g->box = box;
    for (uint32_t i = 0; i < n; i++) {
        napi_value item, a[4]; bool ia = false; uint32_t len = 0;
        if (napi_get_element(env, argv[1], i, &item) != napi_ok || napi_is_array(env, item, &ia) != napi_ok || !ia || napi_get_array_length(env, item, &len) != napi_ok ||
            len < 2 || len > 3) { train_group_free(env, g); napi_throw_type_error(env, NULL, usage); return NULL; }
        a[0] = argv[0];
        for (uint32_t k = 0; k < len; k++) if (napi_get_element(env, item, k, &a[k + 1]) != napi_ok) { train_group_free(env, g); napi_throw_type_error(env, NULL, usage); return NULL; }
        train_job *j = train_job_from(env, box, (size_t)len + 1, a);
        if (!j) { train_group_free(env, g); return NULL; }
        g->job[g->n++] = j;
    }
    napi_value promise, name;
    if (napi_create_promise(env, &g->deferred, &promise) != napi_ok || napi_create_string_utf8(env, "wsa_train_group", NAPI_AUTO_LENGTH, &name) != napi_ok ||
        napi_create_threadsafe_function(env, NULL, NULL, name, 0, 1, NULL, NULL, NULL, train_group_call_js, &g->tsfn) != napi_ok) {
        train_group_free(env, g); napi_throw_error(env, NULL, "trainGroup: could not set up the job"); return NULL;
    }
    box->children++;                                             /* until the run's last message: destroy() refuses meanwhile */
    if (pthread_create(&g->thread, NULL, train_group_thread, g) != 0) {
        box->children--; napi_release_threadsafe_function(g->tsfn, napi_tsfn_release);
        napi_value msg; napi_create_string_utf8(env, "trainGroup: could not start a thread", NAPI_AUTO_LENGTH, &msg); napi_reject_deferred(env, g->deferred, msg);
        train_group_free(env, g);
    }
    return promise;
}

/* ---- a regression model's values (wsa_regress_rows): regressRows(ctx, model, features: Float64Array [n][the model's inputs], outMin, outMax) -> Float64Array [n].
 * What the app's predict_db_nn does over stored rows (ref src/neuralmodel.js:410-535).  Synchronous: the rows go through one page-locked
 * allocation the device reads and writes in place. */
static napi_value fn_regress_rows(napi_env env, napi_callback_info info) {
    size_t argc = 5; napi_value argv[5]; void *p = NULL;
    NAPI_OK(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
    ctx_box *box = argc ? get_box(env, argv[0]) : NULL;
    const char *usage = "regressRows(ctx, model, features: Float64Array [n][the model's inputs], outMin, outMax)";
    bool ta = false; napi_typedarray_type tt; size_t nf = 0; void *feat = NULL; double lo = 0, hi = 0;
    if (!box || !box->ctx || argc < 5 || napi_get_value_external(env, argv[1], &p) != napi_ok || !p ||
        napi_is_typedarray(env, argv[2], &ta) != napi_ok || !ta || napi_get_typedarray_info(env, argv[2], &tt, &nf, &feat, NULL, NULL) != napi_ok ||
        tt != napi_float64_array ||
        napi_get_value_double(env, argv[3], &lo) != napi_ok || napi_get_value_double(env, argv[4], &hi) != napi_ok) { napi_throw_type_error(env, NULL, usage); return NULL; }
    model_box *mb = (model_box *)p;
    if (!mb->m || mb->owner != box) { napi_throw_error(env, NULL, "regressRows: the model was destroyed or belongs to another context"); return NULL; }
    if (nf % mb->n_inputs || nf / mb->n_inputs > 0xffffffffu) { napi_throw_type_error(env, NULL, usage); return NULL; }
    const size_t n = nf / mb->n_inputs;
    void *slab = NULL;
    if (wsa_host_alloc(box->ctx, (uint64_t)(nf + n) * sizeof(double), &slab) != WSA_OK) { napi_throw_error(env, NULL, wsa_last_error(box->ctx)); return NULL; }
    double *rows = (double *)slab, *value = rows + nf;
    if (nf) memcpy(rows, feat, nf * sizeof(double));
    wsa_status st = wsa_regress_rows(mb->m, lo, hi, rows, (uint32_t)n, value, box->queue);
    if (st == WSA_OK) st = wsa_queue_synchronize(box->ctx, box->queue);
    napi_value out = NULL;
    if (st == WSA_OK) out = make_typed(env, napi_float64_array, value, n, sizeof(double));
    else napi_throw_error(env, NULL, wsa_last_error(box->ctx));
    wsa_host_free(slab);
    return out;
}

/* ---- predicting a labelled feature DB and the app's results table (wsa_dbstats_*, K8, specification DS-1): what the app's Predict button does over
 * the stored rows (ref src/neuralmodel.js:410-535 predict_db_nn, src/localstore.js:498-627 shows_stats_table).  Both calls are synchronous and
 * build the device object for the call; js/dbstats.js resolves everything that is a string and hands over indices and values.
 *   dbPredict(ctx, model, features: Float64Array [n][the model's inputs], ords: boolean, outMin, outMax) -> Int32Array [n] legend indices (-1 = the reference's
 *     null) for a classifier, Float64Array [n] values for a regression model
 *   dbTable(ctx, {durations: Float64Array [n], vocab: Uint32Array [nCat], trueIdx, predIdx: Int32Array [nCat][n], trueVal, predVal: Float64Array
 *     [nOrd][n]}) -> {cat: Float64Array [nCat][3] correct, wrong, blank; cls: Float64Array [sum vocab][5] count, correct, wrong, duration,
 *     first_row (4294967295 = none); ord: Float64Array [nOrd][5] true_n, pred_n, min, max, sq_sum} */
static int typed_arg(napi_env env, napi_value v, napi_typedarray_type want, void **data, size_t *len) {
    bool ta = false; napi_typedarray_type t;
    if (napi_is_typedarray(env, v, &ta) != napi_ok || !ta) return 0;
    return napi_get_typedarray_info(env, v, &t, len, data, NULL, NULL) == napi_ok && t == want;
}
static napi_value fn_db_predict(napi_env env, napi_callback_info info) {
    size_t argc = 6; napi_value argv[6]; void *p = NULL;
    NAPI_OK(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
    ctx_box *box = argc ? get_box(env, argv[0]) : NULL;
    const char *usage = "dbPredict(ctx, model, features: Float64Array [n][the model's inputs], ords: boolean, outMin, outMax)";
    size_t nf = 0; void *feat = NULL; bool ords = false; double lo = 0, hi = 1;
    if (!box || !box->ctx || argc < 4 || napi_get_value_external(env, argv[1], &p) != napi_ok || !p || !typed_arg(env, argv[2], napi_float64_array, &feat, &nf) ||
        napi_get_value_bool(env, argv[3], &ords) != napi_ok ||
        (ords && (argc < 6 || napi_get_value_double(env, argv[4], &lo) != napi_ok || napi_get_value_double(env, argv[5], &hi) != napi_ok))) {
        napi_throw_type_error(env, NULL, usage); return NULL;
    }
    model_box *mb = (model_box *)p;
    if (!mb->m || mb->owner != box) { napi_throw_error(env, NULL, "dbPredict: the model was destroyed or belongs to another context"); return NULL; }
    if (nf % mb->n_inputs || nf / mb->n_inputs > 0xffffffffu) { napi_throw_type_error(env, NULL, usage); return NULL; }
    const uint32_t n = (uint32_t)(nf / mb->n_inputs), vocab = mb->n_classes;
    double *dur = calloc(n ? n : 1, sizeof(double));
    void *out = malloc((n ? n : 1) * sizeof(double));
    int32_t map[WSA_MODEL_MAX_CLASSES];
    for (int c = 0; c < WSA_MODEL_MAX_CLASSES; c++) map[c] = c;
    wsa_dbstats *db = NULL;
    wsa_status st = dur && out ? wsa_wide_dbstats_create(box->ctx, (const double *)feat, mb->n_inputs, dur, n, ords ? 0 : 1, &vocab, ords ? 1 : 0, &db) : WSA_ERR_INVALID;
    if (st == WSA_OK) st = ords ? wsa_dbstats_predict_values(db, 0, mb->m, lo, hi, box->queue) : wsa_dbstats_predict_classes(db, 0, mb->m, map, box->queue);
    if (st == WSA_OK) st = ords ? wsa_dbstats_copy_values(db, 0, box->queue, (double *)out) : wsa_dbstats_copy_classes(db, 0, box->queue, (int32_t *)out);
    napi_value res = NULL;
    if (st == WSA_OK) res = ords ? make_typed(env, napi_float64_array, out, n, sizeof(double)) : make_typed(env, napi_int32_array, out, n, sizeof(int32_t));
    else napi_throw_error(env, NULL, dur && out ? wsa_last_error(box->ctx) : "out of memory");
    if (db) wsa_dbstats_destroy(db);
    free(dur); free(out);
    return res;
}
static napi_value fn_db_table(napi_env env, napi_callback_info info) {
    size_t argc = 2; napi_value argv[2];
    NAPI_OK(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
    ctx_box *box = argc ? get_box(env, argv[0]) : NULL;
    const char *usage = "dbTable(ctx, {durations: Float64Array [n], vocab: Uint32Array [nCat], trueIdx, predIdx: Int32Array [nCat][n], trueVal, predVal: Float64Array [nOrd][n]})";
    double *dur = NULL, *tv = NULL, *pv = NULL; uint32_t *vocab = NULL; int32_t *ti = NULL, *pi = NULL;
    size_t n = 0, n_cat = 0, nti = 0, npi = 0, ntv = 0, npv = 0;
    if (!box || !box->ctx || argc < 2 || !typed_of(env, argv[1], "durations", napi_float64_array, (void **)&dur, &n) ||
        !typed_of(env, argv[1], "vocab", napi_uint32_array, (void **)&vocab, &n_cat) || !typed_of(env, argv[1], "trueIdx", napi_int32_array, (void **)&ti, &nti) ||
        !typed_of(env, argv[1], "predIdx", napi_int32_array, (void **)&pi, &npi) || !typed_of(env, argv[1], "trueVal", napi_float64_array, (void **)&tv, &ntv) ||
        !typed_of(env, argv[1], "predVal", napi_float64_array, (void **)&pv, &npv) || n < 1 || n > 0xffffffffu || nti != n_cat * n || npi != nti || ntv % n || npv != ntv) {
        napi_throw_type_error(env, NULL, usage); return NULL;
    }
    const size_t n_ord = ntv / n;
    if (n_cat > 0xffff || n_ord > 0xffff) { napi_throw_type_error(env, NULL, usage); return NULL; }
    wsa_dbstats *db = NULL;
    wsa_status st = wsa_dbstats_create(box->ctx, NULL, dur, (uint32_t)n, (uint32_t)n_cat, vocab, (uint32_t)n_ord, &db);
    size_t items = 0;
    for (size_t h = 0; st == WSA_OK && h < n_cat; h++) { items += vocab[h]; st = wsa_dbstats_set_classes(db, (uint32_t)h, ti + h * n, pi + h * n); }
    for (size_t o = 0; st == WSA_OK && o < n_ord; o++) st = wsa_dbstats_set_values(db, (uint32_t)o, tv + o * n, pv + o * n);
    wsa_dbstats_cat *cat = calloc(n_cat ? n_cat : 1, sizeof *cat); wsa_dbstats_class *cls = calloc(items ? items : 1, sizeof *cls);
    wsa_dbstats_ord *od = calloc(n_ord ? n_ord : 1, sizeof *od);
    double *flat = calloc((n_cat * 3 + items * 5 + n_ord * 5) + 1, sizeof(double));
    napi_value res = NULL;
    if (st == WSA_OK && !(cat && cls && od && flat)) { napi_throw_error(env, NULL, "out of memory"); goto done; }
    if (st == WSA_OK) st = wsa_dbstats_table(db, box->queue, cat, cls, od);
    if (st != WSA_OK) { napi_throw_error(env, NULL, wsa_last_error(box->ctx)); goto done; }
    {
        double *fc = flat, *fk = fc + n_cat * 3, *fo = fk + items * 5;
        for (size_t h = 0; h < n_cat; h++) { fc[h * 3] = (double)cat[h].correct; fc[h * 3 + 1] = (double)cat[h].wrong; fc[h * 3 + 2] = (double)cat[h].blank; }
        for (size_t i = 0; i < items; i++) {
            fk[i * 5] = (double)cls[i].count; fk[i * 5 + 1] = (double)cls[i].correct; fk[i * 5 + 2] = (double)cls[i].wrong;
            fk[i * 5 + 3] = cls[i].duration; fk[i * 5 + 4] = (double)cls[i].first_row;
        }
        for (size_t o = 0; o < n_ord; o++) {
            fo[o * 5] = (double)od[o].true_n; fo[o * 5 + 1] = (double)od[o].pred_n; fo[o * 5 + 2] = od[o].min; fo[o * 5 + 3] = od[o].max; fo[o * 5 + 4] = od[o].sq_sum;
        }
        napi_value a, b, c;
        if (napi_create_object(env, &res) != napi_ok) { res = NULL; goto done; }
        a = make_typed(env, napi_float64_array, fc, n_cat * 3, sizeof(double));
        b = make_typed(env, napi_float64_array, fk, items * 5, sizeof(double));
        c = make_typed(env, napi_float64_array, fo, n_ord * 5, sizeof(double));
        if (!a || !b || !c || napi_set_named_property(env, res, "cat", a) != napi_ok || napi_set_named_property(env, res, "cls", b) != napi_ok ||
            napi_set_named_property(env, res, "ord", c) != napi_ok) res = NULL;
    }
done:
    if (db) wsa_dbstats_destroy(db);
    free(cat); free(cls); free(od); free(flat);
    return res;
}

/* ---- evaluating a labelled DB beyond the panel (include/wsa_eval.h, K8e, specification EV-1): one synchronous call that builds the device object,
 * predicts the heads that have a model, folds per file and returns every table; js/dbstats.js resolves the strings and assembles the result.
 *   dbEval(ctx, {durations, vocab, trueIdx, predIdx, trueVal, predVal (as dbTable),
 *                features: Float64Array [n][width], width (only with models), catModels: [model | null] per categorical head, catMaps: Int32Array [nCat][64]
 *                legend -> vocabulary, ordModels: [model | null] per ordinal head, ordRange: Float64Array [nOrd][2],
 *                nFiles (0: no file level), fileOfRow, callbackOfRow: Int32Array [n], fileTrueIdx: Int32Array [nCat][nFiles], fileTrueVal: Float64Array [nOrd][nFiles]})
 *     -> {rows: {cat, cls, ord (as dbTable), conf: Float64Array, every head's [V][V + 1] one after the other, agree: Float64Array [nOrd][8] n, mean_true, mean_pred,
 *         var_true, var_pred, cov, ccc, pearson}, predIdx: Int32Array [nCat][n], predVal: Float64Array [nOrd][n] (after the predictions),
 *         files: null | {cat, cls, ord, conf, agree, idx: Int32Array [nCat][nFiles], val: Float64Array [nOrd][nFiles], sums: [Float64Array [nFiles][C] | null]}} */
static int set_typed(napi_env env, napi_value o, const char *name, napi_typedarray_type type, const void *src, size_t count, size_t elt) {
    napi_value v = make_typed(env, type, src, count, elt);
    return v && napi_set_named_property(env, o, name, v) == napi_ok;
}
/* one level's tables into a new object: files = 0 the rows, 1 the files */
static napi_value eval_level(napi_env env, ctx_box *box, wsa_dbstats *db, int files, size_t n_cat, const uint32_t *vocab, size_t n_ord, wsa_status *st) {
    size_t items = 0, cells = 0;
    for (size_t h = 0; h < n_cat; h++) { items += vocab[h]; cells += (size_t)vocab[h] * (vocab[h] + 1); }
    wsa_dbstats_cat *cat = calloc(n_cat ? n_cat : 1, sizeof *cat); wsa_dbstats_class *cls = calloc(items ? items : 1, sizeof *cls);
    wsa_dbstats_ord *od = calloc(n_ord ? n_ord : 1, sizeof *od); wsa_dbstats_agree *ag = calloc(n_ord ? n_ord : 1, sizeof *ag);
    uint64_t *m = calloc(cells ? cells : 1, sizeof *m);
    double *flat = calloc(n_cat * 3 + items * 5 + n_ord * 5 + cells + n_ord * 8 + 1, sizeof(double));
    napi_value res = NULL;
    if (!(cat && cls && od && ag && m && flat)) { *st = WSA_ERR_INVALID; napi_throw_error(env, NULL, "out of memory"); goto done; }
    *st = files ? wsa_dbstats_file_table(db, box->queue, cat, cls, od) : wsa_dbstats_table(db, box->queue, cat, cls, od);
    for (size_t h = 0, off = 0; *st == WSA_OK && h < n_cat; off += (size_t)vocab[h] * (vocab[h] + 1), h++)
        *st = files ? wsa_dbstats_file_confusion(db, (uint32_t)h, box->queue, m + off) : wsa_dbstats_confusion(db, (uint32_t)h, box->queue, m + off);
    if (*st == WSA_OK && n_ord) *st = files ? wsa_dbstats_file_agreement(db, box->queue, ag) : wsa_dbstats_agreement(db, box->queue, ag);
    if (*st != WSA_OK) { napi_throw_error(env, NULL, wsa_last_error(box->ctx)); goto done; }
    {
        double *fc = flat, *fk = fc + n_cat * 3, *fo = fk + items * 5, *fm = fo + n_ord * 5, *fa = fm + cells;
        for (size_t h = 0; h < n_cat; h++) { fc[h * 3] = (double)cat[h].correct; fc[h * 3 + 1] = (double)cat[h].wrong; fc[h * 3 + 2] = (double)cat[h].blank; }
        for (size_t i = 0; i < items; i++) {
            fk[i * 5] = (double)cls[i].count; fk[i * 5 + 1] = (double)cls[i].correct; fk[i * 5 + 2] = (double)cls[i].wrong;
            fk[i * 5 + 3] = cls[i].duration; fk[i * 5 + 4] = (double)cls[i].first_row;
        }
        for (size_t o = 0; o < n_ord; o++) {
            fo[o * 5] = (double)od[o].true_n; fo[o * 5 + 1] = (double)od[o].pred_n; fo[o * 5 + 2] = od[o].min; fo[o * 5 + 3] = od[o].max; fo[o * 5 + 4] = od[o].sq_sum;
            fa[o * 8] = (double)ag[o].n; fa[o * 8 + 1] = ag[o].mean_true; fa[o * 8 + 2] = ag[o].mean_pred; fa[o * 8 + 3] = ag[o].var_true;
            fa[o * 8 + 4] = ag[o].var_pred; fa[o * 8 + 5] = ag[o].cov; fa[o * 8 + 6] = ag[o].ccc; fa[o * 8 + 7] = ag[o].pearson;
        }
        for (size_t i = 0; i < cells; i++) fm[i] = (double)m[i];
        if (napi_create_object(env, &res) != napi_ok ||
            !set_typed(env, res, "cat", napi_float64_array, fc, n_cat * 3, sizeof(double)) || !set_typed(env, res, "cls", napi_float64_array, fk, items * 5, sizeof(double)) ||
            !set_typed(env, res, "ord", napi_float64_array, fo, n_ord * 5, sizeof(double)) || !set_typed(env, res, "conf", napi_float64_array, fm, cells, sizeof(double)) ||
            !set_typed(env, res, "agree", napi_float64_array, fa, n_ord * 8, sizeof(double))) { res = NULL; *st = WSA_ERR_INVALID; napi_throw_error(env, NULL, "dbEval: result allocation failed"); }
    }
done:
    free(cat); free(cls); free(od); free(ag); free(m); free(flat);
    return res;
}
/* element i of the array property `name`: a live model of this context, NULL for null / undefined; *bad set when it is anything else */
static model_box *eval_model(napi_env env, napi_value spec, const char *name, uint32_t i, ctx_box *box, int *bad) {
    napi_value arr, el; bool has = false, is_arr = false; napi_valuetype t; void *p = NULL; uint32_t len = 0;
    if (napi_has_named_property(env, spec, name, &has) != napi_ok || !has) return NULL;
    if (napi_get_named_property(env, spec, name, &arr) != napi_ok || napi_is_array(env, arr, &is_arr) != napi_ok || !is_arr || napi_get_array_length(env, arr, &len) != napi_ok) { *bad = 1; return NULL; }
    if (i >= len || napi_get_element(env, arr, i, &el) != napi_ok || napi_typeof(env, el, &t) != napi_ok) { *bad = 1; return NULL; }
    if (t == napi_null || t == napi_undefined) return NULL;
    if (t != napi_external || napi_get_value_external(env, el, &p) != napi_ok || !p || !((model_box *)p)->m || ((model_box *)p)->owner != box) { *bad = 1; return NULL; }
    return (model_box *)p;
}
static napi_value fn_db_eval(napi_env env, napi_callback_info info) {
    size_t argc = 2; napi_value argv[2];
    NAPI_OK(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
    ctx_box *box = argc ? get_box(env, argv[0]) : NULL;
    const char *usage = "dbEval(ctx, {durations, vocab, trueIdx, predIdx, trueVal, predVal, [features, width, catModels, catMaps, ordModels, ordRange], [nFiles, fileOfRow, callbackOfRow, fileTrueIdx, fileTrueVal]})";
    double *dur = NULL, *tv = NULL, *pv = NULL, *feat = NULL, *range = NULL, *ftv = NULL; uint32_t *vocab = NULL; int32_t *ti = NULL, *pi = NULL, *maps = NULL, *fo = NULL, *co = NULL, *fti = NULL;
    size_t n = 0, n_cat = 0, nti = 0, npi = 0, ntv = 0, npv = 0, nfeat = 0, nmaps = 0, nrange = 0, nfo = 0, nco = 0, nfti = 0, nftv = 0;
    uint32_t width = 0, n_files = 0; napi_value v;
    wsa_dbstats *db = NULL;
    napi_value res = NULL, rows = NULL, files = NULL, sums = NULL;
    int32_t *idx = NULL; double *val = NULL, *fs = NULL;
    wsa_status st = WSA_OK;
    if (!box || !box->ctx || argc < 2 || !typed_of(env, argv[1], "durations", napi_float64_array, (void **)&dur, &n) ||
        !typed_of(env, argv[1], "vocab", napi_uint32_array, (void **)&vocab, &n_cat) || !typed_of(env, argv[1], "trueIdx", napi_int32_array, (void **)&ti, &nti) ||
        !typed_of(env, argv[1], "predIdx", napi_int32_array, (void **)&pi, &npi) || !typed_of(env, argv[1], "trueVal", napi_float64_array, (void **)&tv, &ntv) ||
        !typed_of(env, argv[1], "predVal", napi_float64_array, (void **)&pv, &npv) || n < 1 || n > 0xffffffffu || nti != n_cat * n || npi != nti || ntv % n || npv != ntv) {
        napi_throw_type_error(env, NULL, usage); return NULL;
    }
    const size_t n_ord = ntv / n;
    if (n_cat > WSA_DBSTATS_MAX_HEADS || n_ord > WSA_DBSTATS_MAX_HEADS) { napi_throw_type_error(env, NULL, usage); return NULL; }
    if (napi_get_named_property(env, argv[1], "nFiles", &v) == napi_ok) (void)napi_get_value_uint32(env, v, &n_files);
    if (napi_get_named_property(env, argv[1], "width", &v) == napi_ok) (void)napi_get_value_uint32(env, v, &width);
    const int with_feat = typed_of(env, argv[1], "features", napi_float64_array, (void **)&feat, &nfeat);
    if (with_feat && (!width || nfeat != n * (size_t)width)) { napi_throw_type_error(env, NULL, usage); return NULL; }
    (void)typed_of(env, argv[1], "catMaps", napi_int32_array, (void **)&maps, &nmaps);
    (void)typed_of(env, argv[1], "ordRange", napi_float64_array, (void **)&range, &nrange);
    if (n_files && (!typed_of(env, argv[1], "fileOfRow", napi_int32_array, (void **)&fo, &nfo) || !typed_of(env, argv[1], "callbackOfRow", napi_int32_array, (void **)&co, &nco) ||
                    !typed_of(env, argv[1], "fileTrueIdx", napi_int32_array, (void **)&fti, &nfti) || !typed_of(env, argv[1], "fileTrueVal", napi_float64_array, (void **)&ftv, &nftv) ||
                    nfo != n || nco != n || nfti != n_cat * n_files || nftv != n_ord * n_files)) { napi_throw_type_error(env, NULL, usage); return NULL; }
    model_box *cm[WSA_DBSTATS_MAX_HEADS] = {0}, *om[WSA_DBSTATS_MAX_HEADS] = {0};
    int bad = 0, any = 0;
    for (size_t h = 0; h < n_cat; h++) cm[h] = eval_model(env, argv[1], "catModels", (uint32_t)h, box, &bad);
    for (size_t o = 0; o < n_ord; o++) om[o] = eval_model(env, argv[1], "ordModels", (uint32_t)o, box, &bad);
    if (bad) { napi_throw_error(env, NULL, "dbEval: catModels / ordModels hold one model handle of this context, or null, per head"); return NULL; }
    for (size_t h = 0; h < WSA_DBSTATS_MAX_HEADS; h++) any |= cm[h] != NULL || om[h] != NULL;
    if (any && (!with_feat || nmaps != n_cat * WSA_MODEL_MAX_CLASSES || nrange != n_ord * 2)) { napi_throw_type_error(env, NULL, usage); return NULL; }

    const size_t longest = n > n_files ? n : n_files;
    idx = calloc(n_cat * longest + 1, sizeof *idx); val = calloc(n_ord * longest + 1, sizeof *val);
    fs = calloc((size_t)(n_files ? n_files : 1) * WSA_MODEL_MAX_CLASSES, sizeof *fs);
    if (!idx || !val || !fs) { napi_throw_error(env, NULL, "out of memory"); goto done; }
    st = with_feat ? wsa_wide_dbstats_create(box->ctx, feat, width, dur, (uint32_t)n, (uint32_t)n_cat, vocab, (uint32_t)n_ord, &db)
                   : wsa_dbstats_create(box->ctx, NULL, dur, (uint32_t)n, (uint32_t)n_cat, vocab, (uint32_t)n_ord, &db);
    for (size_t h = 0; st == WSA_OK && h < n_cat; h++) st = wsa_dbstats_set_classes(db, (uint32_t)h, ti + h * n, pi + h * n);
    for (size_t o = 0; st == WSA_OK && o < n_ord; o++) st = wsa_dbstats_set_values(db, (uint32_t)o, tv + o * n, pv + o * n);
    if (st == WSA_OK && n_files) st = wsa_dbstats_set_files(db, fo, co, n_files);
    for (size_t h = 0; st == WSA_OK && n_files && h < n_cat; h++) st = wsa_dbstats_set_file_classes(db, (uint32_t)h, fti + h * n_files);
    for (size_t o = 0; st == WSA_OK && n_files && o < n_ord; o++) st = wsa_dbstats_set_file_values(db, (uint32_t)o, ftv + o * n_files);
    if (st == WSA_OK && n_files && napi_create_array_with_length(env, n_cat, &sums) != napi_ok) { napi_throw_error(env, NULL, "dbEval: result allocation failed"); goto done; }
    for (size_t h = 0; st == WSA_OK && h < n_cat; h++) {       /* a head is folded right after its prediction: the fold reads the probabilities that call kept */
        napi_value s_h = NULL;
        if (cm[h]) {
            st = wsa_dbstats_predict_classes(db, (uint32_t)h, cm[h]->m, maps + h * WSA_MODEL_MAX_CLASSES, box->queue);
            if (st == WSA_OK && n_files) st = wsa_dbstats_fold_files(db, (uint32_t)h, box->queue);
            if (st == WSA_OK && n_files) st = wsa_dbstats_copy_file_sums(db, (uint32_t)h, box->queue, fs, cm[h]->n_classes);
            if (st == WSA_OK && n_files) s_h = make_typed(env, napi_float64_array, fs, (size_t)n_files * cm[h]->n_classes, sizeof(double));
        }
        if (st == WSA_OK && n_files) { if (!s_h) napi_get_null(env, &s_h); napi_set_element(env, sums, (uint32_t)h, s_h); }
    }
    for (size_t o = 0; st == WSA_OK && o < n_ord; o++) {
        if (om[o]) st = wsa_dbstats_predict_values(db, (uint32_t)o, om[o]->m, range[o * 2], range[o * 2 + 1], box->queue);
        if (st == WSA_OK && n_files) st = wsa_dbstats_fold_file_values(db, (uint32_t)o, box->queue);
    }
    for (size_t h = 0; st == WSA_OK && h < n_cat; h++) st = wsa_dbstats_copy_classes(db, (uint32_t)h, box->queue, idx + h * n);
    for (size_t o = 0; st == WSA_OK && o < n_ord; o++) st = wsa_dbstats_copy_values(db, (uint32_t)o, box->queue, val + o * n);
    if (st != WSA_OK) { napi_throw_error(env, NULL, wsa_last_error(box->ctx)); goto done; }
    if (napi_create_object(env, &res) != napi_ok || !set_typed(env, res, "predIdx", napi_int32_array, idx, n_cat * n, sizeof(int32_t)) ||
        !set_typed(env, res, "predVal", napi_float64_array, val, n_ord * n, sizeof(double))) { res = NULL; napi_throw_error(env, NULL, "dbEval: result allocation failed"); goto done; }
    rows = eval_level(env, box, db, 0, n_cat, vocab, n_ord, &st);
    if (!rows) { res = NULL; goto done; }
    napi_set_named_property(env, res, "rows", rows);
    if (n_files) {
        files = eval_level(env, box, db, 1, n_cat, vocab, n_ord, &st);
        if (!files) { res = NULL; goto done; }
        for (size_t h = 0; st == WSA_OK && h < n_cat; h++) st = wsa_dbstats_copy_file_classes(db, (uint32_t)h, box->queue, idx + h * n_files);
        for (size_t o = 0; st == WSA_OK && o < n_ord; o++) st = wsa_dbstats_copy_file_values(db, (uint32_t)o, box->queue, val + o * n_files);
        if (st != WSA_OK) { res = NULL; napi_throw_error(env, NULL, wsa_last_error(box->ctx)); goto done; }
        if (!set_typed(env, files, "idx", napi_int32_array, idx, n_cat * n_files, sizeof(int32_t)) || !set_typed(env, files, "val", napi_float64_array, val, n_ord * n_files, sizeof(double)) ||
            napi_set_named_property(env, files, "sums", sums) != napi_ok) { res = NULL; napi_throw_error(env, NULL, "dbEval: result allocation failed"); goto done; }
    } else napi_get_null(env, &files);
    napi_set_named_property(env, res, "files", files);
done:
    if (db) wsa_dbstats_destroy(db);
    free(idx); free(val); free(fs);
    return res;
}

/* ---- the feature DB that stays on the device (wsa_featdb_*, K10, specification FD-1).  Every call is synchronous, on the context's own stream.
 *   featdbCreate(ctx, width, capacity) -> handle;  featdbDestroy(handle);  featdbCount(handle) -> rows held
 *   featdbAppendBatch(ctx, db) -> {first, kept: Int32Array}: the rows of the context's last processBatch that the app's storing keeps
 *     (wsa_featdb_append_batch on its kept plan), kept[i] = the source row (level 11: utterance row) of DB row first + i
 *   featdbCopyRows(db) -> Float64Array [count][width];  featdbRanges(db, rows: Uint32Array) -> {min, max}: Float64Array [width] */
static void fdb_finalize(napi_env env, void *data, void *hint) {
    fdb_box *fb = (fdb_box *)data;
    if (!fb->db && !fb->owner) free(fb);             /* a live DB stays (explicit destroy only, as models) */
}
static fdb_box *get_fdb(napi_env env, napi_value v) {
    void *p = NULL; napi_valuetype t = napi_undefined;
    if (napi_typeof(env, v, &t) != napi_ok || t != napi_external || napi_get_value_external(env, v, &p) != napi_ok) return NULL;
    return (fdb_box *)p;
}
static napi_value fn_featdb_create(napi_env env, napi_callback_info info) {
    size_t argc = 3; napi_value argv[3];
    NAPI_OK(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
    ctx_box *box = argc ? get_box(env, argv[0]) : NULL;
    int32_t width = 0; uint32_t cap = 0;
    if (!box || !box->ctx || argc < 3 || napi_get_value_int32(env, argv[1], &width) != napi_ok || napi_get_value_uint32(env, argv[2], &cap) != napi_ok) {
        napi_throw_type_error(env, NULL, "featdbCreate(ctx, width, capacity)"); return NULL;
    }
    wsa_featdb *db = NULL;
    if (wsa_featdb_create(box->ctx, width, cap, &db) != WSA_OK) { napi_throw_error(env, NULL, wsa_last_error(box->ctx)); return NULL; }
    fdb_box *fb = calloc(1, sizeof *fb);
    if (!fb) { wsa_featdb_destroy(db); napi_throw_error(env, NULL, "out of memory"); return NULL; }
    fb->db = db; fb->owner = box; fb->width = (uint32_t)width; fb->next = box->fdbs; box->fdbs = fb;
    napi_value ext; NAPI_OK(env, napi_create_external(env, fb, fdb_finalize, NULL, &ext));
    return ext;
}
static napi_value fn_featdb_destroy(napi_env env, napi_callback_info info) {
    size_t argc = 1; napi_value argv[1];
    NAPI_OK(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
    fdb_box *fb = argc ? get_fdb(env, argv[0]) : NULL;
    if (!fb) { napi_throw_type_error(env, NULL, "featdbDestroy(db)"); return NULL; }
    if (fb->owner && fb->owner->children) { napi_throw_error(env, NULL, "the device DB's context has a batch or a training run in flight"); return NULL; }
    if (fb->db) { wsa_featdb_destroy(fb->db); fb->db = NULL; }
    fdb_unlink(fb);
    return NULL;
}
/* the live DB of a handle with its context idle, or NULL with an exception pending */
static fdb_box *fdb_idle(napi_env env, napi_value v, const char *usage) {
    fdb_box *fb = get_fdb(env, v);
    if (!fb) { napi_throw_type_error(env, NULL, usage); return NULL; }
    if (!fb->db || !fb->owner || !fb->owner->ctx) { napi_throw_error(env, NULL, "the device DB was destroyed"); return NULL; }
    if (fb->owner->children) { napi_throw_error(env, NULL, "the device DB's context has a batch or a training run in flight"); return NULL; }
    return fb;
}
static napi_value fn_featdb_count(napi_env env, napi_callback_info info) {
    size_t argc = 1; napi_value argv[1];
    NAPI_OK(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
    fdb_box *fb = argc ? fdb_idle(env, argv[0], "featdbCount(db)") : NULL;
    if (!fb) { if (!argc) napi_throw_type_error(env, NULL, "featdbCount(db)"); return NULL; }
    uint32_t n = 0; napi_value out;
    wsa_featdb_count(fb->db, &n);
    NAPI_OK(env, napi_create_uint32(env, n, &out));
    return out;
}
static napi_value fn_featdb_append_batch(napi_env env, napi_callback_info info) {
    size_t argc = 2; napi_value argv[2];
    NAPI_OK(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
    ctx_box *box = argc ? get_box(env, argv[0]) : NULL;
    if (!box || !box->ctx || argc < 2) { napi_throw_type_error(env, NULL, "featdbAppendBatch(ctx, db)"); return NULL; }
    fdb_box *fb = fdb_idle(env, argv[1], "featdbAppendBatch(ctx, db)");
    if (!fb) return NULL;
    if (fb->owner != box) { napi_throw_error(env, NULL, "featdbAppendBatch: the device DB belongs to another context"); return NULL; }
    if (!box->plan) { napi_throw_error(env, NULL, "featdbAppendBatch: no finished processBatch on this context (or one is in flight)"); return NULL; }
    wsa_batch_info bi;
    if (wsa_batch_get_info(box->plan, &bi) != WSA_OK) { napi_throw_error(env, NULL, wsa_last_error(box->ctx)); return NULL; }
    const uint32_t cap = bi.rows_cap > bi.n_clips ? bi.rows_cap : bi.n_clips;
    int32_t *kept = malloc(sizeof(int32_t) * (size_t)(cap ? cap : 1));
    if (!kept) { napi_throw_error(env, NULL, "out of memory"); return NULL; }
    uint32_t first = 0, added = 0;
    napi_value out = NULL, v;
    if (wsa_featdb_append_batch(fb->db, box->plan, box->queue, &first, &added, kept, cap ? cap : 1) != WSA_OK) napi_throw_error(env, NULL, wsa_last_error(box->ctx));
    else if (napi_create_object(env, &out) == napi_ok && napi_create_uint32(env, first, &v) == napi_ok) {
        napi_set_named_property(env, out, "first", v);
        napi_set_named_property(env, out, "kept", make_typed(env, napi_int32_array, kept, added, 4));
    }
    free(kept);
    return out;
}
/* ---- live streams collect into the device DB (wsa_stream_set_featdb, specification FD-2).
 *   streamSetFeatdb(stream, db | null): every streamStep of the stream object appends its rows to the DB on the device; the DB must be of the
 *     stream's context and outlive the stream object (featdbDestroy refuses while the context has open streams)
 *   streamDbRows(stream) -> {first, added, replaced, notFitted, kept: Int32Array, replacedRows: Int32Array [replaced][2]} of the last streamStep */
static napi_value fn_stream_set_featdb(napi_env env, napi_callback_info info) {
    size_t argc = 2; napi_value argv[2];
    NAPI_OK(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
    stream_t *h = argc ? get_stream(env, argv[0]) : NULL;
    if (!h || !h->st || argc < 2) { napi_throw_type_error(env, NULL, "streamSetFeatdb(stream, db | null)"); return NULL; }
    fdb_box *fb = NULL;
    napi_valuetype t;
    NAPI_OK(env, napi_typeof(env, argv[1], &t));
    if (t != napi_null && t != napi_undefined) {
        fb = get_fdb(env, argv[1]);
        if (!fb || !fb->db || !fb->owner) { napi_throw_error(env, NULL, "streamSetFeatdb: the device DB was destroyed (or is not a device DB)"); return NULL; }
        if (fb->owner != h->box) { napi_throw_error(env, NULL, "streamSetFeatdb: the device DB belongs to another context"); return NULL; }
    }
    if (wsa_stream_set_featdb(h->st, fb ? fb->db : NULL) != WSA_OK) { napi_throw_error(env, NULL, wsa_last_error(h->ctx)); return NULL; }
    return NULL;
}
static napi_value fn_stream_db_rows(napi_env env, napi_callback_info info) {
    size_t argc = 1; napi_value argv[1];
    NAPI_OK(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
    stream_t *h = argc ? get_stream(env, argv[0]) : NULL;
    if (!h || !h->st) { napi_throw_type_error(env, NULL, "streamDbRows(stream)"); return NULL; }
    wsa_stream_db_result r;
    if (wsa_stream_db_rows(h->st, &r) != WSA_OK) { napi_throw_error(env, NULL, wsa_last_error(h->ctx)); return NULL; }
    napi_value out = NULL, v;
    NAPI_OK(env, napi_create_object(env, &out));
    const struct { const char *name; uint32_t val; } words[] = {{"first", r.first_row}, {"added", r.n_added}, {"replaced", r.n_replaced}, {"notFitted", r.not_fitted}};
    for (size_t i = 0; i < 4; i++) { NAPI_OK(env, napi_create_uint32(env, words[i].val, &v)); napi_set_named_property(env, out, words[i].name, v); }
    napi_set_named_property(env, out, "kept", make_typed(env, napi_int32_array, r.kept, r.n_added, 4));
    napi_set_named_property(env, out, "replacedRows", make_typed(env, napi_int32_array, r.replaced, r.replaced ? 2 * (size_t)r.n_replaced : 0, 4));
    return out;
}
static napi_value fn_featdb_copy_rows(napi_env env, napi_callback_info info) {
    size_t argc = 1; napi_value argv[1];
    NAPI_OK(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
    fdb_box *fb = argc ? fdb_idle(env, argv[0], "featdbCopyRows(db)") : NULL;
    if (!fb) { if (!argc) napi_throw_type_error(env, NULL, "featdbCopyRows(db)"); return NULL; }
    uint32_t n = 0;
    wsa_featdb_count(fb->db, &n);
    napi_value ab, ta; void *data = NULL;
    const size_t words = (size_t)n * fb->width;
    if (napi_create_arraybuffer(env, words * sizeof(double), &data, &ab) != napi_ok || napi_create_typedarray(env, napi_float64_array, words, ab, 0, &ta) != napi_ok) {
        napi_throw_error(env, NULL, "out of memory"); return NULL;
    }
    if (wsa_featdb_copy_rows(fb->db, fb->owner->queue, 0, n, (double *)data) != WSA_OK) { napi_throw_error(env, NULL, wsa_last_error(fb->owner->ctx)); return NULL; }
    return ta;
}
static napi_value fn_featdb_ranges(napi_env env, napi_callback_info info) {
    size_t argc = 2; napi_value argv[2];
    NAPI_OK(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
    const char *usage = "featdbRanges(db, rows: Uint32Array)";
    fdb_box *fb = argc ? fdb_idle(env, argv[0], usage) : NULL;
    if (!fb) { if (!argc) napi_throw_type_error(env, NULL, usage); return NULL; }
    void *rows = NULL; size_t n = 0;
    if (argc < 2 || !typed_arg(env, argv[1], napi_uint32_array, &rows, &n) || n < 1 || n > 0xffffffffu) { napi_throw_type_error(env, NULL, usage); return NULL; }
    double mn[WSA_NUTT], mx[WSA_NUTT];
    if (wsa_featdb_ranges(fb->db, (const uint32_t *)rows, (uint32_t)n, fb->owner->queue, mn, mx) != WSA_OK) { napi_throw_error(env, NULL, wsa_last_error(fb->owner->ctx)); return NULL; }
    napi_value out; NAPI_OK(env, napi_create_object(env, &out));
    napi_set_named_property(env, out, "min", make_typed(env, napi_float64_array, mn, fb->width, 8));
    napi_set_named_property(env, out, "max", make_typed(env, napi_float64_array, mx, fb->width, 8));
    return out;
}

/* ---- the app's ml5 KNN classifier (wsa_knn_*, K9, specification KN-1): what train_knn does with ml5.KNNClassifier() (ref src/neuralmodel.js:729-837).
 * js/knn.js resolves the labels (ml5's class order) and hands over class indices.  Every call is synchronous; rows travel through one page-locked
 * allocation the device reads and writes in place.
 *   knnCreate(ctx, width, nClasses, capacity) -> handle;  knnDestroy(handle)
 *   knnAdd(knn, features: Float64Array [n][width], classes: Int32Array [n]) -> {rows, perClass: Uint32Array [nClasses]}  (addExample, n rows at once)
 *   knnClassify(knn, features: Float64Array [n][width], k) -> {label: Int32Array [n], conf: Float64Array [n][nClasses], nbr: Int32Array [n][k],
 *     sim: Float32Array [n][k], k, kEff, nClasses}  (the tables of wsa_knn_classify_rows)
 *   batchKnn(ctx, knn, k) -> the same tables over the rows of the context's last processBatch (wsa_batch_knn on its kept plan; level 11: the
 *     utterance rows) */
static void knn_finalize(napi_env env, void *data, void *hint) {
    knn_box *kb = (knn_box *)data;
    if (!kb->k && !kb->owner) free(kb);              /* a live store stays (explicit destroy only, as models) */
}
static knn_box *get_knn(napi_env env, napi_value v) {
    void *p = NULL; napi_valuetype t = napi_undefined;
    if (napi_typeof(env, v, &t) != napi_ok || t != napi_external || napi_get_value_external(env, v, &p) != napi_ok) return NULL;
    return (knn_box *)p;
}
static napi_value fn_knn_create(napi_env env, napi_callback_info info) {
    size_t argc = 4; napi_value argv[4];
    NAPI_OK(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
    ctx_box *box = argc ? get_box(env, argv[0]) : NULL;
    int32_t width = 0, classes = 0; uint32_t cap = 0;
    if (!box || !box->ctx || argc < 4 || napi_get_value_int32(env, argv[1], &width) != napi_ok || napi_get_value_int32(env, argv[2], &classes) != napi_ok ||
        napi_get_value_uint32(env, argv[3], &cap) != napi_ok) { napi_throw_type_error(env, NULL, "knnCreate(ctx, width, nClasses, capacity)"); return NULL; }
    wsa_knn *k = NULL;
    if (wsa_knn_create(box->ctx, width, classes, cap, &k) != WSA_OK) { napi_throw_error(env, NULL, wsa_last_error(box->ctx)); return NULL; }
    knn_box *kb = calloc(1, sizeof *kb);
    if (!kb) { wsa_knn_destroy(k); napi_throw_error(env, NULL, "out of memory"); return NULL; }
    kb->k = k; kb->owner = box; kb->width = (uint32_t)width; kb->n_classes = (uint32_t)classes; kb->next = box->knns; box->knns = kb;
    napi_value ext; NAPI_OK(env, napi_create_external(env, kb, knn_finalize, NULL, &ext));
    return ext;
}
static napi_value fn_knn_destroy(napi_env env, napi_callback_info info) {
    size_t argc = 1; napi_value argv[1];
    NAPI_OK(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
    knn_box *kb = argc ? get_knn(env, argv[0]) : NULL;
    if (!kb) { napi_throw_type_error(env, NULL, "knnDestroy(knn)"); return NULL; }
    if (kb->owner && kb->owner->children) { napi_throw_error(env, NULL, "the KNN store's context has a batch in flight or open streams"); return NULL; }
    if (kb->owner) box_drop_plan(kb->owner);         /* the kept plan's KNN tables name the store */
    if (kb->k) { wsa_knn_destroy(kb->k); kb->k = NULL; }
    knn_unlink(kb);
    return NULL;
}
static napi_value fn_knn_add(napi_env env, napi_callback_info info) {
    size_t argc = 3; napi_value argv[3];
    NAPI_OK(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
    const char *usage = "knnAdd(knn, features: Float64Array [n][width], classes: Int32Array [n])";
    knn_box *kb = argc ? get_knn(env, argv[0]) : NULL;
    void *feat = NULL, *cls = NULL; size_t nf = 0, n = 0;
    if (!kb || argc < 3 || !typed_arg(env, argv[1], napi_float64_array, &feat, &nf) || !typed_arg(env, argv[2], napi_int32_array, &cls, &n) ||
        (kb->width && (nf != n * kb->width || n > 0xffffffffu))) { napi_throw_type_error(env, NULL, usage); return NULL; }
    if (!kb->k || !kb->owner || !kb->owner->ctx) { napi_throw_error(env, NULL, "knnAdd: the KNN store was destroyed"); return NULL; }
    ctx_box *box = kb->owner;
    void *slab = NULL;
    if (wsa_host_alloc(box->ctx, (uint64_t)(nf + 1) * sizeof(double) + (uint64_t)(n + 1) * sizeof(int32_t), &slab) != WSA_OK) { napi_throw_error(env, NULL, wsa_last_error(box->ctx)); return NULL; }
    double *rows = (double *)slab; int32_t *ci = (int32_t *)(rows + nf + 1);
    if (nf) memcpy(rows, feat, nf * sizeof(double));
    if (n) memcpy(ci, cls, n * sizeof(int32_t));
    uint32_t total = 0, per[WSA_MODEL_MAX_CLASSES] = {0};
    wsa_status st = wsa_knn_add(kb->k, rows, ci, (uint32_t)n, box->queue);
    if (st == WSA_OK) st = wsa_knn_count(kb->k, box->queue, &total, per);
    napi_value out = NULL;
    if (st == WSA_OK) {
        napi_value nr;
        napi_create_object(env, &out); napi_create_uint32(env, total, &nr);
        napi_set_named_property(env, out, "rows", nr);
        napi_set_named_property(env, out, "perClass", make_typed(env, napi_uint32_array, per, kb->n_classes, 4));
    } else napi_throw_error(env, NULL, wsa_last_error(box->ctx));
    wsa_host_free(slab);
    return out;
}
/* the four tables out of one page-locked slab laid out [label n][nbr n k][sim n k][conf n C] behind `head` bytes */
static napi_value knn_tables(napi_env env, const char *slab, size_t head, size_t n, uint32_t k, uint32_t k_eff, uint32_t C) {
    const int32_t *label = (const int32_t *)(slab + head), *nbr = label + n; const float *sim = (const float *)(nbr + n * k);
    const double *conf = (const double *)(slab + head + ((n + 2 * n * k) * 4 + 7) / 8 * 8);
    napi_value o, v;
    napi_create_object(env, &o);
    napi_set_named_property(env, o, "label", make_typed(env, napi_int32_array, label, n, 4));
    napi_set_named_property(env, o, "nbr", make_typed(env, napi_int32_array, nbr, n * k, 4));
    napi_set_named_property(env, o, "sim", make_typed(env, napi_float32_array, sim, n * k, 4));
    napi_set_named_property(env, o, "conf", make_typed(env, napi_float64_array, conf, n * C, 8));
    napi_create_uint32(env, k, &v); napi_set_named_property(env, o, "k", v);
    napi_create_uint32(env, k_eff, &v); napi_set_named_property(env, o, "kEff", v);
    napi_create_uint32(env, C, &v); napi_set_named_property(env, o, "nClasses", v);
    return o;
}
static size_t knn_tables_bytes(size_t n, uint32_t k, uint32_t C) { return ((n + 2 * n * k) * 4 + 7) / 8 * 8 + n * C * 8 + 8; }
static napi_value fn_knn_classify(napi_env env, napi_callback_info info) {
    size_t argc = 3; napi_value argv[3];
    NAPI_OK(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
    const char *usage = "knnClassify(knn, features: Float64Array [n][width], k)";
    knn_box *kb = argc ? get_knn(env, argv[0]) : NULL;
    void *feat = NULL; size_t nf = 0; uint32_t k = 0;
    if (!kb || argc < 3 || !typed_arg(env, argv[1], napi_float64_array, &feat, &nf) || napi_get_value_uint32(env, argv[2], &k) != napi_ok ||
        (kb->width && (nf % kb->width || nf / kb->width > 0xffffffffu))) { napi_throw_type_error(env, NULL, usage); return NULL; }
    if (!kb->k || !kb->owner || !kb->owner->ctx) { napi_throw_error(env, NULL, "knnClassify: the KNN store was destroyed"); return NULL; }
    if (k < 1 || k > WSA_KNN_MAX_K) { napi_throw_error(env, NULL, "knnClassify: k must be 1 .. 64"); return NULL; }
    ctx_box *box = kb->owner;
    const size_t n = nf / kb->width, head = (nf + 1) * sizeof(double);
    const uint32_t C = kb->n_classes;
    void *slab = NULL;
    if (wsa_host_alloc(box->ctx, (uint64_t)head + knn_tables_bytes(n, k, C), &slab) != WSA_OK) { napi_throw_error(env, NULL, wsa_last_error(box->ctx)); return NULL; }
    char *base = (char *)slab;
    if (nf) memcpy(base, feat, nf * sizeof(double));
    int32_t *label = (int32_t *)(base + head), *nbr = label + n; float *sim = (float *)(nbr + n * k);
    double *conf = (double *)(base + head + ((n + 2 * n * k) * 4 + 7) / 8 * 8);
    uint32_t total = 0;
    wsa_status st = wsa_knn_classify_rows(kb->k, (const double *)base, (uint32_t)n, k, label, conf, nbr, sim, box->queue);
    if (st == WSA_OK) st = wsa_knn_count(kb->k, box->queue, &total, NULL);          /* synchronises; k_eff = min(k, rows) */
    napi_value out = NULL;
    if (st == WSA_OK) out = knn_tables(env, base, head, n, k, k < total ? k : total, C);
    else napi_throw_error(env, NULL, wsa_last_error(box->ctx));
    wsa_host_free(slab);
    return out;
}
static napi_value fn_batch_knn(napi_env env, napi_callback_info info) {
    size_t argc = 3; napi_value argv[3];
    NAPI_OK(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
    ctx_box *box = argc ? get_box(env, argv[0]) : NULL;
    knn_box *kb = argc > 1 ? get_knn(env, argv[1]) : NULL;
    uint32_t k = 0;
    if (!box || !box->ctx || !kb || argc < 3 || napi_get_value_uint32(env, argv[2], &k) != napi_ok) { napi_throw_type_error(env, NULL, "batchKnn(ctx, knn, k)"); return NULL; }
    if (!kb->k || kb->owner != box) { napi_throw_error(env, NULL, "batchKnn: the KNN store was destroyed or belongs to another context"); return NULL; }
    if (!box->plan) { napi_throw_error(env, NULL, "batchKnn: no finished processBatch on this context (or one is in flight)"); return NULL; }
    wsa_knn_result r;
    wsa_status st = wsa_batch_knn(box->plan, kb->k, k, box->queue);
    if (st == WSA_OK) st = wsa_batch_knn_result(box->plan, box->queue, &r);
    if (st != WSA_OK) { napi_throw_error(env, NULL, wsa_last_error(box->ctx)); return NULL; }
    const size_t n = r.n_rows;
    char *buf = malloc(knn_tables_bytes(n, r.k, r.n_classes));
    if (!buf) { napi_throw_error(env, NULL, "out of memory"); return NULL; }
    int32_t *label = (int32_t *)buf, *nbr = label + n; float *sim = (float *)(nbr + n * r.k);
    double *conf = (double *)(buf + ((n + 2 * n * r.k) * 4 + 7) / 8 * 8);
    st = wsa_batch_copy_knn(box->plan, box->queue, label, conf, nbr, sim, (uint32_t)(n ? n : 1));
    napi_value out = NULL;
    if (st == WSA_OK) out = knn_tables(env, buf, 0, n, r.k, r.k_eff, r.n_classes);
    else napi_throw_error(env, NULL, wsa_last_error(box->ctx));
    free(buf);
    return out;
}
/* batchKnnFold(ctx) -> {cb: Int32Array [n][4], cbLabel: Int32Array [n], cbConf: Float64Array [n], clipConf: Float64Array [clips][nClasses], nClasses}:
 * the fold KN-2 over the tables of the context's last batchKnn (wsa_batch_knn_fold; output_level 13) */
static napi_value fn_batch_knn_fold(napi_env env, napi_callback_info info) {
    size_t argc = 1; napi_value argv[1];
    NAPI_OK(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
    ctx_box *box = argc ? get_box(env, argv[0]) : NULL;
    if (!box || !box->ctx) { napi_throw_type_error(env, NULL, "batchKnnFold(ctx)"); return NULL; }
    if (!box->plan) { napi_throw_error(env, NULL, "batchKnnFold: no finished processBatch on this context (or one is in flight)"); return NULL; }
    wsa_knn_fold_result r;
    wsa_status st = wsa_batch_knn_fold(box->plan, box->queue);
    if (st == WSA_OK) st = wsa_batch_knn_fold_result(box->plan, box->queue, &r);
    if (st != WSA_OK) { napi_throw_error(env, NULL, wsa_last_error(box->ctx)); return NULL; }
    const size_t n = r.n_callbacks, nc = (size_t)r.n_clips * r.n_classes;
    double *conf = malloc((n + nc + 1) * sizeof(double));
    int32_t *cb = malloc((5 * n + 1) * sizeof(int32_t));
    napi_value out = NULL;
    if (!conf || !cb) napi_throw_error(env, NULL, "out of memory");
    else if (wsa_batch_copy_knn_fold(box->plan, box->queue, cb, cb + 4 * n, conf, (uint32_t)(n ? n : 1), conf + n) != WSA_OK) napi_throw_error(env, NULL, wsa_last_error(box->ctx));
    else {
        napi_value v;
        napi_create_object(env, &out);
        napi_set_named_property(env, out, "cb", make_typed(env, napi_int32_array, cb, n * 4, 4));
        napi_set_named_property(env, out, "cbLabel", make_typed(env, napi_int32_array, cb + 4 * n, n, 4));
        napi_set_named_property(env, out, "cbConf", make_typed(env, napi_float64_array, conf, n, 8));
        napi_set_named_property(env, out, "clipConf", make_typed(env, napi_float64_array, conf + n, nc, 8));
        napi_create_uint32(env, r.n_classes, &v); napi_set_named_property(env, out, "nClasses", v);
    }
    free(conf); free(cb);
    return out;
}

/* ---- regression groups (wsa_regress_group_*, specification RG-1): V, A and D per callback.  [models]: 1 .. 8 handles of modelCreate on the same context, each a
 * regression model of 53 inputs; outMin / outMax: Float64Array, one range per model.  The library refuses whatever is not one. */
static int group_args(napi_env env, const char *who, napi_value arr, napi_value lo, napi_value hi, ctx_box *box, model_box **mbs, const wsa_model **ms,
                      const double **out_min, const double **out_max, uint32_t *n) {
    char msg[160];
    bool is_arr = false, ta = false; napi_typedarray_type tt; size_t nl = 0, nh = 0; void *pl = NULL, *ph = NULL;
    if (napi_is_array(env, arr, &is_arr) != napi_ok || !is_arr || napi_get_array_length(env, arr, n) != napi_ok || *n < 1 || *n > WSA_REGRESS_GROUP_MAX) {
        snprintf(msg, sizeof msg, "%s: a regression group has 1 .. 8 models", who); napi_throw_error(env, NULL, msg); return 0;
    }
    for (uint32_t d = 0; d < *n; d++) {
        napi_value el; napi_valuetype et = napi_undefined; void *p = NULL;
        if (napi_get_element(env, arr, d, &el) != napi_ok || napi_typeof(env, el, &et) != napi_ok || et != napi_external || napi_get_value_external(env, el, &p) != napi_ok || !p || !((model_box *)p)->m) {
            snprintf(msg, sizeof msg, "%s: a model handle was destroyed (or is not a model)", who); napi_throw_error(env, NULL, msg); return 0;
        }
        mbs[d] = (model_box *)p; ms[d] = mbs[d]->m;
        if (mbs[d]->owner != box) { snprintf(msg, sizeof msg, "%s: a model belongs to another context", who); napi_throw_error(env, NULL, msg); return 0; }
    }
    if (napi_is_typedarray(env, lo, &ta) != napi_ok || !ta || napi_get_typedarray_info(env, lo, &tt, &nl, &pl, NULL, NULL) != napi_ok || tt != napi_float64_array || nl != *n ||
        napi_is_typedarray(env, hi, &ta) != napi_ok || !ta || napi_get_typedarray_info(env, hi, &tt, &nh, &ph, NULL, NULL) != napi_ok || tt != napi_float64_array || nh != *n) {
        snprintf(msg, sizeof msg, "%s: outMin and outMax are Float64Arrays with one entry per model", who); napi_throw_type_error(env, NULL, msg); return 0;
    }
    *out_min = (const double *)pl; *out_max = (const double *)ph;
    return 1;
}
/* streamSetRegress(stream, [models] | null, outMin, outMax): the stream object owns the wsa_regress_group it makes of them, until it is replaced, detached or closed */
static napi_value fn_stream_set_regress(napi_env env, napi_callback_info info) {
    size_t argc = 4; napi_value argv[4];
    NAPI_OK(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
    stream_t *h = argc ? get_stream(env, argv[0]) : NULL;
    if (!h || !h->st || argc < 2) { napi_throw_type_error(env, NULL, "streamSetRegress(stream, [models] | null, outMin, outMax)"); return NULL; }
    model_box *mbs[WSA_REGRESS_GROUP_MAX] = {0}; const wsa_model *ms[WSA_REGRESS_GROUP_MAX]; const double *lo = NULL, *hi = NULL; uint32_t n = 0;
    napi_valuetype t;
    NAPI_OK(env, napi_typeof(env, argv[1], &t));
    if (t != napi_null && t != napi_undefined) {
        if (argc < 4) { napi_throw_type_error(env, NULL, "streamSetRegress(stream, [models] | null, outMin, outMax)"); return NULL; }
        if (!group_args(env, "streamSetRegress", argv[1], argv[2], argv[3], h->box, mbs, ms, &lo, &hi, &n)) return NULL;
    }
    wsa_regress_group *g = NULL;
    if (n && wsa_regress_group_create(h->ctx, ms, lo, hi, n, &g) != WSA_OK) { napi_throw_error(env, NULL, wsa_last_error(h->ctx)); return NULL; }
    if (wsa_stream_set_regress(h->st, g) != WSA_OK) { if (g) wsa_regress_group_destroy(g); napi_throw_error(env, NULL, wsa_last_error(h->ctx)); return NULL; }
    stream_drop_regress(h);
    if (g) {
        h->reg = g; h->n_reg = n; memcpy(h->reg_models, mbs, sizeof h->reg_models);
        for (uint32_t d = 0; d < n; d++) mbs[d]->busy++;            /* modelDestroy() refuses while a stream holds the model */
    }
    return NULL;
}
/* batchRegressGroup(ctx, [models], outMin, outMax) -> {value: Float64Array [H][rows], cb: Int32Array [n][4], cbValue, cbWeight: Float64Array [H][n], clipSum, clipWeight,
 * clipValue: Float64Array [H][clips], nHeads}: the grouped launch and the fold RG-1 over the rows of the context's last processBatch (output_level 5: value and nHeads only) */
static napi_value fn_batch_regress_group(napi_env env, napi_callback_info info) {
    size_t argc = 4; napi_value argv[4];
    NAPI_OK(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
    ctx_box *box = argc ? get_box(env, argv[0]) : NULL;
    if (!box || !box->ctx || argc < 4) { napi_throw_type_error(env, NULL, "batchRegressGroup(ctx, [models], outMin, outMax)"); return NULL; }
    if (!box->plan) { napi_throw_error(env, NULL, "batchRegressGroup: no finished processBatch on this context (or one is in flight)"); return NULL; }
    model_box *mbs[WSA_REGRESS_GROUP_MAX] = {0}; const wsa_model *ms[WSA_REGRESS_GROUP_MAX]; const double *lo = NULL, *hi = NULL; uint32_t H = 0;
    if (!group_args(env, "batchRegressGroup", argv[1], argv[2], argv[3], box, mbs, ms, &lo, &hi, &H)) return NULL;
    bool same = box->reg != NULL && box->reg_n == H;             /* the context's kept group, if it was made of these models and ranges */
    for (uint32_t d = 0; same && d < H; d++) same = box->reg_models[d] == mbs[d] && box->reg_lo[d] == lo[d] && box->reg_hi[d] == hi[d];
    if (!same) {
        wsa_regress_group *g = NULL;
        if (wsa_regress_group_create(box->ctx, ms, lo, hi, H, &g) != WSA_OK) { napi_throw_error(env, NULL, wsa_last_error(box->ctx)); return NULL; }
        box_drop_regress(box);
        box->reg = g; box->reg_n = H; memcpy(box->reg_models, mbs, sizeof box->reg_models);
        for (uint32_t d = 0; d < H; d++) { box->reg_lo[d] = lo[d]; box->reg_hi[d] = hi[d]; }
    }
    wsa_value_result r;
    wsa_status st = wsa_batch_regress_group(box->plan, box->reg, box->queue);
    if (st == WSA_OK) st = wsa_batch_value_result(box->plan, box->queue, &r);
    if (st != WSA_OK) { napi_throw_error(env, NULL, wsa_last_error(box->ctx)); return NULL; }
    const size_t R = r.n_rows, K = r.n_callbacks, N = r.n_clips;
    const int fold = r.d_cb != NULL;
    double *buf = malloc(((size_t)H * (R + 2 * K + 3 * N) + 1) * sizeof(double));
    int32_t *cb = malloc((4 * K + 1) * sizeof(int32_t));
    napi_value out = NULL;
    if (!buf || !cb) napi_throw_error(env, NULL, "out of memory");
    else {
        double *value = buf, *cbv = value + (size_t)H * R, *cbw = cbv + (size_t)H * K, *cs = cbw + (size_t)H * K, *cw = cs + (size_t)H * N, *cv = cw + (size_t)H * N;
        wsa_value_host dst;
        memset(&dst, 0, sizeof dst);
        dst.rows_cap = (uint32_t)(R ? R : 1); dst.cb_cap = (uint32_t)(K ? K : 1);
        for (uint32_t h = 0; h < H; h++) {
            dst.value[h] = value + (size_t)h * R;
            if (!fold) continue;
            dst.cb_value[h] = cbv + (size_t)h * K; dst.cb_weight[h] = cbw + (size_t)h * K;
            dst.clip_sum[h] = cs + (size_t)h * N; dst.clip_weight[h] = cw + (size_t)h * N; dst.clip_value[h] = cv + (size_t)h * N;
        }
        dst.cb = fold ? cb : NULL;
        if (wsa_batch_copy_value_fold(box->plan, box->queue, &dst) != WSA_OK) napi_throw_error(env, NULL, wsa_last_error(box->ctx));
        else {
            napi_value v;
            napi_create_object(env, &out);
            napi_set_named_property(env, out, "value", make_typed(env, napi_float64_array, value, (size_t)H * R, 8));
            if (fold) {
                napi_set_named_property(env, out, "cb", make_typed(env, napi_int32_array, cb, K * 4, 4));
                napi_set_named_property(env, out, "cbValue", make_typed(env, napi_float64_array, cbv, (size_t)H * K, 8));
                napi_set_named_property(env, out, "cbWeight", make_typed(env, napi_float64_array, cbw, (size_t)H * K, 8));
                napi_set_named_property(env, out, "clipSum", make_typed(env, napi_float64_array, cs, (size_t)H * N, 8));
                napi_set_named_property(env, out, "clipWeight", make_typed(env, napi_float64_array, cw, (size_t)H * N, 8));
                napi_set_named_property(env, out, "clipValue", make_typed(env, napi_float64_array, cv, (size_t)H * N, 8));
            }
            napi_create_uint32(env, H, &v); napi_set_named_property(env, out, "nHeads", v);
        }
    }
    free(buf); free(cb);
    return out;
}

NAPI_MODULE_INIT() {
    /* the structures below follow the header this file was compiled against: refuse a libwsa.so of another ABI version */
    if (wsa_abi_version() != WSA_ABI_VERSION) { napi_throw_error(env, NULL, "libwsa.so ABI version differs from the one wsa_napi.node was built against (include/wsa.h): rebuild"); return NULL; }
    const struct { const char *name; napi_callback fn; } fns[] = {
        {"abiVersion", fn_abi_version}, {"freePinned", fn_free_pinned}, {"defaults", fn_defaults}, {"create", fn_create}, {"destroy", fn_destroy},
        {"geometry", fn_geometry}, {"allocPinned", fn_alloc_pinned}, {"binsHz", fn_bins_hz}, {"processBatch", fn_process_batch}, {"gatherRows", fn_gather_rows},
        {"streamOpen", fn_stream_open}, {"streamOpenMixed", fn_stream_open_mixed}, {"streamInfo", fn_stream_info}, {"streamPaced", fn_stream_paced}, {"streamInput", fn_stream_input}, {"streamSetInput", fn_stream_set_input}, {"decodePcm", fn_decode_pcm}, {"streamStep", fn_stream_step}, {"streamClose", fn_stream_close}, {"streamSetModel", fn_stream_set_model}, {"streamSetEnsemble", fn_stream_set_ensemble}, {"streamSetKnn", fn_stream_set_knn},
        {"modelCreate", fn_model_create}, {"modelDestroy", fn_model_destroy}, {"train", fn_train}, {"trainGroup", fn_train_group}, {"regressRows", fn_regress_rows},
        {"dbPredict", fn_db_predict}, {"dbTable", fn_db_table}, {"dbEval", fn_db_eval},
        {"knnCreate", fn_knn_create}, {"knnDestroy", fn_knn_destroy}, {"knnAdd", fn_knn_add}, {"knnClassify", fn_knn_classify}, {"batchKnn", fn_batch_knn}, {"batchKnnFold", fn_batch_knn_fold},
        {"streamSetRegress", fn_stream_set_regress}, {"batchRegressGroup", fn_batch_regress_group},
        {"featdbCreate", fn_featdb_create}, {"featdbDestroy", fn_featdb_destroy}, {"featdbCount", fn_featdb_count}, {"featdbAppendBatch", fn_featdb_append_batch},
        {"featdbCopyRows", fn_featdb_copy_rows}, {"featdbRanges", fn_featdb_ranges}, {"streamSetFeatdb", fn_stream_set_featdb}, {"streamDbRows", fn_stream_db_rows}};
    for (size_t i = 0; i < sizeof fns / sizeof fns[0]; i++) {
        napi_value f;
        if (napi_create_function(env, fns[i].name, NAPI_AUTO_LENGTH, fns[i].fn, NULL, &f) != napi_ok) return NULL;
        if (napi_set_named_property(env, exports, fns[i].name, f) != napi_ok) return NULL;
    }
    return exports;
}
