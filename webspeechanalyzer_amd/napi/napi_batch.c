// napi_batch.c — batches: processBatch and gatherRows (napi_async_work: the library runs on a worker thread, the promise settles on the JS thread).  The
// synchronous calls over the plan a finished processBatch leaves in its context's box are in napi_plan.c.
#include <pthread.h>
#include "napi_handles.h"

// ---- processBatch(ctx, clips: Float32Array[] | Int16Array[], fs[, output_level[, analysis_rate[, channels[, deferRows[, model | [models][, formats[,
// select, source]]]]]]])
//   -> Promise<{meta, feat, segments, rowOff, segOff, stageMs[, formants, frameOff][, uttMeta, uttFeat, uttOff][, trackOff, trackPoints, trackRanked]
//               [, nClasses, prob, cb, cbLabel, cbConf, clipConf][, ens]}>
//   runs wsa_batch_create / wsa_batch_run_host / wsa_batch_copy_rows on a worker thread so the JS thread stays free.
//   fs: a number, or a Float64Array with one rate per clip (the clips are then converted to analysisRate, each from its own rate).
//   clips: all Float32Array (mono floats) or all Int16Array (16-bit PCM as a WAV file holds it, interleaved over channels[i] channels given by the
//     optional 6th argument, a Uint32Array; channel 0 is analysed and the conversion runs on the device: wsa_batch_run_host_i16).
//   deferRows: the rows stay on the device (gatherRows collects them from all shards with one RCCL exchange).
//   8th argument: a model of modelCreate on this context (classify the rows: wsa_batch_classify), an array of 1 .. 8 of them (an ensemble:
//     wsa_batch_classify_ensemble, the result gains `ens`), or undefined / null.
//   9th argument (formats): an Int32Array of WSA_PCM_* numbers, one per clip: every clip a Uint8Array over the bytes a file holds, clip i in formats[i]
//     and interleaved over channels[i] channels — any mix of encodings in one batch, unpacked on the device (wsa_batch_run_host_packed, spec PK-2).
//   10th / 11th argument (select, source; with formats): Uint32Arrays, one word per clip: clip i takes channel select[i] (0xFFFFFFFF: the mix) of the bytes
//     of clip source[i], which travel once (wsa_batch_run_host_channels, spec PK-3).  A consumer's entry of the clip array is its source's Uint8Array (its
//     length gives the frames; the library does not read a consumer's pointer).
typedef struct {
    napi_async_work work; napi_deferred deferred;
    wsa_ctx *ctx; double fs; double fs_out;      /* fs_out != fs: convert in front (wsa_batch_create_resampled) */
    double *fs_each;                             /* one rate per clip: wsa_batch_create_mixed, fs is 0 */
    uint32_t n_clips; uint32_t *n_samples; const float **pcm;
    napi_ref *clip_refs; uint32_t n_refs;        /* the clips' typed arrays, kept alive while the worker reads them: n_refs taken so far */
    int is_i16; uint32_t *channels;   /* Int16Array clips (pcm[] then holds int16 pointers) */
    uint32_t *select, *source;        /* one allocation */
    int32_t *formats;                 /* (pcm[] holds byte pointers) */
    wsa_batch *plan; int plan_reused; /* taken from / returned to the box on the JS thread */
    /* results */
    wsa_status st; char err[512];
    uint32_t n_rows, n_segs; int32_t *meta; double *feat; int32_t *segs; uint32_t *row_off, *seg_off; float stage_ms[4];
    uint32_t n_frames; float *formants; uint32_t *frame_off;      /* levels 4 / 10 */
    uint32_t n_utt; int32_t *utt_meta; double *utt_feat; uint32_t *utt_off;   /* level 11 */
    int defer_rows;
    int level; uint32_t trk_segs; uint64_t trk_np, trk_nr; uint64_t *trk_off; int32_t *trk_pts, *trk_rank;   /* level 3 */
    ctx_box *box;                 /* the JS handle's box: one child while the job runs */
    void *queue;                  /* the context's stream (ctx_box.queue) */
    model_box *model;             /* classify the rows with it (levels 5 / 13), or NULL */
    uint32_t n_classes, n_cb; float *prob; int32_t *cb, *cb_label; double *cb_conf, *clip_conf;
    /* ... or with an ensemble of n_ens models: the tables of wsa_batch_copy_ensemble */
    model_box *ens_models[WSA_ENSEMBLE_MAX]; uint32_t n_ens; int ens_done; uint32_t ens_classes[WSA_ENSEMBLE_MAX]; wsa_ensemble_host eh;
} job_t;

static void ens_host_free(wsa_ensemble_host *h) {
    for (int d = 0; d < WSA_ENSEMBLE_MAX; d++) { free(h->prob[d]); free(h->cb_label[d]); free(h->cb_conf[d]); free(h->cb_all_max[d]); free(h->clip_conf[d]); }
    free(h->cb); free(h->cb_db); free(h->cb_top_label); free(h->cb_top_conf); free(h->cb_min_db); free(h->cb_entropy); free(h->clip_min_db);
}
/* everything a job may own (the struct is calloc'ed: what was never allocated is NULL), the clip references taken so far included; JS thread */
static void job_release(napi_env env, job_t *j) {
    for (uint32_t i = 0; i < j->n_refs; i++) napi_delete_reference(env, j->clip_refs[i]);
    ens_host_free(&j->eh);
    free(j->prob); free(j->cb); free(j->cb_label); free(j->cb_conf); free(j->clip_conf);
    free(j->meta); free(j->feat); free(j->segs); free(j->row_off); free(j->seg_off); free(j->formants); free(j->frame_off);
    free(j->utt_meta); free(j->utt_feat); free(j->utt_off); free(j->trk_off); free(j->trk_pts); free(j->trk_rank);
    free(j->n_samples); free(j->fs_each); free((void *)j->pcm); free(j->clip_refs); free(j->channels); free(j->formats); free(j->select); free(j);
}

/* -- the worker's steps, one per result family: each returns the library's status; out of memory leaves its text in j->err */
static wsa_status job_oom(job_t *j) { snprintf(j->err, sizeof j->err, "out of memory"); return WSA_ERR_INVALID; }
static wsa_status job_plan(job_t *j) {          /* the context's stream and a planned batch of this shape */
    if (!j->box->queue) {           /* (one job at a time uses a context, so nobody else looks at the box's stream now) */
        const wsa_status st = wsa_queue_create(j->ctx, &j->box->queue);
        if (st != WSA_OK) return st;
    }
    j->queue = j->box->queue;
    if (j->plan) return WSA_OK;
    wsa_batch *b = NULL;
    const wsa_status st = j->fs_each ? wsa_batch_create_mixed(j->ctx, j->n_clips, j->n_samples, j->fs_each, j->fs_out, &b)
                        : (j->fs_out > 0 && j->fs_out != j->fs) ? wsa_batch_create_resampled(j->ctx, j->n_clips, j->n_samples, j->fs, j->fs_out, &b)
                                                                : wsa_batch_create(j->ctx, j->n_clips, j->n_samples, j->fs, &b);
    if (st == WSA_OK) j->plan = b;
    return st;
}
static wsa_status job_run(job_t *j, wsa_device_result *r) {
    wsa_batch *b = j->plan;
    const wsa_status st = j->select ? wsa_batch_run_host_channels(b, (const void *const *)j->pcm, j->formats, j->channels, j->select, j->source, j->queue)
                        : j->formats ? wsa_batch_run_host_packed(b, (const void *const *)j->pcm, j->formats, j->channels, j->queue)
                        : j->is_i16 ? wsa_batch_run_host_i16(b, (const int16_t *const *)j->pcm, j->channels, j->queue) : wsa_batch_run_host(b, j->pcm,
                            j->queue);
    return st != WSA_OK ? st : wsa_batch_result(b, j->queue, r);
}
static wsa_status job_rows(job_t *j, const wsa_device_result *r) {
    const size_t R = OR1(r->n_rows), S = OR1(r->n_segments);
    j->n_rows = r->n_rows; j->n_segs = r->n_segments;
    j->meta = malloc(sizeof(int32_t) * 8 * R); j->feat = malloc(sizeof(double) * WSA_NFEAT * R); j->segs = malloc(sizeof(int32_t) * 4 * S);
    j->row_off = malloc(sizeof(uint32_t) * ((size_t)j->n_clips + 1)); j->seg_off = malloc(sizeof(uint32_t) * ((size_t)j->n_clips + 1));
    if (!j->meta || !j->feat || !j->segs || !j->row_off || !j->seg_off) return job_oom(j);
    return wsa_batch_copy_rows(j->plan, j->queue, j->defer_rows ? NULL : j->meta, j->defer_rows ? NULL : j->feat, (uint32_t)R, j->segs, (uint32_t)S,
        j->row_off, j->seg_off);
}
static wsa_status job_formants(job_t *j, const wsa_device_result *r) {          /* levels 4 / 10: the straightened frames */
    j->n_frames = r->n_frames_total;
    j->formants = malloc(sizeof(float) * 9 * (size_t)OR1(r->n_frames_total)); j->frame_off = malloc(sizeof(uint32_t) * ((size_t)j->n_clips + 1));
    if (!j->formants || !j->frame_off) return job_oom(j);
    const wsa_status st = wsa_batch_copy_formants(j->plan, j->queue, j->formants, OR1(r->n_frames_total));
    return st != WSA_OK ? st : wsa_batch_copy_spectra(j->plan, j->queue, NULL, 0, j->frame_off);
}
static wsa_status job_utterance(job_t *j, const wsa_device_result *r) {         /* level 11: utterance features after every result */
    j->n_utt = r->n_utterance_rows;
    j->utt_meta = malloc(sizeof(int32_t) * 4 * (size_t)OR1(j->n_utt)); j->utt_feat = malloc(sizeof(double) * WSA_NUTT * (size_t)OR1(j->n_utt));
    j->utt_off = malloc(sizeof(uint32_t) * ((size_t)j->n_clips + 1));
    if (!j->utt_meta || !j->utt_feat || !j->utt_off) return job_oom(j);
    return wsa_batch_copy_utterance(j->plan, j->queue, j->utt_meta, j->utt_feat, OR1(j->n_utt), j->utt_off);
}
static wsa_status job_tracks(job_t *j) {                                        /* level 3: the ranked raw tracks (points + ranked ids per segment) */
    wsa_tracks_info ti;
    const wsa_status st = wsa_batch_tracks_info(j->plan, j->queue, &ti);
    if (st != WSA_OK) return st;
    j->trk_segs = ti.n_segments; j->trk_np = ti.n_points; j->trk_nr = ti.n_ranked;
    j->trk_off = malloc(sizeof(uint64_t) * 2 * ((size_t)ti.n_segments + 1));
    j->trk_pts = malloc(sizeof(int32_t) * 8 * (size_t)OR1(ti.n_points)); j->trk_rank = malloc(sizeof(int32_t) * (size_t)OR1(ti.n_ranked));
    if (!j->trk_off || !j->trk_pts || !j->trk_rank) return job_oom(j);
    return wsa_batch_copy_tracks(j->plan, j->queue, j->trk_off, j->trk_pts, ti.n_points, j->trk_rank, ti.n_ranked);
}
static wsa_status job_classes(job_t *j) {                                       /* K6 (+ K6b at level 13) on the batch's rows: the app's classifier */
    wsa_class_result cr;
    wsa_status st = wsa_batch_classify(j->plan, model_of(j->model), j->queue);
    if (st == WSA_OK) st = wsa_batch_class_result(j->plan, j->queue, &cr);
    if (st != WSA_OK) return st;
    const size_t R = OR1(cr.n_rows), K = OR1(cr.n_callbacks);
    j->n_classes = cr.n_classes; j->n_cb = cr.n_callbacks;
    j->prob = malloc(sizeof(float) * (size_t)cr.n_classes * R);
    j->cb = malloc(sizeof(int32_t) * 4 * K); j->cb_label = malloc(sizeof(int32_t) * K); j->cb_conf = malloc(sizeof(double) * K);
    j->clip_conf = malloc(sizeof(double) * (size_t)cr.n_classes * OR1(j->n_clips));
    if (!j->prob || !j->cb || !j->cb_label || !j->cb_conf || !j->clip_conf) return job_oom(j);
    memset(j->clip_conf, 0, sizeof(double) * (size_t)cr.n_classes * j->n_clips);
    return wsa_batch_copy_classes(j->plan, j->queue, j->prob, (uint32_t)R, j->cb, j->cb_label, j->cb_conf, (uint32_t)K, j->clip_conf);
}
/* the context's kept ensemble, if it was made of the job's models, else a new one in its place */
static wsa_status job_ensemble_of_box(job_t *j) {
    ctx_box *bx = j->box;
    int same = bx->ens && bx->ens_n == j->n_ens;
    for (uint32_t d = 0; same && d < j->n_ens; d++) same = bx->ens_models[d] == j->ens_models[d];
    if (same) return WSA_OK;
    const wsa_model *ms[WSA_ENSEMBLE_MAX];
    for (uint32_t d = 0; d < j->n_ens; d++) ms[d] = model_of(j->ens_models[d]);
    box_drop_ensemble(bx);
    const wsa_status st = wsa_ensemble_create(j->ctx, ms, j->n_ens, &bx->ens);
    if (st == WSA_OK) { bx->ens_n = j->n_ens; memcpy(bx->ens_models, j->ens_models, sizeof bx->ens_models); }
    return st;
}
static wsa_status job_ensemble(job_t *j) {                /* K6e (+ K6b-e and the decision at level 13): every model DB of the app at once */
    wsa_ensemble_result er;
    wsa_status st = job_ensemble_of_box(j);
    if (st == WSA_OK) st = wsa_batch_classify_ensemble(j->plan, j->box->ens, j->queue);
    if (st == WSA_OK) st = wsa_batch_ensemble_result(j->plan, j->queue, &er);
    if (st != WSA_OK) return st;
    const size_t R = OR1(er.n_rows), K = OR1(er.n_callbacks), NC = OR1(j->n_clips);
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
    if (fold) ok = ok && (h->cb = malloc(sizeof(int32_t) * 4 * K)) && (h->cb_db = malloc(sizeof(int32_t) * K))
        && (h->cb_top_label = malloc(sizeof(int32_t) * K))
                   && (h->cb_top_conf = malloc(sizeof(double) * K)) && (h->cb_min_db = malloc(sizeof(int32_t) * K))
                       && (h->cb_entropy = malloc(sizeof(double) * K))
                   && (h->clip_min_db = malloc(sizeof(int32_t) * NC));
    if (!ok) return job_oom(j);
    st = wsa_batch_copy_ensemble(j->plan, j->queue, h);
    if (st == WSA_OK) j->ens_done = fold ? 2 : 1;
    return st;
}
static void job_execute(napi_env env, void *data) {
    job_t *j = (job_t *)data;
    wsa_device_result r;
    wsa_status st = job_plan(j);
    if (st == WSA_OK) st = job_run(j, &r);
    if (st == WSA_OK) st = job_rows(j, &r);
    if (st == WSA_OK && r.d_formants) st = job_formants(j, &r);
    if (st == WSA_OK && r.d_utt_feat) st = job_utterance(j, &r);
    if (st == WSA_OK && j->level == 3) st = job_tracks(j);
    if (st == WSA_OK && j->model) st = job_classes(j);
    if (st == WSA_OK && j->n_ens) st = job_ensemble(j);
    if (st == WSA_OK) wsa_batch_stage_ms(j->plan, j->stage_ms);
    else if (!j->err[0]) snprintf(j->err, sizeof j->err, "%s", wsa_last_error(j->ctx));
    j->st = st;
    /* the plan goes back to the box in job_complete (JS thread) */
}

static napi_value job_result(napi_env env, const job_t *j) {
    napi_value o = new_object(env);
    const size_t offs = (size_t)j->n_clips + 1;
    if (!j->defer_rows) put_rows(env, o, j->meta, j->feat, j->n_rows);
    put_typed(env, o, "segments", napi_int32_array, j->segs, (size_t)j->n_segs * 4);
    put_typed(env, o, "rowOff", napi_uint32_array, j->row_off, offs);
    put_typed(env, o, "segOff", napi_uint32_array, j->seg_off, offs);
    put_typed(env, o, "stageMs", napi_float32_array, j->stage_ms, 4);
    if (j->utt_feat) { put_utterance(env, o, j->utt_meta, j->utt_feat, j->n_utt); put_typed(env, o, "uttOff", napi_uint32_array, j->utt_off, offs); }
    if (j->trk_off) put_tracks(env, o, j->trk_off, j->trk_segs, j->trk_pts, (size_t)j->trk_np, j->trk_rank, (size_t)j->trk_nr);
    if (j->formants) {
        put_typed(env, o, "formants", napi_float32_array, j->formants, (size_t)j->n_frames * 9);
        put_typed(env, o, "frameOff", napi_uint32_array, j->frame_off, offs);
    }
    if (j->prob) {                    /* the classifier's tables (include/wsa.h wsa_batch_copy_classes) */
        const class_view v = {j->n_classes, j->n_rows, j->n_cb, j->n_clips, 1, "clipConf", j->prob, j->cb, j->cb_label, j->cb_conf, j->clip_conf};
        put_u32(env, o, "nClasses", j->n_classes);
        put_classes(env, o, &v);
    }
    if (j->ens_done) {                /* the ensemble's tables (include/wsa.h wsa_batch_copy_ensemble) */
        const wsa_ensemble_host *h = &j->eh;
        const ens_view v = {j->n_ens, j->n_rows, j->n_cb, j->n_clips, j->ens_classes, j->ens_done == 2,
                            (const float *const *)h->prob, (const int32_t *const *)h->cb_label, (const double *const *)h->cb_conf,
                                (const double *const *)h->cb_all_max,
                            (const double *const *)h->clip_conf, h->cb, h->cb_db, h->cb_top_label, h->cb_min_db, h->clip_min_db, h->cb_top_conf, h->cb_entropy};
        put(env, o, "ens", ens_object(env, &v));
    }
    return o;
}
static void job_complete(napi_env env, napi_status status, void *data) {
    job_t *j = (job_t *)data;
    ctx_box *box = j->box;
    if (box && box->children) box->children--;
    if (j->model && j->model->busy) j->model->busy--;
    for (uint32_t d = 0; d < j->n_ens; d++) if (j->ens_models[d]->busy) j->ens_models[d]->busy--;
    if (j->plan) {                       /* keep the plan for the next call of the same shape (one entry; a failed run drops it) */
        if (box && box->ctx && j->st == WSA_OK && !box->plan) {
            box->plan = j->plan; box->plan_n = j->n_clips; box->plan_fs = j->fs; box->plan_fs_out = j->fs_out;
            box->plan_ns = j->n_samples; j->n_samples = NULL; box->plan_fs_each = j->fs_each; j->fs_each = NULL;
        } else wsa_batch_destroy(j->plan);
        j->plan = NULL;
    }
    if (j->st != WSA_OK) settle(env, j->deferred, j->err, NULL);
    else if (status != napi_ok) settle(env, j->deferred, "async work cancelled", NULL);
    else settle(env, j->deferred, NULL, job_result(env, j));
    napi_delete_async_work(env, j->work);
    job_release(env, j);
}

/* -- the parser's steps (JS thread): each returns 1, or 0 with an exception pending */
static const char *BATCH_USAGE = "processBatch(ctx, Float32Array[] | Int16Array[], fs[, level[, analysisRate[, channels[, deferRows]]]])";
/* the model argument: one model, an array of 1 .. 8 of them, or undefined / null */
static int parse_models(napi_env env, size_t argc, const napi_value *argv, job_t *j) {
    uint32_t len = 0;
    if (argc < 8) return 1;
    if (array_arg(env, argv[7], &len)) {
        j->n_ens = model_list_arg(env, argv[7], j->box, WSA_ENSEMBLE_MAX, j->ens_models, NULL, "processBatch: an ensemble has 1 .. 8 models",
                                  "processBatch: a model handle of the ensemble was destroyed (or is not a model)",
                                  "processBatch: a model of the ensemble belongs to another context");
        return j->n_ens != 0;
    }
    if (is_nullish(env, argv[7])) return 1;
    j->model = model_arg(env, argv[7], j->box, "processBatch: the model handle was destroyed (or is not a model)",
        "processBatch: the model belongs to another context");
    return j->model != NULL;
}
/* the clip array's length, the rates (fs: a number, or one rate per clip), level, analysis rate, deferRows; the per-clip tables allocated */
static int parse_rates(napi_env env, size_t argc, const napi_value *argv, job_t *j) {
    double *fs_each = NULL; size_t fs_each_n = 0; bool fs_ok = false; uint32_t n = 0;
    if (argc >= 3) {
        if (napi_get_value_double(env, argv[2], &j->fs) == napi_ok) fs_ok = true;
        else if (typed_arg(env, argv[2], napi_float64_array, (void **)&fs_each, &fs_each_n)) { fs_ok = true; j->fs = 0; }
    }
    if (!j->ctx || argc < 3 || !fs_ok || !array_arg(env, argv[1], &n) || (fs_each && fs_each_n != n)) { fail_usage(env, BATCH_USAGE); return 0; }
    j->n_clips = n;
    if (argc >= 7) { bool d = false; if (napi_get_value_bool(env, argv[6], &d) == napi_ok) j->defer_rows = d ? 1 : 0; }
    /* the ctx's output_level: 3 adds the raw tracks */
    if (argc >= 4) { int32_t lv = 0; if (napi_get_value_int32(env, argv[3], &lv) == napi_ok) j->level = lv; }
    if (argc >= 5) { double fo = 0; if (napi_get_value_double(env, argv[4], &fo) == napi_ok) j->fs_out = fo; }
    if (fs_each) j->fs_each = dup_bytes(fs_each, sizeof(double) * n);
    j->n_samples = calloc(OR1(n), sizeof(uint32_t)); j->pcm = calloc(OR1(n), sizeof(float *)); j->clip_refs = calloc(OR1(n), sizeof(napi_ref));
    if ((fs_each && !j->fs_each) || !j->n_samples || !j->pcm || !j->clip_refs) { fail_oom(env); return 0; }
    return 1;
}
static int parse_formats(napi_env env, size_t argc, const napi_value *argv, job_t *j) {
    const size_t n = j->n_clips; void *fd = NULL;
    if (argc < 9 || is_nullish(env, argv[8])) return 1;
    if (!typed_arg_n(env, argv[8], napi_int32_array, n, &fd)) {
        fail_usage(env, "processBatch: formats is an Int32Array with one WSA_PCM_* number per clip"); return 0;
    }
    j->formats = dup_bytes(fd, sizeof(int32_t) * n); j->channels = calloc(OR1(n), sizeof(uint32_t));
    if (!j->formats || !j->channels) { fail_oom(env); return 0; }
    return 1;
}
static int parse_select(napi_env env, size_t argc, const napi_value *argv, job_t *j) {
    const size_t n = j->n_clips; void *sd = NULL, *ud = NULL;
    if (argc < 11 || !j->formats || is_nullish(env, argv[9])) return 1;
    if (!typed_arg_n(env, argv[9], napi_uint32_array, n, &sd) || !typed_arg_n(env, argv[10], napi_uint32_array, n, &ud)) {
        fail_usage(env, "processBatch: select and source are Uint32Arrays with one word per clip"); return 0;
    }
    j->select = malloc(sizeof(uint32_t) * 2 * OR1(n));
    if (!j->select) { fail_oom(env); return 0; }
    j->source = j->select + OR1(n);
    memcpy(j->select, sd, sizeof(uint32_t) * n); memcpy(j->source, ud, sizeof(uint32_t) * n);
    return 1;
}
/* clip i of a batch with formats; `ch` its channel count.  NULL, or what is wrong with it */
static const char *clip_packed(napi_env env, job_t *j, uint32_t i, napi_value el, uint32_t ch) {
    const int32_t f = j->formats[i];
    const uint32_t sb = (f == WSA_PCM_F32 || f == WSA_PCM_I32) ? 4u : f == WSA_PCM_I16 ? 2u : f == WSA_PCM_I24 ? 3u : f == WSA_PCM_F64 ? 8u
                      : (f == WSA_PCM_MULAW || f == WSA_PCM_ALAW || f == WSA_PCM_U8) ? 1u : 0u;
    size_t len = 0; void *data = NULL;
    if (!el || !typed_arg(env, el, napi_uint8_array, &data, &len)) return "with formats every clip must be a Uint8Array over the file's bytes";
    if (!sb) return "processBatch: unknown input format";
    if (ch < 1 || ch > 64) return "processBatch: channels must be 1 .. 64";
    j->channels[i] = ch; j->n_samples[i] = (uint32_t)(len / ((size_t)sb * ch)); j->pcm[i] = (const float *)data;
    return NULL;
}
/* clip i of a batch of floats or of 16-bit PCM; `ch` the channel count the caller gave it, 0 for none */
static const char *clip_plain(napi_env env, job_t *j, uint32_t i, napi_value el, uint32_t ch) {
    napi_typedarray_type tt; size_t len = 0; void *data = NULL;
    if (!el || !typed_info(env, el, &tt, &data, &len) || (tt != napi_float32_array && tt != napi_int16_array))
        return "every clip must be a Float32Array or an Int16Array";
    if (i > 0 && (tt == napi_int16_array) != (j->is_i16 != 0)) return "the clips of one batch must be of one kind";
    if (i == 0) { j->is_i16 = tt == napi_int16_array; if (j->is_i16) j->channels = calloc(j->n_clips, sizeof(uint32_t)); }
    if (!j->is_i16 || ch < 1) ch = 1;
    if (j->is_i16) j->channels[i] = ch;
    j->n_samples[i] = (uint32_t)(len / ch); j->pcm[i] = (const float *)data;
    return NULL;
}
/* the clip loop: lengths and pointers, one reference per clip (it keeps the PCM alive while the worker reads it) */
static int parse_clips(napi_env env, size_t argc, const napi_value *argv, job_t *j) {
    uint32_t *chan = NULL; size_t chan_len = 0;
    if (argc >= 6 && !typed_arg(env, argv[5], napi_uint32_array, (void **)&chan, &chan_len)) chan = NULL;
    for (uint32_t i = 0; i < j->n_clips; i++) {
        napi_value el = NULL;
        const int has = chan && i < chan_len;
        if (napi_get_element(env, argv[1], i, &el) != napi_ok) el = NULL;
        const char *bad = j->formats ? clip_packed(env, j, i, el, has ? chan[i] : 1) : clip_plain(env, j, i, el, has ? chan[i] : 0);
        if (bad) { fail_usage(env, bad); return 0; }
        napi_create_reference(env, el, 1, &j->clip_refs[i]);
        j->n_refs = i + 1;
    }
    return 1;
}
/* a plan of exactly this shape waiting in the box?  (one job at a time uses a context: the plan leaves the box while it runs) */
static void take_plan(job_t *j) {
    ctx_box *b = j->box;
    if (!b->plan) return;
    int same = b->plan_n == j->n_clips && b->plan_fs == j->fs && b->plan_fs_out == j->fs_out && (b->plan_fs_each != NULL) == (j->fs_each != NULL);
    for (uint32_t i = 0; same && i < j->n_clips; i++) same = b->plan_ns[i] == j->n_samples[i] && (!j->fs_each || b->plan_fs_each[i] == j->fs_each[i]);
    if (!same) { box_drop_plan(b); return; }
    j->plan = b->plan; j->plan_reused = 1; b->plan = NULL;
    box_drop_plan(b);                     /* (the shape tables alone: the plan is the job's now) */
}
/* the promise of an async work `execute` / `complete` over `data`, queued; NULL with an exception pending */
static napi_value queue_work(napi_env env, const char *what, napi_async_execute_callback execute, napi_async_complete_callback complete, void *data,
                             napi_deferred *deferred, napi_async_work *work) {
    napi_value promise, name;
    NAPI_OK(env, napi_create_promise(env, deferred, &promise));
    NAPI_OK(env, napi_create_string_utf8(env, what, NAPI_AUTO_LENGTH, &name));
    NAPI_OK(env, napi_create_async_work(env, NULL, name, execute, complete, data, work));
    NAPI_OK(env, napi_queue_async_work(env, *work));
    return promise;
}
napi_value fn_process_batch(napi_env env, napi_callback_info info) {
    ARGS(11);
    job_t *j = calloc(1, sizeof *j);
    if (!j) return fail_oom(env);
    j->box = argc ? get_box(env, argv[0]) : NULL; j->ctx = j->box ? j->box->ctx : NULL;
    if (!parse_models(env, argc, argv, j) || !parse_rates(env, argc, argv, j) || !parse_formats(env, argc, argv, j) || !parse_select(env, argc, argv, j) ||
        !parse_clips(env, argc, argv, j)) { job_release(env, j); return NULL; }
    take_plan(j);
    napi_value promise = queue_work(env, "wsa.processBatch", job_execute, job_complete, j, &j->deferred, &j->work);
    if (!promise) return NULL;
    j->box->children++;                                          /* until job_complete */
    if (j->model) j->model->busy++;
    for (uint32_t d = 0; d < j->n_ens; d++) j->ens_models[d]->busy++;
    return promise;
}

// ---- gatherRows(ctx[]) -> Promise<{meta, feat, rowsPerRank}>: the rows of the contexts' last batches (processBatch(..., deferRows = true)) collected on the
// first context's device by one RCCL exchange (wsa_gather_rows) and copied to the host once
typedef struct {
    napi_async_work work; napi_deferred deferred;
    uint32_t n; ctx_box **boxes; wsa_ctx **ctxs; wsa_batch **plans;
    wsa_status st; char err[512];
    uint32_t n_rows; uint32_t *per; int32_t *meta; double *feat;
} gjob_t;
/* the communicator of gatherRows (one at a time; rebuilt when the set of contexts changes, dropped before any of its contexts is destroyed) */
static wsa_gather *g_gather = NULL; static wsa_ctx **g_gather_ctxs = NULL; static uint32_t g_gather_n = 0;
// gatherRows jobs run on libuv worker threads, destroy() on the JS thread: every access to the three words above holds this lock
// (a wsa_gather is not thread-safe either: one exchange at a time)
static pthread_mutex_t g_gather_lock = PTHREAD_MUTEX_INITIALIZER;
static void gather_drop(void) {          /* caller holds g_gather_lock */
    if (g_gather) wsa_gather_destroy(g_gather);
    free(g_gather_ctxs); g_gather = NULL; g_gather_ctxs = NULL; g_gather_n = 0;
}
void gather_forget(wsa_ctx *ctx) {
    pthread_mutex_lock(&g_gather_lock);
    for (uint32_t i = 0; i < g_gather_n; i++) if (g_gather_ctxs[i] == ctx) { gather_drop(); break; }
    pthread_mutex_unlock(&g_gather_lock);
}
static void gjob_release(gjob_t *j) {
    free(j->per); free(j->meta); free(j->feat); free(j->boxes); free(j->ctxs); free(j->plans); free(j);
}
static wsa_status gjob_oom(gjob_t *j) { snprintf(j->err, sizeof j->err, "out of memory"); return WSA_ERR_INVALID; }
static wsa_status gjob_communicator(gjob_t *j) {          /* caller holds g_gather_lock */
    int same = g_gather && g_gather_n == j->n;
    for (uint32_t i = 0; same && i < j->n; i++) same = g_gather_ctxs[i] == j->ctxs[i];
    if (same) return WSA_OK;
    gather_drop();
    const wsa_status st = wsa_gather_create(j->ctxs, (int32_t)j->n, 0, &g_gather);
    if (st != WSA_OK) { snprintf(j->err, sizeof j->err, "%s", wsa_last_error(j->ctxs[0])); g_gather = NULL; return st; }
    g_gather_ctxs = dup_bytes(j->ctxs, sizeof(wsa_ctx *) * j->n); g_gather_n = j->n;
    if (!g_gather_ctxs) { gather_drop(); return gjob_oom(j); }
    return WSA_OK;
}
static wsa_status gjob_exchange(gjob_t *j) {              /* caller holds g_gather_lock */
    wsa_gather_result r;
    const wsa_status st = wsa_gather_rows(g_gather, j->plans, NULL, &r);
    if (st != WSA_OK) return st;
    j->n_rows = r.n_rows;
    j->per = dup_bytes(r.rows_per_rank, sizeof(uint32_t) * j->n);
    j->meta = malloc(sizeof(int32_t) * 8 * (size_t)OR1(r.n_rows)); j->feat = malloc(sizeof(double) * WSA_NFEAT * (size_t)OR1(r.n_rows));
    if (!j->per || !j->meta || !j->feat) return gjob_oom(j);
    return wsa_gather_copy_rows(g_gather, j->meta, j->feat, OR1(r.n_rows));
}
static void gjob_execute(napi_env env, void *data) {
    gjob_t *j = (gjob_t *)data;
    pthread_mutex_lock(&g_gather_lock);
    j->st = gjob_communicator(j);
    if (j->st == WSA_OK) {
        j->st = gjob_exchange(j);
        /* a failed exchange leaves the communicators unusable: the next job builds new ones */
        if (j->st != WSA_OK && !j->err[0]) { snprintf(j->err, sizeof j->err, "%s", wsa_last_error(j->ctxs[0])); gather_drop(); }
    }
    pthread_mutex_unlock(&g_gather_lock);
}
static void gjob_complete(napi_env env, napi_status status, void *data) {
    gjob_t *j = (gjob_t *)data;
    for (uint32_t i = 0; i < j->n; i++) if (j->boxes[i]->children) j->boxes[i]->children--;
    if (j->st != WSA_OK) settle(env, j->deferred, j->err, NULL);
    else if (status != napi_ok) settle(env, j->deferred, "async work cancelled", NULL);
    else {
        napi_value o = new_object(env);
        put_rows(env, o, j->meta, j->feat, j->n_rows);
        put_typed(env, o, "rowsPerRank", napi_uint32_array, j->per, j->n);
        settle(env, j->deferred, NULL, o);
    }
    napi_delete_async_work(env, j->work);
    gjob_release(j);
}
napi_value fn_gather_rows(napi_env env, napi_callback_info info) {
    ARGS(1);
    uint32_t n = 0;
    if (argc < 1 || !array_arg(env, argv[0], &n) || n < 1) return fail_usage(env, "gatherRows(ctx[])");
    gjob_t *j = calloc(1, sizeof *j);
    if (j) { j->n = n; j->boxes = calloc(n, sizeof(ctx_box *)); j->ctxs = calloc(n, sizeof(wsa_ctx *)); j->plans = calloc(n, sizeof(wsa_batch *)); }
    if (!j || !j->boxes || !j->ctxs || !j->plans) { if (j) gjob_release(j); return fail_oom(env); }
    for (uint32_t i = 0; i < n; i++) {
        napi_value el;
        ctx_box *b = napi_get_element(env, argv[0], i, &el) == napi_ok ? get_box(env, el) : NULL;
        if (!b || !b->ctx || !b->plan) {       /* the rows to collect are those of the plan the context's last processBatch left in its box */
            gjob_release(j);
            return fail_error(env, "gatherRows: every context needs a finished processBatch(..., deferRows = true)");
        }
        j->boxes[i] = b; j->ctxs[i] = b->ctx; j->plans[i] = b->plan;
    }
    napi_value promise = queue_work(env, "wsa.gatherRows", gjob_execute, gjob_complete, j, &j->deferred, &j->work);
    if (!promise) return NULL;
    for (uint32_t i = 0; i < n; i++) j->boxes[i]->children++;      /* the contexts (and their plans) stay until gjob_complete */
    return promise;
}
