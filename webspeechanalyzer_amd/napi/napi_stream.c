// napi_stream.c — live streams: the 14 exports named stream*, and decodePcm.  A step is one hipGraph launch, well under a millisecond, so everything here
// runs on the calling thread.
#include "napi_handles.h"

// What JS holds for a stream set (wsa_stream).  input_ref: the ArrayBuffer over the pinned input, detached at close; model, ens_models, reg_models: what is
// attached (each holds its models' busy counts; the stream object owns the ensemble and the regress group it makes of them); knn, and the feature DB the
// library holds, stay the caller's
typedef struct {
    wsa_stream *st; wsa_ctx *ctx; ctx_box *box; uint32_t n, sps; int32_t fmt; napi_ref input_ref;
    model_box *model;
    wsa_ensemble *ens; model_box *ens_models[WSA_ENSEMBLE_MAX]; uint32_t n_ens;
    knn_box *knn;
    wsa_regress_group *reg; model_box *reg_models[WSA_REGRESS_GROUP_MAX]; uint32_t n_reg;
} stream_t;
static void stream_finalize(napi_env env, void *data, void *hint) { /* explicit streamClose() only */ }
/* argv[0] as an open stream set, else NULL (nothing thrown) */
static stream_t *stream_arg(napi_env env, size_t argc, const napi_value *argv) {
    stream_t *h = argc ? (stream_t *)external_of(env, argv[0]) : NULL;
    return h && h->st ? h : NULL;
}
static void stream_drop_model(stream_t *h) {
    if (h->model && h->model->busy) h->model->busy--;
    h->model = NULL;
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
/* the JS handle of a stream set the library made (st == WSA_OK) on the context of `box`; one child of the context until streamClose */
static napi_value stream_opened(napi_env env, stream_t *h, wsa_status st, ctx_box *box) {
    if (st != WSA_OK) { free(h); return fail_lib(env, box->ctx); }
    h->box->children++;
    wsa_stream_enable_graph(h->st, 1);
    h->sps = wsa_stream_input_stride(h->st);                     /* (a plain set: samples_per_step) */
    napi_value ext; NAPI_OK(env, napi_create_external(env, h, stream_finalize, NULL, &ext));
    return ext;
}
static stream_t *stream_new(ctx_box *box, uint32_t n) {
    stream_t *h = calloc(1, sizeof *h);
    h->ctx = box->ctx; h->n = n; h->box = box;
    return h;
}
/* streamOpen(ctx, nStreams, fs, framesPerStep, maxSpanFrames) -> external stream (wsa_stream_create) */
napi_value fn_stream_open(napi_env env, napi_callback_info info) {
    ARGS(5); double fs = 0; uint32_t n = 0, fps = 1, span = 1024;
    ctx_box *box = box_arg(env, argc, argv);
    if (!box || argc < 3 || napi_get_value_uint32(env, argv[1], &n) != napi_ok || napi_get_value_double(env, argv[2], &fs) != napi_ok)
        return fail_usage(env, "streamOpen(ctx, nStreams, fs, framesPerStep, maxSpanFrames)");
    if (argc > 3) napi_get_value_uint32(env, argv[3], &fps);
    if (argc > 4) napi_get_value_uint32(env, argv[4], &span);
    stream_t *h = stream_new(box, n);
    return stream_opened(env, h, wsa_stream_create(box->ctx, n, fs, fps, span, &h->st), box);
}
// streamOpenMixed(ctx, nStreams, rates: Float64Array, fsOut, framesPerStep, maxSpanFrames) -> external stream (wsa_stream_create_mixed: stream i arrives at
// rates[i] and is converted to fsOut inside the step)
napi_value fn_stream_open_mixed(napi_env env, napi_callback_info info) {
    ARGS(6); double fs_out = 0; uint32_t n = 0, fps = 1, span = 1024; void *rates = NULL;
    ctx_box *box = box_arg(env, argc, argv);
    if (!box || argc < 4 || napi_get_value_uint32(env, argv[1], &n) != napi_ok || !typed_arg_n(env, argv[2], napi_float64_array, n, &rates)
        || napi_get_value_double(env, argv[3], &fs_out) != napi_ok)
        return fail_usage(env, "streamOpenMixed(ctx, nStreams, rates: Float64Array(nStreams), fsOut, framesPerStep, maxSpanFrames)");
    if (argc > 4) napi_get_value_uint32(env, argv[4], &fps);
    if (argc > 5) napi_get_value_uint32(env, argv[5], &span);
    stream_t *h = stream_new(box, n);
    return stream_opened(env, h, wsa_stream_create_mixed(box->ctx, n, (const double *)rates, fs_out, fps, span, &h->st), box);
}
// streamInfo(stream) -> {capacity: Uint32Array, inputStride, samplesPerStep, inputStrideBytes} (wsa_stream_input_capacity / _input_stride / _samples_per_step /
// _input_stride_bytes)
napi_value fn_stream_info(napi_env env, napi_callback_info info) {
    ARGS(1);
    stream_t *h = stream_arg(env, argc, argv);
    if (!h) return fail_usage(env, "streamInfo(stream)");
    uint32_t *cap = malloc(sizeof(uint32_t) * OR1(h->n));
    for (uint32_t i = 0; i < h->n; i++) cap[i] = wsa_stream_input_capacity(h->st, i);
    napi_value o = new_object(env);
    put_typed(env, o, "capacity", napi_uint32_array, cap, h->n);
    free(cap);
    put_u32(env, o, "inputStride", wsa_stream_input_stride(h->st));
    put_u32(env, o, "samplesPerStep", wsa_stream_samples_per_step(h->st));
    put_u32(env, o, "inputStrideBytes", wsa_stream_input_stride_bytes(h->st));
    return o;
}
// streamSetInput(stream, format 0 .. 3, channels: Uint32Array(nStreams) | null[, select, source: Uint32Array(nStreams) | null]) before the first streamInput:
// wsa_stream_set_input_format; streamInput then gives an Int16Array / Uint8Array over the packed pinned buffer, [nStreams][streamInfo().inputStrideBytes /
// element size].  With a select or a source: wsa_stream_set_input_channels (spec PK-3: stream i takes channel select[i], 0xFFFFFFFF the mix, of the packed
// row of stream source[i])
napi_value fn_stream_set_input(napi_env env, napi_callback_info info) {
    ARGS(5); int32_t fmt = 0;
    stream_t *h = stream_arg(env, argc, argv);
    if (!h || argc < 2 || napi_get_value_int32(env, argv[1], &fmt) != napi_ok) return fail_usage(env, "streamSetInput(stream, format, channels)");
    if (h->input_ref) return fail_error(env, "streamSetInput: the input buffer of this stream object has been handed out already");
    void *chan = NULL, *ss[2] = {NULL, NULL};
    if (argc > 2 && typed_opt(env, argv[2], napi_uint32_array, h->n, &chan) < 0)
        return fail_usage(env, "channels must be a Uint32Array with one count per stream");
    for (size_t a = 3; a < argc && a < 5; a++)
        if (typed_opt(env, argv[a], napi_uint32_array, h->n, &ss[a - 3]) < 0)
            return fail_usage(env, "select and source must be Uint32Arrays with one word per stream");
    const wsa_status sst = (ss[0] || ss[1]) ? wsa_stream_set_input_channels(h->st, fmt, chan, ss[0], ss[1]) : wsa_stream_set_input_format(h->st, fmt, chan);
    if (sst != WSA_OK) return fail_lib(env, h->ctx);
    h->fmt = fmt;
    return NULL;
}
// decodePcm(format, typedArray, channels[, select]) -> Float32Array: wsa_pcm_decode_select, channel `select` (0; 0xFFFFFFFF: the mix) of the interleaved frames
// (specs PK-1 / PK-3, no device)
napi_value fn_decode_pcm(napi_env env, napi_callback_info info) {
    ARGS(4); int32_t fmt = 0; uint32_t ch = 1, sel = 0;
    napi_typedarray_type tt = napi_int8_array; size_t len = 0; void *data = NULL;
    if (argc < 2 || napi_get_value_int32(env, argv[0], &fmt) != napi_ok || !typed_info(env, argv[1], &tt, &data, &len))
        return fail_usage(env, "decodePcm(format, typedArray, channels)");
    if (argc > 2) napi_get_value_uint32(env, argv[2], &ch);
    const napi_typedarray_type want = fmt == WSA_PCM_F32 ? napi_float32_array : fmt == WSA_PCM_I16 ? napi_int16_array : napi_uint8_array;
    if (fmt < WSA_PCM_F32 || fmt > WSA_PCM_ALAW) return fail_error(env, "decodePcm: unknown input format");
    if (tt != want) return fail_usage(env, "decodePcm: f32 takes a Float32Array, i16 an Int16Array, mulaw / alaw a Uint8Array");
    if (ch < 1 || ch > 64) return fail_error(env, "decodePcm: channel count outside 1 .. 64");
    if (argc > 3) napi_get_value_uint32(env, argv[3], &sel);
    if (sel >= ch && sel != WSA_CHANNEL_MIX) return fail_error(env, "decodePcm: select is neither a channel below the channel count nor the mix");
    const size_t last = sel == WSA_CHANNEL_MIX ? ch - 1u : sel;           /* the last channel of a frame that is read */
    const size_t frames = len > last ? (len - 1 - last) / ch + 1 : 0;
    napi_value ab, ta; void *out = NULL;
    NAPI_OK(env, napi_create_arraybuffer(env, frames * sizeof(float), &out, &ab));
    if (wsa_pcm_decode_select(fmt, data, frames, ch, sel, (float *)out) != WSA_OK) return fail_error(env, "decodePcm: refused");
    NAPI_OK(env, napi_create_typedarray(env, napi_float32_array, frames, ab, 0, &ta));
    return ta;
}
/* streamPaced(stream) -> Uint32Array: the samples a paced step takes from every stream next (wsa_stream_paced_input) */
napi_value fn_stream_paced(napi_env env, napi_callback_info info) {
    ARGS(1);
    stream_t *h = stream_arg(env, argc, argv);
    if (!h) return fail_usage(env, "streamPaced(stream)");
    uint32_t *cnt = malloc(sizeof(uint32_t) * OR1(h->n));
    for (uint32_t i = 0; i < h->n; i++) cnt[i] = wsa_stream_paced_input(h->st, i);
    napi_value ta = make_typed(env, napi_uint32_array, cnt, h->n);
    free(cnt);
    return ta;
}
// streamInput(stream) -> Float32Array over the pinned [nStreams][inputStride] input buffer (no copy; inputStride = samplesPerStep on a plain set); after
// streamSetInput the Int16Array / Uint8Array over the pinned packed buffer, [nStreams][inputStrideBytes / element size]
napi_value fn_stream_input(napi_env env, napi_callback_info info) {
    ARGS(1);
    stream_t *h = stream_arg(env, argc, argv);
    if (!h) return fail_usage(env, "streamInput(stream)");
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

/* -- a step's tables of what is attached: each returns 1, or 0 with the library's error pending */
static int step_classes(napi_env env, napi_value o, stream_t *h) {        /* named as processBatch's (streamConf: per stream, carried) */
    wsa_stream_class_result c;
    if (wsa_stream_classes(h->st, &c) != WSA_OK) { fail_lib(env, h->ctx); return 0; }
    const class_view v = {c.n_classes, c.n_rows, c.n_callbacks, c.n_streams, c.cb != NULL, "streamConf", c.prob, c.cb, c.cb_label, c.cb_conf, c.stream_conf};
    put_classes(env, o, &v);
    put_u32(env, o, "nClasses", c.n_classes);
    return 1;
}
static int step_knn(napi_env env, napi_value o, stream_t *h) {            /* K9s; level 13: the fold KN-2, knnStreamConf per stream, carried */
    wsa_stream_knn_result c;
    if (wsa_stream_knn_classes(h->st, &c) != WSA_OK) { fail_lib(env, h->ctx); return 0; }
    put_typed(env, o, "knnLabel", napi_int32_array, c.label, c.n_rows);
    put_typed(env, o, "knnConf", napi_float64_array, c.conf, (size_t)c.n_rows * c.n_classes);
    if (c.cb) {
        put_typed(env, o, "knnCb", napi_int32_array, c.cb, (size_t)c.n_callbacks * 4);
        put_typed(env, o, "knnCbLabel", napi_int32_array, c.cb_label, c.n_callbacks);
        put_typed(env, o, "knnCbConf", napi_float64_array, c.cb_conf, c.n_callbacks);
        put_typed(env, o, "knnStreamConf", napi_float64_array, c.stream_conf, (size_t)c.n_streams * c.n_classes);
    }
    put_u32(env, o, "knnNClasses", c.n_classes);
    return 1;
}
static int step_ensemble(napi_env env, napi_value o, stream_t *h) {       /* conf / minDb: per stream, carried */
    wsa_stream_ensemble_result c;
    if (wsa_stream_ensemble_classes(h->st, &c) != WSA_OK) { fail_lib(env, h->ctx); return 0; }
    const ens_view v = {c.n_members, c.n_rows, c.n_callbacks, c.n_streams, c.n_classes, c.cb != NULL, c.prob, c.cb_label, c.cb_conf, c.cb_all_max,
        c.stream_conf,
                        c.cb, c.cb_db, c.cb_top_label, c.cb_min_db, c.stream_min_db, c.cb_top_conf, c.cb_entropy};
    put(env, o, "ens", ens_object(env, &v));
    return 1;
}
static int step_values(napi_env env, napi_value o, stream_t *h) {         /* level 13: the fold RG-1; regSum / regWeight / regRunValue per stream, carried */
    wsa_stream_value_result c;
    if (wsa_stream_values(h->st, &c) != WSA_OK) { fail_lib(env, h->ctx); return 0; }
    put_heads(env, o, "regValue", c.value, c.n_heads, c.n_rows);
    if (c.cb) {
        put_typed(env, o, "regCb", napi_int32_array, c.cb, (size_t)c.n_callbacks * 4);
        put_heads(env, o, "regCbValue", c.cb_value, c.n_heads, c.n_callbacks);
        put_heads(env, o, "regCbWeight", c.cb_weight, c.n_heads, c.n_callbacks);
        put_heads(env, o, "regSum", c.stream_sum, c.n_heads, c.n_streams);
        put_heads(env, o, "regWeight", c.stream_weight, c.n_heads, c.n_streams);
        put_heads(env, o, "regRunValue", c.stream_value, c.n_heads, c.n_streams);
    }
    put_u32(env, o, "regNHeads", c.n_heads);
    return 1;
}
// streamStep(stream, ctl: Uint8Array | null[, counts: Uint32Array | null]) -> {meta, feat, segments, cuts, flags[, uttMeta, uttFeat][, formantOff, formants]
//   [, trackOff, trackPoints, trackRanked]} (wsa_stream_step_host[_n] + wsa_stream_collect; counts: samples per stream in this step, else paced), and per
// attachment: a model (streamSetModel): prob, cb, cbLabel, cbConf, streamConf, nClasses; a KNN store (streamSetKnn): knnLabel, knnConf, knnCb, knnCbLabel,
// knnCbConf, knnStreamConf, knnNClasses; an ensemble (streamSetEnsemble): ens; a regress group (streamSetRegress): regValue [H][rows], regCb, regCbValue /
// regCbWeight [H][callbacks], regSum / regWeight / regRunValue [H][streams], regNHeads.  flags: WSA_FLAG_* (8: a span was cut in this step)
napi_value fn_stream_step(napi_env env, napi_callback_info info) {
    ARGS(3);
    stream_t *h = stream_arg(env, argc, argv);
    if (!h) return fail_usage(env, "streamStep(stream, ctl[, counts])");
    void *ctl = NULL, *counts = NULL;
    if (argc > 2 && typed_opt(env, argv[2], napi_uint32_array, h->n, &counts) < 0)
        return fail_usage(env, "counts must be a Uint32Array with one count per stream");
    if (argc > 1 && typed_opt(env, argv[1], napi_uint8_array, h->n, &ctl) < 0) return fail_usage(env, "ctl must be a Uint8Array with one byte per stream");
    wsa_stream_rows r;
    if ((counts ? wsa_stream_step_host_n(h->st, counts, ctl, NULL) : wsa_stream_step_host(h->st, ctl, NULL)) != WSA_OK || wsa_stream_collect(h->st, NULL,
        &r) != WSA_OK)
        return fail_lib(env, h->ctx);
    napi_value o = new_object(env);
    put_rows(env, o, r.row_meta, r.row_feat, r.n_rows);
    put_typed(env, o, "segments", napi_int32_array, r.segments, (size_t)r.n_segments * 4);
    put_typed(env, o, "cuts", napi_uint32_array, r.stream_cuts, h->n);
    if (r.utt_feat) put_utterance(env, o, r.utt_meta, r.utt_feat, r.n_utterance_rows);          /* level 11: one 264-vector per result of the step */
    if (r.formants && r.row_formant_off) {          /* levels 4 / 10: the straightened frames of the rows */
        put_typed(env, o, "formantOff", napi_uint32_array, r.row_formant_off, (size_t)r.n_rows + 1);
        put_typed(env, o, "formants", napi_float32_array, r.formants, (size_t)r.row_formant_off[r.n_rows] * 9);
    }
    /* level 3: ranked raw tracks of the step's segments, as processBatch's */
    if (r.track_off) put_tracks(env, o, r.track_off, r.n_segments, r.track_points, (size_t)r.n_track_points, r.track_ranked, (size_t)r.n_track_ranked);
    put_u32(env, o, "flags", r.status_flags);
    if ((h->model && !step_classes(env, o, h)) || (h->knn && !step_knn(env, o, h)) || (h->ens && !step_ensemble(env, o, h)) || (h->reg && !step_values(env,
        o, h))) return NULL;
    return o;
}
/* streamClose(stream): the pinned input is detached, the models' busy counts and the stream object's own ensemble and regress group go */
napi_value fn_stream_close(napi_env env, napi_callback_info info) {
    ARGS(1);
    stream_t *h = stream_arg(env, argc, argv);
    if (!h) return NULL;
    if (h->input_ref) {                  /* the pinned buffer goes away with the stream object: views on it must not outlive it */
        napi_value ab;
        if (napi_get_reference_value(env, h->input_ref, &ab) == napi_ok && ab) napi_detach_arraybuffer(env, ab);
        napi_delete_reference(env, h->input_ref); h->input_ref = NULL;
    }
    wsa_stream_destroy(h->st); h->st = NULL;
    h->knn = NULL;
    stream_drop_regress(h);
    stream_drop_model(h);
    stream_drop_ensemble(h);
    if (h->box && h->box->children) h->box->children--;
    return NULL;
}
/* streamSetModel(stream, model | null): wsa_stream_set_model; modelDestroy() refuses while a stream holds the model */
napi_value fn_stream_set_model(napi_env env, napi_callback_info info) {
    ARGS(2);
    stream_t *h = stream_arg(env, argc, argv);
    if (!h || argc < 2) return fail_usage(env, "streamSetModel(stream, model | null)");
    model_box *mb = NULL;
    if (!is_nullish(env, argv[1]) &&
        !(mb = model_arg(env, argv[1], h->box, "streamSetModel: the model handle was destroyed (or is not a model)",
            "streamSetModel: the model belongs to another context"))) return NULL;
    if (wsa_stream_set_model(h->st, mb ? model_of(mb) : NULL) != WSA_OK) return fail_lib(env, h->ctx);
    stream_drop_model(h);
    h->model = mb;
    if (mb) { mb->busy++; stream_drop_ensemble(h); }            /* (the library detached the ensemble) */
    return NULL;
}
// streamSetKnn(stream, knn | null, k): wsa_stream_set_knn, beside a model or an ensemble, not in place of one; the store stays the caller's; knnDestroy()
// refuses while its context has open streams
napi_value fn_stream_set_knn(napi_env env, napi_callback_info info) {
    ARGS(3);
    stream_t *h = stream_arg(env, argc, argv);
    if (!h || argc < 2) return fail_usage(env, "streamSetKnn(stream, knn | null, k)");
    knn_box *kb = NULL;
    uint32_t k = 0;
    if (!is_nullish(env, argv[1])) {
        if (!(kb = knn_arg(env, argv[1], h->box, "streamSetKnn: the KNN store was destroyed (or is not a store)",
            "streamSetKnn: the KNN store belongs to another context"))) return NULL;
        if (argc < 3 || napi_get_value_uint32(env, argv[2], &k) != napi_ok) return fail_usage(env, "streamSetKnn(stream, knn | null, k)");
    }
    if (wsa_stream_set_knn(h->st, kb ? knn_of(kb) : NULL, k) != WSA_OK) return fail_lib(env, h->ctx);
    h->knn = kb;
    return NULL;
}
// streamSetEnsemble(stream, [models] | null): wsa_stream_set_ensemble; the stream object owns the wsa_ensemble it makes of them, until it is replaced,
// detached or closed
napi_value fn_stream_set_ensemble(napi_env env, napi_callback_info info) {
    ARGS(2);
    stream_t *h = stream_arg(env, argc, argv);
    if (!h || argc < 2) return fail_usage(env, "streamSetEnsemble(stream, [models] | null)");
    model_box *mbs[WSA_ENSEMBLE_MAX] = {0}; const wsa_model *ms[WSA_ENSEMBLE_MAX]; uint32_t n = 0;
    if (!is_nullish(env, argv[1]) &&
        !(n = model_list_arg(env, argv[1], h->box, WSA_ENSEMBLE_MAX, mbs, ms, "streamSetEnsemble: an ensemble has 1 .. 8 models",
                             "streamSetEnsemble: a model handle was destroyed (or is not a model)",
                                 "streamSetEnsemble: a model belongs to another context"))) return NULL;
    wsa_ensemble *e = NULL;
    if (n && wsa_ensemble_create(h->ctx, ms, n, &e) != WSA_OK) return fail_lib(env, h->ctx);
    if (wsa_stream_set_ensemble(h->st, e) != WSA_OK) { if (e) wsa_ensemble_destroy(e); return fail_lib(env, h->ctx); }
    stream_drop_ensemble(h);
    if (e) {
        h->ens = e; h->n_ens = n; memcpy(h->ens_models, mbs, sizeof h->ens_models);
        for (uint32_t d = 0; d < n; d++) mbs[d]->busy++;
        stream_drop_model(h);                                   /* (the library detached the model) */
    }
    return NULL;
}
// streamSetRegress(stream, [models] | null, outMin: Float64Array, outMax: Float64Array): wsa_stream_set_regress; the stream object owns the wsa_regress_group
// it makes of them, until it is replaced, detached or closed
napi_value fn_stream_set_regress(napi_env env, napi_callback_info info) {
    ARGS(4);
    stream_t *h = stream_arg(env, argc, argv);
    if (!h || argc < 2) return fail_usage(env, "streamSetRegress(stream, [models] | null, outMin, outMax)");
    model_box *mbs[WSA_REGRESS_GROUP_MAX] = {0}; const wsa_model *ms[WSA_REGRESS_GROUP_MAX]; const double *lo = NULL, *hi = NULL; uint32_t n = 0;
    if (!is_nullish(env, argv[1])) {
        if (argc < 4) return fail_usage(env, "streamSetRegress(stream, [models] | null, outMin, outMax)");
        if (!regress_group_arg(env, "streamSetRegress", argv[1], argv[2], argv[3], h->box, mbs, ms, &lo, &hi, &n)) return NULL;
    }
    wsa_regress_group *g = NULL;
    if (n && wsa_regress_group_create(h->ctx, ms, lo, hi, n, &g) != WSA_OK) return fail_lib(env, h->ctx);
    if (wsa_stream_set_regress(h->st, g) != WSA_OK) { if (g) wsa_regress_group_destroy(g); return fail_lib(env, h->ctx); }
    stream_drop_regress(h);
    if (g) {
        h->reg = g; h->n_reg = n; memcpy(h->reg_models, mbs, sizeof h->reg_models);
        for (uint32_t d = 0; d < n; d++) mbs[d]->busy++;            /* modelDestroy() refuses while a stream holds the model */
    }
    return NULL;
}
// streamSetFeatdb(stream, db | null): wsa_stream_set_featdb, specification FD-2: every streamStep of the stream object appends its rows to the DB on the device
// (flags gain WSA_FLAG_DB_FULL); the DB must be of the stream's context and outlive the stream object (featdbDestroy refuses while the context has open
// streams)
napi_value fn_stream_set_featdb(napi_env env, napi_callback_info info) {
    ARGS(2);
    stream_t *h = stream_arg(env, argc, argv);
    if (!h || argc < 2) return fail_usage(env, "streamSetFeatdb(stream, db | null)");
    fdb_box *fb = NULL;
    if (!is_nullish(env, argv[1]) &&
        !(fb = fdb_arg(env, argv[1], h->box, "streamSetFeatdb: the device DB was destroyed (or is not a device DB)",
            "streamSetFeatdb: the device DB belongs to another context"))) return NULL;
    if (wsa_stream_set_featdb(h->st, fb ? fdb_of(fb) : NULL) != WSA_OK) return fail_lib(env, h->ctx);
    return NULL;
}
// streamDbRows(stream) -> {first, added, replaced, notFitted, kept: Int32Array, replacedRows: Int32Array [replaced][2]}
// (wsa_stream_db_rows of the last streamStep)
napi_value fn_stream_db_rows(napi_env env, napi_callback_info info) {
    ARGS(1);
    stream_t *h = stream_arg(env, argc, argv);
    if (!h) return fail_usage(env, "streamDbRows(stream)");
    wsa_stream_db_result r;
    if (wsa_stream_db_rows(h->st, &r) != WSA_OK) return fail_lib(env, h->ctx);
    napi_value out = NULL;
    NAPI_OK(env, napi_create_object(env, &out));
    put_u32(env, out, "first", r.first_row); put_u32(env, out, "added", r.n_added); put_u32(env, out, "replaced", r.n_replaced); put_u32(env, out,
        "notFitted", r.not_fitted);
    put_typed(env, out, "kept", napi_int32_array, r.kept, r.n_added);
    put_typed(env, out, "replacedRows", napi_int32_array, r.replaced, r.replaced ? 2 * (size_t)r.n_replaced : 0);
    return out;
}
