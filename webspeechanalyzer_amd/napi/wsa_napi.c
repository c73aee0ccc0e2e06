// wsa_napi.c — thin N-API binding of the C ABI (include/wsa.h, include/wsa_eval.h) for the JavaScript host (webspeechanalyzer_amd/js/formantanalyzer.js).
// Raw node_api.h, N-API >= 4 (async work, thread-safe functions).  Rejections carry the library's error string.  No compute happens in the addon.
//
// This file holds the module's registration alone.  Each export is documented above its function; the plumbing they are written in is napi_util.h, the
// boxes behind the handles napi_handles.h.
//
// napi_handles.c — contexts and page-locked buffers
//   abiVersion() -> number
//   defaults() -> config object
//   create(config, device) -> ctx
//   destroy(ctx)
//   geometry(ctx, fs) -> {nfft, win, hop, bands, kmax}
//   binsHz(ctx, fs) -> Float64Array
//   allocPinned(ctx, bytes) -> ArrayBuffer over page-locked host memory
//   freePinned(arrayBuffer) -> boolean
// napi_batch.c — batches, on worker threads
// processBatch(ctx, clips[], fs[, level[, analysisRate[, channels[, deferRows[, model | [models][, formats[, select, source]]]]]]]) -> Promise of the result
//   tables
//   gatherRows(ctx[]) -> Promise of {meta, feat, rowsPerRank}
// napi_plan.c — over the plan the context's last processBatch left
//   batchKnn(ctx, knn, k) -> knnClassify's tables
//   batchKnnFold(ctx) -> {cb, cbLabel, cbConf, clipConf, nClasses}
//   batchRegressGroup(ctx, [models], outMin, outMax) -> {value, cb, cbValue, cbWeight, clipSum, clipWeight, clipValue, nHeads}
//   featdbAppendBatch(ctx, db) -> {first, kept}
// napi_stream.c — live streams
//   streamOpen(ctx, nStreams, fs, framesPerStep, maxSpanFrames) -> stream
//   streamOpenMixed(ctx, nStreams, rates, fsOut, framesPerStep, maxSpanFrames) -> stream
//   streamInfo(stream) -> {capacity, inputStride, samplesPerStep, inputStrideBytes}
//   streamPaced(stream) -> Uint32Array
//   streamInput(stream) -> typed array over the pinned input buffer
//   streamSetInput(stream, format, channels[, select, source])
//   streamStep(stream, ctl[, counts]) -> the step's tables
//   streamClose(stream)
//   streamSetModel(stream, model | null)
//   streamSetEnsemble(stream, [models] | null)
//   streamSetKnn(stream, knn | null, k)
//   streamSetRegress(stream, [models] | null, outMin, outMax)
//   streamSetFeatdb(stream, db | null)
//   streamDbRows(stream) -> {first, added, replaced, notFitted, kept, replacedRows}
//   decodePcm(format, typedArray, channels[, select]) -> Float32Array
// napi_train.c — models and training
//   modelCreate(ctx, spec) -> model
//   modelDestroy(model)
//   train(ctx, spec, run, onEpoch?) -> Promise of {kernels, biases, history}
//   trainGroup(ctx, [[spec, run, onEpoch?], ...]) -> Promise of an array of train's results
//   regressRows(ctx, model, features, outMin, outMax) -> Float64Array
// napi_db.c — stored rows
//   dbPredict(ctx, model, features, ords, outMin, outMax) -> Int32Array | Float64Array
//   dbTable(ctx, tables) -> {cat, cls, ord}
//   dbEval(ctx, tables) -> {rows, predIdx, predVal, files}          (with foldOfRow / nFolds: a head's models may be an array, one per fold)
//   featdbCreate(ctx, width, capacity) -> db
//   featdbDestroy(db)
//   featdbCount(db) -> number
//   featdbCopyRows(db) -> Float64Array
//   featdbRanges(db, rows) -> {min, max}
//   knnCreate(ctx, width, nClasses, capacity) -> knn
//   knnDestroy(knn)
//   knnAdd(knn, features, classes) -> {rows, perClass}
//   knnClassify(knn, features, k) -> {label, conf, nbr, sim, k, kEff, nClasses}
#include <node_api.h>
#include "../../include/wsa.h"

#define EXPORTS(X) \
    X(abiVersion, fn_abi_version) X(freePinned, fn_free_pinned) X(defaults, fn_defaults) X(create, fn_create) X(destroy, fn_destroy) \
    X(geometry, fn_geometry) X(allocPinned, fn_alloc_pinned) X(binsHz, fn_bins_hz) X(processBatch, fn_process_batch) X(gatherRows, fn_gather_rows) \
    X(streamOpen, fn_stream_open) X(streamOpenMixed, fn_stream_open_mixed) X(streamInfo, fn_stream_info) X(streamPaced, fn_stream_paced) \
    X(streamInput, fn_stream_input) X(streamSetInput, fn_stream_set_input) X(decodePcm, fn_decode_pcm) X(streamStep, fn_stream_step) \
    X(streamClose, fn_stream_close) X(streamSetModel, fn_stream_set_model) X(streamSetEnsemble, fn_stream_set_ensemble) X(streamSetKnn, fn_stream_set_knn) \
    X(modelCreate, fn_model_create) X(modelDestroy, fn_model_destroy) X(train, fn_train) X(trainGroup, fn_train_group) X(regressRows, fn_regress_rows) \
    X(dbPredict, fn_db_predict) X(dbTable, fn_db_table) X(dbEval, fn_db_eval) \
    X(knnCreate, fn_knn_create) X(knnDestroy, fn_knn_destroy) X(knnAdd, fn_knn_add) X(knnClassify, fn_knn_classify) X(batchKnn, fn_batch_knn) \
    X(batchKnnFold, fn_batch_knn_fold) X(streamSetRegress, fn_stream_set_regress) X(batchRegressGroup, fn_batch_regress_group) \
    X(featdbCreate, fn_featdb_create) X(featdbDestroy, fn_featdb_destroy) X(featdbCount, fn_featdb_count) X(featdbAppendBatch, fn_featdb_append_batch) \
    X(featdbCopyRows, fn_featdb_copy_rows) X(featdbRanges, fn_featdb_ranges) X(streamSetFeatdb, fn_stream_set_featdb) X(streamDbRows, fn_stream_db_rows)

#define DECLARE(name, fn) napi_value fn(napi_env env, napi_callback_info info);
EXPORTS(DECLARE)

NAPI_MODULE_INIT() {
    /* the structures the addon reads and fills follow the header it was compiled against: refuse a libwsa.so of another ABI version */
    if (wsa_abi_version() != WSA_ABI_VERSION) { napi_throw_error(env, NULL,
        "libwsa.so ABI version differs from the one wsa_napi.node was built against (include/wsa.h): rebuild"); return NULL; }
#define ENTRY(name, fn) {#name, fn},
    const struct { const char *name; napi_callback fn; } fns[] = {EXPORTS(ENTRY)};
    for (size_t i = 0; i < sizeof fns / sizeof fns[0]; i++) {
        napi_value f;
        if (napi_create_function(env, fns[i].name, NAPI_AUTO_LENGTH, fns[i].fn, NULL, &f) != napi_ok) return NULL;
        if (napi_set_named_property(env, exports, fns[i].name, f) != napi_ok) return NULL;
    }
    return exports;
}
