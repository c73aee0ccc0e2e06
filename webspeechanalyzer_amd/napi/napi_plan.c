// napi_plan.c — the synchronous calls over the plan that the context's last processBatch left in its box (ctx_box.plan): batchKnn, batchKnnFold,
// batchRegressGroup, featdbAppendBatch.  They run on the calling thread, on the context's own stream.
#include "napi_handles.h"

/* ---- over the kept plan.  Each refuses, in its own name, a context without one */
static ctx_box *planned_box(napi_env env, ctx_box *box, const char *none) {
    if (!box->plan) { fail_error(env, none); return NULL; }
    return box;
}
// batchKnn(ctx, knn, k) -> knnClassify's tables over the rows of the context's last processBatch (wsa_batch_knn on its kept plan; level 11: the
// utterance rows)
napi_value fn_batch_knn(napi_env env, napi_callback_info info) {
    ARGS(3);
    ctx_box *box = box_arg(env, argc, argv);
    knn_box *kb = argc > 1 ? (knn_box *)external_of(env, argv[1]) : NULL;
    uint32_t k = 0;
    if (!box || !kb || argc < 3 || napi_get_value_uint32(env, argv[2], &k) != napi_ok) return fail_usage(env, "batchKnn(ctx, knn, k)");
    if (!child_is(&kb->link, box)) return fail_error(env, "batchKnn: the KNN store was destroyed or belongs to another context");
    if (!planned_box(env, box, "batchKnn: no finished processBatch on this context (or one is in flight)")) return NULL;
    wsa_knn_result r;
    wsa_status st = wsa_batch_knn(box->plan, knn_of(kb), k, box->queue);
    if (st == WSA_OK) st = wsa_batch_knn_result(box->plan, box->queue, &r);
    if (st != WSA_OK) return fail_lib(env, box->ctx);
    const size_t n = r.n_rows;
    char *buf = malloc(knn_slab_bytes(n, r.k, r.n_classes));
    if (!buf) return fail_oom(env);
    const knn_slab t = knn_slab_at(buf, n, r.k);
    st = wsa_batch_copy_knn(box->plan, box->queue, t.label, t.conf, t.nbr, t.sim, (uint32_t)OR1(n));
    napi_value out = st == WSA_OK ? knn_object(env, &t, n, r.k, r.k_eff, r.n_classes) : fail_lib(env, box->ctx);
    free(buf);
    return out;
}
// batchKnnFold(ctx) -> {cb: Int32Array [n][4], cbLabel: Int32Array [n], cbConf: Float64Array [n], clipConf: Float64Array [clips][nClasses], nClasses}:
// the fold KN-2 over the tables of the context's last batchKnn (wsa_batch_knn_fold; output_level 13)
napi_value fn_batch_knn_fold(napi_env env, napi_callback_info info) {
    ARGS(1);
    ctx_box *box = box_arg(env, argc, argv);
    if (!box) return fail_usage(env, "batchKnnFold(ctx)");
    if (!planned_box(env, box, "batchKnnFold: no finished processBatch on this context (or one is in flight)")) return NULL;
    wsa_knn_fold_result r;
    wsa_status st = wsa_batch_knn_fold(box->plan, box->queue);
    if (st == WSA_OK) st = wsa_batch_knn_fold_result(box->plan, box->queue, &r);
    if (st != WSA_OK) return fail_lib(env, box->ctx);
    const size_t n = r.n_callbacks, nc = (size_t)r.n_clips * r.n_classes;
    double *conf = malloc((n + nc + 1) * sizeof(double));
    int32_t *cb = malloc((5 * n + 1) * sizeof(int32_t));
    napi_value out = NULL;
    if (!conf || !cb) fail_oom(env);
    else if (wsa_batch_copy_knn_fold(box->plan, box->queue, cb, cb + 4 * n, conf, (uint32_t)OR1(n), conf + n) != WSA_OK) fail_lib(env, box->ctx);
    else {
        out = new_object(env);
        put_typed(env, out, "cb", napi_int32_array, cb, n * 4);
        put_typed(env, out, "cbLabel", napi_int32_array, cb + 4 * n, n);
        put_typed(env, out, "cbConf", napi_float64_array, conf, n);
        put_typed(env, out, "clipConf", napi_float64_array, conf + n, nc);
        put_u32(env, out, "nClasses", r.n_classes);
    }
    free(conf); free(cb);
    return out;
}
/* the context's kept regression group, if it was made of these models and ranges, else a new one in its place; NULL with an exception pending */
static wsa_regress_group *group_of_box(napi_env env, ctx_box *box, model_box **mbs, const wsa_model **ms, const double *lo, const double *hi, uint32_t H) {
    bool same = box->reg != NULL && box->reg_n == H;
    for (uint32_t d = 0; same && d < H; d++) same = box->reg_models[d] == mbs[d] && box->reg_lo[d] == lo[d] && box->reg_hi[d] == hi[d];
    if (same) return box->reg;
    wsa_regress_group *g = NULL;
    if (wsa_regress_group_create(box->ctx, ms, lo, hi, H, &g) != WSA_OK) { fail_lib(env, box->ctx); return NULL; }
    box_drop_regress(box);
    box->reg = g; box->reg_n = H; memcpy(box->reg_models, mbs, sizeof box->reg_models);
    for (uint32_t d = 0; d < H; d++) { box->reg_lo[d] = lo[d]; box->reg_hi[d] = hi[d]; }
    return g;
}
// batchRegressGroup(ctx, [models], outMin, outMax) -> {value: Float64Array [H][rows], cb: Int32Array [n][4], cbValue, cbWeight: Float64Array [H][n], clipSum,
// clipWeight,
// clipValue: Float64Array [H][clips], nHeads}: the grouped launch and the fold RG-1 over the rows of the context's last processBatch (wsa_batch_regress_group
// on its
// kept plan; output_level 5: value and nHeads only)
napi_value fn_batch_regress_group(napi_env env, napi_callback_info info) {
    ARGS(4);
    ctx_box *box = box_arg(env, argc, argv);
    if (!box || argc < 4) return fail_usage(env, "batchRegressGroup(ctx, [models], outMin, outMax)");
    if (!planned_box(env, box, "batchRegressGroup: no finished processBatch on this context (or one is in flight)")) return NULL;
    model_box *mbs[WSA_REGRESS_GROUP_MAX] = {0}; const wsa_model *ms[WSA_REGRESS_GROUP_MAX]; const double *lo = NULL, *hi = NULL; uint32_t H = 0;
    if (!regress_group_arg(env, "batchRegressGroup", argv[1], argv[2], argv[3], box, mbs, ms, &lo, &hi, &H)) return NULL;
    if (!group_of_box(env, box, mbs, ms, lo, hi, H)) return NULL;
    wsa_value_result r;
    wsa_status st = wsa_batch_regress_group(box->plan, box->reg, box->queue);
    if (st == WSA_OK) st = wsa_batch_value_result(box->plan, box->queue, &r);
    if (st != WSA_OK) return fail_lib(env, box->ctx);
    const size_t R = r.n_rows, K = r.n_callbacks, N = r.n_clips;
    const int fold = r.d_cb != NULL;
    /* one allocation [value H R][cbValue H K][cbWeight H K][clipSum H N][clipWeight H N][clipValue H N]: table t of head h starts at at[t] + h * len[t] */
    const size_t len[6] = {R, K, K, N, N, N};
    double *buf = malloc(((size_t)H * (R + 2 * K + 3 * N) + 1) * sizeof(double)), *at[6];
    int32_t *cb = malloc((4 * K + 1) * sizeof(int32_t));
    napi_value out = NULL;
    if (!buf || !cb) { free(buf); free(cb); return fail_oom(env); }
    for (int t = 0; t < 6; t++) at[t] = t ? at[t - 1] + (size_t)H * len[t - 1] : buf;
    wsa_value_host dst;
    memset(&dst, 0, sizeof dst);
    dst.rows_cap = (uint32_t)OR1(R); dst.cb_cap = (uint32_t)OR1(K); dst.cb = fold ? cb : NULL;
    for (uint32_t h = 0; h < H; h++) {
        dst.value[h] = at[0] + (size_t)h * R;
        if (!fold) continue;
        dst.cb_value[h] = at[1] + (size_t)h * K; dst.cb_weight[h] = at[2] + (size_t)h * K;
        dst.clip_sum[h] = at[3] + (size_t)h * N; dst.clip_weight[h] = at[4] + (size_t)h * N; dst.clip_value[h] = at[5] + (size_t)h * N;
    }
    if (wsa_batch_copy_value_fold(box->plan, box->queue, &dst) != WSA_OK) fail_lib(env, box->ctx);
    else {
        static const char *names[6] = {"value", "cbValue", "cbWeight", "clipSum", "clipWeight", "clipValue"};
        out = new_object(env);
        put_typed(env, out, names[0], napi_float64_array, at[0], (size_t)H * R);
        if (fold) put_typed(env, out, "cb", napi_int32_array, cb, K * 4);
        for (int t = 1; fold && t < 6; t++) put_typed(env, out, names[t], napi_float64_array, at[t], (size_t)H * len[t]);
        put_u32(env, out, "nHeads", H);
    }
    free(buf); free(cb);
    return out;
}
// featdbAppendBatch(ctx, db) -> {first, kept: Int32Array}: the rows of the context's last processBatch that the app's storing keeps
// (wsa_featdb_append_batch on its kept plan), kept[i] = the source row (level 11: utterance row) of DB row first + i
napi_value fn_featdb_append_batch(napi_env env, napi_callback_info info) {
    ARGS(2);
    ctx_box *box = box_arg(env, argc, argv);
    if (!box || argc < 2) return fail_usage(env, "featdbAppendBatch(ctx, db)");
    fdb_box *fb = fdb_idle(env, argv[1], "featdbAppendBatch(ctx, db)");
    if (!fb) return NULL;
    if (fb->link.owner != box) return fail_error(env, "featdbAppendBatch: the device DB belongs to another context");
    if (!planned_box(env, box, "featdbAppendBatch: no finished processBatch on this context (or one is in flight)")) return NULL;
    wsa_batch_info bi;
    if (wsa_batch_get_info(box->plan, &bi) != WSA_OK) return fail_lib(env, box->ctx);
    const uint32_t cap = OR1(bi.rows_cap > bi.n_clips ? bi.rows_cap : bi.n_clips);
    int32_t *kept = malloc(sizeof(int32_t) * (size_t)cap);
    if (!kept) return fail_oom(env);
    uint32_t first = 0, added = 0;
    napi_value out = NULL;
    if (wsa_featdb_append_batch(fdb_of(fb), box->plan, box->queue, &first, &added, kept, cap) != WSA_OK) fail_lib(env, box->ctx);
    else if ((out = new_object(env)) != NULL) {
        put_u32(env, out, "first", first);
        put_typed(env, out, "kept", napi_int32_array, kept, added);
    }
    free(kept);
    return out;
}
