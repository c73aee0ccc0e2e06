// napi_db.c — stored rows: predicting and evaluating a labelled feature DB (dbPredict, dbTable, dbEval), the feature DB that stays on the device (featdb*)
// and the app's ml5 KNN classifier (knn*).  Every call is synchronous, on the context's own stream.
#include "napi_handles.h"
#include "../../include/wsa_eval.h"
#include "../../include/wsa_crossval.h"

// ---- predicting a labelled feature DB and the app's results table (wsa_dbstats_*, K8, specification DS-1): what the app's Predict button does over
// the stored rows (ref src/neuralmodel.js:410-535 predict_db_nn, src/localstore.js:498-627 shows_stats_table).  The calls build the device object for
// the call; js/dbstats.js resolves everything that is a string and hands over indices and values.

// what dbTable and dbEval both take: durations: Float64Array [n], vocab: Uint32Array [nCat], trueIdx, predIdx: Int32Array [nCat][n], trueVal, predVal:
// Float64Array [nOrd][n]
typedef struct { double *dur, *tv, *pv; uint32_t *vocab; int32_t *ti, *pi; size_t n, n_cat, n_ord; } table_args;
static int table_read(napi_env env, napi_value o, table_args *a) {
    size_t nti = 0, npi = 0, ntv = 0, npv = 0;
    if (!typed_of(env, o, "durations", napi_float64_array, (void **)&a->dur, &a->n) || !typed_of(env, o, "vocab", napi_uint32_array, (void **)&a->vocab,
        &a->n_cat) ||
        !typed_of(env, o, "trueIdx", napi_int32_array, (void **)&a->ti, &nti) || !typed_of(env, o, "predIdx", napi_int32_array, (void **)&a->pi, &npi) ||
        !typed_of(env, o, "trueVal", napi_float64_array, (void **)&a->tv, &ntv) || !typed_of(env, o, "predVal", napi_float64_array, (void **)&a->pv, &npv) ||
        a->n < 1 || a->n > 0xffffffffu || nti != a->n_cat * a->n || npi != nti || ntv % a->n || npv != ntv) return 0;
    a->n_ord = ntv / a->n;
    return 1;
}
/* the labels and predictions of every head into the device object */
static wsa_status table_set(wsa_dbstats *db, const table_args *a) {
    wsa_status st = WSA_OK;
    for (size_t h = 0; st == WSA_OK && h < a->n_cat; h++) st = wsa_dbstats_set_classes(db, (uint32_t)h, a->ti + h * a->n, a->pi + h * a->n);
    for (size_t o = 0; st == WSA_OK && o < a->n_ord; o++) st = wsa_dbstats_set_values(db, (uint32_t)o, a->tv + o * a->n, a->pv + o * a->n);
    return st;
}
// one level's tables, as the library fills them and as doubles in one allocation: cat [nCat][3] correct, wrong, blank; cls [items][5] count, correct, wrong,
// duration, first_row (4294967295 = none); ord [nOrd][5] true_n, pred_n, min, max, sq_sum; and for dbEval conf [cells] and agree [nOrd][8] n, mean_true,
// mean_pred, var_true, var_pred, cov, ccc, pearson
typedef struct {
    size_t n_cat, items, n_ord, cells;
    wsa_dbstats_cat *cat; wsa_dbstats_class *cls; wsa_dbstats_ord *od; wsa_dbstats_agree *ag; uint64_t *m;
    double *flat, *fc, *fk, *fo, *fm, *fa;
} level_tables;
static int level_alloc(level_tables *t, size_t n_cat, const uint32_t *vocab, size_t n_ord, int eval) {          /* eval: with conf and agree */
    memset(t, 0, sizeof *t);
    t->n_cat = n_cat; t->n_ord = n_ord;
    for (size_t h = 0; h < n_cat; h++) { t->items += vocab[h]; if (eval) t->cells += (size_t)vocab[h] * (vocab[h] + 1); }
    t->cat = calloc(OR1(n_cat), sizeof *t->cat); t->cls = calloc(OR1(t->items), sizeof *t->cls);
    t->od = calloc(OR1(n_ord), sizeof *t->od); t->ag = calloc(eval ? OR1(n_ord) : 1, sizeof *t->ag);
    t->m = calloc(OR1(t->cells), sizeof *t->m);
    t->flat = calloc(n_cat * 3 + t->items * 5 + n_ord * 5 + t->cells + (eval ? n_ord * 8 : 0) + 1, sizeof(double));
    if (!(t->cat && t->cls && t->od && t->ag && t->m && t->flat)) return 0;
    t->fc = t->flat; t->fk = t->fc + n_cat * 3; t->fo = t->fk + t->items * 5; t->fm = t->fo + n_ord * 5; t->fa = t->fm + t->cells;
    return 1;
}
static void level_free(level_tables *t) { free(t->cat); free(t->cls); free(t->od); free(t->ag); free(t->m); free(t->flat); }
static void level_flatten(level_tables *t, int eval) {
    for (size_t h = 0; h < t->n_cat; h++) { t->fc[h * 3] = (double)t->cat[h].correct; t->fc[h * 3 + 1] = (double)t->cat[h].wrong;
        t->fc[h * 3 + 2] = (double)t->cat[h].blank; }
    for (size_t i = 0; i < t->items; i++) {
        double *k = t->fk + i * 5; const wsa_dbstats_class *c = &t->cls[i];
        k[0] = (double)c->count; k[1] = (double)c->correct; k[2] = (double)c->wrong; k[3] = c->duration; k[4] = (double)c->first_row;
    }
    for (size_t o = 0; o < t->n_ord; o++) {
        double *d = t->fo + o * 5; const wsa_dbstats_ord *r = &t->od[o];
        d[0] = (double)r->true_n; d[1] = (double)r->pred_n; d[2] = r->min; d[3] = r->max; d[4] = r->sq_sum;
        if (!eval) continue;
        double *a = t->fa + o * 8; const wsa_dbstats_agree *g = &t->ag[o];
        a[0] = (double)g->n; a[1] = g->mean_true; a[2] = g->mean_pred; a[3] = g->var_true; a[4] = g->var_pred; a[5] = g->cov; a[6] = g->ccc; a[7] = g->pearson;
    }
    for (size_t i = 0; i < t->cells; i++) t->fm[i] = (double)t->m[i];
}
/* {cat, cls, ord} of the flattened tables; NULL when the object cannot be made */
static napi_value level_object(napi_env env, const level_tables *t) {
    napi_value res = NULL;
    if (napi_create_object(env, &res) != napi_ok || !put_typed(env, res, "cat", napi_float64_array, t->fc, t->n_cat * 3) ||
        !put_typed(env, res, "cls", napi_float64_array, t->fk, t->items * 5) || !put_typed(env, res, "ord", napi_float64_array, t->fo, t->n_ord * 5))
            return NULL;
    return res;
}

// dbPredict(ctx, model, features: Float64Array [n][the model's inputs], ords: boolean, outMin, outMax) -> Int32Array [n] legend indices (-1 = the reference's
// null) for a classifier, Float64Array [n] values for a regression model
napi_value fn_db_predict(napi_env env, napi_callback_info info) {
    ARGS(6);
    ctx_box *box = box_arg(env, argc, argv);
    const char *usage = "dbPredict(ctx, model, features: Float64Array [n][the model's inputs], ords: boolean, outMin, outMax)";
    size_t nf = 0; void *feat = NULL; bool ords = false; double lo = 0, hi = 1; model_box *mb = NULL;
    if (!box || argc < 4 || !(mb = (model_box *)external_of(env, argv[1])) || !typed_arg(env, argv[2], napi_float64_array, &feat, &nf) ||
        napi_get_value_bool(env, argv[3], &ords) != napi_ok ||
        (ords && (argc < 6 || napi_get_value_double(env, argv[4], &lo) != napi_ok || napi_get_value_double(env, argv[5], &hi) != napi_ok)))
            return fail_usage(env, usage);
    if (!child_is(&mb->link, box)) return fail_error(env, "dbPredict: the model was destroyed or belongs to another context");
    if (nf % mb->n_inputs || nf / mb->n_inputs > 0xffffffffu) return fail_usage(env, usage);
    const uint32_t n = (uint32_t)(nf / mb->n_inputs), vocab = mb->n_classes;
    double *dur = calloc(OR1(n), sizeof(double));
    void *out = malloc(OR1(n) * sizeof(double));
    int32_t map[WSA_MODEL_MAX_CLASSES];
    for (int c = 0; c < WSA_MODEL_MAX_CLASSES; c++) map[c] = c;
    wsa_dbstats *db = NULL;
    wsa_status st = dur && out ? wsa_wide_dbstats_create(box->ctx, (const double *)feat, mb->n_inputs, dur, n, ords ? 0 : 1, &vocab, ords ? 1 : 0, &db)
        : WSA_ERR_INVALID;
    if (st == WSA_OK) st = ords ? wsa_dbstats_predict_values(db, 0, model_of(mb), lo, hi, box->queue) : wsa_dbstats_predict_classes(db, 0, model_of(mb), map,
        box->queue);
    if (st == WSA_OK) st = ords ? wsa_dbstats_copy_values(db, 0, box->queue, (double *)out) : wsa_dbstats_copy_classes(db, 0, box->queue, (int32_t *)out);
    napi_value res = NULL;
    if (st == WSA_OK) res = make_typed(env, ords ? napi_float64_array : napi_int32_array, out, n);
    else if (dur && out) fail_lib(env, box->ctx);
    else fail_oom(env);
    if (db) wsa_dbstats_destroy(db);
    free(dur); free(out);
    return res;
}
// dbTable(ctx, {durations, vocab, trueIdx, predIdx, trueVal, predVal})
//   -> {cat: Float64Array [nCat][3], cls: Float64Array [sum vocab][5], ord: Float64Array [nOrd][5]}
napi_value fn_db_table(napi_env env, napi_callback_info info) {
    ARGS(2);
    ctx_box *box = box_arg(env, argc, argv);
    const char *usage = "dbTable(ctx, {durations: Float64Array [n], vocab: Uint32Array [nCat], trueIdx, predIdx: Int32Array [nCat][n], "
                        "trueVal, predVal: Float64Array [nOrd][n]})";
    table_args a;
    if (!box || argc < 2 || !table_read(env, argv[1], &a) || a.n_cat > 0xffff || a.n_ord > 0xffff) return fail_usage(env, usage);
    wsa_dbstats *db = NULL;
    wsa_status st = wsa_dbstats_create(box->ctx, NULL, a.dur, (uint32_t)a.n, (uint32_t)a.n_cat, a.vocab, (uint32_t)a.n_ord, &db);
    if (st == WSA_OK) st = table_set(db, &a);
    level_tables t;
    napi_value res = NULL;
    const int room = level_alloc(&t, a.n_cat, a.vocab, a.n_ord, 0);
    if (st == WSA_OK && !room) fail_oom(env);
    else {
        if (st == WSA_OK) st = wsa_dbstats_table(db, box->queue, t.cat, t.cls, t.od);
        if (st != WSA_OK) fail_lib(env, box->ctx);
        else { level_flatten(&t, 0); res = level_object(env, &t); }
    }
    if (db) wsa_dbstats_destroy(db);
    level_free(&t);
    return res;
}

// ---- evaluating a labelled DB beyond the panel (include/wsa_eval.h, K8e, specification EV-1): one synchronous call that builds the device object,
// predicts the heads that have a model, folds per file and returns every table; js/dbstats.js resolves the strings and assembles the result.
//   dbEval(ctx, {durations, vocab, trueIdx, predIdx, trueVal, predVal (as dbTable),
//                features: Float64Array [n][width], width (only with models), catModels: [model | null] per categorical head, catMaps: Int32Array [nCat][64]
//                legend -> vocabulary, ordModels: [model | null] per ordinal head, ordRange: Float64Array [nOrd][2],
// nFiles (0: no file level), fileOfRow, callbackOfRow: Int32Array [n], fileTrueIdx: Int32Array [nCat][nFiles], fileTrueVal: Float64Array [nOrd][nFiles]})
// -> {rows: {cat, cls, ord (as dbTable), conf: Float64Array, every head's [V][V + 1] one after the other, agree: Float64Array [nOrd][8] n, mean_true,
//     mean_pred,
//         var_true, var_pred, cov, ccc, pearson}, predIdx: Int32Array [nCat][n], predVal: Float64Array [nOrd][n] (after the predictions),
// files: null | {cat, cls, ord, conf, agree, idx: Int32Array [nCat][nFiles], val: Float64Array [nOrd][nFiles], sums: [Float64Array [nFiles][C] | null]}}
// Cross-validation (include/wsa_crossval.h, K6f, specification CV-1): with foldOfRow: Int32Array [n] (-1: never held out) and nFolds, a head's entry of
// catModels / ordModels may be an ARRAY of nFolds model handles — model k predicts the rows of fold k, one launch per head — and ordRange is then
// Float64Array [nOrd][nFolds][2], a range per member.  Without foldOfRow nothing changes.
typedef struct {
    table_args a;
    double *feat, *range, *ftv; int32_t *maps, *fo, *co, *fti, *fold; uint32_t width, n_files, n_folds;
    model_box *cm[WSA_DBSTATS_MAX_HEADS], *om[WSA_DBSTATS_MAX_HEADS];
    model_box *cmf[WSA_DBSTATS_MAX_HEADS][WSA_CROSSVAL_MAX_FOLDS], *omf[WSA_DBSTATS_MAX_HEADS][WSA_CROSSVAL_MAX_FOLDS];   /* [h][0] set: the head is predicted fold-wise */
} eval_args;
static napi_value eval_alloc_failed(napi_env env) { return fail_error(env, "dbEval: result allocation failed"); }
/* one level's tables into a new object: files = 0 the rows, 1 the files */
static napi_value eval_level(napi_env env, ctx_box *box, wsa_dbstats *db, int files, const table_args *a, wsa_status *st) {
    level_tables t;
    napi_value res = NULL;
    if (!level_alloc(&t, a->n_cat, a->vocab, a->n_ord, 1)) { *st = WSA_ERR_INVALID; fail_oom(env); level_free(&t); return NULL; }
    *st = files ? wsa_dbstats_file_table(db, box->queue, t.cat, t.cls, t.od) : wsa_dbstats_table(db, box->queue, t.cat, t.cls, t.od);
    for (size_t h = 0, off = 0; *st == WSA_OK && h < a->n_cat; off += (size_t)a->vocab[h] * (a->vocab[h] + 1), h++)
        *st = files ? wsa_dbstats_file_confusion(db, (uint32_t)h, box->queue, t.m + off) : wsa_dbstats_confusion(db, (uint32_t)h, box->queue, t.m + off);
    if (*st == WSA_OK && a->n_ord) *st = files ? wsa_dbstats_file_agreement(db, box->queue, t.ag) : wsa_dbstats_agreement(db, box->queue, t.ag);
    if (*st != WSA_OK) fail_lib(env, box->ctx);
    else {
        level_flatten(&t, 1);
        res = level_object(env, &t);
        if (!res || !put_typed(env, res, "conf", napi_float64_array, t.fm, t.cells) || !put_typed(env, res, "agree", napi_float64_array, t.fa, a->n_ord * 8)) {
            *st = WSA_ERR_INVALID; res = eval_alloc_failed(env);
        }
    }
    level_free(&t);
    return res;
}
/* element i of the array property `name`: a live model of this context, NULL for null / undefined; *bad set when it is anything else */
static model_box *eval_model(napi_env env, napi_value spec, const char *name, uint32_t i, ctx_box *box, int *bad) {
    napi_value arr, el; bool has = false; uint32_t len = 0;
    if (napi_has_named_property(env, spec, name, &has) != napi_ok || !has) return NULL;
    if (napi_get_named_property(env, spec, name, &arr) != napi_ok || !array_arg(env, arr, &len) || i >= len || napi_get_element(env, arr, i, &el) != napi_ok)
        { *bad = 1; return NULL; }
    if (is_nullish(env, el)) return NULL;
    model_box *mb = (model_box *)external_of(env, el);
    if (!mb || !child_is(&mb->link, box)) { *bad = 1; return NULL; }
    return mb;
}
/* the same element as an array of n_folds live models of this context into out[]: 1 when it is one, 0 when it is no array (or there are no folds) */
static int eval_fold_models(napi_env env, napi_value spec, const char *name, uint32_t i, ctx_box *box, uint32_t n_folds, model_box **out, int *bad) {
    napi_value arr, el, m; bool has = false, is = false; uint32_t len = 0, k = 0;
    if (!n_folds || napi_has_named_property(env, spec, name, &has) != napi_ok || !has) return 0;
    if (napi_get_named_property(env, spec, name, &arr) != napi_ok || !array_arg(env, arr, &len) || i >= len || napi_get_element(env, arr, i, &el) != napi_ok) return 0;
    if (napi_is_array(env, el, &is) != napi_ok || !is) return 0;
    if (napi_get_array_length(env, el, &len) != napi_ok || len != n_folds) { *bad = 1; return 1; }
    for (; k < n_folds; k++) {
        if (napi_get_element(env, el, k, &m) != napi_ok || !(out[k] = (model_box *)external_of(env, m)) || !child_is(&out[k]->link, box)) { *bad = 1; return 1; }
    }
    return 1;
}
/* dbEval's argument object: 1, or 0 with an exception pending */
static int eval_read(napi_env env, napi_value o, ctx_box *box, const char *usage, eval_args *e) {
    size_t nfeat = 0, nmaps = 0, nrange = 0, nfo = 0, nco = 0, nfti = 0, nftv = 0; napi_value v;
    memset(e, 0, sizeof *e);
    table_args *a = &e->a;
    if (!table_read(env, o, a) || a->n_cat > WSA_DBSTATS_MAX_HEADS || a->n_ord > WSA_DBSTATS_MAX_HEADS) { fail_usage(env, usage); return 0; }
    if (napi_get_named_property(env, o, "nFiles", &v) == napi_ok) (void)napi_get_value_uint32(env, v, &e->n_files);
    if (napi_get_named_property(env, o, "width", &v) == napi_ok) (void)napi_get_value_uint32(env, v, &e->width);
    const int with_feat = typed_of(env, o, "features", napi_float64_array, (void **)&e->feat, &nfeat);
    if (!with_feat) e->feat = NULL;
    if (with_feat && (!e->width || nfeat != a->n * (size_t)e->width)) { fail_usage(env, usage); return 0; }
    (void)typed_of(env, o, "catMaps", napi_int32_array, (void **)&e->maps, &nmaps);
    (void)typed_of(env, o, "ordRange", napi_float64_array, (void **)&e->range, &nrange);
    if (e->n_files && (!typed_of(env, o, "fileOfRow", napi_int32_array, (void **)&e->fo, &nfo) || !typed_of(env, o, "callbackOfRow", napi_int32_array,
        (void **)&e->co, &nco) ||
                       !typed_of(env, o, "fileTrueIdx", napi_int32_array, (void **)&e->fti, &nfti) || !typed_of(env, o, "fileTrueVal", napi_float64_array,
                           (void **)&e->ftv, &nftv) ||
                       nfo != a->n || nco != a->n || nfti != a->n_cat * e->n_files || nftv != a->n_ord * e->n_files)) { fail_usage(env, usage); return 0; }
    int bad = 0, any = 0;
    size_t nfold = 0;
    if (typed_of(env, o, "foldOfRow", napi_int32_array, (void **)&e->fold, &nfold)) {
        if (napi_get_named_property(env, o, "nFolds", &v) == napi_ok) (void)napi_get_value_uint32(env, v, &e->n_folds);
        if (nfold != a->n || e->n_folds < 2 || e->n_folds > WSA_CROSSVAL_MAX_FOLDS) { fail_error(env, "dbEval: foldOfRow is an Int32Array [n] and comes with nFolds 2 .. 32"); return 0; }
    } else e->fold = NULL;
    for (size_t h = 0; h < a->n_cat; h++)
        if (!eval_fold_models(env, o, "catModels", (uint32_t)h, box, e->n_folds, e->cmf[h], &bad)) e->cm[h] = eval_model(env, o, "catModels", (uint32_t)h, box, &bad);
    for (size_t h = 0; h < a->n_ord; h++)
        if (!eval_fold_models(env, o, "ordModels", (uint32_t)h, box, e->n_folds, e->omf[h], &bad)) e->om[h] = eval_model(env, o, "ordModels", (uint32_t)h, box, &bad);
    if (bad) {
        fail_error(env, e->n_folds ? "dbEval: catModels / ordModels hold one model handle of this context, an array of nFolds of them, or null, per head"
                                   : "dbEval: catModels / ordModels hold one model handle of this context, or null, per head");
        return 0;
    }
    for (size_t h = 0; h < WSA_DBSTATS_MAX_HEADS; h++) any |= e->cm[h] != NULL || e->om[h] != NULL || e->cmf[h][0] != NULL || e->omf[h][0] != NULL;
    if (any && (!with_feat || nmaps != a->n_cat * WSA_MODEL_MAX_CLASSES || nrange != a->n_ord * 2 * (e->n_folds ? e->n_folds : 1))) { fail_usage(env, usage); return 0; }
    return 1;
}
/* the device object with every label, prediction and file table set */
static wsa_status eval_create(ctx_box *box, const eval_args *e, wsa_dbstats **db) {
    const table_args *a = &e->a; const uint32_t nf = e->n_files;
    wsa_status st = e->feat ? wsa_wide_dbstats_create(box->ctx, e->feat, e->width, a->dur, (uint32_t)a->n, (uint32_t)a->n_cat, a->vocab, (uint32_t)a->n_ord, db)
                            : wsa_dbstats_create(box->ctx, NULL, a->dur, (uint32_t)a->n, (uint32_t)a->n_cat, a->vocab, (uint32_t)a->n_ord, db);
    if (st == WSA_OK) st = table_set(*db, a);
    if (st == WSA_OK && nf) st = wsa_dbstats_set_files(*db, e->fo, e->co, nf);
    for (size_t h = 0; st == WSA_OK && nf && h < a->n_cat; h++) st = wsa_dbstats_set_file_classes(*db, (uint32_t)h, e->fti + h * nf);
    for (size_t o = 0; st == WSA_OK && nf && o < a->n_ord; o++) st = wsa_dbstats_set_file_values(*db, (uint32_t)o, e->ftv + o * nf);
    if (st == WSA_OK && e->fold && e->feat) st = wsa_dbstats_set_folds(*db, e->fold, e->n_folds);
    return st;
}
// the heads that have a model predicted and folded per file (a head is folded right after its prediction: the fold reads the probabilities that call
// kept), sums[h] set to the head's file sums or null; then every head's predictions into idx / val
static wsa_status eval_predict(napi_env env, ctx_box *box, wsa_dbstats *db, const eval_args *e, napi_value sums, double *fs, int32_t *idx, double *val) {
    const table_args *a = &e->a; const uint32_t nf = e->n_files, K = e->n_folds, per = K ? K : 1;     /* per: ranges per ordinal head */
    const wsa_model *members[WSA_CROSSVAL_MAX_FOLDS]; double lo[WSA_CROSSVAL_MAX_FOLDS], hi[WSA_CROSSVAL_MAX_FOLDS];
    wsa_status st = WSA_OK;
    for (size_t h = 0; st == WSA_OK && h < a->n_cat; h++) {
        napi_value s_h = NULL;
        const model_box *first = e->cmf[h][0] ? e->cmf[h][0] : e->cm[h];
        if (first) {
            if (e->cmf[h][0]) {
                for (uint32_t k = 0; k < K; k++) members[k] = model_of(e->cmf[h][k]);
                st = wsa_dbstats_predict_classes_folds(db, (uint32_t)h, members, K, e->maps + h * WSA_MODEL_MAX_CLASSES, box->queue);
            } else st = wsa_dbstats_predict_classes(db, (uint32_t)h, model_of(e->cm[h]), e->maps + h * WSA_MODEL_MAX_CLASSES, box->queue);
            if (st == WSA_OK && nf) st = wsa_dbstats_fold_files(db, (uint32_t)h, box->queue);
            if (st == WSA_OK && nf) st = wsa_dbstats_copy_file_sums(db, (uint32_t)h, box->queue, fs, first->n_classes);
            if (st == WSA_OK && nf) s_h = make_typed(env, napi_float64_array, fs, (size_t)nf * first->n_classes);
        }
        if (st == WSA_OK && nf) { if (!s_h) napi_get_null(env, &s_h); napi_set_element(env, sums, (uint32_t)h, s_h); }
    }
    for (size_t o = 0; st == WSA_OK && o < a->n_ord; o++) {
        if (e->omf[o][0]) {
            for (uint32_t k = 0; k < K; k++) { members[k] = model_of(e->omf[o][k]); lo[k] = e->range[(o * K + k) * 2]; hi[k] = e->range[(o * K + k) * 2 + 1]; }
            st = wsa_dbstats_predict_values_folds(db, (uint32_t)o, members, K, lo, hi, box->queue);
        } else if (e->om[o]) st = wsa_dbstats_predict_values(db, (uint32_t)o, model_of(e->om[o]), e->range[o * per * 2], e->range[o * per * 2 + 1], box->queue);
        if (st == WSA_OK && nf) st = wsa_dbstats_fold_file_values(db, (uint32_t)o, box->queue);
    }
    for (size_t h = 0; st == WSA_OK && h < a->n_cat; h++) st = wsa_dbstats_copy_classes(db, (uint32_t)h, box->queue, idx + h * a->n);
    for (size_t o = 0; st == WSA_OK && o < a->n_ord; o++) st = wsa_dbstats_copy_values(db, (uint32_t)o, box->queue, val + o * a->n);
    return st;
}
/* the file level: its tables with idx, val and sums; NULL with an exception pending */
static napi_value eval_files(napi_env env, ctx_box *box, wsa_dbstats *db, const eval_args *e, napi_value sums, int32_t *idx, double *val) {
    const table_args *a = &e->a; const uint32_t nf = e->n_files;
    wsa_status st = WSA_OK;
    napi_value files = eval_level(env, box, db, 1, a, &st);
    if (!files) return NULL;
    for (size_t h = 0; st == WSA_OK && h < a->n_cat; h++) st = wsa_dbstats_copy_file_classes(db, (uint32_t)h, box->queue, idx + h * nf);
    for (size_t o = 0; st == WSA_OK && o < a->n_ord; o++) st = wsa_dbstats_copy_file_values(db, (uint32_t)o, box->queue, val + o * nf);
    if (st != WSA_OK) return fail_lib(env, box->ctx);
    if (!put_typed(env, files, "idx", napi_int32_array, idx, a->n_cat * nf) || !put_typed(env, files, "val", napi_float64_array, val, a->n_ord * nf) ||
        !put(env, files, "sums", sums)) return eval_alloc_failed(env);
    return files;
}
napi_value fn_db_eval(napi_env env, napi_callback_info info) {
    ARGS(2);
    ctx_box *box = box_arg(env, argc, argv);
    const char *usage = "dbEval(ctx, {durations, vocab, trueIdx, predIdx, trueVal, predVal, [features, width, catModels, catMaps, ordModels, ordRange], "
                        "[nFiles, fileOfRow, callbackOfRow, fileTrueIdx, fileTrueVal]})";
    eval_args e;
    if (!box || argc < 2) return fail_usage(env, usage);
    if (!eval_read(env, argv[1], box, usage, &e)) return NULL;
    const table_args *a = &e.a;
    wsa_dbstats *db = NULL;
    napi_value res = NULL, rows = NULL, files = NULL, sums = NULL;
    const size_t longest = a->n > e.n_files ? a->n : e.n_files;
    int32_t *idx = calloc(a->n_cat * longest + 1, sizeof *idx); double *val = calloc(a->n_ord * longest + 1, sizeof *val);
    double *fs = calloc((size_t)OR1(e.n_files) * WSA_MODEL_MAX_CLASSES, sizeof *fs);
    wsa_status st = WSA_OK;
    if (!idx || !val || !fs) { fail_oom(env); goto done; }
    st = eval_create(box, &e, &db);
    if (st == WSA_OK && e.n_files && napi_create_array_with_length(env, a->n_cat, &sums) != napi_ok) { eval_alloc_failed(env); goto done; }
    if (st == WSA_OK) st = eval_predict(env, box, db, &e, sums, fs, idx, val);
    if (st != WSA_OK) { fail_lib(env, box->ctx); goto done; }
    if (napi_create_object(env, &res) != napi_ok || !put_typed(env, res, "predIdx", napi_int32_array, idx, a->n_cat * a->n) ||
        !put_typed(env, res, "predVal", napi_float64_array, val, a->n_ord * a->n)) { res = eval_alloc_failed(env); goto done; }
    rows = eval_level(env, box, db, 0, a, &st);
    if (e.n_files) files = rows ? eval_files(env, box, db, &e, sums, idx, val) : NULL;
    else napi_get_null(env, &files);
    if (!rows || !files) { res = NULL; goto done; }
    put(env, res, "rows", rows);
    put(env, res, "files", files);
done:
    if (db) wsa_dbstats_destroy(db);
    free(idx); free(val); free(fs);
    return res;
}

// ---- the feature DB that stays on the device (wsa_featdb_*, K10, specification FD-1).  featdbAppendBatch is with the batches (napi_batch.c),
// streamSetFeatdb and
// streamDbRows with the streams (napi_stream.c).
/* featdbCreate(ctx, width, capacity) -> handle */
napi_value fn_featdb_create(napi_env env, napi_callback_info info) {
    ARGS(3);
    ctx_box *box = box_arg(env, argc, argv);
    int32_t width = 0; uint32_t cap = 0;
    if (!box || argc < 3 || napi_get_value_int32(env, argv[1], &width) != napi_ok || napi_get_value_uint32(env, argv[2], &cap) != napi_ok)
        return fail_usage(env, "featdbCreate(ctx, width, capacity)");
    wsa_featdb *db = NULL;
    if (wsa_featdb_create(box->ctx, width, cap, &db) != WSA_OK) return fail_lib(env, box->ctx);
    fdb_box *fb = (fdb_box *)child_new(sizeof *fb, db, box, &box->fdbs);
    if (!fb) { wsa_featdb_destroy(db); return fail_oom(env); }
    fb->width = (uint32_t)width;
    return child_handle(env, &fb->link);
}
/* featdbDestroy(handle): refused while the DB's context has a batch or a training run in flight or open streams */
napi_value fn_featdb_destroy(napi_env env, napi_callback_info info) {
    ARGS(1);
    fdb_box *fb = argc ? (fdb_box *)external_of(env, argv[0]) : NULL;
    if (!fb) return fail_usage(env, "featdbDestroy(db)");
    ctx_box *box = fb->link.owner;
    if (box && box->children) return fail_error(env, "the device DB's context has a batch or a training run in flight");
    if (fb->link.obj) { wsa_featdb_destroy(fdb_of(fb)); fb->link.obj = NULL; }
    if (box) child_unlink(&fb->link, &box->fdbs);
    return NULL;
}
/* the idle DB of argv[0] for the export `usage`, or NULL with an exception pending */
static fdb_box *fdb_arg0(napi_env env, size_t argc, const napi_value *argv, const char *usage) {
    if (!argc) { fail_usage(env, usage); return NULL; }
    return fdb_idle(env, argv[0], usage);
}
/* featdbCount(handle) -> rows held */
napi_value fn_featdb_count(napi_env env, napi_callback_info info) {
    ARGS(1);
    fdb_box *fb = fdb_arg0(env, argc, argv, "featdbCount(db)");
    if (!fb) return NULL;
    uint32_t n = 0; napi_value out;
    wsa_featdb_count(fdb_of(fb), &n);
    NAPI_OK(env, napi_create_uint32(env, n, &out));
    return out;
}
/* featdbCopyRows(db) -> Float64Array [count][width] */
napi_value fn_featdb_copy_rows(napi_env env, napi_callback_info info) {
    ARGS(1);
    fdb_box *fb = fdb_arg0(env, argc, argv, "featdbCopyRows(db)");
    if (!fb) return NULL;
    uint32_t n = 0;
    wsa_featdb_count(fdb_of(fb), &n);
    napi_value ab, ta; void *data = NULL;
    const size_t words = (size_t)n * fb->width;
    if (napi_create_arraybuffer(env, words * sizeof(double), &data, &ab) != napi_ok || napi_create_typedarray(env, napi_float64_array, words, ab, 0,
        &ta) != napi_ok) return fail_oom(env);
    if (wsa_featdb_copy_rows(fdb_of(fb), fb->link.owner->queue, 0, n, (double *)data) != WSA_OK) return fail_lib(env, fb->link.owner->ctx);
    return ta;
}
/* featdbRanges(db, rows: Uint32Array) -> {min, max}: Float64Array [width] */
napi_value fn_featdb_ranges(napi_env env, napi_callback_info info) {
    ARGS(2);
    const char *usage = "featdbRanges(db, rows: Uint32Array)";
    fdb_box *fb = fdb_arg0(env, argc, argv, usage);
    if (!fb) return NULL;
    void *rows = NULL; size_t n = 0;
    if (argc < 2 || !typed_arg(env, argv[1], napi_uint32_array, &rows, &n) || n < 1 || n > 0xffffffffu) return fail_usage(env, usage);
    double mn[WSA_NUTT], mx[WSA_NUTT];
    if (wsa_featdb_ranges(fdb_of(fb), (const uint32_t *)rows, (uint32_t)n, fb->link.owner->queue, mn, mx) != WSA_OK) return fail_lib(env, fb->link.owner->ctx);
    napi_value out; NAPI_OK(env, napi_create_object(env, &out));
    put_typed(env, out, "min", napi_float64_array, mn, fb->width);
    put_typed(env, out, "max", napi_float64_array, mx, fb->width);
    return out;
}

// ---- the app's ml5 KNN classifier (wsa_knn_*, K9, specification KN-1): what train_knn does with ml5.KNNClassifier() (ref src/neuralmodel.js:729-837).
// js/knn.js resolves the labels (ml5's class order) and hands over class indices.  Rows travel through one page-locked allocation the device reads and
// writes in place.  batchKnn and batchKnnFold are with the batches (napi_batch.c), streamSetKnn with the streams (napi_stream.c).
/* knnCreate(ctx, width, nClasses, capacity) -> handle */
napi_value fn_knn_create(napi_env env, napi_callback_info info) {
    ARGS(4);
    ctx_box *box = box_arg(env, argc, argv);
    int32_t width = 0, classes = 0; uint32_t cap = 0;
    if (!box || argc < 4 || napi_get_value_int32(env, argv[1], &width) != napi_ok || napi_get_value_int32(env, argv[2], &classes) != napi_ok ||
        napi_get_value_uint32(env, argv[3], &cap) != napi_ok) return fail_usage(env, "knnCreate(ctx, width, nClasses, capacity)");
    wsa_knn *k = NULL;
    if (wsa_knn_create(box->ctx, width, classes, cap, &k) != WSA_OK) return fail_lib(env, box->ctx);
    knn_box *kb = (knn_box *)child_new(sizeof *kb, k, box, &box->knns);
    if (!kb) { wsa_knn_destroy(k); return fail_oom(env); }
    kb->width = (uint32_t)width; kb->n_classes = (uint32_t)classes;
    return child_handle(env, &kb->link);
}
/* knnDestroy(handle): refused while the store's context has a batch in flight or open streams */
napi_value fn_knn_destroy(napi_env env, napi_callback_info info) {
    ARGS(1);
    knn_box *kb = argc ? (knn_box *)external_of(env, argv[0]) : NULL;
    if (!kb) return fail_usage(env, "knnDestroy(knn)");
    ctx_box *box = kb->link.owner;
    if (box && box->children) return fail_error(env, "the KNN store's context has a batch in flight or open streams");
    if (box) box_drop_plan(box);         /* the kept plan's KNN tables name the store */
    if (kb->link.obj) { wsa_knn_destroy(knn_of(kb)); kb->link.obj = NULL; }
    if (box) child_unlink(&kb->link, &box->knns);
    return NULL;
}
/* knnAdd(knn, features: Float64Array [n][width], classes: Int32Array [n]) -> {rows, perClass: Uint32Array [nClasses]}  (addExample, n rows at once) */
napi_value fn_knn_add(napi_env env, napi_callback_info info) {
    ARGS(3);
    const char *usage = "knnAdd(knn, features: Float64Array [n][width], classes: Int32Array [n])";
    knn_box *kb = argc ? (knn_box *)external_of(env, argv[0]) : NULL;
    void *feat = NULL, *cls = NULL; size_t nf = 0, n = 0;
    if (!kb || argc < 3 || !typed_arg(env, argv[1], napi_float64_array, &feat, &nf) || !typed_arg(env, argv[2], napi_int32_array, &cls, &n) ||
        (kb->width && (nf != n * kb->width || n > 0xffffffffu))) return fail_usage(env, usage);
    ctx_box *box = kb->link.owner;
    if (!kb->link.obj || !box || !box->ctx) return fail_error(env, "knnAdd: the KNN store was destroyed");
    void *slab = NULL;
    if (wsa_host_alloc(box->ctx, (uint64_t)(nf + 1) * sizeof(double) + (uint64_t)(n + 1) * sizeof(int32_t), &slab) != WSA_OK) return fail_lib(env, box->ctx);
    double *rows = (double *)slab; int32_t *ci = (int32_t *)(rows + nf + 1);
    if (nf) memcpy(rows, feat, nf * sizeof(double));
    if (n) memcpy(ci, cls, n * sizeof(int32_t));
    uint32_t total = 0, per[WSA_MODEL_MAX_CLASSES] = {0};
    wsa_status st = wsa_knn_add(knn_of(kb), rows, ci, (uint32_t)n, box->queue);
    if (st == WSA_OK) st = wsa_knn_count(knn_of(kb), box->queue, &total, per);
    napi_value out = NULL;
    if (st != WSA_OK) fail_lib(env, box->ctx);
    else {
        out = new_object(env);
        put_u32(env, out, "rows", total);
        put_typed(env, out, "perClass", napi_uint32_array, per, kb->n_classes);
    }
    wsa_host_free(slab);
    return out;
}
// knnClassify(knn, features: Float64Array [n][width], k) -> {label: Int32Array [n], conf: Float64Array [n][nClasses], nbr: Int32Array [n][k],
// sim: Float32Array [n][k], k, kEff, nClasses}  (the tables of wsa_knn_classify_rows)
napi_value fn_knn_classify(napi_env env, napi_callback_info info) {
    ARGS(3);
    const char *usage = "knnClassify(knn, features: Float64Array [n][width], k)";
    knn_box *kb = argc ? (knn_box *)external_of(env, argv[0]) : NULL;
    void *feat = NULL; size_t nf = 0; uint32_t k = 0;
    if (!kb || argc < 3 || !typed_arg(env, argv[1], napi_float64_array, &feat, &nf) || napi_get_value_uint32(env, argv[2], &k) != napi_ok ||
        (kb->width && (nf % kb->width || nf / kb->width > 0xffffffffu))) return fail_usage(env, usage);
    ctx_box *box = kb->link.owner;
    if (!kb->link.obj || !box || !box->ctx) return fail_error(env, "knnClassify: the KNN store was destroyed");
    if (k < 1 || k > WSA_KNN_MAX_K) return fail_error(env, "knnClassify: k must be 1 .. 64");
    const size_t n = nf / kb->width, head = (nf + 1) * sizeof(double);       /* the rows in front of the tables, in one page-locked slab */
    const uint32_t C = kb->n_classes;
    void *slab = NULL;
    if (wsa_host_alloc(box->ctx, (uint64_t)head + knn_slab_bytes(n, k, C), &slab) != WSA_OK) return fail_lib(env, box->ctx);
    if (nf) memcpy(slab, feat, nf * sizeof(double));
    const knn_slab t = knn_slab_at((char *)slab + head, n, k);
    uint32_t total = 0;
    wsa_status st = wsa_knn_classify_rows(knn_of(kb), (const double *)slab, (uint32_t)n, k, t.label, t.conf, t.nbr, t.sim, box->queue);
    if (st == WSA_OK) st = wsa_knn_count(knn_of(kb), box->queue, &total, NULL);          /* synchronises; k_eff = min(k, rows) */
    napi_value out = st == WSA_OK ? knn_object(env, &t, n, k, k < total ? k : total, C) : fail_lib(env, box->ctx);
    wsa_host_free(slab);
    return out;
}
