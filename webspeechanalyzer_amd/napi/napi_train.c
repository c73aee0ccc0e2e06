// napi_train.c — the app's models: modelCreate / modelDestroy, train and trainGroup (each run on a thread of its own, its messages delivered through a
// thread-safe function), regressRows.
#include <pthread.h>
#include "napi_handles.h"

/* -- a model spec ({units, activation, kernels, biases, inMin, inMax}), as modelCreate and train read it */
typedef struct { int32_t *units, *act; double *mn, *mx; size_t nu, na; napi_value ka, ba; } spec_args;
/* units (2 .. WSA_MODEL_MAX_LAYERS + 1 widths), activation (one per layer), inMin / inMax (units[0] entries) */
static int spec_read(napi_env env, napi_value spec, spec_args *s) {
    size_t nmn = 0, nmx = 0;
    return typed_of(env, spec, "units", napi_int32_array, (void **)&s->units, &s->nu) && typed_of(env, spec, "activation", napi_int32_array,
        (void **)&s->act, &s->na) &&
           typed_of(env, spec, "inMin", napi_float64_array, (void **)&s->mn, &nmn) && typed_of(env, spec, "inMax", napi_float64_array, (void **)&s->mx, &nmx) &&
           s->nu >= 2 && s->na == s->nu - 1 && s->na <= WSA_MODEL_MAX_LAYERS && s->units[0] >= 1 && nmn == (size_t)s->units[0] && nmx == (size_t)s->units[0];
}
/* kernels / biases: arrays with one entry per layer */
static int spec_weights(napi_env env, napi_value spec, spec_args *s) {
    uint32_t nk = 0, nb = 0;
    return napi_get_named_property(env, spec, "kernels", &s->ka) == napi_ok && array_arg(env, s->ka, &nk) &&
           napi_get_named_property(env, spec, "biases", &s->ba) == napi_ok && array_arg(env, s->ba, &nb) && nk == s->na && nb == s->na;
}
/* layer l: kernels[l] a Float32Array of units[l] x units[l+1], biases[l] one of units[l+1] */
static int spec_layer(napi_env env, const spec_args *s, uint32_t l, const float **k, const float **b) {
    napi_value kv, bv;
    return napi_get_element(env, s->ka, l, &kv) == napi_ok && typed_arg_n(env, kv, napi_float32_array, (size_t)s->units[l] * (size_t)s->units[l + 1],
        (void **)k) &&
           napi_get_element(env, s->ba, l, &bv) == napi_ok && typed_arg_n(env, bv, napi_float32_array, (size_t)s->units[l + 1], (void **)b);
}
/* labels (optional): nl strings, legend order; NULL when the spec has none of that count */
static char **spec_labels(napi_env env, napi_value spec, uint32_t nl) {
    napi_value la; uint32_t n = 0;
    if (napi_get_named_property(env, spec, "labels", &la) != napi_ok || !array_arg(env, la, &n) || n != nl) return NULL;
    char **labels = calloc(nl, sizeof(char *));
    for (uint32_t i = 0; labels && i < nl; i++) {
        napi_value e; size_t len = 0;
        if (napi_get_element(env, la, i, &e) != napi_ok || napi_get_value_string_utf8(env, e, NULL, 0, &len) != napi_ok) { labels[i] = calloc(1, 1); continue; }
        labels[i] = calloc(len + 1, 1);
        if (labels[i]) napi_get_value_string_utf8(env, e, labels[i], len + 1, &len);
    }
    return labels;
}

// modelCreate(ctx, {units, activation, kernels, biases, inMin, inMax, labels}) -> handle (wsa_model_create): the app's classifier or regression model.  The
// handle is a box: after modelDestroy() or its context's destroy() any use throws instead of touching freed memory.
napi_value fn_model_create(napi_env env, napi_callback_info info) {
    ARGS(2);
    ctx_box *box = box_arg(env, argc, argv);
    const char *usage = "modelCreate(ctx, {units: Int32Array, activation: Int32Array, kernels: Float32Array[], biases: Float32Array[], "
                        "inMin: Float64Array, inMax: Float64Array, labels: string[]})";
    spec_args s;
    if (!box || argc < 2 || !spec_read(env, argv[1], &s) || !spec_weights(env, argv[1], &s)) return fail_usage(env, usage);
    const float *kp[WSA_MODEL_MAX_LAYERS], *bp[WSA_MODEL_MAX_LAYERS];
    for (uint32_t l = 0; l < s.na; l++)
        if (!spec_layer(env, &s, l, &kp[l], &bp[l]))
            return fail_usage(env, "modelCreate: kernels[i] must be a Float32Array of units[i] x units[i+1], biases[i] one of units[i+1]");
    const uint32_t nl = (uint32_t)s.units[s.na];
    char **labels = spec_labels(env, argv[1], nl);
    wsa_model_desc d = {(int32_t)s.na, s.units, s.act, kp, bp, s.mn, s.mx, (const char *const *)labels};
    wsa_model *m = NULL;
    const wsa_status st = wsa_model_create(box->ctx, &d, &m);
    for (uint32_t i = 0; labels && i < nl; i++) free(labels[i]);
    free(labels);
    if (st != WSA_OK) return fail_lib(env, box->ctx);
    model_box *mb = (model_box *)child_new(sizeof *mb, m, box, &box->models);
    if (!mb) { wsa_model_destroy(m); return fail_oom(env); }
    mb->n_classes = nl; mb->n_inputs = (uint32_t)s.units[0];
    return child_handle(env, &mb->link);
}
// modelDestroy(model): refused while a batch in flight or an open stream uses the model; the context's kept ensemble and regress group go first if they
// hold it
napi_value fn_model_destroy(napi_env env, napi_callback_info info) {
    ARGS(1);
    model_box *mb = argc ? (model_box *)external_of(env, argv[0]) : NULL;
    if (!mb) return fail_usage(env, "modelDestroy(model)");
    ctx_box *box = mb->link.owner;
    if (mb->busy) return fail_error(env, "the model is in use by a batch in flight or an open stream");
    if (box && box->ens) {          /* the context's kept ensemble may hold it: no job is in flight with it (busy is 0), so it goes first */
        for (uint32_t d = 0; d < box->ens_n; d++) if (box->ens_models[d] == mb) {
            if (box->children) return fail_error(env, "the model is part of the context's ensemble while a batch is in flight");
            box_drop_ensemble(box); break;
        }
    }
    if (box && box->reg)            /* ... and so may its kept regression group (batchRegressGroup is synchronous: nothing is in flight with it) */
        for (uint32_t d = 0; d < box->reg_n; d++) if (box->reg_models[d] == mb) { box_drop_regress(box); break; }
    if (mb->link.obj) { wsa_model_destroy(model_of(mb)); mb->link.obj = NULL; }
    if (box) child_unlink(&mb->link, &box->models);
    return NULL;
}

// ---- training (wsa_trainer_*, K7): train(ctx, spec, {features: Float64Array [n][units[0]] (53, 264 or 23 wide) | db + rows: Uint32Array, y: Int32Array [n] |
// values: Float64Array + outMin + outMax, nVal, batchSize, learningRate, epochs, orders: Uint32Array [epochs][n - nVal] | undefined}, onEpoch | undefined)
// -> Promise of {kernels: Float32Array[], biases: Float32Array[], history: Float64Array [epochs][4] = loss, acc, val_loss, val_acc}.  `spec` is modelCreate's
// object and holds the INITIAL weights.  `values` (the label's real values) with `outMin` / `outMax` in place of `y`: a regression run (specification TR-2).
// `db` (a featdbCreate handle of this context) with `rows` (its row indices) in place of `features`: the rows stay on the device.  The epochs run on a
// thread of their own (the inputs are copied first); after every epoch onEpoch(epoch, {loss, acc, val_loss, val_acc}) is queued to the JS thread (ml5's
// whileTraining), and the Promise settles after the last of them was delivered: both go through one first-in first-out queue.
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
/* what both kinds of run send to the JS thread: epoch >= 0: job `member` finished that epoch; epoch < 0: the run is over */
typedef struct { void *run; uint32_t member; int32_t epoch; wsa_train_stats s; } train_msg;

/* everything a job owns, its onEpoch reference included (JS thread; env NULL: the environment is gone and took the reference with it) */
static void train_job_release(napi_env env, train_job *j) {
    if (env && j->on_epoch) napi_delete_reference(env, j->on_epoch);
    for (int l = 0; l < WSA_MODEL_MAX_LAYERS; l++) { free(j->kernel[l]); free(j->bias[l]); }
    free(j->feat); free(j->y); free(j->values); free(j->orders); free(j->history); free(j->rows); free(j);
}
/* the trainer of a job: from host rows, or from the rows of a device feature DB */
static wsa_status train_job_trainer(wsa_ctx *ctx, const train_job *j, wsa_trainer **t) {
    const wsa_model_desc d = {j->nl, j->units, j->act, (const float *const *)j->kernel, (const float *const *)j->bias, j->mn, j->mx, NULL};
    if (j->db) return j->values ? wsa_regress_trainer_create_db(ctx, &d, j->db, j->rows, j->values, j->n, j->n_val, j->batch, j->lr, j->out_min, j->out_max, t)
                                : wsa_trainer_create_db(ctx, &d, j->db, j->rows, j->y, j->n, j->n_val, j->batch, j->lr, t);
    return j->values ? wsa_regress_trainer_create(ctx, &d, j->feat, j->values, j->n, j->n_val, j->batch, j->lr, j->out_min, j->out_max, t)
                     : wsa_trainer_create(ctx, &d, j->feat, j->y, j->n, j->n_val, j->batch, j->lr, t);
}
static const uint32_t *train_job_order(const train_job *j, uint32_t epoch) { return j->orders ? j->orders + (size_t)epoch * (j->n - j->n_val) : NULL; }
/* (worker thread) an epoch's statistics into the job's history and, as a message, to the JS thread */
static void train_job_epoch_done(train_job *j, void *run, uint32_t member, uint32_t e, const wsa_train_stats *s, napi_threadsafe_function tsfn) {
    j->history[4 * e] = s->loss; j->history[4 * e + 1] = s->acc; j->history[4 * e + 2] = s->val_loss; j->history[4 * e + 3] = s->val_acc;
    train_msg *m = malloc(sizeof *m);
    if (m) { m->run = run; m->member = member; m->epoch = (int32_t)e; m->s = *s; if (napi_call_threadsafe_function(tsfn, m,
        napi_tsfn_blocking) != napi_ok) free(m); }
}
static void train_run_over(void *run, napi_threadsafe_function tsfn) {
    train_msg *m = malloc(sizeof *m);                       /* (a few bytes: if even this fails the Promise stays pending) */
    if (m) { m->run = run; m->member = 0; m->epoch = -1; napi_call_threadsafe_function(tsfn, m, napi_tsfn_blocking); }
}
static void *train_thread(void *arg) {
    train_job *j = (train_job *)arg;
    wsa_ctx *ctx = j->box->ctx;
    wsa_trainer *t = NULL;
    j->st = train_job_trainer(ctx, j, &t);
    for (uint32_t e = 0; j->st == WSA_OK && e < j->epochs; e++) {
        j->st = wsa_trainer_epoch(t, train_job_order(j, e), j->box->queue);
        wsa_train_stats s;
        if (j->st == WSA_OK) j->st = wsa_trainer_stats(t, j->box->queue, &s);
        if (j->st != WSA_OK) break;
        train_job_epoch_done(j, j, 0, e, &s, j->tsfn);
    }
    if (j->st == WSA_OK) j->st = wsa_trainer_copy_weights(t, j->box->queue, j->kernel, j->bias);
    if (j->st != WSA_OK) snprintf(j->err, sizeof j->err, "%s", wsa_last_error(ctx));
    if (t) wsa_trainer_destroy(t);
    train_run_over(j, j->tsfn);
    return NULL;
}
/* {kernels, biases, history} of a finished job */
static napi_value train_result(napi_env env, train_job *j) {
    napi_value o = new_object(env), ka, ba;
    napi_create_array_with_length(env, (size_t)j->nl, &ka); napi_create_array_with_length(env, (size_t)j->nl, &ba);
    for (int l = 0; l < j->nl; l++) {
        napi_set_element(env, ka, (uint32_t)l, make_typed(env, napi_float32_array, j->kernel[l], (size_t)j->units[l] * (size_t)j->units[l + 1]));
        napi_set_element(env, ba, (uint32_t)l, make_typed(env, napi_float32_array, j->bias[l], (size_t)j->units[l + 1]));
    }
    put(env, o, "kernels", ka); put(env, o, "biases", ba);
    put_typed(env, o, "history", napi_float64_array, j->history, (size_t)j->epochs * 4);
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
    train_job *j = (train_job *)m->run;
    const int32_t epoch = m->epoch; const wsa_train_stats s = m->s;
    free(m);
    if (!env) return;
    if (epoch >= 0) { train_on_epoch(env, j, epoch, &s); return; }
    pthread_join(j->thread, NULL);
    if (j->box->children) j->box->children--;
    settle(env, j->deferred, j->st != WSA_OK ? j->err : NULL, j->st != WSA_OK ? NULL : train_result(env, j));
    napi_release_threadsafe_function(j->tsfn, napi_tsfn_release);
    train_job_release(env, j);
}
static const char *TRAIN_USAGE = "train(ctx, {units, activation, kernels, biases, inMin, inMax}, {features: Float64Array | db + rows: Uint32Array, "
                                 "y: Int32Array | values: Float64Array + outMin + outMax, nVal, batchSize, learningRate, epochs, "
                                 "orders?: Uint32Array}, onEpoch?)";
/* what a run object (train's third argument) holds, checked against the spec's input width */
typedef struct {
    int32_t *y; double *feat, *values; uint32_t *orders, *rows; size_t ny, nf, no, nr; fdb_box *fb;
    double n_val, batch, lr, epochs, out_min, out_max;
} run_args;
/* 1, or 0 with an exception pending */
static int run_read(napi_env env, napi_value run, ctx_box *box, const spec_args *s, int spec_ok, run_args *r) {
    memset(r, 0, sizeof *r);
    const int regress = typed_of(env, run, "values", napi_float64_array, (void **)&r->values, &r->ny);
    napi_value dv;
    if (napi_get_named_property(env, run, "db", &dv) == napi_ok) r->fb = (fdb_box *)external_of(env, dv);
    if (r->fb && !child_is(&r->fb->link, box)) { fail_error(env, "train: the device DB was destroyed or belongs to another context"); return 0; }
    const int ok = (!r->fb || typed_of(env, run, "rows", napi_uint32_array, (void **)&r->rows, &r->nr)) &&
        (!regress || (num_of(env, run, "outMin", &r->out_min) && num_of(env, run, "outMax", &r->out_max))) &&
        spec_ok && s->units[0] <= WSA_NUTT &&
        (r->fb || typed_of(env, run, "features", napi_float64_array, (void **)&r->feat, &r->nf)) && (regress || typed_of(env, run, "y", napi_int32_array,
            (void **)&r->y, &r->ny)) &&
        r->ny >= 1 && (r->fb ? r->nr == r->ny : r->nf == r->ny * (size_t)s->units[0]) && r->ny <= 0xffffffffu &&
        num_of(env, run, "nVal", &r->n_val) && num_of(env, run, "batchSize", &r->batch) && num_of(env, run, "learningRate", &r->lr) && num_of(env, run,
            "epochs", &r->epochs) &&
        r->n_val >= 0 && r->n_val < (double)r->ny && r->batch >= 0 && r->batch <= 4294967295.0 && r->epochs >= 1 && r->epochs <= 1e6;
    if (!ok) { fail_usage(env, TRAIN_USAGE); return 0; }
    const uint32_t n_train = (uint32_t)r->ny - (uint32_t)r->n_val;
    if (typed_of(env, run, "orders", napi_uint32_array, (void **)&r->orders, &r->no) && r->no != (size_t)r->epochs * n_train) {
        fail_usage(env, "train: orders must hold epochs x (rows - nVal) indices"); return 0;
    }
    return 1;
}
// a job from train's arguments (argv[0] unused, argv[1] the spec, argv[2] the run, argv[3] onEpoch when argc > 3), the inputs copied; NULL with an
// exception pending
static train_job *train_job_from(napi_env env, ctx_box *box, size_t argc, const napi_value *argv) {
    spec_args s; run_args r;
    const int spec_ok = spec_read(env, argv[1], &s);
    if (!run_read(env, argv[2], box, &s, spec_ok, &r)) return NULL;
    if (!spec_weights(env, argv[1], &s)) { fail_usage(env, TRAIN_USAGE); return NULL; }
    for (size_t l = 0; l <= s.na; l++)
        if (s.units[l] < 1 || s.units[l] > WSA_MODEL_MAX_WIDTH) { fail_usage(env, "train: layer widths are 1 .. 1024"); return NULL; }
    train_job *j = calloc(1, sizeof *j);
    if (!j) { fail_oom(env); return NULL; }
    j->box = box; j->nl = (int32_t)s.na; j->n = (uint32_t)r.ny; j->n_val = (uint32_t)r.n_val; j->batch = (uint32_t)r.batch; j->epochs = (uint32_t)r.epochs;
        j->lr = r.lr;
    memcpy(j->units, s.units, s.nu * sizeof(int32_t)); memcpy(j->act, s.act, s.na * sizeof(int32_t));
    memcpy(j->mn, s.mn, (size_t)s.units[0] * sizeof(double)); memcpy(j->mx, s.mx, (size_t)s.units[0] * sizeof(double));
    bool ok = true;
    for (uint32_t l = 0; l < s.na && ok; l++) {
        const float *dk = NULL, *db = NULL;
        ok = spec_layer(env, &s, l, &dk, &db);
        if (ok) { j->kernel[l] = dup_bytes(dk, (size_t)s.units[l] * (size_t)s.units[l + 1] * sizeof(float)); j->bias[l] = dup_bytes(db,
            (size_t)s.units[l + 1] * sizeof(float)); ok = j->kernel[l] && j->bias[l]; }
    }
    if (!ok) {
        train_job_release(env, j);
        fail_usage(env, "train: kernels[i] must be a Float32Array of units[i] x units[i+1], biases[i] one of units[i+1]"); return NULL;
    }
    if (r.fb) { j->db = fdb_of(r.fb); j->rows = dup_bytes(r.rows, r.nr * sizeof(uint32_t)); }
    else j->feat = dup_bytes(r.feat, r.nf * sizeof(double));
    j->history = calloc((size_t)j->epochs * 4, sizeof(double));
    if (r.values) { j->values = dup_bytes(r.values, r.ny * sizeof(double)); j->out_min = r.out_min; j->out_max = r.out_max; }
    else j->y = dup_bytes(r.y, r.ny * sizeof(int32_t));
    if (r.orders) j->orders = dup_bytes(r.orders, r.no * sizeof(uint32_t));
    if ((r.fb ? !j->rows : !j->feat) || (r.values ? !j->values : !j->y) || !j->history || (r.orders && !j->orders)) {
        train_job_release(env, j); fail_oom(env); return NULL;
    }
    napi_valuetype ft = napi_undefined;
    if (argc > 3 && napi_typeof(env, argv[3], &ft) == napi_ok && ft == napi_function && napi_create_reference(env, argv[3], 1,
        &j->on_epoch) != napi_ok) j->on_epoch = NULL;
    return j;
}
/* a promise and the thread-safe function `call_js` that will settle it; NULL (nothing thrown) when either cannot be made */
static napi_value train_promise(napi_env env, const char *what, napi_threadsafe_function_call_js call_js, napi_deferred *deferred,
    napi_threadsafe_function *tsfn) {
    napi_value promise, name;
    if (napi_create_promise(env, deferred, &promise) != napi_ok || napi_create_string_utf8(env, what, NAPI_AUTO_LENGTH, &name) != napi_ok ||
        napi_create_threadsafe_function(env, NULL, NULL, name, 0, 1, NULL, NULL, NULL, call_js, tsfn) != napi_ok) return NULL;
    return promise;
}
napi_value fn_train(napi_env env, napi_callback_info info) {
    ARGS(4);
    ctx_box *box = box_arg(env, argc, argv);
    if (!box || argc < 3) return fail_usage(env, TRAIN_USAGE);
    train_job *j = train_job_from(env, box, argc, argv);
    if (!j) return NULL;
    napi_value promise = train_promise(env, "wsa_train", train_call_js, &j->deferred, &j->tsfn);
    if (!promise) { train_job_release(env, j); return fail_error(env, "train: could not set up the job"); }
    box->children++;                                             /* until the run's last message: destroy() refuses meanwhile */
    if (pthread_create(&j->thread, NULL, train_thread, j) != 0) {
        box->children--; napi_release_threadsafe_function(j->tsfn, napi_tsfn_release);
        settle(env, j->deferred, "train: could not start a thread", NULL);
        train_job_release(env, j);
    }
    return promise;
}

// ---- training groups (wsa_train_group_*, K7g, specification TG-1): trainGroup(ctx, [[spec, run, onEpoch | undefined], ...]) -> Promise of an array with,
// per job and in job order, what train resolves to.  1 .. WSA_TRAIN_GROUP_MAX jobs, each with train's own arguments; classifiers and regression
// models mix.  All jobs' trainers step in lock step on one thread, one launch per stage for all of them; a job with fewer epochs leaves and the group
// is formed again from the rest, so every job's result equals its own train call bit for bit.  A job's onEpoch fires after each of ITS epochs.
typedef struct {
    ctx_box *box; napi_deferred deferred; napi_threadsafe_function tsfn; pthread_t thread;
    uint32_t n; train_job *job[WSA_TRAIN_GROUP_MAX];
    wsa_status st; char err[512];
} train_group_job;

static void train_group_release(napi_env env, train_group_job *g) {
    for (uint32_t i = 0; i < g->n; i++) train_job_release(env, g->job[i]);
    free(g);
}
/* one epoch of the jobs live[0 .. n_live) in lock step, their statistics delivered */
static wsa_status train_group_epoch(train_group_job *g, wsa_train_group *grp, const uint32_t *live, uint32_t n_live, uint32_t e) {
    const uint32_t *orders[WSA_TRAIN_GROUP_MAX];
    wsa_train_stats s[WSA_TRAIN_GROUP_MAX];
    for (uint32_t k = 0; k < n_live; k++) orders[k] = train_job_order(g->job[live[k]], e);
    wsa_status st = wsa_train_group_epoch(grp, orders, g->box->queue);
    if (st == WSA_OK) st = wsa_train_group_stats(grp, g->box->queue, s);
    for (uint32_t k = 0; st == WSA_OK && k < n_live; k++) train_job_epoch_done(g->job[live[k]], g, live[k], e, &s[k], g->tsfn);
    return st;
}
static void *train_group_thread(void *arg) {
    train_group_job *g = (train_group_job *)arg;
    wsa_ctx *ctx = g->box->ctx;
    wsa_trainer *t[WSA_TRAIN_GROUP_MAX] = {0};
    uint32_t longest = 0;
    g->st = WSA_OK;
    for (uint32_t i = 0; i < g->n && g->st == WSA_OK; i++) {
        g->st = train_job_trainer(ctx, g->job[i], &t[i]);
        if (g->job[i]->epochs > longest) longest = g->job[i]->epochs;
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
        g->st = train_group_epoch(g, grp, live, n_live, e);
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
    train_run_over(g, g->tsfn);
    return NULL;
}
static void train_group_call_js(napi_env env, napi_value js_cb, void *context, void *data) {
    train_msg *m = (train_msg *)data;
    train_group_job *g = (train_group_job *)m->run;
    const int32_t epoch = m->epoch; const uint32_t member = m->member; const wsa_train_stats s = m->s;
    free(m);
    if (!env) return;
    if (epoch >= 0) { train_on_epoch(env, g->job[member], epoch, &s); return; }
    pthread_join(g->thread, NULL);
    if (g->box->children) g->box->children--;
    if (g->st != WSA_OK) settle(env, g->deferred, g->err, NULL);
    else {
        napi_value out; napi_create_array_with_length(env, (size_t)g->n, &out);
        for (uint32_t i = 0; i < g->n; i++) napi_set_element(env, out, i, train_result(env, g->job[i]));
        settle(env, g->deferred, NULL, out);
    }
    napi_release_threadsafe_function(g->tsfn, napi_tsfn_release);
    train_group_release(env, g);
}
napi_value fn_train_group(napi_env env, napi_callback_info info) {
    ARGS(2);
    ctx_box *box = box_arg(env, argc, argv);
    const char *usage = "trainGroup(ctx, [[spec, run, onEpoch?], ...]): 1 .. 32 jobs, each with train's arguments";
    uint32_t n = 0;
    if (!box || argc < 2 || !array_arg(env, argv[1], &n) || n < 1 || n > WSA_TRAIN_GROUP_MAX) return fail_usage(env, usage);
    train_group_job *g = calloc(1, sizeof *g);
    if (!g) return fail_oom(env);
    g->box = box;
    for (uint32_t i = 0; i < n; i++) {
        napi_value item, a[4]; uint32_t len = 0;
        int ok = napi_get_element(env, argv[1], i, &item) == napi_ok && array_arg(env, item, &len) && len >= 2 && len <= 3;
        a[0] = argv[0];
        for (uint32_t k = 0; ok && k < len; k++) ok = napi_get_element(env, item, k, &a[k + 1]) == napi_ok;
        if (!ok) { train_group_release(env, g); return fail_usage(env, usage); }
        train_job *j = train_job_from(env, box, (size_t)len + 1, a);
        if (!j) { train_group_release(env, g); return NULL; }
        g->job[g->n++] = j;
    }
    napi_value promise = train_promise(env, "wsa_train_group", train_group_call_js, &g->deferred, &g->tsfn);
    if (!promise) { train_group_release(env, g); return fail_error(env, "trainGroup: could not set up the job"); }
    box->children++;                                             /* until the run's last message: destroy() refuses meanwhile */
    if (pthread_create(&g->thread, NULL, train_group_thread, g) != 0) {
        box->children--; napi_release_threadsafe_function(g->tsfn, napi_tsfn_release);
        settle(env, g->deferred, "trainGroup: could not start a thread", NULL);
        train_group_release(env, g);
    }
    return promise;
}

// ---- regressRows(ctx, model, features: Float64Array [n][the model's inputs], outMin, outMax) -> Float64Array [n]: a regression model's values
// (wsa_regress_rows).
// What the app's predict_db_nn does over stored rows (ref src/neuralmodel.js:410-535).  Synchronous: the rows go through one page-locked
// allocation the device reads and writes in place.
napi_value fn_regress_rows(napi_env env, napi_callback_info info) {
    ARGS(5);
    ctx_box *box = box_arg(env, argc, argv);
    const char *usage = "regressRows(ctx, model, features: Float64Array [n][the model's inputs], outMin, outMax)";
    size_t nf = 0; void *feat = NULL; double lo = 0, hi = 0; model_box *mb = NULL;
    if (!box || argc < 5 || !(mb = (model_box *)external_of(env, argv[1])) || !typed_arg(env, argv[2], napi_float64_array, &feat, &nf) ||
        napi_get_value_double(env, argv[3], &lo) != napi_ok || napi_get_value_double(env, argv[4], &hi) != napi_ok) return fail_usage(env, usage);
    if (!child_is(&mb->link, box)) return fail_error(env, "regressRows: the model was destroyed or belongs to another context");
    if (nf % mb->n_inputs || nf / mb->n_inputs > 0xffffffffu) return fail_usage(env, usage);
    const size_t n = nf / mb->n_inputs;
    void *slab = NULL;
    if (wsa_host_alloc(box->ctx, (uint64_t)(nf + n) * sizeof(double), &slab) != WSA_OK) return fail_lib(env, box->ctx);
    double *rows = (double *)slab, *value = rows + nf;
    if (nf) memcpy(rows, feat, nf * sizeof(double));
    wsa_status st = wsa_regress_rows(model_of(mb), lo, hi, rows, (uint32_t)n, value, box->queue);
    if (st == WSA_OK) st = wsa_queue_synchronize(box->ctx, box->queue);
    napi_value out = st == WSA_OK ? make_typed(env, napi_float64_array, value, n) : fail_lib(env, box->ctx);
    wsa_host_free(slab);
    return out;
}
