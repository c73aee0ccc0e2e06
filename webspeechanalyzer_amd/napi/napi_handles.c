/* napi_handles.c — the boxes behind JS handles (napi_handles.h), the context's own exports and the page-locked buffers. */
#include "napi_handles.h"

/* ---- the children of a context */
child_box *child_arg(napi_env env, napi_value v, const ctx_box *owner, const char *dead, const char *foreign) {
    child_box *c = (child_box *)external_of(env, v);
    if (!c || !c->obj) { fail_error(env, dead); return NULL; }
    if (c->owner != owner) { fail_error(env, foreign); return NULL; }
    return c;
}
uint32_t model_list_arg(napi_env env, napi_value arr, const ctx_box *owner, uint32_t max, model_box **mbs, const wsa_model **ms,
                        const char *count, const char *dead, const char *foreign) {
    uint32_t n = 0;
    if (!array_arg(env, arr, &n) || n < 1 || n > max) { fail_error(env, count); return 0; }
    for (uint32_t d = 0; d < n; d++) {
        napi_value el;
        if (napi_get_element(env, arr, d, &el) != napi_ok) { fail_error(env, dead); return 0; }
        if (!(mbs[d] = model_arg(env, el, owner, dead, foreign))) return 0;
        if (ms) ms[d] = model_of(mbs[d]);
    }
    return n;
}
int regress_group_arg(napi_env env, const char *who, napi_value arr, napi_value lo, napi_value hi, ctx_box *box, model_box **mbs, const wsa_model **ms,
                      const double **out_min, const double **out_max, uint32_t *n) {
    char count[160], dead[160], foreign[160], msg[160];
    snprintf(count, sizeof count, "%s: a regression group has 1 .. 8 models", who);
    snprintf(dead, sizeof dead, "%s: a model handle was destroyed (or is not a model)", who);
    snprintf(foreign, sizeof foreign, "%s: a model belongs to another context", who);
    if (!(*n = model_list_arg(env, arr, box, WSA_REGRESS_GROUP_MAX, mbs, ms, count, dead, foreign))) return 0;
    if (!typed_arg_n(env, lo, napi_float64_array, *n, (void **)out_min) || !typed_arg_n(env, hi, napi_float64_array, *n, (void **)out_max)) {
        snprintf(msg, sizeof msg, "%s: outMin and outMax are Float64Arrays with one entry per model", who); fail_usage(env, msg); return 0;
    }
    return 1;
}
fdb_box *fdb_idle(napi_env env, napi_value v, const char *usage) {
    fdb_box *fb = (fdb_box *)external_of(env, v);
    if (!fb) { fail_usage(env, usage); return NULL; }
    if (!fb->link.obj || !fb->link.owner || !fb->link.owner->ctx) { fail_error(env, "the device DB was destroyed"); return NULL; }
    if (fb->link.owner->children) { fail_error(env, "the device DB's context has a batch or a training run in flight"); return NULL; }
    return fb;
}
static void child_finalize(napi_env env, void *data, void *hint) {          /* the JS handle is gone */
    child_box *c = (child_box *)data;
    if (!c->obj && !c->owner) free(c);               /* a live object stays (explicit destroy only, as contexts) */
}
child_box *child_new(size_t size, void *obj, ctx_box *owner, child_box **list) {
    child_box *c = calloc(1, size);
    if (c) { c->obj = obj; c->owner = owner; c->next = *list; *list = c; }
    return c;
}
napi_value child_handle(napi_env env, child_box *c) {
    napi_value ext; NAPI_OK(env, napi_create_external(env, c, child_finalize, NULL, &ext));
    return ext;
}
void child_unlink(child_box *c, child_box **list) {
    if (c->owner) for (child_box **q = list; *q; q = &(*q)->next) if (*q == c) { *q = c->next; break; }
    c->owner = NULL; c->next = NULL;
}
static void destroy_model(void *m) { wsa_model_destroy((wsa_model *)m); }
static void destroy_knn(void *k) { wsa_knn_destroy((wsa_knn *)k); }
static void destroy_fdb(void *db) { wsa_featdb_destroy((wsa_featdb *)db); }
static void children_destroy(child_box **list, void (*destroy)(void *)) {          /* children go before their context */
    while (*list) { child_box *c = *list; destroy(c->obj); c->obj = NULL; child_unlink(c, list); }
}

/* ---- the context's box */
void box_drop_ensemble(ctx_box *b) {
    if (b->ens) wsa_ensemble_destroy(b->ens);
    b->ens = NULL; b->ens_n = 0;
}
void box_drop_regress(ctx_box *b) {
    if (b->reg) wsa_regress_group_destroy(b->reg);
    b->reg = NULL; b->reg_n = 0;
}
void box_drop_plan(ctx_box *b) {
    if (b->plan) wsa_batch_destroy(b->plan);
    free(b->plan_ns); free(b->plan_fs_each); b->plan = NULL; b->plan_ns = NULL; b->plan_fs_each = NULL; b->plan_n = 0;
}
ctx_box *box_arg(napi_env env, size_t argc, const napi_value *argv) {
    ctx_box *b = argc ? get_box(env, argv[0]) : NULL;
    return b && b->ctx ? b : NULL;
}
wsa_ctx *ctx_arg(napi_env env, size_t argc, const napi_value *argv) {        /* NULL once destroy() has run */
    ctx_box *b = box_arg(env, argc, argv);
    return b ? b->ctx : NULL;
}
static void ctx_finalize(napi_env env, void *data, void *hint) {          /* the JS handle is gone */
    ctx_box *b = (ctx_box *)data;
    /* a context nobody destroyed stays (explicit destroy() only: the finalizer may run at process exit, after the HIP runtime) */
    if (!b->ctx && b->children == 0) free(b);
}

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

/* abiVersion() -> number: the wsa_abi_version of the libwsa.so that is loaded */
napi_value fn_abi_version(napi_env env, napi_callback_info info) {
    napi_value v; NAPI_OK(env, napi_create_int32(env, wsa_abi_version(), &v)); return v;
}
/* defaults() -> config object (wsa_config_default, ref @B2965) */
napi_value fn_defaults(napi_env env, napi_callback_info info) {
    wsa_config c; wsa_config_default(&c); return config_to_js(env, &c);
}
/* create(config, device) -> external ctx (wsa_create) */
napi_value fn_create(napi_env env, napi_callback_info info) {
    ARGS(2);
    wsa_config c; int32_t device = 0;
    if (argc < 1 || !js_to_config(env, argv[0], &c)) return fail_usage(env, "create(config, device)");
    if (argc > 1) napi_get_value_int32(env, argv[1], &device);
    wsa_ctx *ctx = NULL;
    if (wsa_create(&c, device, &ctx) != WSA_OK) return fail_lib(env, NULL);
    ctx_box *box = calloc(1, sizeof *box);
    box->ctx = ctx;
    napi_value ext; NAPI_OK(env, napi_create_external(env, box, ctx_finalize, NULL, &ext));
    return ext;
}
// destroy(ctx): refused while the context has batches in flight, training runs or open streams; what the box kept goes first, in this order: plan,
// ensemble (before its models), regress group, models, KNN stores, feature DBs, queue, context.  A second destroy() is a no-op.
napi_value fn_destroy(napi_env env, napi_callback_info info) {
    ARGS(1);
    ctx_box *b = box_arg(env, argc, argv);
    if (!b) return NULL;
    if (b->children) return fail_error(env, "context still has batches in flight or open streams");
    gather_forget(b->ctx);
    box_drop_plan(b);
    box_drop_ensemble(b);
    box_drop_regress(b);
    children_destroy(&b->models, destroy_model);
    children_destroy(&b->knns, destroy_knn);
    children_destroy(&b->fdbs, destroy_fdb);
    if (b->queue) { wsa_queue_destroy(b->ctx, b->queue); b->queue = NULL; }
    wsa_destroy(b->ctx); b->ctx = NULL;
    return NULL;
}
/* geometry(ctx, fs) -> {nfft, win, hop, bands, kmax} (wsa_geometry_for) */
napi_value fn_geometry(napi_env env, napi_callback_info info) {
    ARGS(2); double fs = 0;
    wsa_ctx *ctx = ctx_arg(env, argc, argv);
    if (!ctx || argc < 2 || napi_get_value_double(env, argv[1], &fs) != napi_ok) return fail_usage(env, "geometry(ctx, fs)");
    wsa_geometry g;
    if (wsa_geometry_for(ctx, fs, &g) != WSA_OK) return fail_lib(env, ctx);
    napi_value o, v; NAPI_OK(env, napi_create_object(env, &o));
    const char *names[5] = {"nfft", "win", "hop", "bands", "kmax"}; const int32_t vals[5] = {g.nfft, g.win, g.hop, g.bands, g.kmax};
    for (int i = 0; i < 5; i++) { NAPI_OK(env, napi_create_int32(env, vals[i], &v)); NAPI_OK(env, napi_set_named_property(env, o, names[i], v)); }
    return o;
}
/* binsHz(ctx, fs) -> Float64Array (wsa_bins_hz, ref @B8380) */
napi_value fn_bins_hz(napi_env env, napi_callback_info info) {
    ARGS(2); double fs = 0;
    wsa_ctx *ctx = ctx_arg(env, argc, argv);
    if (!ctx || argc < 2 || napi_get_value_double(env, argv[1], &fs) != napi_ok) return fail_usage(env, "binsHz(ctx, fs)");
    wsa_geometry g;
    if (wsa_geometry_for(ctx, fs, &g) != WSA_OK) return fail_lib(env, ctx);
    napi_value ab, ta; void *data = NULL;
    NAPI_OK(env, napi_create_arraybuffer(env, sizeof(double) * (size_t)g.bands, &data, &ab));
    if (wsa_bins_hz(ctx, fs, (double *)data, g.bands) != WSA_OK) return fail_lib(env, ctx);
    NAPI_OK(env, napi_create_typedarray(env, napi_float64_array, (size_t)g.bands, ab, 0, &ta));
    return ta;
}

// ---- page-locked buffers.  Every buffer handed to JS has a record: freePinned(ab) releases the memory at a moment of the caller's choosing (hipHostFree
// synchronises the device: inside the garbage collector's finalizer that stall hits the event loop whenever V8 decides) and detaches the ArrayBuffer; the
// finalizer then finds nothing left to do
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
// allocPinned(ctx, bytes) -> ArrayBuffer over page-locked host memory (wsa_host_alloc): clips read into views of it reach the device by DMA at the
// link's rate instead of through the runtime's staging copies.  The memory is released when the ArrayBuffer is collected.
napi_value fn_alloc_pinned(napi_env env, napi_callback_info info) {
    ARGS(2); double bytes = 0;
    wsa_ctx *ctx = ctx_arg(env, argc, argv);
    if (!ctx || argc < 2 || napi_get_value_double(env, argv[1], &bytes) != napi_ok || bytes < 0 || bytes > 68719476736.0)
        return fail_usage(env, "allocPinned(ctx, bytes)");
    void *p = NULL;
    if (wsa_host_alloc(ctx, (uint64_t)bytes, &p) != WSA_OK) return fail_lib(env, ctx);
    pinned_rec *r = calloc(1, sizeof *r);
    if (!r) { wsa_host_free(p); return fail_oom(env); }
    r->p = p; r->bytes = (uint64_t)bytes;
    napi_value ab;
    if (napi_create_external_arraybuffer(env, p, (size_t)bytes, pinned_finalize, r, &ab) != napi_ok) {
        wsa_host_free(p); free(r); return fail_error(env, "napi_create_external_arraybuffer failed");
    }
    r->next = g_pinned; g_pinned = r;
    { int64_t now = 0; napi_adjust_external_memory(env, (int64_t)bytes, &now); }
    return ab;
}
// freePinned(ab): the page-locked memory behind an ArrayBuffer of allocPinned goes back NOW (no run may still be reading it) and the ArrayBuffer is detached:
// views on it have length 0 from here on.  Returns true when it was such a buffer and still allocated.
napi_value fn_free_pinned(napi_env env, napi_callback_info info) {
    ARGS(1); void *data = NULL; size_t len = 0; bool is_ab = false;
    if (argc < 1 || napi_is_arraybuffer(env, argv[0], &is_ab) != napi_ok || !is_ab || napi_get_arraybuffer_info(env, argv[0], &data, &len) != napi_ok)
        return fail_usage(env, "freePinned(arrayBuffer)");
    bool done = false;
    for (pinned_rec *r = g_pinned; r; r = r->next) if (r->p == data && !r->freed) { pinned_release(env, r); done = true; break; }
    if (done) (void)napi_detach_arraybuffer(env, argv[0]);
    napi_value v; NAPI_OK(env, napi_get_boolean(env, done, &v)); return v;
}
