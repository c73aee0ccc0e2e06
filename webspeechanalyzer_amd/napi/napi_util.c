/* napi_util.c — the addon's plumbing (napi_util.h): argument readers, throws, result writers and the tables batches and streams share. */
#include "napi_util.h"

int is_nullish(napi_env env, napi_value v) {
    napi_valuetype t = napi_undefined;
    napi_typeof(env, v, &t);
    return t == napi_undefined || t == napi_null;
}
void *external_of(napi_env env, napi_value v) {
    void *p = NULL; if (napi_get_value_external(env, v, &p) != napi_ok) return NULL; return p;
}

int typed_info(napi_env env, napi_value v, napi_typedarray_type *type, void **data, size_t *len) {
    bool ta = false;
    if (napi_is_typedarray(env, v, &ta) != napi_ok || !ta) return 0;
    return napi_get_typedarray_info(env, v, type, len, data, NULL, NULL) == napi_ok;
}
int typed_arg(napi_env env, napi_value v, napi_typedarray_type want, void **data, size_t *len) {
    napi_typedarray_type t;
    return typed_info(env, v, &t, data, len) && t == want;
}
int typed_arg_n(napi_env env, napi_value v, napi_typedarray_type want, size_t n, void **data) {
    size_t len = 0;
    return typed_arg(env, v, want, data, &len) && len == n;
}
int typed_of(napi_env env, napi_value o, const char *name, napi_typedarray_type want, void **data, size_t *len) {
    napi_value v;
    return napi_get_named_property(env, o, name, &v) == napi_ok && typed_arg(env, v, want, data, len);
}
int typed_opt(napi_env env, napi_value v, napi_typedarray_type want, size_t n, void **data) {
    bool ta = false; void *p = NULL;
    if (napi_is_typedarray(env, v, &ta) != napi_ok || !ta) return 0;
    if (!typed_arg_n(env, v, want, n, &p)) return -1;
    *data = p;
    return 1;
}
int num_of(napi_env env, napi_value o, const char *name, double *out) {
    napi_value v; napi_valuetype t;
    return napi_get_named_property(env, o, name, &v) == napi_ok && napi_typeof(env, v, &t) == napi_ok && t == napi_number && napi_get_value_double(env, v,
        out) == napi_ok;
}
int array_arg(napi_env env, napi_value v, uint32_t *n) {
    bool is_arr = false;
    return napi_is_array(env, v, &is_arr) == napi_ok && is_arr && napi_get_array_length(env, v, n) == napi_ok;
}
void *dup_bytes(const void *p, size_t bytes) { void *q = malloc(bytes ? bytes : 1); if (q && bytes) memcpy(q, p, bytes); return q; }

napi_value fail_usage(napi_env env, const char *text) { napi_throw_type_error(env, NULL, text); return NULL; }
napi_value fail_error(napi_env env, const char *text) { napi_throw_error(env, NULL, text); return NULL; }
napi_value fail_lib(napi_env env, wsa_ctx *ctx) { napi_throw_error(env, NULL, wsa_last_error(ctx)); return NULL; }
napi_value fail_oom(napi_env env) { napi_throw_error(env, NULL, "out of memory"); return NULL; }
void settle(napi_env env, napi_deferred deferred, const char *err, napi_value value) {
    if (!err) { napi_resolve_deferred(env, deferred, value); return; }
    napi_value msg;
    napi_create_string_utf8(env, err, NAPI_AUTO_LENGTH, &msg);
    napi_reject_deferred(env, deferred, msg);
}

static size_t elt_of(napi_typedarray_type kind) {
    switch (kind) {
        case napi_int8_array: case napi_uint8_array: case napi_uint8_clamped_array: return 1;
        case napi_int16_array: case napi_uint16_array: return 2;
        case napi_int32_array: case napi_uint32_array: case napi_float32_array: return 4;
        default: return 8;
    }
}
napi_value make_typed(napi_env env, napi_typedarray_type kind, const void *src, size_t count) {
    napi_value ab, ta; void *data = NULL; const size_t elt = elt_of(kind);
    if (napi_create_arraybuffer(env, count * elt, &data, &ab) != napi_ok) return NULL;
    if (count) memcpy(data, src, count * elt);
    if (napi_create_typedarray(env, kind, count, ab, 0, &ta) != napi_ok) return NULL;
    return ta;
}
napi_value new_object(napi_env env) { napi_value o = NULL; napi_create_object(env, &o); return o; }
int put(napi_env env, napi_value o, const char *name, napi_value v) { return v && napi_set_named_property(env, o, name, v) == napi_ok; }
int put_typed(napi_env env, napi_value o, const char *name, napi_typedarray_type kind, const void *src, size_t count) {
    return put(env, o, name, make_typed(env, kind, src, count));
}
int put_u32(napi_env env, napi_value o, const char *name, uint32_t v) {
    napi_value n;
    return napi_create_uint32(env, v, &n) == napi_ok && put(env, o, name, n);
}
int put_heads(napi_env env, napi_value o, const char *name, const double *const *src, uint32_t H, size_t count) {
    napi_value ab, ta; void *data = NULL;
    if (napi_create_arraybuffer(env, (size_t)H * count * 8, &data, &ab) != napi_ok) return 0;
    for (uint32_t h = 0; count && h < H; h++) memcpy((double *)data + (size_t)h * count, src[h], count * 8);
    if (napi_create_typedarray(env, napi_float64_array, (size_t)H * count, ab, 0, &ta) != napi_ok) return 0;
    return put(env, o, name, ta);
}

void put_rows(napi_env env, napi_value o, const int32_t *meta, const double *feat, size_t n_rows) {
    put_typed(env, o, "meta", napi_int32_array, meta, n_rows * 8);
    put_typed(env, o, "feat", napi_float64_array, feat, n_rows * WSA_NFEAT);
}
void put_utterance(napi_env env, napi_value o, const int32_t *meta, const double *feat, size_t n) {
    put_typed(env, o, "uttMeta", napi_int32_array, meta, n * 4);
    put_typed(env, o, "uttFeat", napi_float64_array, feat, n * WSA_NUTT);
}
void put_tracks(napi_env env, napi_value o, const uint64_t *off, size_t n_segments, const int32_t *points, size_t np, const int32_t *ranked, size_t nr) {
    const size_t n = 2 * (n_segments + 1);
    double *od = malloc(sizeof(double) * n);
    for (size_t i = 0; i < n; i++) od[i] = (double)off[i];
    put_typed(env, o, "trackOff", napi_float64_array, od, n);
    free(od);
    put_typed(env, o, "trackPoints", napi_int32_array, points, np * 8);
    put_typed(env, o, "trackRanked", napi_int32_array, ranked, nr);
}
void put_classes(napi_env env, napi_value o, const class_view *v) {
    put_typed(env, o, "prob", napi_float32_array, v->prob, v->n_rows * v->n_classes);
    if (!v->fold) return;
    put_typed(env, o, "cb", napi_int32_array, v->cb, v->n_cb * 4);
    put_typed(env, o, "cbLabel", napi_int32_array, v->cb_label, v->n_cb);
    put_typed(env, o, "cbConf", napi_float64_array, v->cb_conf, v->n_cb);
    put_typed(env, o, v->unit_name, napi_float64_array, v->unit_conf, v->n_units * v->n_classes);
}
napi_value ens_object(napi_env env, const ens_view *v) {
    napi_value o = new_object(env), a_prob, a_lab, a_conf, a_max, a_acc;
    put_u32(env, o, "nMembers", v->n);
    put_typed(env, o, "nClasses", napi_uint32_array, v->n_classes, v->n);
    napi_create_array_with_length(env, v->n, &a_prob); napi_create_array_with_length(env, v->n, &a_lab); napi_create_array_with_length(env, v->n, &a_conf);
    napi_create_array_with_length(env, v->n, &a_max); napi_create_array_with_length(env, v->n, &a_acc);
    for (uint32_t d = 0; d < v->n; d++) {
        napi_set_element(env, a_prob, d, make_typed(env, napi_float32_array, v->prob[d], (size_t)v->n_rows * v->n_classes[d]));
        if (!v->fold) continue;
        napi_set_element(env, a_lab, d, make_typed(env, napi_int32_array, v->cb_label[d], v->n_cb));
        napi_set_element(env, a_conf, d, make_typed(env, napi_float64_array, v->cb_conf[d], v->n_cb));
        napi_set_element(env, a_max, d, make_typed(env, napi_float64_array, v->cb_all_max[d], v->n_cb));
        napi_set_element(env, a_acc, d, make_typed(env, napi_float64_array, v->conf[d], (size_t)v->n_units * v->n_classes[d]));
    }
    put(env, o, "prob", a_prob);
    if (!v->fold) return o;
    put(env, o, "cbLabel", a_lab); put(env, o, "cbConf", a_conf); put(env, o, "cbAllMax", a_max); put(env, o, "conf", a_acc);
    put_typed(env, o, "cb", napi_int32_array, v->cb, (size_t)v->n_cb * 4);
    put_typed(env, o, "cbDb", napi_int32_array, v->cb_db, v->n_cb);
    put_typed(env, o, "cbTopLabel", napi_int32_array, v->cb_top_label, v->n_cb);
    put_typed(env, o, "cbTopConf", napi_float64_array, v->cb_top_conf, v->n_cb);
    put_typed(env, o, "cbMinDb", napi_int32_array, v->cb_min_db, v->n_cb);
    put_typed(env, o, "cbEntropy", napi_float64_array, v->cb_entropy, v->n_cb);
    put_typed(env, o, "minDb", napi_int32_array, v->min_db, v->n_units);
    return o;
}
size_t knn_slab_bytes(size_t n, uint32_t k, uint32_t C) { return ((n + 2 * n * k) * 4 + 7) / 8 * 8 + n * C * 8 + 8; }
knn_slab knn_slab_at(void *base, size_t n, uint32_t k) {
    knn_slab t;
    t.label = (int32_t *)base; t.nbr = t.label + n; t.sim = (float *)(t.nbr + n * k);
    t.conf = (double *)((char *)base + ((n + 2 * n * k) * 4 + 7) / 8 * 8);
    return t;
}
napi_value knn_object(napi_env env, const knn_slab *t, size_t n, uint32_t k, uint32_t k_eff, uint32_t C) {
    napi_value o = new_object(env);
    put_typed(env, o, "label", napi_int32_array, t->label, n);
    put_typed(env, o, "nbr", napi_int32_array, t->nbr, n * k);
    put_typed(env, o, "sim", napi_float32_array, t->sim, n * k);
    put_typed(env, o, "conf", napi_float64_array, t->conf, n * C);
    put_u32(env, o, "k", k); put_u32(env, o, "kEff", k_eff); put_u32(env, o, "nClasses", C);
    return o;
}
