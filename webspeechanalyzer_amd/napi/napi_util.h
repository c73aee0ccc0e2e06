// napi_util.h — the plumbing every fn_* of the addon is written in: take the arguments, read typed arrays and numbers, throw, write result tables.
// No C-ABI call but wsa_last_error (fail_lib).  An fn_* body reads: take arguments, refuse, call the library, emit tables.
#ifndef WSA_NAPI_UTIL_H
#define WSA_NAPI_UTIL_H
#include <node_api.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "../../include/wsa.h"

#define NAPI_OK(env, call) do { if ((call) != napi_ok) { napi_throw_error((env), NULL, "N-API call failed: " #call); return NULL; } } while (0)

/* ---- arguments: ARGS(n) at the head of an fn_* declares argc (at most n) and argv[n] */
#define ARGS(n) size_t argc = (n); napi_value argv[(n)]; NAPI_OK(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL))

#define OR1(x) ((x) ? (x) : 1)                       /* a table of no entries is still allocated, and copied with room for one */

int is_nullish(napi_env env, napi_value v);          /* undefined or null */
void *external_of(napi_env env, napi_value v);       /* the pointer of an external (a handle), NULL for anything else */

// ---- typed arrays.  typed_info: any kind; typed_arg: of kind `want`; typed_arg_n: of kind `want` and length n; typed_of: typed_arg of the property `name`;
// typed_opt: 0 for a value that is no typed array (*data stays NULL), 1 for one of kind `want` and length n, -1 for any other typed array
int typed_info(napi_env env, napi_value v, napi_typedarray_type *type, void **data, size_t *len);
int typed_arg(napi_env env, napi_value v, napi_typedarray_type want, void **data, size_t *len);
int typed_arg_n(napi_env env, napi_value v, napi_typedarray_type want, size_t n, void **data);
int typed_of(napi_env env, napi_value o, const char *name, napi_typedarray_type want, void **data, size_t *len);
int typed_opt(napi_env env, napi_value v, napi_typedarray_type want, size_t n, void **data);
int num_of(napi_env env, napi_value o, const char *name, double *out);      /* the number property `name` */
int array_arg(napi_env env, napi_value v, uint32_t *n);                      /* a JS array and its length */
void *dup_bytes(const void *p, size_t bytes);

/* ---- throws: each leaves the exception pending and returns NULL, so `return fail_*(...)` ends an fn_* */
napi_value fail_usage(napi_env env, const char *text);      /* TypeError */
napi_value fail_error(napi_env env, const char *text);      /* Error */
napi_value fail_lib(napi_env env, wsa_ctx *ctx);            /* Error with the library's last message */
napi_value fail_oom(napi_env env);
/* how a job's promise settles: rejected with the string `err` (the reference rejects with strings, ref @B4554), else resolved with `value` */
void settle(napi_env env, napi_deferred deferred, const char *err, napi_value value);

// ---- result writers: a typed array owns a copy of `count` elements of `src`; the element size follows from `kind`.  put_* return 1 when the property
// is set
napi_value make_typed(napi_env env, napi_typedarray_type kind, const void *src, size_t count);
napi_value new_object(napi_env env);
int put(napi_env env, napi_value o, const char *name, napi_value v);
int put_typed(napi_env env, napi_value o, const char *name, napi_typedarray_type kind, const void *src, size_t count);
int put_u32(napi_env env, napi_value o, const char *name, uint32_t v);
/* H tables of `count` doubles as one Float64Array [H][count] */
int put_heads(napi_env env, napi_value o, const char *name, const double *const *src, uint32_t H, size_t count);

/* ---- the tables batches and streams both emit */
void put_rows(napi_env env, napi_value o, const int32_t *meta, const double *feat, size_t n_rows);                         /* meta [n][8], feat [n][53] */
/* uttMeta [n][4], uttFeat [n][264] */
void put_utterance(napi_env env, napi_value o, const int32_t *meta, const double *feat, size_t n);
// trackOff (the offsets as doubles, exact below 2^53: [n_segments + 1][2] = first point / first ranked id of a segment), trackPoints [np][8],
// trackRanked [nr]
void put_tracks(napi_env env, napi_value o, const uint64_t *off, size_t n_segments, const int32_t *points, size_t np, const int32_t *ranked, size_t nr);
/* a classifier's tables: prob [rows][classes], and with a fold cb [n][4], cbLabel, cbConf [n] and `unit_name` [units][classes] (clipConf / streamConf) */
typedef struct {
    uint32_t n_classes; size_t n_rows, n_cb, n_units; int fold; const char *unit_name;
    const float *prob; const int32_t *cb, *cb_label; const double *cb_conf, *unit_conf;
} class_view;
void put_classes(napi_env env, napi_value o, const class_view *v);
// the ensemble tables as a JS object: {nMembers, nClasses, prob[], cbLabel[], cbConf[], cbAllMax[], conf[] (Label_conf_all per clip / stream),
// cb, cbDb, cbTopLabel, cbTopConf, cbMinDb, cbEntropy, minDb (per clip / stream)}; fold = 0 (level 5): nMembers, nClasses and prob only
typedef struct {
    uint32_t n, n_rows, n_cb, n_units; const uint32_t *n_classes; int fold;
    const float *const *prob; const int32_t *const *cb_label; const double *const *cb_conf; const double *const *cb_all_max; const double *const *conf;
    const int32_t *cb, *cb_db, *cb_top_label, *cb_min_db, *min_db; const double *cb_top_conf, *cb_entropy;
} ens_view;
napi_value ens_object(napi_env env, const ens_view *v);
// the four KNN tables of n rows in one allocation, laid out [label n][nbr n k][sim n k][conf n C] (conf 8-aligned) with 8 spare bytes; knn_object:
// {label: Int32Array [n], nbr: Int32Array [n][k], sim: Float32Array [n][k], conf: Float64Array [n][C], k, kEff, nClasses} (knnClassify, batchKnn)
typedef struct { int32_t *label, *nbr; float *sim; double *conf; } knn_slab;
size_t knn_slab_bytes(size_t n, uint32_t k, uint32_t C);
knn_slab knn_slab_at(void *base, size_t n, uint32_t k);
napi_value knn_object(napi_env env, const knn_slab *t, size_t n, uint32_t k, uint32_t k_eff, uint32_t C);

#endif
