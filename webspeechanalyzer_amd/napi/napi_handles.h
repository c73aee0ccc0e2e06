// napi_handles.h — what JavaScript holds for the library's objects: boxes that outlive them, so that a handle used after its object's destroy (or
// destroyed twice) finds NULL instead of freed memory.
#ifndef WSA_NAPI_HANDLES_H
#define WSA_NAPI_HANDLES_H
#include "napi_util.h"

typedef struct ctx_box ctx_box;
// What the three child kinds of a context (model, KNN store, device feature DB) share, as their first member: the library's object (NULL once destroyed),
// the context's box, and the link of the context's list of that kind.  destroy() destroys the children with their context.
typedef struct child_box { void *obj; ctx_box *owner; struct child_box *next; } child_box;
// a model (wsa_model): `busy` counts the jobs and streams that classify with it (modelDestroy() refuses meanwhile); n_inputs: units[0], the width of the
// rows the model takes (53, 264 or 23)
typedef struct model_box { child_box link; uint32_t busy, n_classes, n_inputs; } model_box;
/* a KNN store (wsa_knn): every call on a store is synchronous, so it is never busy */
typedef struct knn_box { child_box link; uint32_t width, n_classes; } knn_box;
/* a device feature DB (wsa_featdb): every call on a DB is synchronous but train, which counts as a child of the context */
typedef struct fdb_box { child_box link; uint32_t width; } fdb_box;
static inline wsa_model *model_of(const model_box *mb) { return (wsa_model *)mb->link.obj; }
static inline wsa_knn *knn_of(const knn_box *kb) { return (wsa_knn *)kb->link.obj; }
static inline wsa_featdb *fdb_of(const fdb_box *fb) { return (wsa_featdb *)fb->link.obj; }

// What JS holds for a context: the box counts the batches in flight, the training runs and the open streams created from the context — destroy() refuses
// while any of them is alive (their wsa_batch / wsa_stream objects point into the context).
struct ctx_box {
    wsa_ctx *ctx; uint32_t children;
    // the planned batch of the last processBatch call: a call with the same clip lengths and rates reuses it (planning a 1024-clip
    // batch allocates GBs of work space: ~3 ms and more); taken out of the box while a job uses it, dropped by destroy()
    /* plan_fs_each: one rate per clip (wsa_batch_create_mixed), else NULL */
    wsa_batch *plan; uint32_t plan_n; uint32_t *plan_ns; double plan_fs, plan_fs_out; double *plan_fs_each;
    // the context's own HIP stream (wsa_queue_create, made by the first processBatch): every job of the context runs on it, so that the jobs of TWO
    // contexts on one device overlap — the upload of one batch under the kernels of the other — instead of queueing on the device's null stream
    void *queue;
    child_box *models, *knns, *fdbs;      /* the children created on this context (modelCreate, knnCreate, featdbCreate) */
    // the ensemble of the last processBatch call that had one (wsa_ensemble_create over ens_models): a call with the same list reuses it, so the
    // kept plan keeps its ensemble tables too; made and replaced by the job (one job at a time uses a context), dropped by destroy()
    wsa_ensemble *ens; model_box *ens_models[WSA_ENSEMBLE_MAX]; uint32_t ens_n;
    // the regression group of the last batchRegressGroup call (wsa_regress_group_create over reg_models and their ranges): a call with the same models
    // and ranges reuses it, so the kept plan keeps its group tables and allocates nothing; replaced by the next other list, dropped by destroy()
    wsa_regress_group *reg; model_box *reg_models[WSA_REGRESS_GROUP_MAX]; double reg_lo[WSA_REGRESS_GROUP_MAX], reg_hi[WSA_REGRESS_GROUP_MAX]; uint32_t reg_n;
};
void box_drop_plan(ctx_box *b);
void box_drop_ensemble(ctx_box *b);
void box_drop_regress(ctx_box *b);

/* ---- readers */
static inline ctx_box *get_box(napi_env env, napi_value v) { return (ctx_box *)external_of(env, v); }
ctx_box *box_arg(napi_env env, size_t argc, const napi_value *argv);        /* argv[0] as the box of a live context, else NULL (nothing thrown) */
wsa_ctx *ctx_arg(napi_env env, size_t argc, const napi_value *argv);        /* ... its context */
/* a child handle: is its object alive and of the context `owner`? */
static inline int child_is(const child_box *c, const ctx_box *owner) { return c->obj && c->owner == owner; }
// the live child of context `owner` behind a JS value, or NULL with an Error pending: `dead` for a value that is no handle or whose object is gone,
// `foreign` for one of another context
child_box *child_arg(napi_env env, napi_value v, const ctx_box *owner, const char *dead, const char *foreign);
#define model_arg(env, v, owner, dead, foreign) ((model_box *)child_arg(env, v, owner, dead, foreign))
#define knn_arg(env, v, owner, dead, foreign) ((knn_box *)child_arg(env, v, owner, dead, foreign))
#define fdb_arg(env, v, owner, dead, foreign) ((fdb_box *)child_arg(env, v, owner, dead, foreign))
/* an array of 1 .. max live models of context `owner` into mbs[] and ms[]: their count, or 0 with an Error pending (`count` for a wrong length) */
uint32_t model_list_arg(napi_env env, napi_value arr, const ctx_box *owner, uint32_t max, model_box **mbs, const wsa_model **ms,
                        const char *count, const char *dead, const char *foreign);

// a regression group's arguments ([models]: 1 .. 8 regression models of context `box`, outMin / outMax: Float64Arrays with one range per model) for the
// export `who`: 1, or 0 with an exception pending.  The library refuses whatever is not a regression model of 53 inputs.
int regress_group_arg(napi_env env, const char *who, napi_value arr, napi_value lo, napi_value hi, ctx_box *box, model_box **mbs, const wsa_model **ms,
                      const double **out_min, const double **out_max, uint32_t *n);
/* the live device DB of a handle with its context idle, or NULL with an exception pending (`usage` as a TypeError for a value that is no handle) */
fdb_box *fdb_idle(napi_env env, napi_value v, const char *usage);

// ---- making and unmaking a child: a new box of `size` bytes at the head of its context's list (NULL: out of memory; the caller fills what follows the
// link), the JS external over it, and the box out of the list when its object is gone
child_box *child_new(size_t size, void *obj, ctx_box *owner, child_box **list);
napi_value child_handle(napi_env env, child_box *c);
void child_unlink(child_box *c, child_box **list);

/* napi_batch.c: the communicator of gatherRows goes before any of its contexts (destroy) */
void gather_forget(wsa_ctx *ctx);

#endif
