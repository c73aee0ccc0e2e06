// knn_fold.hip — specification KN-2: the app's per-callback fold K6b (classify_fold.hpp) fed KNN confidences, for a batch
// (wsa_batch_knn_fold, one accumulator per clip) and inside a stream object's step (wsa_stream_set_knn: K9s on every step's rows, then the
// fold carried from step to step on the device, with the step's tables pushed to mapped pinned memory).  knn.hip owns the store and the
// K9 / K9s kernels; stream_step.hip captures these launches into the stream object's step.
//
// The fold sees, per row, the C pairs (class index, votes / k_eff as the f64 K9's epilogue writes).  The legend is the class indices
// themselves, so every label is an array-index key: Object.keys order is class order (key_rank[c] = c).
#include <cstring>
#include <string>
#include <vector>
#include "knn_internal.hpp"
#include "classify_internal.hpp"
#include "classify_fold.hpp"

using wsa_api::fail;
using namespace wsa_classify;
using namespace wsa_knn_detail;

namespace {

// key_rank of the class-index legend: [WSA_MODEL_MAX_CLASSES] = 0, 1, 2, ...
bool upload_index_legend(wsa::DevArena& A, int64_t** out) {
    std::vector<int64_t> iota(WSA_MODEL_MAX_CLASSES);
    for (int c = 0; c < WSA_MODEL_MAX_CLASSES; c++) iota[c] = c;
    return A.upload(out, iota);
}

}  // namespace

// ---- batches: KN-2 over the tables of the batch's last wsa_batch_knn
struct wsa_kfold {
    int device = 0;
    uint32_t cap_c = 0;
    int32_t *d_t_label = nullptr, *d_t_n = nullptr, *d_t_local = nullptr, *d_cb = nullptr, *d_cb_label = nullptr; int64_t* d_key_rank = nullptr;
    double *d_t_conf = nullptr, *d_cb_conf = nullptr, *d_clip_conf = nullptr;
    uint32_t *d_clip_cb = nullptr, *d_cb_off = nullptr;
    uint32_t *h_count = nullptr, *h_count_dev = nullptr;     // pinned + mapped: callbacks of the last fold
    wsa::DevArena mem;
};

void wsa_kfold_free(wsa_kfold* f) { free_on_device(f); }

namespace {

wsa_status enqueue_batch_fold(const wsa_batch_view& v, const wsa_kcls* c, hipStream_t s) {
    const wsa_kfold* f = c->fold;
    FoldParams<double> p{};
    p.n_clips = v.n_clips; p.C = (uint32_t)c->knn->C; p.step_s = v.ctx->cfg.window_step / 1e3;
    p.meta = v.d_meta; p.row_off = v.d_row_off; p.prob = c->d_conf; p.key_rank = f->d_key_rank;
    p.t_label = f->d_t_label; p.t_conf = f->d_t_conf; p.t_n = f->d_t_n; p.t_local = f->d_t_local;
    p.clip_cb = f->d_clip_cb; p.clip_conf = f->d_clip_conf;
    launch_fold(p, f->d_cb_off, f->d_cb, f->d_cb_label, f->d_cb_conf, f->h_count_dev, s);
    HIP_TRY(v.ctx, hipGetLastError());
    return WSA_OK;
}

}  // namespace

extern "C" {

wsa_status wsa_batch_knn_fold(wsa_batch* b, void* stream) {
    if (!b) return WSA_ERR_INVALID;
    wsa_batch_view v;
    wsa_batch_view_internal(b, &v);
    wsa_ctx* ctx = v.ctx;
    wsa_kcls* c = *v.kcls;
    if (!c || !c->knn) return fail(ctx, WSA_ERR_INVALID, "no wsa_batch_knn on this batch yet");
    if (v.level != 13 || c->level != 13)
        return fail(ctx, WSA_ERR_INVALID, "wsa_batch_knn_fold needs a batch at output_level 13 (syllable features: callbacks of several rows), not " + std::to_string(v.level));
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (!c->fold || c->fold->cap_c < (uint32_t)c->knn->C) {          // first call (or more classes): the only allocation of this path
        wsa_kfold* f = new wsa_kfold();
        f->device = ctx->device; f->cap_c = (uint32_t)c->knn->C;
        const size_t R = c->cap_rows ? c->cap_rows : 1, N = v.n_clips;
        wsa::DevArena& A = f->mem;
        if (!(A.alloc(&f->d_t_label, R) && A.alloc(&f->d_t_conf, R) && A.alloc(&f->d_t_n, R) && A.alloc(&f->d_t_local, R) && A.alloc(&f->d_cb, R * 4)
              && A.alloc(&f->d_cb_label, R) && A.alloc(&f->d_cb_conf, R) && A.alloc(&f->d_clip_conf, N * f->cap_c) && A.alloc(&f->d_clip_cb, N)
              && A.alloc(&f->d_cb_off, N) && A.pin(&f->h_count, &f->h_count_dev, 4) && upload_index_legend(A, &f->d_key_rank)))
            return alloc_failed(ctx, f);
        wsa_kfold_free(c->fold);
        c->fold = f;
    }
    return enqueue_batch_fold(v, c, reinterpret_cast<hipStream_t>(stream));
}

wsa_status wsa_batch_knn_fold_result(wsa_batch* b, void* stream, wsa_knn_fold_result* out) {
    if (!b || !out) return WSA_ERR_INVALID;
    wsa_batch_view v;
    wsa_batch_view_internal(b, &v);
    wsa_ctx* ctx = v.ctx;
    wsa_kcls* c = *v.kcls;
    if (!c || !c->knn || !c->fold) return fail(ctx, WSA_ERR_INVALID, "no wsa_batch_knn_fold on this batch yet");
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const uint32_t before = c->reruns;
    wsa_knn_result r;
    wsa_status st = wsa_batch_knn_result(b, stream, &r);          // (a rerun of the back end classifies the new rows again ...)
    if (st != WSA_OK) return st;
    if (c->reruns != before) {                                     // ... and they are folded again
        wsa_batch_view_internal(b, &v);
        if ((st = enqueue_batch_fold(v, c, s)) != WSA_OK) return st;
    }
    HIP_TRY(ctx, hipStreamSynchronize(s));
    const wsa_kfold* f = c->fold;
    out->n_callbacks = ((const volatile uint32_t*)f->h_count)[0]; out->n_classes = (uint32_t)c->knn->C; out->n_clips = v.n_clips;
    out->d_cb = f->d_cb; out->d_cb_label = f->d_cb_label; out->d_cb_conf = f->d_cb_conf; out->d_clip_conf = f->d_clip_conf;
    return WSA_OK;
}

wsa_status wsa_batch_copy_knn_fold(wsa_batch* b, void* stream, int32_t* cb, int32_t* cb_label, double* cb_conf, uint32_t cb_cap, double* clip_conf) {
    if (!b) return WSA_ERR_INVALID;
    wsa_knn_fold_result r;
    const wsa_status st = wsa_batch_knn_fold_result(b, stream, &r);
    if (st != WSA_OK) return st;
    wsa_batch_view v;
    wsa_batch_view_internal(b, &v);
    wsa_ctx* ctx = v.ctx;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if ((cb || cb_label || cb_conf) && cb_cap < r.n_callbacks) return fail(ctx, WSA_ERR_INVALID, "KNN fold result buffer too small");
    const size_t K = r.n_callbacks, NC = (size_t)r.n_clips * r.n_classes;
    if (cb && K) HIP_TRY(ctx, hipMemcpyAsync(cb, r.d_cb, K * 4 * sizeof(int32_t), hipMemcpyDefault, s));
    if (cb_label && K) HIP_TRY(ctx, hipMemcpyAsync(cb_label, r.d_cb_label, K * sizeof(int32_t), hipMemcpyDefault, s));
    if (cb_conf && K) HIP_TRY(ctx, hipMemcpyAsync(cb_conf, r.d_cb_conf, K * sizeof(double), hipMemcpyDefault, s));
    if (clip_conf && NC) HIP_TRY(ctx, hipMemcpyAsync(clip_conf, r.d_clip_conf, NC * sizeof(double), hipMemcpyDefault, s));
    HIP_TRY(ctx, hipStreamSynchronize(s));
    return WSA_OK;
}

}  // extern "C"

// ---- streams (wsa_stream_set_knn): K9s on every step's rows, KN-2 carried per stream at level 13; everything allocated at attach time
namespace {

// (StreamKnnParams, classify_internal.hpp)

// `per` entries of each of rows r0 .. r1 - 1 below `cap` (the D2H window) to the pinned table
template <typename T>
__device__ __forceinline__ void push_rows(T* host, const T* dev, uint32_t r0, uint32_t r1, uint32_t cap, uint32_t per, int lane) {
    const uint32_t pe = (r1 < cap ? r1 : cap) * per;
    for (uint32_t i = r0 * per + lane; i < pe; i += 64) host[i] = dev[i];
}

// one wave per stream: its rows' four tables to the mapped pinned buffers, then (level 13) KN-2 with the stream's carried fold
__global__ void __launch_bounds__(256) stream_knn_kernel(StreamKnnParams p) {
    const int lane = threadIdx.x & 63;
    const uint32_t s = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (s >= p.n) return;
    const uint32_t r0 = p.row_off[s], r1 = p.row_off[s + 1];
    push_rows(p.h_label, p.label, r0, r1, p.t.cap, 1u, lane);
    push_rows(p.h_conf, p.conf, r0, r1, p.t.cap, p.C, lane);
    push_rows(p.h_nbr, p.nbr, r0, r1, p.t.cap, p.k, lane);
    push_rows(p.h_sim, p.sim, r0, r1, p.t.cap, p.k, lane);
    if (!p.fold) return;
    fold_stream_step(p.meta, p.conf, p.C, p.step_s, lane, (uint32_t)lane < p.C ? (long long)p.key_rank[lane] : -1, s, p.n, r0, r1, p.carried, p.bits[s] & 1u, p.t);
}

}  // namespace

void wsa_classify::launch_stream_knn(const StreamKnnParams& p, hipStream_t s) {      // four streams per workgroup
    hipLaunchKernelGGL(stream_knn_kernel, dim3((p.n + 3) / 4), dim3(256), 0, s, p);
}

struct wsa_sknn {
    int device = 0;
    const wsa_knn* knn = nullptr;
    wsa_scls_view v{};
    uint32_t C = 0, k = 0;
    KnnParams p{};                           // the store as it stood at attach (row count, k_eff) and the step's tables
    KnnSplit sp;
    int32_t *d_label = nullptr, *d_nbr = nullptr; int64_t* d_key_rank = nullptr; double* d_conf = nullptr; float* d_sim = nullptr;
    CarriedFold carried{};
    double* d_cb_conf = nullptr; int32_t *d_cb = nullptr, *d_cb_label = nullptr;
    wsa::DevArena mem;
    int32_t *h_label = nullptr, *h_label_dev = nullptr, *h_nbr = nullptr, *h_nbr_dev = nullptr; float *h_sim = nullptr, *h_sim_dev = nullptr;
    double *h_conf = nullptr, *h_conf_dev = nullptr;
    int32_t *h_cb = nullptr, *h_cb_dev = nullptr, *h_cb_label = nullptr, *h_cb_label_dev = nullptr;
    double *h_cb_conf = nullptr, *h_cb_conf_dev = nullptr, *h_all = nullptr, *h_all_dev = nullptr;
    uint32_t *h_count = nullptr, *h_count_dev = nullptr;
    std::vector<int32_t> x_label, x_nbr, x_cb, x_cb_label; std::vector<double> x_conf, x_cb_conf; std::vector<float> x_sim;     // steps beyond the D2H window
};

void wsa_sknn_free(wsa_sknn* c) { free_on_device(c); }

wsa_status wsa_sknn_create(const wsa_scls_view& v, const wsa_knn* kn, uint32_t k, wsa_sknn** out) {
    wsa_ctx* ctx = v.ctx;
    *out = nullptr;
    if ((v.level != 5 && v.level != 13) || kn->width != WSA_NFEAT)
        return fail(ctx, WSA_ERR_INVALID, "wsa_stream_set_knn needs streams at output_level 5 (segment features) or 13 (syllable features) and a store of "
                                          + std::to_string(WSA_NFEAT) + "-feature rows: these streams are at output_level " + std::to_string(v.level)
                                          + ", the KNN store holds rows of " + std::to_string(kn->width) + " features");
    if (kn->ctx != ctx) return fail(ctx, WSA_ERR_INVALID, "the KNN store was created on another context (or device) than the streams");
    if (const wsa_status st = knn_refusal(kn, k)) { ctx->err = kn->ctx->err; return st; }
    // K9 takes the rows of a step beyond the D2H window from the window's last query tile on (wsa_sknn_enqueue): the window must end on a tile
    int32_t query_tile = 0;
    wsa_knn_tile_info(nullptr, &query_tile);
    if (v.rows_cap > v.d2h_rows && v.d2h_rows % (uint32_t)query_tile)
        return fail(ctx, WSA_ERR_INVALID, "a D2H window of " + std::to_string(v.d2h_rows) + " rows is not a whole number of " + std::to_string(query_tile) + "-row query tiles");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    wsa_sknn* c = new wsa_sknn();
    c->device = ctx->device; c->knn = kn; c->v = v; c->C = (uint32_t)kn->C; c->k = k;
    const size_t R = v.rows_cap ? v.rows_cap : 1, W = v.d2h_rows ? v.d2h_rows : 1, C = c->C;
    wsa::DevArena& A = c->mem;
    bool ok = A.alloc(&c->d_label, R) && A.alloc(&c->d_conf, R * C) && A.alloc(&c->d_nbr, R * k) && A.alloc(&c->d_sim, R * k)
              && knn_split_alloc(A, kn, v.d2h_rows, k, 0, c->sp)
              && A.pin(&c->h_label, &c->h_label_dev, W) && A.pin(&c->h_conf, &c->h_conf_dev, W * C) && A.pin(&c->h_nbr, &c->h_nbr_dev, W * k) && A.pin(&c->h_sim, &c->h_sim_dev, W * k);
    if (ok && v.level == 13) {
        ok = A.alloc(&c->carried.acc_all, v.n_streams * C, true) && A.alloc(&c->carried.in_all, v.n_streams * C, true) && A.alloc(&c->carried.first, v.n_streams * C, true)
             && A.alloc(&c->carried.stamp, (size_t)v.n_streams, true) && upload_index_legend(A, &c->d_key_rank)
             && A.alloc(&c->d_cb, R * 4) && A.alloc(&c->d_cb_label, R) && A.alloc(&c->d_cb_conf, R)
             && A.pin(&c->h_cb, &c->h_cb_dev, W * 4) && A.pin(&c->h_cb_label, &c->h_cb_label_dev, W)
             && A.pin(&c->h_cb_conf, &c->h_cb_conf_dev, W) && A.pin(&c->h_all, &c->h_all_dev, (size_t)v.n_streams * C) && A.pin(&c->h_count, &c->h_count_dev, 4);
    }
    ok = ok && hipDeviceSynchronize() == hipSuccess;
    if (!ok) return alloc_failed(ctx, c);
    c->p = knn_params(kn, v.d_feat, 0, v.d_totals, k);
    c->p.stride = WSA_NFEAT;
    c->p.label = c->d_label; c->p.conf = c->d_conf; c->p.nbr = c->d_nbr; c->p.sim = c->d_sim;
    *out = c;
    return WSA_OK;
}

// K9s on the rows of the step's D2H window (partial + merge; the row count is read on the device), K9 itself on the rows of a step beyond
// it (no workgroup of it finds a tile otherwise), then the push / fold kernel: the KNN nodes of the captured step
wsa_status wsa_sknn_enqueue(wsa_sknn* c, hipStream_t s) {
    const wsa_scls_view& v = c->v;
    launch_knn_split(c->knn, c->p, c->sp, s);
    HIP_TRY(v.ctx, hipGetLastError());
    if (v.rows_cap > c->sp.window) {           // (the window then ends on a query tile: checked at attach)
        KnnParams tail = c->p;
        tail.qt0 = c->sp.window / 64u;
        const uint32_t beyond = v.rows_cap - c->sp.window, most = 64u * (uint32_t)(v.ctx->n_cu > 0 ? v.ctx->n_cu : 256);
        launch_knn(c->knn, tail, beyond < most ? beyond : most, s);
        HIP_TRY(v.ctx, hipGetLastError());
    }
    StreamKnnParams p{};
    p.n = v.n_streams; p.C = c->C; p.k = c->k; p.fold = v.level == 13 ? 1 : 0; p.step_s = v.ctx->cfg.window_step / 1e3;
    p.meta = v.d_meta; p.row_off = v.d_row_off; p.bits = v.d_bits; p.key_rank = c->d_key_rank;
    p.label = c->d_label; p.conf = c->d_conf; p.nbr = c->d_nbr; p.sim = c->d_sim;
    p.carried = c->carried;
    p.t = StepFoldTables{v.d2h_rows, c->d_cb, c->d_cb_label, c->d_cb_conf, c->h_cb_dev, c->h_cb_label_dev, c->h_cb_conf_dev, c->h_all_dev, c->h_count_dev};
    p.h_label = c->h_label_dev; p.h_conf = c->h_conf_dev; p.h_nbr = c->h_nbr_dev; p.h_sim = c->h_sim_dev;
    launch_stream_knn(p, s);
    HIP_TRY(v.ctx, hipGetLastError());
    return WSA_OK;
}

// after the step has completed: the tables of `rows` rows; a step beyond the D2H window is fetched from the device here
wsa_status wsa_sknn_result(wsa_sknn* c, uint32_t rows, wsa_stream_knn_result* o) {
    const wsa_scls_view& v = c->v;
    wsa_ctx* ctx = v.ctx;
    const bool fold = v.level == 13;
    const uint32_t ncb = fold ? ((const volatile uint32_t*)c->h_count)[0] : 0u;
    o->n_rows = rows; o->n_classes = c->C; o->k = c->k; o->k_eff = c->p.k_eff; o->n_callbacks = ncb; o->n_streams = v.n_streams; o->slices = c->sp.slices;
    o->label = c->h_label; o->conf = c->h_conf; o->nbr = c->h_nbr; o->sim = c->h_sim;
    o->cb = fold ? c->h_cb : nullptr; o->cb_label = fold ? c->h_cb_label : nullptr; o->cb_conf = fold ? c->h_cb_conf : nullptr;
    o->stream_conf = fold ? c->h_all : nullptr;
    if (rows > v.d2h_rows) {
        HIP_TRY(ctx, hipSetDevice(ctx->device));
        wsa_status st = fetch_table(ctx, c->x_label, (const int32_t*)c->d_label, rows, &o->label);
        if (st == WSA_OK) st = fetch_table(ctx, c->x_conf, (const double*)c->d_conf, (size_t)rows * c->C, &o->conf);
        if (st == WSA_OK) st = fetch_table(ctx, c->x_nbr, (const int32_t*)c->d_nbr, (size_t)rows * c->k, &o->nbr);
        if (st == WSA_OK) st = fetch_table(ctx, c->x_sim, (const float*)c->d_sim, (size_t)rows * c->k, &o->sim);
        if (fold) {
            if (st == WSA_OK) st = fetch_table(ctx, c->x_cb, (const int32_t*)c->d_cb, (size_t)ncb * 4, &o->cb);
            if (st == WSA_OK) st = fetch_table(ctx, c->x_cb_label, (const int32_t*)c->d_cb_label, ncb, &o->cb_label);
            if (st == WSA_OK) st = fetch_table(ctx, c->x_cb_conf, (const double*)c->d_cb_conf, ncb, &o->cb_conf);
        }
        return st;
    }
    return WSA_OK;
}
