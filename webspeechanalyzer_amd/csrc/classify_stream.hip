// classify_stream.hip — the classifier inside a stream object's step (wsa_stream_set_model / wsa_stream_set_ensemble): K6 (or K6e) on
// every step's rows, and at level 13 the app's per-callback fold K6b (classify_fold.hpp) carried from step to step on the device, with
// the step's tables pushed to mapped pinned memory.  stream_step.hip captures these launches into the stream object's step.
#include <cstring>
#include <string>
#include <vector>
#include "classify_internal.hpp"
#include "classify_fold.hpp"

using wsa_api::fail;
using namespace wsa_classify;

namespace {

// ---- K6b on a stream step: one wave per stream pushes its rows' probabilities to the mapped pinned table (rows below the D2H window)
// and, at level 13, folds them with the stream's carried fold (fold_stream_step, classify_fold.hpp).
// (StreamClsParams, classify_internal.hpp)

// the probabilities of rows r0 .. r1 - 1 below `cap` (the D2H window), C per row, to the pinned table
__device__ __forceinline__ void push_prob(float* h_prob, const float* prob, uint32_t r0, uint32_t r1, uint32_t cap, uint32_t C, int lane) {
    const uint32_t pe = (r1 < cap ? r1 : cap) * C;
    for (uint32_t i = r0 * C + lane; i < pe; i += 64) h_prob[i] = prob[i];
}

__global__ void __launch_bounds__(256) stream_classes_kernel(StreamClsParams p) {
    const int lane = threadIdx.x & 63;
    const uint32_t s = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (s >= p.n) return;
    const uint32_t r0 = p.row_off[s], r1 = p.row_off[s + 1];
    push_prob(p.h_prob, p.prob, r0, r1, p.t.cap, p.C, lane);
    if (!p.fold) return;
    fold_stream_step(p.meta, p.prob, p.C, p.step_s, lane, (uint32_t)lane < p.C ? (long long)p.key_rank[lane] : -1, s, p.n, r0, r1, p.carried, p.bits[s] & 1u, p.t);
}

// ---- K6b-e on a stream step: one wave per (stream, member) folds with that pair's carried accumulator and writes the member's entries
// straight to the step's tables (the index as in stream_classes_kernel); then one wave per stream decides — winners with callbacks on
// lanes, min_entropy_db by lane 0 in callback order with the stream's running max_inv_entropy / min_entropy_db carried on the device and
// reset by START (ref reset_predictions(true), prediction.js:24-36; the device also forgets min_entropy_db, see wsa.h).  In a step the
// members' tables (FoldMember t_*) are indexed by callback, not by row.
// (StreamMember, StreamEnsParams: classify_internal.hpp)

__global__ void __launch_bounds__(256) stream_fold_group_kernel(StreamEnsParams p) {
    const int lane = threadIdx.x & 63;
    const uint32_t w = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (w >= p.n * p.n_members) return;
    const uint32_t s = w / p.n_members, d = w - s * p.n_members;
    const FoldMember m = p.tab[d];
    const StreamMember sm = p.stab[d];
    const uint32_t r0 = p.row_off[s], r1 = p.row_off[s + 1];
    push_prob(sm.h_prob, m.prob, r0, r1, p.cap, m.C, lane);
    if (!p.fold) return;
    const bool cls = (uint32_t)lane < m.C;
    const long long kr = cls ? (long long)m.key_rank[lane] : -1;
    const size_t sc = (size_t)s * m.C + lane;
    FoldAcc a = load_fold(sm.carried, s, sc, cls, p.bits[s] & 1u);
    uint32_t k = callback_starts(p.meta, 0, r0, lane);
    for (uint32_t r = r0; r < r1;) {
        const int si = p.meta[(size_t)r * 8 + 1];
        const uint32_t e = callback_end(p.meta, r, r1);
        int label; double conf, seg_max, all_max, all_sum;
        fold_callback(p.meta, m.prob, m.C, p.step_s, lane, cls, kr, r, e, a, label, conf, seg_max);
        all_max_and_sum(a, m.C, lane, cls, kr, all_max, all_sum);
        if (lane == 0) {
            m.t_label[k] = label; m.t_conf[k] = conf; m.t_seg[k] = seg_max; m.t_all_max[k] = all_max; m.t_all_sum[k] = all_sum;
            if (k < p.cap) { sm.h_cb_label[k] = label; sm.h_cb_conf[k] = conf; sm.h_cb_all_max[k] = all_max; }
            if (d == 0) {
                write_callback(p.o.cb, k, (int32_t)s, si, r, (int32_t)(e - r));
                if (k < p.cap) write_callback(p.h.cb, k, (int32_t)s, si, r, (int32_t)(e - r));
            }
        }
        k++;
        r = e;
    }
    store_fold(sm.carried, s, sc, cls, lane, a);
    if (cls) sm.h_conf[sc] = a.acc_all;
    if (lane == 0 && d == 0 && s == p.n - 1) p.h_count[0] = k;
}

// member d's figures for callback `at` of the step, where stream_fold_group_kernel left them (the members' step tables)
struct StepFigures {
    const FoldMember* tab; size_t at;
    __device__ MemberFigures operator()(uint32_t d) const { const FoldMember& m = tab[d]; return {m.t_seg[at], m.t_label[at], m.t_conf[at], m.t_all_max[at], m.t_all_sum[at]}; }
};

__global__ void __launch_bounds__(256) stream_decide_kernel(StreamEnsParams p) {
    const int lane = threadIdx.x & 63;
    const uint32_t s = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (s >= p.n) return;
    const uint32_t r0 = p.row_off[s], r1 = p.row_off[s + 1];
    const uint32_t k0 = callback_starts(p.meta, 0, r0, lane), k1 = k0 + callback_starts(p.meta, r0, r1, lane);
    for (uint32_t k = k0 + lane; k < k1; k += 64) {
        int db, label; double conf;
        ensemble_winner(StepFigures{p.tab, k}, p.n_members, db, label, conf);
        if (p.tab[0].t_label[k] == -2) db = -2;
        p.o.cb_db[k] = db; p.o.cb_top_label[k] = label; p.o.cb_top_conf[k] = conf;
        if (k < p.cap) { p.h.cb_db[k] = db; p.h.cb_top_label[k] = label; p.h.cb_top_conf[k] = conf; }
    }
    if (lane != 0) return;
    double max_inv = 0.0; int min_db = -1;
    if (!(p.bits[s] & 1u)) { max_inv = p.max_inv[s]; min_db = p.min_db[s]; }
    for (uint32_t k = k0; k < k1; k++) {
        const double ent = ensemble_min_db(StepFigures{p.tab, k}, p.n_members, p.tab[0].t_label[k] == -2, max_inv, min_db);
        p.o.cb_min_db[k] = min_db; p.o.cb_entropy[k] = ent;
        if (k < p.cap) { p.h.cb_min_db[k] = min_db; p.h.cb_entropy[k] = ent; }
    }
    p.max_inv[s] = max_inv; p.min_db[s] = min_db;
    p.h.clip_min_db[s] = min_db;
}

// the carried fold of n streams with C classes each, zeroed
bool alloc_carried(wsa::DevArena& A, CarriedFold& f, size_t n, size_t C) {
    return A.alloc(&f.acc_all, n * C, true) && A.alloc(&f.in_all, n * C, true) && A.alloc(&f.first, n * C, true) && A.alloc(&f.stamp, n, true);
}

}  // namespace

// ---- the step's fold launches (classify_internal.hpp): four streams, or four (stream, member) pairs, per workgroup
namespace wsa_classify {

void launch_stream_classes(const StreamClsParams& p, hipStream_t s) {
    hipLaunchKernelGGL(stream_classes_kernel, dim3((p.n + 3) / 4), dim3(256), 0, s, p);
}
void launch_stream_ensemble(const StreamEnsParams& p, hipStream_t s) {
    const uint32_t waves = p.n * p.n_members;
    hipLaunchKernelGGL(stream_fold_group_kernel, dim3((waves + 3) / 4), dim3(256), 0, s, p);
    if (p.fold) hipLaunchKernelGGL(stream_decide_kernel, dim3((p.n + 3) / 4), dim3(256), 0, s, p);
}

}  // namespace wsa_classify

// ---- streams (wsa_stream_set_model): K6 on every step's rows, the carried fold at level 13; everything allocated at attach time
struct wsa_scls {
    int device = 0;
    const wsa_model* model = nullptr;
    wsa_scls_view v{};
    uint32_t C = 0;
    float* d_prob = nullptr;
    CarriedFold carried{};
    double* d_cb_conf = nullptr; int32_t *d_cb = nullptr, *d_cb_label = nullptr;
    wsa::DevArena mem;
    float *h_prob = nullptr, *h_prob_dev = nullptr;
    int32_t *h_cb = nullptr, *h_cb_dev = nullptr, *h_cb_label = nullptr, *h_cb_label_dev = nullptr;
    double *h_cb_conf = nullptr, *h_cb_conf_dev = nullptr, *h_conf = nullptr, *h_conf_dev = nullptr;
    uint32_t *h_count = nullptr, *h_count_dev = nullptr;
    std::vector<float> x_prob; std::vector<int32_t> x_cb, x_cb_label; std::vector<double> x_cb_conf;     // steps beyond the D2H window
};

void wsa_scls_free(wsa_scls* c) { free_on_device(c); }

wsa_status wsa_scls_create(const wsa_scls_view& v, const wsa_model* m, wsa_scls** out) {
    wsa_ctx* ctx = v.ctx;
    *out = nullptr;
    if (const wsa_status st = pairing_check(ctx, "wsa_stream_set_model", ON_STREAMS, v.level, ONE_MODEL, m->ctx, m->nin, m->softmax)) return st;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    wsa_scls* c = new wsa_scls();
    c->device = ctx->device; c->model = m; c->v = v; c->C = (uint32_t)m->C;
    const size_t R = v.rows_cap ? v.rows_cap : 1, W = v.d2h_rows ? v.d2h_rows : 1;
    wsa::DevArena& A = c->mem;
    bool ok = A.alloc(&c->d_prob, R * c->C);
    if (ok && v.level == 13) {
        ok = alloc_carried(A, c->carried, v.n_streams, c->C) && A.alloc(&c->d_cb, R * 4) && A.alloc(&c->d_cb_label, R) && A.alloc(&c->d_cb_conf, R)
             && A.pin(&c->h_cb, &c->h_cb_dev, W * 4) && A.pin(&c->h_cb_label, &c->h_cb_label_dev, W)
             && A.pin(&c->h_cb_conf, &c->h_cb_conf_dev, W) && A.pin(&c->h_conf, &c->h_conf_dev, (size_t)v.n_streams * c->C) && A.pin(&c->h_count, &c->h_count_dev, 4);
    }
    ok = ok && A.pin(&c->h_prob, &c->h_prob_dev, W * c->C) && hipDeviceSynchronize() == hipSuccess;
    if (!ok) return alloc_failed(ctx, c);
    *out = c;
    return WSA_OK;
}

// K6 on the step's compacted rows (count on the device), then the stream fold / push: two kernel nodes of the captured step
wsa_status wsa_scls_enqueue(wsa_scls* c, hipStream_t s) {
    const wsa_scls_view& v = c->v;
    const wsa_model* m = c->model;
    // a step at config 5 has tens to hundreds of rows: tiles of 16 rows spread them over as many CUs as possible, and the grid covers the
    // D2H window (1024 rows) in one pass — a larger step strides over its tiles instead of launching rows_cap / 16 mostly idle workgroups
    launch_classify(m, cls_params(m, v.d_feat, 0, v.d_totals, c->d_prob), v.rows_cap < v.d2h_rows ? v.rows_cap : v.d2h_rows, s, 1);
    HIP_TRY(v.ctx, hipGetLastError());
    StreamClsParams p{};
    p.n = v.n_streams; p.C = c->C; p.fold = v.level == 13 ? 1 : 0; p.step_s = v.ctx->cfg.window_step / 1e3;
    p.meta = v.d_meta; p.row_off = v.d_row_off; p.prob = c->d_prob; p.key_rank = m->d_key_rank; p.bits = v.d_bits;
    p.carried = c->carried;
    p.t = StepFoldTables{v.d2h_rows, c->d_cb, c->d_cb_label, c->d_cb_conf, c->h_cb_dev, c->h_cb_label_dev, c->h_cb_conf_dev, c->h_conf_dev, c->h_count_dev};
    p.h_prob = c->h_prob_dev;
    launch_stream_classes(p, s);
    HIP_TRY(v.ctx, hipGetLastError());
    return WSA_OK;
}

// after the step has completed: the tables of `rows` rows; a step beyond the D2H window is fetched from the device here
wsa_status wsa_scls_result(wsa_scls* c, uint32_t rows, wsa_stream_class_result* o) {
    const wsa_scls_view& v = c->v;
    wsa_ctx* ctx = v.ctx;
    const bool fold = v.level == 13;
    const uint32_t ncb = fold ? ((const volatile uint32_t*)c->h_count)[0] : 0u;
    o->n_rows = rows; o->n_classes = c->C; o->n_callbacks = ncb; o->n_streams = v.n_streams;
    o->prob = c->h_prob;
    o->cb = fold ? c->h_cb : nullptr; o->cb_label = fold ? c->h_cb_label : nullptr; o->cb_conf = fold ? c->h_cb_conf : nullptr;
    o->stream_conf = fold ? c->h_conf : nullptr;
    if (rows > v.d2h_rows) {
        HIP_TRY(ctx, hipSetDevice(ctx->device));
        wsa_status st = fetch_table(ctx, c->x_prob, (const float*)c->d_prob, (size_t)rows * c->C, &o->prob);
        if (fold) {
            if (st == WSA_OK) st = fetch_table(ctx, c->x_cb, (const int32_t*)c->d_cb, (size_t)ncb * 4, &o->cb);
            if (st == WSA_OK) st = fetch_table(ctx, c->x_cb_label, (const int32_t*)c->d_cb_label, ncb, &o->cb_label);
            if (st == WSA_OK) st = fetch_table(ctx, c->x_cb_conf, (const double*)c->d_cb_conf, ncb, &o->cb_conf);
        }
        return st;
    }
    return WSA_OK;
}

// ---- streams with an ensemble (wsa_stream_set_ensemble): K6e, the (stream, member) folds and the per-stream decision as three kernels of the step
struct wsa_sens {
    int device = 0;
    const wsa_ensemble* ens = nullptr;
    wsa_scls_view v{};
    uint32_t n = 0, grid = 1;
    uint32_t C[WSA_ENSEMBLE_MAX] = {};
    float* d_prob[WSA_ENSEMBLE_MAX] = {};
    FoldMember fm[WSA_ENSEMBLE_MAX] = {};
    StreamMember sm[WSA_ENSEMBLE_MAX] = {};                     // (device pointers)
    float* h_prob[WSA_ENSEMBLE_MAX] = {}; int32_t* h_cb_label[WSA_ENSEMBLE_MAX] = {};
    double *h_cb_conf[WSA_ENSEMBLE_MAX] = {}, *h_cb_all_max[WSA_ENSEMBLE_MAX] = {}, *h_conf[WSA_ENSEMBLE_MAX] = {};
    ClsGroupEntry* d_ctab = nullptr; FoldMember* d_ftab = nullptr; StreamMember* d_stab = nullptr;
    EnsTables o{}, h{}, h_dev{};
    double* d_max_inv = nullptr; int32_t* d_min_db = nullptr;
    uint32_t *h_count = nullptr, *h_count_dev = nullptr;
    wsa::DevArena mem;
    // steps beyond the D2H window
    std::vector<float> x_prob[WSA_ENSEMBLE_MAX]; std::vector<int32_t> x_cb_label[WSA_ENSEMBLE_MAX]; std::vector<double> x_cb_conf[WSA_ENSEMBLE_MAX], x_cb_all_max[WSA_ENSEMBLE_MAX];
    std::vector<int32_t> x_cb, x_cb_db, x_cb_top_label, x_cb_min_db; std::vector<double> x_cb_top_conf, x_cb_entropy;
};

void wsa_sens_free(wsa_sens* c) { free_on_device(c); }

wsa_status wsa_sens_create(const wsa_scls_view& v, const wsa_ensemble* e, wsa_sens** out) {
    wsa_ctx* ctx = v.ctx;
    *out = nullptr;
    if (const wsa_status st = pairing_check(ctx, "wsa_stream_set_ensemble", ON_STREAMS, v.level, AN_ENSEMBLE, e->ctx, WSA_NFEAT, e->softmax)) return st;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    wsa_sens* c = new wsa_sens();
    c->device = ctx->device; c->ens = e; c->v = v; c->n = e->n;
    const bool fold = v.level == 13;
    const size_t R = v.rows_cap ? v.rows_cap : 1, W = v.d2h_rows ? v.d2h_rows : 1, NS = v.n_streams;
    wsa::DevArena& A = c->mem;
    bool ok = true;
    if (fold) {
        ok = alloc_ens_tables(A, c->o, R, NS) && pin_ens_tables(A, c->h, c->h_dev, W, NS)
             && A.alloc(&c->d_max_inv, NS, true) && A.alloc(&c->d_min_db, NS) && A.pin(&c->h_count, &c->h_count_dev, 4)
             && hipMemset(c->d_min_db, 0xff, (NS ? NS : 1) * sizeof(int32_t)) == hipSuccess;
        for (size_t i = 0; ok && i < NS; i++) c->h.clip_min_db[i] = -1;
    }
    for (uint32_t d = 0; d < e->n && ok; d++) {
        const wsa_model* m = e->m[d];
        const size_t Cd = (size_t)m->C;
        FoldMember& f = c->fm[d];
        StreamMember& q = c->sm[d];
        c->C[d] = (uint32_t)Cd;
        ok = A.alloc(&c->d_prob[d], R * Cd) && A.pin(&c->h_prob[d], &q.h_prob, W * Cd);
        f.C = (uint32_t)Cd; f.prob = c->d_prob[d]; f.key_rank = m->d_key_rank;
        if (ok && fold) {
            ok = A.alloc(&f.t_label, R) && A.alloc(&f.t_conf, R) && A.alloc(&f.t_seg, R) && A.alloc(&f.t_all_max, R) && A.alloc(&f.t_all_sum, R)
                 && alloc_carried(A, q.carried, NS, Cd)
                 && A.pin(&c->h_cb_label[d], &q.h_cb_label, W) && A.pin(&c->h_cb_conf[d], &q.h_cb_conf, W)
                 && A.pin(&c->h_cb_all_max[d], &q.h_cb_all_max, W) && A.pin(&c->h_conf[d], &q.h_conf, NS * Cd);
            f.cb_label = f.t_label; f.cb_conf = f.t_conf; f.cb_all_max = f.t_all_max;
        }
    }
    if (ok) {
        // as for one model: tiles of 16 rows, and a grid that covers the D2H window in one pass
        std::vector<ClsGroupEntry> tab;
        c->grid = group_table(e, v.d_feat, v.d_totals, c->d_prob, v.rows_cap < v.d2h_rows ? v.rows_cap : v.d2h_rows, true, tab);
        std::vector<FoldMember> ftab(c->fm, c->fm + e->n);
        std::vector<StreamMember> stab(c->sm, c->sm + e->n);
        ok = A.upload(&c->d_ctab, tab) && A.upload(&c->d_ftab, ftab) && A.upload(&c->d_stab, stab) && hipDeviceSynchronize() == hipSuccess;
    }
    if (!ok) return alloc_failed(ctx, c);
    *out = c;
    return WSA_OK;
}

wsa_status wsa_sens_enqueue(wsa_sens* c, hipStream_t s) {
    const wsa_scls_view& v = c->v;
    launch_classify_group(c->d_ctab, c->n, v.d_totals, c->grid, c->ens->lds_stream, s);
    HIP_TRY(v.ctx, hipGetLastError());
    StreamEnsParams p{};
    p.n = v.n_streams; p.n_members = c->n; p.cap = v.d2h_rows; p.fold = v.level == 13 ? 1 : 0; p.step_s = v.ctx->cfg.window_step / 1e3;
    p.meta = v.d_meta; p.row_off = v.d_row_off; p.bits = v.d_bits; p.tab = c->d_ftab; p.stab = c->d_stab;
    p.o = c->o; p.h = c->h_dev; p.max_inv = c->d_max_inv; p.min_db = c->d_min_db; p.h_count = c->h_count_dev;
    launch_stream_ensemble(p, s);
    HIP_TRY(v.ctx, hipGetLastError());
    return WSA_OK;
}

// after the step has completed: the tables of `rows` rows; a step beyond the D2H window is fetched from the device here
wsa_status wsa_sens_result(wsa_sens* c, uint32_t rows, wsa_stream_ensemble_result* o) {
    const wsa_scls_view& v = c->v;
    wsa_ctx* ctx = v.ctx;
    const bool fold = v.level == 13;
    const uint32_t ncb = fold ? ((const volatile uint32_t*)c->h_count)[0] : 0u;
    std::memset(o, 0, sizeof(*o));
    o->n_rows = rows; o->n_members = c->n; o->n_callbacks = ncb; o->n_streams = v.n_streams;
    for (uint32_t d = 0; d < c->n; d++) {
        o->n_classes[d] = c->C[d]; o->prob[d] = c->h_prob[d];
        if (fold) { o->cb_label[d] = c->h_cb_label[d]; o->cb_conf[d] = c->h_cb_conf[d]; o->cb_all_max[d] = c->h_cb_all_max[d]; o->stream_conf[d] = c->h_conf[d]; }
    }
    if (fold) {
        o->cb = c->h.cb; o->cb_db = c->h.cb_db; o->cb_top_label = c->h.cb_top_label; o->cb_top_conf = c->h.cb_top_conf;
        o->cb_min_db = c->h.cb_min_db; o->cb_entropy = c->h.cb_entropy; o->stream_min_db = c->h.clip_min_db;
    }
    if (rows > v.d2h_rows) {
        HIP_TRY(ctx, hipSetDevice(ctx->device));
        wsa_status st = WSA_OK;
        for (uint32_t d = 0; d < c->n && st == WSA_OK; d++) {
            st = fetch_table(ctx, c->x_prob[d], (const float*)c->d_prob[d], (size_t)rows * c->C[d], &o->prob[d]);
            if (!fold) continue;
            if (st == WSA_OK) st = fetch_table(ctx, c->x_cb_label[d], (const int32_t*)c->fm[d].t_label, ncb, &o->cb_label[d]);
            if (st == WSA_OK) st = fetch_table(ctx, c->x_cb_conf[d], (const double*)c->fm[d].t_conf, ncb, &o->cb_conf[d]);
            if (st == WSA_OK) st = fetch_table(ctx, c->x_cb_all_max[d], (const double*)c->fm[d].t_all_max, ncb, &o->cb_all_max[d]);
        }
        if (fold) {
            if (st == WSA_OK) st = fetch_table(ctx, c->x_cb, (const int32_t*)c->o.cb, (size_t)ncb * 4, &o->cb);
            if (st == WSA_OK) st = fetch_table(ctx, c->x_cb_db, (const int32_t*)c->o.cb_db, ncb, &o->cb_db);
            if (st == WSA_OK) st = fetch_table(ctx, c->x_cb_top_label, (const int32_t*)c->o.cb_top_label, ncb, &o->cb_top_label);
            if (st == WSA_OK) st = fetch_table(ctx, c->x_cb_top_conf, (const double*)c->o.cb_top_conf, ncb, &o->cb_top_conf);
            if (st == WSA_OK) st = fetch_table(ctx, c->x_cb_min_db, (const int32_t*)c->o.cb_min_db, ncb, &o->cb_min_db);
            if (st == WSA_OK) st = fetch_table(ctx, c->x_cb_entropy, (const double*)c->o.cb_entropy, ncb, &o->cb_entropy);
        }
        if (st != WSA_OK) return st;
    }
    return WSA_OK;
}
