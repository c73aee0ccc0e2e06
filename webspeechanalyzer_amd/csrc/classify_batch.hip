// classify_batch.hip — the classifier on a batch: K6 (or K6e) over the batch's compacted rows, then at level 13 the app's per-callback
// fold K6b (classify_fold.hpp) with one wave per clip, or per (clip, member) of an ensemble, and the compaction of its per-row tables
// into per-callback ones; the batch's classification state and the wsa_batch_* classification and regression entry points
// (include/wsa.h "Syllable classification").
#include <cstring>
#include <string>
#include <vector>
#include "classify_internal.hpp"
#include "classify_fold.hpp"

using wsa_api::fail;
using namespace wsa_classify;

// the classification buffers of one batch (the first wsa_batch_classify or wsa_batch_regress allocates them)
struct wsa_cls {
    int device = 0;
    uint32_t cap_rows = 0, cap_c = 0, n_clips = 0;
    float* d_prob = nullptr;
    int32_t *d_t_label = nullptr, *d_t_n = nullptr, *d_t_local = nullptr, *d_cb = nullptr, *d_cb_label = nullptr;
    double *d_t_conf = nullptr, *d_cb_conf = nullptr, *d_clip_conf = nullptr;
    uint32_t *d_clip_cb = nullptr, *d_cb_off = nullptr;
    uint32_t *h_count = nullptr, *h_count_dev = nullptr;     // pinned + mapped: callbacks of the last fold
    wsa::DevArena mem;
    const wsa_model* model = nullptr; int level = 0, n_classes = 0; uint32_t reruns = 0; bool done = false;
    double* d_value = nullptr; double out_min = 0.0, out_span = 0.0;      // wsa_batch_regress: one value per row
};

// the ensemble tables of one batch, built for one ensemble
struct wsa_ecls {
    int device = 0;
    const wsa_ensemble* ens = nullptr; uint64_t serial = 0;
    uint32_t n = 0, n_clips = 0, reruns = 0; int level = 0;
    uint32_t C[WSA_ENSEMBLE_MAX] = {};
    float* d_prob[WSA_ENSEMBLE_MAX] = {};
    FoldMember fm[WSA_ENSEMBLE_MAX] = {};
    ClsGroupEntry* d_ctab = nullptr; FoldMember* d_ftab = nullptr;
    int32_t *d_t_n = nullptr, *d_t_local = nullptr; uint32_t *d_clip_cb = nullptr, *d_cb_off = nullptr;
    size_t lds = 0;                          // K6e's dynamic LDS (kept here: the ensemble object is only compared, never read, after the tables exist)
    EnsTables t{}, o{};                      // the decision per row (written by the fold) / per callback (the compaction)
    uint32_t *h_count = nullptr, *h_count_dev = nullptr;
    uint32_t grid = 1;
    wsa::DevArena mem;
};

void wsa_cls_free(wsa_cls* c) { free_on_device(c); }
void wsa_ecls_free(wsa_ecls* c) { free_on_device(c); }

namespace {

// ---- K6b-e: the fold for every member of an ensemble, one wave per (clip, member) (FoldGroupParams, classify_internal.hpp)
// One workgroup per clip, one wave per member: the waves walk the clip's callbacks in step (the rows and so the trip counts are the same
// for all of them), leave each callback's three figures in LDS, and after one barrier every thread holds the decision — so the running
// max_inv_entropy / min_entropy_db, a chain over the clip's callbacks, costs nothing beyond the fold's own walk.  Two LDS sets by callback
// parity make one barrier per callback enough.
__global__ void __launch_bounds__(64 * WSA_ENSEMBLE_MAX) fold_group_kernel(FoldGroupParams p) {
    __shared__ double s_seg[2][WSA_ENSEMBLE_MAX], s_max[2][WSA_ENSEMBLE_MAX], s_sum[2][WSA_ENSEMBLE_MAX], s_conf[2][WSA_ENSEMBLE_MAX];
    __shared__ int s_label[2][WSA_ENSEMBLE_MAX];
    const int lane = threadIdx.x & 63;
    const uint32_t clip = blockIdx.x, d = threadIdx.x >> 6;
    const FoldMember m = p.tab[d];
    const uint32_t r0 = p.row_off[clip], r1 = p.row_off[clip + 1];
    const bool cls = (uint32_t)lane < m.C;
    const long long kr = cls ? (long long)m.key_rank[lane] : -1;
    FoldAcc a{0.0, false, 0, 0};
    uint32_t ncb = 0;
    double max_inv = 0.0; int min_db = -1;
    for (uint32_t r = r0; r < r1;) {
        const uint32_t e = callback_end(p.meta, r, r1);
        int label; double conf, seg_max, all_max, all_sum;
        fold_callback(p.meta, m.prob, m.C, p.step_s, lane, cls, kr, r, e, a, label, conf, seg_max);
        all_max_and_sum(a, m.C, lane, cls, kr, all_max, all_sum);
        const int pb = (int)(ncb & 1u);
        if (lane == 0) {
            m.t_label[r] = label; m.t_conf[r] = conf; m.t_all_max[r] = all_max;
            s_seg[pb][d] = seg_max; s_max[pb][d] = all_max; s_sum[pb][d] = all_sum; s_conf[pb][d] = conf; s_label[pb][d] = label;
        }
        __syncthreads();
        int db, top_label; double top_conf;
        const auto of = [&](uint32_t j) { return MemberFigures{s_seg[pb][j], s_label[pb][j], s_conf[pb][j], s_max[pb][j], s_sum[pb][j]}; };
        ensemble_winner(of, p.n_members, db, top_label, top_conf);
        const bool skipped = label == -2;                       // the durations, not the model, decide it: the same for every member
        const double ent = ensemble_min_db(of, p.n_members, skipped, max_inv, min_db);
        if (threadIdx.x == 0) {
            p.t_n[r] = (int32_t)(e - r); p.t_local[r] = (int32_t)ncb;
            p.t.cb_db[r] = skipped ? -2 : db; p.t.cb_top_label[r] = top_label; p.t.cb_top_conf[r] = top_conf; p.t.cb_min_db[r] = min_db; p.t.cb_entropy[r] = ent;
        }
        for (uint32_t q = r + 1 + threadIdx.x; q < e; q += blockDim.x) p.t_n[q] = 0;
        ncb++;
        r = e;
    }
    if (cls) m.clip_conf[(size_t)clip * m.C + lane] = a.acc_all;
    if (threadIdx.x == 0) { p.clip_cb[clip] = ncb; p.t.clip_min_db[clip] = min_db; }
}

// the compaction of K6b for an ensemble: every callback's per-member entries and decision from the row it starts at
__global__ void __launch_bounds__(1024) fold_compact_group_kernel(uint32_t n_clips, uint32_t n_members, const uint32_t* row_off, const int32_t* meta,
                                                                  const uint32_t* clip_cb, uint32_t* cb_off, const int32_t* t_n, const int32_t* t_local,
                                                                  const FoldMember* tab, EnsTables t, EnsTables o, uint32_t* host) {
    __shared__ uint32_t s_part[1024];
    __shared__ uint32_t s_base;
    const int tid = threadIdx.x;
    const uint32_t n_cb = compact_offsets(n_clips, clip_cb, cb_off, s_part, &s_base);
    const uint32_t n_rows = row_off[n_clips];
    __syncthreads();
    for (uint32_t r = tid; r < n_rows; r += 1024) {
        const int32_t nsyl = t_n[r];
        if (nsyl <= 0) continue;
        const int32_t clip = meta[(size_t)r * 8];
        const uint32_t k = cb_off[clip] + (uint32_t)t_local[r];
        write_callback(o.cb, k, clip, meta[(size_t)r * 8 + 1], r, nsyl);
        for (uint32_t d = 0; d < n_members; d++) {
            const FoldMember& m = tab[d];
            m.cb_label[k] = m.t_label[r]; m.cb_conf[k] = m.t_conf[r]; m.cb_all_max[k] = m.t_all_max[r];
        }
        o.cb_db[k] = t.cb_db[r]; o.cb_top_label[k] = t.cb_top_label[r]; o.cb_top_conf[k] = t.cb_top_conf[r];
        o.cb_min_db[k] = t.cb_min_db[r]; o.cb_entropy[k] = t.cb_entropy[r];
    }
    if (tid == 0) host[0] = n_cb;
}

}  // namespace

// ---- the folds' launches (classify_internal.hpp): four clips per workgroup of K6b, one workgroup per clip of K6b-e, one workgroup of 1024 for
// either compaction
namespace wsa_classify {

template <typename P>
void launch_fold(const FoldParams<P>& f, uint32_t* cb_off, int32_t* cb, int32_t* cb_label, double* cb_conf, uint32_t* host, hipStream_t s) {
    if (f.n_clips) hipLaunchKernelGGL(fold_kernel<P>, dim3((f.n_clips + 3) / 4), dim3(256), 0, s, f);
    hipLaunchKernelGGL(fold_compact_kernel, dim3(1), dim3(1024), 0, s, f.n_clips, f.row_off, f.meta, f.clip_cb, cb_off,
                       f.t_label, f.t_conf, f.t_n, f.t_local, cb, cb_label, cb_conf, host);
}
template void launch_fold<float>(const FoldParams<float>&, uint32_t*, int32_t*, int32_t*, double*, uint32_t*, hipStream_t);
template void launch_fold<double>(const FoldParams<double>&, uint32_t*, int32_t*, int32_t*, double*, uint32_t*, hipStream_t);

void launch_fold_group(const FoldGroupParams& f, uint32_t* cb_off, const EnsTables& o, uint32_t* host, hipStream_t s) {
    if (f.n_clips) hipLaunchKernelGGL(fold_group_kernel, dim3(f.n_clips), dim3(64 * f.n_members), 0, s, f);
    hipLaunchKernelGGL(fold_compact_group_kernel, dim3(1), dim3(1024), 0, s, f.n_clips, f.n_members, f.row_off, f.meta, f.clip_cb, cb_off,
                       f.t_n, f.t_local, f.tab, f.t, o, host);
}

}  // namespace wsa_classify

namespace {

// ---- the host side
// the rows a batch hands K6: the row table (levels 5 and 13; level 12 at its stride of WSA_NFEAT, slots 0 .. 22, slot 23 the throw mark)
// or the utterance table (level 11); both counts sit on the device
ClsParams batch_params(const wsa_batch_view& v, const wsa_model* m, float* prob) {
    ClsParams p = cls_params(m, v.d_feat, 0, v.d_row_off + v.n_clips, prob);
    if (v.level == 11) { p.feat = v.d_utt_feat; p.d_n_rows = v.d_utt_off + v.n_clips; }
    if (v.level == 12) { p.stride = WSA_NFEAT; p.nan_slot = L12_NCOEF; }
    return p;
}

// every pairing of a batch's level and a model's input count but 5 / 13 with 53, 11 with 264 and 12 with 23 is refused
wsa_status batch_pairing_check(wsa_ctx* ctx, const char* entry, int level, const wsa_model* m) {
    const int have = wsa_level_feature_count(level);
    if (have == m->nin) return WSA_OK;
    const char* levels = m->nin == WSA_NUTT ? "output_level 11 (utterance features)" : m->nin == L12_NCOEF ? "output_level 12 (syllable coefficients)"
                                            : "output_level 5 (segment features) or 13 (syllable features)";
    return fail(ctx, WSA_ERR_INVALID, std::string(entry) + " needs a batch at " + levels + ", not " + std::to_string(level) + ": the model takes " + std::to_string(m->nin)
                                      + " inputs" + (have ? ", the rows of output_level " + std::to_string(level) + " have " + std::to_string(have) + " features" : std::string())
                                      + " (264-input models go with output_level 11, 23-input models with output_level 12)");
}

wsa_status enqueue_batch(const wsa_batch_view& v, wsa_cls* c, const wsa_model* m, hipStream_t s) {
    wsa_ctx* ctx = v.ctx;
    const uint32_t cap = v.level == 11 ? v.utt_cap : v.rows_cap;
    if (*v.cls_last == 3) {                       // wsa_batch_regress: no fold, no per-callback decision
        launch_classify(m, regress_params(batch_params(v, m, nullptr), c->d_value, c->out_min, c->out_span), cap, s);
        HIP_TRY(ctx, hipGetLastError());
        return WSA_OK;
    }
    launch_classify(m, batch_params(v, m, c->d_prob), cap, s);
    HIP_TRY(ctx, hipGetLastError());
    if (v.level == 13) {
        FoldParams<float> f{};
        f.n_clips = v.n_clips; f.C = (uint32_t)m->C; f.step_s = ctx->cfg.window_step / 1e3;
        f.meta = v.d_meta; f.row_off = v.d_row_off; f.prob = c->d_prob; f.key_rank = m->d_key_rank;
        f.t_label = c->d_t_label; f.t_conf = c->d_t_conf; f.t_n = c->d_t_n; f.t_local = c->d_t_local;
        f.clip_cb = c->d_clip_cb; f.clip_conf = c->d_clip_conf;
        launch_fold(f, c->d_cb_off, c->d_cb, c->d_cb_label, c->d_cb_conf, c->h_count_dev, s);
        HIP_TRY(ctx, hipGetLastError());
    }
    return WSA_OK;
}

wsa_status ecls_create(const wsa_batch_view& v, const wsa_ensemble* e, wsa_ecls** out) {
    wsa_ctx* ctx = v.ctx;
    wsa_ecls* c = new wsa_ecls();
    c->device = ctx->device; c->ens = e; c->serial = e->serial; c->n = e->n; c->n_clips = v.n_clips; c->lds = e->lds_batch;
    const size_t R = v.rows_cap ? v.rows_cap : 1;
    wsa::DevArena& A = c->mem;
    bool ok = A.alloc(&c->d_t_n, R) && A.alloc(&c->d_t_local, R) && A.alloc(&c->d_clip_cb, (size_t)v.n_clips) && A.alloc(&c->d_cb_off, (size_t)v.n_clips)
              && alloc_ens_tables(A, c->o, R, v.n_clips) && alloc_ens_tables(A, c->t, R, 0, true) && A.pin(&c->h_count, &c->h_count_dev, 4);
    c->t.clip_min_db = c->o.clip_min_db;
    for (uint32_t d = 0; d < e->n && ok; d++) {
        const wsa_model* m = e->m[d];
        FoldMember& f = c->fm[d];
        c->C[d] = (uint32_t)m->C;
        ok = A.alloc(&c->d_prob[d], R * m->C) && A.alloc(&f.t_label, R) && A.alloc(&f.t_conf, R) && A.alloc(&f.t_all_max, R)
             && A.alloc(&f.clip_conf, (size_t)v.n_clips * m->C) && A.alloc(&f.cb_label, R) && A.alloc(&f.cb_conf, R)
             && A.alloc(&f.cb_all_max, R);
        f.C = (uint32_t)m->C; f.prob = c->d_prob[d]; f.key_rank = m->d_key_rank;
    }
    if (ok) {
        std::vector<ClsGroupEntry> tab;
        c->grid = group_table(e, v.d_feat, v.d_row_off + v.n_clips, c->d_prob, v.rows_cap, false, tab);
        std::vector<FoldMember> ftab(c->fm, c->fm + e->n);
        ok = A.upload(&c->d_ctab, tab) && A.upload(&c->d_ftab, ftab);
    }
    if (!ok) return alloc_failed(ctx, c);
    *out = c;
    return WSA_OK;
}

// K6e, then (level 13) K6b-e and its compaction with the decision: three launches whatever the number of members
wsa_status enqueue_batch_ensemble(const wsa_batch_view& v, wsa_ecls* c, hipStream_t s) {
    wsa_ctx* ctx = v.ctx;
    launch_classify_group(c->d_ctab, c->n, v.d_row_off + v.n_clips, c->grid, c->lds, s);
    HIP_TRY(ctx, hipGetLastError());
    if (v.level == 13) {
        FoldGroupParams f{};
        f.n_clips = v.n_clips; f.n_members = c->n; f.step_s = ctx->cfg.window_step / 1e3;
        f.meta = v.d_meta; f.row_off = v.d_row_off; f.tab = c->d_ftab; f.t_n = c->d_t_n; f.t_local = c->d_t_local; f.clip_cb = c->d_clip_cb; f.t = c->t;
        launch_fold_group(f, c->d_cb_off, c->o, c->h_count_dev, s);
        HIP_TRY(ctx, hipGetLastError());
    }
    return WSA_OK;
}

// What every result function does first: the batch's counters; if fetching them reran the back end with the full tracker table, the rows
// are classified again (c: one model's or a regression's state, else ec: an ensemble's); then the stream is drained and the counts are read.
wsa_status settle_batch(wsa_batch* b, wsa_batch_view& v, hipStream_t s, wsa_cls* c, wsa_ecls* ec, wsa_device_result& r) {
    wsa_status st = wsa_batch_fetch_internal(b, s);
    if (st != WSA_OK) return st;
    wsa_batch_view_internal(b, &v);
    uint32_t& reruns = c ? c->reruns : ec->reruns;
    if (v.reruns != reruns) {
        reruns = v.reruns;
        st = c ? enqueue_batch(v, c, c->model, s) : enqueue_batch_ensemble(v, ec, s);
        if (st != WSA_OK) return st;
    }
    HIP_TRY(v.ctx, hipStreamSynchronize(s));
    return wsa_batch_result(b, s, &r);
}

// queues one table's copy to the caller's buffer unless an earlier one failed (st); nothing to do without a destination, a source or entries
template <typename T>
void copy_out(wsa_status& st, wsa_ctx* ctx, T* to, const T* from, size_t count, hipStream_t s) {
    if (st != WSA_OK || !to || !from || !count) return;
    const hipError_t e = hipMemcpyAsync(to, from, count * sizeof(T), hipMemcpyDefault, s);
    if (e != hipSuccess) st = fail(ctx, WSA_ERR_HIP, std::string("hipMemcpyAsync: ") + hipGetErrorString(e));
}

}  // namespace

extern "C" {

wsa_status wsa_batch_classify(wsa_batch* b, const wsa_model* m, void* stream) {
    if (!b || !m) return WSA_ERR_INVALID;
    wsa_batch_view v;
    wsa_batch_view_internal(b, &v);
    wsa_ctx* ctx = v.ctx;
    if (const wsa_status st = batch_pairing_check(ctx, "wsa_batch_classify", v.level, m)) return st;
    if (const wsa_status st = pairing_check(ctx, nullptr, ON_BATCH, v.level, ONE_MODEL, m->ctx, m->nin, m->softmax)) return st;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    wsa_cls*& c = *v.cls;
    if (!c || c->cap_c < (uint32_t)m->C) {        // first call (or a model of more classes): the only allocation of this path
        wsa_cls* n = new wsa_cls();
        n->device = ctx->device; n->cap_rows = v.rows_cap; n->cap_c = (uint32_t)m->C; n->n_clips = v.n_clips;
        const uint32_t cap = v.level == 11 ? v.utt_cap : v.rows_cap;           // level 11: one output row per utterance row
        const size_t R = cap ? cap : 1;
        wsa::DevArena& A = n->mem;
        bool ok = A.alloc(&n->d_prob, R * m->C) && A.alloc(&n->d_t_label, R) && A.alloc(&n->d_t_conf, R)
                  && A.alloc(&n->d_t_n, R) && A.alloc(&n->d_t_local, R) && A.alloc(&n->d_cb, R * 4)
                  && A.alloc(&n->d_cb_label, R) && A.alloc(&n->d_cb_conf, R)
                  && A.alloc(&n->d_clip_conf, (size_t)v.n_clips * m->C) && A.alloc(&n->d_clip_cb, (size_t)v.n_clips)
                  && A.alloc(&n->d_cb_off, (size_t)v.n_clips);
        ok = ok && A.pin(&n->h_count, &n->h_count_dev, 4);
        if (!ok) return alloc_failed(ctx, n);
        wsa_cls_free(c);
        c = n;
    }
    *v.cls_last = 1;
    c->model = m; c->level = v.level; c->n_classes = m->C; c->reruns = v.reruns; c->done = true;
    return enqueue_batch(v, c, m, reinterpret_cast<hipStream_t>(stream));
}

wsa_status wsa_batch_class_result(wsa_batch* b, void* stream, wsa_class_result* out) {
    if (!b || !out) return WSA_ERR_INVALID;
    wsa_batch_view v;
    wsa_batch_view_internal(b, &v);
    wsa_ctx* ctx = v.ctx;
    wsa_cls* c = *v.cls;
    if (!c || !c->done) return fail(ctx, WSA_ERR_INVALID, "no wsa_batch_classify on this batch yet");
    if (*v.cls_last == 3) return fail(ctx, WSA_ERR_INVALID, "the batch's last model call was wsa_batch_regress: its values are wsa_batch_copy_values'");
    if (*v.cls_last == 4) return fail(ctx, WSA_ERR_INVALID, "the batch's last model call was wsa_batch_regress_group: its tables are wsa_batch_value_result's");
    if (*v.cls_last != 1) return fail(ctx, WSA_ERR_INVALID, "the batch's last classification was an ensemble's: its tables are wsa_batch_ensemble_result's");
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    wsa_device_result r;
    if (const wsa_status st = settle_batch(b, v, s, c, nullptr, r)) return st;
    out->n_rows = c->level == 11 ? r.n_utterance_rows : r.n_rows; out->n_classes = (uint32_t)c->n_classes; out->n_clips = v.n_clips;
    out->d_prob = c->d_prob;
    const bool fold = c->level == 13;
    out->n_callbacks = fold ? ((const volatile uint32_t*)c->h_count)[0] : 0u;
    out->d_cb = fold ? c->d_cb : nullptr; out->d_cb_label = fold ? c->d_cb_label : nullptr;
    out->d_cb_conf = fold ? c->d_cb_conf : nullptr; out->d_clip_conf = fold ? c->d_clip_conf : nullptr;
    return WSA_OK;
}

wsa_status wsa_batch_copy_classes(wsa_batch* b, void* stream, float* prob, uint32_t rows_cap, int32_t* cb, int32_t* cb_label, double* cb_conf,
                                  uint32_t cb_cap, double* clip_conf) {
    if (!b) return WSA_ERR_INVALID;
    wsa_class_result r;
    wsa_status st = wsa_batch_class_result(b, stream, &r);
    if (st != WSA_OK) return st;
    wsa_batch_view v;
    wsa_batch_view_internal(b, &v);
    wsa_ctx* ctx = v.ctx;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (prob && rows_cap < r.n_rows) return fail(ctx, WSA_ERR_INVALID, "probability buffer too small");
    if ((cb || cb_label || cb_conf) && cb_cap < r.n_callbacks) return fail(ctx, WSA_ERR_INVALID, "callback buffer too small");
    const size_t K = r.n_callbacks;
    copy_out(st, ctx, prob, r.d_prob, (size_t)r.n_rows * r.n_classes, s);
    copy_out(st, ctx, cb, r.d_cb, K * 4, s);
    copy_out(st, ctx, cb_label, r.d_cb_label, K, s);
    copy_out(st, ctx, cb_conf, r.d_cb_conf, K, s);
    copy_out(st, ctx, clip_conf, r.d_clip_conf, (size_t)r.n_clips * r.n_classes, s);
    if (st != WSA_OK) return st;
    HIP_TRY(ctx, hipStreamSynchronize(s));
    return WSA_OK;
}

wsa_status wsa_batch_regress(wsa_batch* b, const wsa_model* m, double out_min, double out_max, void* stream) {
    if (!b || !m) return WSA_ERR_INVALID;
    wsa_batch_view v;
    wsa_batch_view_internal(b, &v);
    wsa_ctx* ctx = v.ctx;
    if (const wsa_status st = batch_pairing_check(ctx, "wsa_batch_regress", v.level, m)) return st;
    if (m->ctx != ctx) return fail(ctx, WSA_ERR_INVALID, "the model was created on another context (or device) than the batch");
    if (const char* why = regress_refusal(m, out_min, out_max)) return fail(ctx, WSA_ERR_INVALID, why);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    wsa_cls*& c = *v.cls;
    if (!c) { c = new wsa_cls(); c->device = ctx->device; c->cap_rows = v.rows_cap; c->n_clips = v.n_clips; }   // cap_c 0: a later classify builds its own tables
    const uint32_t cap = v.level == 11 ? v.utt_cap : v.rows_cap;
    if (!c->d_value && !c->mem.alloc(&c->d_value, cap ? cap : 1))                   // first call: the only allocation of this path
        return alloc_failed(ctx);
    *v.cls_last = 3;
    c->model = m; c->level = v.level; c->n_classes = 1; c->reruns = v.reruns; c->done = true;
    c->out_min = out_min; c->out_span = out_max - out_min;
    return enqueue_batch(v, c, m, reinterpret_cast<hipStream_t>(stream));
}

wsa_status wsa_batch_copy_values(wsa_batch* b, void* stream, double* value, uint32_t rows_cap, uint32_t* n_rows) {
    if (!b) return WSA_ERR_INVALID;
    wsa_batch_view v;
    wsa_batch_view_internal(b, &v);
    wsa_ctx* ctx = v.ctx;
    wsa_cls* c = *v.cls;
    if (!c || !c->done || *v.cls_last != 3) return fail(ctx, WSA_ERR_INVALID, "the batch's last model call was not wsa_batch_regress");
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    wsa_device_result r;
    if (const wsa_status st = settle_batch(b, v, s, c, nullptr, r)) return st;
    const uint32_t rows = c->level == 11 ? r.n_utterance_rows : r.n_rows;
    if (n_rows) *n_rows = rows;
    if (value && rows_cap < rows) return fail(ctx, WSA_ERR_INVALID, "value buffer too small");
    if (value && rows) {
        HIP_TRY(ctx, hipMemcpyAsync(value, c->d_value, (size_t)rows * sizeof(double), hipMemcpyDefault, s));
        HIP_TRY(ctx, hipStreamSynchronize(s));
    }
    return WSA_OK;
}

wsa_status wsa_batch_classify_ensemble(wsa_batch* b, const wsa_ensemble* e, void* stream) {
    if (!b || !e) return WSA_ERR_INVALID;
    wsa_batch_view v;
    wsa_batch_view_internal(b, &v);
    wsa_ctx* ctx = v.ctx;
    if (const wsa_status st = pairing_check(ctx, "wsa_batch_classify_ensemble", ON_BATCH, v.level, AN_ENSEMBLE, e->ctx, WSA_NFEAT, e->softmax)) return st;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    wsa_ecls*& c = *v.ecls;
    if (!c || c->ens != e || c->serial != e->serial) {     // first call with this ensemble: the only allocation of this path
        wsa_ecls* n = nullptr;
        const wsa_status st = ecls_create(v, e, &n);
        if (st != WSA_OK) return st;
        wsa_ecls_free(c);
        c = n;
    }
    *v.cls_last = 2;
    c->level = v.level; c->reruns = v.reruns;
    return enqueue_batch_ensemble(v, c, reinterpret_cast<hipStream_t>(stream));
}

wsa_status wsa_batch_ensemble_result(wsa_batch* b, void* stream, wsa_ensemble_result* out) {
    if (!b || !out) return WSA_ERR_INVALID;
    wsa_batch_view v;
    wsa_batch_view_internal(b, &v);
    wsa_ctx* ctx = v.ctx;
    wsa_ecls* ec = *v.ecls;
    if (!ec) return fail(ctx, WSA_ERR_INVALID, "no wsa_batch_classify_ensemble on this batch yet");
    if (*v.cls_last == 4) return fail(ctx, WSA_ERR_INVALID, "the batch's last model call was wsa_batch_regress_group: its tables are wsa_batch_value_result's");
    if (*v.cls_last != 2) return fail(ctx, WSA_ERR_INVALID, "the batch's last classification was one model's: its tables are wsa_batch_class_result's");
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    wsa_device_result r;
    if (const wsa_status st = settle_batch(b, v, s, nullptr, ec, r)) return st;
    std::memset(out, 0, sizeof(*out));
    const bool fold = ec->level == 13;
    out->n_rows = r.n_rows; out->n_members = ec->n; out->n_clips = v.n_clips;
    out->n_callbacks = fold ? ((const volatile uint32_t*)ec->h_count)[0] : 0u;
    for (uint32_t d = 0; d < ec->n; d++) {
        out->n_classes[d] = ec->C[d]; out->d_prob[d] = ec->d_prob[d];
        if (!fold) continue;
        out->d_cb_label[d] = ec->fm[d].cb_label; out->d_cb_conf[d] = ec->fm[d].cb_conf; out->d_cb_all_max[d] = ec->fm[d].cb_all_max;
        out->d_clip_conf[d] = ec->fm[d].clip_conf;
    }
    if (fold) {
        out->d_cb = ec->o.cb; out->d_cb_db = ec->o.cb_db; out->d_cb_top_label = ec->o.cb_top_label; out->d_cb_top_conf = ec->o.cb_top_conf;
        out->d_cb_min_db = ec->o.cb_min_db; out->d_cb_entropy = ec->o.cb_entropy; out->d_clip_min_db = ec->o.clip_min_db;
    }
    return WSA_OK;
}

wsa_status wsa_batch_copy_ensemble(wsa_batch* b, void* stream, const wsa_ensemble_host* dst) {
    if (!b || !dst) return WSA_ERR_INVALID;
    wsa_ensemble_result r;
    wsa_status st = wsa_batch_ensemble_result(b, stream, &r);
    if (st != WSA_OK) return st;
    wsa_batch_view v;
    wsa_batch_view_internal(b, &v);
    wsa_ctx* ctx = v.ctx;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    bool any_prob = false, any_cb = dst->cb || dst->cb_db || dst->cb_top_label || dst->cb_top_conf || dst->cb_min_db || dst->cb_entropy;
    for (uint32_t d = 0; d < r.n_members; d++) { any_prob = any_prob || dst->prob[d]; any_cb = any_cb || dst->cb_label[d] || dst->cb_conf[d] || dst->cb_all_max[d]; }
    if (any_prob && dst->rows_cap < r.n_rows) return fail(ctx, WSA_ERR_INVALID, "probability buffer too small");
    if (any_cb && dst->cb_cap < r.n_callbacks) return fail(ctx, WSA_ERR_INVALID, "callback buffer too small");
    const size_t K = r.n_callbacks;
    for (uint32_t d = 0; d < r.n_members; d++) {
        copy_out(st, ctx, dst->prob[d], r.d_prob[d], (size_t)r.n_rows * r.n_classes[d], s);
        copy_out(st, ctx, dst->cb_label[d], r.d_cb_label[d], K, s);
        copy_out(st, ctx, dst->cb_conf[d], r.d_cb_conf[d], K, s);
        copy_out(st, ctx, dst->cb_all_max[d], r.d_cb_all_max[d], K, s);
        copy_out(st, ctx, dst->clip_conf[d], r.d_clip_conf[d], (size_t)r.n_clips * r.n_classes[d], s);
    }
    copy_out(st, ctx, dst->cb, r.d_cb, K * 4, s);
    copy_out(st, ctx, dst->cb_db, r.d_cb_db, K, s);
    copy_out(st, ctx, dst->cb_top_label, r.d_cb_top_label, K, s);
    copy_out(st, ctx, dst->cb_top_conf, r.d_cb_top_conf, K, s);
    copy_out(st, ctx, dst->cb_min_db, r.d_cb_min_db, K, s);
    copy_out(st, ctx, dst->cb_entropy, r.d_cb_entropy, K, s);
    copy_out(st, ctx, dst->clip_min_db, r.d_clip_min_db, (size_t)r.n_clips, s);
    if (st != WSA_OK) return st;
    HIP_TRY(ctx, hipStreamSynchronize(s));
    return WSA_OK;
}

}  // extern "C"
