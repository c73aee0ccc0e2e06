// regress_fold.hip — regression groups (include/wsa.h "Regression groups", specification RG-1 of DESIGN.md §3): 1 .. 8 regression heads
// (the app's ords_<label> models for V, A and D) through ONE grouped K6 launch (classify.hip's classify_group_kernel with the regression
// epilogue), and the fold RG-1 (regress_fold.hpp) behind it: on a batch one wave per clip and a compaction (wsa_batch_regress_group),
// inside a stream object's step one wave per stream with the running sums carried on the device (wsa_stream_set_regress).
// classify.hip owns the models and K6; batch_run.hip and stream_step.hip run the batch and the stream object's step and capture these launches.
#include <atomic>
#include <cstring>
#include <string>
#include <vector>
#include "regress_internal.hpp"
#include "regress_fold.hpp"

using wsa_api::fail;
using namespace wsa_classify;
using namespace wsa_regress;

namespace {

// ---- RG-1 on a batch
__global__ void __launch_bounds__(64) regress_fold_kernel(RegressFoldParams p) {
    __shared__ double s_terms[RG_LDS];
    const int lane = threadIdx.x;
    const uint32_t clip = blockIdx.x;
    const uint32_t r0 = p.row_off[clip], r1 = p.row_off[clip + 1];
    const bool head = (uint32_t)lane < p.H;
    double A = 0.0, B = 0.0;
    const uint32_t ncb = regress_walk(p.meta, p.value, p.H, p.step_s, lane, r0, r1, s_terms, p.t_n, A, B,
        [&](uint32_t first, uint32_t rows, uint32_t local, bool, double v, double w) {
            if (head) { p.t_value[(size_t)lane * p.stride + first] = v; p.t_weight[(size_t)lane * p.stride + first] = w; }
            if (lane == 0) { p.t_n[first] = (int32_t)rows; p.t_local[first] = (int32_t)local; }
        });
    if (head) {
        const size_t at = (size_t)lane * p.n_clips + clip;
        p.clip_sum[at] = A; p.clip_weight[at] = B; p.clip_value[at] = B == 0.0 ? nan_d() : A / B;
    }
    if (lane == 0) p.clip_cb[clip] = ncb;
}

// the offsets, then every callback's record and its heads' figures from the row it starts at; the count goes to the host's mapped word
__global__ void __launch_bounds__(1024) regress_compact_kernel(RegressFoldParams p) {
    __shared__ uint32_t s_part[1024];
    __shared__ uint32_t s_base;
    const int tid = threadIdx.x;
    const uint32_t n_cb = compact_offsets(p.n_clips, p.clip_cb, p.cb_off, s_part, &s_base);
    const uint32_t n_rows = p.row_off[p.n_clips];
    __syncthreads();
    for (uint32_t r = tid; r < n_rows; r += 1024) {
        const int32_t nsyl = p.t_n[r];
        if (nsyl <= 0) continue;
        const int32_t clip = p.meta[(size_t)r * 8];
        const uint32_t k = p.cb_off[clip] + (uint32_t)p.t_local[r];
        write_callback(p.cb, k, clip, p.meta[(size_t)r * 8 + 1], r, nsyl);
        for (uint32_t h = 0; h < p.H; h++) {
            p.cb_value[(size_t)h * p.stride + k] = p.t_value[(size_t)h * p.stride + r];
            p.cb_weight[(size_t)h * p.stride + k] = p.t_weight[(size_t)h * p.stride + r];
        }
    }
    if (tid == 0) p.host[0] = n_cb;
}

// ---- RG-1 on a stream step
__global__ void __launch_bounds__(64) regress_step_kernel(RegressStepParams p) {
    __shared__ double s_terms[RG_LDS];
    const int lane = threadIdx.x;
    const uint32_t s = blockIdx.x;
    const uint32_t r0 = p.row_off[s], r1 = p.row_off[s + 1];
    const uint32_t pe = r1 < p.cap ? r1 : p.cap;                   // the rows' values below the D2H window
    for (uint32_t h = 0; h < p.H; h++)
        for (uint32_t i = r0 + lane; i < pe; i += 64) p.h_value[(size_t)h * p.cap + i] = p.value[h][i];
    if (!p.fold) return;
    const bool head = (uint32_t)lane < p.H;
    const size_t at = (size_t)lane * p.n + s;
    double A = 0.0, B = 0.0;
    if (head && !(p.bits[s] & 1u)) { A = p.run_sum[at]; B = p.run_weight[at]; }
    const uint32_t k0 = callback_starts(p.meta, 0, r0, lane);
    const uint32_t ncb = regress_walk(p.meta, p.value, p.H, p.step_s, lane, r0, r1, s_terms, nullptr, A, B,
        [&](uint32_t first, uint32_t rows, uint32_t local, bool, double v, double w) {
            const uint32_t k = k0 + local;
            if (head) {
                p.cb_value[(size_t)lane * p.stride + k] = v; p.cb_weight[(size_t)lane * p.stride + k] = w;
                if (k < p.cap) { p.h_cb_value[(size_t)lane * p.cap + k] = v; p.h_cb_weight[(size_t)lane * p.cap + k] = w; }
            }
            if (lane == 0) {
                const int32_t si = p.meta[(size_t)first * 8 + 1];
                write_callback(p.cb, k, (int32_t)s, si, first, (int32_t)rows);
                if (k < p.cap) write_callback(p.h_cb, k, (int32_t)s, si, first, (int32_t)rows);
            }
        });
    if (head) {
        p.run_sum[at] = A; p.run_weight[at] = B;
        p.h_sum[at] = A; p.h_weight[at] = B; p.h_run_value[at] = B == 0.0 ? nan_d() : A / B;
    }
    if (lane == 0 && s == p.n - 1) p.h_count[0] = k0 + ncb;
}

std::atomic<uint64_t> g_serial{0};

// the grouped launch's table: the heads in work-list order, each with the row-block factor it gets (its own for batches, 1 in a stream
// step) and its value column; returns the grid, one workgroup per (head, tile) pair of rows_cap rows by classify_grid's rule
uint32_t regress_table(const wsa_regress_group* g, const double* feat, const uint32_t* d_n_rows, double* const* value, uint32_t rows_cap, bool one_block,
                       ClsGroupEntry* tab) {
    uint64_t tiles = 0;
    for (uint32_t i = 0; i < g->n; i++) {
        const int h = g->order[i];
        tab[i].p = regress_params(cls_params(g->m[h], feat, 0, d_n_rows, nullptr), value[h], g->out_min[h], g->out_span[h]);
        tab[i].rb = one_block ? 1 : g->m[h]->rb;
        tiles += (rows_cap + 16u * tab[i].rb - 1) / (16u * tab[i].rb);
    }
    return classify_grid(g->ctx, tiles);
}

}  // namespace

namespace wsa_regress {

void launch_regress_fold(const RegressFoldParams& p, hipStream_t s) {
    if (p.n_clips) hipLaunchKernelGGL(regress_fold_kernel, dim3(p.n_clips), dim3(64), 0, s, p);
    hipLaunchKernelGGL(regress_compact_kernel, dim3(1), dim3(1024), 0, s, p);
}
void launch_regress_step(const RegressStepParams& p, hipStream_t s) {
    if (p.n) hipLaunchKernelGGL(regress_step_kernel, dim3(p.n), dim3(64), 0, s, p);
}

}  // namespace wsa_regress

// ---- the tables of one batch, built for one group (the first wsa_batch_regress_group with it allocates them)
struct wsa_rcls {
    int device = 0;
    const wsa_regress_group* grp = nullptr; uint64_t serial = 0;
    uint32_t H = 0, n_clips = 0, reruns = 0, grid = 1, stride = 1; int level = 0;
    size_t lds = 0;
    double *d_value = nullptr, *d_t_value = nullptr, *d_t_weight = nullptr, *d_cb_value = nullptr, *d_cb_weight = nullptr;      // [H][stride]
    double *d_clip_sum = nullptr, *d_clip_weight = nullptr, *d_clip_value = nullptr;                                             // [H][n_clips]
    int32_t *d_t_n = nullptr, *d_t_local = nullptr, *d_cb = nullptr; uint32_t *d_clip_cb = nullptr, *d_cb_off = nullptr;
    ClsGroupEntry* d_ctab = nullptr;
    uint32_t *h_count = nullptr, *h_count_dev = nullptr;
    wsa::DevArena mem;
};

void wsa_rcls_free(wsa_rcls* c) { free_on_device(c); }

namespace {

wsa_status rcls_create(const wsa_batch_view& v, const wsa_regress_group* g, wsa_rcls** out) {
    wsa_ctx* ctx = v.ctx;
    wsa_rcls* c = new wsa_rcls();
    c->device = ctx->device; c->grp = g; c->serial = g->serial; c->H = g->n; c->n_clips = v.n_clips; c->lds = g->lds_batch;
    const size_t R = v.rows_cap ? v.rows_cap : 1, H = g->n, N = v.n_clips;
    c->stride = (uint32_t)R;
    wsa::DevArena& A = c->mem;
    bool ok = A.alloc(&c->d_value, H * R);
    if (ok && v.level == 13)
        ok = A.alloc(&c->d_t_value, H * R) && A.alloc(&c->d_t_weight, H * R) && A.alloc(&c->d_cb_value, H * R) && A.alloc(&c->d_cb_weight, H * R)
             && A.alloc(&c->d_clip_sum, H * N) && A.alloc(&c->d_clip_weight, H * N) && A.alloc(&c->d_clip_value, H * N)
             && A.alloc(&c->d_t_n, R) && A.alloc(&c->d_t_local, R) && A.alloc(&c->d_cb, R * 4) && A.alloc(&c->d_clip_cb, N) && A.alloc(&c->d_cb_off, N)
             && A.pin(&c->h_count, &c->h_count_dev, 4);
    if (ok) {
        double* value[WSA_REGRESS_GROUP_MAX] = {};
        for (size_t h = 0; h < H; h++) value[h] = c->d_value + h * R;
        std::vector<ClsGroupEntry> tab(H);
        c->grid = regress_table(g, v.d_feat, v.d_row_off + v.n_clips, value, v.rows_cap, false, tab.data());
        ok = A.upload(&c->d_ctab, tab);
    }
    if (!ok) return alloc_failed(ctx, c);
    *out = c;
    return WSA_OK;
}

// the grouped K6, then (level 13) the fold and its compaction: three launches whatever the number of heads
wsa_status enqueue_batch_group(const wsa_batch_view& v, const wsa_rcls* c, hipStream_t s) {
    wsa_ctx* ctx = v.ctx;
    launch_classify_group(c->d_ctab, c->H, v.d_row_off + v.n_clips, c->grid, c->lds, s);
    HIP_TRY(ctx, hipGetLastError());
    if (c->level == 13) {
        RegressFoldParams p{};
        p.n_clips = v.n_clips; p.H = c->H; p.stride = c->stride; p.step_s = ctx->cfg.window_step / 1e3;
        p.meta = v.d_meta; p.row_off = v.d_row_off;
        for (uint32_t h = 0; h < c->H; h++) p.value[h] = c->d_value + (size_t)h * c->stride;
        p.t_value = c->d_t_value; p.t_weight = c->d_t_weight; p.t_n = c->d_t_n; p.t_local = c->d_t_local;
        p.clip_cb = c->d_clip_cb; p.cb_off = c->d_cb_off;
        p.clip_sum = c->d_clip_sum; p.clip_weight = c->d_clip_weight; p.clip_value = c->d_clip_value;
        p.cb = c->d_cb; p.cb_value = c->d_cb_value; p.cb_weight = c->d_cb_weight; p.host = c->h_count_dev;
        launch_regress_fold(p, s);
        HIP_TRY(ctx, hipGetLastError());
    }
    return WSA_OK;
}

template <typename T>
void copy_out(wsa_status& st, wsa_ctx* ctx, T* to, const T* from, size_t count, hipStream_t s) {
    if (st != WSA_OK || !to || !from || !count) return;
    const hipError_t e = hipMemcpyAsync(to, from, count * sizeof(T), hipMemcpyDefault, s);
    if (e != hipSuccess) st = fail(ctx, WSA_ERR_HIP, std::string("hipMemcpyAsync: ") + hipGetErrorString(e));
}

}  // namespace

extern "C" {

wsa_status wsa_regress_group_create(wsa_ctx* ctx, const wsa_model* const* models, const double* out_min, const double* out_max, uint32_t n,
                                    wsa_regress_group** out) {
    if (!ctx || !out) return fail(ctx, WSA_ERR_INVALID, "null argument");
    *out = nullptr;
    if (n < 1 || n > WSA_REGRESS_GROUP_MAX) return fail(ctx, WSA_ERR_INVALID, "a regression group has 1 .. 8 heads, got " + std::to_string(n));
    if (!models || !out_min || !out_max) return fail(ctx, WSA_ERR_INVALID, "null model / out_min / out_max array");
    for (uint32_t h = 0; h < n; h++) {
        const std::string who = "head " + std::to_string(h);
        if (!models[h]) return fail(ctx, WSA_ERR_INVALID, who + " is NULL");
        if (models[h]->ctx != ctx) return fail(ctx, WSA_ERR_INVALID, who + " was created on another context (or device) than the group");
        if (models[h]->nin != WSA_NFEAT)
            return fail(ctx, WSA_ERR_INVALID, who + " takes " + std::to_string(models[h]->nin) + " inputs: a regression group predicts from the 53-feature rows of output_level 5 and 13");
        if (const char* why = regress_refusal(models[h], out_min[h], out_max[h])) return fail(ctx, WSA_ERR_INVALID, who + ": " + why);
    }
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    wsa_regress_group* g = new wsa_regress_group();
    g->ctx = ctx; g->device = ctx->device; g->n = n; g->serial = ++g_serial;
    double cost[WSA_REGRESS_GROUP_MAX];
    for (uint32_t h = 0; h < n; h++) {
        const wsa_model* m = models[h];
        g->m[h] = m; g->out_min[h] = out_min[h]; g->out_span[h] = out_max[h] - out_min[h]; g->order[h] = (int)h;
        double w = 0.0;
        for (int l = 0; l < m->n_layers; l++) w += (double)m->L[l].kp * m->L[l].np;
        cost[h] = w * 16.0 * m->rb;                                // multiply-adds of one tile
        const size_t lb = (size_t)2 * 16 * m->rb * m->S * sizeof(float), ls = (size_t)2 * 16 * m->S * sizeof(float);
        g->lds_batch = lb > g->lds_batch ? lb : g->lds_batch; g->lds_stream = ls > g->lds_stream ? ls : g->lds_stream;
    }
    for (uint32_t i = 1; i < n; i++)                               // stable insertion sort, descending
        for (uint32_t j = i; j > 0 && cost[g->order[j]] > cost[g->order[j - 1]]; j--) { const int t = g->order[j]; g->order[j] = g->order[j - 1]; g->order[j - 1] = t; }
    wsa::DevArena& A = g->mem;
    // the table and, in the slot behind its last entry, the row count: one staging buffer, one device buffer, ONE copy per call
    ClsGroupEntry* tab_dev = nullptr;                                // (the staging is copied from, not read in place)
    if (!(A.pin(&g->h_tab, &tab_dev, (size_t)n + 1) && A.alloc(&g->d_tab, (size_t)n + 1)
          && hipEventCreateWithFlags(&g->done, hipEventDisableTiming) == hipSuccess)) {
        const wsa_status st = alloc_failed(ctx);
        wsa_regress_group_destroy(g);
        return st;
    }
    g->h_n = reinterpret_cast<uint32_t*>(g->h_tab + n); g->d_n = reinterpret_cast<uint32_t*>(g->d_tab + n);
    *out = g;
    return WSA_OK;
}

void wsa_regress_group_destroy(wsa_regress_group* g) {
    if (!g) return;
    (void)hipSetDevice(g->device);
    if (g->done) { (void)hipEventSynchronize(g->done); (void)hipEventDestroy(g->done); }
    delete g;
}

wsa_status wsa_regress_group_rows(wsa_regress_group* g, const double* d_feat, uint32_t n_rows, double* const* d_value, void* stream) {
    if (!g) return WSA_ERR_INVALID;
    wsa_ctx* ctx = g->ctx;
    if (!d_value) return fail(ctx, WSA_ERR_INVALID, "null value pointer array");
    for (uint32_t h = 0; h < g->n; h++)
        if (n_rows && !d_value[h]) return fail(ctx, WSA_ERR_INVALID, "null value pointer of head " + std::to_string(h));
    if (n_rows && !d_feat) return fail(ctx, WSA_ERR_INVALID, "null feature pointer");
    if (!n_rows) return WSA_OK;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    HIP_TRY(ctx, hipEventSynchronize(g->done));                    // the previous call's launch has read the table
    const uint32_t grid = regress_table(g, d_feat, g->d_n, d_value, n_rows, false, g->h_tab);
    g->h_n[0] = n_rows;
    HIP_TRY(ctx, hipMemcpyAsync(g->d_tab, g->h_tab, ((size_t)g->n + 1) * sizeof(ClsGroupEntry), hipMemcpyHostToDevice, s));
    launch_classify_group(g->d_tab, g->n, g->d_n, grid, g->lds_batch, s);
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipEventRecord(g->done, s));
    return WSA_OK;
}

wsa_status wsa_batch_regress_group(wsa_batch* b, const wsa_regress_group* g, void* stream) {
    if (!b || !g) return WSA_ERR_INVALID;
    wsa_batch_view v;
    wsa_batch_view_internal(b, &v);
    wsa_ctx* ctx = v.ctx;
    if (v.level != 5 && v.level != 13)
        return fail(ctx, WSA_ERR_INVALID, "wsa_batch_regress_group needs a batch at output_level 5 (segment features) or 13 (syllable features), not " + std::to_string(v.level));
    if (g->ctx != ctx) return fail(ctx, WSA_ERR_INVALID, "the regression group was created on another context (or device) than the batch");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    wsa_rcls*& c = *v.rcls;
    if (!c || c->grp != g || c->serial != g->serial) {             // first call with this group: the only allocation of this path
        wsa_rcls* n = nullptr;
        const wsa_status st = rcls_create(v, g, &n);
        if (st != WSA_OK) return st;
        wsa_rcls_free(c);
        c = n;
    }
    *v.cls_last = 4;
    c->level = v.level; c->reruns = v.reruns;
    return enqueue_batch_group(v, c, reinterpret_cast<hipStream_t>(stream));
}

wsa_status wsa_batch_value_result(wsa_batch* b, void* stream, wsa_value_result* out) {
    if (!b || !out) return WSA_ERR_INVALID;
    wsa_batch_view v;
    wsa_batch_view_internal(b, &v);
    wsa_ctx* ctx = v.ctx;
    wsa_rcls* c = *v.rcls;
    if (!c) return fail(ctx, WSA_ERR_INVALID, "no wsa_batch_regress_group on this batch yet");
    if (*v.cls_last != 4) return fail(ctx, WSA_ERR_INVALID, "the batch's last model call was not wsa_batch_regress_group");
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    // the batch's counters; if fetching them reran the back end with the full tracker table, the new rows go through the group again
    wsa_status st = wsa_batch_fetch_internal(b, s);
    if (st != WSA_OK) return st;
    wsa_batch_view_internal(b, &v);
    if (v.reruns != c->reruns) {
        c->reruns = v.reruns;
        if ((st = enqueue_batch_group(v, c, s)) != WSA_OK) return st;
    }
    HIP_TRY(ctx, hipStreamSynchronize(s));
    wsa_device_result r;
    if ((st = wsa_batch_result(b, s, &r)) != WSA_OK) return st;
    std::memset(out, 0, sizeof(*out));
    const bool fold = c->level == 13;
    out->n_rows = r.n_rows; out->n_heads = c->H; out->n_clips = v.n_clips;
    out->n_callbacks = fold ? ((const volatile uint32_t*)c->h_count)[0] : 0u;
    for (uint32_t h = 0; h < c->H; h++) {
        out->d_value[h] = c->d_value + (size_t)h * c->stride;
        if (!fold) continue;
        out->d_cb_value[h] = c->d_cb_value + (size_t)h * c->stride; out->d_cb_weight[h] = c->d_cb_weight + (size_t)h * c->stride;
        out->d_clip_sum[h] = c->d_clip_sum + (size_t)h * v.n_clips; out->d_clip_weight[h] = c->d_clip_weight + (size_t)h * v.n_clips;
        out->d_clip_value[h] = c->d_clip_value + (size_t)h * v.n_clips;
    }
    out->d_cb = fold ? c->d_cb : nullptr;
    return WSA_OK;
}

wsa_status wsa_batch_copy_value_fold(wsa_batch* b, void* stream, const wsa_value_host* dst) {
    if (!b || !dst) return WSA_ERR_INVALID;
    wsa_value_result r;
    wsa_status st = wsa_batch_value_result(b, stream, &r);
    if (st != WSA_OK) return st;
    wsa_batch_view v;
    wsa_batch_view_internal(b, &v);
    wsa_ctx* ctx = v.ctx;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    bool any_value = false, any_cb = dst->cb != nullptr;
    for (uint32_t h = 0; h < r.n_heads; h++) { any_value = any_value || dst->value[h]; any_cb = any_cb || dst->cb_value[h] || dst->cb_weight[h]; }
    if (any_value && dst->rows_cap < r.n_rows) return fail(ctx, WSA_ERR_INVALID, "value buffer too small");
    if (any_cb && dst->cb_cap < r.n_callbacks) return fail(ctx, WSA_ERR_INVALID, "callback buffer too small");
    const size_t K = r.n_callbacks;
    for (uint32_t h = 0; h < r.n_heads; h++) {
        copy_out(st, ctx, dst->value[h], r.d_value[h], (size_t)r.n_rows, s);
        copy_out(st, ctx, dst->cb_value[h], r.d_cb_value[h], K, s);
        copy_out(st, ctx, dst->cb_weight[h], r.d_cb_weight[h], K, s);
        copy_out(st, ctx, dst->clip_sum[h], r.d_clip_sum[h], (size_t)r.n_clips, s);
        copy_out(st, ctx, dst->clip_weight[h], r.d_clip_weight[h], (size_t)r.n_clips, s);
        copy_out(st, ctx, dst->clip_value[h], r.d_clip_value[h], (size_t)r.n_clips, s);
    }
    copy_out(st, ctx, dst->cb, r.d_cb, K * 4, s);
    if (st != WSA_OK) return st;
    HIP_TRY(ctx, hipStreamSynchronize(s));
    return WSA_OK;
}

}  // extern "C"

// ---- streams (wsa_stream_set_regress): the grouped K6 on every step's rows, RG-1 carried per (stream, head) at level 13; everything
// allocated at attach time
struct wsa_sreg {
    int device = 0;
    const wsa_regress_group* grp = nullptr;
    wsa_scls_view v{};
    uint32_t H = 0, grid = 1, stride = 1, cap = 1;
    size_t lds = 0;
    double *d_value = nullptr, *d_cb_value = nullptr, *d_cb_weight = nullptr, *d_run_sum = nullptr, *d_run_weight = nullptr; int32_t* d_cb = nullptr;
    ClsGroupEntry* d_ctab = nullptr;
    wsa::DevArena mem;
    double *h_value = nullptr, *h_value_dev = nullptr, *h_cb_value = nullptr, *h_cb_value_dev = nullptr, *h_cb_weight = nullptr, *h_cb_weight_dev = nullptr;
    double *h_sum = nullptr, *h_sum_dev = nullptr, *h_weight = nullptr, *h_weight_dev = nullptr, *h_run_value = nullptr, *h_run_value_dev = nullptr;
    int32_t *h_cb = nullptr, *h_cb_dev = nullptr; uint32_t *h_count = nullptr, *h_count_dev = nullptr;
    std::vector<double> x_value[WSA_REGRESS_GROUP_MAX], x_cb_value[WSA_REGRESS_GROUP_MAX], x_cb_weight[WSA_REGRESS_GROUP_MAX]; std::vector<int32_t> x_cb;   // steps beyond the D2H window
};

void wsa_sreg_free(wsa_sreg* c) { free_on_device(c); }

wsa_status wsa_sreg_create(const wsa_scls_view& v, const wsa_regress_group* g, wsa_sreg** out) {
    wsa_ctx* ctx = v.ctx;
    *out = nullptr;
    if (v.level != 5 && v.level != 13)
        return fail(ctx, WSA_ERR_INVALID, "wsa_stream_set_regress needs streams at output_level 5 (segment features) or 13 (syllable features), not " + std::to_string(v.level));
    if (g->ctx != ctx) return fail(ctx, WSA_ERR_INVALID, "the regression group was created on another context (or device) than the streams");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    wsa_sreg* c = new wsa_sreg();
    c->device = ctx->device; c->grp = g; c->v = v; c->H = g->n; c->lds = g->lds_stream;
    const size_t R = v.rows_cap ? v.rows_cap : 1, W = v.d2h_rows ? v.d2h_rows : 1, H = g->n, N = v.n_streams;
    c->stride = (uint32_t)R; c->cap = v.d2h_rows;
    wsa::DevArena& A = c->mem;
    bool ok = A.alloc(&c->d_value, H * R) && A.pin(&c->h_value, &c->h_value_dev, H * W);
    if (ok && v.level == 13)
        ok = A.alloc(&c->d_cb_value, H * R) && A.alloc(&c->d_cb_weight, H * R) && A.alloc(&c->d_cb, R * 4)
             && A.alloc(&c->d_run_sum, H * N, true) && A.alloc(&c->d_run_weight, H * N, true)
             && A.pin(&c->h_cb_value, &c->h_cb_value_dev, H * W) && A.pin(&c->h_cb_weight, &c->h_cb_weight_dev, H * W) && A.pin(&c->h_cb, &c->h_cb_dev, W * 4)
             && A.pin(&c->h_sum, &c->h_sum_dev, H * N) && A.pin(&c->h_weight, &c->h_weight_dev, H * N) && A.pin(&c->h_run_value, &c->h_run_value_dev, H * N)
             && A.pin(&c->h_count, &c->h_count_dev, 4);
    if (ok) {
        // as one model's K6 in a step: tiles of 16 rows, and a grid that covers the D2H window in one pass (a larger step strides over its tiles)
        double* value[WSA_REGRESS_GROUP_MAX] = {};
        for (size_t h = 0; h < H; h++) value[h] = c->d_value + h * R;
        std::vector<ClsGroupEntry> tab(H);
        c->grid = regress_table(g, v.d_feat, v.d_totals, value, v.rows_cap < v.d2h_rows ? v.rows_cap : v.d2h_rows, true, tab.data());
        ok = A.upload(&c->d_ctab, tab);
    }
    ok = ok && hipDeviceSynchronize() == hipSuccess;
    if (!ok) return alloc_failed(ctx, c);
    *out = c;
    return WSA_OK;
}

// the grouped K6 on the step's compacted rows (count on the device), then the push / fold kernel: two kernel nodes of the captured step
wsa_status wsa_sreg_enqueue(wsa_sreg* c, hipStream_t s) {
    const wsa_scls_view& v = c->v;
    launch_classify_group(c->d_ctab, c->H, v.d_totals, c->grid, c->lds, s);
    HIP_TRY(v.ctx, hipGetLastError());
    RegressStepParams p{};
    p.n = v.n_streams; p.H = c->H; p.stride = c->stride; p.cap = c->cap; p.fold = v.level == 13 ? 1 : 0; p.step_s = v.ctx->cfg.window_step / 1e3;
    p.meta = v.d_meta; p.row_off = v.d_row_off; p.bits = v.d_bits;
    for (uint32_t h = 0; h < c->H; h++) p.value[h] = c->d_value + (size_t)h * c->stride;
    p.run_sum = c->d_run_sum; p.run_weight = c->d_run_weight; p.cb = c->d_cb; p.cb_value = c->d_cb_value; p.cb_weight = c->d_cb_weight;
    p.h_value = c->h_value_dev; p.h_cb = c->h_cb_dev; p.h_cb_value = c->h_cb_value_dev; p.h_cb_weight = c->h_cb_weight_dev;
    p.h_sum = c->h_sum_dev; p.h_weight = c->h_weight_dev; p.h_run_value = c->h_run_value_dev; p.h_count = c->h_count_dev;
    launch_regress_step(p, s);
    HIP_TRY(v.ctx, hipGetLastError());
    return WSA_OK;
}

// after the step has completed: the tables of `rows` rows; a step beyond the D2H window is fetched from the device here
wsa_status wsa_sreg_result(wsa_sreg* c, uint32_t rows, wsa_stream_value_result* o) {
    const wsa_scls_view& v = c->v;
    wsa_ctx* ctx = v.ctx;
    const bool fold = v.level == 13;
    const uint32_t ncb = fold ? ((const volatile uint32_t*)c->h_count)[0] : 0u;
    const size_t W = c->cap ? c->cap : 1;
    std::memset(o, 0, sizeof(*o));
    o->n_rows = rows; o->n_heads = c->H; o->n_callbacks = ncb; o->n_streams = v.n_streams;
    o->cb = fold ? c->h_cb : nullptr;
    for (uint32_t h = 0; h < c->H; h++) {
        o->value[h] = c->h_value + h * W;
        if (!fold) continue;
        o->cb_value[h] = c->h_cb_value + h * W; o->cb_weight[h] = c->h_cb_weight + h * W;
        o->stream_sum[h] = c->h_sum + (size_t)h * v.n_streams; o->stream_weight[h] = c->h_weight + (size_t)h * v.n_streams;
        o->stream_value[h] = c->h_run_value + (size_t)h * v.n_streams;
    }
    if (rows > v.d2h_rows) {
        HIP_TRY(ctx, hipSetDevice(ctx->device));
        wsa_status st = WSA_OK;
        for (uint32_t h = 0; h < c->H && st == WSA_OK; h++) {
            st = fetch_table(ctx, c->x_value[h], (const double*)c->d_value + (size_t)h * c->stride, rows, &o->value[h]);
            if (fold && st == WSA_OK) st = fetch_table(ctx, c->x_cb_value[h], (const double*)c->d_cb_value + (size_t)h * c->stride, ncb, &o->cb_value[h]);
            if (fold && st == WSA_OK) st = fetch_table(ctx, c->x_cb_weight[h], (const double*)c->d_cb_weight + (size_t)h * c->stride, ncb, &o->cb_weight[h]);
        }
        if (fold && st == WSA_OK) st = fetch_table(ctx, c->x_cb, (const int32_t*)c->d_cb, (size_t)ncb * 4, &o->cb);
        return st;
    }
    return WSA_OK;
}
