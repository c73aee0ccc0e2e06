// stream_featdb.hip — a stream step's rows appended to the device feature DB, inside the step (specification FD-2, DESIGN.md §3;
// include/wsa.h "Live streams collect into the device DB").  Two kernels of the step: the plan kernel — ONE workgroup applies the keep
// rule, scans, decides whether the step fits and leaves the copy list — and the copy kernel, whose grid is fixed at attach and which
// reads the row count from the device.  Nothing here does arithmetic on a feature: every stored value is the source's bits.
//
// Stands in for the reference APPLICATION's storing path as live sources reach it: src/index.js:35-100 (call_backed -> StoreFeatures),
// src/localstore.js:39-65 (an identity that is stored again replaces its vector: level 11 files every result under part 0).
#include <string>
#include <vector>
#include "api_internal.hpp"
#include "featdb_internal.hpp"
#include "featdb_keep.hpp"

using wsa_api::fail;
using wsa_fd::FD_ALL; using wsa_fd::FD_L12; using wsa_fd::FD_L11; using wsa_fd::FD_WAVE; using wsa_fd::FD_WAVES; using wsa_fd::FD_WG;

namespace {

constexpr int SF_COPY_THREADS = 256;
constexpr int SF_COPY_ROWS = 64;                          // stored rows per workgroup tile of the copy kernel
constexpr int SF_COPY_GRID = 64;                          // its grid is at most this: a step rarely stores more than a few tiles

struct SfPlan {
    int mode;
    const int32_t* meta; const uint64_t* feat; uint32_t stride;           // FD_L12: the step's row table
    const uint32_t* off; const uint32_t* bits; int32_t* slot; uint32_t n_streams;      // FD_L11: utterance offsets, control words, the DB row each stream owns (-1: none)
    const uint32_t* n_rows; uint32_t rows_cap;            // rows in the source table (FD_L11: utterance rows), and what it can hold
    const uint32_t *flags, *lost;                         // WSA_FLAG_CAPACITY: bit 0 of *flags, or *lost (may be NULL) nonzero
    const uint32_t* h_count; uint32_t capacity;           // mapped host word: the DB's count before this step
    uint32_t *src, *dst;                                  // the copy list: source row (FD_L12, FD_L11) and DB row (FD_L11) of every stored row
    uint32_t* plan;                                       // [2] = {rows the copy kernel moves, the first new DB row}
    uint32_t* h_push;                                     // mapped host words {first_row, n_added, n_replaced, not_fitted}
    int32_t *h_kept, *h_replaced;                         // mapped host lists (FD_L12, FD_L11)
};

// thread 0: the capacity decision of a step that would add `add` rows, the copy's two words and the four push words
__device__ __forceinline__ void sf_finish(const SfPlan& p, uint32_t count, uint32_t add, bool fits, uint32_t n_copy, uint32_t n_replaced) {
    p.plan[0] = fits ? n_copy : 0u; p.plan[1] = count;
    p.h_push[0] = count; p.h_push[1] = fits ? add : 0u; p.h_push[2] = fits ? n_replaced : 0u; p.h_push[3] = fits ? 0u : add;
    __threadfence_system();
}

// No workgroup waits on another and nothing is accumulated atomically: the order of the output is the source order whatever the device
// schedules.  Levels 5 / 13 walk nothing (every row is kept: the count is the decision); level 12 walks the rows FD_WG at a time with
// K10's rule (featdb_keep.hpp); level 11 walks the streams twice: the new rows are counted before a slot is handed out.
__global__ void __launch_bounds__(FD_WG) stream_featdb_plan_kernel(SfPlan p) {
    __shared__ wsa_fd::KeepShared sh;
    __shared__ uint32_t s_count, s_n, s_bad, s_new[FD_WAVES];
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (tid == 0) {
        s_count = *p.h_count;
        s_bad = (p.flags[0] & 1u) | ((p.lost && p.lost[0]) ? 1u : 0u);
        const uint32_t n = p.n_rows[0];
        s_n = s_bad ? 0u : (n < p.rows_cap ? n : p.rows_cap);
    }
    __syncthreads();
    const uint32_t count = s_count, n = s_n;
    const bool bad = s_bad != 0;
    if (p.mode == FD_ALL) {
        if (tid == 0) sf_finish(p, count, n, (uint64_t)count + n <= p.capacity, n, 0u);
        return;
    }
    if (p.mode == FD_L12) {
        uint32_t base = 0;
        bool carry = false;
        for (uint64_t t0 = 0; t0 < n; t0 += FD_WG) {
            const uint64_t r = t0 + (uint64_t)tid;
            const bool keep = wsa_fd::keep_l12(p.meta, p.feat, p.stride, r, r < n, carry, sh);
            uint32_t before, tot;
            wsa_fd::scan_step(keep, sh, &before, &tot);
            if (keep) { p.src[base + before] = (uint32_t)r; p.h_kept[base + before] = (int32_t)r; }
            base += tot;
        }
        if (tid == 0) sf_finish(p, count, base, (uint64_t)count + base <= p.capacity, base, 0u);
        return;
    }
    // FD_L11.  A stream's START forgets its row before its results are looked at; that is control, not storing, and holds in every step
    uint32_t mine = 0;
    for (uint32_t i = (uint32_t)tid; i < p.n_streams; i += FD_WG) {
        const int32_t sl = (p.bits[i] & 1u) ? -1 : p.slot[i];
        const uint32_t lo = p.off[i], hi = p.off[i + 1];
        mine += (hi > lo && hi <= n && sl < 0) ? 1u : 0u;
    }
    mine = wsa::wave_sum_u32(mine);
    if (lane == 0) s_new[wave] = mine;
    __syncthreads();
    uint32_t add = 0;
    for (int w = 0; w < FD_WAVES; w++) add += s_new[w];
    const bool store = !bad && (uint64_t)count + add <= p.capacity;
    uint32_t base_all = 0, base_new = 0;
    for (uint32_t t0 = 0; t0 < p.n_streams; t0 += FD_WG) {
        const uint32_t i = t0 + (uint32_t)tid;
        const bool valid = i < p.n_streams;
        const int32_t old = valid ? p.slot[i] : -1;
        const int32_t sl = valid && (p.bits[i] & 1u) ? -1 : old;
        const uint32_t lo = valid ? p.off[i] : 0u, hi = valid ? p.off[i + 1] : 0u;
        const bool has = store && valid && hi > lo && hi <= n, fresh = has && sl < 0;
        uint32_t before_a, tot_a, before_n, tot_n;
        wsa_fd::scan_step(has, sh, &before_a, &tot_a);
        wsa_fd::scan_step(fresh, sh, &before_n, &tot_n);
        int32_t now = sl;
        if (has) {
            const uint32_t j = base_all + before_a, k = base_new + before_n;
            if (fresh) { now = (int32_t)(count + k); p.h_kept[k] = (int32_t)(hi - 1u); }
            else { p.h_replaced[2 * (j - k)] = (int32_t)(hi - 1u); p.h_replaced[2 * (j - k) + 1] = sl; }
            p.src[j] = hi - 1u; p.dst[j] = (uint32_t)now;
        }
        if (valid && now != old) p.slot[i] = now;
        base_all += tot_a; base_new += tot_n;
    }
    if (tid == 0) sf_finish(p, count, add, store, base_all, base_all - base_new);
}

struct SfCopy {
    const uint64_t* feat; uint32_t stride;                // row s of the source at feat + s * stride
    const uint32_t *src, *dst;                            // source row / DB row of stored row i; nullptr: i / first new row + i
    const uint32_t* plan;                                 // {rows to move, first new DB row}, left by the plan kernel
    int width; uint32_t capacity;
    uint64_t* db;                                         // the DB's table [capacity][width]
};

// the stable copy with a grid that does not know the step's count: workgroups without a tile return at once
__global__ void __launch_bounds__(SF_COPY_THREADS) stream_featdb_copy_kernel(SfCopy p) {
    const uint32_t n = p.plan[0], base = p.plan[1];
    const uint32_t tiles = (n + SF_COPY_ROWS - 1) / SF_COPY_ROWS;
    for (uint32_t t = blockIdx.x; t < tiles; t += gridDim.x) {
        const uint32_t r0 = t * SF_COPY_ROWS;
        const uint32_t rows = n - r0 < (uint32_t)SF_COPY_ROWS ? n - r0 : (uint32_t)SF_COPY_ROWS;
        const uint32_t words = rows * (uint32_t)p.width;
        for (uint32_t e = threadIdx.x; e < words; e += SF_COPY_THREADS) {
            const uint32_t i = e / (uint32_t)p.width, k = e - i * (uint32_t)p.width;
            const uint32_t s = p.src ? p.src[r0 + i] : r0 + i;
            const uint32_t d = p.dst ? p.dst[r0 + i] : base + r0 + i;
            if (d < p.capacity) p.db[(uint64_t)d * (uint32_t)p.width + k] = p.feat[(uint64_t)s * p.stride + k];      // (the plan kernel never hands out a row beyond the capacity)
        }
    }
}

}  // namespace

struct wsa_sfdb {
    int device = 0;
    wsa_featdb* db = nullptr;
    wsa_sfdb_view v{};
    int mode = 0;
    uint32_t copy_grid = 1;
    uint32_t *d_src = nullptr, *d_dst = nullptr, *d_plan = nullptr;
    int32_t* d_slot = nullptr;                            // level 11: the DB row every stream owns (the caller's table in the test entry)
    uint32_t *h_count = nullptr, *h_count_dev = nullptr, *h_push = nullptr, *h_push_dev = nullptr;
    int32_t *h_kept = nullptr, *h_kept_dev = nullptr, *h_replaced = nullptr, *h_replaced_dev = nullptr;
    std::vector<int32_t> identity;                        // levels 5 / 13: kept[i] = i
    uint32_t last[4] = {0, 0, 0, 0};                      // the outcome of the last settled step
    wsa::DevArena mem;
};

void wsa_sfdb_free(wsa_sfdb* c) {
    if (!c) return;
    (void)hipSetDevice(c->device);
    if (c->db->attached_to == c) { c->db->attached_to = nullptr; c->db->step_pending = false; }
    delete c;
}

wsa_status wsa_sfdb_create(const wsa_sfdb_view& v, wsa_featdb* db, int32_t* d_slot, wsa_sfdb** out) {
    wsa_ctx* ctx = v.ctx;
    *out = nullptr;
    if (db->ctx != ctx) return fail(ctx, WSA_ERR_INVALID, "the feature DB was created on another context (or device) than the streams");
    const int mode = wsa_fd::mode_for(v.level, db->width);
    if (mode < 0)
        return fail(ctx, WSA_ERR_INVALID, "streams at output_level " + std::to_string(v.level) + " do not feed a feature DB of " + std::to_string(db->width)
                                          + " features per row (53: levels 5 and 13, 264: level 11, 23: level 12; levels 3, 4 and 10 store nothing)");
    if (db->attached_to && static_cast<const wsa_sfdb*>(db->attached_to)->v.owner != v.owner)
        return fail(ctx, WSA_ERR_INVALID, "the feature DB (" + std::to_string(db->count) + " of " + std::to_string(db->capacity) + " rows) is already attached to another stream set of "
                                          + std::to_string(static_cast<const wsa_sfdb*>(db->attached_to)->v.n_streams) + " streams: detach it there first");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    wsa_sfdb* c = new wsa_sfdb();
    c->device = ctx->device; c->db = db; c->v = v; c->mode = mode;
    const size_t R = v.rows_cap ? v.rows_cap : 1, N = v.n_streams ? v.n_streams : 1;
    const size_t items = mode == FD_L11 ? N : R;          // the most rows one step stores
    const size_t tiles = (items + SF_COPY_ROWS - 1) / SF_COPY_ROWS;
    c->copy_grid = (uint32_t)(tiles < (size_t)SF_COPY_GRID ? tiles : (size_t)SF_COPY_GRID);
    wsa::DevArena& A = c->mem;
    bool ok = A.alloc(&c->d_plan, 2, true) && A.pin(&c->h_count, &c->h_count_dev, 1) && A.pin(&c->h_push, &c->h_push_dev, 4);
    if (ok && mode == FD_ALL) c->identity.resize(R);
    if (ok && mode == FD_L12) ok = A.alloc(&c->d_src, R) && A.pin(&c->h_kept, &c->h_kept_dev, R);
    if (ok && mode == FD_L11) {
        ok = A.alloc(&c->d_src, N) && A.alloc(&c->d_dst, N) && A.pin(&c->h_kept, &c->h_kept_dev, N) && A.pin(&c->h_replaced, &c->h_replaced_dev, 2 * N);
        if (ok && !d_slot) {
            ok = A.alloc(&c->d_slot, N) && hipMemset(c->d_slot, 0xff, N * sizeof(int32_t)) == hipSuccess;      // all -1
            d_slot = c->d_slot;
        }
        c->d_slot = d_slot;
    }
    ok = ok && hipDeviceSynchronize() == hipSuccess;
    if (!ok) {
        const wsa_status st = fail(ctx, WSA_ERR_HIP, std::string("device allocation failed: ") + hipGetErrorString(hipGetLastError()));
        delete c;
        return st;
    }
    for (size_t i = 0; i < c->identity.size(); i++) c->identity[i] = (int32_t)i;
    db->attached_to = c; db->step_pending = false;
    *out = c;
    return WSA_OK;
}

uint32_t wsa_sfdb_settle(wsa_sfdb* c) {
    if (c->db->step_pending) {
        const volatile uint32_t* h = c->h_push;
        for (int i = 0; i < 4; i++) c->last[i] = h[i];
        if ((uint64_t)c->db->count + c->last[1] <= c->db->capacity) c->db->count += c->last[1];
        c->db->step_pending = false;
    }
    return c->last[3];
}

void wsa_sfdb_begin_step(wsa_sfdb* c) {
    (void)wsa_sfdb_settle(c);                             // (a step that was not collected)
    for (int i = 0; i < 4; i++) c->h_push[i] = 0;          // a launch that fails leaves an outcome of nothing
    *c->h_count = c->db->count;
    c->db->step_pending = true;
}

wsa_status wsa_sfdb_enqueue(wsa_sfdb* c, hipStream_t s) {
    const wsa_sfdb_view& v = c->v;
    SfPlan p{};
    p.mode = c->mode; p.meta = v.d_meta; p.feat = reinterpret_cast<const uint64_t*>(v.d_feat); p.stride = v.stride;
    p.off = v.d_utt_off; p.bits = v.d_bits; p.slot = c->d_slot; p.n_streams = v.n_streams;
    p.n_rows = v.d_n_rows; p.rows_cap = v.rows_cap; p.flags = v.d_flags; p.lost = v.d_lost;
    p.h_count = c->h_count_dev; p.capacity = c->db->capacity;
    p.src = c->d_src; p.dst = c->d_dst; p.plan = c->d_plan; p.h_push = c->h_push_dev; p.h_kept = c->h_kept_dev; p.h_replaced = c->h_replaced_dev;
    hipLaunchKernelGGL(stream_featdb_plan_kernel, dim3(1), dim3(FD_WG), 0, s, p);
    HIP_TRY(v.ctx, hipGetLastError());
    SfCopy q{};
    q.feat = p.feat; q.stride = v.stride; q.src = c->d_src; q.dst = c->d_dst; q.plan = c->d_plan; q.width = c->db->width; q.capacity = c->db->capacity;
    q.db = reinterpret_cast<uint64_t*>(c->db->d_feat);
    hipLaunchKernelGGL(stream_featdb_copy_kernel, dim3(c->copy_grid), dim3(SF_COPY_THREADS), 0, s, q);
    HIP_TRY(v.ctx, hipGetLastError());
    return WSA_OK;
}

wsa_status wsa_sfdb_result(wsa_sfdb* c, wsa_stream_db_result* o) {
    (void)wsa_sfdb_settle(c);
    o->first_row = c->last[0]; o->n_added = c->last[1]; o->n_replaced = c->last[2]; o->not_fitted = c->last[3];
    o->kept = c->mode == FD_ALL ? c->identity.data() : c->h_kept;
    o->replaced = c->mode == FD_L11 ? c->h_replaced : nullptr;
    return WSA_OK;
}

extern "C" {

// behind wsa_debug_stream_featdb_step (debug.hip; not part of wsa.h): the step's two DB kernels once over caller-given device tables.
// d_meta [rows][8] (level 12), d_feat rows at feat_stride doubles with room for rows_cap rows, d_utt_off [n_streams + 1], d_bits and
// d_slot [n_streams] (level 11; the slot table is updated in place), *d_n_rows rows in the table, bit 0 of *d_flags = WSA_FLAG_CAPACITY.
// out4 = {first_row, n_added, n_replaced, not_fitted}; the DB's count advances as after a collected step.
wsa_status wsa_sfdb_debug_step(wsa_featdb* db, int32_t level, const int32_t* d_meta, const double* d_feat, uint32_t feat_stride, uint32_t rows_cap,
                               const uint32_t* d_utt_off, uint32_t n_streams, const uint32_t* d_n_rows, const uint32_t* d_flags, const uint32_t* d_bits,
                               int32_t* d_slot, void* stream, uint32_t* out4, int32_t* kept, uint32_t kept_cap, int32_t* replaced, uint32_t replaced_cap) {
    if (!db) return WSA_ERR_INVALID;
    wsa_ctx* ctx = db->ctx;
    if (!d_n_rows || !d_flags || !out4) return fail(ctx, WSA_ERR_INVALID, "null row-count word, flags word or result");
    const int mode = wsa_fd::mode_for(level, db->width);
    if (mode >= 0) {
        if (rows_cap && !d_feat) return fail(ctx, WSA_ERR_INVALID, "null feature table");
        if (mode == FD_L12 && rows_cap && !d_meta) return fail(ctx, WSA_ERR_INVALID, "null metadata table");
        if (mode == FD_L11 && (!d_utt_off || !d_bits || !d_slot || !n_streams)) return fail(ctx, WSA_ERR_INVALID, "level 11 needs utterance offsets, control words and a slot table");
        if (feat_stride < (uint32_t)(mode == FD_L12 ? wsa_fd::FD_MARK_SLOT + 1 : db->width)) return fail(ctx, WSA_ERR_INVALID, "feat_stride " + std::to_string(feat_stride) + " is shorter than a row");
    }
    if (db->attached_to) return fail(ctx, WSA_ERR_INVALID, "the feature DB is attached to a stream set");
    const wsa_sfdb_view v{ctx, level, n_streams, rows_cap, d_meta, d_feat, feat_stride, d_utt_off, d_n_rows, d_flags, nullptr, d_bits, nullptr};
    wsa_sfdb* c = nullptr;
    if (const wsa_status st = wsa_sfdb_create(v, db, d_slot, &c); st != WSA_OK) return st;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    wsa_sfdb_begin_step(c);
    wsa_status st = wsa_sfdb_enqueue(c, s);
    if (st == WSA_OK && hipStreamSynchronize(s) != hipSuccess) st = fail(ctx, WSA_ERR_HIP, std::string("hipStreamSynchronize: ") + hipGetErrorString(hipGetLastError()));
    if (st == WSA_OK) {
        wsa_stream_db_result r{};
        wsa_sfdb_result(c, &r);
        out4[0] = r.first_row; out4[1] = r.n_added; out4[2] = r.n_replaced; out4[3] = r.not_fitted;
        if ((kept && kept_cap < r.n_added) || (replaced && replaced_cap < r.n_replaced)) st = fail(ctx, WSA_ERR_INVALID, "kept / replaced too small for " + std::to_string(r.n_added) + " / " + std::to_string(r.n_replaced) + " rows");
        else {
            for (uint32_t i = 0; kept && i < r.n_added; i++) kept[i] = r.kept[i];
            for (uint32_t i = 0; replaced && r.replaced && i < 2 * r.n_replaced; i++) replaced[i] = r.replaced[i];
        }
    } else c->db->step_pending = false;
    wsa_sfdb_free(c);
    return st;
}

// test access (not part of wsa.h): the DB's whole table, rows beyond the count included, so that a stray write shows.  Waits for the device.
int wsa_debug_featdb_copy_capacity(wsa_featdb* db, double* out) {
    if (!db || !out) return WSA_ERR_INVALID;
    wsa_ctx* ctx = db->ctx;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipDeviceSynchronize());
    HIP_TRY(ctx, hipMemcpy(out, db->d_feat, (size_t)db->capacity * db->width * sizeof(double), hipMemcpyDeviceToHost));
    return WSA_OK;
}

wsa_status wsa_stream_featdb_tile_info(int32_t* rows_per_wave_tile, int32_t* rows_per_workgroup, int32_t* copy_tile_rows, int32_t* copy_grid) {
    if (rows_per_wave_tile) *rows_per_wave_tile = FD_WAVE;
    if (rows_per_workgroup) *rows_per_workgroup = FD_WG;
    if (copy_tile_rows) *copy_tile_rows = SF_COPY_ROWS;
    if (copy_grid) *copy_grid = SF_COPY_GRID;
    return WSA_OK;
}

}  // extern "C"
