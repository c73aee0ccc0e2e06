// featdb.hip — K10: the feature DB that stays on the device (specification FD-1; include/wsa.h "A feature DB that stays on
// the device").  Append is a keep mask, an exclusive scan and a stable copy; gather is the same copy through a row list; ranges selects
// per column on the bit patterns.  Nothing here does arithmetic on a feature: every stored value is the source's bits.
//
// Stands in for the reference APPLICATION's storing path: src/index.js:35-100 (call_backed -> StoreFeatures) with js/featuredb.js:88-97,
// and the dispatch rule of js/formantanalyzer.js:712-726 that decides which rows of a level-12 callback reach it.
#include <cstring>
#include <string>
#include "featdb_internal.hpp"
#include "featdb_keep.hpp"

using wsa_api::fail;

namespace {

using wsa_fd::FD_ALL; using wsa_fd::FD_L12; using wsa_fd::FD_L11;
using wsa_fd::FD_WAVE; using wsa_fd::FD_WG; using wsa_fd::FD_MARK_SLOT;      // (featdb_keep.hpp: source rows one wave ballots, rows per step of the keep kernel's walk)
constexpr int FD_COPY_THREADS = 256;
constexpr int FD_COPY_ROWS = 64;                          // appended rows per workgroup tile of the copy kernel
constexpr int FD_COPY_GRID = 512;                         // its grid is capped here: FD_COPY_GRID * FD_COPY_ROWS rows per pass
constexpr int FD_RANGE_ROWS = 256;                        // selected rows per chunk of the ranges kernel

struct FdKeep {
    int mode;                                             // FD_L12 or FD_L11
    const int32_t* meta;                                  // FD_L12: [n_items][8], columns 0 and 1 name the callback
    const uint64_t* feat; uint32_t stride;                // FD_L12: slot 23 of row r at feat[r * stride + 23]
    const uint32_t* off;                                  // FD_L11: [n_items + 1] utterance-row offsets per clip
    uint32_t n_items, n_src;                              // items walked (rows; FD_L11: clips), rows of the source table
    uint32_t* kept;                                       // [n_items] source row of the i-th kept row
    uint32_t* total;                                      // mapped host word: rows kept
};

// ---- keep + scan: ONE workgroup walks the items FD_WG at a time, so that the output order is the source order whatever the device does.
// No workgroup waits on another.  What is carried from step to step is uniform: the rows kept so far and, at level 12, whether the callback
// that is open at the end of the step has been marked.  Level 12 takes a callback to be a RUN of rows with one (clip, si), which is what the
// row table holds (it is in (clip, si) order); FD-1's "no earlier row of the same (clip, si) is marked" and this agree on such tables only.
__global__ void __launch_bounds__(FD_WG) featdb_keep_kernel(FdKeep p) {
    __shared__ wsa_fd::KeepShared sh;
    const int tid = (int)threadIdx.x;
    uint32_t base = 0;
    bool carry = false;
    for (uint64_t t0 = 0; t0 < p.n_items; t0 += FD_WG) {
        const uint64_t r = t0 + (uint64_t)tid;
        const bool valid = r < p.n_items;
        bool keep = false;
        uint32_t src = (uint32_t)r;
        if (p.mode == FD_L11) {
            const uint32_t lo = valid ? p.off[r] : 0u, hi = valid ? p.off[r + 1] : 0u;
            keep = valid && hi > lo && hi <= p.n_src;
            src = hi - 1u;
        } else keep = wsa_fd::keep_l12(p.meta, p.feat, p.stride, r, valid, carry, sh);      // (the rule itself: featdb_keep.hpp)
        uint32_t before, tot;
        wsa_fd::scan_step(keep, sh, &before, &tot);
        if (keep) p.kept[base + before] = src;
        base += tot;
    }
    if (tid == 0) { *p.total = base; __threadfence_system(); }
}

struct FdCopy {
    const uint64_t* src; uint32_t stride;                 // row s of the source at src + s * stride
    const uint32_t* list;                                 // [n] source row of output row i, or nullptr: i
    uint32_t n; int width;
    uint64_t* dst;                                        // [n][width] dense
};

// ---- the stable copy: output row i = source row list[i], as 64-bit words.  A workgroup takes tiles of FD_COPY_ROWS output rows, a thread
// one word at a time, so that reads and writes of a row are contiguous.
__global__ void __launch_bounds__(FD_COPY_THREADS) featdb_copy_kernel(FdCopy p) {
    const uint32_t tiles = (p.n + FD_COPY_ROWS - 1) / FD_COPY_ROWS;
    for (uint32_t t = blockIdx.x; t < tiles; t += gridDim.x) {
        const uint32_t r0 = t * FD_COPY_ROWS;
        const uint32_t rows = p.n - r0 < (uint32_t)FD_COPY_ROWS ? p.n - r0 : (uint32_t)FD_COPY_ROWS;
        const uint32_t words = rows * (uint32_t)p.width;
        for (uint32_t e = threadIdx.x; e < words; e += FD_COPY_THREADS) {
            const uint32_t i = e / (uint32_t)p.width, k = e - i * (uint32_t)p.width;
            const uint32_t s = p.list ? p.list[r0 + i] : r0 + i;
            p.dst[(uint64_t)(r0 + i) * (uint32_t)p.width + k] = p.src[(uint64_t)s * p.stride + k];
        }
    }
}

// ---- ranges.  A double's bits become a key whose unsigned order is the order of the values with -0 below +0; minimum and maximum are
// selections among keys, exact and independent of the order they are taken in.  NaN is kept out of the keys and flagged.
__device__ __forceinline__ uint64_t fd_key(uint64_t bits) { return bits ^ ((bits >> 63) ? ~0ull : 0x8000000000000000ull); }
__device__ __forceinline__ uint64_t fd_unkey(uint64_t key) { return key ^ ((key >> 63) ? 0x8000000000000000ull : ~0ull); }

struct FdRange {
    const uint64_t* feat; const uint32_t* list; uint32_t n; int width;
    uint64_t* part;                                       // [chunks][3][width]: min key, max key, NaN seen
    uint32_t chunks;
    uint64_t* out;                                        // [2][width]: the minimum's and the maximum's bits
};

__global__ void __launch_bounds__(256) featdb_range_chunk_kernel(FdRange p) {
    const uint32_t r0 = blockIdx.x * (uint32_t)FD_RANGE_ROWS;
    const uint32_t r1 = p.n - r0 < (uint32_t)FD_RANGE_ROWS ? p.n : r0 + (uint32_t)FD_RANGE_ROWS;
    for (int k = (int)threadIdx.x; k < p.width; k += 256) {
        uint64_t mn = ~0ull, mx = 0ull, nan = 0ull;
        for (uint32_t i = r0; i < r1; i++) {
            const uint32_t s = p.list ? p.list[i] : i;
            const uint64_t bits = p.feat[(uint64_t)s * (uint32_t)p.width + k];
            if ((bits & 0x7fffffffffffffffull) > 0x7ff0000000000000ull) { nan = 1; continue; }
            const uint64_t key = fd_key(bits);
            mn = key < mn ? key : mn; mx = key > mx ? key : mx;
        }
        uint64_t* q = p.part + (uint64_t)blockIdx.x * 3u * (uint32_t)p.width;
        q[k] = mn; q[p.width + k] = mx; q[2 * p.width + k] = nan;
    }
}

__global__ void __launch_bounds__(256) featdb_range_finish_kernel(FdRange p) {
    for (int k = (int)threadIdx.x; k < p.width; k += 256) {
        uint64_t mn = ~0ull, mx = 0ull, nan = 0ull;
        for (uint32_t c = 0; c < p.chunks; c++) {
            const uint64_t* q = p.part + (uint64_t)c * 3u * (uint32_t)p.width;
            mn = q[k] < mn ? q[k] : mn; mx = q[p.width + k] > mx ? q[p.width + k] : mx; nan |= q[2 * p.width + k];
        }
        p.out[k] = nan ? 0x7ff8000000000000ull : fd_unkey(mn);
        p.out[p.width + k] = nan ? 0x7ff8000000000000ull : fd_unkey(mx);
    }
}

void launch_copy(const FdCopy& c, hipStream_t s) {
    if (!c.n) return;
    const uint32_t tiles = (c.n + FD_COPY_ROWS - 1) / FD_COPY_ROWS;
    hipLaunchKernelGGL(featdb_copy_kernel, dim3(tiles < (uint32_t)FD_COPY_GRID ? tiles : (uint32_t)FD_COPY_GRID), dim3(FD_COPY_THREADS), 0, s, c);
}

using wsa_fd::mode_for;      // (featdb_internal.hpp: the level that goes with a width)

struct Source { const int32_t* meta; const double* feat; uint32_t stride; const uint32_t* off; uint32_t n_src, n_clips; };

// keep, scan, the capacity check and the copy, over device tables; what wsa_featdb_append_batch and wsa_debug_featdb_append share
wsa_status append_tables(wsa_featdb* db, int mode, const Source& src, hipStream_t s, uint32_t* first_row, uint32_t* n_added, int32_t* kept, uint32_t kept_cap) {
    wsa_ctx* ctx = db->ctx;
    const uint32_t n_items = mode == FD_L11 ? src.n_clips : src.n_src;
    if (first_row) *first_row = db->count;
    if (n_added) *n_added = 0;
    if (n_items == 0 || src.n_src == 0) return WSA_OK;
    uint32_t add = n_items;                                                   // levels 5 / 13: every row, known without a kernel
    if (mode != FD_ALL) {
        if (!db->kept.ensure(n_items)) return fail(ctx, WSA_ERR_HIP, std::string("device allocation failed: ") + hipGetErrorString(hipGetLastError()));
        FdKeep k{};
        k.mode = mode; k.meta = src.meta; k.feat = reinterpret_cast<const uint64_t*>(src.feat); k.stride = src.stride; k.off = src.off;
        k.n_items = n_items; k.n_src = src.n_src; k.kept = db->kept.p; k.total = db->d_total;
        hipLaunchKernelGGL(featdb_keep_kernel, dim3(1), dim3(FD_WG), 0, s, k);
        HIP_TRY(ctx, hipGetLastError());
        HIP_TRY(ctx, hipStreamSynchronize(s));
        add = *reinterpret_cast<const volatile uint32_t*>(db->h_total);
        if (add > n_items) return fail(ctx, WSA_ERR_HIP, "the keep kernel reported more rows than it was given");
    }
    if ((uint64_t)db->count + add > db->capacity)
        return fail(ctx, WSA_ERR_CAPACITY, "the feature DB holds " + std::to_string(db->count) + " rows, " + std::to_string(add) + " rows to add do not fit its capacity of "
                                           + std::to_string(db->capacity));
    if (kept && kept_cap < add) return fail(ctx, WSA_ERR_INVALID, "kept has room for " + std::to_string(kept_cap) + " entries, " + std::to_string(add) + " rows are added");
    FdCopy c{};
    c.src = reinterpret_cast<const uint64_t*>(src.feat); c.stride = src.stride; c.list = mode == FD_ALL ? nullptr : db->kept.p; c.n = add; c.width = db->width;
    c.dst = reinterpret_cast<uint64_t*>(db->d_feat + (size_t)db->count * db->width);
    launch_copy(c, s);
    HIP_TRY(ctx, hipGetLastError());
    if (kept && mode == FD_ALL) for (uint32_t i = 0; i < add; i++) kept[i] = (int32_t)i;
    else if (kept && add) {
        HIP_TRY(ctx, hipMemcpyAsync(kept, db->kept.p, (size_t)add * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
        HIP_TRY(ctx, hipStreamSynchronize(s));
    }
    db->count += add;
    if (n_added) *n_added = add;
    return WSA_OK;
}

// rows[0 .. n-1] through the pinned staging into db->rows on s
wsa_status stage_rows(wsa_featdb* db, const uint32_t* rows, uint32_t n, hipStream_t s) {
    wsa_ctx* ctx = db->ctx;
    HIP_TRY(ctx, hipEventSynchronize(db->ev_rows));                           // the copy that last read the staging
    if (db->h_rows_cap < n) {
        if (db->h_rows) { (void)hipHostFree(db->h_rows); db->h_rows = nullptr; db->h_rows_cap = 0; }
        HIP_TRY(ctx, hipHostMalloc(reinterpret_cast<void**>(&db->h_rows), (size_t)n * sizeof(uint32_t), hipHostMallocDefault));
        db->h_rows_cap = n;
    }
    if (!db->rows.ensure(n)) return fail(ctx, WSA_ERR_HIP, std::string("device allocation failed: ") + hipGetErrorString(hipGetLastError()));
    std::memcpy(db->h_rows, rows, (size_t)n * sizeof(uint32_t));
    HIP_TRY(ctx, hipMemcpyAsync(db->rows.p, db->h_rows, (size_t)n * sizeof(uint32_t), hipMemcpyHostToDevice, s));
    HIP_TRY(ctx, hipEventRecord(db->ev_rows, s));
    return WSA_OK;
}

}  // namespace

extern "C" {

wsa_status wsa_featdb_create(wsa_ctx* ctx, int32_t width, uint32_t capacity_rows, wsa_featdb** out) {
    if (!ctx || !out) return fail(ctx, WSA_ERR_INVALID, "null argument");
    *out = nullptr;
    if (const char* why = wsa_model_width_refusal(width)) return fail(ctx, WSA_ERR_INVALID, "a feature DB of " + std::to_string(width) + why);
    if (capacity_rows == 0) return fail(ctx, WSA_ERR_INVALID, "a feature DB has room for at least one row");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    wsa_featdb* db = new wsa_featdb();
    db->ctx = ctx; db->width = width; db->capacity = capacity_rows;
    if (!(db->mem.alloc(&db->d_feat, (size_t)capacity_rows * (size_t)width) && db->mem.pin(&db->h_total, &db->d_total, 1)
          && hipEventCreateWithFlags(&db->ev_rows, hipEventDisableTiming) == hipSuccess)) {
        const std::string msg = std::string("device allocation failed: ") + hipGetErrorString(hipGetLastError());
        wsa_featdb_destroy(db);
        return fail(ctx, WSA_ERR_HIP, msg);
    }
    *out = db;
    return WSA_OK;
}

void wsa_featdb_destroy(wsa_featdb* db) {
    if (!db) return;
    (void)hipSetDevice(db->ctx->device);
    if (db->ev_rows) { (void)hipEventSynchronize(db->ev_rows); (void)hipEventDestroy(db->ev_rows); }
    if (db->h_rows) (void)hipHostFree(db->h_rows);
    delete db;
}

wsa_status wsa_featdb_clear(wsa_featdb* db) {
    if (!db) return WSA_ERR_INVALID;
    if (db->attached_to)
        return fail(db->ctx, WSA_ERR_INVALID, "wsa_featdb_clear on a feature DB that is attached to a stream set (" + std::to_string(db->count)
                                              + " rows): detach it (wsa_stream_set_featdb with NULL), clear, attach again");
    db->count = 0;
    return WSA_OK;
}

wsa_status wsa_featdb_count(const wsa_featdb* db, uint32_t* n_rows) {
    if (!db) return WSA_ERR_INVALID;
    if (!n_rows) return fail(db->ctx, WSA_ERR_INVALID, "null argument");
    *n_rows = db->count;
    return WSA_OK;
}

wsa_status wsa_featdb_append_batch(wsa_featdb* db, wsa_batch* batch, void* stream, uint32_t* first_row, uint32_t* n_added, int32_t* kept, uint32_t kept_cap) {
    if (!db) return WSA_ERR_INVALID;
    if (const std::string why = wsa_fd::pending_refusal(db, "wsa_featdb_append_batch"); !why.empty()) return fail(db->ctx, WSA_ERR_INVALID, why);
    wsa_ctx* ctx = db->ctx;
    if (!batch) return fail(ctx, WSA_ERR_INVALID, "null batch");
    wsa_batch_view v{};
    wsa_batch_view_internal(batch, &v);
    if (v.ctx != ctx) return fail(ctx, WSA_ERR_INVALID, "the batch belongs to another context");
    const int mode = mode_for(v.level, db->width);
    if (mode < 0)
        return fail(ctx, WSA_ERR_INVALID, "a batch of output_level " + std::to_string(v.level) + " does not feed a feature DB of " + std::to_string(db->width)
                                          + " features per row (53: levels 5 and 13, 264: level 11, 23: level 12)");
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    wsa_device_result res{};
    // refuses a batch without a run (WSA_ERR_INVALID) and a run with WSA_FLAG_CAPACITY set (WSA_ERR_CAPACITY), with the batch's own message: same context
    if (const wsa_status st = wsa_batch_result(batch, stream, &res); st != WSA_OK) return st;
    Source src{};
    src.meta = res.d_row_meta; src.n_clips = res.n_clips;
    if (mode == FD_L11) { src.feat = res.d_utt_feat; src.stride = WSA_NUTT; src.off = res.d_clip_utt_off; src.n_src = res.n_utterance_rows; }
    else { src.feat = res.d_row_feat; src.stride = WSA_NFEAT; src.off = res.d_clip_row_off; src.n_src = res.n_rows; }
    return append_tables(db, mode, src, s, first_row, n_added, kept, kept_cap);
}

// test access to K10 on caller-given device tables (not part of include/wsa.h): level picks the keep rule and must go with the DB's width;
// d_meta [n_src][8] (level 12), d_feat rows at feat_stride doubles, d_clip_off [n_clips + 1] (level 11).  Precondition at level 12, as for the
// batch's row table: the rows of one (clip, si) are contiguous.  On a table that repeats a (clip, si) further down, the kernel treats the
// second run as a new callback, FD-1's sentence (and tests/featdb_ref.py) as the same one.
wsa_status wsa_debug_featdb_append(wsa_featdb* db, int32_t level, const int32_t* d_meta, const double* d_feat, uint32_t feat_stride, const uint32_t* d_clip_off,
                                   uint32_t n_src, uint32_t n_clips, void* stream, uint32_t* first_row, uint32_t* n_added, int32_t* kept, uint32_t kept_cap) {
    if (!db) return WSA_ERR_INVALID;
    wsa_ctx* ctx = db->ctx;
    const int mode = mode_for(level, db->width);
    if (mode < 0) return fail(ctx, WSA_ERR_INVALID, "output_level " + std::to_string(level) + " does not go with a DB of " + std::to_string(db->width) + " features per row");
    if (n_src && !d_feat) return fail(ctx, WSA_ERR_INVALID, "null feature table");
    if (mode == FD_L12 && n_src && !d_meta) return fail(ctx, WSA_ERR_INVALID, "null metadata table");
    if (mode == FD_L11 && !d_clip_off) return fail(ctx, WSA_ERR_INVALID, "null clip offsets");
    if (feat_stride < (uint32_t)(mode == FD_L12 ? FD_MARK_SLOT + 1 : db->width)) return fail(ctx, WSA_ERR_INVALID, "feat_stride " + std::to_string(feat_stride) + " is shorter than a row");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const Source src{d_meta, d_feat, feat_stride, d_clip_off, n_src, n_clips};
    return append_tables(db, mode, src, reinterpret_cast<hipStream_t>(stream), first_row, n_added, kept, kept_cap);
}

wsa_status wsa_featdb_append_host(wsa_featdb* db, const double* feat, uint32_t n, void* stream) {
    if (!db) return WSA_ERR_INVALID;
    if (const std::string why = wsa_fd::pending_refusal(db, "wsa_featdb_append_host"); !why.empty()) return fail(db->ctx, WSA_ERR_INVALID, why);
    wsa_ctx* ctx = db->ctx;
    if (n && !feat) return fail(ctx, WSA_ERR_INVALID, "null feature pointer");
    if ((uint64_t)db->count + n > db->capacity)
        return fail(ctx, WSA_ERR_CAPACITY, "the feature DB holds " + std::to_string(db->count) + " rows, " + std::to_string(n) + " rows to add do not fit its capacity of "
                                           + std::to_string(db->capacity));
    if (!n) return WSA_OK;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipMemcpyAsync(db->d_feat + (size_t)db->count * db->width, feat, (size_t)n * db->width * sizeof(double), hipMemcpyHostToDevice, s));
    HIP_TRY(ctx, hipStreamSynchronize(s));
    db->count += n;
    return WSA_OK;
}

wsa_status wsa_featdb_device_rows(const wsa_featdb* db, const double** d_feat) {
    if (!db) return WSA_ERR_INVALID;
    if (!d_feat) return fail(db->ctx, WSA_ERR_INVALID, "null argument");
    *d_feat = db->d_feat;
    return WSA_OK;
}

wsa_status wsa_featdb_copy_rows(wsa_featdb* db, void* stream, uint32_t first, uint32_t n, double* out) {
    if (!db) return WSA_ERR_INVALID;
    if (const std::string why = wsa_fd::pending_refusal(db, "wsa_featdb_copy_rows"); !why.empty()) return fail(db->ctx, WSA_ERR_INVALID, why);
    wsa_ctx* ctx = db->ctx;
    if ((uint64_t)first + n > db->count)
        return fail(ctx, WSA_ERR_INVALID, "rows " + std::to_string(first) + " .. " + std::to_string((uint64_t)first + n) + " are outside the DB's " + std::to_string(db->count) + " rows");
    if (n && !out) return fail(ctx, WSA_ERR_INVALID, "null argument");
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (n) HIP_TRY(ctx, hipMemcpyAsync(out, db->d_feat + (size_t)first * db->width, (size_t)n * db->width * sizeof(double), hipMemcpyDeviceToHost, s));
    HIP_TRY(ctx, hipStreamSynchronize(s));
    return WSA_OK;
}

wsa_status wsa_featdb_gather(wsa_featdb* db, const uint32_t* rows, uint32_t n, double* d_out, void* stream) {
    if (!db) return WSA_ERR_INVALID;
    if (const std::string why = wsa_fd::pending_refusal(db, "wsa_featdb_gather"); !why.empty()) return fail(db->ctx, WSA_ERR_INVALID, why);
    wsa_ctx* ctx = db->ctx;
    if (n && (!rows || !d_out)) return fail(ctx, WSA_ERR_INVALID, "null row list / output pointer");
    const std::string why = wsa_fd::rows_refusal(db, rows, n);
    if (!why.empty()) return fail(ctx, WSA_ERR_INVALID, why);
    if (!n) return WSA_OK;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (const wsa_status st = stage_rows(db, rows, n, s)) return st;
    FdCopy c{};
    c.src = reinterpret_cast<const uint64_t*>(db->d_feat); c.stride = (uint32_t)db->width; c.list = db->rows.p; c.n = n; c.width = db->width;
    c.dst = reinterpret_cast<uint64_t*>(d_out);
    launch_copy(c, s);
    HIP_TRY(ctx, hipGetLastError());
    return WSA_OK;
}

wsa_status wsa_featdb_ranges(wsa_featdb* db, const uint32_t* rows, uint32_t n, void* stream, double* in_min, double* in_max) {
    if (!db) return WSA_ERR_INVALID;
    if (const std::string why = wsa_fd::pending_refusal(db, "wsa_featdb_ranges"); !why.empty()) return fail(db->ctx, WSA_ERR_INVALID, why);
    wsa_ctx* ctx = db->ctx;
    if (!in_min || !in_max) return fail(ctx, WSA_ERR_INVALID, "null in_min / in_max");
    if (n == 0) return fail(ctx, WSA_ERR_INVALID, "ranges over no row");
    if (rows) {
        const std::string why = wsa_fd::rows_refusal(db, rows, n);
        if (!why.empty()) return fail(ctx, WSA_ERR_INVALID, why);
    } else if (n > db->count) return fail(ctx, WSA_ERR_INVALID, std::to_string(n) + " rows asked for, the DB holds " + std::to_string(db->count));
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (rows) if (const wsa_status st = stage_rows(db, rows, n, s)) return st;
    const uint32_t W = (uint32_t)db->width, chunks = (n + FD_RANGE_ROWS - 1) / FD_RANGE_ROWS;
    if (!db->part.ensure(((size_t)chunks * 3 + 2) * W)) return fail(ctx, WSA_ERR_HIP, std::string("device allocation failed: ") + hipGetErrorString(hipGetLastError()));
    FdRange p{};
    p.feat = reinterpret_cast<const uint64_t*>(db->d_feat); p.list = rows ? db->rows.p : nullptr; p.n = n; p.width = db->width;
    p.part = db->part.p; p.chunks = chunks; p.out = db->part.p + (size_t)chunks * 3 * W;
    hipLaunchKernelGGL(featdb_range_chunk_kernel, dim3(chunks), dim3(256), 0, s, p);
    hipLaunchKernelGGL(featdb_range_finish_kernel, dim3(1), dim3(256), 0, s, p);
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipMemcpyAsync(in_min, p.out, (size_t)W * sizeof(double), hipMemcpyDeviceToHost, s));
    HIP_TRY(ctx, hipMemcpyAsync(in_max, p.out + W, (size_t)W * sizeof(double), hipMemcpyDeviceToHost, s));
    HIP_TRY(ctx, hipStreamSynchronize(s));
    return WSA_OK;
}

wsa_status wsa_featdb_tile_info(int32_t* rows_per_wave_tile, int32_t* rows_per_workgroup, int32_t* rows_per_pass) {
    if (rows_per_wave_tile) *rows_per_wave_tile = FD_WAVE;
    if (rows_per_workgroup) *rows_per_workgroup = FD_WG;
    if (rows_per_pass) *rows_per_pass = FD_COPY_GRID * FD_COPY_ROWS;
    return WSA_OK;
}

}  // extern "C"
