// dbstats.hip — K8: predicting a labelled feature DB and the numbers of the app's results table (specification DS-1),
// and its part of the C ABI (include/wsa.h "Predicting a labelled feature DB").
//
// Stands in for the reference APPLICATION's Predict button: src/neuralmodel.js:410-535 (predict_db_nn -> nn_db_results_handler),
// src/localstore.js:723-769 (update_pred_label) and :498-627 (shows_stats_table).  The probabilities and values come from K6 through
// wsa_classify_rows / wsa_regress_rows, unchanged; K8 adds three kernels:
//   decide   [n][C] f32 -> [n] i32     a group of G = next power of two >= C lanes per row (64 / G rows per wave): a coalesced load, the
//                                      lane-wise maximum of the probabilities above 0 and the lowest lane that holds it
//   chunk    pass 1 of the table       one workgroup per chunk of R = 256 consecutive rows; the chunk's columns staged in LDS; every
//                                      counter of every head owned by ONE lane that walks the chunk in row order and stores its partial
//                                      into the chunk's slab
//   sum      pass 2, the next launch   one workgroup per head; every counter summed over the slabs in chunk order, first_row by min
// Every sum has one owner and one order that does not depend on the grid; there are no atomics on floating-point values, no tickets and
// no fences: the second launch is the ordering.
#include <cmath>
#include <cstring>
#include <limits>
#include <string>
#include <vector>
#include "dbstats_internal.hpp"

#pragma clang fp contract(off)

using wsa_api::fail;
using namespace wsa_dbstats_detail;        // DsTable, struct wsa_dbstats' parts, check_head: shared with K8e (dbeval.hip)

namespace {

struct DsDecide {
    const float* prob; int32_t* out; uint32_t n_rows; int C, G;
    int32_t map[WSA_MODEL_MAX_CLASSES];
};

// ref neuralmodel.js nn_db_results_handler over ml5's stably sorted result: the class of the largest probability, the first in legend order
// on a tie, if it is > 0.  key = p where p > 0 else 0 (a NaN compares false and so never wins); the row's answer is the lowest lane whose
// key equals the group's maximum when that maximum is above 0.
__global__ void __launch_bounds__(DS_THREADS) dbstats_decide_kernel(DsDecide p) {
    __shared__ int32_t s_map[WSA_MODEL_MAX_CLASSES];
    if (threadIdx.x < WSA_MODEL_MAX_CLASSES) s_map[threadIdx.x] = p.map[threadIdx.x];
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int per_wave = 64 / p.G, sub = lane / p.G, c = lane % p.G;
    const uint64_t row = ((uint64_t)blockIdx.x * (DS_THREADS / 64) + wave) * per_wave + sub;
    const bool live = row < p.n_rows && c < p.C;
    const float v = live ? p.prob[row * p.C + c] : 0.f;
    const float key = v > 0.f ? v : 0.f;
    float best = key;
    for (int d = 1; d < p.G; d <<= 1) { const float o = __shfl_xor(best, d); best = o > best ? o : best; }
    int first = (best > 0.f && key == best) ? c : 64;
    for (int d = 1; d < p.G; d <<= 1) { const int o = __shfl_xor(first, d); first = o < first ? o : first; }
    if (c == 0 && row < p.n_rows) p.out[row] = first < 64 ? s_map[first] : -1;
}

// (DsTable, the parameter block of the two table passes: dbstats_internal.hpp)
// LDS of pass 1: durations, then per ordinal head true / predicted values, then per categorical head true / predicted indices
inline size_t chunk_lds(uint32_t n_cat, uint32_t n_ord) { return (size_t)DS_R * (sizeof(double) * (1 + 2 * n_ord) + sizeof(int32_t) * 2 * n_cat); }

__global__ void __launch_bounds__(DS_THREADS) dbstats_chunk_kernel(DsTable p) {
    extern __shared__ double ds_lds[];
    double* s_dur = ds_lds;
    double* s_tv = s_dur + DS_R;
    double* s_pv = s_tv + (size_t)p.n_ord * DS_R;
    int32_t* s_ti = reinterpret_cast<int32_t*>(s_pv + (size_t)p.n_ord * DS_R);
    int32_t* s_pi = s_ti + (size_t)p.n_cat * DS_R;
    const uint32_t chunk = blockIdx.x, tid = threadIdx.x, r0 = chunk * DS_R;
    const uint32_t rows = p.n_rows - r0 < (uint32_t)DS_R ? p.n_rows - r0 : (uint32_t)DS_R;
    const bool in = tid < rows;
    const uint64_t r = (uint64_t)r0 + tid;
    s_dur[tid] = in ? p.dur[r] : 0.0;
    for (uint32_t h = 0; h < p.n_cat; h++) {
        s_ti[h * DS_R + tid] = in ? p.t_idx[h][r] : -1;
        s_pi[h * DS_R + tid] = in ? p.p_idx[h][r] : -1;
    }
    for (uint32_t o = 0; o < p.n_ord; o++) {
        s_tv[o * DS_R + tid] = in ? p.t_val[o][r] : 0.0;
        s_pv[o * DS_R + tid] = in ? p.p_val[o][r] : 0.0;
    }
    __syncthreads();
    // one lane per (head, vocabulary entry): ref localstore.js:523-553 for the rows whose true class is this entry, in row order
    for (uint32_t item = tid; item < p.items; item += DS_THREADS) {
        uint32_t h = 0;
        for (uint32_t k = 1; k < p.n_cat; k++) if (item >= p.voff[k]) h = k;
        const int32_t v = (int32_t)(item - p.voff[h]);
        const int32_t* ti = s_ti + h * DS_R; const int32_t* pi = s_pi + h * DS_R;
        uint32_t count = 0, correct = 0, wrong = 0, first = 0xffffffffu;
        double dur = 0.0;
        for (uint32_t i = 0; i < rows; i++) {
            if (ti[i] != v) continue;
            if (!count) first = r0 + i;
            count++;
            dur += s_dur[i];
            const int32_t q = pi[i];
            if (q >= 0) { if (q == v) correct++; else wrong++; }
        }
        uint32_t* su = p.s_u32 + (size_t)chunk * 4 * p.items;
        su[item] = count; su[p.items + item] = correct; su[2 * (size_t)p.items + item] = wrong; su[3 * (size_t)p.items + item] = first;
        p.s_dur[(size_t)chunk * p.items + item] = dur;
    }
    // one lane per ordinal head: ref localstore.js:584-598; "truthy and not NaN" is v == v && v != 0
    if (tid < p.n_ord) {
        const double* tv = s_tv + tid * DS_R; const double* pv = s_pv + tid * DS_R;
        uint32_t true_n = 0, pred_n = 0;
        double mn = INFINITY, mx = 0.0, sq = 0.0;
        for (uint32_t i = 0; i < rows; i++) {
            const double t = tv[i];
            if (!(t == t && t != 0.0)) continue;
            true_n++;
            if (t < mn) mn = t;
            if (t > mx) mx = t;
            const double q = pv[i];
            if (q == q && q != 0.0) { pred_n++; const double d = q - t; sq += d * d; }
        }
        p.o_u32[((size_t)tid * 2 + 0) * p.n_chunks + chunk] = true_n;
        p.o_u32[((size_t)tid * 2 + 1) * p.n_chunks + chunk] = pred_n;
        p.o_f64[((size_t)tid * 3 + 0) * p.n_chunks + chunk] = mn;
        p.o_f64[((size_t)tid * 3 + 1) * p.n_chunks + chunk] = mx;
        p.o_f64[((size_t)tid * 3 + 2) * p.n_chunks + chunk] = sq;
    }
}

// pass 2: block b < n_cat sums categorical head b (thread v owns vocabulary entry v), block n_cat + o ordinal head o.  Chunk order.
__global__ void __launch_bounds__(DS_THREADS) dbstats_sum_kernel(DsTable p) {
    __shared__ unsigned long long s_tot[3];
    __shared__ double s_a[DS_THREADS], s_b[DS_THREADS];
    __shared__ unsigned long long s_n[2][DS_THREADS];
    const uint32_t b = blockIdx.x, tid = threadIdx.x;
    if (b < p.n_cat) {
        if (tid < 3) s_tot[tid] = 0;
        __syncthreads();
        const uint32_t V = p.voff[b + 1] - p.voff[b];
        if (tid < V) {
            const uint32_t item = p.voff[b] + tid;
            unsigned long long count = 0, correct = 0, wrong = 0;
            uint32_t first = 0xffffffffu;
            double dur = 0.0;
            for (uint32_t c = 0; c < p.n_chunks; c++) {
                const uint32_t* su = p.s_u32 + (size_t)c * 4 * p.items;
                count += su[item]; correct += su[p.items + item]; wrong += su[2 * (size_t)p.items + item];
                const uint32_t f = su[3 * (size_t)p.items + item];
                first = f < first ? f : first;
                dur += p.s_dur[(size_t)c * p.items + item];
            }
            wsa_dbstats_class e;
            e.count = count; e.correct = correct; e.wrong = wrong; e.duration = dur; e.first_row = first; e.reserved = 0;
            p.cls[item] = e;
            atomicAdd(&s_tot[0], correct); atomicAdd(&s_tot[1], wrong); atomicAdd(&s_tot[2], count - correct - wrong);
        }
        __syncthreads();
        if (tid == 0) { wsa_dbstats_cat h; h.correct = s_tot[0]; h.wrong = s_tot[1]; h.blank = s_tot[2]; p.cat[b] = h; }
        return;
    }
    const uint32_t o = b - p.n_cat;
    const uint32_t* un = p.o_u32 + (size_t)o * 2 * p.n_chunks;
    const double* uf = p.o_f64 + (size_t)o * 3 * p.n_chunks;
    unsigned long long tn = 0, pn = 0;
    double mn = INFINITY, mx = 0.0, sq = 0.0;
    for (uint32_t c0 = 0; c0 < p.n_chunks; c0 += DS_THREADS) {
        const uint32_t c = c0 + tid, m = p.n_chunks - c0 < (uint32_t)DS_THREADS ? p.n_chunks - c0 : (uint32_t)DS_THREADS;
        if (c < p.n_chunks) {
            tn += un[c]; pn += un[p.n_chunks + c];
            const double a = uf[c], z = uf[p.n_chunks + c];
            if (a < mn) mn = a;
            if (z > mx) mx = z;
            s_a[tid] = uf[2 * (size_t)p.n_chunks + c];
        }
        __syncthreads();
        if (tid == 0) for (uint32_t i = 0; i < m; i++) sq += s_a[i];       // the one owner of the squared error, in chunk order
        __syncthreads();
    }
    s_a[tid] = mn; s_b[tid] = mx; s_n[0][tid] = tn; s_n[1][tid] = pn;
    __syncthreads();
    if (tid == 0) {
        for (int i = 1; i < DS_THREADS; i++) {
            if (s_a[i] < mn) mn = s_a[i];
            if (s_b[i] > mx) mx = s_b[i];
            tn += s_n[0][i]; pn += s_n[1][i];
        }
        wsa_dbstats_ord e;
        e.true_n = tn; e.pred_n = pn; e.min = mn; e.max = mx; e.sq_sum = sq;
        p.ord[o] = e;
    }
}

}  // namespace

// (struct wsa_dbstats and check_head: dbstats_internal.hpp)
namespace {

// predict_db_nn runs a model over the stored rows as they are: the model's input count must be the DB's width
wsa_status check_width(wsa_dbstats* db, const wsa_model* m) {
    const int nin = wsa_model_inputs_internal(m);
    if ((uint32_t)nin == db->n_feat) return WSA_OK;
    return fail(db->ctx, WSA_ERR_INVALID, "the model takes " + std::to_string(nin) + " inputs; the DB's rows have " + std::to_string(db->n_feat) + " features");
}

wsa_status check_map(wsa_dbstats* db, uint32_t head, const int32_t* map, uint32_t C, DsDecide* p) {
    if (!map) return fail(db->ctx, WSA_ERR_INVALID, "null legend_to_vocab");
    const int32_t V = (int32_t)(db->voff[head + 1] - db->voff[head]);
    for (uint32_t c = 0; c < (uint32_t)WSA_MODEL_MAX_CLASSES; c++) {
        if (c < C && (map[c] < -1 || map[c] >= V))
            return fail(db->ctx, WSA_ERR_INVALID, "legend_to_vocab[" + std::to_string(c) + "] = " + std::to_string(map[c]) + " is outside -1 .. " + std::to_string(V - 1));
        p->map[c] = c < C ? map[c] : -1;
    }
    return WSA_OK;
}

void launch_decide(wsa_dbstats* db, uint32_t head, const float* d_prob, uint32_t C, DsDecide& p, hipStream_t s) {
    int G = 1;
    while (G < (int)C) G <<= 1;
    p.prob = d_prob; p.out = db->d_p_idx[head]; p.n_rows = db->n_rows; p.C = (int)C; p.G = G;
    const uint32_t per_block = (uint32_t)(DS_THREADS / G);
    hipLaunchKernelGGL(dbstats_decide_kernel, dim3((db->n_rows + per_block - 1) / per_block), dim3(DS_THREADS), 0, s, p);
}

}  // namespace

extern "C" {

wsa_status wsa_dbstats_create(wsa_ctx* ctx, const double* feat, const double* duration, uint32_t n_rows, uint32_t n_cat, const uint32_t* vocab,
                              uint32_t n_ord, wsa_dbstats** out) {
    return wsa_wide_dbstats_create(ctx, feat, WSA_NFEAT, duration, n_rows, n_cat, vocab, n_ord, out);
}

wsa_status wsa_wide_dbstats_create(wsa_ctx* ctx, const double* feat, uint32_t n_feat, const double* duration, uint32_t n_rows, uint32_t n_cat,
                                   const uint32_t* vocab, uint32_t n_ord, wsa_dbstats** out) {
    if (!ctx || !out) return fail(ctx, WSA_ERR_INVALID, "null argument");
    *out = nullptr;
    if (n_feat > 0x7fffffffu || wsa_model_width_refusal((int)n_feat))
        return fail(ctx, WSA_ERR_INVALID, "a feature DB of " + std::to_string(n_feat) + " features per row; the feature rows have 53 (output_level 5 and 13), 264 (output_level 11) or 23 (output_level 12)");
    if (n_rows == 0) return fail(ctx, WSA_ERR_INVALID, "a feature DB has at least one row");
    if (!duration) return fail(ctx, WSA_ERR_INVALID, "null duration pointer");
    if (n_cat > (uint32_t)DS_H) return fail(ctx, WSA_ERR_INVALID, std::to_string(n_cat) + " categorical heads (limit " + std::to_string(DS_H) + ")");
    if (n_ord > (uint32_t)DS_H) return fail(ctx, WSA_ERR_INVALID, std::to_string(n_ord) + " ordinal heads (limit " + std::to_string(DS_H) + ")");
    if (n_cat + n_ord == 0) return fail(ctx, WSA_ERR_INVALID, "a feature DB needs at least one head");
    if (n_cat && !vocab) return fail(ctx, WSA_ERR_INVALID, "null vocabulary sizes");
    for (uint32_t h = 0; h < n_cat; h++)
        if (vocab[h] < 1 || vocab[h] > (uint32_t)WSA_DBSTATS_MAX_CLASSES)
            return fail(ctx, WSA_ERR_INVALID, "categorical head " + std::to_string(h) + " has a vocabulary of " + std::to_string(vocab[h]) + " classes (1 .. "
                                              + std::to_string(WSA_DBSTATS_MAX_CLASSES) + ")");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    wsa_dbstats* db = new wsa_dbstats();
    db->ctx = ctx; db->n_rows = n_rows; db->n_cat = n_cat; db->n_ord = n_ord; db->n_feat = n_feat;
    db->n_chunks = (uint32_t)(((uint64_t)n_rows + DS_R - 1) / DS_R);
    for (uint32_t h = 0; h < n_cat; h++) db->voff[h + 1] = db->voff[h] + vocab[h];
    for (uint32_t h = n_cat; h < (uint32_t)DS_H; h++) db->voff[h + 1] = db->voff[h];
    db->items = db->voff[n_cat];
    const std::vector<int32_t> blank(n_rows, -1);
    const std::vector<double> missing(n_rows, std::numeric_limits<double>::quiet_NaN());
    DsTable& t = db->tab;
    bool ok = db->mem.alloc(&db->d_dur, n_rows) && hipMemcpy(db->d_dur, duration, (size_t)n_rows * sizeof(double), hipMemcpyHostToDevice) == hipSuccess;
    if (feat) ok = ok && db->mem.alloc(&db->d_feat, (size_t)n_rows * n_feat)
                      && hipMemcpy(db->d_feat, feat, (size_t)n_rows * n_feat * sizeof(double), hipMemcpyHostToDevice) == hipSuccess;
    for (uint32_t h = 0; h < n_cat && ok; h++) ok = db->mem.upload(&db->d_t_idx[h], blank) && db->mem.upload(&db->d_p_idx[h], blank);
    for (uint32_t o = 0; o < n_ord && ok; o++) ok = db->mem.upload(&db->d_t_val[o], missing) && db->mem.upload(&db->d_p_val[o], missing);
    ok = ok && db->mem.alloc(&t.s_u32, (size_t)db->n_chunks * 4 * db->items) && db->mem.alloc(&t.s_dur, (size_t)db->n_chunks * db->items)
            && db->mem.alloc(&t.o_u32, (size_t)n_ord * 2 * db->n_chunks) && db->mem.alloc(&t.o_f64, (size_t)n_ord * 3 * db->n_chunks)
            && db->mem.alloc(&t.cat, n_cat, true) && db->mem.alloc(&t.cls, db->items, true) && db->mem.alloc(&t.ord, n_ord, true);
    if (!ok) {
        const std::string msg = std::string("device allocation / copy failed: ") + hipGetErrorString(hipGetLastError());
        wsa_dbstats_destroy(db);
        return fail(ctx, WSA_ERR_HIP, msg);
    }
    t.n_rows = n_rows; t.n_chunks = db->n_chunks; t.n_cat = n_cat; t.n_ord = n_ord; t.items = db->items; t.dur = db->d_dur;
    std::memcpy(t.voff, db->voff, sizeof(t.voff));
    for (int h = 0; h < DS_H; h++) { t.t_idx[h] = db->d_t_idx[h]; t.p_idx[h] = db->d_p_idx[h]; t.t_val[h] = db->d_t_val[h]; t.p_val[h] = db->d_p_val[h]; }
    *out = db;
    return WSA_OK;
}

// the same DB with its feature rows taken from a device feature DB (FD-1): rows first_row .. first_row + n_rows - 1, device to device
wsa_status wsa_featdb_dbstats_create(wsa_ctx* ctx, const wsa_featdb* src, uint32_t first_row, uint32_t n_rows, const double* duration, uint32_t n_cat,
                                 const uint32_t* vocab, uint32_t n_ord, wsa_dbstats** out) {
    if (!ctx || !out) return fail(ctx, WSA_ERR_INVALID, "null argument");
    *out = nullptr;
    if (!src) return fail(ctx, WSA_ERR_INVALID, "null feature DB");
    if (src->ctx != ctx) return fail(ctx, WSA_ERR_INVALID, "the feature DB belongs to another context");
    if (const std::string why = wsa_fd::pending_refusal(src, "wsa_featdb_dbstats_create"); !why.empty()) return fail(ctx, WSA_ERR_INVALID, why);
    if ((uint64_t)first_row + n_rows > src->count)
        return fail(ctx, WSA_ERR_INVALID, "rows " + std::to_string(first_row) + " .. " + std::to_string((uint64_t)first_row + n_rows) + " are outside the DB's "
                                          + std::to_string(src->count) + " rows");
    wsa_dbstats* db = nullptr;
    if (const wsa_status st = wsa_wide_dbstats_create(ctx, nullptr, (uint32_t)src->width, duration, n_rows, n_cat, vocab, n_ord, &db)) return st;
    const size_t words = (size_t)n_rows * (size_t)src->width;
    if (!(hipDeviceSynchronize() == hipSuccess && db->mem.alloc(&db->d_feat, words)
          && hipMemcpy(db->d_feat, src->d_feat + (size_t)first_row * src->width, words * sizeof(double), hipMemcpyDeviceToDevice) == hipSuccess)) {
        const std::string msg = std::string("device allocation / copy failed: ") + hipGetErrorString(hipGetLastError());
        wsa_dbstats_destroy(db);
        return fail(ctx, WSA_ERR_HIP, msg);
    }
    *out = db;
    return WSA_OK;
}

void wsa_dbstats_destroy(wsa_dbstats* db) {
    if (!db) return;
    (void)hipSetDevice(db->ctx->device);
    if (db->eval.files) wsa_dbstats_destroy(db->eval.files);      // the file-level DB of wsa_dbstats_set_files
    delete db;
}

wsa_status wsa_dbstats_set_classes(wsa_dbstats* db, uint32_t head, const int32_t* true_idx, const int32_t* pred_idx) {
    if (!db) return WSA_ERR_INVALID;
    wsa_ctx* ctx = db->ctx;
    if (const wsa_status st = check_head(db, head, true)) return st;
    if (!true_idx) return fail(ctx, WSA_ERR_INVALID, "null true_idx");
    const int32_t V = (int32_t)(db->voff[head + 1] - db->voff[head]);
    for (uint32_t r = 0; r < db->n_rows; r++) {
        if (true_idx[r] < -1 || true_idx[r] >= V)
            return fail(ctx, WSA_ERR_INVALID, "true class " + std::to_string(true_idx[r]) + " of row " + std::to_string(r) + " is outside -1 .. " + std::to_string(V - 1));
        if (pred_idx && (pred_idx[r] < -1 || pred_idx[r] >= V))
            return fail(ctx, WSA_ERR_INVALID, "predicted class " + std::to_string(pred_idx[r]) + " of row " + std::to_string(r) + " is outside -1 .. " + std::to_string(V - 1));
    }
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipMemcpy(db->d_t_idx[head], true_idx, (size_t)db->n_rows * sizeof(int32_t), hipMemcpyHostToDevice));
    if (pred_idx) HIP_TRY(ctx, hipMemcpy(db->d_p_idx[head], pred_idx, (size_t)db->n_rows * sizeof(int32_t), hipMemcpyHostToDevice));
    else HIP_TRY(ctx, hipMemset(db->d_p_idx[head], 0xff, (size_t)db->n_rows * sizeof(int32_t)));
    return WSA_OK;
}

wsa_status wsa_dbstats_set_values(wsa_dbstats* db, uint32_t head, const double* true_value, const double* pred_value) {
    if (!db) return WSA_ERR_INVALID;
    wsa_ctx* ctx = db->ctx;
    if (const wsa_status st = check_head(db, head, false)) return st;
    if (!true_value) return fail(ctx, WSA_ERR_INVALID, "null true_value");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipMemcpy(db->d_t_val[head], true_value, (size_t)db->n_rows * sizeof(double), hipMemcpyHostToDevice));
    if (pred_value) HIP_TRY(ctx, hipMemcpy(db->d_p_val[head], pred_value, (size_t)db->n_rows * sizeof(double), hipMemcpyHostToDevice));
    else {
        const std::vector<double> missing(db->n_rows, std::numeric_limits<double>::quiet_NaN());
        HIP_TRY(ctx, hipMemcpy(db->d_p_val[head], missing.data(), (size_t)db->n_rows * sizeof(double), hipMemcpyHostToDevice));
    }
    return WSA_OK;
}

wsa_status wsa_dbstats_decide_rows(wsa_dbstats* db, uint32_t head, const float* d_prob, uint32_t n_classes, const int32_t* legend_to_vocab, void* stream) {
    if (!db) return WSA_ERR_INVALID;
    wsa_ctx* ctx = db->ctx;
    if (const wsa_status st = check_head(db, head, true)) return st;
    if (!d_prob) return fail(ctx, WSA_ERR_INVALID, "null probability pointer");
    if (n_classes < 1 || n_classes > (uint32_t)WSA_MODEL_MAX_CLASSES) return fail(ctx, WSA_ERR_INVALID, std::to_string(n_classes) + " classes (1 .. 64)");
    DsDecide p{};
    if (const wsa_status st = check_map(db, head, legend_to_vocab, n_classes, &p)) return st;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    launch_decide(db, head, d_prob, n_classes, p, reinterpret_cast<hipStream_t>(stream));
    HIP_TRY(ctx, hipGetLastError());
    return WSA_OK;
}

wsa_status wsa_dbstats_predict_classes(wsa_dbstats* db, uint32_t head, const wsa_model* m, const int32_t* legend_to_vocab, void* stream) {
    if (!db || !m) return WSA_ERR_INVALID;
    wsa_ctx* ctx = db->ctx;
    if (const wsa_status st = check_head(db, head, true)) return st;
    wsa_ctx* mctx = nullptr; int C = 0, softmax = 0;
    wsa_model_info_internal(m, &mctx, &C, &softmax);
    if (mctx != ctx) return fail(ctx, WSA_ERR_INVALID, "the model belongs to another context");
    if (C == 1 && !softmax) return fail(ctx, WSA_ERR_INVALID, "a regression model (one unit, no softmax) predicts values, not classes: wsa_dbstats_predict_values");
    if (!db->d_feat) return fail(ctx, WSA_ERR_INVALID, "the DB was created without feature rows");
    if (const wsa_status st = check_width(db, m)) return st;
    DsDecide p{};
    if (const wsa_status st = check_map(db, head, legend_to_vocab, (uint32_t)C, &p)) return st;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (!db->d_prob && !db->mem.alloc(&db->d_prob, (size_t)db->n_rows * WSA_MODEL_MAX_CLASSES))
        return fail(ctx, WSA_ERR_HIP, std::string("device allocation failed: ") + hipGetErrorString(hipGetLastError()));
    if (!db->d_prob_key_rank && !db->mem.alloc(&db->d_prob_key_rank, (size_t)WSA_MODEL_MAX_CLASSES))
        return fail(ctx, WSA_ERR_HIP, std::string("device allocation failed: ") + hipGetErrorString(hipGetLastError()));
    if (const wsa_status st = wsa_classify_rows(m, db->d_feat, db->n_rows, db->d_prob, stream)) return st;
    db->prob_classes = (uint32_t)C;
    // kept for the per-file fold (K8e, wsa_dbstats_fold_files): whose probabilities these are, and the key order of their legend
    db->prob_head = (int)head;
    std::memcpy(db->prob_map, p.map, sizeof(db->prob_map));
    HIP_TRY(ctx, hipMemcpyAsync(db->d_prob_key_rank, wsa_model_key_rank_internal(m), (size_t)C * sizeof(int64_t), hipMemcpyDeviceToDevice, reinterpret_cast<hipStream_t>(stream)));
    launch_decide(db, head, db->d_prob, (uint32_t)C, p, reinterpret_cast<hipStream_t>(stream));
    HIP_TRY(ctx, hipGetLastError());
    return WSA_OK;
}

wsa_status wsa_dbstats_predict_values(wsa_dbstats* db, uint32_t head, const wsa_model* m, double out_min, double out_max, void* stream) {
    if (!db || !m) return WSA_ERR_INVALID;
    wsa_ctx* ctx = db->ctx;
    if (const wsa_status st = check_head(db, head, false)) return st;
    wsa_ctx* mctx = nullptr; int C = 0, softmax = 0;
    wsa_model_info_internal(m, &mctx, &C, &softmax);
    if (mctx != ctx) return fail(ctx, WSA_ERR_INVALID, "the model belongs to another context");
    if (!db->d_feat) return fail(ctx, WSA_ERR_INVALID, "the DB was created without feature rows");
    if (const wsa_status st = check_width(db, m)) return st;
    return wsa_regress_rows(m, out_min, out_max, db->d_feat, db->n_rows, db->d_p_val[head], stream);   // refuses a classifier and a bad range
}

wsa_status wsa_dbstats_table(wsa_dbstats* db, void* stream, wsa_dbstats_cat* cat, wsa_dbstats_class* cls, wsa_dbstats_ord* ord) {
    if (!db) return WSA_ERR_INVALID;
    wsa_ctx* ctx = db->ctx;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipLaunchKernelGGL(dbstats_chunk_kernel, dim3(db->n_chunks), dim3(DS_THREADS), chunk_lds(db->n_cat, db->n_ord), s, db->tab);
    hipLaunchKernelGGL(dbstats_sum_kernel, dim3(db->n_cat + db->n_ord), dim3(DS_THREADS), 0, s, db->tab);
    HIP_TRY(ctx, hipGetLastError());
    if (cat && db->n_cat) HIP_TRY(ctx, hipMemcpyAsync(cat, db->tab.cat, (size_t)db->n_cat * sizeof(wsa_dbstats_cat), hipMemcpyDeviceToHost, s));
    if (cls && db->items) HIP_TRY(ctx, hipMemcpyAsync(cls, db->tab.cls, (size_t)db->items * sizeof(wsa_dbstats_class), hipMemcpyDeviceToHost, s));
    if (ord && db->n_ord) HIP_TRY(ctx, hipMemcpyAsync(ord, db->tab.ord, (size_t)db->n_ord * sizeof(wsa_dbstats_ord), hipMemcpyDeviceToHost, s));
    HIP_TRY(ctx, hipStreamSynchronize(s));
    return WSA_OK;
}

wsa_status wsa_dbstats_copy_classes(wsa_dbstats* db, uint32_t head, void* stream, int32_t* pred_idx) {
    if (!db) return WSA_ERR_INVALID;
    wsa_ctx* ctx = db->ctx;
    if (const wsa_status st = check_head(db, head, true)) return st;
    if (!pred_idx) return fail(ctx, WSA_ERR_INVALID, "null argument");
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipMemcpyAsync(pred_idx, db->d_p_idx[head], (size_t)db->n_rows * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    HIP_TRY(ctx, hipStreamSynchronize(s));
    return WSA_OK;
}

wsa_status wsa_dbstats_copy_values(wsa_dbstats* db, uint32_t head, void* stream, double* pred_value) {
    if (!db) return WSA_ERR_INVALID;
    wsa_ctx* ctx = db->ctx;
    if (const wsa_status st = check_head(db, head, false)) return st;
    if (!pred_value) return fail(ctx, WSA_ERR_INVALID, "null argument");
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipMemcpyAsync(pred_value, db->d_p_val[head], (size_t)db->n_rows * sizeof(double), hipMemcpyDeviceToHost, s));
    HIP_TRY(ctx, hipStreamSynchronize(s));
    return WSA_OK;
}

wsa_status wsa_dbstats_copy_probs(wsa_dbstats* db, void* stream, float* prob, uint32_t n_classes) {
    if (!db) return WSA_ERR_INVALID;
    wsa_ctx* ctx = db->ctx;
    if (!prob) return fail(ctx, WSA_ERR_INVALID, "null argument");
    if (!db->d_prob || !db->prob_classes) return fail(ctx, WSA_ERR_INVALID, "no class prediction has run on this DB yet");
    if (n_classes != db->prob_classes) return fail(ctx, WSA_ERR_INVALID, "the last prediction's model has " + std::to_string(db->prob_classes) + " classes, not " + std::to_string(n_classes));
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipMemcpyAsync(prob, db->d_prob, (size_t)db->n_rows * n_classes * sizeof(float), hipMemcpyDeviceToHost, s));
    HIP_TRY(ctx, hipStreamSynchronize(s));
    return WSA_OK;
}

}  // extern "C"
