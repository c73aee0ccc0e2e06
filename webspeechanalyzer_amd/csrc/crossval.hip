// crossval.hip — held-out prediction of a labelled feature DB (specification CV-1), and its part of the C ABI
// (include/wsa_crossval.h).  Works on a wsa_dbstats object (dbstats.hip, DS-1): the rows are dealt to folds once
// (wsa_dbstats_set_folds), and a prediction runs the K models of a head in ONE launch of K6f (classify.hip), model k over the rows of
// fold k, reading the dense rows where they are and writing the DB's own probability table / predicted column at those rows.  Rows
// without a fold keep what the call put there first: zero probabilities (DS-1 then decides blank) or NaN.  Everything after that is
// DS-1 and EV-1 on the columns these entries leave.
//
// Stands in for what a user of the reference APPLICATION has to do by hand for an honest figure: its Predict button
// (src/neuralmodel.js:410) runs a model over the rows it was trained on.
#include <cmath>
#include <cstring>
#include <limits>
#include <string>
#include <vector>
#include "classify_internal.hpp"
#include "dbstats_internal.hpp"

using wsa_api::fail;
using namespace wsa_classify;
using namespace wsa_dbstats_detail;

static_assert(WSA_CROSSVAL_MAX_FOLDS == WSA_TRAIN_GROUP_MAX, "a cross-validation's models train as one training group");

namespace {

__global__ void __launch_bounds__(DS_THREADS) crossval_fill_kernel(double* out, uint32_t n, double v) {
    const uint32_t i = blockIdx.x * DS_THREADS + threadIdx.x;
    if (i < n) out[i] = v;
}

// what both predictions refuse alike before they look at a member's kind; the members' width is the DB's
wsa_status check_members(wsa_dbstats* db, const wsa_model* const* models, uint32_t n_models) {
    wsa_ctx* ctx = db->ctx;
    const DsFolds& f = db->folds;
    if (!f.n_folds) return fail(ctx, WSA_ERR_INVALID, "the DB's rows have no folds yet: wsa_dbstats_set_folds");
    if (n_models != f.n_folds) return fail(ctx, WSA_ERR_INVALID, std::to_string(n_models) + " models for " + std::to_string(f.n_folds) + " folds: one model per fold");
    if (!models) return fail(ctx, WSA_ERR_INVALID, "null member array");
    for (uint32_t k = 0; k < n_models; k++) {
        const std::string who = "member " + std::to_string(k);
        if (!models[k]) return fail(ctx, WSA_ERR_INVALID, who + " is NULL");
        if (models[k]->ctx != ctx) return fail(ctx, WSA_ERR_INVALID, who + " belongs to another context");
        if ((uint32_t)models[k]->nin != db->n_feat)
            return fail(ctx, WSA_ERR_INVALID, who + " takes " + std::to_string(models[k]->nin) + " inputs; the DB's rows have " + std::to_string(db->n_feat) + " features");
    }
    return WSA_OK;
}

// the table through its staging buffer, then K6f; tiles == 0: every list is empty and nothing is launched
wsa_status enqueue_folds(wsa_dbstats* db, const wsa_model* const* models, float* prob, double* value, const double* out_min, const double* out_max, hipStream_t s) {
    wsa_ctx* ctx = db->ctx;
    DsFolds& f = db->folds;
    HIP_TRY(ctx, hipEventSynchronize(f.done));                     // the previous call's launch has read the table
    size_t lds = 0;
    const uint64_t tiles = folds_table(models, f.n_folds, db->d_feat, f.d_rows, f.off.data(), prob, value, out_min, out_max, f.h_tab, &lds);
    if (!tiles) return WSA_OK;
    HIP_TRY(ctx, hipMemcpyAsync(f.d_tab, f.h_tab, (size_t)f.n_folds * sizeof(ClsFoldEntry), hipMemcpyHostToDevice, s));
    launch_classify_folds(ctx, f.d_tab, f.n_folds, tiles, lds, s);
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipEventRecord(f.done, s));
    return WSA_OK;
}

}  // namespace

extern "C" {

wsa_status wsa_crossval_tiles(const uint32_t* rows_per_fold, const int32_t* rb, uint32_t n, uint64_t* tiles) {
    if (!rows_per_fold || !rb || !tiles || n == 0 || n > WSA_CROSSVAL_MAX_FOLDS) return WSA_ERR_INVALID;
    uint64_t t = 0;
    for (uint32_t k = 0; k < n; k++) {
        if (rb[k] != 1 && rb[k] != 2 && rb[k] != 4) return WSA_ERR_INVALID;
        t += fold_tiles(rows_per_fold[k], rb[k]);
    }
    *tiles = t;
    return WSA_OK;
}

wsa_status wsa_dbstats_set_folds(wsa_dbstats* db, const int32_t* fold_of_row, uint32_t n_folds) {
    if (!db) return WSA_ERR_INVALID;
    wsa_ctx* ctx = db->ctx;
    if (!fold_of_row) return fail(ctx, WSA_ERR_INVALID, "null fold_of_row");
    if (n_folds < 2 || n_folds > WSA_CROSSVAL_MAX_FOLDS)
        return fail(ctx, WSA_ERR_INVALID, "a cross-validation has 2 .. " + std::to_string(WSA_CROSSVAL_MAX_FOLDS) + " folds, got " + std::to_string(n_folds));
    DsFolds& f = db->folds;
    if (f.n_folds) return fail(ctx, WSA_ERR_INVALID, "the DB's folds are set already; they are set once");
    if (!db->d_feat) return fail(ctx, WSA_ERR_INVALID, "the DB was created without feature rows");
    // everything is checked before anything is kept: a refusal leaves the object as it was
    std::vector<uint32_t> off(n_folds + 1, 0);
    for (uint32_t r = 0; r < db->n_rows; r++) {
        const int32_t k = fold_of_row[r];
        if (k < -1 || (k >= 0 && (uint32_t)k >= n_folds))
            return fail(ctx, WSA_ERR_INVALID, "fold " + std::to_string(k) + " of row " + std::to_string(r) + " is outside -1 .. " + std::to_string(n_folds - 1));
        if (k >= 0) off[(size_t)k + 1]++;
    }
    for (uint32_t k = 0; k < n_folds; k++) off[k + 1] += off[k];
    std::vector<uint32_t> rows(off[n_folds]), at(off.begin(), off.end() - 1);
    for (uint32_t r = 0; r < db->n_rows; r++)
        if (fold_of_row[r] >= 0) rows[at[fold_of_row[r]]++] = r;    // row order: every list ascends
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    uint32_t* d_rows = nullptr; ClsFoldEntry *h_tab = nullptr, *tab_dev = nullptr, *d_tab = nullptr; hipEvent_t done = nullptr;
    if (!(db->mem.upload(&d_rows, rows) && db->mem.pin(&h_tab, &tab_dev, (size_t)n_folds) && db->mem.alloc(&d_tab, (size_t)n_folds)
          && hipEventCreateWithFlags(&done, hipEventDisableTiming) == hipSuccess))
        return alloc_failed(ctx);
    f.off = off; f.d_rows = d_rows; f.h_tab = h_tab; f.d_tab = d_tab; f.done = done; f.n_folds = n_folds;
    return WSA_OK;
}

wsa_status wsa_dbstats_predict_classes_folds(wsa_dbstats* db, uint32_t head, const wsa_model* const* models, uint32_t n_models,
                                             const int32_t* legend_to_vocab, void* stream) {
    if (!db) return WSA_ERR_INVALID;
    wsa_ctx* ctx = db->ctx;
    if (const wsa_status st = check_head(db, head, true)) return st;
    if (const wsa_status st = check_members(db, models, n_models)) return st;
    const int C = models[0]->C;
    for (uint32_t k = 0; k < n_models; k++) {
        const wsa_model* m = models[k];
        const std::string who = "member " + std::to_string(k);
        if (m->C == 1 && !m->softmax)
            return fail(ctx, WSA_ERR_INVALID, who + " is a regression model (one unit, no softmax): it predicts values, not classes: wsa_dbstats_predict_values_folds");
        if (m->C != C) return fail(ctx, WSA_ERR_INVALID, who + " has " + std::to_string(m->C) + " classes, member 0 has " + std::to_string(C) + ": the folds' models share one legend");
        if (m->key_rank != models[0]->key_rank)
            return fail(ctx, WSA_ERR_INVALID, who + "'s legend has other key ranks than member 0's: the folds' models share one legend");
    }
    if (!legend_to_vocab) return fail(ctx, WSA_ERR_INVALID, "null legend_to_vocab");
    const int32_t V = (int32_t)(db->voff[head + 1] - db->voff[head]);
    int32_t map[WSA_MODEL_MAX_CLASSES];
    for (int c = 0; c < WSA_MODEL_MAX_CLASSES; c++) {
        if (c < C && (legend_to_vocab[c] < -1 || legend_to_vocab[c] >= V))
            return fail(ctx, WSA_ERR_INVALID, "legend_to_vocab[" + std::to_string(c) + "] = " + std::to_string(legend_to_vocab[c]) + " is outside -1 .. " + std::to_string(V - 1));
        map[c] = c < C ? legend_to_vocab[c] : -1;
    }
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (!db->d_prob && !db->mem.alloc(&db->d_prob, (size_t)db->n_rows * WSA_MODEL_MAX_CLASSES)) return alloc_failed(ctx);
    if (!db->d_prob_key_rank && !db->mem.alloc(&db->d_prob_key_rank, (size_t)WSA_MODEL_MAX_CLASSES)) return alloc_failed(ctx);
    HIP_TRY(ctx, hipMemsetAsync(db->d_prob, 0, (size_t)db->n_rows * C * sizeof(float), s));
    if (const wsa_status st = enqueue_folds(db, models, db->d_prob, nullptr, nullptr, nullptr, s)) return st;
    // kept for the per-file fold (K8e), as wsa_dbstats_predict_classes keeps them
    db->prob_classes = (uint32_t)C;
    db->prob_head = (int)head;
    std::memcpy(db->prob_map, map, sizeof(db->prob_map));
    HIP_TRY(ctx, hipMemcpyAsync(db->d_prob_key_rank, models[0]->d_key_rank, (size_t)C * sizeof(int64_t), hipMemcpyDeviceToDevice, s));
    return wsa_dbstats_decide_rows(db, head, db->d_prob, (uint32_t)C, legend_to_vocab, stream);
}

wsa_status wsa_dbstats_predict_values_folds(wsa_dbstats* db, uint32_t head, const wsa_model* const* models, uint32_t n_models,
                                            const double* out_min, const double* out_max, void* stream) {
    if (!db) return WSA_ERR_INVALID;
    wsa_ctx* ctx = db->ctx;
    if (const wsa_status st = check_head(db, head, false)) return st;
    if (const wsa_status st = check_members(db, models, n_models)) return st;
    if (!out_min || !out_max) return fail(ctx, WSA_ERR_INVALID, "null out_min / out_max array");
    for (uint32_t k = 0; k < n_models; k++)
        if (const char* why = regress_refusal(models[k], out_min[k], out_max[k])) return fail(ctx, WSA_ERR_INVALID, "member " + std::to_string(k) + ": " + why);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipLaunchKernelGGL(crossval_fill_kernel, dim3((db->n_rows + DS_THREADS - 1) / DS_THREADS), dim3(DS_THREADS), 0, s, db->d_p_val[head], db->n_rows,
                       std::numeric_limits<double>::quiet_NaN());
    HIP_TRY(ctx, hipGetLastError());
    return enqueue_folds(db, models, nullptr, db->d_p_val[head], out_min, out_max, s);
}

}  // extern "C"
