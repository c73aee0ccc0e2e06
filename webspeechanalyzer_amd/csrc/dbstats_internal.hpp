// dbstats_internal.hpp — what K8 (dbstats.hip, specification DS-1) and K8e (dbeval.hip, specification EV-1) share: the labelled DB on
// the device (struct wsa_dbstats), the parameter block of DS-1's two table passes, and the check of a head's index.
#pragma once
#include <string>
#include <vector>
#include "host_plan.hpp"
#include "featdb_internal.hpp"
#include "../../include/wsa_eval.h"
#include "../../include/wsa_crossval.h"

namespace wsa_classify { struct ClsFoldEntry; }            // classify_internal.hpp

namespace wsa_dbstats_detail {

constexpr int DS_R = WSA_DBSTATS_CHUNK_ROWS;
constexpr int DS_THREADS = 256;
constexpr int DS_H = WSA_DBSTATS_MAX_HEADS;
static_assert(DS_THREADS == DS_R, "pass 1 stages one row per thread");
static_assert(WSA_DBSTATS_MAX_CLASSES <= DS_THREADS, "pass 2 owns one vocabulary entry per thread");

struct DsTable {
    uint32_t n_rows, n_chunks, n_cat, n_ord, items;        // items = the sum of the vocabulary sizes
    uint32_t voff[DS_H + 1];                               // head h owns items voff[h] .. voff[h + 1] - 1
    const int32_t *t_idx[DS_H], *p_idx[DS_H];
    const double *t_val[DS_H], *p_val[DS_H];
    const double* dur;
    uint32_t* s_u32;      // slabs: [chunk][4][items] count, correct, wrong, first_row
    double* s_dur;        //        [chunk][items]
    uint32_t* o_u32;      //        [n_ord][2][n_chunks] true_n, pred_n
    double* o_f64;        //        [n_ord][3][n_chunks] min, max, sq_sum
    wsa_dbstats_cat* cat; wsa_dbstats_class* cls; wsa_dbstats_ord* ord;
};

// K8e's workspace, allocated by the first call that needs it (dbeval.hip)
struct DsEval {
    uint32_t conf_groups = 0, conf_cells = 0;              // the confusion slabs: [conf_groups][conf_cells] u32, conf_cells = the largest V (V + 1)
    uint32_t* d_conf_slab = nullptr;
    uint64_t* d_conf = nullptr;                            // [conf_cells]
    uint32_t* d_agree_n = nullptr;                         // [n_ord][n_chunks]
    double* d_agree_part = nullptr;                        // [n_ord][3][n_chunks]: pass 1 the two sums, pass 3 the three central sums
    double* d_agree_mean = nullptr;                        // [n_ord][2]
    uint64_t* d_agree_count = nullptr;                     // [n_ord]
    wsa_dbstats_agree* d_agree = nullptr;                  // [n_ord]
    // per file (wsa_dbstats_set_files): the rows that belong to a file, in row order, as the tables K6b and RG-1 walk
    wsa_dbstats* files = nullptr;                          // the file-level DB: one row per file, the same heads; owned
    uint32_t n_files = 0, n_sel = 0;
    uint32_t *d_sel = nullptr, *d_row_off = nullptr;       // [n_sel] the DB row of every selected row; [n_files + 1] offsets into the selection
    int32_t* d_meta = nullptr;                             // [n_sel][8]: file, callback, 0, whole milliseconds - 1, 0 ..
    float* d_sel_prob = nullptr; uint32_t sel_prob_width = 0;   // [n_sel][C], the kept probabilities of the selected rows; allocated for sel_prob_width classes
    uint32_t file_sums_width[DS_H] = {};                   // classes d_file_sums[head] was allocated for
    double* d_sel_val = nullptr;                           // [n_sel], a predicted column of the selected rows
    double* d_file_sums[DS_H] = {}; uint32_t file_classes[DS_H] = {};   // [n_files][C] per categorical head, after its wsa_dbstats_fold_files
    int32_t* d_map = nullptr;                              // [WSA_MODEL_MAX_CLASSES] legend_to_vocab of the kept prediction
};

// the folds of a cross-validation (specification CV-1, wsa_dbstats_set_folds; crossval.hip): the rows of every fold, and K6f's table
struct DsFolds {
    uint32_t n_folds = 0;                                  // 0: not set
    std::vector<uint32_t> off;                             // [n_folds + 1] offsets into d_rows
    uint32_t* d_rows = nullptr;                            // the rows of fold 0 ascending, then fold 1's, ..: every row with a fold >= 0 once
    wsa_classify::ClsFoldEntry *h_tab = nullptr, *d_tab = nullptr;   // [n_folds] pinned staging (copied from, not read in place) and the device table
    hipEvent_t done = nullptr;                             // the last launch that read d_tab
    DsFolds() = default;
    DsFolds(const DsFolds&) = delete;
    DsFolds& operator=(const DsFolds&) = delete;
    ~DsFolds() { if (done) { (void)hipEventSynchronize(done); (void)hipEventDestroy(done); } }
};

}  // namespace wsa_dbstats_detail

struct wsa_dbstats {
    wsa_ctx* ctx = nullptr;
    uint32_t n_rows = 0, n_chunks = 0, n_cat = 0, n_ord = 0, items = 0, n_feat = 0;     // n_feat: features per row (53, 264 or 23)
    uint32_t voff[wsa_dbstats_detail::DS_H + 1] = {};
    double *d_feat = nullptr, *d_dur = nullptr;
    int32_t *d_t_idx[wsa_dbstats_detail::DS_H] = {}, *d_p_idx[wsa_dbstats_detail::DS_H] = {};
    double *d_t_val[wsa_dbstats_detail::DS_H] = {}, *d_p_val[wsa_dbstats_detail::DS_H] = {};
    float* d_prob = nullptr; uint32_t prob_classes = 0;     // [n_rows][WSA_MODEL_MAX_CLASSES], allocated by the first wsa_dbstats_predict_classes
    // what the last wsa_dbstats_predict_classes leaves for wsa_dbstats_fold_files beside d_prob: its head, its legend_to_vocab, and a copy
    // of the model's key ranks (Object.keys order of the legend; the model may be gone by then)
    int prob_head = -1; int32_t prob_map[WSA_MODEL_MAX_CLASSES] = {}; int64_t* d_prob_key_rank = nullptr;
    wsa_dbstats_detail::DsTable tab{};
    wsa_dbstats_detail::DsEval eval{};
    wsa::DevArena mem;
    wsa_dbstats_detail::DsFolds folds;                      // (after mem: it waits for its last launch before mem frees the table)
};

namespace wsa_dbstats_detail {

inline wsa_status check_head(wsa_dbstats* db, uint32_t head, bool cat) {
    const uint32_t n = cat ? db->n_cat : db->n_ord;
    if (head >= n) return wsa_api::fail(db->ctx, WSA_ERR_INVALID, std::string(cat ? "categorical" : "ordinal") + " head " + std::to_string(head) + " of " + std::to_string(n));
    return WSA_OK;
}

}  // namespace wsa_dbstats_detail
