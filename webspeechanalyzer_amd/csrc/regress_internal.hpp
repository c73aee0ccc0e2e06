// regress_internal.hpp — what regress_fold.hip (regression groups: the grouped K6 over regression heads and the fold RG-1, on batches
// and inside a stream step) shares with debug_fold.hip (wsa_debug_regress_fold): the group object, the two fold kernels' parameter blocks
// and their launches.  Nothing here is exported.
#pragma once
#include "classify_internal.hpp"

struct wsa_regress_group {
    wsa_ctx* ctx = nullptr;
    int device = 0;
    uint32_t n = 0;
    const wsa_model* m[WSA_REGRESS_GROUP_MAX] = {};
    double out_min[WSA_REGRESS_GROUP_MAX] = {}, out_span[WSA_REGRESS_GROUP_MAX] = {};
    int order[WSA_REGRESS_GROUP_MAX] = {};   // heads by descending cost per tile (the grouped launch's work list)
    size_t lds_batch = 0, lds_stream = 0;    // the largest member's need, with its own row-block factor / with one row block
    uint64_t serial = 0;                     // tells a new group at a recycled address from the one a table was built for
    // wsa_regress_group_rows: the launch table and, behind its last entry, the row count (h_n, d_n point there), staged in pinned memory and
    // copied to the device by one copy in front of the launch;
    // `done` is recorded behind the launch, and the next call waits for it before it rewrites the staging
    wsa_classify::ClsGroupEntry *h_tab = nullptr, *d_tab = nullptr;
    uint32_t *h_n = nullptr, *d_n = nullptr;
    hipEvent_t done = nullptr;
    wsa::DevArena mem;
};

namespace wsa_regress {

// ---- RG-1 on a batch: one wave per clip.  Like K6b, a callback's figures are left at the row it starts at (t_*), and the compaction turns
// them into per-callback tables in (clip, callback) order: the same order and the same cb records as K6b's.
struct RegressFoldParams {
    uint32_t n_clips, H, stride;                                   // stride: doubles from one head's column to the next in t_* / cb_*
    double step_s;
    const int32_t* meta; const uint32_t* row_off;
    const double* value[WSA_REGRESS_GROUP_MAX];                    // [rows] per head
    double* t_value; double* t_weight; int32_t* t_n; int32_t* t_local;
    uint32_t* clip_cb; uint32_t* cb_off;                           // [n_clips] callbacks per clip, their offsets
    double* clip_sum; double* clip_weight; double* clip_value;     // [H][n_clips]
    int32_t* cb; double* cb_value; double* cb_weight;              // [..][4], [H][stride]
    uint32_t* host;                                                // mapped pinned: the number of callbacks
};
void launch_regress_fold(const RegressFoldParams& p, hipStream_t s);      // the fold, then the compaction

// ---- RG-1 on a stream step: one wave per stream, the running sums carried in device memory from step to step ([H][n]); they start from
// zero when the step's control word has START (bit 0).  Callbacks go straight to their place in the step's tables (callback_starts); the
// rows' values, the callbacks below the D2H window `cap` and the running sums also go to mapped pinned tables.
struct RegressStepParams {
    uint32_t n, H, stride, cap;                                    // stride: as above, for value / cb_value / cb_weight; the pinned tables' is cap
    int fold; double step_s;                                       // fold 0 (level 5): the rows' values are pushed and nothing else
    const int32_t* meta; const uint32_t* row_off; const uint32_t* bits;
    const double* value[WSA_REGRESS_GROUP_MAX];
    double* run_sum; double* run_weight;                           // carried [H][n]
    int32_t* cb; double* cb_value; double* cb_weight;              // device: every callback of the step, [..][4], [H][stride]
    double* h_value; int32_t* h_cb; double* h_cb_value; double* h_cb_weight;      // mapped pinned: [H][cap], [cap][4], [H][cap]
    double* h_sum; double* h_weight; double* h_run_value;          // mapped pinned [H][n]
    uint32_t* h_count;
};
void launch_regress_step(const RegressStepParams& p, hipStream_t s);

}  // namespace wsa_regress
