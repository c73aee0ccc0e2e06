// api_internal.hpp — what the sources behind include/wsa.h share (api.hip: context and host helpers, batch_*.hip: batches, stream_*.hip:
// streams): the context object and the error plumbing of the C ABI.
#pragma once
#include <string>
#include "wsa_internal.hpp"

struct wsa_ctx {
    wsa_config cfg;
    int device = 0;
    int n_cu = 0;
    std::string err;
};

namespace wsa_api {
extern thread_local std::string g_create_error;
inline wsa_status fail(wsa_ctx* c, wsa_status st, const std::string& msg) {
    if (c) c->err = msg; else g_create_error = msg;
    return st;
}
#pragma GCC visibility push(hidden)
// api.hip: the page-locked slab of wsa_host_alloc that p lies in, if any (batch_input.hip merges uploads only inside one)
bool slab_of(const void* p, uintptr_t* base, size_t* size);
#pragma GCC visibility pop
}  // namespace wsa_api

// classify_batch.hip (K6 / K6b) reads a batch's compacted rows and keeps its own per-batch state; batch_internal.hpp has the batch object
struct wsa_cls;                                 // classification buffers of one batch (allocated by the first wsa_batch_classify)
void wsa_cls_free(wsa_cls* c);                  // (wsa_batch_destroy)
struct wsa_ecls;                                // ensemble tables of one batch (allocated by the first wsa_batch_classify_ensemble with an ensemble)
void wsa_ecls_free(wsa_ecls* c);
struct wsa_kcls;                                // KNN tables of one batch (allocated by the first wsa_batch_knn, knn.hip)
void wsa_kcls_free(wsa_kcls* c);
struct wsa_rcls;                                // regression-group tables of one batch (allocated by the first wsa_batch_regress_group, regress_fold.hip)
void wsa_rcls_free(wsa_rcls* c);
struct wsa_batch_view {
    wsa_ctx* ctx; int level; uint32_t n_clips, rows_cap;
    const int32_t* d_meta; const double* d_feat; const uint32_t* d_row_off;     // compacted rows, d_row_off[n_clips] = rows on the device
    const double* d_utt_feat; const uint32_t* d_utt_off; uint32_t utt_cap;      // level 11: utterance rows [..][WSA_NUTT], d_utt_off[n_clips] = their count on the device
    uint32_t reruns;                                                            // wsa_batch_backend_reruns
    wsa_cls** cls; wsa_ecls** ecls; wsa_kcls** kcls; wsa_rcls** rcls;
    int* cls_last;                                                              // 1: the last classification was one model's, 2: an ensemble's, 3: wsa_batch_regress, 4: wsa_batch_regress_group
};
extern "C" {
void wsa_batch_view_internal(wsa_batch* b, wsa_batch_view* v);
// fetch_totals: synchronise, read the counters (reruns the back end on a table overflow)
wsa_status wsa_batch_fetch_internal(wsa_batch* b, hipStream_t s);
// debug.hip (wsa_debug_batch_tiers): keep >= 0 sets whether the batch's runs leave their device counters standing (1) instead of having the fused
// compaction clear them for the next run (0, the default); returns the batch's 16 device counters
const uint32_t* wsa_batch_counters_internal(wsa_batch* b, int keep, wsa_ctx** ctx);
// debug.hip (wsa_debug_stream_spectra): the u32 frames of a stream set's last step on the device, [n_streams][frames_per_step][bands]
const uint32_t* wsa_stream_spec_internal(wsa_stream* b, wsa_ctx** ctx, uint32_t* n_streams, uint32_t* frames_per_step, uint32_t* bands);
// debug.hip (wsa_debug_stream_ctl): the device control words of a stream set's last step, word w of stream s at [w * n_streams + s]
const uint32_t* wsa_stream_ctl_internal(wsa_stream* b, wsa_ctx** ctx, uint32_t* n_streams, int* mixed);
// debug.hip (wsa_debug_stream_step_backend): one step of a plain stream set from hand-built u32 frames, the product's back-end launches behind them
wsa_status wsa_stream_step_backend_internal(wsa_stream* b, const uint32_t* n_frames, const uint8_t* ctl, const uint32_t* frames, uint32_t bands, void* stream);
void wsa_model_info_internal(const wsa_model* m, wsa_ctx** ctx, int* n_classes, int* softmax);   // classify.hip, for dbstats.hip (K8)
int wsa_model_inputs_internal(const wsa_model* m);                                               // units[0]
const int64_t* wsa_model_key_rank_internal(const wsa_model* m);                                  // device [classes]: the legend's Object.keys ranks (K8e's per-file fold)
}

// classify_stream.hip runs K6 / K6b inside a stream object's step (wsa_stream_set_model); stream_internal.hpp has the stream object
struct wsa_scls;                                // classification state of one stream object: class tables, carried fold, pinned D2H tables
struct wsa_scls_view {
    wsa_ctx* ctx; int level; uint32_t n_streams, rows_cap, d2h_rows;
    const int32_t* d_meta; const double* d_feat; const uint32_t* d_row_off;     // the step's compacted rows, d_row_off [n_streams + 1]
    const uint32_t* d_totals;                                                   // [0] = rows of the step, on the device
    const uint32_t* d_bits;                                                     // per stream control word of the step (bit 0: START)
};
wsa_status wsa_scls_create(const wsa_scls_view& v, const wsa_model* m, wsa_scls** out);   // checks the model, allocates, zeroes the fold state
void wsa_scls_free(wsa_scls* c);
wsa_status wsa_scls_enqueue(wsa_scls* c, hipStream_t s);                                   // part of enqueue_step (captured)
wsa_status wsa_scls_result(wsa_scls* c, uint32_t rows, wsa_stream_class_result* out);    // after the step completed
// ... or K6e and the ensemble's folds and decision (wsa_stream_set_ensemble)
struct wsa_sens;
wsa_status wsa_sens_create(const wsa_scls_view& v, const wsa_ensemble* e, wsa_sens** out);
void wsa_sens_free(wsa_sens* c);
wsa_status wsa_sens_enqueue(wsa_sens* c, hipStream_t s);
wsa_status wsa_sens_result(wsa_sens* c, uint32_t rows, wsa_stream_ensemble_result* out);

// ... and, beside either, K9s and the fold KN-2 with an attached KNN store (wsa_stream_set_knn; knn_fold.hip)
struct wsa_sknn;
wsa_status wsa_sknn_create(const wsa_scls_view& v, const wsa_knn* kn, uint32_t k, wsa_sknn** out);   // checks the store and k, allocates, zeroes the fold state
void wsa_sknn_free(wsa_sknn* c);
wsa_status wsa_sknn_enqueue(wsa_sknn* c, hipStream_t s);
wsa_status wsa_sknn_result(wsa_sknn* c, uint32_t rows, wsa_stream_knn_result* out);

// ... and, beside all of them, grouped K6 over regression heads and the fold RG-1 (wsa_stream_set_regress; regress_fold.hip)
struct wsa_sreg;
wsa_status wsa_sreg_create(const wsa_scls_view& v, const wsa_regress_group* g, wsa_sreg** out);     // checks the level, allocates, zeroes the carried sums
void wsa_sreg_free(wsa_sreg* c);
wsa_status wsa_sreg_enqueue(wsa_sreg* c, hipStream_t s);
wsa_status wsa_sreg_result(wsa_sreg* c, uint32_t rows, wsa_stream_value_result* out);

// ... and, beside all of those, the step's rows appended to a device feature DB (wsa_stream_set_featdb, spec FD-2; stream_featdb.hip)
struct wsa_sfdb;
struct wsa_sfdb_view {
    wsa_ctx* ctx; int level; uint32_t n_streams;
    uint32_t rows_cap;                                     // rows the source table can hold (level 11: utterance rows)
    const int32_t* d_meta; const double* d_feat; uint32_t stride;      // the source table (level 11: the utterance rows, stride WSA_NUTT)
    const uint32_t* d_utt_off;                             // level 11: [n_streams + 1] utterance-row offsets of the step
    const uint32_t* d_n_rows;                              // device word: rows in the source table
    const uint32_t *d_flags, *d_lost;                      // device words: bit 0 of *d_flags, or a nonzero *d_lost (may be NULL), is WSA_FLAG_CAPACITY
    const uint32_t* d_bits;                                // per stream control word of the step (bit 0: START)
    const void* owner;                                     // the stream set (a DB feeds one)
};
// checks the DB against the view (context, level / width, not attached elsewhere), allocates everything, marks the DB attached.
// d_slot: level 11's slot table [n_streams] if the caller owns it (the test entry), NULL: allocated here, all -1
wsa_status wsa_sfdb_create(const wsa_sfdb_view& v, wsa_featdb* db, int32_t* d_slot, wsa_sfdb** out);
void wsa_sfdb_free(wsa_sfdb* c);                           // (the DB is attached to nothing afterwards, unless it was attached again meanwhile)
void wsa_sfdb_begin_step(wsa_sfdb* c);                     // host side, the previous step done: settles it, hands the DB's count to the step about to be launched
wsa_status wsa_sfdb_enqueue(wsa_sfdb* c, hipStream_t s);   // part of enqueue_step (captured): the plan and the copy kernel
uint32_t wsa_sfdb_settle(wsa_sfdb* c);                     // the launched step is done: reads its outcome once, advances the DB's count; returns not_fitted
wsa_status wsa_sfdb_result(wsa_sfdb* c, wsa_stream_db_result* out);
extern "C" wsa_status wsa_sfdb_debug_step(wsa_featdb* db, int32_t level, const int32_t* d_meta, const double* d_feat, uint32_t feat_stride, uint32_t rows_cap,
                                          const uint32_t* d_utt_off, uint32_t n_streams, const uint32_t* d_n_rows, const uint32_t* d_flags, const uint32_t* d_bits,
                                          int32_t* d_slot, void* stream, uint32_t* out4, int32_t* kept, uint32_t kept_cap, int32_t* replaced, uint32_t replaced_cap);

// classify.hip: NULL for the row width of an ML level (53, 264, 23), else the rest of the refusal after "the model takes N"
const char* wsa_model_width_refusal(int n_inputs);

#define HIP_TRY(ctx, call) do { hipError_t e_ = (call); if (e_ != hipSuccess) \
        return wsa_api::fail((ctx), WSA_ERR_HIP, std::string(#call) + ": " + hipGetErrorString(e_)); } while (0)
