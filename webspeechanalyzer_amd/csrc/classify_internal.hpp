// classify_internal.hpp — what the classifier's translation units share on the host: classify.hip (K6 / K6e, the model and ensemble
// objects), classify_batch.hip (a batch's fold and its entry points) and classify_stream.hip (the fold inside a stream step).
// Nothing here is exported.
#pragma once
#include <vector>
#include "host_plan.hpp"

namespace wsa_classify {

constexpr int CLS_THREADS = 512;                 // 8 waves: 2 per SIMD
constexpr int L12_NCOEF = 23;                    // level 12: slots 0 .. 22 of a row are the syllable's coefficients, slot 23 the `numeric threw` mark (coeffs.hip)

struct ClsLayer { const float* w; const float* b; int kp, np, n, act; };     // w [kp][np], b [np], zero padded; n = real width
struct ClsParams {
    ClsLayer L[WSA_MODEL_MAX_LAYERS]; int n_layers, C, S;                      // S = LDS row stride (floats)
    const double* in_min; const double* in_max;
    const double* feat; uint32_t n_rows; const uint32_t* d_n_rows;           // rows = *d_n_rows when set (a batch's count, on the device)
    int nin, stride, nan_slot;               // inputs read per row (units[0]); doubles from one row to the next; nan_slot >= 0: a row whose
                                             // slot nan_slot is not 0 (level 12: uncmin threw) gets NaN in every output
    float* prob;
    double* value; double out_min, out_span;                                 // value != NULL: a regression model, one f64 per row instead of prob
    const uint32_t* row_map;                 // K6f only: row i of the launch is row row_map[i] of feat and of prob / value (i < the list's length)
};
struct ClsGroupEntry { ClsParams p; int rb; };   // one member of K6e's work list, with its row-block factor
struct ClsFoldEntry { ClsParams p; int rb; uint32_t n; };   // one member of K6f's work list: its row-block factor and the length of p.row_map

// one member of an ensemble's fold (K6b-e), one wave per (clip, member) or (stream, member).  In a stream step the t_* tables are indexed
// by callback, not by row
struct FoldMember {
    uint32_t C; const float* prob; const int64_t* key_rank;
    int32_t* t_label; double* t_conf; double* t_all_max;                                     // per row: the callback that starts there
    double* t_seg; double* t_all_sum;                                                        // (stream steps only: batches keep these two in LDS)
    double* clip_conf;                                                                       // [n_clips][C]
    int32_t* cb_label; double* cb_conf; double* cb_all_max;                                  // [n_callbacks], written by the compaction
};
// an ensemble's decision per callback (cb_*) and per clip or stream (clip_min_db)
struct EnsTables {
    int32_t* cb; int32_t* cb_db; int32_t* cb_top_label; double* cb_top_conf; int32_t* cb_min_db; double* cb_entropy; int32_t* clip_min_db;
};

// ---- the folds' kernel parameters (the kernels: classify_fold.hpp, classify_batch.hip, classify_stream.hip, knn_fold.hip)
// K6b on a batch: one wave per clip.  P is the type the confidences arrive in (float: K6's probabilities, double: K9's votes / k_eff)
template <typename P>
struct FoldParams {
    uint32_t n_clips, C; double step_s;
    const int32_t* meta; const uint32_t* row_off; const P* prob;
    const int64_t* key_rank;                 // [C] array-index value of the label (0 .. 2^32 - 2), or -1
    int32_t* t_label; double* t_conf; int32_t* t_n; int32_t* t_local;   // per row: the callback that starts there (t_n = 0 elsewhere)
    uint32_t* clip_cb;                       // [n_clips] callbacks per clip
    double* clip_conf;                       // [n_clips][C]
};
// K6b-e on a batch: one wave per (clip, member)
struct FoldGroupParams {
    uint32_t n_clips, n_members; double step_s;
    const int32_t* meta; const uint32_t* row_off; const FoldMember* tab;
    int32_t* t_n; int32_t* t_local; uint32_t* clip_cb;                                       // shared by the members
    EnsTables t;                                                                             // the decision per row (callback starts); cb unused
};
// A stream's fold lives in device memory from step to step: [n][C], [n][C], [n][C], [n].  It starts from nothing when the step's control
// word has START (bit 0: the step's rows belong to the new launch).
struct CarriedFold { double* acc_all; int32_t* in_all; long long* first; long long* stamp; };
// a stream step's callback tables: on the device every callback of the step, in mapped pinned memory those below `cap`
struct StepFoldTables {
    uint32_t cap;
    int32_t* cb; int32_t* cb_label; double* cb_conf;                               // device: every callback of the step
    int32_t* h_cb; int32_t* h_cb_label; double* h_cb_conf; double* h_conf; uint32_t* h_count;   // mapped pinned
};
struct StreamClsParams {
    uint32_t n, C; int fold; double step_s;
    const int32_t* meta; const uint32_t* row_off; const float* prob; const int64_t* key_rank; const uint32_t* bits;
    CarriedFold carried;
    StepFoldTables t;
    float* h_prob;                                                                 // mapped pinned
};
struct StreamKnnParams {
    uint32_t n, C, k; int fold; double step_s;
    const int32_t* meta; const uint32_t* row_off; const uint32_t* bits; const int64_t* key_rank;
    const int32_t* label; const double* conf; const int32_t* nbr; const float* sim;       // K9s' tables of the step
    CarriedFold carried;
    StepFoldTables t;
    int32_t* h_label; double* h_conf; int32_t* h_nbr; float* h_sim;                       // mapped pinned
};
struct StreamMember {
    CarriedFold carried;
    float* h_prob; int32_t* h_cb_label; double* h_cb_conf; double* h_cb_all_max; double* h_conf;   // mapped pinned
};
struct StreamEnsParams {
    uint32_t n, n_members, cap; int fold; double step_s;
    const int32_t* meta; const uint32_t* row_off; const uint32_t* bits;
    const FoldMember* tab; const StreamMember* stab;
    EnsTables o, h;                                                                           // device / mapped pinned (clip_min_db: per stream)
    double* max_inv; int32_t* min_db;                                                         // carried per stream
    uint32_t* h_count;
};

// ---- the folds' launches, with the product's geometry; the drivers and the test entry wsa_debug_class_fold (debug_fold.hip) both go through these
// K6b and its compaction (classify_batch.hip; P = float and double): cb_off [n_clips] scratch, cb [.][4], cb_label, cb_conf per callback,
// host: the callback count
template <typename P>
void launch_fold(const FoldParams<P>& f, uint32_t* cb_off, int32_t* cb, int32_t* cb_label, double* cb_conf, uint32_t* host, hipStream_t s);
// K6b-e and its compaction with the decision (classify_batch.hip): t the per-row decision (f.t), o the per-callback tables
void launch_fold_group(const FoldGroupParams& f, uint32_t* cb_off, const EnsTables& o, uint32_t* host, hipStream_t s);
// the stream step's push / fold kernels (classify_stream.hip, knn_fold.hip)
void launch_stream_classes(const StreamClsParams& p, hipStream_t s);
void launch_stream_knn(const StreamKnnParams& p, hipStream_t s);
void launch_stream_ensemble(const StreamEnsParams& p, hipStream_t s);
// "0", "17" (no sign, no leading zero) up to 2^32 - 2: an array index for Object.keys (classify.hip)
bool array_index_key(const char* s, int64_t* out);

// ---- the launches (classify.hip)
ClsParams cls_params(const wsa_model* m, const double* feat, uint32_t n_rows, const uint32_t* d_n_rows, float* prob);
// rows_cap sizes the grid (classify_grid; the kernel strides over tiles beyond); rb = 16-row blocks per tile (the model's own choice for
// batches; streams pass 1).  A row's probabilities do not depend on the tile it lands in.
void launch_classify(const wsa_model* m, const ClsParams& p, uint32_t rows_cap, hipStream_t s, int rb = 0);
// the same rows through the regression epilogue: value [rows] f64 = the one output unit, un-normalised with the caller's range
inline ClsParams regress_params(ClsParams p, double* value, double out_min, double out_span) {
    p.value = value; p.out_min = out_min; p.out_span = out_span;
    return p;
}
// K6e's device table: the members in work-list order, each with the row-block factor it gets (its own for batches, 1 in a stream step);
// returns the grid, one workgroup per (member, tile) pair of rows_cap rows by classify_grid's rule
uint32_t group_table(const wsa_ensemble* e, const double* feat, const uint32_t* d_n_rows, float* const* prob, uint32_t rows_cap, bool one_block,
                     std::vector<ClsGroupEntry>& tab);
// K6e over the uploaded table: every member's rows (their count on the device) in one launch
void launch_classify_group(const ClsGroupEntry* d_tab, uint32_t n_members, const uint32_t* d_n_rows, uint32_t grid, size_t lds, hipStream_t s);
// K6f's table in work-list order (descending multiply-adds per tile, a stable sort) for members m[0 .. n): member k runs over the n_k =
// off[k + 1] - off[k] rows d_rows[off[k] ..] of feat and writes prob (value == NULL) or value at those rows, un-normalised with its own
// out_min[k] / out_max[k]; tab holds n entries.  Returns the tile count of the launch (0: nothing to launch), *lds the dynamic LDS
uint64_t folds_table(const wsa_model* const* m, uint32_t n, const double* feat, const uint32_t* d_rows, const uint32_t* off, float* prob, double* value,
                     const double* out_min, const double* out_max, ClsFoldEntry* tab, size_t* lds);
// K6f over the uploaded table; tiles > 0
void launch_classify_folds(const wsa_ctx* ctx, const ClsFoldEntry* d_tab, uint32_t n_members, uint64_t tiles, size_t lds, hipStream_t s);
// the tiles of a list of `rows` rows at row-block factor rb
inline uint64_t fold_tiles(uint32_t rows, int rb) { return ((uint64_t)rows + 16u * (uint32_t)rb - 1) / (16u * (uint32_t)rb); }
// what every regression entry point refuses (all WSA_ERR_INVALID); NULL when the model and the range will do
const char* regress_refusal(const wsa_model* m, double out_min, double out_max);

// ---- small host helpers
// one workgroup per tile, up to one per CU
inline uint32_t classify_grid(const wsa_ctx* ctx, uint64_t tiles) {
    const uint64_t n_cu = ctx->n_cu > 0 ? ctx->n_cu : 256;
    return (uint32_t)(tiles < n_cu ? (tiles ? tiles : 1) : n_cu);
}

// a classification state object (wsa_cls, wsa_ecls, wsa_scls, wsa_sens) goes on the device it was made on
template <typename T>
void free_on_device(T* c) {
    if (!c) return;
    (void)hipSetDevice(c->device);
    delete c;
}

// the refusal of every allocation here; a half-built object goes after the message is made (freeing replaces HIP's last error)
inline wsa_status alloc_failed(wsa_ctx* ctx) {
    return wsa_api::fail(ctx, WSA_ERR_HIP, std::string("device allocation failed: ") + hipGetErrorString(hipGetLastError()));
}
template <typename T>
wsa_status alloc_failed(wsa_ctx* ctx, T* half_built) {
    const wsa_status st = alloc_failed(ctx);
    free_on_device(half_built);
    return st;
}

// a stream step beyond the D2H window: one of its tables from the device into x
template <typename T>
inline wsa_status fetch_table(wsa_ctx* ctx, std::vector<T>& x, const T* dev, size_t count, const T** out) {
    x.resize(count + 1);
    if (count) HIP_TRY(ctx, hipMemcpy(x.data(), dev, count * sizeof(T), hipMemcpyDeviceToHost));
    *out = x.data();
    return WSA_OK;
}

// What pairing a model or an ensemble with a batch or with streams refuses alike: a level other than 5 or 13 (entry == NULL: the caller has
// paired level and width itself), a model of another context, (streams) a model of another width than the rows', and at level 13, whose
// fold needs probabilities, a last layer that is not softmax.
enum PairTarget { ON_BATCH, ON_STREAMS };
enum PairSubject { ONE_MODEL, AN_ENSEMBLE };
inline wsa_status pairing_check(wsa_ctx* ctx, const char* entry, PairTarget target, int level, PairSubject subject, const wsa_ctx* made_on, int nin, bool softmax) {
    using wsa_api::fail;
    const bool streams = target == ON_STREAMS, ensemble = subject == AN_ENSEMBLE;
    const std::string noun = ensemble ? "ensemble" : "model";
    if (entry && level != 5 && level != 13)
        return fail(ctx, WSA_ERR_INVALID, std::string(entry) + " needs " + (streams ? "streams" : "a batch") + " at output_level 5 (segment features) or 13 (syllable features), not " + std::to_string(level));
    if (made_on != ctx) return fail(ctx, WSA_ERR_INVALID, "the " + noun + " was created on another context (or device) than the " + (streams ? "streams" : "batch"));
    if (streams && nin != WSA_NFEAT)
        return fail(ctx, WSA_ERR_INVALID, "the model takes " + std::to_string(nin) + " inputs: streams classify the 53-feature rows of output_level 5 and 13");
    if (level == 13 && !softmax)
        return fail(ctx, WSA_ERR_INVALID, std::string("the level-13 fold needs class probabilities: ") + (ensemble ? "a member's" : "the model's") + " last layer is not softmax");
    return WSA_OK;
}

// an EnsTables of R callbacks and N clips or streams on the device (decision_only: without the callback records and the per-clip column),
// and as a mapped pinned pair
inline bool alloc_ens_tables(wsa::DevArena& A, EnsTables& t, size_t R, size_t N, bool decision_only = false) {
    return A.alloc(&t.cb_db, R) && A.alloc(&t.cb_top_label, R) && A.alloc(&t.cb_top_conf, R) && A.alloc(&t.cb_min_db, R) && A.alloc(&t.cb_entropy, R)
           && (decision_only || (A.alloc(&t.cb, R * 4) && A.alloc(&t.clip_min_db, N)));
}
inline bool pin_ens_tables(wsa::DevArena& A, EnsTables& host, EnsTables& dev, size_t R, size_t N) {
    return A.pin(&host.cb, &dev.cb, R * 4) && A.pin(&host.cb_db, &dev.cb_db, R) && A.pin(&host.cb_top_label, &dev.cb_top_label, R)
           && A.pin(&host.cb_top_conf, &dev.cb_top_conf, R) && A.pin(&host.cb_min_db, &dev.cb_min_db, R)
           && A.pin(&host.cb_entropy, &dev.cb_entropy, R) && A.pin(&host.clip_min_db, &dev.clip_min_db, N);
}

}  // namespace wsa_classify

struct wsa_model {
    wsa_ctx* ctx = nullptr;
    int n_layers = 0, C = 0, S = 0, rb = 0, nin = 0;      // nin = units[0], the row width of the level the model was trained at
    wsa_classify::ClsLayer L[WSA_MODEL_MAX_LAYERS] = {};
    double *d_min = nullptr, *d_max = nullptr;
    int64_t* d_key_rank = nullptr;
    std::vector<int64_t> key_rank;           // d_key_rank as the host made it
    bool softmax = false;
    wsa::DevArena mem;
};

struct wsa_ensemble {
    wsa_ctx* ctx = nullptr;
    uint32_t n = 0;
    const wsa_model* m[WSA_ENSEMBLE_MAX] = {};
    int order[WSA_ENSEMBLE_MAX] = {};        // members by descending cost per tile (K6e's work list)
    bool softmax = true;                     // every member ends in softmax
    size_t lds_batch = 0, lds_stream = 0;    // the largest member's need, with its own row-block factor / with one row block
    uint64_t serial = 0;                     // tells a new ensemble at a recycled address from the one a table was built for
};
