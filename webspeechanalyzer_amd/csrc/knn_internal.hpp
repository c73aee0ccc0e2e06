// knn_internal.hpp — what the KNN classifier's translation units share on the host: knn.hip (the store, K9 and K9s, the row and batch
// entry points) and knn_fold.hip (KN-2: the per-callback fold over KNN confidences for batches, and K9s + KN-2 inside a stream step).
// Nothing here is exported.
#pragma once
#include <memory>
#include "host_plan.hpp"

namespace wsa_knn_detail {
// K9s' scratch table for `window` query rows and a slice count
struct KnnSplit {
    uint32_t window = 0, slices = 0, tiles_per_slice = 0;
    float* key = nullptr; int32_t *rank = nullptr, *idx = nullptr, *cnt = nullptr;
};
}  // namespace wsa_knn_detail

struct wsa_knn {
    wsa_ctx* ctx = nullptr;
    int width = 0, wp = 0, C = 0;
    uint32_t cap = 0, count = 0;
    float* d_rows = nullptr;
    int32_t *d_cls = nullptr, *d_within = nullptr, *d_rank = nullptr;
    uint32_t *d_class_count = nullptr, *d_bad = nullptr;
    wsa::DevArena mem;
    // wsa_debug_knn_split's scratch table, kept from call to call (test access only; a stream set has its own)
    struct DebugSplit { std::unique_ptr<wsa::DevArena> mem; wsa_knn_detail::KnnSplit sp; uint32_t k = 0, count = 0; };
    mutable DebugSplit debug_split;
};

struct wsa_kfold;                                // KN-2's tables of one batch (the first wsa_batch_knn_fold allocates them, knn_fold.hip)
void wsa_kfold_free(wsa_kfold* f);

// the KNN tables of one batch (the first wsa_batch_knn allocates them)
struct wsa_kcls {
    int device = 0;
    uint32_t cap_rows = 0, cap_c = 0, cap_k = 0;
    int32_t *d_label = nullptr, *d_nbr = nullptr; double* d_conf = nullptr; float* d_sim = nullptr;
    const wsa_knn* knn = nullptr; uint32_t k = 0, k_eff = 0, reruns = 0; int level = 0;
    wsa_kfold* fold = nullptr;
    wsa::DevArena mem;
};

namespace wsa_knn_detail {

struct KnnParams {
    const float* rows; const int32_t* cls; const int32_t* rank; uint32_t n_store;
    const double* feat; uint32_t n_rows; const uint32_t* d_n_rows;          // rows = *d_n_rows when set (a batch's count, on the device)
    int width, stride, nan_slot;             // features read per row; doubles from one row to the next; nan_slot >= 0: a row whose slot
                                             // nan_slot is not 0 (level 12: uncmin threw) gets label -1 and NaN in every other output
    int C; uint32_t k, k_eff;                // k_eff = min(k, n_store): ml5 clamps k to the number of examples
    int32_t* label; double* conf; int32_t* nbr; float* sim;                 // any may be NULL
    uint32_t qt0;                            // the first query tile (0; a stream step hands K9 only the rows past its D2H window)
    // K9s: the store in `slices` runs of tiles_per_slice whole tiles, rows below q_limit only (0: all); a (query, slice) pair's partial
    // list is entries [(q * slices + slice) * k ..] of pt_key / pt_rank / pt_idx, its length pt_cnt[q * slices + slice]
    uint32_t slices, tiles_per_slice, q_limit;
    float* pt_key; int32_t* pt_rank; int32_t* pt_idx; int32_t* pt_cnt;
};

KnnParams knn_params(const wsa_knn* kn, const double* feat, uint32_t n_rows, const uint32_t* d_n_rows, uint32_t k);
// what every classification refuses: k outside 1 .. WSA_KNN_MAX_K and a store without examples
wsa_status knn_refusal(const wsa_knn* kn, uint32_t k);
// K9: rows_cap sizes the grid (the kernel strides over query tiles beyond it)
void launch_knn(const wsa_knn* kn, const KnnParams& p, uint32_t rows_cap, hipStream_t s);
// K9s' slice count for `window` query rows against the store as it stands (the rule is at its definition and in include/wsa.h)
uint32_t knn_split_slices(const wsa_knn* kn, uint32_t window, uint32_t k);
// the scratch of `slices` slices (0: the rule's) for `window` rows; false when the device has no room
bool knn_split_alloc(wsa::DevArena& A, const wsa_knn* kn, uint32_t window, uint32_t k, uint32_t slices, KnnSplit& out);
// K9s over the rows below sp.window (p as for launch_knn): the partial kernel, then the merge
void launch_knn_split(const wsa_knn* kn, KnnParams p, const KnnSplit& sp, hipStream_t s);

}  // namespace wsa_knn_detail
