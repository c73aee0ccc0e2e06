// debug_classify.hip — test entry of libwsa that is NOT part of include/wsa.h, for the dense classifier K6 / K6e (csrc/classify.hip: classify_kernel through
// launch_classify, classify_group_kernel through launch_classify_group): hand-built feature rows in, the product's own parameter blocks and launches,
// the output tables back whole.
#include <vector>
#include "api_internal.hpp"
#include "debug_internal.hpp"
#include "classify_internal.hpp"

using namespace wsa_debug;

// K6 / K6e (csrc/classify.hip) on hand-built rows through the product's own launches: cls_params / regress_params / launch_classify for one
// model, wsa_ensemble_create / group_table / launch_classify_group for 2 .. 8 (all of 53 inputs: an ensemble's rule).  No kernel code here.
//   feat [feat_rows][stride] f64 (host), stride >= the model's inputs; nan_slot -1, or a slot below stride (a row whose slot is not 0 gets NaN).
//   n_dev >= 0: the row count lives on the device (the batch and stream forms), n_rows is ignored; n_dev < 0: n_rows is the launch's own count
//   (one model only).  rows_cap sizes the grid, as the drivers' capacity does: it may be above or below the count.
//   rb 0: the model's own row-block factor; 1, 2, 4: that one (launch_classify keeps the model's when the LDS does not allow it).
//   one_block (groups): every member with one row block, as a stream step runs them.
//   regress != 0 (one model): the regression epilogue with out_min / out_max; out[0] is then [out_rows] f64, else out[d] is [out_rows][C_d] f32.
// Every out table goes to the device as the caller filled it and comes back whole: what no row writes keeps the caller's pattern.
// Refused, nothing run: a count above feat_rows or out_rows, and whatever else would make a kernel read or write outside these tables.
struct wsa_debug_classify_io {
    const wsa_model* const* models; uint32_t n_models;
    const double* feat; uint32_t feat_rows, stride; int32_t nan_slot;
    uint32_t n_rows, rows_cap; int32_t n_dev, rb, one_block, regress;
    double out_min, out_max;
    void* out[WSA_ENSEMBLE_MAX]; uint32_t out_rows;
};

extern "C" int wsa_debug_classify(const wsa_debug_classify_io* io) {
    using namespace wsa_classify;
    if (!io || !io->models || io->n_models < 1 || io->n_models > WSA_ENSEMBLE_MAX || !io->feat) return WSA_ERR_INVALID;
    const uint32_t M = io->n_models;
    for (uint32_t d = 0; d < M; d++) if (!io->models[d] || !io->out[d] || io->models[d]->ctx != io->models[0]->ctx) return WSA_ERR_INVALID;
    const wsa_model* m0 = io->models[0];
    wsa_ctx* ctx = m0->ctx;
    const bool group = M > 1, regress = io->regress != 0;
    const uint32_t n = io->n_dev >= 0 ? (uint32_t)io->n_dev : io->n_rows;
    if (io->feat_rows < 1 || io->feat_rows > (1u << 22) || io->out_rows < 1 || io->out_rows > (1u << 22) || io->rows_cap < 1 || io->rows_cap > (1u << 22)) return WSA_ERR_INVALID;
    if (n > io->feat_rows || n > io->out_rows || io->stride > 4096 || io->nan_slot >= (int32_t)io->stride) return WSA_ERR_INVALID;
    for (uint32_t d = 0; d < M; d++) if ((int)io->stride < io->models[d]->nin) return WSA_ERR_INVALID;
    if (io->rb != 0 && io->rb != 1 && io->rb != 2 && io->rb != 4) return WSA_ERR_INVALID;
    if (group && (io->n_dev < 0 || regress || io->rb != 0)) return WSA_ERR_INVALID;
    if (!group && io->one_block) return WSA_ERR_INVALID;
    if (regress) if (const char* why = regress_refusal(m0, io->out_min, io->out_max)) return wsa_api::fail(ctx, WSA_ERR_INVALID, why);
    if (hipSetDevice(ctx->device) != hipSuccess) return WSA_ERR_NO_DEVICE;
    wsa::DevArena A;
    double* d_feat = nullptr; uint32_t* d_n = nullptr; ClsGroupEntry* d_tab = nullptr;
    void* d_out[WSA_ENSEMBLE_MAX] = {};
    size_t out_bytes[WSA_ENSEMBLE_MAX] = {};
    const std::vector<uint32_t> count(1, n);
    bool ok = up(A, &d_feat, io->feat, (size_t)io->feat_rows * io->stride) && A.upload(&d_n, count);
    for (uint32_t d = 0; d < M && ok; d++) {
        out_bytes[d] = regress ? (size_t)io->out_rows * sizeof(double) : (size_t)io->out_rows * io->models[d]->C * sizeof(float);
        char* q = nullptr;
        ok = up(A, &q, static_cast<const char*>(io->out[d]), out_bytes[d]);
        d_out[d] = q;
    }
    if (!ok) return WSA_ERR_HIP;
    if (!group) {
        ClsParams p = cls_params(m0, d_feat, n, io->n_dev >= 0 ? d_n : nullptr, regress ? nullptr : static_cast<float*>(d_out[0]));
        p.stride = (int)io->stride; p.nan_slot = io->nan_slot;
        if (regress) p = regress_params(p, static_cast<double*>(d_out[0]), io->out_min, io->out_max - io->out_min);
        launch_classify(m0, p, io->rows_cap, nullptr, io->rb);
    } else {
        wsa_ensemble* e = nullptr;
        if (wsa_ensemble_create(ctx, io->models, M, &e) != WSA_OK) return WSA_ERR_INVALID;
        std::vector<ClsGroupEntry> tab;
        float* prob[WSA_ENSEMBLE_MAX] = {};
        for (uint32_t d = 0; d < M; d++) prob[d] = static_cast<float*>(d_out[d]);
        const uint32_t grid = group_table(e, d_feat, d_n, prob, io->rows_cap, io->one_block != 0, tab);
        for (ClsGroupEntry& t : tab) { t.p.stride = (int)io->stride; t.p.nan_slot = io->nan_slot; }
        const size_t lds = io->one_block ? e->lds_stream : e->lds_batch;
        ok = A.upload(&d_tab, tab);
        if (ok) launch_classify_group(d_tab, M, d_n, grid, lds, nullptr);
        wsa_ensemble_destroy(e);
        if (!ok) return WSA_ERR_HIP;
    }
    ok = ran();
    for (uint32_t d = 0; d < M && ok; d++) ok = down(static_cast<char*>(io->out[d]), static_cast<const char*>(d_out[d]), out_bytes[d]);
    return ok ? WSA_OK : WSA_ERR_HIP;
}
