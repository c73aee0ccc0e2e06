// train.hip — K7: minibatch SGD for the app's Dense classifiers (specification TR-1) and Adam for its regression models
// (TR-2): the solo trainer's kernels and its part of the C ABI (include/wsa.h "Training").  The stages themselves, and how their
// parameters follow from a trainer's description, are train_stages.hpp; a group of trainers stepped in lock step is train_group.hip.
//
// Stands in for the reference APPLICATION's training path: src/neuralmodel.js:163-403 (train_nn) -> ml5 0.6.0
// neuralNetwork.train: tfjs 1.7.2 model.fit with categoricalCrossentropy, tf.train.sgd(learningRate), metrics ["accuracy"].
#include <cmath>
#include <cstring>
#include <string>
#include <vector>
#include "train_internal.hpp"
#include "featdb_internal.hpp"

using wsa_api::fail;
using namespace wsa_train;

namespace {

// ---- the solo kernels: a stage of ONE trainer, its parameters built on the host (train_stages.hpp) and passed by value
__global__ void __launch_bounds__(TR_THREADS) train_forward_kernel(TrFwd p) { tr_forward_body(p, blockIdx.x); }

__global__ void __launch_bounds__(TR_LOSS_THREADS) train_loss_kernel(TrLoss p) {
    __shared__ double s_loss[TR_LOSS_THREADS];
    __shared__ uint32_t s_hit[TR_LOSS_THREADS];
    tr_loss_body(p, s_loss, s_hit);
}

__global__ void __launch_bounds__(TR_THREADS) train_backward_kernel(TrBack p) { tr_backward_body(p, blockIdx.x); }

__global__ void __launch_bounds__(TR_THREADS) train_update_kernel(TrUpd p) { tr_update_body<TrSgd>(p, blockIdx.x); }

__global__ void __launch_bounds__(TR_LOSS_THREADS) train_loss_mse_kernel(TrLossMse p) {
    __shared__ double s_loss[TR_LOSS_THREADS];
    __shared__ uint32_t s_hit[TR_LOSS_THREADS];
    tr_loss_mse_body(p, s_loss, s_hit);
}

__global__ void __launch_bounds__(TR_THREADS) train_update_adam_kernel(TrUpdAdam q) { tr_update_body<TrAdam>(q, blockIdx.x); }

__global__ void train_adam_reset_kernel(float* adam) {                      // accBeta = beta: no step taken yet
    if (threadIdx.x == 0 && blockIdx.x == 0) { adam[0] = ADAM_BETA1; adam[1] = ADAM_BETA2; adam[2] = 1.f - ADAM_BETA1; adam[3] = 1.f - ADAM_BETA2; }
}

// ---- create: a regression model's targets, (y - min) / (max - min) in double, rounded to f32 (ml5 normalizeData on the output `y`)
__global__ void __launch_bounds__(256) train_normalise_target_kernel(const double* y, double mn, double mx, uint64_t n_rows, float* t) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n_rows) t[i] = (float)((y[i] - mn) / (mx - mn));
}

__global__ void __launch_bounds__(TR_FINISH_THREADS) train_finish_kernel(TrFin p) {
    __shared__ double s_loss[TR_FINISH_THREADS];
    __shared__ uint32_t s_hit[TR_FINISH_THREADS];
    tr_finish_body(p, s_loss, s_hit);
}

// ---- create: (x - min) / (max - min) in double, rounded to f32 (ml5 normalizeValue, as K6); feat [n_rows][nin] dense, x [n_rows][xs],
// xs = nin padded to 16-column blocks, the padding written as zero
__global__ void __launch_bounds__(256) train_normalise_kernel(const double* feat, const double* mn, const double* mx, uint64_t n_rows, int nin, int xs, float* x) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n_rows * (uint64_t)xs) return;
    const uint64_t r = i / (uint64_t)xs; const int k = (int)(i % (uint64_t)xs);
    x[i] = k < nin ? (float)((feat[r * (uint64_t)nin + k] - mn[k]) / (mx[k] - mn[k])) : 0.f;
}

// ---- create from a device feature DB (FD-1): the same, x[r] from row rows[r] of the DB's dense table
__global__ void __launch_bounds__(256) train_normalise_db_kernel(const double* db, const uint32_t* rows, const double* mn, const double* mx, uint64_t n_rows, int nin, int xs, float* x) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n_rows * (uint64_t)xs) return;
    const uint64_t r = i / (uint64_t)xs; const int k = (int)(i % (uint64_t)xs);
    x[i] = k < nin ? (float)((db[(uint64_t)rows[r] * (uint64_t)nin + k] - mn[k]) / (mx[k] - mn[k])) : 0.f;
}

// one launch of the solo trainer's epoch: the stage's kernel on the parameters built from the description; idx: the order or identity buffer
void solo_launch(wsa_trainer* t, const uint32_t* idx, TrStage stage, uint32_t step, int pos, hipStream_t s) {
    const TrainDesc& d = t->desc;
    const TrStep r = tr_step(d, step, idx);
    const dim3 grid(stage_blocks(d, stage, step, pos));
    switch (stage) {
        case TR_FORWARD: hipLaunchKernelGGL(train_forward_kernel, grid, dim3(TR_THREADS), 0, s, tr_forward_params(d, r, pos)); break;
        case TR_LOSS:
            if (d.regress) hipLaunchKernelGGL(train_loss_mse_kernel, grid, dim3(TR_LOSS_THREADS), 0, s, tr_loss_mse_params(d, r));
            else hipLaunchKernelGGL(train_loss_kernel, grid, dim3(TR_LOSS_THREADS), 0, s, tr_loss_params(d, r));
            break;
        case TR_BACKWARD: hipLaunchKernelGGL(train_backward_kernel, grid, dim3(TR_THREADS), 0, s, tr_backward_params(d, r, pos)); break;
        case TR_UPDATE: {
            const TrUpd u = tr_update_params(d, r, pos);
            if (d.regress) hipLaunchKernelGGL(train_update_adam_kernel, grid, dim3(TR_THREADS), 0, s, tr_update_adam_params(d, u, pos));
            else hipLaunchKernelGGL(train_update_kernel, grid, dim3(TR_THREADS), 0, s, u);
            break;
        }
        case TR_FINISH: hipLaunchKernelGGL(train_finish_kernel, grid, dim3(TR_FINISH_THREADS), 0, s, tr_finish_params(d, ++t->epoch)); break;
    }
}

// what trainer_create is asked for; label != NULL a classifier's (TR-1), target != NULL a regression model's (TR-2)
struct CreateArgs {
    const wsa_model_desc* d; const double* feat; const int32_t* label; const double* target; bool regress;
    uint32_t n_rows, n_val, batch_size; double learning_rate, out_min, out_max;
    const wsa_featdb* db = nullptr; const uint32_t* rows = nullptr;          // wsa_trainer_create_db: row r is DB row rows[r], feat is NULL
};

// "" or why the arguments are refused; host only, nothing is allocated before it has passed
std::string create_refusal(const CreateArgs& a) {
    const wsa_model_desc* d = a.d;
    const int nl = d->n_layers;
    if (nl < 1 || nl > WSA_MODEL_MAX_LAYERS) return "a model has 1 .. 8 Dense layers, got " + std::to_string(nl);
    if (!d->units || !d->activation || !d->kernel || !d->bias) return "null units / activation / kernel / bias array";
    if (const char* why = wsa_model_width_refusal(d->units[0])) return "the model takes " + std::to_string(d->units[0]) + why;
    const int nin = d->units[0];
    for (int l = 0; l < nl; l++) {
        const int u = d->units[l + 1], act = d->activation[l];
        if (u < 1 || u > WSA_MODEL_MAX_WIDTH) return "layer " + std::to_string(l) + " has " + std::to_string(u) + " units (limit 1024)";
        if (act < WSA_ACT_LINEAR || act > WSA_ACT_SOFTMAX) return "layer " + std::to_string(l) + ": unknown activation " + std::to_string(act);
        if (act == WSA_ACT_SOFTMAX && l != nl - 1) return "softmax is only supported on the last layer";
        if (!d->kernel[l] || !d->bias[l]) return "null kernel / bias of layer " + std::to_string(l);
    }
    if (a.regress) {
        if (d->activation[nl - 1] == WSA_ACT_SOFTMAX) return "a regression model's last layer is linear, relu, sigmoid or tanh, not softmax (meanSquaredError)";
        if (d->units[nl] != 1) return "a regression model has one output unit, got " + std::to_string(d->units[nl]);
    } else if (d->activation[nl - 1] != WSA_ACT_SOFTMAX) return "training needs a softmax output layer (categoricalCrossentropy)";
    const int C = d->units[nl];
    if (C > WSA_MODEL_MAX_CLASSES) return "the output layer has " + std::to_string(C) + " units (limit 64)";
    if (!d->in_min || !d->in_max) return "null in_min / in_max";
    for (int k = 0; k < nin; k++) {
        if (!std::isfinite(d->in_min[k]) || !std::isfinite(d->in_max[k])) return "non-finite in_min / in_max of input " + std::to_string(k);
        if (d->in_max[k] == d->in_min[k]) return "feature " + std::to_string(k) + " has max == min: it cannot be normalised";
    }
    if ((a.db ? !a.rows : !a.feat) || (a.regress ? !a.target : !a.label)) return a.regress ? "null feature / target pointer" : "null feature / label pointer";
    if (a.db) {
        if (a.db->width != nin) return "the model takes " + std::to_string(nin) + " inputs; the DB's rows have " + std::to_string(a.db->width) + " features";
        const std::string why = wsa_fd::rows_refusal(a.db, a.rows, a.n_rows);
        if (!why.empty()) return why;
    }
    if (a.n_val >= a.n_rows) return "n_val " + std::to_string(a.n_val) + " leaves no training rows of " + std::to_string(a.n_rows);
    if (a.batch_size == 0) return "batch_size must be at least 1";
    if (!std::isfinite(a.learning_rate) || !std::isfinite((float)a.learning_rate)) return "the learning rate is not finite as an f32";
    if (a.regress) {
        if (!std::isfinite(a.out_min) || !std::isfinite(a.out_max)) return "non-finite out_min / out_max";
        if (a.out_max == a.out_min) return "the output has max == min: it cannot be normalised";
        for (uint32_t r = 0; r < a.n_rows; r++)
            if (!std::isfinite(a.target[r]) || !std::isfinite((float)((a.target[r] - a.out_min) / (a.out_max - a.out_min))))
                return "the target of row " + std::to_string(r) + " is not finite as a normalised f32";
    }
    if (!a.regress) for (uint32_t r = 0; r < a.n_rows; r++)
        if (a.label[r] < 0 || a.label[r] >= C) return "label " + std::to_string(a.label[r]) + " of row " + std::to_string(r) + " is outside 0 .. " + std::to_string(C - 1);
    return std::string();
}

// t's shapes are set: its buffers, filling the description as they are allocated, and what create computes on the device (the
// normalised rows and targets, Adam's first state).  false: an allocation, a copy or a launch failed, and t is to be destroyed
bool create_buffers(wsa_trainer* t, const CreateArgs& a) {
    const wsa_model_desc* d = a.d;
    TrainDesc& D = t->desc;
    wsa::DevArena& M = t->mem;
    const uint32_t n_rows = a.n_rows;
    const int nl = D.nl, nin = D.units[0];
    const size_t xs = (size_t)D.pad[0];                                       // stride of the normalised rows
    int pmax = 0;
    for (int l = 1; l <= nl; l++) if (D.pad[l] > pmax) pmax = D.pad[l];
    for (int l = 0; l < nl; l++) {                                            // zero padded as K6 pads them
        const int K = d->units[l], N = d->units[l + 1], kp = D.pad[l], np = D.pad[l + 1];
        std::vector<float> w((size_t)kp * np, 0.f), bb(np, 0.f);
        for (int k = 0; k < K; k++) std::memcpy(&w[(size_t)k * np], d->kernel[l] + (size_t)k * N, N * sizeof(float));
        std::memcpy(bb.data(), d->bias[l], N * sizeof(float));
        if (!(M.upload(&D.w[l], w) && M.upload(&D.b[l], bb) && M.alloc(&D.a[l + 1], (size_t)t->mcap * np, true))) return false;
        if (a.regress && !(M.alloc(&D.mw[l], w.size(), true) && M.alloc(&D.vw[l], w.size(), true)
                           && M.alloc(&D.mb[l], bb.size(), true) && M.alloc(&D.vb[l], bb.size(), true))) return false;
    }
    std::vector<uint32_t> ident(D.n_train);
    for (uint32_t i = 0; i < D.n_train; i++) ident[i] = i;
    if (!(M.alloc(&D.dz[0], (size_t)t->mcap * pmax, true) && M.alloc(&D.dz[1], (size_t)t->mcap * pmax, true) && M.alloc(&D.x, (size_t)n_rows * xs)
          && (a.regress ? M.alloc(&D.target, n_rows) && M.alloc(&D.adam, 4) : M.alloc(&D.label, n_rows))
          && M.alloc(&D.order, D.n_train) && M.upload(&D.identity, ident)
          && M.alloc(&D.part_loss, D.n_steps + 1, true) && M.alloc(&D.part_hit, D.n_steps + 1, true) && M.alloc(&D.stats, 1, true))) return false;
    for (int i = 0; i < 2; i++)                                               // the order's staging
        if (hipHostMalloc(reinterpret_cast<void**>(&t->h_order[i]), (size_t)D.n_train * sizeof(uint32_t), hipHostMallocDefault) != hipSuccess) return false;
    for (int i = 0; i < 2; i++) if (hipEventCreateWithFlags(&t->ev[i], hipEventDisableTiming) != hipSuccess) return false;
    wsa::DevArena tmp;                                                        // the double rows live only until they are normalised
    double *d_feat = nullptr, *d_mn = nullptr, *d_mx = nullptr, *d_y = nullptr;
    uint32_t* d_rows = nullptr;
    if (a.db) {                                                               // the DB's rows stay where they are: only the row list travels
        if (!(hipDeviceSynchronize() == hipSuccess && tmp.alloc(&d_rows, (size_t)n_rows)
              && hipMemcpy(d_rows, a.rows, (size_t)n_rows * sizeof(uint32_t), hipMemcpyHostToDevice) == hipSuccess)) return false;
    } else if (!(tmp.alloc(&d_feat, (size_t)n_rows * nin)
                 && hipMemcpy(d_feat, a.feat, (size_t)n_rows * nin * sizeof(double), hipMemcpyHostToDevice) == hipSuccess)) return false;
    if (!(tmp.alloc(&d_mn, (size_t)nin) && tmp.alloc(&d_mx, (size_t)nin)
          && hipMemcpy(d_mn, d->in_min, (size_t)nin * sizeof(double), hipMemcpyHostToDevice) == hipSuccess
          && hipMemcpy(d_mx, d->in_max, (size_t)nin * sizeof(double), hipMemcpyHostToDevice) == hipSuccess)) return false;
    if (a.regress) {
        if (!(tmp.alloc(&d_y, n_rows) && hipMemcpy(d_y, a.target, (size_t)n_rows * sizeof(double), hipMemcpyHostToDevice) == hipSuccess)) return false;
        hipLaunchKernelGGL(train_normalise_target_kernel, dim3((n_rows + 255) / 256), dim3(256), 0, nullptr, d_y, a.out_min, a.out_max, (uint64_t)n_rows, D.target);
        hipLaunchKernelGGL(train_adam_reset_kernel, dim3(1), dim3(1), 0, nullptr, D.adam);
    } else if (hipMemcpy(D.label, a.label, (size_t)n_rows * sizeof(int32_t), hipMemcpyHostToDevice) != hipSuccess) return false;
    const uint64_t total = (uint64_t)n_rows * xs;
    if (a.db) hipLaunchKernelGGL(train_normalise_db_kernel, dim3((uint32_t)((total + 255) / 256)), dim3(256), 0, nullptr, a.db->d_feat, d_rows, d_mn, d_mx, (uint64_t)n_rows, nin, (int)xs, D.x);
    else hipLaunchKernelGGL(train_normalise_kernel, dim3((uint32_t)((total + 255) / 256)), dim3(256), 0, nullptr, d_feat, d_mn, d_mx, (uint64_t)n_rows, nin, (int)xs, D.x);
    return hipGetLastError() == hipSuccess && hipDeviceSynchronize() == hipSuccess;
}

wsa_status trainer_create(wsa_ctx* ctx, const CreateArgs& a, wsa_trainer** out) {
    if (!ctx || !a.d || !out) return fail(ctx, WSA_ERR_INVALID, "null argument");
    *out = nullptr;
    const std::string why = create_refusal(a);
    if (!why.empty()) return fail(ctx, WSA_ERR_INVALID, why);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const wsa_model_desc* d = a.d;
    const int nl = d->n_layers, nin = d->units[0], C = d->units[nl];
    wsa_trainer* t = new wsa_trainer();
    TrainDesc& D = t->desc;
    t->ctx = ctx; t->n_rows = a.n_rows;
    D.nl = nl; D.regress = a.regress ? 1 : 0; D.lr = (float)a.learning_rate;
    D.n_val = a.n_val; D.n_train = a.n_rows - a.n_val;
    D.batch = a.batch_size < D.n_train ? a.batch_size : D.n_train;           // a larger batch is one step over all training rows
    D.n_steps = (D.n_train + D.batch - 1) / D.batch;
    t->mcap = up16(D.batch > a.n_val ? D.batch : a.n_val);
    for (int l = 0; l <= nl; l++) { D.units[l] = d->units[l]; D.pad[l] = (d->units[l] + 15) & ~15; }
    for (int l = 0; l < nl; l++) D.act[l] = d->activation[l];
    t->in_min.assign(d->in_min, d->in_min + nin); t->in_max.assign(d->in_max, d->in_max + nin);
    if (d->labels) { t->has_labels = true; for (int c = 0; c < C; c++) t->labels.emplace_back(d->labels[c] ? d->labels[c] : ""); }
    if (!create_buffers(t, a)) {
        const std::string msg = std::string("device allocation / copy failed: ") + hipGetErrorString(hipGetLastError());
        wsa_trainer_destroy(t);
        return fail(ctx, WSA_ERR_HIP, msg);
    }
    *out = t;
    return WSA_OK;
}

}  // namespace

extern "C" {

wsa_status wsa_trainer_create(wsa_ctx* ctx, const wsa_model_desc* d, const double* feat, const int32_t* label, uint32_t n_rows,
                              uint32_t n_val, uint32_t batch_size, double learning_rate, wsa_trainer** out) {
    return trainer_create(ctx, CreateArgs{d, feat, label, nullptr, false, n_rows, n_val, batch_size, learning_rate, 0.0, 1.0}, out);
}

wsa_status wsa_regress_trainer_create(wsa_ctx* ctx, const wsa_model_desc* d, const double* feat, const double* target, uint32_t n_rows,
                                      uint32_t n_val, uint32_t batch_size, double learning_rate, double out_min, double out_max, wsa_trainer** out) {
    return trainer_create(ctx, CreateArgs{d, feat, nullptr, target, true, n_rows, n_val, batch_size, learning_rate, out_min, out_max}, out);
}

wsa_status wsa_trainer_create_db(wsa_ctx* ctx, const wsa_model_desc* d, const wsa_featdb* db, const uint32_t* rows, const int32_t* label, uint32_t n_rows,
                                 uint32_t n_val, uint32_t batch_size, double learning_rate, wsa_trainer** out) {
    if (!db) return fail(ctx, WSA_ERR_INVALID, "null feature DB");
    if (db->ctx != ctx) return fail(ctx, WSA_ERR_INVALID, "the feature DB belongs to another context");
    if (const std::string why = wsa_fd::pending_refusal(db, "wsa_trainer_create_db"); !why.empty()) return fail(ctx, WSA_ERR_INVALID, why);
    CreateArgs a{d, nullptr, label, nullptr, false, n_rows, n_val, batch_size, learning_rate, 0.0, 1.0};
    a.db = db; a.rows = rows;
    return trainer_create(ctx, a, out);
}

wsa_status wsa_regress_trainer_create_db(wsa_ctx* ctx, const wsa_model_desc* d, const wsa_featdb* db, const uint32_t* rows, const double* target, uint32_t n_rows,
                                         uint32_t n_val, uint32_t batch_size, double learning_rate, double out_min, double out_max, wsa_trainer** out) {
    if (!db) return fail(ctx, WSA_ERR_INVALID, "null feature DB");
    if (db->ctx != ctx) return fail(ctx, WSA_ERR_INVALID, "the feature DB belongs to another context");
    if (const std::string why = wsa_fd::pending_refusal(db, "wsa_regress_trainer_create_db"); !why.empty()) return fail(ctx, WSA_ERR_INVALID, why);
    CreateArgs a{d, nullptr, nullptr, target, true, n_rows, n_val, batch_size, learning_rate, out_min, out_max};
    a.db = db; a.rows = rows;
    return trainer_create(ctx, a, out);
}

void wsa_trainer_destroy(wsa_trainer* t) {
    if (!t) return;
    (void)hipSetDevice(t->ctx->device);
    if (t->group) tg_orphan(t->group);                                       // against the documented order: the group refuses from here on
    for (int i = 0; i < 2; i++) {
        if (t->ev[i]) { (void)hipEventSynchronize(t->ev[i]); (void)hipEventDestroy(t->ev[i]); }
        if (t->h_order[i]) (void)hipHostFree(t->h_order[i]);
    }
    delete t;
}

wsa_status wsa_trainer_epoch(wsa_trainer* t, const uint32_t* order, void* stream) {
    if (!t) return WSA_ERR_INVALID;
    wsa_ctx* ctx = t->ctx;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (order) {
        const std::string why = order_refusal(t, order);
        if (!why.empty()) return fail(ctx, WSA_ERR_INVALID, why);
    }
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const uint32_t* idx = t->desc.identity;
    if (order) {
        const wsa_status st = stage_order(t, order, s);
        if (st != WSA_OK) return st;
        idx = t->desc.order;
    }
    group_plan(&t, 1, [&](TrStage stage, uint32_t step, int pos) { solo_launch(t, idx, stage, step, pos, s); });
    HIP_TRY(ctx, hipGetLastError());
    return WSA_OK;
}

wsa_status wsa_trainer_stats(wsa_trainer* t, void* stream, wsa_train_stats* out) {
    if (!t) return WSA_ERR_INVALID;
    wsa_ctx* ctx = t->ctx;
    if (!out) return fail(ctx, WSA_ERR_INVALID, "null argument");
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipMemcpyAsync(out, t->desc.stats, sizeof(wsa_train_stats), hipMemcpyDeviceToHost, s));
    HIP_TRY(ctx, hipStreamSynchronize(s));
    return WSA_OK;
}

wsa_status wsa_trainer_copy_weights(wsa_trainer* t, void* stream, float* const* kernel, float* const* bias) {
    if (!t) return WSA_ERR_INVALID;
    wsa_ctx* ctx = t->ctx;
    const TrainDesc& D = t->desc;
    if (!kernel || !bias) return fail(ctx, WSA_ERR_INVALID, "null kernel / bias array");
    for (int l = 0; l < D.nl; l++) if (!kernel[l] || !bias[l]) return fail(ctx, WSA_ERR_INVALID, "null kernel / bias of layer " + std::to_string(l));
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    for (int l = 0; l < D.nl; l++) {                                         // strided: the padded columns stay behind
        const size_t n = (size_t)D.units[l + 1] * sizeof(float);
        HIP_TRY(ctx, hipMemcpy2DAsync(kernel[l], n, D.w[l], (size_t)D.pad[l + 1] * sizeof(float), n, D.units[l], hipMemcpyDeviceToHost, s));
        HIP_TRY(ctx, hipMemcpyAsync(bias[l], D.b[l], n, hipMemcpyDeviceToHost, s));
    }
    HIP_TRY(ctx, hipStreamSynchronize(s));
    return WSA_OK;
}

wsa_status wsa_trainer_model(wsa_trainer* t, void* stream, wsa_model** out) {
    if (!t) return WSA_ERR_INVALID;
    wsa_ctx* ctx = t->ctx;
    const TrainDesc& D = t->desc;
    if (!out) return fail(ctx, WSA_ERR_INVALID, "null argument");
    *out = nullptr;
    std::vector<std::vector<float>> k(D.nl), b(D.nl);
    std::vector<float*> kp(D.nl), bp(D.nl);
    for (int l = 0; l < D.nl; l++) {
        k[l].resize((size_t)D.units[l] * D.units[l + 1]); b[l].resize(D.units[l + 1]);
        kp[l] = k[l].data(); bp[l] = b[l].data();
    }
    const wsa_status st = wsa_trainer_copy_weights(t, stream, kp.data(), bp.data());
    if (st != WSA_OK) return st;
    std::vector<const char*> lab;
    for (const std::string& x : t->labels) lab.push_back(x.c_str());
    wsa_model_desc d{};
    d.n_layers = D.nl; d.units = D.units; d.activation = D.act;
    d.kernel = kp.data(); d.bias = bp.data(); d.in_min = t->in_min.data(); d.in_max = t->in_max.data();
    d.labels = t->has_labels ? lab.data() : nullptr;
    return wsa_model_create(ctx, &d, out);
}

}  // extern "C"
