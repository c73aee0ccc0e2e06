// train_stages.hpp — K7 / K7g: what the solo trainer (train.hip) and the training group (train_group.hip) share on the device and in
// building a stage's parameters: the description of one trainer, the stages' parameter structs, the functions that build them (host and
// device: the solo path calls them on the host and passes the struct by value, the grouped kernels call them on a row of the group's
// device table) and the stage bodies.  Specifications TR-1, TR-2 and TG-1, DESIGN.md "K7", "K7g".
//
// One step is a chain of kernels on the caller's stream; every dependency between stages is a kernel boundary:
//   forward  l = 0 .. L-1   A[l+1] = act_l(A[l] W_l + b_l)          one wave per 16 x 16 tile of A[l+1]; f32 MFMA partial sums, added in double
//   loss                    p, per-row loss / hit, dZ_{L-1}          one workgroup, fixed-order sums -> the step's partial
//   backward l = L-1 .. 0   dZ_{l-1} = (dZ_l W_l^T) . act'(A[l])     one wave per 16 x 16 tile (l > 0 only), BEFORE W_l changes
//                           W_l -= lr A[l]^T dZ_l, b_l -= lr 1^T dZ_l one wave per 16 x 16 tile of W_l: it owns the whole sum over the
//                                                                    batch rows (ascending, four per MFMA) and applies the update
// Every sum has one owner and one order, nothing is accumulated with atomics, so a run is reproducible bit for bit.
//
// The app's regression models (ords_<label>, specification TR-2: one output unit, tfjs meanSquaredError, tf.train.adam; ref
// src/neuralmodel.js:268-333 and nn_default_options_ords, src/neuralmodel_aux.js:127-150) run the same chain with two stages swapped:
//   loss     mean squared error   per-row squared error and dZ_{L-1} = 2 (p - t) / b . act'(p) in double; its thread 0 also advances
//                                 Adam's device-side step state (accumulated betas), so an epoch needs no host round trip
//   update   Adam                 the same tile owner and the same ascending sum, then tfjs's AdamOptimizer.applyGradients on the
//                                 owner's elements of w, m and v
// mfma_f32_16x16x4f32 as in K6: lane l holds A[row l&15][k l>>4], B[k l>>4][col l&15]; D col = l&15, row = 4 (l>>4) + i.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/wsa.h"

namespace wsa_train {

// One trainer, as its stages see it: everything of it that does not change from create to destroy.  wsa_trainer holds it on the host
// (trainer_create fills it as it allocates); a group's device table is its members' descriptions, one row each.
struct TrainDesc {
    float* x; uint32_t* order; uint32_t* identity;                          // normalised rows [n_rows][pad[0]]; the epoch's order, 0 .. n_train-1
    int32_t* label; float* target; float* adam;                             // TR-1: label; TR-2 (regress): target, Adam's step state [4]
    float *w[WSA_MODEL_MAX_LAYERS], *b[WSA_MODEL_MAX_LAYERS];
    float *mw[WSA_MODEL_MAX_LAYERS], *vw[WSA_MODEL_MAX_LAYERS], *mb[WSA_MODEL_MAX_LAYERS], *vb[WSA_MODEL_MAX_LAYERS];   // Adam's moments (regress)
    float* a[WSA_MODEL_MAX_LAYERS + 1];                                     // a[l], l >= 1: the output of layer l - 1, [mcap][pad[l]]
    float* dz[2];                                                           // [mcap][widest layer]: dZ of a layer and of the one below it
    double* part_loss; uint32_t* part_hit; wsa_train_stats* stats;          // [n_steps + 1]: the steps' partials, then the validation pass's
    int units[WSA_MODEL_MAX_LAYERS + 1], pad[WSA_MODEL_MAX_LAYERS + 1], act[WSA_MODEL_MAX_LAYERS];
    int nl, regress; uint32_t n_train, n_val, batch, n_steps; float lr;
};

constexpr int TR_THREADS = 256;                  // 4 waves, one 16 x 16 output tile each
constexpr int TR_WAVES = TR_THREADS / 64;
constexpr int TR_LOSS_THREADS = 1024;
constexpr int TR_FINISH_THREADS = 256;
constexpr uint32_t TR_VALIDATION = 0xFFFFFFFFu;  // the `step` of the pass over the validation rows

// The rows of `step` (read through idx, the trainer's order or identity buffer) or, step == TR_VALIDATION, the validation rows behind
// the training rows; `slot` is where the loss leaves the step's partial.
struct TrStep { const uint32_t* idx; uint32_t off, m, mp, slot; bool training; };

__host__ __device__ __forceinline__ TrStep tr_step(const TrainDesc& t, uint32_t step, const uint32_t* idx) {
    TrStep s;
    s.training = step != TR_VALIDATION;
    if (s.training) {
        s.idx = idx;
        s.off = step * t.batch; s.m = t.n_train - s.off < t.batch ? t.n_train - s.off : t.batch;
        s.slot = step;
    } else { s.idx = nullptr; s.off = t.n_train; s.m = t.n_val; s.slot = t.n_steps; }
    s.mp = (s.m + 15u) & ~15u;
    return s;
}

}  // namespace wsa_train

namespace {

using namespace wsa_train;

typedef float f32x4 __attribute__((ext_vector_type(4)));

// rows of a step's input: row r of the step is base[(idx ? idx[off + r] : off + r) * stride]; rows >= m read as zero
struct TrRows { const float* base; int stride; const uint32_t* idx; uint32_t off, m; };
// ---- forward: out [mp][np] = act(in [m][kp] . w [kp][np] + b), rows m .. mp-1 and columns n .. np-1 written as zero
struct TrFwd { TrRows in; const float* w; const float* b; float* out; int kp, np, n, act; uint32_t mp; };
// ---- loss: softmax (K6's formula), tfjs categoricalCrossentropy and categoricalAccuracy per row, dZ of the last layer; one workgroup:
// thread t sums rows t, t + 1024, ... in that order, then a fixed tree over the threads -> part_loss / part_hit [slot]
struct TrLoss {
    const float* z; int np, C; uint32_t m, mp;
    const int32_t* label; const uint32_t* idx; uint32_t off;
    float* dz;                                                              // NULL: evaluation only
    double* part_loss; uint32_t* part_hit; uint32_t slot;
};
// ---- loss of a regression model (TR-2): tfjs meanSquaredError over the one output unit, binaryAccuracy (what "accuracy" resolves to for
// a one-unit output: the target equals 1 if p > 0.5 else 0), dZ of the last layer THROUGH its activation (the forward pass has applied
// it: z holds p).  The same fixed-order sums as the softmax loss.  adam != NULL (a training step): thread 0 publishes this step's
// 1 - accBeta1 / 1 - accBeta2 for the update kernels behind it on the stream and advances accBeta (tfjs: sub(1, accBeta) before the
// variables, accBeta.mul(beta) after them); the state is {accBeta1, accBeta2, 1 - accBeta1, 1 - accBeta2}, all f32 as tfjs keeps them.
struct TrLossMse {
    const float* z; int np, act; uint32_t m, mp;
    const float* target; const uint32_t* idx; uint32_t off;
    float* dz;                                                              // NULL: evaluation only
    float* adam;                                                            // NULL: evaluation only
    double* part_loss; uint32_t* part_hit; uint32_t slot;
};
// ---- backward through one layer's kernel: dzp [mp][kp] = (dz [mp][np] . w^T) . act'(a [mp][kp]); columns k .. kp-1, rows m .. zero
struct TrBack { const float* dz; const float* w; const float* a; float* dzp; int kp, np, k, act; uint32_t m, mp; };
// ---- update: w [kp][np] -= lr a^T dz, b -= lr 1^T dz.  Tiles (kb, cb), kb = kp / 16 is the bias's tile (A = ones).  The wave that
// owns a tile sums over all batch rows in ascending order and writes the new weights; padded rows / columns stay zero.
struct TrUpd { TrRows a; const float* dz; float* w; float* b; int kp, np, k, n; uint32_t mp; float lr; };
// ---- update of a regression model: the same tiles, owners and order of summation; the owner then applies Adam to its own elements of
// w / m / v (mw, vw [kp][np] and mb, vb [np]: padded exactly as the weights are; padded elements are never touched and stay 0)
struct TrUpdAdam { TrUpd u; float* mw; float* vw; float* mb; float* vb; const float* adam; };
// ---- epoch end: the steps' partials in a fixed order -> the epoch's statistics (history of tfjs's BaseLogger / testLoop)
struct TrFin { const double* part_loss; const uint32_t* part_hit; uint32_t n_steps, n_train, n_val, epoch; wsa_train_stats* out; };

// ---- a stage's parameters from the trainer's description, the step's rows and the stage's position: said here once, for the host
// (solo launches) and for the device (grouped kernels)
// the input of layer l: the step's rows of x, or the output of the layer below
__host__ __device__ __forceinline__ TrRows tr_layer_input(const TrainDesc& t, const TrStep& s, int l) {
    return l == 0 ? TrRows{t.x, t.pad[0], s.idx, s.off, s.m} : TrRows{t.a[l], t.pad[l], nullptr, 0, s.m};
}

__host__ __device__ __forceinline__ TrFwd tr_forward_params(const TrainDesc& t, const TrStep& s, int l) {
    TrFwd f;
    f.in = tr_layer_input(t, s, l);
    f.w = t.w[l]; f.b = t.b[l]; f.out = t.a[l + 1];
    f.kp = t.pad[l]; f.np = t.pad[l + 1]; f.n = t.units[l + 1]; f.act = t.act[l]; f.mp = s.mp;
    return f;
}

// both losses leave dZ of the last layer in dz[0] in a training step and none in validation
__host__ __device__ __forceinline__ TrLoss tr_loss_params(const TrainDesc& t, const TrStep& s) {
    TrLoss p;
    p.z = t.a[t.nl]; p.np = t.pad[t.nl]; p.C = t.units[t.nl]; p.m = s.m; p.mp = s.mp;
    p.label = t.label; p.idx = s.idx; p.off = s.off; p.dz = s.training ? t.dz[0] : nullptr;
    p.part_loss = t.part_loss; p.part_hit = t.part_hit; p.slot = s.slot;
    return p;
}

__host__ __device__ __forceinline__ TrLossMse tr_loss_mse_params(const TrainDesc& t, const TrStep& s) {
    TrLossMse p;
    p.z = t.a[t.nl]; p.np = t.pad[t.nl]; p.act = t.act[t.nl - 1]; p.m = s.m; p.mp = s.mp;
    p.target = t.target; p.idx = s.idx; p.off = s.off; p.dz = s.training ? t.dz[0] : nullptr; p.adam = s.training ? t.adam : nullptr;
    p.part_loss = t.part_loss; p.part_hit = t.part_hit; p.slot = s.slot;
    return p;
}

// position j of the backward / update stages is layer nl - 1 - j; dZ of that layer is in dz[j & 1], dZ of the one below goes to the other
__host__ __device__ __forceinline__ TrBack tr_backward_params(const TrainDesc& t, const TrStep& s, int j) {
    const int l = t.nl - 1 - j, cur = j & 1;                                // l > 0: a trainer has no backward at its last position
    TrBack b;
    b.dz = t.dz[cur]; b.w = t.w[l]; b.a = t.a[l]; b.dzp = t.dz[cur ^ 1];
    b.kp = t.pad[l]; b.np = t.pad[l + 1]; b.k = t.units[l]; b.act = t.act[l - 1]; b.m = s.m; b.mp = s.mp;
    return b;
}

__host__ __device__ __forceinline__ TrUpd tr_update_params(const TrainDesc& t, const TrStep& s, int j) {
    const int l = t.nl - 1 - j, cur = j & 1;
    TrUpd u;
    u.a = tr_layer_input(t, s, l);
    u.dz = t.dz[cur]; u.w = t.w[l]; u.b = t.b[l];
    u.kp = t.pad[l]; u.np = t.pad[l + 1]; u.k = t.units[l]; u.n = t.units[l + 1]; u.mp = s.mp; u.lr = t.lr;
    return u;
}

// the same update with Adam's moments beside it: u is tr_update_params(t, s, j)
__host__ __device__ __forceinline__ TrUpdAdam tr_update_adam_params(const TrainDesc& t, const TrUpd& u, int j) {
    const int l = t.nl - 1 - j;
    return TrUpdAdam{u, t.mw[l], t.vw[l], t.mb[l], t.vb[l], t.adam};
}

__host__ __device__ __forceinline__ TrFin tr_finish_params(const TrainDesc& t, uint32_t epoch) {   // epoch: the one just finished
    return TrFin{t.part_loss, t.part_hit, t.n_steps, t.n_train, t.n_val, epoch, t.stats};
}

// ---- the stage bodies.  They take the workgroup's index within their launch's part for ONE trainer: blockIdx.x in the solo kernels, the
// index past the member's prefix in the grouped ones; the arithmetic and its order are the same in both.
__device__ __forceinline__ const float* tr_row(const TrRows& a, uint32_t r) {
    if (r >= a.m) return nullptr;
    const size_t g = a.idx ? a.idx[a.off + r] : a.off + r;
    return a.base + g * (size_t)a.stride;
}

__device__ __forceinline__ float tr_activate(float v, int act) {            // K6's activate
    switch (act) {
        case WSA_ACT_RELU: return v < 0.f ? 0.f : v;
        case WSA_ACT_SIGMOID: return 1.f / (1.f + expf(-v));
        case WSA_ACT_TANH: return tanhf(v);
        default: return v;
    }
}

template <typename T>
__device__ __forceinline__ T tr_derivative(T a, int act) {                  // tfjs gradients, from the layer's OUTPUT a; f32 or f64
    switch (act) {
        case WSA_ACT_RELU: return a > T(0) ? T(1) : T(0);                   // step(x); a > 0 exactly when x > 0
        case WSA_ACT_SIGMOID: return a * (T(1) - a);
        case WSA_ACT_TANH: return T(1) - a * a;
        default: return T(1);
    }
}

// the workgroup's sum of every thread's (loss, hit): a fixed halving tree over LDS [THREADS], the sums left in s_loss[0], s_hit[0]
template <int THREADS>
__device__ __forceinline__ void tr_block_sum(double* s_loss, uint32_t* s_hit, double loss, uint32_t hit) {
    const int tid = threadIdx.x;
    s_loss[tid] = loss; s_hit[tid] = hit;
    __syncthreads();
    for (int w = THREADS / 2; w > 0; w >>= 1) {
        if (tid < w) { s_loss[tid] += s_loss[tid + w]; s_hit[tid] += s_hit[tid + w]; }
        __syncthreads();
    }
}

__device__ __forceinline__ void tr_forward_body(const TrFwd& p, uint32_t block) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t cbs = p.np / 16, tile = block * TR_WAVES + wave;
    if (tile >= (p.mp / 16) * cbs) return;
    const uint32_t r0 = (tile / cbs) * 16; const int n0 = (tile % cbs) * 16;
    const float* ap = tr_row(p.in, r0 + (lane & 15));
    const float* wp = p.w + (size_t)(lane >> 4) * p.np + n0 + (lane & 15);
    // Every MFMA starts from zero and its f32 result (four products) is added to a double accumulator: a layer's output is rounded to
    // f32 once, as tfjs's CPU backend rounds it (it sums each dot product in a double); DESIGN.md "K7" has the finding that asks for it.
    double acc[4] = {0.0, 0.0, 0.0, 0.0};
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    for (int k1 = 0; k1 < p.kp; k1 += 16) {                                 // kp is a multiple of 16: four loads in flight
        float av[4], bv[4];
#pragma unroll
        for (int j = 0; j < 4; j++) { av[j] = ap ? ap[k1 + 4 * j + (lane >> 4)] : 0.f; bv[j] = wp[(size_t)(k1 + 4 * j) * p.np]; }
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const f32x4 part = __builtin_amdgcn_mfma_f32_16x16x4f32(av[j], bv[j], zero, 0, 0, 0);
#pragma unroll
            for (int i = 0; i < 4; i++) acc[i] += (double)part[i];          // K ascending, one owner: the same bits every run
        }
    }
    const int col = n0 + (lane & 15);
    const double bias = (double)p.b[col];
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const uint32_t row = r0 + (lane >> 4) * 4 + i;
        float v = (float)(acc[i] + bias);                                   // tfjs Dense: matMul + bias, then the activation
        if (p.act != WSA_ACT_SOFTMAX) v = tr_activate(v, p.act);
        if (col >= p.n || row >= p.in.m) v = 0.f;
        p.out[(size_t)row * p.np + col] = v;
    }
}

__device__ __forceinline__ void tr_loss_body(const TrLoss& p, double* s_loss, uint32_t* s_hit) {   // s_loss, s_hit: LDS [TR_LOSS_THREADS]
    const int tid = threadIdx.x;
    double loss = 0.0; uint32_t hit = 0;
    for (uint32_t r = tid; r < p.mp; r += TR_LOSS_THREADS) {
        float* d = p.dz ? p.dz + (size_t)r * p.np : nullptr;
        if (r >= p.m) {
            if (d) for (int c = 0; c < p.np; c++) d[c] = 0.f;
            continue;
        }
        const float* x = p.z + (size_t)r * p.np;
        const int t = p.label[p.idx ? p.idx[p.off + r] : p.off + r];
        // the f32 logits' softmax and loss in double: a row costs C exponentials, and the step's gradient starts without libm's f32 error
        double mx = x[0];
        for (int c = 1; c < p.C; c++) mx = fmax(mx, (double)x[c]);
        double s = 0.0;
        for (int c = 0; c < p.C; c++) s += exp((double)x[c] - mx);
        const double lse = mx + log(s);
        double sum = 0.0, pt = 0.0, best = -1.0; int arg = 0;
        for (int c = 0; c < p.C; c++) {
            const double pc = exp((double)x[c] - lse);
            sum += pc;
            if (c == t) pt = pc;
            if (pc > best) { best = pc; arg = c; }                          // first maximum on a tie
        }
        const double q = pt / sum, lo = 1e-7, hi = 1.0 - 1e-7;              // the loss renormalises, then clips
        const bool clipped = q < lo;
        loss += -log(q < lo ? lo : (q > hi ? hi : q));
        hit += arg == t ? 1u : 0u;
        if (d) {
            const double b = (double)p.m;
            for (int c = 0; c < p.np; c++) {
                float g = 0.f;
                if (c < p.C && !clipped) g = (float)((exp((double)x[c] - lse) - (c == t ? 1.0 : 0.0)) / b);   // tfjs's clip passes no gradient below its minimum
                d[c] = g;
            }
        }
    }
    tr_block_sum<TR_LOSS_THREADS>(s_loss, s_hit, loss, hit);
    if (tid == 0) { p.part_loss[p.slot] = s_loss[0]; p.part_hit[p.slot] = s_hit[0]; }
}

__device__ __forceinline__ void tr_backward_body(const TrBack& p, uint32_t block) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t kbs = p.kp / 16, tile = block * TR_WAVES + wave;
    if (tile >= (p.mp / 16) * kbs) return;
    const uint32_t r0 = (tile / kbs) * 16; const int k0 = (tile % kbs) * 16;
    const float* ap = p.dz + (size_t)(r0 + (lane & 15)) * p.np + (lane >> 4);
    const float* wp = p.w + (size_t)(k0 + (lane & 15)) * p.np + (lane >> 4);      // B[n][k] = w[k][n]
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    for (int n1 = 0; n1 < p.np; n1 += 16) {
        float av[4], bv[4];
#pragma unroll
        for (int j = 0; j < 4; j++) { av[j] = ap[n1 + 4 * j]; bv[j] = wp[n1 + 4 * j]; }
#pragma unroll
        for (int j = 0; j < 4; j++) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(av[j], bv[j], acc, 0, 0, 0);
    }
    const int col = k0 + (lane & 15);
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const uint32_t row = r0 + (lane >> 4) * 4 + i;
        const size_t at = (size_t)row * p.kp + col;
        float v = acc[i] * tr_derivative(p.a[at], p.act);
        if (col >= p.k || row >= p.m) v = 0.f;
        p.dzp[at] = v;
    }
}

// the gradient tile a wave owns: sum over the batch rows of a[r][k0 + ..] dz[r][n0 + ..] (bias: of dz alone), rows ascending, four per MFMA
__device__ __forceinline__ f32x4 tr_gradient_tile(const TrUpd& p, int lane, int k0, int n0, bool bias) {
    const float* dp = p.dz + (size_t)(lane >> 4) * p.np + n0 + (lane & 15);
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    for (uint32_t r1 = 0; r1 < p.mp; r1 += 16) {                            // mp is a multiple of 16; dz rows m .. mp-1 are zero
        float av[4], bv[4];
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const uint32_t r = r1 + 4 * j + (lane >> 4);
            if (bias) av[j] = 1.f;
            else { const float* ar = tr_row(p.a, r); av[j] = ar ? ar[k0 + (lane & 15)] : 0.f; }
            bv[j] = dp[(size_t)(r1 + 4 * j) * p.np];
        }
#pragma unroll
        for (int j = 0; j < 4; j++) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(av[j], bv[j], acc, 0, 0, 0);
    }
    return acc;
}

constexpr float ADAM_BETA1 = 0.9f, ADAM_BETA2 = 0.999f;                     // tf.train.adam's defaults as f32 scalars
constexpr float ADAM_ONE_M_BETA1 = (float)(1.0 - 0.9), ADAM_ONE_M_BETA2 = (float)(1.0 - 0.999);   // `1 - this.beta`: a double, then the f32 scalar
constexpr float ADAM_EPSILON = 1e-7f;                                       // the CPU backend's epsilon()

// ---- tfjs 1.7.2 AdamOptimizer.applyGradients on one element, operation for operation; every intermediate is rounded to f32 once, as
// the CPU backend's Float32Array stores round it.  Its divisions and its square root are JavaScript doubles stored to f32: written
// that way here, so their rounding does not hang on how the compiler expands an f32 division or square root.  No contraction: JavaScript
// has no fused multiply-add.  A gradient of exactly 0 with m = v = 0 gives 0 / (0 + epsilon) . (-lr) + w = w.
__device__ __forceinline__ float adam_step(float w, float g, float* m, float* v, float c1, float c2, float neg_lr) {
#pragma clang fp contract(off)
    const float m0 = *m * ADAM_BETA1, m1 = g * ADAM_ONE_M_BETA1, mn = m0 + m1;
    const float g2 = g * g;
    const float v0 = *v * ADAM_BETA2, v1 = g2 * ADAM_ONE_M_BETA2, vn = v0 + v1;
    *m = mn; *v = vn;
    const float mh = (float)((double)mn / (double)c1);
    const float vh = (float)((double)vn / (double)c2);
    const float den = (float)sqrt((double)vh) + ADAM_EPSILON;
    const float q = (float)((double)mh / (double)den);
    const float step = q * neg_lr;
    return step + w;
}

// ---- what the owner of a gradient element does with it: the new value of w (an element `at` of the kernel, or, bias, of the bias)
struct TrSgd {                                                              // tf.train.sgd: value + (-lr) gradient, in f32
    typedef TrUpd Params;
    float lr;
    __device__ __forceinline__ static const TrUpd& tiles(const TrUpd& p) { return p; }
    __device__ __forceinline__ explicit TrSgd(const TrUpd& p) : lr(p.lr) {}
    __device__ __forceinline__ float operator()(float w, float g, size_t, bool) const { return w - lr * g; }
};

struct TrAdam {                                                             // adam_step on the element and its two moments
    typedef TrUpdAdam Params;
    float *mw, *vw, *mb, *vb; float c1, c2, neg_lr;
    __device__ __forceinline__ static const TrUpd& tiles(const TrUpdAdam& q) { return q.u; }
    __device__ __forceinline__ explicit TrAdam(const TrUpdAdam& q) : mw(q.mw), vw(q.vw), mb(q.mb), vb(q.vb), c1(q.adam[2]), c2(q.adam[3]), neg_lr(-q.u.lr) {}
    __device__ __forceinline__ float operator()(float w, float g, size_t at, bool bias) const {
        return adam_step(w, g, (bias ? mb : mw) + at, (bias ? vb : vw) + at, c1, c2, neg_lr);
    }
};

template <typename Rule>
__device__ __forceinline__ void tr_update_body(const typename Rule::Params& q, uint32_t block) {
    const TrUpd& p = Rule::tiles(q);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t cbs = p.np / 16, kbs = p.kp / 16, tile = block * TR_WAVES + wave;
    if (tile >= (kbs + 1) * cbs) return;
    const uint32_t kb = tile / cbs; const int n0 = (tile % cbs) * 16, k0 = kb * 16;
    const bool bias = kb == kbs;
    const f32x4 acc = tr_gradient_tile(p, lane, k0, n0, bias);
    const int col = n0 + (lane & 15);
    if (col >= p.n) return;
    const Rule rule(q);
    if (bias) {
        if ((lane >> 4) == 0) p.b[col] = rule(p.b[col], acc[0], col, true);     // every row of the tile holds the column sums
        return;
    }
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const int row = k0 + (lane >> 4) * 4 + i;
        if (row >= p.k) continue;
        const size_t at = (size_t)row * p.np + col;
        p.w[at] = rule(p.w[at], acc[i], at, false);
    }
}

__device__ __forceinline__ void tr_loss_mse_body(const TrLossMse& p, double* s_loss, uint32_t* s_hit) {   // s_loss, s_hit: LDS [TR_LOSS_THREADS]
    const int tid = threadIdx.x;
    double loss = 0.0; uint32_t hit = 0;
    for (uint32_t r = tid; r < p.mp; r += TR_LOSS_THREADS) {
        float* d = p.dz ? p.dz + (size_t)r * p.np : nullptr;
        float g = 0.f;
        if (r < p.m) {
            const float pf = p.z[(size_t)r * p.np];
            const float tf = p.target[p.idx ? p.idx[p.off + r] : p.off + r];
            const double e = (double)pf - (double)tf;
            loss += e * e;
            hit += tf == (pf > 0.5f ? 1.f : 0.f) ? 1u : 0u;
            g = (float)(2.0 * e / (double)p.m * tr_derivative((double)pf, p.act));   // the short last batch divides by its own size
        }
        if (d) {
            d[0] = g;
            for (int c = 1; c < p.np; c++) d[c] = 0.f;
        }
    }
    tr_block_sum<TR_LOSS_THREADS>(s_loss, s_hit, loss, hit);
    if (tid == 0) {
        p.part_loss[p.slot] = s_loss[0]; p.part_hit[p.slot] = s_hit[0];
        if (p.adam) {
            const float a1 = p.adam[0], a2 = p.adam[1];
            p.adam[2] = 1.f - a1; p.adam[3] = 1.f - a2;
            p.adam[0] = a1 * ADAM_BETA1; p.adam[1] = a2 * ADAM_BETA2;
        }
    }
}

__device__ __forceinline__ void tr_finish_body(const TrFin& p, double* s_loss, uint32_t* s_hit) {   // s_loss, s_hit: LDS [TR_FINISH_THREADS]
    const int tid = threadIdx.x;
    double loss = 0.0; uint32_t hit = 0;
    for (uint32_t i = tid; i < p.n_steps; i += TR_FINISH_THREADS) { loss += p.part_loss[i]; hit += p.part_hit[i]; }
    tr_block_sum<TR_FINISH_THREADS>(s_loss, s_hit, loss, hit);
    if (tid == 0) {
        wsa_train_stats st;
        st.epochs_done = p.epoch;
        st.loss = s_loss[0] / (double)p.n_train; st.acc = (double)s_hit[0] / (double)p.n_train;
        st.val_loss = p.n_val ? p.part_loss[p.n_steps] / (double)p.n_val : 0.0;
        st.val_acc = p.n_val ? (double)p.part_hit[p.n_steps] / (double)p.n_val : 0.0;
        *p.out = st;
    }
}

}  // namespace
