// train.hip — K7: minibatch SGD for the app's Dense classifiers (specification TR-1), and its part of the C ABI
// (include/wsa.h "Training").
//
// Stands in for the reference APPLICATION's training path: src/neuralmodel.js:163-403 (train_nn) -> ml5 0.6.0
// neuralNetwork.train: tfjs 1.7.2 model.fit with categoricalCrossentropy, tf.train.sgd(learningRate), metrics ["accuracy"].
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
// src/neuralmodel.js:268-333 and nn_default_options_ords, src/neuralmodel_aux.js:127-150) run the same chain with two kernels swapped:
//   loss     train_loss_mse_kernel     per-row squared error and dZ_{L-1} = 2 (p - t) / b . act'(p) in double; its thread 0 also advances
//                                      Adam's device-side step state (accumulated betas), so an epoch needs no host round trip
//   update   train_update_adam_kernel  the same tile owner and the same ascending sum, then tfjs's AdamOptimizer.applyGradients on the
//                                      owner's elements of w, m and v
// mfma_f32_16x16x4f32 as in K6: lane l holds A[row l&15][k l>>4], B[k l>>4][col l&15]; D col = l&15, row = 4 (l>>4) + i.
#include <cmath>
#include <cstring>
#include <string>
#include <vector>
#include "host_plan.hpp"

using wsa_api::fail;

namespace {

constexpr int TR_THREADS = 256;                  // 4 waves, one 16 x 16 output tile each
constexpr int TR_WAVES = TR_THREADS / 64;
constexpr int TR_LOSS_THREADS = 1024;

typedef float f32x4 __attribute__((ext_vector_type(4)));

// rows of a step's input: row r of the step is base[(idx ? idx[off + r] : off + r) * stride]; rows >= m read as zero
struct TrRows { const float* base; int stride; const uint32_t* idx; uint32_t off, m; };

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

__device__ __forceinline__ float tr_derivative(float a, int act) {          // tfjs gradients, from the layer's OUTPUT a
    switch (act) {
        case WSA_ACT_RELU: return a > 0.f ? 1.f : 0.f;                      // step(x); a > 0 exactly when x > 0
        case WSA_ACT_SIGMOID: return a * (1.f - a);
        case WSA_ACT_TANH: return 1.f - a * a;
        default: return 1.f;
    }
}

// ---- forward: out [mp][np] = act(in [m][kp] . w [kp][np] + b), rows m .. mp-1 and columns n .. np-1 written as zero
struct TrFwd { TrRows in; const float* w; const float* b; float* out; int kp, np, n, act; uint32_t mp; };

// (the stage bodies take the workgroup's index within their launch's part for ONE trainer: blockIdx.x in the solo kernels, the index
// past the member's prefix in the grouped ones, K7g below; the arithmetic and its order are the same in both)
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

__global__ void __launch_bounds__(TR_THREADS) train_forward_kernel(TrFwd p) { tr_forward_body(p, blockIdx.x); }

// ---- loss: softmax (K6's formula), tfjs categoricalCrossentropy and categoricalAccuracy per row, dZ of the last layer; one workgroup:
// thread t sums rows t, t + 1024, ... in that order, then a fixed tree over the threads -> part_loss / part_hit [slot]
struct TrLoss {
    const float* z; int np, C; uint32_t m, mp;
    const int32_t* label; const uint32_t* idx; uint32_t off;
    float* dz;                                                              // NULL: evaluation only
    double* part_loss; uint32_t* part_hit; uint32_t slot;
};

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
    s_loss[tid] = loss; s_hit[tid] = hit;
    __syncthreads();
    for (int w = TR_LOSS_THREADS / 2; w > 0; w >>= 1) {
        if (tid < w) { s_loss[tid] += s_loss[tid + w]; s_hit[tid] += s_hit[tid + w]; }
        __syncthreads();
    }
    if (tid == 0) { p.part_loss[p.slot] = s_loss[0]; p.part_hit[p.slot] = s_hit[0]; }
}

__global__ void __launch_bounds__(TR_LOSS_THREADS) train_loss_kernel(TrLoss p) {
    __shared__ double s_loss[TR_LOSS_THREADS];
    __shared__ uint32_t s_hit[TR_LOSS_THREADS];
    tr_loss_body(p, s_loss, s_hit);
}

// ---- backward through one layer's kernel: dzp [mp][kp] = (dz [mp][np] . w^T) . act'(a [mp][kp]); columns k .. kp-1, rows m .. zero
struct TrBack { const float* dz; const float* w; const float* a; float* dzp; int kp, np, k, act; uint32_t m, mp; };

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

__global__ void __launch_bounds__(TR_THREADS) train_backward_kernel(TrBack p) { tr_backward_body(p, blockIdx.x); }

// ---- update: w [kp][np] -= lr a^T dz, b -= lr 1^T dz.  Tiles (kb, cb), kb = kp / 16 is the bias's tile (A = ones).  The wave that
// owns a tile sums over all batch rows in ascending order and writes the new weights; padded rows / columns stay zero.
struct TrUpd { TrRows a; const float* dz; float* w; float* b; int kp, np, k, n; uint32_t mp; float lr; };

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

__device__ __forceinline__ void tr_update_body(const TrUpd& p, uint32_t block) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t cbs = p.np / 16, kbs = p.kp / 16, tile = block * TR_WAVES + wave;
    if (tile >= (kbs + 1) * cbs) return;
    const uint32_t kb = tile / cbs; const int n0 = (tile % cbs) * 16, k0 = kb * 16;
    const bool bias = kb == kbs;
    const f32x4 acc = tr_gradient_tile(p, lane, k0, n0, bias);
    const int col = n0 + (lane & 15);
    if (col >= p.n) return;
    if (bias) {
        if ((lane >> 4) == 0) p.b[col] = p.b[col] - p.lr * acc[0];          // every row of the tile holds the column sums
        return;
    }
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const int row = k0 + (lane >> 4) * 4 + i;
        if (row >= p.k) continue;
        const size_t at = (size_t)row * p.np + col;
        p.w[at] = p.w[at] - p.lr * acc[i];                                  // tf.train.sgd: value + (-lr) gradient, in f32
    }
}

__global__ void __launch_bounds__(TR_THREADS) train_update_kernel(TrUpd p) { tr_update_body(p, blockIdx.x); }

// ---- loss of a regression model (TR-2): tfjs meanSquaredError over the one output unit, binaryAccuracy (what "accuracy" resolves to for
// a one-unit output: the target equals 1 if p > 0.5 else 0), dZ of the last layer THROUGH its activation (the forward pass has applied
// it: z holds p).  The same fixed-order sums as train_loss_kernel.  adam != NULL (a training step): thread 0 publishes this step's
// 1 - accBeta1 / 1 - accBeta2 for the update kernels behind it on the stream and advances accBeta (tfjs: sub(1, accBeta) before the
// variables, accBeta.mul(beta) after them); the state is {accBeta1, accBeta2, 1 - accBeta1, 1 - accBeta2}, all f32 as tfjs keeps them.
constexpr float ADAM_BETA1 = 0.9f, ADAM_BETA2 = 0.999f;                     // tf.train.adam's defaults as f32 scalars
constexpr float ADAM_ONE_M_BETA1 = (float)(1.0 - 0.9), ADAM_ONE_M_BETA2 = (float)(1.0 - 0.999);   // `1 - this.beta`: a double, then the f32 scalar
constexpr float ADAM_EPSILON = 1e-7f;                                       // the CPU backend's epsilon()

struct TrLossMse {
    const float* z; int np, act; uint32_t m, mp;
    const float* target; const uint32_t* idx; uint32_t off;
    float* dz;                                                              // NULL: evaluation only
    float* adam;                                                            // NULL: evaluation only
    double* part_loss; uint32_t* part_hit; uint32_t slot;
};

__device__ __forceinline__ double tr_derivative_f64(double a, int act) {    // tr_derivative in double
    switch (act) {
        case WSA_ACT_RELU: return a > 0.0 ? 1.0 : 0.0;
        case WSA_ACT_SIGMOID: return a * (1.0 - a);
        case WSA_ACT_TANH: return 1.0 - a * a;
        default: return 1.0;
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
            g = (float)(2.0 * e / (double)p.m * tr_derivative_f64((double)pf, p.act));   // the short last batch divides by its own size
        }
        if (d) {
            d[0] = g;
            for (int c = 1; c < p.np; c++) d[c] = 0.f;
        }
    }
    s_loss[tid] = loss; s_hit[tid] = hit;
    __syncthreads();
    for (int w = TR_LOSS_THREADS / 2; w > 0; w >>= 1) {
        if (tid < w) { s_loss[tid] += s_loss[tid + w]; s_hit[tid] += s_hit[tid + w]; }
        __syncthreads();
    }
    if (tid == 0) {
        p.part_loss[p.slot] = s_loss[0]; p.part_hit[p.slot] = s_hit[0];
        if (p.adam) {
            const float a1 = p.adam[0], a2 = p.adam[1];
            p.adam[2] = 1.f - a1; p.adam[3] = 1.f - a2;
            p.adam[0] = a1 * ADAM_BETA1; p.adam[1] = a2 * ADAM_BETA2;
        }
    }
}

__global__ void __launch_bounds__(TR_LOSS_THREADS) train_loss_mse_kernel(TrLossMse p) {
    __shared__ double s_loss[TR_LOSS_THREADS];
    __shared__ uint32_t s_hit[TR_LOSS_THREADS];
    tr_loss_mse_body(p, s_loss, s_hit);
}

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

// ---- update of a regression model: train_update_kernel's tiles, owners and order of summation; the owner then applies Adam to its own
// elements of w / m / v (mw, vw [kp][np] and mb, vb [np]: padded exactly as the weights are; padded elements are never touched and stay 0)
struct TrUpdAdam { TrUpd u; float* mw; float* vw; float* mb; float* vb; const float* adam; };

__device__ __forceinline__ void tr_update_adam_body(const TrUpdAdam& q, uint32_t block) {
    const TrUpd& p = q.u;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t cbs = p.np / 16, kbs = p.kp / 16, tile = block * TR_WAVES + wave;
    if (tile >= (kbs + 1) * cbs) return;
    const uint32_t kb = tile / cbs; const int n0 = (tile % cbs) * 16, k0 = kb * 16;
    const bool bias = kb == kbs;
    const f32x4 acc = tr_gradient_tile(p, lane, k0, n0, bias);
    const int col = n0 + (lane & 15);
    if (col >= p.n) return;
    const float c1 = q.adam[2], c2 = q.adam[3], neg_lr = -p.lr;
    if (bias) {
        if ((lane >> 4) == 0) p.b[col] = adam_step(p.b[col], acc[0], q.mb + col, q.vb + col, c1, c2, neg_lr);   // every row of the tile holds the column sums
        return;
    }
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const int row = k0 + (lane >> 4) * 4 + i;
        if (row >= p.k) continue;
        const size_t at = (size_t)row * p.np + col;
        p.w[at] = adam_step(p.w[at], acc[i], q.mw + at, q.vw + at, c1, c2, neg_lr);
    }
}

__global__ void __launch_bounds__(TR_THREADS) train_update_adam_kernel(TrUpdAdam q) { tr_update_adam_body(q, blockIdx.x); }

__global__ void train_adam_reset_kernel(float* adam) {                      // accBeta = beta: no step taken yet
    if (threadIdx.x == 0 && blockIdx.x == 0) { adam[0] = ADAM_BETA1; adam[1] = ADAM_BETA2; adam[2] = 1.f - ADAM_BETA1; adam[3] = 1.f - ADAM_BETA2; }
}

// ---- create: a regression model's targets, (y - min) / (max - min) in double, rounded to f32 (ml5 normalizeData on the output `y`)
__global__ void __launch_bounds__(256) train_normalise_target_kernel(const double* y, double mn, double mx, uint64_t n_rows, float* t) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n_rows) t[i] = (float)((y[i] - mn) / (mx - mn));
}

// ---- epoch end: the steps' partials in a fixed order -> the epoch's statistics (history of tfjs's BaseLogger / testLoop)
struct TrFin { const double* part_loss; const uint32_t* part_hit; uint32_t n_steps, n_train, n_val, epoch; wsa_train_stats* out; };

__device__ __forceinline__ void tr_finish_body(const TrFin& p, double* s_loss, uint32_t* s_hit) {   // s_loss, s_hit: LDS [256]
    const int tid = threadIdx.x;
    double loss = 0.0; uint32_t hit = 0;
    for (uint32_t i = tid; i < p.n_steps; i += 256) { loss += p.part_loss[i]; hit += p.part_hit[i]; }
    s_loss[tid] = loss; s_hit[tid] = hit;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if (tid < w) { s_loss[tid] += s_loss[tid + w]; s_hit[tid] += s_hit[tid + w]; }
        __syncthreads();
    }
    if (tid == 0) {
        wsa_train_stats st;
        st.epochs_done = p.epoch;
        st.loss = s_loss[0] / (double)p.n_train; st.acc = (double)s_hit[0] / (double)p.n_train;
        st.val_loss = p.n_val ? p.part_loss[p.n_steps] / (double)p.n_val : 0.0;
        st.val_acc = p.n_val ? (double)p.part_hit[p.n_steps] / (double)p.n_val : 0.0;
        *p.out = st;
    }
}

__global__ void __launch_bounds__(256) train_finish_kernel(TrFin p) {
    __shared__ double s_loss[256];
    __shared__ uint32_t s_hit[256];
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

// ---- K7g: the same stages for a GROUP of trainers stepped in lock step (specification TG-1; wsa_train_group_* below).  One
// launch covers one stage of every member that has that stage in this step.  Whole workgroups belong to one member: member i owns
// workgroups prefix[i] .. prefix[i + 1] - 1 (none when it has dropped out of the epoch or has no layer at this position), its
// workgroup's index within its part is blockIdx.x - prefix[i], and from there on the solo kernel's body runs on parameters built from
// the member's row of the descriptor table (device memory, written once at wsa_train_group_create) and the step's offset and size,
// computed here from (step, n_train, batch).  Members share no buffer, no sum crosses a workgroup: a member's bits are its solo run's.
// The loss and the update each have ONE grouped kernel that takes the member's kind (softmax + SGD, or mean squared error + Adam)
// from its descriptor, so a step of a mixed group still costs 3 . max nl launches.
constexpr int TG_MAX = WSA_TRAIN_GROUP_MAX;
constexpr uint32_t TG_VALIDATION = 0xFFFFFFFFu;                             // TgLaunch::step of the pass over the validation rows

struct TgMember {                                                           // what enqueue_step reads of a wsa_trainer
    const float* x; const uint32_t* order; const uint32_t* identity;
    const int32_t* label; const float* target; float* adam;
    float *w[WSA_MODEL_MAX_LAYERS], *b[WSA_MODEL_MAX_LAYERS];
    float *mw[WSA_MODEL_MAX_LAYERS], *vw[WSA_MODEL_MAX_LAYERS], *mb[WSA_MODEL_MAX_LAYERS], *vb[WSA_MODEL_MAX_LAYERS];
    float* a[WSA_MODEL_MAX_LAYERS + 1]; float* dz[2];
    double* part_loss; uint32_t* part_hit; wsa_train_stats* stats;
    int units[WSA_MODEL_MAX_LAYERS + 1], pad[WSA_MODEL_MAX_LAYERS + 1], act[WSA_MODEL_MAX_LAYERS];
    int nl, regress; uint32_t n_train, n_val, batch, n_steps; float lr;
};

// by value, 37 words: the workgroup-count prefix over the members, the step (or TG_VALIDATION), bit i of order_mask set when member i
// reads its rows through its order buffer in this epoch (clear: the identity), and the layer position of the launch
struct TgLaunch { uint32_t prefix[TG_MAX + 1]; uint32_t n, step, order_mask; int pos; };

__device__ __forceinline__ uint32_t tg_member_of(const TgLaunch& g, uint32_t block) {    // uniform over the workgroup
    uint32_t i = 0;
    while (i + 1 < g.n && block >= g.prefix[i + 1]) i++;
    return i;
}

struct TgStep { const uint32_t* idx; uint32_t off, m, mp; bool training; };

__device__ __forceinline__ TgStep tg_step(const TgMember& t, const TgLaunch& g, uint32_t i) {
    TgStep s;
    s.training = g.step != TG_VALIDATION;
    if (s.training) {
        s.idx = (g.order_mask >> i) & 1u ? t.order : t.identity;
        s.off = g.step * t.batch; s.m = t.n_train - s.off < t.batch ? t.n_train - s.off : t.batch;
    } else { s.idx = nullptr; s.off = t.n_train; s.m = t.n_val; }
    s.mp = (s.m + 15u) & ~15u;
    return s;
}

__device__ __forceinline__ TrRows tg_layer_input(const TgMember& t, const TgStep& s, int l) {
    return l == 0 ? TrRows{t.x, t.pad[0], s.idx, s.off, s.m} : TrRows{t.a[l], t.pad[l], nullptr, 0, s.m};
}

__global__ void __launch_bounds__(TR_THREADS) train_group_forward_kernel(const TgMember* tab, TgLaunch g) {   // g.pos: the layer
    const uint32_t i = tg_member_of(g, blockIdx.x);
    const TgMember& t = tab[i];
    const TgStep s = tg_step(t, g, i);
    const int l = g.pos;
    TrFwd f;
    f.in = tg_layer_input(t, s, l);
    f.w = t.w[l]; f.b = t.b[l]; f.out = t.a[l + 1];
    f.kp = t.pad[l]; f.np = t.pad[l + 1]; f.n = t.units[l + 1]; f.act = t.act[l]; f.mp = s.mp;
    tr_forward_body(f, blockIdx.x - g.prefix[i]);
}

__global__ void __launch_bounds__(TR_LOSS_THREADS) train_group_loss_kernel(const TgMember* tab, TgLaunch g) {   // one workgroup per member
    __shared__ double s_loss[TR_LOSS_THREADS];
    __shared__ uint32_t s_hit[TR_LOSS_THREADS];
    const uint32_t i = tg_member_of(g, blockIdx.x);
    const TgMember& t = tab[i];
    const TgStep s = tg_step(t, g, i);
    float* dz = s.training ? t.dz[0] : nullptr;
    const uint32_t slot = s.training ? g.step : t.n_steps;
    if (t.regress) {
        TrLossMse p;
        p.z = t.a[t.nl]; p.np = t.pad[t.nl]; p.act = t.act[t.nl - 1]; p.m = s.m; p.mp = s.mp;
        p.target = t.target; p.idx = s.idx; p.off = s.off; p.dz = dz; p.adam = s.training ? t.adam : nullptr;
        p.part_loss = t.part_loss; p.part_hit = t.part_hit; p.slot = slot;
        tr_loss_mse_body(p, s_loss, s_hit);
    } else {
        TrLoss p;
        p.z = t.a[t.nl]; p.np = t.pad[t.nl]; p.C = t.units[t.nl]; p.m = s.m; p.mp = s.mp;
        p.label = t.label; p.idx = s.idx; p.off = s.off; p.dz = dz;
        p.part_loss = t.part_loss; p.part_hit = t.part_hit; p.slot = slot;
        tr_loss_body(p, s_loss, s_hit);
    }
}

// pos j of the backward / update launches is layer nl - 1 - j of a member; dZ of that layer is in dz[j & 1], as enqueue_step's `cur`
__global__ void __launch_bounds__(TR_THREADS) train_group_backward_kernel(const TgMember* tab, TgLaunch g) {
    const uint32_t i = tg_member_of(g, blockIdx.x);
    const TgMember& t = tab[i];
    const TgStep s = tg_step(t, g, i);
    const int l = t.nl - 1 - g.pos, cur = g.pos & 1;                        // l > 0: the host gives a member with l <= 0 no workgroup
    TrBack b;
    b.dz = t.dz[cur]; b.w = t.w[l]; b.a = t.a[l]; b.dzp = t.dz[cur ^ 1];
    b.kp = t.pad[l]; b.np = t.pad[l + 1]; b.k = t.units[l]; b.act = t.act[l - 1]; b.m = s.m; b.mp = s.mp;
    tr_backward_body(b, blockIdx.x - g.prefix[i]);
}

__global__ void __launch_bounds__(TR_THREADS) train_group_update_kernel(const TgMember* tab, TgLaunch g) {
    const uint32_t i = tg_member_of(g, blockIdx.x);
    const TgMember& t = tab[i];
    const TgStep s = tg_step(t, g, i);
    const int l = t.nl - 1 - g.pos, cur = g.pos & 1;
    TrUpdAdam q;
    TrUpd& u = q.u;
    u.a = tg_layer_input(t, s, l);
    u.dz = t.dz[cur]; u.w = t.w[l]; u.b = t.b[l];
    u.kp = t.pad[l]; u.np = t.pad[l + 1]; u.k = t.units[l]; u.n = t.units[l + 1]; u.mp = s.mp; u.lr = t.lr;
    if (t.regress) {
        q.mw = t.mw[l]; q.vw = t.vw[l]; q.mb = t.mb[l]; q.vb = t.vb[l]; q.adam = t.adam;
        tr_update_adam_body(q, blockIdx.x - g.prefix[i]);
    } else {
        tr_update_body(u, blockIdx.x - g.prefix[i]);
    }
}

struct TgFinish { uint32_t epoch[TG_MAX]; };                                // by value: the epoch each member has just finished

__global__ void __launch_bounds__(256) train_group_finish_kernel(const TgMember* tab, TgFinish g) {   // workgroup i: member i
    __shared__ double s_loss[256];
    __shared__ uint32_t s_hit[256];
    const TgMember& t = tab[blockIdx.x];
    const TrFin f{t.part_loss, t.part_hit, t.n_steps, t.n_train, t.n_val, g.epoch[blockIdx.x], t.stats};
    tr_finish_body(f, s_loss, s_hit);
}

}  // namespace

struct wsa_trainer {
    wsa_ctx* ctx = nullptr;
    wsa_train_group* group = nullptr;                          // the living group that has adopted this trainer, if any
    int nl = 0;
    int units[WSA_MODEL_MAX_LAYERS + 1] = {}, pad[WSA_MODEL_MAX_LAYERS + 1] = {}, act[WSA_MODEL_MAX_LAYERS] = {};
    uint32_t n_rows = 0, n_train = 0, n_val = 0, batch = 0, n_steps = 0, mcap = 0, epoch = 0;
    float lr = 0.f;
    float* d_x = nullptr; int32_t* d_label = nullptr;
    bool regress = false;                                      // TR-2: d_target instead of d_label, Adam's moments beside the weights
    float* d_target = nullptr; float* d_adam = nullptr;
    float *d_mw[WSA_MODEL_MAX_LAYERS] = {}, *d_vw[WSA_MODEL_MAX_LAYERS] = {}, *d_mb[WSA_MODEL_MAX_LAYERS] = {}, *d_vb[WSA_MODEL_MAX_LAYERS] = {};
    float *d_w[WSA_MODEL_MAX_LAYERS] = {}, *d_b[WSA_MODEL_MAX_LAYERS] = {};
    float* d_a[WSA_MODEL_MAX_LAYERS + 1] = {};                 // d_a[l], l >= 1: the output of layer l - 1, [mcap][pad[l]]
    float* d_dz[2] = {};                                       // [mcap][widest layer]: dZ of a layer and of the one below it
    uint32_t *d_order = nullptr, *d_identity = nullptr;
    uint32_t* h_order[2] = {}; hipEvent_t ev[2] = {};          // pinned staging of the order, two epochs deep
    double* d_part_loss = nullptr; uint32_t* d_part_hit = nullptr;
    wsa_train_stats* d_stats = nullptr;
    std::vector<double> in_min, in_max;
    std::vector<std::string> labels; bool has_labels = false;
    wsa::DevArena mem;
};

namespace {

inline uint32_t up16(uint32_t v) { return (v + 15u) & ~15u; }
inline uint32_t blocks_for(uint64_t tiles) { return (uint32_t)((tiles + TR_WAVES - 1) / TR_WAVES); }

// the forward pass over m rows (a step's, through `idx`, or the validation rows); leaves the logits in d_a[nl]
void enqueue_forward(wsa_trainer* t, const uint32_t* idx, uint32_t off, uint32_t m, hipStream_t s) {
    const uint32_t mp = up16(m);
    for (int l = 0; l < t->nl; l++) {
        TrFwd f{};
        f.in = l == 0 ? TrRows{t->d_x, t->pad[0], idx, off, m} : TrRows{t->d_a[l], t->pad[l], nullptr, 0, m};
        f.w = t->d_w[l]; f.b = t->d_b[l]; f.out = t->d_a[l + 1];
        f.kp = t->pad[l]; f.np = t->pad[l + 1]; f.n = t->units[l + 1]; f.act = t->act[l]; f.mp = mp;
        hipLaunchKernelGGL(train_forward_kernel, dim3(blocks_for((uint64_t)(mp / 16) * (f.np / 16))), dim3(TR_THREADS), 0, s, f);
    }
}

void enqueue_loss(wsa_trainer* t, const uint32_t* idx, uint32_t off, uint32_t m, float* dz, uint32_t slot, hipStream_t s) {
    if (t->regress) {
        TrLossMse p{};
        p.z = t->d_a[t->nl]; p.np = t->pad[t->nl]; p.act = t->act[t->nl - 1]; p.m = m; p.mp = up16(m);
        p.target = t->d_target; p.idx = idx; p.off = off; p.dz = dz; p.adam = dz ? t->d_adam : nullptr;
        p.part_loss = t->d_part_loss; p.part_hit = t->d_part_hit; p.slot = slot;
        hipLaunchKernelGGL(train_loss_mse_kernel, dim3(1), dim3(TR_LOSS_THREADS), 0, s, p);
        return;
    }
    TrLoss p{};
    p.z = t->d_a[t->nl]; p.np = t->pad[t->nl]; p.C = t->units[t->nl]; p.m = m; p.mp = up16(m);
    p.label = t->d_label; p.idx = idx; p.off = off; p.dz = dz;
    p.part_loss = t->d_part_loss; p.part_hit = t->d_part_hit; p.slot = slot;
    hipLaunchKernelGGL(train_loss_kernel, dim3(1), dim3(TR_LOSS_THREADS), 0, s, p);
}

void enqueue_step(wsa_trainer* t, const uint32_t* idx, uint32_t step, hipStream_t s) {
    const uint32_t off = step * t->batch, m = t->n_train - off < t->batch ? t->n_train - off : t->batch, mp = up16(m);
    enqueue_forward(t, idx, off, m, s);
    int cur = 0;
    enqueue_loss(t, idx, off, m, t->d_dz[cur], step, s);
    for (int l = t->nl - 1; l >= 0; l--) {
        if (l > 0) {                                                       // reads W_l: enqueued before W_l's update
            TrBack b{};
            b.dz = t->d_dz[cur]; b.w = t->d_w[l]; b.a = t->d_a[l]; b.dzp = t->d_dz[cur ^ 1];
            b.kp = t->pad[l]; b.np = t->pad[l + 1]; b.k = t->units[l]; b.act = t->act[l - 1]; b.m = m; b.mp = mp;
            hipLaunchKernelGGL(train_backward_kernel, dim3(blocks_for((uint64_t)(mp / 16) * (b.kp / 16))), dim3(TR_THREADS), 0, s, b);
        }
        TrUpd u{};
        u.a = l == 0 ? TrRows{t->d_x, t->pad[0], idx, off, m} : TrRows{t->d_a[l], t->pad[l], nullptr, 0, m};
        u.dz = t->d_dz[cur]; u.w = t->d_w[l]; u.b = t->d_b[l];
        u.kp = t->pad[l]; u.np = t->pad[l + 1]; u.k = t->units[l]; u.n = t->units[l + 1]; u.mp = mp; u.lr = t->lr;
        const dim3 grid(blocks_for((uint64_t)(u.kp / 16 + 1) * (u.np / 16)));
        if (t->regress) {
            const TrUpdAdam q{u, t->d_mw[l], t->d_vw[l], t->d_mb[l], t->d_vb[l], t->d_adam};
            hipLaunchKernelGGL(train_update_adam_kernel, grid, dim3(TR_THREADS), 0, s, q);
        } else {
            hipLaunchKernelGGL(train_update_kernel, grid, dim3(TR_THREADS), 0, s, u);
        }
        cur ^= 1;
    }
}

void tg_orphan(wsa_train_group* g);                                          // with wsa_train_group, below

// "" or why `order` (not NULL) is refused: an entry outside the training rows
std::string order_refusal(const wsa_trainer* t, const uint32_t* order) {
    for (uint32_t i = 0; i < t->n_train; i++)
        if (order[i] >= t->n_train) return "order[" + std::to_string(i) + "] = " + std::to_string(order[i]) + " is outside 0 .. " + std::to_string(t->n_train - 1);
    return "";
}

// the epoch's order through the trainer's pinned staging (two epochs deep) into d_order, on s
wsa_status stage_order(wsa_trainer* t, const uint32_t* order, hipStream_t s) {
    wsa_ctx* ctx = t->ctx;
    const int slot = t->epoch & 1;                                           // the copy that last read this staging buffer is two epochs back
    HIP_TRY(ctx, hipEventSynchronize(t->ev[slot]));
    std::memcpy(t->h_order[slot], order, (size_t)t->n_train * sizeof(uint32_t));
    HIP_TRY(ctx, hipMemcpyAsync(t->d_order, t->h_order[slot], (size_t)t->n_train * sizeof(uint32_t), hipMemcpyHostToDevice, s));
    HIP_TRY(ctx, hipEventRecord(t->ev[slot], s));
    return WSA_OK;
}

}  // namespace

namespace {

// both kinds of trainer: label != NULL a classifier's (TR-1), target != NULL a regression model's (TR-2)
wsa_status trainer_create(wsa_ctx* ctx, const wsa_model_desc* d, const double* feat, const int32_t* label, const double* target, bool regress,
                          uint32_t n_rows, uint32_t n_val, uint32_t batch_size, double learning_rate, double out_min, double out_max,
                          wsa_trainer** out) {
    if (!ctx || !d || !out) return fail(ctx, WSA_ERR_INVALID, "null argument");
    *out = nullptr;
    const int nl = d->n_layers;
    if (nl < 1 || nl > WSA_MODEL_MAX_LAYERS) return fail(ctx, WSA_ERR_INVALID, "a model has 1 .. 8 Dense layers, got " + std::to_string(nl));
    if (!d->units || !d->activation || !d->kernel || !d->bias) return fail(ctx, WSA_ERR_INVALID, "null units / activation / kernel / bias array");
    if (const char* why = wsa_model_width_refusal(d->units[0])) return fail(ctx, WSA_ERR_INVALID, "the model takes " + std::to_string(d->units[0]) + why);
    const int nin = d->units[0];
    const size_t xs = (size_t)((nin + 15) & ~15);                            // stride of the normalised rows: pad[0]
    for (int l = 0; l < nl; l++) {
        const int u = d->units[l + 1], a = d->activation[l];
        if (u < 1 || u > WSA_MODEL_MAX_WIDTH) return fail(ctx, WSA_ERR_INVALID, "layer " + std::to_string(l) + " has " + std::to_string(u) + " units (limit 1024)");
        if (a < WSA_ACT_LINEAR || a > WSA_ACT_SOFTMAX) return fail(ctx, WSA_ERR_INVALID, "layer " + std::to_string(l) + ": unknown activation " + std::to_string(a));
        if (a == WSA_ACT_SOFTMAX && l != nl - 1) return fail(ctx, WSA_ERR_INVALID, "softmax is only supported on the last layer");
        if (!d->kernel[l] || !d->bias[l]) return fail(ctx, WSA_ERR_INVALID, "null kernel / bias of layer " + std::to_string(l));
    }
    if (regress) {
        if (d->activation[nl - 1] == WSA_ACT_SOFTMAX) return fail(ctx, WSA_ERR_INVALID, "a regression model's last layer is linear, relu, sigmoid or tanh, not softmax (meanSquaredError)");
        if (d->units[nl] != 1) return fail(ctx, WSA_ERR_INVALID, "a regression model has one output unit, got " + std::to_string(d->units[nl]));
    } else if (d->activation[nl - 1] != WSA_ACT_SOFTMAX) return fail(ctx, WSA_ERR_INVALID, "training needs a softmax output layer (categoricalCrossentropy)");
    const int C = d->units[nl];
    if (C > WSA_MODEL_MAX_CLASSES) return fail(ctx, WSA_ERR_INVALID, "the output layer has " + std::to_string(C) + " units (limit 64)");
    if (!d->in_min || !d->in_max) return fail(ctx, WSA_ERR_INVALID, "null in_min / in_max");
    for (int k = 0; k < nin; k++) {
        if (!std::isfinite(d->in_min[k]) || !std::isfinite(d->in_max[k])) return fail(ctx, WSA_ERR_INVALID, "non-finite in_min / in_max of input " + std::to_string(k));
        if (d->in_max[k] == d->in_min[k]) return fail(ctx, WSA_ERR_INVALID, "feature " + std::to_string(k) + " has max == min: it cannot be normalised");
    }
    if (!feat || (regress ? !target : !label)) return fail(ctx, WSA_ERR_INVALID, regress ? "null feature / target pointer" : "null feature / label pointer");
    if (n_val >= n_rows) return fail(ctx, WSA_ERR_INVALID, "n_val " + std::to_string(n_val) + " leaves no training rows of " + std::to_string(n_rows));
    if (batch_size == 0) return fail(ctx, WSA_ERR_INVALID, "batch_size must be at least 1");
    if (!std::isfinite(learning_rate) || !std::isfinite((float)learning_rate)) return fail(ctx, WSA_ERR_INVALID, "the learning rate is not finite as an f32");
    if (regress) {
        if (!std::isfinite(out_min) || !std::isfinite(out_max)) return fail(ctx, WSA_ERR_INVALID, "non-finite out_min / out_max");
        if (out_max == out_min) return fail(ctx, WSA_ERR_INVALID, "the output has max == min: it cannot be normalised");
        for (uint32_t r = 0; r < n_rows; r++)
            if (!std::isfinite(target[r]) || !std::isfinite((float)((target[r] - out_min) / (out_max - out_min))))
                return fail(ctx, WSA_ERR_INVALID, "the target of row " + std::to_string(r) + " is not finite as a normalised f32");
    }
    if (!regress) for (uint32_t r = 0; r < n_rows; r++)
        if (label[r] < 0 || label[r] >= C) return fail(ctx, WSA_ERR_INVALID, "label " + std::to_string(label[r]) + " of row " + std::to_string(r) + " is outside 0 .. " + std::to_string(C - 1));
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    wsa_trainer* t = new wsa_trainer();
    t->ctx = ctx; t->nl = nl; t->n_rows = n_rows; t->n_val = n_val; t->n_train = n_rows - n_val;
    t->batch = batch_size < t->n_train ? batch_size : t->n_train;            // a larger batch is one step over all training rows
    t->n_steps = (t->n_train + t->batch - 1) / t->batch;
    t->mcap = up16(t->batch > n_val ? t->batch : n_val);
    t->lr = (float)learning_rate; t->regress = regress;
    t->in_min.assign(d->in_min, d->in_min + nin); t->in_max.assign(d->in_max, d->in_max + nin);
    if (d->labels) { t->has_labels = true; for (int c = 0; c < C; c++) t->labels.emplace_back(d->labels[c] ? d->labels[c] : ""); }
    int pmax = 0;
    for (int l = 0; l <= nl; l++) { t->units[l] = d->units[l]; t->pad[l] = (d->units[l] + 15) & ~15; if (l && t->pad[l] > pmax) pmax = t->pad[l]; }
    for (int l = 0; l < nl; l++) t->act[l] = d->activation[l];
    bool ok = true;
    for (int l = 0; l < nl && ok; l++) {                                      // zero padded as K6 pads them
        const int K = d->units[l], N = d->units[l + 1], kp = t->pad[l], np = t->pad[l + 1];
        std::vector<float> w((size_t)kp * np, 0.f), bb(np, 0.f);
        for (int k = 0; k < K; k++) std::memcpy(&w[(size_t)k * np], d->kernel[l] + (size_t)k * N, N * sizeof(float));
        std::memcpy(bb.data(), d->bias[l], N * sizeof(float));
        ok = t->mem.upload(&t->d_w[l], w) && t->mem.upload(&t->d_b[l], bb) && t->mem.alloc(&t->d_a[l + 1], (size_t)t->mcap * np, true);
        if (regress) ok = ok && t->mem.alloc(&t->d_mw[l], w.size(), true) && t->mem.alloc(&t->d_vw[l], w.size(), true)
                          && t->mem.alloc(&t->d_mb[l], bb.size(), true) && t->mem.alloc(&t->d_vb[l], bb.size(), true);
    }
    std::vector<uint32_t> ident(t->n_train);
    for (uint32_t i = 0; i < t->n_train; i++) ident[i] = i;
    double *d_feat = nullptr, *d_mn = nullptr, *d_mx = nullptr, *d_y = nullptr;
    {
        wsa::DevArena tmp;                                                   // the double rows live only until they are normalised
        ok = ok && t->mem.alloc(&t->d_dz[0], (size_t)t->mcap * pmax, true) && t->mem.alloc(&t->d_dz[1], (size_t)t->mcap * pmax, true)
             && t->mem.alloc(&t->d_x, (size_t)n_rows * xs) && (regress ? t->mem.alloc(&t->d_target, n_rows) && t->mem.alloc(&t->d_adam, 4) : t->mem.alloc(&t->d_label, n_rows))
             && t->mem.alloc(&t->d_order, t->n_train) && t->mem.upload(&t->d_identity, ident)
             && t->mem.alloc(&t->d_part_loss, t->n_steps + 1, true) && t->mem.alloc(&t->d_part_hit, t->n_steps + 1, true)
             && t->mem.alloc(&t->d_stats, 1, true)
             && hipHostMalloc(reinterpret_cast<void**>(&t->h_order[0]), (size_t)t->n_train * sizeof(uint32_t), hipHostMallocDefault) == hipSuccess
             && hipHostMalloc(reinterpret_cast<void**>(&t->h_order[1]), (size_t)t->n_train * sizeof(uint32_t), hipHostMallocDefault) == hipSuccess
             && hipEventCreateWithFlags(&t->ev[0], hipEventDisableTiming) == hipSuccess && hipEventCreateWithFlags(&t->ev[1], hipEventDisableTiming) == hipSuccess
             && tmp.alloc(&d_feat, (size_t)n_rows * nin) && tmp.alloc(&d_mn, (size_t)nin) && tmp.alloc(&d_mx, (size_t)nin)
             && hipMemcpy(d_feat, feat, (size_t)n_rows * nin * sizeof(double), hipMemcpyHostToDevice) == hipSuccess
             && hipMemcpy(d_mn, d->in_min, (size_t)nin * sizeof(double), hipMemcpyHostToDevice) == hipSuccess
             && hipMemcpy(d_mx, d->in_max, (size_t)nin * sizeof(double), hipMemcpyHostToDevice) == hipSuccess
             && (regress ? tmp.alloc(&d_y, n_rows) && hipMemcpy(d_y, target, (size_t)n_rows * sizeof(double), hipMemcpyHostToDevice) == hipSuccess
                         : hipMemcpy(t->d_label, label, (size_t)n_rows * sizeof(int32_t), hipMemcpyHostToDevice) == hipSuccess);
        if (ok && regress) {
            hipLaunchKernelGGL(train_normalise_target_kernel, dim3((n_rows + 255) / 256), dim3(256), 0, nullptr, d_y, out_min, out_max, (uint64_t)n_rows, t->d_target);
            hipLaunchKernelGGL(train_adam_reset_kernel, dim3(1), dim3(1), 0, nullptr, t->d_adam);
        }
        if (ok) {
            const uint64_t total = (uint64_t)n_rows * xs;
            hipLaunchKernelGGL(train_normalise_kernel, dim3((uint32_t)((total + 255) / 256)), dim3(256), 0, nullptr, d_feat, d_mn, d_mx, (uint64_t)n_rows, nin, (int)xs, t->d_x);
            ok = hipGetLastError() == hipSuccess && hipDeviceSynchronize() == hipSuccess;
        }
    }
    if (!ok) {
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
    return trainer_create(ctx, d, feat, label, nullptr, false, n_rows, n_val, batch_size, learning_rate, 0.0, 1.0, out);
}

wsa_status wsa_regress_trainer_create(wsa_ctx* ctx, const wsa_model_desc* d, const double* feat, const double* target, uint32_t n_rows,
                                      uint32_t n_val, uint32_t batch_size, double learning_rate, double out_min, double out_max, wsa_trainer** out) {
    return trainer_create(ctx, d, feat, nullptr, target, true, n_rows, n_val, batch_size, learning_rate, out_min, out_max, out);
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
    const uint32_t* idx = t->d_identity;
    if (order) {
        const wsa_status st = stage_order(t, order, s);
        if (st != WSA_OK) return st;
        idx = t->d_order;
    }
    for (uint32_t step = 0; step < t->n_steps; step++) enqueue_step(t, idx, step, s);
    if (t->n_val) {                                                          // the same forward over the validation rows, after the last update
        enqueue_forward(t, nullptr, t->n_train, t->n_val, s);
        enqueue_loss(t, nullptr, t->n_train, t->n_val, nullptr, t->n_steps, s);
    }
    t->epoch++;
    TrFin f{t->d_part_loss, t->d_part_hit, t->n_steps, t->n_train, t->n_val, t->epoch, t->d_stats};
    hipLaunchKernelGGL(train_finish_kernel, dim3(1), dim3(256), 0, s, f);
    HIP_TRY(ctx, hipGetLastError());
    return WSA_OK;
}

wsa_status wsa_trainer_stats(wsa_trainer* t, void* stream, wsa_train_stats* out) {
    if (!t) return WSA_ERR_INVALID;
    wsa_ctx* ctx = t->ctx;
    if (!out) return fail(ctx, WSA_ERR_INVALID, "null argument");
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipMemcpyAsync(out, t->d_stats, sizeof(wsa_train_stats), hipMemcpyDeviceToHost, s));
    HIP_TRY(ctx, hipStreamSynchronize(s));
    return WSA_OK;
}

wsa_status wsa_trainer_copy_weights(wsa_trainer* t, void* stream, float* const* kernel, float* const* bias) {
    if (!t) return WSA_ERR_INVALID;
    wsa_ctx* ctx = t->ctx;
    if (!kernel || !bias) return fail(ctx, WSA_ERR_INVALID, "null kernel / bias array");
    for (int l = 0; l < t->nl; l++) if (!kernel[l] || !bias[l]) return fail(ctx, WSA_ERR_INVALID, "null kernel / bias of layer " + std::to_string(l));
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    for (int l = 0; l < t->nl; l++) {                                        // strided: the padded columns stay behind
        const size_t n = (size_t)t->units[l + 1] * sizeof(float);
        HIP_TRY(ctx, hipMemcpy2DAsync(kernel[l], n, t->d_w[l], (size_t)t->pad[l + 1] * sizeof(float), n, t->units[l], hipMemcpyDeviceToHost, s));
        HIP_TRY(ctx, hipMemcpyAsync(bias[l], t->d_b[l], n, hipMemcpyDeviceToHost, s));
    }
    HIP_TRY(ctx, hipStreamSynchronize(s));
    return WSA_OK;
}

wsa_status wsa_trainer_model(wsa_trainer* t, void* stream, wsa_model** out) {
    if (!t) return WSA_ERR_INVALID;
    wsa_ctx* ctx = t->ctx;
    if (!out) return fail(ctx, WSA_ERR_INVALID, "null argument");
    *out = nullptr;
    std::vector<std::vector<float>> k(t->nl), b(t->nl);
    std::vector<float*> kp(t->nl), bp(t->nl);
    for (int l = 0; l < t->nl; l++) {
        k[l].resize((size_t)t->units[l] * t->units[l + 1]); b[l].resize(t->units[l + 1]);
        kp[l] = k[l].data(); bp[l] = b[l].data();
    }
    const wsa_status st = wsa_trainer_copy_weights(t, stream, kp.data(), bp.data());
    if (st != WSA_OK) return st;
    std::vector<const char*> lab;
    for (const std::string& x : t->labels) lab.push_back(x.c_str());
    wsa_model_desc d{};
    d.n_layers = t->nl; d.units = t->units; d.activation = t->act;
    d.kernel = kp.data(); d.bias = bp.data(); d.in_min = t->in_min.data(); d.in_max = t->in_max.data();
    d.labels = t->has_labels ? lab.data() : nullptr;
    return wsa_model_create(ctx, &d, out);
}

}  // extern "C"

// ---- training groups (K7g, specification TG-1)
struct wsa_train_group {
    wsa_ctx* ctx = nullptr;
    uint32_t n = 0;
    wsa_trainer* member[WSA_TRAIN_GROUP_MAX] = {};
    TgMember* d_tab = nullptr;                                 // all the group owns
    wsa::DevArena mem;
};

namespace {

// TG-1's launch count from the members' shapes alone; walk(step or TG_VALIDATION, Lmax) is called once per step that has a member,
// in the order the launches go out, so wsa_train_group_epoch and the formula cannot drift apart
template <typename Walk>
uint64_t group_plan(const uint32_t* nl, const uint32_t* n_steps, const uint32_t* n_val, uint32_t n, Walk walk) {
    uint32_t longest = 0, lval = 0;
    for (uint32_t i = 0; i < n; i++) { if (n_steps[i] > longest) longest = n_steps[i]; if (n_val[i] && nl[i] > lval) lval = nl[i]; }
    uint64_t launches = 0;
    for (uint32_t step = 0; step < longest; step++) {
        uint32_t lmax = 0;
        for (uint32_t i = 0; i < n; i++) if (n_steps[i] > step && nl[i] > lmax) lmax = nl[i];
        launches += 3ull * lmax;                                             // lmax forward, the loss, lmax - 1 backward, lmax update
        walk(step, lmax);
    }
    if (lval) { launches += lval + 1; walk(TG_VALIDATION, lval); }           // forward + loss over the validation rows
    return launches + 1;                                                     // the finish
}

// does member t take part in the launches of `step` (or of the validation pass)?
inline bool tg_active(const wsa_trainer* t, uint32_t step) { return step == TG_VALIDATION ? t->n_val > 0 : t->n_steps > step; }
inline uint32_t tg_rows(const wsa_trainer* t, uint32_t step) {               // up16(m) of the step
    if (step == TG_VALIDATION) return up16(t->n_val);
    const uint32_t off = step * t->batch;
    return up16(t->n_train - off < t->batch ? t->n_train - off : t->batch);
}

// a member is being destroyed before its group: the table points at its buffers, so the group lets go of every member and is empty
void tg_orphan(wsa_train_group* g) {
    for (uint32_t i = 0; i < g->n; i++) g->member[i]->group = nullptr;
    g->n = 0;
}

enum TgStage { TG_FORWARD, TG_LOSS, TG_BACKWARD, TG_UPDATE };

// one grouped launch: the prefix of workgroup counts over the members that have `stage` at `pos` in `step`, then the kernel
void tg_launch(wsa_train_group* g, TgStage stage, uint32_t step, int pos, uint32_t order_mask, hipStream_t s) {
    TgLaunch a{};
    a.n = g->n; a.step = step; a.order_mask = order_mask; a.pos = pos;
    for (uint32_t i = 0; i < g->n; i++) {
        const wsa_trainer* t = g->member[i];
        uint32_t blocks = 0;
        if (tg_active(t, step)) {
            const uint64_t rb = tg_rows(t, step) / 16;
            const int l = stage == TG_FORWARD ? pos : t->nl - 1 - pos;       // the member's layer at this position
            switch (stage) {
                case TG_FORWARD: if (l < t->nl) blocks = blocks_for(rb * (t->pad[l + 1] / 16)); break;
                case TG_LOSS: blocks = 1; break;
                case TG_BACKWARD: if (l > 0) blocks = blocks_for(rb * (t->pad[l] / 16)); break;
                case TG_UPDATE: if (l >= 0) blocks = blocks_for((uint64_t)(t->pad[l] / 16 + 1) * (t->pad[l + 1] / 16)); break;
            }
        }
        a.prefix[i + 1] = a.prefix[i] + blocks;
    }
    for (uint32_t i = g->n; i < WSA_TRAIN_GROUP_MAX; i++) a.prefix[i + 1] = a.prefix[i];
    const dim3 grid(a.prefix[g->n]);
    if (grid.x == 0) return;
    switch (stage) {
        case TG_FORWARD: hipLaunchKernelGGL(train_group_forward_kernel, grid, dim3(TR_THREADS), 0, s, g->d_tab, a); break;
        case TG_LOSS: hipLaunchKernelGGL(train_group_loss_kernel, grid, dim3(TR_LOSS_THREADS), 0, s, g->d_tab, a); break;
        case TG_BACKWARD: hipLaunchKernelGGL(train_group_backward_kernel, grid, dim3(TR_THREADS), 0, s, g->d_tab, a); break;
        case TG_UPDATE: hipLaunchKernelGGL(train_group_update_kernel, grid, dim3(TR_THREADS), 0, s, g->d_tab, a); break;
    }
}

}  // namespace

extern "C" {

wsa_status wsa_train_group_launch_count(const uint32_t* nl, const uint32_t* n_train, const uint32_t* batch, const uint32_t* n_val,
                                        uint32_t n, uint64_t* per_epoch) {
    if (!nl || !n_train || !batch || !n_val || !per_epoch || n == 0 || n > WSA_TRAIN_GROUP_MAX) return WSA_ERR_INVALID;
    uint32_t steps[WSA_TRAIN_GROUP_MAX];
    for (uint32_t i = 0; i < n; i++) {
        if (nl[i] < 1 || nl[i] > WSA_MODEL_MAX_LAYERS || n_train[i] == 0 || batch[i] == 0) return WSA_ERR_INVALID;
        const uint32_t b = batch[i] < n_train[i] ? batch[i] : n_train[i];
        steps[i] = (n_train[i] + b - 1) / b;
    }
    *per_epoch = group_plan(nl, steps, n_val, n, [](uint32_t, uint32_t) {});
    return WSA_OK;
}

wsa_status wsa_train_group_create(wsa_ctx* ctx, wsa_trainer* const* members, uint32_t n, wsa_train_group** out) {
    if (!ctx || !members || !out) return fail(ctx, WSA_ERR_INVALID, "null argument");
    *out = nullptr;
    if (n == 0 || n > WSA_TRAIN_GROUP_MAX) return fail(ctx, WSA_ERR_INVALID, "a training group has 1 .. " + std::to_string(WSA_TRAIN_GROUP_MAX) + " members, got " + std::to_string(n));
    for (uint32_t i = 0; i < n; i++) {
        const std::string who = "member " + std::to_string(i);
        if (!members[i]) return fail(ctx, WSA_ERR_INVALID, who + " is NULL");
        if (members[i]->ctx != ctx) return fail(ctx, WSA_ERR_INVALID, who + " belongs to another context");
        for (uint32_t j = 0; j < i; j++)
            if (members[j] == members[i]) return fail(ctx, WSA_ERR_INVALID, who + " is the same trainer as member " + std::to_string(j));
        if (members[i]->group) return fail(ctx, WSA_ERR_INVALID, who + " is already in a living group");
    }
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    std::vector<TgMember> tab(n);
    for (uint32_t i = 0; i < n; i++) {
        const wsa_trainer* t = members[i];
        TgMember& m = tab[i];
        std::memset(&m, 0, sizeof m);
        m.x = t->d_x; m.order = t->d_order; m.identity = t->d_identity; m.label = t->d_label; m.target = t->d_target; m.adam = t->d_adam;
        for (int l = 0; l < t->nl; l++) {
            m.w[l] = t->d_w[l]; m.b[l] = t->d_b[l]; m.mw[l] = t->d_mw[l]; m.vw[l] = t->d_vw[l]; m.mb[l] = t->d_mb[l]; m.vb[l] = t->d_vb[l];
            m.act[l] = t->act[l];
        }
        for (int l = 0; l <= t->nl; l++) { m.a[l] = t->d_a[l]; m.units[l] = t->units[l]; m.pad[l] = t->pad[l]; }
        m.dz[0] = t->d_dz[0]; m.dz[1] = t->d_dz[1];
        m.part_loss = t->d_part_loss; m.part_hit = t->d_part_hit; m.stats = t->d_stats;
        m.nl = t->nl; m.regress = t->regress ? 1 : 0;
        m.n_train = t->n_train; m.n_val = t->n_val; m.batch = t->batch; m.n_steps = t->n_steps; m.lr = t->lr;
    }
    wsa_train_group* g = new wsa_train_group();
    g->ctx = ctx; g->n = n;
    if (!g->mem.upload(&g->d_tab, tab)) {
        const std::string msg = std::string("device allocation / copy failed: ") + hipGetErrorString(hipGetLastError());
        delete g;
        return fail(ctx, WSA_ERR_HIP, msg);
    }
    for (uint32_t i = 0; i < n; i++) { g->member[i] = members[i]; members[i]->group = g; }
    *out = g;
    return WSA_OK;
}

void wsa_train_group_destroy(wsa_train_group* g) {
    if (!g) return;
    (void)hipSetDevice(g->ctx->device);
    (void)hipDeviceSynchronize();                                            // launches still in flight read the table
    for (uint32_t i = 0; i < g->n; i++) g->member[i]->group = nullptr;
    delete g;
}

wsa_status wsa_train_group_epoch(wsa_train_group* g, const uint32_t* const* orders, void* stream) {
    if (!g) return WSA_ERR_INVALID;
    wsa_ctx* ctx = g->ctx;
    if (g->n == 0) return fail(ctx, WSA_ERR_INVALID, "a member of the group was destroyed before the group: the group is empty");
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    for (uint32_t i = 0; orders && i < g->n; i++) {                          // every member's order before anything is enqueued
        if (!orders[i]) continue;
        const std::string why = order_refusal(g->member[i], orders[i]);
        if (!why.empty()) return fail(ctx, WSA_ERR_INVALID, "member " + std::to_string(i) + ": " + why);
    }
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    uint32_t order_mask = 0, nl[WSA_TRAIN_GROUP_MAX], n_steps[WSA_TRAIN_GROUP_MAX], n_val[WSA_TRAIN_GROUP_MAX];
    for (uint32_t i = 0; i < g->n; i++) {
        wsa_trainer* t = g->member[i];
        nl[i] = (uint32_t)t->nl; n_steps[i] = t->n_steps; n_val[i] = t->n_val;
        if (orders && orders[i]) {
            const wsa_status st = stage_order(t, orders[i], s);
            if (st != WSA_OK) return st;
            order_mask |= 1u << i;
        }
    }
    group_plan(nl, n_steps, n_val, g->n, [&](uint32_t step, uint32_t lmax) {
        for (uint32_t l = 0; l < lmax; l++) tg_launch(g, TG_FORWARD, step, (int)l, order_mask, s);
        tg_launch(g, TG_LOSS, step, 0, order_mask, s);
        if (step == TG_VALIDATION) return;
        for (uint32_t j = 0; j < lmax; j++) {                                // a layer's backward reads its weights: before their update
            if (j + 1 < lmax) tg_launch(g, TG_BACKWARD, step, (int)j, order_mask, s);
            tg_launch(g, TG_UPDATE, step, (int)j, order_mask, s);
        }
    });
    TgFinish f{};
    for (uint32_t i = 0; i < g->n; i++) f.epoch[i] = ++g->member[i]->epoch;
    hipLaunchKernelGGL(train_group_finish_kernel, dim3(g->n), dim3(256), 0, s, g->d_tab, f);
    HIP_TRY(ctx, hipGetLastError());
    return WSA_OK;
}

wsa_status wsa_train_group_stats(wsa_train_group* g, void* stream, wsa_train_stats* out) {
    if (!g) return WSA_ERR_INVALID;
    wsa_ctx* ctx = g->ctx;
    if (!out) return fail(ctx, WSA_ERR_INVALID, "null argument");
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    for (uint32_t i = 0; i < g->n; i++)
        HIP_TRY(ctx, hipMemcpyAsync(out + i, g->member[i]->d_stats, sizeof(wsa_train_stats), hipMemcpyDeviceToHost, s));
    HIP_TRY(ctx, hipStreamSynchronize(s));
    return WSA_OK;
}

wsa_status wsa_train_group_launches(const wsa_train_group* g, uint32_t* per_epoch) {
    if (!g) return WSA_ERR_INVALID;
    if (!per_epoch) return fail(g->ctx, WSA_ERR_INVALID, "null argument");
    uint32_t nl[WSA_TRAIN_GROUP_MAX], n_steps[WSA_TRAIN_GROUP_MAX], n_val[WSA_TRAIN_GROUP_MAX];
    for (uint32_t i = 0; i < g->n; i++) { nl[i] = (uint32_t)g->member[i]->nl; n_steps[i] = g->member[i]->n_steps; n_val[i] = g->member[i]->n_val; }
    *per_epoch = (uint32_t)group_plan(nl, n_steps, n_val, g->n, [](uint32_t, uint32_t) {});
    return WSA_OK;
}

}  // extern "C"
