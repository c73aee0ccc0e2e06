// classify.hip — K6 (the app's dense classifier over feature rows, f32 MFMA), its grouped forms K6e (every member over every row) and
// K6f (every member over its own row list, crossval.hip), the model and ensemble objects
// and the row-wise part of the C ABI (include/wsa.h "Syllable classification").  The per-callback fold K6b is classify_fold.hpp,
// run over a batch by classify_batch.hip and inside a stream step by classify_stream.hip.
//
// Stands in for the reference APPLICATION's prediction path: ml5 classifyMultiple (tfjs Dense layers, float32) over the syllables of a
// level-13 callback.
#include <atomic>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>
#include "classify_internal.hpp"

using wsa_api::fail;
using namespace wsa_classify;

namespace {

constexpr int CLS_LDS_BUDGET = 160 * 1024;

// ml5 unnormalizeValue on the f32 output of a regression model's one unit (ref dist/ml5.min.js @2469277, t * (max - min) + min with
// JavaScript doubles): the product and the sum are rounded separately, JavaScript has no fused multiply-add
__device__ __forceinline__ double unnormalise_value(float p, double out_min, double out_span) {
#pragma clang fp contract(off)
    const double scaled = (double)p * out_span;
    return scaled + out_min;
}

__device__ __forceinline__ float activate(float v, int act) {
    switch (act) {
        case WSA_ACT_RELU: return v < 0.f ? 0.f : v;                          // tfjs relu
        case WSA_ACT_SIGMOID: return 1.f / (1.f + expf(-v));
        case WSA_ACT_TANH: return tanhf(v);
        default: return v;
    }
}

typedef float f32x4 __attribute__((ext_vector_type(4)));

// One workgroup per tile of TM = 16 RB rows (grid-stride over tiles).  Activations stay in LDS between layers (two buffers of TM x S
// floats); a wave owns 16-column blocks of a layer's output and all RB row blocks of the tile, so one B fragment (weights, from global
// memory, L2-resident) feeds RB MFMAs.  mfma_f32_16x16x4f32: lane l holds A[row l&15][k l>>4], B[k l>>4][col l&15]; D col = l&15,
// row = 4 (l>>4) + i.  S = 64 j + 4 keeps both the A reads and the epilogue's writes on 64 distinct banks.
// The body is one tile (classify_tile): K6's own kernel strides over the tiles of one model, K6e over the (member, tile) pairs of an
// ensemble, so a row's probabilities are the same bits whichever launch computed them.
// MAP (K6f): row i of the n rows of the launch is row p.row_map[i] of feat and of prob / value; the list is read only for i < n.
template <int RB, bool MAP = false>
__device__ __forceinline__ void classify_tile(const ClsParams& p, float* s_act, uint32_t tile, uint32_t n) {
    constexpr int TM = 16 * RB;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nwaves = CLS_THREADS / 64;
    const int S = p.S;
    const auto at = [&](uint32_t i) -> size_t { if constexpr (MAP) return p.row_map[i]; else return i; };
    {
        const uint32_t row0 = tile * TM;
        float* in = s_act;
        float* out = s_act + TM * S;
        const int p0 = p.L[0].kp;
        for (int idx = tid; idx < TM * p0; idx += CLS_THREADS) {
            const int r = idx / p0, k = idx - r * p0;
            float v = 0.f;
            if (row0 + r < n && k < p.nin) {                                   // ml5 normalizeValue in double, then the f32 tensor
                const double x = p.feat[at(row0 + r) * p.stride + k];
                v = (float)((x - p.in_min[k]) / (p.in_max[k] - p.in_min[k]));
            }
            in[r * S + k] = v;
        }
        __syncthreads();
        for (int l = 0; l < p.n_layers; l++) {
            const ClsLayer L = p.L[l];
            const bool last = l == p.n_layers - 1;
            for (int cb = wave; cb < L.np / 16; cb += nwaves) {
                const int n0 = cb * 16;
                f32x4 acc[RB];
#pragma unroll
                for (int rb = 0; rb < RB; rb++) acc[rb] = f32x4{0.f, 0.f, 0.f, 0.f};
                const float* wp = L.w + (size_t)(lane >> 4) * L.np + n0 + (lane & 15);
                const float* ap = in + (lane & 15) * S + (lane >> 4);
                for (int k1 = 0; k1 < L.kp; k1 += 16) {                        // kp is a multiple of 16: four loads in flight
                    float bv[4];
#pragma unroll
                    for (int j = 0; j < 4; j++) bv[j] = wp[(size_t)(k1 + 4 * j) * L.np];
#pragma unroll
                    for (int j = 0; j < 4; j++)
#pragma unroll
                        for (int rb = 0; rb < RB; rb++)
                            acc[rb] = __builtin_amdgcn_mfma_f32_16x16x4f32(ap[rb * 16 * S + k1 + 4 * j], bv[j], acc[rb], 0, 0, 0);
                }
                const int col = n0 + (lane & 15);
                const float bias = L.b[col];
#pragma unroll
                for (int rb = 0; rb < RB; rb++)
#pragma unroll
                    for (int i = 0; i < 4; i++) {
                        const int row = rb * 16 + (lane >> 4) * 4 + i;
                        float v = acc[rb][i] + bias;                            // tfjs Dense: matMul, then the bias, then the activation
                        if (L.act != WSA_ACT_SOFTMAX) v = activate(v, L.act);
                        if (col >= L.n && !last) v = 0.f;                       // padded columns are the next layer's zero K rows
                        out[row * S + col] = v;
                    }
            }
            __syncthreads();
            float* t = in; in = out; out = t;
        }
        // tfjs softmax: exp(x - logSumExp(x)), logSumExp = max + log(sum exp(x - max)); one lane per row
        const bool sm = p.L[p.n_layers - 1].act == WSA_ACT_SOFTMAX;
        for (int r = tid; r < TM; r += CLS_THREADS) {
            if (row0 + r >= n) continue;
            const float* x = in + r * S;
            const size_t row = at(row0 + r);
            if (p.nan_slot >= 0 && p.feat[row * p.stride + p.nan_slot] != 0.0) {   // no coefficients: nothing to predict from
                if (p.value) p.value[row] = __longlong_as_double(0x7ff8000000000000ll);
                else for (int c = 0; c < p.C; c++) p.prob[row * p.C + c] = __int_as_float(0x7fc00000);
                continue;
            }
            if (p.value) {                                                  // K6's regression epilogue: the one unit's output, un-normalised
                p.value[row] = unnormalise_value(x[0], p.out_min, p.out_span);
                continue;
            }
            float* o = p.prob + row * p.C;
            if (sm) {
                float m = x[0];
                for (int c = 1; c < p.C; c++) m = fmaxf(m, x[c]);
                float s = 0.f;
                for (int c = 0; c < p.C; c++) s += expf(x[c] - m);
                const float lse = m + logf(s);
                for (int c = 0; c < p.C; c++) o[c] = expf(x[c] - lse);
            } else {
                for (int c = 0; c < p.C; c++) o[c] = x[c];
            }
        }
        __syncthreads();
    }
}

template <int RB>
__global__ void __launch_bounds__(CLS_THREADS) classify_kernel(ClsParams p) {
    extern __shared__ __attribute__((aligned(16))) float s_act[];
    constexpr int TM = 16 * RB;
    const uint32_t n = p.d_n_rows ? *p.d_n_rows : p.n_rows;
    for (uint32_t tile = blockIdx.x; (uint64_t)tile * TM < n; tile += gridDim.x) classify_tile<RB>(p, s_act, tile, n);
}

// ---- K6e: every member of an ensemble (ref prediction.js:60-63, one nn_prediction per DB of available_DBs) in one launch.  The members'
// parameters sit in a device table, ordered by descending cost per tile; workgroups stride over one list of (member, tile) pairs whose
// tile counts come from the row count on the device, so the wide members' tiles start first and the small ones fill the tail.  Each
// member keeps the row-block factor it has on its own; the dynamic LDS is the largest member's need.
__global__ void __launch_bounds__(CLS_THREADS) classify_group_kernel(const ClsGroupEntry* __restrict__ tab, int n_members, const uint32_t* d_n_rows) {
    extern __shared__ __attribute__((aligned(16))) float s_act[];
    const uint32_t n = *d_n_rows;
    uint32_t total = 0;
    for (int d = 0; d < n_members; d++) { const uint32_t tm = 16u * (uint32_t)tab[d].rb; total += (n + tm - 1) / tm; }
    for (uint32_t i = blockIdx.x; i < total; i += gridDim.x) {
        int d = 0; uint32_t tile = i;
        for (; d < n_members - 1; d++) {
            const uint32_t tm = 16u * (uint32_t)tab[d].rb, t = (n + tm - 1) / tm;
            if (tile < t) break;
            tile -= t;
        }
        const ClsGroupEntry& e = tab[d];
        if (e.rb == 4) classify_tile<4>(e.p, s_act, tile, n);
        else if (e.rb == 2) classify_tile<2>(e.p, s_act, tile, n);
        else classify_tile<1>(e.p, s_act, tile, n);
    }
}

// ---- K6f: K6e with a row list per member (cross-validation, specification CV-1: member k is the model that did not see fold k, its list
// fold k's rows).  Member d runs over tab[d].n rows, row i of them being row tab[d].p.row_map[i] of the dense table: the tile loads from
// there and writes its probabilities or its value there, so the members fill disjoint rows of ONE table in place.  The work list, the order
// (descending cost per tile), the members' own row-block factors and the LDS are K6e's; the counts are the host's (the lists are made
// once), so a member with an empty list has no tile and the host launches nothing when every list is empty.
__global__ void __launch_bounds__(CLS_THREADS) classify_folds_kernel(const ClsFoldEntry* __restrict__ tab, int n_members) {
    extern __shared__ __attribute__((aligned(16))) float s_act[];
    uint32_t total = 0;
    for (int d = 0; d < n_members; d++) { const uint32_t tm = 16u * (uint32_t)tab[d].rb; total += (tab[d].n + tm - 1) / tm; }
    for (uint32_t i = blockIdx.x; i < total; i += gridDim.x) {
        int d = 0; uint32_t tile = i;
        for (; d < n_members - 1; d++) {
            const uint32_t tm = 16u * (uint32_t)tab[d].rb, t = (tab[d].n + tm - 1) / tm;
            if (tile < t) break;
            tile -= t;
        }
        const ClsFoldEntry& e = tab[d];
        if (e.rb == 4) classify_tile<4, true>(e.p, s_act, tile, e.n);
        else if (e.rb == 2) classify_tile<2, true>(e.p, s_act, tile, e.n);
        else classify_tile<1, true>(e.p, s_act, tile, e.n);
    }
}

}  // namespace

namespace wsa_classify {

uint64_t folds_table(const wsa_model* const* m, uint32_t n, const double* feat, const uint32_t* d_rows, const uint32_t* off, float* prob, double* value,
                     const double* out_min, const double* out_max, ClsFoldEntry* tab, size_t* lds) {
    std::vector<int> order(n);
    std::vector<double> cost(n);
    *lds = 0;
    for (uint32_t k = 0; k < n; k++) {
        order[k] = (int)k;
        double w = 0.0;
        for (int l = 0; l < m[k]->n_layers; l++) w += (double)m[k]->L[l].kp * m[k]->L[l].np;
        cost[k] = w * 16.0 * m[k]->rb;                             // multiply-adds of one tile
        const size_t need = (size_t)2 * 16 * m[k]->rb * m[k]->S * sizeof(float);
        *lds = need > *lds ? need : *lds;
    }
    for (uint32_t i = 1; i < n; i++)                               // stable insertion sort, descending
        for (uint32_t j = i; j > 0 && cost[order[j]] > cost[order[j - 1]]; j--) { const int t = order[j]; order[j] = order[j - 1]; order[j - 1] = t; }
    uint64_t tiles = 0;
    for (uint32_t i = 0; i < n; i++) {
        const int k = order[i];
        ClsFoldEntry e{};
        e.p = cls_params(m[k], feat, 0, nullptr, prob);
        if (value) e.p = regress_params(e.p, value, out_min[k], out_max[k] - out_min[k]);
        e.p.row_map = d_rows + off[k];
        e.rb = m[k]->rb; e.n = off[k + 1] - off[k];
        tab[i] = e;
        tiles += fold_tiles(e.n, e.rb);
    }
    return tiles;
}

void launch_classify_folds(const wsa_ctx* ctx, const ClsFoldEntry* d_tab, uint32_t n_members, uint64_t tiles, size_t lds, hipStream_t s) {
    hipLaunchKernelGGL(classify_folds_kernel, dim3(classify_grid(ctx, tiles)), dim3(CLS_THREADS), lds, s, d_tab, (int)n_members);
}

// V8 orders a key as an array index up to 2^32 - 2 ("4294967294"); "4294967295" and beyond are string keys
bool array_index_key(const char* s, int64_t* out) {
    if (!s || !*s) return false;
    if (s[0] == '0' && s[1]) return false;
    int64_t v = 0;
    for (const char* c = s; *c; c++) { if (*c < '0' || *c > '9') return false; v = v * 10 + (*c - '0'); if (v > 0xfffffffell) return false; }
    *out = v;
    return true;
}

ClsParams cls_params(const wsa_model* m, const double* feat, uint32_t n_rows, const uint32_t* d_n_rows, float* prob) {
    ClsParams p{};
    for (int l = 0; l < m->n_layers; l++) p.L[l] = m->L[l];
    p.n_layers = m->n_layers; p.C = m->C; p.S = m->S; p.in_min = m->d_min; p.in_max = m->d_max;
    p.feat = feat; p.n_rows = n_rows; p.d_n_rows = d_n_rows; p.prob = prob;
    p.nin = m->nin; p.stride = m->nin; p.nan_slot = -1;                       // dense rows of the model's own width
    return p;
}

void launch_classify(const wsa_model* m, const ClsParams& p, uint32_t rows_cap, hipStream_t s, int rb) {
    if (rb <= 0 || rb > m->rb) rb = m->rb;
    const int TM = 16 * rb;
    const uint32_t grid = classify_grid(m->ctx, (rows_cap + TM - 1) / TM);
    const size_t lds = (size_t)2 * TM * m->S * sizeof(float);
    if (rb == 4) hipLaunchKernelGGL(classify_kernel<4>, dim3(grid), dim3(CLS_THREADS), lds, s, p);
    else if (rb == 2) hipLaunchKernelGGL(classify_kernel<2>, dim3(grid), dim3(CLS_THREADS), lds, s, p);
    else hipLaunchKernelGGL(classify_kernel<1>, dim3(grid), dim3(CLS_THREADS), lds, s, p);
}

const char* regress_refusal(const wsa_model* m, double out_min, double out_max) {
    if (m->softmax) return "a regression model's last layer is linear, relu, sigmoid or tanh, not softmax";
    if (m->C != 1) return "a regression model has one output unit";
    if (!std::isfinite(out_min) || !std::isfinite(out_max)) return "non-finite out_min / out_max";
    if (out_max == out_min) return "the output has max == min: it cannot be un-normalised";
    return nullptr;
}

uint32_t group_table(const wsa_ensemble* e, const double* feat, const uint32_t* d_n_rows, float* const* prob, uint32_t rows_cap, bool one_block,
                     std::vector<ClsGroupEntry>& tab) {
    tab.assign(e->n, ClsGroupEntry{});
    uint64_t tiles = 0;
    for (uint32_t i = 0; i < e->n; i++) {
        const int d = e->order[i];
        tab[i].p = cls_params(e->m[d], feat, 0, d_n_rows, prob[d]);
        tab[i].rb = one_block ? 1 : e->m[d]->rb;
        tiles += (rows_cap + 16u * tab[i].rb - 1) / (16u * tab[i].rb);
    }
    return classify_grid(e->ctx, tiles);
}

void launch_classify_group(const ClsGroupEntry* d_tab, uint32_t n_members, const uint32_t* d_n_rows, uint32_t grid, size_t lds, hipStream_t s) {
    hipLaunchKernelGGL(classify_group_kernel, dim3(grid), dim3(CLS_THREADS), lds, s, d_tab, (int)n_members, d_n_rows);
}

}  // namespace wsa_classify

// NULL for the row width of an ML level, else the rest of the sentence every layer refuses the width with ("the model takes N" ...)
const char* wsa_model_width_refusal(int n_inputs) {
    if (n_inputs == 53 || n_inputs == 264 || n_inputs == 23) return nullptr;
    return " inputs; the feature rows have 53 (output_level 5 and 13), 264 (output_level 11) or 23 (output_level 12)";
}

extern "C" {

int32_t wsa_level_feature_count(int32_t output_level) {          // ref src/localstore.js:7 process_exp_features_len, src/index.js:723
    switch (output_level) {
        case 5: case 13: return WSA_NFEAT;
        case 11: return WSA_NUTT;
        case 12: return L12_NCOEF;
        default: return 0;
    }
}

wsa_status wsa_model_create(wsa_ctx* ctx, const wsa_model_desc* d, wsa_model** out) {
    if (!ctx || !d || !out) return fail(ctx, WSA_ERR_INVALID, "null argument");
    *out = nullptr;
    const int nl = d->n_layers;
    if (nl < 1 || nl > WSA_MODEL_MAX_LAYERS) return fail(ctx, WSA_ERR_INVALID, "a model has 1 .. 8 Dense layers, got " + std::to_string(nl));
    if (!d->units || !d->activation || !d->kernel || !d->bias) return fail(ctx, WSA_ERR_INVALID, "null units / activation / kernel / bias array");
    if (const char* why = wsa_model_width_refusal(d->units[0])) return fail(ctx, WSA_ERR_INVALID, "the model takes " + std::to_string(d->units[0]) + why);
    const int nin = d->units[0];
    for (int l = 0; l < nl; l++) {
        const int u = d->units[l + 1];
        if (u < 1 || u > WSA_MODEL_MAX_WIDTH) return fail(ctx, WSA_ERR_INVALID, "layer " + std::to_string(l) + " has " + std::to_string(u) + " units (limit 1024)");
        const int a = d->activation[l];
        if (a < WSA_ACT_LINEAR || a > WSA_ACT_SOFTMAX) return fail(ctx, WSA_ERR_INVALID, "layer " + std::to_string(l) + ": unknown activation " + std::to_string(a));
        if (a == WSA_ACT_SOFTMAX && l != nl - 1) return fail(ctx, WSA_ERR_INVALID, "softmax is only supported on the last layer");
        if (!d->kernel[l] || !d->bias[l]) return fail(ctx, WSA_ERR_INVALID, "null kernel / bias of layer " + std::to_string(l));
    }
    if (d->units[nl] > WSA_MODEL_MAX_CLASSES) return fail(ctx, WSA_ERR_INVALID, "the output layer has " + std::to_string(d->units[nl]) + " units (limit 64)");
    if (!d->in_min || !d->in_max) return fail(ctx, WSA_ERR_INVALID, "null in_min / in_max");
    for (int k = 0; k < nin; k++)
        if (!std::isfinite(d->in_min[k]) || !std::isfinite(d->in_max[k])) return fail(ctx, WSA_ERR_INVALID, "non-finite in_min / in_max of input " + std::to_string(k));
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    wsa_model* m = new wsa_model();
    m->ctx = ctx; m->n_layers = nl; m->nin = nin; m->C = d->units[nl]; m->softmax = d->activation[nl - 1] == WSA_ACT_SOFTMAX;
    int pmax = 0;
    std::vector<int> pad(nl + 1);
    for (int l = 0; l <= nl; l++) pad[l] = (d->units[l] + 15) & ~15;          // 16-column blocks; K in steps of 16 (four MFMAs)
    for (int l = 0; l <= nl; l++) pmax = pad[l] > pmax ? pad[l] : pmax;
    m->S = ((pmax + 63) & ~63) + 4;
    m->rb = 4;
    while (m->rb > 1 && (size_t)2 * 16 * m->rb * m->S * sizeof(float) > (size_t)CLS_LDS_BUDGET) m->rb >>= 1;
    bool ok = true;
    for (int l = 0; l < nl && ok; l++) {
        const int K = d->units[l], N = d->units[l + 1], kp = pad[l], np = pad[l + 1];
        std::vector<float> w((size_t)kp * np, 0.f), bb(np, 0.f);
        for (int k = 0; k < K; k++) std::memcpy(&w[(size_t)k * np], d->kernel[l] + (size_t)k * N, N * sizeof(float));
        std::memcpy(bb.data(), d->bias[l], N * sizeof(float));
        float *dw = nullptr, *db = nullptr;
        ok = m->mem.upload(&dw, w) && m->mem.upload(&db, bb);
        m->L[l] = ClsLayer{dw, db, kp, np, N, d->activation[l]};
    }
    std::vector<int64_t> kr(m->C, -1);
    if (d->labels) for (int c = 0; c < m->C; c++) { int64_t v; if (array_index_key(d->labels[c], &v)) kr[c] = v; }
    m->key_rank = kr;
    ok = ok && m->mem.alloc(&m->d_min, (size_t)nin) && m->mem.alloc(&m->d_max, (size_t)nin) && m->mem.upload(&m->d_key_rank, kr)
         && hipMemcpy(m->d_min, d->in_min, (size_t)nin * sizeof(double), hipMemcpyHostToDevice) == hipSuccess
         && hipMemcpy(m->d_max, d->in_max, (size_t)nin * sizeof(double), hipMemcpyHostToDevice) == hipSuccess;
    if (!ok) {
        const std::string msg = std::string("device allocation / copy failed: ") + hipGetErrorString(hipGetLastError());
        wsa_model_destroy(m);
        return fail(ctx, WSA_ERR_HIP, msg);
    }
    *out = m;
    return WSA_OK;
}

void wsa_model_destroy(wsa_model* m) {
    if (!m) return;
    (void)hipSetDevice(m->ctx->device);
    delete m;
}

// what K8 (dbstats.hip) has to know of a model before it hands it to wsa_classify_rows / wsa_regress_rows
void wsa_model_info_internal(const wsa_model* m, wsa_ctx** ctx, int* n_classes, int* softmax) {
    *ctx = m->ctx; *n_classes = m->C; *softmax = m->softmax ? 1 : 0;
}
int wsa_model_inputs_internal(const wsa_model* m) { return m->nin; }
const int64_t* wsa_model_key_rank_internal(const wsa_model* m) { return m->d_key_rank; }

wsa_status wsa_classify_rows(const wsa_model* m, const double* d_feat, uint32_t n_rows, float* d_prob, void* stream) {
    if (!m) return WSA_ERR_INVALID;
    wsa_ctx* ctx = m->ctx;
    if (n_rows && (!d_feat || !d_prob)) return fail(ctx, WSA_ERR_INVALID, "null feature / probability pointer");
    if (!n_rows) return WSA_OK;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    launch_classify(m, cls_params(m, d_feat, n_rows, nullptr, d_prob), n_rows, reinterpret_cast<hipStream_t>(stream));
    HIP_TRY(ctx, hipGetLastError());
    return WSA_OK;
}

// ---- regression models (ords_<label>): K6 with the un-normalising epilogue (ref src/neuralmodel.js:410-585, predict_db_nn / predict_single)
wsa_status wsa_regress_rows(const wsa_model* m, double out_min, double out_max, const double* d_feat, uint32_t n_rows, double* d_value, void* stream) {
    if (!m) return WSA_ERR_INVALID;
    wsa_ctx* ctx = m->ctx;
    if (const char* why = regress_refusal(m, out_min, out_max)) return fail(ctx, WSA_ERR_INVALID, why);
    if (n_rows && (!d_feat || !d_value)) return fail(ctx, WSA_ERR_INVALID, "null feature / value pointer");
    if (!n_rows) return WSA_OK;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    launch_classify(m, regress_params(cls_params(m, d_feat, n_rows, nullptr, nullptr), d_value, out_min, out_max - out_min), n_rows, reinterpret_cast<hipStream_t>(stream));
    HIP_TRY(ctx, hipGetLastError());
    return WSA_OK;
}

// ---- ensembles: every model DB of the app's available_DBs in one pass (ref src/prediction.js:12, 60-63, 127-169)
wsa_status wsa_ensemble_create(wsa_ctx* ctx, const wsa_model* const* models, uint32_t n, wsa_ensemble** out) {
    if (!ctx || !out) return fail(ctx, WSA_ERR_INVALID, "null argument");
    *out = nullptr;
    if (n < 1 || n > WSA_ENSEMBLE_MAX) return fail(ctx, WSA_ERR_INVALID, "an ensemble has 1 .. 8 members, got " + std::to_string(n));
    if (!models) return fail(ctx, WSA_ERR_INVALID, "null member array");
    for (uint32_t d = 0; d < n; d++) {
        if (!models[d]) return fail(ctx, WSA_ERR_INVALID, "member " + std::to_string(d) + " is NULL");
        if (models[d]->ctx != ctx) return fail(ctx, WSA_ERR_INVALID, "member " + std::to_string(d) + " was created on another context (or device) than the ensemble");
        if (models[d]->nin != WSA_NFEAT)
            return fail(ctx, WSA_ERR_INVALID, "member " + std::to_string(d) + " takes " + std::to_string(models[d]->nin) + " inputs: an ensemble classifies the 53-feature rows of output_level 5 and 13");
    }
    static std::atomic<uint64_t> serial{0};
    wsa_ensemble* e = new wsa_ensemble();
    e->ctx = ctx; e->n = n; e->serial = ++serial;
    double cost[WSA_ENSEMBLE_MAX];
    for (uint32_t d = 0; d < n; d++) {
        const wsa_model* m = models[d];
        e->m[d] = m; e->order[d] = (int)d; e->softmax = e->softmax && m->softmax;
        double w = 0.0;
        for (int l = 0; l < m->n_layers; l++) w += (double)m->L[l].kp * m->L[l].np;
        cost[d] = w * 16.0 * m->rb;                                // multiply-adds of one tile
        const size_t lb = (size_t)2 * 16 * m->rb * m->S * sizeof(float), ls = (size_t)2 * 16 * m->S * sizeof(float);
        e->lds_batch = lb > e->lds_batch ? lb : e->lds_batch; e->lds_stream = ls > e->lds_stream ? ls : e->lds_stream;
    }
    for (uint32_t i = 1; i < n; i++)                               // stable insertion sort, descending
        for (uint32_t j = i; j > 0 && cost[e->order[j]] > cost[e->order[j - 1]]; j--) { const int t = e->order[j]; e->order[j] = e->order[j - 1]; e->order[j - 1] = t; }
    *out = e;
    return WSA_OK;
}

void wsa_ensemble_destroy(wsa_ensemble* e) { delete e; }

}  // extern "C"
