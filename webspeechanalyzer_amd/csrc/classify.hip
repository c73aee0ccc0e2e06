// classify.hip — K6 (the app's dense classifier over feature rows, f32 MFMA) and K6b (the app's per-callback fold, exact double),
// and their part of the C ABI (include/wsa.h "Syllable classification").
//
// Stands in for the reference APPLICATION's prediction path: ml5 classifyMultiple (tfjs Dense layers, float32) over the syllables of a
// level-13 callback, then src/prediction.js:86-169 (weights sqrt(duration), per-label sums, segment label, per-launch accumulator).
#include <cmath>
#include <cstring>
#include <string>
#include <vector>
#include "host_plan.hpp"

using wsa_api::fail;

namespace {

constexpr int CLS_THREADS = 512;                 // 8 waves: 2 per SIMD
constexpr int CLS_LDS_BUDGET = 160 * 1024;

struct ClsLayer { const float* w; const float* b; int kp, np, n, act; };     // w [kp][np], b [np], zero padded; n = real width
struct ClsParams {
    ClsLayer L[WSA_MODEL_MAX_LAYERS]; int n_layers, C, S;                      // S = LDS row stride (floats)
    const double* in_min; const double* in_max;
    const double* feat; uint32_t n_rows; const uint32_t* d_n_rows;           // rows = *d_n_rows when set (a batch's count, on the device)
    float* prob;
};

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
template <int RB>
__global__ void __launch_bounds__(CLS_THREADS) classify_kernel(ClsParams p) {
    extern __shared__ __attribute__((aligned(16))) float s_act[];
    constexpr int TM = 16 * RB;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nwaves = CLS_THREADS / 64;
    const uint32_t n = p.d_n_rows ? *p.d_n_rows : p.n_rows;
    const int S = p.S;
    for (uint32_t tile = blockIdx.x; (uint64_t)tile * TM < n; tile += gridDim.x) {
        const uint32_t row0 = tile * TM;
        float* in = s_act;
        float* out = s_act + TM * S;
        const int p0 = p.L[0].kp;
        for (int idx = tid; idx < TM * p0; idx += CLS_THREADS) {
            const int r = idx / p0, k = idx - r * p0;
            float v = 0.f;
            if (row0 + r < n && k < WSA_NFEAT) {                               // ml5 normalizeValue in double, then the f32 tensor
                const double x = p.feat[(size_t)(row0 + r) * WSA_NFEAT + k];
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
            float* o = p.prob + (size_t)(row0 + r) * p.C;
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

// ---- K6b: one wave per clip, classes on lanes, callbacks walked in order (ref prediction.js:86-169 with one model DB)
struct FoldParams {
    uint32_t n_clips, C; double step_s;
    const int32_t* meta; const uint32_t* row_off; const float* prob;
    const int32_t* key_rank;                 // [C] array-index value of the label, or -1
    int32_t* t_label; double* t_conf; int32_t* t_n; int32_t* t_local;   // per row: the callback that starts there (t_n = 0 elsewhere)
    uint32_t* clip_cb;                       // [n_clips] callbacks per clip
    double* clip_conf;                       // [n_clips][C]
};

// parseFloat(x.toFixed(3)): k = the integer nearest to 1000 x (the exact binary value; the larger on a tie), then k / 1000 (correctly
// rounded, = parseFloat of the decimal string).  k is right iff k - 0.5 <= 1000 x < k + 0.5; the sign of fma(x, 1000, -(k -+ 0.5)) is
// that of the exact difference (one rounding never changes a sign).
__device__ double fixed3(double x) {
    double k = floor(x * 1000.0 + 0.5);
    for (int it = 0; it < 4; it++) {
        if (fma(x, 1000.0, -(k - 0.5)) < 0.0) k -= 1.0;
        else if (fma(x, 1000.0, -(k + 0.5)) >= 0.0) k += 1.0;
        else break;
    }
    return k / 1000.0;
}

__device__ __forceinline__ double wave_max_d(double v) {
    for (int o = 32; o > 0; o >>= 1) { const double w = __shfl_xor(v, o); v = w > v ? w : v; }
    return v;
}
__device__ __forceinline__ long long wave_min_ll(long long v) {
    for (int o = 32; o > 0; o >>= 1) { const long long w = __shfl_xor(v, o); v = w < v ? w : v; }
    return v;
}

// what one clip's (or stream's) fold carries from callback to callback, per lane = class
struct FoldAcc {
    double acc_all;                          // Label_conf_all[label]
    bool in_all;                             // the label is a key of Label_conf_all
    long long first;                         // its insertion stamp
    long long stamp;
};

// one callback: rows r .. e - 1 (the same clip / stream and si); label -1 / -2 as wsa_class_result
__device__ __forceinline__ void fold_callback(const int32_t* meta, const float* prob, uint32_t C, double step_s, int lane, bool cls, int kr,
                                              uint32_t r, uint32_t e, FoldAcc& a, int& label, double& conf) {
    const uint32_t nsyl = e - r;
    double seg_weight = 0.0;                 // sum of parseFloat(seg_time[ph][1]) (ref prediction.js:55)
    for (uint32_t q = r; q < e; q++) seg_weight += fixed3((double)(meta[(size_t)q * 8 + 3] + 1) * step_s);
    label = -2; conf = 0.0;
    if (!(seg_weight > 0.0)) return;
    double acc_seg = 0.0; bool in_seg = false;
    for (uint32_t q = r; q < e; q++) {
        const double w = __dsqrt_rn(fixed3((double)(meta[(size_t)q * 8 + 3] + 1) * step_s));
        const float pf = cls ? prob[(size_t)q * C + lane] : 0.f;
        // rank in classifyMultiple's order: confidence descending, ties in legend order (a stable sort)
        int rank = 0;
        for (int j = 0; j < (int)C; j++) {
            const float pj = __shfl(pf, j);
            rank += (pj > pf || (pj == pf && j < lane)) ? 1 : 0;
        }
        const bool add = cls && (nsyl > 1 || rank == 0);   // one syllable: only result_out[0] (the one-input quirk)
        if (add) {
            const double wc = (double)pf * w;
            // `if(!acc[label]) acc[label] = wconf; else acc[label] += wconf;` — a present 0 or NaN is overwritten
            acc_seg = (in_seg && acc_seg != 0.0 && acc_seg == acc_seg) ? acc_seg + wc : wc; in_seg = true;
            a.acc_all = (a.in_all && a.acc_all != 0.0 && a.acc_all == a.acc_all) ? a.acc_all + wc : wc;
            if (!a.in_all) { a.in_all = true; a.first = a.stamp + rank; }
        }
        a.stamp += C;
    }
    // segment label: keys of Label_conf_all in Object.keys order, the first whose segment sum exceeds the running maximum (from 0)
    const double v = (in_seg && acc_seg > 0.0) ? acc_seg : 0.0;
    const double mx = wave_max_d(v);
    const long long key = (kr >= 0) ? (long long)kr : ((1ll << 40) + a.first);
    const long long best = wave_min_ll((in_seg && a.in_all && v == mx && mx > 0.0) ? key : 0x7fffffffffffffffll);
    if (mx > 0.0) {
        const unsigned long long hit = __ballot(cls && in_seg && a.in_all && v == mx && key == best);
        label = (int)__ffsll(hit) - 1;
    } else label = -1;
    conf = mx / seg_weight;
}

__global__ void __launch_bounds__(256) fold_kernel(FoldParams p) {
    const int lane = threadIdx.x & 63;
    const uint32_t clip = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (clip >= p.n_clips) return;
    const uint32_t r0 = p.row_off[clip], r1 = p.row_off[clip + 1];
    const bool cls = (uint32_t)lane < p.C;
    const int kr = cls ? p.key_rank[lane] : -1;
    FoldAcc a{0.0, false, 0, 0};
    uint32_t ncb = 0;
    for (uint32_t r = r0; r < r1;) {
        const int si = p.meta[(size_t)r * 8 + 1];
        uint32_t e = r + 1;
        while (e < r1 && p.meta[(size_t)e * 8 + 1] == si) e++;
        int label; double conf;
        fold_callback(p.meta, p.prob, p.C, p.step_s, lane, cls, kr, r, e, a, label, conf);
        if (lane == 0) { p.t_label[r] = label; p.t_conf[r] = conf; p.t_n[r] = (int32_t)(e - r); p.t_local[r] = (int32_t)ncb; }
        for (uint32_t q = r + 1 + lane; q < e; q += 64) p.t_n[q] = 0;
        ncb++;
        r = e;
    }
    if (cls) p.clip_conf[(size_t)clip * p.C + lane] = a.acc_all;
    if (lane == 0) p.clip_cb[clip] = ncb;
}

// callbacks per clip -> offsets, then every callback's entry from the row it starts at; the count goes to the host's mapped word
__global__ void __launch_bounds__(1024) fold_compact_kernel(uint32_t n_clips, const uint32_t* row_off, const int32_t* meta, const uint32_t* clip_cb,
                                                            uint32_t* cb_off, const int32_t* t_label, const double* t_conf, const int32_t* t_n,
                                                            const int32_t* t_local, int32_t* cb, int32_t* cb_label, double* cb_conf, uint32_t* host) {
    __shared__ uint32_t s_part[1024];
    __shared__ uint32_t s_base;
    const int tid = threadIdx.x;
    if (tid == 0) s_base = 0;
    __syncthreads();
    for (uint32_t c0 = 0; c0 < n_clips; c0 += 1024) {
        const uint32_t c = c0 + tid;
        const uint32_t v = c < n_clips ? clip_cb[c] : 0u;
        s_part[tid] = v;
        __syncthreads();
        for (int o = 1; o < 1024; o <<= 1) {                       // inclusive scan (Hillis-Steele)
            const uint32_t t = tid >= o ? s_part[tid - o] : 0u;
            __syncthreads();
            s_part[tid] += t;
            __syncthreads();
        }
        if (c < n_clips) cb_off[c] = s_base + s_part[tid] - v;
        __syncthreads();
        if (tid == 1023) s_base += s_part[1023];
        __syncthreads();
    }
    const uint32_t n_rows = row_off[n_clips];
    __syncthreads();
    for (uint32_t r = tid; r < n_rows; r += 1024) {
        const int32_t nsyl = t_n[r];
        if (nsyl <= 0) continue;
        const int32_t clip = meta[(size_t)r * 8];
        const uint32_t k = cb_off[clip] + (uint32_t)t_local[r];
        cb[(size_t)k * 4 + 0] = clip; cb[(size_t)k * 4 + 1] = meta[(size_t)r * 8 + 1]; cb[(size_t)k * 4 + 2] = (int32_t)r; cb[(size_t)k * 4 + 3] = nsyl;
        cb_label[k] = t_label[r]; cb_conf[k] = t_conf[r];
    }
    if (tid == 0) host[0] = s_base;
}

// ---- K6b on a stream step: one wave per stream, classes on lanes.  The fold's state (Label_conf_all, key insertion stamps) lives in
// device memory from step to step, zeroed here when the step's control word has START (bit 0: the step's rows belong to the new launch).
// Callbacks are written straight to their place in the step's table: a stream's first callback index is the number of callback starts
// (a row whose stream or si differs from the row before) among the rows in front of it — a ballot over tens to hundreds of rows, instead
// of a scan kernel.  Probabilities, callbacks and the per-stream sums go to the mapped pinned buffers (rows / callbacks below `cap`).
struct StreamClsParams {
    uint32_t n, C, cap; int fold; double step_s;
    const int32_t* meta; const uint32_t* row_off; const float* prob; const int32_t* key_rank; const uint32_t* bits;
    double* acc_all; int32_t* in_all; long long* first; long long* stamp;          // [n][C], [n][C], [n][C], [n]
    int32_t* cb; int32_t* cb_label; double* cb_conf;                               // device: every callback of the step
    float* h_prob; int32_t* h_cb; int32_t* h_cb_label; double* h_cb_conf; double* h_conf; uint32_t* h_count;   // mapped pinned
};

__global__ void __launch_bounds__(256) stream_classes_kernel(StreamClsParams p) {
    const int lane = threadIdx.x & 63;
    const uint32_t s = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (s >= p.n) return;
    const uint32_t r0 = p.row_off[s], r1 = p.row_off[s + 1];
    const uint32_t pe = (r1 < p.cap ? r1 : p.cap) * p.C;
    for (uint32_t i = r0 * p.C + lane; i < pe; i += 64) p.h_prob[i] = p.prob[i];
    if (!p.fold) return;
    const bool cls = (uint32_t)lane < p.C;
    const int kr = cls ? p.key_rank[lane] : -1;
    const size_t sc = (size_t)s * p.C + lane;
    FoldAcc a{0.0, false, 0, 0};
    if (!(p.bits[s] & 1u)) {
        if (cls) { a.acc_all = p.acc_all[sc]; a.in_all = p.in_all[sc] != 0; a.first = p.first[sc]; }
        a.stamp = p.stamp[s];
    }
    uint32_t k = 0;
    for (uint32_t q0 = 0; q0 < r0; q0 += 64) {
        const uint32_t q = q0 + lane;
        const bool start = q < r0 && (q == 0 || p.meta[(size_t)q * 8] != p.meta[(size_t)(q - 1) * 8] || p.meta[(size_t)q * 8 + 1] != p.meta[(size_t)(q - 1) * 8 + 1]);
        k += (uint32_t)__popcll(__ballot(start));
    }
    for (uint32_t r = r0; r < r1;) {
        const int si = p.meta[(size_t)r * 8 + 1];
        uint32_t e = r + 1;
        while (e < r1 && p.meta[(size_t)e * 8 + 1] == si) e++;
        int label; double conf;
        fold_callback(p.meta, p.prob, p.C, p.step_s, lane, cls, kr, r, e, a, label, conf);
        if (lane == 0) {
            p.cb[(size_t)k * 4 + 0] = (int32_t)s; p.cb[(size_t)k * 4 + 1] = si; p.cb[(size_t)k * 4 + 2] = (int32_t)r; p.cb[(size_t)k * 4 + 3] = (int32_t)(e - r);
            p.cb_label[k] = label; p.cb_conf[k] = conf;
            if (k < p.cap) {
                p.h_cb[(size_t)k * 4 + 0] = (int32_t)s; p.h_cb[(size_t)k * 4 + 1] = si; p.h_cb[(size_t)k * 4 + 2] = (int32_t)r; p.h_cb[(size_t)k * 4 + 3] = (int32_t)(e - r);
                p.h_cb_label[k] = label; p.h_cb_conf[k] = conf;
            }
        }
        k++;
        r = e;
    }
    if (cls) { p.acc_all[sc] = a.acc_all; p.in_all[sc] = a.in_all ? 1 : 0; p.first[sc] = a.first; p.h_conf[sc] = a.acc_all; }
    if (lane == 0) { p.stamp[s] = a.stamp; if (s == p.n - 1) p.h_count[0] = k; }
}

}  // namespace

struct wsa_model {
    wsa_ctx* ctx = nullptr;
    int n_layers = 0, C = 0, S = 0, rb = 0;
    ClsLayer L[WSA_MODEL_MAX_LAYERS] = {};
    double *d_min = nullptr, *d_max = nullptr;
    int32_t* d_key_rank = nullptr;
    bool softmax = false;
    wsa::DevArena mem;
};

struct wsa_cls {
    int device = 0;
    uint32_t cap_rows = 0, cap_c = 0, n_clips = 0;
    float* d_prob = nullptr;
    int32_t *d_t_label = nullptr, *d_t_n = nullptr, *d_t_local = nullptr, *d_cb = nullptr, *d_cb_label = nullptr;
    double *d_t_conf = nullptr, *d_cb_conf = nullptr, *d_clip_conf = nullptr;
    uint32_t *d_clip_cb = nullptr, *d_cb_off = nullptr;
    uint32_t *h_count = nullptr, *h_count_dev = nullptr;     // pinned + mapped: callbacks of the last fold
    wsa::DevArena mem;
    const wsa_model* model = nullptr; int level = 0, n_classes = 0; uint32_t reruns = 0; bool done = false;
};

void wsa_cls_free(wsa_cls* c) {
    if (!c) return;
    (void)hipSetDevice(c->device);
    delete c;
}

namespace {

bool array_index_key(const char* s, int32_t* out) {       // "0", "17" (no sign, no leading zero) below 2^31: an array index for Object.keys
    if (!s || !*s) return false;
    if (s[0] == '0' && s[1]) return false;
    long long v = 0;
    for (const char* c = s; *c; c++) { if (*c < '0' || *c > '9') return false; v = v * 10 + (*c - '0'); if (v > 0x7fffffff) return false; }
    *out = (int32_t)v;
    return true;
}

// rows_cap sizes the grid (one workgroup per tile up to one per CU; the kernel strides over tiles beyond); rb = 16-row blocks per tile
// (the model's own choice for batches; streams pass 1).  A row's probabilities do not depend on the tile it lands in.
void launch_classify(const wsa_model* m, const double* feat, uint32_t n_rows, const uint32_t* d_n_rows, uint32_t rows_cap, float* prob, hipStream_t s, int rb = 0) {
    ClsParams p{};
    for (int l = 0; l < m->n_layers; l++) p.L[l] = m->L[l];
    p.n_layers = m->n_layers; p.C = m->C; p.S = m->S; p.in_min = m->d_min; p.in_max = m->d_max;
    p.feat = feat; p.n_rows = n_rows; p.d_n_rows = d_n_rows; p.prob = prob;
    if (rb <= 0 || rb > m->rb) rb = m->rb;
    const int TM = 16 * rb;
    int n_cu = m->ctx->n_cu > 0 ? m->ctx->n_cu : 256;
    const uint32_t tiles = (rows_cap + TM - 1) / TM;
    const uint32_t grid = tiles < (uint32_t)n_cu ? (tiles ? tiles : 1) : (uint32_t)n_cu;
    const size_t lds = (size_t)2 * TM * m->S * sizeof(float);
    if (rb == 4) hipLaunchKernelGGL(classify_kernel<4>, dim3(grid), dim3(CLS_THREADS), lds, s, p);
    else if (rb == 2) hipLaunchKernelGGL(classify_kernel<2>, dim3(grid), dim3(CLS_THREADS), lds, s, p);
    else hipLaunchKernelGGL(classify_kernel<1>, dim3(grid), dim3(CLS_THREADS), lds, s, p);
}

wsa_status enqueue_batch(wsa_batch* b, const wsa_batch_view& v, wsa_cls* c, const wsa_model* m, hipStream_t s) {
    wsa_ctx* ctx = v.ctx;
    launch_classify(m, v.d_feat, 0, v.d_row_off + v.n_clips, v.rows_cap, c->d_prob, s);
    HIP_TRY(ctx, hipGetLastError());
    if (v.level == 13) {
        FoldParams f{};
        f.n_clips = v.n_clips; f.C = (uint32_t)m->C; f.step_s = ctx->cfg.window_step / 1e3;
        f.meta = v.d_meta; f.row_off = v.d_row_off; f.prob = c->d_prob; f.key_rank = m->d_key_rank;
        f.t_label = c->d_t_label; f.t_conf = c->d_t_conf; f.t_n = c->d_t_n; f.t_local = c->d_t_local;
        f.clip_cb = c->d_clip_cb; f.clip_conf = c->d_clip_conf;
        if (v.n_clips) hipLaunchKernelGGL(fold_kernel, dim3((v.n_clips + 3) / 4), dim3(256), 0, s, f);
        hipLaunchKernelGGL(fold_compact_kernel, dim3(1), dim3(1024), 0, s, v.n_clips, v.d_row_off, v.d_meta, c->d_clip_cb, c->d_cb_off,
                           c->d_t_label, c->d_t_conf, c->d_t_n, c->d_t_local, c->d_cb, c->d_cb_label, c->d_cb_conf, c->h_count_dev);
        HIP_TRY(ctx, hipGetLastError());
    }
    (void)b;
    return WSA_OK;
}

// ---- streams (wsa_stream_set_model): K6 on every step's rows, the carried fold at level 13; everything allocated at attach time
wsa_status stream_cls_check(wsa_ctx* ctx, int level, const wsa_model* m) {
    if (level != 5 && level != 13)
        return fail(ctx, WSA_ERR_INVALID, "wsa_stream_set_model needs streams at output_level 5 (segment features) or 13 (syllable features), not " + std::to_string(level));
    if (m->ctx != ctx) return fail(ctx, WSA_ERR_INVALID, "the model was created on another context (or device) than the streams");
    if (level == 13 && !m->softmax) return fail(ctx, WSA_ERR_INVALID, "the level-13 fold needs class probabilities: the model's last layer is not softmax");
    return WSA_OK;
}

}  // namespace

struct wsa_scls {
    int device = 0;
    const wsa_model* model = nullptr;
    wsa_scls_view v{};
    uint32_t C = 0;
    float* d_prob = nullptr;
    double *d_acc = nullptr, *d_cb_conf = nullptr; int32_t *d_in = nullptr, *d_cb = nullptr, *d_cb_label = nullptr; long long *d_first = nullptr, *d_stamp = nullptr;
    wsa::DevArena mem;
    float *h_prob = nullptr, *h_prob_dev = nullptr;
    int32_t *h_cb = nullptr, *h_cb_dev = nullptr, *h_cb_label = nullptr, *h_cb_label_dev = nullptr;
    double *h_cb_conf = nullptr, *h_cb_conf_dev = nullptr, *h_conf = nullptr, *h_conf_dev = nullptr;
    uint32_t *h_count = nullptr, *h_count_dev = nullptr;
    std::vector<float> x_prob; std::vector<int32_t> x_cb, x_cb_label; std::vector<double> x_cb_conf;     // steps beyond the D2H window
};

void wsa_scls_free(wsa_scls* c) {
    if (!c) return;
    (void)hipSetDevice(c->device);
    delete c;
}

wsa_status wsa_scls_create(const wsa_scls_view& v, const wsa_model* m, wsa_scls** out) {
    wsa_ctx* ctx = v.ctx;
    *out = nullptr;
    const wsa_status chk = stream_cls_check(ctx, v.level, m);
    if (chk != WSA_OK) return chk;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    wsa_scls* c = new wsa_scls();
    c->device = ctx->device; c->model = m; c->v = v; c->C = (uint32_t)m->C;
    const size_t R = v.rows_cap ? v.rows_cap : 1, NC = (size_t)v.n_streams * c->C, W = v.d2h_rows ? v.d2h_rows : 1;
    wsa::DevArena& A = c->mem;
    bool ok = A.alloc(&c->d_prob, R * c->C);
    if (ok && v.level == 13) {
        ok = A.alloc(&c->d_acc, NC, true) && A.alloc(&c->d_in, NC, true) && A.alloc(&c->d_first, NC, true) && A.alloc(&c->d_stamp, (size_t)v.n_streams, true)
             && A.alloc(&c->d_cb, R * 4) && A.alloc(&c->d_cb_label, R) && A.alloc(&c->d_cb_conf, R)
             && A.pin(&c->h_cb, &c->h_cb_dev, W * 4) && A.pin(&c->h_cb_label, &c->h_cb_label_dev, W)
             && A.pin(&c->h_cb_conf, &c->h_cb_conf_dev, W) && A.pin(&c->h_conf, &c->h_conf_dev, NC) && A.pin(&c->h_count, &c->h_count_dev, 4);
    }
    ok = ok && A.pin(&c->h_prob, &c->h_prob_dev, W * c->C) && hipDeviceSynchronize() == hipSuccess;
    if (!ok) {
        const std::string msg = std::string("device allocation failed: ") + hipGetErrorString(hipGetLastError());
        wsa_scls_free(c);
        return fail(ctx, WSA_ERR_HIP, msg);
    }
    *out = c;
    return WSA_OK;
}

// K6 on the step's compacted rows (count on the device), then the stream fold / push: two kernel nodes of the captured step
wsa_status wsa_scls_enqueue(wsa_scls* c, hipStream_t s) {
    const wsa_scls_view& v = c->v;
    const wsa_model* m = c->model;
    // a step at config 5 has tens to hundreds of rows: tiles of 16 rows spread them over as many CUs as possible, and the grid covers the
    // D2H window (1024 rows) in one pass — a larger step strides over its tiles instead of launching rows_cap / 16 mostly idle workgroups
    launch_classify(m, v.d_feat, 0, v.d_totals, v.rows_cap < v.d2h_rows ? v.rows_cap : v.d2h_rows, c->d_prob, s, 1);
    HIP_TRY(v.ctx, hipGetLastError());
    StreamClsParams p{};
    p.n = v.n_streams; p.C = c->C; p.cap = v.d2h_rows; p.fold = v.level == 13 ? 1 : 0; p.step_s = v.ctx->cfg.window_step / 1e3;
    p.meta = v.d_meta; p.row_off = v.d_row_off; p.prob = c->d_prob; p.key_rank = m->d_key_rank; p.bits = v.d_bits;
    p.acc_all = c->d_acc; p.in_all = c->d_in; p.first = c->d_first; p.stamp = c->d_stamp;
    p.cb = c->d_cb; p.cb_label = c->d_cb_label; p.cb_conf = c->d_cb_conf;
    p.h_prob = c->h_prob_dev; p.h_cb = c->h_cb_dev; p.h_cb_label = c->h_cb_label_dev; p.h_cb_conf = c->h_cb_conf_dev; p.h_conf = c->h_conf_dev; p.h_count = c->h_count_dev;
    hipLaunchKernelGGL(stream_classes_kernel, dim3((v.n_streams + 3) / 4), dim3(256), 0, s, p);
    HIP_TRY(v.ctx, hipGetLastError());
    return WSA_OK;
}

// after the step has completed: the tables of `rows` rows; a step beyond the D2H window is fetched from the device here
wsa_status wsa_scls_result(wsa_scls* c, uint32_t rows, wsa_stream_class_result* o) {
    const wsa_scls_view& v = c->v;
    wsa_ctx* ctx = v.ctx;
    const bool fold = v.level == 13;
    const uint32_t ncb = fold ? ((const volatile uint32_t*)c->h_count)[0] : 0u;
    o->n_rows = rows; o->n_classes = c->C; o->n_callbacks = ncb; o->n_streams = v.n_streams;
    o->prob = c->h_prob;
    o->cb = fold ? c->h_cb : nullptr; o->cb_label = fold ? c->h_cb_label : nullptr; o->cb_conf = fold ? c->h_cb_conf : nullptr;
    o->stream_conf = fold ? c->h_conf : nullptr;
    if (rows > v.d2h_rows) {
        HIP_TRY(ctx, hipSetDevice(ctx->device));
        c->x_prob.resize((size_t)rows * c->C);
        HIP_TRY(ctx, hipMemcpy(c->x_prob.data(), c->d_prob, c->x_prob.size() * sizeof(float), hipMemcpyDeviceToHost));
        o->prob = c->x_prob.data();
        if (fold) {
            c->x_cb.resize((size_t)ncb * 4 + 4); c->x_cb_label.resize((size_t)ncb + 1); c->x_cb_conf.resize((size_t)ncb + 1);
            if (ncb) {
                HIP_TRY(ctx, hipMemcpy(c->x_cb.data(), c->d_cb, (size_t)ncb * 4 * sizeof(int32_t), hipMemcpyDeviceToHost));
                HIP_TRY(ctx, hipMemcpy(c->x_cb_label.data(), c->d_cb_label, (size_t)ncb * sizeof(int32_t), hipMemcpyDeviceToHost));
                HIP_TRY(ctx, hipMemcpy(c->x_cb_conf.data(), c->d_cb_conf, (size_t)ncb * sizeof(double), hipMemcpyDeviceToHost));
            }
            o->cb = c->x_cb.data(); o->cb_label = c->x_cb_label.data(); o->cb_conf = c->x_cb_conf.data();
        }
    }
    return WSA_OK;
}

extern "C" {

wsa_status wsa_model_create(wsa_ctx* ctx, const wsa_model_desc* d, wsa_model** out) {
    if (!ctx || !d || !out) return fail(ctx, WSA_ERR_INVALID, "null argument");
    *out = nullptr;
    const int nl = d->n_layers;
    if (nl < 1 || nl > WSA_MODEL_MAX_LAYERS) return fail(ctx, WSA_ERR_INVALID, "a model has 1 .. 8 Dense layers, got " + std::to_string(nl));
    if (!d->units || !d->activation || !d->kernel || !d->bias) return fail(ctx, WSA_ERR_INVALID, "null units / activation / kernel / bias array");
    if (d->units[0] != WSA_NFEAT) return fail(ctx, WSA_ERR_INVALID, "the model takes " + std::to_string(d->units[0]) + " inputs; the feature rows have 53");
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
    for (int k = 0; k < WSA_NFEAT; k++)
        if (!std::isfinite(d->in_min[k]) || !std::isfinite(d->in_max[k])) return fail(ctx, WSA_ERR_INVALID, "non-finite in_min / in_max of input " + std::to_string(k));
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    wsa_model* m = new wsa_model();
    m->ctx = ctx; m->n_layers = nl; m->C = d->units[nl]; m->softmax = d->activation[nl - 1] == WSA_ACT_SOFTMAX;
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
    std::vector<int32_t> kr(m->C, -1);
    if (d->labels) for (int c = 0; c < m->C; c++) { int32_t v; if (array_index_key(d->labels[c], &v)) kr[c] = v; }
    ok = ok && m->mem.alloc(&m->d_min, WSA_NFEAT) && m->mem.alloc(&m->d_max, WSA_NFEAT) && m->mem.upload(&m->d_key_rank, kr)
         && hipMemcpy(m->d_min, d->in_min, WSA_NFEAT * sizeof(double), hipMemcpyHostToDevice) == hipSuccess
         && hipMemcpy(m->d_max, d->in_max, WSA_NFEAT * sizeof(double), hipMemcpyHostToDevice) == hipSuccess;
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

wsa_status wsa_classify_rows(const wsa_model* m, const double* d_feat, uint32_t n_rows, float* d_prob, void* stream) {
    if (!m) return WSA_ERR_INVALID;
    wsa_ctx* ctx = m->ctx;
    if (n_rows && (!d_feat || !d_prob)) return fail(ctx, WSA_ERR_INVALID, "null feature / probability pointer");
    if (!n_rows) return WSA_OK;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    launch_classify(m, d_feat, n_rows, nullptr, n_rows, d_prob, reinterpret_cast<hipStream_t>(stream));
    HIP_TRY(ctx, hipGetLastError());
    return WSA_OK;
}

wsa_status wsa_batch_classify(wsa_batch* b, const wsa_model* m, void* stream) {
    if (!b || !m) return WSA_ERR_INVALID;
    wsa_batch_view v;
    wsa_batch_view_internal(b, &v);
    wsa_ctx* ctx = v.ctx;
    if (v.level != 5 && v.level != 13)
        return fail(ctx, WSA_ERR_INVALID, "wsa_batch_classify needs a batch at output_level 5 (segment features) or 13 (syllable features), not " + std::to_string(v.level));
    if (m->ctx != ctx) return fail(ctx, WSA_ERR_INVALID, "the model was created on another context (or device) than the batch");
    if (v.level == 13 && !m->softmax) return fail(ctx, WSA_ERR_INVALID, "the level-13 fold needs class probabilities: the model's last layer is not softmax");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    wsa_cls*& c = *v.cls;
    if (!c || c->cap_c < (uint32_t)m->C) {        // first call (or a model of more classes): the only allocation of this path
        wsa_cls* n = new wsa_cls();
        n->device = ctx->device; n->cap_rows = v.rows_cap; n->cap_c = (uint32_t)m->C; n->n_clips = v.n_clips;
        const size_t R = v.rows_cap ? v.rows_cap : 1;
        wsa::DevArena& A = n->mem;
        bool ok = A.alloc(&n->d_prob, R * m->C) && A.alloc(&n->d_t_label, R) && A.alloc(&n->d_t_conf, R)
                  && A.alloc(&n->d_t_n, R) && A.alloc(&n->d_t_local, R) && A.alloc(&n->d_cb, R * 4)
                  && A.alloc(&n->d_cb_label, R) && A.alloc(&n->d_cb_conf, R)
                  && A.alloc(&n->d_clip_conf, (size_t)v.n_clips * m->C) && A.alloc(&n->d_clip_cb, (size_t)v.n_clips)
                  && A.alloc(&n->d_cb_off, (size_t)v.n_clips);
        ok = ok && A.pin(&n->h_count, &n->h_count_dev, 4);
        if (!ok) {
            const std::string msg = std::string("device allocation failed: ") + hipGetErrorString(hipGetLastError());
            wsa_cls_free(n);
            return fail(ctx, WSA_ERR_HIP, msg);
        }
        wsa_cls_free(c);
        c = n;
    }
    c->model = m; c->level = v.level; c->n_classes = m->C; c->reruns = v.reruns; c->done = true;
    return enqueue_batch(b, v, c, m, reinterpret_cast<hipStream_t>(stream));
}

wsa_status wsa_batch_class_result(wsa_batch* b, void* stream, wsa_class_result* out) {
    if (!b || !out) return WSA_ERR_INVALID;
    wsa_batch_view v;
    wsa_batch_view_internal(b, &v);
    wsa_ctx* ctx = v.ctx;
    wsa_cls* c = *v.cls;
    if (!c || !c->done) return fail(ctx, WSA_ERR_INVALID, "no wsa_batch_classify on this batch yet");
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    wsa_status st = wsa_batch_fetch_internal(b, s);
    if (st != WSA_OK) return st;
    wsa_batch_view_internal(b, &v);
    if (v.reruns != c->reruns) {                  // the back end was rerun with the full tracker table: classify its rows again
        c->reruns = v.reruns;
        st = enqueue_batch(b, v, c, c->model, s);
        if (st != WSA_OK) return st;
    }
    HIP_TRY(ctx, hipStreamSynchronize(s));
    wsa_device_result r;
    st = wsa_batch_result(b, stream, &r);
    if (st != WSA_OK) return st;
    out->n_rows = r.n_rows; out->n_classes = (uint32_t)c->n_classes; out->n_clips = v.n_clips;
    out->d_prob = c->d_prob;
    const bool fold = c->level == 13;
    out->n_callbacks = fold ? ((const volatile uint32_t*)c->h_count)[0] : 0u;
    out->d_cb = fold ? c->d_cb : nullptr; out->d_cb_label = fold ? c->d_cb_label : nullptr;
    out->d_cb_conf = fold ? c->d_cb_conf : nullptr; out->d_clip_conf = fold ? c->d_clip_conf : nullptr;
    return WSA_OK;
}

wsa_status wsa_batch_copy_classes(wsa_batch* b, void* stream, float* prob, uint32_t rows_cap, int32_t* cb, int32_t* cb_label, double* cb_conf,
                                  uint32_t cb_cap, double* clip_conf) {
    if (!b) return WSA_ERR_INVALID;
    wsa_class_result r;
    const wsa_status st = wsa_batch_class_result(b, stream, &r);
    if (st != WSA_OK) return st;
    wsa_batch_view v;
    wsa_batch_view_internal(b, &v);
    wsa_ctx* ctx = v.ctx;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (prob && rows_cap < r.n_rows) return fail(ctx, WSA_ERR_INVALID, "probability buffer too small");
    if ((cb || cb_label || cb_conf) && cb_cap < r.n_callbacks) return fail(ctx, WSA_ERR_INVALID, "callback buffer too small");
    if (prob && r.n_rows) HIP_TRY(ctx, hipMemcpyAsync(prob, r.d_prob, (size_t)r.n_rows * r.n_classes * sizeof(float), hipMemcpyDefault, s));
    if (r.n_callbacks) {
        if (cb) HIP_TRY(ctx, hipMemcpyAsync(cb, r.d_cb, (size_t)r.n_callbacks * 4 * sizeof(int32_t), hipMemcpyDefault, s));
        if (cb_label) HIP_TRY(ctx, hipMemcpyAsync(cb_label, r.d_cb_label, (size_t)r.n_callbacks * sizeof(int32_t), hipMemcpyDefault, s));
        if (cb_conf) HIP_TRY(ctx, hipMemcpyAsync(cb_conf, r.d_cb_conf, (size_t)r.n_callbacks * sizeof(double), hipMemcpyDefault, s));
    }
    if (clip_conf && r.d_clip_conf && r.n_clips) HIP_TRY(ctx, hipMemcpyAsync(clip_conf, r.d_clip_conf, (size_t)r.n_clips * r.n_classes * sizeof(double), hipMemcpyDefault, s));
    HIP_TRY(ctx, hipStreamSynchronize(s));
    return WSA_OK;
}

}  // extern "C"
