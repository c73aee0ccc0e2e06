// classify.hip — K6 (the app's dense classifier over feature rows, f32 MFMA) and K6b (the app's per-callback fold, exact double),
// and their part of the C ABI (include/wsa.h "Syllable classification").
//
// Stands in for the reference APPLICATION's prediction path: ml5 classifyMultiple (tfjs Dense layers, float32) over the syllables of a
// level-13 callback, then src/prediction.js:86-169 (weights sqrt(duration), per-label sums, segment label, per-launch accumulator).
#include <atomic>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>
#include "host_plan.hpp"

using wsa_api::fail;

namespace {

constexpr int CLS_THREADS = 512;                 // 8 waves: 2 per SIMD
constexpr int CLS_LDS_BUDGET = 160 * 1024;
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
};

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
template <int RB>
__device__ __forceinline__ void classify_tile(const ClsParams& p, float* s_act, uint32_t tile, uint32_t n) {
    constexpr int TM = 16 * RB;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nwaves = CLS_THREADS / 64;
    const int S = p.S;
    {
        const uint32_t row0 = tile * TM;
        float* in = s_act;
        float* out = s_act + TM * S;
        const int p0 = p.L[0].kp;
        for (int idx = tid; idx < TM * p0; idx += CLS_THREADS) {
            const int r = idx / p0, k = idx - r * p0;
            float v = 0.f;
            if (row0 + r < n && k < p.nin) {                                   // ml5 normalizeValue in double, then the f32 tensor
                const double x = p.feat[(size_t)(row0 + r) * p.stride + k];
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
            if (p.nan_slot >= 0 && p.feat[(size_t)(row0 + r) * p.stride + p.nan_slot] != 0.0) {   // no coefficients: nothing to predict from
                if (p.value) p.value[row0 + r] = __longlong_as_double(0x7ff8000000000000ll);
                else for (int c = 0; c < p.C; c++) p.prob[(size_t)(row0 + r) * p.C + c] = __int_as_float(0x7fc00000);
                continue;
            }
            if (p.value) {                                                  // K6's regression epilogue: the one unit's output, un-normalised
                p.value[row0 + r] = unnormalise_value(x[0], p.out_min, p.out_span);
                continue;
            }
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
struct ClsGroupEntry { ClsParams p; int rb; };

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
                                              uint32_t r, uint32_t e, FoldAcc& a, int& label, double& conf, double& seg_max) {
    const uint32_t nsyl = e - r;
    double seg_weight = 0.0;                 // sum of parseFloat(seg_time[ph][1]) (ref prediction.js:55)
    for (uint32_t q = r; q < e; q++) seg_weight += fixed3((double)(meta[(size_t)q * 8 + 3] + 1) * step_s);
    label = -2; conf = 0.0; seg_max = 0.0;
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
    seg_max = mx;                            // DB_entropies_seg of this model DB (ref prediction.js:154)
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
        int label; double conf, seg_max;
        fold_callback(p.meta, p.prob, p.C, p.step_s, lane, cls, kr, r, e, a, label, conf, seg_max);
        if (lane == 0) { p.t_label[r] = label; p.t_conf[r] = conf; p.t_n[r] = (int32_t)(e - r); p.t_local[r] = (int32_t)ncb; }
        for (uint32_t q = r + 1 + lane; q < e; q += 64) p.t_n[q] = 0;
        ncb++;
        r = e;
    }
    if (cls) p.clip_conf[(size_t)clip * p.C + lane] = a.acc_all;
    if (lane == 0) p.clip_cb[clip] = ncb;
}

// callbacks per clip -> offsets (one workgroup of 1024 threads; returns the total to every thread)
__device__ __forceinline__ uint32_t compact_offsets(uint32_t n_clips, const uint32_t* clip_cb, uint32_t* cb_off, uint32_t* s_part, uint32_t* s_base) {
    const int tid = threadIdx.x;
    if (tid == 0) *s_base = 0;
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
        if (c < n_clips) cb_off[c] = *s_base + s_part[tid] - v;
        __syncthreads();
        if (tid == 1023) *s_base += s_part[1023];
        __syncthreads();
    }
    return *s_base;
}

// the offsets, then every callback's entry from the row it starts at; the count goes to the host's mapped word
__global__ void __launch_bounds__(1024) fold_compact_kernel(uint32_t n_clips, const uint32_t* row_off, const int32_t* meta, const uint32_t* clip_cb,
                                                            uint32_t* cb_off, const int32_t* t_label, const double* t_conf, const int32_t* t_n,
                                                            const int32_t* t_local, int32_t* cb, int32_t* cb_label, double* cb_conf, uint32_t* host) {
    __shared__ uint32_t s_part[1024];
    __shared__ uint32_t s_base;
    const int tid = threadIdx.x;
    const uint32_t n_cb = compact_offsets(n_clips, clip_cb, cb_off, s_part, &s_base);
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
    if (tid == 0) host[0] = n_cb;
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
        int label; double conf, seg_max;
        fold_callback(p.meta, p.prob, p.C, p.step_s, lane, cls, kr, r, e, a, label, conf, seg_max);
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


// ---- K6b-e: the fold for every member of an ensemble (ref prediction.js:47-169 with several model DBs in available_DBs), one wave per
// (clip, member) or (stream, member).  Besides what K6b writes, a callback leaves what seg_confidence_sort derives from the member's tables:
// DB_entropies_seg (the segment maximum), DB_entropies_all (the maximum of Label_conf_all, strict > from 0 in key order — a maximum does not
// depend on the order) and the sum plot_prediction_meters forms over Label_conf_all in Object.keys order (ref prediction.js:182-184).
struct FoldMember {
    uint32_t C; const float* prob; const int32_t* key_rank;
    int32_t* t_label; double* t_conf; double* t_all_max;                                     // per row: the callback that starts there
    double* t_seg; double* t_all_sum;                                                        // (stream steps only: batches keep these two in LDS)
    double* clip_conf;                                                                       // [n_clips][C]
    int32_t* cb_label; double* cb_conf; double* cb_all_max;                                  // [n_callbacks], written by the compaction
};
struct EnsTables {
    int32_t* cb; int32_t* cb_db; int32_t* cb_top_label; double* cb_top_conf; int32_t* cb_min_db; double* cb_entropy; int32_t* clip_min_db;
};
struct FoldGroupParams {
    uint32_t n_clips, n_members; double step_s;
    const int32_t* meta; const uint32_t* row_off; const FoldMember* tab;
    int32_t* t_n; int32_t* t_local; uint32_t* clip_cb;                                       // shared by the members
    EnsTables t;                                                                             // the decision per row (callback starts); cb unused
};

__device__ __forceinline__ void all_max_and_sum(const FoldAcc& a, uint32_t C, int lane, bool cls, int kr, double& all_max, double& all_sum) {
    const bool in = cls && a.in_all;
    all_max = wave_max_d((in && a.acc_all > 0.0) ? a.acc_all : 0.0);
    const long long key = (kr >= 0) ? (long long)kr : ((1ll << 40) + a.first);
    int rank = 0;                                                  // place among the keys in Object.keys order
    for (int j = 0; j < (int)C; j++) {
        const long long kj = __shfl(key, j);
        const int inj = __shfl(in ? 1 : 0, j);
        rank += (inj && (kj < key || (kj == key && j < lane))) ? 1 : 0;
    }
    const int cnt = (int)__popcll(__ballot(in));
    double s = 0.0;                                                // `let all_class_sum = 0; ... +=` in that order
    for (int i = 0; i < cnt; i++) {
        const int src = (int)__ffsll(__ballot(in && rank == i)) - 1;
        s += __shfl(a.acc_all, src);
    }
    all_sum = s;
}

// The decision of seg_confidence_sort (ref prediction.js:127-169) for one callback, from the members' figures for it: the winner is the
// first member whose segment maximum exceeds the running one (from 0).  -1: no member has a sum above 0.
__device__ __forceinline__ void ensemble_winner(const double* seg, const int* label, const double* conf, uint32_t n_members, int& db, int& top_label, double& top_conf) {
    double best = 0.0;
    db = -1; top_label = -1; top_conf = 0.0;
    for (uint32_t d = 0; d < n_members; d++)
        if (seg[d] > best) { best = seg[d]; db = (int)d; top_label = label[d]; top_conf = conf[d]; }   // max_conf_db_seg / seg_weight: the member's own quotient
}

// min_entropy_db after one callback (ref prediction.js:161-165): updated only where a member's DB_entropies_all exceeds max_inv_entropy,
// which runs across the launch's callbacks; then the readout of plot_prediction_meters (ref prediction.js:207), NaN while there is no DB
__device__ __forceinline__ double ensemble_min_db(const double* all_max, const double* all_sum, uint32_t n_members, bool skipped, double& max_inv, int& min_db) {
    if (!skipped)
        for (uint32_t d = 0; d < n_members; d++)
            if (all_max[d] > max_inv) { max_inv = all_max[d]; min_db = (int)d; }
    if (min_db < 0) return __longlong_as_double(0x7ff8000000000000ll);
    return 1.0 - all_max[min_db] / all_sum[min_db];
}

// the same two for a stream step, whose members' figures sit in their step tables at callback index `at`
__device__ __forceinline__ void ensemble_winner_at(const FoldMember* tab, uint32_t n_members, size_t at, int& db, int& top_label, double& top_conf) {
    double best = 0.0;
    db = -1; top_label = -1; top_conf = 0.0;
    for (uint32_t d = 0; d < n_members; d++) {
        const double seg = tab[d].t_seg[at];
        if (seg > best) { best = seg; db = (int)d; top_label = tab[d].t_label[at]; top_conf = tab[d].t_conf[at]; }
    }
}
__device__ __forceinline__ double ensemble_min_db_at(const FoldMember* tab, uint32_t n_members, size_t at, bool skipped, double& max_inv, int& min_db) {
    if (!skipped)
        for (uint32_t d = 0; d < n_members; d++) {
            const double am = tab[d].t_all_max[at];
            if (am > max_inv) { max_inv = am; min_db = (int)d; }
        }
    if (min_db < 0) return __longlong_as_double(0x7ff8000000000000ll);
    return 1.0 - tab[min_db].t_all_max[at] / tab[min_db].t_all_sum[at];
}

// One workgroup per clip, one wave per member: the waves walk the clip's callbacks in step (the rows and so the trip counts are the same
// for all of them), leave each callback's three figures in LDS, and after one barrier every thread holds the decision — so the running
// max_inv_entropy / min_entropy_db, a chain over the clip's callbacks, costs nothing beyond the fold's own walk.  Two LDS sets by callback
// parity make one barrier per callback enough.
__global__ void __launch_bounds__(64 * WSA_ENSEMBLE_MAX) fold_group_kernel(FoldGroupParams p) {
    __shared__ double s_seg[2][WSA_ENSEMBLE_MAX], s_max[2][WSA_ENSEMBLE_MAX], s_sum[2][WSA_ENSEMBLE_MAX], s_conf[2][WSA_ENSEMBLE_MAX];
    __shared__ int s_label[2][WSA_ENSEMBLE_MAX];
    const int lane = threadIdx.x & 63;
    const uint32_t clip = blockIdx.x, d = threadIdx.x >> 6;
    const FoldMember m = p.tab[d];
    const uint32_t r0 = p.row_off[clip], r1 = p.row_off[clip + 1];
    const bool cls = (uint32_t)lane < m.C;
    const int kr = cls ? m.key_rank[lane] : -1;
    FoldAcc a{0.0, false, 0, 0};
    uint32_t ncb = 0;
    double max_inv = 0.0; int min_db = -1;
    for (uint32_t r = r0; r < r1;) {
        const int si = p.meta[(size_t)r * 8 + 1];
        uint32_t e = r + 1;
        while (e < r1 && p.meta[(size_t)e * 8 + 1] == si) e++;
        int label; double conf, seg_max, all_max, all_sum;
        fold_callback(p.meta, m.prob, m.C, p.step_s, lane, cls, kr, r, e, a, label, conf, seg_max);
        all_max_and_sum(a, m.C, lane, cls, kr, all_max, all_sum);
        const int pb = (int)(ncb & 1u);
        if (lane == 0) {
            m.t_label[r] = label; m.t_conf[r] = conf; m.t_all_max[r] = all_max;
            s_seg[pb][d] = seg_max; s_max[pb][d] = all_max; s_sum[pb][d] = all_sum; s_conf[pb][d] = conf; s_label[pb][d] = label;
        }
        __syncthreads();
        int db, top_label; double top_conf;
        ensemble_winner(s_seg[pb], s_label[pb], s_conf[pb], p.n_members, db, top_label, top_conf);
        const bool skipped = label == -2;                       // the durations, not the model, decide it: the same for every member
        const double ent = ensemble_min_db(s_max[pb], s_sum[pb], p.n_members, skipped, max_inv, min_db);
        if (threadIdx.x == 0) {
            p.t_n[r] = (int32_t)(e - r); p.t_local[r] = (int32_t)ncb;
            p.t.cb_db[r] = skipped ? -2 : db; p.t.cb_top_label[r] = top_label; p.t.cb_top_conf[r] = top_conf; p.t.cb_min_db[r] = min_db; p.t.cb_entropy[r] = ent;
        }
        for (uint32_t q = r + 1 + threadIdx.x; q < e; q += blockDim.x) p.t_n[q] = 0;
        ncb++;
        r = e;
    }
    if (cls) m.clip_conf[(size_t)clip * m.C + lane] = a.acc_all;
    if (threadIdx.x == 0) { p.clip_cb[clip] = ncb; p.t.clip_min_db[clip] = min_db; }
}

// the compaction of K6b for an ensemble: every callback's per-member entries and decision from the row it starts at
__global__ void __launch_bounds__(1024) fold_compact_group_kernel(uint32_t n_clips, uint32_t n_members, const uint32_t* row_off, const int32_t* meta,
                                                                  const uint32_t* clip_cb, uint32_t* cb_off, const int32_t* t_n, const int32_t* t_local,
                                                                  const FoldMember* tab, EnsTables t, EnsTables o, uint32_t* host) {
    __shared__ uint32_t s_part[1024];
    __shared__ uint32_t s_base;
    const int tid = threadIdx.x;
    const uint32_t n_cb = compact_offsets(n_clips, clip_cb, cb_off, s_part, &s_base);
    const uint32_t n_rows = row_off[n_clips];
    __syncthreads();
    for (uint32_t r = tid; r < n_rows; r += 1024) {
        const int32_t nsyl = t_n[r];
        if (nsyl <= 0) continue;
        const int32_t clip = meta[(size_t)r * 8];
        const uint32_t k = cb_off[clip] + (uint32_t)t_local[r];
        o.cb[(size_t)k * 4 + 0] = clip; o.cb[(size_t)k * 4 + 1] = meta[(size_t)r * 8 + 1]; o.cb[(size_t)k * 4 + 2] = (int32_t)r; o.cb[(size_t)k * 4 + 3] = nsyl;
        for (uint32_t d = 0; d < n_members; d++) {
            const FoldMember& m = tab[d];
            m.cb_label[k] = m.t_label[r]; m.cb_conf[k] = m.t_conf[r]; m.cb_all_max[k] = m.t_all_max[r];
        }
        o.cb_db[k] = t.cb_db[r]; o.cb_top_label[k] = t.cb_top_label[r]; o.cb_top_conf[k] = t.cb_top_conf[r];
        o.cb_min_db[k] = t.cb_min_db[r]; o.cb_entropy[k] = t.cb_entropy[r];
    }
    if (tid == 0) host[0] = n_cb;
}

// ---- K6b-e on a stream step: one wave per (stream, member) folds with that pair's carried accumulator and writes the member's entries
// straight to the step's tables (the index as in stream_classes_kernel); then one wave per stream decides — winners with callbacks on
// lanes, min_entropy_db by lane 0 in callback order with the stream's running max_inv_entropy / min_entropy_db carried on the device and
// reset by START (ref reset_predictions(true), prediction.js:24-36; the device also forgets min_entropy_db, see wsa.h).  In a step the
// members' tables (FoldMember t_*) are indexed by callback, not by row.
struct StreamMember {
    double* acc_all; int32_t* in_all; long long* first; long long* stamp;                   // carried: [n][C], [n][C], [n][C], [n]
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

__device__ __forceinline__ bool callback_start(const int32_t* meta, uint32_t q) {
    return q == 0 || meta[(size_t)q * 8] != meta[(size_t)(q - 1) * 8] || meta[(size_t)q * 8 + 1] != meta[(size_t)(q - 1) * 8 + 1];
}
__device__ __forceinline__ uint32_t callback_starts(const int32_t* meta, uint32_t a, uint32_t b, int lane) {   // among rows a .. b - 1
    uint32_t k = 0;
    for (uint32_t q0 = a; q0 < b; q0 += 64) {
        const uint32_t q = q0 + lane;
        k += (uint32_t)__popcll(__ballot(q < b && callback_start(meta, q)));
    }
    return k;
}

__global__ void __launch_bounds__(256) stream_fold_group_kernel(StreamEnsParams p) {
    const int lane = threadIdx.x & 63;
    const uint32_t w = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (w >= p.n * p.n_members) return;
    const uint32_t s = w / p.n_members, d = w - s * p.n_members;
    const FoldMember m = p.tab[d];
    const StreamMember sm = p.stab[d];
    const uint32_t r0 = p.row_off[s], r1 = p.row_off[s + 1];
    const uint32_t pe = (r1 < p.cap ? r1 : p.cap) * m.C;
    for (uint32_t i = r0 * m.C + lane; i < pe; i += 64) sm.h_prob[i] = m.prob[i];
    if (!p.fold) return;
    const bool cls = (uint32_t)lane < m.C;
    const int kr = cls ? m.key_rank[lane] : -1;
    const size_t sc = (size_t)s * m.C + lane;
    FoldAcc a{0.0, false, 0, 0};
    if (!(p.bits[s] & 1u)) {
        if (cls) { a.acc_all = sm.acc_all[sc]; a.in_all = sm.in_all[sc] != 0; a.first = sm.first[sc]; }
        a.stamp = sm.stamp[s];
    }
    uint32_t k = callback_starts(p.meta, 0, r0, lane);
    for (uint32_t r = r0; r < r1;) {
        const int si = p.meta[(size_t)r * 8 + 1];
        uint32_t e = r + 1;
        while (e < r1 && p.meta[(size_t)e * 8 + 1] == si) e++;
        int label; double conf, seg_max, all_max, all_sum;
        fold_callback(p.meta, m.prob, m.C, p.step_s, lane, cls, kr, r, e, a, label, conf, seg_max);
        all_max_and_sum(a, m.C, lane, cls, kr, all_max, all_sum);
        if (lane == 0) {
            m.t_label[k] = label; m.t_conf[k] = conf; m.t_seg[k] = seg_max; m.t_all_max[k] = all_max; m.t_all_sum[k] = all_sum;
            if (k < p.cap) { sm.h_cb_label[k] = label; sm.h_cb_conf[k] = conf; sm.h_cb_all_max[k] = all_max; }
            if (d == 0) {
                p.o.cb[(size_t)k * 4 + 0] = (int32_t)s; p.o.cb[(size_t)k * 4 + 1] = si; p.o.cb[(size_t)k * 4 + 2] = (int32_t)r; p.o.cb[(size_t)k * 4 + 3] = (int32_t)(e - r);
                if (k < p.cap) {
                    p.h.cb[(size_t)k * 4 + 0] = (int32_t)s; p.h.cb[(size_t)k * 4 + 1] = si; p.h.cb[(size_t)k * 4 + 2] = (int32_t)r; p.h.cb[(size_t)k * 4 + 3] = (int32_t)(e - r);
                }
            }
        }
        k++;
        r = e;
    }
    if (cls) { sm.acc_all[sc] = a.acc_all; sm.in_all[sc] = a.in_all ? 1 : 0; sm.first[sc] = a.first; sm.h_conf[sc] = a.acc_all; }
    if (lane == 0) { sm.stamp[s] = a.stamp; if (d == 0 && s == p.n - 1) p.h_count[0] = k; }
}

__global__ void __launch_bounds__(256) stream_decide_kernel(StreamEnsParams p) {
    const int lane = threadIdx.x & 63;
    const uint32_t s = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (s >= p.n) return;
    const uint32_t r0 = p.row_off[s], r1 = p.row_off[s + 1];
    const uint32_t k0 = callback_starts(p.meta, 0, r0, lane), k1 = k0 + callback_starts(p.meta, r0, r1, lane);
    for (uint32_t k = k0 + lane; k < k1; k += 64) {
        int db, label; double conf;
        ensemble_winner_at(p.tab, p.n_members, k, db, label, conf);
        if (p.tab[0].t_label[k] == -2) db = -2;
        p.o.cb_db[k] = db; p.o.cb_top_label[k] = label; p.o.cb_top_conf[k] = conf;
        if (k < p.cap) { p.h.cb_db[k] = db; p.h.cb_top_label[k] = label; p.h.cb_top_conf[k] = conf; }
    }
    if (lane != 0) return;
    double max_inv = 0.0; int min_db = -1;
    if (!(p.bits[s] & 1u)) { max_inv = p.max_inv[s]; min_db = p.min_db[s]; }
    for (uint32_t k = k0; k < k1; k++) {
        const double ent = ensemble_min_db_at(p.tab, p.n_members, k, p.tab[0].t_label[k] == -2, max_inv, min_db);
        p.o.cb_min_db[k] = min_db; p.o.cb_entropy[k] = ent;
        if (k < p.cap) { p.h.cb_min_db[k] = min_db; p.h.cb_entropy[k] = ent; }
    }
    p.max_inv[s] = max_inv; p.min_db[s] = min_db;
    p.h.clip_min_db[s] = min_db;
}

}  // namespace

struct wsa_model {
    wsa_ctx* ctx = nullptr;
    int n_layers = 0, C = 0, S = 0, rb = 0, nin = 0;      // nin = units[0], the row width of the level the model was trained at
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
    double* d_value = nullptr; double out_min = 0.0, out_span = 0.0;      // wsa_batch_regress: one value per row
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

// the ensemble tables of one batch, built for one ensemble
struct wsa_ecls {
    int device = 0;
    const wsa_ensemble* ens = nullptr; uint64_t serial = 0;
    uint32_t n = 0, n_clips = 0, reruns = 0; int level = 0;
    uint32_t C[WSA_ENSEMBLE_MAX] = {};
    float* d_prob[WSA_ENSEMBLE_MAX] = {};
    FoldMember fm[WSA_ENSEMBLE_MAX] = {};
    ClsGroupEntry* d_ctab = nullptr; FoldMember* d_ftab = nullptr;
    int32_t *d_t_n = nullptr, *d_t_local = nullptr; uint32_t *d_clip_cb = nullptr, *d_cb_off = nullptr;
    size_t lds = 0;                          // K6e's dynamic LDS (kept here: the ensemble object is only compared, never read, after the tables exist)
    EnsTables t{}, o{};                      // the decision per row (written by the fold) / per callback (the compaction)
    uint32_t *h_count = nullptr, *h_count_dev = nullptr;
    uint32_t grid = 1;
    wsa::DevArena mem;
};

void wsa_cls_free(wsa_cls* c) {
    if (!c) return;
    (void)hipSetDevice(c->device);
    delete c;
}

void wsa_ecls_free(wsa_ecls* c) {
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

ClsParams cls_params(const wsa_model* m, const double* feat, uint32_t n_rows, const uint32_t* d_n_rows, float* prob) {
    ClsParams p{};
    for (int l = 0; l < m->n_layers; l++) p.L[l] = m->L[l];
    p.n_layers = m->n_layers; p.C = m->C; p.S = m->S; p.in_min = m->d_min; p.in_max = m->d_max;
    p.feat = feat; p.n_rows = n_rows; p.d_n_rows = d_n_rows; p.prob = prob;
    p.nin = m->nin; p.stride = m->nin; p.nan_slot = -1;                       // dense rows of the model's own width
    return p;
}

// rows_cap sizes the grid (one workgroup per tile up to one per CU; the kernel strides over tiles beyond); rb = 16-row blocks per tile
// (the model's own choice for batches; streams pass 1).  A row's probabilities do not depend on the tile it lands in.
void launch_classify(const wsa_model* m, const ClsParams& p, uint32_t rows_cap, hipStream_t s, int rb = 0) {
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

void launch_classify(const wsa_model* m, const double* feat, uint32_t n_rows, const uint32_t* d_n_rows, uint32_t rows_cap, float* prob, hipStream_t s, int rb = 0) {
    launch_classify(m, cls_params(m, feat, n_rows, d_n_rows, prob), rows_cap, s, rb);
}

// the same launch with the regression epilogue: value [rows] f64 = the one output unit, un-normalised with the caller's range
void launch_regress(const wsa_model* m, const double* feat, uint32_t n_rows, const uint32_t* d_n_rows, uint32_t rows_cap, double* value,
                    double out_min, double out_span, hipStream_t s) {
    ClsParams p = cls_params(m, feat, n_rows, d_n_rows, nullptr);
    p.value = value; p.out_min = out_min; p.out_span = out_span;
    launch_classify(m, p, rows_cap, s);
}

// what every regression entry point refuses (all WSA_ERR_INVALID); NULL when the model and the range will do
const char* regress_refusal(const wsa_model* m, double out_min, double out_max) {
    if (m->softmax) return "a regression model's last layer is linear, relu, sigmoid or tanh, not softmax";
    if (m->C != 1) return "a regression model has one output unit";
    if (!std::isfinite(out_min) || !std::isfinite(out_max)) return "non-finite out_min / out_max";
    if (out_max == out_min) return "the output has max == min: it cannot be un-normalised";
    return nullptr;
}

// the rows a batch hands K6: the row table (levels 5 and 13; level 12 at its stride of WSA_NFEAT, slots 0 .. 22, slot 23 the throw mark)
// or the utterance table (level 11); both counts sit on the device
ClsParams batch_params(const wsa_batch_view& v, const wsa_model* m, float* prob) {
    ClsParams p = cls_params(m, v.d_feat, 0, v.d_row_off + v.n_clips, prob);
    if (v.level == 11) { p.feat = v.d_utt_feat; p.d_n_rows = v.d_utt_off + v.n_clips; }
    if (v.level == 12) { p.stride = WSA_NFEAT; p.nan_slot = L12_NCOEF; }
    return p;
}

// every pairing of a batch's level and a model's input count but 5 / 13 with 53, 11 with 264 and 12 with 23 is refused
wsa_status batch_pairing_check(wsa_ctx* ctx, const char* entry, int level, const wsa_model* m) {
    const int have = wsa_level_feature_count(level);
    if (have == m->nin) return WSA_OK;
    const char* levels = m->nin == WSA_NUTT ? "output_level 11 (utterance features)" : m->nin == L12_NCOEF ? "output_level 12 (syllable coefficients)"
                                            : "output_level 5 (segment features) or 13 (syllable features)";
    return fail(ctx, WSA_ERR_INVALID, std::string(entry) + " needs a batch at " + levels + ", not " + std::to_string(level) + ": the model takes " + std::to_string(m->nin)
                                      + " inputs" + (have ? ", the rows of output_level " + std::to_string(level) + " have " + std::to_string(have) + " features" : std::string())
                                      + " (264-input models go with output_level 11, 23-input models with output_level 12)");
}

wsa_status enqueue_batch(wsa_batch* b, const wsa_batch_view& v, wsa_cls* c, const wsa_model* m, hipStream_t s) {
    wsa_ctx* ctx = v.ctx;
    const uint32_t cap = v.level == 11 ? v.utt_cap : v.rows_cap;
    if (*v.cls_last == 3) {                       // wsa_batch_regress: no fold, no per-callback decision
        ClsParams p = batch_params(v, m, nullptr);
        p.value = c->d_value; p.out_min = c->out_min; p.out_span = c->out_span;
        launch_classify(m, p, cap, s);
        HIP_TRY(ctx, hipGetLastError());
        return WSA_OK;
    }
    launch_classify(m, batch_params(v, m, c->d_prob), cap, s);
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

// K6e's device table: the members in work-list order, each with the row-block factor it gets (its own for batches, 1 in a stream step);
// returns the grid, one workgroup per (member, tile) pair of rows_cap rows up to one per CU
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
    const uint64_t n_cu = e->ctx->n_cu > 0 ? e->ctx->n_cu : 256;
    return (uint32_t)(tiles < n_cu ? (tiles ? tiles : 1) : n_cu);
}

wsa_status ecls_create(const wsa_batch_view& v, const wsa_ensemble* e, wsa_ecls** out) {
    wsa_ctx* ctx = v.ctx;
    wsa_ecls* c = new wsa_ecls();
    c->device = ctx->device; c->ens = e; c->serial = e->serial; c->n = e->n; c->n_clips = v.n_clips; c->lds = e->lds_batch;
    const size_t R = v.rows_cap ? v.rows_cap : 1;
    wsa::DevArena& A = c->mem;
    bool ok = A.alloc(&c->d_t_n, R) && A.alloc(&c->d_t_local, R) && A.alloc(&c->d_clip_cb, (size_t)v.n_clips) && A.alloc(&c->d_cb_off, (size_t)v.n_clips)
              && A.alloc(&c->o.cb, R * 4) && A.alloc(&c->o.cb_db, R) && A.alloc(&c->o.cb_top_label, R) && A.alloc(&c->o.cb_top_conf, R)
              && A.alloc(&c->o.cb_min_db, R) && A.alloc(&c->o.cb_entropy, R) && A.alloc(&c->o.clip_min_db, (size_t)v.n_clips)
              && A.alloc(&c->t.cb_db, R) && A.alloc(&c->t.cb_top_label, R) && A.alloc(&c->t.cb_top_conf, R) && A.alloc(&c->t.cb_min_db, R)
              && A.alloc(&c->t.cb_entropy, R) && A.pin(&c->h_count, &c->h_count_dev, 4);
    c->t.clip_min_db = c->o.clip_min_db;
    for (uint32_t d = 0; d < e->n && ok; d++) {
        const wsa_model* m = e->m[d];
        FoldMember& f = c->fm[d];
        c->C[d] = (uint32_t)m->C;
        ok = A.alloc(&c->d_prob[d], R * m->C) && A.alloc(&f.t_label, R) && A.alloc(&f.t_conf, R) && A.alloc(&f.t_all_max, R)
             && A.alloc(&f.clip_conf, (size_t)v.n_clips * m->C) && A.alloc(&f.cb_label, R) && A.alloc(&f.cb_conf, R)
             && A.alloc(&f.cb_all_max, R);
        f.C = (uint32_t)m->C; f.prob = c->d_prob[d]; f.key_rank = m->d_key_rank;
    }
    if (ok) {
        std::vector<ClsGroupEntry> tab;
        c->grid = group_table(e, v.d_feat, v.d_row_off + v.n_clips, c->d_prob, v.rows_cap, false, tab);
        std::vector<FoldMember> ftab(c->fm, c->fm + e->n);
        ok = A.upload(&c->d_ctab, tab) && A.upload(&c->d_ftab, ftab);
    }
    if (!ok) {
        const std::string msg = std::string("device allocation failed: ") + hipGetErrorString(hipGetLastError());
        delete c;
        return fail(ctx, WSA_ERR_HIP, msg);
    }
    *out = c;
    return WSA_OK;
}

// K6e, then (level 13) K6b-e and its compaction with the decision: three launches whatever the number of members
wsa_status enqueue_batch_ensemble(const wsa_batch_view& v, wsa_ecls* c, hipStream_t s) {
    wsa_ctx* ctx = v.ctx;
    hipLaunchKernelGGL(classify_group_kernel, dim3(c->grid), dim3(CLS_THREADS), c->lds, s, c->d_ctab, (int)c->n, v.d_row_off + v.n_clips);
    HIP_TRY(ctx, hipGetLastError());
    if (v.level == 13) {
        FoldGroupParams f{};
        f.n_clips = v.n_clips; f.n_members = c->n; f.step_s = ctx->cfg.window_step / 1e3;
        f.meta = v.d_meta; f.row_off = v.d_row_off; f.tab = c->d_ftab; f.t_n = c->d_t_n; f.t_local = c->d_t_local; f.clip_cb = c->d_clip_cb; f.t = c->t;
        if (v.n_clips) hipLaunchKernelGGL(fold_group_kernel, dim3(v.n_clips), dim3(64 * c->n), 0, s, f);
        hipLaunchKernelGGL(fold_compact_group_kernel, dim3(1), dim3(1024), 0, s, v.n_clips, c->n, v.d_row_off, v.d_meta, c->d_clip_cb, c->d_cb_off,
                           c->d_t_n, c->d_t_local, c->d_ftab, c->t, c->o, c->h_count_dev);
        HIP_TRY(ctx, hipGetLastError());
    }
    return WSA_OK;
}

// ---- streams (wsa_stream_set_model): K6 on every step's rows, the carried fold at level 13; everything allocated at attach time
wsa_status stream_cls_check(wsa_ctx* ctx, int level, const wsa_model* m) {
    if (level != 5 && level != 13)
        return fail(ctx, WSA_ERR_INVALID, "wsa_stream_set_model needs streams at output_level 5 (segment features) or 13 (syllable features), not " + std::to_string(level));
    if (m->ctx != ctx) return fail(ctx, WSA_ERR_INVALID, "the model was created on another context (or device) than the streams");
    if (m->nin != WSA_NFEAT)
        return fail(ctx, WSA_ERR_INVALID, "the model takes " + std::to_string(m->nin) + " inputs: streams classify the 53-feature rows of output_level 5 and 13");
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

// ---- streams with an ensemble (wsa_stream_set_ensemble): K6e, the (stream, member) folds and the per-stream decision as three kernels of the step
struct wsa_sens {
    int device = 0;
    const wsa_ensemble* ens = nullptr;
    wsa_scls_view v{};
    uint32_t n = 0, grid = 1;
    uint32_t C[WSA_ENSEMBLE_MAX] = {};
    float* d_prob[WSA_ENSEMBLE_MAX] = {};
    FoldMember fm[WSA_ENSEMBLE_MAX] = {};
    StreamMember sm[WSA_ENSEMBLE_MAX] = {};                     // (device pointers)
    float* h_prob[WSA_ENSEMBLE_MAX] = {}; int32_t* h_cb_label[WSA_ENSEMBLE_MAX] = {};
    double *h_cb_conf[WSA_ENSEMBLE_MAX] = {}, *h_cb_all_max[WSA_ENSEMBLE_MAX] = {}, *h_conf[WSA_ENSEMBLE_MAX] = {};
    ClsGroupEntry* d_ctab = nullptr; FoldMember* d_ftab = nullptr; StreamMember* d_stab = nullptr;
    EnsTables o{}, h{}, h_dev{};
    double* d_max_inv = nullptr; int32_t* d_min_db = nullptr;
    uint32_t *h_count = nullptr, *h_count_dev = nullptr;
    wsa::DevArena mem;
    // steps beyond the D2H window
    std::vector<float> x_prob[WSA_ENSEMBLE_MAX]; std::vector<int32_t> x_cb_label[WSA_ENSEMBLE_MAX]; std::vector<double> x_cb_conf[WSA_ENSEMBLE_MAX], x_cb_all_max[WSA_ENSEMBLE_MAX];
    std::vector<int32_t> x_cb, x_cb_db, x_cb_top_label, x_cb_min_db; std::vector<double> x_cb_top_conf, x_cb_entropy;
};

void wsa_sens_free(wsa_sens* c) {
    if (!c) return;
    (void)hipSetDevice(c->device);
    delete c;
}

wsa_status wsa_sens_create(const wsa_scls_view& v, const wsa_ensemble* e, wsa_sens** out) {
    wsa_ctx* ctx = v.ctx;
    *out = nullptr;
    if (v.level != 5 && v.level != 13)
        return fail(ctx, WSA_ERR_INVALID, "wsa_stream_set_ensemble needs streams at output_level 5 (segment features) or 13 (syllable features), not " + std::to_string(v.level));
    if (e->ctx != ctx) return fail(ctx, WSA_ERR_INVALID, "the ensemble was created on another context (or device) than the streams");
    if (v.level == 13 && !e->softmax) return fail(ctx, WSA_ERR_INVALID, "the level-13 fold needs class probabilities: a member's last layer is not softmax");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    wsa_sens* c = new wsa_sens();
    c->device = ctx->device; c->ens = e; c->v = v; c->n = e->n;
    const bool fold = v.level == 13;
    const size_t R = v.rows_cap ? v.rows_cap : 1, W = v.d2h_rows ? v.d2h_rows : 1, NS = v.n_streams;
    wsa::DevArena& A = c->mem;
    bool ok = true;
    if (fold) {
        ok = A.alloc(&c->o.cb, R * 4) && A.alloc(&c->o.cb_db, R) && A.alloc(&c->o.cb_top_label, R) && A.alloc(&c->o.cb_top_conf, R)
             && A.alloc(&c->o.cb_min_db, R) && A.alloc(&c->o.cb_entropy, R) && A.alloc(&c->o.clip_min_db, NS)
             && A.pin(&c->h.cb, &c->h_dev.cb, W * 4) && A.pin(&c->h.cb_db, &c->h_dev.cb_db, W) && A.pin(&c->h.cb_top_label, &c->h_dev.cb_top_label, W)
             && A.pin(&c->h.cb_top_conf, &c->h_dev.cb_top_conf, W) && A.pin(&c->h.cb_min_db, &c->h_dev.cb_min_db, W)
             && A.pin(&c->h.cb_entropy, &c->h_dev.cb_entropy, W) && A.pin(&c->h.clip_min_db, &c->h_dev.clip_min_db, NS)
             && A.alloc(&c->d_max_inv, NS, true) && A.alloc(&c->d_min_db, NS) && A.pin(&c->h_count, &c->h_count_dev, 4)
             && hipMemset(c->d_min_db, 0xff, (NS ? NS : 1) * sizeof(int32_t)) == hipSuccess;
        for (size_t i = 0; ok && i < NS; i++) c->h.clip_min_db[i] = -1;
    }
    for (uint32_t d = 0; d < e->n && ok; d++) {
        const wsa_model* m = e->m[d];
        const size_t Cd = (size_t)m->C, NC = NS * Cd;
        FoldMember& f = c->fm[d];
        StreamMember& q = c->sm[d];
        c->C[d] = (uint32_t)Cd;
        ok = A.alloc(&c->d_prob[d], R * Cd) && A.pin(&c->h_prob[d], &q.h_prob, W * Cd);
        f.C = (uint32_t)Cd; f.prob = c->d_prob[d]; f.key_rank = m->d_key_rank;
        if (ok && fold) {
            ok = A.alloc(&f.t_label, R) && A.alloc(&f.t_conf, R) && A.alloc(&f.t_seg, R) && A.alloc(&f.t_all_max, R) && A.alloc(&f.t_all_sum, R)
                 && A.alloc(&q.acc_all, NC, true) && A.alloc(&q.in_all, NC, true) && A.alloc(&q.first, NC, true) && A.alloc(&q.stamp, NS, true)
                 && A.pin(&c->h_cb_label[d], &q.h_cb_label, W) && A.pin(&c->h_cb_conf[d], &q.h_cb_conf, W)
                 && A.pin(&c->h_cb_all_max[d], &q.h_cb_all_max, W) && A.pin(&c->h_conf[d], &q.h_conf, NC);
            f.cb_label = f.t_label; f.cb_conf = f.t_conf; f.cb_all_max = f.t_all_max;
        }
    }
    if (ok) {
        // as for one model: tiles of 16 rows, and a grid that covers the D2H window in one pass
        std::vector<ClsGroupEntry> tab;
        c->grid = group_table(e, v.d_feat, v.d_totals, c->d_prob, v.rows_cap < v.d2h_rows ? v.rows_cap : v.d2h_rows, true, tab);
        std::vector<FoldMember> ftab(c->fm, c->fm + e->n);
        std::vector<StreamMember> stab(c->sm, c->sm + e->n);
        ok = A.upload(&c->d_ctab, tab) && A.upload(&c->d_ftab, ftab) && A.upload(&c->d_stab, stab) && hipDeviceSynchronize() == hipSuccess;
    }
    if (!ok) {
        const std::string msg = std::string("device allocation failed: ") + hipGetErrorString(hipGetLastError());
        wsa_sens_free(c);
        return fail(ctx, WSA_ERR_HIP, msg);
    }
    *out = c;
    return WSA_OK;
}

wsa_status wsa_sens_enqueue(wsa_sens* c, hipStream_t s) {
    const wsa_scls_view& v = c->v;
    hipLaunchKernelGGL(classify_group_kernel, dim3(c->grid), dim3(CLS_THREADS), c->ens->lds_stream, s, c->d_ctab, (int)c->n, v.d_totals);
    HIP_TRY(v.ctx, hipGetLastError());
    StreamEnsParams p{};
    p.n = v.n_streams; p.n_members = c->n; p.cap = v.d2h_rows; p.fold = v.level == 13 ? 1 : 0; p.step_s = v.ctx->cfg.window_step / 1e3;
    p.meta = v.d_meta; p.row_off = v.d_row_off; p.bits = v.d_bits; p.tab = c->d_ftab; p.stab = c->d_stab;
    p.o = c->o; p.h = c->h_dev; p.max_inv = c->d_max_inv; p.min_db = c->d_min_db; p.h_count = c->h_count_dev;
    const uint32_t waves = v.n_streams * c->n;
    hipLaunchKernelGGL(stream_fold_group_kernel, dim3((waves + 3) / 4), dim3(256), 0, s, p);
    if (p.fold) hipLaunchKernelGGL(stream_decide_kernel, dim3((v.n_streams + 3) / 4), dim3(256), 0, s, p);
    HIP_TRY(v.ctx, hipGetLastError());
    return WSA_OK;
}

namespace {
template <typename T>
wsa_status fetch_table(wsa_ctx* ctx, std::vector<T>& x, const T* dev, size_t count, const T** out) {
    x.resize(count + 1);
    if (count) HIP_TRY(ctx, hipMemcpy(x.data(), dev, count * sizeof(T), hipMemcpyDeviceToHost));
    *out = x.data();
    return WSA_OK;
}
}  // namespace

// after the step has completed: the tables of `rows` rows; a step beyond the D2H window is fetched from the device here
wsa_status wsa_sens_result(wsa_sens* c, uint32_t rows, wsa_stream_ensemble_result* o) {
    const wsa_scls_view& v = c->v;
    wsa_ctx* ctx = v.ctx;
    const bool fold = v.level == 13;
    const uint32_t ncb = fold ? ((const volatile uint32_t*)c->h_count)[0] : 0u;
    std::memset(o, 0, sizeof(*o));
    o->n_rows = rows; o->n_members = c->n; o->n_callbacks = ncb; o->n_streams = v.n_streams;
    for (uint32_t d = 0; d < c->n; d++) {
        o->n_classes[d] = c->C[d]; o->prob[d] = c->h_prob[d];
        if (fold) { o->cb_label[d] = c->h_cb_label[d]; o->cb_conf[d] = c->h_cb_conf[d]; o->cb_all_max[d] = c->h_cb_all_max[d]; o->stream_conf[d] = c->h_conf[d]; }
    }
    if (fold) {
        o->cb = c->h.cb; o->cb_db = c->h.cb_db; o->cb_top_label = c->h.cb_top_label; o->cb_top_conf = c->h.cb_top_conf;
        o->cb_min_db = c->h.cb_min_db; o->cb_entropy = c->h.cb_entropy; o->stream_min_db = c->h.clip_min_db;
    }
    if (rows > v.d2h_rows) {
        HIP_TRY(ctx, hipSetDevice(ctx->device));
        wsa_status st = WSA_OK;
        for (uint32_t d = 0; d < c->n && st == WSA_OK; d++) {
            st = fetch_table(ctx, c->x_prob[d], (const float*)c->d_prob[d], (size_t)rows * c->C[d], &o->prob[d]);
            if (!fold) continue;
            if (st == WSA_OK) st = fetch_table(ctx, c->x_cb_label[d], (const int32_t*)c->fm[d].t_label, ncb, &o->cb_label[d]);
            if (st == WSA_OK) st = fetch_table(ctx, c->x_cb_conf[d], (const double*)c->fm[d].t_conf, ncb, &o->cb_conf[d]);
            if (st == WSA_OK) st = fetch_table(ctx, c->x_cb_all_max[d], (const double*)c->fm[d].t_all_max, ncb, &o->cb_all_max[d]);
        }
        if (fold) {
            if (st == WSA_OK) st = fetch_table(ctx, c->x_cb, (const int32_t*)c->o.cb, (size_t)ncb * 4, &o->cb);
            if (st == WSA_OK) st = fetch_table(ctx, c->x_cb_db, (const int32_t*)c->o.cb_db, ncb, &o->cb_db);
            if (st == WSA_OK) st = fetch_table(ctx, c->x_cb_top_label, (const int32_t*)c->o.cb_top_label, ncb, &o->cb_top_label);
            if (st == WSA_OK) st = fetch_table(ctx, c->x_cb_top_conf, (const double*)c->o.cb_top_conf, ncb, &o->cb_top_conf);
            if (st == WSA_OK) st = fetch_table(ctx, c->x_cb_min_db, (const int32_t*)c->o.cb_min_db, ncb, &o->cb_min_db);
            if (st == WSA_OK) st = fetch_table(ctx, c->x_cb_entropy, (const double*)c->o.cb_entropy, ncb, &o->cb_entropy);
        }
        if (st != WSA_OK) return st;
    }
    return WSA_OK;
}

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
    std::vector<int32_t> kr(m->C, -1);
    if (d->labels) for (int c = 0; c < m->C; c++) { int32_t v; if (array_index_key(d->labels[c], &v)) kr[c] = v; }
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
    if (const wsa_status st = batch_pairing_check(ctx, "wsa_batch_classify", v.level, m)) return st;
    if (m->ctx != ctx) return fail(ctx, WSA_ERR_INVALID, "the model was created on another context (or device) than the batch");
    if (v.level == 13 && !m->softmax) return fail(ctx, WSA_ERR_INVALID, "the level-13 fold needs class probabilities: the model's last layer is not softmax");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    wsa_cls*& c = *v.cls;
    if (!c || c->cap_c < (uint32_t)m->C) {        // first call (or a model of more classes): the only allocation of this path
        wsa_cls* n = new wsa_cls();
        n->device = ctx->device; n->cap_rows = v.rows_cap; n->cap_c = (uint32_t)m->C; n->n_clips = v.n_clips;
        const uint32_t cap = v.level == 11 ? v.utt_cap : v.rows_cap;           // level 11: one output row per utterance row
        const size_t R = cap ? cap : 1;
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
    *v.cls_last = 1;
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
    if (*v.cls_last == 3) return fail(ctx, WSA_ERR_INVALID, "the batch's last model call was wsa_batch_regress: its values are wsa_batch_copy_values'");
    if (*v.cls_last != 1) return fail(ctx, WSA_ERR_INVALID, "the batch's last classification was an ensemble's: its tables are wsa_batch_ensemble_result's");
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
    out->n_rows = c->level == 11 ? r.n_utterance_rows : r.n_rows; out->n_classes = (uint32_t)c->n_classes; out->n_clips = v.n_clips;
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

// ---- regression models (ords_<label>): K6 with the un-normalising epilogue (ref src/neuralmodel.js:410-585, predict_db_nn / predict_single)
wsa_status wsa_regress_rows(const wsa_model* m, double out_min, double out_max, const double* d_feat, uint32_t n_rows, double* d_value, void* stream) {
    if (!m) return WSA_ERR_INVALID;
    wsa_ctx* ctx = m->ctx;
    if (const char* why = regress_refusal(m, out_min, out_max)) return fail(ctx, WSA_ERR_INVALID, why);
    if (n_rows && (!d_feat || !d_value)) return fail(ctx, WSA_ERR_INVALID, "null feature / value pointer");
    if (!n_rows) return WSA_OK;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    launch_regress(m, d_feat, n_rows, nullptr, n_rows, d_value, out_min, out_max - out_min, reinterpret_cast<hipStream_t>(stream));
    HIP_TRY(ctx, hipGetLastError());
    return WSA_OK;
}

wsa_status wsa_batch_regress(wsa_batch* b, const wsa_model* m, double out_min, double out_max, void* stream) {
    if (!b || !m) return WSA_ERR_INVALID;
    wsa_batch_view v;
    wsa_batch_view_internal(b, &v);
    wsa_ctx* ctx = v.ctx;
    if (const wsa_status st = batch_pairing_check(ctx, "wsa_batch_regress", v.level, m)) return st;
    if (m->ctx != ctx) return fail(ctx, WSA_ERR_INVALID, "the model was created on another context (or device) than the batch");
    if (const char* why = regress_refusal(m, out_min, out_max)) return fail(ctx, WSA_ERR_INVALID, why);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    wsa_cls*& c = *v.cls;
    if (!c) { c = new wsa_cls(); c->device = ctx->device; c->cap_rows = v.rows_cap; c->n_clips = v.n_clips; }   // cap_c 0: a later classify builds its own tables
    const uint32_t cap = v.level == 11 ? v.utt_cap : v.rows_cap;
    if (!c->d_value && !c->mem.alloc(&c->d_value, cap ? cap : 1))                   // first call: the only allocation of this path
        return fail(ctx, WSA_ERR_HIP, std::string("device allocation failed: ") + hipGetErrorString(hipGetLastError()));
    *v.cls_last = 3;
    c->model = m; c->level = v.level; c->n_classes = 1; c->reruns = v.reruns; c->done = true;
    c->out_min = out_min; c->out_span = out_max - out_min;
    return enqueue_batch(b, v, c, m, reinterpret_cast<hipStream_t>(stream));
}

wsa_status wsa_batch_copy_values(wsa_batch* b, void* stream, double* value, uint32_t rows_cap, uint32_t* n_rows) {
    if (!b) return WSA_ERR_INVALID;
    wsa_batch_view v;
    wsa_batch_view_internal(b, &v);
    wsa_ctx* ctx = v.ctx;
    wsa_cls* c = *v.cls;
    if (!c || !c->done || *v.cls_last != 3) return fail(ctx, WSA_ERR_INVALID, "the batch's last model call was not wsa_batch_regress");
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    wsa_status st = wsa_batch_fetch_internal(b, s);
    if (st != WSA_OK) return st;
    wsa_batch_view_internal(b, &v);
    if (v.reruns != c->reruns) {                  // the back end was rerun with the full tracker table: its rows again
        c->reruns = v.reruns;
        st = enqueue_batch(b, v, c, c->model, s);
        if (st != WSA_OK) return st;
    }
    HIP_TRY(ctx, hipStreamSynchronize(s));
    wsa_device_result r;
    st = wsa_batch_result(b, stream, &r);
    if (st != WSA_OK) return st;
    const uint32_t rows = c->level == 11 ? r.n_utterance_rows : r.n_rows;
    if (n_rows) *n_rows = rows;
    if (value && rows_cap < rows) return fail(ctx, WSA_ERR_INVALID, "value buffer too small");
    if (value && rows) {
        HIP_TRY(ctx, hipMemcpyAsync(value, c->d_value, (size_t)rows * sizeof(double), hipMemcpyDefault, s));
        HIP_TRY(ctx, hipStreamSynchronize(s));
    }
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

wsa_status wsa_batch_classify_ensemble(wsa_batch* b, const wsa_ensemble* e, void* stream) {
    if (!b || !e) return WSA_ERR_INVALID;
    wsa_batch_view v;
    wsa_batch_view_internal(b, &v);
    wsa_ctx* ctx = v.ctx;
    if (v.level != 5 && v.level != 13)
        return fail(ctx, WSA_ERR_INVALID, "wsa_batch_classify_ensemble needs a batch at output_level 5 (segment features) or 13 (syllable features), not " + std::to_string(v.level));
    if (e->ctx != ctx) return fail(ctx, WSA_ERR_INVALID, "the ensemble was created on another context (or device) than the batch");
    if (v.level == 13 && !e->softmax) return fail(ctx, WSA_ERR_INVALID, "the level-13 fold needs class probabilities: a member's last layer is not softmax");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    wsa_ecls*& c = *v.ecls;
    if (!c || c->ens != e || c->serial != e->serial) {     // first call with this ensemble: the only allocation of this path
        wsa_ecls* n = nullptr;
        const wsa_status st = ecls_create(v, e, &n);
        if (st != WSA_OK) return st;
        wsa_ecls_free(c);
        c = n;
    }
    *v.cls_last = 2;
    c->level = v.level; c->reruns = v.reruns;
    return enqueue_batch_ensemble(v, c, reinterpret_cast<hipStream_t>(stream));
}

wsa_status wsa_batch_ensemble_result(wsa_batch* b, void* stream, wsa_ensemble_result* out) {
    if (!b || !out) return WSA_ERR_INVALID;
    wsa_batch_view v;
    wsa_batch_view_internal(b, &v);
    wsa_ctx* ctx = v.ctx;
    wsa_ecls* ec = *v.ecls;
    if (!ec) return fail(ctx, WSA_ERR_INVALID, "no wsa_batch_classify_ensemble on this batch yet");
    if (*v.cls_last != 2) return fail(ctx, WSA_ERR_INVALID, "the batch's last classification was one model's: its tables are wsa_batch_class_result's");
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    wsa_status st = wsa_batch_fetch_internal(b, s);
    if (st != WSA_OK) return st;
    wsa_batch_view_internal(b, &v);
    if (v.reruns != ec->reruns) {                  // the back end was rerun with the full tracker table: classify its rows again
        ec->reruns = v.reruns;
        st = enqueue_batch_ensemble(v, ec, s);
        if (st != WSA_OK) return st;
    }
    HIP_TRY(ctx, hipStreamSynchronize(s));
    wsa_device_result r;
    st = wsa_batch_result(b, stream, &r);
    if (st != WSA_OK) return st;
    std::memset(out, 0, sizeof(*out));
    const bool fold = ec->level == 13;
    out->n_rows = r.n_rows; out->n_members = ec->n; out->n_clips = v.n_clips;
    out->n_callbacks = fold ? ((const volatile uint32_t*)ec->h_count)[0] : 0u;
    for (uint32_t d = 0; d < ec->n; d++) {
        out->n_classes[d] = ec->C[d]; out->d_prob[d] = ec->d_prob[d];
        if (!fold) continue;
        out->d_cb_label[d] = ec->fm[d].cb_label; out->d_cb_conf[d] = ec->fm[d].cb_conf; out->d_cb_all_max[d] = ec->fm[d].cb_all_max;
        out->d_clip_conf[d] = ec->fm[d].clip_conf;
    }
    if (fold) {
        out->d_cb = ec->o.cb; out->d_cb_db = ec->o.cb_db; out->d_cb_top_label = ec->o.cb_top_label; out->d_cb_top_conf = ec->o.cb_top_conf;
        out->d_cb_min_db = ec->o.cb_min_db; out->d_cb_entropy = ec->o.cb_entropy; out->d_clip_min_db = ec->o.clip_min_db;
    }
    return WSA_OK;
}

wsa_status wsa_batch_copy_ensemble(wsa_batch* b, void* stream, const wsa_ensemble_host* dst) {
    if (!b || !dst) return WSA_ERR_INVALID;
    wsa_ensemble_result r;
    const wsa_status st = wsa_batch_ensemble_result(b, stream, &r);
    if (st != WSA_OK) return st;
    wsa_batch_view v;
    wsa_batch_view_internal(b, &v);
    wsa_ctx* ctx = v.ctx;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    bool any_prob = false, any_cb = dst->cb || dst->cb_db || dst->cb_top_label || dst->cb_top_conf || dst->cb_min_db || dst->cb_entropy;
    for (uint32_t d = 0; d < r.n_members; d++) { any_prob = any_prob || dst->prob[d]; any_cb = any_cb || dst->cb_label[d] || dst->cb_conf[d] || dst->cb_all_max[d]; }
    if (any_prob && dst->rows_cap < r.n_rows) return fail(ctx, WSA_ERR_INVALID, "probability buffer too small");
    if (any_cb && dst->cb_cap < r.n_callbacks) return fail(ctx, WSA_ERR_INVALID, "callback buffer too small");
    const size_t K = r.n_callbacks;
#define WSA_COPY_(to, from, count, type) \
    do { if ((to) && (from) && (count)) HIP_TRY(ctx, hipMemcpyAsync((to), (from), (size_t)(count) * sizeof(type), hipMemcpyDefault, s)); } while (0)
    for (uint32_t d = 0; d < r.n_members; d++) {
        WSA_COPY_(dst->prob[d], r.d_prob[d], (size_t)r.n_rows * r.n_classes[d], float);
        WSA_COPY_(dst->cb_label[d], r.d_cb_label[d], K, int32_t);
        WSA_COPY_(dst->cb_conf[d], r.d_cb_conf[d], K, double);
        WSA_COPY_(dst->cb_all_max[d], r.d_cb_all_max[d], K, double);
        WSA_COPY_(dst->clip_conf[d], r.d_clip_conf[d], (size_t)r.n_clips * r.n_classes[d], double);
    }
    WSA_COPY_(dst->cb, r.d_cb, K * 4, int32_t);
    WSA_COPY_(dst->cb_db, r.d_cb_db, K, int32_t);
    WSA_COPY_(dst->cb_top_label, r.d_cb_top_label, K, int32_t);
    WSA_COPY_(dst->cb_top_conf, r.d_cb_top_conf, K, double);
    WSA_COPY_(dst->cb_min_db, r.d_cb_min_db, K, int32_t);
    WSA_COPY_(dst->cb_entropy, r.d_cb_entropy, K, double);
    WSA_COPY_(dst->clip_min_db, r.d_clip_min_db, r.n_clips, int32_t);
#undef WSA_COPY_
    HIP_TRY(ctx, hipStreamSynchronize(s));
    return WSA_OK;
}

}  // extern "C"
