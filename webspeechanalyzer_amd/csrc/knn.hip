// knn.hip — K9: the app's ml5 KNN classifier (specification KN-1) on the device: the store object, knn_add_kernel,
// knn_classify_kernel and the wsa_knn_* / wsa_batch_knn* entry points (include/wsa.h "KNN classifier"); and K9s, the same selection with
// the store split over workgroups for the few rows of a stream step (knn_partial_kernel, knn_merge_kernel; knn_fold.hip puts them into
// the step).
//
// Stands in for ref src/neuralmodel.js:729-837 (train_knn): ml5.KNNClassifier().addExample(features, label) over a labelled feature DB and
// classify(features, 10, ...) — in dist/ml5.min.js the tfjs knn-classifier: rows normalised to unit length, sim = train . q as one f32
// matMul, a stable descending top-k, one vote per neighbour, confidence = votes / k.
//
// The store keeps the unit rows as f32 [capacity][WP] (WP = the width padded to the k step of two MFMAs, 8), zero padded, in insertion
// order; rows never move.  A row's grouped rank (its position in ml5's per-class concatenation) is recomputed after every add from the
// per-class counts.  knn_classify_kernel keeps a tile of KNN_QT query rows resident (their MFMA A fragments in registers), streams the store
// through LDS in tiles of KNN_T rows and selects as it goes: the [queries][train] matrix never exists.  A query's neighbours are defined
// by (similarity, rank) alone and a similarity by its (query, train row) pair alone — the k order of the MFMA chain is fixed — so the
// result does not depend on tile shape or grid.
#include <cmath>
#include <cstring>
#include <memory>
#include <string>
#include <vector>
#include "knn_internal.hpp"
#include "wave_ops.hpp"

using wsa_api::fail;
using namespace wsa_knn_detail;

namespace {

constexpr int KNN_T = 64;               // train rows per tile (wsa_knn_tile_info)
constexpr int KNN_QT = 64;              // query rows per workgroup: 16 per wave
constexpr int KNN_THREADS = 256;
constexpr int L12_THROW_SLOT = 23;      // level 12: slot 23 of a row marks a syllable whose fit threw (coeffs.hip)

typedef float f32x4 __attribute__((ext_vector_type(4)));

__host__ __device__ constexpr int knn_padded(int width) { return (width + 7) & ~7; }
// LDS row stride in floats: 4 mod 64, so the 8-byte B reads of a 32-lane half (16 rows x 2 k pairs) fall on 64 distinct banks
__host__ __device__ constexpr int knn_stride(int wp) { return ((wp - 4 + 63) / 64) * 64 + 4; }
constexpr size_t knn_lds_bytes(int wp) {
    return ((size_t)KNN_T * knn_stride(wp) + 3 * (size_t)KNN_QT * WSA_KNN_MAX_K + 4 * (size_t)KNN_QT) * sizeof(float);
}

// ml5 normalizeVectorToUnitLength (ref dist/ml5.min.js, knn-classifier): the row rounded to f32, divided by its Euclidean norm in f32.
// ONE owner and ONE order per row for stored rows and queries alike, so equal rows give equal unit rows, bit for bit: the squares go
// into eight partial sums (feature c into partial c mod 8, ascending), which are added as a tree.  (Eight short chains lose less than one
// long one; tfjs sums the squares in double.)
__device__ __forceinline__ void knn_unit_row(const double* x, int width, int wp, float* out) {
#pragma clang fp contract(off)
    float part[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    for (int c0 = 0; c0 < width; c0 += 8)
#pragma unroll
        for (int j = 0; j < 8; j++)
            if (c0 + j < width) { const float v = (float)x[c0 + j]; part[j] += v * v; }
    const float ss = ((part[0] + part[1]) + (part[2] + part[3])) + ((part[4] + part[5]) + (part[6] + part[7]));
    const float nrm = sqrtf(ss);
    for (int c = 0; c < width; c++) out[c] = (float)x[c] / nrm;
    for (int c = width; c < wp; c++) out[c] = 0.f;
}

__global__ void __launch_bounds__(256) knn_add_kernel(const double* __restrict__ feat, const int32_t* __restrict__ cls_in, uint32_t n, uint32_t base,
                                                      int width, int wp, int C, float* rows, int32_t* cls, uint32_t* bad) {
    const uint32_t r = blockIdx.x * 256u + threadIdx.x;
    if (r >= n) return;
    knn_unit_row(feat + (size_t)r * width, width, wp, rows + (size_t)(base + r) * wp);
    int32_t c = cls_in[r];
    if (c < 0 || c >= C) { atomicMax(bad, r + 1u); c = 0; }       // reported by wsa_knn_count; the index stays inside the vote table
    cls[base + r] = c;
}

// One wave walks the new rows in insertion order: lane c carries the rows class c has so far, a row's index within its class is that count
// plus the earlier rows of its class in the same 64-row chunk.
__global__ void __launch_bounds__(64) knn_within_kernel(const int32_t* __restrict__ cls, uint32_t base, uint32_t n, int C, uint32_t* class_count, int32_t* within) {
    const int lane = threadIdx.x;
    uint32_t mine = class_count[lane];
    for (uint32_t r0 = 0; r0 < n; r0 += 64) {
        const uint32_t r = r0 + lane;
        const int c = r < n ? cls[base + r] : -1;
        for (int cc = 0; cc < C; cc++) {
            const uint64_t m = __ballot(c == cc);
            if (!m) continue;
            const uint32_t before = (uint32_t)__shfl((int)mine, cc);
            if (c == cc) within[base + r] = (int32_t)(before + (uint32_t)__popcll(m & wsa::lanemask_lt(lane)));
            if (lane == cc) mine += (uint32_t)__popcll(m);
        }
    }
    class_count[lane] = mine;
}

// rank = rows of earlier classes + index within the own class (ml5's train matrix: the per-class matrices concatenated in key order)
__global__ void __launch_bounds__(256) knn_rank_kernel(const int32_t* __restrict__ cls, const int32_t* __restrict__ within, const uint32_t* __restrict__ class_count,
                                                       uint32_t n, int32_t* rank) {
    __shared__ uint32_t s_off[WSA_MODEL_MAX_CLASSES];
    if (threadIdx.x == 0) { uint32_t a = 0; for (int c = 0; c < WSA_MODEL_MAX_CLASSES; c++) { s_off[c] = a; a += class_count[c]; } }
    __syncthreads();
    const uint32_t r = blockIdx.x * 256u + threadIdx.x;
    if (r < n) rank[r] = (int32_t)s_off[cls[r]] + within[r];
}

// One candidate into one query's list (entry j on lane j, best first).  Order: the larger key, then the lower rank; ranks are unique, so
// the order is total and the list does not depend on the order candidates arrive in.
__device__ __forceinline__ void knn_insert(float* s_key, int* s_rk, int* s_ix, float* s_thr, int* s_cnt, int q, float ck, int cidx, int crank, int k_eff, int lane) {
    const int cnt = s_cnt[q];
    float* lk = s_key + q * WSA_KNN_MAX_K; int* lr = s_rk + q * WSA_KNN_MAX_K; int* li = s_ix + q * WSA_KNN_MAX_K;
    const float ek = lk[lane]; const int er = lr[lane], ei = li[lane];
    const bool valid = lane < cnt;
    const bool beats = valid && (ek > ck || (ek == ck && er < crank));
    const int pos = (int)__popcll(__ballot(beats));          // the list is sorted: the entries that beat the candidate are 0 .. pos - 1
    if (pos >= k_eff) return;                                // (wave-uniform) equal to the k-th by value, behind it by rank
    if (valid && lane >= pos && lane + 1 < k_eff) { lk[lane + 1] = ek; lr[lane + 1] = er; li[lane + 1] = ei; }
    const int ncnt = cnt + 1 < k_eff ? cnt + 1 : k_eff;
    const float up = __shfl(ek, k_eff >= 2 ? k_eff - 2 : 0);  // the entry that moves into the last place
    if (lane == 0) {
        lk[pos] = ck; lr[pos] = crank; li[pos] = cidx; s_cnt[q] = ncnt;
        if (ncnt == k_eff) s_thr[q] = pos == k_eff - 1 ? ck : up;
    }
    wsa::wsync();
}

// What a query's finished list becomes (lane j holds entry j): votes, confidences and the label (ml5 calculateTopClass: the first class, in
// key order, whose confidence exceeds a maximum that starts at 0), and the neighbours in selection order
__device__ __forceinline__ void knn_epilogue(const KnnParams& p, uint32_t q, bool thrown, float key, int idx, int lane) {
    const int k_eff = (int)p.k_eff;
    const float NEG_INF = -__builtin_huge_valf();
    const bool in = lane < k_eff && !thrown;
    const int c = in ? p.cls[idx] : -1;
    int votes = 0;
    for (int j = 0; j < k_eff; j++) votes += __shfl(c, j) == lane ? 1 : 0;
    const uint32_t best = wsa::wave_max_u32(lane < p.C ? ((uint32_t)votes << 6) | (uint32_t)(63 - lane) : 0u);
    if (p.label && lane == 0) p.label[q] = thrown ? -1 : 63 - (int)(best & 63u);
    if (p.conf && lane < p.C) p.conf[(size_t)q * p.C + lane] = thrown ? __longlong_as_double(0x7ff8000000000000ll) : (double)votes / (double)k_eff;
    if ((uint32_t)lane < p.k) {
        if (p.nbr) p.nbr[(size_t)q * p.k + lane] = in ? idx : -1;
        if (p.sim) p.sim[(size_t)q * p.k + lane] = in && key != NEG_INF ? key : __int_as_float(0x7fc00000);
    }
}

// mfma_f32_16x16x4f32 as in K6 / K7: lane l holds A[row l&15][k l>>4], B[k l>>4][col l&15]; D col = l&15, row = 4 (l>>4) + i.  Here A
// = 16 query rows of the wave, B = 16 train rows of the tile, and the k index of MFMA 2 jj + m is feature 8 jj + 2 (l>>4) + m on both
// sides (a fixed permutation of the sum's terms), so a lane's B operands of two MFMAs are one 8-byte LDS read.  An MFMA is a k-ordered
// chain of f32 fused multiply-adds; the steps of 8 features alternate between two accumulators that are added at the end, which halves the
// chain's length (and its rounding error) at the price of four registers per block.
//
// SPLIT (K9s, knn_partial_kernel): blockIdx.y is a slice of the store, a contiguous run of whole tiles.  The workgroup selects within its
// slice only and leaves each query's list in the scratch table for knn_merge_kernel; tiles, fragments, the chain and the list logic are
// the code below either way, so a (query, train row) pair has the same similarity bits in both kernels.
template <int WP, bool SPLIT>
__device__ __forceinline__ void knn_body(const KnnParams& p) {
    extern __shared__ __attribute__((aligned(16))) float s_mem[];
    constexpr int S = knn_stride(WP), V4 = WP / 4, NV = (KNN_T * V4 + KNN_THREADS - 1) / KNN_THREADS;
    float* s_tile = s_mem;
    float* s_key = s_tile + KNN_T * S;
    int* s_rk = reinterpret_cast<int*>(s_key + KNN_QT * WSA_KNN_MAX_K);
    int* s_ix = s_rk + KNN_QT * WSA_KNN_MAX_K;
    float* s_thr = reinterpret_cast<float*>(s_ix + KNN_QT * WSA_KNN_MAX_K);
    int* s_cnt = reinterpret_cast<int*>(s_thr + KNN_QT);
    int* s_flag = s_cnt + KNN_QT;
    int* s_trank = s_flag + KNN_QT;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    uint32_t nq = p.d_n_rows ? *p.d_n_rows : p.n_rows;
    const uint32_t n = p.n_store;
    const int k_eff = (int)p.k_eff;
    const float NEG_INF = -__builtin_huge_valf(), POS_INF = __builtin_huge_valf();
    // the slice's rows t_lo .. t_hi - 1 (the whole store for K9); an empty slice has nothing to say
    uint32_t t_lo = 0, t_hi = n;
    if constexpr (SPLIT) {
        const uint64_t per = (uint64_t)p.tiles_per_slice * KNN_T, lo = (uint64_t)blockIdx.y * per;
        if (lo >= n) return;
        t_lo = (uint32_t)lo; t_hi = lo + per < n ? (uint32_t)(lo + per) : n;
        if (p.q_limit && nq > p.q_limit) nq = p.q_limit;
    }
    for (uint32_t qt = blockIdx.x + p.qt0; (uint64_t)qt * KNN_QT < nq; qt += gridDim.x) {
        const uint32_t q0 = qt * KNN_QT;
        __syncthreads();
        // the tile's queries as unit rows (one owner per row); a row past the end or thrown takes no part in the selection
        if (tid < KNN_QT) {
            const uint32_t q = q0 + tid;
            float* out = s_tile + tid * S;
            int flag = q < nq ? 0 : 2;
            if (!flag && p.nan_slot >= 0 && p.feat[(size_t)q * p.stride + p.nan_slot] != 0.0) flag = 1;
            if (!flag) knn_unit_row(p.feat + (size_t)q * p.stride, p.width, WP, out);
            else for (int c = 0; c < WP; c++) out[c] = 0.f;
            s_flag[tid] = flag; s_cnt[tid] = 0; s_thr[tid] = flag ? POS_INF : NEG_INF;
        }
        __syncthreads();
        float a[WP / 4];
        {
            const float* ap = s_tile + (wave * 16 + (lane & 15)) * S + 2 * (lane >> 4);
#pragma unroll
            for (int jj = 0; jj < WP / 8; jj++) { const float2 v = *reinterpret_cast<const float2*>(ap + 8 * jj); a[2 * jj] = v.x; a[2 * jj + 1] = v.y; }
        }
        float thr[4];
#pragma unroll
        for (int i = 0; i < 4; i++) thr[i] = s_thr[wave * 16 + 4 * (lane >> 4) + i];
        // the store, tile by tile: the next tile's loads are in flight while this one is multiplied and selected
        float4 pf[NV]; int pr = 0;
        const auto fetch = [&](uint32_t t0) {
#pragma unroll
            for (int v = 0; v < NV; v++) {
                const int e = tid + v * KNN_THREADS;
                const int row = e / V4, c4 = e - row * V4;
                const uint32_t gr = t0 + (uint32_t)row;
                pf[v] = (e < KNN_T * V4 && gr < n) ? *reinterpret_cast<const float4*>(p.rows + (size_t)gr * WP + 4 * c4) : float4{0.f, 0.f, 0.f, 0.f};
            }
            if (tid < KNN_T) pr = t0 + (uint32_t)tid < n ? p.rank[t0 + tid] : 0;
        };
        fetch(t_lo);
        for (uint32_t t0 = t_lo; t0 < t_hi; t0 += KNN_T) {
            __syncthreads();                                   // the queries' fragments, or the previous tile, have been read
#pragma unroll
            for (int v = 0; v < NV; v++) {
                const int e = tid + v * KNN_THREADS;
                const int row = e / V4, c4 = e - row * V4;
                if (e < KNN_T * V4) *reinterpret_cast<float4*>(s_tile + row * S + 4 * c4) = pf[v];
            }
            if (tid < KNN_T) s_trank[tid] = pr;
            __syncthreads();
            if (t0 + KNN_T < t_hi) fetch(t0 + KNN_T);
            f32x4 acc[KNN_T / 16], odd[KNN_T / 16];            // two chains per block of 16 train rows: the even and the odd steps of 8 features
#pragma unroll
            for (int cb = 0; cb < KNN_T / 16; cb++) acc[cb] = odd[cb] = f32x4{0.f, 0.f, 0.f, 0.f};
            const float* bp = s_tile + (lane & 15) * S + 2 * (lane >> 4);
#pragma unroll
            for (int jj = 0; jj < WP / 8; jj++) {
                float2 b[KNN_T / 16];
#pragma unroll
                for (int cb = 0; cb < KNN_T / 16; cb++) b[cb] = *reinterpret_cast<const float2*>(bp + cb * 16 * S + 8 * jj);
                f32x4* to = jj & 1 ? odd : acc;
#pragma unroll
                for (int cb = 0; cb < KNN_T / 16; cb++) to[cb] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[2 * jj], b[cb].x, to[cb], 0, 0, 0);
#pragma unroll
                for (int cb = 0; cb < KNN_T / 16; cb++) to[cb] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[2 * jj + 1], b[cb].y, to[cb], 0, 0, 0);
            }
#pragma unroll
            for (int cb = 0; cb < KNN_T / 16; cb++) acc[cb] += odd[cb];
            // selection: one compare per candidate against its query's k-th; whatever passes goes through the list, one at a time
#pragma unroll
            for (int cb = 0; cb < KNN_T / 16; cb++) {
                const bool cv = t0 + (uint32_t)(cb * 16 + (lane & 15)) < n;
                float key[4]; bool ps[4];
#pragma unroll
                for (int i = 0; i < 4; i++) {
                    const float s = acc[cb][i];
                    key[i] = s == s ? s : NEG_INF;             // a NaN similarity is lower than every number; ranks decide among NaNs
                    ps[i] = cv && key[i] >= thr[i];
                }
                if (!__ballot(ps[0] || ps[1] || ps[2] || ps[3])) continue;
#pragma unroll
                for (int i = 0; i < 4; i++) {
                    uint64_t m = __ballot(ps[i]);
                    while (m) {
                        const int l = __ffsll((unsigned long long)m) - 1;
                        m &= m - 1;
                        const int tl = cb * 16 + (l & 15);
                        knn_insert(s_key, s_rk, s_ix, s_thr, s_cnt, wave * 16 + 4 * (l >> 4) + i, __shfl(key[i], l), (int)(t0 + (uint32_t)tl), s_trank[tl], k_eff, lane);
                    }
                }
                wsa::wsync();
#pragma unroll
                for (int i = 0; i < 4; i++) thr[i] = s_thr[wave * 16 + 4 * (lane >> 4) + i];
            }
        }
        wsa::wsync();
        for (int r = 0; r < 16; r++) {
            const int ql = wave * 16 + r;
            const uint32_t q = q0 + (uint32_t)ql;
            if (q >= nq) break;
            const float key = s_key[ql * WSA_KNN_MAX_K + lane];
            const int idx = s_ix[ql * WSA_KNN_MAX_K + lane];
            if constexpr (SPLIT) {
                const size_t at = (size_t)q * p.slices + blockIdx.y;
                const int cnt = s_cnt[ql];
                if (lane < cnt) { p.pt_key[at * p.k + lane] = key; p.pt_rank[at * p.k + lane] = s_rk[ql * WSA_KNN_MAX_K + lane]; p.pt_idx[at * p.k + lane] = idx; }
                if (lane == 0) p.pt_cnt[at] = cnt;
            } else {
                knn_epilogue(p, q, s_flag[ql] != 0, key, idx, lane);
            }
        }
    }
}

template <int WP>
__global__ void __launch_bounds__(KNN_THREADS) knn_classify_kernel(KnnParams p) { knn_body<WP, false>(p); }
template <int WP>
__global__ void __launch_bounds__(KNN_THREADS) knn_partial_kernel(KnnParams p) { knn_body<WP, true>(p); }

// K9s, the merge: one wave per query row below q_limit.  The partial lists of the query's slices go through the same list (knn_insert:
// the order is total, so neither the split nor the order the slices arrive in matters), best first each, then K9's epilogue.  A slice
// without rows was never written and is not read; neither is the list of a thrown row.
__global__ void __launch_bounds__(256) knn_merge_kernel(KnnParams p) {
    __shared__ float s_key[4 * WSA_KNN_MAX_K], s_thr[4];
    __shared__ int s_rk[4 * WSA_KNN_MAX_K], s_ix[4 * WSA_KNN_MAX_K], s_cnt[4];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    uint32_t nq = p.d_n_rows ? *p.d_n_rows : p.n_rows;
    if (p.q_limit && nq > p.q_limit) nq = p.q_limit;
    const int k_eff = (int)p.k_eff;
    const uint64_t per = (uint64_t)p.tiles_per_slice * KNN_T;
    for (uint32_t q = blockIdx.x * 4 + w; q < nq; q += gridDim.x * 4) {
        const bool thrown = p.nan_slot >= 0 && p.feat[(size_t)q * p.stride + p.nan_slot] != 0.0;
        if (lane == 0) { s_cnt[w] = 0; s_thr[w] = -__builtin_huge_valf(); }
        wsa::wsync();
        for (uint32_t sl = 0; !thrown && sl < p.slices && (uint64_t)sl * per < p.n_store; sl++) {
            const size_t at = (size_t)q * p.slices + sl;
            const int cnt = p.pt_cnt[at];
            const float ck = lane < cnt ? p.pt_key[at * p.k + lane] : 0.f;
            const int cr = lane < cnt ? p.pt_rank[at * p.k + lane] : 0, ci = lane < cnt ? p.pt_idx[at * p.k + lane] : 0;
            uint64_t m = __ballot(lane < cnt && ck >= s_thr[w]);
            while (m) {
                const int l = __ffsll((unsigned long long)m) - 1;
                m &= m - 1;
                knn_insert(s_key, s_rk, s_ix, s_thr, s_cnt, w, __shfl(ck, l), __shfl(ci, l), __shfl(cr, l), k_eff, lane);
            }
            wsa::wsync();
        }
        knn_epilogue(p, q, thrown, s_key[w * WSA_KNN_MAX_K + lane], s_ix[w * WSA_KNN_MAX_K + lane], lane);
        wsa::wsync();
    }
}

}  // namespace

void wsa_kcls_free(wsa_kcls* c) {
    if (!c) return;
    (void)hipSetDevice(c->device);
    wsa_kfold_free(c->fold);
    delete c;
}

namespace wsa_knn_detail {

void launch_knn(const wsa_knn* kn, const KnnParams& p, uint32_t rows_cap, hipStream_t s) {
    const uint64_t tiles = ((uint64_t)rows_cap + KNN_QT - 1) / KNN_QT;
    const uint64_t most = 8ull * (uint64_t)(kn->ctx->n_cu > 0 ? kn->ctx->n_cu : 256);
    const uint32_t grid = (uint32_t)(tiles < most ? (tiles ? tiles : 1) : most);
    const size_t lds = knn_lds_bytes(kn->wp);
    if (kn->wp == 24) hipLaunchKernelGGL(knn_classify_kernel<24>, dim3(grid), dim3(KNN_THREADS), lds, s, p);
    else if (kn->wp == 56) hipLaunchKernelGGL(knn_classify_kernel<56>, dim3(grid), dim3(KNN_THREADS), lds, s, p);
    else hipLaunchKernelGGL(knn_classify_kernel<264>, dim3(grid), dim3(KNN_THREADS), lds, s, p);
}

KnnParams knn_params(const wsa_knn* kn, const double* feat, uint32_t n_rows, const uint32_t* d_n_rows, uint32_t k) {
    KnnParams p{};
    p.rows = kn->d_rows; p.cls = kn->d_cls; p.rank = kn->d_rank; p.n_store = kn->count;
    p.feat = feat; p.n_rows = n_rows; p.d_n_rows = d_n_rows; p.width = kn->width; p.stride = kn->width; p.nan_slot = -1;
    p.C = kn->C; p.k = k; p.k_eff = k < kn->count ? k : kn->count;
    return p;
}

// what every classification refuses: k outside 1 .. WSA_KNN_MAX_K and a store without examples (ml5: "You have not added any examples")
wsa_status knn_refusal(const wsa_knn* kn, uint32_t k) {
    if (k < 1 || k > WSA_KNN_MAX_K) return fail(kn->ctx, WSA_ERR_INVALID, "k must be 1 .. " + std::to_string(WSA_KNN_MAX_K) + ", got " + std::to_string(k));
    if (!kn->count) return fail(kn->ctx, WSA_ERR_INVALID, "the KNN store has no examples yet");
    return WSA_OK;
}

// ---- K9s on the host.  The slice count S for a window of query rows: as many slices as give every CU two workgroups (K9's LDS lets two
// share a CU) over the window's query tiles, S = ceil(2 n_cu / query tiles) — but no slice shorter than KNN_SPLIT_MIN_TILES store tiles
// (below that a workgroup's fixed cost, its queries' unit rows and its list write, outweighs its share of the store), no more than
// WSA_KNN_SPLIT_MAX_SLICES (the merge walks a query's slices one after the other), and no more than the scratch bound
// WSA_KNN_SPLIT_SCRATCH_BYTES allows at (12 k + 4) bytes per (query row, slice).
constexpr uint32_t KNN_SPLIT_MIN_TILES = 4;

uint32_t knn_split_slices(const wsa_knn* kn, uint32_t window, uint32_t k) {
    const uint64_t q_tiles = ((uint64_t)(window ? window : 1) + KNN_QT - 1) / KNN_QT, tiles = ((uint64_t)kn->count + KNN_T - 1) / KNN_T;
    const uint64_t n_cu = kn->ctx->n_cu > 0 ? kn->ctx->n_cu : 256;
    uint64_t S = (2 * n_cu + q_tiles - 1) / q_tiles;
    const uint64_t by_store = (tiles + KNN_SPLIT_MIN_TILES - 1) / KNN_SPLIT_MIN_TILES;
    const uint64_t by_scratch = (uint64_t)WSA_KNN_SPLIT_SCRATCH_BYTES / ((uint64_t)(window ? window : 1) * (12ull * k + 4ull));
    if (S > by_store) S = by_store;
    if (S > WSA_KNN_SPLIT_MAX_SLICES) S = WSA_KNN_SPLIT_MAX_SLICES;
    if (S > by_scratch) S = by_scratch;
    return S ? (uint32_t)S : 1u;
}

bool knn_split_alloc(wsa::DevArena& A, const wsa_knn* kn, uint32_t window, uint32_t k, uint32_t slices, KnnSplit& out) {
    const uint32_t tiles = (uint32_t)(((uint64_t)kn->count + KNN_T - 1) / KNN_T);
    out.window = window; out.slices = slices ? slices : knn_split_slices(kn, window, k);
    out.tiles_per_slice = (tiles + out.slices - 1) / out.slices;
    if (!out.tiles_per_slice) out.tiles_per_slice = 1;
    const size_t pairs = (size_t)(window ? window : 1) * out.slices;
    return A.alloc(&out.key, pairs * k) && A.alloc(&out.rank, pairs * k) && A.alloc(&out.idx, pairs * k) && A.alloc(&out.cnt, pairs);
}

void launch_knn_split(const wsa_knn* kn, KnnParams p, const KnnSplit& sp, hipStream_t s) {
    p.slices = sp.slices; p.tiles_per_slice = sp.tiles_per_slice; p.q_limit = sp.window;
    p.pt_key = sp.key; p.pt_rank = sp.rank; p.pt_idx = sp.idx; p.pt_cnt = sp.cnt;
    const uint32_t q_tiles = (sp.window + KNN_QT - 1) / KNN_QT;
    const dim3 grid(q_tiles ? q_tiles : 1, sp.slices);
    const size_t lds = knn_lds_bytes(kn->wp);
    if (kn->wp == 24) hipLaunchKernelGGL(knn_partial_kernel<24>, grid, dim3(KNN_THREADS), lds, s, p);
    else if (kn->wp == 56) hipLaunchKernelGGL(knn_partial_kernel<56>, grid, dim3(KNN_THREADS), lds, s, p);
    else hipLaunchKernelGGL(knn_partial_kernel<264>, grid, dim3(KNN_THREADS), lds, s, p);
    hipLaunchKernelGGL(knn_merge_kernel, dim3((sp.window + 3) / 4 ? (sp.window + 3) / 4 : 1), dim3(256), 0, s, p);
}

}  // namespace wsa_knn_detail

namespace {

// the rows a batch hands K9 (the rule of wsa_batch_classify): the row table (levels 5 and 13; level 12 at its stride of WSA_NFEAT, slots
// 0 .. 22, slot 23 the throw mark) or the utterance table (level 11); both counts sit on the device
wsa_status enqueue_batch_knn(const wsa_batch_view& v, const wsa_kcls* c, hipStream_t s) {
    KnnParams p = knn_params(c->knn, v.d_feat, 0, v.d_row_off + v.n_clips, c->k);
    p.k_eff = c->k_eff;
    uint32_t cap = v.rows_cap;
    if (v.level == 11) { p.feat = v.d_utt_feat; p.d_n_rows = v.d_utt_off + v.n_clips; cap = v.utt_cap; }
    else { p.stride = WSA_NFEAT; if (v.level == 12) p.nan_slot = L12_THROW_SLOT; }
    p.label = c->d_label; p.conf = c->d_conf; p.nbr = c->d_nbr; p.sim = c->d_sim;
    launch_knn(c->knn, p, cap, s);
    HIP_TRY(v.ctx, hipGetLastError());
    return WSA_OK;
}

}  // namespace

extern "C" {

wsa_status wsa_knn_tile_info(int32_t* train_rows, int32_t* query_rows) {
    if (train_rows) *train_rows = KNN_T;
    if (query_rows) *query_rows = KNN_QT;
    return WSA_OK;
}

wsa_status wsa_knn_create(wsa_ctx* ctx, int32_t width, int32_t n_classes, uint32_t capacity, wsa_knn** out) {
    if (!ctx || !out) return fail(ctx, WSA_ERR_INVALID, "null argument");
    *out = nullptr;
    if (const char* why = wsa_model_width_refusal(width)) return fail(ctx, WSA_ERR_INVALID, "the KNN store takes " + std::to_string(width) + why);
    if (n_classes < 1 || n_classes > WSA_MODEL_MAX_CLASSES)
        return fail(ctx, WSA_ERR_INVALID, "a KNN store has 1 .. " + std::to_string(WSA_MODEL_MAX_CLASSES) + " classes, got " + std::to_string(n_classes));
    if (capacity < 1 || capacity > 0x7fffffffu / 512u) return fail(ctx, WSA_ERR_INVALID, "a KNN store holds 1 .. " + std::to_string(0x7fffffffu / 512u) + " rows, got " + std::to_string(capacity));
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    wsa_knn* kn = new wsa_knn();
    kn->ctx = ctx; kn->width = width; kn->wp = knn_padded(width); kn->C = n_classes; kn->cap = capacity;
    wsa::DevArena& A = kn->mem;
    const size_t lds = knn_lds_bytes(kn->wp);
    hipError_t e = hipSuccess;
    const auto allow_lds = [&](const void* kernel) { if (e == hipSuccess) e = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds); };
    if (kn->wp == 24) { allow_lds(reinterpret_cast<const void*>(knn_classify_kernel<24>)); allow_lds(reinterpret_cast<const void*>(knn_partial_kernel<24>)); }
    else if (kn->wp == 56) { allow_lds(reinterpret_cast<const void*>(knn_classify_kernel<56>)); allow_lds(reinterpret_cast<const void*>(knn_partial_kernel<56>)); }
    else { allow_lds(reinterpret_cast<const void*>(knn_classify_kernel<264>)); allow_lds(reinterpret_cast<const void*>(knn_partial_kernel<264>)); }
    const bool ok = e == hipSuccess && A.alloc(&kn->d_rows, (size_t)capacity * kn->wp) && A.alloc(&kn->d_cls, (size_t)capacity) && A.alloc(&kn->d_within, (size_t)capacity)
                    && A.alloc(&kn->d_rank, (size_t)capacity) && A.alloc(&kn->d_class_count, (size_t)WSA_MODEL_MAX_CLASSES, true) && A.alloc(&kn->d_bad, 1, true);
    if (!ok) {
        const std::string msg = std::string("device allocation failed: ") + hipGetErrorString(e != hipSuccess ? e : hipGetLastError());
        wsa_knn_destroy(kn);
        return fail(ctx, WSA_ERR_HIP, msg);
    }
    *out = kn;
    return WSA_OK;
}

void wsa_knn_destroy(wsa_knn* kn) {
    if (!kn) return;
    (void)hipSetDevice(kn->ctx->device);
    delete kn;
}

wsa_status wsa_knn_add(wsa_knn* kn, const double* d_feat, const int32_t* d_class, uint32_t n, void* stream) {
    if (!kn) return WSA_ERR_INVALID;
    wsa_ctx* ctx = kn->ctx;
    if (!n) return WSA_OK;
    if (!d_feat || !d_class) return fail(ctx, WSA_ERR_INVALID, "null feature / class pointer");
    if (n > kn->cap - kn->count)
        return fail(ctx, WSA_ERR_CAPACITY, "the KNN store holds " + std::to_string(kn->count) + " of " + std::to_string(kn->cap) + " rows: no room for " + std::to_string(n) + " more");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const uint32_t base = kn->count, total = base + n;
    hipLaunchKernelGGL(knn_add_kernel, dim3((n + 255) / 256), dim3(256), 0, s, d_feat, d_class, n, base, kn->width, kn->wp, kn->C, kn->d_rows, kn->d_cls, kn->d_bad);
    hipLaunchKernelGGL(knn_within_kernel, dim3(1), dim3(64), 0, s, kn->d_cls, base, n, kn->C, kn->d_class_count, kn->d_within);
    hipLaunchKernelGGL(knn_rank_kernel, dim3((total + 255) / 256), dim3(256), 0, s, kn->d_cls, kn->d_within, kn->d_class_count, total, kn->d_rank);
    HIP_TRY(ctx, hipGetLastError());
    kn->count = total;
    return WSA_OK;
}

wsa_status wsa_knn_count(wsa_knn* kn, void* stream, uint32_t* n_rows, uint32_t* class_rows) {
    if (!kn) return WSA_ERR_INVALID;
    wsa_ctx* ctx = kn->ctx;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    uint32_t bad = 0, counts[WSA_MODEL_MAX_CLASSES];
    HIP_TRY(ctx, hipMemcpyAsync(&bad, kn->d_bad, sizeof(bad), hipMemcpyDeviceToHost, s));
    HIP_TRY(ctx, hipMemcpyAsync(counts, kn->d_class_count, sizeof(counts), hipMemcpyDeviceToHost, s));
    HIP_TRY(ctx, hipStreamSynchronize(s));
    if (n_rows) *n_rows = kn->count;
    if (class_rows) std::memcpy(class_rows, counts, (size_t)kn->C * sizeof(uint32_t));
    if (bad) return fail(ctx, WSA_ERR_INVALID, "row " + std::to_string(bad - 1) + " of a wsa_knn_add had a class index outside 0 .. " + std::to_string(kn->C - 1) + " (stored as class 0)");
    return WSA_OK;
}

wsa_status wsa_knn_classify_rows(const wsa_knn* kn, const double* d_feat, uint32_t n_rows, uint32_t k, int32_t* d_label, double* d_conf, int32_t* d_nbr,
                                 float* d_sim, void* stream) {
    if (!kn) return WSA_ERR_INVALID;
    wsa_ctx* ctx = kn->ctx;
    if (const wsa_status st = knn_refusal(kn, k)) return st;
    if (n_rows && !d_feat) return fail(ctx, WSA_ERR_INVALID, "null feature pointer");
    if (!n_rows) return WSA_OK;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    KnnParams p = knn_params(kn, d_feat, n_rows, nullptr, k);
    p.label = d_label; p.conf = d_conf; p.nbr = d_nbr; p.sim = d_sim;
    launch_knn(kn, p, n_rows, reinterpret_cast<hipStream_t>(stream));
    HIP_TRY(ctx, hipGetLastError());
    return WSA_OK;
}

wsa_status wsa_batch_knn(wsa_batch* b, const wsa_knn* kn, uint32_t k, void* stream) {
    if (!b || !kn) return WSA_ERR_INVALID;
    wsa_batch_view v;
    wsa_batch_view_internal(b, &v);
    wsa_ctx* ctx = v.ctx;
    const int have = wsa_level_feature_count(v.level);
    if (have != kn->width) {
        const char* levels = kn->width == WSA_NUTT ? "output_level 11 (utterance features)" : kn->width == L12_THROW_SLOT ? "output_level 12 (syllable coefficients)"
                                                   : "output_level 5 (segment features) or 13 (syllable features)";
        return fail(ctx, WSA_ERR_INVALID, std::string("wsa_batch_knn needs a batch at ") + levels + ", not " + std::to_string(v.level) + ": the KNN store holds rows of "
                                          + std::to_string(kn->width) + " features" + (have ? ", the rows of output_level " + std::to_string(v.level) + " have " + std::to_string(have) : std::string()));
    }
    if (kn->ctx != ctx) return fail(ctx, WSA_ERR_INVALID, "the KNN store was created on another context (or device) than the batch");
    if (const wsa_status st = knn_refusal(kn, k)) { ctx->err = kn->ctx->err; return st; }
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    wsa_kcls*& c = *v.kcls;
    const uint32_t cap = v.level == 11 ? v.utt_cap : v.rows_cap;
    if (!c || c->cap_c < (uint32_t)kn->C || c->cap_k < k) {          // first call (or more classes / a larger k): the only allocation of this path
        wsa_kcls* n = new wsa_kcls();
        n->device = ctx->device; n->cap_rows = cap; n->cap_c = (uint32_t)kn->C; n->cap_k = k;
        const size_t R = cap ? cap : 1;
        wsa::DevArena& A = n->mem;
        if (!(A.alloc(&n->d_label, R) && A.alloc(&n->d_conf, R * kn->C) && A.alloc(&n->d_nbr, R * k) && A.alloc(&n->d_sim, R * k))) {
            const wsa_status st = fail(ctx, WSA_ERR_HIP, std::string("device allocation failed: ") + hipGetErrorString(hipGetLastError()));
            wsa_kcls_free(n);
            return st;
        }
        wsa_kcls_free(c);
        c = n;
    }
    c->knn = kn; c->k = k; c->k_eff = k < kn->count ? k : kn->count; c->level = v.level; c->reruns = v.reruns;
    return enqueue_batch_knn(v, c, reinterpret_cast<hipStream_t>(stream));
}

wsa_status wsa_batch_knn_result(wsa_batch* b, void* stream, wsa_knn_result* out) {
    if (!b || !out) return WSA_ERR_INVALID;
    wsa_batch_view v;
    wsa_batch_view_internal(b, &v);
    wsa_ctx* ctx = v.ctx;
    wsa_kcls* c = *v.kcls;
    if (!c || !c->knn) return fail(ctx, WSA_ERR_INVALID, "no wsa_batch_knn on this batch yet");
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    wsa_status st = wsa_batch_fetch_internal(b, s);
    if (st != WSA_OK) return st;
    wsa_batch_view_internal(b, &v);
    if (v.reruns != c->reruns) {                 // fetching the counters reran the back end with the full tracker table: classify the new rows
        c->reruns = v.reruns;
        if ((st = enqueue_batch_knn(v, c, s)) != WSA_OK) return st;
    }
    HIP_TRY(ctx, hipStreamSynchronize(s));
    wsa_device_result r;
    if ((st = wsa_batch_result(b, s, &r)) != WSA_OK) return st;
    out->n_rows = c->level == 11 ? r.n_utterance_rows : r.n_rows; out->n_classes = (uint32_t)c->knn->C; out->k = c->k; out->k_eff = c->k_eff;
    out->d_label = c->d_label; out->d_conf = c->d_conf; out->d_nbr = c->d_nbr; out->d_sim = c->d_sim;
    return WSA_OK;
}

wsa_status wsa_batch_copy_knn(wsa_batch* b, void* stream, int32_t* label, double* conf, int32_t* nbr, float* sim, uint32_t rows_cap) {
    if (!b) return WSA_ERR_INVALID;
    wsa_knn_result r;
    const wsa_status st = wsa_batch_knn_result(b, stream, &r);
    if (st != WSA_OK) return st;
    wsa_batch_view v;
    wsa_batch_view_internal(b, &v);
    wsa_ctx* ctx = v.ctx;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if ((label || conf || nbr || sim) && rows_cap < r.n_rows) return fail(ctx, WSA_ERR_INVALID, "KNN result buffer too small");
    const size_t R = r.n_rows;
    if (!R) return WSA_OK;
    if (label) HIP_TRY(ctx, hipMemcpyAsync(label, r.d_label, R * sizeof(int32_t), hipMemcpyDefault, s));
    if (conf) HIP_TRY(ctx, hipMemcpyAsync(conf, r.d_conf, R * r.n_classes * sizeof(double), hipMemcpyDefault, s));
    if (nbr) HIP_TRY(ctx, hipMemcpyAsync(nbr, r.d_nbr, R * r.k * sizeof(int32_t), hipMemcpyDefault, s));
    if (sim) HIP_TRY(ctx, hipMemcpyAsync(sim, r.d_sim, R * r.k * sizeof(float), hipMemcpyDefault, s));
    HIP_TRY(ctx, hipStreamSynchronize(s));
    return WSA_OK;
}

// ---- test access (not part of include/wsa.h; in the manner of debug.hip): K9s over n_rows dense device rows with `slices` slices of
// the store (0: the rule's), outputs as wsa_knn_classify_rows.  Only enqueues; the scratch table is kept with the store and allocated at
// the first call or when a call needs a larger one (`stream` is drained first then).  With n_rows = 0 the kernels are launched all the
// same (one query tile, no row): what a stream step without rows runs.
wsa_status wsa_debug_knn_split(const wsa_knn* kn, const double* d_feat, uint32_t n_rows, uint32_t k, uint32_t slices, int32_t* d_label, double* d_conf,
                               int32_t* d_nbr, float* d_sim, void* stream) {
    if (!kn) return WSA_ERR_INVALID;
    wsa_ctx* ctx = kn->ctx;
    if (const wsa_status st = knn_refusal(kn, k)) return st;
    if (n_rows && !d_feat) return fail(ctx, WSA_ERR_INVALID, "null feature pointer");
    if (slices > WSA_KNN_SPLIT_MAX_SLICES || (uint64_t)slices * n_rows * (12ull * k + 4ull) > WSA_KNN_SPLIT_SCRATCH_BYTES)
        return fail(ctx, WSA_ERR_INVALID, std::to_string(slices) + " slices for " + std::to_string(n_rows) + " rows: K9s takes at most " + std::to_string(WSA_KNN_SPLIT_MAX_SLICES)
                                          + " slices and " + std::to_string(WSA_KNN_SPLIT_SCRATCH_BYTES) + " bytes of scratch");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    wsa_knn::DebugSplit& d = kn->debug_split;
    const uint32_t S = slices ? slices : knn_split_slices(kn, n_rows, k);
    if (!d.mem || d.sp.window < n_rows || d.sp.slices != S || d.k != k || d.count != kn->count) {
        HIP_TRY(ctx, hipStreamSynchronize(s));                 // an earlier call may still use the table that goes
        d.mem.reset(new wsa::DevArena());
        d.k = k; d.count = kn->count;
        if (!knn_split_alloc(*d.mem, kn, n_rows, k, S, d.sp)) { d.mem.reset(); return fail(ctx, WSA_ERR_HIP, std::string("device allocation failed: ") + hipGetErrorString(hipGetLastError())); }
    }
    KnnSplit sp = d.sp;
    sp.window = n_rows;
    KnnParams p = knn_params(kn, d_feat, n_rows, nullptr, k);
    p.label = d_label; p.conf = d_conf; p.nbr = d_nbr; p.sim = d_sim;
    launch_knn_split(kn, p, sp, s);
    HIP_TRY(ctx, hipGetLastError());
    return WSA_OK;
}

}  // extern "C"
