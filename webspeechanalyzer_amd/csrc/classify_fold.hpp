// classify_fold.hpp — K6b's device code: what the four fold kernels (fold_kernel and fold_group_kernel in classify_batch.hip,
// stream_classes_kernel and stream_fold_group_kernel in classify_stream.hip), stream_decide_kernel and KN-2's two (knn_fold.hip) share.  Stands in for the reference
// APPLICATION's src/prediction.js:86-169 (weights sqrt(duration), per-label sums, segment label, per-launch accumulator, the ensemble's
// decision); this is the part that must match the JavaScript bit for bit, so each piece is written once.  Device only; every
// translation unit that includes it gets its own copy.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "classify_internal.hpp"

namespace {
using namespace wsa_classify;

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

// ---- the callback walk: the rows of one clip or stream are in order, and rows with the same si form one callback
// the end of the callback that starts at row r (r < r1, the end of the clip's or stream's rows)
__device__ __forceinline__ uint32_t callback_end(const int32_t* meta, uint32_t r, uint32_t r1) {
    const int si = meta[(size_t)r * 8 + 1];
    uint32_t e = r + 1;
    while (e < r1 && meta[(size_t)e * 8 + 1] == si) e++;
    return e;
}
// A stream step writes callbacks straight to their place in the step's table: a stream's first callback index is the number of callback
// starts (a row whose stream or si differs from the row before) among the rows in front of it — a ballot over tens to hundreds of rows,
// instead of a scan kernel.
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
// callback k's record: {clip or stream, si, first row, syllables}
__device__ __forceinline__ void write_callback(int32_t* cb, uint32_t k, int32_t who, int32_t si, uint32_t r, int32_t nsyl) {
    cb[(size_t)k * 4 + 0] = who; cb[(size_t)k * 4 + 1] = si; cb[(size_t)k * 4 + 2] = (int32_t)r; cb[(size_t)k * 4 + 3] = nsyl;
}

// what one clip's (or stream's) fold carries from callback to callback, per lane = class
struct FoldAcc {
    double acc_all;                          // Label_conf_all[label]
    bool in_all;                             // the label is a key of Label_conf_all
    long long first;                         // its insertion stamp
    long long stamp;
};

// (a stream's fold between steps: CarriedFold, classify_internal.hpp)
__device__ __forceinline__ FoldAcc load_fold(const CarriedFold& c, uint32_t s, size_t sc, bool cls, bool start) {
    FoldAcc a{0.0, false, 0, 0};
    if (!start) {
        if (cls) { a.acc_all = c.acc_all[sc]; a.in_all = c.in_all[sc] != 0; a.first = c.first[sc]; }
        a.stamp = c.stamp[s];
    }
    return a;
}
__device__ __forceinline__ void store_fold(const CarriedFold& c, uint32_t s, size_t sc, bool cls, int lane, const FoldAcc& a) {
    if (cls) { c.acc_all[sc] = a.acc_all; c.in_all[sc] = a.in_all ? 1 : 0; c.first[sc] = a.first; }
    if (lane == 0) c.stamp[s] = a.stamp;
}

// one callback: rows r .. e - 1 (the same clip / stream and si); label -1 / -2 as wsa_class_result.  P is the type the confidences
// arrive in: float for a network's probabilities (K6), double for KNN's votes / k_eff (K9, specification KN-2); the sums are double.
template <typename P>
__device__ __forceinline__ void fold_callback(const int32_t* meta, const P* prob, uint32_t C, double step_s, int lane, bool cls, long long kr,
                                              uint32_t r, uint32_t e, FoldAcc& a, int& label, double& conf, double& seg_max) {
    const uint32_t nsyl = e - r;
    double seg_weight = 0.0;                 // sum of parseFloat(seg_time[ph][1]) (ref prediction.js:55)
    for (uint32_t q = r; q < e; q++) seg_weight += fixed3((double)(meta[(size_t)q * 8 + 3] + 1) * step_s);
    label = -2; conf = 0.0; seg_max = 0.0;
    if (!(seg_weight > 0.0)) return;
    double acc_seg = 0.0; bool in_seg = false;
    for (uint32_t q = r; q < e; q++) {
        const double w = __dsqrt_rn(fixed3((double)(meta[(size_t)q * 8 + 3] + 1) * step_s));
        const P pf = cls ? prob[(size_t)q * C + lane] : P(0);
        // rank in classifyMultiple's order: confidence descending, ties in legend order (a stable sort).  A row that is NaN throughout (K6's
        // answer to a non-finite feature) stays in legend order: ml5's comparator `b - a` answers NaN, which the sort reads as "not before",
        // so a NaN ranks behind the NaNs in front of it.  (A row that mixes NaN and numbers has no specified order; K6 produces none.)
        int rank = 0;
        for (int j = 0; j < (int)C; j++) {
            const P pj = __shfl(pf, j);
            rank += (pj > pf || ((pj == pf || (pj != pj && pf != pf)) && j < lane)) ? 1 : 0;
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
    const long long key = (kr >= 0) ? kr : ((1ll << 40) + a.first);
    const long long best = wave_min_ll((in_seg && a.in_all && v == mx && mx > 0.0) ? key : 0x7fffffffffffffffll);
    if (mx > 0.0) {
        const unsigned long long hit = __ballot(cls && in_seg && a.in_all && v == mx && key == best);
        label = (int)__ffsll(hit) - 1;
    } else label = -1;
    conf = mx / seg_weight;
    seg_max = mx;                            // DB_entropies_seg of this model DB (ref prediction.js:154)
}

// ---- K6b on a batch: one wave per clip, classes on lanes, callbacks walked in order (ref prediction.js:86-169 with one model DB); P as
// for fold_callback
template <typename P>
__global__ void __launch_bounds__(256) fold_kernel(FoldParams<P> p) {
    const int lane = threadIdx.x & 63;
    const uint32_t clip = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (clip >= p.n_clips) return;
    const uint32_t r0 = p.row_off[clip], r1 = p.row_off[clip + 1];
    const bool cls = (uint32_t)lane < p.C;
    const long long kr = cls ? (long long)p.key_rank[lane] : -1;
    FoldAcc a{0.0, false, 0, 0};
    uint32_t ncb = 0;
    for (uint32_t r = r0; r < r1;) {
        const uint32_t e = callback_end(p.meta, r, r1);
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
        write_callback(cb, k, clip, meta[(size_t)r * 8 + 1], r, nsyl);
        cb_label[k] = t_label[r]; cb_conf[k] = t_conf[r];
    }
    if (tid == 0) host[0] = n_cb;
}

// ---- the same fold on a stream step: one wave per stream with the stream's carried fold.  Callbacks are written straight to their place
// in the step's table (callback_starts); callbacks and the per-stream sums also go to the mapped pinned tables (callbacks below `cap`).
template <typename P>
__device__ __forceinline__ void fold_stream_step(const int32_t* meta, const P* prob, uint32_t C, double step_s, int lane, long long kr, uint32_t s, uint32_t n,
                                                 uint32_t r0, uint32_t r1, const CarriedFold& carried, bool start, const StepFoldTables& t) {
    const bool cls = (uint32_t)lane < C;
    const size_t sc = (size_t)s * C + lane;
    FoldAcc a = load_fold(carried, s, sc, cls, start);
    uint32_t k = callback_starts(meta, 0, r0, lane);
    for (uint32_t r = r0; r < r1;) {
        const int si = meta[(size_t)r * 8 + 1];
        const uint32_t e = callback_end(meta, r, r1);
        int label; double conf, seg_max;
        fold_callback(meta, prob, C, step_s, lane, cls, kr, r, e, a, label, conf, seg_max);
        if (lane == 0) {
            write_callback(t.cb, k, (int32_t)s, si, r, (int32_t)(e - r));
            t.cb_label[k] = label; t.cb_conf[k] = conf;
            if (k < t.cap) {
                write_callback(t.h_cb, k, (int32_t)s, si, r, (int32_t)(e - r));
                t.h_cb_label[k] = label; t.h_cb_conf[k] = conf;
            }
        }
        k++;
        r = e;
    }
    store_fold(carried, s, sc, cls, lane, a);
    if (cls) t.h_conf[sc] = a.acc_all;
    if (lane == 0 && s == n - 1) t.h_count[0] = k;
}

// ---- an ensemble (ref prediction.js:47-169 with several model DBs in available_DBs).  Besides what one model's fold writes, a callback
// leaves what seg_confidence_sort derives from each member's tables: DB_entropies_seg (the segment maximum), DB_entropies_all (the maximum
// of Label_conf_all, strict > from 0 in key order — a maximum does not depend on the order) and the sum plot_prediction_meters forms over
// Label_conf_all in Object.keys order (ref prediction.js:182-184).
__device__ __forceinline__ void all_max_and_sum(const FoldAcc& a, uint32_t C, int lane, bool cls, long long kr, double& all_max, double& all_sum) {
    const bool in = cls && a.in_all;
    all_max = wave_max_d((in && a.acc_all > 0.0) ? a.acc_all : 0.0);
    const long long key = (kr >= 0) ? kr : ((1ll << 40) + a.first);
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

// what one member's fold leaves of a callback for the decision; `of(d)` below yields member d's: a batch's fold keeps them in LDS, a
// stream step reads the members' step tables
struct MemberFigures { double seg; int label; double conf, all_max, all_sum; };

// The decision of seg_confidence_sort (ref prediction.js:127-169) for one callback, from the members' figures for it: the winner is the
// first member whose segment maximum exceeds the running one (from 0).  -1: no member has a sum above 0.
template <typename F>
__device__ __forceinline__ void ensemble_winner(const F& of, uint32_t n_members, int& db, int& top_label, double& top_conf) {
    double best = 0.0;
    db = -1; top_label = -1; top_conf = 0.0;
    for (uint32_t d = 0; d < n_members; d++) {
        const MemberFigures f = of(d);
        if (f.seg > best) { best = f.seg; db = (int)d; top_label = f.label; top_conf = f.conf; }   // max_conf_db_seg / seg_weight: the member's own quotient
    }
}

// min_entropy_db after one callback (ref prediction.js:161-165): updated only where a member's DB_entropies_all exceeds max_inv_entropy,
// which runs across the launch's callbacks; then the readout of plot_prediction_meters (ref prediction.js:207), NaN while there is no DB
template <typename F>
__device__ __forceinline__ double ensemble_min_db(const F& of, uint32_t n_members, bool skipped, double& max_inv, int& min_db) {
    if (!skipped)
        for (uint32_t d = 0; d < n_members; d++) {
            const double am = of(d).all_max;
            if (am > max_inv) { max_inv = am; min_db = (int)d; }
        }
    const double nan = __longlong_as_double(0x7ff8000000000000ll);
    if (min_db < 0) return nan;
    const double e = 1.0 - of(min_db).all_max / of(min_db).all_sum;
    return e == e ? e : nan;                 // JavaScript has one NaN ("Entropy: NaN" once a sum is NaN): one bit pattern here, whatever the subtraction leaves
}

}  // namespace
