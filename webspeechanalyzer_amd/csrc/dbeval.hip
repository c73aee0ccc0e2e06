// dbeval.hip — K8e: the evaluation of a labelled feature DB beyond the app's results table (specification EV-1), and its part
// of the C ABI (include/wsa_eval.h).  Works on a wsa_dbstats object (dbstats.hip, DS-1) and reads the columns DS-1 counts; it writes none
// of them and nothing wsa_dbstats_table uses.
//
// The confusion matrix of one categorical head, V x (V + 1) counters (column V: blank predictions), two launches:
//   group    pass 1    The matrix of V = 256 is 256 x 257 counters: too many for one workgroup's LDS, and a slab of it per 256-row chunk
//                      would be 263 KB per chunk (387 MB at the app's 376 634 rows).  So the partials are sized from both ends.  A
//                      workgroup owns a BAND of EV_BAND = 32 true classes, 32 x 257 u32 = 32.9 KB of LDS at most, and a GROUP of
//                      consecutive chunks: the chunks are dealt to at most EV_GROUPS = 64 groups (ceil(n_chunks / 64) chunks each), so the
//                      slabs are at most 64 x V (V + 1) u32 = 16.8 MB whatever the row count, and a V = 8 head's are 18 KB.  The
//                      workgroup walks its group chunk by chunk, one row per thread; a row whose true class lies in the band adds 1
//                      to its cell with an integer atomic in LDS; the band is stored to the group's slab.  ceil(V / 32) bands re-read the
//                      two index columns (8 bytes per row).  A cell holds at most the group's rows, below 2^32.
//   sum      pass 2    one thread per cell adds the groups' slabs in group order into a u64.
// Counts are integers, so any order gives the same matrix; the grid is a function of (n_rows, V) alone all the same.
//
// The agreement of the ordinal heads, four launches, every f64 sum in DS-1's order (rows of a 256-row chunk in row order, one owner lane
// per head; then chunks in chunk order, one owner per head):
//   sums     pass 1    per chunk and head: n, sum t, sum p over the rows whose t and p both pass v == v && v != 0
//   means    pass 2    per head: the chunk partials in chunk order; mean = sum / n, left in device memory
//   central  pass 3    per chunk and head: sum (t - mt)^2, sum (p - mp)^2, sum (t - mt)(p - mp); means read from device memory.  No
//                      product is fused into its addition (contraction is off; the restatement rounds each product, as JavaScript does)
//   quotient pass 4    per head: chunk order again; / n, then ccc and pearson.  A NaN leaves as the one quiet NaN 0x7ff8000000000000.
// No floating-point atomics, no tickets, no fences: the next launch is the ordering.
#include <cmath>
#include <string>
#include <vector>
#include "dbstats_internal.hpp"
#include "regress_fold.hpp"

#pragma clang fp contract(off)

using wsa_api::fail;
using namespace wsa_dbstats_detail;

namespace {

constexpr uint32_t EV_BAND = 32;           // true classes per workgroup of the confusion's pass 1
constexpr uint32_t EV_GROUPS = 64;         // groups of consecutive chunks at most

struct EvConf {
    uint32_t n_rows, n_chunks, per_group, n_groups, V;
    const int32_t *t, *p;
    uint32_t* slab;       // [n_groups][V][V + 1]
    uint64_t* out;        // [V][V + 1]
};

__global__ void __launch_bounds__(DS_THREADS) dbeval_confusion_group_kernel(EvConf p) {
    extern __shared__ uint32_t ev_cnt[];                    // [rows of the band][V + 1]
    const uint32_t tid = threadIdx.x, group = blockIdx.x, W = p.V + 1;
    const uint32_t b0 = blockIdx.y * EV_BAND, nb = p.V - b0 < EV_BAND ? p.V - b0 : EV_BAND, cells = nb * W;
    for (uint32_t i = tid; i < cells; i += DS_THREADS) ev_cnt[i] = 0;
    __syncthreads();
    const uint32_t c0 = group * p.per_group, c1 = c0 + p.per_group < p.n_chunks ? c0 + p.per_group : p.n_chunks;
    for (uint32_t c = c0; c < c1; c++) {
        const uint64_t r = (uint64_t)c * DS_R + tid;
        if (r >= p.n_rows) continue;
        const int32_t t = p.t[r];
        if (t < (int32_t)b0 || t >= (int32_t)(b0 + nb)) continue;          // not this band's, or a row that does not count (-1)
        const int32_t q = p.p[r];
        const uint32_t col = (uint32_t)q < p.V ? (uint32_t)q : p.V;       // blank (-1) -> column V
        atomicAdd(&ev_cnt[((uint32_t)t - b0) * W + col], 1u);
    }
    __syncthreads();
    uint32_t* slab = p.slab + (size_t)group * p.V * W + (size_t)b0 * W;
    for (uint32_t i = tid; i < cells; i += DS_THREADS) slab[i] = ev_cnt[i];
}

__global__ void __launch_bounds__(DS_THREADS) dbeval_confusion_sum_kernel(EvConf p) {
    const uint32_t cells = p.V * (p.V + 1), i = blockIdx.x * DS_THREADS + threadIdx.x;
    if (i >= cells) return;
    unsigned long long s = 0;
    for (uint32_t g = 0; g < p.n_groups; g++) s += p.slab[(size_t)g * cells + i];
    p.out[i] = s;
}

struct EvAgree {
    uint32_t n_rows, n_chunks, n_ord;
    const double *t[DS_H], *p[DS_H];
    uint32_t* part_n;     // [n_ord][n_chunks]
    double* part;         // [n_ord][3][n_chunks]
    double* mean;         // [n_ord][2] true, predicted
    uint64_t* count;      // [n_ord]
    wsa_dbstats_agree* out;
};

__device__ __forceinline__ bool ev_counted(double v) { return v == v && v != 0.0; }
__device__ __forceinline__ double ev_one_nan(double v) { return v == v ? v : __longlong_as_double(0x7ff8000000000000ll); }

// passes 1 (CENTRAL = false) and 3 (true): one workgroup per chunk, the chunk's two columns per head staged in LDS, lane o owns head o
template <bool CENTRAL>
__global__ void __launch_bounds__(DS_THREADS) dbeval_agree_chunk_kernel(EvAgree p) {
    extern __shared__ double ev_lds[];                      // [n_ord][2][DS_R]
    const uint32_t chunk = blockIdx.x, tid = threadIdx.x, r0 = chunk * DS_R;
    const uint32_t rows = p.n_rows - r0 < (uint32_t)DS_R ? p.n_rows - r0 : (uint32_t)DS_R;
    const uint64_t r = (uint64_t)r0 + tid;
    for (uint32_t o = 0; o < p.n_ord; o++) {
        ev_lds[(o * 2 + 0) * DS_R + tid] = tid < rows ? p.t[o][r] : 0.0;
        ev_lds[(o * 2 + 1) * DS_R + tid] = tid < rows ? p.p[o][r] : 0.0;
    }
    __syncthreads();
    if (tid >= p.n_ord) return;
    const double* tv = ev_lds + (tid * 2 + 0) * DS_R; const double* pv = ev_lds + (tid * 2 + 1) * DS_R;
    double* part = p.part + (size_t)tid * 3 * p.n_chunks;
    if (!CENTRAL) {
        uint32_t n = 0;
        double st = 0.0, sp = 0.0;
        for (uint32_t i = 0; i < rows; i++) {
            const double t = tv[i], q = pv[i];
            if (!(ev_counted(t) && ev_counted(q))) continue;
            n++; st += t; sp += q;
        }
        p.part_n[(size_t)tid * p.n_chunks + chunk] = n;
        part[chunk] = st; part[p.n_chunks + chunk] = sp;
    } else {
        const double mt = p.mean[tid * 2 + 0], mp = p.mean[tid * 2 + 1];
        double a = 0.0, b = 0.0, c = 0.0;
        for (uint32_t i = 0; i < rows; i++) {
            const double t = tv[i], q = pv[i];
            if (!(ev_counted(t) && ev_counted(q))) continue;
            const double dt = t - mt, dp = q - mp;
            const double tt = dt * dt, pp = dp * dp, tp = dt * dp;          // each product rounded before it is added
            a += tt; b += pp; c += tp;
        }
        part[chunk] = a; part[p.n_chunks + chunk] = b; part[2 * (size_t)p.n_chunks + chunk] = c;
    }
}

// passes 2 and 4: one workgroup per head; the chunk partials pass through LDS 256 at a time and thread 0, their one owner, adds them in
// chunk order
template <bool CENTRAL>
__global__ void __launch_bounds__(DS_THREADS) dbeval_agree_sum_kernel(EvAgree p) {
    __shared__ double s_f[3][DS_THREADS];
    __shared__ uint32_t s_n[DS_THREADS];
    const uint32_t o = blockIdx.x, tid = threadIdx.x;
    const double* part = p.part + (size_t)o * 3 * p.n_chunks;
    unsigned long long n = 0;
    double a = 0.0, b = 0.0, c = 0.0;
    for (uint32_t c0 = 0; c0 < p.n_chunks; c0 += DS_THREADS) {
        const uint32_t k = c0 + tid, m = p.n_chunks - c0 < (uint32_t)DS_THREADS ? p.n_chunks - c0 : (uint32_t)DS_THREADS;
        if (k < p.n_chunks) {
            s_f[0][tid] = part[k]; s_f[1][tid] = part[p.n_chunks + k];
            s_f[2][tid] = CENTRAL ? part[2 * (size_t)p.n_chunks + k] : 0.0;
            s_n[tid] = CENTRAL ? 0u : p.part_n[(size_t)o * p.n_chunks + k];
        }
        __syncthreads();
        if (tid == 0) for (uint32_t i = 0; i < m; i++) { a += s_f[0][i]; b += s_f[1][i]; c += s_f[2][i]; n += s_n[i]; }
        __syncthreads();
    }
    if (tid != 0) return;
    if (!CENTRAL) {
        const double dn = (double)n;
        p.count[o] = n; p.mean[o * 2 + 0] = a / dn; p.mean[o * 2 + 1] = b / dn;
        return;
    }
    const double dn = (double)p.count[o], mt = p.mean[o * 2 + 0], mp = p.mean[o * 2 + 1];
    const double vt = a / dn, vp = b / dn, cov = c / dn;
    const double d = mp - mt, dd = d * d, den = (vt + vp) + dd, two = 2.0 * cov, prod = vt * vp;
    wsa_dbstats_agree e;
    e.n = p.count[o];
    e.mean_true = ev_one_nan(mt); e.mean_pred = ev_one_nan(mp); e.var_true = ev_one_nan(vt); e.var_pred = ev_one_nan(vp); e.cov = ev_one_nan(cov);
    e.ccc = ev_one_nan(two / den);
    e.pearson = ev_one_nan(cov / __dsqrt_rn(prod));
    p.out[o] = e;
}


// ---- per file.  The rows that belong to a file are SELECTED (sel, in row order) and the tables K6b and RG-1 walk are built for the
// selection once (wsa_dbstats_set_files): meta [.][8] with the file where a batch has the clip, the callback index where it has si, and
// whole milliseconds - 1 where it has t_len, so that with step_s = 1e-3 fixed3((t_len + 1) step_s) is the stored duration itself.
__global__ void __launch_bounds__(DS_THREADS) dbeval_gather_prob_kernel(const uint32_t* sel, uint32_t n_sel, uint32_t C, const float* prob, float* out) {
    const uint64_t i = (uint64_t)blockIdx.x * DS_THREADS + threadIdx.x;
    if (i >= (uint64_t)n_sel * C) return;
    out[i] = prob[(size_t)sel[i / C] * C + i % C];
}
__global__ void __launch_bounds__(DS_THREADS) dbeval_gather_value_kernel(const uint32_t* sel, uint32_t n_sel, const double* value, double* out) {
    const uint32_t i = blockIdx.x * DS_THREADS + threadIdx.x;
    if (i < n_sel) out[i] = value[sel[i]];
}

struct EvFold {
    uint32_t n_files, C; double step_s;
    const int32_t* meta; const uint32_t* row_off; const float* prob; const int64_t* key_rank; const int32_t* map;
    double* sums;         // [n_files][C] Label_conf_all at the file's end
    int32_t* pred;        // [n_files] vocabulary index, -1 blank
};

// K6b with a file where fold_kernel (classify_fold.hpp) has a clip: one wave per file, classes on lanes, fold_callback per callback.  What
// is ours is the file's class: the largest meter sum above 0, the first in the fold's own key order on a tie (seg_confidence_sort takes
// the same strict > from 0 over Label_conf_all but keeps only the maximum), through legend_to_vocab; blank when no sum is above 0.
__global__ void __launch_bounds__(DS_THREADS) dbeval_fold_files_kernel(EvFold p) {
    const int lane = threadIdx.x & 63;
    const uint32_t file = blockIdx.x * (DS_THREADS / 64) + (threadIdx.x >> 6);
    if (file >= p.n_files) return;
    const uint32_t r0 = p.row_off[file], r1 = p.row_off[file + 1];
    const bool cls = (uint32_t)lane < p.C;
    const long long kr = cls ? (long long)p.key_rank[lane] : -1;
    FoldAcc a{0.0, false, 0, 0};
    for (uint32_t r = r0; r < r1;) {
        const uint32_t e = callback_end(p.meta, r, r1);
        int label; double conf, seg_max;
        fold_callback(p.meta, p.prob, p.C, p.step_s, lane, cls, kr, r, e, a, label, conf, seg_max);
        r = e;
    }
    const bool in = cls && a.in_all;
    const double v = (in && a.acc_all > 0.0) ? a.acc_all : 0.0;
    const double mx = wave_max_d(v);
    const long long key = (kr >= 0) ? kr : ((1ll << 40) + a.first);
    const bool top = in && mx > 0.0 && v == mx;
    const long long best = wave_min_ll(top ? key : 0x7fffffffffffffffll);
    const unsigned long long hit = __ballot(top && key == best);
    if (cls) p.sums[(size_t)file * p.C + lane] = a.acc_all;
    if (lane == 0) p.pred[file] = hit ? p.map[__ffsll(hit) - 1] : -1;
}

struct EvFoldValue {
    double step_s;
    const int32_t* meta; const uint32_t* row_off; const double* value[1];
    double* out;          // [n_files]
};

// RG-1 with a file where regress_fold_kernel has a clip: the running value at the file's end, sum v sqrt(d) / sum sqrt(d) over the
// file's rows with a finite v, callback by callback (a callback whose durations sum to 0 adds nothing); NaN when no row added
__global__ void __launch_bounds__(64) dbeval_fold_file_values_kernel(EvFoldValue p) {
    __shared__ double s_terms[RG_LDS];
    const int lane = threadIdx.x;
    const uint32_t file = blockIdx.x;
    double A = 0.0, B = 0.0;
    regress_walk(p.meta, p.value, 1u, p.step_s, lane, p.row_off[file], p.row_off[file + 1], s_terms, nullptr, A, B,
                 [](uint32_t, uint32_t, uint32_t, bool, double, double) {});
    if (lane == 0) p.out[file] = B == 0.0 ? nan_d() : A / B;
}

wsa_status need_files(wsa_dbstats* db) {
    if (!db->eval.files) return fail(db->ctx, WSA_ERR_INVALID, "the DB's rows have no files yet: wsa_dbstats_set_files");
    return WSA_OK;
}

}  // namespace

extern "C" {

wsa_status wsa_dbstats_confusion(wsa_dbstats* db, uint32_t head, void* stream, uint64_t* m) {
    if (!db) return WSA_ERR_INVALID;
    wsa_ctx* ctx = db->ctx;
    if (const wsa_status st = check_head(db, head, true)) return st;
    if (!m) return fail(ctx, WSA_ERR_INVALID, "null argument");
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    DsEval& ev = db->eval;
    if (!ev.d_conf) {                                        // sized for the largest head, once
        uint32_t cells = 0;
        for (uint32_t h = 0; h < db->n_cat; h++) { const uint32_t V = db->voff[h + 1] - db->voff[h]; if (V * (V + 1) > cells) cells = V * (V + 1); }
        const uint32_t groups = db->n_chunks < EV_GROUPS ? db->n_chunks : EV_GROUPS;
        uint32_t* slab = nullptr; uint64_t* out = nullptr;
        if (!(db->mem.alloc(&slab, (size_t)groups * cells) && db->mem.alloc(&out, cells)))
            return fail(ctx, WSA_ERR_HIP, std::string("device allocation failed: ") + hipGetErrorString(hipGetLastError()));
        ev.conf_groups = groups; ev.conf_cells = cells; ev.d_conf_slab = slab; ev.d_conf = out;
    }
    EvConf p{};
    p.n_rows = db->n_rows; p.n_chunks = db->n_chunks; p.V = db->voff[head + 1] - db->voff[head];
    p.per_group = (db->n_chunks + EV_GROUPS - 1) / EV_GROUPS;
    p.n_groups = (db->n_chunks + p.per_group - 1) / p.per_group;            // <= conf_groups
    p.t = db->d_t_idx[head]; p.p = db->d_p_idx[head]; p.slab = ev.d_conf_slab; p.out = ev.d_conf;
    const uint32_t cells = p.V * (p.V + 1), bands = (p.V + EV_BAND - 1) / EV_BAND, band_rows = p.V < EV_BAND ? p.V : EV_BAND;
    hipLaunchKernelGGL(dbeval_confusion_group_kernel, dim3(p.n_groups, bands), dim3(DS_THREADS), (size_t)band_rows * (p.V + 1) * sizeof(uint32_t), s, p);
    hipLaunchKernelGGL(dbeval_confusion_sum_kernel, dim3((cells + DS_THREADS - 1) / DS_THREADS), dim3(DS_THREADS), 0, s, p);
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipMemcpyAsync(m, ev.d_conf, (size_t)cells * sizeof(uint64_t), hipMemcpyDeviceToHost, s));
    HIP_TRY(ctx, hipStreamSynchronize(s));
    return WSA_OK;
}

wsa_status wsa_dbstats_agreement(wsa_dbstats* db, void* stream, wsa_dbstats_agree* out) {
    if (!db) return WSA_ERR_INVALID;
    wsa_ctx* ctx = db->ctx;
    if (!db->n_ord) return fail(ctx, WSA_ERR_INVALID, "the DB has no ordinal head");
    if (!out) return fail(ctx, WSA_ERR_INVALID, "null argument");
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    DsEval& ev = db->eval;
    if (!ev.d_agree) {
        uint32_t* pn = nullptr; double *part = nullptr, *mean = nullptr; uint64_t* count = nullptr; wsa_dbstats_agree* res = nullptr;
        if (!(db->mem.alloc(&pn, (size_t)db->n_ord * db->n_chunks) && db->mem.alloc(&part, (size_t)db->n_ord * 3 * db->n_chunks)
              && db->mem.alloc(&mean, (size_t)db->n_ord * 2) && db->mem.alloc(&count, db->n_ord) && db->mem.alloc(&res, db->n_ord, true)))
            return fail(ctx, WSA_ERR_HIP, std::string("device allocation failed: ") + hipGetErrorString(hipGetLastError()));
        ev.d_agree_n = pn; ev.d_agree_part = part; ev.d_agree_mean = mean; ev.d_agree_count = count; ev.d_agree = res;
    }
    EvAgree p{};
    p.n_rows = db->n_rows; p.n_chunks = db->n_chunks; p.n_ord = db->n_ord;
    for (int h = 0; h < DS_H; h++) { p.t[h] = db->d_t_val[h]; p.p[h] = db->d_p_val[h]; }
    p.part_n = ev.d_agree_n; p.part = ev.d_agree_part; p.mean = ev.d_agree_mean; p.count = ev.d_agree_count; p.out = ev.d_agree;
    const size_t lds = (size_t)db->n_ord * 2 * DS_R * sizeof(double);
    hipLaunchKernelGGL(dbeval_agree_chunk_kernel<false>, dim3(db->n_chunks), dim3(DS_THREADS), lds, s, p);
    hipLaunchKernelGGL(dbeval_agree_sum_kernel<false>, dim3(db->n_ord), dim3(DS_THREADS), 0, s, p);
    hipLaunchKernelGGL(dbeval_agree_chunk_kernel<true>, dim3(db->n_chunks), dim3(DS_THREADS), lds, s, p);
    hipLaunchKernelGGL(dbeval_agree_sum_kernel<true>, dim3(db->n_ord), dim3(DS_THREADS), 0, s, p);
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipMemcpyAsync(out, ev.d_agree, (size_t)db->n_ord * sizeof(wsa_dbstats_agree), hipMemcpyDeviceToHost, s));
    HIP_TRY(ctx, hipStreamSynchronize(s));
    return WSA_OK;
}


wsa_status wsa_dbstats_set_files(wsa_dbstats* db, const int32_t* file_of_row, const int32_t* callback_of_row, uint32_t n_files) {
    if (!db) return WSA_ERR_INVALID;
    wsa_ctx* ctx = db->ctx;
    if (!file_of_row || !callback_of_row) return fail(ctx, WSA_ERR_INVALID, "null argument");
    if (n_files == 0) return fail(ctx, WSA_ERR_INVALID, "a DB evaluated per file has at least one file");
    DsEval& ev = db->eval;
    if (ev.files) return fail(ctx, WSA_ERR_INVALID, "the DB's files are set already; they are set once");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    std::vector<double> dur(db->n_rows);
    HIP_TRY(ctx, hipMemcpy(dur.data(), db->d_dur, (size_t)db->n_rows * sizeof(double), hipMemcpyDeviceToHost));
    // everything is checked before anything is kept: a refusal leaves the object as it was
    std::vector<uint32_t> sel, row_off(n_files + 1, 0);
    std::vector<int32_t> meta;
    std::vector<double> file_dur(n_files, 0.0);
    int32_t last = -1; uint32_t last_row = 0;
    for (uint32_t r = 0; r < db->n_rows; r++) {
        const int32_t f = file_of_row[r];
        if (f < -1 || (f >= 0 && (uint32_t)f >= n_files))
            return fail(ctx, WSA_ERR_INVALID, "file " + std::to_string(f) + " of row " + std::to_string(r) + " is outside -1 .. " + std::to_string(n_files - 1));
        if (f < 0) continue;
        if (f < last)
            return fail(ctx, WSA_ERR_INVALID, "file_of_row is not non-decreasing: row " + std::to_string(r) + " has file " + std::to_string(f) + " after file "
                                              + std::to_string(last) + " of row " + std::to_string(last_row));
        const double d = dur[r], k = std::nearbyint(d * 1000.0);
        if (!(d >= 0.0) || !(k <= 2147483647.0) || k / 1000.0 != d)
            return fail(ctx, WSA_ERR_INVALID, "the duration " + std::to_string(d) + " of row " + std::to_string(r) + " is not a whole number of milliseconds (0 .. 2147483647)");
        last = f; last_row = r;
        sel.push_back(r);
        const int32_t m[8] = {f, callback_of_row[r], 0, (int32_t)((long long)k - 1), 0, 0, 0, 0};
        meta.insert(meta.end(), m, m + 8);
        row_off[(size_t)f + 1]++;
        file_dur[f] += d;                                    // a file's duration: its rows' in row order
    }
    for (uint32_t f = 0; f < n_files; f++) row_off[f + 1] += row_off[f];
    std::vector<uint32_t> vocab(db->n_cat ? db->n_cat : 1, 1);
    for (uint32_t h = 0; h < db->n_cat; h++) vocab[h] = db->voff[h + 1] - db->voff[h];
    wsa_dbstats* files = nullptr;
    if (const wsa_status st = wsa_wide_dbstats_create(ctx, nullptr, db->n_feat, file_dur.data(), n_files, db->n_cat, vocab.data(), db->n_ord, &files)) return st;
    const size_t n_sel = sel.size();
    uint32_t *d_sel = nullptr, *d_off = nullptr; int32_t *d_meta = nullptr, *d_map = nullptr; double* d_val = nullptr;
    if (!(db->mem.upload(&d_sel, sel) && db->mem.upload(&d_off, row_off) && db->mem.upload(&d_meta, meta) && db->mem.alloc(&d_val, n_sel)
          && db->mem.alloc(&d_map, (size_t)WSA_MODEL_MAX_CLASSES))) {
        const std::string msg = std::string("device allocation / copy failed: ") + hipGetErrorString(hipGetLastError());
        wsa_dbstats_destroy(files);
        return fail(ctx, WSA_ERR_HIP, msg);
    }
    ev.files = files; ev.n_files = n_files; ev.n_sel = (uint32_t)n_sel;
    ev.d_sel = d_sel; ev.d_row_off = d_off; ev.d_meta = d_meta; ev.d_sel_val = d_val; ev.d_map = d_map;
    return WSA_OK;
}

wsa_status wsa_dbstats_set_file_classes(wsa_dbstats* db, uint32_t head, const int32_t* true_idx) {
    if (!db) return WSA_ERR_INVALID;
    wsa_ctx* ctx = db->ctx;
    if (const wsa_status st = need_files(db)) return st;
    if (const wsa_status st = check_head(db, head, true)) return st;
    if (!true_idx) return fail(ctx, WSA_ERR_INVALID, "null true_idx");
    const int32_t V = (int32_t)(db->voff[head + 1] - db->voff[head]);
    for (uint32_t f = 0; f < db->eval.n_files; f++)
        if (true_idx[f] < -1 || true_idx[f] >= V)
            return fail(ctx, WSA_ERR_INVALID, "true class " + std::to_string(true_idx[f]) + " of file " + std::to_string(f) + " is outside -1 .. " + std::to_string(V - 1));
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipMemcpy(db->eval.files->d_t_idx[head], true_idx, (size_t)db->eval.n_files * sizeof(int32_t), hipMemcpyHostToDevice));   // the predicted column stays
    return WSA_OK;
}

wsa_status wsa_dbstats_set_file_values(wsa_dbstats* db, uint32_t head, const double* true_value) {
    if (!db) return WSA_ERR_INVALID;
    wsa_ctx* ctx = db->ctx;
    if (const wsa_status st = need_files(db)) return st;
    if (const wsa_status st = check_head(db, head, false)) return st;
    if (!true_value) return fail(ctx, WSA_ERR_INVALID, "null true_value");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipMemcpy(db->eval.files->d_t_val[head], true_value, (size_t)db->eval.n_files * sizeof(double), hipMemcpyHostToDevice));
    return WSA_OK;
}

wsa_status wsa_dbstats_fold_files(wsa_dbstats* db, uint32_t head, void* stream) {
    if (!db) return WSA_ERR_INVALID;
    wsa_ctx* ctx = db->ctx;
    if (const wsa_status st = need_files(db)) return st;
    if (const wsa_status st = check_head(db, head, true)) return st;
    if (!db->d_prob || !db->prob_classes || db->prob_head < 0) return fail(ctx, WSA_ERR_INVALID, "no class prediction has run on this DB yet: wsa_dbstats_predict_classes");
    if ((uint32_t)db->prob_head != head)
        return fail(ctx, WSA_ERR_INVALID, "the kept probabilities are those of categorical head " + std::to_string(db->prob_head) + ", not of head " + std::to_string(head)
                                          + ": fold a head right after its wsa_dbstats_predict_classes");
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    DsEval& ev = db->eval;
    const uint32_t C = db->prob_classes;
    // both tables are as wide as the model has classes (the shipped 8-class model: an eighth of 64).  A later fold with a wider model takes a
    // new table; the narrower one stays with the object (work enqueued before may still read it) and goes with it.
    if (C > ev.sel_prob_width) {
        float* q = nullptr;
        if (!db->mem.alloc(&q, (size_t)ev.n_sel * C)) return fail(ctx, WSA_ERR_HIP, std::string("device allocation failed: ") + hipGetErrorString(hipGetLastError()));
        ev.d_sel_prob = q; ev.sel_prob_width = C;
    }
    if (C > ev.file_sums_width[head]) {
        double* q = nullptr;
        if (!db->mem.alloc(&q, (size_t)ev.n_files * C)) return fail(ctx, WSA_ERR_HIP, std::string("device allocation failed: ") + hipGetErrorString(hipGetLastError()));
        ev.d_file_sums[head] = q; ev.file_sums_width[head] = C;
    }
    HIP_TRY(ctx, hipMemcpyAsync(ev.d_map, db->prob_map, sizeof(db->prob_map), hipMemcpyHostToDevice, s));
    const uint64_t cells = (uint64_t)ev.n_sel * C;
    if (cells) hipLaunchKernelGGL(dbeval_gather_prob_kernel, dim3((uint32_t)((cells + DS_THREADS - 1) / DS_THREADS)), dim3(DS_THREADS), 0, s, ev.d_sel, ev.n_sel, C, db->d_prob, ev.d_sel_prob);
    EvFold p{};
    p.n_files = ev.n_files; p.C = C; p.step_s = 1e-3;
    p.meta = ev.d_meta; p.row_off = ev.d_row_off; p.prob = ev.d_sel_prob; p.key_rank = db->d_prob_key_rank; p.map = ev.d_map;
    p.sums = ev.d_file_sums[head]; p.pred = ev.files->d_p_idx[head];
    hipLaunchKernelGGL(dbeval_fold_files_kernel, dim3((ev.n_files + 3) / 4), dim3(DS_THREADS), 0, s, p);
    HIP_TRY(ctx, hipGetLastError());
    ev.file_classes[head] = C;
    return WSA_OK;
}

wsa_status wsa_dbstats_fold_file_values(wsa_dbstats* db, uint32_t head, void* stream) {
    if (!db) return WSA_ERR_INVALID;
    wsa_ctx* ctx = db->ctx;
    if (const wsa_status st = need_files(db)) return st;
    if (const wsa_status st = check_head(db, head, false)) return st;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    DsEval& ev = db->eval;
    if (ev.n_sel) hipLaunchKernelGGL(dbeval_gather_value_kernel, dim3((ev.n_sel + DS_THREADS - 1) / DS_THREADS), dim3(DS_THREADS), 0, s, ev.d_sel, ev.n_sel, db->d_p_val[head], ev.d_sel_val);
    EvFoldValue p{};
    p.step_s = 1e-3; p.meta = ev.d_meta; p.row_off = ev.d_row_off; p.value[0] = ev.d_sel_val; p.out = ev.files->d_p_val[head];
    hipLaunchKernelGGL(dbeval_fold_file_values_kernel, dim3(ev.n_files), dim3(64), 0, s, p);
    HIP_TRY(ctx, hipGetLastError());
    return WSA_OK;
}

wsa_status wsa_dbstats_file_table(wsa_dbstats* db, void* stream, wsa_dbstats_cat* cat, wsa_dbstats_class* cls, wsa_dbstats_ord* ord) {
    if (!db) return WSA_ERR_INVALID;
    if (const wsa_status st = need_files(db)) return st;
    return wsa_dbstats_table(db->eval.files, stream, cat, cls, ord);
}

wsa_status wsa_dbstats_file_confusion(wsa_dbstats* db, uint32_t head, void* stream, uint64_t* m) {
    if (!db) return WSA_ERR_INVALID;
    if (const wsa_status st = need_files(db)) return st;
    return wsa_dbstats_confusion(db->eval.files, head, stream, m);
}

wsa_status wsa_dbstats_file_agreement(wsa_dbstats* db, void* stream, wsa_dbstats_agree* out) {
    if (!db) return WSA_ERR_INVALID;
    if (const wsa_status st = need_files(db)) return st;
    return wsa_dbstats_agreement(db->eval.files, stream, out);
}

wsa_status wsa_dbstats_copy_file_sums(wsa_dbstats* db, uint32_t head, void* stream, double* sums, uint32_t n_classes) {
    if (!db) return WSA_ERR_INVALID;
    wsa_ctx* ctx = db->ctx;
    if (const wsa_status st = need_files(db)) return st;
    if (const wsa_status st = check_head(db, head, true)) return st;
    if (!sums) return fail(ctx, WSA_ERR_INVALID, "null argument");
    const DsEval& ev = db->eval;
    if (!ev.file_classes[head]) return fail(ctx, WSA_ERR_INVALID, "categorical head " + std::to_string(head) + " has not been folded per file yet: wsa_dbstats_fold_files");
    if (n_classes != ev.file_classes[head])
        return fail(ctx, WSA_ERR_INVALID, "the head was folded with a model of " + std::to_string(ev.file_classes[head]) + " classes, not " + std::to_string(n_classes));
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipMemcpyAsync(sums, ev.d_file_sums[head], (size_t)ev.n_files * n_classes * sizeof(double), hipMemcpyDeviceToHost, s));
    HIP_TRY(ctx, hipStreamSynchronize(s));
    return WSA_OK;
}

wsa_status wsa_dbstats_copy_file_classes(wsa_dbstats* db, uint32_t head, void* stream, int32_t* pred_idx) {
    if (!db) return WSA_ERR_INVALID;
    if (const wsa_status st = need_files(db)) return st;
    return wsa_dbstats_copy_classes(db->eval.files, head, stream, pred_idx);
}

wsa_status wsa_dbstats_copy_file_values(wsa_dbstats* db, uint32_t head, void* stream, double* pred_value) {
    if (!db) return WSA_ERR_INVALID;
    if (const wsa_status st = need_files(db)) return st;
    return wsa_dbstats_copy_values(db->eval.files, head, stream, pred_value);
}

}  // extern "C"
