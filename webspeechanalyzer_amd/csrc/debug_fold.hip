// debug_fold.hip — test entries of libwsa that are NOT part of include/wsa.h, for the per-callback folds: RG-1 (csrc/regress_fold.hpp: launch_regress_fold,
// launch_regress_step) and K6b / K6b-e (csrc/classify_fold.hpp through classify_internal.hpp's launch_fold, launch_fold_group, launch_stream_classes,
// launch_stream_knn, launch_stream_ensemble).  Hand-built rows in, the product's own launches, the tables back whole.  Both folds read their row
// tables through ONE host walk (RowWalk).
#include <vector>
#include "api_internal.hpp"
#include "debug_internal.hpp"
#include "regress_internal.hpp"
#include "classify_internal.hpp"

using namespace wsa_debug;

namespace {
// the folds' row tables, walked once on the host: row_off [tables][n + 1] counts from each table's first row (one table for a batch, one per step for
// streams), meta [n_rows][8].  Every table: offsets in order, rows of their own clip / stream, t_len neither negative nor INT32_MAX; callbacks counted.
struct RowWalk {
    uint64_t rows = 0, callbacks = 0;
    std::vector<uint64_t> step_row0, step_cb0;      // [tables + 1]: the rows / callbacks in front of table k
    std::vector<uint32_t> bits;                     // [tables][n]: the device control word's bit 0, WSA_STREAM_START of ctl (a batch: zeros)
    // class_rules: the class fold's two own refusals, a negative si and a stream's callback whose rows continue in the next step.  false: refused
    bool walk(const int32_t* meta, const uint32_t* row_off, const uint8_t* ctl, uint32_t n, uint32_t n_steps, uint32_t n_rows, uint32_t cb_cap, bool class_rules) {
        const uint32_t tables = n_steps ? n_steps : 1;
        step_row0.assign(tables + 1, 0); step_cb0.assign(tables + 1, 0);
        bits.assign((size_t)tables * n, 0u);
        for (size_t i = 0; n_steps && i < bits.size(); i++) bits[i] = (ctl[i] & WSA_STREAM_START) ? 1u : 0u;
        std::vector<int64_t> last_si(n, -1);                            // the si a stream's rows ended on in an earlier step of its launch; -1: none
        for (uint32_t k = 0; k < tables; k++) {
            const uint32_t* off = row_off + (size_t)k * (n + 1);
            if (off[0] != 0) return false;
            for (uint32_t c = 0; c < n; c++) if (off[c + 1] < off[c]) return false;
            if (rows + off[n] > n_rows) return false;
            for (uint32_t c = 0; c < n; c++) {
                if (bits[(size_t)k * n + c]) last_si[c] = -1;
                for (uint32_t r = off[c]; r < off[c + 1]; r++) {
                    const int32_t* m = meta + (rows + r) * 8;
                    if (m[0] != (int32_t)c || (class_rules && m[1] < 0) || m[3] < 0 || m[3] == 0x7fffffff) return false;
                    if (class_rules && r == off[c] && (int64_t)m[1] == last_si[c]) return false;       // a callback's rows split across steps
                    callbacks += (r == off[c] || m[1] != m[1 - 8]) ? 1 : 0;
                }
                if (n_steps && off[c + 1] > off[c]) last_si[c] = meta[(rows + off[c + 1] - 1) * 8 + 1];
            }
            rows += off[n];
            step_row0[k + 1] = rows; step_cb0[k + 1] = callbacks;
        }
        return rows == n_rows && callbacks <= cb_cap;
    }
};
}  // namespace

// RG-1 (csrc/regress_fold.hpp) on its own: hand-built row meta [n_rows][8] i32 (slot 0 the clip or stream, 1 si, 3 len) and H value columns
// values [H][n_rows] f64 straight into the batch fold or the stream-step fold; no audio, no model.
//   n_steps == 0, a batch of n clips: row_off [n + 1].  Out: n_cb [1]; cb [cb_cap][4]; cb_value, cb_weight [H][cb_cap]; run_sum, run_weight,
//   run_value [H][n].
//   n_steps > 0, n streams: the tables hold the steps' rows one step after the other; row_off [n_steps][n + 1] counts from each step's first row
//   (row_off[k][n] = the rows of step k), ctl [n_steps][n] the steps' control bytes (WSA_STREAM_START resets the stream's sums; a stream
//   without rows in a step is idle whatever its byte says otherwise).  The running sums start from zero and are carried from
//   step to step on the device.  Out: n_cb [n_steps]; the steps' callbacks one step after the other in cb, cb_value, cb_weight (first rows count
//   from their step's first row); run_* [n_steps][H][n], as each step leaves them.
// Every slot of cb_value / cb_weight / cb that no callback fills keeps what the caller put there.  Refused, nothing run and nothing written:
// whatever would make a kernel read or write outside these tables.
extern "C" int wsa_debug_regress_fold(int32_t device, const int32_t* meta, const double* values, uint32_t n_rows, uint32_t H, double step_s, uint32_t n,
                                      uint32_t n_steps, const uint32_t* row_off, const uint8_t* ctl, uint32_t cb_cap, uint32_t* n_cb, int32_t* cb,
                                      double* cb_value, double* cb_weight, double* run_sum, double* run_weight, double* run_value) {
    if (!row_off || !n_cb || !cb || !cb_value || !cb_weight || !run_sum || !run_weight || !run_value) return WSA_ERR_INVALID;
    if ((n_rows && (!meta || !values)) || H < 1 || H > WSA_REGRESS_GROUP_MAX || n < 1 || n > (1u << 16) || n_rows > (1u << 22) || cb_cap < 1 || cb_cap > (1u << 22)) return WSA_ERR_INVALID;
    if (n_steps > (1u << 12) || (n_steps && !ctl)) return WSA_ERR_INVALID;
    RowWalk W;
    if (!W.walk(meta, row_off, ctl, n, n_steps, n_rows, cb_cap, false)) return WSA_ERR_INVALID;
    if (hipSetDevice(device) != hipSuccess) return WSA_ERR_NO_DEVICE;
    wsa::DevArena A;
    int32_t *d_meta = nullptr, *d_cb = nullptr, *d_t_n = nullptr, *d_t_local = nullptr; double *d_val = nullptr, *d_cbv = nullptr, *d_cbw = nullptr, *d_tv = nullptr, *d_tw = nullptr;
    double *d_sum = nullptr, *d_weight = nullptr, *d_value = nullptr, *d_carry_s = nullptr, *d_carry_w = nullptr;
    uint32_t *d_off = nullptr, *d_bits = nullptr, *d_clip_cb = nullptr, *d_cb_off = nullptr, *d_count = nullptr;
    const size_t R = n_rows ? n_rows : 1, K = cb_cap, HN = (size_t)H * n, callbacks = (size_t)W.callbacks;
    bool ok = A.alloc(&d_meta, R * 8) && put(d_meta, meta, (size_t)n_rows * 8) && A.alloc(&d_val, (size_t)H * R) && put(d_val, values, (size_t)H * n_rows)
           && A.upload(&d_bits, W.bits) && up(A, &d_off, row_off, (size_t)(n_steps ? n_steps : 1) * (n + 1))
           && up(A, &d_cb, cb, K * 4) && up(A, &d_cbv, cb_value, (size_t)H * K) && up(A, &d_cbw, cb_weight, (size_t)H * K) && A.alloc(&d_tv, (size_t)H * R) && A.alloc(&d_tw, (size_t)H * R)
           && A.alloc(&d_t_n, R) && A.alloc(&d_t_local, R) && A.alloc(&d_clip_cb, (size_t)n) && A.alloc(&d_cb_off, (size_t)n) && zeros(A, &d_count, 1)
           && A.alloc(&d_sum, HN) && A.alloc(&d_weight, HN) && A.alloc(&d_value, HN) && zeros(A, &d_carry_s, HN) && zeros(A, &d_carry_w, HN);
    if (!ok) return WSA_ERR_HIP;
    if (!n_steps) {
        wsa_regress::RegressFoldParams p{};
        p.n_clips = n; p.H = H; p.stride = (uint32_t)R; p.step_s = step_s; p.meta = d_meta; p.row_off = d_off;
        for (uint32_t h = 0; h < H; h++) p.value[h] = d_val + (size_t)h * n_rows;
        p.t_value = d_tv; p.t_weight = d_tw; p.t_n = d_t_n; p.t_local = d_t_local; p.clip_cb = d_clip_cb; p.cb_off = d_cb_off;
        p.clip_sum = d_sum; p.clip_weight = d_weight; p.clip_value = d_value; p.cb = d_cb; p.host = d_count;
        // (the compaction's tables have the rows' stride; the callbacks come out through a staging pair of that stride)
        double *d_kv = nullptr, *d_kw = nullptr;
        ok = A.alloc(&d_kv, (size_t)H * R) && A.alloc(&d_kw, (size_t)H * R);
        p.cb_value = d_kv; p.cb_weight = d_kw;
        if (ok) wsa_regress::launch_regress_fold(p, nullptr);
        ok = ok && ran() && down(n_cb, d_count, 1);
        for (uint32_t h = 0; ok && h < H; h++) ok = down(cb_value + (size_t)h * K, d_kv + (size_t)h * R, callbacks) && down(cb_weight + (size_t)h * K, d_kw + (size_t)h * R, callbacks);
        ok = ok && down(cb, d_cb, callbacks * 4) && down(run_sum, d_sum, HN) && down(run_weight, d_weight, HN) && down(run_value, d_value, HN);
        return ok ? WSA_OK : WSA_ERR_HIP;
    }
    uint64_t cb0 = 0;
    for (uint32_t k = 0; ok && k < n_steps; k++) {
        const uint64_t row0 = W.step_row0[k];
        wsa_regress::RegressStepParams p{};
        p.n = n; p.H = H; p.stride = (uint32_t)K; p.cap = 0; p.fold = 1; p.step_s = step_s;       // cap 0: nothing goes to a D2H window
        p.meta = d_meta + row0 * 8; p.row_off = d_off + (size_t)k * (n + 1); p.bits = d_bits + (size_t)k * n;
        for (uint32_t h = 0; h < H; h++) p.value[h] = d_val + (size_t)h * n_rows + row0;
        p.run_sum = d_carry_s; p.run_weight = d_carry_w;
        p.cb = d_cb + cb0 * 4; p.cb_value = d_cbv + cb0; p.cb_weight = d_cbw + cb0;                // this step's callbacks behind the earlier steps'
        p.h_value = nullptr; p.h_cb = nullptr; p.h_cb_value = nullptr; p.h_cb_weight = nullptr;
        p.h_sum = d_sum; p.h_weight = d_weight; p.h_run_value = d_value; p.h_count = d_count;
        wsa_regress::launch_regress_step(p, nullptr);
        ok = ran() && down(n_cb + k, d_count, 1) && down(run_sum + (size_t)k * HN, d_sum, HN) && down(run_weight + (size_t)k * HN, d_weight, HN)
             && down(run_value + (size_t)k * HN, d_value, HN);
        if (ok && cb0 + n_cb[k] > callbacks) return WSA_ERR_HIP;                                    // (cannot happen: the host counted them)
        cb0 += ok ? n_cb[k] : 0;
    }
    ok = ok && down(cb, d_cb, K * 4) && down(cb_value, d_cbv, (size_t)H * K) && down(cb_weight, d_cbw, (size_t)H * K);
    return ok ? WSA_OK : WSA_ERR_HIP;
}

// K6b / K6b-e (csrc/classify_fold.hpp) on their own: hand-built row meta [n_rows][8] i32 (slot 0 the clip or stream, 1 si, 3 t_len) and, per member
// d of n_members, a legend of C[d] strings and confidences conf[d] [n_rows][C[d]] (float, or double with f64 set) straight into the product's fold
// launches (classify_internal.hpp launch_*); no audio, no model.  key_rank comes from the legend through array_index_key.
//   n_steps == 0, a batch of n clips, row_off [n + 1]: single set (one member) runs fold_kernel<float / double> + fold_compact_kernel, else
//   fold_group_kernel + fold_compact_group_kernel (float only).  Out: n_cb [1]; cb [cb_cap][4]; per member cb_label, cb_conf [cb_cap], run_conf
//   [n][C[d]]; for the group also cb_all_max per member, cb_db, cb_top_label, cb_top_conf, cb_min_db, cb_entropy [cb_cap] and run_min_db [n].
//   n_steps > 0, n streams: tables, row_off [n_steps][n + 1] and ctl [n_steps][n] as wsa_debug_regress_fold; one launch_stream_classes /
//   launch_stream_knn (single) or launch_stream_ensemble per step, the carried folds (and the group's max_inv / min_db) zeroed at entry and kept
//   on the device between steps.  Out: n_cb [n_steps]; the steps' callbacks one after the other in the cb* tables; run_conf [n_steps][n][C[d]] and
//   run_min_db [n_steps][n] as each step leaves them; h_* [n_steps][max(cap, 1)]: what the step wrote to its D2H window of `cap` callbacks
//   (plain device buffers here).
// Every output table goes to the device as the caller filled it and comes back whole: a slot no callback fills keeps the caller's value.
// Refused, nothing run and nothing written: whatever would make a kernel read or write outside these tables — offsets out of order, a row filed
// under another clip, a negative si, t_len negative or INT32_MAX, more callbacks than cb_cap, a stream's callback whose rows continue in the next
// step, class or member counts past the library's limits.
struct wsa_debug_fold_io {
    const int32_t* meta; const uint32_t* row_off; const uint8_t* ctl;
    double step_s;
    uint32_t n_rows, n, n_steps, cap, n_members, cb_cap; int32_t single, f64;
    uint32_t C[WSA_ENSEMBLE_MAX];
    const char* const* legend[WSA_ENSEMBLE_MAX];
    const void* conf[WSA_ENSEMBLE_MAX];
    uint32_t* n_cb; int32_t* cb;
    int32_t* cb_label[WSA_ENSEMBLE_MAX]; double* cb_conf[WSA_ENSEMBLE_MAX]; double* cb_all_max[WSA_ENSEMBLE_MAX]; double* run_conf[WSA_ENSEMBLE_MAX];
    int32_t* cb_db; int32_t* cb_top_label; double* cb_top_conf; int32_t* cb_min_db; double* cb_entropy; int32_t* run_min_db;
    int32_t* h_cb; int32_t* h_cb_label[WSA_ENSEMBLE_MAX]; double* h_cb_conf[WSA_ENSEMBLE_MAX]; double* h_cb_all_max[WSA_ENSEMBLE_MAX];
    int32_t* h_cb_db; int32_t* h_cb_top_label; double* h_cb_top_conf; int32_t* h_cb_min_db; double* h_cb_entropy;
};

namespace {
using namespace wsa_classify;

// the device tables both halves of wsa_debug_class_fold run over: the rows, the callback tables, and per member its confidences, key_rank and running sums
struct ClassFoldDev {
    wsa::DevArena A; size_t R = 1, K = 0;
    int32_t *meta = nullptr, *cb = nullptr, *t_n = nullptr, *t_local = nullptr;
    uint32_t *off = nullptr, *bits = nullptr, *clip_cb = nullptr, *cb_off = nullptr, *count = nullptr;
    const void* conf[WSA_ENSEMBLE_MAX] = {}; int64_t* kr[WSA_ENSEMBLE_MAX] = {};
    int32_t* cb_label[WSA_ENSEMBLE_MAX] = {}; double *cb_conf[WSA_ENSEMBLE_MAX] = {}, *cb_all_max[WSA_ENSEMBLE_MAX] = {}, *run[WSA_ENSEMBLE_MAX] = {};
    EnsTables o{};                                  // the group's decision per callback; clip_min_db per clip (streams: the step's pinned column)
};

// a batch: fold_kernel + fold_compact_kernel (single), or the group pair; n_cb, run_conf and run_min_db back
bool class_fold_batch(const wsa_debug_fold_io* io, ClassFoldDev& D) {
    wsa::DevArena& A = D.A;
    const uint32_t n = io->n, M = io->n_members;
    const size_t R = D.R;
    const bool single = io->single != 0;
    bool ok;
    if (single) {
        int32_t* d_t_label = nullptr; double* d_t_conf = nullptr;
        ok = A.alloc(&d_t_label, R) && A.alloc(&d_t_conf, R);
        if (ok && io->f64) {
            FoldParams<double> f{n, io->C[0], io->step_s, D.meta, D.off, (const double*)D.conf[0], D.kr[0], d_t_label, d_t_conf, D.t_n, D.t_local, D.clip_cb, D.run[0]};
            launch_fold(f, D.cb_off, D.cb, D.cb_label[0], D.cb_conf[0], D.count, nullptr);
        } else if (ok) {
            FoldParams<float> f{n, io->C[0], io->step_s, D.meta, D.off, (const float*)D.conf[0], D.kr[0], d_t_label, d_t_conf, D.t_n, D.t_local, D.clip_cb, D.run[0]};
            launch_fold(f, D.cb_off, D.cb, D.cb_label[0], D.cb_conf[0], D.count, nullptr);
        }
    } else {
        std::vector<FoldMember> ftab(M);
        EnsTables t{};
        ok = alloc_ens_tables(A, t, R, 0, true);
        t.clip_min_db = D.o.clip_min_db;
        for (uint32_t d = 0; ok && d < M; d++) {
            FoldMember& m = ftab[d];
            m = FoldMember{};
            m.C = io->C[d]; m.prob = (const float*)D.conf[d]; m.key_rank = D.kr[d];
            ok = A.alloc(&m.t_label, R) && A.alloc(&m.t_conf, R) && A.alloc(&m.t_all_max, R);
            m.clip_conf = D.run[d]; m.cb_label = D.cb_label[d]; m.cb_conf = D.cb_conf[d]; m.cb_all_max = D.cb_all_max[d];
        }
        FoldMember* d_ftab = nullptr;
        ok = ok && A.upload(&d_ftab, ftab);
        if (ok) {
            FoldGroupParams f{};
            f.n_clips = n; f.n_members = M; f.step_s = io->step_s; f.meta = D.meta; f.row_off = D.off; f.tab = d_ftab;
            f.t_n = D.t_n; f.t_local = D.t_local; f.clip_cb = D.clip_cb; f.t = t;
            launch_fold_group(f, D.cb_off, D.o, D.count, nullptr);
        }
    }
    ok = ok && ran() && down(io->n_cb, D.count, 1);
    for (uint32_t d = 0; ok && d < M; d++) ok = down(io->run_conf[d], D.run[d], (size_t)n * io->C[d]);
    if (ok && !single) ok = down(io->run_min_db, D.o.clip_min_db, (size_t)n);
    return ok;
}

// streams: one launch_stream_classes / _knn / _ensemble per step over the carried state, zeroed (min_db: -1); n_cb, run_conf and run_min_db back per
// step, the steps' D2H windows (one after the other) behind the last
bool class_fold_steps(const wsa_debug_fold_io* io, ClassFoldDev& D, const RowWalk& walk) {
    wsa::DevArena& A = D.A;
    const uint32_t n = io->n, n_steps = io->n_steps, M = io->n_members;
    const bool single = io->single != 0, f64 = io->f64 != 0;
    const size_t W = io->cap ? io->cap : 1, HW = (size_t)n_steps * W, K = D.K;
    CarriedFold carried[WSA_ENSEMBLE_MAX] = {};
    int32_t *d_h_cb = nullptr, *d_h_cb_label[WSA_ENSEMBLE_MAX] = {}, *d_h_min = nullptr, *d_min_db = nullptr;
    double *d_h_cb_conf[WSA_ENSEMBLE_MAX] = {}, *d_h_cb_all_max[WSA_ENSEMBLE_MAX] = {}, *d_seg[WSA_ENSEMBLE_MAX] = {}, *d_sum[WSA_ENSEMBLE_MAX] = {}, *d_max_inv = nullptr;
    float* d_h_prob[WSA_ENSEMBLE_MAX] = {};
    EnsTables h{};
    bool ok = up(A, &d_h_cb, io->h_cb, HW * 4);
    for (uint32_t d = 0; ok && d < M; d++) {
        const size_t Cd = io->C[d];
        ok = zeros(A, &carried[d].acc_all, (size_t)n * Cd) && zeros(A, &carried[d].in_all, (size_t)n * Cd) && zeros(A, &carried[d].first, (size_t)n * Cd)
             && zeros(A, &carried[d].stamp, (size_t)n) && up(A, &d_h_cb_label[d], io->h_cb_label[d], HW) && up(A, &d_h_cb_conf[d], io->h_cb_conf[d], HW) && A.alloc(&d_h_prob[d], W * Cd);
        if (ok && !single) ok = up(A, &d_h_cb_all_max[d], io->h_cb_all_max[d], HW) && A.alloc(&d_seg[d], K) && A.alloc(&d_sum[d], K);
    }
    if (ok && !single)
        ok = up(A, &h.cb_db, io->h_cb_db, HW) && up(A, &h.cb_top_label, io->h_cb_top_label, HW) && up(A, &h.cb_top_conf, io->h_cb_top_conf, HW) && up(A, &h.cb_min_db, io->h_cb_min_db, HW)
             && up(A, &h.cb_entropy, io->h_cb_entropy, HW) && A.alloc(&d_h_min, (size_t)n) && zeros(A, &d_max_inv, (size_t)n)
             && A.alloc(&d_min_db, (size_t)n) && hipMemset(d_min_db, 0xff, (size_t)n * sizeof(int32_t)) == hipSuccess;
    // the KNN step kernel also pushes its rows' labels (one per row) and neighbours (k per row; none here)
    int32_t *d_klabel = nullptr, *d_h_klabel = nullptr; double* d_h_kconf = nullptr;
    if (ok && f64) ok = zeros(A, &d_klabel, D.R) && A.alloc(&d_h_klabel, W) && A.alloc(&d_h_kconf, W * io->C[0]);
    // the members' tables of every step (a step's callbacks sit behind the earlier steps')
    FoldMember* d_ftab = nullptr; StreamMember* d_stab = nullptr;
    if (ok && !single) {
        std::vector<FoldMember> ftab((size_t)n_steps * M);
        std::vector<StreamMember> stab((size_t)n_steps * M);
        for (uint32_t k = 0; k < n_steps; k++)
            for (uint32_t d = 0; d < M; d++) {
                const size_t cb0 = walk.step_cb0[k], hw0 = (size_t)k * W;
                FoldMember& m = ftab[(size_t)k * M + d];
                m = FoldMember{};
                m.C = io->C[d]; m.prob = (const float*)D.conf[d] + walk.step_row0[k] * io->C[d]; m.key_rank = D.kr[d];
                m.t_label = D.cb_label[d] + cb0; m.t_conf = D.cb_conf[d] + cb0; m.t_all_max = D.cb_all_max[d] + cb0; m.t_seg = d_seg[d] + cb0; m.t_all_sum = d_sum[d] + cb0;
                m.cb_label = m.t_label; m.cb_conf = m.t_conf; m.cb_all_max = m.t_all_max;
                stab[(size_t)k * M + d] = StreamMember{carried[d], d_h_prob[d], d_h_cb_label[d] + hw0, d_h_cb_conf[d] + hw0, d_h_cb_all_max[d] + hw0, D.run[d]};
            }
        ok = A.upload(&d_ftab, ftab) && A.upload(&d_stab, stab);
    }
    for (uint32_t k = 0; ok && k < n_steps; k++) {
        const size_t row0 = walk.step_row0[k], cb0 = walk.step_cb0[k], hw0 = (size_t)k * W;
        const uint32_t* off = D.off + (size_t)k * (n + 1);
        const uint32_t* bk = D.bits + (size_t)k * n;
        if (single) {
            const StepFoldTables t{io->cap, D.cb + cb0 * 4, D.cb_label[0] + cb0, D.cb_conf[0] + cb0, d_h_cb + hw0 * 4, d_h_cb_label[0] + hw0, d_h_cb_conf[0] + hw0, D.run[0], D.count};
            if (f64) {
                StreamKnnParams p{};
                p.n = n; p.C = io->C[0]; p.k = 0; p.fold = 1; p.step_s = io->step_s; p.meta = D.meta + row0 * 8; p.row_off = off; p.bits = bk; p.key_rank = D.kr[0];
                p.label = d_klabel; p.conf = (const double*)D.conf[0] + row0 * io->C[0]; p.carried = carried[0]; p.t = t;
                p.h_label = d_h_klabel; p.h_conf = d_h_kconf;
                launch_stream_knn(p, nullptr);
            } else {
                StreamClsParams p{};
                p.n = n; p.C = io->C[0]; p.fold = 1; p.step_s = io->step_s; p.meta = D.meta + row0 * 8; p.row_off = off; p.prob = (const float*)D.conf[0] + row0 * io->C[0];
                p.key_rank = D.kr[0]; p.bits = bk; p.carried = carried[0]; p.t = t; p.h_prob = d_h_prob[0];
                launch_stream_classes(p, nullptr);
            }
        } else {
            const EnsTables& o = D.o;
            StreamEnsParams p{};
            p.n = n; p.n_members = M; p.cap = io->cap; p.fold = 1; p.step_s = io->step_s; p.meta = D.meta + row0 * 8; p.row_off = off; p.bits = bk;
            p.tab = d_ftab + (size_t)k * M; p.stab = d_stab + (size_t)k * M;
            p.o = EnsTables{D.cb + cb0 * 4, o.cb_db + cb0, o.cb_top_label + cb0, o.cb_top_conf + cb0, o.cb_min_db + cb0, o.cb_entropy + cb0, nullptr};
            p.h = EnsTables{d_h_cb + hw0 * 4, h.cb_db + hw0, h.cb_top_label + hw0, h.cb_top_conf + hw0, h.cb_min_db + hw0, h.cb_entropy + hw0, d_h_min};
            p.max_inv = d_max_inv; p.min_db = d_min_db; p.h_count = D.count;
            launch_stream_ensemble(p, nullptr);
        }
        ok = ran() && down(io->n_cb + k, D.count, 1);
        for (uint32_t d = 0; ok && d < M; d++) ok = down(io->run_conf[d] + (size_t)k * n * io->C[d], D.run[d], (size_t)n * io->C[d]);
        if (ok && !single) ok = down(io->run_min_db + (size_t)k * n, d_h_min, (size_t)n);
    }
    ok = ok && down(io->h_cb, d_h_cb, HW * 4);
    for (uint32_t d = 0; ok && d < M; d++) {
        ok = down(io->h_cb_label[d], d_h_cb_label[d], HW) && down(io->h_cb_conf[d], d_h_cb_conf[d], HW);
        if (ok && !single) ok = down(io->h_cb_all_max[d], d_h_cb_all_max[d], HW);
    }
    if (ok && !single)
        ok = down(io->h_cb_db, h.cb_db, HW) && down(io->h_cb_top_label, h.cb_top_label, HW) && down(io->h_cb_top_conf, h.cb_top_conf, HW)
             && down(io->h_cb_min_db, h.cb_min_db, HW) && down(io->h_cb_entropy, h.cb_entropy, HW);
    return ok;
}
}  // namespace

extern "C" int wsa_debug_class_fold(int32_t device, const wsa_debug_fold_io* io) {
    using namespace wsa_classify;
    if (!io || !io->row_off || !io->n_cb || !io->cb) return WSA_ERR_INVALID;
    const uint32_t n = io->n, n_rows = io->n_rows, n_steps = io->n_steps, M = io->n_members;
    if ((n_rows && !io->meta) || M < 1 || M > WSA_ENSEMBLE_MAX || n < 1 || n > (1u << 16) || n_rows > (1u << 22) || io->cb_cap < 1 || io->cb_cap > (1u << 22)) return WSA_ERR_INVALID;
    if (n_steps > (1u << 12) || (n_steps && !io->ctl) || io->cap > (1u << 22)) return WSA_ERR_INVALID;
    const bool single = io->single != 0, f64 = io->f64 != 0, streams = n_steps != 0;
    if (single ? M != 1 : f64) return WSA_ERR_INVALID;                  // double confidences are the single fold's (KN-2)
    const size_t W = io->cap ? io->cap : 1;
    if (streams && (uint64_t)n_steps * W > (1u << 24)) return WSA_ERR_INVALID;
    for (uint32_t d = 0; d < M; d++) {
        if (io->C[d] < 1 || io->C[d] > WSA_MODEL_MAX_CLASSES || !io->legend[d] || (n_rows && !io->conf[d])) return WSA_ERR_INVALID;
        for (uint32_t c = 0; c < io->C[d]; c++) if (!io->legend[d][c]) return WSA_ERR_INVALID;
        if (!io->cb_label[d] || !io->cb_conf[d] || !io->run_conf[d] || (!single && !io->cb_all_max[d])) return WSA_ERR_INVALID;
        if (streams && (!io->h_cb_label[d] || !io->h_cb_conf[d] || (!single && !io->h_cb_all_max[d]))) return WSA_ERR_INVALID;
    }
    if (!single && (!io->cb_db || !io->cb_top_label || !io->cb_top_conf || !io->cb_min_db || !io->cb_entropy || !io->run_min_db)) return WSA_ERR_INVALID;
    if (streams && (!io->h_cb || (!single && (!io->h_cb_db || !io->h_cb_top_label || !io->h_cb_top_conf || !io->h_cb_min_db || !io->h_cb_entropy)))) return WSA_ERR_INVALID;
    RowWalk walk;
    if (!walk.walk(io->meta, io->row_off, io->ctl, n, n_steps, n_rows, io->cb_cap, true)) return WSA_ERR_INVALID;
    if (hipSetDevice(device) != hipSuccess) return WSA_ERR_NO_DEVICE;

    ClassFoldDev D; wsa::DevArena& A = D.A;
    D.R = n_rows ? n_rows : 1; D.K = io->cb_cap;
    const size_t R = D.R, K = D.K;
    bool ok = up(A, &D.meta, io->meta, (size_t)n_rows * 8) && up(A, &D.off, io->row_off, (size_t)(streams ? n_steps : 1) * (n + 1)) && A.upload(&D.bits, walk.bits)
           && up(A, &D.cb, io->cb, K * 4) && A.alloc(&D.t_n, R) && A.alloc(&D.t_local, R) && A.alloc(&D.clip_cb, (size_t)n) && A.alloc(&D.cb_off, (size_t)n) && zeros(A, &D.count, 1);
    for (uint32_t d = 0; ok && d < M; d++) {                            // per member: confidences, key_rank, the callback tables, the running sums
        const size_t Cd = io->C[d];
        std::vector<int64_t> kr(Cd, -1);
        for (size_t c = 0; c < Cd; c++) { int64_t v; if (array_index_key(io->legend[d][c], &v)) kr[c] = v; }
        if (f64) { double* p = nullptr; ok = up(A, &p, (const double*)io->conf[d], (size_t)n_rows * Cd); D.conf[d] = p; }
        else { float* p = nullptr; ok = up(A, &p, (const float*)io->conf[d], (size_t)n_rows * Cd); D.conf[d] = p; }
        ok = ok && A.upload(&D.kr[d], kr) && up(A, &D.cb_label[d], io->cb_label[d], K) && up(A, &D.cb_conf[d], io->cb_conf[d], K) && A.alloc(&D.run[d], (size_t)n * Cd);
        if (ok && !single) ok = up(A, &D.cb_all_max[d], io->cb_all_max[d], K);
    }
    EnsTables& o = D.o;
    if (ok && !single)
        ok = up(A, &o.cb_db, io->cb_db, K) && up(A, &o.cb_top_label, io->cb_top_label, K) && up(A, &o.cb_top_conf, io->cb_top_conf, K) && up(A, &o.cb_min_db, io->cb_min_db, K)
             && up(A, &o.cb_entropy, io->cb_entropy, K) && up(A, &o.clip_min_db, io->run_min_db, (size_t)n);
    o.cb = D.cb;
    if (!ok) return WSA_ERR_HIP;

    ok = streams ? class_fold_steps(io, D, walk) : class_fold_batch(io, D);
    ok = ok && down(io->cb, D.cb, K * 4);
    for (uint32_t d = 0; ok && d < M; d++) {
        ok = down(io->cb_label[d], D.cb_label[d], K) && down(io->cb_conf[d], D.cb_conf[d], K);
        if (ok && !single) ok = down(io->cb_all_max[d], D.cb_all_max[d], K);
    }
    if (ok && !single)
        ok = down(io->cb_db, o.cb_db, K) && down(io->cb_top_label, o.cb_top_label, K) && down(io->cb_top_conf, o.cb_top_conf, K)
             && down(io->cb_min_db, o.cb_min_db, K) && down(io->cb_entropy, o.cb_entropy, K);
    return ok ? WSA_OK : WSA_ERR_HIP;
}
