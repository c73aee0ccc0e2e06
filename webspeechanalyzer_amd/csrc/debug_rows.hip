// debug_rows.hip — test entries of libwsa that are NOT part of include/wsa.h, for the kernels behind the tracker that are fed hand-built segment, row and
// frame tables: K3 (csrc/tracker.hip launch_compact: compact_count_kernel, compact_scan_kernel, compact_gather_kernel), K4 (csrc/utterance.hip
// launch_utterance) and K5 (csrc/coeffs.hip launch_coeffs).  Each entry refuses on the host whatever would make its kernel leave the tables.
#include <cstring>
#include <vector>
#include "api_internal.hpp"
#include "debug_internal.hpp"

using namespace wsa_debug;

// K4 (csrc/utterance.hip) on its own: hand-built segments, syllable rows and frames straight into ONE launch_utterance, in the batch geometry
// (state == NULL, ring_mask = ~0: clip c's frames are rows frame_off[c] .. frame_off[c + 1] of `formants`, the tables hold the whole clips) or the
// streams' (state, carry and ctl given, ring_mask = ring - 1: stream c's ring is rows frame_off[c] .. + ring, the tables hold ONE step's segments and
// rows, carry [n_clips][CARRY_WORDS] is already advanced over them as compact_gather_kernel leaves it, state [n_clips][UTT_STATE_WORDS] goes in and
// comes back).  segments [n_segs][4] i32 {clip, start, len, flag}, clip_seg_off / clip_row_off / frame_off [n_clips + 1], row_meta [n_rows][8] i32
// (slot 0 the clip, 1 the result index, 6 the syllable's first frame, 7 its length).  Out: utt_feat [rows_cap][264] f64 and utt_meta [rows_cap][4] i32,
// every slot starting as `sentinel`, clip_utt_off [n_clips + 1] and totals[3] likewise; totals[0 .. 2] start as 0 (K4 only ever ORs into totals[2]).
// Refused, nothing run and nothing written: whatever would make the kernel read or write outside these tables.
extern "C" int wsa_debug_utterance(int32_t device, const int32_t* segments, uint32_t n_segs, const uint32_t* clip_seg_off, const int32_t* row_meta, uint32_t n_rows,
                                   const uint32_t* clip_row_off, const float* formants, const uint32_t* frame_off, uint32_t n_clips, uint32_t rows_cap,
                                   uint32_t ring_mask, uint32_t* state, const int32_t* carry, const uint32_t* ctl, int32_t sentinel,
                                   double* utt_feat, int32_t* utt_meta, uint32_t* clip_utt_off, uint32_t* totals4) {
    if (!clip_seg_off || !clip_row_off || !frame_off || !utt_feat || !utt_meta || !clip_utt_off || !totals4) return WSA_ERR_INVALID;
    if ((!segments && n_segs) || (!row_meta && n_rows) || n_clips < 1 || n_clips > (1u << 16) || rows_cap < 1 || rows_cap > (1u << 20)) return WSA_ERR_INVALID;
    const bool streams = state != nullptr;
    if (streams != (carry != nullptr) || streams != (ctl != nullptr)) return WSA_ERR_INVALID;          // the three stream tables come together
    const uint64_t ring = (uint64_t)ring_mask + 1;
    if ((ring & (ring - 1)) != 0) return WSA_ERR_INVALID;                                               // frames are read at (st + o) & ring_mask
    if (streams == (ring_mask == 0xffffffffu)) return WSA_ERR_INVALID;                                  // batches do not wrap, streams do
    if (clip_seg_off[0] != 0 || clip_row_off[0] != 0 || frame_off[0] != 0) return WSA_ERR_INVALID;
    for (uint32_t c = 0; c < n_clips; c++) {
        if (clip_seg_off[c + 1] < clip_seg_off[c] || clip_row_off[c + 1] < clip_row_off[c] || frame_off[c + 1] < frame_off[c]) return WSA_ERR_INVALID;
        if (frame_off[c + 1] > (1u << 26)) return WSA_ERR_INVALID;
        if (streams && frame_off[c + 1] - frame_off[c] < ring) return WSA_ERR_INVALID;                 // a whole ring per stream
    }
    if (clip_seg_off[n_clips] != n_segs || clip_row_off[n_clips] != n_rows || (formants == nullptr && frame_off[n_clips] != 0)) return WSA_ERR_INVALID;
    uint64_t results = 0;
    for (uint32_t c = 0; c < n_clips; c++) {
        const uint32_t nseg = clip_seg_off[c + 1] - clip_seg_off[c];
        for (uint32_t s = clip_seg_off[c]; s < clip_seg_off[c + 1]; s++) results += segments[(size_t)s * 4 + 3] >= 0 ? 1 : 0;
        const uint64_t frames = frame_off[c + 1] - frame_off[c];
        for (uint32_t r = clip_row_off[c]; r < clip_row_off[c + 1]; r++) {
            const int32_t* m = row_meta + (size_t)r * 8;
            if (m[0] < 0 || (uint32_t)m[0] >= n_clips || (uint32_t)m[0] != c || m[6] < 0 || m[7] < 0) return WSA_ERR_INVALID;   // a row of another clip, or of none
            if (streams ? (uint64_t)m[7] > ring : (uint64_t)m[6] + (uint64_t)m[7] > frames) return WSA_ERR_INVALID;             // a syllable outside its clip's frames (its ring)
        }
        if (streams && nseg) {
            const int32_t* cy = carry + (size_t)c * wsa::CARRY_WORDS;
            if (cy[0] < 0 || (uint32_t)cy[0] < nseg) return WSA_ERR_INVALID;                            // K3 has counted this step's segments in already
            if (!(ctl[c] & 1u) && state[(size_t)c * wsa::UTT_STATE_WORDS + 280] > 0x7fffffffu) return WSA_ERR_INVALID;    // the history is indexed with the result count
        }
    }
    if (results > rows_cap) return WSA_ERR_INVALID;
    if (hipSetDevice(device) != hipSuccess) return WSA_ERR_NO_DEVICE;
    const size_t frames_all = frame_off[n_clips], n1 = (size_t)n_clips + 1;
    std::vector<double> hf((size_t)rows_cap * 264, (double)sentinel);
    std::vector<int32_t> hm((size_t)rows_cap * 4, sentinel);
    std::vector<uint32_t> ho(n1, (uint32_t)sentinel), hs;
    uint32_t tot[4] = {0, 0, 0, (uint32_t)sentinel};
    wsa::DevArena A; float* dfr = nullptr; int32_t *dseg = nullptr, *dmeta = nullptr, *dum = nullptr, *dcarry = nullptr; double* duf = nullptr;
    uint32_t *dso = nullptr, *dro = nullptr, *dfo = nullptr, *duo = nullptr, *dtot = nullptr, *dstate = nullptr, *dctl = nullptr;
    // (the three input tables have one entry of slack behind the caller's)
    bool ok = A.alloc(&dfr, frames_all * 9 + 1) && put(dfr, formants, frames_all * 9) && A.alloc(&dseg, (size_t)n_segs * 4 + 1) && put(dseg, segments, (size_t)n_segs * 4)
           && A.alloc(&dmeta, (size_t)n_rows * 8 + 1) && put(dmeta, row_meta, (size_t)n_rows * 8) && up(A, &dso, clip_seg_off, n1) && up(A, &dro, clip_row_off, n1)
           && up(A, &dfo, frame_off, n1) && A.upload(&duo, ho) && up(A, &dtot, tot, 4) && A.upload(&duf, hf) && A.upload(&dum, hm);
    const size_t nstate = (size_t)n_clips * wsa::UTT_STATE_WORDS;
    if (ok && streams) ok = up(A, &dstate, state, nstate) && up(A, &dcarry, carry, (size_t)n_clips * wsa::CARRY_WORDS) && up(A, &dctl, ctl, n_clips);
    if (ok) {
        wsa::UttParams u;
        u.n_clips = n_clips; u.segments = dseg; u.row_meta = dmeta; u.clip_seg_off = dso; u.clip_row_off = dro; u.frame_off = dfo; u.formants = dfr;
        u.clip_utt_off = duo; u.utt_meta = dum; u.utt_feat = duf; u.totals = dtot;
        u.state = dstate; u.carry = dcarry; u.ctl = dctl; u.ring_mask = ring_mask;
        wsa::launch_utterance(u, nullptr);
        ok = ran() && down(hf.data(), duf, hf.size()) && down(hm.data(), dum, hm.size()) && down(ho.data(), duo, n1) && down(tot, dtot, 4);
        if (ok && streams) { hs.resize(nstate); ok = down(hs.data(), dstate, nstate); }
        if (ok) {                                                            // all or nothing: a failed run leaves the caller's tables as they were
            memcpy(utt_feat, hf.data(), hf.size() * sizeof(double)); memcpy(utt_meta, hm.data(), hm.size() * sizeof(int32_t));
            memcpy(clip_utt_off, ho.data(), n1 * sizeof(uint32_t)); memcpy(totals4, tot, sizeof(tot));
            if (streams) memcpy(state, hs.data(), nstate * sizeof(uint32_t));
        }
    }
    return ok ? WSA_OK : WSA_ERR_HIP;
}

// K5 (csrc/coeffs.hip) on its own: hand-built syllables straight into coeffs_kernel, in the batch geometry (ring_mask = ~0, scratch_stride = 0: clip c's
// frames are rows frame_off[c] .. frame_off[c + 1] of the frame tables) or the streams' (ring_mask = ring - 1, scratch_stride >= ring_mask + longest
// syllable: stream c's ring is rows frame_off[c] .. + ring).  formants [frame_off[n_clips]][9] f32, sums [frame_off[n_clips]] f32, frame_off [n_clips + 1],
// row_meta [n_rows][8] i32 (slot 0 the clip, 6 the syllable's first frame, 7 its length), one launch_coeffs over rows_cap >= n_rows rows.
// out [rows_cap][WSA_NFEAT] f64: every slot starts as `sentinel`, slot 23 of the first n_rows rows as 0 (what the level-10 row leaves there).
// total_frames is the drivers': all frames of a batch (batch_run.hip), n x 2 x ring for streams (stream_step.hip; here n x scratch_stride).
// Refused, nothing run: whatever would make the kernel read or write outside these tables.
extern "C" int wsa_debug_coeffs(int32_t device, const float* formants, const float* sums, const uint32_t* frame_off, uint32_t n_clips,
                                const int32_t* row_meta, uint32_t n_rows, uint32_t rows_cap, uint32_t ring_mask, uint32_t scratch_stride,
                                double sentinel, double* out) {
    if (!formants || !sums || !frame_off || !row_meta || !out || n_clips < 1 || n_clips > (1u << 16) || n_rows < 1 || rows_cap < n_rows || rows_cap > (1u << 20)) return WSA_ERR_INVALID;
    const uint64_t ring = (uint64_t)ring_mask + 1;
    if ((ring & (ring - 1)) != 0) return WSA_ERR_INVALID;                                   // frames are read at (st + r) & ring_mask
    if (scratch_stride == 0 && ring_mask != 0xffffffffu) return WSA_ERR_INVALID;            // batches do not wrap
    if (scratch_stride != 0 && ring_mask == 0xffffffffu) return WSA_ERR_INVALID;
    for (uint32_t c = 0; c < n_clips; c++) {
        if (frame_off[c + 1] < frame_off[c] || frame_off[c + 1] > (1u << 24)) return WSA_ERR_INVALID;
        if (scratch_stride && frame_off[c + 1] - frame_off[c] < ring) return WSA_ERR_INVALID;    // a whole ring per stream
    }
    for (uint32_t r = 0; r < n_rows; r++) {
        const int32_t* m = row_meta + (size_t)r * 8;
        if (m[0] < 0 || (uint32_t)m[0] >= n_clips || m[6] < 0 || m[7] < 0) return WSA_ERR_INVALID;
        const uint64_t frames = frame_off[m[0] + 1] - frame_off[m[0]];
        if (scratch_stride == 0 ? (uint64_t)m[6] + (uint64_t)m[7] > frames : (uint64_t)m[7] > ring) return WSA_ERR_INVALID;      // a syllable outside its clip's frames (its ring)
        if (scratch_stride && (uint64_t)ring_mask + (uint64_t)m[7] > scratch_stride) return WSA_ERR_INVALID;                    // scratch rows (st & ring_mask) .. + sl stay inside the stream's region
    }
    const uint64_t frames_all = frame_off[n_clips];
    const uint64_t total = scratch_stride ? (uint64_t)n_clips * scratch_stride : frames_all;
    if (total > (1u << 26)) return WSA_ERR_INVALID;
    if (hipSetDevice(device) != hipSuccess) return WSA_ERR_NO_DEVICE;
    std::vector<double> h((size_t)rows_cap * WSA_NFEAT, sentinel);
    for (uint32_t r = 0; r < n_rows; r++) h[(size_t)r * WSA_NFEAT + 23] = 0.0;
    const uint32_t totals[4] = {n_rows, 0, 0, 0};
    wsa::DevArena A; float *dfr = nullptr, *dsum = nullptr; uint32_t *doff = nullptr, *dtot = nullptr; int32_t* dmeta = nullptr; double *dfeat = nullptr, *dws = nullptr;
    bool ok = up(A, &dfr, formants, (size_t)frames_all * 9) && up(A, &dsum, sums, (size_t)frames_all) && up(A, &doff, frame_off, (size_t)n_clips + 1) && up(A, &dtot, totals, 4)
           && up(A, &dmeta, row_meta, (size_t)n_rows * 8) && A.upload(&dfeat, h) && zeros(A, &dws, (size_t)total * 8);
    if (ok) {
        wsa::CoefParams q;
        q.row_meta = dmeta; q.row_feat = dfeat; q.frame_off = doff; q.totals = dtot; q.formants = dfr; q.sums = dsum;
        q.ws = dws; q.total_frames = (uint32_t)total; q.ring_mask = ring_mask; q.scratch_stride = scratch_stride;
        wsa::launch_coeffs(q, rows_cap, nullptr);
        ok = ran() && down(out, dfeat, h.size());
    }
    return ok ? WSA_OK : WSA_ERR_HIP;
}

// K3 (csrc/tracker.hip: compact_count_kernel, compact_scan_kernel, compact_gather_kernel) on its own: hand-built segment tables and a hand-built row
// pool straight into launch_compact, which picks its form from n, fused, clip_rows and carry itself (path = what compact_path said it ran).
//   n_steps == 0, a batch of n clips: seg_i [n][seg_cap][8], seg_count [n], clip_rows [n] (or NULL: no fused form) — the per-clip row counters as the
//   tracker leaves them, which must equal the rows of the clip's reported segments.  counters [16] (word 1 is the flag word the fused form publishes), totals
//   [4] and hist [SPAN_BUCKETS] go to the device as the caller seeded them and come back as the run left them; give_clr hands counters and hist over as
//   clr_counters / clr_hist, give_host the four host words (mapped pinned memory, as the batch driver's).
//   n_steps > 0, n streams: seg_i [n_steps][n][seg_cap][8], seg_count and ctl [n_steps][n]; each step runs launch_stream_prepare (ctl bit 0 START clears the
//   stream's carry) and launch_compact with the carry, which starts as carry_in [n][CARRY_WORDS] (NULL: zeros) and stays on the device between steps.  The
//   seeded totals go up afresh before every step; carry [n_steps][n][CARRY_WORDS] comes back as each step left it.
// The pool (row_meta_in [pool][8], row_feat_in [pool][53]) is one for all steps.  Out, per step: seg_out [segs_cap][4], row_meta_out [rows_cap][8], row_feat_out
// [rows_cap][53], clip_row_off / clip_seg_off [n + 1], totals [4].  Every output table goes to the device as the caller filled it and comes back whole: a slot
// the kernels do not write keeps the caller's value.
// Refused, nothing run and nothing written: whatever would make a kernel index outside these tables — seg_count > seg_cap, SEG_ROW0 + SEG_NROWS past the
// pool, a negative SEG_NROWS or SEG_ROW0, more rows or segments in a step than rows_cap / segs_cap, clip_rows that differ from the rows reported, a carry whose
// counts are negative or that has counted more results than segments (the result index would then run ahead of the step's table), an unknown level.
struct wsa_debug_compact_io {
    const int32_t* seg_i; const uint32_t* seg_count; const uint32_t* ctl; const int32_t* row_meta_in; const double* row_feat_in; const uint32_t* clip_rows;
    const int32_t* carry_in;
    uint32_t n, seg_cap, pool, n_steps, rows_cap, segs_cap; int32_t level, fused, give_clr, give_host;
    int32_t* seg_out; int32_t* row_meta_out; double* row_feat_out; uint32_t* clip_row_off; uint32_t* clip_seg_off; uint32_t* totals;
    uint32_t* host4; uint32_t* counters; uint32_t* hist; int32_t* path; int32_t* carry;
};

// the segment tables of every step stay inside the pool, the output tables and the carry's range (the pointers and sizes are checked already)
static bool compact_tables_fit(const wsa_debug_compact_io* io) {
    using namespace wsa;
    const uint32_t n = io->n, pool = io->pool;
    const bool streams = io->n_steps != 0;
    const uint32_t tables = streams ? io->n_steps : 1;
    const size_t seg_cap = io->seg_cap, segs = (size_t)n * seg_cap;
    std::vector<int64_t> seg_before(n, 0), res_before(n, 0);
    for (uint32_t c = 0; streams && io->carry_in && c < n; c++) {
        const int32_t* cy = io->carry_in + (size_t)c * CARRY_WORDS;
        if (cy[0] < 0 || cy[1] < 0 || cy[1] > cy[0]) return false;
        seg_before[c] = cy[0]; res_before[c] = cy[1];
    }
    for (uint32_t k = 0; k < tables; k++) {
        uint64_t rows = 0, nsegs = 0;
        for (uint32_t c = 0; c < n; c++) {
            const uint32_t ns = io->seg_count[(size_t)k * n + c];
            if (ns > seg_cap) return false;
            if (streams && (io->ctl[(size_t)k * n + c] & ~3u)) return false;
            if (streams && (io->ctl[(size_t)k * n + c] & 1u)) { seg_before[c] = 0; res_before[c] = 0; }
            uint64_t clip_rows = 0, results = 0;
            for (uint32_t q = 0; q < ns; q++) {
                const int32_t* sg = io->seg_i + ((size_t)k * segs + (size_t)c * seg_cap + q) * 8;
                if (sg[SEG_NROWS] < 0 || sg[SEG_ROW0] < 0 || (uint64_t)sg[SEG_ROW0] + (uint64_t)sg[SEG_NROWS] > pool) return false;
                if (sg[SEG_FLAG] >= 0) { clip_rows += (uint32_t)sg[SEG_NROWS]; results++; }
            }
            if (io->clip_rows && io->clip_rows[c] != clip_rows) return false;
            seg_before[c] += ns; res_before[c] += (int64_t)results;
            if (seg_before[c] > (1 << 30)) return false;
            rows += clip_rows; nsegs += ns;
        }
        if (rows > io->rows_cap || nsegs > io->segs_cap) return false;
    }
    return true;
}

extern "C" int wsa_debug_compact(int32_t device, const wsa_debug_compact_io* io) {
    using namespace wsa;
    if (!io || !io->seg_i || !io->seg_count || !io->seg_out || !io->row_meta_out || !io->row_feat_out || !io->clip_row_off || !io->clip_seg_off || !io->totals
        || !io->host4 || !io->counters || !io->hist || !io->path) return WSA_ERR_INVALID;
    const uint32_t n = io->n, n_steps = io->n_steps, pool = io->pool;
    const bool streams = n_steps != 0;
    if (n < 1 || n > (1u << 14) || io->seg_cap < 1 || io->seg_cap > (1u << 12) || pool > (1u << 20) || (pool && (!io->row_meta_in || !io->row_feat_in))) return WSA_ERR_INVALID;
    if (io->rows_cap < 1 || io->rows_cap > (1u << 20) || io->segs_cap < 1 || io->segs_cap > (1u << 20) || n_steps > (1u << 12)) return WSA_ERR_INVALID;
    if (io->level != 3 && io->level != 4 && io->level != 5 && io->level != 10 && io->level != 13) return WSA_ERR_INVALID;
    if (streams && (!io->ctl || !io->carry || io->clip_rows || io->give_clr || io->give_host)) return WSA_ERR_INVALID;        // the fused form is the batches'
    if (!streams && (io->carry_in || io->carry)) return WSA_ERR_INVALID;
    if (!compact_tables_fit(io)) return WSA_ERR_INVALID;
    if (hipSetDevice(device) != hipSuccess) return WSA_ERR_NO_DEVICE;
    const uint32_t tables = streams ? n_steps : 1;
    const size_t seg_cap = io->seg_cap, segs = (size_t)n * seg_cap, R = io->rows_cap, S = io->segs_cap, n1 = (size_t)n + 1;
    DevArena A;
    int32_t *d_seg_i = nullptr, *d_meta_in = nullptr, *d_seg_out = nullptr, *d_meta_out = nullptr, *d_carry = nullptr; double *d_feat_in = nullptr, *d_feat_out = nullptr, *d_state = nullptr;
    uint32_t *d_seg_count = nullptr, *d_clip_rows = nullptr, *d_ctl = nullptr, *d_row_off = nullptr, *d_seg_off = nullptr, *d_totals = nullptr, *d_counters = nullptr, *d_hist = nullptr;
    uint32_t *h_host = nullptr, *h_host_dev = nullptr;
    bool ok = A.alloc(&d_seg_i, segs * 8) && A.alloc(&d_seg_count, n) && up(A, &d_meta_in, io->row_meta_in, (size_t)pool * 8) && up(A, &d_feat_in, io->row_feat_in, (size_t)pool * WSA_NFEAT)
           && A.alloc(&d_seg_out, S * 4) && A.alloc(&d_meta_out, R * 8) && A.alloc(&d_feat_out, R * WSA_NFEAT) && A.alloc(&d_row_off, n1) && A.alloc(&d_seg_off, n1)
           && A.alloc(&d_totals, 4) && up(A, &d_counters, io->counters, 16) && up(A, &d_hist, io->hist, (size_t)SPAN_BUCKETS) && A.pin(&h_host, &h_host_dev, 4);
    if (ok && io->clip_rows) ok = up(A, &d_clip_rows, io->clip_rows, n);
    if (ok && streams) ok = A.alloc(&d_ctl, n) && zeros(A, &d_state, (size_t)n * GATE_STATE) && zeros(A, &d_carry, (size_t)n * CARRY_WORDS) && (!io->carry_in || put(d_carry, io->carry_in, (size_t)n * CARRY_WORDS));
    if (!ok) return WSA_ERR_HIP;
    for (int q = 0; q < 4; q++) h_host[q] = io->host4[q];
    for (uint32_t k = 0; ok && k < tables; k++) {
        ok = put(d_seg_i, io->seg_i + (size_t)k * segs * 8, segs * 8) && put(d_seg_count, io->seg_count + (size_t)k * n, n) && put(d_seg_out, io->seg_out + (size_t)k * S * 4, S * 4)
          && put(d_meta_out, io->row_meta_out + (size_t)k * R * 8, R * 8) && put(d_feat_out, io->row_feat_out + (size_t)k * R * WSA_NFEAT, R * WSA_NFEAT)
          && put(d_row_off, io->clip_row_off + (size_t)k * n1, n1) && put(d_seg_off, io->clip_seg_off + (size_t)k * n1, n1) && put(d_totals, io->totals + (size_t)k * 4, 4)
          && (!streams || put(d_ctl, io->ctl + (size_t)k * n, n));
        if (!ok) break;
        CompactParams cp;
        cp.n_clips = n; cp.seg_cap = (int)seg_cap; cp.level = io->level; cp.seg_i = d_seg_i; cp.seg_count = d_seg_count; cp.row_meta_in = d_meta_in; cp.row_feat_in = d_feat_in;
        cp.seg_out = d_seg_out; cp.row_meta_out = d_meta_out; cp.row_feat_out = d_feat_out; cp.clip_row_off = d_row_off; cp.clip_seg_off = d_seg_off; cp.totals = d_totals;
        if (streams) {
            launch_stream_prepare(d_state, d_carry, nullptr, d_ctl, n, 0.0, 0.0, nullptr);
            cp.carry = d_carry; cp.ctl = d_ctl;
        } else {
            cp.clip_rows = d_clip_rows; cp.flags = d_counters + 1; cp.fused = io->fused ? 1 : 0; cp.host = io->give_host ? h_host_dev : nullptr;
            cp.clr_counters = io->give_clr ? d_counters : nullptr; cp.clr_hist = io->give_clr ? d_hist : nullptr;
        }
        io->path[k] = compact_path(cp);
        launch_compact(cp, nullptr);
        ok = ran() && down(io->seg_out + (size_t)k * S * 4, d_seg_out, S * 4) && down(io->row_meta_out + (size_t)k * R * 8, d_meta_out, R * 8)
          && down(io->row_feat_out + (size_t)k * R * WSA_NFEAT, d_feat_out, R * WSA_NFEAT) && down(io->clip_row_off + (size_t)k * n1, d_row_off, n1)
          && down(io->clip_seg_off + (size_t)k * n1, d_seg_off, n1) && down(io->totals + (size_t)k * 4, d_totals, 4)
          && (!streams || down(io->carry + (size_t)k * n * CARRY_WORDS, d_carry, (size_t)n * CARRY_WORDS));
    }
    ok = ok && down(io->counters, d_counters, 16) && down(io->hist, d_hist, (size_t)SPAN_BUCKETS);
    if (ok) for (int q = 0; q < 4; q++) io->host4[q] = h_host[q];
    return ok ? WSA_OK : WSA_ERR_HIP;
}
