// host_plan.hpp — what the two host-side drivers of the kernel chain (batch_*.hip: batches, stream_*.hip: lock-step stream sets) plan in the
// same way: device memory ownership, the front end's device tables, the rules that come from the reference's configuration, the back end's
// buffers with the common part of every kernel parameter block, the level-3 raw-track gather and the rate check.  Nothing here is exported.
#pragma once
#include <cmath>
#include <cstring>
#include <string>
#include <vector>
#include "api_internal.hpp"

namespace wsa {

constexpr size_t LDS_LIMIT = 160 * 1024;      // dynamic LDS one workgroup may have (front-end tables, the stream rate converter's input window)

// ---- device memory of one object (batch, stream set, model, classifier state): everything handed out here is freed by release() / the destructor.
// The owner's destroy function calls hipSetDevice before it deletes the object.
struct DevArena {
    std::vector<void*> dev, pinned;
    size_t dev_bytes = 0;                      // device bytes handed out (wsa_batch_info::workspace_bytes)
    DevArena() = default;
    DevArena(const DevArena&) = delete;
    DevArena& operator=(const DevArena&) = delete;
    ~DevArena() { release(); }
    void release() {
        for (void* p : dev) (void)hipFree(p);
        for (void* p : pinned) (void)hipHostFree(p);
        dev.clear(); pinned.clear(); dev_bytes = 0;
    }
    template <typename T>
    bool alloc(T** p, size_t count, bool zero = false) {
        const size_t bytes = (count ? count : 1) * sizeof(T);
        void* q = nullptr;
        if (hipMalloc(&q, bytes) != hipSuccess) return false;
        dev.push_back(q); dev_bytes += bytes;
        *p = reinterpret_cast<T*>(q);
        return !zero || hipMemset(q, 0, bytes) == hipSuccess;
    }
    template <typename T, typename U>
    bool upload(T** p, const std::vector<U>& v) {
        static_assert(sizeof(U) <= sizeof(T) && sizeof(T) % sizeof(U) == 0, "upload type");
        return alloc(p, v.size() * sizeof(U) / sizeof(T)) && (v.empty() || hipMemcpy(*p, v.data(), v.size() * sizeof(U), hipMemcpyHostToDevice) == hipSuccess);
    }
    // mapped pinned host memory, zeroed: *host for the CPU, *device for kernels
    template <typename T>
    bool pin(T** host, T** device, size_t count) {
        const size_t bytes = (count ? count : 1) * sizeof(T);
        void* q = nullptr;
        if (hipHostMalloc(&q, bytes, hipHostMallocMapped) != hipSuccess) return false;
        pinned.push_back(q);
        std::memset(q, 0, bytes);
        *host = reinterpret_cast<T*>(q);
        return hipHostGetDevicePointer(reinterpret_cast<void**>(device), q, 0) == hipSuccess;
    }
};

// ---- the front end's plan on the device: the host plan, its ten tables, the tap bounds the kernel is launched with
struct FeDev {
    FePlanHost plan;
    int mel_max_taps = 0, mel_max_taps_lo = 0;      // most taps of any band / of the bands below 64
    float *d_window = nullptr, *d_mel_w = nullptr, *d_emph = nullptr;
    float2 *d_tw_n2 = nullptr, *d_tw_64 = nullptr, *d_tw_nfft = nullptr, *d_tw_m = nullptr;
    int32_t *d_mel_k0 = nullptr, *d_mel_cnt = nullptr, *d_mel_off = nullptr;
    enum Refusal { OK = 0, BAD_CONFIG, BAD_FFT, LDS };      // `err` says why; the batch driver words BAD_FFT itself and adds advice to LDS
    // the kernel keeps its tables (window, twiddles, mel taps / power rows) in LDS: a geometry that needs more than a workgroup may have is refused here, not at the first launch
    Refusal build(const wsa_config& cfg, double fs, bool fat, std::string& err) {
        if (!build_fe_plan(cfg, fs, plan, err)) return BAD_CONFIG;
        if (!fe_supported_R(plan.R, plan.three)) { err = "unsupported FFT length for this sample rate / band setting"; return BAD_FFT; }
        if (const size_t need = fe_lds_required(plan, fat); need > LDS_LIMIT) {
            err = "this window / band setting needs " + std::to_string(need) + " bytes of LDS for the front end's tables (limit " + std::to_string(LDS_LIMIT) + ")";
            return LDS;
        }
        for (size_t i = 0; i < plan.mel_cnt.size(); i++) {
            if (plan.mel_cnt[i] > mel_max_taps) mel_max_taps = plan.mel_cnt[i];
            if (i < 64 && plan.mel_cnt[i] > mel_max_taps_lo) mel_max_taps_lo = plan.mel_cnt[i];
        }
        return OK;
    }
    bool upload(DevArena& A) {
        const FePlanHost& P = plan;
        return A.upload(&d_window, P.window) && A.upload(&d_tw_n2, P.tw_n2) && A.upload(&d_tw_m, P.tw_m) && A.upload(&d_tw_64, P.tw_64)
            && A.upload(&d_tw_nfft, P.tw_nfft) && A.upload(&d_mel_k0, P.mel_k0) && A.upload(&d_mel_cnt, P.mel_cnt)
            && A.upload(&d_mel_off, P.mel_off) && A.upload(&d_mel_w, P.mel_w) && A.upload(&d_emph, P.emph);
    }
    // the plan-constant fields; a driver adds pcm, clip_stride, n_frames, frame_off, spec, frames_per_wave and what only it uses
    void fill(FeParams& p, bool fat) const {
        const FePlanHost& P = plan;
        p.win = P.win; p.hop = P.hop; p.kmax = P.kmax; p.bands = P.bands; p.spec_type = P.spec_type; p.mel_total = (int)P.mel_w.size();
        p.mel_max_taps = mel_max_taps; p.mel_max_taps_lo = mel_max_taps_lo; p.fat = fat ? 1 : 0;
        p.window = d_window; p.tw_n2 = d_tw_n2; p.tw_64 = d_tw_64; p.tw_nfft = d_tw_nfft; p.tw_m = d_tw_m;
        p.mel_k0 = d_mel_k0; p.mel_cnt = d_mel_cnt; p.mel_off = d_mel_off; p.mel_w = d_mel_w; p.emph = d_emph; p.gain = P.gain;
    }
};

// ---- what the reference's configuration object decides for the back end (ref dist/main.js:2 inner module 1)
struct Derived {
    int level = 0, klevel = 0, period = 1, max_voiced_bin = 0, auto_gate = 0;
    double breaker = 0, min_frames = 0, ctx_max0 = 0, floor0 = 0;
    bool has_formants = false, syllable_rows = false, raw_tracks = false, tail_kernel = false;
    Derived() = default;
    Derived(const wsa_config& c, int bands) {
        level = c.output_level;
        tail_kernel = level == 11 || level == 12;                         // K4 / K5 run behind the compaction ...
        klevel = tail_kernel ? 10 : c.output_level;                       // ... on what level 10 stores (12: + the energy sums; ref @B27713, @B27240)
        has_formants = level == 4 || klevel == 10;                        // straightened frames [frames][9]
        syllable_rows = klevel == 10 || level == 13;                      // rows per syllable, not per segment
        raw_tracks = level == 3;                                          // ref @B28273
        max_voiced_bin = (int)std::trunc(0.7 * bands);                                                         // ref @B25136
        breaker = c.pause_length > 2 * c.window_step ? c.pause_length / c.window_step : 250 / c.window_step;   // ref @B25188
        min_frames = std::trunc(c.min_seg_length / c.window_step);                                             // ref @B25218
        period = (int)min_frames + 1 + (int)std::floor(breaker);          // fewest frames from one segment's start to the next one's
        if (period < 1) period = 1;
        auto_gate = c.auto_noise_gate ? 1 : 0;
        if (auto_gate) { ctx_max0 = 50; floor0 = 2; }                                                          // ref @B25471
        else { ctx_max0 = std::pow(10.0, c.voiced_max_dB / 20); floor0 = std::pow(10.0, c.voiced_min_dB / 20); }
    }
};

// capacities that follow from `period` (DESIGN.md "capacities"): segments a clip of max_frames frames can finalize (+ the one segment_truncate adds, + 1),
// segments one step of F frames can close (+ the ones STOP and a ring cut add), and a stream's ring: max_span frames of an open span plus one more step
inline int batch_seg_cap(uint32_t max_frames, const Derived& D) { return (int)max_frames / D.period + 2; }
inline int stream_seg_cap(uint32_t F, const Derived& D) { return (int)F / D.period + 3; }
inline uint32_t stream_ring_frames(uint32_t F, uint32_t max_span_frames) {
    uint32_t want = max_span_frames ? max_span_frames : 1024u;
    if (want < 2 * F + 64) want = 2 * F + 64;
    uint32_t ring = 64; while (ring < want + F) ring <<= 1;
    return ring;
}

// ---- the back end's buffers, embedded by wsa_batch (n = clips, frames = all frames of the batch) and wsa_stream (n = streams, frames = n rings),
// and the part of each kernel parameter block that follows from them.  A driver writes the rest: only the fields it means.
struct BackEnd {
    uint32_t n = 0;
    int seg_cap = 0, row_cap = 0, tcap = 0, pcap = 0, fcap = 0;
    size_t ws_stride = 0;
    RecPtrs rec = {nullptr, nullptr, nullptr};      // frame records (wsa_internal.hpp)
    char* d_ws = nullptr;                           // tracker work spaces
    int32_t *d_fr_info = nullptr, *d_seg_i = nullptr, *d_meta_pool = nullptr, *d_meta = nullptr, *d_seg = nullptr;
    double *d_fr_v = nullptr, *d_fr_fl = nullptr, *d_seg_d = nullptr, *d_feat_pool = nullptr, *d_feat = nullptr;
    uint32_t *d_seg_count = nullptr, *d_clip_rows = nullptr, *d_counters = nullptr, *d_row_off = nullptr, *d_seg_off = nullptr, *d_totals = nullptr;
    float* d_formants = nullptr;                    // levels 4 / 10 / 11 / 12: [frames][9]
    float* d_sums = nullptr; double* d_coef_ws = nullptr;                                          // level 12
    int4* d_trk_pts = nullptr; int32_t *d_trk_rank = nullptr, *d_trk_seg = nullptr;                // level 3: raw-track pools, per segment {pool offset lo, points, ranked, offset hi}
    int32_t* d_utt_meta = nullptr; double* d_utt_feat = nullptr; uint32_t* d_utt_off = nullptr;    // level 11

    // capacity bounds (DESIGN.md "capacities") from the most frames one span can hold: the longest clip, or the ring.  seg_cap and row_cap are the
    // driver's: a batch bounds them by the clip, a stream by what one step can close (+ the segments STOP and a ring cut add)
    void set_caps(const Derived& D, int bands, uint32_t frame_bound) {
        fcap = (int)frame_bound + 2;
        tcap = ((bands + 1) / 2) * fcap; pcap = tcap;
        ws_stride = tracker_ws_bytes(tcap, pcap, fcap, D.raw_tracks);
    }
    // everything but d_ws, d_counters, d_coef_ws and the level-3 pools, whose sizes are the driver's.  zero_state: a stream's buffers that carry state between steps start at zero
    bool alloc(DevArena& A, const Derived& D, size_t frames, bool zero_state) {
        const size_t segs = (size_t)n * seg_cap, rows = (size_t)n * row_cap;
        bool ok = true;
        if (D.level > 2) {
            ok = A.alloc(&rec.hdr, frames) && A.alloc(&rec.amp, frames * CAND_CAP) && A.alloc(&rec.ent, frames * CAND_CAP)
              && A.alloc(&d_fr_info, frames) && A.alloc(&d_fr_v, frames) && A.alloc(&d_fr_fl, frames)
              && A.alloc(&d_seg_i, segs * 8) && A.alloc(&d_seg_d, segs * 2) && A.alloc(&d_seg_count, n, zero_state) && A.alloc(&d_clip_rows, n, zero_state)
              && A.alloc(&d_meta_pool, rows * 8) && A.alloc(&d_feat_pool, rows * WSA_NFEAT) && A.alloc(&d_meta, rows * 8) && A.alloc(&d_feat, rows * WSA_NFEAT)
              && A.alloc(&d_seg, segs * 4)
              && (!D.has_formants || A.alloc(&d_formants, frames * 9, zero_state))
              && (!D.raw_tracks || A.alloc(&d_trk_seg, segs * 4, zero_state))
              && (D.level != 12 || A.alloc(&d_sums, frames, zero_state))
              && (D.level != 11 || (A.alloc(&d_utt_meta, segs * 4) && A.alloc(&d_utt_feat, segs * WSA_NUTT) && A.alloc(&d_utt_off, (size_t)n + 1)));
        }
        return ok && A.alloc(&d_row_off, (size_t)n + 1) && A.alloc(&d_seg_off, (size_t)n + 1) && A.alloc(&d_totals, 4, zero_state);
    }
    void fill(GateParams& g, const Derived& D) const {
        g.rec = rec; g.n_clips = n; g.level = D.klevel; g.max_voiced_bin = D.max_voiced_bin; g.breaker = D.breaker; g.min_frames = D.min_frames;
        g.auto_gate = D.auto_gate; g.ctx_max0 = D.ctx_max0; g.floor0 = D.floor0;
        g.fr_info = d_fr_info; g.fr_v = d_fr_v; g.fr_fl = d_fr_fl;
        g.seg_i = d_seg_i; g.seg_d = d_seg_d; g.seg_cap = seg_cap; g.seg_count = d_seg_count; g.clip_rows = d_clip_rows;
        g.counters = d_counters + 4; g.shared = d_counters;      // counters[4]: largest per-clip segment count, counters[1]: flags
    }
    void fill(TrParams& t, const Derived& D) const {
        t.rec = rec; t.level = D.klevel; t.fr_info = d_fr_info; t.fr_v = d_fr_v; t.fr_fl = d_fr_fl;
        t.seg_i = d_seg_i; t.seg_d = d_seg_d; t.seg_cap = seg_cap; t.seg_count = d_seg_count; t.n_clips = n; t.counters = d_counters + 4; t.shared = d_counters;
        t.ws = d_ws; t.ws_stride = ws_stride; t.tcap = tcap; t.pcap = pcap; t.fcap = fcap;
        t.row_meta = d_meta_pool; t.row_feat = d_feat_pool; t.row_cap = (uint32_t)row_cap; t.clip_rows = d_clip_rows;
        t.formants = d_formants; t.sums = d_sums; t.trk_pts = d_trk_pts; t.trk_rank = d_trk_rank; t.trk_seg = d_trk_seg;
    }
    void fill(CompactParams& cp, const Derived& D) const {
        cp.n_clips = n; cp.seg_cap = seg_cap; cp.level = D.klevel;
        cp.seg_i = d_seg_i; cp.seg_count = d_seg_count; cp.row_meta_in = d_meta_pool; cp.row_feat_in = d_feat_pool;
        cp.seg_out = d_seg; cp.row_meta_out = d_meta; cp.row_feat_out = d_feat;
        cp.clip_row_off = d_row_off; cp.clip_seg_off = d_seg_off; cp.totals = d_totals;
    }
    void fill(UttParams& u, const uint32_t* frame_off) const {
        u.n_clips = n; u.segments = d_seg; u.row_meta = d_meta; u.clip_seg_off = d_seg_off; u.clip_row_off = d_row_off;
        u.frame_off = frame_off; u.formants = d_formants; u.clip_utt_off = d_utt_off; u.utt_meta = d_utt_meta; u.utt_feat = d_utt_feat; u.totals = d_totals;
    }
    void fill(CoefParams& q, const uint32_t* frame_off) const {
        q.row_meta = d_meta; q.row_feat = d_feat; q.frame_off = frame_off; q.totals = d_totals; q.formants = d_formants; q.sums = d_sums;
        q.ws = d_coef_ws;          // (a fit that numeric would have thrown out of is reported per row, in slot 23: no flag word)
    }
};

// ---- level 3, batch and streams: the ranked raw tracks of the segments, out of the pools into the caller's tables by one gather kernel into a
// staging buffer and two copies (a copy per segment was ~12 000 small copies for a 1024-clip batch).  add() the segments in hand-out order, then run()
struct TrackGather {
    std::vector<uint64_t> desc;                     // per segment {first pool entry (absolute), base of its pool region, points, ranked ids, points / ranked ids in front}
    uint64_t n_points = 0, n_ranked = 0;
    char* d_stage = nullptr; size_t stage_cap = 0;  // [descriptors][points: 8 ints each][ranked ids]; an allocation of its own, grows on demand
    ~TrackGather() { if (d_stage) (void)hipFree(d_stage); }
    uint32_t segments() const { return (uint32_t)(desc.size() / 6); }
    void begin() { desc.clear(); n_points = n_ranked = 0; }
    // quad: the segment's {pool offset lo, points, ranked, offset hi} as the tracker left it (TrParams::trk_seg)
    void add(const int32_t* quad, uint64_t region_base) {
        const uint64_t pool0 = (uint64_t)(uint32_t)quad[0] | ((uint64_t)(uint32_t)quad[3] << 32);
        const uint64_t d[6] = {pool0, region_base, (uint32_t)quad[1], (uint32_t)quad[2], n_points, n_ranked};
        desc.insert(desc.end(), d, d + 6);
        n_points += d[2]; n_ranked += d[3];
    }
    void offsets(uint64_t* off) const {             // [segments + 1][2]
        const uint32_t ns = segments();
        for (uint32_t q = 0; q < ns; q++) { off[2 * q] = desc[6 * (size_t)q + 4]; off[2 * q + 1] = desc[6 * (size_t)q + 5]; }
        off[2 * (size_t)ns] = n_points; off[2 * (size_t)ns + 1] = n_ranked;
    }
    // region: entries of one pool region (a stream's ring of ring * 64; a batch's pool does not wrap: 2^63).  The copies are queued on s: the caller synchronises
    wsa_status run(wsa_ctx* ctx, uint64_t region, const int4* pts, const int32_t* rank, int32_t* points, int32_t* ranked, hipStream_t s);
};

// wsa_batch_create_resampled (n = 1, what = nullptr), wsa_batch_create_mixed ("clip"), wsa_stream_create_mixed ("stream")
inline wsa_status check_rates(wsa_ctx* ctx, const double* fs_in, uint32_t n, double fs_out, const char* what) {
    const std::string msg = "sample rates must be positive and at most a factor 16 apart";
    if (!(fs_out > 0)) return wsa_api::fail(ctx, WSA_ERR_INVALID, msg);
    for (uint32_t i = 0; i < n; i++)
        if (!(fs_in[i] > 0) || fs_in[i] / fs_out > 16 || fs_out / fs_in[i] > 16)
            return wsa_api::fail(ctx, WSA_ERR_INVALID, what ? msg + " (" + what + " " + std::to_string(i) + ")" : msg);
    return WSA_OK;
}

}  // namespace wsa
