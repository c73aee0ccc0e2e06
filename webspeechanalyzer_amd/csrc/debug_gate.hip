// debug_gate.hip — test entries of libwsa that are NOT part of include/wsa.h, for K1b (csrc/peaks.hip: launch_peaks, launch_peaks_mode), K2a (csrc/gate.hip:
// launch_gate_blocks, launch_gate_stream_blocks) and the span order behind the batch gate (csrc/tracker.hip launch_span_order): host spectra in, the kernels'
// tables back as they are.  The two peaks entries share one buffer layout, the gate and the span order one set-up and one batch scan.
#include <cstring>
#include <vector>
#include "api_internal.hpp"
#include "debug_internal.hpp"

using namespace wsa_debug;

namespace {
using namespace wsa;

// the peaks entries' device buffer: spectra, hdr [n_frames][4], amp [n_frames * 64], ent [n_frames * 64][4] and the flag word, each at a multiple of 256 bytes
// of ONE zero-filled allocation, and the PkParams over it
struct PeaksRig {
    DevArena A; char* d = nullptr; PkParams p{};
    size_t nh = 0, na = 0, ne = 0, o_h = 0, o_a = 0, o_e = 0, o_f = 0;
    bool set(const uint32_t* spec, uint32_t n_frames, int32_t bands) {
        const auto pad = [](size_t bytes) { return (bytes + 255) & ~(size_t)255; };
        const size_t nsp = (size_t)n_frames * bands * 4;
        nh = (size_t)n_frames * 16; na = (size_t)n_frames * CAND_CAP * 4; ne = (size_t)n_frames * CAND_CAP * 16;
        o_h = pad(nsp); o_a = o_h + pad(nh); o_e = o_a + pad(na); o_f = o_e + pad(ne);
        if (!zeros(A, &d, o_f + 256) || !put(d, reinterpret_cast<const char*>(spec), nsp)) return false;
        p.spec = reinterpret_cast<const uint32_t*>(d);
        p.rec.hdr = reinterpret_cast<uint4*>(d + o_h); p.rec.amp = reinterpret_cast<uint32_t*>(d + o_a); p.rec.ent = reinterpret_cast<uint4*>(d + o_e);
        p.frame0 = 0; p.total_frames = n_frames; p.bands = bands; p.flags = reinterpret_cast<uint32_t*>(d + o_f);
        return true;
    }
};

// what wsa_debug_gate and wsa_debug_span_order set up alike.  plan() and caps() are host work in front of hipSetDevice; tables() and scan() need the device.
struct GateRig {
    wsa_config c{}; std::vector<uint32_t> foff; uint64_t total = 0; uint32_t max_frames = 0;       // plan()
    Derived D; int seg_cap = 0; uint32_t ring = 0;                                                  // caps()
    DevArena A; PkParams pk; GateParams g;                                                          // tables()
    uint32_t *d_spec = nullptr, *d_nfr = nullptr, *d_foff = nullptr, *d_seg_count = nullptr, *d_clip_rows = nullptr, *d_counters = nullptr;
    int32_t *d_info = nullptr, *d_seg_i = nullptr; double *d_v = nullptr, *d_fl = nullptr, *d_seg_d = nullptr;

    // the six settings into wsa_config and the clips' frame offsets, with their limits; false: refused
    bool plan(int32_t variant, const uint32_t* spec, const uint32_t* n_frames, uint32_t n_clips, int32_t bands, const double* settings6) {
        c.output_level = 5; c.N_mel_bins = bands; c.window_width = c.window_step = settings6[0]; c.pause_length = settings6[1]; c.min_seg_length = settings6[2];
        c.auto_noise_gate = settings6[3] != 0 ? 1 : 0; c.voiced_max_dB = settings6[4]; c.voiced_min_dB = settings6[5];
        if (!(c.window_step > 0) || !(c.pause_length >= 0) || !(c.min_seg_length >= 0)) return false;
        if (variant < 2 && !c.auto_noise_gate) return false;                           // the integer kernel's state is integers only under the auto gate
        foff.assign((size_t)n_clips + 1, 0);
        for (uint32_t i = 0; i < n_clips; i++) {
            if (n_frames[i] > (1u << 20)) return false;
            total += n_frames[i]; foff[i + 1] = (uint32_t)total; if (n_frames[i] > max_frames) max_frames = n_frames[i];
        }
        return total <= (1u << 22) && (!total || spec);
    }
    // seg_cap as the drivers size a clip's / a step's segment table, ring as a stream set of F frames per step and max_span sizes it (batches: 0)
    void caps(int32_t bands, bool streams, uint32_t F, uint32_t max_span) {
        D = Derived(c, bands);
        seg_cap = streams ? stream_seg_cap(F, D) : batch_seg_cap(max_frames, D);
        ring = streams ? stream_ring_frames(F, max_span) : 0;
    }
    // the tables both entries need, zero-filled, for `slots` frame records and `spec_rows` rows of spectra, and the two parameter blocks over them
    bool tables(int32_t variant, uint32_t n_clips, int32_t bands, size_t slots, size_t spec_rows) {
        const size_t segs = (size_t)n_clips * seg_cap;
        RecPtrs rec;
        if (!(zeros(A, &d_spec, spec_rows * bands + 4) && A.alloc(&d_nfr, n_clips) && A.upload(&d_foff, foff) && zeros(A, &rec.hdr, slots)
              && zeros(A, &rec.amp, slots * CAND_CAP) && zeros(A, &rec.ent, slots * CAND_CAP) && zeros(A, &d_info, slots) && zeros(A, &d_v, slots)
              && zeros(A, &d_fl, slots) && zeros(A, &d_seg_i, segs * 8) && zeros(A, &d_seg_d, segs * 2) && zeros(A, &d_seg_count, n_clips)
              && zeros(A, &d_clip_rows, n_clips) && zeros(A, &d_counters, 16))) return false;
        pk.spec = d_spec; pk.rec = rec; pk.bands = bands; pk.flags = d_counters + 8;
        g.rec = rec; g.n_frames = d_nfr; g.frame_off = d_foff; g.n_clips = n_clips; g.level = D.klevel; g.max_voiced_bin = D.max_voiced_bin; g.breaker = D.breaker;
        g.min_frames = D.min_frames; g.auto_gate = D.auto_gate; g.ctx_max0 = D.ctx_max0; g.floor0 = D.floor0; g.fr_info = d_info; g.fr_v = d_v; g.fr_fl = d_fl;
        g.seg_i = d_seg_i; g.seg_d = d_seg_d; g.seg_cap = seg_cap; g.seg_count = d_seg_count; g.clip_rows = d_clip_rows; g.counters = d_counters + 4; g.shared = d_counters;
        g.dbg = variant == 1 ? DBG_GATE_GENERAL : (variant == 2 ? DBG_GATE_F64 : 0);
        return true;
    }
    // a batch's frames and frame counts up and the peak scan over them.  WSA_ERR_INVALID, found only here and so after device work: a frame with more than
    // CAND_CAP candidates, whose table is cut short
    int scan(const uint32_t* spec, const uint32_t* n_frames, uint32_t n_clips, int32_t bands) {
        bool ok = put(d_nfr, n_frames, n_clips) && put(d_spec, spec, (size_t)total * bands);
        if (ok && total) {
            uint32_t cnt[16];
            pk.total_frames = (uint32_t)total;
            launch_peaks(pk, nullptr);
            ok = ran() && down(cnt, d_counters, 16);
            if (ok && (cnt[8] & 1u)) return WSA_ERR_INVALID;
        }
        return ok ? WSA_OK : WSA_ERR_HIP;
    }
};

// wsa_debug_gate's stream schedule stays inside the clips and the step buffer
bool schedule_fits(const uint32_t* n_frames, uint32_t n_clips, uint32_t F, uint32_t n_steps, const uint32_t* step_nfr, const uint32_t* step_ctl) {
    std::vector<uint64_t> fed(n_clips, 0);
    for (uint32_t k = 0; k < n_steps; k++)
        for (uint32_t i = 0; i < n_clips; i++) {
            const uint32_t nf = step_nfr[(size_t)k * n_clips + i];
            if (nf > F || (step_ctl[(size_t)k * n_clips + i] & ~3u)) return false;
            fed[i] += nf;
            if (fed[i] > n_frames[i]) return false;
        }
    return true;
}

// wsa_debug_gate, variant 3: one prepare + scan + gate per step, every step's tables copied back behind it
int gate_stream_steps(GateRig& R, const uint32_t* spec, uint32_t n_clips, int32_t bands, uint32_t blocks, uint32_t F, uint32_t n_steps, const uint32_t* step_nfr,
                      const uint32_t* step_ctl, int32_t* fr_info, double* fr_v, double* fr_fl, int32_t* fr_span, int32_t* seg_i, double* seg_d, uint32_t* seg_count,
                      uint32_t* flags2, double* state) {
    const uint32_t ring = R.ring;
    const size_t slots = (size_t)n_clips * ring, spec_rows = (size_t)n_clips * F, segs = (size_t)n_clips * R.seg_cap;
    int32_t *d_span = nullptr, *d_carry = nullptr; double* d_state = nullptr; uint32_t* d_ctl = nullptr;
    if (!(zeros(R.A, &d_span, slots) && zeros(R.A, &d_state, (size_t)n_clips * GATE_STATE) && zeros(R.A, &d_carry, (size_t)n_clips * CARRY_WORDS) && zeros(R.A, &d_ctl, n_clips)))
        return WSA_ERR_HIP;
    PkParams& pk = R.pk; GateParams& g = R.g;
    pk.stream_state = d_state; pk.n_frames = R.d_nfr; pk.step_frames = F; pk.ring = ring; pk.total_frames = n_clips * F;
    g.state = d_state; g.ctl = d_ctl; g.ring = ring; g.step_frames = F; g.fr_span = d_span;
    std::vector<uint32_t> hspec(spec_rows * bands), fed(n_clips, 0);
    std::vector<int32_t> h_info(slots), h_span(slots); std::vector<double> h_v(slots), h_fl(slots);
    uint32_t cnt[16];
    flags2[0] = 0; flags2[1] = 0;
    for (uint32_t k = 0; k < n_steps; k++) {
        const uint32_t* nf = step_nfr + (size_t)k * n_clips;
        for (uint32_t i = 0; i < n_clips; i++)
            if (nf[i]) memcpy(&hspec[(size_t)i * F * bands], spec + ((size_t)R.foff[i] + fed[i]) * bands, (size_t)nf[i] * bands * sizeof(uint32_t));
        const uint32_t zero16[16] = {0};
        if (!(put(R.d_spec, hspec.data(), hspec.size()) && put(R.d_nfr, nf, n_clips) && put(d_ctl, step_ctl + (size_t)k * n_clips, n_clips) && put(R.d_counters, zero16, 16)))
            return WSA_ERR_HIP;
        launch_stream_prepare(d_state, d_carry, nullptr, d_ctl, n_clips, R.D.ctx_max0, R.D.floor0, nullptr);
        launch_peaks(pk, nullptr);
        if (!(ran() && down(cnt, R.d_counters, 16))) return WSA_ERR_HIP;
        if (cnt[8] & 1u) return WSA_ERR_INVALID;
        launch_gate_stream_blocks(g, blocks, nullptr);
        if (!(ran() && down(cnt, R.d_counters, 16) && down(h_info.data(), R.d_info, slots) && down(h_span.data(), d_span, slots)
              && down(h_v.data(), R.d_v, slots) && down(h_fl.data(), R.d_fl, slots) && down(seg_i + (size_t)k * segs * 8, R.d_seg_i, segs * 8)
              && down(seg_d + (size_t)k * segs * 2, R.d_seg_d, segs * 2) && down(seg_count + (size_t)k * n_clips, R.d_seg_count, n_clips)
              && down(state + (size_t)k * n_clips * GATE_STATE, d_state, (size_t)n_clips * GATE_STATE))) return WSA_ERR_HIP;
        flags2[0] |= cnt[1]; if (cnt[4] > flags2[1]) flags2[1] = cnt[4];
        for (uint32_t i = 0; i < n_clips; i++) {
            // the stream's frame count after this step (state word 0) minus the step's frames = the absolute number of the step's first frame
            const uint32_t seen = (uint32_t)state[((size_t)k * n_clips + i) * GATE_STATE] - nf[i];
            for (uint32_t j = 0; j < nf[i]; j++) {
                const size_t slot = (size_t)i * ring + ((seen + j) & (ring - 1)), dst = (size_t)R.foff[i] + fed[i] + j;
                fr_info[dst] = h_info[slot]; fr_span[dst] = h_span[slot]; fr_v[dst] = h_v[slot]; fr_fl[dst] = h_fl[slot];
            }
            fed[i] += nf[i];
        }
    }
    return WSA_OK;
}
}  // namespace

// the peak-candidate scan on its own: `spec` = n_frames rows of `bands` u32 (host); mode as launch_peaks_mode takes it: 0 = by size, 1 = one lane per
// frame, 2 = one wave per frame (up to 128 bands; wider frames fall to the lane kernel), 3 / 4 = one lane per frame in rounds of 16 / 32 bins
// (peaks_kernel<16> / <32>); out: hdr [n_frames][4], amp [n_frames * 64], ent [n_frames * 64][4] (u32, candidate tables zero-filled beforehand), flags
extern "C" int wsa_debug_peaks(int32_t device, const uint32_t* spec, uint32_t n_frames, int32_t bands, int32_t mode,
                               uint32_t* hdr, uint32_t* amp, uint32_t* ent, uint32_t* flags) {
    if (!spec || !hdr || !amp || !ent || !flags || bands < 1 || n_frames < 1) return WSA_ERR_INVALID;
    if (hipSetDevice(device) != hipSuccess) return WSA_ERR_NO_DEVICE;
    PeaksRig R;
    bool ok = R.set(spec, n_frames, bands);
    if (ok) {
        wsa::launch_peaks_mode(R.p, mode, nullptr);
        ok = ran() && down(reinterpret_cast<char*>(hdr), R.d + R.o_h, R.nh) && down(reinterpret_cast<char*>(amp), R.d + R.o_a, R.na)
             && down(reinterpret_cast<char*>(ent), R.d + R.o_e, R.ne) && down(reinterpret_cast<char*>(flags), R.d + R.o_f, 4);
    }
    return ok ? WSA_OK : WSA_ERR_HIP;
}

// timing of the peak-candidate scan on its own (tuning): the same frames `reps` times, average kernel time in ms; dbg = PkParams::dbg (PK_DBG_* bits)
extern "C" int wsa_debug_peaks_time(int32_t device, const uint32_t* spec, uint32_t n_frames, int32_t bands, int32_t mode, int32_t dbg, int32_t reps, float* ms) {
    if (!spec || !ms || bands < 1 || n_frames < 1 || reps < 1) return WSA_ERR_INVALID;
    if (hipSetDevice(device) != hipSuccess) return WSA_ERR_NO_DEVICE;
    PeaksRig R;
    bool ok = R.set(spec, n_frames, bands);
    hipEvent_t e0 = nullptr, e1 = nullptr;
    ok = ok && hipEventCreate(&e0) == hipSuccess && hipEventCreate(&e1) == hipSuccess;
    if (ok) {
        R.p.dbg = dbg;
        wsa::launch_peaks_mode(R.p, mode, nullptr);
        (void)hipEventRecord(e0, nullptr);
        for (int r = 0; r < reps; r++) wsa::launch_peaks_mode(R.p, mode, nullptr);
        (void)hipEventRecord(e1, nullptr);
        ok = ran() && hipEventElapsedTime(ms, e0, e1) == hipSuccess;
        *ms /= (float)reps;
    }
    if (e0) (void)hipEventDestroy(e0);
    if (e1) (void)hipEventDestroy(e1);
    return ok ? WSA_OK : WSA_ERR_HIP;
}

// K2a (csrc/gate.hip) on its own: host spectra through the peak scan and ONE gate variant, the gate's outputs copied back as they are.
//   variant 0: the integer kernel with its runs (gate_kernel_auto<false>)      1: the integer kernel, every frame through the general path (<true>, WSA_DBG 4096)
//           2: the f64 lane-per-candidate kernel (gate_kernel_t<false>; what a fixed gate uses, and WSA_DBG 2048)      3: the stream step kernel (gate_kernel_t<true>)
// spec = the clips' frames one after the other ([sum n_frames][bands] u32), settings6 = {window_step, pause_length, min_seg_length, auto_noise_gate, voiced_max_dB,
// voiced_min_dB}; blocks = workgroups of the gate launch (0: one per clip; fewer: a workgroup walks several clips).
// caps_io = {seg_cap, ring}: called with seg_cap 0 the entry only fills in both (seg_cap as the drivers size a clip's / a step's segment table from host_plan.hpp's
// period, ring as a stream set of F frames per step and max_span sizes it) and runs nothing; a run must be handed the same numbers back.
// Batch (variants 0 .. 2) out: fr_info / fr_v / fr_fl [sum n_frames], seg_i [n_clips][seg_cap][8], seg_d [n_clips][seg_cap][2], seg_count [n_clips], flags2 = {the overflow
// flag word, counters[0]}; fr_span and state are not touched.
// Streams (variant 3): clip c is stream c; step k feeds it its next step_nfr[k][c] <= F frames under step_ctl[k][c] (bit 0 START: launch state first, bit 1 STOP:
// segment_truncate behind the frames), launch_stream_prepare + the peak scan + launch_gate_stream once per step.  Out: the per-frame arrays (fr_span too) at the frames'
// place in their clip, read from their ring slot right behind their step; seg_i [n_steps][n_clips][seg_cap][8], seg_d, seg_count [n_steps][n_clips] and state
// [n_steps][n_clips][GATE_STATE] per step; flags2 = {OR of the flag words, largest counters[0]}.  Frames never fed keep what the caller put there.
// Refused, nothing run: the integer kernel under a fixed gate, more than CAND_CAP candidates in a frame (reported after the scan, the gate not run), a step that
// feeds more than F frames or more than the clip has left, a ring the caller did not get from here.
extern "C" int wsa_debug_gate(int32_t device, int32_t variant, const uint32_t* spec, const uint32_t* n_frames, uint32_t n_clips, int32_t bands, const double* settings6,
                              uint32_t blocks, uint32_t F, uint32_t max_span, uint32_t n_steps, const uint32_t* step_nfr, const uint32_t* step_ctl, int32_t* caps_io,
                              int32_t* fr_info, double* fr_v, double* fr_fl, int32_t* fr_span, int32_t* seg_i, double* seg_d, uint32_t* seg_count, uint32_t* flags2, double* state) {
    using namespace wsa;
    if (!n_frames || !settings6 || !caps_io || variant < 0 || variant > 3 || n_clips < 1 || n_clips > 4096 || bands < 4 || bands > 256) return WSA_ERR_INVALID;
    const bool streams = variant == 3;
    GateRig R;
    if (!R.plan(variant, spec, n_frames, n_clips, bands, settings6)) return WSA_ERR_INVALID;
    if (streams && (F < 1 || F > 4096 || n_steps < 1 || n_steps > (1u << 20) || !step_nfr || !step_ctl || max_span > (1u << 16))) return WSA_ERR_INVALID;
    R.caps(bands, streams, F, max_span);
    if (caps_io[0] == 0) { caps_io[0] = R.seg_cap; caps_io[1] = (int32_t)R.ring; return WSA_OK; }
    if (caps_io[0] != R.seg_cap || caps_io[1] != (int32_t)R.ring) return WSA_ERR_INVALID;
    if (!fr_info || !fr_v || !fr_fl || !seg_i || !seg_d || !seg_count || !flags2 || (streams && (!fr_span || !state))) return WSA_ERR_INVALID;
    if (streams && !schedule_fits(n_frames, n_clips, F, n_steps, step_nfr, step_ctl)) return WSA_ERR_INVALID;
    if (hipSetDevice(device) != hipSuccess) return WSA_ERR_NO_DEVICE;
    const size_t total = (size_t)R.total, segs = (size_t)n_clips * R.seg_cap;
    // frame records and per-frame outputs: one per frame, or one per ring slot; spectra: every frame, or one step's
    if (!R.tables(variant, n_clips, bands, streams ? (size_t)n_clips * R.ring : total, streams ? (size_t)n_clips * F : total)) return WSA_ERR_HIP;
    if (streams)
        return gate_stream_steps(R, spec, n_clips, bands, blocks, F, n_steps, step_nfr, step_ctl, fr_info, fr_v, fr_fl, fr_span, seg_i, seg_d, seg_count, flags2, state);
    if (const int refused = R.scan(spec, n_frames, n_clips, bands)) return refused;
    launch_gate_blocks(R.g, blocks, nullptr);
    uint32_t cnt[16];
    const bool ok = ran() && down(cnt, R.d_counters, 16) && down(fr_info, R.d_info, total) && down(fr_v, R.d_v, total) && down(fr_fl, R.d_fl, total)
                 && down(seg_i, R.d_seg_i, segs * 8) && down(seg_d, R.d_seg_d, segs * 2) && down(seg_count, R.d_seg_count, n_clips);
    if (ok) { flags2[0] = cnt[1]; flags2[1] = cnt[4]; }
    return ok ? WSA_OK : WSA_ERR_HIP;
}

// The span order on its own: wsa_debug_gate's batch form (variants 0 .. 2, `blocks`, the same settings6 and caps_io) with the gate's counting switched on
// — span_hist / span_key set as the batch driver sets them — and launch_span_order behind it.  Out: seg_i [n_clips][seg_cap][8], seg_count [n_clips], hist
// [SPAN_BUCKETS] (zero before the gate, as the batch's clear leaves it), key [n_clips][seg_cap][2] and order [n_clips * seg_cap][2] (both go to the device as
// the caller filled them: a slot nobody writes keeps its value), counters4 = counters[0 .. 3] as the driver hands them to launch_span_order.
// Refused, nothing run: what wsa_debug_gate refuses for a batch, and the stream variant.  One refusal comes AFTER the peak scan has run (as in wsa_debug_gate):
// a frame with more than CAND_CAP candidates, which only the scan finds — the gate and the span order are then not run, and nothing is written to the caller.
extern "C" int wsa_debug_span_order(int32_t device, int32_t variant, const uint32_t* spec, const uint32_t* n_frames, uint32_t n_clips, int32_t bands, const double* settings6,
                                    uint32_t blocks, int32_t* caps_io, int32_t* seg_i, uint32_t* seg_count, uint32_t* hist, uint32_t* key, uint32_t* order, uint32_t* counters4) {
    using namespace wsa;
    if (!n_frames || !settings6 || !caps_io || variant < 0 || variant > 2 || n_clips < 1 || n_clips > 4096 || bands < 4 || bands > 256) return WSA_ERR_INVALID;
    GateRig R;
    if (!R.plan(variant, spec, n_frames, n_clips, bands, settings6)) return WSA_ERR_INVALID;
    R.caps(bands, false, 0, 0);
    if (caps_io[0] == 0) { caps_io[0] = R.seg_cap; return WSA_OK; }
    if (caps_io[0] != R.seg_cap || !seg_i || !seg_count || !hist || !key || !order || !counters4) return WSA_ERR_INVALID;
    if (hipSetDevice(device) != hipSuccess) return WSA_ERR_NO_DEVICE;
    const size_t total = (size_t)R.total, segs = (size_t)n_clips * R.seg_cap;
    uint32_t *d_hist = nullptr, *d_key = nullptr, *d_order = nullptr;
    if (!(R.tables(variant, n_clips, bands, total, total) && zeros(R.A, &d_hist, (size_t)SPAN_BUCKETS) && up(R.A, &d_key, key, segs * 2) && up(R.A, &d_order, order, segs * 2)))
        return WSA_ERR_HIP;
    if (const int refused = R.scan(spec, n_frames, n_clips, bands)) return refused;
    R.g.span_hist = d_hist; R.g.span_key = reinterpret_cast<uint2*>(d_key);
    launch_gate_blocks(R.g, blocks, nullptr);
    TrParams t;
    t.n_clips = n_clips; t.seg_count = R.d_seg_count; t.seg_cap = R.seg_cap; t.seg_i = R.d_seg_i;
    launch_span_order(t, d_hist, reinterpret_cast<const uint2*>(d_key), reinterpret_cast<uint2*>(d_order), R.d_counters + 4, nullptr);
    uint32_t cnt[16];
    const bool ok = ran() && down(cnt, R.d_counters, 16) && down(seg_i, R.d_seg_i, segs * 8) && down(seg_count, R.d_seg_count, n_clips) && down(hist, d_hist, (size_t)SPAN_BUCKETS)
                 && down(key, d_key, segs * 2) && down(order, d_order, segs * 2);
    if (ok) for (int q = 0; q < 4; q++) counters4[q] = cnt[4 + q];
    return ok ? WSA_OK : WSA_ERR_HIP;
}
