// tracker.hip — K2b: formant tracking + segment finalize, ONE WAVEFRONT PER SEGMENT SPAN.
//
// Stands in for (ref = /root/reference/dist/main.js line 2, byte offsets):
//   accumulate_fm x(e,t,n,r,a) + match score _    @B35952, @B37340
//   the result part of finalize O(e)              @B27190-28506
//   get_ranked_formants y(), straighten m()       @B35670, @B35074
//   sep_syllables p(), formant_features u()       @B34757, @B32369 (+ stats helpers @B1978-2277; the feature reduction: tracker_features.hpp)
//   clear_fm                                      @B35919
// including the reference's quirks: stale first-frame filing index, first-peak
// amplitude of a merged association, fp32 storage in straighten, and the segments_ci entry that
// survives a throwing straighten step.
//
// The tracker (`l`, `s`, `c` of ref module 4) is cleared by every reset_segment, so the frames
// between two resets form an independent span; gate.hip (K2a) has already decided which spans end in
// a finalize and with which arguments accumulate_fm is called on each frame.  Spans are dealt out to the
// waves statically.  All decision arithmetic is IEEE double exactly as JavaScript Numbers (-ffp-contract=off;
// Math.log10 from jsmath_device.hpp).  Lanes parallelise the inner loops: peak acceptance (lane =
// candidate), (track, peak) pair scoring (lane = pair), track update (lane = track), new tracks
// (lane = peak), ranking (lane = track), straighten (lane = frame), features (lane = formant).
#include <type_traits>
#include "wsa_internal.hpp"
#include "jsmath_device.hpp"
#include "wave_ops.hpp"
#include "tracker_score.hpp"
#include "tracker_features.hpp"

// Tuning switches of the tracker (the DBG_* bits of wsa_internal.hpp marked TUNING) exist only in a library built with
// `make TUNING=1`: a dozen tests of a kernel argument per frame are not free in a kernel that is bound by instruction issue.  The
// switches the tests use are always there and are tested as `p.dbg & DBG_...`.
#ifdef WSA_TUNING
#define WSA_TUNE(bits_) (p.dbg & (bits_))
#else
#define WSA_TUNE(bits_) false
#endif

namespace wsa {

constexpr int MAXC = 64;            // peak candidates per frame record (bands <= 128)
constexpr int AC_MAX = 320;         // worst case of the active-track table: tracks not yet 4 filing indices old (<= 5 x 63)
constexpr int PAIR_AC = 64;         // active-track table of one half-wave in the paired variant
constexpr int PAIR_GSZ = 4384;      // LDS bytes per half there: table (48 B per entry) + peak / pair scratch (40 B per peak) + the bin map
constexpr int QUAD_AC = 38;         // ... of one quarter-wave (16 lanes = a DPP row) in the variant that tracks four spans per wave
constexpr int QUAD_GSZ = 2496;      // 38 x 48 + 16 x 40 + 24, 16-byte aligned: four of them stay inside 8 LDS allocation units (10 240 B)
constexpr int AC_FAST = 140;        // what the default kernel variant holds in LDS (16 waves per CU); see the kernels at the end of this file

struct Ws {                          // per-wave work space carved out of global memory
    int32_t *tr_len, *tr_slot, *tr_rank;           // per track id: summary (written when the track leaves the active table) + finalize scratch (tr_slot: rank << 2 | slot of the
                                                   // generic finalize; tr_rank: unused since round 6, kept so that the span regions' layout — tracker_pool_bpf — stays what it was)
    double *tr_sumE, *tr_sumEbin;
    int4* pt;                                      // per point: {track id, bin | width << 8 | min(filing index, 0x7fff) << 17, band energy (f64 in .z/.w)}
    int4* ptx;                                     // level 3 only: {start bin, amplitude, filing index, end bin} of the point
    int32_t* pt_key;
    int32_t *d_p0, *d_p1, *d_gen;
    float *fr, *sm1;
    double *dB, *Aev;
    int32_t *q_idx, *sorted; double* q_mb;
};

__host__ __device__ inline size_t align16(size_t x) { return (x + 15) & ~(size_t)15; }

// lays the per-wave arrays out back to back (16-byte aligned); returns the pointers by value so
// that they live in registers, and the total size through *bytes
__host__ __device__ __forceinline__ Ws carve_ws(char* base, int T, int P, int F, int PX, size_t* bytes) {
    Ws w;
    size_t o = 0;
#define WSA_CARVE(field, type, count) do { w.field = reinterpret_cast<type*>(base + o); \
        o = align16(o + sizeof(type) * (size_t)(count)); } while (0)
    WSA_CARVE(tr_len, int32_t, T); WSA_CARVE(tr_slot, int32_t, T); WSA_CARVE(tr_rank, int32_t, T);
    WSA_CARVE(tr_sumE, double, T); WSA_CARVE(tr_sumEbin, double, T);
    WSA_CARVE(pt, int4, P); WSA_CARVE(ptx, int4, PX); WSA_CARVE(pt_key, int32_t, P);
    WSA_CARVE(d_p0, int32_t, F + 2); WSA_CARVE(d_p1, int32_t, F + 2); WSA_CARVE(d_gen, int32_t, F + 2);
    WSA_CARVE(fr, float, (size_t)(F + 2) * 9); WSA_CARVE(sm1, float, F + 2);
    WSA_CARVE(dB, double, (size_t)3 * (F + 2)); WSA_CARVE(Aev, double, (size_t)3 * (F + 2));
    WSA_CARVE(q_idx, int32_t, T); WSA_CARVE(sorted, int32_t, T); WSA_CARVE(q_mb, double, T);
#undef WSA_CARVE
    if (bytes) *bytes = o;
    return w;
}

// bytes per frame of the span regions of the split finalize (TrParams::pool): a span of F frames needs carve_ws(64 F, 64 F, F) <= F * carve_ws(64, 64, 1)
// (the SPLIT kernels write a span's tracks and points without capacity checks: a frame adds at most GW <= 32 of either, and the region holds MAXC per frame)
constexpr int GW_MAX = 32;          // lanes per span of the paired kernels (GW of tracker_group.hpp)
static_assert(GW_MAX <= MAXC, "a frame's new tracks / points (one per lane of its span's group) fit the MAXC per frame that tracker_pool_bpf gives a span region");
size_t tracker_pool_bpf() { size_t b = 0; (void)carve_ws(nullptr, MAXC, MAXC, 1, 0, &b); return align16(b) + 256; }
size_t tracker_ws_bytes(int tcap, int pcap, int fcap, bool raw_tracks) { size_t b = 0; (void)carve_ws(nullptr, tcap, pcap, fcap, raw_tracks ? pcap : 0, &b); return align16(b) + 256; }
// cycles per phase of a piece of code (tuning): lap(on, k) adds the cycles since the last start / lap to slot k.  `on` is a WSA_TUNE(...) test, so
// all of it compiles to nothing in a library built without TUNING=1
struct PhaseClock {
    unsigned long long cy[5] = {0, 0, 0, 0, 0}, t0 = 0;
    __device__ __forceinline__ void start(bool on) { if (on) t0 = __builtin_readcyclecounter(); }
    __device__ __forceinline__ void lap(bool on, int k) { if (on) { const unsigned long long now = __builtin_readcyclecounter(); cy[k] += now - t0; t0 = now; } }
};

// ---- what the pieces of the tracker (tracker_finalize.hpp, tracker_one.hpp, tracker_group.hpp) share about the span a wave works on: each takes it by
//      reference next to the kernel's parameters, its view of the LDS block and the lane; the kernels' bodies at the end of this file own it.
struct SpanState {
    uint32_t clip; int my_seg; int32_t* sg; uint32_t foff;                                    // the span: clip, segment, its words in p.seg_i, the clip's first frame
    int start, len, c_ci; uint32_t f_begin, f_end; double ctx_max, floor_;                    // the segment words gate.hip left (load_segment)
    int n_tr, n_pt, n_act, stale_d, stale_p1, gen;                                            // tracks, points, live tracks; the stale filing index and its points; d_gen mark
    // the two running sums of accumulate_fm (ref @B35952: `S += g; S -= E; C += E` per updated track): all terms are integers below
    // 2^40, so any order is exact — accG collects the g's (uniform), accL this lane's share of the E's, and the two totals are
    // formed where they are read (finalize, the trace, a stream's saved state) instead of by a wave reduction on every frame
    double accG, accL;
    bool overflow, act_overflow;                                                              // an arena overflowed; it was (only) the LDS active-track table
    Ws W; int aev_stride;                                                                     // the span's work space, stride of W.Aev
    unsigned long long ph[4]; PhaseClock acp;                                                 // tuning: finalize phase stamps (WSA_DBG bit 16), cycles per accumulate phase (bit 512)
    __device__ __forceinline__ void clear_tracks() { n_tr = n_pt = n_act = 0; stale_d = -1; stale_p1 = 0; accG = accL = 0; }
    // a new span: nothing tracked yet, segment words (and sg) not loaded
    __device__ __forceinline__ void begin(const TrParams& p, uint32_t clip_, int seg_) {
        clip = clip_; my_seg = seg_; foff = p.frame_off[clip];
        start = len = c_ci = 0; f_begin = f_end = 0; ctx_max = floor_ = 0;
        clear_tracks(); overflow = act_overflow = false;
        ph[0] = ph[1] = ph[2] = ph[3] = 0; acp = PhaseClock();
    }
    // the words of segment my_seg; frames = false (streams): f_begin / f_end stay what they are, the frames of the step
    __device__ __forceinline__ void load_segment(const TrParams& p, bool frames) {
        sg = p.seg_i + ((uint64_t)clip * p.seg_cap + my_seg) * 8;
        start = sg[SEG_START]; len = sg[SEG_LEN]; c_ci = sg[SEG_CCI];
        if (frames) { f_begin = (uint32_t)sg[SEG_FBEGIN]; f_end = (uint32_t)sg[SEG_FEND]; }
        ctx_max = p.seg_d[((uint64_t)clip * p.seg_cap + my_seg) * 2];
        floor_ = p.seg_d[((uint64_t)clip * p.seg_cap + my_seg) * 2 + 1];
    }
    __device__ __forceinline__ void totals(double& S, double& C) const { C = wave_sum_f64(accL); S = accG - C; }
};

// ---- One LDS block, carved by hand so that finalize can have ALL of it.  First part, two lives: while a span is tracked it holds the active tracks (ref `l`, the
//      live part, in track order: a_*); at finalize the tracks are dead and the same bytes hold the ranking scratch and the straightened formant frames (f_*), so
//      that finalize works out of LDS, not HBM.  Behind it the per-frame scratch of accumulate_fm (s_*; dead at finalize as well: finalize_lds runs over the whole
//      block).  The group kernels lay their own tables over the block (GroupLds, tracker_group.hpp); QUAD: four of them.
template <int AC, bool QUAD = false>
struct OneLds {
    static constexpr int SCRATCH = MAXC * (4 + 4 + 8 + 8) + 64 * 8 + MAXC * 8 + MAXC * 4;
    static constexpr int LDS_ONE = AC * 52 + SCRATCH;
    static constexpr int BYTES = (QUAD && 4 * QUAD_GSZ > LDS_ONE) ? 4 * QUAD_GSZ : LDS_ONE;
    static_assert((AC * 52) % 16 == 0, "the scratch arrays start 16-byte aligned");
    // finalize view: q_mb[AC] f64 | q_idx[AC] | sorted[AC] | fr[FRCAP][9] f32 | sm[FRCAP] f32
    static constexpr int FRCAP = (AC * 52 - AC * 16) / 40;
    static_assert(FRCAP <= FEAT_LDS_MAX, "finalize_generic hands formant_features_lds every span that fits the block");
    unsigned char* big;
    double *s_plo, *s_phi;                                       // accepted peaks of the current frame, compacted (lane o <-> peak o)
    unsigned long long* s_best; uint32_t *s_pk, *s_amp;         // per-peak arg-max scratch ...
    int32_t *s_pr_j, *s_pr_o, *s_asg;                            // ... and the (track, peak) pairs of one scoring pass
    double *a_vel, *a_sumE, *a_sumEbin;
    unsigned long long* a_mmask;                                 // peaks assigned to the track this frame
    int32_t *a_last_frame, *a_len, *a_gid;
    uint32_t *a_bins, *a_amp;                                    // a_bins: last bin | P[h-2] << 8 | P[h-3] << 16
    double* f_qmb; int32_t *f_qidx, *f_sorted; float *f_fr, *f_sm;
    __device__ __forceinline__ explicit OneLds(unsigned char* b) : big(b) {
        a_vel = reinterpret_cast<double*>(big); a_sumE = a_vel + AC; a_sumEbin = a_sumE + AC;
        a_mmask = reinterpret_cast<unsigned long long*>(a_sumEbin + AC);
        a_last_frame = reinterpret_cast<int32_t*>(a_mmask + AC); a_len = a_last_frame + AC; a_gid = a_len + AC;
        a_bins = reinterpret_cast<uint32_t*>(a_gid + AC); a_amp = a_bins + AC;
        f_qmb = reinterpret_cast<double*>(big); f_qidx = reinterpret_cast<int32_t*>(f_qmb + AC); f_sorted = f_qidx + AC;
        f_fr = reinterpret_cast<float*>(f_sorted + AC); f_sm = f_fr + FRCAP * 9;
        s_plo = reinterpret_cast<double*>(big + AC * 52); s_phi = s_plo + MAXC;
        s_best = reinterpret_cast<unsigned long long*>(s_phi + MAXC);
        s_pk = reinterpret_cast<uint32_t*>(s_best + MAXC); s_amp = s_pk + MAXC;
        s_pr_j = reinterpret_cast<int32_t*>(s_amp + MAXC); s_pr_o = s_pr_j + 64; s_asg = s_pr_o + 64;
    }
};
template <int AC, bool QUAD = false>
__device__ __forceinline__ OneLds<AC, QUAD> carve_lds() {
    __shared__ __attribute__((aligned(16))) unsigned char s_big[OneLds<AC, QUAD>::BYTES];
    return OneLds<AC, QUAD>(s_big);
}

// ---- next span.  Spans = (clip, segment) pairs, dealt out statically: item i -> clip i % n_clips, segment
//      i / n_clips, wave w takes items w, w + waves, ...  (A work queue costs a device-wide atomic per span on one
//      address, served at ~30 ns a piece on this chip: with all waves pulling together the last one got its first
//      span ~90 us into the kernel, and the queue line also slowed every other access to its memory channel.)
//      Four orders: DEAL_FINALIZE, DEAL_GROUPS and, for the one-span kernels (DEAL_SPANS), the sorted list or the enumeration (a stream's wave has its stream:
//      stream_body deals nothing).  Returns SPAN_DONE (no more), SPAN_SKIP (this turn is empty) or SPAN_TAKE.
struct SpanTurn { uint32_t item, clip = 0, seg = 0, total = 0; uint64_t group = 0; };      // group / total: DEAL_GROUPS — which NGR entries of the list, how many the list holds
enum { DEAL_SPANS, DEAL_GROUPS, DEAL_FINALIZE };  enum { SPAN_DONE, SPAN_SKIP, SPAN_TAKE };
template <int DEAL, int NGR = 1>
__device__ __forceinline__ int next_span(const TrParams& p, SpanTurn& t) {
    if (DEAL == DEAL_FINALIZE) {
        // finalize kernel: the spans in the tracker's order (longest first), wave w takes entries w, w + waves, ...
        const uint32_t total = p.counters[p.order_cnt];
        const uint64_t idx = (uint64_t)t.item * gridDim.x + blockIdx.x;
        if (idx >= total) return SPAN_DONE;
        t.item++;
        const uint2 e = p.order[idx];
        t.clip = e.x; t.seg = e.y;
    }
    else if (DEAL == DEAL_GROUPS) {
        // pairs of neighbours in the length-sorted list (entries 2 i and 2 i + 1: spans of nearly the same number of frames), dealt out in snake order
        t.total = p.counters[p.order_cnt];
        const uint32_t npairs = (t.total + (uint32_t)NGR - 1u) / (uint32_t)NGR, W_ = gridDim.x, r = t.item;
        if ((uint64_t)r * W_ >= npairs) return SPAN_DONE;
        t.item++;
        t.group = (uint64_t)r * W_ + ((r & 1u) ? W_ - 1u - blockIdx.x : blockIdx.x);
        if (t.group >= npairs) return SPAN_SKIP;
    }
    else if (p.order) {
        // spans sorted by their number of frames, longest first (span_order_kernel), dealt out in snake order — round r hands wave w entry r W + w (r even) or r W +
        // W-1-w (r odd) — so that every wave gets a long and a short one: with the
        // (clip, segment) enumeration the busiest wave of the 1024-clip batch worked 1.5x the mean.  (First span static, the rest
        // from an atomic queue — longest-processing-time-first proper — was slower: 0.62 vs 0.44 ms, profiles/r02_notes.md.)
        const uint32_t total = p.counters[p.order_cnt], W_ = gridDim.x, r = t.item;       // `item` counts the rounds here
        if ((uint64_t)r * W_ >= total) return SPAN_DONE;
        t.item++;
        const uint64_t idx = (uint64_t)r * W_ + ((r & 1u) ? W_ - 1u - blockIdx.x : blockIdx.x);
        if (idx >= total) return SPAN_SKIP;
        const uint2 e = p.order[idx];
        t.clip = e.x; t.seg = e.y;
    } else {
        t.seg = t.item / p.n_clips; t.clip = t.item - t.seg * p.n_clips;
        if (t.seg >= p.counters[0]) return SPAN_DONE;
        t.item += gridDim.x;
        if (t.seg >= p.seg_count[t.clip]) return SPAN_SKIP;
    }
    return SPAN_TAKE;
}

}  // namespace wsa
#include "tracker_finalize.hpp"
#include "tracker_one.hpp"
#include "tracker_group.hpp"
namespace wsa {

// ---- the kernels' bodies.  RAW = output_level 3: the points carry their extra words and the span ends in the raw-track export instead of a finalize
//      (its own instantiation: the usual kernels do not pay registers for it).  One span per wave and turn, tracked and finalized: tracker_kernel_fast / _full / _raw
template <int AC, bool RAW>
__device__ __forceinline__ void one_span_body(const TrParams& p) {
    const OneLds<AC> L = carve_lds<AC>();
    const int lane = threadIdx.x;
    SpanState sp;
    sp.W = carve_ws(p.ws + (uint64_t)blockIdx.x * p.ws_stride, p.tcap, p.pcap, p.fcap, RAW ? p.pcap : 0, nullptr);
    sp.gen = 0; sp.aev_stride = p.fcap + 2;
    for (int d = lane; d < p.fcap + 2; d += 64) sp.W.d_gen[d] = 0;
    wsync();
    SpanTurn t{p.order ? 0u : blockIdx.x};
    for (;;) {
        const int turn = next_span<DEAL_SPANS>(p, t);
        if (turn == SPAN_DONE) break;
        if (turn == SPAN_SKIP) continue;
        sp.begin(p, t.clip, (int)t.seg); sp.load_segment(p, true); sp.gen++;
        const unsigned long long tk0 = (WSA_TUNE(DBG_CYCLES)) ? __builtin_readcyclecounter() : 0ull;
        track_span<AC, RAW>(p, sp, L, lane);
        const unsigned long long tk1 = (WSA_TUNE(DBG_CYCLES)) ? __builtin_readcyclecounter() : 0ull;
        finish_span<AC, RAW, false>(p, sp, L, lane);
        trace_span_cycles(p, sp, lane, tk0, tk1);
        // bit0: an arena overflowed (results invalid); bit1: it was (only) the LDS active-track table of
        // the fast variant — the host then reruns the back end with the full-size variant
        if (sp.overflow && lane == 0) atomicOr(&p.shared[1], sp.act_overflow && AC < AC_MAX ? 2u : 1u);
        wsync();
    }
}
// incremental streaming, one wave per stream and step, tracker state carried in HBM between steps: tracker_kernel_stream / _stream_raw
template <int AC, bool RAW>
__device__ __forceinline__ void stream_body(const TrParams& p) {
    const OneLds<AC> L = carve_lds<AC>();
    const int lane = threadIdx.x;
    SpanState sp;
    sp.W = carve_ws(p.ws + (uint64_t)blockIdx.x * p.ws_stride, p.tcap, p.pcap, p.fcap, RAW ? p.pcap : 0, nullptr);
    sp.aev_stride = p.fcap + 2;
    wsync();
    sp.begin(p, blockIdx.x, 0);                                  // wave = stream, one pass
    const unsigned long long tk0 = (WSA_TUNE(DBG_CYCLES)) ? __builtin_readcyclecounter() : 0ull;
    track_stream<AC, RAW>(p, sp, L, lane);
    trace_span_cycles(p, sp, lane, tk0, tk0);
    if (sp.overflow && lane == 0) atomicOr(&p.shared[1], 1u);
    wsync();
}
// GW = 32: two spans per wave, one per half-wave, tracked in lock step; 16: four (the DPP rows; SPLIT = 1 only).  SPLIT = 0 (tracker_kernel_pair):
// finalize follows, wave-wide per span; SPLIT = 1 (tracker_kernel_pair_acc / _quad_acc): accumulate only — tracks and points go to the span's region
// of p.pool, a header per span is left in p.span_hdr
template <int AC, int GW, int SPLIT>
__device__ __forceinline__ void group_body(const TrParams& p) {
    const OneLds<AC, GW == 16> L = carve_lds<AC, GW == 16>();
    const int lane = threadIdx.x;
    SpanState sp;
    sp.gen = 0; sp.aev_stride = p.fcap + 2;
    if (!SPLIT) for (int h = 0; h < 2; h++) {
        const Ws Wh = carve_ws(p.ws + ((uint64_t)blockIdx.x * 2 + h) * p.ws_stride, p.tcap, p.pcap, p.fcap, 0, nullptr);
        for (int d = lane; d < p.fcap + 2; d += 64) Wh.d_gen[d] = 0;
    }
    wsync();
    SpanTurn t{p.order ? 0u : blockIdx.x};
    for (;;) {
        const int turn = next_span<DEAL_GROUPS, 64 / GW>(p, t);
        if (turn == SPAN_DONE) break;
        if (turn == SPAN_SKIP) continue;
        sp.gen++;                                                // marks this turn's entries of the halves' d_* tables (unsplit pair)
        track_group<AC, GW, SPLIT>(p, sp, L, lane, t);
    }
}
// finalize only, one span per wave and turn, out of the regions and headers the SPLIT = 1 kernels left: tracker_kernel_finalize
template <int AC>
__device__ __forceinline__ void finalize_body(const TrParams& p) {
    const OneLds<AC> L = carve_lds<AC>();
    const int lane = threadIdx.x;
    SpanState sp;
    wsync();
    SpanTurn t{p.order ? 0u : blockIdx.x};
    for (;;) {
        if (next_span<DEAL_FINALIZE>(p, t) == SPAN_DONE) break;
        sp.begin(p, t.clip, (int)t.seg); sp.load_segment(p, true);
        finalize_from_header<AC>(p, sp, L, lane);
    }
}

// The fast variant is held to 128 VGPRs (4 waves per SIMD; ~80 registers spill to scratch) and its active-track table to
// AC_FAST = 140 entries (10 096 B of LDS: 8 of the CU's 1 280-byte allocation units, 16 waves per CU).  The kernel is bound by
// instruction issue with most lanes idle, so waves in flight beat spill traffic: 3 per SIMD (168 VGPRs, 192 entries) 0.409 ms,
// 4 per SIMD 0.381 ms, 5 per SIMD (96 VGPRs, 100 entries, 241 spills) 0.643 ms on the 1024-clip batch (profiles/r02_notes.md).
// Mind the allocation unit: 16 bytes of LDS more than 12 800 cost the 3-per-SIMD variant a twelfth wave per CU and 50 % of its speed.
// The full-table variant is LDS-limited to 8 waves per CU and keeps its registers.
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(4, 4))) void tracker_kernel_fast(TrParams p) { one_span_body<AC_FAST, false>(p); }
// two spans per wave (half-waves in lock step): 3 waves per SIMD (168 VGPRs) are all the pairs of a 1024-clip batch need
// (held to 128 registers / 4 waves it spills 78 of them: 1.02 -> 1.12 ms per batch alone, 0.73 -> 0.75 ms pipelined)
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(3, 4))) void tracker_kernel_pair(TrParams p) {
    __builtin_amdgcn_s_setprio(3);      // the dependent chains of this kernel go first, the front end of the next batch fills what they leave (0.686 -> 0.680 ms per pipelined step)
    group_body<AC_FAST, 32, 0>(p);
}
// split finalize: the paired accumulate on its own (its waves end with the tracking: fewer registers, shorter lives) and the finalize of every span, one span per
// wave and turn, out of the span regions (TrParams::pool); rows bit for bit those of the kernel above (tests/test_gpu_parity.py)
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(4, 4))) void tracker_kernel_pair_acc(TrParams p) {
    __builtin_amdgcn_s_setprio(3);
    group_body<AC_FAST, 32, 1>(p);
}
// four spans per wave: the quarters of a wave (its four DPP rows) track four neighbours of the length-sorted span list in lock step; a frame brings a
// span at most 16 accepted peaks here and its table holds 38 live tracks (4 % of the spans need more: redo list).  Every instruction serves four frames
// instead of two; the loops over the tracks take two chunks of 16 where the halves took one of 32
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(4, 4))) void tracker_kernel_quad_acc(TrParams p) {
    __builtin_amdgcn_s_setprio(3);
    group_body<AC_FAST, 16, 1>(p);
}
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(4, 4))) void tracker_kernel_finalize(TrParams p) {
    __builtin_amdgcn_s_setprio(3);
    finalize_body<AC_FAST>(p);
}
__global__ __launch_bounds__(64) void tracker_kernel_full(TrParams p) { one_span_body<AC_MAX, false>(p); }
__global__ __launch_bounds__(64) void tracker_kernel_raw(TrParams p) { one_span_body<AC_MAX, true>(p); }
__global__ __launch_bounds__(64) void tracker_kernel_stream(TrParams p) { stream_body<AC_MAX, false>(p); }
__global__ __launch_bounds__(64) void tracker_kernel_stream_raw(TrParams p) { stream_body<AC_MAX, true>(p); }      // level 3 for streams

// ---- span order: all (clip, segment) pairs the gate kernel produced, sorted by span length (frames between the resets that
// bound the span: what the tracker's time goes with), longest first — a counting sort whose counting the gate kernel has done already
// (GateParams::span_hist / span_key: every finalized segment took a rank inside its length bucket).  Here: an exclusive scan over the
// buckets (one workgroup) and the scatter (one thread per clip).  The order inside a bucket is whatever the atomics made it — the
// tracker's results do not depend on the order the spans are processed in, rows are put back in callback order by K3.
// counters[1] = number of spans.
// One kernel: every workgroup forms the exclusive scan of the histogram itself (2 048 counts: 8 KB out of L2, a few microseconds) and keeps the
// offsets in LDS, then scatters the spans of its clips — a scan kernel in front was one more dependent launch on the run's chain (~15 us of
// kernel + the launch gap, for a 1024-clip batch) to save each of a handful of workgroups that scan.  The histogram itself stays as counted.
constexpr int ORDER_T = 256;
__global__ __launch_bounds__(ORDER_T) void span_order_kernel(const uint32_t* hist, const uint2* key, const uint32_t* seg_count, uint32_t n_clips, int seg_cap, uint2* order, uint32_t* counters) {
    __shared__ uint32_t offs[SPAN_BUCKETS], part[ORDER_T];
    const int tid = threadIdx.x;
    constexpr int PER = SPAN_BUCKETS / ORDER_T;
    uint32_t mine[PER], sum = 0;
#pragma unroll
    for (int q = 0; q < PER; q++) { mine[q] = hist[tid * PER + q]; sum += mine[q]; }
    part[tid] = sum;
    __syncthreads();
    for (int d = 1; d < ORDER_T; d <<= 1) {
        const uint32_t add = tid >= d ? part[tid - d] : 0u;
        __syncthreads();
        part[tid] += add;
        __syncthreads();
    }
    uint32_t run = part[tid] - sum;
#pragma unroll
    for (int q = 0; q < PER; q++) { offs[tid * PER + q] = run; run += mine[q]; }
    if (blockIdx.x == 0 && tid == ORDER_T - 1) counters[1] = part[tid];
    __syncthreads();
    const uint32_t clip = blockIdx.x * ORDER_T + tid;
    if (clip >= n_clips) return;
    const uint32_t ns = seg_count[clip];
    for (uint32_t k = 0; k < ns; k++) {
        const uint2 e = key[(uint64_t)clip * seg_cap + k];
        order[offs[e.x] + e.y] = make_uint2(clip, k);
    }
}

void launch_span_order(const TrParams& p, uint32_t* span_hist, const uint2* span_key, uint2* order, uint32_t* counters, hipStream_t s) {
    if (p.n_clips == 0) return;
    hipLaunchKernelGGL(span_order_kernel, dim3((p.n_clips + ORDER_T - 1) / ORDER_T), dim3(ORDER_T), 0, s, span_hist, span_key, p.seg_count, p.n_clips, p.seg_cap, order, counters);
}

void launch_tracker_stream(const TrParams& p, uint32_t n_streams, hipStream_t s) {
    if (n_streams == 0) return;
    static_assert(AC_MAX == TR_ACT_MAX, "the streams' saved active table is sized for the full variant");
    if (p.level == 3) hipLaunchKernelGGL(tracker_kernel_stream_raw, dim3(n_streams), dim3(64), 0, s, p);
    else hipLaunchKernelGGL(tracker_kernel_stream, dim3(n_streams), dim3(64), 0, s, p);
}

void launch_tracker(const TrParams& p, int n_waves, bool full_table, bool pair, hipStream_t s) {
    if (n_waves <= 0) return;
    if (p.level == 3) hipLaunchKernelGGL(tracker_kernel_raw, dim3(n_waves), dim3(64), 0, s, p);
    else if (full_table) hipLaunchKernelGGL(tracker_kernel_full, dim3(n_waves), dim3(64), 0, s, p);
    else if (pair && p.order && p.redo && (!p.trace || (p.dbg & DBG_CYCLES))) {
        // two spans per wave; what the paired variant declines goes through the one-span kernel right behind it (usually nothing: its waves find an empty list)
        if (p.pool && p.span_hdr) {
            if (p.quad) hipLaunchKernelGGL(tracker_kernel_quad_acc, dim3(p.quad_waves > 0 ? p.quad_waves : n_waves), dim3(64), 0, s, p);
            else hipLaunchKernelGGL(tracker_kernel_pair_acc, dim3(n_waves), dim3(64), 0, s, p);
            hipLaunchKernelGGL(tracker_kernel_finalize, dim3(p.fin_waves > 0 ? p.fin_waves : 2 * n_waves), dim3(64), 0, s, p);
        }
        else hipLaunchKernelGGL(tracker_kernel_pair, dim3(n_waves), dim3(64), 0, s, p);
        TrParams r = p; r.order = p.redo; r.order_cnt = 2; r.pool = nullptr; r.span_hdr = nullptr;
        // (its waves find an empty list almost always — the paired kernel declines 1 span in 10^4, the quad kernel 1 in 10^2 — and every wave costs its set-up)
        const int redo_waves = p.quad ? 1024 : 128;
        hipLaunchKernelGGL(tracker_kernel_fast, dim3(n_waves < redo_waves ? n_waves : redo_waves), dim3(64), 0, s, r);
    }
    else hipLaunchKernelGGL(tracker_kernel_fast, dim3(n_waves), dim3(64), 0, s, p);
}

// ---- K3 compaction: segment table + row pool -> dense tables in (clip, si, syllable) order, the order
// in which the reference's dispatcher P() (ref @B28869) would have invoked the callback.
// per-clip row counts (a thread per clip walks its segment table: chains of dependent loads, so as many clips at once as the chip takes),
// then one workgroup turns the per-clip row / segment counts into offsets
__global__ void compact_count_kernel(CompactParams p) {
    const uint32_t c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= p.n_clips) return;
    const uint32_t ns = p.seg_count[c];
    const int32_t* sg = p.seg_i + (uint64_t)c * p.seg_cap * 8;
    uint32_t r = 0;
    for (uint32_t k = 0; k < ns; k++) if (sg[8 * k + SEG_FLAG] >= 0) r += (uint32_t)sg[8 * k + SEG_NROWS];
    p.clip_row_off[c] = r;                // count for now; compact_scan_kernel turns it into an offset
}
constexpr int CSCAN_T = 1024;
template <bool COUNT>          // COUNT: small launches (streams, up to two clips per thread) count their rows here and save a kernel
__global__ __launch_bounds__(CSCAN_T) void compact_scan_kernel(CompactParams p) {
    // single block: exclusive scan of the per-clip row / segment counts (a thread owns a run of consecutive clips)
    __shared__ uint32_t s_rows[CSCAN_T], s_segs[CSCAN_T];
    const int tid = threadIdx.x;
    const uint32_t per = (p.n_clips + CSCAN_T - 1) / CSCAN_T;
    const uint32_t c0 = min(p.n_clips, tid * per), c1 = min(p.n_clips, c0 + per);
    uint32_t rs = 0, ss = 0;
    for (uint32_t c = c0; c < c1; c++) {
        if (COUNT) {
            const uint32_t ns = p.seg_count[c];
            const int32_t* sg = p.seg_i + (uint64_t)c * p.seg_cap * 8;
            uint32_t r = 0;
            for (uint32_t k = 0; k < ns; k++) if (sg[8 * k + SEG_FLAG] >= 0) r += (uint32_t)sg[8 * k + SEG_NROWS];
            p.clip_row_off[c] = r;
        }
        ss += p.seg_count[c]; rs += p.clip_row_off[c];
    }
    s_rows[tid] = rs; s_segs[tid] = ss;
    __syncthreads();
    for (int d = 1; d < CSCAN_T; d <<= 1) {          // inclusive scan of both columns
        const uint32_t ar_ = tid >= d ? s_rows[tid - d] : 0u, as_ = tid >= d ? s_segs[tid - d] : 0u;
        __syncthreads();
        s_rows[tid] += ar_; s_segs[tid] += as_;
        __syncthreads();
    }
    if (tid == CSCAN_T - 1) {
        p.totals[0] = s_rows[tid]; p.totals[1] = s_segs[tid];
        p.clip_row_off[p.n_clips] = s_rows[tid]; p.clip_seg_off[p.n_clips] = s_segs[tid];
    }
    uint32_t ar = s_rows[tid] - rs, as = s_segs[tid] - ss;
    for (uint32_t c = c0; c < c1; c++) {
        const uint32_t r = p.clip_row_off[c];
        p.clip_row_off[c] = ar; p.clip_seg_off[c] = as; as += p.seg_count[c]; ar += r;
    }
}

// FUSED (batches of up to a few thousand clips): no scan kernel in front — the wave of clip c sums the row / segment counts of the clips before it
// itself (the per-clip row count is the clip's row counter, which the tracker bumped once per result), writes its two offsets, and the wave of
// clip 0 also forms the totals and hands the run's result counters to the host (p.host: mapped pinned words).  Three dependent launches less at
// the end of every run: with several batches in flight a stream's run is as long as the chain of its kernels, and these three were ~90 us of it
// in which the stream kept next to nothing of the GPU busy.
template <bool FUSED>
__global__ __launch_bounds__(64) void compact_gather_kernel(CompactParams p) {
    const uint32_t clip = blockIdx.x;
    const int lane = threadIdx.x;
    const uint32_t nseg = p.seg_count[clip];
    if (FUSED) {
        uint32_t rs = 0, ss = 0;
        for (uint32_t i = lane; i < clip; i += 64) { rs += p.clip_rows[i]; ss += p.seg_count[i]; }
        rs = wave_sum_u32(rs); ss = wave_sum_u32(ss);
        if (lane == 0) { p.clip_row_off[clip] = rs; p.clip_seg_off[clip] = ss; }
        if (clip == 0) {
            uint32_t rt = 0, st = 0;
            for (uint32_t i = lane; i < p.n_clips; i += 64) { rt += p.clip_rows[i]; st += p.seg_count[i]; }
            rt = wave_sum_u32(rt); st = wave_sum_u32(st);
            if (lane == 0) {
                p.totals[0] = rt; p.totals[1] = st; p.clip_row_off[p.n_clips] = rt; p.clip_seg_off[p.n_clips] = st;
                if (p.host) { p.host[0] = rt; p.host[1] = st; p.host[2] = p.flags[0]; p.host[3] = p.totals[3]; __threadfence_system(); }
            }
            if (p.clr_counters) {
                // every kernel that looks at the run's counters, totals or span histogram is through (stream order; the other waves of this one read none
                // of them): cleared here, the next run of the batch needs no clear kernel in front — one dependent launch less on its chain
                wsync();
                if (lane < 16) p.clr_counters[lane] = 0u;
                if (lane < 4) p.totals[lane] = 0u;
                if (p.clr_hist) for (int b = lane; b < SPAN_BUCKETS; b += 64) p.clr_hist[b] = 0u;
            }
        }
        wsync();
    }
    const uint32_t so = p.clip_seg_off[clip];
    const int32_t* sg = p.seg_i + (uint64_t)clip * p.seg_cap * 8;
    for (uint32_t i = lane; i < nseg; i += 64) {
        int32_t* o = p.seg_out + (uint64_t)(so + i) * 4;
        o[0] = (int32_t)clip; o[1] = sg[8 * i + SEG_START]; o[2] = sg[8 * i + SEG_LEN]; o[3] = sg[8 * i + SEG_FLAG];
    }
    // results in segment order; si = index among the segments that produced a result entry
    uint32_t ro = p.clip_row_off[clip];
    int si = 0;
    // streaming: segments / results of earlier steps (the table holds this step's segments only)
    int32_t* cy = p.carry ? p.carry + (uint64_t)clip * CARRY_WORDS : nullptr;
    const int seg_before = cy ? cy[0] : 0, res_before = cy ? cy[1] : 0;
    bool lost = false;
    for (uint32_t k = 0; k < nseg; k++) {
        const int flag = sg[8 * k + SEG_FLAG];
        if (flag < 0) continue;                       // straighten threw: segments_ci entry without a result
        const int nr = sg[8 * k + SEG_NROWS];
        const uint32_t r0 = (uint32_t)sg[8 * k + SEG_ROW0];
        // the dispatcher indexes segments_ci with the RESULT index (ref @B29138 / @B29622): after a
        // dropped segment the timestamps come from the wrong entry — reproduced, not repaired
        const int gsi = res_before + si;              // result index since the launch
        int32_t ts, tl;
        if (gsi >= seg_before) { ts = sg[8 * (gsi - seg_before) + SEG_START]; tl = sg[8 * (gsi - seg_before) + SEG_LEN]; }
        else {                                        // an entry of an earlier step
            if (seg_before - gsi > CARRY_HIST) lost = true;
            ts = cy[2 + 2 * (gsi % CARRY_HIST)]; tl = cy[3 + 2 * (gsi % CARRY_HIST)];
        }
        for (int i = lane; i < nr; i += 64) {
            const int32_t* m = p.row_meta_in + (uint64_t)(r0 + i) * 8;
            int32_t* o = p.row_meta_out + (uint64_t)(ro + i) * 8;
            o[0] = m[0]; o[1] = gsi; o[4] = seg_before + m[4]; o[5] = m[5]; o[6] = m[6]; o[7] = m[7];
            if (p.level == 10 || p.level == 13) { o[2] = ts + m[2]; o[3] = m[3]; }     // syllable row (ref @B31114)
            else { o[2] = ts; o[3] = tl; }                                            // segment row (ref @B31504)
        }
        for (int i = lane; i < nr * WSA_NFEAT; i += 64) p.row_feat_out[(uint64_t)ro * WSA_NFEAT + i] = p.row_feat_in[(uint64_t)r0 * WSA_NFEAT + i];
        ro += (uint32_t)nr;
        si++;
    }
    if (cy) {
        wsync();
        if (lane == 0) {
            for (uint32_t k = 0; k < nseg; k++) {
                const int g = seg_before + (int)k;
                cy[2 + 2 * (g % CARRY_HIST)] = sg[8 * k + SEG_START]; cy[3 + 2 * (g % CARRY_HIST)] = sg[8 * k + SEG_LEN];
            }
            cy[0] = seg_before + (int)nseg; cy[1] = res_before + si;
            if (lost) atomicOr(&p.totals[2], 1u);
        }
    }
}

// which of its three forms launch_compact runs (the one place that decides; the tests assert it at every clip count they sit on)
int compact_path(const CompactParams& p) {
    if (p.n_clips == 0) return COMPACT_NOTHING;
    if (p.fused && !p.carry && p.clip_rows && p.n_clips <= 4096) return COMPACT_FUSED;
    return p.n_clips <= 2 * CSCAN_T ? COMPACT_SCAN : COMPACT_COUNT_SCAN;
}
void launch_compact(const CompactParams& p, hipStream_t s) {
    const int path = compact_path(p);
    if (path == COMPACT_NOTHING) return;
    if (path == COMPACT_FUSED) { hipLaunchKernelGGL(compact_gather_kernel<true>, dim3(p.n_clips), dim3(64), 0, s, p); return; }
    if (path == COMPACT_SCAN) hipLaunchKernelGGL(compact_scan_kernel<true>, dim3(1), dim3(CSCAN_T), 0, s, p);
    else {
        hipLaunchKernelGGL(compact_count_kernel, dim3((p.n_clips + 255) / 256), dim3(256), 0, s, p);
        hipLaunchKernelGGL(compact_scan_kernel<false>, dim3(1), dim3(CSCAN_T), 0, s, p);
    }
    hipLaunchKernelGGL(compact_gather_kernel<false>, dim3(p.n_clips), dim3(64), 0, s, p);
}
bool compact_is_fused(const CompactParams& p) { return compact_path(p) == COMPACT_FUSED; }

}  // namespace wsa
