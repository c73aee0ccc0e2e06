// stream_api.hip — the wsa_stream_* part of include/wsa.h: n_streams concurrent launches that advance
// in lock step, one hipGraph launch per step.
//
// Stands in for the reference's online path (ref dist/main.js:2): worklet process() -> port message ->
// spectrum_push (@B8752, @B30392) once per frame with module-level state, callbacks as segments close
// (@B28869), StopAudioNodes -> segment_truncate (@B5699, @B30757).  The kernels are the batch ones:
//   front end   frontend.hip on the step's samples (n_frames = frames of this step per stream)
//   peaks       peaks.hip, records written into per-stream rings (slot = absolute frame & (ring - 1))
//   gate        gate.hip gate_kernel_t<true>: state in HBM between steps, segments of this step only
//   tracker     tracker.hip over the spans that closed in this step (ring-indexed frames)
//   compaction  tracker.hip, callback index / segments_ci history carried in HBM
// A span (frames between two segmenter resets) stays in its stream's ring until it closes, so results
// are those of one clip holding the whole signal; tests/test_gpu_stream.py checks exactly that.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include "host_plan.hpp"
#include "pcm_formats.hpp"

using namespace wsa;
using wsa_api::fail;

struct wsa_stream {
    wsa_ctx* ctx = nullptr;
    uint32_t n = 0, F = 0, ring = 0;
    std::vector<uint32_t> seen_cuts;        // stream_cuts as of the previous collect (WSA_FLAG_STREAM_CUT)
    double fs = 0;
    DevArena mem;                           // device and pinned memory (host_plan.hpp); collect's staging buffers grow on demand and are their own allocations
    FeDev fe;                               // front-end plan and its device tables
    Derived D;                              // what the configuration decides for the back end
    BackEnd be;                             // back-end buffers and capacities; frames live in per-stream rings
    Tuning tune;                            // test switches, read from the environment when the stream set is planned
    uint32_t hist = 0, q = 1, step_samples = 0, stage_stride = 0;     // hist = (q - 1) * hop samples of history, q = ceil(win / hop)
    float *d_stage = nullptr, *d_pcm_in = nullptr;
    uint32_t *d_ctl = nullptr;              // [3][n]: n_frames, pcm_off, ctl bits
    uint32_t *d_frame_off = nullptr, *d_ring_off = nullptr, *d_spec = nullptr;
    TrackGather trk; std::vector<uint64_t> x_trk_off; std::vector<int32_t> x_trk_pts, x_trk_rank, x_trk_seg;      // level 3: the raw-track pools are per stream a ring of ring x 64 entries
    uint32_t* d_utt_state = nullptr;        // level 11: per-stream histogram state
    std::vector<int32_t> x_utt_meta; std::vector<double> x_utt_feat;
    std::vector<float> x_formants; std::vector<uint32_t> x_formant_off;      // levels 4 / 10: the straightened frames of the last step's rows, gathered at collect
    char* d_collect = nullptr; size_t collect_cap = 0;                        // collect's staging (levels 4 / 10): the step's pieces out of the rings, gathered by one kernel, fetched by one copy
    double* d_state = nullptr;              // the gate's state of every stream between steps
    int32_t *d_tr_state = nullptr, *d_fr_span = nullptr; char* d_tr_act = nullptr;      // incremental tracker: state of every stream between steps
    int32_t* d_carry = nullptr;
    // pinned host side
    uint32_t* h_ctl = nullptr;              // [3][n]
    float* h_pcm = nullptr;                 // [n][step_samples]
    float* h_pcm_dev = nullptr;             // the same buffers as the device sees them
    uint32_t *h_ctl_dev = nullptr, *h_totals_dev = nullptr; int32_t *h_meta_dev = nullptr, *h_seg_dev = nullptr; double* h_feat_dev = nullptr;
    uint32_t* h_totals = nullptr;           // rows, segs, lost, flags, then per stream the spans cut at the ring's capacity
    hipStream_t last_stream = nullptr;      // where the previous step was enqueued
    int32_t *h_meta = nullptr, *h_seg = nullptr;
    double* h_feat = nullptr;
    uint32_t d2h_rows = 0, d2h_segs = 0, rows_cap = 0, segs_cap = 0;
    std::vector<int32_t> x_meta, x_seg; std::vector<double> x_feat;      // overflow of the fixed D2H window
    std::vector<uint32_t> warm;             // frames still to skip after START (windows reaching before time zero)
    uint64_t steps = 0;
    bool graph_on = false, stepped = false;
    hipGraphExec_t gexec = nullptr;
    hipStream_t own = nullptr; hipEvent_t ev_in = nullptr;   // the legacy NULL stream cannot be captured: steps given stream 0 run on `own`
    const float* g_pcm = nullptr; uint64_t g_stride = 0; hipStream_t g_stream = nullptr; bool g_host = false;
    wsa_scls* scls = nullptr;               // the attached classifier's tables and carried fold (wsa_stream_set_model), or NULL
    wsa_sens* sens = nullptr;               // ... or the attached ensemble's (wsa_stream_set_ensemble); never both
    wsa_sknn* sknn = nullptr;               // the attached KNN store's tables, scratch and carried fold (wsa_stream_set_knn), beside either
    wsa_sreg* sreg = nullptr;               // the attached regression group's tables and carried sums (wsa_stream_set_regress), beside all of them
    uint32_t in_stride = 0, ctl_words = 3;  // floats per stream in the input buffers (a plain set: step_samples), control words per stream
    // a mixed set (wsa_stream_create_mixed): F above is the step's internal frame CAPACITY (resample_step_frames_bound), F_user the caller's frames_per_step
    bool mixed = false;
    uint32_t F_user = 0, out_cap = 0, conv_stride = 0, xcap = 0;
    std::vector<double> fs_in, ratio;
    std::vector<uint32_t> in_cap, last_nfr, last_out;      // per stream: samples one step accepts, frames / outputs of its last active step
    std::vector<uint64_t> cN, cY, cK, cS;                  // per stream since START: inputs received, outputs handed on, frames analysed, active steps
    float *d_conv = nullptr, *d_hist = nullptr, *d_rs_tables = nullptr; RsClass* d_rs_cls = nullptr; uint32_t* d_rs_class = nullptr;
    // packed input (spec PK-1, wsa_stream_set_input_format): own allocations, replaced whenever the format is set
    int32_t fmt = WSA_PCM_F32, g_fmt = WSA_PCM_F32;
    std::vector<uint32_t> chan;             // channels per stream (empty: mono)
    uint8_t *h_pk = nullptr, *h_pk_dev = nullptr;      // [n][pk_stride] bytes, mapped pinned
    uint32_t pk_stride = 0, max_ch = 1;
    uint32_t* d_chan = nullptr;
    // spec PK-3 (wsa_stream_set_input_channels): stream i takes channel sel[i] (or the mix) of the packed row of stream src[i]; d_sel = [sel | src]
    bool chsel = false;
    uint32_t* d_sel = nullptr;
};

namespace wsa {
// history shuffle for overlapping windows: stage[s] = [last `hist` samples of the previous stage | new samples]
__global__ __launch_bounds__(256) void stream_stage_kernel(float* stage, uint32_t stage_stride, const float* pcm, uint64_t pcm_stride,
                                                           const uint32_t* ctl_bits, uint32_t hist, uint32_t step_samples) {
    extern __shared__ float s_hist[];
    const uint32_t s = blockIdx.x;
    if (!(ctl_bits[s] & 4u)) return;                       // bit 2 of the device control word: stream active in this step
    float* st = stage + (uint64_t)s * stage_stride;
    for (uint32_t i = threadIdx.x; i < hist; i += 256) s_hist[i] = st[step_samples + i];
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < hist; i += 256) st[i] = s_hist[i];
    const float* src = pcm + (uint64_t)s * pcm_stride;
    for (uint32_t i = threadIdx.x; i < step_samples; i += 256) st[hist + i] = src[i];
}
// host -> device through the mapped pinned buffer (a kernel node: H2D memcpy nodes of more than a few KB from
// pinned memory faulted inside captured graphs on ROCm 7.2 / gfx950, the same copy outside a graph was fine)
__global__ __launch_bounds__(256) void stream_pull_kernel(float* dst, const float* __restrict__ src, size_t n) {
    const size_t i = ((size_t)blockIdx.x * 256 + threadIdx.x) * 4;
    if (i + 3 < n) *reinterpret_cast<float4*>(dst + i) = *reinterpret_cast<const float4*>(src + i);
    else for (size_t k = i; k < n; k++) dst[k] = src[k];
}
// packed host or device input -> floats in d_pcm_in (spec PK-1), a kernel node like the float pull.  One block row per stream; a lane takes
// whole 16-byte chunks of the stream's row (8 i16 samples or 16 G.711 codes), decodes channel 0's samples in registers and stores floats.
// Rows of streams that are not active in the step are skipped, and so is everything behind the step's count of a stream.
// ctl: the device control words the step's prologue has just written (word w of stream s at ctl[w * n + s]); count_word = 0: every
// active stream carries fixed_count samples (a plain set), else the word that holds the stream's count (RS_CTL_NIN of a mixed set).
// The caller guarantees count * channels * sample size <= src_stride, src and src_stride multiples of 16, count <= dst_stride.
template <int FORMAT>
__global__ __launch_bounds__(128) void stream_pull_packed_kernel(float* __restrict__ dst, uint32_t dst_stride, const uint8_t* __restrict__ src, uint64_t src_stride,
                                                                 const uint32_t* __restrict__ chan, const uint32_t* __restrict__ ctl, uint32_t n,
                                                                 uint32_t count_word, uint32_t fixed_count) {
    constexpr uint32_t E = FORMAT == WSA_PCM_I16 ? 8u : 16u;      // samples in a 16-byte chunk
    constexpr uint32_t PER = E / 4u;                               // samples per 32-bit word
    constexpr uint32_t BITS = 32u / PER, MASK = BITS == 16u ? 0xFFFFu : 0xFFu;
    const uint32_t s = blockIdx.x;
    if (!(ctl[RS_CTL_BITS * n + s] & 4u)) return;
    const uint32_t cnt = count_word ? ctl[count_word * n + s] : fixed_count;
    if (cnt == 0) return;
    const uint32_t ch = chan[s];
    const uint4* row = reinterpret_cast<const uint4*>(src + (uint64_t)s * src_stride);
    float* out = dst + (uint64_t)s * dst_stride;
    const uint32_t n_el = (cnt - 1u) * ch + 1u;                   // elements of the row up to channel 0 of the last frame (cnt <= 2^24, ch <= 64)
    const uint32_t n_chunks = (n_el + E - 1u) / E;
    const bool vec = (dst_stride & 3u) == 0;                       // rows of d_pcm_in start on 16 bytes
    for (uint32_t c = blockIdx.y * 128u + threadIdx.x; c < n_chunks; c += gridDim.y * 128u) {
        const uint32_t e0 = c * E;
        if (ch == 1u) {
            const uint4 v = row[c];
            const uint32_t w[4] = {v.x, v.y, v.z, v.w};
            float f[E];
#pragma unroll
            for (uint32_t k = 0; k < E; k++) f[k] = pcm_decode_one<FORMAT>((w[k / PER] >> (BITS * (k % PER))) & MASK);
            if (vec && e0 + E <= cnt) {
#pragma unroll
                for (uint32_t k = 0; k < E; k += 4) *reinterpret_cast<float4*>(out + e0 + k) = make_float4(f[k], f[k + 1], f[k + 2], f[k + 3]);
            } else {
#pragma unroll
                for (uint32_t k = 0; k < E; k++) if (e0 + k < cnt) out[e0 + k] = f[k];
            }
        } else {
            uint32_t j = (e0 + ch - 1u) / ch;                      // first frame whose channel 0 lies in this chunk or behind it
            uint32_t next = j * ch - e0;
            if (next >= E || j >= cnt) continue;                   // no sample of channel 0 in this chunk: not loaded
            const uint4 v = row[c];
            const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
            for (uint32_t k = 0; k < E; k++)
                if (k == next && j < cnt) { out[j] = pcm_decode_one<FORMAT>((w[k / PER] >> (BITS * (k % PER))) & MASK); j++; next += ch; }
        }
    }
}
// spec PK-3 for streams: stream s takes channel sel[s], or the mix, of the packed row of stream srcs[s] — one sample per lane from the sample's own
// bytes (a step's few hundred samples per stream; the source's row is read once per stream that takes from it).  Counts and control words are the
// stream's own; the caller guarantees that the source's row holds the stream's count of frames.
template <int FORMAT>
__global__ __launch_bounds__(128) void stream_pull_channels_kernel(float* __restrict__ dst, uint32_t dst_stride, const uint8_t* __restrict__ src, uint64_t src_stride,
                                                                   const uint32_t* __restrict__ chan, const uint32_t* __restrict__ sel, const uint32_t* __restrict__ srcs,
                                                                   const uint32_t* __restrict__ ctl, uint32_t n, uint32_t count_word, uint32_t fixed_count) {
    constexpr uint32_t SB = FORMAT == WSA_PCM_I16 ? 2u : 1u;
    const uint32_t s = blockIdx.x;
    if (!(ctl[RS_CTL_BITS * n + s] & 4u)) return;
    const uint32_t cnt = count_word ? ctl[count_word * n + s] : fixed_count;
    const uint32_t ch = chan[s], pick = sel[s];
    const uint8_t* row = src + (uint64_t)srcs[s] * src_stride;
    float* out = dst + (uint64_t)s * dst_stride;
    for (uint32_t j = blockIdx.y * 128u + threadIdx.x; j < cnt; j += gridDim.y * 128u) {
        const uint8_t* fr = row + (uint64_t)j * ch * SB;
        out[j] = pick == WSA_CHANNEL_MIX ? pcm_mix_frame(ch, [&](uint32_t c) { return pcm_decode_bytes(FORMAT, fr + c * SB); }) : pcm_decode_bytes(FORMAT, fr + pick * SB);
    }
}
// step prologue: control words host -> device (mapped pinned memory), counters cleared
// (level 3: the per (stream, k of this step) table of the segments' track pools starts every step empty, so that an entry the step did not write reads as
//  "no tracks", not as a previous step's pool offsets — cleared HERE, by a kernel: a memset node inside the captured step did not replay reliably on this ROCm)
__global__ __launch_bounds__(256) void stream_begin_kernel(uint32_t* d_ctl, const uint32_t* __restrict__ h_ctl, uint32_t words, uint32_t* counters, uint32_t* totals,
                                                           int32_t* trk_seg, uint32_t trk_seg_words) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i < words) d_ctl[i] = h_ctl[i];
    if (i < 8) counters[i] = 0;
    if (i < 4) totals[i] = 0;
    for (uint32_t k = i; k < trk_seg_words; k += gridDim.x * 256) trk_seg[k] = 0;
}
// step epilogue: this step's totals and rows device -> host (mapped pinned memory); only what exists is sent
__global__ __launch_bounds__(256) void stream_push_kernel(const uint32_t* __restrict__ totals, const uint32_t* __restrict__ shared,
                                                          const int32_t* __restrict__ meta, const double* __restrict__ feat, const int32_t* __restrict__ seg,
                                                          uint32_t* h_totals, int32_t* h_meta, double* h_feat, int32_t* h_seg, uint32_t cap_rows, uint32_t cap_segs,
                                                          const double* __restrict__ state, uint32_t n_streams) {
    const uint32_t rows = min(totals[0], cap_rows), segs = min(totals[1], cap_segs);
    const uint32_t tid = blockIdx.x * 256 + threadIdx.x, nth = gridDim.x * 256;
    for (uint32_t i = tid; i < rows * 8; i += nth) h_meta[i] = meta[i];
    for (uint32_t i = tid; i < rows * WSA_NFEAT; i += nth) h_feat[i] = feat[i];
    for (uint32_t i = tid; i < segs * 4; i += nth) h_seg[i] = seg[i];
    if (tid == 0) { h_totals[0] = totals[0]; h_totals[1] = totals[1]; h_totals[2] = totals[2]; h_totals[3] = shared[1]; }
    for (uint32_t i = tid; i < n_streams; i += nth) h_totals[4 + i] = (uint32_t)state[(uint64_t)i * GATE_STATE + 12];     // spans cut at the ring's capacity
}
}  // namespace wsa

extern "C" {

void wsa_stream_destroy(wsa_stream* b) {
    if (!b) return;
    (void)hipSetDevice(b->ctx->device);
    if (b->gexec) (void)hipGraphExecDestroy(b->gexec);
    if (b->own) (void)hipStreamDestroy(b->own);
    if (b->ev_in) (void)hipEventDestroy(b->ev_in);
    if (b->d_collect) (void)hipFree(b->d_collect);
    if (b->h_pk) (void)hipHostFree(b->h_pk);
    if (b->d_chan) (void)hipFree(b->d_chan);
    if (b->d_sel) (void)hipFree(b->d_sel);
    wsa_scls_free(b->scls);
    wsa_sens_free(b->sens);
    wsa_sknn_free(b->sknn);
    wsa_sreg_free(b->sreg);
    delete b;                               // (the arena frees the rest)
}

// fs_in == nullptr: a plain set (every stream at fs); else a mixed set, stream i arriving at fs_in[i] and analysed at fs
static wsa_status create_impl(wsa_ctx* ctx, uint32_t n_streams, const double* fs_in, double fs, uint32_t frames_per_step, uint32_t max_span_frames, wsa_stream** out) {
    if (!ctx || !out || n_streams == 0 || frames_per_step == 0) return fail(ctx, WSA_ERR_INVALID, "bad stream arguments");
    *out = nullptr;
    if (fs_in) if (const wsa_status st = check_rates(ctx, fs_in, n_streams, fs, "stream"); st != WSA_OK) return st;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const wsa_config& c = ctx->cfg;
    if (!(c.output_level == 5 || c.output_level == 13 || c.output_level == 4 || c.output_level == 10 || c.output_level == 12 || c.output_level == 11 || c.output_level == 3))
        return fail(ctx, WSA_ERR_INVALID, "streams support output_level 3, 4, 5, 10, 11, 12 and 13");
    wsa_stream* b = new wsa_stream();
    b->tune = Tuning::from_env();
    b->ctx = ctx; b->n = n_streams; b->F = frames_per_step; b->fs = fs;
    std::string err;
    if (b->fe.build(c, fs, b->tune.fe_fat, err) != FeDev::OK) { delete b; return fail(ctx, WSA_ERR_INVALID, err); }
    const FePlanHost& P = b->fe.plan;
    b->q = (uint32_t)((P.win + P.hop - 1) / P.hop);
    b->hist = (b->q - 1) * (uint32_t)P.hop;
    b->step_samples = b->F * (uint32_t)P.hop;
    b->stage_stride = (b->hist + b->step_samples + (uint32_t)P.win + 3u) & ~3u;
    b->in_stride = b->step_samples; b->F_user = b->F;
    RsMixedPlan rs;
    if (fs_in) {
        // the step's frame capacity — everything F sizes below — comes from the bound on what one step can produce at the set's smallest ratio
        // (resample.hip), not from frames_per_step: a step fed its capacity completes frames_per_step + 1 frames now and then, a STOP step adds the tail
        b->mixed = true; b->ctl_words = RS_CTL_WORDS; b->hist = 0;
        b->fs_in.assign(fs_in, fs_in + n_streams); b->ratio.resize(n_streams); b->in_cap.resize(n_streams);
        b->last_nfr.assign(n_streams, 0); b->last_out.assign(n_streams, 0);
        b->cN.assign(n_streams, 0); b->cY.assign(n_streams, 0); b->cK.assign(n_streams, 0); b->cS.assign(n_streams, 0);
        double min_ratio = 0; uint64_t max_in = 0;
        for (uint32_t i = 0; i < n_streams; i++) {
            b->ratio[i] = fs_in[i] / fs;
            const uint64_t cap = fs_in[i] == fs ? (uint64_t)b->step_samples : (uint64_t)std::ceil((double)b->step_samples * b->ratio[i]);
            if (fs_in[i] != fs && (min_ratio == 0 || b->ratio[i] < min_ratio)) min_ratio = b->ratio[i];
            if (cap > max_in) max_in = cap;
            b->in_cap[i] = (uint32_t)cap;
        }
        b->out_cap = resample_step_outputs_bound(b->F_user, (uint32_t)P.hop, min_ratio);
        b->F = resample_step_frames_bound(b->F_user, (uint32_t)P.hop, min_ratio);
        b->in_stride = ((uint32_t)max_in + 3u) & ~3u;
        b->conv_stride = (b->out_cap + 3u) & ~3u;
        b->xcap = ((uint32_t)RS_HIST + (uint32_t)max_in + (uint32_t)RS_TAPS + 3u) & ~3u;
        b->stage_stride = ((uint32_t)P.win + b->out_cap + 7u) & ~3u;          // fewer than win carried samples in front of at most out_cap new ones
        if (const size_t need = resample_stream_lds(b->xcap); need > LDS_LIMIT) {
            delete b;
            return fail(ctx, WSA_ERR_INVALID, "a step of " + std::to_string(max_in) + " input samples per stream needs " + std::to_string(need) + " bytes of LDS for the rate converter (limit 163840): fewer frames per step");
        }
        std::vector<uint32_t> none(n_streams, 0);
        if (!plan_resample_mixed(n_streams, none.data(), fs_in, fs, rs, err)) { delete b; return fail(ctx, WSA_ERR_INVALID, err); }
    }
    const uint32_t ring = stream_ring_frames(b->F, max_span_frames);
    b->ring = ring;
    const Derived& D = b->D = Derived(c, P.bands);
    BackEnd& B = b->be;
    B.n = n_streams;
    B.set_caps(D, P.bands, ring);
    B.seg_cap = stream_seg_cap(b->F, D);
    B.row_cap = D.syllable_rows ? (int)(ring + b->F) / 2 + 4 : B.seg_cap;
    b->rows_cap = n_streams * (uint32_t)b->be.row_cap; b->segs_cap = n_streams * (uint32_t)b->be.seg_cap;
    b->d2h_rows = b->rows_cap < 1024u ? b->rows_cap : 1024u;
    b->d2h_segs = b->segs_cap < 1024u ? b->segs_cap : 1024u;
    b->warm.assign(n_streams, 0);

    std::vector<uint32_t> foff(n_streams + 1);
    for (uint32_t i = 0; i <= n_streams; i++) foff[i] = i * b->F;
    std::vector<uint32_t> roff(n_streams + 1);
    for (uint32_t i = 0; i <= n_streams; i++) roff[i] = i * ring;
    const size_t nfr_ring = (size_t)n_streams * ring;
    DevArena& A = b->mem;
    bool ok = b->fe.upload(A) && A.upload(&b->d_frame_off, foff) && A.upload(&b->d_ring_off, roff)
           && A.alloc(&b->d_ctl, (size_t)b->ctl_words * n_streams, true) && A.alloc(&b->d_spec, (size_t)n_streams * b->F * P.bands)
           && B.alloc(A, D, nfr_ring, true) && A.alloc(&B.d_counters, 8, true)
           && A.alloc(&B.d_ws, B.ws_stride * (size_t)n_streams, true)      /* one tracker work space per stream (its filing generations start at zero) */
           && (!D.raw_tracks || (A.alloc(&B.d_trk_pts, nfr_ring * 64 * 2) && A.alloc(&B.d_trk_rank, nfr_ring * 64)))
           && (D.level != 11 || A.alloc(&b->d_utt_state, (size_t)n_streams * UTT_STATE_WORDS, true))
           && (D.level != 12 || A.alloc(&B.d_coef_ws, 8 * 2 * nfr_ring))      // a syllable's scratch rows do not wrap: 2 x ring rows per stream
           && A.alloc(&b->d_state, (size_t)n_streams * GATE_STATE, true) && A.alloc(&b->d_carry, (size_t)n_streams * CARRY_WORDS, true)
           && A.alloc(&b->d_tr_state, (size_t)n_streams * TR_STATE_WORDS, true) && A.alloc(&b->d_tr_act, (size_t)n_streams * TR_ACT_BYTES, true)
           && A.alloc(&b->d_fr_span, nfr_ring, true)
           && A.alloc(&b->d_pcm_in, (size_t)n_streams * b->in_stride);
    if (ok && (b->hist || b->mixed)) ok = A.alloc(&b->d_stage, (size_t)n_streams * b->stage_stride, true);
    if (ok && b->mixed) {
        if (rs.tables.empty()) rs.tables.assign(4, 0.f);                   // (every stream at the analysis rate: no table is read)
        ok = A.alloc(&b->d_conv, (size_t)n_streams * b->conv_stride, true) && A.alloc(&b->d_hist, (size_t)n_streams * RS_HIST, true)
          && A.upload(&b->d_rs_tables, rs.tables) && A.upload(&b->d_rs_cls, rs.cls) && A.upload(&b->d_rs_class, rs.clip_class);
    }
    ok = ok && A.pin(&b->h_ctl, &b->h_ctl_dev, (size_t)b->ctl_words * n_streams) && A.pin(&b->h_pcm, &b->h_pcm_dev, (size_t)n_streams * b->in_stride)
            && A.pin(&b->h_totals, &b->h_totals_dev, 4 + (size_t)n_streams) && A.pin(&b->h_meta, &b->h_meta_dev, (size_t)b->d2h_rows * 8)
            && A.pin(&b->h_feat, &b->h_feat_dev, (size_t)b->d2h_rows * WSA_NFEAT) && A.pin(&b->h_seg, &b->h_seg_dev, (size_t)b->d2h_segs * 4);
    ok = ok && hipStreamCreateWithFlags(&b->own, hipStreamNonBlocking) == hipSuccess && hipEventCreateWithFlags(&b->ev_in, hipEventDisableTiming) == hipSuccess;
    if (!ok) {
        const std::string m = std::string("stream allocation failed: ") + hipGetErrorString(hipGetLastError());
        wsa_stream_destroy(b);
        return fail(ctx, WSA_ERR_HIP, m);
    }
    *out = b;
    return WSA_OK;
}

wsa_status wsa_stream_create(wsa_ctx* ctx, uint32_t n_streams, double fs, uint32_t frames_per_step, uint32_t max_span_frames, wsa_stream** out) {
    return create_impl(ctx, n_streams, nullptr, fs, frames_per_step, max_span_frames, out);
}
wsa_status wsa_stream_create_mixed(wsa_ctx* ctx, uint32_t n_streams, const double* fs_in, double fs_out, uint32_t frames_per_step, uint32_t max_span_frames, wsa_stream** out) {
    if (ctx && out && n_streams && !fs_in) return fail(ctx, WSA_ERR_INVALID, "null argument: fs_in holds one rate per stream (stream 0 has none)");
    return create_impl(ctx, n_streams, fs_in, fs_out, frames_per_step, max_span_frames, out);
}

const uint32_t* wsa_stream_spec_internal(wsa_stream* b, wsa_ctx** ctx, uint32_t* n_streams, uint32_t* frames_per_step, uint32_t* bands) {
    *ctx = b->ctx; *n_streams = b->n; *frames_per_step = b->F; *bands = (uint32_t)b->fe.plan.bands;
    return b->d_spec;
}

uint32_t wsa_stream_samples_per_step(const wsa_stream* b) { return b ? b->step_samples : 0; }
uint32_t wsa_stream_input_capacity(const wsa_stream* b, uint32_t i) { return !b || i >= b->n ? 0 : (b->mixed ? b->in_cap[i] : b->step_samples); }
uint32_t wsa_stream_input_stride(const wsa_stream* b) { return b ? b->in_stride : 0; }
uint32_t wsa_stream_step_frame_capacity(const wsa_stream* b) { return b ? b->F : 0; }
// the paced count of a stream's s-th active step since START: floor((s + 1) F hop ratio) - floor(s F hop ratio)
static uint32_t paced_count(const wsa_stream* b, uint32_t i, uint64_t s) {
    if (b->fs_in[i] == b->fs) return b->step_samples;
    const double r = b->ratio[i];
    return (uint32_t)((uint64_t)std::floor((double)((s + 1) * b->step_samples) * r) - (uint64_t)std::floor((double)(s * b->step_samples) * r));
}
uint32_t wsa_stream_paced_input(const wsa_stream* b, uint32_t i) { return !b || i >= b->n ? 0 : (b->mixed ? paced_count(b, i, b->cS[i]) : b->step_samples); }
uint64_t wsa_resample_ready(uint64_t n_in, double fs_in, double fs_out) { return fs_in > 0 && fs_out > 0 ? resample_ready(n_in, fs_in, fs_out) : 0; }
uint32_t wsa_stream_frames_bound(uint32_t frames_per_step, uint32_t hop, double min_ratio) { return resample_step_frames_bound(frames_per_step, hop, min_ratio); }
float* wsa_stream_host_input(wsa_stream* b) { return b ? b->h_pcm : nullptr; }
void* wsa_stream_host_input_packed(wsa_stream* b) { return b && b->fmt != WSA_PCM_F32 ? b->h_pk : nullptr; }
uint32_t wsa_stream_input_stride_bytes(const wsa_stream* b) { return !b ? 0 : (b->fmt != WSA_PCM_F32 ? b->pk_stride : b->in_stride * (uint32_t)sizeof(float)); }

// wsa_stream_set_input_format (select and source NULL, chsel false: the PK-1 pull kernel) and wsa_stream_set_input_channels (PK-3)
static wsa_status set_input_impl(wsa_stream* b, int32_t format, const uint32_t* channels, const uint32_t* select, const uint32_t* source, bool chsel) {
    wsa_ctx* ctx = b->ctx;
    if (format != WSA_PCM_F32 && format != WSA_PCM_I16 && format != WSA_PCM_MULAW && format != WSA_PCM_ALAW)
        return fail(ctx, WSA_ERR_INVALID, "unknown input format " + std::to_string(format) + " (WSA_PCM_F32 0, WSA_PCM_I16 1, WSA_PCM_MULAW 2, WSA_PCM_ALAW 3)");
    uint32_t max_ch = 1;
    for (uint32_t i = 0; channels && i < b->n; i++) {
        if (chsel && source && source[i] != i) continue;          // a consumer takes its source's channel count, its own entry is not read
        if (channels[i] < 1 || channels[i] > 64) return fail(ctx, WSA_ERR_INVALID, "stream " + std::to_string(i) + ": channel count " + std::to_string(channels[i]) + " outside 1 .. 64");
        if (format == WSA_PCM_F32 && channels[i] != 1)
            return fail(ctx, WSA_ERR_INVALID, "stream " + std::to_string(i) + ": " + std::to_string(channels[i]) + " channels with WSA_PCM_F32: float input is mono, interleaved channels need a packed format");
        if (channels[i] > max_ch) max_ch = channels[i];
    }
    std::vector<uint32_t> ss(chsel ? 2 * (size_t)b->n : 0, 0u);     // [select | source], a consumer's channel count is its source's
    std::vector<uint32_t> ch_of(b->n, 1u);
    for (uint32_t i = 0; chsel && i < b->n; i++) {
        const uint32_t src = source ? source[i] : i;
        if (src >= b->n) return fail(ctx, WSA_ERR_INVALID, "stream " + std::to_string(i) + ": source " + std::to_string(src) + " outside 0 .. " + std::to_string(b->n - 1));
        if ((source ? source[src] : src) != src)
            return fail(ctx, WSA_ERR_INVALID, "stream " + std::to_string(i) + ": source " + std::to_string(src) + " is not its own source (it reads stream " + std::to_string(source[src]) + ")");
        ch_of[i] = channels ? channels[src] : 1u;
        ss[i] = select ? select[i] : 0u; ss[b->n + i] = src;
        if (!pcm_select_known(ss[i], ch_of[i]))
            return fail(ctx, WSA_ERR_INVALID, "stream " + std::to_string(i) + ": select " + std::to_string(ss[i]) + " is neither a channel below " + std::to_string(ch_of[i]) + " nor WSA_CHANNEL_MIX");
        if (format == WSA_PCM_F32 && src != i)
            return fail(ctx, WSA_ERR_INVALID, "stream " + std::to_string(i) + ": source " + std::to_string(src) + " with WSA_PCM_F32: float input has one row per stream, shared rows need a packed format");
    }
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (b->stepped) HIP_TRY(ctx, hipStreamSynchronize(b->last_stream ? b->last_stream : b->own));     // the last step may still read the buffer
    if (b->gexec) { (void)hipGraphExecDestroy(b->gexec); b->gexec = nullptr; }         // the next step recaptures with the format's pull kernel
    if (b->h_pk) { (void)hipHostFree(b->h_pk); b->h_pk = b->h_pk_dev = nullptr; }
    if (b->d_chan) { (void)hipFree(b->d_chan); b->d_chan = nullptr; }
    if (b->d_sel) { (void)hipFree(b->d_sel); b->d_sel = nullptr; }
    b->fmt = WSA_PCM_F32; b->chan.clear(); b->pk_stride = 0; b->max_ch = 1; b->chsel = false;
    if (format == WSA_PCM_F32) return WSA_OK;
    std::vector<uint32_t> ch(b->n, 1u);
    if (chsel) ch = ch_of;
    else if (channels) ch.assign(channels, channels + b->n);
    const uint64_t row = ((uint64_t)b->in_stride * max_ch * pcm_sample_bytes(format) + 15u) & ~(uint64_t)15u;
    if (row > 0xFFFFFFF0ull) return fail(ctx, WSA_ERR_INVALID, "a packed input row of " + std::to_string(row) + " bytes: fewer channels or frames per step");
    void *hp = nullptr, *hd = nullptr, *dc = nullptr, *ds = nullptr;
    bool ok = hipHostMalloc(&hp, (size_t)row * b->n, hipHostMallocMapped) == hipSuccess;
    if (ok && chsel) ok = hipMalloc(&ds, ss.size() * sizeof(uint32_t)) == hipSuccess && hipMemcpy(ds, ss.data(), ss.size() * sizeof(uint32_t), hipMemcpyHostToDevice) == hipSuccess;
    if (ok) { std::memset(hp, 0, (size_t)row * b->n); ok = hipHostGetDevicePointer(&hd, hp, 0) == hipSuccess; }
    ok = ok && hipMalloc(&dc, (size_t)b->n * sizeof(uint32_t)) == hipSuccess && hipMemcpy(dc, ch.data(), (size_t)b->n * sizeof(uint32_t), hipMemcpyHostToDevice) == hipSuccess;
    if (!ok) {
        const std::string m = std::string("packed input buffer allocation failed: ") + hipGetErrorString(hipGetLastError());
        if (hp) (void)hipHostFree(hp);
        if (dc) (void)hipFree(dc);
        if (ds) (void)hipFree(ds);
        return fail(ctx, WSA_ERR_HIP, m);
    }
    b->h_pk = static_cast<uint8_t*>(hp); b->h_pk_dev = static_cast<uint8_t*>(hd); b->d_chan = static_cast<uint32_t*>(dc); b->d_sel = static_cast<uint32_t*>(ds);
    b->fmt = format; b->chan = ch; b->pk_stride = (uint32_t)row; b->max_ch = max_ch; b->chsel = chsel;
    return WSA_OK;
}
wsa_status wsa_stream_set_input_format(wsa_stream* b, int32_t format, const uint32_t* channels) {
    return b ? set_input_impl(b, format, channels, nullptr, nullptr, false) : WSA_ERR_INVALID;
}
wsa_status wsa_stream_set_input_channels(wsa_stream* b, int32_t format, const uint32_t* channels, const uint32_t* select, const uint32_t* source) {
    return b ? set_input_impl(b, format, channels, select, source, true) : WSA_ERR_INVALID;
}

wsa_status wsa_stream_enable_graph(wsa_stream* b, int32_t on) {
    if (!b) return WSA_ERR_INVALID;
    b->graph_on = on != 0;
    if (!on && b->gexec) { (void)hipGraphExecDestroy(b->gexec); b->gexec = nullptr; }
    return WSA_OK;
}

// One step in two halves, enqueued one after the other (this is what the graph holds).
// The input half: prologue, the step's samples (pull / stage / K0s) and the front end; it leaves the step's u32 frames in d_spec.
static void enqueue_input(wsa_stream* b, const float* d_pcm, uint64_t stride, bool host_in, hipStream_t s) {
    const Derived& D = b->D;
    const BackEnd& B = b->be;
    const FePlanHost& P = b->fe.plan;
    const uint32_t n = b->n;
    // no memcpy / memset nodes: everything that crosses PCIe goes through mapped pinned buffers, moved by kernels
    const uint32_t cw = b->ctl_words * n;
    hipLaunchKernelGGL(stream_begin_kernel, dim3((cw + 255) / 256), dim3(256), 0, s, b->d_ctl, b->h_ctl_dev, cw, B.d_counters, B.d_totals,
                       B.d_trk_seg, B.d_trk_seg ? (uint32_t)((size_t)n * B.seg_cap * 4) : 0u);
    if (b->fmt != WSA_PCM_F32) {           // packed input (PK-1): d_pcm / stride are the packed device buffer and its row stride in bytes, or the mapped pinned one
        const uint8_t* src = host_in ? b->h_pk_dev : reinterpret_cast<const uint8_t*>(d_pcm);
        const uint64_t src_stride = host_in ? b->pk_stride : stride;
        const uint32_t per_chunk = b->fmt == WSA_PCM_I16 ? 8u : 16u;
        const uint64_t chunks = ((uint64_t)b->in_stride * b->max_ch + per_chunk - 1) / per_chunk;
        const dim3 grid(n, (unsigned)std::min<uint64_t>((chunks + 127) / 128, 1024));
        const uint32_t count_word = b->mixed ? (uint32_t)RS_CTL_NIN : 0u;
        if (b->chsel) {                    // PK-3: a lane per frame
            const dim3 gsel(n, (unsigned)std::min<uint32_t>((b->in_stride + 127u) / 128u, 1024u));
            if (b->fmt == WSA_PCM_I16)
                hipLaunchKernelGGL(stream_pull_channels_kernel<WSA_PCM_I16>, gsel, dim3(128), 0, s, b->d_pcm_in, b->in_stride, src, src_stride, b->d_chan, b->d_sel, b->d_sel + n, b->d_ctl, n, count_word, b->step_samples);
            else if (b->fmt == WSA_PCM_MULAW)
                hipLaunchKernelGGL(stream_pull_channels_kernel<WSA_PCM_MULAW>, gsel, dim3(128), 0, s, b->d_pcm_in, b->in_stride, src, src_stride, b->d_chan, b->d_sel, b->d_sel + n, b->d_ctl, n, count_word, b->step_samples);
            else
                hipLaunchKernelGGL(stream_pull_channels_kernel<WSA_PCM_ALAW>, gsel, dim3(128), 0, s, b->d_pcm_in, b->in_stride, src, src_stride, b->d_chan, b->d_sel, b->d_sel + n, b->d_ctl, n, count_word, b->step_samples);
        } else if (b->fmt == WSA_PCM_I16)
            hipLaunchKernelGGL(stream_pull_packed_kernel<WSA_PCM_I16>, grid, dim3(128), 0, s, b->d_pcm_in, b->in_stride, src, src_stride, b->d_chan, b->d_ctl, n, count_word, b->step_samples);
        else if (b->fmt == WSA_PCM_MULAW)
            hipLaunchKernelGGL(stream_pull_packed_kernel<WSA_PCM_MULAW>, grid, dim3(128), 0, s, b->d_pcm_in, b->in_stride, src, src_stride, b->d_chan, b->d_ctl, n, count_word, b->step_samples);
        else
            hipLaunchKernelGGL(stream_pull_packed_kernel<WSA_PCM_ALAW>, grid, dim3(128), 0, s, b->d_pcm_in, b->in_stride, src, src_stride, b->d_chan, b->d_ctl, n, count_word, b->step_samples);
        d_pcm = b->d_pcm_in; stride = b->in_stride;
    } else if (host_in) {
        const size_t cnt = (size_t)n * b->in_stride;
        hipLaunchKernelGGL(stream_pull_kernel, dim3((unsigned)((cnt / 4 + 256) / 256)), dim3(256), 0, s, b->d_pcm_in, b->h_pcm_dev, cnt);
        d_pcm = b->d_pcm_in; stride = b->in_stride;
    }
    const uint32_t *d_nfr = b->d_ctl, *d_off = b->d_ctl + n, *d_bits = b->d_ctl + 2 * n;
    launch_stream_prepare(b->d_state, b->d_carry, b->d_tr_state, d_bits, n, D.ctx_max0, D.floor0, s);
    if (b->mixed) {                        // K0s in the place of the history shuffle: carried converted samples to the front, this step's outputs behind them
        RsStreamParams r;
        r.stage = b->d_stage; r.stage_stride = b->stage_stride; r.conv = b->d_conv; r.conv_stride = b->conv_stride; r.in = d_pcm; r.in_stride = stride;
        r.hist = b->d_hist; r.ctl = b->d_ctl; r.n = n; r.tables = b->d_rs_tables; r.cls = b->d_rs_cls; r.stream_class = b->d_rs_class; r.xcap = b->xcap;
        launch_resample_stream(r, s);
        d_pcm = b->d_stage; stride = b->stage_stride;
    } else if (b->hist) {
        hipLaunchKernelGGL(stream_stage_kernel, dim3(n), dim3(256), (size_t)b->hist * sizeof(float), s,
                           b->d_stage, b->stage_stride, d_pcm, stride, d_bits, b->hist, b->step_samples);
        d_pcm = b->d_stage; stride = b->stage_stride;
    }
    FeParams p;
    b->fe.fill(p, b->tune.fe_fat);
    p.pcm = d_pcm; p.clip_stride = stride; p.n_frames = d_nfr; p.frame_off = b->d_frame_off; p.spec = b->d_spec; p.pcm_off = d_off;
    p.frames_per_wave = (int)((b->F + 3) / 4); if (p.frames_per_wave > 25) p.frames_per_wave = 25;
    launch_frontend(p, (int)n, (int)b->F, P.R, P.three, s);
}
// The back-end half, from the u32 frames in d_spec and the control words in d_ctl: peak scan, gate, tracker, compaction, the level's and the attached
// models' kernels, epilogue.  (wsa_debug_stream_step_backend enqueues this half behind hand-built frames.)
static wsa_status enqueue_backend(wsa_stream* b, hipStream_t s) {
    wsa_ctx* ctx = b->ctx;
    const Derived& D = b->D;
    const BackEnd& B = b->be;
    const FePlanHost& P = b->fe.plan;
    const uint32_t n = b->n;
    const uint32_t *d_nfr = b->d_ctl, *d_bits = b->d_ctl + 2 * n;
    PkParams pk;
    pk.spec = b->d_spec; pk.rec = B.rec; pk.total_frames = n * b->F; pk.bands = P.bands;
    pk.stream_state = b->d_state; pk.n_frames = d_nfr; pk.step_frames = b->F; pk.ring = b->ring; pk.flags = B.d_counters + 1; pk.lanes_only = b->tune.peaks_lanes ? 1 : 0; pk.round_bins = b->tune.peaks_w;
    launch_peaks(pk, s);
    GateParams g;
    B.fill(g, D);
    g.n_frames = d_nfr; g.state = b->d_state; g.ctl = d_bits; g.ring = b->ring; g.step_frames = b->F; g.fr_span = b->d_fr_span;
    launch_gate_stream(g, s);
    TrParams t;
    B.fill(t, D);
    t.frame_off = b->d_ring_off; t.ring_mask = b->ring - 1;
    t.st_state = b->d_tr_state; t.st_act = b->d_tr_act; t.fr_span = b->d_fr_span; t.n_frames_step = d_nfr; t.gate_state = b->d_state;
    launch_tracker_stream(t, n, s);       // one wave per stream: this step's frames go into the stream's tracker state, closed segments are finalized
    CompactParams cp;
    B.fill(cp, D);
    cp.carry = b->d_carry; cp.ctl = d_bits;
    launch_compact(cp, s);
    HIP_TRY(ctx, hipGetLastError());
    if (D.level == 12) {                   // K5 on the step's syllable rows: four polynomial fits each, frames and energy sums out of the rings
        CoefParams q;
        B.fill(q, b->d_ring_off);
        q.total_frames = n * 2 * b->ring; q.ring_mask = b->ring - 1; q.scratch_stride = 2 * b->ring;
        launch_coeffs(q, b->rows_cap, s);
        HIP_TRY(ctx, hipGetLastError());
    }
    if (D.level == 11) {                   // K4 on the step's results: the launch's histograms are carried per stream
        UttParams u;
        B.fill(u, b->d_ring_off);
        u.state = b->d_utt_state; u.carry = b->d_carry; u.ctl = d_bits; u.ring_mask = b->ring - 1;
        launch_utterance(u, s);
        HIP_TRY(ctx, hipGetLastError());
    }
    if (b->scls) {                         // K6 on the step's rows, then (level 13) the fold carried per stream; both push their tables themselves
        const wsa_status st = wsa_scls_enqueue(b->scls, s);
        if (st != WSA_OK) return st;
    }
    if (b->sens) {                         // K6e, the (stream, member) folds and the decision
        const wsa_status st = wsa_sens_enqueue(b->sens, s);
        if (st != WSA_OK) return st;
    }
    if (b->sknn) {                         // K9s (partial, merge), then the push / KN-2 fold kernel
        const wsa_status st = wsa_sknn_enqueue(b->sknn, s);
        if (st != WSA_OK) return st;
    }
    if (b->sreg) {                         // the grouped K6 over the regression heads, then the push / RG-1 fold kernel
        const wsa_status st = wsa_sreg_enqueue(b->sreg, s);
        if (st != WSA_OK) return st;
    }
    hipLaunchKernelGGL(stream_push_kernel, dim3(16), dim3(256), 0, s, b->be.d_totals, b->be.d_counters, b->be.d_meta, b->be.d_feat, b->be.d_seg,
                       b->h_totals_dev, b->h_meta_dev, b->h_feat_dev, b->h_seg_dev, b->d2h_rows, b->d2h_segs, b->d_state, b->n);
    HIP_TRY(ctx, hipGetLastError());
    return WSA_OK;
}
static wsa_status enqueue_step(wsa_stream* b, const float* d_pcm, uint64_t stride, bool host_in, hipStream_t s) {
    enqueue_input(b, d_pcm, stride, host_in, s);
    return enqueue_backend(b, s);
}

// Test entry behind wsa_debug_stream_step_backend (debug.hip; not part of wsa.h): one step of a plain set whose u32 frames come from the caller instead of
// the front end.  Stream i gets n_frames[i] <= frames_per_step frames (frames [n][frames_per_step][bands] on the host, the first n_frames[i] of its block)
// under the control byte ctl[i].  The control words are written as step_impl writes them (nfr as given, off 0, the same bits; no warm-up frames are
// skipped), then the product's own launches run without capture: the prologue, launch_stream_prepare and the back-end half of the step.
// wsa_stream_collect works as after any step.  The step counter, `stepped` and `last_stream` move as in step_impl, but nothing here feeds the input
// half's carried samples: an object steps EITHER through this entry OR through wsa_stream_step*, never both.
wsa_status wsa_stream_step_backend_internal(wsa_stream* b, const uint32_t* n_frames, const uint8_t* ctl, const uint32_t* frames, uint32_t bands, void* stream) {
    wsa_ctx* ctx = b->ctx;
    const uint32_t n = b->n, F = b->F, own_bands = (uint32_t)b->fe.plan.bands;
    if (b->mixed) return fail(ctx, WSA_ERR_INVALID, "wsa_debug_stream_step_backend: a mixed-rate stream set has no step of whole frames (streams 0 .. " + std::to_string(n - 1) + " convert their input)");
    if (!n_frames || !ctl || !frames) return fail(ctx, WSA_ERR_INVALID, std::string("wsa_debug_stream_step_backend: null ") + (!n_frames ? "frame counts" : !ctl ? "control bytes" : "frames") + " for streams 0 .. " + std::to_string(n - 1));
    if (bands != own_bands) return fail(ctx, WSA_ERR_INVALID, "wsa_debug_stream_step_backend: frames of " + std::to_string(bands) + " bands, streams 0 .. " + std::to_string(n - 1) + " analyse " + std::to_string(own_bands));
    for (uint32_t i = 0; i < n; i++)
        if (n_frames[i] > F) return fail(ctx, WSA_ERR_INVALID, "wsa_debug_stream_step_backend: stream " + std::to_string(i) + ": " + std::to_string(n_frames[i]) + " frames in one step, frames_per_step is " + std::to_string(F));
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (!s) {
        HIP_TRY(ctx, hipEventRecord(b->ev_in, nullptr));
        s = b->own;
        HIP_TRY(ctx, hipStreamWaitEvent(s, b->ev_in, 0));
    }
    if (b->stepped) HIP_TRY(ctx, hipStreamSynchronize(b->last_stream ? b->last_stream : s));      // the previous step still reads the pinned control words
    b->last_stream = s;
    for (uint32_t i = 0; i < n; i++) {
        const uint32_t cb = ctl[i];
        uint32_t bits = 0;
        if (cb & WSA_STREAM_START) bits |= 1u;
        if (cb & WSA_STREAM_ACTIVE) bits |= 4u;
        if (cb & WSA_STREAM_STOP) bits |= 2u;
        b->h_ctl[i] = (cb & WSA_STREAM_ACTIVE) ? n_frames[i] : 0u; b->h_ctl[n + i] = 0; b->h_ctl[2 * n + i] = bits;
    }
    // (the copy is ordered behind the previous step by the synchronize above, the launches below behind the copy by the stream)
    HIP_TRY(ctx, hipMemcpyAsync(b->d_spec, frames, (size_t)n * F * own_bands * sizeof(uint32_t), hipMemcpyHostToDevice, s));
    const uint32_t cw = b->ctl_words * n;
    hipLaunchKernelGGL(stream_begin_kernel, dim3((cw + 255) / 256), dim3(256), 0, s, b->d_ctl, b->h_ctl_dev, cw, b->be.d_counters, b->be.d_totals,
                       b->be.d_trk_seg, b->be.d_trk_seg ? (uint32_t)((size_t)n * b->be.seg_cap * 4) : 0u);
    launch_stream_prepare(b->d_state, b->d_carry, b->d_tr_state, b->d_ctl + 2 * n, n, b->D.ctx_max0, b->D.floor0, s);
    const wsa_status st = enqueue_backend(b, s);
    if (st != WSA_OK) return st;
    b->steps++; b->stepped = true;
    return WSA_OK;
}

static wsa_status step_impl(wsa_stream* b, const float* d_pcm, uint64_t stride, bool host_in, const uint32_t* n_in, const uint8_t* ctl, hipStream_t s) {
    wsa_ctx* ctx = b->ctx;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (!s) {                      // NULL stream: run on the object's own stream, after what the NULL stream holds now
        HIP_TRY(ctx, hipEventRecord(b->ev_in, nullptr));
        s = b->own;
        HIP_TRY(ctx, hipStreamWaitEvent(s, b->ev_in, 0));
    }
    if (!host_in && !d_pcm) return fail(ctx, WSA_ERR_INVALID, "null PCM pointer");
    const bool packed = b->fmt != WSA_PCM_F32;
    if (packed && !host_in) {              // device-resident packed input: rows are read in whole 16-byte chunks
        if (stride % 16 != 0) return fail(ctx, WSA_ERR_INVALID, "stream_stride_bytes " + std::to_string(stride) + " is not a multiple of 16");
        if (reinterpret_cast<uintptr_t>(d_pcm) % 16 != 0) return fail(ctx, WSA_ERR_INVALID, "the packed input pointer is not aligned to 16 bytes");
    }
    if (!packed && !b->mixed && !host_in && stride < b->step_samples && b->n > 1) return fail(ctx, WSA_ERR_INVALID, "stream_stride smaller than samples_per_step");
    const auto ctl_of = [&](uint32_t i) -> uint32_t { return ctl ? ctl[i] : (b->steps == 0 ? (WSA_STREAM_ACTIVE | WSA_STREAM_START) : WSA_STREAM_ACTIVE); };
    for (uint32_t i = 0; n_in && i < b->n; i++) {           // counts are checked before anything is counted
        if (!(ctl_of(i) & WSA_STREAM_ACTIVE)) continue;
        if (!b->mixed && n_in[i] != b->step_samples)
            return fail(ctx, WSA_ERR_INVALID, "stream " + std::to_string(i) + ": a plain stream set takes exactly " + std::to_string(b->step_samples) + " samples per step, not " + std::to_string(n_in[i]));
        if (b->mixed && n_in[i] > b->in_cap[i])
            return fail(ctx, WSA_ERR_INVALID, "stream " + std::to_string(i) + ": " + std::to_string(n_in[i]) + " samples in one step, its capacity is " + std::to_string(b->in_cap[i]));
        if (!packed && b->mixed && !host_in && b->n > 1 && stride < n_in[i]) return fail(ctx, WSA_ERR_INVALID, "stream_stride smaller than the samples of stream " + std::to_string(i));
    }
    for (uint32_t i = 0; packed && !host_in && i < b->n; i++) {        // the largest row any active stream can have in this step fits the stride
        if (!(ctl_of(i) & WSA_STREAM_ACTIVE)) continue;
        const uint64_t cnt = n_in ? n_in[i] : (b->mixed ? b->in_cap[i] : b->step_samples);
        const uint64_t need = cnt * b->chan[i] * pcm_sample_bytes(b->fmt);
        if (need > stride)
            return fail(ctx, WSA_ERR_INVALID, "stream_stride_bytes " + std::to_string(stride) + " too small: stream " + std::to_string(i) + " carries " + std::to_string(cnt) + " frames of "
                        + std::to_string(b->chan[i]) + " channels, " + std::to_string(need) + " bytes");
    }
    for (uint32_t i = 0; !packed && b->mixed && !n_in && !host_in && b->n > 1 && i < b->n; i++)      // paced: no count exceeds the capacity
        if (stride < b->in_cap[i]) return fail(ctx, WSA_ERR_INVALID, "stream_stride smaller than the input capacity of stream " + std::to_string(i));
    // the pinned control words are read by the step's first H2D copy: the previous step must be done
    if (b->stepped) HIP_TRY(ctx, hipStreamSynchronize(b->last_stream ? b->last_stream : s));      // ... on whichever stream it ran
    b->last_stream = s;
    const uint32_t n = b->n, F = b->F;
    for (uint32_t i = 0; b->mixed && i < n; i++) {
        // Every count of a mixed set is decided here, in integers and one exact predicate in double (resample_ready); the device only carries them out.
        const uint32_t cb = ctl_of(i), hop = (uint32_t)b->fe.plan.hop, win = (uint32_t)b->fe.plan.win;
        uint32_t* w = b->h_ctl + i;
        uint32_t bits = 0;
        if (cb & WSA_STREAM_START) { b->cN[i] = b->cY[i] = b->cK[i] = b->cS[i] = 0; b->last_nfr[i] = 0; bits |= 1u; }
        if (cb & WSA_STREAM_STOP) bits |= 2u;
        b->last_out[i] = 0;
        w[RS_CTL_NFR * n] = 0; w[RS_CTL_OFF * n] = 0; w[RS_CTL_NIN * n] = 0; w[RS_CTL_NOUT * n] = 0;
        if (cb & WSA_STREAM_ACTIVE) {
            bits |= 4u;
            const uint32_t cnt = n_in ? n_in[i] : paced_count(b, i, b->cS[i]);
            const uint64_t N0 = b->cN[i], Y0 = b->cY[i], K0 = b->cK[i], N1 = N0 + cnt;
            uint64_t Y1 = (cb & WSA_STREAM_STOP) ? resample_length(N1, b->fs_in[i], b->fs) : resample_ready(N1, b->fs_in[i], b->fs);
            if (b->fs_in[i] == b->fs) Y1 = N1;
            if (Y1 < Y0) Y1 = Y0;                          // (active again after a STOP without a START: nothing is taken back)
            const uint64_t K1 = Y1 >= win ? (Y1 - win) / hop + 1 : 0;
            const int64_t in0 = (int64_t)N0 - RS_HIST, dst0 = (int64_t)Y0 - (int64_t)(K0 * hop);
            const bool conv = b->fs_in[i] != b->fs && Y1 > Y0;
            if (Y1 - Y0 > b->out_cap || K1 < K0 || K1 - K0 > b->F || dst0 + (int64_t)(Y1 - Y0) > (int64_t)b->stage_stride || dst0 < -(int64_t)hop || (conv && (int64_t)std::floor((double)Y0 * b->ratio[i]) - RS_TAPS / 2 < in0)
                || (conv && (int64_t)std::floor((double)(Y1 - 1) * b->ratio[i]) + RS_TAPS / 2 - in0 > (int64_t)b->xcap))
                return fail(ctx, WSA_ERR_CAPACITY, "stream " + std::to_string(i) + ": a step outside the derived bounds (" + std::to_string(Y1 - Y0) + " outputs, "
                            + std::to_string(K1 - K0) + " frames; capacity " + std::to_string(b->out_cap) + ", " + std::to_string(b->F) + ")");
            w[RS_CTL_NFR * n] = (uint32_t)(K1 - K0); w[RS_CTL_NIN * n] = cnt; w[RS_CTL_NOUT * n] = (uint32_t)(Y1 - Y0);
            w[RS_CTL_DST * n] = (uint32_t)(int32_t)dst0; w[RS_CTL_SHIFT * n] = b->last_nfr[i] * hop; w[RS_CTL_CARRY * n] = dst0 > 0 ? (uint32_t)dst0 : 0u;
            w[RS_CTL_Y_LO * n] = (uint32_t)Y0; w[RS_CTL_Y_HI * n] = (uint32_t)(Y0 >> 32);
            w[RS_CTL_IN0_LO * n] = (uint32_t)(uint64_t)in0; w[RS_CTL_IN0_HI * n] = (uint32_t)((uint64_t)in0 >> 32);
            b->cN[i] = N1; b->cY[i] = Y1; b->cK[i] = K1; b->cS[i]++;
            b->last_nfr[i] = (uint32_t)(K1 - K0); b->last_out[i] = (uint32_t)(Y1 - Y0);
        }
        w[RS_CTL_BITS * n] = bits;
    }
    for (uint32_t i = 0; !b->mixed && i < n; i++) {
        const uint32_t cb = ctl_of(i);
        uint32_t bits = 0, nfr = 0, off = 0;
        if (cb & WSA_STREAM_START) { b->warm[i] = b->q - 1; bits |= 1u; }
        if (cb & WSA_STREAM_ACTIVE) {
            const uint32_t skip = b->warm[i] < F ? b->warm[i] : F;
            b->warm[i] -= skip; nfr = F - skip; off = skip * (uint32_t)b->fe.plan.hop; bits |= 4u;
        }
        if (cb & WSA_STREAM_STOP) bits |= 2u;
        b->h_ctl[i] = nfr; b->h_ctl[n + i] = off; b->h_ctl[2 * n + i] = bits;
    }
    if (b->graph_on && b->steps >= 1) {
        if (b->gexec && (b->g_pcm != d_pcm || b->g_stride != stride || b->g_stream != s || b->g_host != host_in || b->g_fmt != b->fmt)) { (void)hipGraphExecDestroy(b->gexec); b->gexec = nullptr; }
        if (!b->gexec) {
            hipGraph_t graph = nullptr;
            HIP_TRY(ctx, hipStreamBeginCapture(s, hipStreamCaptureModeThreadLocal));
            const wsa_status st = enqueue_step(b, d_pcm, stride, host_in, s);
            const hipError_t e = hipStreamEndCapture(s, &graph);
            if (st != WSA_OK) { if (graph) (void)hipGraphDestroy(graph); return st; }
            if (e != hipSuccess) return fail(ctx, WSA_ERR_HIP, std::string("hipStreamEndCapture: ") + hipGetErrorString(e));
            const hipError_t e2 = hipGraphInstantiate(&b->gexec, graph, nullptr, nullptr, 0);
            (void)hipGraphDestroy(graph);
            if (e2 != hipSuccess) { b->gexec = nullptr; return fail(ctx, WSA_ERR_HIP, std::string("hipGraphInstantiate: ") + hipGetErrorString(e2)); }
            b->g_pcm = d_pcm; b->g_stride = stride; b->g_stream = s; b->g_host = host_in; b->g_fmt = b->fmt;
        }
        HIP_TRY(ctx, hipGraphLaunch(b->gexec, s));
    } else {
        const wsa_status st = enqueue_step(b, d_pcm, stride, host_in, s);
        if (st != WSA_OK) return st;
    }
    b->steps++; b->stepped = true;
    return WSA_OK;
}

static wsa_status refuse_float_entry(wsa_stream* b, const char* name) {
    return fail(b->ctx, WSA_ERR_INVALID, std::string(name) + " takes floats, this set's input format is " + pcm_format_name(b->fmt)
                + ": use wsa_stream_step_packed, or wsa_stream_set_input_format(WSA_PCM_F32)");
}
wsa_status wsa_stream_step(wsa_stream* b, const float* d_pcm, uint64_t stream_stride, const uint8_t* ctl, void* stream) {
    if (!b) return WSA_ERR_INVALID;
    if (b->fmt != WSA_PCM_F32) return refuse_float_entry(b, "wsa_stream_step");
    return step_impl(b, d_pcm, stream_stride, false, nullptr, ctl, reinterpret_cast<hipStream_t>(stream));
}
wsa_status wsa_stream_step_host(wsa_stream* b, const uint8_t* ctl, void* stream) {
    if (!b) return WSA_ERR_INVALID;
    return step_impl(b, nullptr, 0, true, nullptr, ctl, reinterpret_cast<hipStream_t>(stream));
}
wsa_status wsa_stream_step_n(wsa_stream* b, const float* d_pcm, uint64_t stream_stride, const uint32_t* n_in, const uint8_t* ctl, void* stream) {
    if (!b) return WSA_ERR_INVALID;
    if (b->fmt != WSA_PCM_F32) return refuse_float_entry(b, "wsa_stream_step_n");
    return step_impl(b, d_pcm, stream_stride, false, n_in, ctl, reinterpret_cast<hipStream_t>(stream));
}
wsa_status wsa_stream_step_packed(wsa_stream* b, const void* d_pcm, uint64_t stream_stride_bytes, const uint32_t* n_in, const uint8_t* ctl, void* stream) {
    if (!b) return WSA_ERR_INVALID;
    if (b->fmt == WSA_PCM_F32) return fail(b->ctx, WSA_ERR_INVALID, "wsa_stream_step_packed on a set whose input format is WSA_PCM_F32: set a packed format with wsa_stream_set_input_format first");
    return step_impl(b, static_cast<const float*>(d_pcm), stream_stride_bytes, false, n_in, ctl, reinterpret_cast<hipStream_t>(stream));
}
wsa_status wsa_stream_step_host_n(wsa_stream* b, const uint32_t* n_in, const uint8_t* ctl, void* stream) {
    if (!b) return WSA_ERR_INVALID;
    return step_impl(b, nullptr, 0, true, n_in, ctl, reinterpret_cast<hipStream_t>(stream));
}
wsa_status wsa_stream_copy_converted(wsa_stream* b, float* out, uint32_t cap, uint32_t* counts) {
    if (!b) return WSA_ERR_INVALID;
    wsa_ctx* ctx = b->ctx;
    if (!b->mixed) return fail(ctx, WSA_ERR_INVALID, "no converted samples: the stream set must come from wsa_stream_create_mixed");
    if (!b->stepped) return fail(ctx, WSA_ERR_INVALID, "no step on this stream object yet");
    for (uint32_t i = 0; i < b->n; i++) {
        if (out && b->last_out[i] > cap) return fail(ctx, WSA_ERR_INVALID, "stream " + std::to_string(i) + " produced " + std::to_string(b->last_out[i]) + " converted samples in the last step, the buffer holds " + std::to_string(cap) + " per stream");
        if (counts) counts[i] = b->last_out[i];
    }
    if (!out) return WSA_OK;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipStreamSynchronize(b->last_stream ? b->last_stream : b->own));
    const uint32_t wcols = cap < b->conv_stride ? cap : b->conv_stride;
    if (wcols) HIP_TRY(ctx, hipMemcpy2D(out, (size_t)cap * sizeof(float), b->d_conv, (size_t)b->conv_stride * sizeof(float), (size_t)wcols * sizeof(float), b->n, hipMemcpyDeviceToHost));
    return WSA_OK;
}

}  // extern "C"

// ---- collect helpers (levels 3 / 4 / 10): a step's rows / segments point into the streams' rings; one kernel gathers the pieces (a span
// may wrap around its ring) into a staging buffer in the order the host hands them out, and one copy fetches them — instead of a
// synchronous copy per piece (dozens per step at many streams).
__global__ __launch_bounds__(64) void stream_gather_formants_kernel(const int32_t* meta, uint32_t rows, const float* formants, uint32_t ring, float* out) {
    const uint32_t r = blockIdx.x, lane = threadIdx.x;
    uint32_t off = 0;                                        // frames of the rows in front of this one (rows per step: tens)
    for (uint32_t q = lane; q < r; q += 64) off += (uint32_t)meta[8 * q + 7];
    for (int d = 32; d > 0; d >>= 1) off += (uint32_t)__shfl_xor((int)off, d, 64);
    const uint32_t sidx = (uint32_t)meta[8 * r], f0 = (uint32_t)meta[8 * r + 6], len = (uint32_t)meta[8 * r + 7];
    for (uint32_t i = lane; i < len * 9u; i += 64) {
        const uint32_t fr = i / 9u, c = i - fr * 9u;
        out[(size_t)(off + fr) * 9 + c] = formants[((size_t)sidx * ring + ((f0 + fr) & (ring - 1))) * 9 + c];
    }
}
static bool collect_stage(wsa_stream* b, size_t bytes) {
    if (bytes <= b->collect_cap) return true;
    if (b->d_collect) { (void)hipFree(b->d_collect); b->d_collect = nullptr; b->collect_cap = 0; }
    const size_t want = bytes + bytes / 2 + 4096;
    if (hipMalloc(reinterpret_cast<void**>(&b->d_collect), want) != hipSuccess) { (void)hipGetLastError(); return false; }
    b->collect_cap = want;
    return true;
}

extern "C" {

wsa_status wsa_stream_collect(wsa_stream* b, void* stream, wsa_stream_rows* o) {
    if (!b || !o) return WSA_ERR_INVALID;
    wsa_ctx* ctx = b->ctx;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (!s) s = b->own;
    if (!b->stepped) return fail(ctx, WSA_ERR_INVALID, "no step on this stream object yet");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipStreamSynchronize(s));
    const uint32_t rows = b->h_totals[0], segs = b->h_totals[1];
    o->n_rows = rows; o->n_segments = segs; o->status_flags = (b->h_totals[3] & 1u) | (b->h_totals[2] ? 1u : 0u);
    o->row_meta = b->h_meta; o->row_feat = b->h_feat; o->segments = b->h_seg; o->stream_cuts = b->h_totals + 4;
    // a span cut at the ring's capacity in this step is flagged for hosts that do not look at the per-stream counters
    if (b->seen_cuts.size() != b->n) b->seen_cuts.assign(b->n, 0u);
    for (uint32_t i = 0; i < b->n; i++) if (b->h_totals[4 + i] != b->seen_cuts[i]) { o->status_flags |= WSA_FLAG_STREAM_CUT; b->seen_cuts[i] = b->h_totals[4 + i]; }
    if (rows > b->d2h_rows) {                 // more rows than the fixed window of the step: fetch them all
        b->x_meta.resize((size_t)rows * 8); b->x_feat.resize((size_t)rows * WSA_NFEAT);
        HIP_TRY(ctx, hipMemcpy(b->x_meta.data(), b->be.d_meta, (size_t)rows * 8 * sizeof(int32_t), hipMemcpyDeviceToHost));
        HIP_TRY(ctx, hipMemcpy(b->x_feat.data(), b->be.d_feat, (size_t)rows * WSA_NFEAT * sizeof(double), hipMemcpyDeviceToHost));
        o->row_meta = b->x_meta.data(); o->row_feat = b->x_feat.data();
    }
    if (segs > b->d2h_segs) {
        b->x_seg.resize((size_t)segs * 4);
        HIP_TRY(ctx, hipMemcpy(b->x_seg.data(), b->be.d_seg, (size_t)segs * 4 * sizeof(int32_t), hipMemcpyDeviceToHost));
        o->segments = b->x_seg.data();
    }
    o->formants = nullptr; o->row_formant_off = nullptr;
    o->n_track_points = 0; o->n_track_ranked = 0; o->track_off = nullptr; o->track_points = nullptr; o->track_ranked = nullptr;
    if (b->be.d_trk_pts) {
        // level 3: the ranked raw tracks of every segment of this step (as wsa_batch_copy_tracks: offsets [n_segments + 1][2], points [8 ints], ranked
        // track ids), unwrapped out of the stream's pool ring.  Segments arrive in (stream, k) order; the device table is per (stream, k of this step)
        const int32_t* sgm = o->segments;
        b->x_trk_seg.resize((size_t)b->n * b->be.seg_cap * 4);
        if (segs) HIP_TRY(ctx, hipMemcpy(b->x_trk_seg.data(), b->be.d_trk_seg, b->x_trk_seg.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
        TrackGather& G = b->trk;
        G.begin();
        uint32_t kk = 0; int32_t last_stream = -1;
        const uint64_t region = (uint64_t)b->ring * 64;
        for (uint32_t q = 0; q < segs; q++) {
            const int32_t sidx = sgm[4 * q];
            kk = sidx == last_stream ? kk + 1 : 0; last_stream = sidx;
            G.add(&b->x_trk_seg[((size_t)sidx * b->be.seg_cap + kk) * 4], (uint64_t)sidx * region);
        }
        const uint64_t np = G.n_points, nr = G.n_ranked;
        b->x_trk_off.resize(2 * ((size_t)segs + 1)); G.offsets(b->x_trk_off.data());
        b->x_trk_pts.resize((size_t)np * 8 + 8); b->x_trk_rank.resize((size_t)nr + 1);
        if (const wsa_status gs = G.run(ctx, region, b->be.d_trk_pts, b->be.d_trk_rank, b->x_trk_pts.data(), b->x_trk_rank.data(), s); gs != WSA_OK) return gs;
        if (np + nr) HIP_TRY(ctx, hipStreamSynchronize(s));
        o->n_track_points = np; o->n_track_ranked = nr; o->track_off = b->x_trk_off.data(); o->track_points = b->x_trk_pts.data(); o->track_ranked = b->x_trk_rank.data();
    }
    o->n_utterance_rows = 0; o->utt_meta = nullptr; o->utt_feat = nullptr;
    if (b->d_utt_state) {
        // level 11: one 264-vector per result of this step (in (stream, result) order: the segments of the step that produced a result entry)
        uint32_t nu = 0;
        for (uint32_t k = 0; k < segs; k++) nu += o->segments[4 * k + 3] >= 0 ? 1u : 0u;
        b->x_utt_meta.resize((size_t)nu * 4 + 1); b->x_utt_feat.resize((size_t)nu * WSA_NUTT + 1);
        if (nu) {
            HIP_TRY(ctx, hipMemcpy(b->x_utt_meta.data(), b->be.d_utt_meta, (size_t)nu * 4 * sizeof(int32_t), hipMemcpyDeviceToHost));
            HIP_TRY(ctx, hipMemcpy(b->x_utt_feat.data(), b->be.d_utt_feat, (size_t)nu * WSA_NUTT * sizeof(double), hipMemcpyDeviceToHost));
        }
        o->n_utterance_rows = nu; o->utt_meta = b->x_utt_meta.data(); o->utt_feat = b->x_utt_feat.data();
    }
    if (b->be.d_formants && !b->be.d_sums && !b->d_utt_state) {
        // levels 4 / 10: the straightened frames of every row's segment / syllable (meta[6] = first frame since the stream's START,
        // meta[7] frames) come out of the stream's ring: one gather kernel and one copy at collect time (not part of the graph)
        const int32_t* m = o->row_meta;
        b->x_formant_off.resize((size_t)rows + 1);
        size_t tot = 0;
        for (uint32_t r = 0; r < rows; r++) { b->x_formant_off[r] = (uint32_t)tot; tot += (size_t)m[8 * r + 7]; }
        b->x_formant_off[rows] = (uint32_t)tot;
        b->x_formants.resize(tot * 9 + 1);
        if (tot) {
            // the rows' table on the device is the one the host holds (b->be.d_meta: compacted rows of this step)
            if (!collect_stage(b, tot * 9 * sizeof(float))) return fail(ctx, WSA_ERR_HIP, "no device memory for the collect staging buffer");
            hipLaunchKernelGGL(stream_gather_formants_kernel, dim3(rows), dim3(64), 0, s, b->be.d_meta, rows, b->be.d_formants, b->ring, reinterpret_cast<float*>(b->d_collect));
            HIP_TRY(ctx, hipGetLastError());
            HIP_TRY(ctx, hipMemcpyAsync(b->x_formants.data(), b->d_collect, tot * 9 * sizeof(float), hipMemcpyDeviceToHost, s));
            HIP_TRY(ctx, hipStreamSynchronize(s));
        }
        o->formants = b->x_formants.data(); o->row_formant_off = b->x_formant_off.data();
    }
    if (o->status_flags & 1u)
        return fail(ctx, WSA_ERR_CAPACITY, "a device-side arena overflowed; results are invalid (step "
                    + std::to_string(b->steps) + ", flags " + std::to_string(b->h_totals[3]) + ", history " + std::to_string(b->h_totals[2]) + ")");
    return WSA_OK;
}

wsa_status wsa_stream_set_model(wsa_stream* b, const wsa_model* m) {
    if (!b) return WSA_ERR_INVALID;
    wsa_ctx* ctx = b->ctx;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (b->stepped) HIP_TRY(ctx, hipStreamSynchronize(b->last_stream ? b->last_stream : b->own));     // the last step may still read the tables
    wsa_scls* n = nullptr;
    if (m) {
        const wsa_scls_view v{ctx, ctx->cfg.output_level, b->n, b->rows_cap, b->d2h_rows, b->be.d_meta, b->be.d_feat, b->be.d_row_off, b->be.d_totals, b->d_ctl + 2 * (size_t)b->n};
        const wsa_status st = wsa_scls_create(v, m, &n);
        if (st != WSA_OK) return st;
    }
    if (b->gexec) { (void)hipGraphExecDestroy(b->gexec); b->gexec = nullptr; }         // the next step recaptures with (or without) the classifier
    wsa_scls_free(b->scls);
    b->scls = n;
    if (m) { wsa_sens_free(b->sens); b->sens = nullptr; }      // setting a model detaches an ensemble
    return WSA_OK;
}

wsa_status wsa_stream_set_ensemble(wsa_stream* b, const wsa_ensemble* e) {
    if (!b) return WSA_ERR_INVALID;
    wsa_ctx* ctx = b->ctx;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (b->stepped) HIP_TRY(ctx, hipStreamSynchronize(b->last_stream ? b->last_stream : b->own));     // the last step may still read the tables
    wsa_sens* n = nullptr;
    if (e) {
        const wsa_scls_view v{ctx, ctx->cfg.output_level, b->n, b->rows_cap, b->d2h_rows, b->be.d_meta, b->be.d_feat, b->be.d_row_off, b->be.d_totals, b->d_ctl + 2 * (size_t)b->n};
        const wsa_status st = wsa_sens_create(v, e, &n);
        if (st != WSA_OK) return st;
    }
    if (b->gexec) { (void)hipGraphExecDestroy(b->gexec); b->gexec = nullptr; }         // the next step recaptures with (or without) the ensemble
    wsa_sens_free(b->sens);
    b->sens = n;
    if (e) { wsa_scls_free(b->scls); b->scls = nullptr; }      // setting an ensemble detaches a model
    return WSA_OK;
}

wsa_status wsa_stream_set_knn(wsa_stream* b, const wsa_knn* kn, uint32_t k) {
    if (!b) return WSA_ERR_INVALID;
    wsa_ctx* ctx = b->ctx;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (b->stepped) HIP_TRY(ctx, hipStreamSynchronize(b->last_stream ? b->last_stream : b->own));     // the last step may still read the tables
    wsa_sknn* n = nullptr;
    if (kn) {
        const wsa_scls_view v{ctx, ctx->cfg.output_level, b->n, b->rows_cap, b->d2h_rows, b->be.d_meta, b->be.d_feat, b->be.d_row_off, b->be.d_totals, b->d_ctl + 2 * (size_t)b->n};
        const wsa_status st = wsa_sknn_create(v, kn, k, &n);
        if (st != WSA_OK) return st;
    }
    if (b->gexec) { (void)hipGraphExecDestroy(b->gexec); b->gexec = nullptr; }         // the next step recaptures with (or without) the KNN kernels
    wsa_sknn_free(b->sknn);
    b->sknn = n;                                                                       // (a model or an ensemble stays attached)
    return WSA_OK;
}

wsa_status wsa_stream_knn_classes(wsa_stream* b, wsa_stream_knn_result* out) {
    if (!b || !out) return WSA_ERR_INVALID;
    wsa_ctx* ctx = b->ctx;
    if (!b->sknn) return fail(ctx, WSA_ERR_INVALID, "no KNN store attached to these streams (wsa_stream_set_knn)");
    if (!b->stepped) return fail(ctx, WSA_ERR_INVALID, "no step on this stream object yet");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipStreamSynchronize(b->last_stream ? b->last_stream : b->own));
    return wsa_sknn_result(b->sknn, b->h_totals[0], out);
}

wsa_status wsa_stream_set_regress(wsa_stream* b, const wsa_regress_group* g) {
    if (!b) return WSA_ERR_INVALID;
    wsa_ctx* ctx = b->ctx;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (b->stepped) HIP_TRY(ctx, hipStreamSynchronize(b->last_stream ? b->last_stream : b->own));     // the last step may still read the tables
    wsa_sreg* n = nullptr;
    if (g) {
        const wsa_scls_view v{ctx, ctx->cfg.output_level, b->n, b->rows_cap, b->d2h_rows, b->be.d_meta, b->be.d_feat, b->be.d_row_off, b->be.d_totals, b->d_ctl + 2 * (size_t)b->n};
        const wsa_status st = wsa_sreg_create(v, g, &n);
        if (st != WSA_OK) return st;
    }
    if (b->gexec) { (void)hipGraphExecDestroy(b->gexec); b->gexec = nullptr; }         // the next step recaptures with (or without) the group's kernels
    wsa_sreg_free(b->sreg);
    b->sreg = n;                                                                       // (a model, an ensemble and a KNN store stay attached)
    return WSA_OK;
}

wsa_status wsa_stream_values(wsa_stream* b, wsa_stream_value_result* out) {
    if (!b || !out) return WSA_ERR_INVALID;
    wsa_ctx* ctx = b->ctx;
    if (!b->sreg) return fail(ctx, WSA_ERR_INVALID, "no regression group attached to these streams (wsa_stream_set_regress)");
    if (!b->stepped) return fail(ctx, WSA_ERR_INVALID, "no step on this stream object yet");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipStreamSynchronize(b->last_stream ? b->last_stream : b->own));
    return wsa_sreg_result(b->sreg, b->h_totals[0], out);
}

wsa_status wsa_stream_ensemble_classes(wsa_stream* b, wsa_stream_ensemble_result* out) {
    if (!b || !out) return WSA_ERR_INVALID;
    wsa_ctx* ctx = b->ctx;
    if (!b->sens) return fail(ctx, WSA_ERR_INVALID, "no ensemble attached to these streams (wsa_stream_set_ensemble)");
    if (!b->stepped) return fail(ctx, WSA_ERR_INVALID, "no step on this stream object yet");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipStreamSynchronize(b->last_stream ? b->last_stream : b->own));
    return wsa_sens_result(b->sens, b->h_totals[0], out);
}

wsa_status wsa_stream_classes(wsa_stream* b, wsa_stream_class_result* out) {
    if (!b || !out) return WSA_ERR_INVALID;
    wsa_ctx* ctx = b->ctx;
    if (!b->scls) return fail(ctx, WSA_ERR_INVALID, "no classifier attached to these streams (wsa_stream_set_model)");
    if (!b->stepped) return fail(ctx, WSA_ERR_INVALID, "no step on this stream object yet");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipStreamSynchronize(b->last_stream ? b->last_stream : b->own));
    return wsa_scls_result(b->scls, b->h_totals[0], out);
}

// Timed steps for the latency figure of BASELINE config 5: step k copies feed[k mod feed_steps] (n_streams x samples_per_step floats,
// the audio "arriving") into the pinned input buffer — outside the timed region — then times wsa_stream_step_host +
// wsa_stream_collect with the host's monotonic clock and notes the microseconds (no interpreter between the two calls).
// `feed` blocks of block_bytes each go into `dst`, the pinned input buffer of the set's format
static wsa_status time_steps_impl(wsa_stream* b, uint32_t n_steps, const void* feed, size_t block_bytes, void* dst, uint32_t feed_steps, void* stream, double* out_us, uint64_t* rows_total) {
    uint64_t rows = 0;
    for (uint32_t k = 0; k < n_steps; k++) {
        if (feed) std::memcpy(dst, static_cast<const uint8_t*>(feed) + (size_t)(k % feed_steps) * block_bytes, block_bytes);
        const auto t0 = std::chrono::steady_clock::now();
        wsa_status st = wsa_stream_step_host(b, nullptr, stream);
        wsa_stream_rows r;
        if (st == WSA_OK) st = wsa_stream_collect(b, stream, &r);
        const auto t1 = std::chrono::steady_clock::now();
        if (st != WSA_OK) return st;
        out_us[k] = std::chrono::duration<double, std::micro>(t1 - t0).count();
        rows += r.n_rows;
    }
    if (rows_total) *rows_total = rows;
    return WSA_OK;
}
wsa_status wsa_stream_time_steps(wsa_stream* b, uint32_t n_steps, const float* feed, uint32_t feed_steps, void* stream, double* out_us, uint64_t* rows_total) {
    if (!b || !out_us || (feed && feed_steps == 0)) return WSA_ERR_INVALID;
    if (feed && b->fmt != WSA_PCM_F32)
        return fail(b->ctx, WSA_ERR_INVALID, std::string("wsa_stream_time_steps with a float feed, this set's input format is ") + pcm_format_name(b->fmt) + ": use wsa_stream_time_steps_packed");
    return time_steps_impl(b, n_steps, feed, (size_t)b->n * b->in_stride * sizeof(float), b->h_pcm, feed_steps, stream, out_us, rows_total);
}
// the same with feed blocks of [n_streams][wsa_stream_input_stride_bytes] bytes in the set's packed format
wsa_status wsa_stream_time_steps_packed(wsa_stream* b, uint32_t n_steps, const void* feed, uint32_t feed_steps, void* stream, double* out_us, uint64_t* rows_total) {
    if (!b || !out_us || (feed && feed_steps == 0)) return WSA_ERR_INVALID;
    if (feed && b->fmt == WSA_PCM_F32)
        return fail(b->ctx, WSA_ERR_INVALID, "wsa_stream_time_steps_packed with a packed feed on a set whose input format is WSA_PCM_F32: use wsa_stream_time_steps");
    return time_steps_impl(b, n_steps, feed, (size_t)b->n * b->pk_stride, b->h_pk, feed_steps, stream, out_us, rows_total);
}

// spec PK-3 on the host: channel `select` of the frames, or their mix
wsa_status wsa_pcm_decode_select(int32_t format, const void* in, uint64_t n_frames, uint32_t channels, uint32_t select, float* out) {
    if (channels < 1 || channels > 64 || (n_frames && (!in || !out)) || !pcm_format_known(format) || !pcm_select_known(select, channels)) return WSA_ERR_INVALID;
    const uint8_t* p = static_cast<const uint8_t*>(in);
    const uint32_t sb = pcm_sample_bytes(format);
    const uint64_t step = (uint64_t)channels * sb;
    for (uint64_t j = 0; j < n_frames; j++) {
        const uint8_t* fr = p + j * step;
        out[j] = select == WSA_CHANNEL_MIX ? pcm_mix_frame(channels, [&](uint32_t c) { return pcm_decode_bytes(format, fr + c * sb); }) : pcm_decode_bytes(format, fr + (uint64_t)select * sb);
    }
    return WSA_OK;
}

// specs PK-1 / PK-2 on the host, no device involved: channel 0 of n_frames interleaved frames -> floats
wsa_status wsa_pcm_decode(int32_t format, const void* in, uint64_t n_frames, uint32_t channels, float* out) {
    if (channels < 1 || channels > 64 || (n_frames && (!in || !out)) || !pcm_format_known(format)) return WSA_ERR_INVALID;
    const uint8_t* p = static_cast<const uint8_t*>(in);
    const uint64_t step = (uint64_t)channels * pcm_sample_bytes(format);
    for (uint64_t j = 0; j < n_frames; j++) out[j] = pcm_decode_bytes(format, p + j * step);
    return WSA_OK;
}

}  // extern "C"
