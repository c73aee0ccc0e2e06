// stream_step.hip — one step of a stream set: the arguments are checked, the step's control words are decided on the host (a mixed set's in integers
// from the per-stream counters), then the step's launches — prologue, pull, K0s or the history shuffle, front end, back end, attached models,
// epilogue — are enqueued, or captured into a hipGraph once and replayed.
#include "stream_internal.hpp"

using namespace wsa;
using wsa_api::fail;

namespace wsa {
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

// ---- what the step entries and the test entry (wsa_stream_step_backend_internal) do alike
// the NULL stream: run on the object's own stream, after what the NULL stream holds now
static wsa_status own_stream_for_null(wsa_stream* b, hipStream_t* stream) {
    wsa_ctx* ctx = b->ctx;
    if (*stream) return WSA_OK;
    HIP_TRY(ctx, hipEventRecord(b->ev_in, nullptr));
    hipStream_t s = b->own;
    HIP_TRY(ctx, hipStreamWaitEvent(s, b->ev_in, 0));
    *stream = s;
    return WSA_OK;
}
// the pinned control words are read by the step's prologue: the previous step must be done, on whichever stream it ran
static wsa_status await_previous_step(wsa_stream* b, hipStream_t s) {
    wsa_ctx* ctx = b->ctx;
    if (b->stepped) HIP_TRY(ctx, hipStreamSynchronize(b->last_stream ? b->last_stream : s));
    b->last_stream = s;
    return WSA_OK;
}
// FD-2, behind await_previous_step: an attached feature DB reads the previous step's outcome if no collect did, and its count goes to the step about to
// be launched through a mapped pinned word, like the control words
static void hand_count_to_step(wsa_stream* b) { if (b->sfdb) wsa_sfdb_begin_step(b->sfdb); }
// a stream's control byte (WSA_STREAM_*) -> the device control word's bits: 1 START, 2 STOP, 4 active in this step
static uint32_t ctl_bits(uint32_t cb) { return (cb & WSA_STREAM_START ? 1u : 0u) | (cb & WSA_STREAM_STOP ? 2u : 0u) | (cb & WSA_STREAM_ACTIVE ? 4u : 0u); }
// the control words to the device, counters cleared; then the streams' carried state reset where START says so
// (no memcpy / memset nodes: everything that crosses PCIe goes through mapped pinned buffers, moved by kernels)
static void enqueue_prologue(wsa_stream* b, hipStream_t s) {
    const BackEnd& B = b->be;
    const uint32_t n = b->n, cw = b->ctl_words * n;
    hipLaunchKernelGGL(stream_begin_kernel, dim3((cw + 255) / 256), dim3(256), 0, s, b->d_ctl, b->h_ctl_dev, cw, B.d_counters, B.d_totals,
                       B.d_trk_seg, B.d_trk_seg ? (uint32_t)((size_t)n * B.seg_cap * 4) : 0u);
}
static void enqueue_prepare(wsa_stream* b, hipStream_t s) {
    launch_stream_prepare(b->d_state, b->d_carry, b->d_tr_state, b->d_ctl + 2 * b->n, b->n, b->D.ctx_max0, b->D.floor0, s);
}

// One step in two halves, enqueued one after the other (this is what the graph holds).
// The input half: prologue, the step's samples (pull / stage / K0s) and the front end; it leaves the step's u32 frames in d_spec.
static void enqueue_input(wsa_stream* b, const float* d_pcm, uint64_t stride, bool host_in, hipStream_t s) {
    const FePlanHost& P = b->fe.plan;
    const uint32_t n = b->n;
    enqueue_prologue(b, s);
    wsa_api::launch_stream_pull(b, &d_pcm, &stride, host_in, s);
    enqueue_prepare(b, s);
    if (b->mixed) {                        // K0s in the place of the history shuffle: carried converted samples to the front, this step's outputs behind them
        RsStreamParams r;
        r.stage = b->d_stage; r.stage_stride = b->stage_stride; r.conv = b->d_conv; r.conv_stride = b->conv_stride; r.in = d_pcm; r.in_stride = stride;
        r.hist = b->d_hist; r.ctl = b->d_ctl; r.n = n; r.tables = b->d_rs_tables; r.cls = b->d_rs_cls; r.stream_class = b->d_rs_class; r.xcap = b->xcap;
        launch_resample_stream(r, s);
        d_pcm = b->d_stage; stride = b->stage_stride;
    } else if (b->hist) {
        wsa_api::launch_stream_stage(b, d_pcm, stride, s);
        d_pcm = b->d_stage; stride = b->stage_stride;
    }
    FeParams p;
    b->fe.fill(p, b->tune.fe_fat);
    p.pcm = d_pcm; p.clip_stride = stride; p.n_frames = b->d_ctl; p.frame_off = b->d_frame_off; p.spec = b->d_spec; p.pcm_off = b->d_ctl + n;
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
    // the attached models.  K6 on the step's rows, then (level 13) the fold carried per stream; both push their tables themselves
    if (b->scls) if (const wsa_status st = wsa_scls_enqueue(b->scls, s); st != WSA_OK) return st;
    // K6e, the (stream, member) folds and the decision
    if (b->sens) if (const wsa_status st = wsa_sens_enqueue(b->sens, s); st != WSA_OK) return st;
    // K9s (partial, merge), then the push / KN-2 fold kernel
    if (b->sknn) if (const wsa_status st = wsa_sknn_enqueue(b->sknn, s); st != WSA_OK) return st;
    // the grouped K6 over the regression heads, then the push / RG-1 fold kernel
    if (b->sreg) if (const wsa_status st = wsa_sreg_enqueue(b->sreg, s); st != WSA_OK) return st;
    // FD-2: the plan and the copy kernel that append the step's rows to the attached feature DB
    if (b->sfdb) if (const wsa_status st = wsa_sfdb_enqueue(b->sfdb, s); st != WSA_OK) return st;
    hipLaunchKernelGGL(stream_push_kernel, dim3(16), dim3(256), 0, s, b->be.d_totals, b->be.d_counters, b->be.d_meta, b->be.d_feat, b->be.d_seg,
                       b->h_totals_dev, b->h_meta_dev, b->h_feat_dev, b->h_seg_dev, b->d2h_rows, b->d2h_segs, b->d_state, b->n);
    HIP_TRY(ctx, hipGetLastError());
    return WSA_OK;
}
static wsa_status enqueue_step(wsa_stream* b, const float* d_pcm, uint64_t stride, bool host_in, hipStream_t s) {
    enqueue_input(b, d_pcm, stride, host_in, s);
    return enqueue_backend(b, s);
}

// ---- step_impl's named steps
// a stream's control byte: the caller's, or ACTIVE with START on the set's first step
static uint32_t step_ctl(const wsa_stream* b, const uint8_t* ctl, uint32_t i) {
    return ctl ? ctl[i] : (b->steps == 0 ? (WSA_STREAM_ACTIVE | WSA_STREAM_START) : WSA_STREAM_ACTIVE);
}

// every refusal that needs no counter: pointers, strides and counts — nothing is counted and no stream awaited before these pass
static wsa_status check_step_args(wsa_stream* b, const float* d_pcm, uint64_t stride, bool host_in, const uint32_t* n_in, const uint8_t* ctl) {
    wsa_ctx* ctx = b->ctx;
    if (!host_in && !d_pcm) return fail(ctx, WSA_ERR_INVALID, "null PCM pointer");
    const bool packed = b->fmt != WSA_PCM_F32;
    if (packed && !host_in) {              // device-resident packed input: rows are read in whole 16-byte chunks
        if (stride % 16 != 0) return fail(ctx, WSA_ERR_INVALID, "stream_stride_bytes " + std::to_string(stride) + " is not a multiple of 16");
        if (reinterpret_cast<uintptr_t>(d_pcm) % 16 != 0) return fail(ctx, WSA_ERR_INVALID, "the packed input pointer is not aligned to 16 bytes");
    }
    if (!packed && !b->mixed && !host_in && stride < b->step_samples && b->n > 1) return fail(ctx, WSA_ERR_INVALID, "stream_stride smaller than samples_per_step");
    for (uint32_t i = 0; n_in && i < b->n; i++) {           // counts are checked before anything is counted
        if (!(step_ctl(b, ctl, i) & WSA_STREAM_ACTIVE)) continue;
        if (!b->mixed && n_in[i] != b->step_samples)
            return fail(ctx, WSA_ERR_INVALID, "stream " + std::to_string(i) + ": a plain stream set takes exactly " + std::to_string(b->step_samples) + " samples per step, not " + std::to_string(n_in[i]));
        if (b->mixed && n_in[i] > b->in_cap[i])
            return fail(ctx, WSA_ERR_INVALID, "stream " + std::to_string(i) + ": " + std::to_string(n_in[i]) + " samples in one step, its capacity is " + std::to_string(b->in_cap[i]));
        if (!packed && b->mixed && !host_in && b->n > 1 && stride < n_in[i]) return fail(ctx, WSA_ERR_INVALID, "stream_stride smaller than the samples of stream " + std::to_string(i));
    }
    for (uint32_t i = 0; packed && !host_in && i < b->n; i++) {        // the largest row any active stream can have in this step fits the stride
        if (!(step_ctl(b, ctl, i) & WSA_STREAM_ACTIVE)) continue;
        const uint64_t cnt = n_in ? n_in[i] : (b->mixed ? b->in_cap[i] : b->step_samples);
        const uint64_t need = cnt * b->chan[i] * pcm_sample_bytes(b->fmt);
        if (need > stride)
            return fail(ctx, WSA_ERR_INVALID, "stream_stride_bytes " + std::to_string(stride) + " too small: stream " + std::to_string(i) + " carries " + std::to_string(cnt) + " frames of "
                        + std::to_string(b->chan[i]) + " channels, " + std::to_string(need) + " bytes");
    }
    for (uint32_t i = 0; !packed && b->mixed && !n_in && !host_in && b->n > 1 && i < b->n; i++)      // paced: no count exceeds the capacity
        if (stride < b->in_cap[i]) return fail(ctx, WSA_ERR_INVALID, "stream_stride smaller than the input capacity of stream " + std::to_string(i));
    return WSA_OK;
}

// A mixed set's step: every count is decided here, in integers and one exact predicate in double (resample_ready), from the per-stream counters; the
// device only carries them out.  Writes the streams' control words and moves the counters; no HIP call.
static wsa_status plan_mixed_step(wsa_stream* b, const uint32_t* n_in, const uint8_t* ctl) {
    const uint32_t n = b->n, hop = (uint32_t)b->fe.plan.hop, win = (uint32_t)b->fe.plan.win;
    for (uint32_t i = 0; i < n; i++) {
        const uint32_t cb = step_ctl(b, ctl, i);
        uint32_t* w = b->h_ctl + i;
        if (cb & WSA_STREAM_START) { b->cN[i] = b->cY[i] = b->cK[i] = b->cS[i] = 0; b->last_nfr[i] = 0; }
        b->last_out[i] = 0;
        w[RS_CTL_NFR * n] = 0; w[RS_CTL_OFF * n] = 0; w[RS_CTL_NIN * n] = 0; w[RS_CTL_NOUT * n] = 0;
        if (cb & WSA_STREAM_ACTIVE) {
            const uint32_t cnt = n_in ? n_in[i] : b->paced_count(i, b->cS[i]);
            const uint64_t N0 = b->cN[i], Y0 = b->cY[i], K0 = b->cK[i], N1 = N0 + cnt;
            uint64_t Y1 = (cb & WSA_STREAM_STOP) ? resample_length(N1, b->fs_in[i], b->fs) : resample_ready(N1, b->fs_in[i], b->fs);
            if (b->fs_in[i] == b->fs) Y1 = N1;
            if (Y1 < Y0) Y1 = Y0;                          // (active again after a STOP without a START: nothing is taken back)
            const uint64_t K1 = Y1 >= win ? (Y1 - win) / hop + 1 : 0;
            const int64_t in0 = (int64_t)N0 - RS_HIST, dst0 = (int64_t)Y0 - (int64_t)(K0 * hop);
            const bool conv = b->fs_in[i] != b->fs && Y1 > Y0;
            if (Y1 - Y0 > b->out_cap || K1 < K0 || K1 - K0 > b->F || dst0 + (int64_t)(Y1 - Y0) > (int64_t)b->stage_stride || dst0 < -(int64_t)hop || (conv && (int64_t)std::floor((double)Y0 * b->ratio[i]) - RS_TAPS / 2 < in0)
                || (conv && (int64_t)std::floor((double)(Y1 - 1) * b->ratio[i]) + RS_TAPS / 2 - in0 > (int64_t)b->xcap))
                return fail(b->ctx, WSA_ERR_CAPACITY, "stream " + std::to_string(i) + ": a step outside the derived bounds (" + std::to_string(Y1 - Y0) + " outputs, "
                            + std::to_string(K1 - K0) + " frames; capacity " + std::to_string(b->out_cap) + ", " + std::to_string(b->F) + ")");
            w[RS_CTL_NFR * n] = (uint32_t)(K1 - K0); w[RS_CTL_NIN * n] = cnt; w[RS_CTL_NOUT * n] = (uint32_t)(Y1 - Y0);
            w[RS_CTL_DST * n] = (uint32_t)(int32_t)dst0; w[RS_CTL_SHIFT * n] = b->last_nfr[i] * hop; w[RS_CTL_CARRY * n] = dst0 > 0 ? (uint32_t)dst0 : 0u;
            w[RS_CTL_Y_LO * n] = (uint32_t)Y0; w[RS_CTL_Y_HI * n] = (uint32_t)(Y0 >> 32);
            w[RS_CTL_IN0_LO * n] = (uint32_t)(uint64_t)in0; w[RS_CTL_IN0_HI * n] = (uint32_t)((uint64_t)in0 >> 32);
            b->cN[i] = N1; b->cY[i] = Y1; b->cK[i] = K1; b->cS[i]++;
            b->last_nfr[i] = (uint32_t)(K1 - K0); b->last_out[i] = (uint32_t)(Y1 - Y0);
        }
        w[RS_CTL_BITS * n] = ctl_bits(cb);
    }
    return WSA_OK;
}

// A plain set's step: whole frames, the first q - 1 after START skipped (their windows reach before time zero)
static void plan_plain_step(wsa_stream* b, const uint8_t* ctl) {
    const uint32_t n = b->n, F = b->F;
    for (uint32_t i = 0; i < n; i++) {
        const uint32_t cb = step_ctl(b, ctl, i);
        uint32_t nfr = 0, off = 0;
        if (cb & WSA_STREAM_START) b->warm[i] = b->q - 1;
        if (cb & WSA_STREAM_ACTIVE) {
            const uint32_t skip = b->warm[i] < F ? b->warm[i] : F;
            b->warm[i] -= skip; nfr = F - skip; off = skip * (uint32_t)b->fe.plan.hop;
        }
        b->h_ctl[i] = nfr; b->h_ctl[n + i] = off; b->h_ctl[2 * n + i] = ctl_bits(cb);
    }
}

// the step as one graph launch: captured on its first use and whenever what the graph holds (input pointer, stride, stream, format) has changed
static wsa_status launch_step_graph(wsa_stream* b, const float* d_pcm, uint64_t stride, bool host_in, hipStream_t s) {
    wsa_ctx* ctx = b->ctx;
    if (b->gexec && (b->g_pcm != d_pcm || b->g_stride != stride || b->g_stream != s || b->g_host != host_in || b->g_fmt != b->fmt)) b->drop_graph();
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
    return WSA_OK;
}

static wsa_status step_impl(wsa_stream* b, const float* d_pcm, uint64_t stride, bool host_in, const uint32_t* n_in, const uint8_t* ctl, hipStream_t s) {
    wsa_ctx* ctx = b->ctx;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (const wsa_status st = own_stream_for_null(b, &s); st != WSA_OK) return st;
    if (const wsa_status st = check_step_args(b, d_pcm, stride, host_in, n_in, ctl); st != WSA_OK) return st;
    if (const wsa_status st = await_previous_step(b, s); st != WSA_OK) return st;
    hand_count_to_step(b);
    if (b->mixed) {
        if (const wsa_status st = plan_mixed_step(b, n_in, ctl); st != WSA_OK) {
            if (b->sfdb) (void)wsa_sfdb_settle(b->sfdb);      // nothing was launched: the attached DB has no outcome to wait for
            return st;
        }
    }
    else plan_plain_step(b, ctl);
    const wsa_status st = b->graph_on && b->steps >= 1 ? launch_step_graph(b, d_pcm, stride, host_in, s) : enqueue_step(b, d_pcm, stride, host_in, s);
    if (st != WSA_OK) return st;
    b->steps++; b->stepped = true;
    return WSA_OK;
}

static wsa_status refuse_float_entry(wsa_stream* b, const char* name) {
    return fail(b->ctx, WSA_ERR_INVALID, std::string(name) + " takes floats, this set's input format is " + pcm_format_name(b->fmt)
                + ": use wsa_stream_step_packed, or wsa_stream_set_input_format(WSA_PCM_F32)");
}

extern "C" {

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
    if (const wsa_status st = own_stream_for_null(b, &s); st != WSA_OK) return st;
    if (const wsa_status st = await_previous_step(b, s); st != WSA_OK) return st;
    hand_count_to_step(b);
    for (uint32_t i = 0; i < n; i++) { b->h_ctl[i] = (ctl[i] & WSA_STREAM_ACTIVE) ? n_frames[i] : 0u; b->h_ctl[n + i] = 0; b->h_ctl[2 * n + i] = ctl_bits(ctl[i]); }
    // (the copy is ordered behind the previous step by the synchronize above, the launches below behind the copy by the stream)
    HIP_TRY(ctx, hipMemcpyAsync(b->d_spec, frames, (size_t)n * F * own_bands * sizeof(uint32_t), hipMemcpyHostToDevice, s));
    enqueue_prologue(b, s);
    enqueue_prepare(b, s);
    if (const wsa_status st = enqueue_backend(b, s); st != WSA_OK) return st;
    b->steps++; b->stepped = true;
    return WSA_OK;
}

}  // extern "C"
