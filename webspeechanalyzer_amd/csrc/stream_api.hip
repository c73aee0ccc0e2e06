// stream_api.hip — the wsa_stream_* part of include/wsa.h: n_streams concurrent launches that advance
// in lock step, one hipGraph launch per step.  Here: the set is planned and destroyed, its getters, the converted samples, the timed steps.
// (Input formats and the pull kernels: stream_input.hip; the step: stream_step.hip; results and attached models: stream_collect.hip.)
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
#include <chrono>
#include "stream_internal.hpp"

using namespace wsa;
using wsa_api::fail;

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
    wsa_sfdb_free(b->sfdb);
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
const uint32_t* wsa_stream_ctl_internal(wsa_stream* b, wsa_ctx** ctx, uint32_t* n_streams, int* mixed) {
    *ctx = b->ctx; *n_streams = b->n; *mixed = b->mixed ? 1 : 0;
    return b->d_ctl;
}

uint32_t wsa_stream_samples_per_step(const wsa_stream* b) { return b ? b->step_samples : 0; }
uint32_t wsa_stream_input_capacity(const wsa_stream* b, uint32_t i) { return !b || i >= b->n ? 0 : (b->mixed ? b->in_cap[i] : b->step_samples); }
uint32_t wsa_stream_input_stride(const wsa_stream* b) { return b ? b->in_stride : 0; }
uint32_t wsa_stream_step_frame_capacity(const wsa_stream* b) { return b ? b->F : 0; }
uint32_t wsa_stream_paced_input(const wsa_stream* b, uint32_t i) { return !b || i >= b->n ? 0 : (b->mixed ? b->paced_count(i, b->cS[i]) : b->step_samples); }
uint32_t wsa_stream_frames_bound(uint32_t frames_per_step, uint32_t hop, double min_ratio) { return resample_step_frames_bound(frames_per_step, hop, min_ratio); }
float* wsa_stream_host_input(wsa_stream* b) { return b ? b->h_pcm : nullptr; }
void* wsa_stream_host_input_packed(wsa_stream* b) { return b && b->fmt != WSA_PCM_F32 ? b->h_pk : nullptr; }
uint32_t wsa_stream_input_stride_bytes(const wsa_stream* b) { return !b ? 0 : (b->fmt != WSA_PCM_F32 ? b->pk_stride : b->in_stride * (uint32_t)sizeof(float)); }

wsa_status wsa_stream_enable_graph(wsa_stream* b, int32_t on) {
    if (!b) return WSA_ERR_INVALID;
    b->graph_on = on != 0;
    if (!on) b->drop_graph();
    return WSA_OK;
}

wsa_status wsa_stream_copy_converted(wsa_stream* b, float* out, uint32_t cap, uint32_t* counts) {
    if (!b) return WSA_ERR_INVALID;
    wsa_ctx* ctx = b->ctx;
    if (!b->mixed) return fail(ctx, WSA_ERR_INVALID, "no converted samples: the stream set must come from wsa_stream_create_mixed");
    if (!b->stepped) return wsa_api::no_step_yet(b);
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

}  // extern "C"
