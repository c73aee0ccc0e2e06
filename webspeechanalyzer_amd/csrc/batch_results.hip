// batch_results.hip — what a run left behind, handed to the caller: the device result table (wsa_batch_result), the copies into host tables
// (wsa_batch_copy_*), level 3's raw tracks, the per-frame trace, the stage timings and the run's small switches.
#include <initializer_list>
#include "batch_internal.hpp"

using namespace wsa;
using wsa_api::fail;
using wsa_api::fetch_totals;

// the tail of a wsa_batch_copy_* entry: every table the caller gave a buffer for and that holds something is queued on s, then s is synchronised
struct CopyOut { void* dst; const void* src; size_t bytes; };
static wsa_status copy_out(wsa_batch* b, hipStream_t s, std::initializer_list<CopyOut> tables) {
    wsa_ctx* ctx = b->ctx;
    for (const CopyOut& t : tables) if (t.dst && t.bytes) HIP_TRY(ctx, hipMemcpyAsync(t.dst, t.src, t.bytes, hipMemcpyDefault, s));
    HIP_TRY(ctx, hipStreamSynchronize(s));
    return WSA_OK;
}

// ---- level 3: the ranked raw tracks of every segment (ref @B28273 `s.push(i)`, dispatched at @B30132)
static wsa_status fetch_track_tables(wsa_batch* b, hipStream_t s) {
    wsa_ctx* ctx = b->ctx;
    if (!b->be.d_trk_seg) return fail(ctx, WSA_ERR_INVALID, "no raw tracks: output_level must be 3");
    if (const wsa_status st = fetch_totals(b, s); st != WSA_OK) return st;
    b->h_trk_seg.resize((size_t)b->n_clips * b->be.seg_cap * 4); b->h_seg_count.resize(b->n_clips);
    if (b->n_clips) {
        HIP_TRY(ctx, hipMemcpyAsync(b->h_trk_seg.data(), b->be.d_trk_seg, b->h_trk_seg.size() * sizeof(int32_t), hipMemcpyDefault, s));
        HIP_TRY(ctx, hipMemcpyAsync(b->h_seg_count.data(), b->be.d_seg_count, b->h_seg_count.size() * sizeof(uint32_t), hipMemcpyDefault, s));
        HIP_TRY(ctx, hipStreamSynchronize(s));
    }
    return WSA_OK;
}

static void batch_track_list(wsa_batch* b) {          // the segments in hand-out order: (clip, k); the batch's pool is one region
    b->trk.begin();
    for (uint32_t c = 0; c < b->n_clips; c++)
        for (uint32_t k = 0; k < b->h_seg_count[c]; k++) b->trk.add(&b->h_trk_seg[((size_t)c * b->be.seg_cap + k) * 4], 0);
}

extern "C" {

wsa_status wsa_batch_result(wsa_batch* b, void* stream, wsa_device_result* o) {
    if (!b || !o) return WSA_ERR_INVALID;
    const wsa_status st = fetch_totals(b, reinterpret_cast<hipStream_t>(stream));
    o->n_clips = b->n_clips; o->n_rows = b->res_rows; o->n_segments = b->res_segs; o->n_frames_total = b->total_frames;
    o->status_flags = b->res_flags;
    o->d_row_meta = b->be.d_meta; o->d_row_feat = b->be.d_feat; o->d_segments = b->be.d_seg; o->d_clip_row_off = b->be.d_row_off; o->d_clip_seg_off = b->be.d_seg_off;
    o->d_spectra = b->spec_in_use; o->d_clip_frame_off = b->d_frame_off; o->d_formants = b->be.d_formants;
    o->n_utterance_rows = b->be.d_utt_feat ? b->res_utt : 0; o->d_utt_meta = b->be.d_utt_meta; o->d_utt_feat = b->be.d_utt_feat; o->d_clip_utt_off = b->be.d_utt_off;
    return st;
}

wsa_status wsa_batch_copy_rows(wsa_batch* b, void* stream, int32_t* row_meta, double* row_feat, uint32_t rows_cap,
                               int32_t* segments, uint32_t seg_cap, uint32_t* clip_row_off, uint32_t* clip_seg_off) {
    if (!b) return WSA_ERR_INVALID;
    wsa_ctx* ctx = b->ctx;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (const wsa_status st = fetch_totals(b, s); st != WSA_OK) return st;
    if ((row_meta || row_feat) && rows_cap < b->res_rows) return fail(ctx, WSA_ERR_INVALID, "row buffer too small");
    if (segments && seg_cap < b->res_segs) return fail(ctx, WSA_ERR_INVALID, "segment buffer too small");
    const size_t offsets = ((size_t)b->n_clips + 1) * sizeof(uint32_t);
    return copy_out(b, s, {{row_meta, b->be.d_meta, (size_t)b->res_rows * 8 * sizeof(int32_t)}, {row_feat, b->be.d_feat, (size_t)b->res_rows * WSA_NFEAT * sizeof(double)},
                           {segments, b->be.d_seg, (size_t)b->res_segs * 4 * sizeof(int32_t)}, {clip_row_off, b->be.d_row_off, offsets}, {clip_seg_off, b->be.d_seg_off, offsets}});
}

// (the frames come without a fetch of the counters, and the offsets from the host's plan)
wsa_status wsa_batch_copy_spectra(wsa_batch* b, void* stream, uint32_t* spectra, uint64_t cap_words, uint32_t* clip_frame_off) {
    if (!b) return WSA_ERR_INVALID;
    wsa_ctx* ctx = b->ctx;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (!b->ran) return wsa_api::no_run_yet(b);
    if (spectra && !b->spec_in_use) return fail(ctx, WSA_ERR_INVALID, "the u32 frames of this run were not stored: call wsa_batch_keep_spectra(batch, 1) before the run");
    const uint64_t words = (uint64_t)b->total_frames * (uint32_t)b->fe.plan.bands;
    if (spectra && cap_words < words) return fail(ctx, WSA_ERR_INVALID, "spectra buffer too small");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (spectra && words) HIP_TRY(ctx, hipMemcpyAsync(spectra, b->spec_in_use, words * sizeof(uint32_t), hipMemcpyDefault, s));
    if (clip_frame_off) std::memcpy(clip_frame_off, b->frame_off.data(), ((size_t)b->n_clips + 1) * sizeof(uint32_t));
    HIP_TRY(ctx, hipStreamSynchronize(s));
    return WSA_OK;
}

wsa_status wsa_batch_copy_utterance(wsa_batch* b, void* stream, int32_t* utt_meta, double* utt_feat, uint32_t cap_rows, uint32_t* clip_utt_off) {
    if (!b) return WSA_ERR_INVALID;
    wsa_ctx* ctx = b->ctx;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (!b->be.d_utt_feat) return fail(ctx, WSA_ERR_INVALID, "no utterance features: output_level must be 11");
    if (const wsa_status st = fetch_totals(b, s); st != WSA_OK) return st;
    if ((utt_meta || utt_feat) && cap_rows < b->res_utt) return fail(ctx, WSA_ERR_INVALID, "utterance buffer too small");
    return copy_out(b, s, {{utt_meta, b->be.d_utt_meta, (size_t)b->res_utt * 4 * sizeof(int32_t)}, {utt_feat, b->be.d_utt_feat, (size_t)b->res_utt * WSA_NUTT * sizeof(double)},
                           {clip_utt_off, b->be.d_utt_off, ((size_t)b->n_clips + 1) * sizeof(uint32_t)}});
}

wsa_status wsa_batch_copy_formants(wsa_batch* b, void* stream, float* formants, uint64_t cap_frames) {
    if (!b || !formants) return WSA_ERR_INVALID;
    wsa_ctx* ctx = b->ctx;
    if (!b->ran || !b->be.d_formants) return fail(ctx, WSA_ERR_INVALID, "no formant frames: output_level must be 4, 10, 11 or 12 and the batch must have run");
    if (cap_frames < b->total_frames) return fail(ctx, WSA_ERR_INVALID, "formant buffer too small");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    return copy_out(b, reinterpret_cast<hipStream_t>(stream), {{formants, b->be.d_formants, (size_t)b->total_frames * 9 * sizeof(float)}});
}

wsa_status wsa_batch_tracks_info(wsa_batch* b, void* stream, wsa_tracks_info* out) {
    if (!b || !out) return WSA_ERR_INVALID;
    if (const wsa_status st = fetch_track_tables(b, reinterpret_cast<hipStream_t>(stream)); st != WSA_OK) return st;
    batch_track_list(b);
    out->n_segments = b->trk.segments(); out->n_points = b->trk.n_points; out->n_ranked = b->trk.n_ranked;
    return WSA_OK;
}

wsa_status wsa_batch_copy_tracks(wsa_batch* b, void* stream, uint64_t* seg_off, int32_t* points, uint64_t cap_points, int32_t* ranked, uint64_t cap_ranked) {
    if (!b || !seg_off || !points || !ranked) return WSA_ERR_INVALID;
    wsa_ctx* ctx = b->ctx;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (const wsa_status st = fetch_track_tables(b, s); st != WSA_OK) return st;
    TrackGather& G = b->trk;
    batch_track_list(b);
    if (G.n_points > cap_points || G.n_ranked > cap_ranked) return fail(ctx, WSA_ERR_INVALID, "track buffers too small");
    G.offsets(seg_off);
    if (const wsa_status gs = G.run(ctx, 1ull << 63, b->be.d_trk_pts, b->be.d_trk_rank, points, ranked, s); gs != WSA_OK) return gs;
    HIP_TRY(ctx, hipStreamSynchronize(s));
    return WSA_OK;
}

// (a copy per clip: the caller's stride is not the batch's)
wsa_status wsa_batch_copy_pcm(wsa_batch* b, void* stream, float* pcm, uint64_t stride) {
    if (!b || !pcm) return WSA_ERR_INVALID;
    wsa_ctx* ctx = b->ctx;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (!b->rs_on || !b->ran) return fail(ctx, WSA_ERR_INVALID, "no converted PCM: the batch must come from wsa_batch_create_resampled / wsa_batch_create_mixed and must have run");
    if (stride < b->max_samples) return fail(ctx, WSA_ERR_INVALID, "stride smaller than the longest converted clip");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    for (uint32_t i = 0; i < b->n_clips; i++)
        if (b->n_samples[i]) HIP_TRY(ctx, hipMemcpyAsync(pcm + (size_t)i * stride, b->d_rs_pcm + (size_t)i * b->rs_stride, (size_t)b->n_samples[i] * sizeof(float), hipMemcpyDefault, s));
    HIP_TRY(ctx, hipStreamSynchronize(s));
    return WSA_OK;
}

wsa_status wsa_batch_stage_ms(wsa_batch* b, float out[4]) {
    if (!b || !out) return WSA_ERR_INVALID;
    wsa_ctx* ctx = b->ctx;
    if (!b->ran || !b->timing) return fail(ctx, WSA_ERR_INVALID, "no timed run on this batch");
    HIP_TRY(ctx, hipEventSynchronize(b->ev[4]));
    for (int i = 0; i < 4; i++) HIP_TRY(ctx, hipEventElapsedTime(&out[i], b->ev[i], b->ev[i + 1]));
    return WSA_OK;
}

wsa_status wsa_batch_enable_trace(wsa_batch* b, int32_t on) {
    if (!b) return WSA_ERR_INVALID;
    if (on && !b->d_trace) {
        HIP_TRY(b->ctx, hipSetDevice(b->ctx->device));
        const size_t rows = b->total_frames ? b->total_frames : 1;      // an empty batch still gets a valid (unused) buffer
        if (!b->mem.alloc(&b->d_trace, rows * 12)) return fail(b->ctx, WSA_ERR_HIP, "trace allocation failed");
        HIP_TRY(b->ctx, hipMemset(b->d_trace, 0, rows * 12 * sizeof(double)));
    }
    if (!on) b->d_trace = nullptr;       // the allocation stays owned by the batch
    return WSA_OK;
}

wsa_status wsa_batch_copy_trace(wsa_batch* b, void* stream, double* out, uint64_t cap_rows) {
    if (!b || !out) return WSA_ERR_INVALID;
    wsa_ctx* ctx = b->ctx;
    if (!b->d_trace || !b->ran) return fail(ctx, WSA_ERR_INVALID, "trace not enabled or no run yet");
    if (cap_rows < b->total_frames) return fail(ctx, WSA_ERR_INVALID, "trace buffer too small");
    return copy_out(b, reinterpret_cast<hipStream_t>(stream), {{out, b->d_trace, (size_t)b->total_frames * 12 * sizeof(double)}});
}

wsa_status wsa_batch_keep_spectra(wsa_batch* b, int32_t on) {
    if (!b) return WSA_ERR_INVALID;
    (void)on;                                          // the front end hands the u32 frames to the peak scan through the array: they are always there
    return WSA_OK;
}

wsa_status wsa_batch_backend_reruns(const wsa_batch* b, uint32_t* out) {
    if (!b || !out) return WSA_ERR_INVALID;
    *out = b->reruns;
    return WSA_OK;
}

wsa_status wsa_batch_enable_timing(wsa_batch* b, int32_t on) {
    if (!b) return WSA_ERR_INVALID;
    b->timing = on != 0;
    return WSA_OK;
}

}  // extern "C"
