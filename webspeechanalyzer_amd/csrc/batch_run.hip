// batch_run.hip — one run of a planned batch: the stage launches in order (clear, K0, front end, peak scan, gate, span order, tracker, compaction, the
// level's tail kernel, publish), the counters' fetch with its rerun on a tracker-table overflow, and the accessors the other sources reach a batch through.
#include <algorithm>
#include "batch_internal.hpp"

using namespace wsa;
using wsa_api::fail;

namespace wsa {
// run epilogue: the four result counters go to the batch's mapped pinned words, so that the host reads them behind a stream synchronize.  (Three
// 4-byte hipMemcpyAsync D2H were three blit-kernel dispatches: behind the other batches' kernels each waited 50 - 300 us for a free slot on a full
// GPU, ~430 us per step before the host heard that the batch was done — with three batches in flight the step was bound by that round trip.)
__global__ void batch_publish_kernel(const uint32_t* totals, const uint32_t* counters, uint32_t* host) {
    if (threadIdx.x == 0) {
        host[0] = totals[0]; host[1] = totals[1]; host[2] = counters[1]; host[3] = totals[3];
        __threadfence_system();
    }
}
// run prologue: work-queue counters and totals back to zero.  A kernel, not hipMemsetAsync: memset / memcpy nodes of a
// captured graph did not replay reliably on ROCm 7.2 / gfx950 (see stream_step.hip), a kernel node does.
__global__ void batch_clear_kernel(uint32_t* counters, uint32_t* totals, uint32_t* span_hist) {
    if (threadIdx.x < 16) counters[threadIdx.x] = 0;
    if (threadIdx.x < 4) totals[threadIdx.x] = 0;
    if (span_hist) for (int b = threadIdx.x; b < SPAN_BUCKETS; b += blockDim.x) span_hist[b] = 0;
}
}  // namespace wsa

static wsa_status run_backend_stages(wsa_batch* b, const uint32_t* d_spec, bool skip_peaks, hipStream_t s) {
    wsa_ctx* ctx = b->ctx;
    const Derived& D = b->D;
    const BackEnd& B = b->be;
    b->published = false;
    if (D.level <= 2) return WSA_OK;
    const int dbg = b->tune.dbg;
    uint32_t* counters = B.d_counters + 4;              // [0] largest per-clip segment count
    PkParams pk; pk.spec = d_spec; pk.rec = B.rec; pk.total_frames = b->total_frames; pk.bands = b->fe.plan.bands;
    pk.flags = B.d_counters + 1; pk.dbg = (b->tune.dbg >> DBG_PEAKS_SHIFT) & 0xff; pk.lanes_only = b->tune.peaks_lanes ? 1 : 0;      // (WSA_DBG bits 20 .. 27: the peak scan's what-if switches, TUNING=1 builds only)
    pk.wpc = b->tune.peaks_wpc; pk.round_bins = b->tune.peaks_w;
    if (!skip_peaks) launch_peaks(pk, s);         // (a rerun of the back end finds the frame records in place)
    GateParams g;
    B.fill(g, D);
    g.n_frames = b->d_n_frames; g.frame_off = b->d_frame_off; g.trace = b->d_trace; g.dbg = dbg; g.prio = 1;
    const bool ordered = !(dbg & DBG_UNSORTED_SPANS);            // (clip, segment) enumeration instead of the length-sorted order
    g.span_hist = ordered ? b->d_span_hist : nullptr; g.span_key = b->d_span_key;
    launch_gate(g, s);
    TrParams t;
    B.fill(t, D);
    t.frame_off = b->d_frame_off; t.trace = b->d_trace; t.dbg = dbg;
    t.order = ordered ? b->d_order : nullptr; t.redo = b->d_redo; t.redo_count = counters + 2;
    t.fin_waves = b->tune.fin_wpc >= 1 && b->tune.fin_wpc <= 32 ? ctx->n_cu * b->tune.fin_wpc : 0;
    // four spans per wave where the batch has spans enough to keep every wave slot busy that way (the 12 500-clip shard: -5 % per step); a 1024-clip batch
    // has ~6 000 spans = 1 500 such waves on 4 096 slots, and the longer waves cost more than the instructions they save (WSA_QUAD=1 / WSA_NO_QUAD=1 force it)
    t.quad = b->split && !b->tune.no_quad && (b->tune.quad || b->total_frames >= 1200000u) ? 1 : 0;
    t.quad_waves = (int)std::min<size_t>((size_t)b->n_waves, ((size_t)b->n_clips * (size_t)B.seg_cap + 3) / 4 + 1);
    t.pool = b->split ? b->d_pool : nullptr; t.pool_bpf = (uint32_t)b->pool_bpf; t.span_hdr = b->split ? b->d_span_hdr : nullptr;
    if (t.order) launch_span_order(t, b->d_span_hist, b->d_span_key, b->d_order, counters, s);
    if (b->timing) HIP_TRY(ctx, hipEventRecord(b->ev[2], s));          // stage 1 = peak scan + gate + span order, stage 2 = tracker
    launch_tracker(t, b->n_waves, b->full_table, b->pair, s);
    if (b->timing) HIP_TRY(ctx, hipEventRecord(b->ev[3], s));
    CompactParams cp;
    B.fill(cp, D);
    // levels 11 / 12 run a kernel behind the compaction that adds to the result counters: they keep the separate publish at the end of the run
    cp.clip_rows = B.d_clip_rows; cp.flags = B.d_counters + 1; cp.fused = b->tune.no_fuse ? 0 : 1;
    cp.host = D.tail_kernel ? nullptr : b->h_totals_dev;
    b->published = compact_is_fused(cp) && cp.host != nullptr;
    // ... and, outside a stream capture, it leaves the counters cleared for the batch's next run (a captured run keeps its own clear kernel: a graph must not depend on what ran before it)
    const bool self_clear = b->published && !b->capturing && !b->keep_counters;
    cp.clr_counters = self_clear ? B.d_counters : nullptr; cp.clr_hist = self_clear ? b->d_span_hist : nullptr;
    b->end_clears = self_clear;
    launch_compact(cp, s);
    if (D.level == 11) {
        UttParams u;
        B.fill(u, b->d_frame_off);
        launch_utterance(u, s);
    }
    if (D.level == 12) {
        CoefParams q;
        B.fill(q, b->d_frame_off);
        q.total_frames = b->total_frames;
        launch_coeffs(q, b->n_clips * (uint32_t)B.row_cap, s);
    }
    HIP_TRY(ctx, hipGetLastError());
    return WSA_OK;
}

wsa_status wsa_api::run_impl(wsa_batch* b, const float* d_pcm, uint64_t stride, const uint32_t* d_spec_in, bool fe, bool be, hipStream_t s) {
    wsa_ctx* ctx = b->ctx;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    {
        hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
        if (s && hipStreamIsCapturing(s, &cap) != hipSuccess) { (void)hipGetLastError(); cap = hipStreamCaptureStatusNone; }
        b->capturing = cap != hipStreamCaptureStatusNone;
        if (b->capturing) b->ever_captured = true;
    }
    // (the previous run's last kernel has cleared the counters already when it was the fused compaction: b->counters_clean.  A batch that has ever been
    //  captured into a graph clears in front of every run: a replay is a run this function does not see)
    if (!b->counters_clean || b->ever_captured) hipLaunchKernelGGL(batch_clear_kernel, dim3(1), dim3(256), 0, s, b->be.d_counters, b->be.d_totals, b->d_span_hist);
    b->counters_clean = false; b->end_clears = false;
    if (b->timing) HIP_TRY(ctx, hipEventRecord(b->ev[0], s));
    const uint32_t* spec = d_spec_in ? d_spec_in : b->d_spec;
    if (fe) {
        if (!d_pcm && b->total_frames) return fail(ctx, WSA_ERR_INVALID, "null PCM pointer");
        if (stride < b->max_host_samples() && b->n_clips > 1) return fail(ctx, WSA_ERR_INVALID, "clip_stride smaller than the longest clip");
        if (b->rs_mixed) {                   // K0 over the planned work list: every clip from its own rate (or copied as it is)
            RsMixedParams r; r.in = d_pcm; r.stride_in = stride; r.out = b->d_rs_pcm; r.stride_out = b->rs_stride; r.n_in = b->d_rs_n_in; r.n_out = b->d_rs_n_out;
            r.tables = b->d_rs_table; r.cls = b->d_rs_cls; r.clip_class = b->d_rs_clip_class; r.work = b->d_rs_work;
            launch_resample_mixed(r, b->rs_plan, !b->tune.rs_one_launch, s);       // (one launch per class beat one launch over the whole list: profiles/mixed_rate.md)
            HIP_TRY(ctx, hipGetLastError());
            d_pcm = b->d_rs_pcm; stride = b->rs_stride;
        } else if (b->rs_on) {               // K0: the caller's PCM (fs_in) -> the batch's own buffer at the analysis rate
            RsParams r; r.in = d_pcm; r.stride_in = stride; r.out = b->d_rs_pcm; r.stride_out = b->rs_stride;
            r.n_in = b->d_rs_n_in; r.n_out = b->d_rs_n_out; r.table = b->d_rs_table;
            resample_shape(b->fs_in, b->fs, b->tune.rs_s, b->tune.rs_j, b->tune.rs_c, r);
            launch_resample(r, b->n_clips, b->max_samples, s);
            HIP_TRY(ctx, hipGetLastError());
            d_pcm = b->d_rs_pcm; stride = b->rs_stride;
        }
        FeParams p;
        b->fe.fill(p, b->tune.fe_fat);
        p.pcm = d_pcm; p.clip_stride = stride; p.n_frames = b->d_n_frames; p.frame_off = b->d_frame_off; p.spec = b->d_spec;
        p.frames_per_wave = b->tune.fpw > 0 ? b->tune.fpw : 25; p.wg_per_cu = b->tune.fe_wg_per_cu;
        p.queue = b->tune.fe_no_queue ? nullptr : b->be.d_counters + 8; p.n_cu = b->ctx->n_cu;      // (counters[8]: the front end's chunk queue, zeroed by batch_clear_kernel)
        launch_frontend(p, (int)b->n_clips, (int)b->max_frames, b->fe.plan.R, b->fe.plan.three, s);
        HIP_TRY(ctx, hipGetLastError());
    }
    if (b->timing) HIP_TRY(ctx, hipEventRecord(b->ev[1], s));
    if (be) {
        if (const wsa_status st = run_backend_stages(b, spec, false, s); st != WSA_OK) return st;
    } else if (b->timing) { HIP_TRY(ctx, hipEventRecord(b->ev[2], s)); HIP_TRY(ctx, hipEventRecord(b->ev[3], s)); }
    if (!(be && b->published)) hipLaunchKernelGGL(batch_publish_kernel, dim3(1), dim3(64), 0, s, b->be.d_totals, b->be.d_counters, b->h_totals_dev);
    if (b->timing) HIP_TRY(ctx, hipEventRecord(b->ev[4], s));
    b->ran = true; b->spec_in_use = spec;
    b->counters_clean = be && b->end_clears && !b->capturing;
    return WSA_OK;
}

wsa_status wsa_api::fetch_totals(wsa_batch* b, hipStream_t s) {
    wsa_ctx* ctx = b->ctx;
    if (!b->ran) return no_run_yet(b);
    // always re-read: a captured graph may have re-run the batch without wsa_batch_run being called again
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipStreamSynchronize(s));             // the run's last kernel has written the counters into the mapped pinned words
    const volatile uint32_t* ht = b->h_totals;
    b->res_rows = ht[0]; b->res_segs = ht[1]; b->res_flags = ht[2]; b->res_utt = ht[3];
    if (b->res_flags & 2u) {
        // the fast tracker variant ran out of LDS active-track slots: rerun the back end (frame
        // records are still in place) with the worst-case table, for this and all later runs.
        // Unconditional on full_table: a hipGraph captured before the switch keeps replaying the fast
        // variant and may overflow again (wsa.h: re-capture after wsa_batch_backend_reruns() changed).
        b->full_table = true; b->reruns++;
        hipLaunchKernelGGL(batch_clear_kernel, dim3(1), dim3(256), 0, s, b->be.d_counters, b->be.d_totals, b->d_span_hist);
        const bool tm = b->timing; b->timing = false;
        const wsa_status st = run_backend_stages(b, b->spec_in_use, true, s);
        b->timing = tm;
        if (st != WSA_OK) return st;
        if (!b->published) hipLaunchKernelGGL(batch_publish_kernel, dim3(1), dim3(64), 0, s, b->be.d_totals, b->be.d_counters, b->h_totals_dev);
        HIP_TRY(ctx, hipStreamSynchronize(s));
        b->res_rows = ht[0]; b->res_segs = ht[1]; b->res_flags = ht[2]; b->res_utt = ht[3];
    }
    if (b->res_flags & 1u) return fail(ctx, WSA_ERR_CAPACITY, "a device-side arena overflowed; results are invalid");
    return WSA_OK;
}

extern "C" {

wsa_status wsa_batch_run(wsa_batch* b, const float* d_pcm, uint64_t clip_stride, void* stream) {
    if (!b) return WSA_ERR_INVALID;
    return wsa_api::run_impl(b, d_pcm, clip_stride, nullptr, true, true, reinterpret_cast<hipStream_t>(stream));
}
wsa_status wsa_batch_run_frontend(wsa_batch* b, const float* d_pcm, uint64_t clip_stride, void* stream) {
    if (!b) return WSA_ERR_INVALID;
    return wsa_api::run_impl(b, d_pcm, clip_stride, nullptr, true, false, reinterpret_cast<hipStream_t>(stream));
}
wsa_status wsa_batch_run_backend(wsa_batch* b, const uint32_t* d_spectra, void* stream) {
    if (!b || !d_spectra) return WSA_ERR_INVALID;
    return wsa_api::run_impl(b, nullptr, 0, d_spectra, false, true, reinterpret_cast<hipStream_t>(stream));
}

// ---- what the classifiers, debug.hip and gather.cpp reach a batch through (api_internal.hpp)
void wsa_batch_view_internal(wsa_batch* b, wsa_batch_view* v) {
    v->ctx = b->ctx; v->level = b->ctx->cfg.output_level; v->n_clips = b->n_clips; v->rows_cap = b->n_clips * (uint32_t)b->be.row_cap;
    v->d_utt_feat = b->be.d_utt_feat; v->d_utt_off = b->be.d_utt_off; v->utt_cap = b->n_clips * (uint32_t)b->be.seg_cap;
    v->d_meta = b->be.d_meta; v->d_feat = b->be.d_feat; v->d_row_off = b->be.d_row_off; v->reruns = b->reruns; v->cls = &b->cls; v->ecls = &b->ecls; v->cls_last = &b->cls_last; v->kcls = &b->kcls; v->rcls = &b->rcls;
}
wsa_status wsa_batch_fetch_internal(wsa_batch* b, hipStream_t s) { return wsa_api::fetch_totals(b, s); }
const uint32_t* wsa_batch_counters_internal(wsa_batch* b, int keep, wsa_ctx** ctx) {
    if (keep >= 0) b->keep_counters = keep != 0;
    if (ctx) *ctx = b->ctx;
    return b->be.d_counters;
}

// (gather.cpp checks that a rank's batch belongs to the rank's context)
wsa_ctx* wsa_batch_ctx_internal(const wsa_batch* b) { return b ? b->ctx : nullptr; }

// tuning (not part of wsa.h): the batch's 16 device counters as the last run left them
int wsa_debug_batch_counters(wsa_batch* b, uint32_t* out16) {
    if (!b || !out16) return WSA_ERR_INVALID;
    return hipMemcpy(out16, b->be.d_counters, 16 * sizeof(uint32_t), hipMemcpyDeviceToHost) == hipSuccess ? WSA_OK : WSA_ERR_HIP;
}

}  // extern "C"
