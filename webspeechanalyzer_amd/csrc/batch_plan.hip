// batch_plan.hip — a batch is planned once: frame counts, capacities, the tracker variant, every device buffer (wsa_batch_create*), and destroyed.
#include "batch_internal.hpp"

using namespace wsa;
using wsa_api::fail;

extern "C" {

void wsa_batch_destroy(wsa_batch* b) {
    if (!b) return;
    (void)hipSetDevice(b->ctx->device);
    if (b->d_i16) (void)hipFree(b->d_i16);
    if (b->d_pk) (void)hipFree(b->d_pk);
    for (auto& st : b->up_stream) if (st) (void)hipStreamDestroy(st);
    for (auto& e : b->up_event) if (e) (void)hipEventDestroy(e);
    if (b->up_start) (void)hipEventDestroy(b->up_start);
    for (auto& e : b->ev) if (e) (void)hipEventDestroy(e);
    wsa_cls_free(b->cls);
    wsa_ecls_free(b->ecls);
    wsa_kcls_free(b->kcls);
    wsa_rcls_free(b->rcls);
    delete b;                           // (the arena frees the rest)
}

static wsa_status batch_create_impl(wsa_ctx* ctx, uint32_t n_clips, const uint32_t* n_samples, double fs, const uint32_t* n_samples_in, double fs_in, wsa_batch** out, const double* fs_in_each = nullptr) {
    if (!ctx || !out || (n_clips && !n_samples)) return fail(ctx, WSA_ERR_INVALID, "null argument");
    *out = nullptr;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    wsa_batch* b = new wsa_batch();
    b->ctx = ctx; b->n_clips = n_clips; b->fs = fs;
    b->tune = Tuning::from_env();
    std::string err;
    const FeDev::Refusal refused = b->fe.build(ctx->cfg, fs, b->tune.fe_fat, err);
    if (refused == FeDev::BAD_FFT) err = "unsupported FFT length: NFFT = the smallest of {2^k, 3 * 2^k} >= max(window, fs * N_fft_bins / f_max) must lie in 256 .. 8192 or be 3 * 2^k up to 12288";
    if (refused == FeDev::LDS) err += ": shorten the window or lower f_max / N_fft_bins";
    if (refused != FeDev::OK) { delete b; return fail(ctx, WSA_ERR_INVALID, err); }
    const FePlanHost& P = b->fe.plan;
    b->n_samples.assign(n_samples, n_samples + n_clips);
    b->n_frames.resize(n_clips); b->frame_off.resize(n_clips + 1);
    uint64_t tot = 0;
    for (uint32_t i = 0; i < n_clips; i++) {
        const uint32_t ns = n_samples[i];
        const uint32_t nf = ns < (uint32_t)P.win ? 0u : (ns - (uint32_t)P.win) / (uint32_t)P.hop + 1u;     // FE-1 F1: tail dropped
        b->n_frames[i] = nf; b->frame_off[i] = (uint32_t)tot; tot += nf;
        if (nf > b->max_frames) b->max_frames = nf;
        if (ns > b->max_samples) b->max_samples = ns;
    }
    if (tot * CAND_CAP > 0xfffffff0ull) { delete b; return fail(ctx, WSA_ERR_INVALID, "batch has too many frames"); }     // candidate indices are 32-bit
    b->frame_off[n_clips] = (uint32_t)tot; b->total_frames = (uint32_t)tot;

    // capacity bounds (DESIGN.md "capacities"): nothing below can overflow for any input
    const Derived& D = b->D = Derived(ctx->cfg, P.bands);
    BackEnd& B = b->be;
    B.n = n_clips;
    B.set_caps(D, P.bands, b->max_frames);
    B.seg_cap = batch_seg_cap(b->max_frames, D);
    B.row_cap = D.syllable_rows ? (int)b->max_frames / 2 + 2 : B.seg_cap;
    // two spans per wave (two work spaces each) wherever the paired tracker variant applies: its bit map of peak bins covers 128 bands,
    // level 3 and the per-frame trace keep the one-span kernel (WSA_NO_PAIR=1: test hook)
    b->pair = !D.raw_tracks && P.bands <= 128 && !b->tune.no_pair;
    // split finalize (the paired accumulate and the finalize as two kernels; WSA_NO_SPLIT=1: test hook for the one-kernel variant): the spans' tracks and points
    // live in regions of one pool (4.7 KB per frame of the batch) instead of per-wave work spaces
    b->pool_bpf = tracker_pool_bpf();
    b->split = b->pair && !b->tune.no_split && (size_t)b->total_frames * b->pool_bpf <= ((size_t)48 << 30);      // (a plan of more than ~10 M frames keeps the per-wave work spaces: bounded memory)
    const size_t budget = (size_t)(b->pair ? 16 : 8) << 30;
    size_t waves = budget / ((b->be.ws_stride ? b->be.ws_stride : 1) * (b->pair ? 2 : 1));
    size_t wpc = 16;                                          // tracker waves per CU = what the default variant's registers and LDS allow (tuning knob WSA_TRACKER_WPC)
    if (b->tune.tracker_wpc >= 1 && b->tune.tracker_wpc <= 32) wpc = (size_t)b->tune.tracker_wpc;
    const size_t want = (size_t)ctx->n_cu * wpc;
    if (waves > want) waves = want;
    if (waves > (size_t)n_clips * (size_t)b->be.seg_cap) waves = (size_t)n_clips * (size_t)b->be.seg_cap;
    if (b->pair && waves > ((size_t)n_clips * (size_t)b->be.seg_cap + 1) / 2 && n_clips * (size_t)b->be.seg_cap > 256) waves = ((size_t)n_clips * (size_t)b->be.seg_cap + 1) / 2;   // a wave takes two spans (the redo kernel runs on up to 1024 of them)
    if (waves < 1) waves = 1;
    b->n_waves = (int)waves;

    DevArena& A = b->mem;
    const size_t spans = (size_t)n_clips * B.seg_cap;
    bool ok = b->fe.upload(A) && A.upload(&b->d_n_frames, b->n_frames) && A.upload(&b->d_frame_off, b->frame_off) && A.alloc(&b->d_spec, (size_t)b->total_frames * P.bands);
    if (ok && D.level > 2 && b->split) {
        // split finalize: the span pool (4.7 KB per frame of the batch) and the span headers first — when the device cannot give them (several planned batches,
        // a cached plan, a smaller device), the plan falls back to the one-kernel paired tracker with its per-wave work spaces instead of failing
        size_t free_b = 0, total_b = 0;
        const size_t pool_bytes = (size_t)b->total_frames * b->pool_bpf;
        const bool room = hipMemGetInfo(&free_b, &total_b) != hipSuccess || free_b > pool_bytes + ((size_t)2 << 30);
        if (!(room && A.alloc(&b->d_pool, pool_bytes) && A.alloc(&b->d_span_hdr, spans * 8))) {
            (void)hipGetLastError();
            b->split = false; b->d_pool = nullptr; b->d_span_hdr = nullptr;
        }
    }
    ok = ok && B.alloc(A, D, b->total_frames, false) && A.alloc(&B.d_counters, 16);
    if (D.level > 2)
        ok = ok && A.alloc(&B.d_ws, B.ws_stride * (size_t)b->n_waves * (b->pair && !b->split ? 2 : 1)) && A.alloc(&b->d_redo, spans) && A.alloc(&b->d_order, spans)
                && A.alloc(&b->d_span_hist, (size_t)SPAN_BUCKETS) && A.alloc(&b->d_span_key, spans)
                && (!D.raw_tracks || (A.alloc(&B.d_trk_pts, ((size_t)b->total_frames + 1) * 64 * 2) && A.alloc(&B.d_trk_rank, ((size_t)b->total_frames + 1) * 64)))
                && (D.level != 12 || A.alloc(&B.d_coef_ws, (size_t)b->total_frames * 8));
    ok = ok && A.pin(&b->h_totals, &b->h_totals_dev, 8);
    for (auto& e : b->ev) if (ok) ok = hipEventCreate(&e) == hipSuccess;
    if (b->tune.full_table >= 0) b->full_table = b->tune.full_table != 0;       // test hook: start with the worst-case tracker variant
    if (ok && n_samples_in) {              // K0 in front: the caller's PCM is at fs_in, everything planned above works on the converted clips
        b->rs_on = true; b->fs_in = fs_in; b->n_samples_in.assign(n_samples_in, n_samples_in + n_clips);
        for (uint32_t i = 0; i < n_clips; i++) if (n_samples_in[i] > b->max_samples_in) b->max_samples_in = n_samples_in[i];
        b->rs_stride = ((uint64_t)b->max_samples + 3u) & ~3ull;
        ok = A.upload(&b->d_rs_n_in, b->n_samples_in) && A.upload(&b->d_rs_n_out, b->n_samples) && b->mem.alloc(&b->d_rs_pcm, (size_t)n_clips * b->rs_stride + 4);
        if (ok && fs_in_each) {            // one rate per clip: classes + work list
            b->rs_mixed = true;
            if (!plan_resample_mixed(n_clips, b->n_samples.data(), fs_in_each, fs, b->rs_plan, err)) { wsa_batch_destroy(b); return fail(ctx, WSA_ERR_INVALID, err); }
            RsMixedPlan& M = b->rs_plan;
            ok = A.upload(&b->d_rs_table, M.tables) && A.upload(&b->d_rs_cls, M.cls) && A.upload(&b->d_rs_clip_class, M.clip_class) && A.upload(&b->d_rs_work, M.work);
            std::vector<float>().swap(M.tables); std::vector<RsWork>().swap(M.work);
        } else if (ok) {
            std::vector<float> K0, K; build_resample_table(fs_in, fs, K0); resample_table_image(K0, K);
            ok = A.upload(&b->d_rs_table, K);
        }
    }
    if (!ok) {
        const std::string m = std::string("device allocation failed: ") + hipGetErrorString(hipGetLastError());
        wsa_batch_destroy(b);
        return fail(ctx, WSA_ERR_HIP, m);
    }
    *out = b;
    return WSA_OK;
}

wsa_status wsa_batch_create(wsa_ctx* ctx, uint32_t n_clips, const uint32_t* n_samples, double fs, wsa_batch** out) {
    return batch_create_impl(ctx, n_clips, n_samples, fs, nullptr, 0, out);
}

wsa_status wsa_batch_create_resampled(wsa_ctx* ctx, uint32_t n_clips, const uint32_t* n_samples_in, double fs_in, double fs_out, wsa_batch** out) {
    if (!ctx || !out || (n_clips && !n_samples_in)) return fail(ctx, WSA_ERR_INVALID, "null argument");
    if (const wsa_status st = check_rates(ctx, &fs_in, 1, fs_out, nullptr); st != WSA_OK) return st;
    std::vector<uint32_t> n_out(n_clips);
    for (uint32_t i = 0; i < n_clips; i++) {
        const uint64_t n = resample_length(n_samples_in[i], fs_in, fs_out);
        if (n > 0xfffffff0ull) return fail(ctx, WSA_ERR_INVALID, "a converted clip would exceed 2^32 samples");
        n_out[i] = (uint32_t)n;
    }
    return batch_create_impl(ctx, n_clips, n_out.data(), fs_out, n_samples_in, fs_in, out);
}

wsa_status wsa_batch_create_mixed(wsa_ctx* ctx, uint32_t n_clips, const uint32_t* n_samples_in, const double* fs_in, double fs_out, wsa_batch** out) {
    if (!ctx || !out || (n_clips && (!n_samples_in || !fs_in))) return fail(ctx, WSA_ERR_INVALID, n_clips && ctx && out && !fs_in ? "null argument: fs_in holds one rate per clip (clip 0 has none)" : "null argument");
    if (const wsa_status st = check_rates(ctx, fs_in, n_clips, fs_out, "clip"); st != WSA_OK) return st;
    std::vector<uint32_t> n_out(n_clips);
    for (uint32_t i = 0; i < n_clips; i++) {
        const uint64_t n = resample_length(n_samples_in[i], fs_in[i], fs_out);
        if (n > 0xfffffff0ull) return fail(ctx, WSA_ERR_INVALID, "a converted clip would exceed 2^32 samples (clip " + std::to_string(i) + ")");
        n_out[i] = (uint32_t)n;
    }
    return batch_create_impl(ctx, n_clips, n_out.data(), fs_out, n_samples_in, 0, out, fs_in);
}

wsa_status wsa_batch_get_info(const wsa_batch* b, wsa_batch_info* o) {
    if (!b || !o) return WSA_ERR_INVALID;
    o->n_clips = b->n_clips; o->n_frames_total = b->total_frames; o->max_frames_per_clip = b->max_frames; o->bands = (uint32_t)b->fe.plan.bands;
    o->rows_cap = b->n_clips * (uint32_t)b->be.row_cap; o->segments_cap = b->n_clips * (uint32_t)b->be.seg_cap; o->workspace_bytes = b->mem.dev_bytes;
    return WSA_OK;
}

}  // extern "C"
