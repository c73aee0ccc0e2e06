// stream_collect.hip — what a step left behind, handed to the caller: wsa_stream_collect with one gather per level, and the models a stream set
// can have attached (classifier, ensemble, KNN store, regression group, feature DB) with their per-step results.
#include "stream_internal.hpp"

using namespace wsa;
using wsa_api::fail;

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

// more rows / segments than the fixed window the step's epilogue pushes: fetch them all
static wsa_status collect_overflow(wsa_stream* b, uint32_t rows, uint32_t segs, wsa_stream_rows* o) {
    wsa_ctx* ctx = b->ctx;
    if (rows > b->d2h_rows) {
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
    return WSA_OK;
}

// level 3: the ranked raw tracks of every segment of this step (as wsa_batch_copy_tracks: offsets [n_segments + 1][2], points [8 ints], ranked
// track ids), unwrapped out of the stream's pool ring.  Segments arrive in (stream, k) order; the device table is per (stream, k of this step)
static wsa_status collect_tracks(wsa_stream* b, uint32_t segs, hipStream_t s, wsa_stream_rows* o) {
    wsa_ctx* ctx = b->ctx;
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
    return WSA_OK;
}

// level 11: one 264-vector per result of this step (in (stream, result) order: the segments of the step that produced a result entry)
static wsa_status collect_utterance(wsa_stream* b, uint32_t segs, wsa_stream_rows* o) {
    wsa_ctx* ctx = b->ctx;
    uint32_t nu = 0;
    for (uint32_t k = 0; k < segs; k++) nu += o->segments[4 * k + 3] >= 0 ? 1u : 0u;
    b->x_utt_meta.resize((size_t)nu * 4 + 1); b->x_utt_feat.resize((size_t)nu * WSA_NUTT + 1);
    if (nu) {
        HIP_TRY(ctx, hipMemcpy(b->x_utt_meta.data(), b->be.d_utt_meta, (size_t)nu * 4 * sizeof(int32_t), hipMemcpyDeviceToHost));
        HIP_TRY(ctx, hipMemcpy(b->x_utt_feat.data(), b->be.d_utt_feat, (size_t)nu * WSA_NUTT * sizeof(double), hipMemcpyDeviceToHost));
    }
    o->n_utterance_rows = nu; o->utt_meta = b->x_utt_meta.data(); o->utt_feat = b->x_utt_feat.data();
    return WSA_OK;
}

// levels 4 / 10: the straightened frames of every row's segment / syllable (meta[6] = first frame since the stream's START,
// meta[7] frames) come out of the stream's ring: one gather kernel and one copy at collect time (not part of the graph)
static wsa_status collect_formants(wsa_stream* b, uint32_t rows, hipStream_t s, wsa_stream_rows* o) {
    wsa_ctx* ctx = b->ctx;
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
    return WSA_OK;
}

// One attach entry (wsa_stream_set_*): the last step is awaited, then the new state is built — a refusal there leaves the old state, the other
// attachments and the graph as they were; only then the graph is dropped (the next step recaptures with or without the state's kernels) and the old
// state freed.  on = false detaches.  create(view, &state) is the state's wsa_s*_create with the entry's own arguments bound
template <typename STATE, typename CREATE>
static wsa_status attach_state(wsa_stream* b, STATE** slot, void (*free_state)(STATE*), bool on, CREATE create) {
    wsa_ctx* ctx = b->ctx;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (b->stepped) HIP_TRY(ctx, hipStreamSynchronize(b->last_stream ? b->last_stream : b->own));     // the last step may still read the tables
    STATE* n = nullptr;
    if (on) {
        const wsa_scls_view v{ctx, ctx->cfg.output_level, b->n, b->rows_cap, b->d2h_rows, b->be.d_meta, b->be.d_feat, b->be.d_row_off, b->be.d_totals, b->d_ctl + 2 * (size_t)b->n};
        const wsa_status st = create(v, &n);
        if (st != WSA_OK) return st;
    }
    b->drop_graph();
    free_state(*slot);
    *slot = n;
    return WSA_OK;
}

// One result entry: the attached state's tables of the last step, once that step is done
template <typename STATE, typename RESULT>
static wsa_status attached_result(wsa_stream* b, STATE* state, const char* none_attached, wsa_status (*result)(STATE*, uint32_t, RESULT*), RESULT* out) {
    wsa_ctx* ctx = b->ctx;
    if (!state) return fail(ctx, WSA_ERR_INVALID, none_attached);
    if (!b->stepped) return wsa_api::no_step_yet(b);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipStreamSynchronize(b->last_stream ? b->last_stream : b->own));
    return result(state, b->h_totals[0], out);
}

extern "C" {

wsa_status wsa_stream_collect(wsa_stream* b, void* stream, wsa_stream_rows* o) {
    if (!b || !o) return WSA_ERR_INVALID;
    wsa_ctx* ctx = b->ctx;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (!s) s = b->own;
    if (!b->stepped) return wsa_api::no_step_yet(b);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipStreamSynchronize(s));
    const uint32_t rows = b->h_totals[0], segs = b->h_totals[1];
    o->n_rows = rows; o->n_segments = segs; o->status_flags = (b->h_totals[3] & 1u) | (b->h_totals[2] ? 1u : 0u);
    o->row_meta = b->h_meta; o->row_feat = b->h_feat; o->segments = b->h_seg; o->stream_cuts = b->h_totals + 4;
    // FD-2: the step's outcome for the attached feature DB is read here, once, and the DB's count advances
    if (b->sfdb && wsa_sfdb_settle(b->sfdb)) o->status_flags |= WSA_FLAG_DB_FULL;
    // a span cut at the ring's capacity in this step is flagged for hosts that do not look at the per-stream counters
    if (b->seen_cuts.size() != b->n) b->seen_cuts.assign(b->n, 0u);
    for (uint32_t i = 0; i < b->n; i++) if (b->h_totals[4 + i] != b->seen_cuts[i]) { o->status_flags |= WSA_FLAG_STREAM_CUT; b->seen_cuts[i] = b->h_totals[4 + i]; }
    if (const wsa_status st = collect_overflow(b, rows, segs, o); st != WSA_OK) return st;
    o->formants = nullptr; o->row_formant_off = nullptr;
    o->n_track_points = 0; o->n_track_ranked = 0; o->track_off = nullptr; o->track_points = nullptr; o->track_ranked = nullptr;
    o->n_utterance_rows = 0; o->utt_meta = nullptr; o->utt_feat = nullptr;
    if (b->be.d_trk_pts) if (const wsa_status st = collect_tracks(b, segs, s, o); st != WSA_OK) return st;
    if (b->d_utt_state) if (const wsa_status st = collect_utterance(b, segs, o); st != WSA_OK) return st;
    if (b->be.d_formants && !b->be.d_sums && !b->d_utt_state) if (const wsa_status st = collect_formants(b, rows, s, o); st != WSA_OK) return st;
    if (o->status_flags & 1u)
        return fail(ctx, WSA_ERR_CAPACITY, "a device-side arena overflowed; results are invalid (step "
                    + std::to_string(b->steps) + ", flags " + std::to_string(b->h_totals[3]) + ", history " + std::to_string(b->h_totals[2]) + ")");
    return WSA_OK;
}

wsa_status wsa_stream_set_model(wsa_stream* b, const wsa_model* m) {
    if (!b) return WSA_ERR_INVALID;
    const wsa_status st = attach_state(b, &b->scls, wsa_scls_free, m != nullptr, [&](const wsa_scls_view& v, wsa_scls** out) { return wsa_scls_create(v, m, out); });
    if (st == WSA_OK && m) { wsa_sens_free(b->sens); b->sens = nullptr; }      // setting a model detaches an ensemble
    return st;
}
wsa_status wsa_stream_set_ensemble(wsa_stream* b, const wsa_ensemble* e) {
    if (!b) return WSA_ERR_INVALID;
    const wsa_status st = attach_state(b, &b->sens, wsa_sens_free, e != nullptr, [&](const wsa_scls_view& v, wsa_sens** out) { return wsa_sens_create(v, e, out); });
    if (st == WSA_OK && e) { wsa_scls_free(b->scls); b->scls = nullptr; }      // setting an ensemble detaches a model
    return st;
}
wsa_status wsa_stream_set_knn(wsa_stream* b, const wsa_knn* kn, uint32_t k) {      // (a model or an ensemble stays attached)
    if (!b) return WSA_ERR_INVALID;
    return attach_state(b, &b->sknn, wsa_sknn_free, kn != nullptr, [&](const wsa_scls_view& v, wsa_sknn** out) { return wsa_sknn_create(v, kn, k, out); });
}
wsa_status wsa_stream_set_regress(wsa_stream* b, const wsa_regress_group* g) {      // (a model, an ensemble and a KNN store stay attached)
    if (!b) return WSA_ERR_INVALID;
    return attach_state(b, &b->sreg, wsa_sreg_free, g != nullptr, [&](const wsa_scls_view& v, wsa_sreg** out) { return wsa_sreg_create(v, g, out); });
}

// (a model, an ensemble, a KNN store and a regression group stay attached; neither of them detaches the DB)
wsa_status wsa_stream_set_featdb(wsa_stream* b, wsa_featdb* db) {
    if (!b) return WSA_ERR_INVALID;
    wsa_ctx* ctx = b->ctx;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (b->stepped) HIP_TRY(ctx, hipStreamSynchronize(b->last_stream ? b->last_stream : b->own));     // the last step may still write the DB
    if (b->sfdb) (void)wsa_sfdb_settle(b->sfdb);              // ... and its rows count
    wsa_sfdb* n = nullptr;
    if (db) {
        const bool utt = ctx->cfg.output_level == 11;
        const wsa_sfdb_view v{ctx, ctx->cfg.output_level, b->n, utt ? b->n * (uint32_t)b->be.seg_cap : b->rows_cap, b->be.d_meta, utt ? b->be.d_utt_feat : b->be.d_feat,
                              utt ? (uint32_t)WSA_NUTT : (uint32_t)WSA_NFEAT, b->be.d_utt_off, b->be.d_totals + (utt ? 3 : 0), b->be.d_counters + 1, b->be.d_totals + 2,
                              b->d_ctl + 2 * (size_t)b->n, b};
        if (const wsa_status st = wsa_sfdb_create(v, db, nullptr, &n); st != WSA_OK) return st;
    }
    b->drop_graph();
    wsa_sfdb_free(b->sfdb);
    b->sfdb = n;
    return WSA_OK;
}
wsa_status wsa_stream_db_rows(wsa_stream* b, wsa_stream_db_result* out) {
    if (!b || !out) return WSA_ERR_INVALID;
    wsa_ctx* ctx = b->ctx;
    if (!b->sfdb) return fail(ctx, WSA_ERR_INVALID, "no feature DB attached to these streams (wsa_stream_set_featdb)");
    if (!b->stepped) return wsa_api::no_step_yet(b);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipStreamSynchronize(b->last_stream ? b->last_stream : b->own));
    return wsa_sfdb_result(b->sfdb, out);
}

wsa_status wsa_stream_classes(wsa_stream* b, wsa_stream_class_result* out) {
    if (!b || !out) return WSA_ERR_INVALID;
    return attached_result(b, b->scls, "no classifier attached to these streams (wsa_stream_set_model)", wsa_scls_result, out);
}
wsa_status wsa_stream_ensemble_classes(wsa_stream* b, wsa_stream_ensemble_result* out) {
    if (!b || !out) return WSA_ERR_INVALID;
    return attached_result(b, b->sens, "no ensemble attached to these streams (wsa_stream_set_ensemble)", wsa_sens_result, out);
}
wsa_status wsa_stream_knn_classes(wsa_stream* b, wsa_stream_knn_result* out) {
    if (!b || !out) return WSA_ERR_INVALID;
    return attached_result(b, b->sknn, "no KNN store attached to these streams (wsa_stream_set_knn)", wsa_sknn_result, out);
}
wsa_status wsa_stream_values(wsa_stream* b, wsa_stream_value_result* out) {
    if (!b || !out) return WSA_ERR_INVALID;
    return attached_result(b, b->sreg, "no regression group attached to these streams (wsa_stream_set_regress)", wsa_sreg_result, out);
}

}  // extern "C"
