// debug.hip — test entries of libwsa that are NOT part of include/wsa.h: the accessors of live objects, which reach a batch or a stream set through the
// *_internal accessors of api_internal.hpp (batch_run.hip, stream_step.hip, stream_featdb.hip) and launch nothing of their own.  The entries that feed
// hand-built tables to one kernel family are in debug_units.hip, debug_gate.hip, debug_rows.hip, debug_fold.hip, debug_classify.hip and debug_input.hip.
#include "api_internal.hpp"
#include "debug_internal.hpp"

using namespace wsa_debug;

// which tier of the tracker did a batch's work: out3 = {flag word (bit 0: an arena overflowed, bit 1: the 140-entry table did), spans, spans on the
// redo list} as the batch's last run left them on the device.  A run normally ends with its compaction clearing these counters for the next run, so
// wsa_debug_batch_keep_counters(b, 1) comes first: from then on the batch's runs leave them standing (and start with the clear kernel).  Call it behind
// the run and BEFORE the first fetch of results: a fetch that sees flag bit 1 reruns the back end with the full table, and the counters are the rerun's then.
extern "C" int wsa_debug_batch_keep_counters(wsa_batch* b, int32_t on) {
    if (!b) return WSA_ERR_INVALID;
    (void)wsa_batch_counters_internal(b, on ? 1 : 0, nullptr);
    return WSA_OK;
}
extern "C" int wsa_debug_batch_tiers(wsa_batch* b, void* stream, uint32_t* out3) {
    if (!b || !out3) return WSA_ERR_INVALID;
    wsa_ctx* ctx = nullptr;
    const uint32_t* d = wsa_batch_counters_internal(b, -1, &ctx);
    uint32_t c[16] = {0};
    if (!ctx || !d || hipSetDevice(ctx->device) != hipSuccess) return WSA_ERR_NO_DEVICE;
    if (hipStreamSynchronize(reinterpret_cast<hipStream_t>(stream)) != hipSuccess || !down(c, d, 16)) return WSA_ERR_HIP;
    out3[0] = c[1]; out3[1] = c[5]; out3[2] = c[6];       // d_counters[1]: flags; [4 + 1]: spans (span_order_kernel); [4 + 2]: TrParams::redo_count
    return WSA_OK;
}

// the u32 frames the front end wrote in a stream set's last step, [n_streams][frames_per_step][bands] (a stream that had fewer frames in the step
// leaves the rest of its block as it was); call behind collect
extern "C" int wsa_debug_stream_spectra(wsa_stream* st, uint32_t* out, uint64_t cap_words) {
    if (!st || !out) return WSA_ERR_INVALID;
    wsa_ctx* ctx = nullptr; uint32_t n = 0, F = 0, bands = 0;
    const uint32_t* d = wsa_stream_spec_internal(st, &ctx, &n, &F, &bands);
    const uint64_t words = (uint64_t)n * F * bands;
    if (!ctx || !d || cap_words < words) return WSA_ERR_INVALID;
    if (hipSetDevice(ctx->device) != hipSuccess) return WSA_ERR_NO_DEVICE;
    if (hipDeviceSynchronize() != hipSuccess || !down(out, d, words)) return WSA_ERR_HIP;
    return WSA_OK;
}
// the control words the last step of a PLAIN stream set ran under, as the step's prologue left them on the device: out [3][n_streams] = nfr (frames of
// the stream in the step), off (samples its first frame lies behind the start of its row: the skipped warm-up frames times hop), bits (1 START, 2 STOP,
// 4 active); call behind collect.  A mixed-rate set is refused: its step has other words (RS_CTL_*), planned and tested in tests/stream_resample_model.py
extern "C" int wsa_debug_stream_ctl(wsa_stream* st, uint32_t* out, uint64_t cap_words) {
    if (!st || !out) return WSA_ERR_INVALID;
    wsa_ctx* ctx = nullptr; uint32_t n = 0; int mixed = 0;
    const uint32_t* d = wsa_stream_ctl_internal(st, &ctx, &n, &mixed);
    if (!ctx || !d || mixed || cap_words < 3ull * n) return WSA_ERR_INVALID;
    if (hipSetDevice(ctx->device) != hipSuccess) return WSA_ERR_NO_DEVICE;
    if (hipDeviceSynchronize() != hipSuccess || !down(out, d, 3 * (size_t)n)) return WSA_ERR_HIP;
    return WSA_OK;
}
// One stream step past the front end (stream_step.hip wsa_stream_step_backend_internal): stream i of a plain set gets the first n_frames[i] <= frames_per_step
// frames of its block of frames [n_streams][frames_per_step][bands] (u32, on the host) under the control byte ctl[i] (WSA_STREAM_ACTIVE / START / STOP); the
// control words are written as wsa_stream_step writes them and the product's own launches follow, uncaptured: the step's prologue, launch_stream_prepare,
// then the step's back-end half from the peak scan to the epilogue.  wsa_stream_collect afterwards, as behind any step.  Refused with the stream named: a
// mixed-rate set, a count above frames_per_step, a band count other than the set's, a null pointer.  The step counter and what the next step waits for
// move as in wsa_stream_step, but the input half's carried samples do not: an object is stepped through this entry only, or never through it.
extern "C" int wsa_debug_stream_step_backend(wsa_stream* st, const uint32_t* n_frames, const uint8_t* ctl, const uint32_t* frames, uint32_t bands, void* stream) {
    if (!st) return WSA_ERR_INVALID;
    return wsa_stream_step_backend_internal(st, n_frames, ctl, frames, bands, stream);
}

// Test access to the stream step's feature-DB kernels (spec FD-2; stream_featdb.hip has the body): the plan and the copy kernel once
// over caller-given device tables, so that tests can place rows on the kernels' edges without speech that happens to land there
extern "C" int wsa_debug_stream_featdb_step(wsa_featdb* db, int32_t level, const int32_t* d_meta, const double* d_feat, uint32_t feat_stride, uint32_t rows_cap,
                                            const uint32_t* d_utt_off, uint32_t n_streams, const uint32_t* d_n_rows, const uint32_t* d_flags, const uint32_t* d_bits,
                                            int32_t* d_slot, void* stream, uint32_t* out4, int32_t* kept, uint32_t kept_cap, int32_t* replaced, uint32_t replaced_cap) {
    return wsa_sfdb_debug_step(db, level, d_meta, d_feat, feat_stride, rows_cap, d_utt_off, n_streams, d_n_rows, d_flags, d_bits, d_slot, stream, out4, kept, kept_cap,
                               replaced, replaced_cap);
}
