// batch_internal.hpp — the batch object of include/wsa.h and the few functions its sources call across files: batch_plan.hip (create / destroy),
// batch_run.hip (the stage launches, the fetch), batch_input.hip (host and packed input), batch_results.hip (result tables).  Nothing here is
// exported; debug.hip and the classifiers reach a batch through the *_internal accessors of api_internal.hpp.
#pragma once
#include "host_plan.hpp"      // (and with it <cmath>, <cstring>, <string>, <vector>)
#include "pcm_formats.hpp"

struct wsa_batch {
    wsa_ctx* ctx = nullptr;
    uint32_t n_clips = 0;
    double fs = 0;
    std::vector<uint32_t> n_samples, n_frames, frame_off;
    uint32_t total_frames = 0, max_frames = 0, max_samples = 0;
    wsa::DevArena mem;                   // device and pinned memory (host_plan.hpp); the buffers that grow on demand (d_i16, the track gather's staging) are their own allocations
    wsa::FeDev fe;                       // front-end plan and its device tables
    wsa::Derived D;                      // what the configuration decides for the back end
    wsa::BackEnd be;                     // back-end buffers and capacities
    int n_waves = 0;
    uint32_t *d_n_frames = nullptr, *d_frame_off = nullptr, *d_spec = nullptr;
    uint2* d_order = nullptr;            // spans sorted by length, longest first (launch_span_order)
    uint2* d_redo = nullptr;             // spans the paired tracker variant hands to the one-span kernel
    char* d_pool = nullptr; double* d_span_hdr = nullptr; bool split = false; size_t pool_bpf = 0;   // split finalize: span regions (pool_bpf bytes per frame) + a header per span
    hipStream_t up_stream[8] = {}; hipEvent_t up_event[8] = {}, up_start = nullptr; bool up_ready = false;   // upload_clips
    int16_t* d_i16 = nullptr; uint64_t i16_cap = 0; uint64_t* d_i16_off = nullptr; uint32_t *d_i16_ch = nullptr, *d_i16_ns = nullptr;   // wsa_batch_run_host_i16: upload buffer (own allocation, grows) + clip tables
    std::vector<uint64_t> h_i16_off; std::vector<uint32_t> h_i16_ch;
    // packed clips of any format (spec PK-2, batch_pcm.hip).  wsa_batch_run_host_packed: upload buffer (own allocation, grows) + its descriptor table;
    // wsa_batch_set_input_format / wsa_batch_run_packed: the planned layout's table and offsets — two tables, so that a host run never rewrites what a captured graph reads
    uint8_t* d_pk = nullptr; uint64_t pk_cap = 0; wsa::PcmClipDesc* d_pk_desc = nullptr; std::vector<wsa::PcmClipDesc> h_pk_desc;
    wsa::PcmClipDesc* d_pkf_desc = nullptr; std::vector<uint64_t> pkf_off; bool pkf_set = false;
    bool pkf_channels = false;              // the planned table is PK-3's (wsa_batch_set_input_channels): wsa_batch_run_packed launches batch_deinterleave_kernel
    bool pair = false;                   // tracker: two spans per wave (tracker_kernel_pair)
    bool published = false;              // the last back-end run's compaction kernel has handed the result counters to the host itself
    wsa::Tuning tune;                    // tuning / test switches, read from the environment when the batch is planned
    uint32_t* d_span_hist = nullptr; uint2* d_span_key = nullptr;       // the gate's part of that sort: bucket counts, {bucket, rank} per segment
    float* d_pcm_own = nullptr;
    // sample-rate conversion in front of the path (wsa_batch_create_resampled): input lengths / rate, offset-kernel table, converted PCM
    bool rs_on = false; double fs_in = 0; std::vector<uint32_t> n_samples_in; uint32_t max_samples_in = 0;
    uint32_t *d_rs_n_in = nullptr, *d_rs_n_out = nullptr; float *d_rs_table = nullptr, *d_rs_pcm = nullptr; uint64_t rs_stride = 0;
    // ... for clips of different rates (wsa_batch_create_mixed): rate classes and the work list of K0's blocks, planned once (tables and list live on the device)
    bool rs_mixed = false; wsa::RsMixedPlan rs_plan; wsa::RsClass* d_rs_cls = nullptr; uint32_t* d_rs_clip_class = nullptr; wsa::RsWork* d_rs_work = nullptr;
    bool keep_counters = false;          // test hook (wsa_debug_batch_tiers): the runs leave their counters standing, the next run clears in front
    bool counters_clean = false, end_clears = false, capturing = false, ever_captured = false;      // the fused compaction of the previous run has left the counters cleared: the next run launches no clear kernel
    wsa::TrackGather trk;                                                                       // level 3: wsa_batch_copy_tracks gathers through this
    std::vector<int32_t> h_trk_seg; std::vector<uint32_t> h_seg_count;                          // level 3: host copies for wsa_batch_copy_tracks
    uint32_t res_utt = 0;
    double* d_trace = nullptr;
    uint32_t* h_totals = nullptr;           // pinned + mapped: rows, segs, flags, utterance results — written by batch_publish_kernel at the end of every run
    uint32_t* h_totals_dev = nullptr;       // ... as the device sees it
    hipEvent_t ev[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
    bool timing = true, ran = false, full_table = false;
    uint32_t reruns = 0;
    uint32_t res_rows = 0, res_segs = 0, res_flags = 0;
    const uint32_t* spec_in_use = nullptr;
    wsa_cls* cls = nullptr;                 // wsa_batch_classify (classify_batch.hip)
    wsa_ecls* ecls = nullptr;               // wsa_batch_classify_ensemble (classify_batch.hip)
    int cls_last = 0;                       // which the last classification was (1 / 2; 3: wsa_batch_regress; 4: wsa_batch_regress_group): their results stay apart
    wsa_kcls* kcls = nullptr;               // wsa_batch_knn (knn.hip): its tables stand beside the model calls'
    wsa_rcls* rcls = nullptr;               // wsa_batch_regress_group (regress_fold.hip)

    // what the caller holds: clips at the input rate (a converting batch: before K0) — their lengths, the longest, and the row stride of the float staging buffer
    const std::vector<uint32_t>& host_samples() const { return rs_on ? n_samples_in : n_samples; }
    uint32_t max_host_samples() const { return rs_on ? max_samples_in : max_samples; }
    uint64_t staging_stride() const { return (max_host_samples() + 3u) & ~3ull; }
};

namespace wsa_api {
#pragma GCC visibility push(hidden)
// batch_run.hip.  run_impl: one run on s — the clear kernel where the counters need it, K0 and the front end (fe) from d_pcm at `stride` floats per
// clip, the back end (be) on d_spec_in or the batch's own frames, the publish.  fetch_totals: synchronise, read the counters (reruns the back end on a table overflow)
wsa_status run_impl(wsa_batch* b, const float* d_pcm, uint64_t stride, const uint32_t* d_spec_in, bool fe, bool be, hipStream_t s);
wsa_status fetch_totals(wsa_batch* b, hipStream_t s);
inline wsa_status no_run_yet(wsa_batch* b) { return fail(b->ctx, WSA_ERR_INVALID, "no run on this batch yet"); }
#pragma GCC visibility pop
}  // namespace wsa_api
