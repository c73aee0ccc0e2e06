// stream_internal.hpp — the stream-set object of include/wsa.h and the few functions its sources call across files: stream_api.hip (create / destroy,
// getters), stream_input.hip (input formats, the pull kernels), stream_step.hip (the step), stream_collect.hip (results, attached models).  Nothing here is
// exported; debug.hip reaches a stream set through the *_internal accessors of api_internal.hpp.
#pragma once
#include "host_plan.hpp"      // (and with it <cmath>, <cstring>, <string>, <vector>)
#include "pcm_formats.hpp"

struct wsa_stream {
    wsa_ctx* ctx = nullptr;
    uint32_t n = 0, F = 0, ring = 0;
    std::vector<uint32_t> seen_cuts;        // stream_cuts as of the previous collect (WSA_FLAG_STREAM_CUT)
    double fs = 0;
    wsa::DevArena mem;                      // device and pinned memory (host_plan.hpp); collect's staging buffers grow on demand and are their own allocations
    wsa::FeDev fe;                          // front-end plan and its device tables
    wsa::Derived D;                         // what the configuration decides for the back end
    wsa::BackEnd be;                        // back-end buffers and capacities; frames live in per-stream rings
    wsa::Tuning tune;                       // test switches, read from the environment when the stream set is planned
    uint32_t hist = 0, q = 1, step_samples = 0, stage_stride = 0;     // hist = (q - 1) * hop samples of history, q = ceil(win / hop)
    float *d_stage = nullptr, *d_pcm_in = nullptr;
    uint32_t *d_ctl = nullptr;              // [3][n]: n_frames, pcm_off, ctl bits
    uint32_t *d_frame_off = nullptr, *d_ring_off = nullptr, *d_spec = nullptr;
    wsa::TrackGather trk; std::vector<uint64_t> x_trk_off; std::vector<int32_t> x_trk_pts, x_trk_rank, x_trk_seg;      // level 3: the raw-track pools are per stream a ring of ring x 64 entries
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
    wsa_sfdb* sfdb = nullptr;               // the attached feature DB's plan tables, slots and push words (wsa_stream_set_featdb, spec FD-2), beside all of them
    uint32_t in_stride = 0, ctl_words = 3;  // floats per stream in the input buffers (a plain set: step_samples), control words per stream
    // a mixed set (wsa_stream_create_mixed): F above is the step's internal frame CAPACITY (resample_step_frames_bound), F_user the caller's frames_per_step
    bool mixed = false;
    uint32_t F_user = 0, out_cap = 0, conv_stride = 0, xcap = 0;
    std::vector<double> fs_in, ratio;
    std::vector<uint32_t> in_cap, last_nfr, last_out;      // per stream: samples one step accepts, frames / outputs of its last active step
    std::vector<uint64_t> cN, cY, cK, cS;                  // per stream since START: inputs received, outputs handed on, frames analysed, active steps
    float *d_conv = nullptr, *d_hist = nullptr, *d_rs_tables = nullptr; wsa::RsClass* d_rs_cls = nullptr; uint32_t* d_rs_class = nullptr;
    // packed input (spec PK-1, wsa_stream_set_input_format): own allocations, replaced whenever the format is set
    int32_t fmt = WSA_PCM_F32, g_fmt = WSA_PCM_F32;
    std::vector<uint32_t> chan;             // channels per stream (empty: mono)
    uint8_t *h_pk = nullptr, *h_pk_dev = nullptr;      // [n][pk_stride] bytes, mapped pinned
    uint32_t pk_stride = 0, max_ch = 1;
    uint32_t* d_chan = nullptr;
    // spec PK-3 (wsa_stream_set_input_channels): stream i takes channel sel[i] (or the mix) of the packed row of stream src[i]; d_sel = [sel | src]
    bool chsel = false;
    uint32_t* d_sel = nullptr;

    // the paced count of stream i's s-th active step since START: floor((s + 1) F hop ratio) - floor(s F hop ratio)
    uint32_t paced_count(uint32_t i, uint64_t s) const {
        if (fs_in[i] == fs) return step_samples;
        const double r = ratio[i];
        return (uint32_t)((uint64_t)std::floor((double)((s + 1) * step_samples) * r) - (uint64_t)std::floor((double)(s * step_samples) * r));
    }
    void drop_graph() { if (gexec) { (void)hipGraphExecDestroy(gexec); gexec = nullptr; } }      // the next step recaptures
};

namespace wsa_api {
#pragma GCC visibility push(hidden)
// stream_input.hip, part of the (captured) step: the step's samples as floats — a packed set's rows (d_pcm / stride: the packed device buffer and its
// row stride in bytes, or with host_in the mapped pinned one) decoded, a float set's pinned rows pulled — into d_pcm_in, which *d_pcm / *stride then
// name; device-resident floats stay where they are.  launch_stream_stage: the history shuffle of a plain set with overlapping windows
void launch_stream_pull(wsa_stream* b, const float** d_pcm, uint64_t* stride, bool host_in, hipStream_t s);
void launch_stream_stage(wsa_stream* b, const float* d_pcm, uint64_t stride, hipStream_t s);
inline wsa_status no_step_yet(wsa_stream* b) { return fail(b->ctx, WSA_ERR_INVALID, "no step on this stream object yet"); }
#pragma GCC visibility pop
}  // namespace wsa_api
