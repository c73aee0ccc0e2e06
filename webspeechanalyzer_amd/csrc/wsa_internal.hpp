// wsa_internal.hpp — shared declarations of libwsa (host plan + device kernel parameter blocks).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string>
#include <vector>
#include "../../include/wsa.h"

namespace wsa {

// ---- front-end plan: everything (config, fs) determines; tables computed on the host in fp64 and
// rounded once to fp32 (DESIGN.md "FE-1").  Stands in for what the reference's worklet derives
// from its config message (ref dist/main.js:2 @B6726).
struct FePlanHost {
    int win = 0, hop = 0, nfft = 0, n2 = 0, R = 0, kmax = 0, bands = 0, spec_type = 1;
    int three = 0, M = 0;               // N2 = 3 M (three) or N2 = M; M = 64 R
    std::vector<float> window;          // win
    std::vector<float> tw_n2;           // 2*n2   W_N2^j = (cos, -sin)
    std::vector<float> tw_m;            // 2*M    W_M^j (only when three)
    std::vector<float> tw_64;           // 2*64
    std::vector<float> tw_nfft;         // 2*(kmax+1)
    std::vector<int32_t> mel_k0, mel_cnt, mel_off;
    std::vector<float> mel_w;           // 0.25 * triangle weights, flat
    std::vector<float> emph;            // bands
    float gain = 0;
    std::vector<double> bins_hz;        // bands
};
bool build_fe_plan(const wsa_config& cfg, double fs, FePlanHost& out, std::string& err);

// ---- tuning and test switches (tools/README.md).  The environment is read ONCE per planned batch / stream set (wsa_batch_create,
// wsa_stream_create) and the values travel in the plan: no launch path looks at the environment.
struct Tuning {
    int dbg = 0;                        // WSA_DBG: the DBG_* bits below
    bool no_pair = false, no_split = false, fe_fat = false, peaks_lanes = false;      // WSA_NO_PAIR, WSA_NO_SPLIT, WSA_FE_FAT, WSA_PEAKS_LANES
    bool no_quad = false, quad = false; // WSA_NO_QUAD / WSA_QUAD: two / four spans per wave in the split tracker's tracking kernel whatever the batch size
    bool no_fuse = false;               // WSA_NO_FUSE: the separate scan / gather / publish kernels at the end of a run instead of the fused compaction
    int full_table = -1;                // WSA_FULL_TABLE (-1: not set)
    int tracker_wpc = 0, fin_wpc = 0;   // WSA_TRACKER_WPC, WSA_FIN_WPC: waves per CU of the tracking / finalize kernels (0: default)
    int fpw = 0;                        // WSA_FPW: frames per front-end wave (0: default)
    int fe_wg_per_cu = 0;               // WSA_FE_WGS: workgroups per CU of the persistent 1024-point front end (1 .. 4; 0: default); -1 .. -3: one chunk per workgroup, capped by LDS padding
    bool fe_no_queue = false;           // WSA_FE_NO_QUEUE: one chunk per workgroup instead of the persistent launch
    int peaks_wpc = 0;                  // WSA_PEAKS_WPC: cap on the peak scan's waves per CU (same mechanism)
    int peaks_w = 0;                    // WSA_PEAKS_W: bins per round of the lane-per-frame peak scan, 16 or 32 (0: default)
    int upload_threads = 0;             // WSA_UPLOAD_THREADS (0: default)
    int rs_s = 0, rs_j = 0, rs_c = 0;   // WSA_RS_S / WSA_RS_J / WSA_RS_C: the rate converter's outputs per block row / per lane and run, runs per block (0: default)
    bool rs_one_launch = false;         // WSA_RS_ONE_LAUNCH: a mixed-rate batch's K0 as one launch over the whole work list instead of one per rate class
    static Tuning from_env();
};

// The bits of WSA_DBG (Tuning::dbg, handed to the kernels as GateParams::dbg / TrParams::dbg; tools/README.md lists the numbers, which tests and tools
// pass through the environment).  TUNING: the switch exists only in a library built with `make TUNING=1` (tracker.hip's WSA_TUNE).
enum : int {
    DBG_NO_FINALIZE = 1,                // TUNING, tracker: spans are tracked but not finalized (tools/dbg_sweep.sh, tools/span_probe.py)
    DBG_NO_ACCUMULATE = 2,              // TUNING, tracker: the spans' frames are walked, nothing is tracked (tools/dbg_sweep.sh)
    DBG_NO_FEATURES = 4,                // TUNING, tracker: rows without their feature reductions (tools/dbg_sweep.sh, tools/pmc_whatif.sh)
    DBG_NO_STRAIGHTEN = 8,              // TUNING, tracker: finalize without the straighten loop (tools/dbg_sweep.sh, tools/pmc_whatif.sh)
    DBG_CYCLES = 16,                    // the trace buffer holds the tracker's cycle counts, not the reference trace: the gate leaves it alone, the paired kernels may run (always there);
                                        // TUNING: the tracker writes them (tools/span_probe.py, pair_probe.py, fin_probe.py, redo_probe.py)
    DBG_NO_ENTRIES = 32,                // TUNING, tracker: no candidate entries are loaded (tools/span_probe.py what-ifs)
    DBG_NO_PREFETCH = 64,               // TUNING, tracker: the one-span kernel does not fetch frame headers two blocks ahead
    DBG_GENERIC_FINALIZE = 256,         // tracker: the generic (HBM) finalize for every span (tests/test_gpu_parity.py, tools/dbg_sweep.sh)
    DBG_PHASES = 512,                   // TUNING, tracker: with DBG_CYCLES, cycles per accumulate phase of the one-span kernel (tools/span_probe.py)
    DBG_SMALL_TABLE = 1024,             // tracker: the fast variant's track table overflows at 12 tracks — the rerun path (tests/test_gpu_parity.py)
    DBG_GATE_F64 = 2048,                // gate: the f64 lane-per-candidate kernel also under the auto gate (tests/test_gpu_parity.py)
    DBG_GATE_GENERAL = 4096,            // gate: every frame through the integer kernel's general path (tests/test_gpu_parity.py)
    DBG_UNSORTED_SPANS = 8192,          // batch: spans in (clip, segment) order instead of sorted by length (tools/README.md)
    DBG_SMALL_GROUP_TABLE = 16384,      // tracker: the paired / quad variant's table overflows at 12 tracks — the redo list (tests/test_gpu_parity.py, test_gpu_tracker_limits.py)
    DBG_SELECT_LOOP = 32768,            // tracker: straighten keeps the selection loop instead of the [filing index][rank] table (tests/test_gpu_parity.py "select")
    DBG_NO_PACKED_COLUMNS = 65536,      // tracker: feature sums one formant column at a time also for inputs of at most 15 frames (tests/test_gpu_parity.py)
    DBG_EVENTS_BLOCK = 131072,          // tracker: the energy events of every input through energy_events_block (tests/test_gpu_parity.py)
    DBG_NO_THIRD_FORM = 262144,         // tracker: the finalize kernel's third LDS form off (tests/test_gpu_parity.py)
    DBG_PEAKS_SHIFT = 20,               // bits 20 .. 27 are PkParams::dbg of a batch's peak scan, shifted up (the PK_DBG_* below; tools/app_defaults_profile.sh, tools/pmc_whatif.sh)
};
// PkParams::dbg, all TUNING (peaks.hip's WSA_PKT): parts of the peak scan switched off (tools/peaks_probe.py, tools/pmc_probe.sh through wsa_debug_peaks_time)
enum : int {
    PK_DBG_NO_EMISSION = 1,             // the candidate list is not worked off
    PK_DBG_NO_STATE_MACHINE = 2,        // the per-bin walk of a word's remaining bins is skipped
    PK_DBG_NO_MASK_PASS = 4,            // the rise / fall masks of a round are not formed
    PK_DBG_NO_STORES = 8,               // candidates are not stored
    PK_DBG_NO_LDS_ATOMIC = 16,          // no arg-max of the largest candidate
    PK_DBG_NO_GLOBAL_PATH = 32,         // prefix sums below the ring are not fetched from global memory
};

struct FeParams {
    const float* pcm = nullptr; uint64_t clip_stride = 0;
    const uint32_t* n_frames = nullptr; // [n_clips]
    const uint32_t* frame_off = nullptr; // [n_clips+1]
    uint32_t* spec = nullptr;           // [total_frames][bands]
    int win = 0, hop = 0, kmax = 0, bands = 0, spec_type = 0, frames_per_wave = 0, mel_total = 0, mel_max_taps = 0;
    int mel_max_taps_lo = 0;            // ... of the bands below 64 (the lower band of every lane)
    const float* window = nullptr; const float2* tw_n2 = nullptr; const float2* tw_64 = nullptr; const float2* tw_nfft = nullptr;
    const float2* tw_m = nullptr;       // W_M^j of the three M-point transforms behind the radix-3 stage (NFFT = 3 * 2^k), else nullptr
    const int32_t* mel_k0 = nullptr; const int32_t* mel_cnt = nullptr; const int32_t* mel_off = nullptr; const float* mel_w = nullptr;
    const float* emph = nullptr; float gain = 0;
    const uint32_t* pcm_off = nullptr;  // optional per-clip sample offset into the clip's PCM (streaming warm-up), or nullptr
    int fat = 0, wg_per_cu = 0;         // host side only (Tuning::fe_fat, fe_wg_per_cu)
    // persistent launch of the 1024-point kernel: workgroups take chunks of 4 x frames_per_wave frames of a clip from this counter (zeroed before the
    // launch) until all n_chunks = chunks_per_clip x clips are handed out; nullptr: one chunk per workgroup (grid = chunks)
    uint32_t* queue = nullptr; uint32_t chunks_per_clip = 0, n_chunks = 0; int n_cu = 0;
};

// ---- per-frame peak candidates (output of the parallel half of the reference's frame loop D(), ref @B25827).
// Frame records = one 16-byte header per frame + a candidate table in structure-of-arrays form:
//   hdr[frame]  .x = low word of g (g = sum e[1..B-1] < 2^40), .y = high byte of g | n << 8 | bin of the largest candidate << 16,
//               .z = amplitude of the largest candidate (end-of-spectrum emission excluded, first one on ties; 0 if none),
//               .w = index of the frame's first candidate in the table
//   candidate c amp[c] = e[l];  ent[c] = { i | s << 8 | l << 16 | (end-of-spectrum emission) << 24 (shoulders already shrunk),
//               low word of P[i-1] = sum e[0..i-1], low word of P[s] = sum e[0..s], their high bytes (P[i-1] | P[s] << 8) } — exact
//               prefix sums below 2^40: any merged band sum e[st..en] is one subtraction of two of them.
// 20 bytes per candidate, a frame's candidates contiguous (the gate reads only hdr + amp).  Every frame (ring slot of a stream) has
// its own CAND_CAP entries; consumers find a frame's table through hdr.w.
constexpr int CAND_CAP = 64;               // candidates per frame (all a spectrum of <= 128 bands can have)
struct RecPtrs { uint4* hdr = nullptr; uint32_t* amp = nullptr; uint4* ent = nullptr; };
struct PkParams {
    const uint32_t* spec = nullptr; RecPtrs rec; uint32_t frame0 = 0, total_frames = 0; int bands = 0;   // frames [frame0, frame0 + total_frames)
    // streaming (stream_state != nullptr): spec holds step_frames frames per stream; frame j of stream s goes to
    // record slot s * ring + ((frames the stream has seen so far + j) & (ring - 1)); frames j >= n_frames[s] are skipped
    const double* stream_state = nullptr; const uint32_t* n_frames = nullptr; uint32_t step_frames = 0, ring = 0;
    uint32_t* flags = nullptr;          // bit 0 is raised when a frame holds more than CAND_CAP candidates (only possible above 128 bands)
    int dbg = 0;                        // tuning experiments (TUNING=1 builds, wsa_debug_peaks_time): PK_DBG_* bits
    int lanes_only = 0, wpc = 0;        // host side only (Tuning::peaks_lanes, peaks_wpc)
    int round_bins = 0;                 // host side only: bins per round of the lane-per-frame kernel, 16 or 32 (0: default)
};

// ---- sequential half, split in two (DESIGN.md "back end"):
//   K2a gate kernel    one wavefront per CLIP: candidate gating, voiced state machine, auto noise gate.
//                      None of it depends on the formant tracks, so it runs ahead and emits (a) per frame
//                      what accumulate_fm needs and (b) the list of segments that reach a finalize.
//   K2b tracker kernel one wavefront per SEGMENT span: the tracker is cleared at every reset_segment,
//                      so spans are independent of each other and run in parallel.
struct GateParams {
    RecPtrs rec;
    const uint32_t* n_frames = nullptr; const uint32_t* frame_off = nullptr; uint32_t clip0 = 0, n_clips = 0;     // clips [clip0, clip0 + n_clips)
    int level = 0, max_voiced_bin = 0; double breaker = 0, min_frames = 0; int auto_gate = 0; double ctx_max0 = 0, floor0 = 0;   // ref @B24629
    int32_t* fr_info = nullptr;         // per frame: -1 = accumulate_fm not called, else filing index | stale << 30
    double* fr_v = nullptr;             // per frame: noise floor the peak scan used (`v` at frame start)
    double* fr_fl = nullptr;            // per frame: noise floor handed to accumulate_fm (after the gate)
    int32_t* seg_i = nullptr; double* seg_d = nullptr; int seg_cap = 0;   // per clip [seg_cap][8] / [seg_cap][2], see SEG_* below
    uint32_t* seg_count = nullptr;      // [n_clips]
    uint32_t* clip_rows = nullptr;      // [n_clips] rows handed out of the clip's part of the row pool (zeroed here, bumped by the tracker)
    uint32_t* counters = nullptr;       // [0] largest number of segments any clip holds (the tracker's enumeration bound)
    uint32_t* shared = nullptr;         // batch-wide [1] flags (bit0 capacity overflow)
    double* trace = nullptr; int dbg = 0;
    // span order (batch): every finalized segment takes a rank inside the bucket of its span length (longest first) — an atomic on
    // span_hist[bucket] — and notes {bucket, rank} in span_key[clip * seg_cap + segment]; launch_span_order turns them into the sorted list.  nullptr: off
    uint32_t* span_hist = nullptr; uint2* span_key = nullptr;
    int strided = 1;                    // 1: frame slot's candidates start at slot * CAND_CAP (what the peak scans write); 0: a producer that packs the tables (none at present)
    // streaming (gate_stream_kernel): per-stream state carried from step to step, ring-indexed per-frame arrays
    double* state = nullptr;            // [n_streams][GATE_STATE]
    const uint32_t* ctl = nullptr;      // [n_streams] bit0: fresh stream (launch state) before this step, bit1: segment_truncate after it
    uint32_t ring = 0, step_frames = 0; // ring = frames of history per stream (power of two)
    int32_t* fr_span = nullptr;         // streams: per frame (ring-indexed) the first frame of the span the frame's accumulate_fm call belongs to, or nullptr
    int prio = 0;                       // 1: the batch gate kernel raises its wave priority
};
enum { GATE_STATE = 16 };               // doubles per stream: cur_frame, no_fm, c_ci, c_started, ctx_max, floor, last_max, last_floor, w, T, k, span_begin, spans cut at the ring's capacity
enum { SEG_START = 0, SEG_LEN = 1, SEG_FBEGIN = 2, SEG_FEND = 3, SEG_CCI = 4, SEG_FLAG = 5, SEG_NROWS = 6, SEG_ROW0 = 7 };

struct TrParams {
    RecPtrs rec;
    const uint32_t* frame_off = nullptr;
    int level = 0;
    const int32_t* fr_info = nullptr; const double* fr_v = nullptr; const double* fr_fl = nullptr;
    int32_t* seg_i = nullptr; const double* seg_d = nullptr; int seg_cap = 0;
    const uint32_t* seg_count = nullptr; uint32_t n_clips = 0; const uint32_t* counters = nullptr; uint32_t* shared = nullptr;
    char* ws = nullptr; uint64_t ws_stride = 0; int tcap = 0, pcap = 0, fcap = 0;
    int32_t* row_meta = nullptr; double* row_feat = nullptr; uint32_t row_cap = 0; uint32_t* clip_rows = nullptr;     // row pool: row_cap rows per clip, filled in completion order
    double* trace = nullptr;
    int dbg = 0;                        // WSA_DBG: DBG_* bits
    uint32_t ring_mask = 0xffffffffu;   // 0xffffffff for a batch; ring - 1 when frames live in per-stream rings
    float* formants = nullptr;          // levels 4 / 10: [total_frames][9] f32 straightened frames, or nullptr
    // incremental streaming (tracker_kernel_stream): tracker state of every stream between steps
    int32_t* st_state = nullptr; char* st_act = nullptr;    // [n_streams][TR_STATE_WORDS] counters + accumulators, [n_streams][TR_ACT_BYTES] the active-track table
    const int32_t* fr_span = nullptr; const uint32_t* n_frames_step = nullptr; const double* gate_state = nullptr;   // GateParams::fr_span, frames of this step, GateParams::state
    int4* trk_pts = nullptr; int32_t* trk_rank = nullptr; int32_t* trk_seg = nullptr;   // level 3: point pool [frames * 64][2 x int4], ranked track ids [frames * 64], per segment {pool offset lo, points, ranked, offset hi}
    const uint2* order = nullptr;       // batch: spans sorted by length (launch_span_order), counters[1] of them; nullptr: enumerate (clip, segment)
    float* sums = nullptr;              // level 12: [total_frames] f32 per-frame energy sum of straighten (ref sums[d][1]), or nullptr
    // paired spans (tracker_kernel_pair): spans the lock-step variant declines (more than 32 accepted peaks in a frame, more than 64 live tracks)
    // are listed here and redone by the one-span-per-wave kernel, which then runs with order = redo, order_cnt = 2
    uint2* redo = nullptr; uint32_t* redo_count = nullptr;
    int order_cnt = 1;                  // `order` holds counters[order_cnt] entries
    // split finalize (tracker_kernel_pair_acc + tracker_kernel_finalize): a span's tracks and points live in ITS region of `pool` — pool_bpf bytes per frame
    // of the batch, the region of a span starts at its first frame — and the accumulate kernel leaves span_hdr[(clip * seg_cap + segment) * 8] =
    // {tracks, points, stale index, stale points, sum g, sum E, 1 (finalize) | 2 (arena overflow) | 0 (on the redo list)} for the finalize kernel
    char* pool = nullptr; uint32_t pool_bpf = 0; double* span_hdr = nullptr;
    int fin_waves = 0;                  // host side only: grid of the finalize kernel (0: 2 x the tracking kernel's; Tuning::fin_wpc)
    int quad = 0, quad_waves = 0;       // host side only: four spans per wave in the tracking kernel of the split tracker, its grid
};

struct CompactParams {
    uint32_t n_clips = 0; int seg_cap = 0, level = 0;
    const int32_t* seg_i = nullptr; const uint32_t* seg_count = nullptr;
    const int32_t* row_meta_in = nullptr; const double* row_feat_in = nullptr;
    int32_t* seg_out = nullptr; int32_t* row_meta_out = nullptr; double* row_feat_out = nullptr;
    uint32_t* clip_row_off = nullptr; uint32_t* clip_seg_off = nullptr; uint32_t* totals = nullptr;   // totals[0]=rows, [1]=segs
    // streaming: the callback index and the segments_ci history continue across steps
    int32_t* carry = nullptr;           // [n_streams][CARRY_WORDS]: segments so far, results so far, last CARRY_HIST [start, len]
    const uint32_t* ctl = nullptr;      // as GateParams::ctl
    // fused form (batches; compact_gather_kernel<true>): per-clip row counters as the tracker left them, the flag word, the host's mapped result words (or nullptr)
    const uint32_t* clip_rows = nullptr; const uint32_t* flags = nullptr; uint32_t* host = nullptr; int fused = 0;
    // fused form only: the run's last wave leaves the batch's 16 counters, its totals and its span histogram cleared for the next run (nullptr: the caller launches its clear kernel)
    uint32_t* clr_counters = nullptr; uint32_t* clr_hist = nullptr;
};
bool compact_is_fused(const CompactParams& p);
// the form launch_compact runs: nothing (no clips), the fused gather, compact_scan_kernel<true> + gather, compact_count_kernel + compact_scan_kernel<false> + gather
enum { COMPACT_NOTHING = -1, COMPACT_FUSED = 0, COMPACT_SCAN = 1, COMPACT_COUNT_SCAN = 2 };
int compact_path(const CompactParams& p);
enum { CARRY_HIST = 32, CARRY_WORDS = 2 + 2 * CARRY_HIST };

// ---- K4 utterance features (output_level 11): reads the compacted level-10 products
struct UttParams {
    uint32_t n_clips = 0;
    const int32_t* segments = nullptr; const int32_t* row_meta = nullptr;   // compacted tables (K3 output)
    const uint32_t* clip_seg_off = nullptr; const uint32_t* clip_row_off = nullptr; const uint32_t* frame_off = nullptr;
    const float* formants = nullptr;
    uint32_t* clip_utt_off = nullptr;   // [n_clips + 1]
    int32_t* utt_meta = nullptr; double* utt_feat = nullptr; // [results][4] = {clip, k, first start, sum of lengths}, [results][264]
    uint32_t* totals = nullptr;         // totals[3] = number of results
    // streams (state != nullptr): the tables hold this step's segments / rows only and everything the reference accumulates over a launch is
    // carried per stream: [UTT_STATE_WORDS] = 264 histogram bins, 16 ghost counters, results / segments so far, prev_end, tsum, first start;
    // carry = CompactParams::carry (segments_ci history, already advanced over this step), ctl as GateParams::ctl, frames in rings
    uint32_t* state = nullptr; const int32_t* carry = nullptr; const uint32_t* ctl = nullptr; uint32_t ring_mask = 0xffffffffu;
};
enum { UTT_STATE_WORDS = 288 };

// ---- K0 sample-rate conversion (spec RS-1): out[clip][n] from in[clip][...], one lane per output sample
constexpr int RS_TAPS = 32, RS_OFFS = 32;
struct RsParams {
    const float* in; uint64_t stride_in; float* out; uint64_t stride_out;
    const uint32_t* n_in; const uint32_t* n_out;     // [n_clips] samples per clip before / after
    int chunks;                                       // runs of S * J outputs a block converts one after the other
    const float* table; double ratio; int span, S, J; // the LDS image of the [33][32] offset kernels (resample_table_image), fs_in / fs_out, inputs a block of outputs touches, outputs per block row, outputs per lane
};
void build_resample_table(double fs_in, double fs_out, std::vector<float>& K);
void resample_table_image(const std::vector<float>& K, std::vector<float>& img);
uint64_t resample_length(uint64_t n_in, double fs_in, double fs_out);
int resample_stride(double fs_in, double fs_out);
int resample_span(double ratio, int S, int J);
int resample_outputs_per_lane(int S, double ratio);
void resample_shape(double fs_in, double fs_out, int S, int J, int chunks, RsParams& p);      // ratio, S, J, span, chunks of a single-rate launch; S, J, chunks > 0 override the defaults
uint32_t resample_block(const RsParams& p);                                                    // lanes per block and dynamic LDS bytes of that launch
size_t resample_lds(const RsParams& p);
void launch_resample(const RsParams& p, uint32_t n_clips, uint64_t max_out, hipStream_t s);
// K0 for clips of different rates (wsa_batch_create_mixed): one rate class per distinct fs_in, each with the table, S, J and span the single-rate
// launch would choose for it (copy: fs_in == fs_out, the samples pass unfiltered), and a plan-time work list of one entry per block, sorted by class.
// A pass is one launch per class over that class's slice of the list, with the class's own block size and LDS (default), or one launch over the whole
// list with the largest class's (measured slower, profiles/mixed_rate.md: 1.77 against 1.48 ms on 1024 ten-second clips of four rates)
struct RsClass { double ratio; uint32_t table_off; int span, S, J, copy, pad; };      // table_off: floats into RsMixedParams::tables
struct RsWork { uint32_t clip, blk; };                                                 // block blk of its clip: outputs blk * S * J ... of the clip's class (copy: blk * RS_COPY_RUN ...)
struct RsMixedParams {
    const float* in; uint64_t stride_in; float* out; uint64_t stride_out;
    const uint32_t* n_in; const uint32_t* n_out;
    const float* tables; const RsClass* cls; const uint32_t* clip_class; const RsWork* work;
};
struct RsMixedPlan {
    std::vector<float> tables; std::vector<RsClass> cls; std::vector<uint32_t> clip_class; std::vector<RsWork> work;
    std::vector<uint32_t> first, block, lds;          // per class: its slice of the work list [first[c], first[c + 1]), the block size and dynamic LDS of its own launch
    uint32_t max_block = 64, max_lds = 0, n_work = 0;  // (n_work = work.size(): the batch drops the host copies of tables and work once they are on the device)
};
bool plan_resample_mixed(uint32_t n_clips, const uint32_t* n_out, const double* fs_in, double fs_out, RsMixedPlan& P, std::string& err);
void launch_resample_mixed(const RsMixedParams& p, const RsMixedPlan& P, bool per_class, hipStream_t s);     // per_class: one launch per class instead of one over the whole list

// K0s: the conversion inside a stream step (wsa_stream_create_mixed), one workgroup per stream.  Every count is the host's (the step's mapped
// control words, RS_CTL_WORDS per stream, word w of stream s at ctl[w * n + s]); the kernel decides nothing about how many outputs exist.
enum { RS_CTL_NFR = 0, RS_CTL_OFF = 1, RS_CTL_BITS = 2,      // the three words every stream set has: frames of the step, sample offset, control bits
       RS_CTL_NIN = 3, RS_CTL_NOUT = 4,                      // input samples of the step, outputs [Y, Y + n_out) to convert
       RS_CTL_DST = 5,                                       // int32: stage position of output Y = Y - K * hop (negative where windows leave gaps: those outputs belong to no frame)
       RS_CTL_SHIFT = 6, RS_CTL_CARRY = 7,                   // the carried converted samples: `carry` of them move from stage position `shift` to the front
       RS_CTL_Y_LO = 8, RS_CTL_Y_HI = 9,                     // Y, the absolute index of the step's first output
       RS_CTL_IN0_LO = 10, RS_CTL_IN0_HI = 11,               // int64: absolute index of the first sample of [history | step's samples] = N - RS_HIST
       RS_CTL_WORDS = 12 };
// Input history a stream keeps between steps.  The first output a step could not produce, n, failed floor(n ratio) + 16 <= N, so its oldest tap
// floor(n ratio) - 16 >= N - 31: 31 samples are enough — except behind a step that the length clamp stopped one output short (ratios above 15:
// n ratio > N - ratio - 1, oldest tap >= N - 33).  48 covers both and keeps the rows 16-byte multiples; the host checks every step's oldest tap against it.
constexpr int RS_HIST = 48;
struct RsStreamParams {
    float* stage; uint32_t stage_stride;              // per stream: [carried converted samples | this step's outputs], what the front end reads
    float* conv; uint32_t conv_stride;                // per stream: this step's outputs alone (wsa_stream_copy_converted)
    const float* in; uint64_t in_stride;              // per stream: this step's input samples
    float* hist;                                      // [n][RS_HIST] the newest inputs of the previous steps
    const uint32_t* ctl; uint32_t n;
    const float* tables; const RsClass* cls; const uint32_t* stream_class;
    uint32_t xcap;                                    // floats of LDS behind the table image: RS_HIST + the largest input capacity + RS_TAPS
};
void launch_resample_stream(const RsStreamParams& p, hipStream_t s);
size_t resample_stream_lds(uint32_t xcap);
uint64_t resample_ready(uint64_t n_in, double fs_in, double fs_out);      // outputs whose taps have all arrived, never more than resample_length
uint32_t resample_step_frames_bound(uint32_t frames_per_step, uint32_t hop, double min_ratio);   // frames one step can complete (min_ratio: smallest fs_in / fs_out of the converted streams, 0: none)
uint32_t resample_step_outputs_bound(uint32_t frames_per_step, uint32_t hop, double min_ratio);  // converted samples one step can produce, a STOP step's tail included

void launch_frontend(const FeParams& p, int n_clips, int max_frames, int R, int three, hipStream_t s);
bool fe_supported_R(int R, int three);  // packed FFT length 64 R, R in {2, 4, 8, 16, 32, 64}, or 3 * 64 R, R in {1, 2, 4, 8, 16, 32}
size_t fe_lds_required(const FePlanHost& P, bool fat);      // dynamic LDS of the front-end kernel this geometry selects (limit: LDS_LIMIT, host_plan.hpp)
const char* fe_choice_name(const FePlanHost& P, bool fat);  // ... and that kernel's instantiation by name (test entry wsa_debug_fe_choice)
void launch_peaks(const PkParams& p, hipStream_t s);
void launch_peaks_mode(const PkParams& p, int mode, hipStream_t s);   // 1: lane-per-frame kernel, 2: wave-per-frame kernel (tests)
void launch_gate(const GateParams& p, hipStream_t s);
void launch_gate_stream(const GateParams& p, hipStream_t s);
void launch_gate_blocks(const GateParams& p, uint32_t blocks, hipStream_t s);          // blocks workgroups (0: one per clip) — a workgroup walks clips blockIdx.x, + gridDim.x, ...
void launch_gate_stream_blocks(const GateParams& p, uint32_t blocks, hipStream_t s);
void launch_stream_prepare(double* state, int32_t* carry, int32_t* tr_state, const uint32_t* ctl, uint32_t n, double ctx_max0, double floor0, hipStream_t s);
void launch_tracker(const TrParams& p, int n_waves, bool full_table, bool pair, hipStream_t s);
enum { SPAN_BUCKETS = 2048 };          // span lengths 0 .. 2047+ frames, bucket = SPAN_BUCKETS - 1 - min(frames, SPAN_BUCKETS - 1)
void launch_span_order(const TrParams& p, uint32_t* span_hist, const uint2* span_key, uint2* order, uint32_t* counters, hipStream_t s);
void launch_tracker_stream(const TrParams& p, uint32_t n_streams, hipStream_t s);
enum { TR_STATE_WORDS = 16, TR_ACT_MAX = 320, TR_ACT_BYTES = TR_ACT_MAX * 44 };
void launch_compact(const CompactParams& p, hipStream_t s);
void launch_utterance(const UttParams& p, hipStream_t s);

// ---- K5 polynomial coefficients (output_level 12): reads the compacted level-10 rows + frames + energy sums
struct CoefParams {
    const int32_t* row_meta = nullptr; double* row_feat = nullptr;      // compacted rows: 23 numbers go to row_feat[row][0..22]
    const uint32_t* frame_off = nullptr; const uint32_t* totals = nullptr;   // totals[0] = number of rows
    const float* formants = nullptr; const float* sums = nullptr;        // [total_frames][9], [total_frames]
    double* ws = nullptr; uint32_t total_frames = 0;               // scratch: 8 x total_frames doubles (points of the four fits)
    // streams: the frames live in per-stream rings (frame f of stream c at frame_off[c] + (f & ring_mask)); a syllable's scratch rows are
    // then taken from a per-stream region of scratch_stride (= 2 x ring) rows, where they do not wrap.  Batches: ring_mask = ~0, scratch_stride = 0
    uint32_t ring_mask = 0xffffffffu, scratch_stride = 0;
};
void launch_coeffs(const CoefParams& p, uint32_t rows_cap, hipStream_t s);
size_t tracker_ws_bytes(int tcap, int pcap, int fcap, bool raw_tracks);
size_t tracker_pool_bpf();

}  // namespace wsa
