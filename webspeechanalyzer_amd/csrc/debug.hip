// debug.hip — test entries of libwsa that are NOT part of include/wsa.h: unit access to device-side pieces that the public
// entry points only exercise through their consequences (tests/test_gpu_units.py, tests/test_gpu_coeffs.py, tests/test_gpu_utterance.py, tests/test_gpu_gate.py,
// tests/test_gpu_regress_group.py, tests/test_gpu_fold.py, tests/test_gpu_frontend.py, tests/test_gpu_batch_pcm.py, tests/test_gpu_dispatch.py, tests/test_gpu_k6.py, tests/test_gpu_resample_cases.py).
#include <cmath>
#include <cstring>
#include <vector>
#include "host_plan.hpp"
#include "api_internal.hpp"
#include "jsmath_device.hpp"
#include "gate_floor.hpp"
#include "tracker_score.hpp"
#include "tracker_features.hpp"
#include "regress_internal.hpp"
#include "classify_internal.hpp"
#include "pcm_formats.hpp"

namespace wsa {
// fn 0: jsm::log10(x[i]); fn 1: jsm::pow_pos(x[i], y[i]) — the V8 Math.log10 / Math.pow ports the noise gate's
// `parseInt(Math.pow(10, t - 3) / 20)` steps depend on (ref dist/main.js:2 @B28615)
__global__ void debug_jsmath_kernel(int fn, const double* x, const double* y, double* out, uint32_t n) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    out[i] = fn == 0 ? jsm::log10(x[i]) : (fn == 2 ? jsm::log10_fin(x[i]) : jsm::pow_pos(x[i], y[i]));      // fn 2: the branch-free log10 of the feature reductions (positive normal arguments)
}
// rows of 8 doubles {gap, dist, track length, track bin, peak bin, track amp, peak amp, velocity} -> match_score (ref dist/main.js:2 @B37340)
__global__ void debug_score_kernel(const double* a, double* out, uint32_t n) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const double* r = a + 8 * (size_t)i;
    out[i] = match_score((int)r[0], r[1], r[2], r[3], r[4], r[5], r[6], r[7]);
}

// the gate's integer floor law against its f64 evaluation for every y in [lo, hi): out[0] = number of y where they differ, out[1] = the
// smallest such y, out[2] = number of y that took the f64 route inside floor_law
__global__ void debug_floor_law_kernel(uint64_t lo, uint64_t hi, unsigned long long* out) {
    unsigned long long bad = 0, first = ~0ull, exact = 0;
    for (uint64_t y = lo + (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; y < hi; y += (uint64_t)gridDim.x * blockDim.x) {
        uint32_t v;
        if (floor_law_needs_exact((uint32_t)y, v)) exact++;
        if (floor_law((uint32_t)y) != floor_law_exact((uint32_t)y)) { bad++; if (y < first) first = y; }
    }
    if (bad) { atomicAdd(&out[0], bad); atomicMin(&out[1], first); }
    if (exact) atomicAdd(&out[2], exact);
}

// the 53-feature reduction on its own: ONE wavefront over n frames of nine floats.  SEL 0: formant_features_wave (frames and the event list in global
// memory); 1: formant_features_lds, frames in LDS, walking events; 2: the same with block events (no_walk); 3: block events with the frames read from
// global memory (as the generic finalize calls it for spans that do not fit its LDS block); 4: the packed form.  Writes x[5 .. 52] like the tracker's calls.
constexpr int DBG_FEAT_LDS_FRAMES = 1024;           // frames the test kernel holds in LDS (36 KB; the tracker's own blocks hold up to 288)
static_assert(DBG_FEAT_LDS_FRAMES <= FEAT_LDS_MAX, "selector 2 stays inside formant_features_lds's domain");
template <int SEL>
__global__ __launch_bounds__(64) void debug_features_kernel(const float* fr_g, int n, double ctx_max, double* x, double* aev) {
    constexpr int LDSF = SEL == 2 ? DBG_FEAT_LDS_FRAMES : (SEL == 1 ? 128 : (SEL == 4 ? 16 : 1));
    __shared__ __attribute__((aligned(16))) float s_fr[LDSF * 9];
    __shared__ __attribute__((aligned(16))) double s_red[FEAT_SCRATCH];
    const int lane = threadIdx.x;
    if (SEL == 0) { formant_features_wave(fr_g, n, ctx_max, x, aev, n + 2, lane); return; }
    const float* fr = fr_g;
    if (SEL != 3) {
        for (int q = lane; q < 9 * n && q < 9 * LDSF; q += 64) s_fr[q] = fr_g[q];
        wsync();
        fr = s_fr;
    }
    formant_features_lds(fr, n, ctx_max, x, lane, s_red, SEL == 4, SEL == 2 || SEL == 3);
}
}  // namespace wsa

extern "C" int wsa_debug_score(int32_t device, const double* args8, double* out, uint32_t n) {
    if (!args8 || !out) return WSA_ERR_INVALID;
    if (hipSetDevice(device) != hipSuccess) return WSA_ERR_NO_DEVICE;
    wsa::DevArena A; double *da = nullptr, *dout = nullptr;
    bool ok = A.alloc(&da, (size_t)n * 8) && A.alloc(&dout, n);
    ok = ok && hipMemcpy(da, args8, (size_t)n * 64, hipMemcpyHostToDevice) == hipSuccess;
    if (ok && n) {
        hipLaunchKernelGGL(wsa::debug_score_kernel, dim3((n + 255) / 256), dim3(256), 0, nullptr, da, dout, n);
        ok = hipGetLastError() == hipSuccess && hipMemcpy(out, dout, (size_t)n * 8, hipMemcpyDeviceToHost) == hipSuccess;
    }
    return ok ? WSA_OK : WSA_ERR_HIP;
}

extern "C" int wsa_debug_floor_law(int32_t device, uint64_t lo, uint64_t hi, uint64_t* out3) {
    if (!out3 || hi > (1ull << 32) || lo > hi) return WSA_ERR_INVALID;
    if (hipSetDevice(device) != hipSuccess) return WSA_ERR_NO_DEVICE;
    wsa::DevArena A; unsigned long long* d = nullptr;
    unsigned long long init[3] = {0ull, ~0ull, 0ull};
    bool ok = A.alloc(&d, 3) && hipMemcpy(d, init, sizeof(init), hipMemcpyHostToDevice) == hipSuccess;
    if (ok) {
        hipLaunchKernelGGL(wsa::debug_floor_law_kernel, dim3(256 * 32), dim3(256), 0, nullptr, lo, hi, d);
        ok = hipGetLastError() == hipSuccess && hipMemcpy(init, d, sizeof(init), hipMemcpyDeviceToHost) == hipSuccess;
    }
    out3[0] = init[0]; out3[1] = init[1]; out3[2] = init[2];
    return ok ? WSA_OK : WSA_ERR_HIP;
}

extern "C" int wsa_debug_jsmath(int32_t device, int32_t fn, const double* x, const double* y, double* out, uint32_t n) {
    if (!x || !out || (fn == 1 && !y) || fn < 0 || fn > 2) return WSA_ERR_INVALID;
    if (hipSetDevice(device) != hipSuccess) return WSA_ERR_NO_DEVICE;
    wsa::DevArena A; double *dx = nullptr, *dy = nullptr, *dout = nullptr;
    bool ok = A.alloc(&dx, n) && A.alloc(&dy, n) && A.alloc(&dout, n);
    ok = ok && hipMemcpy(dx, x, (size_t)n * sizeof(double), hipMemcpyHostToDevice) == hipSuccess;
    if (ok && y) ok = hipMemcpy(dy, y, (size_t)n * sizeof(double), hipMemcpyHostToDevice) == hipSuccess;
    if (ok && n) {
        hipLaunchKernelGGL(wsa::debug_jsmath_kernel, dim3((n + 255) / 256), dim3(256), 0, nullptr, fn, dx, dy, dout, n);
        ok = hipGetLastError() == hipSuccess && hipMemcpy(out, dout, (size_t)n * sizeof(double), hipMemcpyDeviceToHost) == hipSuccess;
    }
    return ok ? WSA_OK : WSA_ERR_HIP;
}

// selector: see debug_features_kernel; a selector outside its variant's domain (1: n <= 128, 2: n <= DBG_FEAT_LDS_FRAMES, 3: n <= FEAT_LDS_MAX, 4: n <= 15) is refused, never run.
// frames9 = n x [bin, energy, width] x 3 (host), out53 (host): [5 .. 52] are what the device function writes, [0 .. 4] (the caller's in the tracker) stay 0
extern "C" int wsa_debug_features(int32_t device, const float* frames9, uint32_t n, double ctx_max, int32_t selector, double* out53) {
    if (!frames9 || !out53 || n < 1 || n > (1u << 24) || selector < 0 || selector > 4) return WSA_ERR_INVALID;
    if ((selector == 1 && n > 128) || (selector == 2 && n > (uint32_t)wsa::DBG_FEAT_LDS_FRAMES) || (selector == 3 && n > (uint32_t)wsa::FEAT_LDS_MAX) || (selector == 4 && n > 15)) return WSA_ERR_INVALID;
    if (hipSetDevice(device) != hipSuccess) return WSA_ERR_NO_DEVICE;
    wsa::DevArena A; float* dfr = nullptr; double *dx = nullptr, *daev = nullptr;
    const size_t nfr = (size_t)n * 9 * sizeof(float);
    bool ok = A.alloc(&dfr, (size_t)n * 9) && A.alloc(&dx, 53, true) && A.alloc(&daev, (size_t)3 * (n + 2), true) && hipMemcpy(dfr, frames9, nfr, hipMemcpyHostToDevice) == hipSuccess;
    if (ok) {
        const int a = (int)n;
        switch (selector) {
        case 0: hipLaunchKernelGGL(wsa::debug_features_kernel<0>, dim3(1), dim3(64), 0, nullptr, dfr, a, ctx_max, dx, daev); break;
        case 1: hipLaunchKernelGGL(wsa::debug_features_kernel<1>, dim3(1), dim3(64), 0, nullptr, dfr, a, ctx_max, dx, daev); break;
        case 2: hipLaunchKernelGGL(wsa::debug_features_kernel<2>, dim3(1), dim3(64), 0, nullptr, dfr, a, ctx_max, dx, daev); break;
        case 3: hipLaunchKernelGGL(wsa::debug_features_kernel<3>, dim3(1), dim3(64), 0, nullptr, dfr, a, ctx_max, dx, daev); break;
        default: hipLaunchKernelGGL(wsa::debug_features_kernel<4>, dim3(1), dim3(64), 0, nullptr, dfr, a, ctx_max, dx, daev); break;
        }
        ok = hipGetLastError() == hipSuccess && hipMemcpy(out53, dx, 53 * sizeof(double), hipMemcpyDeviceToHost) == hipSuccess;
    }
    return ok ? WSA_OK : WSA_ERR_HIP;
}

// the peak-candidate scan on its own: `spec` = n_frames rows of `bands` u32 (host); mode as launch_peaks_mode takes it: 0 = by size, 1 = one lane per
// frame, 2 = one wave per frame (up to 128 bands; wider frames fall to the lane kernel), 3 / 4 = one lane per frame in rounds of 16 / 32 bins
// (peaks_kernel<16> / <32>); out: hdr [n_frames][4], amp [n_frames * 64], ent [n_frames * 64][4] (u32, candidate tables zero-filled beforehand), flags
extern "C" int wsa_debug_peaks(int32_t device, const uint32_t* spec, uint32_t n_frames, int32_t bands, int32_t mode,
                               uint32_t* hdr, uint32_t* amp, uint32_t* ent, uint32_t* flags) {
    if (!spec || !hdr || !amp || !ent || !flags || bands < 1 || n_frames < 1) return WSA_ERR_INVALID;
    if (hipSetDevice(device) != hipSuccess) return WSA_ERR_NO_DEVICE;
    const size_t nsp = (size_t)n_frames * bands * 4, nh = (size_t)n_frames * 16, na = (size_t)n_frames * wsa::CAND_CAP * 4, ne = (size_t)n_frames * wsa::CAND_CAP * 16;
    wsa::DevArena A; char* d = nullptr;
    const size_t o_h = (nsp + 255) & ~(size_t)255, o_a = o_h + ((nh + 255) & ~(size_t)255), o_e = o_a + ((na + 255) & ~(size_t)255), o_f = o_e + ((ne + 255) & ~(size_t)255);
    bool ok = A.alloc(&d, o_f + 256, true) && hipMemcpy(d, spec, nsp, hipMemcpyHostToDevice) == hipSuccess;
    if (ok) {
        wsa::PkParams p{};
        p.spec = reinterpret_cast<const uint32_t*>(d);
        p.rec.hdr = reinterpret_cast<uint4*>(d + o_h); p.rec.amp = reinterpret_cast<uint32_t*>(d + o_a); p.rec.ent = reinterpret_cast<uint4*>(d + o_e);
        p.frame0 = 0; p.total_frames = n_frames; p.bands = bands; p.flags = reinterpret_cast<uint32_t*>(d + o_f);
        wsa::launch_peaks_mode(p, mode, nullptr);
        ok = hipGetLastError() == hipSuccess && hipDeviceSynchronize() == hipSuccess
             && hipMemcpy(hdr, d + o_h, nh, hipMemcpyDeviceToHost) == hipSuccess && hipMemcpy(amp, d + o_a, na, hipMemcpyDeviceToHost) == hipSuccess
             && hipMemcpy(ent, d + o_e, ne, hipMemcpyDeviceToHost) == hipSuccess && hipMemcpy(flags, d + o_f, 4, hipMemcpyDeviceToHost) == hipSuccess;
    }
    return ok ? WSA_OK : WSA_ERR_HIP;
}

// timing of the peak-candidate scan on its own (tuning): the same frames `reps` times, average kernel time in ms; dbg = PkParams::dbg (PK_DBG_* bits)
extern "C" int wsa_debug_peaks_time(int32_t device, const uint32_t* spec, uint32_t n_frames, int32_t bands, int32_t mode, int32_t dbg, int32_t reps, float* ms) {
    if (!spec || !ms || bands < 1 || n_frames < 1 || reps < 1) return WSA_ERR_INVALID;
    if (hipSetDevice(device) != hipSuccess) return WSA_ERR_NO_DEVICE;
    const size_t nsp = (size_t)n_frames * bands * 4, nh = (size_t)n_frames * 16, na = (size_t)n_frames * wsa::CAND_CAP * 4, ne = (size_t)n_frames * wsa::CAND_CAP * 16;
    wsa::DevArena A; char* d = nullptr;
    const size_t o_h = (nsp + 255) & ~(size_t)255, o_a = o_h + ((nh + 255) & ~(size_t)255), o_e = o_a + ((na + 255) & ~(size_t)255), o_f = o_e + ((ne + 255) & ~(size_t)255);
    bool ok = A.alloc(&d, o_f + 256, true) && hipMemcpy(d, spec, nsp, hipMemcpyHostToDevice) == hipSuccess;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    ok = ok && hipEventCreate(&e0) == hipSuccess && hipEventCreate(&e1) == hipSuccess;
    if (ok) {
        wsa::PkParams p{};
        p.spec = reinterpret_cast<const uint32_t*>(d);
        p.rec.hdr = reinterpret_cast<uint4*>(d + o_h); p.rec.amp = reinterpret_cast<uint32_t*>(d + o_a); p.rec.ent = reinterpret_cast<uint4*>(d + o_e);
        p.frame0 = 0; p.total_frames = n_frames; p.bands = bands; p.flags = reinterpret_cast<uint32_t*>(d + o_f); p.dbg = dbg;
        wsa::launch_peaks_mode(p, mode, nullptr);
        (void)hipEventRecord(e0, nullptr);
        for (int r = 0; r < reps; r++) wsa::launch_peaks_mode(p, mode, nullptr);
        (void)hipEventRecord(e1, nullptr);
        ok = hipGetLastError() == hipSuccess && hipDeviceSynchronize() == hipSuccess && hipEventElapsedTime(ms, e0, e1) == hipSuccess;
        *ms /= (float)reps;
    }
    if (e0) (void)hipEventDestroy(e0);
    if (e1) (void)hipEventDestroy(e1);
    return ok ? WSA_OK : WSA_ERR_HIP;
}

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
    if (hipStreamSynchronize(reinterpret_cast<hipStream_t>(stream)) != hipSuccess || hipMemcpy(c, d, sizeof(c), hipMemcpyDeviceToHost) != hipSuccess) return WSA_ERR_HIP;
    out3[0] = c[1]; out3[1] = c[5]; out3[2] = c[6];       // d_counters[1]: flags; [4 + 1]: spans (span_order_kernel); [4 + 2]: TrParams::redo_count
    return WSA_OK;
}

// which K1 instantiation a geometry runs (csrc/fe_r8.hip, fe_rx.hip, fe_r3.hip fe_select_*): its name as profiles/frontend_split.md writes it, e.g.
// "fe_kernel_r8<4,5,8,true,4,3>", into buf (n bytes, zero terminated).  Plans on the host, launches nothing.
extern "C" int wsa_debug_fe_choice(wsa_ctx* ctx, double fs, char* buf, uint32_t n) {
    if (!ctx || !buf || n < 1) return WSA_ERR_INVALID;
    wsa::FePlanHost P; std::string err;
    if (!wsa::build_fe_plan(ctx->cfg, fs, P, err)) return WSA_ERR_INVALID;
    const char* name = wsa::fe_choice_name(P, wsa::Tuning::from_env().fe_fat);
    if (std::strlen(name) + 1 > n) return WSA_ERR_INVALID;
    std::strcpy(buf, name);
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
    if (hipDeviceSynchronize() != hipSuccess || hipMemcpy(out, d, words * 4, hipMemcpyDeviceToHost) != hipSuccess) return WSA_ERR_HIP;
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
    if (hipDeviceSynchronize() != hipSuccess || hipMemcpy(out, d, 3ull * n * 4, hipMemcpyDeviceToHost) != hipSuccess) return WSA_ERR_HIP;
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

// RG-1 (csrc/regress_fold.hpp) on its own: hand-built row meta [n_rows][8] i32 (slot 0 the clip or stream, 1 si, 3 len) and H value columns
// values [H][n_rows] f64 straight into the batch fold or the stream-step fold; no audio, no model.
//   n_steps == 0, a batch of n clips: row_off [n + 1].  Out: n_cb [1]; cb [cb_cap][4]; cb_value, cb_weight [H][cb_cap]; run_sum, run_weight,
//   run_value [H][n].
//   n_steps > 0, n streams: the tables hold the steps' rows one step after the other; row_off [n_steps][n + 1] counts from each step's first row
//   (row_off[k][n] = the rows of step k), ctl [n_steps][n] the steps' control bytes (WSA_STREAM_START resets the stream's sums; a stream
//   without rows in a step is idle whatever its byte says otherwise).  The running sums start from zero and are carried from
//   step to step on the device.  Out: n_cb [n_steps]; the steps' callbacks one step after the other in cb, cb_value, cb_weight (first rows count
//   from their step's first row); run_* [n_steps][H][n], as each step leaves them.
// Every slot of cb_value / cb_weight / cb that no callback fills keeps what the caller put there.  Refused, nothing run and nothing written:
// whatever would make a kernel read or write outside these tables.
// Test access to the stream step's feature-DB kernels (spec FD-2; stream_featdb.hip has the body): the plan and the copy kernel once
// over caller-given device tables, so that tests can place rows on the kernels' edges without speech that happens to land there
extern "C" int wsa_debug_stream_featdb_step(wsa_featdb* db, int32_t level, const int32_t* d_meta, const double* d_feat, uint32_t feat_stride, uint32_t rows_cap,
                                            const uint32_t* d_utt_off, uint32_t n_streams, const uint32_t* d_n_rows, const uint32_t* d_flags, const uint32_t* d_bits,
                                            int32_t* d_slot, void* stream, uint32_t* out4, int32_t* kept, uint32_t kept_cap, int32_t* replaced, uint32_t replaced_cap) {
    return wsa_sfdb_debug_step(db, level, d_meta, d_feat, feat_stride, rows_cap, d_utt_off, n_streams, d_n_rows, d_flags, d_bits, d_slot, stream, out4, kept, kept_cap,
                               replaced, replaced_cap);
}

extern "C" int wsa_debug_regress_fold(int32_t device, const int32_t* meta, const double* values, uint32_t n_rows, uint32_t H, double step_s, uint32_t n,
                                      uint32_t n_steps, const uint32_t* row_off, const uint8_t* ctl, uint32_t cb_cap, uint32_t* n_cb, int32_t* cb,
                                      double* cb_value, double* cb_weight, double* run_sum, double* run_weight, double* run_value) {
    if (!row_off || !n_cb || !cb || !cb_value || !cb_weight || !run_sum || !run_weight || !run_value) return WSA_ERR_INVALID;
    if ((n_rows && (!meta || !values)) || H < 1 || H > WSA_REGRESS_GROUP_MAX || n < 1 || n > (1u << 16) || n_rows > (1u << 22) || cb_cap < 1 || cb_cap > (1u << 22)) return WSA_ERR_INVALID;
    if (n_steps > (1u << 12) || (n_steps && !ctl)) return WSA_ERR_INVALID;
    const uint32_t tables = n_steps ? n_steps : 1;
    uint64_t rows = 0, callbacks = 0;
    for (uint32_t k = 0; k < tables; k++) {                        // every table: offsets in order, rows of their own clip / stream; callbacks counted
        const uint32_t* off = row_off + (size_t)k * (n + 1);
        if (off[0] != 0) return WSA_ERR_INVALID;
        for (uint32_t c = 0; c < n; c++) if (off[c + 1] < off[c]) return WSA_ERR_INVALID;
        if (rows + off[n] > n_rows) return WSA_ERR_INVALID;
        for (uint32_t c = 0; c < n; c++)
            for (uint32_t r = off[c]; r < off[c + 1]; r++) {
                const int32_t* m = meta + (rows + r) * 8;
                if (m[0] != (int32_t)c || m[3] < 0 || m[3] == 0x7fffffff) return WSA_ERR_INVALID;
                callbacks += (r == off[c] || m[1] != m[1 - 8]) ? 1 : 0;
            }
        rows += off[n];
    }
    if (rows != n_rows || callbacks > cb_cap) return WSA_ERR_INVALID;
    if (hipSetDevice(device) != hipSuccess) return WSA_ERR_NO_DEVICE;
    wsa::DevArena A;
    int32_t *d_meta = nullptr, *d_cb = nullptr, *d_t_n = nullptr, *d_t_local = nullptr; double *d_val = nullptr, *d_cbv = nullptr, *d_cbw = nullptr, *d_tv = nullptr, *d_tw = nullptr;
    double *d_sum = nullptr, *d_weight = nullptr, *d_value = nullptr, *d_carry_s = nullptr, *d_carry_w = nullptr;
    uint32_t *d_off = nullptr, *d_bits = nullptr, *d_clip_cb = nullptr, *d_cb_off = nullptr, *d_count = nullptr;
    const size_t R = n_rows ? n_rows : 1, K = cb_cap, HN = (size_t)H * n;
    std::vector<uint32_t> bits((size_t)tables * n, 0u);
    for (size_t i = 0; n_steps && i < bits.size(); i++) bits[i] = (ctl[i] & WSA_STREAM_START) ? 1u : 0u;      // the device control word's bit 0
    bool ok = A.alloc(&d_meta, R * 8) && A.alloc(&d_val, (size_t)H * R) && A.upload(&d_bits, bits) && A.alloc(&d_off, (size_t)tables * (n + 1))
           && A.alloc(&d_cb, K * 4) && A.alloc(&d_cbv, (size_t)H * K) && A.alloc(&d_cbw, (size_t)H * K) && A.alloc(&d_tv, (size_t)H * R) && A.alloc(&d_tw, (size_t)H * R)
           && A.alloc(&d_t_n, R) && A.alloc(&d_t_local, R) && A.alloc(&d_clip_cb, (size_t)n) && A.alloc(&d_cb_off, (size_t)n) && A.alloc(&d_count, 1, true)
           && A.alloc(&d_sum, HN) && A.alloc(&d_weight, HN) && A.alloc(&d_value, HN) && A.alloc(&d_carry_s, HN, true) && A.alloc(&d_carry_w, HN, true)
           && (n_rows == 0 || (hipMemcpy(d_meta, meta, (size_t)n_rows * 8 * sizeof(int32_t), hipMemcpyHostToDevice) == hipSuccess
                               && hipMemcpy(d_val, values, (size_t)H * n_rows * sizeof(double), hipMemcpyHostToDevice) == hipSuccess))
           && hipMemcpy(d_off, row_off, (size_t)tables * (n + 1) * sizeof(uint32_t), hipMemcpyHostToDevice) == hipSuccess
           && hipMemcpy(d_cb, cb, K * 4 * sizeof(int32_t), hipMemcpyHostToDevice) == hipSuccess
           && hipMemcpy(d_cbv, cb_value, (size_t)H * K * sizeof(double), hipMemcpyHostToDevice) == hipSuccess
           && hipMemcpy(d_cbw, cb_weight, (size_t)H * K * sizeof(double), hipMemcpyHostToDevice) == hipSuccess;
    if (!ok) return WSA_ERR_HIP;
    if (!n_steps) {
        wsa_regress::RegressFoldParams p{};
        p.n_clips = n; p.H = H; p.stride = (uint32_t)R; p.step_s = step_s; p.meta = d_meta; p.row_off = d_off;
        for (uint32_t h = 0; h < H; h++) p.value[h] = d_val + (size_t)h * n_rows;
        p.t_value = d_tv; p.t_weight = d_tw; p.t_n = d_t_n; p.t_local = d_t_local; p.clip_cb = d_clip_cb; p.cb_off = d_cb_off;
        p.clip_sum = d_sum; p.clip_weight = d_weight; p.clip_value = d_value; p.cb = d_cb; p.host = d_count;
        // (the compaction's tables have the rows' stride; the callbacks come out through a staging pair of that stride)
        double *d_kv = nullptr, *d_kw = nullptr;
        ok = A.alloc(&d_kv, (size_t)H * R) && A.alloc(&d_kw, (size_t)H * R);
        p.cb_value = d_kv; p.cb_weight = d_kw;
        if (ok) wsa_regress::launch_regress_fold(p, nullptr);
        ok = ok && hipGetLastError() == hipSuccess && hipDeviceSynchronize() == hipSuccess
             && hipMemcpy(n_cb, d_count, sizeof(uint32_t), hipMemcpyDeviceToHost) == hipSuccess;
        for (uint32_t h = 0; ok && h < H; h++)
            ok = callbacks == 0 || (hipMemcpy(cb_value + (size_t)h * K, d_kv + (size_t)h * R, callbacks * sizeof(double), hipMemcpyDeviceToHost) == hipSuccess
                                    && hipMemcpy(cb_weight + (size_t)h * K, d_kw + (size_t)h * R, callbacks * sizeof(double), hipMemcpyDeviceToHost) == hipSuccess);
        ok = ok && (callbacks == 0 || hipMemcpy(cb, d_cb, callbacks * 4 * sizeof(int32_t), hipMemcpyDeviceToHost) == hipSuccess)
             && hipMemcpy(run_sum, d_sum, HN * sizeof(double), hipMemcpyDeviceToHost) == hipSuccess
             && hipMemcpy(run_weight, d_weight, HN * sizeof(double), hipMemcpyDeviceToHost) == hipSuccess
             && hipMemcpy(run_value, d_value, HN * sizeof(double), hipMemcpyDeviceToHost) == hipSuccess;
        return ok ? WSA_OK : WSA_ERR_HIP;
    }
    uint64_t row0 = 0, cb0 = 0;
    for (uint32_t k = 0; ok && k < n_steps; k++) {
        const uint32_t step_rows = row_off[(size_t)k * (n + 1) + n];
        wsa_regress::RegressStepParams p{};
        p.n = n; p.H = H; p.stride = (uint32_t)K; p.cap = 0; p.fold = 1; p.step_s = step_s;       // cap 0: nothing goes to a D2H window
        p.meta = d_meta + row0 * 8; p.row_off = d_off + (size_t)k * (n + 1); p.bits = d_bits + (size_t)k * n;
        for (uint32_t h = 0; h < H; h++) p.value[h] = d_val + (size_t)h * n_rows + row0;
        p.run_sum = d_carry_s; p.run_weight = d_carry_w;
        p.cb = d_cb + cb0 * 4; p.cb_value = d_cbv + cb0; p.cb_weight = d_cbw + cb0;                // this step's callbacks behind the earlier steps'
        p.h_value = nullptr; p.h_cb = nullptr; p.h_cb_value = nullptr; p.h_cb_weight = nullptr;
        p.h_sum = d_sum; p.h_weight = d_weight; p.h_run_value = d_value; p.h_count = d_count;
        wsa_regress::launch_regress_step(p, nullptr);
        ok = hipGetLastError() == hipSuccess && hipDeviceSynchronize() == hipSuccess
             && hipMemcpy(n_cb + k, d_count, sizeof(uint32_t), hipMemcpyDeviceToHost) == hipSuccess
             && hipMemcpy(run_sum + (size_t)k * HN, d_sum, HN * sizeof(double), hipMemcpyDeviceToHost) == hipSuccess
             && hipMemcpy(run_weight + (size_t)k * HN, d_weight, HN * sizeof(double), hipMemcpyDeviceToHost) == hipSuccess
             && hipMemcpy(run_value + (size_t)k * HN, d_value, HN * sizeof(double), hipMemcpyDeviceToHost) == hipSuccess;
        if (ok && cb0 + n_cb[k] > callbacks) return WSA_ERR_HIP;                                    // (cannot happen: the host counted them)
        row0 += step_rows; cb0 += ok ? n_cb[k] : 0;
    }
    ok = ok && hipMemcpy(cb, d_cb, K * 4 * sizeof(int32_t), hipMemcpyDeviceToHost) == hipSuccess
         && hipMemcpy(cb_value, d_cbv, (size_t)H * K * sizeof(double), hipMemcpyDeviceToHost) == hipSuccess
         && hipMemcpy(cb_weight, d_cbw, (size_t)H * K * sizeof(double), hipMemcpyDeviceToHost) == hipSuccess;
    return ok ? WSA_OK : WSA_ERR_HIP;
}

// K4 (csrc/utterance.hip) on its own: hand-built segments, syllable rows and frames straight into ONE launch_utterance, in the batch geometry
// (state == NULL, ring_mask = ~0: clip c's frames are rows frame_off[c] .. frame_off[c + 1] of `formants`, the tables hold the whole clips) or the
// streams' (state, carry and ctl given, ring_mask = ring - 1: stream c's ring is rows frame_off[c] .. + ring, the tables hold ONE step's segments and
// rows, carry [n_clips][CARRY_WORDS] is already advanced over them as compact_gather_kernel leaves it, state [n_clips][UTT_STATE_WORDS] goes in and
// comes back).  segments [n_segs][4] i32 {clip, start, len, flag}, clip_seg_off / clip_row_off / frame_off [n_clips + 1], row_meta [n_rows][8] i32
// (slot 0 the clip, 1 the result index, 6 the syllable's first frame, 7 its length).  Out: utt_feat [rows_cap][264] f64 and utt_meta [rows_cap][4] i32,
// every slot starting as `sentinel`, clip_utt_off [n_clips + 1] and totals[3] likewise; totals[0 .. 2] start as 0 (K4 only ever ORs into totals[2]).
// Refused, nothing run and nothing written: whatever would make the kernel read or write outside these tables.
extern "C" int wsa_debug_utterance(int32_t device, const int32_t* segments, uint32_t n_segs, const uint32_t* clip_seg_off, const int32_t* row_meta, uint32_t n_rows,
                                   const uint32_t* clip_row_off, const float* formants, const uint32_t* frame_off, uint32_t n_clips, uint32_t rows_cap,
                                   uint32_t ring_mask, uint32_t* state, const int32_t* carry, const uint32_t* ctl, int32_t sentinel,
                                   double* utt_feat, int32_t* utt_meta, uint32_t* clip_utt_off, uint32_t* totals4) {
    if (!clip_seg_off || !clip_row_off || !frame_off || !utt_feat || !utt_meta || !clip_utt_off || !totals4) return WSA_ERR_INVALID;
    if ((!segments && n_segs) || (!row_meta && n_rows) || n_clips < 1 || n_clips > (1u << 16) || rows_cap < 1 || rows_cap > (1u << 20)) return WSA_ERR_INVALID;
    const bool streams = state != nullptr;
    if (streams != (carry != nullptr) || streams != (ctl != nullptr)) return WSA_ERR_INVALID;          // the three stream tables come together
    const uint64_t ring = (uint64_t)ring_mask + 1;
    if ((ring & (ring - 1)) != 0) return WSA_ERR_INVALID;                                               // frames are read at (st + o) & ring_mask
    if (streams == (ring_mask == 0xffffffffu)) return WSA_ERR_INVALID;                                  // batches do not wrap, streams do
    if (clip_seg_off[0] != 0 || clip_row_off[0] != 0 || frame_off[0] != 0) return WSA_ERR_INVALID;
    for (uint32_t c = 0; c < n_clips; c++) {
        if (clip_seg_off[c + 1] < clip_seg_off[c] || clip_row_off[c + 1] < clip_row_off[c] || frame_off[c + 1] < frame_off[c]) return WSA_ERR_INVALID;
        if (frame_off[c + 1] > (1u << 26)) return WSA_ERR_INVALID;
        if (streams && frame_off[c + 1] - frame_off[c] < ring) return WSA_ERR_INVALID;                 // a whole ring per stream
    }
    if (clip_seg_off[n_clips] != n_segs || clip_row_off[n_clips] != n_rows || (formants == nullptr && frame_off[n_clips] != 0)) return WSA_ERR_INVALID;
    uint64_t results = 0;
    for (uint32_t c = 0; c < n_clips; c++) {
        const uint32_t nseg = clip_seg_off[c + 1] - clip_seg_off[c];
        for (uint32_t s = clip_seg_off[c]; s < clip_seg_off[c + 1]; s++) results += segments[(size_t)s * 4 + 3] >= 0 ? 1 : 0;
        const uint64_t frames = frame_off[c + 1] - frame_off[c];
        for (uint32_t r = clip_row_off[c]; r < clip_row_off[c + 1]; r++) {
            const int32_t* m = row_meta + (size_t)r * 8;
            if (m[0] < 0 || (uint32_t)m[0] >= n_clips || (uint32_t)m[0] != c || m[6] < 0 || m[7] < 0) return WSA_ERR_INVALID;   // a row of another clip, or of none
            if (streams ? (uint64_t)m[7] > ring : (uint64_t)m[6] + (uint64_t)m[7] > frames) return WSA_ERR_INVALID;             // a syllable outside its clip's frames (its ring)
        }
        if (streams && nseg) {
            const int32_t* cy = carry + (size_t)c * wsa::CARRY_WORDS;
            if (cy[0] < 0 || (uint32_t)cy[0] < nseg) return WSA_ERR_INVALID;                            // K3 has counted this step's segments in already
            if (!(ctl[c] & 1u) && state[(size_t)c * wsa::UTT_STATE_WORDS + 280] > 0x7fffffffu) return WSA_ERR_INVALID;    // the history is indexed with the result count
        }
    }
    if (results > rows_cap) return WSA_ERR_INVALID;
    if (hipSetDevice(device) != hipSuccess) return WSA_ERR_NO_DEVICE;
    const uint64_t frames_all = frame_off[n_clips];
    std::vector<double> hf((size_t)rows_cap * 264, (double)sentinel);
    std::vector<int32_t> hm((size_t)rows_cap * 4, sentinel);
    std::vector<uint32_t> ho((size_t)n_clips + 1, (uint32_t)sentinel);
    const uint32_t tot0[4] = {0, 0, 0, (uint32_t)sentinel};
    wsa::DevArena A; float* dfr = nullptr; int32_t *dseg = nullptr, *dmeta = nullptr, *dum = nullptr, *dcarry = nullptr; double* duf = nullptr;
    uint32_t *dso = nullptr, *dro = nullptr, *dfo = nullptr, *duo = nullptr, *dtot = nullptr, *dstate = nullptr, *dctl = nullptr;
    const size_t noff = ((size_t)n_clips + 1) * sizeof(uint32_t);
    bool ok = A.alloc(&dfr, (size_t)frames_all * 9 + 1) && A.alloc(&dseg, (size_t)n_segs * 4 + 1) && A.alloc(&dmeta, (size_t)n_rows * 8 + 1) && A.alloc(&dso, (size_t)n_clips + 1)
           && A.alloc(&dro, (size_t)n_clips + 1) && A.alloc(&dfo, (size_t)n_clips + 1) && A.alloc(&duo, (size_t)n_clips + 1) && A.alloc(&dtot, 4) && A.alloc(&duf, hf.size()) && A.alloc(&dum, hm.size())
           && (frames_all == 0 || hipMemcpy(dfr, formants, (size_t)frames_all * 9 * sizeof(float), hipMemcpyHostToDevice) == hipSuccess)
           && (n_segs == 0 || hipMemcpy(dseg, segments, (size_t)n_segs * 4 * sizeof(int32_t), hipMemcpyHostToDevice) == hipSuccess)
           && (n_rows == 0 || hipMemcpy(dmeta, row_meta, (size_t)n_rows * 8 * sizeof(int32_t), hipMemcpyHostToDevice) == hipSuccess)
           && hipMemcpy(dso, clip_seg_off, noff, hipMemcpyHostToDevice) == hipSuccess && hipMemcpy(dro, clip_row_off, noff, hipMemcpyHostToDevice) == hipSuccess
           && hipMemcpy(dfo, frame_off, noff, hipMemcpyHostToDevice) == hipSuccess && hipMemcpy(duo, ho.data(), noff, hipMemcpyHostToDevice) == hipSuccess
           && hipMemcpy(dtot, tot0, sizeof(tot0), hipMemcpyHostToDevice) == hipSuccess
           && hipMemcpy(duf, hf.data(), hf.size() * sizeof(double), hipMemcpyHostToDevice) == hipSuccess
           && hipMemcpy(dum, hm.data(), hm.size() * sizeof(int32_t), hipMemcpyHostToDevice) == hipSuccess;
    const size_t nstate = (size_t)n_clips * wsa::UTT_STATE_WORDS, ncarry = (size_t)n_clips * wsa::CARRY_WORDS;
    if (ok && streams)
        ok = A.alloc(&dstate, nstate) && A.alloc(&dcarry, ncarry) && A.alloc(&dctl, n_clips)
             && hipMemcpy(dstate, state, nstate * sizeof(uint32_t), hipMemcpyHostToDevice) == hipSuccess
             && hipMemcpy(dcarry, carry, ncarry * sizeof(int32_t), hipMemcpyHostToDevice) == hipSuccess
             && hipMemcpy(dctl, ctl, (size_t)n_clips * sizeof(uint32_t), hipMemcpyHostToDevice) == hipSuccess;
    if (ok) {
        wsa::UttParams u;
        u.n_clips = n_clips; u.segments = dseg; u.row_meta = dmeta; u.clip_seg_off = dso; u.clip_row_off = dro; u.frame_off = dfo; u.formants = dfr;
        u.clip_utt_off = duo; u.utt_meta = dum; u.utt_feat = duf; u.totals = dtot;
        u.state = dstate; u.carry = dcarry; u.ctl = dctl; u.ring_mask = ring_mask;
        wsa::launch_utterance(u, nullptr);
        ok = hipGetLastError() == hipSuccess && hipDeviceSynchronize() == hipSuccess
             && hipMemcpy(hf.data(), duf, hf.size() * sizeof(double), hipMemcpyDeviceToHost) == hipSuccess
             && hipMemcpy(hm.data(), dum, hm.size() * sizeof(int32_t), hipMemcpyDeviceToHost) == hipSuccess
             && hipMemcpy(ho.data(), duo, noff, hipMemcpyDeviceToHost) == hipSuccess;
        uint32_t tot[4];
        ok = ok && hipMemcpy(tot, dtot, sizeof(tot), hipMemcpyDeviceToHost) == hipSuccess;
        std::vector<uint32_t> hs;
        if (ok && streams) { hs.resize(nstate); ok = hipMemcpy(hs.data(), dstate, nstate * sizeof(uint32_t), hipMemcpyDeviceToHost) == hipSuccess; }
        if (ok) {                                                            // all or nothing: a failed run leaves the caller's tables as they were
            memcpy(utt_feat, hf.data(), hf.size() * sizeof(double)); memcpy(utt_meta, hm.data(), hm.size() * sizeof(int32_t));
            memcpy(clip_utt_off, ho.data(), noff); memcpy(totals4, tot, sizeof(tot));
            if (streams) memcpy(state, hs.data(), nstate * sizeof(uint32_t));
        }
    }
    return ok ? WSA_OK : WSA_ERR_HIP;
}

// K5 (csrc/coeffs.hip) on its own: hand-built syllables straight into coeffs_kernel, in the batch geometry (ring_mask = ~0, scratch_stride = 0: clip c's
// frames are rows frame_off[c] .. frame_off[c + 1] of the frame tables) or the streams' (ring_mask = ring - 1, scratch_stride >= ring_mask + longest
// syllable: stream c's ring is rows frame_off[c] .. + ring).  formants [frame_off[n_clips]][9] f32, sums [frame_off[n_clips]] f32, frame_off [n_clips + 1],
// row_meta [n_rows][8] i32 (slot 0 the clip, 6 the syllable's first frame, 7 its length), one launch_coeffs over rows_cap >= n_rows rows.
// out [rows_cap][WSA_NFEAT] f64: every slot starts as `sentinel`, slot 23 of the first n_rows rows as 0 (what the level-10 row leaves there).
// total_frames is the drivers': all frames of a batch (batch_run.hip), n x 2 x ring for streams (stream_step.hip; here n x scratch_stride).
// Refused, nothing run: whatever would make the kernel read or write outside these tables.
extern "C" int wsa_debug_coeffs(int32_t device, const float* formants, const float* sums, const uint32_t* frame_off, uint32_t n_clips,
                                const int32_t* row_meta, uint32_t n_rows, uint32_t rows_cap, uint32_t ring_mask, uint32_t scratch_stride,
                                double sentinel, double* out) {
    if (!formants || !sums || !frame_off || !row_meta || !out || n_clips < 1 || n_clips > (1u << 16) || n_rows < 1 || rows_cap < n_rows || rows_cap > (1u << 20)) return WSA_ERR_INVALID;
    const uint64_t ring = (uint64_t)ring_mask + 1;
    if ((ring & (ring - 1)) != 0) return WSA_ERR_INVALID;                                   // frames are read at (st + r) & ring_mask
    if (scratch_stride == 0 && ring_mask != 0xffffffffu) return WSA_ERR_INVALID;            // batches do not wrap
    if (scratch_stride != 0 && ring_mask == 0xffffffffu) return WSA_ERR_INVALID;
    for (uint32_t c = 0; c < n_clips; c++) {
        if (frame_off[c + 1] < frame_off[c] || frame_off[c + 1] > (1u << 24)) return WSA_ERR_INVALID;
        if (scratch_stride && frame_off[c + 1] - frame_off[c] < ring) return WSA_ERR_INVALID;    // a whole ring per stream
    }
    for (uint32_t r = 0; r < n_rows; r++) {
        const int32_t* m = row_meta + (size_t)r * 8;
        if (m[0] < 0 || (uint32_t)m[0] >= n_clips || m[6] < 0 || m[7] < 0) return WSA_ERR_INVALID;
        const uint64_t frames = frame_off[m[0] + 1] - frame_off[m[0]];
        if (scratch_stride == 0 ? (uint64_t)m[6] + (uint64_t)m[7] > frames : (uint64_t)m[7] > ring) return WSA_ERR_INVALID;      // a syllable outside its clip's frames (its ring)
        if (scratch_stride && (uint64_t)ring_mask + (uint64_t)m[7] > scratch_stride) return WSA_ERR_INVALID;                    // scratch rows (st & ring_mask) .. + sl stay inside the stream's region
    }
    const uint64_t frames_all = frame_off[n_clips];
    const uint64_t total = scratch_stride ? (uint64_t)n_clips * scratch_stride : frames_all;
    if (total > (1u << 26)) return WSA_ERR_INVALID;
    if (hipSetDevice(device) != hipSuccess) return WSA_ERR_NO_DEVICE;
    std::vector<double> h((size_t)rows_cap * WSA_NFEAT, sentinel);
    for (uint32_t r = 0; r < n_rows; r++) h[(size_t)r * WSA_NFEAT + 23] = 0.0;
    const uint32_t totals[4] = {n_rows, 0, 0, 0};
    wsa::DevArena A; float *dfr = nullptr, *dsum = nullptr; uint32_t *doff = nullptr, *dtot = nullptr; int32_t* dmeta = nullptr; double *dfeat = nullptr, *dws = nullptr;
    bool ok = A.alloc(&dfr, (size_t)frames_all * 9) && A.alloc(&dsum, (size_t)frames_all) && A.alloc(&doff, (size_t)n_clips + 1) && A.alloc(&dtot, 4)
           && A.alloc(&dmeta, (size_t)n_rows * 8) && A.alloc(&dfeat, h.size()) && A.alloc(&dws, (size_t)total * 8, true)
           && (frames_all == 0 || (hipMemcpy(dfr, formants, (size_t)frames_all * 9 * sizeof(float), hipMemcpyHostToDevice) == hipSuccess
                                   && hipMemcpy(dsum, sums, (size_t)frames_all * sizeof(float), hipMemcpyHostToDevice) == hipSuccess))
           && hipMemcpy(doff, frame_off, ((size_t)n_clips + 1) * sizeof(uint32_t), hipMemcpyHostToDevice) == hipSuccess
           && hipMemcpy(dtot, totals, sizeof(totals), hipMemcpyHostToDevice) == hipSuccess
           && hipMemcpy(dmeta, row_meta, (size_t)n_rows * 8 * sizeof(int32_t), hipMemcpyHostToDevice) == hipSuccess
           && hipMemcpy(dfeat, h.data(), h.size() * sizeof(double), hipMemcpyHostToDevice) == hipSuccess;
    if (ok) {
        wsa::CoefParams q;
        q.row_meta = dmeta; q.row_feat = dfeat; q.frame_off = doff; q.totals = dtot; q.formants = dfr; q.sums = dsum;
        q.ws = dws; q.total_frames = (uint32_t)total; q.ring_mask = ring_mask; q.scratch_stride = scratch_stride;
        wsa::launch_coeffs(q, rows_cap, nullptr);
        ok = hipGetLastError() == hipSuccess && hipDeviceSynchronize() == hipSuccess && hipMemcpy(out, dfeat, h.size() * sizeof(double), hipMemcpyDeviceToHost) == hipSuccess;
    }
    return ok ? WSA_OK : WSA_ERR_HIP;
}

// K2a (csrc/gate.hip) on its own: host spectra through the peak scan and ONE gate variant, the gate's outputs copied back as they are.
//   variant 0: the integer kernel with its runs (gate_kernel_auto<false>)      1: the integer kernel, every frame through the general path (<true>, WSA_DBG 4096)
//           2: the f64 lane-per-candidate kernel (gate_kernel_t<false>; what a fixed gate uses, and WSA_DBG 2048)      3: the stream step kernel (gate_kernel_t<true>)
// spec = the clips' frames one after the other ([sum n_frames][bands] u32), settings6 = {window_step, pause_length, min_seg_length, auto_noise_gate, voiced_max_dB,
// voiced_min_dB}; blocks = workgroups of the gate launch (0: one per clip; fewer: a workgroup walks several clips).
// caps_io = {seg_cap, ring}: called with seg_cap 0 the entry only fills in both (seg_cap as the drivers size a clip's / a step's segment table from host_plan.hpp's
// period, ring as a stream set of F frames per step and max_span sizes it) and runs nothing; a run must be handed the same numbers back.
// Batch (variants 0 .. 2) out: fr_info / fr_v / fr_fl [sum n_frames], seg_i [n_clips][seg_cap][8], seg_d [n_clips][seg_cap][2], seg_count [n_clips], flags2 = {the overflow
// flag word, counters[0]}; fr_span and state are not touched.
// Streams (variant 3): clip c is stream c; step k feeds it its next step_nfr[k][c] <= F frames under step_ctl[k][c] (bit 0 START: launch state first, bit 1 STOP:
// segment_truncate behind the frames), launch_stream_prepare + the peak scan + launch_gate_stream once per step.  Out: the per-frame arrays (fr_span too) at the frames'
// place in their clip, read from their ring slot right behind their step; seg_i [n_steps][n_clips][seg_cap][8], seg_d, seg_count [n_steps][n_clips] and state
// [n_steps][n_clips][GATE_STATE] per step; flags2 = {OR of the flag words, largest counters[0]}.  Frames never fed keep what the caller put there.
// Refused, nothing run: the integer kernel under a fixed gate, more than CAND_CAP candidates in a frame (reported after the scan, the gate not run), a step that
// feeds more than F frames or more than the clip has left, a ring the caller did not get from here.
extern "C" int wsa_debug_gate(int32_t device, int32_t variant, const uint32_t* spec, const uint32_t* n_frames, uint32_t n_clips, int32_t bands, const double* settings6,
                              uint32_t blocks, uint32_t F, uint32_t max_span, uint32_t n_steps, const uint32_t* step_nfr, const uint32_t* step_ctl, int32_t* caps_io,
                              int32_t* fr_info, double* fr_v, double* fr_fl, int32_t* fr_span, int32_t* seg_i, double* seg_d, uint32_t* seg_count, uint32_t* flags2, double* state) {
    using namespace wsa;
    if (!n_frames || !settings6 || !caps_io || variant < 0 || variant > 3 || n_clips < 1 || n_clips > 4096 || bands < 4 || bands > 256) return WSA_ERR_INVALID;
    const bool streams = variant == 3;
    wsa_config c{};
    c.output_level = 5; c.N_mel_bins = bands; c.window_width = c.window_step = settings6[0]; c.pause_length = settings6[1]; c.min_seg_length = settings6[2];
    c.auto_noise_gate = settings6[3] != 0 ? 1 : 0; c.voiced_max_dB = settings6[4]; c.voiced_min_dB = settings6[5];
    if (!(c.window_step > 0) || !(c.pause_length >= 0) || !(c.min_seg_length >= 0)) return WSA_ERR_INVALID;
    if (variant < 2 && !c.auto_noise_gate) return WSA_ERR_INVALID;                     // the integer kernel's state is integers only under the auto gate
    uint64_t total = 0; uint32_t max_frames = 0;
    std::vector<uint32_t> foff((size_t)n_clips + 1, 0);
    for (uint32_t i = 0; i < n_clips; i++) {
        if (n_frames[i] > (1u << 20)) return WSA_ERR_INVALID;
        total += n_frames[i]; foff[i + 1] = (uint32_t)total; if (n_frames[i] > max_frames) max_frames = n_frames[i];
    }
    if (total > (1u << 22) || (total && !spec)) return WSA_ERR_INVALID;
    if (streams && (F < 1 || F > 4096 || n_steps < 1 || n_steps > (1u << 20) || !step_nfr || !step_ctl || max_span > (1u << 16))) return WSA_ERR_INVALID;
    const Derived D(c, bands);
    const int seg_cap = streams ? stream_seg_cap(F, D) : batch_seg_cap(max_frames, D);
    const uint32_t ring = streams ? stream_ring_frames(F, max_span) : 0;
    if (caps_io[0] == 0) { caps_io[0] = seg_cap; caps_io[1] = (int32_t)ring; return WSA_OK; }
    if (caps_io[0] != seg_cap || caps_io[1] != (int32_t)ring) return WSA_ERR_INVALID;
    if (!fr_info || !fr_v || !fr_fl || !seg_i || !seg_d || !seg_count || !flags2 || (streams && (!fr_span || !state))) return WSA_ERR_INVALID;
    if (streams) {                                                                       // the schedule stays inside the clips and the step buffer
        std::vector<uint64_t> fed(n_clips, 0);
        for (uint32_t k = 0; k < n_steps; k++)
            for (uint32_t i = 0; i < n_clips; i++) {
                const uint32_t nf = step_nfr[(size_t)k * n_clips + i];
                if (nf > F || (step_ctl[(size_t)k * n_clips + i] & ~3u)) return WSA_ERR_INVALID;
                fed[i] += nf;
                if (fed[i] > n_frames[i]) return WSA_ERR_INVALID;
            }
    }
    if (hipSetDevice(device) != hipSuccess) return WSA_ERR_NO_DEVICE;
    const size_t slots = streams ? (size_t)n_clips * ring : (size_t)total;              // frame records and per-frame outputs: one per frame, or one per ring slot
    const size_t spec_rows = streams ? (size_t)n_clips * F : (size_t)total;
    const size_t segs = (size_t)n_clips * seg_cap;
    DevArena A;
    uint32_t *d_spec = nullptr, *d_nfr = nullptr, *d_foff = nullptr, *d_seg_count = nullptr, *d_clip_rows = nullptr, *d_counters = nullptr, *d_ctl = nullptr;
    RecPtrs rec; int32_t *d_info = nullptr, *d_span = nullptr, *d_seg_i = nullptr, *d_carry = nullptr; double *d_v = nullptr, *d_fl = nullptr, *d_seg_d = nullptr, *d_state = nullptr;
    bool ok = A.alloc(&d_spec, spec_rows * bands + 4, true) && A.alloc(&d_nfr, n_clips) && A.alloc(&d_foff, (size_t)n_clips + 1) && A.alloc(&rec.hdr, slots, true)
           && A.alloc(&rec.amp, slots * CAND_CAP, true) && A.alloc(&rec.ent, slots * CAND_CAP, true) && A.alloc(&d_info, slots, true) && A.alloc(&d_v, slots, true)
           && A.alloc(&d_fl, slots, true) && A.alloc(&d_seg_i, segs * 8, true) && A.alloc(&d_seg_d, segs * 2, true) && A.alloc(&d_seg_count, n_clips, true)
           && A.alloc(&d_clip_rows, n_clips, true) && A.alloc(&d_counters, 16, true)
           && hipMemcpy(d_foff, foff.data(), foff.size() * sizeof(uint32_t), hipMemcpyHostToDevice) == hipSuccess;
    if (ok && streams) ok = A.alloc(&d_span, slots, true) && A.alloc(&d_state, (size_t)n_clips * GATE_STATE, true) && A.alloc(&d_carry, (size_t)n_clips * CARRY_WORDS, true) && A.alloc(&d_ctl, n_clips, true);
    if (!ok) return WSA_ERR_HIP;
    PkParams pk; pk.spec = d_spec; pk.rec = rec; pk.bands = bands; pk.flags = d_counters + 8;
    GateParams g;
    g.rec = rec; g.n_frames = d_nfr; g.frame_off = d_foff; g.n_clips = n_clips; g.level = D.klevel; g.max_voiced_bin = D.max_voiced_bin; g.breaker = D.breaker;
    g.min_frames = D.min_frames; g.auto_gate = D.auto_gate; g.ctx_max0 = D.ctx_max0; g.floor0 = D.floor0; g.fr_info = d_info; g.fr_v = d_v; g.fr_fl = d_fl;
    g.seg_i = d_seg_i; g.seg_d = d_seg_d; g.seg_cap = seg_cap; g.seg_count = d_seg_count; g.clip_rows = d_clip_rows; g.counters = d_counters + 4; g.shared = d_counters;
    g.dbg = variant == 1 ? DBG_GATE_GENERAL : (variant == 2 ? DBG_GATE_F64 : 0);
    uint32_t cnt[16];
    if (!streams) {
        ok = hipMemcpy(d_nfr, n_frames, (size_t)n_clips * sizeof(uint32_t), hipMemcpyHostToDevice) == hipSuccess
          && (total == 0 || hipMemcpy(d_spec, spec, (size_t)total * bands * sizeof(uint32_t), hipMemcpyHostToDevice) == hipSuccess);
        if (ok && total) {
            pk.total_frames = (uint32_t)total;
            launch_peaks(pk, nullptr);
            ok = hipGetLastError() == hipSuccess && hipDeviceSynchronize() == hipSuccess && hipMemcpy(cnt, d_counters, sizeof(cnt), hipMemcpyDeviceToHost) == hipSuccess;
            if (ok && (cnt[8] & 1u)) return WSA_ERR_INVALID;                            // a frame with more than CAND_CAP candidates: its table is cut short
        }
        if (ok) {
            launch_gate_blocks(g, blocks, nullptr);
            ok = hipGetLastError() == hipSuccess && hipDeviceSynchronize() == hipSuccess && hipMemcpy(cnt, d_counters, sizeof(cnt), hipMemcpyDeviceToHost) == hipSuccess
              && (total == 0 || (hipMemcpy(fr_info, d_info, (size_t)total * sizeof(int32_t), hipMemcpyDeviceToHost) == hipSuccess
                                 && hipMemcpy(fr_v, d_v, (size_t)total * sizeof(double), hipMemcpyDeviceToHost) == hipSuccess
                                 && hipMemcpy(fr_fl, d_fl, (size_t)total * sizeof(double), hipMemcpyDeviceToHost) == hipSuccess))
              && hipMemcpy(seg_i, d_seg_i, segs * 8 * sizeof(int32_t), hipMemcpyDeviceToHost) == hipSuccess
              && hipMemcpy(seg_d, d_seg_d, segs * 2 * sizeof(double), hipMemcpyDeviceToHost) == hipSuccess
              && hipMemcpy(seg_count, d_seg_count, (size_t)n_clips * sizeof(uint32_t), hipMemcpyDeviceToHost) == hipSuccess;
            if (ok) { flags2[0] = cnt[1]; flags2[1] = cnt[4]; }
        }
        return ok ? WSA_OK : WSA_ERR_HIP;
    }
    // ---- streams: one prepare + scan + gate per step
    pk.stream_state = d_state; pk.n_frames = d_nfr; pk.step_frames = F; pk.ring = ring; pk.total_frames = n_clips * F;
    g.state = d_state; g.ctl = d_ctl; g.ring = ring; g.step_frames = F; g.fr_span = d_span;
    std::vector<uint32_t> hspec(spec_rows * bands), fed(n_clips, 0);
    std::vector<int32_t> h_info(slots), h_span(slots); std::vector<double> h_v(slots), h_fl(slots);
    flags2[0] = 0; flags2[1] = 0;
    for (uint32_t k = 0; k < n_steps && ok; k++) {
        const uint32_t* nf = step_nfr + (size_t)k * n_clips;
        for (uint32_t i = 0; i < n_clips; i++)
            if (nf[i]) memcpy(&hspec[(size_t)i * F * bands], spec + ((size_t)foff[i] + fed[i]) * bands, (size_t)nf[i] * bands * sizeof(uint32_t));
        const uint32_t zero16[16] = {0};
        ok = hipMemcpy(d_spec, hspec.data(), hspec.size() * sizeof(uint32_t), hipMemcpyHostToDevice) == hipSuccess
          && hipMemcpy(d_nfr, nf, (size_t)n_clips * sizeof(uint32_t), hipMemcpyHostToDevice) == hipSuccess
          && hipMemcpy(d_ctl, step_ctl + (size_t)k * n_clips, (size_t)n_clips * sizeof(uint32_t), hipMemcpyHostToDevice) == hipSuccess
          && hipMemcpy(d_counters, zero16, sizeof(zero16), hipMemcpyHostToDevice) == hipSuccess;
        if (!ok) break;
        launch_stream_prepare(d_state, d_carry, nullptr, d_ctl, n_clips, D.ctx_max0, D.floor0, nullptr);
        launch_peaks(pk, nullptr);
        ok = hipGetLastError() == hipSuccess && hipDeviceSynchronize() == hipSuccess && hipMemcpy(cnt, d_counters, sizeof(cnt), hipMemcpyDeviceToHost) == hipSuccess;
        if (ok && (cnt[8] & 1u)) return WSA_ERR_INVALID;
        if (!ok) break;
        launch_gate_stream_blocks(g, blocks, nullptr);
        ok = hipGetLastError() == hipSuccess && hipDeviceSynchronize() == hipSuccess && hipMemcpy(cnt, d_counters, sizeof(cnt), hipMemcpyDeviceToHost) == hipSuccess
          && hipMemcpy(h_info.data(), d_info, slots * sizeof(int32_t), hipMemcpyDeviceToHost) == hipSuccess && hipMemcpy(h_span.data(), d_span, slots * sizeof(int32_t), hipMemcpyDeviceToHost) == hipSuccess
          && hipMemcpy(h_v.data(), d_v, slots * sizeof(double), hipMemcpyDeviceToHost) == hipSuccess && hipMemcpy(h_fl.data(), d_fl, slots * sizeof(double), hipMemcpyDeviceToHost) == hipSuccess
          && hipMemcpy(seg_i + (size_t)k * segs * 8, d_seg_i, segs * 8 * sizeof(int32_t), hipMemcpyDeviceToHost) == hipSuccess
          && hipMemcpy(seg_d + (size_t)k * segs * 2, d_seg_d, segs * 2 * sizeof(double), hipMemcpyDeviceToHost) == hipSuccess
          && hipMemcpy(seg_count + (size_t)k * n_clips, d_seg_count, (size_t)n_clips * sizeof(uint32_t), hipMemcpyDeviceToHost) == hipSuccess
          && hipMemcpy(state + (size_t)k * n_clips * GATE_STATE, d_state, (size_t)n_clips * GATE_STATE * sizeof(double), hipMemcpyDeviceToHost) == hipSuccess;
        if (!ok) break;
        flags2[0] |= cnt[1]; if (cnt[4] > flags2[1]) flags2[1] = cnt[4];
        for (uint32_t i = 0; i < n_clips; i++) {
            // the stream's frame count after this step (state word 0) minus the step's frames = the absolute number of the step's first frame
            const uint32_t seen = (uint32_t)state[((size_t)k * n_clips + i) * GATE_STATE] - nf[i];
            for (uint32_t j = 0; j < nf[i]; j++) {
                const size_t slot = (size_t)i * ring + ((seen + j) & (ring - 1)), dst = (size_t)foff[i] + fed[i] + j;
                fr_info[dst] = h_info[slot]; fr_span[dst] = h_span[slot]; fr_v[dst] = h_v[slot]; fr_fl[dst] = h_fl[slot];
            }
            fed[i] += nf[i];
        }
    }
    return ok ? WSA_OK : WSA_ERR_HIP;
}

// K6b / K6b-e (csrc/classify_fold.hpp) on their own: hand-built row meta [n_rows][8] i32 (slot 0 the clip or stream, 1 si, 3 t_len) and, per member
// d of n_members, a legend of C[d] strings and confidences conf[d] [n_rows][C[d]] (float, or double with f64 set) straight into the product's fold
// launches (classify_internal.hpp launch_*); no audio, no model.  key_rank comes from the legend through array_index_key.
//   n_steps == 0, a batch of n clips, row_off [n + 1]: single set (one member) runs fold_kernel<float / double> + fold_compact_kernel, else
//   fold_group_kernel + fold_compact_group_kernel (float only).  Out: n_cb [1]; cb [cb_cap][4]; per member cb_label, cb_conf [cb_cap], run_conf
//   [n][C[d]]; for the group also cb_all_max per member, cb_db, cb_top_label, cb_top_conf, cb_min_db, cb_entropy [cb_cap] and run_min_db [n].
//   n_steps > 0, n streams: tables, row_off [n_steps][n + 1] and ctl [n_steps][n] as wsa_debug_regress_fold; one launch_stream_classes /
//   launch_stream_knn (single) or launch_stream_ensemble per step, the carried folds (and the group's max_inv / min_db) zeroed at entry and kept
//   on the device between steps.  Out: n_cb [n_steps]; the steps' callbacks one after the other in the cb* tables; run_conf [n_steps][n][C[d]] and
//   run_min_db [n_steps][n] as each step leaves them; h_* [n_steps][max(cap, 1)]: what the step wrote to its D2H window of `cap` callbacks
//   (plain device buffers here).
// Every output table goes to the device as the caller filled it and comes back whole: a slot no callback fills keeps the caller's value.
// Refused, nothing run and nothing written: whatever would make a kernel read or write outside these tables — offsets out of order, a row filed
// under another clip, a negative si, t_len negative or INT32_MAX, more callbacks than cb_cap, a stream's callback whose rows continue in the next
// step, class or member counts past the library's limits.
struct wsa_debug_fold_io {
    const int32_t* meta; const uint32_t* row_off; const uint8_t* ctl;
    double step_s;
    uint32_t n_rows, n, n_steps, cap, n_members, cb_cap; int32_t single, f64;
    uint32_t C[WSA_ENSEMBLE_MAX];
    const char* const* legend[WSA_ENSEMBLE_MAX];
    const void* conf[WSA_ENSEMBLE_MAX];
    uint32_t* n_cb; int32_t* cb;
    int32_t* cb_label[WSA_ENSEMBLE_MAX]; double* cb_conf[WSA_ENSEMBLE_MAX]; double* cb_all_max[WSA_ENSEMBLE_MAX]; double* run_conf[WSA_ENSEMBLE_MAX];
    int32_t* cb_db; int32_t* cb_top_label; double* cb_top_conf; int32_t* cb_min_db; double* cb_entropy; int32_t* run_min_db;
    int32_t* h_cb; int32_t* h_cb_label[WSA_ENSEMBLE_MAX]; double* h_cb_conf[WSA_ENSEMBLE_MAX]; double* h_cb_all_max[WSA_ENSEMBLE_MAX];
    int32_t* h_cb_db; int32_t* h_cb_top_label; double* h_cb_top_conf; int32_t* h_cb_min_db; double* h_cb_entropy;
};

namespace {
// a device table holding the caller's `count` entries (one entry at least), and its way back
template <typename T>
bool fold_up(wsa::DevArena& A, T** d, const T* h, size_t count) {
    return A.alloc(d, count) && (!count || hipMemcpy(*d, h, count * sizeof(T), hipMemcpyHostToDevice) == hipSuccess);
}
template <typename T>
bool fold_down(T* h, const T* d, size_t count) { return !count || hipMemcpy(h, d, count * sizeof(T), hipMemcpyDeviceToHost) == hipSuccess; }
}  // namespace

extern "C" int wsa_debug_class_fold(int32_t device, const wsa_debug_fold_io* io) {
    using namespace wsa_classify;
    if (!io || !io->row_off || !io->n_cb || !io->cb) return WSA_ERR_INVALID;
    const uint32_t n = io->n, n_rows = io->n_rows, n_steps = io->n_steps, M = io->n_members;
    if ((n_rows && !io->meta) || M < 1 || M > WSA_ENSEMBLE_MAX || n < 1 || n > (1u << 16) || n_rows > (1u << 22) || io->cb_cap < 1 || io->cb_cap > (1u << 22)) return WSA_ERR_INVALID;
    if (n_steps > (1u << 12) || (n_steps && !io->ctl) || io->cap > (1u << 22)) return WSA_ERR_INVALID;
    const bool single = io->single != 0, f64 = io->f64 != 0, streams = n_steps != 0;
    if (single ? M != 1 : f64) return WSA_ERR_INVALID;                  // double confidences are the single fold's (KN-2)
    const size_t W = io->cap ? io->cap : 1;
    if (streams && (uint64_t)n_steps * W > (1u << 24)) return WSA_ERR_INVALID;
    for (uint32_t d = 0; d < M; d++) {
        if (io->C[d] < 1 || io->C[d] > WSA_MODEL_MAX_CLASSES || !io->legend[d] || (n_rows && !io->conf[d])) return WSA_ERR_INVALID;
        for (uint32_t c = 0; c < io->C[d]; c++) if (!io->legend[d][c]) return WSA_ERR_INVALID;
        if (!io->cb_label[d] || !io->cb_conf[d] || !io->run_conf[d] || (!single && !io->cb_all_max[d])) return WSA_ERR_INVALID;
        if (streams && (!io->h_cb_label[d] || !io->h_cb_conf[d] || (!single && !io->h_cb_all_max[d]))) return WSA_ERR_INVALID;
    }
    if (!single && (!io->cb_db || !io->cb_top_label || !io->cb_top_conf || !io->cb_min_db || !io->cb_entropy || !io->run_min_db)) return WSA_ERR_INVALID;
    if (streams && (!io->h_cb || (!single && (!io->h_cb_db || !io->h_cb_top_label || !io->h_cb_top_conf || !io->h_cb_min_db || !io->h_cb_entropy)))) return WSA_ERR_INVALID;
    const uint32_t tables = streams ? n_steps : 1;
    uint64_t rows = 0, callbacks = 0;
    std::vector<uint64_t> step_cb0(tables + 1, 0), step_row0(tables + 1, 0);
    std::vector<int64_t> last_si(n, -1);                                // the si a stream's rows ended on in an earlier step of its launch; -1: none
    for (uint32_t k = 0; k < tables; k++) {                             // every table: offsets in order, rows of their own clip / stream; callbacks counted
        const uint32_t* off = io->row_off + (size_t)k * (n + 1);
        if (off[0] != 0) return WSA_ERR_INVALID;
        for (uint32_t c = 0; c < n; c++) if (off[c + 1] < off[c]) return WSA_ERR_INVALID;
        if (rows + off[n] > n_rows) return WSA_ERR_INVALID;
        for (uint32_t c = 0; c < n; c++) {
            if (streams && (io->ctl[(size_t)k * n + c] & WSA_STREAM_START)) last_si[c] = -1;
            for (uint32_t r = off[c]; r < off[c + 1]; r++) {
                const int32_t* m = io->meta + (rows + r) * 8;
                if (m[0] != (int32_t)c || m[1] < 0 || m[3] < 0 || m[3] == 0x7fffffff) return WSA_ERR_INVALID;
                if (r == off[c] && (int64_t)m[1] == last_si[c]) return WSA_ERR_INVALID;       // a callback's rows split across steps
                callbacks += (r == off[c] || m[1] != m[1 - 8]) ? 1 : 0;
            }
            if (streams && off[c + 1] > off[c]) last_si[c] = io->meta[(rows + off[c + 1] - 1) * 8 + 1];
        }
        rows += off[n];
        step_cb0[k + 1] = callbacks; step_row0[k + 1] = rows;
    }
    if (rows != n_rows || callbacks > io->cb_cap) return WSA_ERR_INVALID;
    if (hipSetDevice(device) != hipSuccess) return WSA_ERR_NO_DEVICE;

    wsa::DevArena A;
    const size_t R = n_rows ? n_rows : 1, K = io->cb_cap, HW = (size_t)n_steps * W;
    int32_t *d_meta = nullptr, *d_cb = nullptr, *d_t_n = nullptr, *d_t_local = nullptr;
    uint32_t *d_off = nullptr, *d_bits = nullptr, *d_clip_cb = nullptr, *d_cb_off = nullptr, *d_count = nullptr;
    std::vector<uint32_t> bits((size_t)tables * n, 0u);
    for (size_t i = 0; streams && i < bits.size(); i++) bits[i] = (io->ctl[i] & WSA_STREAM_START) ? 1u : 0u;      // the device control word's bit 0
    bool ok = fold_up(A, &d_meta, io->meta, (size_t)n_rows * 8) && fold_up(A, &d_off, io->row_off, (size_t)tables * (n + 1)) && A.upload(&d_bits, bits)
           && fold_up(A, &d_cb, (const int32_t*)io->cb, K * 4) && A.alloc(&d_t_n, R) && A.alloc(&d_t_local, R) && A.alloc(&d_clip_cb, (size_t)n)
           && A.alloc(&d_cb_off, (size_t)n) && A.alloc(&d_count, 1, true);
    // per member: confidences, key_rank, the callback tables, the running sums
    const void* d_conf[WSA_ENSEMBLE_MAX] = {}; int64_t* d_kr[WSA_ENSEMBLE_MAX] = {};
    int32_t* d_cb_label[WSA_ENSEMBLE_MAX] = {}; double *d_cb_conf[WSA_ENSEMBLE_MAX] = {}, *d_cb_all_max[WSA_ENSEMBLE_MAX] = {}, *d_run[WSA_ENSEMBLE_MAX] = {};
    for (uint32_t d = 0; ok && d < M; d++) {
        const size_t Cd = io->C[d];
        std::vector<int64_t> kr(Cd, -1);
        for (size_t c = 0; c < Cd; c++) { int64_t v; if (array_index_key(io->legend[d][c], &v)) kr[c] = v; }
        if (f64) { double* p = nullptr; ok = fold_up(A, &p, (const double*)io->conf[d], (size_t)n_rows * Cd); d_conf[d] = p; }
        else { float* p = nullptr; ok = fold_up(A, &p, (const float*)io->conf[d], (size_t)n_rows * Cd); d_conf[d] = p; }
        ok = ok && A.upload(&d_kr[d], kr) && fold_up(A, &d_cb_label[d], (const int32_t*)io->cb_label[d], K) && fold_up(A, &d_cb_conf[d], (const double*)io->cb_conf[d], K)
             && A.alloc(&d_run[d], (size_t)n * Cd);
        if (ok && !single) ok = fold_up(A, &d_cb_all_max[d], (const double*)io->cb_all_max[d], K);
    }
    EnsTables o{};                                                      // the group's decision per callback; clip_min_db per clip (streams: the step's pinned column)
    if (ok && !single)
        ok = fold_up(A, &o.cb_db, (const int32_t*)io->cb_db, K) && fold_up(A, &o.cb_top_label, (const int32_t*)io->cb_top_label, K)
             && fold_up(A, &o.cb_top_conf, (const double*)io->cb_top_conf, K) && fold_up(A, &o.cb_min_db, (const int32_t*)io->cb_min_db, K)
             && fold_up(A, &o.cb_entropy, (const double*)io->cb_entropy, K) && fold_up(A, &o.clip_min_db, (const int32_t*)io->run_min_db, (size_t)n);
    o.cb = d_cb;
    if (!ok) return WSA_ERR_HIP;

    if (!streams) {
        if (single) {
            int32_t* d_t_label = nullptr; double* d_t_conf = nullptr;
            ok = A.alloc(&d_t_label, R) && A.alloc(&d_t_conf, R);
            if (ok && f64) {
                FoldParams<double> f{n, io->C[0], io->step_s, d_meta, d_off, (const double*)d_conf[0], d_kr[0], d_t_label, d_t_conf, d_t_n, d_t_local, d_clip_cb, d_run[0]};
                launch_fold(f, d_cb_off, d_cb, d_cb_label[0], d_cb_conf[0], d_count, nullptr);
            } else if (ok) {
                FoldParams<float> f{n, io->C[0], io->step_s, d_meta, d_off, (const float*)d_conf[0], d_kr[0], d_t_label, d_t_conf, d_t_n, d_t_local, d_clip_cb, d_run[0]};
                launch_fold(f, d_cb_off, d_cb, d_cb_label[0], d_cb_conf[0], d_count, nullptr);
            }
        } else {
            std::vector<FoldMember> ftab(M);
            EnsTables t{};
            ok = alloc_ens_tables(A, t, R, 0, true);
            t.clip_min_db = o.clip_min_db;
            for (uint32_t d = 0; ok && d < M; d++) {
                FoldMember& m = ftab[d];
                m = FoldMember{};
                m.C = io->C[d]; m.prob = (const float*)d_conf[d]; m.key_rank = d_kr[d];
                ok = A.alloc(&m.t_label, R) && A.alloc(&m.t_conf, R) && A.alloc(&m.t_all_max, R);
                m.clip_conf = d_run[d]; m.cb_label = d_cb_label[d]; m.cb_conf = d_cb_conf[d]; m.cb_all_max = d_cb_all_max[d];
            }
            FoldMember* d_ftab = nullptr;
            ok = ok && A.upload(&d_ftab, ftab);
            if (ok) {
                FoldGroupParams f{};
                f.n_clips = n; f.n_members = M; f.step_s = io->step_s; f.meta = d_meta; f.row_off = d_off; f.tab = d_ftab;
                f.t_n = d_t_n; f.t_local = d_t_local; f.clip_cb = d_clip_cb; f.t = t;
                launch_fold_group(f, d_cb_off, o, d_count, nullptr);
            }
        }
        ok = ok && hipGetLastError() == hipSuccess && hipDeviceSynchronize() == hipSuccess && fold_down(io->n_cb, d_count, 1);
        for (uint32_t d = 0; ok && d < M; d++) ok = fold_down(io->run_conf[d], d_run[d], (size_t)n * io->C[d]);
        if (ok && !single) ok = fold_down(io->run_min_db, o.clip_min_db, (size_t)n);
    } else {
        // the carried state, zeroed (min_db: -1), and the steps' D2H windows one after the other
        CarriedFold carried[WSA_ENSEMBLE_MAX] = {};
        int32_t *d_h_cb = nullptr, *d_h_cb_label[WSA_ENSEMBLE_MAX] = {}, *d_h_min = nullptr, *d_min_db = nullptr;
        double *d_h_cb_conf[WSA_ENSEMBLE_MAX] = {}, *d_h_cb_all_max[WSA_ENSEMBLE_MAX] = {}, *d_seg[WSA_ENSEMBLE_MAX] = {}, *d_sum[WSA_ENSEMBLE_MAX] = {}, *d_max_inv = nullptr;
        float* d_h_prob[WSA_ENSEMBLE_MAX] = {};
        EnsTables h{};
        ok = fold_up(A, &d_h_cb, (const int32_t*)io->h_cb, HW * 4);
        for (uint32_t d = 0; ok && d < M; d++) {
            const size_t Cd = io->C[d];
            ok = A.alloc(&carried[d].acc_all, (size_t)n * Cd, true) && A.alloc(&carried[d].in_all, (size_t)n * Cd, true) && A.alloc(&carried[d].first, (size_t)n * Cd, true)
                 && A.alloc(&carried[d].stamp, (size_t)n, true) && fold_up(A, &d_h_cb_label[d], (const int32_t*)io->h_cb_label[d], HW)
                 && fold_up(A, &d_h_cb_conf[d], (const double*)io->h_cb_conf[d], HW) && A.alloc(&d_h_prob[d], W * Cd);
            if (ok && !single) ok = fold_up(A, &d_h_cb_all_max[d], (const double*)io->h_cb_all_max[d], HW) && A.alloc(&d_seg[d], K) && A.alloc(&d_sum[d], K);
        }
        if (ok && !single)
            ok = fold_up(A, &h.cb_db, (const int32_t*)io->h_cb_db, HW) && fold_up(A, &h.cb_top_label, (const int32_t*)io->h_cb_top_label, HW)
                 && fold_up(A, &h.cb_top_conf, (const double*)io->h_cb_top_conf, HW) && fold_up(A, &h.cb_min_db, (const int32_t*)io->h_cb_min_db, HW)
                 && fold_up(A, &h.cb_entropy, (const double*)io->h_cb_entropy, HW) && A.alloc(&d_h_min, (size_t)n) && A.alloc(&d_max_inv, (size_t)n, true)
                 && A.alloc(&d_min_db, (size_t)n) && hipMemset(d_min_db, 0xff, (size_t)n * sizeof(int32_t)) == hipSuccess;
        // the KNN step kernel also pushes its rows' labels (one per row) and neighbours (k per row; none here)
        int32_t *d_klabel = nullptr, *d_h_klabel = nullptr; double* d_h_kconf = nullptr;
        if (ok && f64) ok = A.alloc(&d_klabel, R, true) && A.alloc(&d_h_klabel, W) && A.alloc(&d_h_kconf, W * io->C[0]);
        // the members' tables of every step (a step's callbacks sit behind the earlier steps')
        FoldMember* d_ftab = nullptr; StreamMember* d_stab = nullptr;
        if (ok && !single) {
            std::vector<FoldMember> ftab((size_t)n_steps * M);
            std::vector<StreamMember> stab((size_t)n_steps * M);
            for (uint32_t k = 0; k < n_steps; k++)
                for (uint32_t d = 0; d < M; d++) {
                    const size_t cb0 = step_cb0[k], hw0 = (size_t)k * W;
                    FoldMember& m = ftab[(size_t)k * M + d];
                    m = FoldMember{};
                    m.C = io->C[d]; m.prob = (const float*)d_conf[d] + step_row0[k] * io->C[d]; m.key_rank = d_kr[d];
                    m.t_label = d_cb_label[d] + cb0; m.t_conf = d_cb_conf[d] + cb0; m.t_all_max = d_cb_all_max[d] + cb0; m.t_seg = d_seg[d] + cb0; m.t_all_sum = d_sum[d] + cb0;
                    m.cb_label = m.t_label; m.cb_conf = m.t_conf; m.cb_all_max = m.t_all_max;
                    stab[(size_t)k * M + d] = StreamMember{carried[d], d_h_prob[d], d_h_cb_label[d] + hw0, d_h_cb_conf[d] + hw0, d_h_cb_all_max[d] + hw0, d_run[d]};
                }
            ok = A.upload(&d_ftab, ftab) && A.upload(&d_stab, stab);
        }
        for (uint32_t k = 0; ok && k < n_steps; k++) {
            const size_t row0 = step_row0[k], cb0 = step_cb0[k], hw0 = (size_t)k * W;
            const uint32_t* off = d_off + (size_t)k * (n + 1);
            const uint32_t* bk = d_bits + (size_t)k * n;
            if (single) {
                const StepFoldTables t{io->cap, d_cb + cb0 * 4, d_cb_label[0] + cb0, d_cb_conf[0] + cb0, d_h_cb + hw0 * 4, d_h_cb_label[0] + hw0, d_h_cb_conf[0] + hw0, d_run[0], d_count};
                if (f64) {
                    StreamKnnParams p{};
                    p.n = n; p.C = io->C[0]; p.k = 0; p.fold = 1; p.step_s = io->step_s; p.meta = d_meta + row0 * 8; p.row_off = off; p.bits = bk; p.key_rank = d_kr[0];
                    p.label = d_klabel; p.conf = (const double*)d_conf[0] + row0 * io->C[0]; p.carried = carried[0]; p.t = t;
                    p.h_label = d_h_klabel; p.h_conf = d_h_kconf;
                    launch_stream_knn(p, nullptr);
                } else {
                    StreamClsParams p{};
                    p.n = n; p.C = io->C[0]; p.fold = 1; p.step_s = io->step_s; p.meta = d_meta + row0 * 8; p.row_off = off; p.prob = (const float*)d_conf[0] + row0 * io->C[0];
                    p.key_rank = d_kr[0]; p.bits = bk; p.carried = carried[0]; p.t = t; p.h_prob = d_h_prob[0];
                    launch_stream_classes(p, nullptr);
                }
            } else {
                StreamEnsParams p{};
                p.n = n; p.n_members = M; p.cap = io->cap; p.fold = 1; p.step_s = io->step_s; p.meta = d_meta + row0 * 8; p.row_off = off; p.bits = bk;
                p.tab = d_ftab + (size_t)k * M; p.stab = d_stab + (size_t)k * M;
                p.o = EnsTables{d_cb + cb0 * 4, o.cb_db + cb0, o.cb_top_label + cb0, o.cb_top_conf + cb0, o.cb_min_db + cb0, o.cb_entropy + cb0, nullptr};
                p.h = EnsTables{d_h_cb + hw0 * 4, h.cb_db + hw0, h.cb_top_label + hw0, h.cb_top_conf + hw0, h.cb_min_db + hw0, h.cb_entropy + hw0, d_h_min};
                p.max_inv = d_max_inv; p.min_db = d_min_db; p.h_count = d_count;
                launch_stream_ensemble(p, nullptr);
            }
            ok = hipGetLastError() == hipSuccess && hipDeviceSynchronize() == hipSuccess && fold_down(io->n_cb + k, d_count, 1);
            for (uint32_t d = 0; ok && d < M; d++) ok = fold_down(io->run_conf[d] + (size_t)k * n * io->C[d], d_run[d], (size_t)n * io->C[d]);
            if (ok && !single) ok = fold_down(io->run_min_db + (size_t)k * n, d_h_min, (size_t)n);
        }
        ok = ok && fold_down(io->h_cb, d_h_cb, HW * 4);
        for (uint32_t d = 0; ok && d < M; d++) {
            ok = fold_down(io->h_cb_label[d], d_h_cb_label[d], HW) && fold_down(io->h_cb_conf[d], d_h_cb_conf[d], HW);
            if (ok && !single) ok = fold_down(io->h_cb_all_max[d], d_h_cb_all_max[d], HW);
        }
        if (ok && !single)
            ok = fold_down(io->h_cb_db, h.cb_db, HW) && fold_down(io->h_cb_top_label, h.cb_top_label, HW) && fold_down(io->h_cb_top_conf, h.cb_top_conf, HW)
                 && fold_down(io->h_cb_min_db, h.cb_min_db, HW) && fold_down(io->h_cb_entropy, h.cb_entropy, HW);
    }
    ok = ok && fold_down(io->cb, d_cb, K * 4);
    for (uint32_t d = 0; ok && d < M; d++) {
        ok = fold_down(io->cb_label[d], d_cb_label[d], K) && fold_down(io->cb_conf[d], d_cb_conf[d], K);
        if (ok && !single) ok = fold_down(io->cb_all_max[d], d_cb_all_max[d], K);
    }
    if (ok && !single)
        ok = fold_down(io->cb_db, o.cb_db, K) && fold_down(io->cb_top_label, o.cb_top_label, K) && fold_down(io->cb_top_conf, o.cb_top_conf, K)
             && fold_down(io->cb_min_db, o.cb_min_db, K) && fold_down(io->cb_entropy, o.cb_entropy, K);
    return ok ? WSA_OK : WSA_ERR_HIP;
}

// PK-2's kernel (csrc/batch_pcm.hip) on its own: host-given packed bytes through ONE launch of batch_unpack_kernel, floats back.  off [n_clips + 1]:
// clip i's bytes start at packed + off[i] (a multiple of 16) and lie in front of off[i + 1]; off[n_clips] = the bytes of `packed`.  out [n_clips][stride]
// goes to the device as the caller filled it and comes back: what the kernel did not write keeps the caller's value.
// Refused, nothing run: an unknown format, channels outside 1 .. 64, an offset that is no multiple of 16, a clip whose frames do not fit between its
// offset and the next or into a row of `stride` floats.
extern "C" int wsa_debug_batch_unpack(int32_t device, const void* packed, const uint64_t* off, const int32_t* formats, const uint32_t* channels,
                                      const uint32_t* n_frames, uint32_t n_clips, float* out, uint64_t stride) {
    if (!off || !formats || !channels || !n_frames || !out || n_clips < 1 || n_clips > 65535u || stride < 1 || stride > (1u << 26)) return WSA_ERR_INVALID;
    if (off[0] != 0 || off[n_clips] > (1ull << 32) || (off[n_clips] && !packed)) return WSA_ERR_INVALID;
    std::vector<wsa::PcmClipDesc> desc(n_clips);
    uint32_t max_frames = 0;
    for (uint32_t i = 0; i < n_clips; i++) {
        if (!wsa::pcm_format_known(formats[i]) || channels[i] < 1 || channels[i] > 64 || (off[i] & 15u) || off[i + 1] < off[i] || n_frames[i] > stride) return WSA_ERR_INVALID;
        const uint64_t need = n_frames[i] ? ((uint64_t)(n_frames[i] - 1u) * channels[i] + 1u) * wsa::pcm_sample_bytes(formats[i]) : 0;   // up to channel 0 of the last frame
        if (need > off[i + 1] - off[i]) return WSA_ERR_INVALID;
        desc[i] = wsa::PcmClipDesc{off[i], formats[i], channels[i], n_frames[i], 0, 0, 0};
        if (n_frames[i] > max_frames) max_frames = n_frames[i];
    }
    if (hipSetDevice(device) != hipSuccess) return WSA_ERR_NO_DEVICE;
    wsa::DevArena A; uint4* dp = nullptr; wsa::PcmClipDesc* dd = nullptr; float* dout = nullptr;
    const size_t nout = (size_t)n_clips * stride;
    bool ok = A.alloc(&dp, (size_t)(off[n_clips] + 15u) / 16u) && A.upload(&dd, desc) && A.alloc(&dout, nout)
           && (off[n_clips] == 0 || hipMemcpy(dp, packed, (size_t)off[n_clips], hipMemcpyHostToDevice) == hipSuccess)
           && hipMemcpy(dout, out, nout * sizeof(float), hipMemcpyHostToDevice) == hipSuccess;
    if (ok) {
        wsa::launch_batch_unpack(dp, dd, n_clips, max_frames, dout, stride, nullptr);
        ok = hipGetLastError() == hipSuccess && hipDeviceSynchronize() == hipSuccess && hipMemcpy(out, dout, nout * sizeof(float), hipMemcpyDeviceToHost) == hipSuccess;
    }
    return ok ? WSA_OK : WSA_ERR_HIP;
}

// PK-3's kernel (csrc/pcm_channels.hip) on its own: host-given packed bytes through ONE launch of batch_deinterleave_kernel, floats back.  The plan is
// pcm_plan_channels', as the batch entries use it: off_out [n_clips + 1] comes back as planned (off_out[i]: where clip i's source starts), `packed` holds
// packed_bytes bytes laid out by it — call with out == NULL first to get the offsets alone.  out [n_clips][stride] (any stride >= the longest clip, multiples
// of four or not) goes to the device as the caller filled it and comes back: what the kernel did not write keeps the caller's value.  The device buffer is
// exactly packed_bytes long.  Refused, nothing run: what the plan refuses (its message goes to err [err_cap], the planning call needs no device), a clip
// longer than `stride`, fewer bytes than the plan needs.
extern "C" int wsa_debug_batch_deinterleave(int32_t device, const void* packed, uint64_t packed_bytes, const int32_t* formats, const uint32_t* channels,
                                            const uint32_t* select, const uint32_t* source, const uint32_t* n_frames, uint32_t n_clips, uint64_t* off_out,
                                            float* out, uint64_t stride, char* err, uint32_t err_cap) {
    if (err && err_cap) err[0] = 0;
    if (!formats || !n_frames || !off_out || n_clips < 1 || n_clips > 65535u) return WSA_ERR_INVALID;
    std::vector<wsa::PcmClipDesc> desc; std::vector<uint64_t> off;
    const std::string why = wsa::pcm_plan_channels(n_clips, n_frames, formats, channels, select, source, desc, off);
    if (!why.empty()) {
        if (err && err_cap) { const size_t k = std::min<size_t>(why.size(), err_cap - 1u); std::memcpy(err, why.data(), k); err[k] = 0; }
        return WSA_ERR_INVALID;
    }
    for (uint32_t i = 0; i <= n_clips; i++) off_out[i] = off[i];
    if (!out) return WSA_OK;
    if (stride < 1 || stride > (1u << 26) || off[n_clips] > (1ull << 32)) return WSA_ERR_INVALID;
    uint32_t max_frames = 0;
    uint64_t need = 0;                                             // the last byte any source's frames reach
    for (uint32_t i = 0; i < n_clips; i++) {
        if (n_frames[i] > stride) return WSA_ERR_INVALID;
        if (n_frames[i] > max_frames) max_frames = n_frames[i];
        if (desc[i].source == i) need = std::max<uint64_t>(need, desc[i].offset + (uint64_t)n_frames[i] * desc[i].channels * wsa::pcm_sample_bytes(desc[i].format));
    }
    if (need > packed_bytes || (packed_bytes && !packed)) return WSA_ERR_INVALID;
    if (hipSetDevice(device) != hipSuccess) return WSA_ERR_NO_DEVICE;
    wsa::DevArena A; uint8_t* dp = nullptr; wsa::PcmClipDesc* dd = nullptr; float* dout = nullptr;
    const size_t nout = (size_t)n_clips * stride;
    bool ok = A.alloc(&dp, (size_t)packed_bytes + 1) && A.upload(&dd, desc) && A.alloc(&dout, nout)
           && (packed_bytes == 0 || hipMemcpy(dp, packed, (size_t)packed_bytes, hipMemcpyHostToDevice) == hipSuccess)
           && hipMemcpy(dout, out, nout * sizeof(float), hipMemcpyHostToDevice) == hipSuccess;
    if (ok) {
        wsa::launch_batch_deinterleave(dp, dd, n_clips, max_frames, dout, stride, nullptr);
        ok = hipGetLastError() == hipSuccess && hipDeviceSynchronize() == hipSuccess && hipMemcpy(out, dout, nout * sizeof(float), hipMemcpyDeviceToHost) == hipSuccess;
    }
    return ok ? WSA_OK : WSA_ERR_HIP;
}

// K3 (csrc/tracker.hip: compact_count_kernel, compact_scan_kernel, compact_gather_kernel) on its own: hand-built segment tables and a hand-built row
// pool straight into launch_compact, which picks its form from n, fused, clip_rows and carry itself (path = what compact_path said it ran).
//   n_steps == 0, a batch of n clips: seg_i [n][seg_cap][8], seg_count [n], clip_rows [n] (or NULL: no fused form) — the per-clip row counters as the
//   tracker leaves them, which must equal the rows of the clip's reported segments.  counters [16] (word 1 is the flag word the fused form publishes), totals
//   [4] and hist [SPAN_BUCKETS] go to the device as the caller seeded them and come back as the run left them; give_clr hands counters and hist over as
//   clr_counters / clr_hist, give_host the four host words (mapped pinned memory, as the batch driver's).
//   n_steps > 0, n streams: seg_i [n_steps][n][seg_cap][8], seg_count and ctl [n_steps][n]; each step runs launch_stream_prepare (ctl bit 0 START clears the
//   stream's carry) and launch_compact with the carry, which starts as carry_in [n][CARRY_WORDS] (NULL: zeros) and stays on the device between steps.  The
//   seeded totals go up afresh before every step; carry [n_steps][n][CARRY_WORDS] comes back as each step left it.
// The pool (row_meta_in [pool][8], row_feat_in [pool][53]) is one for all steps.  Out, per step: seg_out [segs_cap][4], row_meta_out [rows_cap][8], row_feat_out
// [rows_cap][53], clip_row_off / clip_seg_off [n + 1], totals [4].  Every output table goes to the device as the caller filled it and comes back whole: a slot
// the kernels do not write keeps the caller's value.
// Refused, nothing run and nothing written: whatever would make a kernel index outside these tables — seg_count > seg_cap, SEG_ROW0 + SEG_NROWS past the
// pool, a negative SEG_NROWS or SEG_ROW0, more rows or segments in a step than rows_cap / segs_cap, clip_rows that differ from the rows reported, a carry whose
// counts are negative or that has counted more results than segments (the result index would then run ahead of the step's table), an unknown level.
struct wsa_debug_compact_io {
    const int32_t* seg_i; const uint32_t* seg_count; const uint32_t* ctl; const int32_t* row_meta_in; const double* row_feat_in; const uint32_t* clip_rows;
    const int32_t* carry_in;
    uint32_t n, seg_cap, pool, n_steps, rows_cap, segs_cap; int32_t level, fused, give_clr, give_host;
    int32_t* seg_out; int32_t* row_meta_out; double* row_feat_out; uint32_t* clip_row_off; uint32_t* clip_seg_off; uint32_t* totals;
    uint32_t* host4; uint32_t* counters; uint32_t* hist; int32_t* path; int32_t* carry;
};

extern "C" int wsa_debug_compact(int32_t device, const wsa_debug_compact_io* io) {
    using namespace wsa;
    if (!io || !io->seg_i || !io->seg_count || !io->seg_out || !io->row_meta_out || !io->row_feat_out || !io->clip_row_off || !io->clip_seg_off || !io->totals
        || !io->host4 || !io->counters || !io->hist || !io->path) return WSA_ERR_INVALID;
    const uint32_t n = io->n, n_steps = io->n_steps, pool = io->pool;
    const bool streams = n_steps != 0;
    if (n < 1 || n > (1u << 14) || io->seg_cap < 1 || io->seg_cap > (1u << 12) || pool > (1u << 20) || (pool && (!io->row_meta_in || !io->row_feat_in))) return WSA_ERR_INVALID;
    if (io->rows_cap < 1 || io->rows_cap > (1u << 20) || io->segs_cap < 1 || io->segs_cap > (1u << 20) || n_steps > (1u << 12)) return WSA_ERR_INVALID;
    if (io->level != 3 && io->level != 4 && io->level != 5 && io->level != 10 && io->level != 13) return WSA_ERR_INVALID;
    if (streams && (!io->ctl || !io->carry || io->clip_rows || io->give_clr || io->give_host)) return WSA_ERR_INVALID;        // the fused form is the batches'
    if (!streams && (io->carry_in || io->carry)) return WSA_ERR_INVALID;
    const uint32_t tables = streams ? n_steps : 1;
    const size_t seg_cap = io->seg_cap, segs = (size_t)n * seg_cap;
    std::vector<int64_t> seg_before(n, 0), res_before(n, 0);
    for (uint32_t c = 0; streams && io->carry_in && c < n; c++) {
        const int32_t* cy = io->carry_in + (size_t)c * CARRY_WORDS;
        if (cy[0] < 0 || cy[1] < 0 || cy[1] > cy[0]) return WSA_ERR_INVALID;
        seg_before[c] = cy[0]; res_before[c] = cy[1];
    }
    for (uint32_t k = 0; k < tables; k++) {
        uint64_t rows = 0, nsegs = 0;
        for (uint32_t c = 0; c < n; c++) {
            const uint32_t ns = io->seg_count[(size_t)k * n + c];
            if (ns > seg_cap) return WSA_ERR_INVALID;
            if (streams && (io->ctl[(size_t)k * n + c] & ~3u)) return WSA_ERR_INVALID;
            if (streams && (io->ctl[(size_t)k * n + c] & 1u)) { seg_before[c] = 0; res_before[c] = 0; }
            uint64_t clip_rows = 0, results = 0;
            for (uint32_t q = 0; q < ns; q++) {
                const int32_t* sg = io->seg_i + ((size_t)k * segs + (size_t)c * seg_cap + q) * 8;
                if (sg[SEG_NROWS] < 0 || sg[SEG_ROW0] < 0 || (uint64_t)sg[SEG_ROW0] + (uint64_t)sg[SEG_NROWS] > pool) return WSA_ERR_INVALID;
                if (sg[SEG_FLAG] >= 0) { clip_rows += (uint32_t)sg[SEG_NROWS]; results++; }
            }
            if (io->clip_rows && io->clip_rows[c] != clip_rows) return WSA_ERR_INVALID;
            seg_before[c] += ns; res_before[c] += (int64_t)results;
            if (seg_before[c] > (1 << 30)) return WSA_ERR_INVALID;
            rows += clip_rows; nsegs += ns;
        }
        if (rows > io->rows_cap || nsegs > io->segs_cap) return WSA_ERR_INVALID;
    }
    if (hipSetDevice(device) != hipSuccess) return WSA_ERR_NO_DEVICE;
    DevArena A;
    int32_t *d_seg_i = nullptr, *d_meta_in = nullptr, *d_seg_out = nullptr, *d_meta_out = nullptr, *d_carry = nullptr; double *d_feat_in = nullptr, *d_feat_out = nullptr, *d_state = nullptr;
    uint32_t *d_seg_count = nullptr, *d_clip_rows = nullptr, *d_ctl = nullptr, *d_row_off = nullptr, *d_seg_off = nullptr, *d_totals = nullptr, *d_counters = nullptr, *d_hist = nullptr;
    uint32_t *h_host = nullptr, *h_host_dev = nullptr;
    const size_t R = io->rows_cap, S = io->segs_cap;
    bool ok = A.alloc(&d_seg_i, segs * 8) && A.alloc(&d_seg_count, n) && fold_up(A, &d_meta_in, io->row_meta_in, (size_t)pool * 8) && fold_up(A, &d_feat_in, io->row_feat_in, (size_t)pool * WSA_NFEAT)
           && A.alloc(&d_seg_out, S * 4) && A.alloc(&d_meta_out, R * 8) && A.alloc(&d_feat_out, R * WSA_NFEAT) && A.alloc(&d_row_off, (size_t)n + 1) && A.alloc(&d_seg_off, (size_t)n + 1)
           && A.alloc(&d_totals, 4) && fold_up(A, &d_counters, io->counters, 16) && fold_up(A, &d_hist, io->hist, (size_t)SPAN_BUCKETS) && A.pin(&h_host, &h_host_dev, 4);
    if (ok && io->clip_rows) ok = fold_up(A, &d_clip_rows, io->clip_rows, n);
    if (ok && streams) {
        ok = A.alloc(&d_ctl, n) && A.alloc(&d_state, (size_t)n * GATE_STATE, true) && A.alloc(&d_carry, (size_t)n * CARRY_WORDS, true)
          && (!io->carry_in || hipMemcpy(d_carry, io->carry_in, (size_t)n * CARRY_WORDS * sizeof(int32_t), hipMemcpyHostToDevice) == hipSuccess);
    }
    if (!ok) return WSA_ERR_HIP;
    for (int q = 0; q < 4; q++) h_host[q] = io->host4[q];
    for (uint32_t k = 0; ok && k < tables; k++) {
        ok = hipMemcpy(d_seg_i, io->seg_i + (size_t)k * segs * 8, segs * 8 * sizeof(int32_t), hipMemcpyHostToDevice) == hipSuccess
          && hipMemcpy(d_seg_count, io->seg_count + (size_t)k * n, (size_t)n * sizeof(uint32_t), hipMemcpyHostToDevice) == hipSuccess
          && hipMemcpy(d_seg_out, io->seg_out + (size_t)k * S * 4, S * 4 * sizeof(int32_t), hipMemcpyHostToDevice) == hipSuccess
          && hipMemcpy(d_meta_out, io->row_meta_out + (size_t)k * R * 8, R * 8 * sizeof(int32_t), hipMemcpyHostToDevice) == hipSuccess
          && hipMemcpy(d_feat_out, io->row_feat_out + (size_t)k * R * WSA_NFEAT, R * WSA_NFEAT * sizeof(double), hipMemcpyHostToDevice) == hipSuccess
          && hipMemcpy(d_row_off, io->clip_row_off + (size_t)k * (n + 1), ((size_t)n + 1) * sizeof(uint32_t), hipMemcpyHostToDevice) == hipSuccess
          && hipMemcpy(d_seg_off, io->clip_seg_off + (size_t)k * (n + 1), ((size_t)n + 1) * sizeof(uint32_t), hipMemcpyHostToDevice) == hipSuccess
          && hipMemcpy(d_totals, io->totals + (size_t)k * 4, 4 * sizeof(uint32_t), hipMemcpyHostToDevice) == hipSuccess
          && (!streams || hipMemcpy(d_ctl, io->ctl + (size_t)k * n, (size_t)n * sizeof(uint32_t), hipMemcpyHostToDevice) == hipSuccess);
        if (!ok) break;
        CompactParams cp;
        cp.n_clips = n; cp.seg_cap = (int)seg_cap; cp.level = io->level; cp.seg_i = d_seg_i; cp.seg_count = d_seg_count; cp.row_meta_in = d_meta_in; cp.row_feat_in = d_feat_in;
        cp.seg_out = d_seg_out; cp.row_meta_out = d_meta_out; cp.row_feat_out = d_feat_out; cp.clip_row_off = d_row_off; cp.clip_seg_off = d_seg_off; cp.totals = d_totals;
        if (streams) {
            launch_stream_prepare(d_state, d_carry, nullptr, d_ctl, n, 0.0, 0.0, nullptr);
            cp.carry = d_carry; cp.ctl = d_ctl;
        } else {
            cp.clip_rows = d_clip_rows; cp.flags = d_counters + 1; cp.fused = io->fused ? 1 : 0; cp.host = io->give_host ? h_host_dev : nullptr;
            cp.clr_counters = io->give_clr ? d_counters : nullptr; cp.clr_hist = io->give_clr ? d_hist : nullptr;
        }
        io->path[k] = compact_path(cp);
        launch_compact(cp, nullptr);
        ok = hipGetLastError() == hipSuccess && hipDeviceSynchronize() == hipSuccess
          && fold_down(io->seg_out + (size_t)k * S * 4, d_seg_out, S * 4) && fold_down(io->row_meta_out + (size_t)k * R * 8, d_meta_out, R * 8)
          && fold_down(io->row_feat_out + (size_t)k * R * WSA_NFEAT, d_feat_out, R * WSA_NFEAT) && fold_down(io->clip_row_off + (size_t)k * (n + 1), d_row_off, (size_t)n + 1)
          && fold_down(io->clip_seg_off + (size_t)k * (n + 1), d_seg_off, (size_t)n + 1) && fold_down(io->totals + (size_t)k * 4, d_totals, 4)
          && (!streams || fold_down(io->carry + (size_t)k * n * CARRY_WORDS, d_carry, (size_t)n * CARRY_WORDS));
    }
    ok = ok && fold_down(io->counters, d_counters, 16) && fold_down(io->hist, d_hist, (size_t)SPAN_BUCKETS);
    if (ok) for (int q = 0; q < 4; q++) io->host4[q] = h_host[q];
    return ok ? WSA_OK : WSA_ERR_HIP;
}

// The span order on its own: wsa_debug_gate's batch form (variants 0 .. 2, `blocks`, the same settings6 and caps_io) with the gate's counting switched on
// — span_hist / span_key set as the batch driver sets them — and launch_span_order behind it.  Out: seg_i [n_clips][seg_cap][8], seg_count [n_clips], hist
// [SPAN_BUCKETS] (zero before the gate, as the batch's clear leaves it), key [n_clips][seg_cap][2] and order [n_clips * seg_cap][2] (both go to the device as
// the caller filled them: a slot nobody writes keeps its value), counters4 = counters[0 .. 3] as the driver hands them to launch_span_order.
// Refused, nothing run: what wsa_debug_gate refuses for a batch, and the stream variant.  One refusal comes AFTER the peak scan has run (as in wsa_debug_gate):
// a frame with more than CAND_CAP candidates, which only the scan finds — the gate and the span order are then not run, and nothing is written to the caller.
extern "C" int wsa_debug_span_order(int32_t device, int32_t variant, const uint32_t* spec, const uint32_t* n_frames, uint32_t n_clips, int32_t bands, const double* settings6,
                                    uint32_t blocks, int32_t* caps_io, int32_t* seg_i, uint32_t* seg_count, uint32_t* hist, uint32_t* key, uint32_t* order, uint32_t* counters4) {
    using namespace wsa;
    if (!n_frames || !settings6 || !caps_io || variant < 0 || variant > 2 || n_clips < 1 || n_clips > 4096 || bands < 4 || bands > 256) return WSA_ERR_INVALID;
    wsa_config c{};
    c.output_level = 5; c.N_mel_bins = bands; c.window_width = c.window_step = settings6[0]; c.pause_length = settings6[1]; c.min_seg_length = settings6[2];
    c.auto_noise_gate = settings6[3] != 0 ? 1 : 0; c.voiced_max_dB = settings6[4]; c.voiced_min_dB = settings6[5];
    if (!(c.window_step > 0) || !(c.pause_length >= 0) || !(c.min_seg_length >= 0)) return WSA_ERR_INVALID;
    if (variant < 2 && !c.auto_noise_gate) return WSA_ERR_INVALID;                     // the integer kernel's state is integers only under the auto gate
    uint64_t total = 0; uint32_t max_frames = 0;
    std::vector<uint32_t> foff((size_t)n_clips + 1, 0);
    for (uint32_t i = 0; i < n_clips; i++) {
        if (n_frames[i] > (1u << 20)) return WSA_ERR_INVALID;
        total += n_frames[i]; foff[i + 1] = (uint32_t)total; if (n_frames[i] > max_frames) max_frames = n_frames[i];
    }
    if (total > (1u << 22) || (total && !spec)) return WSA_ERR_INVALID;
    const Derived D(c, bands);
    const int seg_cap = batch_seg_cap(max_frames, D);
    if (caps_io[0] == 0) { caps_io[0] = seg_cap; return WSA_OK; }
    if (caps_io[0] != seg_cap || !seg_i || !seg_count || !hist || !key || !order || !counters4) return WSA_ERR_INVALID;
    if (hipSetDevice(device) != hipSuccess) return WSA_ERR_NO_DEVICE;
    const size_t segs = (size_t)n_clips * seg_cap;
    DevArena A;
    uint32_t *d_spec = nullptr, *d_nfr = nullptr, *d_foff = nullptr, *d_seg_count = nullptr, *d_clip_rows = nullptr, *d_counters = nullptr, *d_hist = nullptr, *d_key = nullptr, *d_order = nullptr;
    RecPtrs rec; int32_t *d_info = nullptr, *d_seg_i = nullptr; double *d_v = nullptr, *d_fl = nullptr, *d_seg_d = nullptr;
    bool ok = A.alloc(&d_spec, (size_t)total * bands + 4, true) && A.upload(&d_foff, foff) && fold_up(A, &d_nfr, n_frames, n_clips) && A.alloc(&rec.hdr, (size_t)total, true)
           && A.alloc(&rec.amp, (size_t)total * CAND_CAP, true) && A.alloc(&rec.ent, (size_t)total * CAND_CAP, true) && A.alloc(&d_info, (size_t)total, true) && A.alloc(&d_v, (size_t)total, true)
           && A.alloc(&d_fl, (size_t)total, true) && A.alloc(&d_seg_i, segs * 8, true) && A.alloc(&d_seg_d, segs * 2, true) && A.alloc(&d_seg_count, n_clips, true)
           && A.alloc(&d_clip_rows, n_clips, true) && A.alloc(&d_counters, 16, true) && A.alloc(&d_hist, (size_t)SPAN_BUCKETS, true)
           && fold_up(A, &d_key, key, segs * 2) && fold_up(A, &d_order, order, segs * 2)
           && (total == 0 || hipMemcpy(d_spec, spec, (size_t)total * bands * sizeof(uint32_t), hipMemcpyHostToDevice) == hipSuccess);
    if (!ok) return WSA_ERR_HIP;
    uint32_t cnt[16];
    if (total) {
        PkParams pk; pk.spec = d_spec; pk.rec = rec; pk.bands = bands; pk.flags = d_counters + 8; pk.total_frames = (uint32_t)total;
        launch_peaks(pk, nullptr);
        ok = hipGetLastError() == hipSuccess && hipDeviceSynchronize() == hipSuccess && hipMemcpy(cnt, d_counters, sizeof(cnt), hipMemcpyDeviceToHost) == hipSuccess;
        if (ok && (cnt[8] & 1u)) return WSA_ERR_INVALID;                                // a frame with more than CAND_CAP candidates: its table is cut short
        if (!ok) return WSA_ERR_HIP;
    }
    GateParams g;
    g.rec = rec; g.n_frames = d_nfr; g.frame_off = d_foff; g.n_clips = n_clips; g.level = D.klevel; g.max_voiced_bin = D.max_voiced_bin; g.breaker = D.breaker;
    g.min_frames = D.min_frames; g.auto_gate = D.auto_gate; g.ctx_max0 = D.ctx_max0; g.floor0 = D.floor0; g.fr_info = d_info; g.fr_v = d_v; g.fr_fl = d_fl;
    g.seg_i = d_seg_i; g.seg_d = d_seg_d; g.seg_cap = seg_cap; g.seg_count = d_seg_count; g.clip_rows = d_clip_rows; g.counters = d_counters + 4; g.shared = d_counters;
    g.dbg = variant == 1 ? DBG_GATE_GENERAL : (variant == 2 ? DBG_GATE_F64 : 0);
    g.span_hist = d_hist; g.span_key = reinterpret_cast<uint2*>(d_key);
    launch_gate_blocks(g, blocks, nullptr);
    TrParams t;
    t.n_clips = n_clips; t.seg_count = d_seg_count; t.seg_cap = seg_cap; t.seg_i = d_seg_i;
    launch_span_order(t, d_hist, reinterpret_cast<const uint2*>(d_key), reinterpret_cast<uint2*>(d_order), d_counters + 4, nullptr);
    ok = hipGetLastError() == hipSuccess && hipDeviceSynchronize() == hipSuccess && hipMemcpy(cnt, d_counters, sizeof(cnt), hipMemcpyDeviceToHost) == hipSuccess
      && fold_down(seg_i, d_seg_i, segs * 8) && fold_down(seg_count, d_seg_count, (size_t)n_clips) && fold_down(hist, d_hist, (size_t)SPAN_BUCKETS)
      && fold_down(key, d_key, segs * 2) && fold_down(order, d_order, segs * 2);
    if (ok) for (int q = 0; q < 4; q++) counters4[q] = cnt[4 + q];
    return ok ? WSA_OK : WSA_ERR_HIP;
}

// K6 / K6e (csrc/classify.hip) on hand-built rows through the product's own launches: cls_params / regress_params / launch_classify for one
// model, wsa_ensemble_create / group_table / launch_classify_group for 2 .. 8 (all of 53 inputs: an ensemble's rule).  No kernel code here.
//   feat [feat_rows][stride] f64 (host), stride >= the model's inputs; nan_slot -1, or a slot below stride (a row whose slot is not 0 gets NaN).
//   n_dev >= 0: the row count lives on the device (the batch and stream forms), n_rows is ignored; n_dev < 0: n_rows is the launch's own count
//   (one model only).  rows_cap sizes the grid, as the drivers' capacity does: it may be above or below the count.
//   rb 0: the model's own row-block factor; 1, 2, 4: that one (launch_classify keeps the model's when the LDS does not allow it).
//   one_block (groups): every member with one row block, as a stream step runs them.
//   regress != 0 (one model): the regression epilogue with out_min / out_max; out[0] is then [out_rows] f64, else out[d] is [out_rows][C_d] f32.
// Every out table goes to the device as the caller filled it and comes back whole: what no row writes keeps the caller's pattern.
// Refused, nothing run: a count above feat_rows or out_rows, and whatever else would make a kernel read or write outside these tables.
struct wsa_debug_classify_io {
    const wsa_model* const* models; uint32_t n_models;
    const double* feat; uint32_t feat_rows, stride; int32_t nan_slot;
    uint32_t n_rows, rows_cap; int32_t n_dev, rb, one_block, regress;
    double out_min, out_max;
    void* out[WSA_ENSEMBLE_MAX]; uint32_t out_rows;
};

extern "C" int wsa_debug_classify(const wsa_debug_classify_io* io) {
    using namespace wsa_classify;
    if (!io || !io->models || io->n_models < 1 || io->n_models > WSA_ENSEMBLE_MAX || !io->feat) return WSA_ERR_INVALID;
    const uint32_t M = io->n_models;
    for (uint32_t d = 0; d < M; d++) if (!io->models[d] || !io->out[d] || io->models[d]->ctx != io->models[0]->ctx) return WSA_ERR_INVALID;
    const wsa_model* m0 = io->models[0];
    wsa_ctx* ctx = m0->ctx;
    const bool group = M > 1, regress = io->regress != 0;
    const uint32_t n = io->n_dev >= 0 ? (uint32_t)io->n_dev : io->n_rows;
    if (io->feat_rows < 1 || io->feat_rows > (1u << 22) || io->out_rows < 1 || io->out_rows > (1u << 22) || io->rows_cap < 1 || io->rows_cap > (1u << 22)) return WSA_ERR_INVALID;
    if (n > io->feat_rows || n > io->out_rows || io->stride > 4096 || io->nan_slot >= (int32_t)io->stride) return WSA_ERR_INVALID;
    for (uint32_t d = 0; d < M; d++) if ((int)io->stride < io->models[d]->nin) return WSA_ERR_INVALID;
    if (io->rb != 0 && io->rb != 1 && io->rb != 2 && io->rb != 4) return WSA_ERR_INVALID;
    if (group && (io->n_dev < 0 || regress || io->rb != 0)) return WSA_ERR_INVALID;
    if (!group && io->one_block) return WSA_ERR_INVALID;
    if (regress) if (const char* why = regress_refusal(m0, io->out_min, io->out_max)) return wsa_api::fail(ctx, WSA_ERR_INVALID, why);
    if (hipSetDevice(ctx->device) != hipSuccess) return WSA_ERR_NO_DEVICE;
    wsa::DevArena A;
    double* d_feat = nullptr; uint32_t* d_n = nullptr; ClsGroupEntry* d_tab = nullptr;
    void* d_out[WSA_ENSEMBLE_MAX] = {};
    size_t out_bytes[WSA_ENSEMBLE_MAX] = {};
    const std::vector<uint32_t> count(1, n);
    bool ok = fold_up(A, &d_feat, io->feat, (size_t)io->feat_rows * io->stride) && A.upload(&d_n, count);
    for (uint32_t d = 0; d < M && ok; d++) {
        out_bytes[d] = regress ? (size_t)io->out_rows * sizeof(double) : (size_t)io->out_rows * io->models[d]->C * sizeof(float);
        char* q = nullptr;
        ok = fold_up(A, &q, static_cast<const char*>(io->out[d]), out_bytes[d]);
        d_out[d] = q;
    }
    if (!ok) return WSA_ERR_HIP;
    if (!group) {
        ClsParams p = cls_params(m0, d_feat, n, io->n_dev >= 0 ? d_n : nullptr, regress ? nullptr : static_cast<float*>(d_out[0]));
        p.stride = (int)io->stride; p.nan_slot = io->nan_slot;
        if (regress) p = regress_params(p, static_cast<double*>(d_out[0]), io->out_min, io->out_max - io->out_min);
        launch_classify(m0, p, io->rows_cap, nullptr, io->rb);
    } else {
        wsa_ensemble* e = nullptr;
        if (wsa_ensemble_create(ctx, io->models, M, &e) != WSA_OK) return WSA_ERR_INVALID;
        std::vector<ClsGroupEntry> tab;
        float* prob[WSA_ENSEMBLE_MAX] = {};
        for (uint32_t d = 0; d < M; d++) prob[d] = static_cast<float*>(d_out[d]);
        const uint32_t grid = group_table(e, d_feat, d_n, prob, io->rows_cap, io->one_block != 0, tab);
        for (ClsGroupEntry& t : tab) { t.p.stride = (int)io->stride; t.p.nan_slot = io->nan_slot; }
        const size_t lds = io->one_block ? e->lds_stream : e->lds_batch;
        ok = A.upload(&d_tab, tab);
        if (ok) launch_classify_group(d_tab, M, d_n, grid, lds, nullptr);
        wsa_ensemble_destroy(e);
        if (!ok) return WSA_ERR_HIP;
    }
    ok = hipGetLastError() == hipSuccess && hipDeviceSynchronize() == hipSuccess;
    for (uint32_t d = 0; d < M && ok; d++) ok = fold_down(static_cast<char*>(io->out[d]), static_cast<const char*>(d_out[d]), out_bytes[d]);
    return ok ? WSA_OK : WSA_ERR_HIP;
}

// K0 (csrc/resample.hip) on its own, no front end behind it: host clips in [n_clips][stride_in] through ONE form of the batch rate converter.
//   form 0: resample_kernel, every clip at fs_in[0] (all rates equal); S, J, chunks > 0 override the launch shape as WSA_RS_S / WSA_RS_J / WSA_RS_C do (0: default)
//        1: resample_mixed_kernel, one launch per rate class         2: the mixed kernel as one launch over the whole work list          (1, 2: no overrides)
// The device copy of `in` starts offset_bytes (0, 4, 8 or 12) behind a 16-byte boundary; every byte of that buffer outside the copy holds `fill`.
// out [n_clips][stride_out] goes to the device as the caller filled it and comes back as the kernel left it; n_out [n_clips] = resample_length per clip;
// plan [plan_cap][6] = per rate class {S, J, span, block, lds bytes, copy} in the classes' order (form 0: one class), shape3 = {classes, the block and the
// LDS bytes of form 2's launch (forms 0, 1: of the largest class)}.  The shape comes from resample_shape / plan_resample_mixed, the launches are
// launch_resample / launch_resample_mixed: the product's own.  Refused, nothing launched: an S outside 1 .. 512, a negative J or chunks, a launch whose
// LDS exceeds the device's limit per block, rates that are not positive and finite, a clip or its conversion longer than its row, too few plan rows.
extern "C" int wsa_debug_resample(int32_t device, const float* in, uint32_t n_clips, uint64_t stride_in, uint32_t offset_bytes, uint32_t fill, const uint32_t* n_in,
                                  const double* fs_in, double fs_out, int32_t form, int32_t S, int32_t J, int32_t chunks, float* out, uint64_t stride_out,
                                  uint32_t* n_out, int32_t* plan, uint32_t plan_cap, uint32_t* shape3) {
    using namespace wsa;
    if (!in || !n_in || !fs_in || !out || !n_out || !plan || !shape3 || n_clips < 1 || n_clips > (1u << 16) || form < 0 || form > 2) return WSA_ERR_INVALID;
    if ((offset_bytes & 3u) || offset_bytes > 12 || stride_in < 1 || stride_out < 1 || stride_in > (1ull << 28) || stride_out > (1ull << 28)) return WSA_ERR_INVALID;
    if (S < 0 || S > 512 || J < 0 || J > (1 << 16) || chunks < 0 || chunks > (1 << 16) || (form != 0 && (S || J || chunks))) return WSA_ERR_INVALID;
    if (!(fs_out > 0) || !std::isfinite(fs_out)) return WSA_ERR_INVALID;
    std::vector<uint32_t> len_in(n_in, n_in + n_clips), len_out(n_clips);
    uint64_t max_out = 0;
    for (uint32_t i = 0; i < n_clips; i++) {
        if (!(fs_in[i] > 0) || !std::isfinite(fs_in[i]) || (form == 0 && fs_in[i] != fs_in[0]) || n_in[i] > stride_in) return WSA_ERR_INVALID;
        const uint64_t n = resample_length(n_in[i], fs_in[i], fs_out);
        if (n > stride_out) return WSA_ERR_INVALID;
        len_out[i] = (uint32_t)n;
        if (n > max_out) max_out = n;
    }
    if (hipSetDevice(device) != hipSuccess) return WSA_ERR_NO_DEVICE;
    int lds_limit = 0;
    if (hipDeviceGetAttribute(&lds_limit, hipDeviceAttributeMaxSharedMemoryPerBlock, device) != hipSuccess) return WSA_ERR_HIP;
    RsParams r{}; RsMixedPlan P; std::string err;
    uint32_t n_cls = 1;
    if (form == 0) {
        resample_shape(fs_in[0], fs_out, S, J, chunks, r);
        if (resample_lds(r) > (size_t)lds_limit || (uint64_t)r.S * (uint64_t)r.J * (uint64_t)r.chunks > 0x7fffffffull) return WSA_ERR_INVALID;
        if (plan_cap < 1) return WSA_ERR_INVALID;
        const int32_t row[6] = {r.S, r.J, r.span, (int32_t)resample_block(r), (int32_t)resample_lds(r), 0};
        memcpy(plan, row, sizeof(row));
        shape3[0] = 1; shape3[1] = resample_block(r); shape3[2] = (uint32_t)resample_lds(r);
    } else {
        if (!plan_resample_mixed(n_clips, len_out.data(), fs_in, fs_out, P, err)) return WSA_ERR_INVALID;
        n_cls = (uint32_t)P.cls.size();
        if (P.max_lds > (uint32_t)lds_limit || P.max_block > 512 || plan_cap < n_cls) return WSA_ERR_INVALID;
        for (uint32_t c = 0; c < n_cls; c++) {
            const int32_t row[6] = {P.cls[c].S, P.cls[c].J, P.cls[c].span, (int32_t)P.block[c], (int32_t)P.lds[c], P.cls[c].copy};
            memcpy(plan + (size_t)c * 6, row, sizeof(row));
        }
        shape3[0] = n_cls; shape3[1] = P.max_block; shape3[2] = P.max_lds;
    }
    memcpy(n_out, len_out.data(), (size_t)n_clips * sizeof(uint32_t));
    const size_t words_in = (size_t)n_clips * stride_in, words_out = (size_t)n_clips * stride_out;
    std::vector<uint32_t> padded(words_in + 8, fill);                       // 4 words in front of the clips (the offset) and 4 behind
    const size_t first = offset_bytes / 4;
    memcpy(padded.data() + first, in, words_in * sizeof(float));
    DevArena A; uint32_t *d_in = nullptr, *d_nin = nullptr, *d_nout = nullptr, *d_clip_class = nullptr; float *d_out = nullptr, *d_table = nullptr;
    RsClass* d_cls = nullptr; RsWork* d_work = nullptr;
    bool ok = A.upload(&d_in, padded) && A.upload(&d_nin, len_in) && A.upload(&d_nout, len_out) && A.alloc(&d_out, words_out + 4)
           && hipMemcpy(d_out, out, words_out * sizeof(float), hipMemcpyHostToDevice) == hipSuccess;
    if (ok && form == 0) {
        std::vector<float> K0, K; build_resample_table(fs_in[0], fs_out, K0); resample_table_image(K0, K);
        ok = A.upload(&d_table, K);
    } else if (ok) {
        ok = A.upload(&d_table, P.tables) && A.upload(&d_cls, P.cls) && A.upload(&d_clip_class, P.clip_class) && A.upload(&d_work, P.work);
    }
    if (!ok) return WSA_ERR_HIP;
    const float* base = reinterpret_cast<const float*>(d_in) + first;
    if (form == 0) {
        r.in = base; r.stride_in = stride_in; r.out = d_out; r.stride_out = stride_out; r.n_in = d_nin; r.n_out = d_nout; r.table = d_table;
        launch_resample(r, n_clips, max_out, nullptr);
    } else {
        RsMixedParams m; m.in = base; m.stride_in = stride_in; m.out = d_out; m.stride_out = stride_out; m.n_in = d_nin; m.n_out = d_nout;
        m.tables = d_table; m.cls = d_cls; m.clip_class = d_clip_class; m.work = d_work;
        launch_resample_mixed(m, P, form == 1, nullptr);
    }
    ok = hipGetLastError() == hipSuccess && hipDeviceSynchronize() == hipSuccess && hipMemcpy(out, d_out, words_out * sizeof(float), hipMemcpyDeviceToHost) == hipSuccess;
    return ok ? WSA_OK : WSA_ERR_HIP;
}
