// api.hip — the part of include/wsa.h that needs no batch and no stream set: version, configuration, context, geometry, the tuning switches,
// page-locked host memory, queues and the host-side PCM helpers.  (Batches: batch_plan.hip, batch_run.hip, batch_input.hip, batch_results.hip;
// stream sets: stream_api.hip, stream_input.hip, stream_step.hip, stream_collect.hip.)
// Host-side mirror of the reference's module-level state (ref dist/main.js:2 inner module 1,
// @B2750-5843: config object, LaunchAudioNodes orchestration) for the batch use of the hot path.
#include <cstdlib>
#include <map>
#include <mutex>
#include "host_plan.hpp"
#include "pcm_formats.hpp"

using namespace wsa;

thread_local std::string wsa_api::g_create_error;
using wsa_api::fail;

namespace wsa {
Tuning Tuning::from_env() {
    Tuning t;
    // A library that a host process embeds does not listen to the environment: the switches below (tuning experiments and the equivalence tests'
    // hooks; tools/README.md) are read only when WSA_TUNING_ENV=1 says so — tests/conftest.py and the tools/ scripts set it.
    { const char* on = std::getenv("WSA_TUNING_ENV"); if (!on || on[0] != '1') return t; }
    auto num = [](const char* name, int dflt) { const char* e = std::getenv(name); return e && *e ? std::atoi(e) : dflt; };
    t.dbg = num("WSA_DBG", 0);
    t.no_pair = std::getenv("WSA_NO_PAIR") != nullptr; t.no_split = std::getenv("WSA_NO_SPLIT") != nullptr; t.no_quad = std::getenv("WSA_NO_QUAD") != nullptr; t.quad = std::getenv("WSA_QUAD") != nullptr; t.no_fuse = std::getenv("WSA_NO_FUSE") != nullptr;
    t.fe_fat = std::getenv("WSA_FE_FAT") != nullptr; t.peaks_lanes = std::getenv("WSA_PEAKS_LANES") != nullptr;
    t.full_table = num("WSA_FULL_TABLE", -1);
    t.tracker_wpc = num("WSA_TRACKER_WPC", 0); t.fin_wpc = num("WSA_FIN_WPC", 0); t.fpw = num("WSA_FPW", 0);
    t.fe_wg_per_cu = num("WSA_FE_WGS", 0); t.fe_no_queue = std::getenv("WSA_FE_NO_QUEUE") != nullptr; t.peaks_wpc = num("WSA_PEAKS_WPC", 0); t.peaks_w = num("WSA_PEAKS_W", 0); t.upload_threads = num("WSA_UPLOAD_THREADS", 0);
    t.rs_s = num("WSA_RS_S", 0); t.rs_j = num("WSA_RS_J", 0); t.rs_c = num("WSA_RS_C", 0); t.rs_one_launch = std::getenv("WSA_RS_ONE_LAUNCH") != nullptr;
    return t;
}
}  // namespace wsa

// The page-locked slabs wsa_host_alloc handed out (base -> bytes): upload_clips (batch_input.hip) merges copies only INSIDE one of them — two allocations that
// happen to be adjacent in the address space are still two registrations, and one copy across their seam is not something the runtime has to accept.
static std::mutex g_slab_mu;
static std::map<uintptr_t, size_t> g_slabs;
bool wsa_api::slab_of(const void* p, uintptr_t* base, size_t* size) {
    std::lock_guard<std::mutex> lk(g_slab_mu);
    auto it = g_slabs.upper_bound(reinterpret_cast<uintptr_t>(p));
    if (it == g_slabs.begin()) return false;
    --it;
    if (reinterpret_cast<uintptr_t>(p) >= it->first + it->second) return false;
    *base = it->first; *size = it->second;
    return true;
}

extern "C" {

int wsa_abi_version(void) { return WSA_ABI_VERSION; }

void wsa_config_default(wsa_config* c) {          // ref @B2965 (output_level 4 there as well: "Segment Formants")
    c->spec_type = 1; c->output_level = 4; c->f_min = 50; c->f_max = 4000; c->N_fft_bins = 256; c->N_mel_bins = 128;
    c->window_width = 25; c->window_step = 25; c->pause_length = 200; c->min_seg_length = 50; c->auto_noise_gate = 1;
    c->voiced_max_dB = 100; c->voiced_min_dB = 10; c->pre_norm_gain = 1000; c->high_f_emph = 0;
}

const char* wsa_last_error(const wsa_ctx* ctx) { return ctx ? ctx->err.c_str() : wsa_api::g_create_error.c_str(); }

wsa_status wsa_create(const wsa_config* cfg, int32_t device, wsa_ctx** out) {
    if (!cfg || !out) return fail(nullptr, WSA_ERR_INVALID, "null argument");
    *out = nullptr;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return fail(nullptr, WSA_ERR_NO_DEVICE, "no HIP device visible (libwsa has no CPU path)");
    if (device < 0 || device >= n) return fail(nullptr, WSA_ERR_INVALID, "device ordinal out of range");
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) != hipSuccess) return fail(nullptr, WSA_ERR_NO_DEVICE, "hipGetDeviceProperties failed");
    if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return fail(nullptr, WSA_ERR_NO_DEVICE, std::string("libwsa is built for gfx950 only; device is ") + prop.gcnArchName);
    const int lv = cfg->output_level;
    if (!(lv == 1 || lv == 2 || lv == 3 || lv == 4 || lv == 5 || lv == 10 || lv == 11 || lv == 12 || lv == 13))
        return fail(nullptr, WSA_ERR_INVALID, "output_level must be 1, 2 (spectrum frames only), 3, 4, 5, 10, 11, 12 or 13");
    if (!(cfg->window_step > 0) || !(cfg->window_width > 0)) return fail(nullptr, WSA_ERR_INVALID, "window_width / window_step must be positive");
    wsa_ctx* c = new wsa_ctx();
    c->cfg = *cfg; c->device = device; c->n_cu = prop.multiProcessorCount;
    *out = c;
    return WSA_OK;
}

void wsa_destroy(wsa_ctx* ctx) { delete ctx; }

wsa_status wsa_geometry_for(const wsa_ctx* ctx, double fs, wsa_geometry* out) {
    if (!ctx || !out) return WSA_ERR_INVALID;
    FePlanHost p; std::string err;
    if (!build_fe_plan(ctx->cfg, fs, p, err)) return fail(const_cast<wsa_ctx*>(ctx), WSA_ERR_INVALID, err);
    out->nfft = p.nfft; out->win = p.win; out->hop = p.hop; out->bands = p.bands; out->kmax = p.kmax;
    return WSA_OK;
}

wsa_status wsa_bins_hz(const wsa_ctx* ctx, double fs, double* out, int32_t n) {
    if (!ctx || !out) return WSA_ERR_INVALID;
    FePlanHost p; std::string err;
    if (!build_fe_plan(ctx->cfg, fs, p, err)) return fail(const_cast<wsa_ctx*>(ctx), WSA_ERR_INVALID, err);
    if (n < p.bands) return fail(const_cast<wsa_ctx*>(ctx), WSA_ERR_INVALID, "bins_hz buffer too small");
    for (int i = 0; i < p.bands; i++) out[i] = p.bins_hz[i];
    return WSA_OK;
}

wsa_status wsa_host_alloc(wsa_ctx* ctx, uint64_t bytes, void** out) {
    if (!ctx || !out) return WSA_ERR_INVALID;
    *out = nullptr;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipHostMalloc(out, bytes ? (size_t)bytes : 1, hipHostMallocPortable));
    { std::lock_guard<std::mutex> lk(g_slab_mu); g_slabs[reinterpret_cast<uintptr_t>(*out)] = bytes ? (size_t)bytes : 1; }
    return WSA_OK;
}
void wsa_host_free(void* p) {
    if (!p) return;
    { std::lock_guard<std::mutex> lk(g_slab_mu); g_slabs.erase(reinterpret_cast<uintptr_t>(p)); }
    (void)hipHostFree(p);
}

wsa_status wsa_queue_create(wsa_ctx* ctx, void** stream) {
    if (!ctx || !stream) return WSA_ERR_INVALID;
    *stream = nullptr;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t s = nullptr;
    HIP_TRY(ctx, hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
    *stream = s;
    return WSA_OK;
}
wsa_status wsa_queue_synchronize(wsa_ctx* ctx, void* stream) {
    if (!ctx) return WSA_ERR_INVALID;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipStreamSynchronize(reinterpret_cast<hipStream_t>(stream)));
    return WSA_OK;
}
void wsa_queue_destroy(wsa_ctx* ctx, void* stream) {
    if (!stream) return;
    if (ctx) (void)hipSetDevice(ctx->device);
    (void)hipStreamDestroy(reinterpret_cast<hipStream_t>(stream));
}

// ---- host arithmetic of the rate converter and the PCM formats: no device involved
uint64_t wsa_resample_length(uint64_t n_in, double fs_in, double fs_out) { return fs_in > 0 && fs_out > 0 ? resample_length(n_in, fs_in, fs_out) : 0; }
uint64_t wsa_resample_ready(uint64_t n_in, double fs_in, double fs_out) { return fs_in > 0 && fs_out > 0 ? resample_ready(n_in, fs_in, fs_out) : 0; }

uint32_t wsa_pcm_channels_tile_frames(int32_t format, uint32_t channels) { return pcm_format_known(format) && channels >= 1 && channels <= 64 ? pcm_tile_frames(format, channels) : 0u; }

// spec PK-3 on the host: channel `select` of the frames, or their mix
wsa_status wsa_pcm_decode_select(int32_t format, const void* in, uint64_t n_frames, uint32_t channels, uint32_t select, float* out) {
    if (channels < 1 || channels > 64 || (n_frames && (!in || !out)) || !pcm_format_known(format) || !pcm_select_known(select, channels)) return WSA_ERR_INVALID;
    const uint8_t* p = static_cast<const uint8_t*>(in);
    const uint32_t sb = pcm_sample_bytes(format);
    const uint64_t step = (uint64_t)channels * sb;
    for (uint64_t j = 0; j < n_frames; j++) {
        const uint8_t* fr = p + j * step;
        out[j] = select == WSA_CHANNEL_MIX ? pcm_mix_frame(channels, [&](uint32_t c) { return pcm_decode_bytes(format, fr + c * sb); }) : pcm_decode_bytes(format, fr + (uint64_t)select * sb);
    }
    return WSA_OK;
}

// specs PK-1 / PK-2 on the host, no device involved: channel 0 of n_frames interleaved frames -> floats
wsa_status wsa_pcm_decode(int32_t format, const void* in, uint64_t n_frames, uint32_t channels, float* out) {
    if (channels < 1 || channels > 64 || (n_frames && (!in || !out)) || !pcm_format_known(format)) return WSA_ERR_INVALID;
    const uint8_t* p = static_cast<const uint8_t*>(in);
    const uint64_t step = (uint64_t)channels * pcm_sample_bytes(format);
    for (uint64_t j = 0; j < n_frames; j++) out[j] = pcm_decode_bytes(format, p + j * step);
    return WSA_OK;
}

}  // extern "C"
